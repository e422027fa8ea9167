"""CostDCNet's source model (include/ptta.h PTTA_COSTDC_PLAIN | PTTA_ADAPT_META_ONLY; CostDCNet._forward, CostDCNet_adapt.py:177-205) against
the golden vectors generated from the real reference (tests/golden/make_golden_costdc_source.py): the eval forward of the loaded checkpoint,
EVERY BatchNorm from its loaded running statistics -- Encoder2D's 15 BatchNorm2d and the UNet3D's 28 BatchNorm3d + ELU as constant affines in
their convolutions' epilogues (option "eval_bn_fused"), the sparse encoder's nine as their own launches.

Bound: SOURCE_EVAL below = 2 x the relative MAE of the engine against the fixtures measured on the MI355X (profiles/costdc_source.txt), the
project's rule; the depth must besides stay inside the north-star 1e-3.
The BatchNorm-adaptation baseline (PTTA_COSTDC_PLAIN alone): adapt_parameters('meta_bn') on a model whose head was never prepared -- gamma / beta of
Encoder2D's 15 BatchNorm2d adapt (30 tensors), batch statistics there in train and eval mode, one pass per training forward (BatchNorm3d and the
sparse BatchNorm count ONE batch per step), loss_cos = 0.  BOUND below = 2 x the measured figures, the same rule; gradients relative to max |g|
per tensor (worst over the 30), read beside the fixture's float64 gradients; over the six-frame sequence the error is printed beside the
reference's own one-ulp sensitivity (`alt_rel_mae`)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from proxytta import _lib
from proxytta.engine import Engine
from tests.costdc_source_cases import BASELINE_FIRST, BASELINE_SEQ, MAX_DEPTH, SOURCE_EVAL, baseline_names, source_state_dict
from tests.test_gpu_costdcnet import costdc_frame
from tests.test_gpu_nlspn_source import _exchange_and_head_calls, _refused
from tests.util import rel_mae

pytestmark = pytest.mark.gpu
NORTH_STAR = 1e-3
LOSS_TYPE = 'adapt_meta_selfsup_seq_ema_reverse'
HP = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1)
SOURCE_EVAL_BOUND = 1.05e-5      # measured: 5.212e-6 (64x96 and the facade), 4.348e-6 (72x100, padded), 5.107e-6 (64x64, N = 2)
NAMES = [c[0] for c in SOURCE_EVAL]

_SD = {}


def weights(stage3=False):
    """The fixtures' state dict on the device, made once per form and never written."""
    if stage3 not in _SD:
        _SD[stage3] = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in source_state_dict(stage3=stage3).items()}
    return _SD[stage3]


def make(n, h, w, stage3=False, drop=(), sd=None):
    eng = Engine(n, h, w, backbone='costdcnet', meta='plain', adapt_mode='meta', max_predict_depth=MAX_DEPTH, **HP)
    eng.load_state_dict({k: v for k, v in (sd or weights(stage3)).items() if k not in drop})
    return eng


def frame(h, w, n):
    raw, image1, sparse = costdc_frame(0, h, w, n)
    return torch.from_numpy(image1).cuda(), torch.from_numpy(sparse).cuda()


@pytest.mark.parametrize('name', NAMES)
def test_source_eval_matches_golden_fused_and_unfused(golden_dir, name):
    """64 x 96; 72 x 100, which takes the dual-corner padding (the network batch doubles) and loads the stage-3 form of the checkpoint, whose
    conv1_rgb_meta.*, proj* and pred* keys the handle accepts and ignores; 64 x 64 with N = 2."""
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    h, w, n, _ = [int(x) for x in g['meta']]
    eng = make(n, h, w, stage3=name == NAMES[1])
    assert int(eng.lib.ptta_adapted_count(eng.handle)) == 0 and eng.adapted == [] and eng.rows == 0
    assert eng.get_option('eval_bn_fused') == 1 and eng.get_option('eval_bn_fused_count') == 43      # 15 BatchNorm2d + 28 BatchNorm3d
    image1, sparse = frame(h, w, n)
    fused = eng.forward_eval(image1, sparse).clone()
    eng.set_option('eval_bn_fused', 0)
    assert eng.get_option('eval_bn_fused_count') == 0
    unfused = eng.forward_eval(image1, sparse).clone()
    eng.set_option('eval_bn_fused', 1)
    again = eng.forward_eval(image1, sparse).clone()
    eng.close()
    err = rel_mae(fused, g['depth_eval'])
    print('FIG source_eval[%s] %.3e   (bound %s)' % (name, err, SOURCE_EVAL_BOUND))
    assert err < SOURCE_EVAL_BOUND and err < NORTH_STAR
    assert torch.equal(fused, unfused), 'max |fused - unfused| = %.3e' % float((fused - unfused).abs().max())
    assert torch.equal(fused, again)
    # the fixture tells running statistics from batch statistics: the two evals of the same weights are this far apart
    assert float(g['batch_stat_eval_rel_mae']) > 1e-2 > err


def test_activations_hold_n_frames_not_2n():
    """One pass: every activation tensor of the program is allocated for N frames; the ProxyTTA handle keeps [real | proxy]."""
    src = make(1, 64, 96)
    proxy = Engine(1, 64, 96, backbone='costdcnet', max_predict_depth=MAX_DEPTH, **HP)
    for name in ('in2d', 'enc2d.layer2.0.out', 'feat2d', 'vol', 'unet3d.inc.double_conv.1.a2', 'unet3d.down1.pool', 'unet3d.up4.up', 'unet3d.up4.conv.double_conv.1.a2'):
        a, b = src.debug_tensor(name).numel(), proxy.debug_tensor(name).numel()
        assert a > 0 and 2 * a == b, (name, a, b)
    assert src.debug_tensor('cost').numel() == proxy.debug_tensor('cost').numel()        # the real pass's alone on both
    with pytest.raises(RuntimeError, match=r'\(-2\)'):
        src.debug_tensor('rows')                                                          # no heads, no rows
    src.close()
    proxy.close()


def test_a_second_load_rebuilds_the_tables_and_a_missing_buffer_is_named(golden_dir):
    g = np.load(os.path.join(golden_dir, NAMES[0] + '.npz'))
    h, w, n, _ = [int(x) for x in g['meta']]
    image1, sparse = frame(h, w, n)
    eng = make(n, h, w)
    first = eng.forward_eval(image1, sparse).clone()
    # moved running statistics of one BatchNorm2d and one BatchNorm3d, loaded into the same handle: both tables are rebuilt
    for key in ('enc2d.layer1.0.norm1.running_mean', 'unet3d.up4.conv.double_conv.1.bn2.running_var'):
        sd = dict(weights())
        sd[key] = sd[key] * 1.5 + 0.25
        eng.load_state_dict(sd)
        moved = eng.forward_eval(image1, sparse).clone()
        assert rel_mae(moved, first) > 1e-4, key
    eng.load_state_dict(weights())
    assert torch.equal(eng.forward_eval(image1, sparse), first)
    eng.close()
    # a state dict without one of the buffers loads; the first eval forward names the missing tensor
    for key in ('unet3d.down2.maxpool_conv.1.double_conv.0.bn1.running_var', 'enc2d.layer2.0.norm3.running_mean'):
        eng = make(n, h, w, drop=(key, key.replace('.norm3.', '.downsample.1.')))
        with pytest.raises(RuntimeError, match=r'\(-3\).*' + key.replace('.', r'\.')):
            eng.forward_eval(image1, sparse)
        eng.close()


def test_training_heads_and_exchanges_are_refused_and_the_handle_still_works(golden_dir):
    g = np.load(os.path.join(golden_dir, NAMES[0] + '.npz'))
    h, w, n, _ = [int(x) for x in g['meta']]
    image1, sparse = frame(h, w, n)
    eng = make(n, h, w)
    want = eng.forward_eval(image1, sparse).clone()
    lib, H, P = eng.lib, eng.handle, _lib.ptr
    out, info = torch.empty_like(sparse), torch.empty(4, device='cuda')
    cb = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_longlong, ctypes.c_void_p)(lambda *a: 0)
    buf = torch.zeros(4096, dtype=torch.float64, device='cuda')
    train = [('ptta_forward_train', lambda: lib.ptta_forward_train(H, P(image1), P(sparse), P(out), None, None, None)),
             ('ptta_step', lambda: lib.ptta_step(H, P(image1), None, P(sparse), None, P(out), P(info), None)),
             ('ptta_backward', lambda: lib.ptta_backward(H, P(out), None, None, None, None)),
             ('ptta_adam_step', lambda: lib.ptta_adam_step(H, None, None, None))]
    exchange, heads = _exchange_and_head_calls(eng, image1, sparse, buf, cb)
    _refused(eng, train, b'adapts nothing')
    _refused(eng, exchange, b'more than one rank is not offered')
    _refused(eng, heads, b'has no heads')
    assert torch.equal(eng.forward_eval(image1, sparse), want)
    eng.close()


def test_create_refusals_each_with_its_reason():
    lib = _lib.load()
    hp = _lib.Hparams(3e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 2.0, 0.1, -1.0, MAX_DEPTH)
    P, M = _lib.PTTA_COSTDC_PLAIN, _lib.PTTA_ADAPT_META_ONLY
    assert P == 0x800
    cases = [(_lib.PTTA_BACKBONE_NLSPN, P | M, _lib.PTTA_DTYPE_F32, 'CostDCNet backbone'),
             (_lib.PTTA_BACKBONE_MSG_CHN, P, _lib.PTTA_DTYPE_F32, 'CostDCNet backbone'),
             (_lib.PTTA_BACKBONE_COSTDCNET, P | M | _lib.PTTA_META_2LAYERS, _lib.PTTA_DTYPE_F32, 'PTTA_META_2LAYERS'),
             (_lib.PTTA_BACKBONE_COSTDCNET, P | M | _lib.PTTA_SYNCBN_ADAPT, _lib.PTTA_DTYPE_F32, 'PTTA_SYNCBN_ADAPT'),
             (_lib.PTTA_BACKBONE_COSTDCNET, P | M, _lib.PTTA_DTYPE_MIXED, 'PTTA_DTYPE_MIXED'),
             (_lib.PTTA_BACKBONE_COSTDCNET, P | _lib.PTTA_META_2LAYERS, _lib.PTTA_DTYPE_F32, 'PTTA_META_2LAYERS'),
             (_lib.PTTA_BACKBONE_COSTDCNET, P | _lib.PTTA_SYNCBN_ADAPT, _lib.PTTA_DTYPE_F32, 'PTTA_SYNCBN_ADAPT'),
             (_lib.PTTA_BACKBONE_COSTDCNET, P, _lib.PTTA_DTYPE_MIXED, 'PTTA_DTYPE_MIXED')]
    for backbone, mode, dtype, word in cases:
        hd = ctypes.c_void_p()
        assert lib.ptta_create(ctypes.byref(hd), backbone, mode, 1, 64, 96, dtype, ctypes.byref(hp)) == -38 and not hd.value
        assert word in lib.ptta_last_error(None).decode(), (word, lib.ptta_last_error(None).decode())


def test_facade_pretrain_is_the_source_model_not_the_proxytta_network(golden_dir):
    from proxytta.costdcnet import CostDCNetModel_Adapt
    from tests.costdc_source_cases import PREPARE
    g = np.load(os.path.join(golden_dir, NAMES[0] + '.npz'))
    h, w, n, _ = [int(x) for x in g['meta']]
    image1, sparse = frame(h, w, n)
    model = CostDCNetModel_Adapt(max_depth=MAX_DEPTH)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in source_state_dict().items()})
    model.eval()
    want = model.forward(image1, sparse)                                     # the default loss_type
    err = rel_mae(want, g['depth_eval'])
    print('FIG source_eval[facade] %.3e   (bound %s)' % (err, SOURCE_EVAL_BOUND))
    assert err < SOURCE_EVAL_BOUND and err < NORTH_STAR
    assert torch.equal(model.forward(image1, sparse, loss_type='pretrain_time'), want)
    model.train()
    with pytest.raises(NotImplementedError, match='every parameter'):
        model.forward(image1, sparse, loss_type='pretrain')
    with pytest.raises(RuntimeError, match='meta_bn'):                       # 'bn' in the string, but nothing selected the baseline
        model.forward(image1, sparse, loss_type='pretrain_bn')
    # a prepared model holding the same checkpoint in its stage-3 form: 'pretrain' is still the source model, the TTA string is another network
    prepared = CostDCNetModel_Adapt(max_depth=MAX_DEPTH)
    prepared._prepare_head(PREPARE)
    prepared.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in source_state_dict(stage3=True).items()})
    prepared.eval()
    assert torch.equal(prepared.forward(image1, sparse, loss_type='pretrain'), want)
    other = prepared.forward(image1, sparse, loss_type=LOSS_TYPE)
    assert rel_mae(other, g['depth_eval']) > 1e-2
    # the source engine is no snapshot: after a ProxyTTA step of the same model (BatchNorm3d / sparse buffers move in place, gamma / beta of
    # Encoder2D adapt) 'pretrain' answers for the model as it is now -- what a fresh model loaded with the current state dict returns
    # ... also in the split loop, where an optimizer outside the library writes gamma / beta AFTER the training forward: a 'pretrain' call between
    # the two must not leave the source engine stamped as current
    def fresh_answer(drop):
        fresh = CostDCNetModel_Adapt(max_depth=MAX_DEPTH)
        fresh._prepare_head(PREPARE)
        fresh.load_state_dict({k: v.clone() for k, v in prepared.state_dict().items()})
        if drop:
            fresh.adapt_parameters('meta_bn')
        fresh.eval()
        return fresh.forward(image1, sparse, loss_type='pretrain')
    prepared.train()
    prepared.forward(image1, sparse, loss_type=LOSS_TYPE)                   # moves the BatchNorm3d / sparse buffers
    prepared.eval()
    between = prepared.forward(image1, sparse, loss_type='pretrain')
    assert torch.equal(between, fresh_answer(False)) and not torch.equal(between, want)
    with torch.no_grad():                                                    # what optimizer.step() does: in-place writes of the parameters
        for k, p in prepared.model.named_parameters():
            if k.startswith('enc2d.') and k.endswith('norm1.weight'):
                p.mul_(1.05)
    stepped = prepared.forward(image1, sparse, loss_type='pretrain')
    assert torch.equal(stepped, fresh_answer(False)) and not torch.equal(stepped, between)
    prepared.adapt_parameters('meta_bn')
    assert not [k for k in prepared._engines if k[0] == 'plain']            # the call dropped Encoder2D's statistics: that engine is gone
    prepared.train()
    raw = torch.from_numpy(costdc_frame(0, h, w, n)[0]).cuda()
    prepared.step(image1, sparse, loss_image=raw)
    prepared.eval()
    before = prepared.forward(image1, sparse, loss_type='pretrain')          # the baseline kind now: batch statistics in Encoder2D
    prepared.train()
    prepared.step(image1, sparse, loss_image=raw)
    prepared.eval()
    after = prepared.forward(image1, sparse, loss_type='pretrain')
    assert torch.equal(fresh_answer(True), after) and not torch.equal(after, before)


# ---- the BatchNorm-adaptation baseline -------------------------------------------------------------------------------------------------
# 2 x the measured figures of profiles/costdc_source.txt (worst over the fixtures and the paths that have the quantity)
#   measured:       6.189e-6 (64x64 N 2)   5.696e-6       1.215e-4 (enc2d.layer1.0.norm2.weight; 1.08e-4 from the float64 reference, whose float32
#                   form is 1.4e-5 - 2.2e-5 from it)    9.517e-6 (lr 3e-3)   7.053e-6     9.780e-7 (the 74 updated BatchNorm3d / sparse buffers)
BOUND = dict(depth_train=1.24e-5, loss=1.14e-5, grad=2.43e-4, param=1.9e-5, depth_eval=1.41e-5, buf=1.96e-6,
             # six frames, one parameter set, lr 3e-3: 7.1e-6, 1.1e-4, 2.6e-4, 5.5e-4, 7.4e-4, 7.823e-4 -- the reference against itself one ulp off
             # grows 8.5e-7 -> 7.7e-5 over the same steps (x 90; here x 110 from a first-step error ten times larger): every step inside 1e-3
             seq_depth_eval=1.56e-3, seq_param=4.52e-3)          # measured: 7.823e-4 and 2.261e-3 (both at step 5)
BUFFERS = ('running_mean', 'running_var', 'num_batches_tracked')


def make_baseline(n, h, w):
    """-> (engine, state dict with its own copies of the buffers a training forward updates in place, {adapted name: (param, m, v)})"""
    eng = Engine(n, h, w, backbone='costdcnet', meta='plain', adapt_mode='meta_bn', max_predict_depth=MAX_DEPTH, **HP)
    sd = {k: (v.clone() if k.endswith(BUFFERS) else v) for k, v in weights().items()}
    eng.load_state_dict(sd)
    adapted = {}
    for k in eng.adapted:
        p = sd[k].clone().contiguous()
        adapted[k] = (p, torch.zeros_like(p), torch.zeros_like(p))
        eng.bind_adapted(k, *adapted[k])
    return eng, sd, adapted


def frames(s, h, w, n):
    return [torch.from_numpy(x).cuda() for x in costdc_frame(s, h, w, n)]


def gerr(a, b):
    """gradient error relative to the gradient's largest entry"""
    b = torch.from_numpy(np.asarray(b)).to(a.device)
    return float((a - b).abs().max() / b.abs().max())


def check(figs):
    for k, v in figs:
        print('FIG %-22s %.3e   (bound %.3e)' % (k, v, BOUND[k.split('[')[0]]))
    for k, v in figs:
        assert v < BOUND[k.split('[')[0]], (k, v)


def first_step_figs(g, info, depth, d_eval, grads, adapted, sd=None):
    names = [str(x) for x in g['adapted_names']]
    ref_info = g['s0/loss_info']
    assert float(info[3]) == 0.0 and float(ref_info[3]) == 0.0           # no heads: no cosine term, exactly
    worst, k = max((gerr(grads[k], g['s0/grad/' + k]), k) for k in names)
    w64, k64 = max((gerr(grads[kk], g['s0/grad64/' + kk]), kk) for kk in names)
    r64, kr = max((gerr(torch.from_numpy(g['s0/grad/' + kk]), g['s0/grad64/' + kk]), kk) for kk in names)
    print('F64  worst gradient vs the float32 fixture %.3e %s; vs the float64 reference %.3e %s; float32 reference vs float64 %.3e %s' % (worst, k, w64, k64, r64, kr))
    figs = [('depth_train', rel_mae(depth, g['s0/depth_train'])),
            ('loss', float(np.max(np.abs(info.cpu().numpy()[:3] - ref_info[:3]) / np.abs(ref_info[:3])))),
            ('grad', worst),
            ('param', max(rel_mae(adapted[k][0], g['s0/param/' + k]) for k in names))]
    if sd is not None:           # the buffers the training forward updated in place: ONE update each
        bufs = [k[len('s0/buf/'):] for k in g.files if k.startswith('s0/buf/')]
        assert len(bufs) == 2 * (28 + 9)
        figs.append(('buf', max(rel_mae(sd[k], g['s0/buf/' + k], floor=1e-6) for k in bufs)))
    return figs + [('depth_eval', rel_mae(d_eval, g['s0/depth_eval']))]


@pytest.mark.parametrize('name', [c[0] for c in BASELINE_FIRST])
def test_baseline_first_step_matches_golden(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    h, w, n, steps = [int(x) for x in g['meta']]
    eng, sd, adapted = make_baseline(n, h, w)
    names = [str(x) for x in g['adapted_names']]
    assert int(eng.lib.ptta_adapted_count(eng.handle)) == 30 and eng.adapted == names == baseline_names()
    assert all(eng.adapted_repeat[k] == 1 for k in names) and eng.adapted_numel == {k: sd[k].numel() for k in names}
    assert eng.rows == 0 and int(eng.lib.ptta_embedding_rows(eng.handle)) == 0
    nbt0 = {k: int(v) for k, v in sd.items() if k.endswith('num_batches_tracked') and not k.startswith('enc2d.')}
    raw, image1, sparse = frames(0, h, w, n)
    info, depth = eng.step(image1, sparse, loss_image=raw, want_depth=True)
    grads = {k: eng.grad(k, adapted[k][0]) for k in names}
    d_eval = eng.forward_eval(image1, sparse)
    figs = first_step_figs(g, info, depth, d_eval, grads, adapted, sd)
    # one sparse-encoder call and one UNet3D call per training forward: every tracked BatchNorm counted ONE batch (the ProxyTTA handle: 2)
    assert len(nbt0) == 28 + 9 and all(int(sd[k]) == v + 1 for k, v in nbt0.items()) and int(g['nbt_step']) == 1
    eng.close()
    check(figs)
    assert figs[0][1] < NORTH_STAR and figs[-1][1] < NORTH_STAR


def test_proxytta_handle_counts_two_batches_per_step():
    """What the count above tells apart: the same weights on the ProxyTTA handle, whose two passes update every tracked BatchNorm twice."""
    eng = Engine(1, 64, 96, backbone='costdcnet', max_predict_depth=MAX_DEPTH, **HP)
    sd = {k: (v.clone() if k.endswith(BUFFERS) else v) for k, v in weights(True).items()}
    eng.load_state_dict(sd)
    keep = {k: (sd[k].clone().contiguous(), torch.zeros_like(sd[k]), torch.zeros_like(sd[k])) for k in eng.adapted}
    for k in eng.adapted:
        eng.bind_adapted(k, *keep[k])
    nbt0 = {k: int(v) for k, v in sd.items() if k.endswith('num_batches_tracked') and k.startswith(('unet3d.', 'enc3d.'))}
    raw, image1, sparse = frames(0, 64, 96, 1)
    eng.step(image1, sparse, loss_image=raw)
    torch.cuda.synchronize()
    assert len(nbt0) == 37 and all(int(sd[k]) == v + 2 for k, v in nbt0.items())
    eng.close()


def test_baseline_split_calls_are_the_fused_step(golden_dir):
    """ptta_forward_train (depth only) / ptta_loss_forward / ptta_loss_backward with emb = ref = NULL / ptta_backward with grad_ref = NULL /
    ptta_adam_step on one handle against ptta_step on another."""
    g = np.load(os.path.join(golden_dir, BASELINE_FIRST[0][0] + '.npz'))
    h, w, n, steps = [int(x) for x in g['meta']]
    raw, image1, sparse = frames(0, h, w, n)
    validity = torch.where(sparse > 0, torch.ones_like(sparse), sparse)
    a, _, ad_a = make_baseline(n, h, w)
    info_a, depth_a = a.step(image1, sparse, loss_image=raw, want_depth=True)
    b, _, ad_b = make_baseline(n, h, w)
    depth_b, emb, ref = b.forward_train(image1, sparse)
    assert emb is None and ref is None
    info_b = b.loss_forward(raw, depth_b, sparse, validity, None, None, HP['w_sparse_depth'], HP['w_smoothness'], HP['w_cos'])
    gd, gr = b.loss_backward(raw, depth_b, sparse, validity, None, None)
    assert gr is None and float(info_b[3]) == 0.0
    grads = b.backward_all(gd, None, {k: v[0] for k, v in ad_b.items()})
    b.adam_step()
    torch.cuda.synchronize()
    assert torch.equal(depth_a, depth_b)
    np.testing.assert_allclose(info_b.cpu().numpy(), info_a.cpu().numpy(), rtol=1e-6)
    d_eval = b.forward_eval(image1, sparse)
    check(first_step_figs(g, info_b, depth_b, d_eval, dict(zip(b.adapted, grads)), ad_b))
    # emb_out / ref_out must be NULL on a handle without heads
    junk = torch.empty(16, device='cuda')
    rc = b.lib.ptta_forward_train(b.handle, _lib.ptr(image1), _lib.ptr(sparse), None, _lib.ptr(junk), None, None)
    assert rc == -22 and b'must be NULL' in b.lib.ptta_last_error(b.handle)
    a.close()
    b.close()


def test_baseline_six_frame_sequence_matches_golden_at_every_step(golden_dir):
    g = np.load(os.path.join(golden_dir, BASELINE_SEQ[0] + '.npz'))
    h, w, n, steps = [int(x) for x in g['meta']]
    assert steps == 6 and g['alt_rel_mae'].shape == (6,)
    eng, sd, adapted = make_baseline(n, h, w)
    names = [str(x) for x in g['adapted_names']]
    figs = []
    for s in range(steps):
        raw, image1, sparse = frames(s, h, w, n)
        info, _ = eng.step(image1, sparse, loss_image=raw)
        figs.append(('seq_depth_eval[%d]' % s, rel_mae(eng.forward_eval(image1, sparse), g['s%d/depth_eval' % s])))
        figs.append(('seq_param[%d]' % s, max(rel_mae(adapted[k][0], g['s%d/param/%s' % (s, k)]) for k in names)))
        print('ALT  step %d reference vs itself one ulp off %.3e' % (s, float(g['alt_rel_mae'][s])))
    assert float(info[3]) == 0.0
    eng.close()
    check(figs)
    for k, v in figs:
        if k.startswith('seq_depth_eval'):
            assert v < NORTH_STAR, (k, v)


def test_baseline_allocates_for_n_frames_and_refuses_what_it_has_not(golden_dir):
    base, _, _ = make_baseline(1, 64, 96)
    proxy = Engine(1, 64, 96, backbone='costdcnet', max_predict_depth=MAX_DEPTH, **HP)
    for name in ('in2d', 'enc2d.layer2.0.out', 'feat2d', 'vol', 'unet3d.inc.double_conv.1.a2', 'unet3d.down1.pool', 'unet3d.up4.up'):
        a, b = base.debug_tensor(name).numel(), proxy.debug_tensor(name).numel()
        assert a > 0 and 2 * a == b, (name, a, b)
    proxy.close()
    raw, image1, sparse = frames(0, 64, 96, 1)
    cb = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_longlong, ctypes.c_void_p)(lambda *a: 0)
    buf = torch.zeros(4096, dtype=torch.float64, device='cuda')
    exchange, heads = _exchange_and_head_calls(base, image1, sparse, buf, cb)
    _refused(base, exchange, b'more than one rank is not offered')
    _refused(base, heads, b'has no heads')
    with pytest.raises(RuntimeError, match=r'\(-38\).*eval_bn_fused'):       # batch statistics in Encoder2D: there is no constant affine to fuse
        base.set_option('eval_bn_fused', 0)
    info, depth = base.step(image1, sparse, loss_image=raw, want_depth=True)
    assert torch.isfinite(depth).all() and float(info[3]) == 0.0
    base.close()


def test_facade_reference_loop_and_fused_step_match_golden(golden_dir):
    """src/tta_main.py:610-633 on the model whose head was never prepared: forward('pretrain_bn') -> compute_loss(embedding=None, reference=None)
    -> backward -> torch.optim.Adam.step -> eval forward('pretrain'); then the fused step() on a fresh model."""
    from proxytta.model import ExternalModel_Adapt
    g = np.load(os.path.join(golden_dir, BASELINE_FIRST[0][0] + '.npz'))
    h, w, n, steps = [int(x) for x in g['meta']]
    names = [str(x) for x in g['adapted_names']]
    raw, image1, sparse = frames(0, h, w, n)
    validity = torch.where(sparse > 0, torch.ones_like(sparse), sparse)
    for fused in (False, True):
        model = ExternalModel_Adapt('costdcnet', 0.1, MAX_DEPTH, device=torch.device('cuda'))
        model.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in source_state_dict().items()})
        params = model.adapt_parameters(mode='meta_bn')
        assert len(params) == 30 and model.model.adapted == names
        opt = torch.optim.Adam(params, lr=HP['lr'], betas=HP['betas'], eps=HP['eps'], weight_decay=HP['weight_decay'])
        model.model.set_hparams(**HP)
        named = dict(model.model.model.named_parameters())
        model.train()
        if fused:
            model.model.bind_optimizer(opt)
            info, depth = model.step(image1, sparse, loss_image=raw, want_depth=True)
            eng = model.model._engine(image1)
            grads = {k: eng.grad(k, named[k]) for k in names}
        else:
            depth, emb, ref = model.forward(image=image1, sparse_depth=sparse, loss_type='pretrain_bn')
            assert emb is None and ref is None
            loss, li = model.compute_loss(input_rgb=raw, output_depth=depth, sparse_depth=sparse, validity_map=validity, embedding=emb, reference=ref,
                                          w_loss_sparse_depth=HP['w_sparse_depth'], w_loss_smoothness=HP['w_smoothness'], w_loss_cos=HP['w_cos'],
                                          loss_type='adapt')
            opt.zero_grad()
            loss.backward()
            grads = {k: named[k].grad.clone() for k in names}
            opt.step()
            info = torch.stack([loss.detach(), li['loss_smooth'], li['loss_sparse_depth'], li['loss_cos']])
        model.eval()
        d_eval = model.forward(image1, sparse, loss_type='pretrain')          # the baseline engine's eval forward
        check(first_step_figs(g, info, depth.detach(), d_eval, grads, {k: (named[k].data,) for k in names}))
