"""NLSPN without the meta layer (include/ptta.h PTTA_META_NONE; NLSPNModel_Adapt._forward, nlspnmodel_adapt.py:792-848) against the golden vectors
generated from the real reference (tests/golden/make_golden_nlspn_source.py):
  the source model (PTTA_META_NONE | PTTA_ADAPT_META_ONLY): the eval forward of the loaded checkpoint, every BatchNorm2d from its loaded running
    statistics, as a constant affine in the convolution's epilogue (option "eval_bn_fused");
  the BatchNorm-adaptation baseline (PTTA_META_NONE): adapt_parameters('meta_bn') on a model whose head was never prepared -- gamma / beta of every
    BatchNorm2d adapt (86 tensors), batch statistics in train and eval mode, one pass per training forward, loss_cos = 0.

Bounds (BOUND below) = 2 x the error of the fp32 engine against the fixtures measured on the MI355X (profiles/nlspn_source.txt), as every other
bound of the project; depths as relative MAE, gradients relative to max |g| (worst over the 86 tensors), parameters and Adam moments as
relative MAE (worst over the 86 tensors).  Every depth must besides stay inside the north-star 1e-3.  The fixtures' eval depths are the output
BEFORE hole filling, which is what the engine returns."""
import ctypes
import os

import numpy as np
import pytest
import torch

from proxytta import _lib
from proxytta.engine import Engine
from tests.nlspn_meta_cases import PREPARE
from tests.nlspn_source_cases import BASELINE_FIRST, BASELINE_SEQ, SOURCE_EVAL, baseline_names, source_state_dict
from tests.test_gpu_nlspn import nlspn_frame
from tests.util import rel_mae

pytestmark = pytest.mark.gpu
LOSS_TYPE = 'adapt_meta_selfsup_seq_ema_reverse'
NORTH_STAR = 1e-3
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1, max_input_depth=80.0)

# 2 x the measured figures of profiles/nlspn_source.txt (worst over the fixtures and the paths -- fused step, split calls, the facade -- that have
# the quantity).  The gradient figure is the worst of the 86 tensors, conv5.0.bn1.bias: on a 32x64 frame conv5's BatchNorm2d normalise over 8
# pixels, and the float32 REFERENCE's own gradients sit 1.0e-1 (1.1e-1 at 40x56) from its float64 ones there (`s0/grad64/*`, printed beside).
#   measured:       1.570e-6              1.242e-6             9.231e-6       2.064e-1      8.108e-4 (lr 1e-3: Adam's first step is +-lr)
BOUND = dict(source_eval=3.2e-6, depth_train=2.5e-6, loss=1.85e-5, grad=4.13e-1, param=1.63e-3,
             exp_avg=6.5e-2, exp_avg_sq=7.71e-2, depth_eval=7.5e-5,          # measured: 3.202e-2, 3.850e-2, 3.730e-5
             seq_depth_eval=2.9e-5, seq_param=1.18e-3)                      # measured: 1.413e-5 (step 2 of six), 5.882e-4 (after six steps)


def hp_of(g):
    lr, b1, b2, eps, wd, w_sd, w_sm, w_cos, mid = [float(x) for x in g['hp']]
    return dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, w_sparse_depth=w_sd, w_smoothness=w_sm, w_cos=w_cos, max_input_depth=mid)


_SD = {}


def weights(with_head=False):
    """The fixtures' state dict on the device, made once per form and never written (adapted tensors are cloned before they are bound)."""
    if with_head not in _SD:
        _SD[with_head] = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in source_state_dict(with_head=with_head).items()}
    return _SD[with_head]


def make(kind, n, h, w, hp, legacy=False, with_head=False, drop=()):
    """kind 'source' or 'baseline' -> (engine, state dict, {adapted name: (param, exp_avg, exp_avg_sq)})"""
    eng = Engine(n, h, w, backbone='nlspn', meta='none', adapt_mode='meta' if kind == 'source' else 'meta_bn', legacy_offset=legacy, **hp)
    sd = weights(with_head)
    eng.load_state_dict({k: v for k, v in sd.items() if v.dtype == torch.float32 and k not in drop})
    adapted = {}
    for k in eng.adapted:
        p = sd[k].clone().contiguous()
        adapted[k] = (p, torch.zeros_like(p), torch.zeros_like(p))
        eng.bind_adapted(k, *adapted[k])
    return eng, sd, adapted


def frame(s, h, w, n):
    return [torch.from_numpy(x).cuda() for x in nlspn_frame(s, h, w, n)]


def gerr(a, b):
    """gradient error relative to the gradient's largest entry"""
    b = torch.from_numpy(np.asarray(b)).to(a.device)
    return float((a - b).abs().max() / b.abs().max())


def check(figs):
    for k, v in figs:
        print('FIG %-22s %.3e   (bound %.3e)' % (k, v, BOUND[k.split('[')[0]]))
    for k, v in figs:
        assert v < BOUND[k.split('[')[0]], (k, v)


def first_step_figs(g, info, depth, d_eval, grads, adapted):
    names = [str(x) for x in g['adapted_names']]
    ref_info = g['s0/loss_info']
    assert float(info[3]) == 0.0 and float(ref_info[3]) == 0.0           # no heads: no cosine term, exactly
    worst, k = max((gerr(grads[k], g['s0/grad/' + k]), k) for k in names)
    # beside the bound's figure: the same tensor, and the worst one, against the reference's float64 gradients -- and the float32 reference itself
    for what, e, kk in (('that tensor', gerr(grads[k], g['s0/grad64/' + k]), k),) + (('worst', ) + max((gerr(grads[kk], g['s0/grad64/' + kk]), kk) for kk in names),) + \
            (('float32 reference, worst', ) + max((gerr(torch.from_numpy(g['s0/grad/' + kk]), g['s0/grad64/' + kk]), kk) for kk in names),):
        print('F64  gradient vs float64 reference, %-26s %.3e  %s' % (what, e, kk))
    errs = sorted(gerr(grads[kk], g['s0/grad/' + kk]) for kk in names)
    print('F64  worst gradient vs the float32 fixture: %s; median over the 86 tensors %.3e, above 1e-2: %d' % (k, errs[43], sum(e > 1e-2 for e in errs)))
    figs = [('depth_train', rel_mae(depth, g['s0/depth_train'])),
            ('loss', float(np.max(np.abs(info.cpu().numpy()[:3] - ref_info[:3]) / np.abs(ref_info[:3])))),
            ('grad', worst),
            ('param', max(rel_mae(adapted[k][0], g['s0/param/' + k]) for k in names))]
    if 's0/exp_avg/' + names[0] in g.files and len(adapted[names[0]]) == 3:
        figs += [('exp_avg', max(rel_mae(adapted[k][1], g['s0/exp_avg/' + k], floor=1e-12) for k in names)),
                 ('exp_avg_sq', max(rel_mae(adapted[k][2], g['s0/exp_avg_sq/' + k], floor=1e-24) for k in names))]
    return figs + [('depth_eval', rel_mae(d_eval, g['s0/depth_eval']))]


# ---- the source model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SOURCE_EVAL)
def test_source_eval_matches_golden_fused_and_unfused(golden_dir, name):
    """Both shapes (40x56 with N = 2 and PTTA_NLSPN_LEGACY_OFFSET: ceil-halving maps, decoder crops, a batch); the second loads the stage-3 form
    of the checkpoint, whose conv1_rgb_meta.*, proj* and pred* keys the handle accepts and ignores."""
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    h, w, n, _ = [int(x) for x in g['meta']]
    eng, sd, adapted = make('source', n, h, w, hp_of(g), legacy=bool(int(g['legacy'])), with_head=name == SOURCE_EVAL[1])
    assert int(eng.lib.ptta_adapted_count(eng.handle)) == 0 and eng.adapted == [] and eng.rows == 0
    assert eng.get_option('eval_bn_fused') == 1 and eng.get_option('graph') == 0
    raw, image1, sparse = frame(0, h, w, n)
    fused = eng.forward_eval(image1, sparse).clone()
    eng.set_option('eval_bn_fused', 0)
    unfused = eng.forward_eval(image1, sparse).clone()
    eng.set_option('eval_bn_fused', 1)
    again = eng.forward_eval(image1, sparse).clone()
    eng.close()
    err = rel_mae(fused, g['depth_eval'])
    check([('source_eval', err)])
    assert err < NORTH_STAR
    assert torch.equal(fused, unfused), 'max |fused - unfused| = %.3e' % float((fused - unfused).abs().max())
    assert torch.equal(fused, again)
    assert int((fused == 0).sum()) == int(g['n_zero_eval'])
    # the fixture tells running statistics from batch statistics: the two evals of the same weights are this far apart
    assert float(g['batch_stat_eval_rel_mae']) > 1e-2 > err


def test_source_eval_replays_its_graph_bit_identically(golden_dir):
    g = np.load(os.path.join(golden_dir, SOURCE_EVAL[0] + '.npz'))
    h, w, n, _ = [int(x) for x in g['meta']]
    eng, sd, adapted = make('source', n, h, w, hp_of(g))
    raw, image1, sparse = frame(0, h, w, n)
    plain = eng.forward_eval(image1, sparse).clone()
    eng.set_option('graph', 1)
    outs = [eng.forward_eval(image1, sparse).clone() for _ in range(3)]        # eager, captured, replayed
    eng.close()
    assert all(torch.equal(plain, o) for o in outs)


def test_source_state_dict_without_a_running_statistic_fails_at_the_eval_forward_by_name():
    eng, sd, adapted = make('source', 1, 32, 64, HP, drop=('conv4.1.bn2.running_var',))           # the load itself succeeds
    raw, image1, sparse = frame(0, 32, 64, 1)
    out = torch.full((1, 1, 32, 64), -5.0, device='cuda')
    rc = eng.lib.ptta_forward_eval(eng.handle, _lib.ptr(image1), _lib.ptr(sparse), _lib.ptr(out), None)
    torch.cuda.synchronize()
    assert rc == -3 and b'conv4.1.bn2.running_var' in eng.lib.ptta_last_error(eng.handle)
    assert bool((out == -5.0).all())                     # nothing was normalised with zeros and ones
    eng.load_state_dict({'conv4.1.bn2.running_var': sd['conv4.1.bn2.running_var']})
    assert torch.isfinite(eng.forward_eval(image1, sparse)).all()
    eng.close()


# ---- the BatchNorm-adaptation baseline -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', BASELINE_FIRST)
def test_baseline_first_step_matches_golden(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    h, w, n, steps = [int(x) for x in g['meta']]
    eng, sd, adapted = make('baseline', n, h, w, hp_of(g), legacy=bool(int(g['legacy'])))
    names = [str(x) for x in g['adapted_names']]
    assert int(eng.lib.ptta_adapted_count(eng.handle)) == 86 and eng.adapted == names == baseline_names()
    assert all(eng.adapted_repeat[k] == 1 for k in names) and eng.adapted_numel == {k: sd[k].numel() for k in names}
    assert eng.rows == 0 and int(eng.lib.ptta_embedding_rows(eng.handle)) == 0
    raw, image1, sparse = frame(0, h, w, n)
    info, depth = eng.step(image1, sparse, loss_image=raw, want_depth=True)
    grads = {k: eng.grad(k, adapted[k][0]) for k in names}
    d_eval = eng.forward_eval(image1, sparse)
    figs = first_step_figs(g, info, depth, d_eval, grads, adapted)
    eng.close()
    check(figs)
    assert figs[0][1] < NORTH_STAR and figs[-1][1] < NORTH_STAR


def test_baseline_split_calls_are_the_fused_step(golden_dir):
    """ptta_forward_train (depth only) / ptta_loss_forward / ptta_loss_backward with emb = ref = NULL / ptta_backward with grad_ref = NULL /
    ptta_adam_step on one handle against ptta_step on another: the same launches in the same order, bit for bit."""
    g = np.load(os.path.join(golden_dir, BASELINE_FIRST[0] + '.npz'))
    h, w, n, steps = [int(x) for x in g['meta']]
    hp = hp_of(g)
    raw, image1, sparse = frame(0, h, w, n)
    validity = torch.where(sparse > 0, torch.ones_like(sparse), sparse)
    a, sd, ad_a = make('baseline', n, h, w, hp)
    info_a, depth_a = a.step(image1, sparse, loss_image=raw, want_depth=True)
    b, sd, ad_b = make('baseline', n, h, w, hp)
    depth_b, emb, ref = b.forward_train(image1, sparse)
    assert emb is None and ref is None
    info_b = b.loss_forward(raw, depth_b, sparse, validity, None, None, hp['w_sparse_depth'], hp['w_smoothness'], hp['w_cos'])
    gd, gr = b.loss_backward(raw, depth_b, sparse, validity, None, None)
    assert gr is None and float(info_b[3]) == 0.0
    grads = b.backward_all(gd, None, {k: v[0] for k, v in ad_b.items()})
    b.adam_step()
    torch.cuda.synchronize()
    assert torch.equal(depth_a, depth_b)
    np.testing.assert_allclose(info_b.cpu().numpy(), info_a.cpu().numpy(), rtol=1e-6)       # the same partial sums, finalised by another launch
    # (float atomics in the reductions: gradients and what follows them are not bit for bit -- both paths are held to the fixture instead)
    d_eval = b.forward_eval(image1, sparse)
    check(first_step_figs(g, info_b, depth_b, d_eval, dict(zip(b.adapted, grads)), ad_b))
    assert rel_mae(a.forward_eval(image1, sparse), d_eval) < BOUND['depth_eval']
    # emb_out / ref_out must be NULL on a handle without heads
    junk = torch.empty(16, device='cuda')
    rc = b.lib.ptta_forward_train(b.handle, _lib.ptr(image1), _lib.ptr(sparse), None, _lib.ptr(junk), None, None)
    assert rc == -22 and b'must be NULL' in b.lib.ptta_last_error(b.handle)
    a.close()
    b.close()


def test_baseline_six_frame_sequence_matches_golden_at_every_step(golden_dir):
    """The reference against itself with one adapted gamma entry one ulp off stays at 1.2e-7 .. 1.5e-7 over these six steps (`alt_rel_mae`):
    with every BatchNorm2d renormalising from batch statistics a one-ulp move does not grow."""
    g = np.load(os.path.join(golden_dir, BASELINE_SEQ + '.npz'))
    h, w, n, steps = [int(x) for x in g['meta']]
    assert steps == 6 and g['alt_rel_mae'].shape == (6,)
    eng, sd, adapted = make('baseline', n, h, w, hp_of(g))
    names = [str(x) for x in g['adapted_names']]
    figs = []
    for s in range(steps):
        raw, image1, sparse = frame(s, h, w, n)
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


def test_baseline_step_replays_its_graph(golden_dir):
    """Option "graph" (off by default): three steps and eval forwards replayed against three launched kernel by kernel -- the same launches;
    float atomics in the reductions keep two runs of either kind from being bit-identical (tests/test_gpu_nlspn.py holds the ProxyTTA
    handle to the same figures)."""
    g = np.load(os.path.join(golden_dir, BASELINE_SEQ + '.npz'))
    h, w, n, steps = [int(x) for x in g['meta']]
    res = []
    for graph in (0, 1):
        eng, sd, adapted = make('baseline', n, h, w, hp_of(g))
        assert eng.get_option('graph') == 0
        eng.set_option('graph', graph)
        for s in range(3):
            raw, image1, sparse = frame(s, h, w, n)
            info, depth = eng.step(image1, sparse, loss_image=raw, want_depth=True)
            d_eval = eng.forward_eval(image1, sparse)
        torch.cuda.synchronize()
        res.append((info.clone(), depth.clone(), d_eval.clone()))
        eng.close()
    a, b = res
    assert rel_mae(b[1], a[1]) < 1e-4 and rel_mae(b[2], a[2]) < 1e-4
    np.testing.assert_allclose(b[0].cpu().numpy(), a[0].cpu().numpy(), rtol=1e-3)
    assert rel_mae(b[2], g['s2/depth_eval']) < NORTH_STAR


def test_baseline_allocates_for_n_frames_not_2n():
    """One pass per training forward: every activation of the baseline handle holds N frames where the ProxyTTA handle's holds [real | proxy]."""
    base, sd, _ = make('baseline', 2, 32, 64, HP)
    proxy = Engine(2, 32, 64, backbone='nlspn', **HP)
    for name in ('image', 'fe1', 'conv3.1.out', 'fe6'):
        assert 2 * base.debug_tensor(name).numel() == proxy.debug_tensor(name).numel(), name
    with pytest.raises(RuntimeError, match='unknown debug tensor'):
        base.debug_tensor('rgb1')                       # conv1_rgb writes its slice of fe1 directly
    assert proxy.debug_tensor('rgb1').numel() == 2 * 2 * 32 * 64 * 48
    base.close()
    proxy.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_create_refusals_return_38_with_a_reason():
    for adapt_mode in ('meta_bn', 'meta'):
        for kw, why in ((dict(backbone='msg_chn'), 'NLSPN backbone only'), (dict(backbone='costdcnet', max_predict_depth=8.0), 'NLSPN backbone only'),
                        (dict(backbone='nlspn', dtype='mixed'), 'PTTA_DTYPE_MIXED'), (dict(backbone='nlspn', syncbn_adapted=True), 'no heads to append')):
            with pytest.raises(RuntimeError, match=r'\(-38\).*PTTA_META_NONE.*' + why):
                Engine(1, 32, 64, meta='none', adapt_mode=adapt_mode, **dict(HP, **kw))


def _refused(eng, calls, why):
    for name, call in calls:
        rc = call()
        assert rc == -38, (name, rc)
        assert why in eng.lib.ptta_last_error(eng.handle), (name, eng.lib.ptta_last_error(eng.handle))


def _exchange_and_head_calls(eng, image1, sparse, buf, cb):
    lib, h, P = eng.lib, eng.handle, _lib.ptr
    f1 = torch.zeros(1024, device='cuda')
    has = ctypes.c_int(0)
    exchange = [('ptta_set_stat_sync', lambda: lib.ptta_set_stat_sync(h, ctypes.cast(cb, ctypes.c_void_p), None, ctypes.c_void_p(buf.data_ptr()), 4096, 2)),
                ('ptta_set_stat_sync_rccl', lambda: lib.ptta_set_stat_sync_rccl(h, None, ctypes.c_void_p(buf.data_ptr()), 4096, 1)),
                ('ptta_set_grad_sync_rccl', lambda: lib.ptta_set_grad_sync_rccl(h, None))]
    heads = [('ptta_head_set_form', lambda: lib.ptta_head_set_form(h, 0)),
             ('ptta_head_bind', lambda: lib.ptta_head_bind(h, b'proj.0.bias', P(f1), P(f1), P(f1))),
             ('ptta_head_set_hparams', lambda: lib.ptta_head_set_hparams(h, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.999, -1, None)),
             ('ptta_head_reload', lambda: lib.ptta_head_reload(h, None)),
             ('ptta_head_forward', lambda: lib.ptta_head_forward(h, P(image1), P(sparse), 1, None, None, None)),
             ('ptta_head_backward', lambda: lib.ptta_head_backward(h, P(f1), None)),
             ('ptta_head_adam_step', lambda: lib.ptta_head_adam_step(h, None)),
             ('ptta_head_step', lambda: lib.ptta_head_step(h, P(image1), P(sparse), 1, P(f1), None)),
             ('ptta_head_get_grad', lambda: lib.ptta_head_get_grad(h, b'proj.0.bias', P(f1), 1024, ctypes.byref(has), None))]
    return exchange, heads


def test_source_handle_refuses_everything_but_the_eval_forward_and_stays_usable(golden_dir):
    g = np.load(os.path.join(golden_dir, SOURCE_EVAL[0] + '.npz'))
    h, w, n, _ = [int(x) for x in g['meta']]
    eng, sd, adapted = make('source', n, h, w, hp_of(g))
    lib, H, P = eng.lib, eng.handle, _lib.ptr
    raw, image1, sparse = frame(0, h, w, n)
    before = eng.forward_eval(image1, sparse).clone()
    out, info = torch.empty_like(sparse), torch.empty(4, device='cuda')
    cb = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_longlong, ctypes.c_void_p)(lambda *a: 0)
    buf = torch.zeros(4096, dtype=torch.float64, device='cuda')
    train = [('ptta_forward_train', lambda: lib.ptta_forward_train(H, P(image1), P(sparse), P(out), None, None, None)),
             ('ptta_step', lambda: lib.ptta_step(H, P(image1), P(raw), P(sparse), None, P(out), P(info), None)),
             ('ptta_backward', lambda: lib.ptta_backward(H, P(out), None, None, None, None)),
             ('ptta_adam_step', lambda: lib.ptta_adam_step(H, None, None, None))]
    exchange, heads = _exchange_and_head_calls(eng, image1, sparse, buf, cb)
    _refused(eng, train, b'adapts nothing')
    _refused(eng, exchange, b'more than one rank is not offered')
    _refused(eng, heads, b'has no heads')
    # ... and the handle is what it was
    after = eng.forward_eval(image1, sparse)
    assert torch.equal(before, after) and rel_mae(after, g['depth_eval']) < BOUND['source_eval']
    eng.close()


def test_baseline_handle_refuses_exchanges_and_heads_and_stays_usable(golden_dir):
    g = np.load(os.path.join(golden_dir, BASELINE_FIRST[0] + '.npz'))
    h, w, n, _ = [int(x) for x in g['meta']]
    eng, sd, adapted = make('baseline', n, h, w, hp_of(g))
    raw, image1, sparse = frame(0, h, w, n)
    cb = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_longlong, ctypes.c_void_p)(lambda *a: 0)
    buf = torch.zeros(4096, dtype=torch.float64, device='cuda')
    exchange, heads = _exchange_and_head_calls(eng, image1, sparse, buf, cb)
    _refused(eng, exchange, b'more than one rank is not offered')
    _refused(eng, heads, b'has no heads')
    with pytest.raises(RuntimeError, match=r'\(-38\).*eval_bn_fused'):       # batch statistics: there is no constant affine to fuse
        eng.set_option('eval_bn_fused', 0)
    info, depth = eng.step(image1, sparse, loss_image=raw, want_depth=True)
    assert rel_mae(depth, g['s0/depth_train']) < BOUND['depth_train'] and rel_mae(eng.forward_eval(image1, sparse), g['s0/depth_eval']) < BOUND['depth_eval']
    eng.close()


# ---- the façade ------------------------------------------------------------------------------------------------------------------------
def _facade(prepared=False):
    from proxytta.model import ExternalModel_Adapt
    model = ExternalModel_Adapt('nlspn', 0.0, 80.0, max_input_depth=80.0, device=torch.device('cuda'))
    if prepared:
        model._prepare_head(PREPARE)
    model.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in source_state_dict(with_head=prepared).items()})
    model.model.fill_holes = False         # the fixtures hold the eval output before hole filling
    return model


def test_facade_pretrain_is_the_source_model_not_the_proxytta_network(golden_dir):
    g = np.load(os.path.join(golden_dir, SOURCE_EVAL[0] + '.npz'))
    h, w, n, _ = [int(x) for x in g['meta']]
    raw, image1, sparse = frame(0, h, w, n)
    eng, sd, adapted = make('source', n, h, w, HP)
    want = eng.forward_eval(image1, sparse).clone()
    eng.close()
    model = _facade()
    model.eval()
    for out in (model.forward(image1, sparse), model.forward(image1, sparse, loss_type='pretrain'), model.forward(image1, sparse, loss_type='eval_time')):
        assert torch.equal(out, want)                       # the reference's default loss_type, and a string without adapt / selfsup / meta / head
    assert rel_mae(want, g['depth_eval']) < BOUND['source_eval']
    model.train()
    with pytest.raises(NotImplementedError, match='every parameter'):
        model.forward(image1, sparse, loss_type='pretrain')
    with pytest.raises(RuntimeError, match="adapt_parameters\\('meta_bn'\\)"):
        model.forward(image1, sparse, loss_type='pretrain_bn')
    # a prepared model holding the same checkpoint in its stage-3 form: 'pretrain' is still the source model, the TTA string is another network
    prepared = _facade(prepared=True)
    prepared.eval()
    assert torch.equal(prepared.forward(image1, sparse, loss_type='pretrain'), want)
    tta = prepared.forward(image1, sparse, loss_type=LOSS_TYPE)
    assert rel_mae(tta, want) > 1e-2, 'the ProxyTTA eval forward (meta conv, batch statistics) cannot equal the source model'


def test_facade_baseline_loop_reproduces_the_fused_step(golden_dir):
    """src/tta_main.py:610-633 on the model whose head was never prepared: forward('pretrain_bn') -> compute_loss(embedding=None, reference=None)
    -> backward -> torch.optim.Adam.step -> eval forward('pretrain'); then the fused step() on a fresh model."""
    g = np.load(os.path.join(golden_dir, BASELINE_FIRST[0] + '.npz'))
    h, w, n, steps = [int(x) for x in g['meta']]
    hp = hp_of(g)
    names = [str(x) for x in g['adapted_names']]
    raw, image1, sparse = frame(0, h, w, n)
    validity = torch.where(sparse > 0, torch.ones_like(sparse), sparse)
    outs = []
    for fused_step in (False, True):
        model = _facade()
        params = model.adapt_parameters(mode='meta_bn')
        named = dict(model.model.model.named_parameters())
        assert len(params) == 86 and [id(p) for p in params] == [id(named[k]) for k in names]
        opt = torch.optim.Adam(params, lr=hp['lr'], betas=hp['betas'], eps=hp['eps'], weight_decay=hp['weight_decay'])
        model.model.bind_optimizer(opt)
        model.train()
        adapted = {k: (named[k].detach(),) for k in names}
        if fused_step:
            model.model.set_hparams(w_sparse_depth=hp['w_sparse_depth'], w_smoothness=hp['w_smoothness'], w_cos=hp['w_cos'])
            info, depth = model.step(image1, sparse, loss_image=raw, want_depth=True)
            assert float(info[3]) == 0.0
            grads = {k: model.model._engine(image1).grad(k, named[k].detach()) for k in names}
        else:
            depth, emb, ref = model.forward(image=image1, sparse_depth=sparse, loss_type='pretrain_bn')
            assert emb is None and ref is None
            loss, li = model.compute_loss(input_rgb=raw, output_depth=depth, sparse_depth=sparse, validity_map=validity, embedding=emb, reference=ref,
                                          w_loss_sparse_depth=hp['w_sparse_depth'], w_loss_smoothness=hp['w_smoothness'], w_loss_cos=hp['w_cos'], loss_type='adapt')
            opt.zero_grad()
            loss.backward()
            assert all(named[k].grad is not None for k in names) and named['conv1_rgb.0.weight'].grad is None
            grads = {k: named[k].grad.clone() for k in names}
            opt.step()
            info = torch.stack([torch.as_tensor(li[k]).detach().float().cuda() for k in ('loss', 'loss_smooth', 'loss_sparse_depth', 'loss_cos')])
            assert float(li['loss_cos']) == 0.0
        model.eval()
        d_eval = model.forward(image1, sparse, loss_type='pretrain')          # the baseline engine's batch-statistics eval forward
        check(first_step_figs(g, info, depth.detach(), d_eval, grads, adapted))
        outs.append((depth.detach().clone(), d_eval.clone()))
    assert torch.equal(outs[0][0], outs[1][0])            # the split calls and the fused step run the same training forward
    assert rel_mae(outs[0][1], outs[1][1]) < BOUND['depth_eval']
