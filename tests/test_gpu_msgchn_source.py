"""MSG_CHN's source model (include/ptta.h PTTA_MSGCHN_PLAIN; network._forward, network_exp_msg_chn_adapt.py:418-461) against the golden vectors
generated from the real reference (tests/golden/make_golden_msgchn_source.py): the eval forward of the loaded checkpoint without
conv1_rgb_meta, without the zero-image pass and without the heads.

Bound: SOURCE_EVAL_BOUND[fixture] = 2 x the relative MAE of the engine against that fixture measured on the MI355X
(profiles/msgchn_source.txt), the project's rule; every depth must besides stay inside the north-star 1e-3.
  measured: 1.194e-5 (32x48, and through the facade), 1.253e-5 (32x48, N = 2), 1.173e-5 (36x52, padded)
The identity-meta comparison (the source handle against a ProxyTTA 1layer handle whose meta convolution is the identity) is NOT bit for bit:
the engine's bf16x3 product splits the activation into two bf16 terms (hi + lo, 16 of fp32's 24 mantissa bits) and spends its third MFMA on
the weight's low part, so x . 1 comes back rounded to 16 bits.  Measured: max |m - c2| 7.629e-6 (32x48, N = 2) and 7.510e-6 (36x52) on maps
of order 1, depths 5.147e-6 and 4.570e-6 relative MAE apart -- under the engine's own error against the fixtures.  IDENTITY_BOUND = 2 x the
larger of each."""
import ctypes

import numpy as np
import pytest
import torch

from proxytta import _lib
from proxytta.engine import ADAPTED, Engine
from tests.msgchn_source_cases import MAX_INPUT_DEPTH, ONE, PREPARED, SOURCE_EVAL, TWO, frame, source_state_dict
from tests.test_gpu_nlspn_source import _exchange_and_head_calls, _refused
from tests.util import rel_mae

pytestmark = pytest.mark.gpu
NORTH_STAR = 1e-3
TTA = 'adapt_meta_selfsup_seq_ema_reverse'
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1, max_input_depth=MAX_INPUT_DEPTH)
SOURCE_EVAL_BOUND = {'msgchn_source_32x48': 2.39e-5, 'msgchn_source_32x48_n2': 2.51e-5, 'msgchn_source_36x52_pad': 2.35e-5}
IDENTITY_BOUND = dict(m_abs=1.53e-5, depth=1.03e-5)
NAMES = [c[0] for c in SOURCE_EVAL]

_SD = {}


def weights(stage3=None):
    """The fixtures' state dict on the device, made once per form and never written."""
    if stage3 not in _SD:
        _SD[stage3] = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in source_state_dict(stage3).items()}
    return _SD[stage3]


def make(n, h, w, stage3=None, options=None):
    eng = Engine(n, h, w, backbone='msg_chn', meta='plain', options=options, **HP)
    eng.load_state_dict(weights(stage3))
    return eng


def frames(h, w, n):
    return [torch.from_numpy(x).cuda() for x in frame(h, w, n)]


def golden(golden_dir, name):
    import os
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    return g, [int(x) for x in g['meta'][:3]]


@pytest.mark.parametrize('name', NAMES)
def test_source_eval_matches_golden(golden_dir, name):
    """32 x 48; the same with N = 2; 36 x 52, which takes the dual-corner padding (two network frames per image, mean of the two crops)."""
    g, (h, w, n) = golden(golden_dir, name)
    eng = make(n, h, w)
    assert int(eng.lib.ptta_adapted_count(eng.handle)) == 0 and eng.adapted == [] and eng.rows == 0 and int(eng.lib.ptta_embedding_rows(eng.handle)) == 0
    image, sparse = frames(h, w, n)
    depth = eng.forward_eval(image, sparse).clone()
    again = eng.forward_eval(image, sparse)
    eng.close()
    err = rel_mae(depth, g['depth_eval'])
    print('FIG source_eval[%s] %.3e   (bound %.3e)' % (name, err, SOURCE_EVAL_BOUND[name]))
    assert err < SOURCE_EVAL_BOUND[name] < NORTH_STAR
    assert torch.equal(depth, again)
    assert float(g['tta_eval_rel_mae']) > 1e-2 > err            # the fixture tells the source model from the ProxyTTA network of the same weights


def _identity_meta_engine(n, h, w):
    """A ProxyTTA 1layer handle of the same weights whose meta convolution is the identity: centre tap 1, bias 0."""
    eng = Engine(n, h, w, **HP)
    eng.load_state_dict(weights(ONE))
    wt = torch.zeros(32, 32, 3, 3, device='cuda')
    wt[torch.arange(32), torch.arange(32), 1, 1] = 1.0
    bias = torch.zeros(32, device='cuda')
    keep = [(wt, torch.zeros_like(wt), torch.zeros_like(wt)), (bias, torch.zeros_like(bias), torch.zeros_like(bias))]
    for k, ts in zip(ADAPTED, keep):
        eng.bind_adapted(k, *ts)
    return eng, keep


@pytest.mark.parametrize('name', [NAMES[1], NAMES[2]])
def test_source_is_the_proxytta_network_with_an_identity_meta_conv(golden_dir, name):
    """With the identity as its meta convolution the ProxyTTA handle's `m` is its c2 rounded to two bf16 terms (the header of this file),
    and everything downstream runs the same launches: the two depths differ by that rounding alone."""
    g, (h, w, n) = golden(golden_dir, name)
    image, sparse = frames(h, w, n)
    src = make(n, h, w)
    a = src.forward_eval(image, sparse).clone()
    src.close()
    proxy, keep = _identity_meta_engine(n, h, w)
    b = proxy.forward_eval(image, sparse).clone()
    m, c2 = proxy.debug_tensor('m'), proxy.debug_tensor('c2')
    proxy.close()
    half = m.numel() // 2                                          # the eval forward writes the real half of the [real | proxy] maps
    print('FIG identity_meta[%s] depth max |a - b| %.3e rel MAE %.3e; max |m - c2| %.3e' % (name, float((a - b).abs().max()), rel_mae(a, b),
                                                                                          float((m[:half] - c2[:half]).abs().max())))
    assert float((m[:half] - c2[:half]).abs().max()) < IDENTITY_BOUND['m_abs'] and rel_mae(a, b) < IDENTITY_BOUND['depth']


def _count(eng, key, image, sparse):
    before = eng.get_option(key)
    out = eng.forward_eval(image, sparse).clone()
    return out, eng.get_option(key) - before


@pytest.mark.parametrize('name', [NAMES[0], NAMES[2]])
def test_launch_forms_are_bit_identical(golden_dir, name):
    """Option "graph" (the step's replay: the eval forward is enqueued either way), and each pair of layers as two launches instead of one:
    the same arithmetic in the same order."""
    g, (h, w, n) = golden(golden_dir, name)
    image, sparse = frames(h, w, n)
    eng = make(n, h, w)
    base, tp = _count(eng, 'tpair_fuse_count', image, sparse)
    _, pp = _count(eng, 'pair_fuse_count', image, sparse)
    print('FIG fused launches per eval forward[%s]: transposed pairs %d, strided pairs %d' % (name, tp, pp))
    assert tp == 4 and pp >= 1, (tp, pp)                   # decoder 2's and decoder 3's two transposed pairs each; the small-map strided pairs
    eng.set_option('graph', 1)
    assert torch.equal(eng.forward_eval(image, sparse), base) and torch.equal(eng.forward_eval(image, sparse), base)
    eng.set_option('graph', 0)
    eng.set_option('pair_fuse', 0)
    out, cnt = _count(eng, 'pair_fuse_count', image, sparse)
    assert cnt == 0 and torch.equal(out, base)
    eng.set_option('pair_fuse', 1)
    eng.set_option('tpair_fuse', 0)
    out, cnt = _count(eng, 'tpair_fuse_count', image, sparse)
    assert cnt == 0 and torch.equal(out, base)
    assert eng.debug_tensor('t2').numel() > 0               # the two-launch form writes the intermediate map
    eng.set_option('tpair_fuse', 1)
    assert torch.equal(eng.forward_eval(image, sparse), base)
    with pytest.raises(RuntimeError, match=r'\(-38\).*tpair_fuse'):
        eng.debug_tensor('t2')                              # the fused launch keeps it on chip
    eng.close()


def test_activations_hold_n_frames_not_2n_and_m_does_not_exist():
    src = make(2, 32, 48)
    proxy = Engine(2, 32, 48, **HP)
    for name, per_frame in (('c0', 32 * 48 * 32), ('e3_0', 32 * 48 * 32), ('feat', 8 * 12 * 32), ('c2', 8 * 12 * 32), ('out1', 8 * 12), ('p11', 32 * 48)):
        a, b = src.debug_tensor(name).numel(), proxy.debug_tensor(name).numel()
        assert a == 2 * per_frame and b == 2 * a, (name, a, b)
    assert proxy.debug_tensor('m').numel() == 2 * 2 * 8 * 12 * 32
    for name in ('m', 'emb', 'gW', 'g_feat_f32'):
        with pytest.raises(RuntimeError, match=r'\(-2\).*no debug tensor ' + name):
            src.debug_tensor(name)
    src.close()
    proxy.close()
    # padded sizes double the network batch on both kinds
    src = make(1, 36, 52)
    assert src.debug_tensor('c0').numel() == 2 * 48 * 64 * 32
    src.close()


def test_create_refusals_each_with_its_reason():
    lib = _lib.load()
    hp = _lib.Hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 2.0, 0.1, 80.0, 8.0)
    P = _lib.PTTA_MSGCHN_PLAIN
    M = _lib.PTTA_BACKBONE_MSG_CHN
    cases = [(_lib.PTTA_BACKBONE_NLSPN, P, _lib.PTTA_DTYPE_F32, 'PTTA_MSGCHN_PLAIN: the flag belongs to the MSG_CHN backbone'),
             (_lib.PTTA_BACKBONE_COSTDCNET, P, _lib.PTTA_DTYPE_F32, 'PTTA_MSGCHN_PLAIN: the flag belongs to the MSG_CHN backbone'),
             (M, P | _lib.PTTA_META_2LAYERS, _lib.PTTA_DTYPE_F32, 'PTTA_MSGCHN_PLAIN with PTTA_META_2LAYERS or PTTA_META_NONE'),
             (M, P | _lib.PTTA_META_NONE, _lib.PTTA_DTYPE_F32, 'PTTA_MSGCHN_PLAIN with PTTA_META_2LAYERS or PTTA_META_NONE'),
             (M, P, _lib.PTTA_DTYPE_MIXED, 'PTTA_MSGCHN_PLAIN with PTTA_DTYPE_MIXED'),
             (M, P | _lib.PTTA_NLSPN_LEGACY_OFFSET, _lib.PTTA_DTYPE_F32, 'PTTA_MSGCHN_PLAIN takes no other flag'),
             # the refusals that were there before stay, with their reasons -- also with the new flag OR-ed in
             (M, P | _lib.PTTA_ADAPT_META_ONLY, _lib.PTTA_DTYPE_F32, "only the NLSPN adapter has adapt_mode 'meta'"),
             (M, _lib.PTTA_ADAPT_META_ONLY, _lib.PTTA_DTYPE_F32, "only the NLSPN adapter has adapt_mode 'meta'"),
             (M, _lib.PTTA_META_NONE, _lib.PTTA_DTYPE_F32, 'NLSPN backbone only'),
             (M, _lib.PTTA_COSTDC_PLAIN, _lib.PTTA_DTYPE_F32, 'CostDCNet backbone')]
    for backbone, mode, dtype, word in cases:
        hd = ctypes.c_void_p()
        assert lib.ptta_create(ctypes.byref(hd), backbone, mode, 1, 32, 48, dtype, ctypes.byref(hp)) == -38 and not hd.value, (mode, dtype)
        assert word in lib.ptta_last_error(None).decode(), (word, lib.ptta_last_error(None).decode())
    with pytest.raises(RuntimeError, match=r'\(-38\).*PTTA_MSGCHN_PLAIN with PTTA_DTYPE_MIXED'):
        Engine(1, 32, 48, backbone='msg_chn', meta='plain', dtype='mixed', **HP)
    with pytest.raises(ValueError, match="meta 'plain'"):
        Engine(1, 32, 64, backbone='nlspn', meta='plain', **HP)


def test_everything_but_the_eval_forward_is_refused_and_the_handle_still_works(golden_dir):
    g, (h, w, n) = golden(golden_dir, NAMES[0])
    image, sparse = frames(h, w, n)
    eng = make(n, h, w)
    want = eng.forward_eval(image, sparse).clone()
    lib, H, P = eng.lib, eng.handle, _lib.ptr
    out, info = torch.empty_like(sparse), torch.empty(4, device='cuda')
    cb = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_longlong, ctypes.c_void_p)(lambda *a: 0)
    buf = torch.zeros(4096, dtype=torch.float64, device='cuda')
    validity = (sparse > 0).float()
    train = [('ptta_forward_train', lambda: lib.ptta_forward_train(H, P(image), P(sparse), P(out), None, None, None)),
             ('ptta_step', lambda: lib.ptta_step(H, P(image), None, P(sparse), None, P(out), P(info), None)),
             ('ptta_step_pipelined', lambda: lib.ptta_step_pipelined(H, P(image), None, P(sparse), None, 1, P(image), P(sparse), 2, P(out), P(info), None)),
             ('ptta_forward_eval_last', lambda: lib.ptta_forward_eval_last(H, P(out), None)),
             ('ptta_backward', lambda: lib.ptta_backward(H, P(out), None, None, None, None)),
             ('ptta_adam_step', lambda: lib.ptta_adam_step(H, None, None, None)),
             ('ptta_loss_forward', lambda: lib.ptta_loss_forward(H, P(image), P(out), P(sparse), P(validity), None, None, 0, 1.0, 2.0, 0.1, P(info), None)),
             ('ptta_loss_backward', lambda: lib.ptta_loss_backward(H, P(image), P(out), P(sparse), P(validity), None, None, 0, P(out), None, None))]
    exchange, heads = _exchange_and_head_calls(eng, image, sparse, buf, cb)
    _refused(eng, train, b'adapts nothing')
    _refused(eng, exchange, b'more than one rank is not offered')
    _refused(eng, heads, b'has no heads')
    # the Engine's methods raise the library's reason
    with pytest.raises(RuntimeError, match=r'ptta_step failed \(-38\).*adapts nothing'):
        eng.step(image, sparse)
    with pytest.raises(RuntimeError, match=r'\(-38\).*adapts nothing'):
        eng.forward_train(image, sparse)
    with pytest.raises(RuntimeError, match=r'\(-2\)'):
        eng.bind_adapted('conv1_rgb_meta.weight', *[torch.zeros(32, 32, 3, 3, device='cuda') for _ in range(3)])
    # ... and the handle is what it was, bit for bit
    torch.cuda.synchronize()
    assert torch.equal(eng.forward_eval(image, sparse), want)
    eng.close()


def test_stage0_and_both_stage3_checkpoints_give_the_same_depth(golden_dir):
    g, (h, w, n) = golden(golden_dir, NAMES[0])
    image, sparse = frames(h, w, n)
    outs = []
    for stage3 in (None, ONE, TWO):
        eng = make(n, h, w, stage3)
        outs.append(eng.forward_eval(image, sparse).clone())
        eng.close()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    # a second load into one handle takes effect: another backbone tensor, another depth; the first one back, the first depth
    eng = make(n, h, w)
    sd = dict(weights())
    sd['depth_decoder1.dec1.3.weight'] = sd['depth_decoder1.dec1.3.weight'] * 1.25
    eng.load_state_dict(sd)
    assert rel_mae(eng.forward_eval(image, sparse), outs[0]) > 1e-4
    eng.load_state_dict(weights(TWO))
    assert torch.equal(eng.forward_eval(image, sparse), outs[0])
    eng.close()


def test_image_norm_is_fused_into_the_first_convolution(golden_dir):
    g, (h, w, n) = golden(golden_dir, NAMES[2])                 # the padded size normalises while it pads
    image, sparse = frames(h, w, n)
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    raw = torch.floor(image * 255.0)
    normed = ((raw / 255.0 - torch.tensor(mean, device='cuda').view(1, 3, 1, 1)) / torch.tensor(std, device='cuda').view(1, 3, 1, 1)).contiguous()
    eng = make(n, h, w)
    want = eng.forward_eval(normed, sparse).clone()
    eng.set_image_norm([mean, std])
    got = eng.forward_eval(raw, sparse)
    eng.close()
    # the same network on inputs that agree to fp32 rounding: each result is within the engine's own error of the reference's depth
    assert rel_mae(got, want) < SOURCE_EVAL_BOUND[NAMES[2]]


def _facade(prepare_mode=None, dtype='fp32', tmp_path=None):
    from proxytta.model import ExternalModel_Adapt
    model = ExternalModel_Adapt('msg_chn', 0.0, 80.0, max_input_depth=MAX_INPUT_DEPTH, device=torch.device('cuda'), dtype=dtype)
    if prepare_mode is not None:
        model._prepare_head(prepare_mode)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in source_state_dict(prepare_mode).items()}
    if tmp_path is not None:                                      # restore_model of a checkpoint file
        path = str(tmp_path / 'stage.pth')
        torch.save({'net': sd, 'train_step': 0}, path)
        model.restore_model(path)
    else:
        model.model.load_state_dict(sd)
    return model


def test_facade_pretrain_on_a_never_prepared_and_on_a_prepared_model(golden_dir, tmp_path):
    g, (h, w, n) = golden(golden_dir, NAMES[0])
    gp, _ = golden(golden_dir, PREPARED)
    image, sparse = frames(h, w, n)
    eng = make(n, h, w)
    want = eng.forward_eval(image, sparse).clone()
    eng.close()
    # constructed, restore_model of a stage-0 checkpoint, eval(), forward with its own default argument: no _prepare_head anywhere
    model = _facade(tmp_path=tmp_path)
    model.eval()
    for out in (model.forward(image, sparse), model.forward(image, sparse, loss_type='pretrain'), model.forward(image, sparse, loss_type='pretrain_time')):
        assert torch.equal(out, want)
    assert model.forward(image, sparse, loss_type='get_time')[2] > 0.0
    err = rel_mae(want, g['depth_eval'])
    print('FIG source_eval[facade] %.3e   (bound %.3e)' % (err, SOURCE_EVAL_BOUND[NAMES[0]]))
    assert err < SOURCE_EVAL_BOUND[NAMES[0]]
    with pytest.raises(RuntimeError, match='_prepare_head'):           # the ProxyTTA strings still need the head
        model.forward(image, sparse, loss_type=TTA)
    model.train()
    with pytest.raises(NotImplementedError, match='every parameter'):
        model.forward(image, sparse)
    model.model._clear_engines()
    # a prepared model, in the mixed mode: the source engine is fp32 beside the ProxyTTA engines and answers the prepared fixture
    prepared = _facade(ONE, dtype='mixed')
    opt = torch.optim.Adam(prepared.adapt_parameters('meta'), lr=HP['lr'])
    prepared.model.bind_optimizer(opt)
    prepared.model.set_hparams(w_sparse_depth=HP['w_sparse_depth'], w_smoothness=HP['w_smoothness'], w_cos=HP['w_cos'])
    prepared.eval()
    before = prepared.forward(image, sparse, loss_type='pretrain').clone()
    tta_before = prepared.forward(image, sparse, loss_type=TTA).clone()
    assert torch.equal(before, want) and rel_mae(before, gp['depth_eval']) < SOURCE_EVAL_BOUND[NAMES[0]]
    assert rel_mae(tta_before, before) > 1e-2                         # another network
    assert sorted(k[0] if isinstance(k[0], str) else 'proxytta' for k in prepared.model._engines) == ['proxytta', 'source']
    assert prepared.model._engines[('source', n, h, w)].dtype == 'fp32' and prepared.model._engines[(n, h, w)].dtype == 'mixed'
    prepared.train()
    for _ in range(3):
        prepared.step(image, sparse)
    prepared.eval()
    after = prepared.forward(image, sparse, loss_type='pretrain')
    tta_after = prepared.forward(image, sparse, loss_type=TTA)
    assert torch.equal(after, before)                                 # the meta layer adapts; the source model ignores it
    assert rel_mae(tta_after, tta_before) > 1e-5
    # load_state_dict reloads the source engine with the others; _clear_engines drops it with them
    sd = {k: v.clone() for k, v in prepared.model.model.state_dict().items()}
    sd['depth_decoder1.dec1.3.weight'] = sd['depth_decoder1.dec1.3.weight'] * 1.25
    prepared.model.load_state_dict(sd)
    assert rel_mae(prepared.forward(image, sparse, loss_type='pretrain'), before) > 1e-4
    prepared.model._clear_engines()
    assert prepared.model._engines == {}
