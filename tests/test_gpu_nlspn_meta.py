"""NLSPN adapt_mode 'meta' (src/nlspn_model_adapt.py:302-311; include/ptta.h PTTA_ADAPT_META_ONLY) against the golden vectors generated from the
real reference (tests/golden/make_golden_nlspn_meta.py): the meta conv alone adapts; every BatchNorm2d normalises with batch statistics in
train-mode passes, writes no buffer, and with its LOADED running statistics and gamma / beta in the scored eval forward -- there as a
constant affine in the convolution's epilogue (option "eval_bn_fused").

Bounds (BOUND below) = 2 x the error of the fp32 engine against the fixtures measured on the MI355X (profiles/nlspn_adapt_meta.txt), as every
other gradient bound of the project; depths as relative MAE, gradients relative to max |g|.  The scored post-update depth must besides stay
inside the north-star 1e-3 at every step of the six-frame sequence.  The fixtures' eval depths are the output BEFORE hole filling (a few
exact zeros per frame, see the generator), which is what the engine returns."""
import ctypes
import os

import numpy as np
import pytest
import torch

from proxytta import _lib
from proxytta.engine import Engine
from tests.nlspn_meta_cases import META_NAMES, PREPARE, bn2d_prefixes, meta_state_dict
from tests.test_gpu_nlspn import nlspn_frame
from tests.util import rel_mae

pytestmark = pytest.mark.gpu
LOSS_TYPE = 'adapt_meta_selfsup_seq_ema_reverse'
NORTH_STAR = 1e-3

# 2 x the measured figures of profiles/nlspn_adapt_meta.txt (worst over the fixtures that have the quantity)
#                  measured:  2.011e-6          5.409e-6       3.119e-3        7.236e-4        2.134e-5       2.740e-4
BOUND = dict(depth_train=4.1e-6, loss=1.09e-5, grad_w=6.3e-3, grad_b=1.45e-3, param=4.3e-5, depth_eval=5.5e-4,
             seq_depth_eval=6.2e-4, seq_param=4.6e-4)          # measured: 3.099e-4 (step 5 of six), 2.274e-4 (the bias after six steps)


def hp_of(g):
    lr, b1, b2, eps, wd, w_sd, w_sm, w_cos, mid = [float(x) for x in g['hp']]
    return dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, w_sparse_depth=w_sd, w_smoothness=w_sm, w_cos=w_cos, max_input_depth=mid)


def make_meta(n, h, w, hp, legacy=False, adapt_mode='meta', drop=()):
    eng = Engine(n, h, w, backbone='nlspn', legacy_offset=legacy, adapt_mode=adapt_mode, **hp)
    sd = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in meta_state_dict().items()}
    eng.load_state_dict({k: v for k, v in sd.items() if v.dtype == torch.float32 and k not in drop})
    adapted = {}
    for k in eng.adapted:
        p = sd[k].clone().contiguous()
        adapted[k] = (p, torch.zeros_like(p), torch.zeros_like(p))
        eng.bind_adapted(k, *adapted[k])
    return eng, sd, adapted


def gerr(a, b):
    """gradient error relative to the gradient's largest entry"""
    b = torch.from_numpy(np.asarray(b)).to(a.device)
    return float((a - b).abs().max() / b.abs().max())


def check(figs):
    for k, v in figs:
        print('FIG %-16s %.3e   (bound %.3e)' % (k, v, BOUND[k.split('[')[0]]))
    for k, v in figs:
        assert v < BOUND[k.split('[')[0]], (k, v)


@pytest.mark.parametrize('name', ['nlspn_meta_32x64', 'nlspn_meta_40x56_n2'])
def test_first_step_matches_golden(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    h, w, n, steps = [int(x) for x in g['meta']]
    eng, sd, adapted = make_meta(n, h, w, hp_of(g), legacy=bool(int(g['legacy'])))
    assert eng.adapted == [str(x) for x in g['adapted_names']] == META_NAMES
    raw, image1, sparse = [torch.from_numpy(x).cuda() for x in nlspn_frame(0, h, w, n)]
    info, depth = eng.step(image1, sparse, loss_image=raw, want_depth=True)
    d_eval = eng.forward_eval(image1, sparse)
    wn, bn = META_NAMES
    ref_info = g['s0/loss_info']
    figs = [('depth_train', rel_mae(depth, g['s0/depth_train'])),
            ('loss', float(np.max(np.abs(info.cpu().numpy() - ref_info) / np.abs(ref_info)))),
            ('grad_w', gerr(eng.grad(wn, adapted[wn][0]), g['s0/grad/' + wn])), ('grad_b', gerr(eng.grad(bn, adapted[bn][0]), g['s0/grad/' + bn])),
            ('param[w]', rel_mae(adapted[wn][0], g['s0/param/' + wn])), ('param[b]', rel_mae(adapted[bn][0], g['s0/param/' + bn])),
            ('depth_eval', rel_mae(d_eval, g['s0/depth_eval']))]
    eng.close()
    check(figs)
    assert figs[-1][1] < NORTH_STAR


def test_six_frame_sequence_matches_golden_at_every_step(golden_dir):
    """Floor: the reference against itself with one adapted weight one ulp off is 2.6e-5 .. 2.3e-4 over these six steps (`alt_rel_mae`)."""
    g = np.load(os.path.join(golden_dir, 'nlspn_meta_32x64_seq6.npz'))
    h, w, n, steps = [int(x) for x in g['meta']]
    assert steps == 6
    eng, sd, adapted = make_meta(n, h, w, hp_of(g))
    figs = []
    for s in range(steps):
        raw, image1, sparse = [torch.from_numpy(x).cuda() for x in nlspn_frame(s, h, w, n)]
        eng.step(image1, sparse, loss_image=raw)
        figs.append(('seq_depth_eval[%d]' % s, rel_mae(eng.forward_eval(image1, sparse), g['s%d/depth_eval' % s])))
        figs += [('seq_param[%d,%s]' % (s, k[-1]), rel_mae(adapted[k][0], g['s%d/param/%s' % (s, k)])) for k in META_NAMES]
    eng.close()
    check(figs)
    for k, v in figs:
        if k.startswith('seq_depth_eval'):
            assert v < NORTH_STAR, (k, v)


@pytest.mark.parametrize('shape', [(1, 32, 64), (2, 40, 56)])
def test_fused_and_unfused_eval_forwards_are_bit_identical(shape):
    n, h, w = shape
    hp = dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1, max_input_depth=80.0)
    eng, sd, adapted = make_meta(n, h, w, hp, legacy=True)
    assert eng.get_option('eval_bn_fused') == 1
    raw, image1, sparse = [torch.from_numpy(x).cuda() for x in nlspn_frame(0, h, w, n)]
    eng.step(image1, sparse, loss_image=raw)
    fused = eng.forward_eval(image1, sparse).clone()
    eng.set_option('eval_bn_fused', 0)
    assert eng.get_option('eval_bn_fused') == 0
    unfused = eng.forward_eval(image1, sparse).clone()
    eng.set_option('eval_bn_fused', 1)
    again = eng.forward_eval(image1, sparse).clone()
    eng.close()
    assert bool((fused > 0).any()) and torch.isfinite(fused).all()
    assert torch.equal(fused, unfused), 'max |fused - unfused| = %.3e' % float((fused - unfused).abs().max())
    assert torch.equal(fused, again)


def test_no_batchnorm2d_buffer_or_affine_parameter_is_written(golden_dir):
    g = np.load(os.path.join(golden_dir, 'nlspn_meta_32x64_seq6.npz'))
    h, w, n, steps = [int(x) for x in g['meta']]
    eng, sd, adapted = make_meta(n, h, w, hp_of(g))
    for s in range(steps):
        raw, image1, sparse = [torch.from_numpy(x).cuda() for x in nlspn_frame(s, h, w, n)]
        eng.step(image1, sparse, loss_image=raw)
        eng.forward_eval(image1, sparse)
    prefixes = bn2d_prefixes(sd)
    assert len(prefixes) == 43            # every BatchNorm2d of the backbone: 35 of ResNet34, conv6, four decoders, the three *_dec1 heads
    for pre in prefixes:
        for leaf in ('running_mean', 'running_var', 'weight', 'bias'):
            assert torch.equal(eng.debug_tensor(pre + '.' + leaf), sd[pre + '.' + leaf]), pre + '.' + leaf
    eng.close()


def test_adapted_list_is_the_meta_conv():
    hp = dict(lr=1e-3, w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1, max_input_depth=80.0)
    eng, sd, adapted = make_meta(1, 32, 64, hp)
    assert int(eng.lib.ptta_adapted_count(eng.handle)) == 2
    assert eng.adapted == META_NAMES and eng.adapted_numel == {META_NAMES[0]: 48 * 48 * 9, META_NAMES[1]: 48}
    assert all(eng.adapted_repeat[k] == 1 for k in META_NAMES)
    raw, image1, sparse = [torch.from_numpy(x).cuda() for x in nlspn_frame(0, 32, 64, 1)]
    eng.step(image1, sparse, loss_image=raw)
    assert float(eng.grad(META_NAMES[0], adapted[META_NAMES[0]][0]).abs().max()) > 0
    for name in ('conv2.0.bn1.weight', 'conv6.1.bias', 'conv3.0.downsample.1.weight'):          # adapted under 'meta_bn', frozen here
        with pytest.raises(RuntimeError, match='not an adapted parameter'):
            eng.grad(name, sd[name])
        with pytest.raises(RuntimeError, match='not an adapted parameter'):
            eng.bind_adapted(name, sd[name], sd[name], sd[name])
    eng.close()


def test_refusals_return_38_with_a_reason():
    hp = dict(lr=1e-3, w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1, max_input_depth=80.0)
    lib = _lib.load()
    # at create: before anything is allocated, the reason in ptta_last_error(NULL)
    for kw, why in ((dict(backbone='msg_chn'), 'only the NLSPN adapter'), (dict(backbone='costdcnet', max_predict_depth=8.0), 'only the NLSPN adapter'),
                    (dict(backbone='nlspn', meta='2layers'), 'PTTA_META_2LAYERS'), (dict(backbone='nlspn', dtype='mixed'), 'PTTA_DTYPE_MIXED'),
                    (dict(backbone='nlspn', syncbn_adapted=True), 'SyncBatchNorm')):
        with pytest.raises(RuntimeError, match=r'\(-38\).*' + why):
            Engine(1, 32, 64, adapt_mode='meta', **dict(hp, **kw))
    # the option belongs to meta-only handles
    plain = Engine(1, 32, 64, backbone='nlspn', **hp)
    with pytest.raises(RuntimeError, match=r'\(-38\).*eval_bn_fused'):
        plain.set_option('eval_bn_fused', 0)
    v = ctypes.c_int(7)
    assert lib.ptta_get_option(plain.handle, b'eval_bn_fused', ctypes.byref(v)) == -38
    plain.close()
    # on a meta-only handle: no statistics / gradient exchange; the handle stays as it was and usable
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'nlspn_meta_32x64.npz'))
    eng, sd, adapted = make_meta(1, 32, 64, hp_of(g))
    with pytest.raises(RuntimeError, match=r'\(-22\).*out of range'):
        eng.set_option('eval_bn_fused', 2)
    cb = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_longlong, ctypes.c_void_p)(lambda *a: 0)
    buf = torch.zeros(4096, dtype=torch.float64, device='cuda')
    calls = (lambda: lib.ptta_set_stat_sync(eng.handle, ctypes.cast(cb, ctypes.c_void_p), None, ctypes.c_void_p(buf.data_ptr()), 4096, 2),
             lambda: lib.ptta_set_stat_sync_rccl(eng.handle, None, ctypes.c_void_p(buf.data_ptr()), 4096, 1),
             lambda: lib.ptta_set_grad_sync_rccl(eng.handle, None))
    for call in calls:
        assert call() == -38
        assert b'not offered' in lib.ptta_last_error(eng.handle)
    raw, image1, sparse = [torch.from_numpy(x).cuda() for x in nlspn_frame(0, 32, 64, 1)]
    info, depth = eng.step(image1, sparse, loss_image=raw, want_depth=True)
    assert rel_mae(depth, g['s0/depth_train']) < NORTH_STAR and rel_mae(eng.forward_eval(image1, sparse), g['s0/depth_eval']) < NORTH_STAR
    eng.close()


def test_state_dict_without_running_statistics_fails_at_the_eval_forward_by_name():
    hp = dict(lr=1e-3, w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1, max_input_depth=80.0)
    eng, sd, adapted = make_meta(1, 32, 64, hp, drop=('conv4.1.bn2.running_var',))           # the load itself succeeds
    raw, image1, sparse = [torch.from_numpy(x).cuda() for x in nlspn_frame(0, 32, 64, 1)]
    out = torch.full((1, 1, 32, 64), -5.0, device='cuda')
    rc = eng.lib.ptta_forward_eval(eng.handle, _lib.ptr(image1), _lib.ptr(sparse), _lib.ptr(out), None)
    torch.cuda.synchronize()
    assert rc == -3 and b'conv4.1.bn2.running_var' in eng.lib.ptta_last_error(eng.handle)
    assert bool((out == -5.0).all())                     # nothing was normalised with zeros and ones
    eng.step(image1, sparse, loss_image=raw)             # train-mode passes need no buffer
    eng.load_state_dict({'conv4.1.bn2.running_var': sd['conv4.1.bn2.running_var']})
    assert torch.isfinite(eng.forward_eval(image1, sparse)).all()
    eng.close()


def _facade(mode):
    from proxytta.model import ExternalModel_Adapt
    model = ExternalModel_Adapt('nlspn', 0.0, 80.0, max_input_depth=80.0, device=torch.device('cuda'))
    model._prepare_head(PREPARE)
    model.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in meta_state_dict().items()})
    model.model.fill_holes = False         # the fixtures hold the eval output before hole filling
    params = model.adapt_parameters(mode=mode)
    named = dict(model.model.model.named_parameters())
    assert len(params) == 2 and [id(p) for p in params] == [id(named[k]) for k in META_NAMES]
    return model, params, named


@pytest.mark.parametrize('mode', ['meta', 'meta_fix'])
def test_facade_reference_style_driver_and_fused_step(golden_dir, mode):
    """src/tta_main.py:610-633, :729-736 against the façade in adapt_mode 'meta' / 'meta_fix' (the same numbers): forward -> compute_loss ->
    backward -> torch.optim.Adam.step -> eval forward; then the fused step() on a fresh model; then a 'meta_bn' engine made afterwards on
    the same model object still reproduces nlspn_32x64.npz."""
    g = np.load(os.path.join(golden_dir, 'nlspn_meta_32x64.npz'))
    h, w, n, steps = [int(x) for x in g['meta']]
    hp = hp_of(g)
    raw, image1, sparse = [torch.from_numpy(x).cuda() for x in nlspn_frame(0, h, w, n)]
    validity = torch.where(sparse > 0, torch.ones_like(sparse), sparse)
    outs = []
    for fused_step in (False, True):
        model, params, named = _facade(mode)
        opt = torch.optim.Adam(params, lr=hp['lr'], betas=hp['betas'], eps=hp['eps'], weight_decay=hp['weight_decay'])
        model.model.bind_optimizer(opt)
        model.train()
        if fused_step:
            model.model.set_hparams(w_sparse_depth=hp['w_sparse_depth'], w_smoothness=hp['w_smoothness'], w_cos=hp['w_cos'])
            info, depth = model.step(image1, sparse, loss_image=raw, want_depth=True)
            info = info.cpu().numpy()
        else:
            depth, emb, ref = model.forward(image=image1, sparse_depth=sparse, loss_type=LOSS_TYPE)
            loss, li = model.compute_loss(input_rgb=raw, output_depth=depth, sparse_depth=sparse, validity_map=validity, embedding=emb, reference=ref,
                                          w_loss_sparse_depth=hp['w_sparse_depth'], w_loss_smoothness=hp['w_smoothness'], w_loss_cos=hp['w_cos'], loss_type='adapt')
            opt.zero_grad()
            loss.backward()
            assert all(named[k].grad is not None for k in META_NAMES) and named['conv2.0.bn1.weight'].grad is None
            figs = [('grad_w', gerr(named[META_NAMES[0]].grad, g['s0/grad/' + META_NAMES[0]])), ('grad_b', gerr(named[META_NAMES[1]].grad, g['s0/grad/' + META_NAMES[1]]))]
            opt.step()
            info = np.array([float(torch.as_tensor(li[k]).detach()) for k in ('loss', 'loss_smooth', 'loss_sparse_depth', 'loss_cos')])
            check(figs)
        model.eval()
        d_eval = model.forward(image1, sparse, loss_type=LOSS_TYPE)
        check([('depth_train', rel_mae(depth.detach(), g['s0/depth_train'])), ('loss', float(np.max(np.abs(info - g['s0/loss_info']) / np.abs(g['s0/loss_info'])))),
               ('param[w]', rel_mae(named[META_NAMES[0]].detach(), g['s0/param/' + META_NAMES[0]])),
               ('param[b]', rel_mae(named[META_NAMES[1]].detach(), g['s0/param/' + META_NAMES[1]])), ('depth_eval', rel_mae(d_eval, g['s0/depth_eval']))])
        outs.append((depth.detach().clone(), d_eval.clone()))
        last = model
    assert torch.equal(outs[0][0], outs[1][0])            # the split calls and the fused step run the same training forward
    # switching the mode releases the engines; 'meta_bn' on the formula weights is what it was
    from proxytta import synth
    assert last.model._engines
    g0 = np.load(os.path.join(golden_dir, 'nlspn_32x64.npz'))
    last.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.formula_state_dict_nlspn().items()})
    params = last.adapt_parameters(mode='meta_bn')
    assert len(params) == 88 and not last.model._engines
    opt = torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    last.model.bind_optimizer(opt)
    last.model.set_hparams(w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1)
    last.train()
    info, depth = last.step(image1, sparse, loss_image=raw, want_depth=True)
    assert rel_mae(depth, g0['s0/depth_train']) < 1e-4
    np.testing.assert_allclose(info.cpu().numpy(), g0['s0/loss_info'], rtol=2e-3)
    last.eval()
    assert rel_mae(last.forward(image1, sparse, loss_type=LOSS_TYPE), g0['s0/depth_eval']) < NORTH_STAR
