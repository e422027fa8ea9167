"""SURVEY.md 8f-4 on the GPU: the stage-2 head trainer (ptta_head_* behind Engine.head_*) against the REAL reference's
fixtures (tests/golden/head_*.npz, make_golden_head.py) and against the oracle at a size the fixtures do not hold."""
import os

import numpy as np
import pytest
import torch

from oracle import head_oracle as HO
from proxytta import synth
from proxytta.engine import HEAD_PARAMS, HEAD_TARGETS, Engine
from tests.golden.make_golden_head import perturbed_target
from tests.util import ONE, TWO

pytestmark = pytest.mark.gpu


MODES = ['exact', 'default']          # PTTA_ARITH=exact: fp32 matrix-core arithmetic everywhere (v_mfma_f32_32x32x2_f32); default: bf16x3


def make_head_engine(n, h, w, hp, tau, bind_target=True, mode='default'):
    os.environ.pop('PTTA_ARITH', None)
    if mode == 'exact':
        os.environ['PTTA_ARITH'] = 'exact'
    try:
        eng = Engine(n, h, w, dtype='fp32', max_input_depth=80.0)
    finally:
        os.environ.pop('PTTA_ARITH', None)
    sd_np = synth.formula_state_dict(ONE, 1.0)
    sd_np.update(perturbed_target(sd_np))
    sd = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in sd_np.items()}
    eng.load_state_dict(sd)
    for name in eng.adapted:
        eng.bind_adapted(name, sd[name], torch.zeros_like(sd[name]), torch.zeros_like(sd[name]))
    moments = {}
    for k in HEAD_PARAMS:
        moments[k] = (torch.zeros_like(sd[k]), torch.zeros_like(sd[k]))
        eng.bind_head(k, sd[k], *moments[k])
    if bind_target:
        for k in HEAD_TARGETS:
            eng.bind_head(k, sd[k])
    eng.set_head_hparams(tau=tau, adam_step=0, **hp)
    return eng, sd, sd_np, moments


def _check(z, key, value, rtol, atol, what):
    value = value.detach().cpu().numpy() if torch.is_tensor(value) else np.asarray(value)
    if key in z.files:
        np.testing.assert_allclose(value, z[key], rtol=rtol, atol=atol, err_msg=what)
        return
    idx = np.linspace(0, value.shape[0] - 1, 24).astype(np.int64)
    np.testing.assert_allclose(value[idx], z[key + '#rows'], rtol=rtol, atol=atol, err_msg=what)
    s = z[key + '#sum']
    assert abs(value.sum(dtype=np.float64) - s[0]) <= rtol * s[1] + atol * value.size, what


# Gradient bounds = 2x the worst figure measured on MI355X (tools/grad_report.py, round 3), per arithmetic mode:
#   (worst |entry error| / largest |entry|,  mean |error| / mean |entry|)          first step          later steps
#   exact    (fp32 products): the kernels themselves                               5.7e-6 / 3.6e-6     3.8e-3 / 3.7e-5
#   default  (bf16x3 products, 2^-17 operand error)                                2.0e-2 / 2.4e-3     1.6e-2 / 7.8e-3
# The reference's own fp32 gradients sit 1e-6 from an fp64 evaluation of the same step (well conditioned), so the exact-mode bound
# is the regression detector for linear_wgrad_kernel / the fused BatchNorm-backward transforms: a defect of a few 1e-5 fails it.
# The default-mode figures are ReLU-mask flips: a hidden pre-activation within 1e-5 of zero changes side under the two-way
# operand split, and with 192 - 720 embedding rows one flipped row moves an entry of that hidden unit's gradient by up to 1/rows of
# its magnitude (at 352x1216 there are 26,752 rows).  Later steps also carry Adam's first-step sign noise on near-zero entries.
GRAD_TOL = {'exact': {True: (1.2e-5, 8e-6), False: (8e-3, 8e-5)}, 'default': {True: (4e-2, 5e-3), False: (4e-2, 1.6e-2)}}


def _grad_close(mine, want, first, what, mode='default'):
    mine, want = np.asarray(mine, np.float64), np.asarray(want, np.float64)
    if np.abs(want).max() < 1e-8:
        # mathematically ZERO gradient (a bias in front of a BatchNorm: pred.0.bias, proj.0.bias, and proj.3.bias which only
        # shifts pred's pre-BatchNorm hidden): the reference holds rounding noise
        assert np.abs(mine).max() < 1e-6, what
        return
    tmax, tmean = GRAD_TOL[mode][bool(first)]
    d = np.abs(mine - want)
    assert d.max() <= tmax * np.abs(want).max() + 1e-12, (what, d.max(), np.abs(want).max())
    assert d.mean() <= tmean * np.abs(want).mean() + 1e-12, (what, d.mean(), np.abs(want).mean())


def _grad_check(z, key, g, first, what, mode='default'):
    g = g.detach().cpu().numpy()
    if key in z.files:
        _grad_close(g, z[key], first, what, mode)
        return
    idx = np.linspace(0, g.shape[0] - 1, 24).astype(np.int64)
    _grad_close(g[idx], z[key + '#rows'], first, what, mode)
    s = z[key + '#sum']
    assert abs(g.sum(dtype=np.float64) - s[0]) <= GRAD_TOL[mode][bool(first)][1] * s[1], what


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['head_reverse_32x48_n2', 'head_forward_32x48_n2', 'head_reverse_64x96'])
def test_head_trainer_reproduces_reference(golden_dir, name, mode):
    z = np.load(os.path.join(golden_dir, name + '.npz'))
    h, w, n, steps = (int(v) for v in z['meta'])
    lr, b1, b2, eps, wd, tau = (float(v) for v in z['hp'])
    reverse = 'reverse' in str(z['loss_type'])
    eng, sd, _, _ = make_head_engine(n, h, w, dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd), tau, mode=mode)
    for s in range(steps):
        image, sparse = (torch.from_numpy(a).cuda() for a in synth.synthetic_frame(s, h, w, n))
        emb, ref = eng.head_forward(image, sparse, reverse)
        loss = eng.head_backward()
        p = 's%d/' % s
        idx = z[p + 'row_idx']
        np.testing.assert_allclose(emb.cpu().numpy()[idx], z[p + 'emb_rows'], rtol=2e-3, atol=2e-4 if s == 0 else 5e-3)
        np.testing.assert_allclose(ref.cpu().numpy()[idx], z[p + 'ref_rows'], rtol=2e-3, atol=2e-4 if s == 0 else 5e-3)
        assert abs(float(loss) - float(z[p + 'loss'])) < (2e-5 if s == 0 else 1e-4)
        for k in HEAD_PARAMS:
            g = eng.head_grad(k, sd[k])
            assert bool(z[p + 'has_grad/' + k]) == (g is not None), k
            if g is None:
                continue
            _grad_check(z, p + 'grad/' + k, g, s == 0, k, mode)
        eng.head_adam_step()
    torch.cuda.synchronize()
    last = 's%d/after/' % (steps - 1)
    for k in sd:
        if not k.startswith(('proj', 'pred')):
            continue
        if k in HEAD_PARAMS and (not reverse or k.startswith('pred')):
            # Adam's first steps move every entry by ~lr whatever the gradient's size: entries with a near-zero gradient may
            # take the other sign -> bound by the total travel; the gradients above are the tight check
            _check(z, last + k, sd[k], 0, 2.5 * lr * steps, k)
        elif k.endswith('num_batches_tracked'):
            assert int(sd[k]) == int(z[last + k]), k
        elif k.startswith('proj_t.') and not k.endswith(('running_mean', 'running_var')) and not reverse:
            # EMA of a parameter that itself moved by Adam: (1 - tau) * travel
            _check(z, last + k, sd[k], 1e-6, (1 - tau) * 2.5 * lr * steps * steps + 1e-7, k)
        elif 'running' in k:
            # statistics of hidden activations of magnitude ~30, downstream of Adam-updated weights (not reverse: proj.0 itself
            # moved by +-lr per entry and its inputs are O(10))
            _check(z, last + k, sd[k], 2e-4, 1e-3 if reverse else 2e-2, k)
        else:
            # untouched parameters and (reverse) the EMA of the constant proj
            _check(z, last + k, sd[k], 1e-5, 1e-6, k)


def _rel_dev(a, b):
    """(worst |a - b| / largest |b|, mean |a - b| / mean |b|)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b)
    return d.max() / np.abs(b).max(), d.mean() / np.abs(b).mean()


@pytest.mark.parametrize('mode', MODES)
def test_head_trainer_against_oracle_other_shape(mode):
    """A shape and batch the fixtures do not hold, 2 steps each loss type, incl. the EMA and the step counter.
    Gradients are held to an fp64 evaluation of the same steps.  After Adam's first step a hidden pre-activation of this case lands within
    fp32 rounding of zero (9e-8 from it after frame 10): which side of the ReLU it takes depends on the summation order (it differs between
    CPU thread counts), and one flipped row moves that unit's gradients by 1/720 -- the fp32 oracle then sits 7e-4 (mean) from the fp64
    evaluation.  So the bound is GRAD_TOL or twice the fp32 oracle's own distance from fp64, whichever is larger (as for the CostDCNet
    fixtures, make_golden_costdcnet_fp64.py): on a well-conditioned step that is GRAD_TOL itself."""
    n, h, w = 3, 48, 80
    hp = dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    for loss_type in ('head_selfsup_seq_ema_reverse', 'head_selfsup_seq_ema'):
        eng, sd, sd_np, _ = make_head_engine(n, h, w, hp, 0.99, mode=mode)
        o = HO.HeadTrainerOracle(sd_np, loss_type, max_input_depth=80.0, tau=0.99, **hp)
        sd64 = {k: (torch.from_numpy(np.asarray(v)).double() if np.asarray(v).dtype == np.float32 else torch.from_numpy(np.asarray(v)))
                for k, v in sd_np.items()}
        o64 = HO.HeadTrainerOracle(sd64, loss_type, max_input_depth=80.0, tau=0.99, **hp)
        for s in range(2):
            image, sparse = synth.synthetic_frame(10 + s, h, w, n)
            r = o.step(torch.from_numpy(image), torch.from_numpy(sparse))
            r64 = o64.step(torch.from_numpy(image).double(), torch.from_numpy(sparse).double())
            emb, ref = eng.head_forward(torch.from_numpy(image).cuda(), torch.from_numpy(sparse).cuda(), 'reverse' in loss_type)
            loss = eng.head_backward()
            assert abs(float(loss) - r['loss']) < (2e-5 if s == 0 else 1e-4)
            assert set(r['grads']) == set(r64['grads'])
            for k, g in r64['grads'].items():
                mine = eng.head_grad(k, sd[k]).cpu().numpy()
                g = g.numpy()
                if np.abs(g).max() < 1e-8:
                    _grad_close(mine, g, s == 0, k, mode)          # mathematically zero: the fp32 oracle's rounding noise is not a yardstick
                    continue
                tmax, tmean = GRAD_TOL[mode][s == 0]
                omax, omean = _rel_dev(r['grads'][k].numpy(), g)
                dmax, dmean = _rel_dev(mine, g)
                assert dmax <= max(tmax, 2 * omax) + 1e-12, (k, s, dmax, tmax, omax)
                assert dmean <= max(tmean, 2 * omean) + 1e-12, (k, s, dmean, tmean, omean)
            eng.head_adam_step()
        for k in HEAD_TARGETS:
            np.testing.assert_allclose(sd[k].cpu().numpy(), o.P[k].detach().numpy(), rtol=1e-5, atol=0.01 * 2.5 * 5e-4 * 4 + 1e-7, err_msg=k)
        eng.close()


def test_fused_head_step_equals_split_calls():
    n, h, w = 1, 32, 64
    hp = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    out = []
    for fused in (False, True):
        eng, sd, _, _ = make_head_engine(n, h, w, hp, 0.999)
        losses = []
        for s in range(3):
            image, sparse = (torch.from_numpy(a).cuda() for a in synth.synthetic_frame(s, h, w, n))
            if fused:
                losses.append(eng.head_step(image, sparse, True))
            else:
                eng.head_forward(image, sparse, True, want=False)
                losses.append(eng.head_backward())
                eng.head_adam_step()
        torch.cuda.synchronize()
        out.append((torch.cat(losses).cpu(), {k: sd[k].cpu().clone() for k in HEAD_PARAMS + HEAD_TARGETS}))
        eng.close()
    assert torch.equal(out[0][0], out[1][0])
    for k in out[0][1]:
        assert torch.equal(out[0][1][k], out[1][1][k]), k
    assert float(out[0][0][-1]) < float(out[0][0][0])            # the loss goes down


def test_tta_step_after_head_training_uses_the_trained_heads():
    """The same handle adapts afterwards with the heads it just trained: its TTA step equals the oracle's TTA step from the
    trained state dict."""
    from oracle import proxytta_oracle as O
    n, h, w = 1, 32, 64
    hp = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    eng, sd, _, _ = make_head_engine(n, h, w, hp, 0.999)
    for s in range(2):
        image, sparse = (torch.from_numpy(a).cuda() for a in synth.synthetic_frame(s, h, w, n))
        eng.head_step(image, sparse, True)
    torch.cuda.synchronize()
    trained = {k: v.detach().cpu().clone() for k, v in sd.items()}
    image, sparse = synth.synthetic_frame(7, h, w, n)
    o = O.MsgChnOracle(trained, ONE, max_input_depth=80.0, lr=1e-3, w_sd=1.0, w_sm=1.0, w_cos=1.0)
    r = o.step(torch.from_numpy(image), torch.from_numpy(sparse))
    info, depth = eng.step(torch.from_numpy(image).cuda(), torch.from_numpy(sparse).cuda(), want_depth=True)
    assert float((depth.cpu() - r['depth']).abs().mean() / r['depth'].abs().mean()) < 1e-4
    li = r['loss_info']
    np.testing.assert_allclose(info.cpu().numpy(), [li['loss'], li['loss_smooth'], li['loss_sparse_depth'], li['loss_cos']], rtol=5e-4)


def test_head_trainer_refusals():
    eng = Engine(1, 36, 52, dtype='fp32')              # not divisible by 16: the dual-corner padded path
    with pytest.raises(RuntimeError):
        eng.bind_head('pred.0.weight', torch.zeros(512, 512, device='cuda'), torch.zeros(512, 512, device='cuda'), torch.zeros(512, 512, device='cuda'))
    eng.close()
    eng = Engine(1, 32, 48, dtype='fp32')
    with pytest.raises(RuntimeError):
        eng.bind_head('conv1_rgb_meta.weight', torch.zeros(32, 32, 3, 3, device='cuda'), torch.zeros(32, 32, 3, 3, device='cuda'), torch.zeros(32, 32, 3, 3, device='cuda'))
    with pytest.raises(RuntimeError):
        eng.head_backward()
    eng.close()


def _facade(golden_z):
    from proxytta.model import ExternalModel_Adapt
    lr, b1, b2, eps, wd, tau = (float(v) for v in golden_z['hp'])
    model = ExternalModel_Adapt('msg_chn', 0.0, 80.0, max_input_depth=80.0)
    model._prepare_head(ONE)
    head_params = model.prepare_parameters('head_selfsup_ema')            # re-creates the heads (head_main.py:268)
    sd = synth.formula_state_dict(ONE, 1.0)
    sd.update(perturbed_target(sd))
    model.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    opt = torch.optim.Adam(head_params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    return model, head_params, opt


@pytest.mark.parametrize('name', ['head_reverse_32x48_n2', 'head_forward_32x48_n2'])
def test_reference_style_stage2_loop_through_the_facade(golden_dir, name):
    """The loop of src/head_main.py:441-480 written against the mirror: forward(loss_type) -> compute_loss('prepare') ->
    zero_grad / backward / torch.optim.Adam.step; the losses follow the reference's fixture."""
    z = np.load(os.path.join(golden_dir, name + '.npz'))
    h, w, n, steps = (int(v) for v in z['meta'])
    loss_type = str(z['loss_type'])
    model, head_params, opt = _facade(z)
    names = model.model._head_names
    for s in range(steps):
        image, sparse = (torch.from_numpy(a).cuda() for a in synth.synthetic_frame(s, h, w, n))
        model.train(prepare=True)
        output_depth, embedding, reference = model.forward(image=image, sparse_depth=sparse, loss_type=loss_type)
        assert output_depth is None
        loss, info = model.compute_loss(input_rgb=image, output_depth=output_depth, validity_map=None, ground_truth=None,
                                        embedding=embedding, reference=reference, loss_type='prepare')
        opt.zero_grad()
        loss.backward()
        for k, p in zip(names, head_params):
            assert (p.grad is not None) == bool(z['s%d/has_grad/%s' % (s, k)]), k
        opt.step()
        assert abs(float(loss.detach()) - float(z['s%d/loss' % s])) < (2e-5 if s == 0 else 1e-4)
    state = model.model.model.state_dict()
    _check(z, 's%d/after/proj_t.3.weight' % (steps - 1), state['proj_t.3.weight'], 1e-5, 1e-5, 'proj_t.3.weight')
    assert int(state['pred.1.num_batches_tracked']) == steps


def test_facade_fused_head_step_matches_its_unfused_loop(golden_dir):
    z = np.load(os.path.join(golden_dir, 'head_reverse_32x48_n2.npz'))
    h, w, n, steps = (int(v) for v in z['meta'])
    loss_type = str(z['loss_type'])
    model, head_params, opt = _facade(z)
    model.bind_head_optimizer(opt, tau=float(z['hp'][5]))
    for s in range(steps):
        image, sparse = (torch.from_numpy(a).cuda() for a in synth.synthetic_frame(s, h, w, n))
        loss = model.head_step(image, sparse, loss_type)
        assert abs(float(loss.detach()) - float(z['s%d/loss' % s])) < (2e-5 if s == 0 else 1e-4)
    names = model.model._head_names
    st = opt.state[head_params[names.index('pred.3.weight')]]
    assert int(float(st['step'])) == steps and float(st['exp_avg'].abs().sum()) > 0
    assert 'step' not in opt.state[head_params[names.index('proj.0.weight')]] or int(float(opt.state[head_params[names.index('proj.0.weight')]]['step'])) == 0
    state = model.model.model.state_dict()
    _check(z, 's%d/after/pred.3.weight' % (steps - 1), state['pred.3.weight'], 0, 2.5 * float(z['hp'][0]) * steps, 'pred.3.weight')


def test_head_trainer_with_the_2layers_meta_layer():
    """Stage 2 on the `2layers` recipe (Res_Conv(32,128) with train-mode BatchNorm2d in the no-grad backbone pass): two reverse
    steps against the oracle, incl. the meta BatchNorm's running statistics."""
    n, h, w = 2, 32, 64
    hp = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    from proxytta.engine import adapted_names
    eng = Engine(n, h, w, dtype='fp32', max_input_depth=80.0, meta='2layers')
    sd_np = synth.formula_state_dict(TWO, 1.0)
    sd = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in sd_np.items()}
    eng.load_state_dict(sd)
    for name in adapted_names('2layers'):
        eng.bind_adapted(name, sd[name], torch.zeros_like(sd[name]), torch.zeros_like(sd[name]))
    for k in HEAD_PARAMS:
        eng.bind_head(k, sd[k], torch.zeros_like(sd[k]), torch.zeros_like(sd[k]))
    for k in HEAD_TARGETS:
        eng.bind_head(k, sd[k])
    eng.set_head_hparams(tau=0.999, adam_step=0, **hp)
    o = HO.HeadTrainerOracle(sd_np, 'head_selfsup_seq_ema_reverse', max_input_depth=80.0, tau=0.999, prepare_mode=TWO, **hp)
    for s in range(2):
        image, sparse = synth.synthetic_frame(20 + s, h, w, n)
        r = o.step(torch.from_numpy(image), torch.from_numpy(sparse))
        eng.head_forward(torch.from_numpy(image).cuda(), torch.from_numpy(sparse).cuda(), True, want=False)
        loss = eng.head_backward()
        assert abs(float(loss) - r['loss']) < (2e-5 if s == 0 else 1e-4)
        for k, g in r['grads'].items():
            _grad_close(eng.head_grad(k, sd[k]).cpu().numpy(), g.numpy(), s == 0, k)
        eng.head_adam_step()
    for k in sd:
        if 'conv1_rgb_meta' in k and 'running' in k:
            np.testing.assert_allclose(sd[k].cpu().numpy(), o.P[k].numpy(), rtol=1e-4, atol=1e-5, err_msg=k)
    eng.close()


# ---- the same trainer on the generic engine: NLSPN and CostDCNet handles (csrc/ghead.hip) -----------------------------------------------------
GENERIC_HEAD_PARAMS = tuple('%s.%s.%s' % (m, l, t) for m in ('proj', 'pred') for l in ('0', '1', '3') for t in ('weight', 'bias'))
GENERIC_HEAD_TARGETS = tuple('proj_t' + k[4:] for k in GENERIC_HEAD_PARAMS[:6])


def _rows_check(z, key, value, rtol, atol, what):
    value = value.detach().cpu().numpy() if torch.is_tensor(value) else np.asarray(value)
    if key in z.files:
        np.testing.assert_allclose(value, z[key], rtol=rtol, atol=atol, err_msg=what)
        return
    rows = z[key + '#rows']
    idx = np.linspace(0, value.shape[0] - 1, rows.shape[0]).astype(np.int64)
    np.testing.assert_allclose(value[idx], rows, rtol=rtol, atol=atol, err_msg=what)
    s = z[key + '#sum']
    assert abs(value.sum(dtype=np.float64) - s[0]) <= rtol * s[1] + atol * value.size, what


def make_generic_head_engine(backbone, n, h, w, hp, tau, impl='default'):
    from tests.golden.make_golden_head_generic import perturbed_target
    os.environ.pop('PTTA_CONV_IMPL', None)
    if impl == 'naive':
        os.environ['PTTA_CONV_IMPL'] = 'naive'          # direct fp32 kernels everywhere (exact arithmetic)
    if backbone == 'nlspn':
        from tests.test_gpu_nlspn import HP as BHP
        eng = Engine(n, h, w, backbone='nlspn', legacy_offset=True, **BHP)
        os.environ.pop('PTTA_CONV_IMPL', None)
        sd_np = synth.formula_state_dict_nlspn()
    else:
        from tests.test_gpu_costdcnet import HP as BHP, MAX_DEPTH
        eng = Engine(n, h, w, backbone='costdcnet', max_predict_depth=MAX_DEPTH, **BHP)
        sd_np = synth.formula_state_dict_costdcnet()
        os.environ.pop('PTTA_CONV_IMPL', None)
        for k in list(sd_np):            # one BatchNorm behind two names
            if k.startswith('enc2d.') and '.downsample.1.' in k:
                sd_np[k] = sd_np[k.replace('.downsample.1.', '.norm3.')]
    sd_np.update(perturbed_target(sd_np))
    sd = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in sd_np.items()}
    eng.load_state_dict({k: v for k, v in sd.items() if v.dtype == torch.float32} if backbone == 'nlspn' else sd)
    keep = {}
    for k in eng.adapted:
        keep[k] = (sd[k].clone().contiguous(), torch.zeros_like(sd[k]), torch.zeros_like(sd[k]))
        eng.bind_adapted(k, *keep[k])
    moments = {}
    for k in GENERIC_HEAD_PARAMS:
        moments[k] = (torch.zeros_like(sd[k]), torch.zeros_like(sd[k]))
        eng.bind_head(k, sd[k], *moments[k])
    for k in GENERIC_HEAD_TARGETS:
        eng.bind_head(k, sd[k])
    eng.set_head_hparams(tau=tau, adam_step=0, **hp)
    return eng, sd, sd_np, (keep, moments)


def _generic_head_frame(backbone, s, h, w, n):
    if backbone == 'nlspn':
        from tests.test_gpu_nlspn import nlspn_frame
        return nlspn_frame(s, h, w, n)[1:]
    from tests.test_gpu_costdcnet import costdc_frame
    return costdc_frame(s, h, w, n)[1:]


@pytest.mark.parametrize('name', ['head_nlspn_forward_48x80_n2', 'head_nlspn_reverse_48x80_n2', 'head_nlspn_reverse_96x320',
                                  'head_costdcnet_forward_64x96_n2', 'head_costdcnet_reverse_64x96_n2', 'head_costdcnet_reverse_160x224'])
@pytest.mark.parametrize('impl', ['naive', 'default'])
def test_generic_head_trainer_reproduces_reference(golden_dir, name, impl):
    """Stage 2 (src/head_main.py:464-480) on an NLSPN / CostDCNet handle against the REAL reference's vectors
    (tests/golden/make_golden_head_generic.py): embeddings, loss, all twelve gradients per step, then the trained parameters, the EMA target
    and the BatchNorm1d running statistics.  Bounds as for the MSG_CHN trainer's default arithmetic (bf16x3 products): first step 2x measured."""
    backbone = name.split('_')[1]
    z = np.load(os.path.join(golden_dir, name + '.npz'))
    h, w, n, steps = (int(v) for v in z['meta'][:4])
    lr, b1, b2, eps, wd, tau = (float(v) for v in z['hp'])
    reverse = 'reverse' in str(z['loss_type'])
    eng, sd, _, keep = make_generic_head_engine(backbone, n, h, w, dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd), tau, impl)
    rows = int(z['s0/emb_shape'][0])
    for s in range(steps):
        image, sparse = (torch.from_numpy(a).cuda() for a in _generic_head_frame(backbone, s, h, w, n))
        emb, ref = eng.head_forward(image, sparse, reverse)
        loss = eng.head_backward()
        p = 's%d/' % s
        idx = z[p + 'row_idx']
        np.testing.assert_allclose(emb.cpu().numpy()[idx], z[p + 'emb_rows'], rtol=2e-3, atol=5e-4 if s == 0 else 8e-3)
        np.testing.assert_allclose(ref.cpu().numpy()[idx], z[p + 'ref_rows'], rtol=2e-3, atol=5e-4 if s == 0 else 8e-3)
        assert abs(float(loss) - float(z[p + 'loss'])) < (5e-5 if s == 0 else 3e-4), (s, float(loss), float(z[p + 'loss']))
        for k in GENERIC_HEAD_PARAMS:
            g = eng.head_grad(k, sd[k])
            assert g is not None and bool(z[p + 'has_grad/' + k]), k
            g = g.cpu().numpy()
            key = p + 'grad/' + k
            want = z[key] if key in z.files else z[key + '#rows']
            mine = g if key in z.files else g[np.linspace(0, g.shape[0] - 1, want.shape[0]).astype(np.int64)]
            if np.abs(want).max() < 1e-7:            # a bias in front of a BatchNorm: mathematically zero
                assert np.abs(mine).max() < 1e-5, k
                continue
            d = np.abs(mine - want)
            tmax, tmean = GRAD_TOL['exact' if impl == 'naive' else 'default'][s == 0]
            if impl == 'naive':
                # (different reduction orders of the 512 / 1024-wide layers; later steps: behind Adam's +-lr first move of every weight)
                tmax, tmean = (2e-4, 5e-5) if s == 0 else (4e-2, 1.5e-2)      # (measured: first step <= 2e-5 / 5e-6; second step 5.1e-3 mean)
            else:
                # a hidden pre-activation within 1e-5 of zero changes side under the two-way operand split: with R rows one flipped row moves an
                # entry of that unit's gradient by up to 1 / R of its magnitude (12 - 120 rows here; 26,752 on the MSG_CHN handle)
                # -- ONE term of a 12-term sum, which may be several times the mean term: the exact-arithmetic run above is the tight check
                tmax, tmean = tmax + 4.0 / rows, tmean + 0.5 / rows
            assert d.max() <= tmax * np.abs(want).max() + 1e-12, (k, s, d.max(), np.abs(want).max())
            assert d.mean() <= tmean * np.abs(want).mean() + 1e-12, (k, s, d.mean(), np.abs(want).mean())
        eng.head_adam_step()
    torch.cuda.synchronize()
    last = 's%d/after/' % (steps - 1)
    for k in sd:
        if not k.startswith(('proj', 'pred')):
            continue
        if k in GENERIC_HEAD_PARAMS:
            _rows_check(z, last + k, sd[k], 0, 2.5 * lr * steps, k)                      # Adam's +-lr moves: bounded by the total travel
        elif k.endswith('num_batches_tracked'):
            continue                                                                     # int64 buffers are not bound on this engine
        elif k.startswith('proj_t.') and not k.endswith(('running_mean', 'running_var')):
            _rows_check(z, last + k, sd[k], 1e-6, (1 - tau) * 2.5 * lr * steps * steps + 1e-7, k)      # EMA of a parameter that itself moved by Adam
        elif 'running' in k:
            _rows_check(z, last + k, sd[k], 5e-4, 2e-2, k)
    eng.close()


def test_generic_head_step_equals_split_calls_and_feeds_the_tta_step():
    """ptta_head_step = forward + backward + adam_step bit for bit on an NLSPN handle, the loss goes down, and a TTA step on the same handle
    afterwards runs with the trained heads (its embeddings differ from an untrained handle's)."""
    n, h, w = 1, 48, 80
    hp = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    out = []
    for fused in (False, True):
        eng, sd, _, _ = make_generic_head_engine('nlspn', n, h, w, hp, 0.999)
        losses = []
        for s in range(3):
            image, sparse = (torch.from_numpy(a).cuda() for a in _generic_head_frame('nlspn', s, h, w, n))
            if fused:
                losses.append(eng.head_step(image, sparse, True))
            else:
                eng.head_forward(image, sparse, True, want=False)
                losses.append(eng.head_backward())
                eng.head_adam_step()
        torch.cuda.synchronize()
        depth, emb, ref = eng.forward_train(image, sparse)
        out.append((torch.cat(losses).cpu(), {k: sd[k].cpu().clone() for k in GENERIC_HEAD_PARAMS + GENERIC_HEAD_TARGETS}, emb.cpu().clone()))
        eng.close()
    assert torch.equal(out[0][0], out[1][0])
    for k in out[0][1]:
        assert torch.equal(out[0][1][k], out[1][1][k]), k
    assert float(out[0][0][-1]) < float(out[0][0][0])
    assert torch.equal(out[0][2], out[1][2])
    eng, sd, _, _ = make_generic_head_engine('nlspn', n, h, w, hp, 0.999)
    _, emb0, _ = eng.forward_train(image, sparse)
    assert float((emb0.cpu() - out[0][2]).abs().max()) > 1e-3          # the trained heads are the ones the TTA forward runs
    eng.close()


@pytest.mark.parametrize('name', ['head_nlspn_forward_48x80_n2', 'head_costdcnet_reverse_64x96_n2'])
def test_reference_style_stage2_loop_through_the_generic_facades(golden_dir, name):
    """The loop of src/head_main.py:441-480 written against the mirror for the NLSPN / CostDCNet adapters: _prepare_head,
    prepare_parameters('head_selfsup_ema'), torch.optim.Adam over what it returns, train(prepare=True), forward(loss_type) ->
    compute_loss('prepare') -> zero_grad / backward / step.  All twelve head tensors receive a gradient in both directions; losses follow
    the reference's fixture."""
    from proxytta.model import ExternalModel_Adapt
    from tests.golden.make_golden_head_generic import perturbed_target
    backbone = name.split('_')[1]
    z = np.load(os.path.join(golden_dir, name + '.npz'))
    h, w, n, steps = (int(v) for v in z['meta'][:4])
    lr, b1, b2, eps, wd, tau = (float(v) for v in z['hp'])
    loss_type = str(z['loss_type'])
    if backbone == 'nlspn':
        model = ExternalModel_Adapt('nlspn', 0.0, 80.0, max_input_depth=80.0, offset=True)
        sd = synth.formula_state_dict_nlspn()
    else:
        model = ExternalModel_Adapt('costdcnet', 0.1, 8.0, max_input_depth=None)
        sd = {k: v for k, v in synth.formula_state_dict_costdcnet().items() if not (k.startswith('enc2d.') and '.downsample.1.' in k)}
    model._prepare_head(ONE)
    head_params = model.prepare_parameters('head_selfsup_ema')
    sd.update(perturbed_target(sd))
    model.model.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    opt = torch.optim.Adam(head_params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    names = model.model._head_names
    assert len(names) == 12
    for s in range(steps):
        image, sparse = (torch.from_numpy(a).cuda() for a in _generic_head_frame(backbone, s, h, w, n))
        model.train(prepare=True)
        output_depth, embedding, reference = model.forward(image=image, sparse_depth=sparse, loss_type=loss_type)
        assert output_depth is None
        loss, info = model.compute_loss(input_rgb=image, output_depth=output_depth, validity_map=None, ground_truth=None,
                                        embedding=embedding, reference=reference, loss_type='prepare')
        opt.zero_grad()
        loss.backward()
        assert all(p.grad is not None for p in head_params)
        opt.step()
        assert abs(float(loss.detach()) - float(z['s%d/loss' % s])) < (5e-5 if s == 0 else 5e-4), (s, float(loss.detach()), float(z['s%d/loss' % s]))
    state = model.model.model.state_dict()
    _rows_check(z, 's%d/after/proj_t.3.weight' % (steps - 1), state['proj_t.3.weight'], 1e-5, 1e-5, 'proj_t.3.weight')
