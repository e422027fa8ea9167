"""The 2layers meta block (Res_Conv) on the NLSPN and CostDCNet engines against vectors generated from the real reference
(tests/golden/make_golden_2layers_generic.py: nlspn2l_*, costdcnet2l_*, head_*2l_*).  The frozen oracles know only the 1layer
conv, so every comparison here is against those vectors.

Bounds: depth / eval depth of NLSPN hold the north-star 1e-3 at every step; every other bound is twice the figure measured on
MI355X, written beside it."""
import os

import numpy as np
import pytest
import torch

from proxytta import synth
from proxytta.engine import Engine
from tests.test_gpu_costdcnet import MAX_DEPTH, costdc_frame
from tests.test_gpu_fullsize import _check_map
from tests.test_gpu_head_trainer import GENERIC_HEAD_PARAMS, GENERIC_HEAD_TARGETS, _rows_check
from tests.test_gpu_nlspn import nlspn_frame
from tests.util import rel_mae

pytestmark = pytest.mark.gpu

TWO = 'meta_selfsup_seq_2layers_ema'
BLOCK = 'conv1_rgb_meta.conv1_meta.'
TWICE = tuple(BLOCK + k for k in ('0.1.weight', '0.1.bias', '2.weight', '2.bias'))

# first-step bounds per backbone / mode (2x the worst figure measured on MI355X over the vectors, in brackets): gradient rel. MAE of a stored
# tensor, gradient-norm rtol over all listed entries, parameter rel. MAE after Adam (Adam's first step turns every sign flip of a near-zero
# gradient entry into a 2 lr difference), training depth rel. MAE, loss-term rtol (the cosine term of the zero-image proxy pass, whose
# near-constant maps meet the block's BatchNorm first: 3.0e-3 with matrix-core products, in exact arithmetic within 2e-3)
# 'naive': PTTA_CONV_IMPL=naive, direct fp32 kernels everywhere
# eval: the post-update eval depth of the first step -- the north-star 1e-3 except CostDCNet with matrix-core products, whose arg-max over the
# cost volume turns the block's first Adam move into 1.77e-3 on costdcnet2l_64x96 (1.2e-4 at 72x100, 1.2e-4 in exact arithmetic)
# mixed grad: conv6.1.weight, a 512-channel BatchNorm over the 2 x 4 pixels of a 32 x 64 frame's last map, 1.61e-1 (4.5e-2 at 352x1216)
TOL = {('nlspn', 'fp32'): dict(grad=2.8e-2, gnorm=9e-3, param=2.6e-3, depth=1e-4, loss=6e-3, eval=1e-3),    # (1.38e-2, -, 1.28e-3, 1.4e-6)
       ('nlspn', 'mixed'): dict(grad=3.3e-1, gnorm=4.6e-2, param=1.3e-2, depth=4e-4, loss=6e-3, eval=1e-3),  # (1.61e-1, 2.3e-2, 6.2e-3, 1.4e-6)
       ('nlspn', 'naive'): dict(grad=7e-3, gnorm=9e-3, param=8e-5, depth=1e-5, loss=2e-3, eval=1e-3),        # (3.4e-3, -, 3.8e-5, 2.4e-7)
       ('costdcnet', 'fp32'): dict(grad=5.1e-2, gnorm=1e-2, param=3.1e-2, depth=2e-5, loss=2e-3, eval=3.6e-3,
                                     later=7e-3),                                # (2.53e-2, -, 1.50e-2, 3.1e-6; second step 3.5e-3)
       ('costdcnet', 'naive'): dict(grad=1.6e-2, gnorm=1e-2, param=1.3e-4, depth=1e-5, loss=2e-3, eval=1e-3)}    # (7.6e-3, -, 6.2e-5, 2.0e-6)
# after the first update the trajectories separate: the post-update eval depth of the second step of nlspn2l_32x64 (lr 1e-3) is 1.43e-3
# from the reference's with matrix-core products and 9.7e-4 in exact arithmetic -- later steps are bounded at 3e-3, the sequence test
# holds the reference's own floor beside them (CostDCNet with matrix-core products: `later` of its entry)
LATER = 3e-3


def golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + '.npz'))


def hp_of(g, backbone):
    h = [float(x) for x in g['hp']]
    hp = dict(lr=h[0], betas=(h[1], h[2]), eps=h[3], weight_decay=h[4], w_sparse_depth=h[5], w_smoothness=h[6], w_cos=h[7])
    hp['max_input_depth'] = h[8] if backbone == 'nlspn' else None
    return hp


def state_dict(backbone):
    if backbone == 'nlspn':
        return {k: v for k, v in synth.formula_state_dict_nlspn(TWO).items() if v.dtype == np.float32}
    sd = synth.formula_state_dict_costdcnet(TWO)
    for k in list(sd):            # one BatchNorm behind two names
        if k.startswith('enc2d.') and '.downsample.1.' in k:
            sd[k] = sd[k.replace('.downsample.1.', '.norm3.')]
    return sd


def make(backbone, n, h, w, hp, legacy=False, dtype='fp32', impl='default'):
    """impl 'naive': direct fp32 kernels everywhere (PTTA_CONV_IMPL=naive: exact arithmetic, the tight check)"""
    os.environ.pop('PTTA_CONV_IMPL', None)
    if impl == 'naive':
        os.environ['PTTA_CONV_IMPL'] = 'naive'
    try:
        if backbone == 'nlspn':
            eng = Engine(n, h, w, backbone='nlspn', legacy_offset=legacy, meta='2layers', dtype=dtype, **hp)
        else:
            eng = Engine(n, h, w, backbone='costdcnet', max_predict_depth=MAX_DEPTH, meta='2layers', dtype=dtype, **hp)
    finally:
        os.environ.pop('PTTA_CONV_IMPL', None)
    sd = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in state_dict(backbone).items()}
    eng.load_state_dict(sd)
    adapted = {}
    for k in eng.adapted:
        p = sd[k].clone().contiguous()
        adapted[k] = (p, torch.zeros_like(p), torch.zeros_like(p))
        eng.bind_adapted(k, *adapted[k])
    return eng, sd, adapted


def frame(backbone, s, h, w, n, g):
    if backbone == 'nlspn':
        return [torch.from_numpy(x).cuda() for x in nlspn_frame(s, h, w, n)]
    density = float(g['density']) if 'density' in g.files else 0.05
    return [torch.from_numpy(x).cuda() for x in costdc_frame(s, h, w, n, density)]


def _values(got, g, key):
    """(mine, reference): the full tensor under `key`, or its WSAMP sampled values under 'wsamp/' + key (NLSPN's 110,592-value block
    weights)"""
    a = got.detach().float().cpu().numpy().reshape(-1)
    if key in g.files:
        return a, g[key].reshape(-1)
    return a[g['wsamp_idx']], g['wsamp/' + key]


def _tensor_check(got, g, key, bound, what):
    e = rel_mae(*_values(got, g, key))
    assert e < bound, (what, key, e)
    return e


def _zero_grad(key):
    """the bias of the conv in front of the block's last BatchNorm: its gradient is zero up to rounding (the reference's ~1e-7), so Adam's
    first step moves each entry by +-lr in whichever direction the rounding points"""
    return key.endswith(BLOCK + '1.bias')


def run_vector(g, backbone, dtype='fp32', sampled=False, impl='default'):
    """Steps of one vector: training depth and loss terms every step, first-step gradients of every adapted tensor (norms of all
    listed entries, full or sampled maps where stored), parameters after Adam, post-update eval depth.  Returns the measured figures."""
    h, w, n, steps = [int(x) for x in g['meta'][:4]]
    tol = TOL[(backbone, 'naive' if impl == 'naive' else dtype)]
    legacy = bool(int(g['legacy'])) if 'legacy' in g.files else False
    eng, sd, adapted = make(backbone, n, h, w, hp_of(g, backbone), legacy, dtype, impl)
    listed = [str(x) for x in g['adapted_names']]
    meas = {'depth': [], 'eval': []}
    for s in range(steps):
        raw, image1, sparse = frame(backbone, s, h, w, n, g)
        info, depth = eng.step(image1, sparse, loss_image=raw, want_depth=True)
        p = 's%d/' % s
        dt_bound = tol['depth'] if s == 0 else tol.get('later', LATER)
        if sampled:
            _check_map(depth, g, p + 'depth_train', dt_bound)
        else:
            meas['depth'].append(rel_mae(depth, g[p + 'depth_train']))
            assert meas['depth'][-1] < dt_bound, (s, meas['depth'][-1])
        # (atol: the smoothness term is ~4e-5 on CostDCNet's frames; its second-step value moves by 4.6e-7)
        np.testing.assert_allclose(info.cpu().numpy(), g[p + 'loss_info'], rtol=tol['loss'] if s == 0 else tol.get('later', LATER), atol=1e-6)
        if s == 0:
            if p + 'grad_norms' in g.files:
                gn = np.array([float(eng.grad(k, adapted[k][0]).double().norm()) for k in listed])
                # (atol: the mathematically zero bias gradient, ~1e-7 on both sides)
                np.testing.assert_allclose(gn, g[p + 'grad_norms'], rtol=tol['gnorm'], atol=1e-5)
                meas['gnorm'] = float(np.max(np.abs(gn - g[p + 'grad_norms']) / np.maximum(np.abs(g[p + 'grad_norms']), 1e-6)))
            eg, ep = [0.0], [0.0]
            for k in eng.adapted:
                key = p + 'grad/' + k
                if key in g.files or 'wsamp/' + key in g.files:
                    if _zero_grad(key):
                        mine, want = _values(adapted[k][0], g, p + 'param/' + k)
                        assert float(eng.grad(k, adapted[k][0]).abs().max()) < 1e-4, k
                        assert np.abs(mine - want).max() <= 2.0 * float(g['hp'][0]) * eng.adapted_repeat[k] + 1e-6, k
                        continue
                    eg.append(_tensor_check(eng.grad(k, adapted[k][0]), g, key, tol['grad'], 'grad'))
                    ep.append(_tensor_check(adapted[k][0], g, p + 'param/' + k, tol['param'], 'param'))
            meas['grad'], meas['param'] = max(eg), max(ep)
            assert all(p + 'grad/' + k in g.files or 'wsamp/' + p + 'grad/' + k in g.files for k in eng.adapted if k.startswith(BLOCK))
        d_eval = eng.forward_eval(image1, sparse)
        if sampled:
            _check_map(d_eval, g, p + 'depth_eval', 1e-3)
        else:
            meas['eval'].append(rel_mae(d_eval, g[p + 'depth_eval']))
            assert meas['eval'][-1] < (tol['eval'] if s == 0 else tol.get('later', LATER)), (s, meas['eval'][-1])
    eng.close()
    print('measured', backbone, dtype, impl, {k: v for k, v in meas.items() if v != []})
    return meas


def test_adapted_lists_are_the_references(golden_dir):
    """Unique names = the vector's list without its second occurrences; the repeat counts rebuild the listed list (97 / 41 entries)."""
    for backbone, name, n_unique in (('nlspn', 'nlspn2l_32x64', 93), ('costdcnet', 'costdcnet2l_64x96', 37)):
        g = golden(golden_dir, name)
        listed = [str(x) for x in g['adapted_names']]
        h, w, n = [int(x) for x in g['meta'][:3]]
        eng, _, _ = make(backbone, n, h, w, hp_of(g, backbone))
        unique = list(dict.fromkeys(listed))
        assert eng.adapted == unique and len(unique) == n_unique and len(listed) == n_unique + 4
        assert eng.adapted[:7] == [k for k in listed if k.startswith(BLOCK)][:7]
        assert all(eng.adapted_repeat[k] == listed.count(k) for k in eng.adapted)
        assert [k for k in eng.adapted if eng.adapted_repeat[k] == 2] == list(TWICE)
        eng.close()


@pytest.mark.parametrize('name', ['nlspn2l_32x64', 'nlspn2l_32x64_legacy', 'nlspn2l_40x56_n2_legacy'])
@pytest.mark.parametrize('dtype', ['fp32', 'mixed'])
def test_nlspn_step_matches_reference(golden_dir, name, dtype):
    run_vector(golden(golden_dir, name), 'nlspn', dtype)


def test_nlspn_step_in_exact_arithmetic(golden_dir):
    run_vector(golden(golden_dir, 'nlspn2l_32x64'), 'nlspn', impl='naive')


@pytest.mark.parametrize('dtype', ['fp32', 'mixed'])
def test_nlspn_full_size_step_matches_reference(golden_dir, dtype):
    """352x1216, one step: sampled pixels, block means and checksums of both depth maps, all listed gradient norms, the block's
    weights at sampled indices."""
    run_vector(golden(golden_dir, 'nlspn2l_352x1216_legacy'), 'nlspn', dtype, sampled=True)


@pytest.mark.parametrize('dtype,impl', [('fp32', 'default'), ('mixed', 'default'), ('fp32', 'naive')])
def test_nlspn_sequence_follows_the_reference(golden_dir, dtype, impl):
    """One parameter set adapted over eight different 96x320 frames, the scored (post-update eval) depth after every step.  The fixture
    holds the reference run again with one adapted weight one ulp off (`alt/`): with the 2layers block its own trajectory leaves itself by
    3.6e-5 after one frame, 6.4e-4 after five and 1.3e-3 after eight.  Asserted: the north-star 1e-3 while the reference is within half of
    it, afterwards the order of that floor (3x + 5e-4, as for CostDCNet's sequence)."""
    g = golden(golden_dir, 'nlspn2l_96x320_legacy_seq8')
    h, w, n, steps = [int(x) for x in g['meta'][:4]]
    floor = [rel_mae(g['alt/s%d/depth_eval_pix' % s], g['s%d/depth_eval_pix' % s]) for s in range(steps)]
    assert floor[0] < 1e-4 and floor[-1] > 1e-3                       # the fixture's own statement
    eng, _, _ = make('nlspn', n, h, w, hp_of(g, 'nlspn'), True, dtype, impl)
    errs = []
    for s in range(steps):
        raw, image1, sparse = frame('nlspn', s, h, w, n, g)
        eng.step(image1, sparse, loss_image=raw)
        d_eval = eng.forward_eval(image1, sparse).detach().cpu().numpy().reshape(-1)
        errs.append(rel_mae(d_eval[g['pix_idx']], g['s%d/depth_eval_pix' % s]))
    eng.close()
    print('measured seq8', dtype, impl, ['%.2e' % e for e in errs], 'floor', ['%.2e' % f for f in floor])
    for s, (e, f) in enumerate(zip(errs, floor)):
        assert e < (1e-3 if f < 5e-4 else 3.0 * f + 5e-4), (s, e, f)


@pytest.mark.parametrize('name', ['costdcnet2l_64x96', 'costdcnet2l_72x100_pad'])
@pytest.mark.parametrize('impl', ['naive', 'default'])
def test_costdcnet_step_matches_reference(golden_dir, name, impl):
    run_vector(golden(golden_dir, name), 'costdcnet', impl=impl)


def test_costdcnet_full_size_step_matches_reference(golden_dir):
    run_vector(golden(golden_dir, 'costdcnet2l_480x640'), 'costdcnet', sampled=True)


@pytest.mark.parametrize('backbone,dtype', [('nlspn', 'fp32'), ('nlspn', 'mixed'), ('costdcnet', 'fp32')])
def test_two_runs_of_one_handle_are_bitwise_equal(golden_dir, backbone, dtype):
    """No atomics on the block's path (the wide weight gradient reduces its partials in a fixed order).  CostDCNet: the same two steps
    from the same start give the same bits.  NLSPN: the forwards give the same bits -- its propagation backward accumulates the offset /
    affinity gradients with atomics (nlspn_prop.hip), so its step is not bitwise run to run with any meta layer."""
    g = golden(golden_dir, 'nlspn2l_32x64' if backbone == 'nlspn' else 'costdcnet2l_64x96')
    h, w, n = [int(x) for x in g['meta'][:3]]
    eng, sd, adapted = make(backbone, n, h, w, hp_of(g, backbone), dtype=dtype)
    if backbone == 'nlspn':
        raw, image1, sparse = frame(backbone, 0, h, w, n, g)
        runs = [[t.clone() for t in eng.forward_train(image1, sparse)] + [eng.forward_eval(image1, sparse).clone()] for _ in range(2)]
        assert all(torch.equal(a, b) for a, b in zip(*runs))
        eng.close()
        return
    start = {k: v[0].clone() for k, v in adapted.items()}
    buffers = {k: v.clone() for k, v in sd.items()}           # running statistics of the tracked BatchNorm, bound and updated in place
    runs = []
    for _ in range(2):
        for k, (p, m, v) in adapted.items():
            p.copy_(start[k]); m.zero_(); v.zero_()
        for k, v in buffers.items():
            sd[k].copy_(v)
        eng.set_adam_step(0)
        out = []
        for s in range(2):
            raw, image1, sparse = frame(backbone, s, h, w, n, g)
            info, depth = eng.step(image1, sparse, loss_image=raw, want_depth=True)
            out += [depth.clone(), info.clone()] + [eng.grad(k, adapted[k][0]).clone() for k in adapted]
        out += [adapted[k][0].clone() for k in adapted] + [eng.forward_eval(image1, sparse).clone()]
        runs.append(out)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    eng.close()


@pytest.mark.parametrize('backbone', ['nlspn', 'costdcnet'])
def test_reference_style_facade_loop(golden_dir, backbone):
    """src/tta_main.py:309-354, 610-633 against the mirror: ExternalModel_Adapt -> _prepare_head(2layers) -> load weights ->
    adapt_parameters('meta_bn') (97 / 41 entries, duplicates included) -> torch.optim.Adam -> forward / compute_loss / backward / step.
    torch >= 2.0 on the GPU defaults to the foreach Adam, which steps a duplicated tensor with one bias correction; foreach=False is what
    the reference's torch 1.10.1 runs."""
    from proxytta.model import ExternalModel_Adapt
    name = 'nlspn2l_32x64' if backbone == 'nlspn' else 'costdcnet2l_64x96'
    g = golden(golden_dir, name)
    h, w, n, steps = [int(x) for x in g['meta'][:4]]
    hp = hp_of(g, backbone)
    if backbone == 'nlspn':
        model = ExternalModel_Adapt('nlspn', 0.0, 80.0, max_input_depth=80.0, device=torch.device('cuda'))
        sd = synth.formula_state_dict_nlspn(TWO)
        tol = TOL[('nlspn', 'fp32')]
    else:
        model = ExternalModel_Adapt('costdcnet', 0.1, MAX_DEPTH, max_input_depth=None, device=torch.device('cuda'))
        sd = synth.formula_state_dict_costdcnet(TWO)
        tol = TOL[('costdcnet', 'fp32')]
    model._prepare_head(TWO)
    model.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    params = model.adapt_parameters(mode='meta_bn')
    listed = [str(x) for x in g['adapted_names']]
    named = dict(model.model.model.named_parameters())
    assert [id(p) for p in params] == [id(named[k]) for k in listed]
    opt = torch.optim.Adam(params, lr=hp['lr'], betas=hp['betas'], eps=hp['eps'], weight_decay=hp['weight_decay'], foreach=False)
    for s in range(1):
        raw, image1, sparse = frame(backbone, s, h, w, n, g)
        validity = torch.where(sparse > 0, torch.ones_like(sparse), sparse)
        model.train()
        depth, emb, ref = model.forward(image=image1, sparse_depth=sparse, loss_type='adapt_meta_selfsup_seq_ema_reverse')
        loss, info = model.compute_loss(input_rgb=raw, output_depth=depth, sparse_depth=sparse, validity_map=validity, embedding=emb,
                                        reference=ref, w_loss_sparse_depth=hp['w_sparse_depth'], w_loss_smoothness=hp['w_smoothness'],
                                        w_loss_cos=hp['w_cos'], loss_type='adapt')
        opt.zero_grad()
        loss.backward()
        opt.step()
        p = 's%d/' % s
        assert rel_mae(depth, g[p + 'depth_train']) < (tol['depth'] if s == 0 else 1e-3)
        if s == 0:
            for k in dict.fromkeys(listed):
                key = p + 'param/' + k
                if (key in g.files or 'wsamp/' + key in g.files) and not _zero_grad(k):
                    _tensor_check(named[k], g, key, tol['param'], 'facade param')
                if p + 'exp_avg/' + k in g.files and not _zero_grad(k):
                    _tensor_check(opt.state[named[k]]['exp_avg'], g, p + 'exp_avg/' + k, tol['grad'], 'facade exp_avg')
            for k in TWICE:           # stepped twice per step(): torch's count of this tensor is twice the others'
                assert float(opt.state[named[k]]['step']) == 2.0 * float(opt.state[named[listed[0]]]['step'])
        model.eval()
        with torch.no_grad():
            d_eval = model.forward(image=image1, sparse_depth=sparse, loss_type='adapt_meta_selfsup_seq_ema_reverse')
        assert rel_mae(d_eval, g[p + 'depth_eval']) < tol['eval']


@pytest.mark.parametrize('name', ['head_nlspn2l_forward_48x80_n2', 'head_costdcnet2l_forward_64x96_n2'])
def test_stage2_head_trainer_on_a_2layers_handle(golden_dir, name):
    """ptta_head_* on a 2layers handle: the backbone prefix now holds the block, whose two BatchNorm2d evaluate from their loaded
    running statistics like every other BatchNorm2d under train(prepare=True).  Embeddings, loss and the twelve gradients of the first
    step, then the trained parameters."""
    from tests.golden.make_golden_head_generic import perturbed_target
    z = golden(golden_dir, name)
    backbone = name.split('_')[1][:-2]
    h, w, n, steps = (int(v) for v in z['meta'][:4])
    lr, b1, b2, eps, wd, tau = (float(v) for v in z['hp'])
    if backbone == 'nlspn':
        from tests.test_gpu_nlspn import HP as BHP
        eng = Engine(n, h, w, backbone='nlspn', legacy_offset=True, meta='2layers', **BHP)
        sd_np = synth.formula_state_dict_nlspn(TWO)
    else:
        from tests.test_gpu_costdcnet import HP as BHP
        eng = Engine(n, h, w, backbone='costdcnet', max_predict_depth=MAX_DEPTH, meta='2layers', **BHP)
        sd_np = state_dict('costdcnet')
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
    eng.set_head_hparams(tau=tau, adam_step=0, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for s in range(steps):
        image, sparse = frame(backbone, s, h, w, n, z)[1:]
        emb, ref = eng.head_forward(image, sparse, False)
        loss = eng.head_backward()
        p = 's%d/' % s
        idx = z[p + 'row_idx']
        np.testing.assert_allclose(emb.cpu().numpy()[idx], z[p + 'emb_rows'], rtol=2e-3, atol=5e-4 if s == 0 else 8e-3)
        np.testing.assert_allclose(ref.cpu().numpy()[idx], z[p + 'ref_rows'], rtol=2e-3, atol=5e-4 if s == 0 else 8e-3)
        assert abs(float(loss) - float(z[p + 'loss'])) < (5e-5 if s == 0 else 3e-4), (s, float(loss), float(z[p + 'loss']))
        if s == 0:
            for k in GENERIC_HEAD_PARAMS:
                key = p + 'grad/' + k
                g = eng.head_grad(k, sd[k]).cpu().numpy()
                want = z[key] if key in z.files else z[key + '#rows']
                mine = g if key in z.files else g[np.linspace(0, g.shape[0] - 1, want.shape[0]).astype(np.int64)]
                if np.abs(want).max() < 1e-7:            # a bias in front of a BatchNorm: mathematically zero
                    assert np.abs(mine).max() < 1e-5, k
                    continue
                assert rel_mae(mine, want) < 2e-2, k
        eng.head_adam_step()
    torch.cuda.synchronize()
    last = 's%d/after/' % (steps - 1)
    for k in GENERIC_HEAD_PARAMS:
        _rows_check(z, last + k, sd[k], 0, 2.5 * lr * steps, k)
    eng.close()


def test_refusals_carry_a_message():
    """2layers with the SyncBN-adapted set (either backbone) and CostDCNet 2layers in mixed mode stay -38, with a message."""
    hp = dict(lr=1e-3, max_input_depth=80.0)
    for kw in (dict(backbone='nlspn', syncbn_adapted=True), dict(backbone='nlspn', syncbn_adapted=True, legacy_offset=True),
               dict(backbone='costdcnet', syncbn_adapted=True, max_predict_depth=MAX_DEPTH),
               dict(backbone='costdcnet', dtype='mixed', max_predict_depth=MAX_DEPTH)):
        with pytest.raises(RuntimeError, match=r'ptta_create failed \(-38\): configuration not on the accelerated path .*2layers'):
            Engine(1, 64, 96, meta='2layers', **dict(hp, **kw))
