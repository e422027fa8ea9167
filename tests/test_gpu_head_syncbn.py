"""The SyncBatchNorm form of the stage-2 head trainer (include/ptta.h ptta_head_set_form) on the GPU: what the reference's stage 2 always
runs (src/head_main.py:278-279 convert_syncbn() + DDP, src/train_head.py:178 one rank per GPU), against the REAL reference's vectors
(tests/golden/make_golden_head_syncbn.py).  One rank; two ranks over gloo (two processes on the one GPU, as tests/test_gpu_syncbn.py);
one rank on the library's own RCCL communicator."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

from proxytta import _lib
from tests.test_gpu_head_trainer import (GENERIC_HEAD_PARAMS, GENERIC_HEAD_TARGETS, GRAD_TOL, _generic_head_frame, _rows_check,
                                         make_generic_head_engine, make_head_engine)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
SYNCBN = _lib.PTTA_HEAD_FORM_SYNCBN


def _hp(z):
    lr, b1, b2, eps, wd, tau = (float(v) for v in z['hp'])
    return dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd), tau


def _grad_ok(mine, want, first, rows, what):
    if np.abs(want).max() < 1e-7:                 # a bias in front of a BatchNorm: mathematically zero
        assert np.abs(mine).max() < 1e-5, what
        return
    tmax, tmean = GRAD_TOL['default'][first]
    tmax, tmean = tmax + 4.0 / rows, tmean + 0.5 / rows      # ReLU-side flips under the bf16x3 split (test_gpu_head_trainer.py)
    d = np.abs(mine - want)
    assert d.max() <= tmax * np.abs(want).max() + 1e-12, (what, d.max(), np.abs(want).max())
    assert d.mean() <= tmean * np.abs(want).mean() + 1e-12, (what, d.mean(), np.abs(want).mean())


# BatchNorm1d running statistics of hidden units of magnitude ~30 (variances ~1e4): 2x the worst entry measured on MI355X over these fixtures
# (NLSPN proj.1: 4.3e-3 relative on one variance of the two-rank run, 0.089 absolute on a near-zero mean); single entries, a hidden unit
# whose pre-activation changes ReLU side under the bf16x3 split (test_gpu_head_trainer.py GRAD_TOL)
RUN_RTOL, RUN_ATOL = 1e-2, 0.18


def _moment_check(z, key, t, rel):
    """An Adam moment against the reference's; the moments of a mathematically zero gradient (a bias in front of a BatchNorm) are the
    square / running mean of rounding noise on both sides and are held to staying noise."""
    want = z[key] if key in z.files else z[key + '#rows']
    if np.abs(want).max() < (1e-7 if 'exp_avg/' in key else 1e-14):
        assert float(t.abs().max()) < (1e-6 if 'exp_avg/' in key else 1e-12), key
        return
    _rows_check(z, key, t, rel, 3 * rel * float(np.abs(want).max()), key)      # (one entry measured at 1.46x rel x the largest)


def _sampled(z, key, g):
    want = z[key] if key in z.files else z[key + '#rows']
    mine = g if key in z.files else g[np.linspace(0, g.shape[0] - 1, want.shape[0]).astype(np.int64)]
    return mine, want


@pytest.mark.parametrize('name', ['head_syncbn_nlspn_forward_48x80', 'head_syncbn_nlspn_reverse_48x80',
                                  'head_syncbn_costdcnet_forward_64x96', 'head_syncbn_costdcnet_reverse_64x96'])
def test_syncbn_form_reproduces_reference(name):
    """One rank: loss, the twelve gradients per step, then parameters, both Adam moments, the EMA target and the BatchNorm1d buffers.
    proj_t.1 is in eval mode: its running statistics stay bitwise what was loaded."""
    backbone = name.split('_')[2]
    z = np.load(os.path.join(GOLD, name + '.npz'))
    h, w, n, steps = (int(v) for v in z['meta'][:4])
    hp, tau = _hp(z)
    reverse = 'reverse' in str(z['loss_type'])
    eng, sd, _, (_, moments) = make_generic_head_engine(backbone, n, h, w, hp, tau)
    eng.set_head_form(SYNCBN)
    before = {k: sd[k].clone() for k in ('proj_t.1.running_mean', 'proj_t.1.running_var')}
    rows = None
    for s in range(steps):
        image, sparse = (torch.from_numpy(a).cuda() for a in _generic_head_frame(backbone, s, h, w, n))
        emb, _ = eng.head_forward(image, sparse, reverse)
        rows = emb.shape[0]
        loss = eng.head_backward()
        p = 's%d/' % s
        assert abs(float(loss) - float(z[p + 'loss'])) < (5e-5 if s == 0 else 3e-4), (s, float(loss), float(z[p + 'loss']))
        for k in GENERIC_HEAD_PARAMS:
            g = eng.head_grad(k, sd[k])
            assert g is not None and bool(z[p + 'has_grad/' + k]), k
            _grad_ok(*_sampled(z, p + 'grad/' + k, g.cpu().numpy()), s == 0, rows, (k, s))
        eng.head_adam_step()
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(sd[k], v), k                                   # eval mode: buffers untouched
    last = 's%d/' % (steps - 1)
    lr = hp['lr']
    for k in sd:
        if not k.startswith(('proj', 'pred')) or k.endswith('num_batches_tracked'):
            continue
        if k in GENERIC_HEAD_PARAMS:
            _rows_check(z, last + 'after/' + k, sd[k], 0, 2.5 * lr * steps, k)
        elif k.startswith('proj_t.') and not k.endswith(('running_mean', 'running_var')):
            _rows_check(z, last + 'after/' + k, sd[k], 1e-6, (1 - tau) * 2.5 * lr * steps * steps + 1e-7, k)
        elif 'running' in k:
            _rows_check(z, last + 'after/' + k, sd[k], RUN_RTOL, RUN_ATOL, k)
    for k in GENERIC_HEAD_PARAMS:                                          # both Adam moments after the last step
        for which, t, rel in (('exp_avg/', moments[k][0], 5e-2), ('exp_avg_sq/', moments[k][1], 1e-1)):
            _moment_check(z, last + which + k, t, rel)
    eng.close()


@pytest.mark.parametrize('reverse', [True, False])
def test_msg_chn_syncbn_form_is_the_plain_form_on_one_rank(reverse):
    """src/msg_chn_model_adapt.py:435-440: train_prepare is train(), so one rank of the converted model computes the plain form, bit for bit."""
    z = np.load(os.path.join(GOLD, 'head_syncbn_msg_chn_%s_32x48.npz' % ('reverse' if reverse else 'forward')))
    h, w, n, steps = (int(v) for v in z['meta'][:4])
    hp, tau = _hp(z)
    from proxytta import synth
    out = []
    for form in (_lib.PTTA_HEAD_FORM_PLAIN, SYNCBN):
        eng, sd, _, moments = make_head_engine(n, h, w, hp, tau)
        eng.set_head_form(form)
        losses = []
        for s in range(steps):
            image, sparse = (torch.from_numpy(a).cuda() for a in synth.synthetic_frame(s, h, w, n))
            losses.append(eng.head_step(image, sparse, reverse))
        torch.cuda.synchronize()
        out.append((torch.cat(losses).cpu(), {k: v.cpu().clone() for k, v in sd.items() if k.startswith(('proj', 'pred'))},
                    {k: torch.cat([m.reshape(-1), v.reshape(-1)]).cpu() for k, (m, v) in moments.items()}))
        eng.close()
    assert torch.equal(out[0][0], out[1][0])
    for k in out[0][1]:
        assert torch.equal(out[0][1][k], out[1][1][k]), k
    for k in out[0][2]:
        assert torch.equal(out[0][2][k], out[1][2][k]), k
    for s in range(steps):                              # and the converted reference agrees
        assert abs(float(out[1][0][s]) - float(z['s%d/loss' % s])) < (2e-5 if s == 0 else 1e-4)


def test_form_is_chosen_before_the_first_step():
    eng, sd, _, _ = make_generic_head_engine('nlspn', 1, 48, 80, dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0), 0.999)
    with pytest.raises(RuntimeError):
        eng.set_head_form(7)
    eng.set_head_form(SYNCBN)
    image, sparse = (torch.from_numpy(a).cuda() for a in _generic_head_frame('nlspn', 0, 48, 80, 1))
    eng.head_step(image, sparse, True)
    with pytest.raises(RuntimeError):
        eng.set_head_form(_lib.PTTA_HEAD_FORM_PLAIN)
    eng.close()


@pytest.mark.parametrize('backbone', ['nlspn', 'costdcnet'])
def test_facade_stage2_loop_in_head_main_order(backbone):
    """src/head_main.py:259-280 then :407-480 against the façade: _prepare_head, prepare_parameters('head_selfsup_ema'), Adam,
    convert_syncbn(), train(prepare=True), forward / compute_loss('prepare') / backward / step.  The losses follow the SyncBatchNorm
    vectors, the TTA adapted list is untouched (no PTTA_SYNCBN_ADAPT handle), and proj_t.1's running statistics do not move."""
    from proxytta import synth
    from proxytta.model import ExternalModel_Adapt
    from tests.golden.make_golden_head_generic import perturbed_target
    from tests.util import ONE
    name = 'head_syncbn_%s_forward_%s' % (backbone, '48x80' if backbone == 'nlspn' else '64x96')
    z = np.load(os.path.join(GOLD, name + '.npz'))
    h, w, n, steps = (int(v) for v in z['meta'][:4])
    hp, tau = _hp(z)
    if backbone == 'nlspn':
        model = ExternalModel_Adapt('nlspn', 0.0, 80.0, max_input_depth=80.0, offset=True)
        sd = synth.formula_state_dict_nlspn()
    else:
        model = ExternalModel_Adapt('costdcnet', 0.1, 8.0, max_input_depth=None)
        sd = {k: v for k, v in synth.formula_state_dict_costdcnet().items() if not (k.startswith('enc2d.') and '.downsample.1.' in k)}
    model._prepare_head(ONE)
    adapted = list(model.model.adapted)
    head_params = model.prepare_parameters('head_selfsup_ema')
    sd.update(perturbed_target(sd))
    model.model.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    opt = torch.optim.Adam(head_params, lr=hp['lr'], betas=hp['betas'], eps=hp['eps'], weight_decay=hp['weight_decay'])
    model.convert_syncbn()
    model.distributed_data_parallel(rank=0)
    assert list(model.model.adapted) == adapted and not model.model.sync_bn
    state = model.model.model.state_dict()
    rm0 = state['proj_t.1.running_mean'].clone()
    for s in range(steps):
        image, sparse = (torch.from_numpy(a).cuda() for a in _generic_head_frame(backbone, s, h, w, n))
        model.train(prepare=True)
        output_depth, embedding, reference = model.forward(image=image, sparse_depth=sparse, loss_type=str(z['loss_type']))
        loss, info = model.compute_loss(input_rgb=image, output_depth=output_depth, validity_map=None, ground_truth=None,
                                        embedding=embedding, reference=reference, loss_type='prepare')
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert abs(float(loss.detach()) - float(z['s%d/loss' % s])) < (5e-5 if s == 0 else 5e-4), (s, float(loss.detach()), float(z['s%d/loss' % s]))
    state = model.model.model.state_dict()
    assert torch.equal(state['proj_t.1.running_mean'], rm0)
    _rows_check(z, 's%d/after/proj_t.3.weight' % (steps - 1), state['proj_t.3.weight'], 1e-5, 1e-5, 'proj_t.3.weight')


# ---- two ranks over gloo, one frame each: the batch-2 reference run ---------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


TWO_RANK = {'nlspn': 'head_syncbn_nlspn_reverse_48x80_n2', 'costdcnet': 'head_syncbn_costdcnet_reverse_64x96_n2',
            'msg_chn': 'head_syncbn_msg_chn_reverse_32x48_n2'}


def _head_case(backbone, n, h, w, hp, tau):
    """(engine, bound tensors, Adam moments, frame(s) -> (image, sparse) of the fixture's batch, the twelve names, the six proj_t names)"""
    from proxytta import synth
    from proxytta.engine import HEAD_PARAMS, HEAD_TARGETS
    if backbone == 'msg_chn':
        eng, sd, _, moments = make_head_engine(n, h, w, hp, tau)
        return eng, sd, moments, lambda s, nf: synth.synthetic_frame(s, h, w, nf), list(HEAD_PARAMS), list(HEAD_TARGETS)
    eng, sd, _, (_, moments) = make_generic_head_engine(backbone, n, h, w, hp, tau)
    return eng, sd, moments, lambda s, nf: _generic_head_frame(backbone, s, h, w, nf), list(GENERIC_HEAD_PARAMS), list(GENERIC_HEAD_TARGETS)


def _worker(rank, world, port, backbone, out):
    for p in (ROOT, os.path.join(ROOT, 'tta-depth-completion_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    from proxytta import distributed as D
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    z = np.load(os.path.join(GOLD, TWO_RANK[backbone] + '.npz'))
    h, w, n, steps = (int(v) for v in z['meta'][:4])
    hp, tau = _hp(z)
    eng, sd, moments, frame, params, targets = _head_case(backbone, 1, h, w, hp, tau)
    eng.set_head_form(SYNCBN)
    res = {}
    for s in range(steps):
        image, sparse = (torch.from_numpy(a[rank:rank + 1]).cuda() for a in frame(s, n))
        loss = D.shared_head_step(eng, image, sparse, True)
        torch.cuda.synchronize()
        res['s%d/loss' % s] = float(loss)
        for k in params:
            res['s%d/param/%s' % (s, k)] = sd[k].cpu().numpy().copy()
            res['s%d/exp_avg/%s' % (s, k)] = moments[k][0].cpu().numpy().copy()
            res['s%d/exp_avg_sq/%s' % (s, k)] = moments[k][1].cpu().numpy().copy()
        for k in targets + ['proj.1.running_mean', 'proj.1.running_var', 'pred.1.running_mean', 'pred.1.running_var',
                            'proj_t.1.running_mean']:
            res['s%d/buf/%s' % (s, k)] = sd[k].cpu().numpy().copy()
    res['params'] = params
    out[rank] = res
    eng.close()
    dist.destroy_process_group()


@pytest.mark.parametrize('backbone', ['nlspn', 'costdcnet', 'msg_chn'])
def test_two_ranks_reproduce_the_batch2_reference_run(backbone):
    """Two ranks with one frame each (proxytta.distributed.shared_head_step over gloo) against the reference's batch-2 run: the mean of the
    ranks' losses, proj.1 / pred.1 running statistics of the GLOBAL batch, both Adam moments of the MEAN gradient (a sum instead of a mean
    doubles the first and quadruples the second), and bitwise the same heads, moments, proj_t and buffers on both ranks after every step.
    On MSG_CHN this is the backward's exchange of the BatchNorm sums (partial sums -> exchange -> finalize, d gamma / d beta / world)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    out = ctx.Manager().dict()
    mp.spawn(_worker, args=(2, _free_port(), backbone, out), nprocs=2, join=True)
    r0, r1 = out[0], out[1]
    params = list(r0['params'])
    z = np.load(os.path.join(GOLD, TWO_RANK[backbone] + '.npz'))
    steps = int(z['meta'][3])
    lr = float(z['hp'][0])
    for s in range(steps):
        p = 's%d/' % s
        # the loss is a mean over rows: the batch-2 loss is the mean of the two ranks' losses
        assert abs(0.5 * (r0[p + 'loss'] + r1[p + 'loss']) - float(z[p + 'loss'])) < (5e-5 if s == 0 else 3e-4), s
        for k in [k for k in r0 if k.startswith(p) and k != p + 'loss']:
            assert np.array_equal(r0[k], r1[k]), k                       # every rank holds the same heads, moments and proj_t
        for q in params:
            _rows_check(z, p + 'after/' + q, r0[p + 'param/' + q], 0, 2.5 * lr * (s + 1), q)
        for q in ('proj.1.running_mean', 'proj.1.running_var', 'pred.1.running_mean', 'pred.1.running_var'):
            _rows_check(z, p + 'after/' + q, r0[p + 'buf/' + q], RUN_RTOL, RUN_ATOL, q)      # statistics of the GLOBAL batch
        if backbone != 'msg_chn':                                      # (MSG_CHN: proj_t.1 runs in train mode, as in the reference)
            np.testing.assert_array_equal(r0[p + 'buf/proj_t.1.running_mean'], z['before/proj_t.1.running_mean'])
    last = 's%d/' % (steps - 1)
    for q in params:                                                   # the mean gradient drives Adam: both moments follow it
        for which, rel in (('exp_avg/', 5e-2), ('exp_avg_sq/', 1e-1)):
            key = last + which + q
            if key in z.files or key + '#rows' in z.files:
                _moment_check(z, key, torch.from_numpy(r0[key]), rel)
            else:                                                      # outside the graph (MSG_CHN reverse: proj): never stepped
                assert not bool(z[last + 'has_grad/' + q]) and not np.any(r0[key]), key


@pytest.mark.parametrize('backbone', ['nlspn', 'msg_chn'])
def test_one_rank_rccl_equals_the_world1_run(backbone):
    """ptta_set_stat_sync_rccl + ptta_set_grad_sync_rccl on a one-rank communicator: the exchanges (MSG_CHN: the forward's moments and the
    backward's sums) and the gradient mean run and change nothing beyond the fp64 round trip of the statistics -- losses, gradients of
    the last step and both Adam moments match the run without them."""
    hp = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    h, w = (48, 80) if backbone == 'nlspn' else (32, 48)
    res = []
    for rccl in (False, True):
        eng, sd, moments, frame, params, _ = _head_case(backbone, 1, h, w, hp, 0.999)
        eng.set_head_form(SYNCBN)
        if rccl:
            eng.enable_rccl_sync()
            # the exchange buffer holds the twelve gradients: one message even without the gradient communicator
            assert eng._keep['stat_sync'][0].numel() >= sum(sd[k].numel() for k in params)
        losses = []
        for s in range(2):
            image, sparse = (torch.from_numpy(a).cuda() for a in frame(s, 1))
            eng.head_forward(image, sparse, True, want=False)
            losses.append(eng.head_backward())
            grads = {k: eng.head_grad(k, sd[k]) for k in params}
            eng.head_adam_step()
        torch.cuda.synchronize()
        res.append((torch.cat(losses).cpu(), {k: g.cpu().clone() for k, g in grads.items() if g is not None},
                    {k: (m.cpu().clone(), v.cpu().clone()) for k, (m, v) in moments.items()}))
        if rccl:
            eng.disable_rccl_sync()
        eng.close()
    torch.testing.assert_close(res[1][0], res[0][0], rtol=1e-5, atol=1e-6)
    assert res[0][1].keys() == res[1][1].keys() and res[0][1]
    for k in res[0][1]:
        a, b = res[1][1][k], res[0][1][k]
        torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-3 * float(b.abs().max()) + 1e-9, msg=k)
    for k in res[0][2]:
        for a, b in zip(res[1][2][k], res[0][2][k]):
            torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-3 * float(b.abs().max()) + 1e-20, msg=k)
