"""Option "head_bn_fused" of the generic engine (include/ptta.h ptta_set_option; csrc/gnet.hip GNet::plan_affine): in the stage-2 head trainer's
two no-gradient backbone passes every frozen BatchNorm2d rides in the epilogue of the convolution in front of it.  The epilogue computes
gbn_apply_kernel's expressions word for word (tests/test_gpu_gconv_affine_forms.py), so a head step with the option at 1 must equal the same
step at 0 BIT FOR BIT -- every comparison between the two here is torch.equal -- and the reference's fixtures are reproduced within the
bounds of the existing tests, whose functions are called as they stand (their handles take the option's default, 1)."""
import os

import numpy as np
import pytest
import torch

from proxytta.engine import Engine
from tests import test_gpu_head_trainer as T
from tests import test_gpu_meta2_generic as M2
from tests.test_gpu_head_syncbn import SYNCBN
from tests.test_gpu_head_trainer import GENERIC_HEAD_PARAMS, GENERIC_HEAD_TARGETS, _generic_head_frame, make_generic_head_engine

pytestmark = pytest.mark.gpu
HP = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
# the BatchNorm2d of each handle kind's stage-2 prefix: ResNet34's 35 and conv6 / Encoder2D's 15, and the 2layers block's two.  Every one is
# fused: no epilogue instantiation spills (profiles/head_bn_fused.txt), so no form is held back
COUNTS = {('nlspn', '1layer'): 36, ('nlspn', '2layers'): 38, ('costdcnet', '1layer'): 15, ('costdcnet', '2layers'): 17}


def make_engine(backbone, meta, n, h, w, hp, tau):
    """a bound stage-2 handle: (engine, bound tensors by name, Adam moments by name); 2layers as tests/test_gpu_meta2_generic.py builds it"""
    if meta == '1layer':
        eng, sd, _, (_, moments) = make_generic_head_engine(backbone, n, h, w, hp, tau)
        return eng, sd, moments
    from tests.golden.make_golden_head_generic import perturbed_target
    from proxytta import synth
    if backbone == 'nlspn':
        from tests.test_gpu_nlspn import HP as BHP
        eng = Engine(n, h, w, backbone='nlspn', legacy_offset=True, meta='2layers', **BHP)
        sd_np = synth.formula_state_dict_nlspn(M2.TWO)
    else:
        from tests.test_gpu_costdcnet import HP as BHP, MAX_DEPTH
        eng = Engine(n, h, w, backbone='costdcnet', max_predict_depth=MAX_DEPTH, meta='2layers', **BHP)
        sd_np = M2.state_dict('costdcnet')
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
    eng.set_head_hparams(tau=tau, adam_step=0, lr=hp['lr'], betas=hp['betas'], eps=hp['eps'], weight_decay=hp['weight_decay'])
    return eng, sd, moments


def snapshot(eng, sd, moments, emb, ref, loss):
    """everything one head step leaves behind, on the CPU"""
    out = {'emb': emb.cpu().clone(), 'ref': ref.cpu().clone(), 'loss': loss.cpu().clone()}
    for k in GENERIC_HEAD_PARAMS:
        out['grad/' + k] = eng.head_grad(k, sd[k]).cpu().clone()
    return out


def after(sd, moments):
    out = {}
    for k in GENERIC_HEAD_PARAMS:
        out['param/' + k] = sd[k].cpu().clone()
        out['exp_avg/' + k], out['exp_avg_sq/' + k] = moments[k][0].cpu().clone(), moments[k][1].cpu().clone()
    for k in GENERIC_HEAD_TARGETS:
        out['target/' + k] = sd[k].cpu().clone()
    for k, v in sd.items():                  # the heads' BatchNorm1d buffers and CostDCNet's BatchNorm3d running statistics, which stage 2 moves
        if 'running_' in k and v.dtype == torch.float32:
            out['buf/' + k] = v.cpu().clone()
    return out


def head_steps(backbone, meta, n, h, w, reverse, fused, steps=2, form=None, hp=HP, tau=0.999):
    eng, sd, moments = make_engine(backbone, meta, n, h, w, hp, tau)
    if form is not None:
        eng.set_head_form(form)
    eng.set_option('head_bn_fused', int(fused))
    assert eng.get_option('head_bn_fused_count') == (COUNTS[(backbone, meta)] if fused else 0)
    res = []
    for s in range(steps):
        image, sparse = (torch.from_numpy(a).cuda() for a in _generic_head_frame(backbone, s, h, w, n))
        emb, ref = eng.head_forward(image, sparse, reverse)
        loss = eng.head_backward()
        r = snapshot(eng, sd, moments, emb, ref, loss)
        eng.head_adam_step()
        torch.cuda.synchronize()
        r.update(after(sd, moments))
        res.append(r)
    eng.close()
    return res


def assert_equal_runs(a, b):
    assert len(a) == len(b)
    for s, (ra, rb) in enumerate(zip(a, b)):
        assert set(ra) == set(rb)
        for k in ra:
            assert torch.equal(ra[k], rb[k]), 'step %d, %s: %.3e' % (s, k, float((ra[k] - rb[k]).abs().max()))
        assert bool(torch.isfinite(ra['emb']).all()) and float(ra['emb'].abs().max()) > 0


FIXTURES = ['head_nlspn_forward_48x80_n2', 'head_nlspn_reverse_48x80_n2', 'head_nlspn2l_forward_48x80_n2',
            'head_costdcnet_reverse_64x96_n2', 'head_costdcnet2l_forward_64x96_n2',
            'head_syncbn_nlspn_reverse_48x80_n2', 'head_syncbn_costdcnet_reverse_64x96_n2']


def _fixture_case(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + '.npz'))
    h, w, n = (int(v) for v in z['meta'][:3])
    lr, b1, b2, eps, wd, tau = (float(v) for v in z['hp'])
    kind = name.split('_')[2 if 'syncbn' in name else 1]
    backbone, meta = (kind[:-2], '2layers') if kind.endswith('2l') else (kind, '1layer')
    return dict(backbone=backbone, meta=meta, n=n, h=h, w=w, reverse='reverse' in str(z['loss_type']),
                form=SYNCBN if 'syncbn' in name else None, hp=dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd), tau=tau)


@pytest.mark.parametrize('name', FIXTURES)
def test_two_head_steps_fused_equal_unfused_bit_for_bit(golden_dir, name):
    """The committed fixtures' sizes, batches, directions and hyper-parameters (the SyncBatchNorm form's on one rank): two handles from one
    state, the option at 1 and at 0, two head steps each.  Embedding, reference, loss, the twelve gradients, then the updated parameters,
    both Adam moments, the EMA target and every running statistic stage 2 moves (CostDCNet's BatchNorm3d among them)."""
    c = _fixture_case(golden_dir, name)
    fused, unfused = (head_steps(fused=f, **c) for f in (True, False))
    assert_equal_runs(fused, unfused)
    if c['backbone'] == 'costdcnet' and c['form'] is None:          # (the SyncBatchNorm form evaluates BatchNorm3d: nothing moves there)
        moved = [k for k in fused[0] if k.startswith('buf/unet3d')]
        assert moved and any(not torch.equal(fused[0][k], fused[1][k]) for k in moved)


@pytest.mark.parametrize('name', FIXTURES)
def test_default_option_still_reproduces_the_reference(golden_dir, name):
    """The existing reference tests, called as they are: their handles are created with the option's default (1, asserted by
    test_fused_counts_per_handle_kind), their bounds are theirs.  The SyncBatchNorm form's fixtures are the reference's two-rank run, so
    their checker is the two-process test of tests/test_gpu_head_syncbn.py."""
    if 'syncbn' in name:
        from tests.test_gpu_head_syncbn import TWO_RANK, test_two_ranks_reproduce_the_batch2_reference_run
        backbone = name.split('_')[2]
        assert TWO_RANK[backbone] == name
        test_two_ranks_reproduce_the_batch2_reference_run(backbone)
    elif '2l_' in name:
        M2.test_stage2_head_trainer_on_a_2layers_handle(golden_dir, name)
    else:
        T.test_generic_head_trainer_reproduces_reference(golden_dir, name, 'default')


@pytest.mark.parametrize('backbone,meta', list(COUNTS))
def test_fused_counts_per_handle_kind(backbone, meta):
    kw = dict(max_predict_depth=8.0) if backbone == 'costdcnet' else {}
    eng = Engine(1, 32, 64, backbone=backbone, meta=meta, **kw)
    assert eng.get_option('head_bn_fused') == 1                                   # the default
    assert eng.get_option('head_bn_fused_count') == COUNTS[(backbone, meta)]
    eng.set_option('head_bn_fused', 0)
    assert eng.get_option('head_bn_fused') == 0 and eng.get_option('head_bn_fused_count') == 0
    eng.set_option('head_bn_fused', 1)
    assert eng.get_option('head_bn_fused_count') == COUNTS[(backbone, meta)]
    eng.close()


def test_mixed_handles_keep_the_unfused_path():
    eng = Engine(1, 32, 64, backbone='nlspn', dtype='mixed')
    assert eng.get_option('head_bn_fused') == 1 and eng.get_option('head_bn_fused_count') == 0
    eng.close()


def test_direct_fp32_handles_have_no_convolution_to_ride_in():
    """PTTA_CONV_IMPL=naive: no matrix-core convolution, so nothing is fused whatever the option says"""
    os.environ['PTTA_CONV_IMPL'] = 'naive'
    try:
        eng = Engine(1, 32, 64, backbone='nlspn')
    finally:
        os.environ.pop('PTTA_CONV_IMPL', None)
    assert eng.get_option('head_bn_fused') == 1 and eng.get_option('head_bn_fused_count') == 0
    eng.close()


def test_odd_sizes_fused_equal_unfused():
    """NLSPN at 36 x 52, one frame, synthetic weights: the encoder maps are 18, 9, 5 and 3 rows high (every strided layer reads an odd or
    a non-tile-multiple map, the K-split forms have a handful of pixels)."""
    runs = [head_steps('nlspn', '1layer', 1, 36, 52, True, fused=f, steps=1) for f in (True, False)]
    assert_equal_runs(*runs)


def test_a_tta_step_between_two_head_steps_moves_the_tables():
    """ptta_step adapts gamma / beta of every BatchNorm2d under 'meta_bn': the head step behind it must build its affine tables from the moved
    tensors.  Two handles, the option at 1 and at 0, run head step, TTA step, head step.  NLSPN's TTA step is not reproducible bit for bit
    (the float atomics of its propagation gradient, tests/test_gpu_nlspn.py), so after it the fused handle's state -- the adapted tensors
    with their moments and every bound head tensor and buffer -- is copied INTO the unfused handle's own bound tensors: both then hold one
    state that a TTA step on the handle itself has moved, at unchanged pointers, and the second head steps must agree bit for bit."""
    from tests.test_gpu_nlspn import nlspn_frame
    n, h, w = 1, 48, 80
    image, sparse = (torch.from_numpy(a).cuda() for a in _generic_head_frame('nlspn', 0, h, w, n))
    raw, image1, sp = (torch.from_numpy(a).cuda() for a in nlspn_frame(7, h, w, n))
    handles, first, gamma0 = [], [], None
    for fused in (1, 0):
        eng, sd, _, (keep, moments) = make_generic_head_engine('nlspn', n, h, w, HP, 0.999)
        eng.set_option('head_bn_fused', fused)
        emb, ref = eng.head_forward(image, sparse, True)
        loss = eng.head_backward()
        r = snapshot(eng, sd, moments, emb, ref, loss)
        eng.head_adam_step()
        gamma0 = keep['conv2.0.bn1.weight'][0].clone()
        eng.step(image1, sp, loss_image=raw)
        torch.cuda.synchronize()
        assert not torch.equal(keep['conv2.0.bn1.weight'][0], gamma0)              # the TTA step did move a BatchNorm2d's gamma
        first.append(r)
        handles.append((eng, sd, keep, moments))
    assert_equal_runs([first[0]], [first[1]])
    (_, sd_a, keep_a, mom_a), (_, sd_b, keep_b, mom_b) = handles
    for k in keep_a:
        for t_a, t_b in zip(keep_a[k], keep_b[k]):
            t_b.copy_(t_a)
    for k in sd_a:
        sd_b[k].copy_(sd_a[k])
    for k in mom_a:
        for t_a, t_b in zip(mom_a[k], mom_b[k]):
            t_b.copy_(t_a)
    second = []
    for eng, sd, keep, moments in handles:
        emb, ref = eng.head_forward(image, sparse, True)
        loss = eng.head_backward()
        r = snapshot(eng, sd, moments, emb, ref, loss)
        eng.head_adam_step()
        torch.cuda.synchronize()
        r.update(after(sd, moments))
        second.append(r)
        eng.close()
    assert_equal_runs([second[0]], [second[1]])
    # the same frame and, but for one Adam step, the same heads: the reference branch (proj_t on the real pass) moved with the backbone
    assert not torch.equal(first[0]['ref'], second[0]['ref'])


def test_option_plumbing():
    eng = Engine(1, 32, 64, backbone='nlspn')
    for v in (0, 1):
        eng.set_option('head_bn_fused', v)
        assert eng.get_option('head_bn_fused') == v
    with pytest.raises(RuntimeError, match=r'\(-22\)'):
        eng.set_option('head_bn_fused', 2)
    with pytest.raises(RuntimeError, match=r'\(-22\)'):
        eng.set_option('head_bn_fused_count', 1)                                  # read-only
    assert eng.get_option('head_bn_fused') == 1
    eng.close()
    eng = Engine(1, 32, 48)                                                       # MSG_CHN: no BatchNorm2d
    for key in ('head_bn_fused', 'head_bn_fused_count'):
        with pytest.raises(RuntimeError, match=r'\(-38\)'):
            eng.get_option(key)
        with pytest.raises(RuntimeError, match=r'\(-38\)'):
            eng.set_option(key, 0)
    eng.close()


def test_toggling_between_head_steps_with_graph_replay_on():
    """One handle with "graph" 1 whose TTA step has been captured and replayed: head step fused, the option to 0 (which drops the captured
    graphs), head step unfused, and a TTA step that captures again.  Both head steps equal what two fresh handles give that ran the same
    calls at one setting each.  NLSPN's TTA step is not reproducible bit for bit (float atomics in its propagation gradient), so every
    bound tensor is put back to its loaded value behind the replayed steps; nothing downstream of a TTA step is compared."""
    from tests.test_gpu_nlspn import nlspn_frame
    n, h, w = 1, 48, 80
    raw, image1, sp = (torch.from_numpy(a).cuda() for a in nlspn_frame(5, h, w, n))

    def run(settings):
        eng, sd, _, (keep, moments) = make_generic_head_engine('nlspn', n, h, w, HP, 0.999)
        eng.set_option('graph', 1)
        start = ({k: [t.clone() for t in v] for k, v in keep.items()}, {k: v.clone() for k, v in sd.items()})
        for _ in range(3):                                                         # eager, capture, replay
            eng.step(image1, sp, loss_image=raw)
        torch.cuda.synchronize()
        for k, v in keep.items():
            for t, t0 in zip(v, start[0][k]):
                t.copy_(t0)
        for k, v in sd.items():
            v.copy_(start[1][k])
        eng.head_reload()                                                          # the handle's packed copies follow the bound head tensors
        out = []
        for s, fused in enumerate(settings):
            eng.set_option('head_bn_fused', fused)
            image, sparse = (torch.from_numpy(a).cuda() for a in _generic_head_frame('nlspn', s, h, w, n))
            emb, ref = eng.head_forward(image, sparse, True)
            loss = eng.head_backward()
            r = snapshot(eng, sd, moments, emb, ref, loss)
            eng.head_adam_step()
            torch.cuda.synchronize()
            r.update(after(sd, moments))
            out.append(r)
        for _ in range(2):
            info, depth = eng.step(image1, sp, loss_image=raw, want_depth=True)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(depth).all()) and bool(torch.isfinite(info).all())
        eng.close()
        return out

    toggled, ones, zeros = run((1, 0)), run((1, 1)), run((0, 0))
    assert_equal_runs(toggled, ones)
    assert_equal_runs(toggled, zeros)
