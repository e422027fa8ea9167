"""The inputs and fp64 references of tests/nlspn_det_cases.py, checked without a GPU: what the per-element tests of NLSPN's propagation
gradients compare the kernels against is finite, keeps the pinned pixels free of gradient, and is zero where the upstream gradient is."""
import pytest
import torch

from tests import nlspn_det_cases as C


@pytest.mark.parametrize('case', sorted(C.CASES))
def test_prop_reference_is_sound(case):
    x, r = C.prop_inputs(case), C.prop_reference(case)
    assert tuple(r['gfeat'].shape) == (C.N, C.H, C.W) and tuple(r['goff9'].shape) == (C.N, 18, C.H, C.W) and tuple(r['gaff9'].shape) == (C.N, 9, C.H, C.W)
    for k, v in r.items():
        assert bool(torch.isfinite(v).all()), k
    pinned = x['fix'] > 0
    assert float(r['gfeat'][pinned].abs().sum()) == 0.0                      # no gradient reaches a pinned pixel
    if case == 'g':
        assert 0.2 < float(pinned.float().mean()) < 0.3
        assert torch.equal(x['pinned'][pinned], x['fix'][pinned])
    else:
        assert not bool(pinned.any())
    if case == 'h':
        assert all(float(v.abs().sum()) == 0.0 for v in r.values())
    else:
        assert all(float(v.abs().sum()) > 0.0 for v in r.values())
    # the affinities are what the normalisation leaves: eight of magnitude below 1 in sum, the centre 1 - sum
    a = x['aff9'].double()
    assert float((a.abs().sum(1) - a[:, 4].abs()).max()) < 1.0 and float((a.sum(1) - 1.0).abs().max()) < 1e-6


@pytest.mark.parametrize('legacy', [False, True])
@pytest.mark.parametrize('case', sorted(C.CASES))
def test_affinity_reference_is_sound(case, legacy):
    r = C.aff_reference(case, legacy)
    assert tuple(r['g_oa'].shape) == (C.N, C.H, C.W, 24) and tuple(r['gconf'].shape) == (C.N, C.H, C.W)
    for k, v in r.items():
        assert bool(torch.isfinite(v).all()), k
    if case == 'h':
        assert all(float(v.abs().sum()) == 0.0 for v in r.values())
    else:
        assert all(float(v.abs().sum()) > 0.0 for v in r.values())


def test_cases_exercise_what_they_claim():
    off = {c: C.prop_inputs(c)['off9'].view(C.N, 9, 2, C.H, C.W) for c in C.CASES}
    assert float(off['a'].abs().max()) == 0.0
    assert 0.0 < float(off['b'].abs().max()) < 0.5
    assert 2.5 < float(off['c'].abs().max()) <= 3.0
    assert float(off['d'][:, [0, 1, 2, 3, 5, 6, 7, 8]].abs().min()) >= 9.0            # past the 4-pixel apron from every pixel of a tile
    yy = torch.arange(C.H).view(1, 1, C.H, 1) + torch.tensor([k // 3 - 1 for k in range(9)]).view(1, 9, 1, 1)
    xx = torch.arange(C.W).view(1, 1, 1, C.W) + torch.tensor([k % 3 - 1 for k in range(9)]).view(1, 9, 1, 1)
    h, w = yy + off['e'][:, :, 0], xx + off['e'][:, :, 1]
    assert bool((h <= -1).any()) and bool((h >= C.H).any()) and bool((w <= -1).any()) and bool((w >= C.W).any())
    hf, wf = yy + off['f'][:, :, 0], xx + off['f'][:, :, 1]
    taps = [0, 1, 2, 3, 5, 6, 7, 8]
    assert float((hf[:, taps] - C.TARGET[0]).abs().max()) < 1e-4 and float((wf[:, taps] - C.TARGET[1]).abs().max()) < 1e-4
    g = C.prop_inputs('f')['gout'].abs()
    assert float(g.max() / g.min()) > 2.0 ** 19 and bool((C.prop_inputs('f')['gout'] < 0).any())
    # the twin batches are one sample twice
    for k, v in C.prop_inputs('c', True).items():
        assert torch.equal(v[0], v[1]) and torch.equal(v[0], C.prop_inputs('c')[k][0])
