"""NLSPN's propagation gradients per element, both forms of each (include/ptta.h ptta_op_nl_prop_bwd / ptta_op_nl_affinity_bwd): form 0 the
float-atomic kernels of the default step, form 1 the fixed-point forms of option "deterministic".  Inputs, the fp64 autograd reference and the
bounds are in tests/nlspn_det_cases.py: form 1 is held to twice the error measured for form 0 on the same inputs, its gathers to bitwise
equality with form 0, and its outputs to bitwise equality between calls, streams and the two copies of one sample."""
import functools

import pytest
import torch

from proxytta.engine import op_nl_affinity_bwd, op_nl_prop_bwd
from tests import nlspn_det_cases as C

pytestmark = pytest.mark.gpu
CASE_IDS = sorted(C.CASES)


def run_prop(case, form, twin=False):
    x = {k: v.cuda() for k, v in C.prop_inputs(case, twin).items()}
    goff9, gaff9 = torch.zeros_like(x['off9']), torch.zeros_like(x['aff9'])
    gfeat, _ = op_nl_prop_bwd(x['pinned'], x['fix'], x['off9'], x['aff9'], x['gout'], goff9, gaff9, form=form)
    return dict(gfeat=gfeat, goff9=goff9, gaff9=gaff9)


def run_aff(case, legacy, form, twin=False):
    x = {k: v.cuda() for k, v in C.aff_inputs(case, legacy, twin).items()}
    scale = torch.full((1,), C.AFF_SCALE, device='cuda')
    g_oa, gconf = op_nl_affinity_bwd(x['oa'], x['conf'], scale, x['goff9'], x['gaff9'], legacy=legacy, form=form)
    return dict(g_oa=g_oa, gconf=gconf)


# one run per (case, form), shared by the tests below and never written
prop_once = functools.lru_cache(maxsize=None)(run_prop)
aff_once = functools.lru_cache(maxsize=None)(run_aff)


def check(got, ref, table, key, label):
    figs = [(name, C.rel_mae(got[name], ref[name])) for name in sorted(ref)]
    for name, v in figs:
        print('FIG %s %-6s %.3e   (form-0 figure %.3e)' % (label, name, v, table[key][name]))
    for name, v in figs:
        assert v <= C.bound(table, key, name), (label, name, v)


@pytest.mark.parametrize('form', [0, 1])
@pytest.mark.parametrize('case', CASE_IDS)
def test_prop_bwd_against_fp64(case, form):
    got = prop_once(case, form)
    check(got, C.prop_reference(case), C.FORM0_PROP, case, 'prop %s form %d' % (case, form))
    pinned = C.prop_inputs(case)['fix'].cuda() > 0
    assert float(got['gfeat'][pinned].abs().sum()) == 0.0                     # case g: exactly nothing reaches a pinned pixel
    if case == 'h':
        assert all(float(v.abs().sum()) == 0.0 for v in got.values())


@pytest.mark.parametrize('case', CASE_IDS)
def test_prop_bwd_gathers_keep_their_arithmetic(case):
    a, b = prop_once(case, 0), prop_once(case, 1)
    assert torch.equal(a['goff9'], b['goff9']) and torch.equal(a['gaff9'], b['gaff9'])


@pytest.mark.parametrize('case', CASE_IDS)
def test_prop_bwd_form1_is_reproducible(case):
    a, b = prop_once(case, 1), run_prop(case, 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = run_prop(case, 1)
    side.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    t = run_prop(case, 1, twin=True)
    for k in t:
        assert torch.equal(t[k][0], t[k][1]) and torch.equal(t[k][0], a[k][0]), k


@pytest.mark.parametrize('form', [0, 1])
@pytest.mark.parametrize('legacy', [False, True])
@pytest.mark.parametrize('case', CASE_IDS)
def test_affinity_bwd_against_fp64(case, legacy, form):
    got = aff_once(case, legacy, form)
    check(got, C.aff_reference(case, legacy), C.FORM0_AFF, (case, legacy), 'aff %s legacy %d form %d' % (case, legacy, form))
    if case == 'h':
        assert all(float(v.abs().sum()) == 0.0 for v in got.values())


@pytest.mark.parametrize('legacy', [False, True])
@pytest.mark.parametrize('case', CASE_IDS)
def test_affinity_bwd_g_oa_keeps_its_arithmetic(case, legacy):
    assert torch.equal(aff_once(case, legacy, 0)['g_oa'], aff_once(case, legacy, 1)['g_oa'])


@pytest.mark.parametrize('legacy', [False, True])
@pytest.mark.parametrize('case', CASE_IDS)
def test_affinity_bwd_form1_is_reproducible(case, legacy):
    a, b = aff_once(case, legacy, 1), run_aff(case, legacy, 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = run_aff(case, legacy, 1)
    side.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    t = run_aff(case, legacy, 1, twin=True)
    for k in t:
        assert torch.equal(t[k][0], t[k][1]) and torch.equal(t[k][0], a[k][0]), k


def test_non_finite_and_zero_maxima():
    """A non-finite value anywhere in gout makes the whole deterministic gfeat NaN (documented in include/ptta.h); gout = 0 is case h."""
    x = {k: v.cuda().clone() for k, v in C.prop_inputs('c').items()}
    x['gout'][1, 3, 5] = float('inf')
    gfeat, _ = op_nl_prop_bwd(x['pinned'], x['fix'], x['off9'], x['aff9'], x['gout'], torch.zeros_like(x['off9']), torch.zeros_like(x['aff9']), form=1)
    assert bool(torch.isnan(gfeat).all())
    # tiny and huge finite gradients keep their relative accuracy: the scale follows the maximum
    for mag in (2.0 ** -60, 2.0 ** 60):
        x = {k: v.cuda().clone() for k, v in C.prop_inputs('c').items()}
        x['gout'] *= mag
        gfeat, _ = op_nl_prop_bwd(x['pinned'], x['fix'], x['off9'], x['aff9'], x['gout'], torch.zeros_like(x['off9']), torch.zeros_like(x['aff9']), form=1)
        assert torch.equal(gfeat / mag, prop_once('c', 1)['gfeat'])           # powers of two: the same bits, rescaled
