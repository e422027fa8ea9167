"""CPU-only side of the per-element convolution tests (tests/test_gpu_gconv_elementwise.py): the hook's declaration, the tolerances and
the argument that a per-element bound sees what a mean does not.

Tolerances (tests/gconv_cases.py TOL) are 4 x the CPU emulations' largest error ratio over the cases, profiles/gconv_elementwise.txt:
fp32 3.82e-7, bf16x6 1.39e-7, bf16x3 1.07e-5, hi + lo weights 1.68e-6 (on bf16-exact activations: with full activations their own 2^-9
rounding equals the one-MFMA error and the weight's lo term could not be told from it), one MFMA 2.55e-3 and, against the float64
convolution of the ROUNDED operands, 1.14e-7."""
import os
import re

import pytest
import torch

from oracle import gconv_arith as A
from proxytta import _lib
from tests import gconv_cases as G
from tests.util import assert_elementwise, rel_mae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (case, arithmetic) pairs left out of the discrimination check, with the reason; their BOUND stays
NOT_DISCRIMINATED = {
    # K = 9 x 128: bf16x3's own error per element falls as 1 / sqrt(K) and is 8.5e-7 here, less than twice bf16x6's tolerance
    ('s2_ksplit_six_4x64', 'x6'),
    # the sigmoid's slope is at most 1 / 4, the bound is the pre-activation value's: every arithmetic's error shrinks by 4 or more and
    # the hi + lo weight form's 7.1e-5 is under twice bf16x3's tolerance
    ('s1_17x33_nlspn_cf_dec0', 'x3'),
}


def test_op_gconv_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    m = re.search(r'int ptta_op_gconv\(([^)]*)\);', header)
    assert m, 'ptta_op_gconv not declared'
    nargs = len([a for a in m.group(1).split(',') if a.strip()])
    sig = {name: args for name, _, args in _lib.SIGNATURES}
    assert 'ptta_op_gconv' in sig and len(sig['ptta_op_gconv']) == nargs == 28
    assert re.search(r'#define PTTA_ABI_VERSION 2\b', header) and _lib.PTTA_ABI_VERSION == 2
    from proxytta.engine import GCONV_ACTS, GCONV_FORMS, GCONV_GEOMS, GCONV_IMPLS
    for name, val in (('PTTA_GCONV_S1', GCONV_GEOMS['s1']), ('PTTA_GCONV_S2', GCONV_GEOMS['s2']), ('PTTA_GCONV_T2', GCONV_GEOMS['t2'])):
        assert re.search(r'#define %s %d\b' % (name, val), header)
    assert GCONV_ACTS == {'none': 0, 'relu': 1, 'lrelu': 2, 'sigmoid': 3} and GCONV_IMPLS == {'mfma': 0, 'direct': 1}
    assert GCONV_FORMS == {-1: None, 0: 'plain', 1: 'nco2', 2: 'ksplit'}


def test_dgrad_linear_ops_are_autograd():
    """The data-gradient references of oracle/gconv_arith.py are torch.autograd.grad of the float64 forward convolution."""
    for name in ('dgrad_s1_9x33', 'dgrad_s2_odd_5x17', 'dgrad_t2_8x34', 'dgrad_s1k1_8x33'):
        c = G.BY_NAME[name]
        d = G.make(c)
        ho, wo = G.out_size(c)
        xin = torch.randn(c['b'], c['co'], ho, wo, dtype=torch.float64, requires_grad=True)
        y = A.linear_op(c['k'], c['geom'])(xin, d['w'].double())
        gy = G.nchw(d['x']).double()
        assert y.shape == gy.shape, name
        (gx,) = torch.autograd.grad(y, xin, gy)
        ref, _ = G.reference(c, d)
        assert float((G.nhwc(gx) - ref).abs().max()) < 1e-12, name


@pytest.fixture(scope='module')
def rows():
    torch.manual_seed(0)
    return G.measure([c for c in G.CASES if not c['big']])


def test_tolerances_are_four_times_the_emulations_error(rows):
    """The constants against the ratios recomputed here (the full-size cases are left to `python -m tests.gconv_cases`: only the fp32
    form has its largest ratio there)."""
    worst = G.worst(rows)
    assert set(worst) == set(G.TOL)
    for ar, r in worst.items():
        assert 4.0 * r <= G.TOL[ar] * 1.001, (ar, r, G.TOL[ar])
        if ar != 'fp32':
            assert G.TOL[ar] <= 4.0 * r * 1.001, (ar, r, G.TOL[ar])
    assert G.TOL['fp32'] < 4 * 2.0 ** -20


def test_each_tolerance_is_under_half_the_next_coarser_error(rows):
    """bf16x6 < bf16x3 < hi + lo weights < one MFMA, case by case on the same images: otherwise a six_B image computed as bf16x3, or a
    dropped lo term, would pass."""
    checked = {}
    for name, ar, _, coarser in rows:
        if coarser is None or (name, ar) in NOT_DISCRIMINATED:
            continue
        if ar == 'x3' and G.BY_NAME[name]['xexact']:
            continue                   # bf16-exact activations: their lo plane is zero and bf16x3 IS hi + lo weights
        assert G.TOL[ar] < 0.5 * coarser, (name, ar, G.TOL[ar], coarser)
        checked[ar] = checked.get(ar, 0) + 1
    assert checked['x6'] >= 10 and checked['x3'] >= 50 and checked['w2'] >= 5 and checked['x1r'] >= 8, checked
    for name, ar in NOT_DISCRIMINATED:
        assert any(r[0] == name and r[1] == ar for r in rows)


def _planted(c, d, ref, mag):
    """Three wrong references of a stride-1 3x3 case, each confined to ONE tile of image 0 -- the last tile column of the second tile
    row -- as a wrong tile decode or a wrong edge predicate would be: (what, reference).  (On these uncorrelated inputs a fault along
    a whole column or row of the map is a 100 % error on 1 / 608 or 1 / 176 of the elements and moves the mean by 2e-3: the mean sees
    that; it is the single tile it cannot see.)"""
    lin = G.lin_of(c)
    last = ref.shape[2] - 1
    x0 = last // 32 * 32
    f1 = ref.clone(); f1[0, 8:16, last, :] = ref[0, 8:16, last - 1, :]
    wd = d['w'].clone(); wd[:, :, 0, :] = 0.0                                       # the taps that read the row above
    rd, _ = A.reference(lin, G.nchw(d['x']), wd, d['bias'], G.nchw(d['y_prev']), c['act'])
    f2 = ref.clone(); f2[0, 8, x0:, :] = G.nhwc(rd)[0, 8, x0:, :]
    f3 = ref.clone(); f3[0, 8:16, x0:, ref.shape[3] - 8:] = 0.0
    return (('last column shifted by a pixel', f1), ('top halo row of the second 8-row tile dropped', f2), ('last 8 channels zeroed', f3))


@pytest.mark.parametrize('name', ['s1_stats2_17x65', 's1_full_176x608'])
def test_planted_faults_are_rejected_where_a_mean_accepts_them(name):
    c = G.BY_NAME[name]
    d = G.make(c)
    ref, mag = G.reference(c, d)
    got = G.emulation(c, d, 'x3')
    bound = G.TOL['x3'] * mag
    assert_elementwise(got, ref, bound, name)
    for k, (what, wrong) in enumerate(_planted(c, d, ref, mag)):
        with pytest.raises(AssertionError) as e:
            assert_elementwise(got, wrong, bound, what)
        msg = str(e.value)
        if k == 0:
            assert 'columns %d' % (ref.shape[2] - 1) in msg and 'x mod 32 = %d' % ((ref.shape[2] - 1) % 32) in msg, msg
        if k == 1:
            assert 'rows 8' in msg and 'y mod 8 = 0' in msg, msg
        if k == 2:
            assert 'channels %d..%d' % (ref.shape[3] - 8, ref.shape[3] - 1) in msg, msg
        if c['big'] and k < 2:
            assert rel_mae(got, wrong) < 1e-4, what       # the end-to-end tests' bound lets it through


def test_an_image_on_the_wrong_side_of_the_split_is_rejected():
    c = G.BY_NAME['s1_x1_half_9x33']
    d = G.make(c)
    ref, mag = G.reference(c, d)
    rref, rmag = G.reference_rounded(c, d)
    fine, coarse = G.emulation(c, d, 'x3'), G.emulation(c, d, 'x1')
    assert_elementwise(fine[:1], ref[:1], G.TOL['x3'] * mag[:1], 'image 0, bf16x3')
    assert_elementwise(coarse[1:], ref[1:], G.TOL['x1'] * mag[1:], 'image 1, one MFMA')
    assert_elementwise(coarse[1:], rref[1:], G.TOL['x1r'] * rmag[1:], 'image 1, one MFMA, rounded operands')
    with pytest.raises(AssertionError):          # x1_from_B one too small: image 0 with one MFMA
        assert_elementwise(coarse[:1], ref[:1], G.TOL['x3'] * mag[:1], 'image 0')
    with pytest.raises(AssertionError):          # one too large: image 1 with the finer arithmetic
        assert_elementwise(fine[1:], rref[1:], G.TOL['x1r'] * rmag[1:], 'image 1')
    # ... and the reference of image x1_from_B built with the finer arithmetic
    with pytest.raises(AssertionError):
        assert_elementwise(coarse[1:], ref[1:], G.TOL['x1r'] * mag[1:], 'image 1')


def test_assert_elementwise_counts_every_element():
    ref = torch.zeros(1, 2, 3, 4, dtype=torch.float64)
    got = torch.zeros(1, 2, 3, 4)
    got[0, 1, 2, 3] = float('nan')
    with pytest.raises(AssertionError, match='1 of 24 elements'):
        assert_elementwise(got, ref, torch.ones_like(ref), 'nan')
