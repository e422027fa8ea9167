"""CPU-only: the matrix-free restatement of the biharmonic rows that csrc/inpaint.hip is written against (tests/inpaint_cases.py) against
scipy and against the host code proxytta/inpaint.py, on the cases tests/test_gpu_inpaint_device.py runs, and the properties of those
cases the GPU tests lean on."""
import itertools
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi

from tests import inpaint_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_separable_row_is_the_laplacian_of_the_laplacian_on_every_box():
    """3 offsets x 3 lengths per axis: 81 boxes.  Exact: the entries are small integers."""
    seen = 0
    for oy, ry, ox, rx in itertools.product(range(3), repeat=4):
        delta = np.zeros((oy + 1 + ry, ox + 1 + rx))
        delta[oy, ox] = 1
        want = ndi.laplace(ndi.laplace(delta))
        got = C.box_row(oy, ry, ox, rx)
        assert np.array_equal(got, want), (oy, ry, ox, rx)
        # the row lives on 13 places: the cross of radius 2 and the 3 x 3 block
        on = {(dy, dx) for dy, dx in C.OFFSETS if 0 <= oy + dy < delta.shape[0] and 0 <= ox + dx < delta.shape[1]}
        assert {(y - oy, x - ox) for y, x in np.argwhere(want != 0)} <= on
        seen += 1
    assert seen == 81
    assert C.box_row(2, 2, 2, 2)[2, 2] == 20 and C.box_row(2, 2, 2, 2)[2, 1] == -8 and C.box_row(2, 2, 2, 2)[1, 1] == 2 and C.box_row(2, 2, 2, 2)[0, 2] == 1


@pytest.mark.parametrize('name', C.NAMES)
def test_cg_with_the_matrix_free_operator_matches_the_host_code(name):
    _, m, d = C.case(name)
    out, it, _ = C.cg_fill(d, m, rtol=1e-12)
    want = C.expected(name)
    assert np.array_equal(out[~m], want[~m]) and not (out == 0).any()
    worst = int(C.ulps(out[m], want[m]).max())
    print('%s: %d unknowns, %d iterations, %d ulps' % (name, int(m.sum()), it, worst))
    assert worst <= 1


def test_the_matrix_is_symmetric():
    for name in ('corners_borders', 'random90', 'one_known', 'random30_odd'):
        _, m, d = C.case(name)
        nbr, coef, _ = C.build_rows(d, m)
        A = np.zeros((len(nbr), len(nbr)))
        for j in range(13):
            k = np.where(nbr[:, j] >= 0)[0]
            A[k, nbr[k, j]] += coef[k, j]
        assert np.array_equal(A, A.T)


def test_conditions_the_gpu_tests_lean_on():
    # random90: at least one unknown is clipped to lo or hi
    _, m, d = C.case('random90')
    _, _, x = C.cg_fill(d, m)
    lo, hi = float(d[~m].min()), float(d[~m].max())
    assert ((x < lo) | (x > hi)).any()
    assert np.isin(C.expected('random90')[m], [np.float32(lo), np.float32(hi)]).any()
    # one_known: lo == hi, every unknown is clipped onto it
    _, m, d = C.case('one_known')
    assert int((~m).sum()) == 1
    _, _, x = C.cg_fill(d, m)
    assert (x != float(d[~m][0])).any() and (C.expected('one_known') == d[~m][0]).all()
    # checkerboard48: more unknowns than a workgroup has threads; blob32: a long solve
    assert int(C.case('checkerboard48')[1].sum()) == 1536 > 1024
    _, m, d = C.case('blob32')
    assert int(m.sum()) == 1024 and C.cg_fill(d, m)[1] > 500
    # big12x18 needs more than the 5 iterations the not-converged test allows; random30 has more than 8 unknowns
    _, m, d = C.case('big12x18')
    assert C.cg_fill(d, m)[1] > 5
    assert int(C.case('random30')[1].sum()) > 8


def test_header_and_binding_declare_the_two_entry_points():
    from proxytta import _lib
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    sig = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    P, I = _lib.c_void_p, _lib.c_int
    assert sig['ptta_inpaint_scratch_bytes'] == (_lib.c_int64, [I, I, I, I])
    assert sig['ptta_inpaint_biharmonic'] == (I, [P, I, I, I, I, I, _lib.ctypes.c_double, P, _lib.c_int64, P, P])
    assert re.search(r'^int64_t ptta_inpaint_scratch_bytes\(int n, int height, int width, int max_unknowns\);', header, re.M)
    decl = re.search(r'^int ptta_inpaint_biharmonic\(([^;]*)\);', header, re.M)
    assert decl and len(decl.group(1).split(',')) == 11
    assert int(re.search(r'#define PTTA_ABI_VERSION (\d+)', header).group(1)) == _lib.PTTA_ABI_VERSION == 2
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert hasattr(lib, 'ptta_inpaint_biharmonic')
        # the argument checks run on the host before any launch
        assert lib.ptta_inpaint_scratch_bytes(1, 16, 24, 64) > 0
        assert lib.ptta_inpaint_scratch_bytes(1, 4, 24, 64) == -22 and lib.ptta_inpaint_scratch_bytes(0, 16, 24, 64) == -22
        assert lib.ptta_inpaint_scratch_bytes(2, 16, 24, 64) == 2 * lib.ptta_inpaint_scratch_bytes(1, 16, 24, 64)
        assert lib.ptta_inpaint_biharmonic(None, 1, 16, 24, 64, 10, 1e-12, None, 0, None, None) == -22


def test_fill_holes_switch_values():
    import torch
    from proxytta.nlspn import NlspnModel_Adapt
    m = NlspnModel_Adapt(device=torch.device('cpu'))
    assert m.fill_holes is True                                   # the default stays the host path
    m.fill_holes = 'gpu'
    with pytest.raises(ValueError):
        m._fill(torch.ones(1, 1, 8, 8), 'adapt_meta_selfsup_seq_ema_reverse')
    m.fill_holes = False
    t = torch.zeros(1, 1, 8, 8)
    assert m._fill(t, 'adapt_meta_selfsup_seq_ema_reverse') is t
