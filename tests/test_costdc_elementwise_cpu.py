"""CPU-only side of the per-element tests of CostDCNet's own kernels (tests/test_gpu_costdc_elementwise.py): the hooks' declarations against
the binding, the references (oracle/costdc_arith.py) against torch on the CPU and against oracle/minkowski_lite.py, the tolerances, and
planted wrong arithmetics that the cases must reject.

Tolerances (tests/costdc_cases.py TOL) are 4 x the CPU emulation's largest error ratio per quantity over the cases,
profiles/costdc_elementwise.txt -- never a GPU figure."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import costdc_arith as A
from oracle import costdcnet_oracle as CO
from oracle import minkowski_lite as ML
from proxytta import _lib
from tests import costdc_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
HOOKS = ('ptta_cd_sparse_create', 'ptta_cd_sparse_destroy', 'ptta_cd_sparse_build', 'ptta_cd_sparse_read', 'ptta_op_cd_sparse_conv', 'ptta_op_cd_sbn',
         'ptta_op_cd_densify', 'ptta_op_cd_dense')


def _ctype_of(decl):
    decl = decl.strip()
    if '*' in decl:
        return 'ptr'
    return {'int': ctypes.c_int, 'float': ctypes.c_float, 'long long': ctypes.c_longlong, 'ptta_stream': 'ptr'}[re.sub(r'\s+\w+$', '', decl)]


def test_hooks_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    sig = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    for name in HOOKS:
        m = re.search(r'^(int|void) %s\((.*?)\);' % name, header, re.S | re.M)
        assert m, name
        want = [_ctype_of(a) for a in m.group(2).replace('\n', ' ').split(',')]
        res, args = sig[name]
        assert (res is None) == (m.group(1) == 'void'), name
        assert len(args) == len(want), name
        for k, (a, w) in enumerate(zip(args, want)):
            is_ptr = a is ctypes.c_void_p or hasattr(a, 'contents') or issubclass(a, ctypes._Pointer)
            assert (w == 'ptr' and is_ptr) or a is w, (name, k, a, w)
    body = re.search(r'typedef struct ptta_cd_sbn_args \{(.*?)\} ptta_cd_sbn_args;', header, re.S).group(1)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names += [n.strip(' *') for n in re.sub(r'^(const\s+)?(long long|int|float)\s*\*?', '', decl).split(',')]
    assert names == [n for n, _ in _lib.CdSbnArgs._fields_], names           # the same fields in the same order
    ints = [n for n, t in _lib.CdSbnArgs._fields_ if t is ctypes.c_int]
    assert names[:len(ints)] == ints and all(t is ctypes.c_void_p for _, t in _lib.CdSbnArgs._fields_[len(ints):])
    for op, val in _lib.CD_OPS.items():
        assert re.search(r'#define PTTA_CD_%s %d\b' % (op.upper(), val), header), op
    assert sorted(_lib.CD_OPS.values()) == list(range(15))


@pytest.fixture(scope='module')
def rows():
    return G.measure()


def test_tolerances_are_four_times_the_emulations_error(rows):
    worst = G.worst(rows)
    assert set(worst) == set(G.TOL) == set(G.QUANTITIES)
    for q, r in worst.items():
        assert 4.0 * r <= G.TOL[q] * 1.001 and G.TOL[q] <= 4.0 * r * 1.001, (q, r, G.TOL[q])
    # every tolerance stays a few fp32 roundings of its magnitude, and the BatchNorm's tie margin is at least its forward bound
    assert max(G.TOL.values()) < 32 * 2.0 ** -24 and G.TOL['sbn_y'] <= G.TIE


def test_profile_holds_the_tolerances():
    text = open(os.path.join(ROOT, 'profiles', 'costdc_elementwise.txt')).read()
    for q, r in G.RATIO.items():
        assert re.search(r'^%s\s+%s\s' % (q, re.escape('%.3e' % r)), text, re.M), q


# ---- the references against torch and against minkowski_lite -------------------------------------------------------------------------
def test_plane_rule_is_torch_round():
    for c in G.LEVEL_CASES:
        sp = G.make_levels(c)
        t = torch.round(torch.from_numpy(sp) / np.float32(c['z'])).long().clamp(0, 15).numpy()
        assert np.array_equal(A.plane_of(sp, c['z']), t), c['name']
    c = next(c for c in G.LEVEL_CASES if c['kind'] == 'halves')
    z = A.plane_of(np.array(G.HALVES, F32), c['z'])
    assert list(z[:10]) == [0, 2, 2, 14, 15, 0, 0, 0, 15, 15]              # halves to even, negatives and zero dropped, the clamp


def test_levels_are_the_oracles():
    for c in G.LEVEL_CASES:
        sp = G.make_levels(c)
        coords, f, _ = A.levels_ref(sp, c['z'])
        if len(coords[0]) == 0:
            continue
        st = CO.depth2mdp(torch.from_numpy(sp[:, None]).double(), float(np.float32(c['z'])))
        key = lambda a: a[np.lexsort(a.T[::-1])]
        oc = st.C.numpy()
        order = np.lexsort(oc.T[::-1])
        mine = np.lexsort(coords[0].T[::-1])
        assert np.array_equal(oc[order], coords[0][mine]), c['name']
        # (the oracle forms idx * z_step in torch's default fp32 whatever the input's type: one fp32 rounding of a value below 16 z_step)
        assert np.allclose(st.F.numpy()[order, 0], f[mine], rtol=0, atol=16 * 2.0 ** -24), c['name']
        for l in (1, 2):                            # unique(floor(c / ts) * ts), as a strided MinkowskiConvolution's output map
            out = ML.sparse_conv(ML.SparseTensor(torch.zeros(len(oc), 1), torch.from_numpy(oc), (1, 1 << (l - 1), 1 << (l - 1))) if l == 1 else prev,
                                 torch.zeros(1, 1, 1), 1, (1, 2, 2))
            prev = out
            assert np.array_equal(key(out.C.numpy()), key(coords[l])), (c['name'], l)
        # the emulation of the kernels' numbering satisfies every invariant
        A.check_levels(A.levels_emu(sp, c['z'])[0], sp, c['z'])


@pytest.fixture(scope='module')
def conv_geo():
    return G.conv_geometry(False)


def _stride(lin, lout):
    return (1, 2, 2) if lout > lin else 1


@pytest.mark.parametrize('form', G.CONV_FORMS, ids=str)
def test_sparse_conv_reference_is_minkowski_lite(form, conv_geo):
    """Forward against minkowski_lite.sparse_conv and the transpose against autograd through it, in float64."""
    _, coords, shape = conv_geo
    k, ci, co, lin, lout = form
    cin, cout = coords[lin], coords[lout]
    x, wk, _ = G.make_conv(form, len(cin), len(cout))
    gy, _, _ = G.make_conv(form, len(cin), len(cout), True)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    out = ML.sparse_conv(ML.SparseTensor(xt, torch.from_numpy(cin), (1, 1 << lin, 1 << lin)), torch.from_numpy(wk).double(), k, _stride(lin, lout))
    oc = out.C.numpy()
    assert np.array_equal(oc[np.lexsort(oc.T[::-1])], cout) or np.array_equal(oc, cout)
    perm = np.lexsort(oc.T[::-1]) if not np.array_equal(oc, cout) else np.arange(len(oc))
    pairs = A.conv_pairs(cin, cout, shape, lin, lout, k)
    ref, mag = A.sparse_conv_ref(x, wk, pairs, len(cout))
    assert np.allclose(out.F.detach().numpy()[perm], ref, rtol=0, atol=1e-12 * max(1.0, mag.max()))
    (out.F[torch.from_numpy(perm)] * torch.from_numpy(gy).double()).sum().backward()
    gref, gmag = A.sparse_conv_bwd_ref(gy, wk, pairs, len(cin))
    assert np.allclose(xt.grad.numpy(), gref, rtol=0, atol=1e-12 * max(1.0, gmag.max()))
    # the pairs as the transposed kernel finds them from the input side are the same pairs
    tp = A.bwd_pairs_transposed(cin, cout, shape, lin, lout, k)
    as_set = lambda ps: {(kk, int(u), int(j)) for kk, uu, jj in ps for u, j in zip(uu, jj)}
    assert as_set(tp) == as_set(pairs)
    assert sum(len(u) for _, u, _ in pairs) > 0


def test_conv_set_holds_what_it_claims(conv_geo):
    _, coords, shape = conv_geo
    n27 = lambda l: np.bincount(np.concatenate([u for _, u, _ in A.conv_pairs(coords[l], coords[l], shape, l, l, 3)]), minlength=len(coords[l]))
    assert n27(1).max() == 27 and n27(2).max() == 27 and n27(0).max() >= 9            # a voxel with every neighbour
    assert n27(0).min() == 1 and n27(1).min() == 1 and n27(2).min() == 1              # an isolated voxel: only itself
    for l in range(3):
        z = coords[l][:, 1]
        assert z.min() == 1 and z.max() == 15
        assert coords[l][:, 2].min() == 0 and coords[l][:, 3].min() == 0
    assert coords[0][:, 2].max() == shape[1] - 1 and coords[0][:, 3].max() == shape[2] - 1
    assert len(G.conv_geometry(True)[1][0]) > 4096


def test_sbn_reference_is_torch_batchnorm():
    for c in G.SBN_CASES:
        if c['cnt'] < 2 or c['world'] != 1:
            continue
        d = G.make_sbn(c)
        fw, _ = G.sbn_reference_fwd(c, d)
        x = torch.from_numpy(d['f']).double().requires_grad_(True)
        gamma, beta = torch.from_numpy(d['gamma']).double().requires_grad_(True), torch.from_numpy(d['beta']).double().requires_grad_(True)
        rm = rv = None
        if d['track'] is not None:
            rm, rv = torch.from_numpy(d['track']['rm']).double(), torch.from_numpy(d['track']['rv']).double()
        train = c['mode'] != 'eval'
        for _ in range(2 if c['mode'] == 'tracked' else 1):
            v = F.batch_norm(x, rm, rv, gamma, beta, training=train, momentum=0.1, eps=float(np.float32(1e-5)))
        res = None if d['res'] is None else torch.from_numpy(d['res']).double().requires_grad_(True)
        y = v if res is None else v + res
        y = torch.relu(y) if c['relu'] else y
        assert np.allclose(y.detach().numpy(), fw['y'][0, 0], rtol=0, atol=1e-9), c['name']
        if c['mode'] == 'tracked':
            assert np.allclose(rm.numpy(), fw['rm'], rtol=0, atol=1e-12) and np.allclose(rv.numpy(), fw['rv'], rtol=0, atol=1e-12), c['name']
            assert fw['nbt'] == d['track']['nbt'] + 2
        if train:
            (y * torch.from_numpy(d['g']).double()).sum().backward()
            bw, _ = G.sbn_reference_bwd(c, d, fw, G.sbn_reference_fwd(c, d)[1])
            assert np.allclose(x.grad.numpy(), bw['gx'][0, 0], rtol=0, atol=1e-9), c['name']
            assert np.allclose(gamma.grad.numpy(), bw['dgamma'], rtol=0, atol=1e-9) and np.allclose(beta.grad.numpy(), bw['dbeta'], rtol=0, atol=1e-9)
            if res is not None:
                prev = 0.0 if d['gres_prev'] is None else d['gres_prev'].astype(F64)
                assert np.allclose(res.grad.numpy() + prev, bw['gres'][0, 0], rtol=0, atol=1e-12), c['name']


def _ncdhw(a):
    """[items = frames x planes][H][W][C] or [frames][D][H][W][C] -> torch (frames, C, D, H, W)"""
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(a, -1, 1)))


@pytest.mark.parametrize('c', [c for c in G.POOL_CASES if c['items'] <= 4], ids=lambda c: c['name'])
def test_pool_reference_is_aten(c):
    """Forward and the autograd backward on the tied inputs: 'first maximum' is ATen's."""
    x, gy, _ = G.make_pool(c)
    I, H, W, C = x.shape
    xt = _ncdhw(x.reshape(1, I, H, W, C)).double().requires_grad_(True)
    y = F.max_pool3d(xt, 2)
    assert np.array_equal(np.moveaxis(y.detach().numpy(), 1, -1)[0], A.pool_fwd_ref(x))
    y.backward(_ncdhw(gy.reshape((1,) + gy.shape)).double())
    assert np.array_equal(np.moveaxis(xt.grad.numpy(), 1, -1)[0], A.pool_bwd_ref(x, gy))
    w = A._windows(x)
    assert (w.max(3) == w.min(3)).any() and ((w == w.max(3, keepdims=True)).sum(3) > 1).any() and (w.max(3) == 0).any()     # ties, and windows of zeros


@pytest.mark.parametrize('c', G.UP_CASES, ids=lambda c: c['name'])
def test_up_reference_is_aten(c):
    x, gy, _ = G.make_up(c)
    xt = _ncdhw(x).requires_grad_(True)                                  # float32: ATen computes the source index in the tensor's precision
    y = F.interpolate(xt, size=c['o'], mode='nearest')
    assert np.array_equal(np.moveaxis(y.detach().numpy(), 1, -1), A.up_fwd_ref(x, *c['o']))
    y.backward(_ncdhw(gy))
    ref = A.up_bwd_ref(gy, *c['i'])
    assert np.abs(ref).max() < 2 ** 24 and np.array_equal(np.moveaxis(xt.grad.numpy(), 1, -1).astype(F64), ref)
    for n_in, n_out in zip(c['i'], c['o']):                              # floor never reaches `in` here: the rule's clamp is dead on these sizes
        t = np.floor(np.arange(n_out, dtype=F32) * (F32(n_in) / F32(n_out)))
        assert t.max() <= n_in - 1


@pytest.mark.parametrize('c', G.REGRESS_CASES, ids=lambda c: c['name'])
def test_regress_reference_is_the_oracles(c):
    cost, gpred = G.make_regress(c)
    ct = torch.from_numpy(np.ascontiguousarray(np.moveaxis(cost, -1, 1))).double().requires_grad_(True)      # (b, c, d, h, w)
    zs = float(np.float32(c['z']))
    pred = CO.upsampling(ct)[:, 0] * zs
    ref, emu, mag = A.regress_fwd_ref(cost, c['z'])
    assert np.allclose(pred.detach().numpy(), ref, rtol=0, atol=1e-12)
    pred.backward(torch.from_numpy(gpred).double())
    rb, eb, mb = A.regress_bwd_ref(cost, gpred, c['z'])
    assert np.allclose(np.moveaxis(ct.grad.numpy(), 1, -1), rb, rtol=0, atol=1e-12)
    assert np.ptp(cost[0, :, 0, 0, 0]) == 0 and np.ptp(cost, axis=1).max() > 50


@pytest.mark.parametrize('c', G.FUSION_CASES, ids=lambda c: c['name'])
def test_fusion_reference_is_the_oracles(c):
    feat2d, feat3d, gvol = G.make_fusion(c)
    N = c['n']
    vol, mask = A.fusion_fwd_ref(feat2d, feat3d, c['passes'])
    dense = torch.from_numpy(np.ascontiguousarray(np.moveaxis(feat3d, -1, 1)))                     # (B, C, D, H, W)
    sout = type('S', (), {'dense': lambda self: (dense, None, None)})()
    for p in range(c['passes']):
        f2 = torch.from_numpy(np.ascontiguousarray(np.moveaxis(feat2d[p * N:(p + 1) * N], -1, 1)))
        want = np.moveaxis(CO.fusion(sout, f2).numpy(), 1, -1)
        assert np.array_equal(want, vol[p * N:(p + 1) * N]), p
    planes = (feat3d != 0).any(-1).sum(1)
    assert set(np.unique(planes)) >= {0, 1, 2} and set(np.unique(mask)) >= {-1.0, 0.0, 1.0}
    assert mask[0, 4, 0, 0] == mask[0, 5, 0, 0] and mask[0, 11, 1, 1] - mask[0, 12, 1, 1] == 1.0        # a cell of zeros is empty; 1e-30 is not


def test_rows_reference_is_the_oracles_reshape():
    for c in G.ROWS_CASES:
        feat = G.rng_of('rows/' + c['name']).standard_normal((c['n'], c['d'], c['h'], c['w'], c['c'])).astype(F32)
        t = torch.from_numpy(np.ascontiguousarray(np.moveaxis(feat, -1, 1)))                       # (b, c, d, h, w)
        b, ch, d, h, w = t.shape
        want = t.reshape(b, ch * d, h, w).permute(0, 2, 3, 1).reshape(-1, ch * d).numpy()
        assert np.array_equal(want, A.rows_fwd_ref(feat))
        g = A.rows_fwd_ref(feat)
        assert np.array_equal(A.rows_bwd_ref(g, c['n'], c['d'], c['h'], c['w'], c['c']), feat)   # a permutation's transpose is its inverse


# ---- planted wrong arithmetics -----------------------------------------------------------------------------------------------------
def _raises(sp, z, fault):
    try:
        A.check_levels(A.levels_emu(sp, z, fault)[0], sp, z)
    except AssertionError:
        return True
    return False


def _levels_fault(fault):
    names = {'round_half_away': ('halves',), 'keep_plane0': ('halves', 'w68', 'empty_frame'), 'clamp16': ('halves',),
             'scan_no_carry': ('rows1028', 'rows2056', 'l1rows1152'),
             'popc_off_by_one': tuple(c['name'] for c in G.LEVEL_CASES if c['kind'] != 'empty')}[fault]
    for c in G.LEVEL_CASES:
        sp = G.make_levels(c)
        assert not _raises(sp, c['z'], None), c['name']
        if c['name'] in names:
            assert _raises(sp, c['z'], fault), (fault, c['name'])


def _inside(got, ref, mag, tol):
    return bool((np.abs(np.asarray(got, F64) - ref) <= tol * mag).all())


def _conv_fault(fault):
    _, coords, shape = G.conv_geometry(False)
    hit = 0
    for form in G.CONV_FORMS:
        k, ci, co, lin, lout = form
        applies = {'reversed_offsets': k == 3, 'stride_ts_out': k == 3 and lout > lin, 'downsample_offgrid': k == 1 and lout > lin,
                   'transposed_no_ongrid': lout > lin}[fault]
        if not applies:
            continue
        hit += 1
        cin, cout = coords[lin], coords[lout]
        pairs = A.conv_pairs(cin, cout, shape, lin, lout, k)
        if fault == 'transposed_no_ongrid':
            wrong = A.bwd_pairs_transposed(cin, cout, shape, lin, lout, k, fault)
        else:
            wrong = A.conv_pairs(cin, cout, shape, lin, lout, k, fault)
        x, wk, _ = G.make_conv(form, len(cin), len(cout))
        gy, _, prev = G.make_conv(form, len(cin), len(cout), True)
        if fault != 'transposed_no_ongrid':
            emu = A.sparse_conv_emu(x, wk, pairs, len(cout))
            assert _inside(emu, *A.sparse_conv_ref(x, wk, pairs, len(cout)), G.TOL['conv']), form
            assert not _inside(emu, *A.sparse_conv_ref(x, wk, wrong, len(cout)), G.TOL['conv']), (fault, form)
        for p in (None, prev):
            emu = A.sparse_conv_bwd_emu(gy, wk, pairs, len(cin), p)
            assert _inside(emu, *A.sparse_conv_bwd_ref(gy, wk, pairs, len(cin), p), G.TOL['conv_bwd']), form
            assert not _inside(emu, *A.sparse_conv_bwd_ref(gy, wk, wrong, len(cin), p), G.TOL['conv_bwd']), (fault, form)
    assert hit >= 2


def _sbn_fault(fault):
    applies = {'biased_running_var': lambda c: c['mode'] == 'tracked' and c['cnt'] >= 2,
               'one_running_update': lambda c: c['mode'] == 'tracked',
               'mask_pre_residual': lambda c: c['res'] and c['relu'] and c['mode'] != 'eval' and c['cnt'] >= 2,
               'gres_overwritten': lambda c: c['gres'] == 'acc'}[fault]
    hit = 0
    for c in G.SBN_CASES:
        if not applies(c):
            continue
        hit += 1
        d = G.make_sbn(c)
        fw, fmag = G.sbn_reference_fwd(c, d)
        bw, bmag = G.sbn_reference_bwd(c, d, fw, fmag)
        fe, be = G.sbn_emulation(c, d)
        ok = G.sbn_ratios(c, fe, be, (fw, fmag, bw, bmag))
        for q, r in ok.items():
            assert r <= G.TOL[q], (c['name'], q, r)
        if fault in ('biased_running_var', 'one_running_update'):
            wf, _ = G.sbn_reference_fwd(c, d, fault)
            bad = G.sbn_ratios(c, fe, None, (wf, fmag, bw, bmag))
            assert not bad['sbn_rv'] <= G.TOL['sbn_rv'], (fault, c['name'])
            if fault == 'one_running_update':
                assert not bad['sbn_rm'] <= G.TOL['sbn_rm'] and wf['nbt'] != fw['nbt'], (fault, c['name'])
        else:
            wb, _ = G.sbn_reference_bwd(c, d, fw, fmag, fault)
            width = G.TOL_ACC * bmag['gres']
            assert bool((np.abs(be['gres'] - bw['gres']) <= width).all()), c['name']
            assert not bool((np.abs(be['gres'] - wb['gres']) <= width).all()), (fault, c['name'])
            if fault == 'mask_pre_residual':
                bad = G.sbn_ratios(c, fe, be, (fw, fmag, wb, bmag))
                for q in ('sbn_gx', 'sbn_dbeta', 'sbn_dgamma'):
                    assert not bad[q] <= G.TOL[q], (fault, c['name'], q)
    assert hit >= 2


def _dense_fault(fault):
    if fault in ('last_max', 'pool_odd_last_row'):
        hit = 0
        for c in G.POOL_CASES:
            if c['items'] > 4 or (fault == 'pool_odd_last_row' and c['h'] % 2 == 0):
                continue
            x, gy, prev = G.make_pool(c)
            assert not np.array_equal(A.pool_bwd_ref(x, gy, prev if c['acc'] else None), A.pool_bwd_ref(x, gy, prev if c['acc'] else None, fault)), c['name']
            hit += 1
        assert hit >= 1
    elif fault in ('nearest_ceil', 'up_window_narrow'):
        for c in G.UP_CASES:
            x, gy, prev = G.make_up(c)
            if fault == 'nearest_ceil':
                assert not np.array_equal(A.up_fwd_ref(x, *c['o']), A.up_fwd_ref(x, *c['o'], fault)), c['name']
            else:
                assert not np.array_equal(A.up_bwd_ref(gy, *c['i']), A.up_bwd_ref(gy, *c['i'], fault=fault)), c['name']
    elif fault == 'shuffle_4j_i':
        for c in G.REGRESS_CASES:
            cost, gpred = G.make_regress(c)
            ref, emu, mag = A.regress_fwd_ref(cost, c['z'])
            wrong = A.regress_fwd_ref(cost, c['z'], fault)[0]
            assert _inside(emu, ref, mag, G.TOL['regress']) and not _inside(emu, wrong, mag, G.TOL['regress']), c['name']
            ref, emu, mag = A.regress_bwd_ref(cost, gpred, c['z'])
            wrong = A.regress_bwd_ref(cost, gpred, c['z'], fault)[0]
            assert _inside(emu, ref, mag, G.TOL['regress_bwd']) and not _inside(emu, wrong, mag, G.TOL['regress_bwd']), c['name']
    elif fault == 'rows_d_major':
        for c in G.ROWS_CASES:
            feat = G.rng_of('rows/' + c['name']).standard_normal((c['n'], c['d'], c['h'], c['w'], c['c'])).astype(F32)
            rows = A.rows_fwd_ref(feat)
            assert not np.array_equal(rows, A.rows_fwd_ref(feat, fault)), c['name']
            dims = (c['n'], c['d'], c['h'], c['w'], c['c'])
            assert not np.array_equal(A.rows_bwd_ref(rows, *dims), A.rows_bwd_ref(rows, *dims, fault=fault)), c['name']
    elif fault == 'fusion_no_plus_one':
        for c in G.FUSION_CASES:
            feat2d, feat3d, _ = G.make_fusion(c)
            (v0, m0), (v1, m1) = A.fusion_fwd_ref(feat2d, feat3d, c['passes']), A.fusion_fwd_ref(feat2d, feat3d, c['passes'], fault)
            assert not np.array_equal(v0, v1) and not np.array_equal(m0, m1), c['name']
    elif fault == 'pad_corners_swapped':
        for c in G.PAD_CASES:
            image, sparse, net, g, Hp, Wp = G.make_pad(c)
            assert not np.array_equal(A.pad_dual_ref(image, Hp, Wp, c['pt'], c['pr'])[0], A.pad_dual_ref(image, Hp, Wp, c['pt'], c['pr'], fault=fault)[0]), c['name']
            assert not np.array_equal(A.scatter_dual_grad_ref(g, Hp, Wp, c['pt'], c['pr']), A.scatter_dual_grad_ref(g, Hp, Wp, c['pt'], c['pr'], fault)), c['name']
            ref, emu, mag = A.pad_dual_ref(image, Hp, Wp, c['pt'], c['pr'], G.NORM)
            wrong = A.pad_dual_ref(image, Hp, Wp, c['pt'], c['pr'], G.NORM, fault)[0]
            assert _inside(emu, ref, mag, G.TOL['norm']) and not (np.abs(emu - wrong) <= G.TOL['norm'] * mag).all(), c['name']
    elif fault == 'crop_not_halved':
        for c in G.PAD_CASES:
            image, sparse, net, g, Hp, Wp = G.make_pad(c)
            args = (net, c['n'], c['h'], c['w'], c['pt'], c['pr'])
            assert not np.array_equal(A.crop_avg_ref(*args), A.crop_avg_ref(*args, fault)), c['name']
    else:
        raise AssertionError('no cases for ' + fault)


@pytest.mark.parametrize('fault', A.FAULTS)
def test_planted_wrong_arithmetic_is_rejected(fault):
    """The emulation stands in for a correct GPU result: inside the bound of (or equal to) the true reference, and outside the bound of
    (or unequal to) a reference with the fault planted in it, in every case built for the fault -- so every bound is under the smallest
    planted deviation of its operation."""
    if fault in ('round_half_away', 'keep_plane0', 'clamp16', 'scan_no_carry', 'popc_off_by_one'):
        _levels_fault(fault)
    elif fault in ('reversed_offsets', 'stride_ts_out', 'downsample_offgrid', 'transposed_no_ongrid'):
        _conv_fault(fault)
    elif fault in ('biased_running_var', 'one_running_update', 'mask_pre_residual', 'gres_overwritten'):
        _sbn_fault(fault)
    else:
        _dense_fault(fault)
