"""CPU-only side of the per-element tests of the mixed mode's narrow heads (tests/test_gpu_heads_n_elementwise.py): the hooks' declarations
against the binding, the emulation against the float64 references (oracle/heads_n_arith.py), the tolerances, the exact class's bounds, the
cap on ambiguous ReLU-mask elements, the layout helpers as round trips, and the references themselves against torch in float64.

Tolerances (tests/heads_n_cases.py TOL) are 4 x the CPU emulation's largest error ratio per quantity over the cases,
profiles/heads_n_elementwise.txt -- never a GPU figure."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import heads_n_arith as A
from proxytta import _lib
from tests import heads_n_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
HOOKS = ('ptta_op_hn_tiled_elems', 'ptta_op_hn_gemm', 'ptta_op_hn_moments', 'ptta_op_hn_untile', 'ptta_op_head_bwd_finish')


def test_hooks_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    sig = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    for name in HOOKS:
        m = re.search(r'^(int|long long) %s\((.*?)\);' % name, header, re.S | re.M)
        assert m, name
        res, args = sig[name]
        assert res is (ctypes.c_int if m.group(1) == 'int' else ctypes.c_longlong), name
        decl = [a.strip() for a in m.group(2).replace('\n', ' ').split(',')]
        assert len(args) == len(decl), name
        for a, w in zip(args, decl):
            if '*' in w or w.startswith('ptta_stream'):
                assert a is ctypes.c_void_p or hasattr(a, 'contents') or issubclass(a, ctypes._Pointer), (name, w)
            else:
                assert a is {'int': ctypes.c_int, 'long long': ctypes.c_longlong}[re.sub(r'\s+\w+$', '', w)], (name, w)
    for struct, cls in (('ptta_hn_gemm_args', _lib.HnGemmArgs), ('ptta_hn_moments_args', _lib.HnMomentsArgs)):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct), header, re.S).group(1)
        fields = []
        for decl in body.split(';'):
            decl = decl.strip()
            if decl:
                kind = 'ptr' if '*' in decl else re.match(r'(long long|int|float)', decl).group(1)
                rest = re.sub(r'^(const\s+)?(long long|int|float|double|void)\s*\*?', '', decl)
                fields += [(n.strip(' *'), kind) for n in rest.split(',')]
        want = {'ptr': ctypes.c_void_p, 'int': ctypes.c_int, 'long long': ctypes.c_longlong, 'float': ctypes.c_float}
        assert [(n, want[k]) for n, k in fields] == list(cls._fields_), struct         # the same fields, types and order
    assert re.search(r'#define PTTA_ABI_VERSION 2\b', header) and _lib.PTTA_ABI_VERSION == 2          # a new export changes no ABI version


@pytest.fixture(scope='module')
def rows():
    return G.measure()


def test_tolerances_are_four_times_the_emulations_error(rows):
    worst = G.worst(rows)
    assert set(worst) == set(G.TOL) == set(G.QUANTITIES)
    for q, r in worst.items():
        assert r > 0 and 4.0 * r <= G.TOL[q] * 1.001 and G.TOL[q] <= 4.0 * r * 1.001, (q, r, G.TOL[q])
    # fp32 quantities stay a few fp32 roundings of their magnitude (a single row's column sum sees one of its 512 operands rounded the
    # other way to bf16: 2^-9 / 512 of it); the narrow stores a few bf16 roundings (an ulp is part of their magnitude)
    narrow = ('C', 'finish_bf16', 'P', 'bn_g', 'bn_gx')
    assert max(v for q, v in G.TOL.items() if q not in narrow) < 128 * 2.0 ** -24
    assert max(G.TOL['C'], G.TOL['finish_bf16']) < 4 * 2.0 ** -8 and max(G.TOL['P'], G.TOL['bn_g'], G.TOL['bn_gx']) < 2.0 ** -8


def test_profile_holds_the_tolerances():
    text = open(os.path.join(ROOT, 'profiles', 'heads_n_elementwise.txt')).read()
    for q, r in G.RATIO.items():
        assert re.search(r'^%s\s+%s\s' % (q, re.escape('%.3e' % r)), text, re.M), q


def test_every_key_row_count_and_class_is_a_case():
    have = {(c['key'], c['R'], c['cls']) for c in G.GEMM_CASES}
    assert have >= {(k, R, cls) for k in G.KEYS for R in G.ROWS for cls in ('exact', 'real')}
    assert {c['special'] for c in G.GEMM_CASES} >= {'a_slice', 'w_group', 'zero_rows'}
    assert any(c['epi'] == 3 and c['x_bf16'] and c['cls'] == 'real' for c in G.GEMM_CASES)
    assert {(c['R'], c['x_bf16']) for c in G.MOMENT_CASES} >= {(R, xb) for R in (1, 5, 128, 129, 300, 33000) for xb in (False, True)}
    assert (33000 + 127) // 128 > 256 and {c['flavor'] for c in G.MOMENT_CASES} == {'exact', 'real', 'offset', 'const'}
    assert {(c['R'], c['halves'], c['bf16']) for c in G.FINISH_CASES} == {(R, h, b) for R in (1, 129, 300) for h in (1, 2) for b in (False, True)}


@pytest.mark.parametrize('c', [c for c in G.GEMM_CASES if c['cls'] == 'exact'], ids=lambda c: c['name'])
def test_exact_class_is_exact_in_fp32(c):
    """Every accumulation's sum of |terms| stays below 2^24 units, every narrow value is a bf16 value -- and the fp32 emulation, whose
    summation order is not the GPU's, returns the expected bits."""
    d = G.make_gemm(c)
    ref, mag = G.gemm_reference(c, d)
    bound, narrow = G.exact_bound(c, d, ref, mag)
    assert bound < 2 ** 24 and narrow, (bound, narrow)
    emu = G.gemm_emulation(c, d)
    if c['epi'] == 5:
        emu['cc'], emu['ce'] = A._rowsum_emu(emu['C'], emu['C']), A._rowsum_emu(emu['C'], d['E'])
    for q, w in G.exact_expected(c, d, ref).items():
        assert np.array_equal(emu[q], w), q
    # values differ from K slice to K slice and from column to column
    a = ref['A'].reshape(c['R'], 16, 32)
    if c['special'] is None and c['R'] > 1:
        assert len({a[:, s].tobytes() for s in range(16)}) == 16 and len({d['W'][n].tobytes() for n in range(512)}) == 512
    if c['special'] == 'a_slice':
        assert (np.delete(a, G.A_SLICE, 1) == 0).all() and (a[:, G.A_SLICE] != 0).any()
    if c['special'] == 'w_group':
        v = ref['v'].reshape(c['R'], 16, 32)
        assert (np.delete(v, G.W_GROUP, 1) == 0).all() and (v[:, G.W_GROUP] != 0).any()


@pytest.mark.parametrize('c', [c for c in G.GEMM_CASES if c['cls'] == 'real' and c['epi'] == 3], ids=lambda c: c['name'])
def test_ambiguous_relu_mask_elements_stay_under_the_cap(c):
    d = G.make_gemm(c)
    ref, mag = G.gemm_reference(c, d)
    amb = G.ambiguous(c, d, ref, mag)[0]
    assert amb.mean() <= G.AMB_SHARE and amb.sum(1).max() <= G.AMB_ROW, (amb.mean(), amb.sum(1).max())
    on = (ref['pre'] > 0).mean()
    assert 0.3 < on < 0.7, on                                  # about half the ReLUs active


def test_real_class_holds_what_it_claims():
    c = G.GEMM_BY_NAME['real_k43_r129_zero_rows']
    d = G.make_gemm(c)
    assert not d['A'][5].any() and not d['Bref'][5].any() and tuple(d['rowstats'][5]) == (F32(1e-12), F32(1e-12), 0.0)
    ref, _ = G.gemm_reference(c, d)
    assert not ref['A'][5].any() and np.isfinite(ref['A']).all() and np.abs(ref['A'][4]).max() > 0
    c = G.GEMM_BY_NAME['real_k35_r300_zero_rows_xbf16']
    d = G.make_gemm(c)
    assert d['rs'][7] == 0 and np.array_equal(d['X'], G.bfv(d['X']))
    for c in G.GEMM_CASES:
        if c['cls'] == 'real' and c['pro'] in (1, 3) and c['R'] >= 127:
            a = G.gemm_reference(c, G.make_gemm(c))[0]['A']
            assert 0.3 < (a > 0).mean() < 0.7, c['name']


def test_layout_helpers_round_trip():
    rng = G.rng_of('layouts')
    for R in (1, 127, 128, 129, 300):
        bits = rng.integers(0, 0x7f80, (R, 512)).astype(np.uint16)
        t = A.tile(bits, R)
        assert t.size == A.tiled_elems(R) == ((R + 127) // 128) * 128 * 512
        full = A.untile(t, R)
        assert np.array_equal(full[:R], bits) and (full[R:] == A.NAN_BITS).all() and np.isnan(A.bf16_val(full[R:])).all()
        r, k = int(rng.integers(0, R)), int(rng.integers(0, 512))          # the kernel's own index rule (hn_tiled)
        assert t.view(np.uint16)[((r >> 7) * 16 + (k >> 5)) * 4096 + (r & 127) * 32 + (k & 31)] == bits[r, k]
    w = rng.integers(0, 0x7f80, (512, 512)).astype(np.uint16)
    img = A.pack_w(w)
    assert np.array_equal(A.unpack_w(img), w) and sorted(img.reshape(-1).tolist()) == sorted(w.reshape(-1).tolist())
    n, k = 301, 77                                                          # hn_pack_w_kernel's own index rule
    assert img[k >> 5, n, 8 * (((k & 31) >> 3) ^ ((n >> 2) & 3)) + (k & 7)] == w[n, k]
    x = rng.standard_normal(4096).astype(F32)
    assert np.array_equal(A.round_bf16(x.astype(F64)), A.through_bf16(x).astype(F64))       # one rounding either way from fp32
    assert A.bf16_bits(np.array([1.00390625, 1.01171875], F32)).tolist() == [0x3f80, 0x3f82]      # ties to even


def test_references_are_torch_in_float64():
    """Linear(32, 512) - BatchNorm1d (train) - ReLU - Linear(512, 512) forward and autograd's gradient with respect to the input rows,
    against moments -> PRO 3 / EPI 0 forward and PRO 5 / EPI 3 -> head_bwd_finish backward with every rounding switched off."""
    rng = G.rng_of('torch_chain')
    R = 70
    x, w0, b0 = G.bfv(rng.standard_normal((R, 32))), G.bfv(rng.standard_normal((512, 32)) / np.sqrt(32.0)), rng.standard_normal(512).astype(F32) * 0.1
    w, bias = G.bfv(rng.standard_normal((512, 512)) / np.sqrt(512.0)), rng.standard_normal(512).astype(F32) * 0.1
    gamma, beta = rng.uniform(0.5, 1.5, 512), rng.uniform(-0.5, 0.5, 512)
    gout = rng.standard_normal((R, 512))
    rm0, rv0 = rng.uniform(-1, 1, 512), rng.uniform(0.5, 2, 512)
    t = lambda a: torch.from_numpy(np.asarray(a, F64))
    xt = t(x).requires_grad_(True)
    rm, rv = t(rm0).clone(), t(rv0).clone()
    h = torch.nn.functional.linear(xt, t(w0), t(b0))
    a = torch.relu(torch.nn.functional.batch_norm(h, rm, rv, t(gamma), t(beta), training=True, momentum=A.MOMENTUM, eps=A.BN_EPS))
    c = torch.nn.functional.linear(a, t(w), t(bias))
    c.backward(t(gout))
    mom, mag = A.moments_ref(x, w0, b0)
    bn, _ = A.moments_bn_ref(mom, mag, gamma, beta, rm0, rv0)
    assert np.allclose(bn['rm'], rm.numpy(), rtol=0, atol=1e-12) and np.allclose(bn['rv'], rv.numpy(), rtol=0, atol=1e-12)
    part, _ = A.moments_part_ref(mom, mag)
    assert np.allclose(part[0], h.detach().numpy().sum(0), rtol=0, atol=1e-9) and np.allclose(part[1], (h.detach().numpy() ** 2).sum(0), rtol=0, atol=1e-9)
    aref = A.pro3_ref(x, w0, b0, bn['scale'], bn['shift'], A.identity)
    acc, amag = A.gemm_ref(aref, w)
    assert np.allclose(A.epi0_ref(acc, amag, bias)[0], c.detach().numpy(), rtol=0, atol=1e-10)
    # backward: d L / d a = gout W (the transposed weight), through the ReLU and the BatchNorm into P, then the finish
    g, gmag = A.gemm_ref(A.pro5_ref(gout, A.identity), w.T)
    r3, _ = A.epi3_ref(g, gmag, x, w0, b0, bn['scale'], bn['shift'], bn['mean'], bn['inv'], w0.T, R, A.identity)
    c1, c2 = r3['part'].sum(0) / R
    k2 = bn['scale'] * c2 * bn['inv']
    k12 = np.stack([bn['scale'] * c1 + k2 * (b0.astype(F64) - bn['mean']), k2])
    dx, _ = A.finish_ref(r3['P'][None], x, k12, w0)
    assert np.allclose(dx, xt.grad.numpy(), rtol=0, atol=1e-10)
    # and the row statistics of EPI 5 are F.normalize's cosine
    e = rng.standard_normal((R, 512))
    cv = c.detach().numpy()
    r5, _ = A.epi5_ref(cv, e, (e ** 2).sum(1), R, 3)
    cos = (torch.nn.functional.normalize(t(cv), dim=1) * torch.nn.functional.normalize(t(e), dim=1)).sum(1).numpy()
    assert np.allclose(r5['stats'][:, 2], cos, rtol=0, atol=1e-12) and np.isclose(r5['cpart'][0], (2 - 2 * cos).sum(), rtol=0, atol=1e-10)
    # PRO 4 is the gradient of that loss term with respect to the second operand
    et, rt = t(e).requires_grad_(True), t(cv).requires_grad_(True)
    (0.3 * (2 - 2 * (torch.nn.functional.normalize(et, dim=1) * torch.nn.functional.normalize(rt, dim=1)).sum(1)).sum()).backward()
    stats = np.stack([np.sqrt((e ** 2).sum(1)), r5['stats'][:, 1], r5['stats'][:, 2]], 1).astype(F32)
    got = A.pro4_ref(e, cv, stats, -0.6, A.identity)
    assert np.allclose(got, rt.grad.numpy(), rtol=0, atol=1e-6 * np.abs(got).max())


def test_planted_value_slips_are_outside_the_bounds():
    """The value-only mutations planted on the CPU: row sums taken from the unrounded v, column sums that count the padding rows, and the
    packer's swizzle term (n >> 3) & 3."""
    c = G.GEMM_BY_NAME['real_k12_r129']
    d = G.make_gemm(c)
    ref, mag = G.gemm_reference(c, d)
    emu = G.gemm_emulation(c, d)
    (q, g, rf, m, w), = [t for t in G.gemm_checks(c, d, emu, ref, mag) if t[0] == 'rs']
    assert (np.abs(g - rf) <= G.TOL['rs'] * m).all()
    unrounded = ((ref['v']) ** 2).sum(1)
    assert not (np.abs(unrounded - rf) <= G.TOL['rs'] * m).any()
    # column sums that count the padding rows: PRO 1 turns the NaN padding into zeros, so each of the 127 padding rows of the last block adds the bias
    c = G.GEMM_BY_NAME['real_k11_r129']
    d = G.make_gemm(c)
    ref, mag = G.gemm_reference(c, d)
    (q, g, rf, m, w), = [t for t in G.gemm_checks(c, d, G.gemm_emulation(c, d), ref, mag) if t[0] == 'colsum']
    assert (np.abs(g - rf) <= G.TOL[q] * m).all()
    wrong = g.astype(F64).copy()
    wrong[-1] += 127 * d['bias'].astype(F64)
    assert (np.abs(wrong[0] - rf[0]) <= G.TOL[q] * m[0]).all() and not (np.abs(wrong[-1] - rf[-1]) <= G.TOL[q] * m[-1]).any()
    n, k = np.arange(512)[:, None], np.arange(512)[None, :]
    slip = np.zeros((16, 512, 32), np.uint16)
    bits = A.bf16_bits(d['W'])
    slip[(k >> 5) + 0 * n, n + 0 * k, 8 * (((k & 31) >> 3) ^ ((n >> 3) & 3)) + (k & 7)] = bits
    assert not np.array_equal(slip, A.pack_w(bits))
