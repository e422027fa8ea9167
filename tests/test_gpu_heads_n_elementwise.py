"""The narrow heads of the mixed mode (csrc/heads_n.hip: hn_gemm_kernel in its eight PRO x EPI forms, the moments chain, hn_pack_w_kernel,
hn_untile_kernel) and head_bwd_finish_kernel (csrc/heads_bn.hip) per element, through the stand-alone hooks (include/ptta.h
ptta_op_hn_gemm, ptta_op_hn_moments, ptta_op_hn_untile, ptta_op_head_bwd_finish) against the plain references of oracle/heads_n_arith.py on
the cases of tests/heads_n_cases.py.

Exact-class cases are compared with array_equal (bf16 bits of C, fp32 bits of part, rs, P); arithmetic against the float64 reference within
TOL[quantity] x the element's magnitude (tests/heads_n_cases.py: 4 x the CPU emulation's own error, never a GPU figure), every element, none
excluded.  Every tiled input carries NaN in its padding rows and every output starts as NaN.  Each comparison prints its largest ratio;
profiles/heads_n_elementwise.txt keeps them."""
import numpy as np
import pytest
import torch

from oracle import heads_n_arith as A
from tests import heads_n_cases as G
from tests.util import assert_elementwise

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
NARROW = ('A', 'Bref', 'E')


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')


def host(t):
    return t.cpu().numpy()


def as4(a):
    a = np.asarray(a, F64)
    return a.reshape((1,) * (4 - a.ndim) + a.shape)


def check(name, q, got, ref, mag, widen=0.0):
    got, ref, mag = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(mag, F64)
    print('heads_n %s %s: largest |error| / magnitude %.3e (TOL %.3e)' % (q, name, G.ratio(got, ref, mag, widen), G.TOL[q]))
    assert_elementwise(as4(got), as4(ref), as4(G.TOL[q] * mag + widen), '%s %s' % (q, name))


def gemm_buffers(c, d):
    """the device tensors of a case: tiled inputs with NaN in the padding rows, every output NaN (TAIL rows / CPART_EXTRA slots to spare)"""
    R, epi = c['R'], c['epi']
    nb = A.row_blocks(R)
    t = {k: dev(v) for k, v in d.items() if k not in NARROW and k != 'X'}
    for k in NARROW:
        if k in d:
            t[k] = dev(A.tile(A.bf16_bits(d[k]), R))
    if 'X' in d:
        t['X'] = dev(A.bf16_bits(d['X']).view(np.int16)) if c['x_bf16'] else dev(d['X'])
    if epi != 3:
        t['C'] = dev(np.full(A.tiled_elems(R), A.NAN_BITS, np.uint16).view(np.int16))
    if epi in (1, 3):
        t['part'] = nan(nb, 2, 512)
    if epi == 2:
        t['rs'] = nan(R + G.TAIL)
    if epi == 5:
        t['rowstats_out'], t['cpart'] = nan(R + G.TAIL, 3), nan(nb + G.CPART_EXTRA)
    if epi == 3:
        t['P'] = nan(R + G.TAIL, 32)
        t.pop('bias')                                   # (the gradient GEMM has none)
    return t


def gemm_got(c, t):
    """the outputs as numpy, with the assertions on NaN, the untouched tails and the cleared slots"""
    R, epi = c['R'], c['epi']
    nb = A.row_blocks(R)
    got = {}
    if epi != 3:
        bits = A.untile(host(t['C']), R)[:R]
        got['Cbits'], got['C'] = bits, A.bf16_val(bits).astype(F64)
        assert not np.isnan(got['C']).any()
    if epi in (1, 3):
        got['part'] = host(t['part'])
        assert not np.isnan(got['part']).any()
    for name, key in (('rs', 'rs'), ('stats', 'rowstats_out'), ('P', 'P')):
        if key in t and not (key == 'rs' and epi == 5):
            full = host(t[key])
            got[name] = full[:R]
            assert not np.isnan(full[:R]).any() and np.isnan(full[R:]).all(), key          # rows from R on untouched
    if epi == 5:
        got['cpart'] = host(t['cpart'])
        assert not np.isnan(got['cpart'][:nb]).any() and (got['cpart'][nb:] == 0).all() and not np.signbit(got['cpart'][nb:]).any()
    return got


def check_image(name, image, w):
    """the packers, bit for bit: ptta_split_weight's hi plane through hn_pack_w_kernel's swizzle; names the first element that differs"""
    want = A.pack_w(A.bf16_bits(w))
    bad = np.argwhere(image != want)
    if len(bad):
        s, n, p = bad[0]
        k = 32 * s + 8 * ((p >> 3) ^ ((n >> 2) & 3)) + (p & 7)
        raise AssertionError('packed weight image %s: %d of %d elements differ; first at (slice %d, row n %d, position %d) = W[%d][%d]: got 0x%04x want 0x%04x; '
                             'failing 16-byte chunks %s' % (name, len(bad), want.size, s, n, p, n, k, image[s, n, p], want[s, n, p], np.unique(bad[:, 2] >> 3).tolist()))


@pytest.mark.parametrize('c', G.GEMM_CASES, ids=lambda c: c['name'])
def test_hn_gemm(c):
    from proxytta.engine import hn_tiled_elems, op_hn_gemm
    d = G.make_gemm(c)
    R = c['R']
    assert hn_tiled_elems(R) == A.tiled_elems(R)
    t = gemm_buffers(c, d)
    t['w_image'] = torch.zeros(16, 512, 32, dtype=torch.int16, device='cuda')
    op_hn_gemm(c['pro'], c['epi'], R, x_bf16=c['x_bf16'], cpart_n=A.row_blocks(R) + G.CPART_EXTRA if c['epi'] == 5 else 0, **t)
    got = gemm_got(c, t)
    ref, mag = G.gemm_reference(c, d)
    if c['cls'] == 'exact':
        bound, narrow = G.exact_bound(c, d, ref, mag)
        assert bound < 2 ** 24 and narrow
        want = G.exact_expected(c, d, ref)
        if c['epi'] == 5:                               # the sums EPI 5 takes, recomputed from what it stored
            got['cc'], got['ce'] = (got['C'] ** 2).sum(1).astype(F32), (got['C'] * d['E'].astype(F64)).sum(1).astype(F32)
        for q, w in want.items():
            if not np.array_equal(got[q], w):           # name the worst element before failing
                assert_elementwise(as4(A.bf16_val(got[q]) if q == 'Cbits' else got[q]), as4(A.bf16_val(w) if q == 'Cbits' else w), as4(np.zeros(w.shape)),
                                   'exact %s %s' % (q, c['name']))
                raise AssertionError('exact %s %s: bit patterns differ' % (q, c['name']))
            print('heads_n exact %s %s: equal' % (q, c['name']))
    for q, g, rf, m, w in G.gemm_checks(c, d, got, ref, mag):
        check(c['name'], q, g, rf, m, w)
    check_image(c['name'], host(t['w_image']).view(np.uint16), d['W'])


def test_hn_untile_is_the_layouts_inverse():
    from proxytta.engine import op_hn_untile
    for R in (1, 129, 300):
        bits = A.bf16_bits(G.rng_of('untile/%d' % R).standard_normal((R, 512)).astype(F32))
        out = nan(R + G.TAIL, 512)
        op_hn_untile(dev(A.tile(bits, R)), out, R)
        full = host(out)
        assert np.array_equal(full[:R], A.bf16_val(bits)) and np.isnan(full[R:]).all()
    with pytest.raises(RuntimeError, match=r'\(-22\)'):
        op_hn_untile(dev(A.tile(bits, R)), out, 0)


# ---- the moments chain ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', G.MOMENT_CASES, ids=lambda c: c['name'])
def test_hn_moments(c):
    from proxytta.engine import op_hn_moments
    d = G.make_moments(c)
    R, xb = c['R'], c['x_bf16']
    refs = [G.moments_reference(d, p) for p in range(2)]
    x = dev(A.bf16_bits(d['X']).view(np.int16)) if xb else dev(d['X'])
    w0, b0 = dev(d['W0']), dev(d['b0'])
    pow2 = c['flavor'] == 'exact' and R in (1, 128)          # exact sums and n a power of two: the mean is exact
    for npass in (1, 2):
        part = nan(npass, 2, 2, 512)
        op_hn_moments(x, w0, b0, R, npass=npass, x_bf16=xb, part=part)
        part = host(part)
        assert not np.isnan(part).any()
        for q, g, rf, m in G.moments_checks(d, refs, part=part):
            check('%s npass %d' % (c['name'], npass), q, g, rf, m)
        if pow2:
            for p in range(npass):
                assert np.array_equal(part[p, 0, 0].astype(F64) + part[p, 1, 0].astype(F64), R * refs[p][0]['mean'])
    for tracked in (True, False):
        out = {q: nan(512) for q in ('mean', 'inv', 'scale', 'shift')}
        st = dict(rm=dev(d['rm']), rv=dev(d['rv']), nbt=torch.tensor([d['nbt']], dtype=torch.int64, device='cuda')) if tracked else {}
        op_hn_moments(x, w0, b0, R, x_bf16=xb, bn=True, gamma=dev(d['gamma']), beta=dev(d['beta']), **out, **st)
        bn = {q: host(v) for q, v in dict(out, **st).items()}
        assert not any(np.isnan(v).any() for v in bn.values())
        for q, g, rf, m in G.moments_checks(d, refs, bn=bn, tracked=tracked):
            check('%s tracked %d' % (c['name'], tracked), q, g, rf, m)
        if tracked:
            assert int(bn['nbt'][0]) == d['nbt'] + 1
        if pow2:
            assert np.array_equal(bn['mean'], refs[0][0]['mean'].astype(F32))
        if c['flavor'] == 'const':                       # the variance of a unit that reads nothing, or a constant channel alone, is clamped at 0
            assert bn['inv'][G.ZERO_UNIT] == F32(1.0 / np.sqrt(A.BN_EPS)) and bn['inv'][G.CONST_UNIT] <= F32(1.0 / np.sqrt(A.BN_EPS))


# ---- head_bwd_finish --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', G.FINISH_CASES, ids=lambda c: c['name'])
def test_head_bwd_finish(c):
    from proxytta.engine import op_head_bwd_finish
    d = G.make_finish(c)
    R = c['R']
    if c['bf16']:
        dx = dev(np.full((R + G.TAIL, 32), A.NAN_BITS, np.uint16).view(np.int16))
    else:
        dx = nan(R + G.TAIL, 32)
    op_head_bwd_finish(dev(d['k12']), dev(d['W0']), dev(d['P']), dev(d['X']), R, dx, halves=c['halves'], dx_bf16=c['bf16'])
    full = A.bf16_val(host(dx).view(np.uint16)) if c['bf16'] else host(dx)
    assert not np.isnan(full[:R]).any() and np.isnan(full[R:]).all()
    ref, mag = G.finish_reference(c, d)
    check(c['name'], 'finish_bf16' if c['bf16'] else 'finish', full[:R], ref, mag)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _needs(key):
    pro, epi = key // 10, key % 10
    need = ['W'] + {1: ['A', 'pscale', 'pshift'], 3: ['X', 'W0', 'b0', 'pscale', 'pshift'], 4: ['A', 'Bref', 'rowstats', 'coef'], 5: ['Af']}[pro]
    need += {0: ['C'], 1: ['C', 'part'], 2: ['C', 'rs'], 5: ['C', 'E', 'rs', 'rowstats_out', 'cpart'],
             3: ['X', 'W0', 'W0t', 'b0', 'escale', 'eshift', 'emean', 'einv', 'part', 'P']}[epi]
    return sorted(set(need))


REFUSALS = ([(key, 'no_' + f) for key in G.KEYS for f in _needs(key)] + [(10, 'r0'), (10, 'key_20'), (10, 'key_13'), (35, 'key_32'), (35, 'cpart_short')])


@pytest.mark.parametrize('key,rule', REFUSALS, ids=lambda v: str(v))
def test_hn_gemm_refuses_and_writes_nothing(key, rule):
    """one -22 per rule of ptta_launch_hn_gemm: a pointer its pro / epi needs missing, an unknown key, cpart_n below the grid, R < 1"""
    from proxytta.engine import op_hn_gemm
    c = G.GEMM_BY_NAME['exact_k%d_r300' % key]
    d = G.make_gemm(c)
    t = gemm_buffers(c, d)
    pro, epi, R, cpart_n = c['pro'], c['epi'], c['R'], A.row_blocks(c['R']) + G.CPART_EXTRA
    if rule.startswith('no_'):
        t.pop(rule[3:])
    elif rule == 'r0':
        R = 0
    elif rule.startswith('key_'):
        pro, epi = int(rule[4]), int(rule[5])
    elif rule == 'cpart_short':
        cpart_n = A.row_blocks(R) - 1
    with pytest.raises(RuntimeError, match=r'\(-22\)'):
        op_hn_gemm(pro, epi, R, x_bf16=c['x_bf16'], cpart_n=cpart_n if c['epi'] == 5 else 0, **t)
    for k in ('C', 'part', 'rs', 'rowstats_out', 'cpart', 'P'):
        if k in t and not (k == 'rs' and c['epi'] == 5):
            v = host(t[k])
            assert (v.view(np.uint16) == A.NAN_BITS).all() if k == 'C' else np.isnan(v).all(), k


@pytest.mark.parametrize('rule', ('no_X', 'no_W0', 'no_b0', 'no_output', 'r0', 'npass0', 'bn_npass2', 'bn_no_mean', 'bn_rm_without_rv'))
def test_hn_moments_refuses_and_writes_nothing(rule):
    from proxytta.engine import op_hn_moments
    d = G.make_moments(G.MOMENT_CASES[4])
    a = dict(x=dev(d['X']), w0=dev(d['W0']), b0=dev(d['b0']), r=d['X'].shape[1], npass=1, part=nan(2, 2, 2, 512))
    out = {q: nan(512) for q in ('mean', 'inv', 'scale', 'shift')}
    bn = dict(bn=True, gamma=dev(d['gamma']), beta=dev(d['beta']), **out)
    if rule in ('no_X', 'no_W0', 'no_b0'):
        a[rule[3:].lower()] = None
    elif rule == 'no_output':
        a['part'] = None
    elif rule == 'r0':
        a['r'] = 0
    elif rule == 'npass0':
        a['npass'] = 0
    elif rule == 'bn_npass2':
        a.update(bn, npass=2)
    elif rule == 'bn_no_mean':
        a.update(bn, mean=None)
    elif rule == 'bn_rm_without_rv':
        a.update(bn, rm=dev(d['rm']))
    with pytest.raises(RuntimeError, match=r'\(-22\)'):
        op_hn_moments(a.pop('x'), a.pop('w0'), a.pop('b0'), a.pop('r'), **a)
    assert all(np.isnan(host(v)).all() for v in list(out.values()) + ([a['part']] if a.get('part') is not None else []))
    if rule == 'bn_rm_without_rv':
        assert np.array_equal(host(a['rm']), d['rm'])


def test_head_bwd_finish_refuses():
    from proxytta.engine import op_head_bwd_finish
    c = G.FINISH_CASES[0]
    d = G.make_finish(c)
    dx = nan(c['R'] + G.TAIL, 32)
    for r, halves in ((0, 1), (c['R'], 3), (c['R'], 0)):
        with pytest.raises(RuntimeError, match=r'\(-22\)'):
            op_head_bwd_finish(dev(d['k12']), dev(d['W0']), dev(d['P']), dev(d['X']), r, dx, halves=halves)
    assert np.isnan(host(dx)).all()
