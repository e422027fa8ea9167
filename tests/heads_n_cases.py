"""The cases of the per-element tests of the mixed mode's narrow heads (tests/test_gpu_heads_n_elementwise.py,
tests/test_heads_n_elementwise_cpu.py): seeded inputs, float64 references (oracle/heads_n_arith.py) and the bounds.

Two classes per GEMM key (pro * 10 + epi) and row count:
  exact  small integers and powers of two such that every intermediate is an integer or dyadic rational fp32 holds exactly -- the result is
         the same under ANY summation order, so C (bf16 bits), part, rs and P (fp32 bits) are compared with array_equal.  exact_bound()
         proves it per case: the largest sum of |terms| of any accumulation, in units of its grid, must stay below 2^24.
  real   standard-normal operands at realistic scales, BatchNorm tables from a true batch statistic of the case's own hidden; compared
         against the float64 reference within TOL[quantity] x the element's magnitude.
TOL = 4 x the largest error ratio |emulation - float64| / magnitude of the CPU emulation (numpy fp32 at the kernel's rounding points) over
these cases -- never a figure from a GPU run.  `python -m tests.heads_n_cases [gpu log]` recomputes the ratios and prints the table kept in
profiles/heads_n_elementwise.txt; the CPU test checks the constants against the recomputed ratios.

rs (EPI 2) and the row statistics and block partials of EPI 5 are checked against the run's OWN stored C (and the given E), summed in
float64: that tells sums of stored values from sums of unrounded ones.

ReLU mask of EPI 3 (real class): an element whose pre-activation lies within BAND x TOL['pre'] x its magnitude of zero may fall on either
side; it is not excluded -- the bounds of its two column sums and of its row of P are widened by exactly that element's own term.  At most
AMB_SHARE of a case's elements and AMB_ROW per row may be ambiguous (counted from the reference alone; a seed that breaks the cap is changed)."""
import zlib

import numpy as np

from oracle import heads_n_arith as A

F32, F64 = np.float32, np.float64
# the largest ratios of profiles/heads_n_elementwise.txt (python -m tests.heads_n_cases)
RATIO = {'C': 1.267e-03, 'colsum': 1.042e-06, 'colsq': 4.463e-07, 'rs': 1.872e-07, 'ne': 5.841e-08, 'nr': 1.135e-07, 'cos': 3.864e-08,
         'cpart': 4.574e-08, 'pre': 1.087e-07, 'bn_g': 2.153e-06, 'bn_gx': 3.261e-06, 'P': 2.915e-05, 'm_part': 1.317e-07, 'm_mean': 1.303e-07,
         'm_inv': 4.172e-08, 'm_scale': 7.646e-08, 'm_shift': 3.822e-08, 'm_rm': 1.425e-07, 'm_rv': 6.249e-08, 'finish': 2.045e-08,
         'finish_bf16': 6.167e-04}
TOL = {q: 4.0 * r for q, r in RATIO.items()}
QUANTITIES = tuple(RATIO)
BAND, AMB_SHARE, AMB_ROW = 64.0, 0.005, 2
KEYS = (10, 11, 12, 30, 31, 35, 43, 53)
ROWS = (1, 127, 128, 129, 300)
TAIL = 8                      # rows of NaN behind R in rs, rowstats_out, P and dX: they must stay untouched
CPART_EXTRA = 5               # cpart slots behind the grid: they must come back exactly 0


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def bfv(x):
    """the bf16 values of an fp32 array, as fp32"""
    return A.through_bf16(np.asarray(x, F32))


# ---- the GEMM cases ---------------------------------------------------------------------------------------------------------------------
def _gc(key, R, cls, special=None, x_bf16=False):
    name = '%s_k%d_r%d%s%s' % (cls, key, R, '_' + special if special else '', '_xbf16' if x_bf16 else '')
    return dict(name=name, key=key, pro=key // 10, epi=key % 10, R=R, cls=cls, special=special, x_bf16=x_bf16)


GEMM_CASES = ([_gc(k, R, 'exact', x_bf16=(k in (35, 53) and R == 129)) for k in KEYS for R in ROWS] +
              [_gc(10, 129, 'exact', 'a_slice'), _gc(30, 129, 'exact', 'w_group')] +
              # real: the narrow feature rows of the proxy frames at one row count of every key that reads X; the zero rows at 129 and 300
              [_gc(k, R, 'real', special=('zero_rows' if (k in (43, 35) and R >= 129) else None), x_bf16=(k in (30, 31, 35, 43) and R == 300))
               for k in KEYS for R in ROWS])
GEMM_BY_NAME = {c['name']: c for c in GEMM_CASES}
W_DENSITY = {1: 1 / 8, 3: 1 / 32, 4: 1 / 32, 5: 1 / 8}          # exact class: share of nonzero weights per prologue (keeps |C| <= 256)
A_SLICE, W_GROUP = 5, 11


def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape).astype(F32)


def _pick(rng, values, shape):
    return np.asarray(values, F32)[rng.integers(0, len(values), shape)]


def _sparse_pm(rng, shape, density, values=(1.0, 1.0, 1.0, 2.0)):
    return (np.where(rng.random(shape) < density, 1.0, 0.0) * _pick(rng, values, shape) * _pick(rng, (-1.0, 1.0), shape)).astype(F32)


def _batch_affine(rng, h64, hbatch):
    """BatchNorm tables from a true batch statistic of the hidden's columns (fewer than 8 rows: of a 64-row batch drawn like them)"""
    src = h64 if h64.shape[0] >= 8 else hbatch
    mean, var = src.mean(0), src.var(0)
    gamma, beta = rng.uniform(0.5, 1.5, 512), rng.uniform(-0.5, 0.5, 512)
    inv = 1.0 / np.sqrt(var + A.BN_EPS)
    return (gamma * inv).astype(F32), (beta - mean * gamma * inv).astype(F32), mean.astype(F32), inv.astype(F32)


def make_gemm(c):
    """the inputs of a case: fp32 arrays (narrow ones hold bf16 values), row-major"""
    rng = rng_of('hn_gemm/' + c['name'])
    R, pro, epi, exact = c['R'], c['pro'], c['epi'], c['cls'] == 'exact'
    d = {}
    if exact:
        d['W'] = _sparse_pm(rng, (512, 512), W_DENSITY[pro])
        d['bias'] = _ints(rng, -3, 3, 512)
    else:
        d['W'] = (rng.standard_normal((512, 512)) / np.sqrt(512.0)).astype(F32)
        d['bias'] = (0.1 * rng.standard_normal(512)).astype(F32)
    if pro == 3 or epi == 3:
        if exact:
            d['X'], d['W0'], d['b0'] = _ints(rng, -2, 2, (R, 32)), _sparse_pm(rng, (512, 32), 0.125, (1.0,)), _ints(rng, -2, 2, 512)
        else:
            d['X'] = rng.standard_normal((R, 32)).astype(F32)
            d['W0'], d['b0'] = (rng.standard_normal((512, 32)) / np.sqrt(32.0)).astype(F32), (0.1 * rng.standard_normal(512)).astype(F32)
            if c['x_bf16']:
                d['X'] = bfv(d['X'])
            xb = bfv(rng.standard_normal((64, 32)))
            h, hb = (A.hidden_ref(bfv(x), bfv(d['W0']), d['b0'])[0] for x in (d['X'], xb))
    if pro == 1:
        if exact:
            d['A'], d['pscale'], d['pshift'] = _ints(rng, -2, 2, (R, 512)), _pick(rng, (0.5, 1.0, 2.0), 512), _ints(rng, -1, 1, 512)
        else:
            col = rng.uniform(0.5, 2.0, 512), rng.uniform(-1.0, 1.0, 512)
            d['A'] = bfv(rng.standard_normal((R, 512)) * col[0] + col[1])
            d['pscale'], d['pshift'] = _batch_affine(rng, d['A'].astype(F64), rng.standard_normal((64, 512)) * col[0] + col[1])[:2]
    elif pro == 3:
        if exact:
            d['pscale'], d['pshift'] = _pick(rng, (0.5, 1.0, 2.0), 512), _ints(rng, -2, 2, 512)
        else:
            d['pscale'], d['pshift'] = _batch_affine(rng, h, hb)[:2]
    elif pro == 4:
        if exact:
            d['A'], d['Bref'] = _ints(rng, -2, 2, (R, 512)), _ints(rng, -2, 2, (R, 512))
            d['rowstats'] = np.stack([_pick(rng, (4.0, 8.0), R), np.full(R, 8.0, F32), _pick(rng, (0.5, 1.0, 0.0, -0.5), R)], 1)
            d['coef'] = np.array([128.0], F32)
        else:
            d['A'], d['Bref'] = bfv(rng.standard_normal((R, 512))), bfv(rng.standard_normal((R, 512)))
            if c['special'] == 'zero_rows':
                d['A'][5], d['Bref'][5] = 0, 0
            d['rowstats'] = A.epi5_emu(d['Bref'], d['A'], A.epi2_emu(d['A']), R, A.row_blocks(R))[0]      # (|emb|, |ref|, cos) as EPI 5 leaves them
            d['coef'] = np.array([-0.1 / R], F32)
    elif pro == 5:
        d['Af'] = _ints(rng, -2, 2, (R, 512)) if exact else rng.standard_normal((R, 512)).astype(F32)
    if epi == 5:
        d['E'] = _ints(rng, -2, 2, (R, 512)) if exact else bfv(rng.standard_normal((R, 512)))
        if c['special'] == 'zero_rows':
            d['E'][7] = 0
        d['rs'] = (d['E'].astype(F64) ** 2).sum(1).astype(F32)
    if epi == 3:
        if exact:
            d['escale'], d['eshift'] = _pick(rng, (1.0, 2.0, 4.0), 512), _ints(rng, -2, 2, 512) + F32(0.5)      # (integer hidden: never 0)
            d['emean'], d['einv'] = _ints(rng, -2, 2, 512), _pick(rng, (0.25, 0.5, 1.0), 512)
            d['W0t'] = _sparse_pm(rng, (32, 512), 0.25, (1.0,))
        else:
            d['escale'], d['eshift'], d['emean'], d['einv'] = _batch_affine(rng, h, hb)
            d['W0t'] = np.ascontiguousarray(d['W0'].T)
    if c['special'] == 'a_slice':               # the A operand is zero outside one K slice
        out = np.ones(512, bool)
        out[32 * A_SLICE:32 * A_SLICE + 32] = False
        d['A'][:, out], d['pshift'][out] = 0, 0
    if c['special'] == 'w_group':               # W (and the bias) is zero outside one group of 32 output columns
        out = np.ones(512, bool)
        out[32 * W_GROUP:32 * W_GROUP + 32] = False
        d['W'][out], d['bias'][out] = 0, 0
    return d


def _operands(c, d):
    """what the matrix cores see: bf16 values of X, W0, W0t, W as float64"""
    o = {k: bfv(d[k]).astype(F64) for k in ('W', 'W0', 'W0t', 'X') if k in d}
    return o


def gemm_reference(c, d, rnd=A.round_bf16):
    """-> (ref, mag): A operand, acc, and per epilogue v / part / P ... in float64 with the magnitudes"""
    o, R, pro, epi = _operands(c, d), c['R'], c['pro'], c['epi']
    if pro == 1:
        a = A.pro1_ref(d['A'].astype(F64), d['pscale'], d['pshift'], rnd)
    elif pro == 3:
        a = A.pro3_ref(o['X'], o['W0'], d['b0'], d['pscale'], d['pshift'], rnd)
    elif pro == 4:
        a = A.pro4_ref(d['A'].astype(F64), d['Bref'].astype(F64), d['rowstats'], d['coef'][0], rnd)
    else:
        a = A.pro5_ref(d['Af'], rnd)
    acc, amag = A.gemm_ref(a, o['W'])
    ref, mag = dict(A=a, acc=acc), dict(acc=amag)
    if epi == 3:
        r3, m3 = A.epi3_ref(acc, amag, o['X'], o['W0'], d['b0'], d['escale'], d['eshift'], d['emean'], d['einv'], o['W0t'], R, rnd)
        ref.update(r3)
        mag.update(m3)
        return ref, mag
    ref['v'], mag['v'] = A.epi0_ref(acc, amag, d['bias'])
    if epi == 1:
        ref['part'], mag['part'] = A.epi1_ref(ref['v'], mag['v'], R)
    return ref, mag


def gemm_emulation(c, d):
    """the fp32 emulation's outputs, named as a GPU run's (gemm_got)"""
    o, R, pro, epi = _operands(c, d), c['R'], c['pro'], c['epi']
    if pro == 1:
        a = A.pro1_emu(d['A'], d['pscale'], d['pshift'])
    elif pro == 3:
        a = A.pro3_emu(o['X'], o['W0'], d['b0'], d['pscale'], d['pshift'])
    elif pro == 4:
        a = A.pro4_emu(d['A'], d['Bref'], d['rowstats'], d['coef'][0])
    else:
        a = A.pro5_emu(d['Af'])
    acc = A.mfma_chain(F32(0), a, o['W'])
    if epi == 3:
        part, P = A.epi3_emu(acc, o['X'], o['W0'], d['b0'], d['escale'], d['eshift'], d['emean'], d['einv'], o['W0t'], R)
        return dict(part=part, P=P, pre=A.fma32(A.hidden_emu(o['X'], o['W0'], d['b0']), d['escale'], d['eshift']))
    v, part = A.epi01_emu(acc, d['bias'], R, epi == 1)
    got = dict(Cbits=A.bf16_bits(v), C=bfv(v).astype(F64))
    if epi == 1:
        got['part'] = part
    if epi == 2:
        got['rs'] = A.epi2_emu(bfv(v))
    if epi == 5:
        got['stats'], got['cpart'] = A.epi5_emu(bfv(v), d['E'], d['rs'], R, A.row_blocks(R) + CPART_EXTRA)
    return got


def ambiguous(c, d, ref, mag):
    """EPI 3: (mask of the ambiguous elements, the widening of part, of P) from the reference alone"""
    return A.epi3_widen(ref['acc'], ref, mag, BAND * TOL['pre'], d['escale'], _operands(c, d)['W0t'], c['R'])


def gemm_checks(c, d, got, ref, mag):
    """[(quantity, got, reference, magnitude, widening)] of a run's (or the emulation's) outputs; the bound is TOL[quantity] x magnitude +
    widening.  rs and the EPI 5 statistics refer to the run's OWN stored C."""
    R, epi, out = c['R'], c['epi'], []
    nb = A.row_blocks(R)
    if epi == 3:
        _, wpart, wP = ambiguous(c, d, ref, mag) if c['cls'] == 'real' else (None, np.zeros((nb, 2, 512)), np.zeros((R, 32)))
        if 'pre' in got:
            out.append(('pre', got['pre'], ref['pre'], mag['pre'], 0.0))
        return out + [('bn_g', got['part'][:, 0], ref['part'][:, 0], mag['part'][:, 0], wpart[:, 0]),
                      ('bn_gx', got['part'][:, 1], ref['part'][:, 1], mag['part'][:, 1], wpart[:, 1]), ('P', got['P'], ref['P'], mag['P'], wP)]
    out.append(('C', got['C'], ref['v'], mag['v'], 0.0))
    if epi == 1:
        out += [('colsum', got['part'][:, 0], ref['part'][:, 0], mag['part'][:, 0], 0.0), ('colsq', got['part'][:, 1], ref['part'][:, 1], mag['part'][:, 1], 0.0)]
    if epi == 2:
        out.append(('rs', got['rs'],) + A.epi2_ref(got['C']) + (0.0,))
    if epi == 5:
        r5, m5 = A.epi5_ref(got['C'], d['E'], d['rs'], R, len(got['cpart']))
        out += [(q, got['stats'][:, j], r5['stats'][:, j], m5['stats'][:, j], 0.0) for j, q in enumerate(('ne', 'nr', 'cos'))]
        out.append(('cpart', got['cpart'][:nb], r5['cpart'][:nb], m5['cpart'][:nb], 0.0))
    return out


def exact_expected(c, d, ref):
    """exact class: {output: the array a run must return bit for bit}"""
    epi = c['epi']
    if epi == 3:
        return dict(part=ref['part'].astype(F32), P=ref['P'].astype(F32))
    out = dict(Cbits=A.bf16_bits(ref['v'].astype(F32)))
    if epi == 1:
        out['part'] = ref['part'].astype(F32)
    if epi == 2:
        out['rs'] = (ref['v'] ** 2).sum(1).astype(F32)
    if epi == 5:
        out['cc'], out['ce'] = (ref['v'] ** 2).sum(1).astype(F32), (ref['v'] * d['E'].astype(F64)).sum(1).astype(F32)
    return out


def exact_bound(c, d, ref, mag):
    """The largest |intermediate| of the case in units of its grid (every value is a multiple of the unit), taken as the sum of |terms| of
    each accumulation, which bounds every partial sum in any order; and whether every narrow value is a bf16 value.  < 2^24 and True: fp32
    holds everything exactly."""
    R, pro, epi = c['R'], c['pro'], c['epi']
    ua = 0.5 if pro in (1, 3) else 1.0                      # grid of the A operand (and, W being integers, of the accumulator)
    narrow = [ref['A']]
    sums = [mag['acc'] / ua]
    if pro == 3 or epi == 3:
        o = _operands(c, d)
        sums.append(A.hidden_ref(o['X'], o['W0'], d['b0'])[1])
    for q in (ref['A'], ref['acc']):
        assert np.array_equal(q / ua, np.rint(q / ua))
    if epi == 3:
        sums += [mag['pre'] / 0.5, A._blocks(np.abs(ref['acc']), R).sum(1) / ua,
                 A._blocks(np.abs(ref['acc'] * (ref['h'] - d['emean'].astype(F64)) * d['einv'].astype(F64)), R).sum(1) / (ua * 0.25),
                 (np.abs(ref['dy']) @ np.abs(_operands(c, d)['W0t']).T) / ua]
        narrow.append(ref['acc'] * d['escale'].astype(F64))
        assert (np.abs(ref['pre']) >= 0.5).all()             # no pre-activation anywhere near zero
    else:
        v = ref['v']
        narrow.append(v)
        sums.append(mag['acc'] / ua + np.abs(d['bias'].astype(F64)) / ua)
        if epi == 1:
            sums += [A._blocks(np.abs(v), R).sum(1) / ua, A._blocks(v * v, R).sum(1) / ua ** 2]
        if epi in (2, 5):
            sums.append((v * v).sum(1) / ua ** 2)
        if epi == 5:
            sums.append(np.abs(v * d['E'].astype(F64)).sum(1) / ua)
    return max(float(np.max(s)) for s in sums), all(np.array_equal(A.round_bf16(q), q) for q in narrow)


# ---- the moments chain ------------------------------------------------------------------------------------------------------------------
MOMENT_ROWS = (1, 5, 128, 129, 300, 33000)              # 33000 rows: 258 partial sets, past the reduce kernel's unrolled 256


def _mc(R, flavor, x_bf16):
    return dict(name='%s_r%d_%s' % (flavor, R, 'bf16' if x_bf16 else 'f32'), R=R, flavor=flavor, x_bf16=x_bf16)


MOMENT_CASES = ([_mc(R, f, xb) for f in ('exact', 'real') for R in MOMENT_ROWS for xb in (False, True)] +
                [_mc(R, f, xb) for f in ('offset', 'const') for R in (129, 300) for xb in (False, True)])
CONST_CH, CONST_UNIT, ZERO_UNIT = 7, 3, 4


def make_moments(c):
    """X [2 passes][R][32] (pass 0 alone is the npass = 1 input), W0, b0 and a BatchNorm state"""
    rng = rng_of('hn_moments/' + c['name'])
    R = c['R']
    if c['flavor'] == 'exact':
        x, w0, b0 = _ints(rng, -3, 3, (2, R, 32)), _ints(rng, -2, 2, (512, 32)), _ints(rng, -3, 3, 512)
    else:
        x = (rng.standard_normal((2, R, 32)) * rng.uniform(0.5, 2.0, 32) + rng.uniform(-0.5, 0.5, 32)).astype(F32)
        w0, b0 = (rng.standard_normal((512, 32)) / np.sqrt(32.0)).astype(F32), (0.1 * rng.standard_normal(512)).astype(F32)
        if c['flavor'] == 'offset':             # a common offset of 30 standard deviations: C = S / n - m m^T cancels 900 : 1
            x = (x.astype(F64) / x.std() + 30.0).astype(F32)
        if c['flavor'] == 'const':              # a constant channel, a hidden unit that reads it alone (variance 0), and one that reads nothing
            x[:, :, CONST_CH] = 1.75
            w0[CONST_UNIT], w0[ZERO_UNIT] = 0, 0
            w0[CONST_UNIT, CONST_CH] = 0.8125
    if c['x_bf16']:
        x = bfv(x)
    return dict(X=x, W0=w0, b0=b0, gamma=rng.uniform(0.5, 1.5, 512).astype(F32), beta=rng.uniform(-0.5, 0.5, 512).astype(F32),
                rm=rng.uniform(-1.0, 1.0, 512).astype(F32), rv=rng.uniform(0.5, 2.0, 512).astype(F32), nbt=7)


def moments_reference(d, p):
    return A.moments_ref(d['X'][p], d['W0'], d['b0'])


def moments_checks(d, refs, part=None, bn=None, tracked=False, pass0=0):
    """[(quantity, got, reference, magnitude)]: part [npass][2][2][512] against the passes' references; bn = dict of the direct outputs"""
    out = []
    if part is not None:
        for p in range(part.shape[0]):
            r, m = A.moments_part_ref(*refs[pass0 + p])
            out.append(('m_part', part[p].astype(F64).sum(0), r, m))
    if bn is not None:
        r, m = A.moments_bn_ref(*refs[0], d['gamma'], d['beta'], d['rm'] if tracked else None, d['rv'] if tracked else None)
        out += [('m_' + q, bn[q], r[q], m[q]) for q in ('mean', 'inv', 'scale', 'shift') + (('rm', 'rv') if tracked else ())]
    return out


def moments_emulation(d, p):
    return A.moments_emu(d['X'][p], d['W0'], d['b0'])


# ---- head_bwd_finish --------------------------------------------------------------------------------------------------------------------
FINISH_CASES = [dict(name='r%d_h%d_%s' % (R, hv, 'bf16' if b else 'f32'), R=R, halves=hv, bf16=b) for R in (1, 129, 300) for hv in (1, 2) for b in (False, True)]


def make_finish(c):
    rng = rng_of('hn_finish/' + c['name'])
    R = c['R']
    return dict(P=rng.standard_normal((c['halves'], R, 32)).astype(F32), X=rng.standard_normal((R, 32)).astype(F32),
                W0=(rng.standard_normal((512, 32)) / np.sqrt(32.0)).astype(F32), k12=0.1 * rng.standard_normal((2, 512)))


def finish_reference(c, d):
    ref, mag = A.finish_ref(d['P'], d['X'], d['k12'], d['W0'])
    return ref, mag + (A.ulp_bf16(ref) if c['bf16'] else 0.0)


# ---- the emulation's ratios -------------------------------------------------------------------------------------------------------------
def ratio(got, ref, mag, widen=0.0):
    """largest (|got - ref| - widening) / mag (0 / 0 counts as 0; anything over a zero magnitude as inf)"""
    err = np.maximum(np.abs(np.asarray(got, F64) - ref) - widen, 0.0)
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / mag)
    return float(r.max())


def measure():
    """[(op, case, {quantity: the emulation's ratio})]"""
    rows = []
    for c in GEMM_CASES:
        d = make_gemm(c)
        ref, mag = gemm_reference(c, d)
        r = {}
        for q, g, rf, m, w in gemm_checks(c, d, gemm_emulation(c, d), ref, mag):
            r[q] = max(r.get(q, 0.0), ratio(g, rf, m, w))
        rows.append(('gemm', c['name'], r))
    for c in MOMENT_CASES:
        d = make_moments(c)
        refs = [moments_reference(d, p) for p in range(2)]
        emus = [moments_emulation(d, p) for p in range(2)]
        part = np.stack([np.stack([A.moments_part_emu(e), np.zeros((2, 512))], 0) for e in emus])
        r = {}
        for q, g, rf, m in moments_checks(d, refs, part, A.moments_bn_emu(emus[0], d['gamma'], d['beta'], d['rm'], d['rv']), True):
            r[q] = max(r.get(q, 0.0), ratio(g, rf, m))
        rows.append(('moments', c['name'], r))
    for c in FINISH_CASES:
        d = make_finish(c)
        ref, mag = finish_reference(c, d)
        rows.append(('finish', c['name'], {'finish_bf16' if c['bf16'] else 'finish': ratio(A.finish_emu(d['P'], d['X'], d['k12'], d['W0'], c['bf16']), ref, mag)}))
    return rows


def worst(rows):
    out = {q: 0.0 for q in QUANTITIES}
    for _, _, r in rows:
        for q, v in r.items():
            out[q] = max(out[q], v)
    return out


def report(rows, gpu=None):
    """The generated part of profiles/heads_n_elementwise.txt: the emulation's ratios, TOL = 4 x, and next to each the largest ratio of a GPU
    run (gpu = [(quantity, case, ratio)] read from the test's printed lines; information only)."""
    w = worst(rows)
    big = lambda q: max((r for qq, _, r in gpu or () if qq == q), default=None)
    out = ['quantity      CPU emulation   TOL = 4 x    largest on the GPU (information only, never a bound)']
    for q in QUANTITIES:
        out.append('%-13s %-15.3e %-12.3e %s' % (q, w[q], 4 * w[q], '-' if big(q) is None else '%.3e' % big(q)))
    out += ['', 'Per case, CPU emulation (exact-class GEMM cases whose ratios are all 0 are left out):', '']
    for op, name, r in rows:
        if op != 'gemm' or any(r.values()):
            out.append('%-8s %-28s %s' % (op, name, '  '.join('%s %.3e' % (q, v) for q, v in r.items())))
    if gpu:
        out += ['', 'Per comparison, GPU (nonzero ratios):', ''] + ['%-13s %-44s %.3e' % g for g in gpu if g[2] > 0]
    return '\n'.join(out) + '\n'


def read_gpu_log(path):
    """The 'heads_n <quantity> <case>: largest |error| / magnitude <ratio>' lines tests/test_gpu_heads_n_elementwise.py prints (pytest -s)."""
    import re
    out = []
    for line in open(path):
        m = re.search(r'heads_n (\w+) (.*?): largest \|error\| / magnitude (\S+)', line)
        if m and m.group(1) in QUANTITIES:
            out.append((m.group(1), m.group(2), float(m.group(3))))
    return out


if __name__ == '__main__':
    import sys
    print(report(measure(), read_gpu_log(sys.argv[1]) if len(sys.argv) > 1 else None), end='')
