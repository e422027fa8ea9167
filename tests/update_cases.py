"""The cases of the per-element tests of the update half of a step (tests/test_gpu_update_elementwise.py,
tests/test_update_elementwise_cpu.py): seeded inputs, float64 references (oracle/update_arith.py) and the bounds.

Real-valued outputs: |got - ref64| <= TOL x 2^-24 x scale, scale = the float64 sum of the absolute values of the element's terms
(oracle/update_arith.py).  TOL belongs to ONE case and quantity: 4 x the ratio |emulation - ref64| / (2^-24 scale) that the CPU's fp32
emulation of the same operation shows on that same case (the factor covers another summation order on the device) -- never a figure from a
GPU run.  A case whose emulation is exact (one term, or sums of few short values) has TOL 0: the kernel has to be exact there too.
tests/update_ratios.py holds the emulation's ratios, keyed by operation and case; `python -m tests.update_cases --table` regenerates it,
`python -m tests.update_cases [gpu log]` prints the table kept in profiles/update_elementwise.txt, and the CPU test checks the stored ratios
against recomputed ones.  Exact classes (the same launch through two hooks, a view against the dense call, bf16 against fp32 gradients of
bf16 values, the three sites of ptta_adam_update, the EMA) are compared for equality."""
import functools
import zlib

import numpy as np

from oracle import update_arith as A
from tests.update_ratios import RATIO          # {operation: {case: {quantity: the emulation's ratio, in units of 2^-24 x scale}}}

F32, F64 = np.float32, np.float64
U = A.U
QUANTITIES = ('wgrad32_w', 'wgrad32_b', 'gwgrad_w', 'gwgrad_b', 'adam_p', 'adam_m', 'adam_v', 'lin_w', 'lin_b', 'glin_w', 'glin_b')
PAD = 64                      # NaN elements behind every output: they must stay untouched


def tol(op, case, q):
    """the case's own tolerance: 4 x its emulation's ratio"""
    return 4.0 * RATIO[op][case][q]


def bound(op, case, q, scale):
    return tol(op, case, q) * U * np.asarray(scale, F64)


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def bfv(x):
    return A.through_bf16(np.asarray(x, F32))


def ratio(got, ref, scale):
    """largest |got - ref| / (2^-24 scale) (0 / 0 counts as 0; anything over a zero scale as inf)"""
    err = np.abs(np.asarray(got, F64) - ref)
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / (U * np.asarray(scale, F64)))
    return float(r.max())


# ---- wgrad32 ------------------------------------------------------------------------------------------------------------------------------
# fewer than 8 pixels (every tap but the centre outside); 70 pixels = two chunks, a batch boundary inside a chunk; 513 = 64 x 8 + 1; 33,024 >
# 512 chunks x 64 (per = 72, the chunks from 459 on are empty)
WGRAD32_MAPS = ((1, 1, 1), (1, 1, 3), (1, 3, 1), (2, 5, 7), (1, 9, 57), (1, 96, 344))


def _wc(b, h, w, bf16, co_stride=288, group=0, bias=True):
    name = '%dx%dx%d_%s_s%d_g%d%s' % (b, h, w, 'bf16' if bf16 else 'f32', co_stride, group, '' if bias else '_nobias')
    return dict(name=name, b=b, h=h, w=w, bf16=bf16, co_stride=co_stride, group=group, bias=bias,
                data='%dx%dx%d_%s' % (b, h, w, 'bf16' if bf16 else 'f32'))          # the arithmetic (and the emulation's ratio) is the map's and the type's


WGRAD32_CASES = ([_wc(b, h, w, bf) for (b, h, w) in WGRAD32_MAPS for bf in (False, True)] +
                 # a 32-channel group of a [32][128][3][3] weight at each of the four group offsets, no bias (the 2layers block's call)
                 [_wc(2, 5, 7, bool(g & 1), 1152, g, False) for g in range(4)] + [_wc(1, 9, 57, False, 288, 0, False)])


@functools.lru_cache(maxsize=4)
def wgrad32_data(b, h, w, bf16):
    """x, gy (fp32 arrays; bf16 cases hold bf16 values) and the float64 reference of the values the kernel reads"""
    rng = rng_of('wgrad32/%d/%d/%d/%d' % (b, h, w, bf16))
    x = rng.standard_normal((b, h, w, 32)).astype(F32)
    gy = (rng.standard_normal((b, h, w, 32)) * rng.uniform(0.01, 1.0, 32) + rng.uniform(-0.05, 0.05, 32)).astype(F32)
    if bf16:
        x, gy = bfv(x), bfv(gy)
    ref, mag = A.conv_wgrad_ref(x, gy)
    for a in (x, gy) + ref + mag:
        a.setflags(write=False)
    return x, gy, ref, mag


# ---- gwgrad on views, bf16 gradients, Adam inside the reduction ---------------------------------------------------------------------------
GW_PAIRS = ((32, 32), (24, 32), (64, 64), (32, 128), (128, 32))           # (ci, co): one tile pair, a partly empty tile, 2 x 2, 1 x 4, 4 x 1
GW_MAPS = ((1, 24, 40), (2, 17, 37), (1, 1, 1), (1, 3, 17))               # W = 16 k + 1: a one-pixel last item in every row
GW_CASES = [dict(name='%dto%d_%dx%dx%d' % (ci, co, b, h, w), ci=ci, co=co, b=b, h=h, w=w) for ci, co in GW_PAIRS for b, h, w in GW_MAPS]
GW_REFUSED_BF16 = ((16, 16), (48, 256))
X_OFF, X_PAD, G_OFF, G_PAD = 8, 8, 8, 16                                    # the views: first channel, ld - C


@functools.lru_cache(maxsize=4)
def gwgrad_data(ci, co, b, h, w):
    """x and gy as fp32 with the float64 reference of them, and gy16: gy rounded to bf16 values, as fp32 (so that an fp32 and a bf16 call
    can read the same numbers)"""
    rng = rng_of('gwgrad/%d/%d/%d/%d/%d' % (ci, co, b, h, w))
    x = rng.standard_normal((b, h, w, ci)).astype(F32)
    gy = (rng.standard_normal((b, h, w, co)) * 1e-2 + rng.uniform(-5e-3, 5e-3, co)).astype(F32)
    ref, mag = A.conv_wgrad_ref(x, gy)
    gy16 = bfv(gy)
    for a in (x, gy, gy16) + ref + mag:
        a.setflags(write=False)
    return x, gy, gy16, ref, mag


def view_buffer(a, off, pad):
    """[..., C] -> a NaN-filled [..., C + pad] buffer with the values at channels off .. off + C (flat), and the view's first element"""
    buf = np.full(a.shape[:-1] + (a.shape[-1] + pad,), np.nan, F32)
    buf[..., off:off + a.shape[-1]] = a
    return buf.reshape(-1), off


HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
FUSED_WD = 1e-4                # weight decay of the Adam-inside-the-reduction cases
FUSED_CASES = [dict(name='%dto%d_t%d%s' % (ci, co, t0, '' if bias else '_nobias'), ci=ci, co=co, b=2, h=17, w=37, start=t0, bias=bias)
               for ci, co in ((32, 32), (24, 32)) for t0 in (0, 7) for bias in (True, False)]


def adam_state(name, n, gscale=1.0):
    """p, m, v of n elements as after some steps of gradients of size gscale"""
    rng = rng_of('state/' + name)
    return (rng.standard_normal(n).astype(F32), (0.1 * gscale * rng.standard_normal(n)).astype(F32),
            ((0.1 * gscale * rng.standard_normal(n)) ** 2).astype(F32))


# ---- the Adam and EMA tables --------------------------------------------------------------------------------------------------------------
TABLE_SIZES = (1, 255, 256, 257, 9216, 32, 70001)          # 80,018 elements: above the 256 x 256 threads of adam_multi's largest grid
TABLE_REPS = {'rep1': (1, 1, 1, 1, 1, 1, 1), 'rep0_first': (0, 1, 1, 1, 1, 1, 1), 'rep0_middle': (1, 1, 1, 0, 1, 1, 1),
              'rep0_last': (1, 1, 1, 1, 1, 1, 0), 'rep23': (2, 1, 3, 1, 2, 3, 1), 'rep23_big': (1, 3, 1, 2, 1, 1, 2)}
TABLE_CASES = [dict(name='%s_wd%g_t%d' % (v, wd, t0), reps=TABLE_REPS[v], wd=wd, start=t0) for v in TABLE_REPS for wd in (0.0, 1e-4)
               for t0 in (0, 1, 99999)]
EMA_TAUS = (0.999, 0.5)


@functools.lru_cache(maxsize=1)
def table_data():
    """per tensor (p, m, v, g1, g2): gradient magnitudes from 1e-12 to 1e3 (log-uniform, both signs), exact zeros of g where m = v = 0"""
    out = []
    for k, n in enumerate(TABLE_SIZES):
        rng = rng_of('table/%d' % k)
        mag = 10.0 ** rng.uniform(-12.0, 3.0, n)
        sign = lambda: np.where(rng.random(n) < 0.5, -1.0, 1.0)
        g1, g2 = (mag * sign() * rng.uniform(0.5, 2.0, n)).astype(F32), (mag * sign() * rng.uniform(0.5, 2.0, n)).astype(F32)
        p = rng.standard_normal(n).astype(F32)
        m, v = (0.1 * mag * rng.standard_normal(n)).astype(F32), ((0.3 * mag * rng.standard_normal(n)) ** 2).astype(F32)
        zero = rng.random(n) < 0.1 if n > 1 else np.zeros(n, bool)
        if n >= 32:
            zero[:3] = True
        g1[zero], m[zero], v[zero] = 0, 0, 0               # a fresh element with a zero gradient: v stays 0, the update divides 0 by eps
        for a in (p, m, v, g1, g2):
            a.setflags(write=False)
        out.append((p, m, v, g1, g2))
    return tuple(out)


def hyper_of(wd):
    return A.hyper32(HYPER['lr'], HYPER['b1'], HYPER['b2'], HYPER['eps'], wd)


def adam_checks(name, got, before, g, hyper, t, rep):
    """[(quantity, case, got, ref, scale)] of one launch's p, m, v against the float64 update of that launch's fp32 inputs"""
    ref, mag = A.adam_ref(*before, g, hyper, t, rep)
    return [('adam_' + q, name, got[j], ref[j], mag[j]) for j, q in enumerate('pmv')]


# ---- linear_wgrad ---------------------------------------------------------------------------------------------------------------------------
LIN_SHAPES = ((512, 512), (128, 128), (512, 32))           # (O, I)
LIN_ROWS = (1, 15, 16, 17, 512, 513, 33000)                # one row, the 16-row slice, the 512-row chunk, above 64 chunks (rchunk = 528)
LIN_KEYS = {100: (4, 0, 0), 101: (4, 0, 1), 110: (4, 1, 0), 111: (4, 1, 1), 0: (1, 0, 0), 10: (1, 1, 0)}        # key: (NT, GPRO, XPRO)
LIN_CASES = [dict(name='k%03d_o%d_i%d_r%d' % (key, O, I, R), key=key, O=O, I=I, R=R, gpro=gp, xpro=xp)
             for O, I in LIN_SHAPES for R in LIN_ROWS for key, (nt, gp, xp) in LIN_KEYS.items() if (nt == 1) == (I == 32)]
LIN_REFUSED = (dict(O=64, I=128, R=16), dict(O=128, I=64, R=16), dict(O=128, I=128, R=0), dict(O=128, I=32, R=16, xpro=1))


@functools.lru_cache(maxsize=1)
def linear_data(O, I, R):
    """G with a column offset (so that c1 = mean(G) is not small: a tail row fed through the transform would move db by gscale c1), the
    pre-BatchNorm hidden Gh, X, and the tables of both prologues from true batch statistics (fewer than 8 rows: of a 64-row batch)"""
    rng = rng_of('linear/%d/%d/%d' % (O, I, R))
    n = max(R, 64)
    col = rng.uniform(0.5, 2.0, O), rng.uniform(-1.0, 1.0, O)
    G = (rng.standard_normal((n, O)).astype(F32) * (1e-2 * col[0]).astype(F32) + (5e-3 * col[1]).astype(F32))
    Gh = (rng.standard_normal((n, O)).astype(F32) * col[0][::-1].astype(F32) + col[1][::-1].astype(F32))
    xc = rng.uniform(0.5, 2.0, I), rng.uniform(-1.0, 1.0, I)
    X = (rng.standard_normal((n, I)).astype(F32) * xc[0].astype(F32) + xc[1].astype(F32))
    gt = A.bn_backward_tables(G, Gh, rng.uniform(0.5, 1.5, O))
    xm, xv = X.mean(0, dtype=F64), X.var(0, dtype=F64)
    gam, bet = rng.uniform(0.5, 1.5, I), rng.uniform(-0.5, 0.5, I)
    xs = gam / np.sqrt(xv + 1e-5)
    d = dict(G=G[:R], Gh=Gh[:R], X=X[:R], gt=gt, xscale=xs.astype(F32), xshift=(bet - xm * xs).astype(F32))
    for a in list(d['gt'].values()) + [d[k] for k in ('G', 'Gh', 'X', 'xscale', 'xshift')]:
        a.setflags(write=False)
    return d


def linear_args(c, d):
    """the reference's / emulation's keyword arguments of a case"""
    kw = {}
    if c['gpro']:
        kw.update(Gh=d['Gh'], gt=d['gt'])
    if c['xpro']:
        kw.update(xscale=d['xscale'], xshift=d['xshift'])
    return kw


# ---- glinear_wgrad --------------------------------------------------------------------------------------------------------------------------
GLIN_CASES = [dict(name='i%d_o%d_r%d' % (I, O, R), I=I, O=O, R=R) for I, O in ((1, 1), (63, 65), (64, 64), (130, 70)) for R in (1, 15, 17, 1672)]
GLIN_PAD = (3, 5)                                          # ldx - I, ldg - O


def glinear_data(c):
    rng = rng_of('glinear/' + c['name'])
    return rng.standard_normal((c['R'], c['I'])).astype(F32), (1e-2 * rng.standard_normal((c['R'], c['O'])) + 1e-3).astype(F32)


# ---- the emulation's ratios -----------------------------------------------------------------------------------------------------------------
def measure(big=True):
    """[(op, case, {quantity: the emulation's ratio})]; big = False leaves out the 33,000-row cases at 128 and 512 columns (the CPU test's quick pass)"""
    rows = []
    for c in WGRAD32_CASES:
        if c['co_stride'] != 288 or not c['bias']:
            continue                                        # (the same arithmetic as the dense case of that map)
        x, gy, ref, mag = wgrad32_data(c['b'], c['h'], c['w'], c['bf16'])
        ew, eb = A.wgrad32_emu(x, gy)
        rows.append(('wgrad32', c['data'], dict(wgrad32_w=ratio(ew, ref[0], mag[0]), wgrad32_b=ratio(eb, ref[1], mag[1]))))
    for c in GW_CASES:
        x, gy, _, ref, mag = gwgrad_data(c['ci'], c['co'], c['b'], c['h'], c['w'])
        ew, eb = A.gwgrad_x3_emu(x, gy)
        rows.append(('gwgrad', c['name'], dict(gwgrad_w=ratio(ew, ref[0], mag[0]), gwgrad_b=ratio(eb, ref[1], mag[1]))))
    for c in FUSED_CASES:
        # the gradient of the GPU case is the kernel's own gw / gb; the emulation takes the float64 gradient rounded to fp32 in its place
        _, _, _, ref, _ = gwgrad_data(c['ci'], c['co'], c['b'], c['h'], c['w'])
        hy, r = hyper_of(FUSED_WD), {}
        for part, g in (('/w', ref[0]), ('/b', ref[1]))[:2 if c['bias'] else 1]:
            g = g.reshape(-1).astype(F32)
            state = adam_state(c['name'] + part, g.size, 0.3)
            emu = A.adam_emu(*state, g, hy, c['start'] + 1)
            for q, _, got, rf, mg in adam_checks(c['name'], emu, state, g, hy, c['start'] + 1, 1):
                r[q] = max(r.get(q, 0.0), ratio(got, rf, mg))
        rows.append(('fused', c['name'], r))
    tab = table_data()
    for c in TABLE_CASES:
        hy, r = hyper_of(c['wd']), {}
        for k, (p, m, v, g1, g2) in enumerate(tab):
            rep = c['reps'][k]
            if rep == 0:
                continue
            state = (p, m, v)
            for launch, g in enumerate((g1, g2)):
                t = c['start'] + 1 + launch
                emu = A.adam_emu(*state, g, hy, t, rep)
                for q, _, got, rf, mg in adam_checks(c['name'], emu, state, g, hy, t, rep):
                    r[q] = max(r.get(q, 0.0), ratio(got, rf, mg))
                state = emu
        rows.append(('adam', c['name'], r))
    for c in LIN_CASES:
        if not big and c['R'] > 1000 and c['I'] > 32:
            continue
        d = linear_data(c['O'], c['I'], c['R'])
        kw = linear_args(c, d)
        ref, mag = A.linear_wgrad_ref(d['G'], d['X'], **kw)
        ew, eb = A.linear_wgrad_emu(d['G'], d['X'], **kw)
        rows.append(('linear', c['name'], dict(lin_w=ratio(ew, ref[0], mag[0]), lin_b=ratio(eb, ref[1], mag[1]))))
    for c in GLIN_CASES:
        x, gy = glinear_data(c)
        ref, mag = A.linear_wgrad_ref(gy, x)
        ew, eb = A.glinear_wgrad_emu(x, gy)
        rows.append(('glinear', c['name'], dict(glin_w=ratio(ew, ref[0], mag[0]), glin_b=ratio(eb, ref[1], mag[1]))))
    return rows


def table(rows):
    """the text of tests/update_ratios.py"""
    out = ['"""The fp32 emulation\'s ratios |emulation - float64| / (2^-24 x scale) per operation, case and quantity: generated by',
           '`python -m tests.update_cases --table` (tests/update_cases.py measure()); a case\'s tolerance is 4 x its own ratio."""', 'RATIO = {']
    for op in dict.fromkeys(o for o, _, _ in rows):
        out.append('    %r: {' % op)
        out += ['        %r: {%s},' % (name, ', '.join('%r: %.4e' % (q, v) for q, v in r.items())) for o, name, r in rows if o == op]
        out.append('    },')
    return '\n'.join(out + ['}']) + '\n'


def report(gpu=None):
    """The generated part of profiles/update_elementwise.txt: per operation, case and quantity the emulation's ratio, the case's TOL = 4 x
    it, and the largest ratio a GPU run printed for that case (gpu = read_gpu_log(); information only, never a bound)."""
    big = {}
    for q, key, r in gpu or ():
        big[(q, key)] = max(big.get((q, key), 0.0), r)
    out = ['ratios |error| / (2^-24 x scale)', '', '%-8s %-24s %-10s %-14s %-12s %s' % ('op', 'case', 'quantity', 'CPU emulation', 'TOL = 4 x', 'GPU')]
    for op, cases in RATIO.items():
        for name, r in cases.items():
            for q, v in r.items():
                g = big.get((q, '%s/%s' % (op, name)))
                out.append('%-8s %-24s %-10s %-14.4e %-12.4e %s' % (op, name, q, v, 4 * v, '-' if g is None else '%.4e' % g))
    return '\n'.join(out) + '\n'


def read_gpu_log(path):
    """The 'update <quantity> <op>/<case>...: largest |error| / (2^-24 scale) <ratio>' lines tests/test_gpu_update_elementwise.py prints
    (pytest -s) -> [(quantity, 'op/case', ratio)]"""
    import re
    out = []
    for line in open(path):
        m = re.search(r'update (\w+) (\w+/\S+).*?: largest \|error\| / \(2\^-24 scale\) (\S+)', line)
        if m and m.group(1) in QUANTITIES:
            out.append((m.group(1), m.group(2), float(m.group(3))))
    return out


if __name__ == '__main__':
    import sys
    if sys.argv[1:] == ['--table']:
        print(table(measure()), end='')
    else:
        print(report(read_gpu_log(sys.argv[1]) if len(sys.argv) > 1 else None), end='')
