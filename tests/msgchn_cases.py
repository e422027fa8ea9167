"""The cases of the per-element tests of the MSG_CHN step's first-layer / prediction convolutions, resamplings and loss
(tests/test_gpu_msgchn_elementwise.py, tests/test_msgchn_elementwise_cpu.py): seeded inputs, float64 references (oracle/msgchn_arith.py)
and the bounds.

Bounds.  Exact operations (the clamp, sign-bit words, ReLU masks, untouched pixels, zero-input frames with a bias-only epilogue, gradients
that must be zero) are compared with array_equal.  For arithmetic the bound of an element is

    (TOL[quantity] + EXTRA[quantity] * 2^-23) x its magnitude   (+ half a bf16 ulp for a narrow output)

* TOL = 4 x the largest |float32 emulation - float64| / magnitude over the cases below (`python -m tests.msgchn_cases` recomputes the
  ratios and prints the table kept in profiles/msgchn_elementwise.txt; the CPU test checks the constants) -- never a figure from a GPU run.
* EXTRA counts the device-library results that enter the quantity as factors and that numpy computes differently.  The HIP math API's
  accuracy table (ROCm documentation, "HIP math API", single-precision functions) gives expf and sqrtf a maximum error of 1 ulp = 2^-23
  relative; the emulation uses numpy's exp and correctly rounded sqrt, so each such factor adds 2^-23 of the magnitude:
    loss_sm 1, gdepth 1   one expf per edge weight (the magnitude already carries the weight's conditioning 1 + m)
    rowstats 2            |e| and |ref| one sqrtf each; the cosine divides by both
    loss_cos 2            the mean of 2 - 2 cos
    loss_total 3          its smoothness and cosine terms
    gref 4                coef (e / |e| - cos ref / |ref|) / |ref|: 1 / |e|, cos (two), 1 / |ref| once more outside
    loss_sd, coef 0       sums, one division
  fp32 division itself is correctly rounded in this build: hipcc's -fhip-fp32-correctly-rounded-divide-sqrt is on by default (clang's
  HIP option reference) and csrc/Makefile does not turn it off, so the emulation's IEEE division is the device's and adds nothing.
* The loss's four scalars and the gradient coefficients (STORED) are double-precision results stored once as fp32: the store rounds by at
  most half an fp32 ulp, 2^-24 |ref|, added to their bound.  The emulation makes the same store, but over the cases it draws that
  rounding a dozen times per quantity, not thousands: the format's own bound stands in for the sample.
* Narrow (bf16) outputs are the fp32 result rounded once to 8 significant bits: the error of that rounding is at most half the bf16
  spacing at the value, 2^(floor(log2 |v|) - 8), which lies between 2^-9 |v| (just below a power of two) and 2^-8 |v| (just above one).
  2^-9 |ref| alone cannot hold for a correctly rounded result (1.003 rounds to 1.0, an error of 2^-8.4), so the bound adds the spacing
  itself, taken at |ref| + the fp32 bound (oracle/msgchn_arith.py bf16_half_ulp).  Narrow INPUTS are bf16-representable: their conversion is exact.

Every element is compared; none is excluded.  Ties of the loss's sign functions are exact in fp32 (the difference of two fp32 values has the
exact sign), so no pixel needs a margin; the cosine gate is a condition on the inputs: every case keeps the float64 l_cos at least 1e-3 from 0.3."""
import zlib

import numpy as np

from oracle import msgchn_arith as A

F32, F64 = np.float32, np.float64
# the largest ratios of profiles/msgchn_elementwise.txt (python -m tests.msgchn_cases)
RATIO = {'conv_in': 2.877e-07, 'conv_out1': 1.613e-07, 'pool': 1.359e-07, 'up2': 6.511e-08, 'up2t': 4.057e-08, 'up2t32': 5.343e-08,
         'loss_total': 7.680e-09, 'loss_sm': 5.966e-09, 'loss_sd': 7.695e-09, 'loss_cos': 1.120e-08, 'rowstats': 1.491e-07, 'coef': 5.914e-08,
         'gdepth': 1.307e-07, 'gref': 3.546e-07}
TOL = {q: 4.0 * r for q, r in RATIO.items()}
EXTRA = {'loss_sm': 1, 'gdepth': 1, 'rowstats': 2, 'loss_cos': 2, 'loss_total': 3, 'gref': 4}
QUANTITIES = tuple(RATIO)
STORED = ('loss_total', 'loss_sm', 'loss_sd', 'loss_cos', 'coef')
NORM = (255.0, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
INFO_Q = ('loss_total', 'loss_sm', 'loss_sd', 'loss_cos')
GATE_MARGIN = 1e-3


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def tol(q):
    return TOL[q] + EXTRA.get(q, 0) * 2.0 ** -23


def bound(q, mag, ref=None, narrow=False):
    b = tol(q) * np.asarray(mag, F64)
    if q in STORED:
        b = b + 2.0 ** -24 * np.abs(np.asarray(ref, F64))
    return b + A.bf16_half_ulp(np.abs(ref) + b) if narrow else b


def ratio(got, ref, mag):
    """largest |got - ref| / mag (0 / 0 counts as 0; anything over a zero magnitude as inf)"""
    err = np.abs(np.asarray(got, F64) - ref)
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / mag)
    return float(r.max())


def _maps(rng, shape, narrow, scale=1.0):
    a = (rng.standard_normal(shape) * scale).astype(F32)
    return A.bf16_round(a) if narrow else a


def _weight(rng, shape):
    """asymmetric in (out, in, ky, kx): a different ramp along every axis on top of the noise"""
    w = rng.standard_normal(shape) * 0.3
    for ax, n in enumerate(shape):
        sh = [1] * len(shape)
        sh[ax] = n
        w = w + (np.arange(n).reshape(sh) - 0.37 * n) * 0.05 * (ax + 1)
    return w.astype(F32)


# ---- the first-layer convolution -----------------------------------------------------------------------------------------------------------
def _ci(name, b, h, w, cin, nbs, **kw):
    c = dict(name=name, b=b, h=h, w=w, cin=cin, nbs=nbs, cin_total=cin, cin_first=0, flip=False, norm=False, zero_from_b=1 << 30, bias=True, up=0,
             mask=None, add1=0, a_bits_nb=0, want='raw', dtypes=('fp32', 'mixed'), caps=(0,), form='lds')
    c.update(kw)
    return c


CONV_IN_CASES = [
    _ci('8x32_c3_norm', 2, 8, 32, 3, (2, 2, 2), norm=True),                                       # one exact tile; padding of a normalised plane
    _ci('16x70_c2_zero', 3, 16, 70, 2, (1, 3), zero_from_b=1, a_bits_nb=2, caps=(0, 1, 2)),          # ragged 6-pixel tile, b % nb broadcast, zero word
    _ci('19x33_c1_first1_mask', 3, 19, 33, 1, (3,), cin_total=2, cin_first=1, mask='float', dtypes=('fp32',), caps=(0, 1, 2), form='lds_mask'),
    _ci('19x33_flip_bits', 3, 19, 33, 1, (3,), flip=True, bias=False, mask='bits', caps=(0, 2), form='lds_mask'),      # the 32 -> 1 layer's input gradient
    _ci('3x5_c3_both', 2, 3, 5, 3, (2, 1, 2), norm=True, mask='both', dtypes=('fp32',), zero_from_b=1, form='lds_mask'),
    _ci('16x70_c1_up_add', 3, 16, 70, 1, (3,), up=3, add1=1, mask='float', want='both', dtypes=('fp32',), caps=(0, 1, 2), form='direct'),
    _ci('16x70_c2_up_add_narrow', 3, 16, 70, 2, (3, 1), up=1, add1=3, want='both', dtypes=('mixed',), caps=(0, 2), form='direct'),
    _ci('8x32_c2_sum_only', 2, 8, 32, 2, (2, 2), add1=2, want='sum', zero_from_b=1, form='direct'),
    _ci('19x33_c3_sum_only_lds', 1, 19, 33, 3, (1, 1, 1), want='sum', dtypes=('fp32',)),
]


def make_conv_in(c, dtype='fp32'):
    rng = rng_of('conv_in/' + c['name'])
    nar = dtype != 'fp32'
    b, h, w, cin = c['b'], c['h'], c['w'], c['cin']
    d = dict(weight=_weight(rng, (1, 32, 3, 3) if c['flip'] else (32, c['cin_total'], 3, 3)), bias=_weight(rng, (32,)) if c['bias'] else None)
    planes = []
    for k, nb in enumerate(c['nbs']):
        if c['norm']:                                  # an image plane: 1 .. 255, never the 0 whose normalised value the padding must not show
            planes.append((np.floor(rng.uniform(1, 256, (nb, h, w))).astype(F32), (NORM[0], NORM[1][k], NORM[2][k])))
        else:
            planes.append((rng.standard_normal((nb, h, w)).astype(F32) * F32(2), None))
    d['planes'] = planes
    d['up'] = _maps(rng, (c['up'], h // 2, w // 2, 32), nar) if c['up'] else None
    d['add1'] = _maps(rng, (c['add1'], h, w, 32), nar) if c['add1'] else None
    d['mask'] = rng.standard_normal((b, h, w, 32)).astype(F32) if c['mask'] else None
    if d['mask'] is not None:
        d['mask'][:, 0, 0] = (0.0, -0.0) * 16            # zeros of both signs are not > 0
    d['w_eff'] = A.conv_in_weight(d['weight'], cin, c['cin_first'], c['flip'])
    return d


def conv_in_kwargs(c, d):
    return dict(planes=d['planes'], w_eff=d['w_eff'], B=c['b'], zero_from_b=c['zero_from_b'], bias=d['bias'], up=d['up'], mask=d['mask'], add1=d['add1'])


# ---- the prediction convolution ------------------------------------------------------------------------------------------------------------
def _co(name, b, h, w, in_nb, **kw):
    c = dict(name=name, b=b, h=h, w=w, in_nb=in_nb, relu=True, add_nb=0, bias=True, from_conv_in=False, dtypes=('fp32', 'mixed'), caps=(0,))
    c.update(kw)
    return c


CONV_OUT1_CASES = [
    _co('8x32', 2, 8, 32, 2),
    _co('16x70_add', 3, 16, 70, 3, add_nb=1, caps=(0, 1, 2)),
    _co('19x33_norelu_nobias', 3, 19, 33, 1, relu=False, bias=False, add_nb=3, caps=(0, 1, 2)),
    _co('3x5', 1, 3, 5, 1, relu=False),
    _co('16x70_from_conv_in', 3, 16, 70, 3, relu=False, bias=False, add_nb=3, from_conv_in=True, caps=(0, 2)),      # the first layer's gradient wrt plane 1
]


def make_conv_out1(c, dtype='fp32'):
    rng = rng_of('conv_out1/' + c['name'])
    d = dict(x=_maps(rng, (c['in_nb'], c['h'], c['w'], 32), dtype != 'fp32'), weight=_weight(rng, (32, 2, 3, 3) if c['from_conv_in'] else (1, 32, 3, 3)),
             bias=_weight(rng, (1,)) + F32(0.7) if c['bias'] else None, add=rng.standard_normal((c['add_nb'], c['h'], c['w'])).astype(F32) if c['add_nb'] else None)
    d['w_eff'] = A.conv_out1_weight(d['weight'], 1, c['from_conv_in'])
    return d


def conv_out1_kwargs(c, d):
    return dict(x=d['x'], w_eff=d['w_eff'], B=c['b'], bias=d['bias'], add=d['add'], relu_in=c['relu'])


# ---- resampling ------------------------------------------------------------------------------------------------------------------------------
UP_SIZES = [(1, 1), (1, 7), (2, 3), (3, 2), (5, 40), (11, 152)]
UP_B = 2


def make_up(hin, win, narrow=False):
    """x [B][hin][win], g [B][2 hin][2 win], their 32-channel forms and the addend"""
    rng = rng_of('up/%dx%d/%d' % (hin, win, narrow))
    return dict(x=rng.standard_normal((UP_B, hin, win)).astype(F32), g=rng.standard_normal((UP_B, 2 * hin, 2 * win)).astype(F32),
                g32=_maps(rng, (UP_B, 2 * hin, 2 * win, 32), narrow), add32=_maps(rng, (UP_B, hin, win, 32), narrow))


PREP_CASES = [dict(name='%dx%d_max%g' % (h, w, m), n=2, h=h, w=w, max_d=m) for (h, w), m in zip(((4, 4), (8, 12), (12, 20), (8, 12)), (5.0, 5.0, 5.0, -1.0))]


def make_prep(c):
    """a third of the points valid, some above the clamp, some negative; the first 4 x 4 block (and one 2 x 2 block elsewhere) without any"""
    rng = rng_of('prep/' + c['name'])
    s = np.where(rng.random((c['n'], c['h'], c['w'])) < 0.35, rng.uniform(0.2, 9.0, (c['n'], c['h'], c['w'])), 0.0)
    s = np.where(rng.random(s.shape) < 0.1, -rng.uniform(0.1, 3.0, s.shape), s).astype(F32)
    s[:, :4, :4] = 0
    s[:, -2:, -2:] = 0
    s[0, 3, 3] = -1.5                                    # a negative value inside the empty block: clamped to 0, or kept (and not > 0) without the clamp
    return s


# ---- the loss ----------------------------------------------------------------------------------------------------------------------------------
def _lc(name, n, h, w, r, d, **kw):
    c = dict(name=name, n=n, h=h, w=w, r=r, d=d, validity='derived', max_d=5.0, gate='open', w3=(1.0, 2.0, 0.1), narrow=False)
    c.update(kw)
    return c


LOSS_CASES = [
    _lc('n1_8x12_r5', 1, 8, 12, 5, 512),
    _lc('n3_8x12_r37_d8_closed', 3, 8, 12, 37, 8, gate='closed', validity='given', narrow=True),
    _lc('n2_260x256_r4100', 2, 260, 256, 4100, 512, validity='given'),
    _lc('n16_8x12_r5', 16, 8, 12, 5, 512, max_d=-1.0),
    _lc('n17_8x12_r5', 17, 8, 12, 5, 512, narrow=True),
    _lc('n3_8x12_r5_negative', 3, 8, 12, 5, 512, validity=None),
]
LOSS_BY_NAME = {c['name']: c for c in LOSS_CASES}


def make_loss(c):
    """depth, image [N][3][H][W] in [0, 4), sparse (a third valid, some above the clamp; with validity None some negative: the weight is then
    the value itself), validity (given: differs from the derived one), emb / ref [R][D] bf16-representable.  Planted: exact ties
    depth == clamp(sparse) on valid pixels, equal neighbours along both axes, an all-zero row of ref (row 1) and of emb (row 2).
    gate 'open': ref = a rotation of emb far enough for l_cos >> 0.3; 'closed': ref close to emb, l_cos << 0.3."""
    rng = rng_of('loss/' + c['name'])
    n, h, w, r, dm = c['n'], c['h'], c['w'], c['r'], c['d']
    depth = rng.uniform(0.5, 8.0, (n, h, w)).astype(F32)
    image = rng.uniform(0.0, 4.0, (n, 3, h, w)).astype(F32)
    valid = rng.random((n, h, w)) < 0.35
    sparse = np.where(valid, rng.uniform(0.3, 7.0, (n, h, w)), 0.0).astype(F32)
    if c['validity'] is None:
        neg = rng.random((n, h, w)) < 0.05
        sparse = np.where(neg, -rng.uniform(0.01, 0.2, (n, h, w)), sparse).astype(F32)
    validity = None
    if c['validity'] == 'given':
        validity = (valid & (rng.random((n, h, w)) < 0.8)).astype(F32)
        validity[:, 0, 0] = 1.0
        sparse[:, 0, 0] = np.maximum(sparse[:, 0, 0], F32(1.0))
    sparse[:, 1, 1] = 2.5                                # valid under every rule ...
    if validity is not None:
        validity[:, 1, 1] = 1.0
    cs = A.clamp_ref(sparse, c['max_d'])
    depth[:, 1, 1] = cs[:, 1, 1]                         # ... and an exact tie with the depth
    depth[:, 2, 3:6] = depth[:, 2, 3:4]                  # equal neighbours along x
    depth[:, 3:6, 7] = depth[:, 3:4, 7]                  # and along y
    depth[:, h - 1, w - 2:] = depth[:, h - 1, w - 2:w - 1]      # in the last row, up to the last column
    depth[:, 4:7, 1:4] = depth[:, 4:5, 1:2]              # a 3 x 3 plateau without a valid point: its centre's gradient is exactly zero
    sparse[:, 4:7, 1:4] = 0
    if validity is not None:
        validity[:, 4:7, 1:4] = 0
    emb = rng.standard_normal((r, dm)).astype(F32)
    if c['gate'] == 'open':
        ref = (0.3 * emb + rng.standard_normal((r, dm))).astype(F32)
    else:
        ref = (emb + 0.1 * rng.standard_normal((r, dm))).astype(F32)
    emb, ref = A.bf16_round(emb), A.bf16_round(ref)
    if r > 2:
        ref[1] = 0
        emb[2] = 0
    return dict(depth=depth, image=image, sparse=sparse, validity=validity, emb=emb, ref=ref)


def loss_args(c, d, cos=True):
    return dict(image=d['image'], depth=d['depth'], sparse=d['sparse'], validity=d['validity'], emb=d['emb'] if cos else None, ref=d['ref'] if cos else None,
                w3=c['w3'], max_d=c['max_d'])


def loss_ratios(got, ref):
    out = {}
    for k, q in enumerate(INFO_Q):
        if ref['mag_info'][k] > 0:
            out[q] = ratio(got['info'][k], ref['info'][k], ref['mag_info'][k])
    for q in ('rowstats', 'coef', 'gdepth', 'gref'):
        if q in got and q in ref:
            out[q] = ratio(got[q], ref[q], ref['mag_' + q])
    return out


# ---- the emulation's ratios ------------------------------------------------------------------------------------------------------------------
def measure():
    """[(op, case, {quantity: the emulation's ratio})] -- fp32 storage everywhere: a narrow launch adds one exactly bounded rounding"""
    rows = []
    for c in CONV_IN_CASES:
        d = make_conv_in(c)
        ref, emu = A.conv_in_ref(**conv_in_kwargs(c, d)), A.conv_in_emu(**conv_in_kwargs(c, d))
        rows.append(('conv_in', c['name'], {'conv_in': max(ratio(emu['raw'], ref['raw'], ref['mag_raw']), ratio(emu['sum'], ref['sum'], ref['mag_sum']))}))
    for c in CONV_OUT1_CASES:
        d = make_conv_out1(c)
        ref, mag = A.conv_out1_ref(**conv_out1_kwargs(c, d))
        rows.append(('conv_out1', c['name'], {'conv_out1': ratio(A.conv_out1_emu(**conv_out1_kwargs(c, d)), ref, mag)}))
    for c in PREP_CASES:
        s = make_prep(c)
        _, ref = A.prep_ref(s, c['max_d'])
        _, emu = A.prep_emu(s, c['max_d'])
        rows.append(('prep', c['name'], {'pool': max(ratio(emu[k], *ref[k]) for k in (2, 4))}))
    for hin, win in UP_SIZES:
        d = make_up(hin, win)
        r = {'up2': ratio(A.up2_emu(d['x']), *A.up2_ref(d['x'])), 'up2t': ratio(A.up2t_emu(d['g'], False), *A.up2t_ref(d['g']))}
        r['up2t32'] = max(ratio(A.up2t_emu(d['g32'], True), *A.up2t_ref(d['g32'])), ratio(A.up2t_emu(d['g32'], True, d['add32']), *A.up2t_ref(d['g32'], d['add32'])))
        rows.append(('up', '%dx%d' % (hin, win), r))
    for c in LOSS_CASES:
        d = make_loss(c)
        for cos in (True, False):
            rows.append(('loss', c['name'] + ('' if cos else ' nocos'), loss_ratios(A.loss_emu(**loss_args(c, d, cos)), A.loss_ref(**loss_args(c, d, cos)))))
    return rows


def worst(rows):
    out = {q: 0.0 for q in QUANTITIES}
    for _, _, r in rows:
        for q, v in r.items():
            out[q] = max(out[q], v)
    return out


def report(rows, gpu=None):
    """The generated part of profiles/msgchn_elementwise.txt: the emulation's ratios, TOL = 4 x, the device-library allowance, and next to
    each the largest ratio of a GPU run (gpu = [(quantity, case, ratio)] read from the test's printed lines; information only)."""
    w = worst(rows)
    # (fp32 storage only: a narrow comparison's ratio is its bf16 rounding, 2^-9 .. 2^-8 of the value, and is listed per comparison)
    big = lambda q: max((r for qq, name, r in gpu or () if qq == q and ' mixed' not in name), default=None)
    out = ['quantity      CPU emulation   TOL = 4 x    + EXTRA x 2^-23   largest on the GPU (information only, never a bound)']
    for q in QUANTITIES:
        out.append('%-13s %-15.3e %-12.3e %-17d %s' % (q, w[q], 4 * w[q], EXTRA.get(q, 0), '-' if big(q) is None else '%.3e' % big(q)))
    out += ['', 'Per case, CPU emulation:', '']
    for op, name, r in rows:
        out.append('%-10s %-34s %s' % (op, name, '  '.join('%s %.3e' % (q, v) for q, v in r.items())))
    if gpu:
        out += ['', 'Per comparison, GPU:', ''] + ['%-13s %-52s %.3e' % g for g in gpu]
    return '\n'.join(out) + '\n'


def read_gpu_log(path):
    """The 'msgchn <quantity> <case>: largest |error| / magnitude <ratio>' lines tests/test_gpu_msgchn_elementwise.py prints (pytest -s)."""
    import re
    out = []
    for line in open(path):
        m = re.search(r'msgchn (\w+) (.*?): largest \|error\| / magnitude (\S+)', line)
        if m and m.group(1) in QUANTITIES:
            out.append((m.group(1), m.group(2), float(m.group(3))))
    return out


if __name__ == '__main__':
    import sys
    print(report(measure(), read_gpu_log(sys.argv[1]) if len(sys.argv) > 1 else None), end='')
