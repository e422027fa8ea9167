"""The cases of tests/test_gpu_gbn_elementwise.py and tests/test_gbn_elementwise_cpu.py: one BatchNorm of the generic engine
(csrc/gbn.hip) per case, each the smallest shape that reaches the branch it names; their seeded inputs, references, bounds and tolerances.

bound of a quantity = TOL[quantity] x its magnitude (oracle/gbn_arith.py), TOL = 4 x the largest error ratio |emulation - float64| /
magnitude of the CPU emulation over the cases below -- never a figure from a GPU run.  `python -m tests.gbn_cases` recomputes the ratios
and prints the table kept in profiles/gbn_elementwise.txt; the CPU test checks the constants against the recomputed ratios.

Mask ties.  The backward of ReLU / LeakyReLU is discontinuous where the pre-activation is zero, so make() nudges x (the residual for the
outer ReLU of a residual block) and iterates on the float64 reference until no element of pass 0 has its float64 pre-activation, inner or
outer, within TIE x its own forward magnitude of zero.  TIE = 2^-18 is fixed; the CPU test asserts TOL['y'] <= TIE (the margin is at
least the forward bound) and that no case has an ambiguous element, so no element is left out of any comparison."""
import zlib

import numpy as np

from oracle import gbn_arith as A

EPS = 1e-5
TIE = 2.0 ** -18
QUANTITIES = ('y', 'mean', 'inv', 'rm', 'rv', 'gx', 'dgamma', 'dbeta')
# the largest ratios of profiles/gbn_elementwise.txt (python -m tests.gbn_cases)
RATIO = {'y': 6.277e-08, 'mean': 7.665e-08, 'inv': 1.237e-07, 'rm': 5.097e-08, 'rv': 8.800e-08, 'gx': 8.937e-08, 'dgamma': 5.014e-08,
         'dbeta': 1.055e-07}
TOL = {q: 4.0 * r for q, r in RATIO.items()}
# a gradient buffer's second writer adds once in fp32: half an ulp of the sum, |sum| <= |g| + |previous| (no emulation needed)
TOL_GRES_ACC = 2.0 ** -24
# SyncBatchNorm statistics against the one-rank run: the expand stores the fp64 sum as fp32 hi + lo (2^-48), or hi alone in a
# single-block BatchNorm (2^-24 on each sum); 2^-23 relative to the statistic's magnitude is what that rounding allows
TOL_WORLD_STAT = 2.0 ** -23
# the `views` cases: channels of the sentinel-filled buffer before and after each tensor's slice.  Every offset is a multiple of 4 and the
# six row strides C + before + after are pairwise different, so a kernel that indexed one tensor with another's ld fails
VIEW_PADS = {'x': (8, 4), 'res': (4, 12), 'y': (12, 8), 'g': (16, 8), 'gx': (4, 4), 'gres': (8, 20)}


def C(name, b, h, w, c, npass=1, act='none', res=False, act_first=False, res_relu=True, acc_gx=False, acc_gres=False, frozen=False,
      views=False, nblocks=0, track=False, repeats=1, world=1, data='randn', big=False, note=''):
    return dict(name=name, b=b, h=h, w=w, c=c, npass=npass, act=act, res=res, act_first=act_first, res_relu=res_relu, acc_gx=acc_gx,
                acc_gres=acc_gres, frozen=frozen, views=views, nblocks=nblocks, track=track, repeats=repeats, world=world, data=data,
                big=big, note=note)


CASES = [
    # ---- channel-count geometry: CT = min(C, 256), nsub = 256 / CT, a channel-block loop above 256 ----
    C('c4_nsub64', 1, 10, 15, 4, act='relu'),                                   # 64 pixel sub-slots per block, 3 blocks, threads without a pixel
    C('c48_nsub5_idle16', 1, 5, 7, 48, act='relu'),                             # NLSPN 2layers width: 5 sub-slots, 16 threads of 256 idle
    C('c64', 1, 3, 11, 64, act='lrelu'),
    C('c256_nsub1', 1, 3, 11, 256, act='relu'),
    C('c320_partial_block', 1, 3, 5, 320, act='relu'),                          # second channel block 64 of 256 wide: the c < C guard
    C('c512', 1, 3, 5, 512, act='relu'),
    C('c1024_rows', 1, 37, 1, 1024, act='relu'),                                # the heads' BatchNorm1d(1024): H*W is the row count
    # ---- pixels per pass R ----
    C('r1', 1, 1, 1, 64, act='relu'),                                           # var = 0 in every channel
    C('r2_b2_1x1', 2, 1, 1, 64, act='relu'),
    C('r8_c512_last_map', 1, 2, 4, 512, act='relu', res=True),                  # the 2 x 4 last map of a 32 x 64 frame, a BasicBlock's bn2
    C('r7_below_nsub', 1, 1, 7, 4, act='lrelu'),                                # odd, one block, 57 sub-slots without a pixel
    C('r3072_c256_unroll0', 1, 48, 64, 256, act='relu'),                        # pstride 1024: 3 pixels per thread, the unrolled loop never runs
    C('r3073_c256_unroll1', 1, 7, 439, 256, act='relu'),                        # 3 * pstride + 1: thread 0 alone runs it once
    C('r3074_c256_unroll1', 1, 58, 53, 256, act='relu'),                        # ... threads 0 and 1
    C('r4097_c256_unroll1_tail', 1, 17, 241, 256, act='relu'),                  # once, then one tail pixel for thread 0
    C('r12288_c64_unroll0', 1, 96, 128, 64, act='relu'),                        # nsub 4, grid capped at 1024 blocks: pstride 4096
    C('r12289_c64_unroll1', 1, 1, 12289, 64, act='relu'),
    C('r16385_c64_unroll1_tail', 1, 145, 113, 64, act='lrelu'),                 # R not a multiple of pstride, capped grid
    C('apply_grid_stride', 1, 1024, 2052, 8, act='relu', big=True),             # 4,202,496 float4 > 16384 * 256: the apply kernels' second trip
    # ---- passes: [real | proxy] with very different statistics; the backward belongs to pass 0 ----
    C('npass2_proxy_zero', 2, 5, 7, 64, npass=2, act='relu', data='proxy0'),
    C('npass2_proxy_zero_res', 4, 3, 5, 48, npass=2, res=True, data='proxy0'),
    C('npass2_random', 2, 5, 7, 16, npass=2, act='lrelu'),
    C('npass2_proxy_zero_act_first', 2, 5, 7, 16, npass=2, act='relu', res=True, act_first=True, data='proxy0'),   # the inner mask from pass 0's affine
    # ---- conditioning: channels with mean / std 0, 1, 16, 256, a constant channel and one with var << eps ----
    C('cond_none', 1, 9, 33, 8, data='cond'),
    C('cond_elu', 1, 9, 33, 8, act='elu', data='cond'),
    C('cond_relu', 1, 9, 33, 8, act='relu', data='cond'),
    C('cond_npass2_lrelu', 2, 9, 17, 8, npass=2, act='lrelu', data='cond'),
    # ---- switches ----
    C('act_none', 1, 5, 7, 16),
    C('act_relu_yless', 1, 5, 7, 16, act='relu'),                               # the mask recomputed from fma(x, scale, shift)
    C('act_relu_act_first_no_res', 1, 5, 7, 16, act='relu', act_first=True),    # the same function through the saved output (not YLESS)
    C('act_lrelu', 1, 5, 7, 16, act='lrelu'),
    C('act_elu', 1, 5, 7, 16, act='elu'),
    C('res_basicblock', 1, 5, 7, 16, res=True),                                 # relu(bn(x) + res), NLSPN BasicBlock
    C('res_act_first', 1, 5, 7, 16, act='relu', res=True, act_first=True),      # relu(relu(bn(x)) + res), CostDCNet ResBlock
    C('res_no_relu', 1, 5, 7, 16, res=True, res_relu=False),                    # bn(x) + res, Res_Conv of the 2layers block
    C('res_acc_gx', 1, 5, 7, 16, res=True, acc_gx=True),
    C('res_acc_gres', 1, 5, 7, 16, res=True, acc_gres=True),
    C('res_acc_both', 1, 5, 7, 16, act='relu', res=True, act_first=True, acc_gx=True, acc_gres=True),
    C('acc_gx_no_res', 1, 5, 7, 16, act='lrelu', acc_gx=True),
    C('frozen', 1, 5, 7, 16, act='relu', frozen=True),                          # dgamma and dbeta NULL
    C('frozen_res', 1, 5, 7, 16, res=True, frozen=True),
    # ---- views: channel slices of wider sentinel-filled buffers, another ld and offset per tensor ----
    C('views_res', 2, 5, 7, 24, npass=2, res=True, views=True, acc_gres=True),
    C('views_act_first', 1, 3, 11, 8, act='relu', res=True, act_first=True, views=True, acc_gx=True),
    C('views_yless', 1, 5, 7, 48, act='relu', views=True),
    # ---- caller-made partials (a convolution epilogue's): both loops of gbn_sum_partials_block ----
    C('part_1', 1, 59, 61, 8, nblocks=1),
    C('part_2', 1, 59, 61, 8, nblocks=2),
    C('part_255', 1, 59, 61, 8, nblocks=255),
    C('part_257', 1, 59, 61, 8, nblocks=257),
    C('part_1023', 1, 59, 61, 8, nblocks=1023),
    C('part_1793', 1, 59, 61, 8, nblocks=1024 + 769),                           # the four-load loop twice for thread 0
    C('part_3344_npass2', 2, 59, 61, 8, npass=2, act='relu', nblocks=3344),     # the tile count of a full-resolution layer
    # ---- tracked BatchNorm: running statistics chained over npass x repeats updates ----
    C('track_p1_r1', 1, 5, 7, 16, act='relu', track=True),
    C('track_p1_r2', 1, 5, 7, 16, act='relu', track=True, repeats=2),
    C('track_p2_r1', 2, 5, 7, 16, npass=2, act='relu', track=True),
    C('track_p2_r2', 2, 5, 7, 16, npass=2, act='relu', track=True, repeats=2, data='proxy0'),
    C('track_res_act_first', 2, 5, 7, 16, npass=2, act='relu', res=True, act_first=True, track=True),      # ... and an eval forward with a residual
    C('track_res_basicblock', 1, 5, 7, 16, res=True, track=True, views=True),
    # ---- SyncBatchNorm on world = 2 ranks that hold the same data ----
    C('world2_c48_res', 2, 5, 7, 48, npass=2, res=True, world=2),
    C('world2_c320_track', 1, 3, 5, 320, act='relu', world=2, track=True),
    C('world2_single_block', 1, 1, 3, 64, act='lrelu', world=2),                # one block: the correction term has no block to live in
]
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the one-rank twin of every world = 2 case (same name, same data)
TWIN = {c['name']: dict(c, world=1) for c in CASES if c['world'] > 1}

COND_RATIOS = (0.0, 1.0, 16.0, 256.0, 'const', 'tiny', -16.0, 1.0)       # mean / std per channel of a 'cond' case


def pixels(c):
    return c['b'] // c['npass'] * c['h'] * c['w']


def geometry(c):
    return A.geometry(c['c'], pixels(c))


def fwd_kwargs(c, d):
    return dict(npass=c['npass'], act=c['act'], res=d['res'], act_first=c['act_first'], res_relu=c['res_relu'], track=d['track'],
                world=c['world'])


def bwd_kwargs(c, d):
    return dict(npass=c['npass'], act=c['act'], act_first=c['act_first'], res_relu=c['res_relu'], gx_prev=d['gx_prev'],
                gres_prev=d['gres_prev'], world=c['world'])


def ambiguous(c, d, fw=None, mag=None):
    """(inner, outer) boolean maps over pass 0: the elements whose float64 pre-activation lies within TIE x its forward magnitude of a
    point where the backward is discontinuous."""
    fw = fw or A.forward_ref(d['x'], d['gamma'], d['beta'], EPS, **fwd_kwargs(c, d))
    mag = mag or A.forward_mags(d['x'], d['gamma'], d['beta'], fw, c['npass'], d['res'])
    n0 = c['b'] // c['npass']
    v, mv, my = fw['v'][:n0], mag['v'][:n0], mag['y'][:n0]
    none = np.zeros(v.shape, bool)
    if not c['res']:
        return (np.abs(v) <= TIE * mv) if c['act'] in ('relu', 'lrelu') else none, none
    if not c['res_relu']:
        return none, none
    inner = (np.abs(v) <= TIE * mv) if c['act_first'] else none
    s = (A.act_fn(v, c['act']) if c['act_first'] else v) + d['res'][:n0].astype(np.float64)
    return inner, np.abs(s) <= TIE * my


def make(c):
    """Seeded fp32 inputs of a case: x, res, g, gamma, beta, gx_prev, gres_prev, track, parts -- and `nudged`, the elements moved off
    a mask tie."""
    rng = np.random.default_rng(zlib.crc32(c['name'].encode()))
    b, h, w, ch, npass = c['b'], c['h'], c['w'], c['c'], c['npass']
    n0 = b // npass
    f = np.float32
    sign = lambda n: np.where(rng.random(n) < 0.5, -1.0, 1.0)
    gamma = (sign(ch) * rng.uniform(0.5, 1.5, ch)).astype(f)
    beta = (sign(ch) * rng.uniform(0.25, 1.0, ch)).astype(f)
    if c['data'] == 'cond':
        assert ch == len(COND_RATIOS)
        x = rng.standard_normal((b, h, w, ch))
        for k, r in enumerate(COND_RATIOS):
            if r == 'const':
                x[..., k] = 0.5
            elif r == 'tiny':
                x[..., k] = 0.5 + 1e-4 * x[..., k]            # var = 1e-8 << eps
            else:
                x[..., k] += r
        x = x.astype(f)
    else:
        x = (rng.standard_normal((b, h, w, ch)) * rng.uniform(0.5, 2.0, ch) + rng.uniform(-1.0, 1.0, ch)).astype(f)
        if c['data'] == 'proxy0':
            x[n0:] = 0.0                                       # the proxy image: constant zero
    d = dict(x=x, gamma=gamma, beta=beta, res=None, gx_prev=None, gres_prev=None, track=None, parts=None)
    if c['res']:
        d['res'] = rng.standard_normal((b, h, w, ch)).astype(f)
    d['g'] = rng.standard_normal((n0, h, w, ch)).astype(f)
    if c['acc_gx']:
        d['gx_prev'] = rng.standard_normal((n0, h, w, ch)).astype(f)
    if c['acc_gres']:
        d['gres_prev'] = rng.standard_normal((n0, h, w, ch)).astype(f)
    if c['track']:
        d['track'] = dict(rm=rng.uniform(-1.0, 1.0, ch).astype(f), rv=rng.uniform(0.5, 2.0, ch).astype(f), momentum=0.1, repeats=c['repeats'],
                          nbt=7)
    nudged = 0
    for _ in range(60):
        fw = A.forward_ref(x, gamma, beta, EPS, **fwd_kwargs(c, d))
        mag = A.forward_mags(x, gamma, beta, fw, npass, d['res'])
        inner, outer = ambiguous(c, d, fw, mag)
        if not inner.any() and not outer.any():
            break
        v = fw['v'][:n0]
        if inner.any():                                        # move x so that |v| grows by 4 margins
            step = 4.0 * TIE * mag['v'][:n0] / np.abs(fw['scale'][0]) * np.where(v < 0, -1.0, 1.0) * np.sign(fw['scale'][0])
            x[:n0][inner] += step[inner].astype(f)
            nudged += int(inner.sum())
        if outer.any():
            s = (A.act_fn(v, c['act']) if c['act_first'] else v) + d['res'][:n0]
            d['res'][:n0][outer] += (4.0 * TIE * mag['y'][:n0] * np.where(s < 0, -1.0, 1.0))[outer].astype(f)
            nudged += int(outer.sum())
    d['nudged'] = nudged
    if c['nblocks']:
        d['parts'] = np.stack([A.split_partials(xp, c['nblocks']) for xp in x.reshape(npass, -1, ch)])
    return d


def reference(c, d, fault=None, drop=None):
    """float64 forward, backward and the magnitudes: (fw, fmag, bw, bmag)."""
    fw = A.forward_ref(d['x'], d['gamma'], d['beta'], EPS, fault=fault, drop=drop, **fwd_kwargs(c, d))
    fmag = A.forward_mags(d['x'], d['gamma'], d['beta'], fw, c['npass'], d['res'], d['track'], c['world'])
    bw = A.backward_ref(d['x'], d['g'], fw, d['gamma'], res=d['res'], fault=fault, drop=drop, **bwd_kwargs(c, d))
    bmag = A.backward_mags(d['x'], d['g'], fw, fmag, bw, d['gamma'], c['npass'], c['act'], d['gx_prev'], d['gres_prev'])
    return fw, fmag, bw, bmag


def emulation(c, d):
    fe = A.forward_emu(d['x'], d['gamma'], d['beta'], EPS, parts=d['parts'], **fwd_kwargs(c, d))
    be = A.backward_emu(d['x'], d['g'], fe['y'], fe['st'], d['gamma'], has_res=c['res'], **bwd_kwargs(c, d))
    return fe, be


def ratios(got, ref):
    """Largest |got - reference| / magnitude per quantity; got = dict(y, mean, inv, rm, rv, gx, dgamma, dbeta) (absent ones skipped)."""
    fw, fmag, bw, bmag = ref
    out = {}
    for q, (r, m) in dict(y=(fw['y'], fmag['y']), mean=(fw['mean'], fmag['mean']), inv=(fw['inv'], fmag['inv']),
                          rm=(fw.get('rm'), fmag.get('rm')), rv=(fw.get('rv'), fmag.get('rv')), gx=(bw['gx'], bmag['gx']),
                          dgamma=(bw['dgamma'], bmag['dgamma']), dbeta=(bw['dbeta'], bmag['dbeta'])).items():
        if got.get(q) is None or r is None:
            continue
        out[q] = float((np.abs(np.asarray(got[q], np.float64) - r) / np.maximum(m, 1e-300)).max())
    return out


def emu_quantities(fe, be):
    return dict(y=fe['y'], mean=fe['st'][0], inv=fe['st'][1], rm=fe.get('rm'), rv=fe.get('rv'), gx=be['gx'], dgamma=be['dgamma'],
                dbeta=be['dbeta'])


def measure(cases):
    """[(case name, {quantity: the emulation's ratio}, nudged elements, ambiguous elements)]"""
    rows = []
    for c in cases:
        d = make(c)
        ref = reference(c, d)
        inner, outer = ambiguous(c, d, ref[0], ref[1])
        rows.append((c['name'], ratios(emu_quantities(*emulation(c, d)), ref), d['nudged'], int(inner.sum() + outer.sum())))
    return rows


def worst(rows):
    out = {}
    for _, r, _, _ in rows:
        for q, v in r.items():
            out[q] = max(out.get(q, 0.0), v)
    return out


def table(rows):
    lines = ['%-28s %s  nudged' % ('case', ' '.join('%-9s' % q for q in QUANTITIES))]
    for name, r, nudged, amb in rows:
        assert amb == 0, name
        lines.append('%-28s %s  %d' % (name, ' '.join(('%-9.3e' % r[q]) if q in r else '%-9s' % '-' for q in QUANTITIES), nudged))
    lines.append('')
    for q, v in sorted(worst(rows).items(), key=lambda kv: QUANTITIES.index(kv[0])):
        lines.append('%-7s largest ratio %.3e  -> TOL = 4 x = %.3e' % (q, v, 4 * v))
    return '\n'.join(lines)


NOTES_MARK = '---- notes (kept as written; everything above this line is generated) ----'


def gpu_ratios(log):
    """{case: {quantity: ratio}} from the `GBN_RATIOS` lines tests/test_gpu_gbn_elementwise.py prints (pytest -s)."""
    out = {}
    for line in open(log):
        if 'GBN_RATIOS' in line:
            f = line[line.index('GBN_RATIOS'):].split()
            out[f[1]] = {k: float(v) for k, v in (kv.split('=') for kv in f[2:])}
    return out


def profile_text(rows, gpu):
    """The generated part of profiles/gbn_elementwise.txt: the emulation's ratios, TOL, and the GPU's next to them (information only)."""
    w, extra = worst(rows), ('gres', 'eval_y')
    big = lambda q: max((v[q] for v in gpu.values() if q in v), default=None)
    fmt = lambda v: '-' if v is None else '%.3e' % v
    out = ["Per-element tests of the generic engine's BatchNorm (tests/test_gpu_gbn_elementwise.py): error ratios",
           'ratio = largest |result - float64| / magnitude (oracle/gbn_arith.py) over the cases of tests/gbn_cases.py',
           'written by `python -m tests.gbn_cases --gpu-log LOG --write profiles/gbn_elementwise.txt`, LOG = the output of',
           '`pytest tests/test_gpu_gbn_elementwise.py -m gpu -s` on an MI355X (%d of %d cases in the log)' % (len(gpu), len(CASES)), '',
           'quantity   CPU emulation   TOL = 4 x    largest on the GPU (information only, never a bound)']
    for q in QUANTITIES:
        out.append('%-10s %-15.3e %-12.3e %s' % (q, w[q], 4 * w[q], fmt(big(q))))
    out += ['gres, accumulated (bound 2^-24 (|g| + |previous|): one fp32 addition)      %s' % fmt(big('gres')),
            'eval y from the updated running statistics (TOL = largest of y, rm, rv)   %s' % fmt(big('eval_y')), '',
            'Per case, CPU emulation:', '', table(rows), '', 'Per case, GPU:', '',
            '%-28s %s' % ('case', ' '.join('%-9s' % q for q in QUANTITIES + extra))]
    for name, v in gpu.items():
        out.append('%-28s %s' % (name, ' '.join('%-9s' % fmt(v.get(q)) for q in QUANTITIES + extra)))
    return '\n'.join(out) + '\n'


if __name__ == '__main__':
    import argparse
    import os
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--gpu-log', help='output of pytest -s tests/test_gpu_gbn_elementwise.py: adds the GPU ratios')
    ap.add_argument('--write', help='rewrite the generated part of this profile file, keeping its notes')
    args = ap.parse_args()
    rows = measure(CASES)
    if not args.write:
        print(profile_text(rows, gpu_ratios(args.gpu_log)) if args.gpu_log else table(rows))
    else:
        old = open(args.write).read() if os.path.exists(args.write) else ''
        notes = old[old.index(NOTES_MARK):] if NOTES_MARK in old else NOTES_MARK + '\n'
        open(args.write, 'w').write(profile_text(rows, gpu_ratios(args.gpu_log) if args.gpu_log else {}) + '\n' + notes)
