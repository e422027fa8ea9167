"""The cases of the per-element tests of CostDCNet's own kernels (tests/test_gpu_costdc_elementwise.py, tests/test_costdc_elementwise_cpu.py):
seeded inputs, float64 references (oracle/costdc_arith.py) and the bounds.

Exact operations are compared with array_equal.  For the arithmetic ones the bound of a quantity = TOL[quantity] x its magnitude, TOL = 4 x
the largest error ratio |emulation - float64| / magnitude of the CPU emulation over the cases below -- never a figure from a GPU run.
`python -m tests.costdc_cases` recomputes the ratios and prints the table kept in profiles/costdc_elementwise.txt; the CPU test checks
the constants against the recomputed ratios.

ReLU ties: the sparse BatchNorm's backward masks with y > 0, so make_sbn() moves every element whose float64 pre-activation lies within
TIE x its forward magnitude of zero away from it (through the residual when there is one, else through the element's own input, or
through beta where one or two voxels leave the input no freedom) and recomputes the reference until none is left; no element is excluded
anywhere."""
import zlib

import numpy as np

from oracle import costdc_arith as A

F32, F64 = np.float32, np.float64
TIE = 2.0 ** -18
# the largest ratios of profiles/costdc_elementwise.txt (python -m tests.costdc_cases)
RATIO = {'feat': 2.421e-08, 'conv': 2.604e-07, 'conv_bwd': 2.759e-07, 'sbn_y': 7.281e-08, 'sbn_st': 9.130e-08, 'sbn_rm': 1.181e-07, 'sbn_rv': 1.066e-07,
         'sbn_gx': 7.643e-08, 'sbn_dgamma': 1.871e-08, 'sbn_dbeta': 8.742e-09, 'norm': 4.398e-08, 'fusion_bwd': 1.094e-07, 'regress': 2.258e-07,
         'regress_bwd': 1.931e-07}
TOL = {q: 4.0 * r for q, r in RATIO.items()}
TOL_ACC = 2.0 ** -24          # a gradient buffer's second writer adds once in fp32: half an ulp of the sum, |sum| <= |g| + |previous|
QUANTITIES = tuple(RATIO)
NORM = (255.0, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- voxel levels ----------------------------------------------------------------------------------------------------------------
ZS_ODD = float(F32(7.3 / 16))
LEVEL_CASES = (
    [dict(name='w%d' % w, n=1, h=8, w=w, z=0.5, kind='random') for w in (4, 60, 64, 68, 132, 260)] +
    # (N H is a multiple of 4 because H is: 1020 / 1024 / 1028 rows straddle the scan's chunk of 1024, 2056 carries twice)
    [dict(name='rows%d' % (n * h), n=n, h=h, w=4, z=0.5, kind='random') for n, h in ((1, 1020), (1, 1024), (1, 1028), (2, 1028))] +
    [dict(name='l1rows1024', n=1, h=128, w=8, z=0.5, kind='random'), dict(name='l1rows1152', n=1, h=144, w=8, z=0.5, kind='random'),
     dict(name='empty_frame', n=2, h=8, w=68, z=0.5, kind='empty0'), dict(name='all_empty', n=1, h=8, w=12, z=0.5, kind='empty'),
     dict(name='halves', n=1, h=8, w=68, z=0.5, kind='halves'),
     dict(name='zs0625', n=1, h=12, w=68, z=0.625, kind='offhalf'), dict(name='zs_odd', n=2, h=12, w=132, z=ZS_ODD, kind='offhalf')])
HALVES = (0.25, 0.75, 1.25, 7.25, 7.75, -0.25, -3.0, 0.0, 8.0, 100.0, 7.5, 7.74, 0.2, 0.3)


def make_levels(c):
    """sparse [n][h][w] fp32"""
    rng = rng_of('levels/' + c['name'])
    n, h, w, zs = c['n'], c['h'], c['w'], F32(c['z'])
    if c['kind'] == 'empty':
        return np.zeros((n, h, w), F32)
    if c['kind'] == 'offhalf':                  # arbitrary depths at least 1e-3 planes from a half plane: fp32 and float64 choose the same plane
        d = rng.uniform(-0.6, 16.4, (n, h, w)) * float(zs)
        d = d.astype(F32)
        q = d.astype(F64) / float(zs)
        d[np.abs(q - np.floor(q) - 0.5) < 1e-3] = 0
    else:                                        # dyadic: plane + k / 64, every operation exact
        d = ((rng.integers(1, 16, (n, h, w)) + rng.integers(-28, 29, (n, h, w)) / 64.0) * float(zs)).astype(F32)
    d[rng.random((n, h, w)) > 0.4] = 0
    if c['kind'] == 'empty0':
        d[0] = 0
    if c['kind'] == 'halves':
        d[0, 3, :len(HALVES)] = HALVES
        d[0, 5, 30:30 + len(HALVES)] = HALVES[::-1]
    if h >= 8 and c['kind'] != 'empty0':         # a voxel on columns 0, 63, 64 and W - 1 of rows 1 and 6; row 2 empty; row 4 full
        for x in (0, 63, 64, w - 1):
            if x < w:
                d[:, 1, x] = 3.25 * float(zs)
                d[:, 6, x] = 9.25 * float(zs)
        d[:, 2] = 0
        d[:, 4] = np.where(d[:, 4] == 0, F32(2.125 * float(zs)), d[:, 4])
    return np.ascontiguousarray(d, F32)


# ---- sparse convolution ----------------------------------------------------------------------------------------------------------
# every (ksize, Ci, Co, lin, lout) costdc_engine::build_sparse() creates
CONV_FORMS = [(3, 1, 32, 0, 0), (3, 32, 32, 0, 0), (3, 32, 48, 0, 1), (3, 48, 48, 1, 1), (1, 32, 48, 0, 1), (3, 48, 64, 1, 2), (3, 64, 64, 2, 2),
              (1, 48, 64, 1, 2), (1, 64, 16, 2, 2)]
CONV_SET = dict(n=2, h=32, w=48, z=0.5)
CONV_BIG = dict(n=1, h=64, w=96, z=0.5)      # 6144 voxels on every pixel: the block-stride loop over 4096 blocks


def make_conv_set(big=False):
    """The sparse depth of the convolution cases.  Small: frame 0 holds a clump whose 2 x 2 pixel blocks carry planes 5, 6, 7 (level-1
    voxels of plane 6 inside it have all 27 neighbours), a flat patch on plane 3 (level 0: all 9 in-plane neighbours), one isolated voxel
    (no neighbour at any level), voxels of planes 1 and 15 on the frame's corners; frame 1 is random."""
    c = CONV_BIG if big else CONV_SET
    rng = rng_of('conv_set/%d' % big)
    n, h, w, zs = c['n'], c['h'], c['w'], c['z']
    frac = rng.integers(-28, 29, (n, h, w)) / 64.0
    if big:
        plane = rng.integers(1, 16, (n, h, w))
    else:
        plane = np.zeros((n, h, w), np.int64)
        yy, xx = np.mgrid[0:16, 0:24]
        plane[0, :16, :24] = 5 + ((yy & 1) * 2 + (xx & 1)) % 3
        plane[0, 16:24, :16] = 3
        plane[0, 26, 42] = 9
        plane[0, 0, 47], plane[0, 31, 0], plane[0, 31, 47], plane[0, 30, 47] = 1, 15, 15, 1
        plane[1] = np.where(rng.random((h, w)) < 0.3, rng.integers(1, 16, (h, w)), 0)
        plane[1, 0, 0], plane[1, 0, 1], plane[1, 1, 0], plane[1, 1, 1] = 1, 1, 15, 15
    return np.ascontiguousarray(np.where(plane > 0, (plane + frac) * zs, 0.0), F32)


def make_conv(form, cnt_in, cnt_out, backward=False):
    k, ci, co, lin, lout = form
    rng = rng_of('conv/%s/%d' % (form, backward))
    wk = (rng.standard_normal((k ** 3, ci, co)) * 0.2).astype(F32)
    x = rng.standard_normal((cnt_out, co) if backward else (cnt_in, ci)).astype(F32)
    prev = rng.standard_normal((cnt_in, ci)).astype(F32)
    return x, wk, prev


# ---- sparse BatchNorm ------------------------------------------------------------------------------------------------------------
SBN_SET = dict(n=1, h=16, w=20)               # the first `cnt` pixels hold a voxel
SBN_BIG = dict(n=1, h=96, w=96)               # 9216 voxels x 64 channels > 2048 x 256: the apply kernels' grid-stride loop


def _sbn(name, cnt, c, mode='tracked', relu=True, res=False, world=1, gres='none', big=False):
    return dict(name=name, cnt=cnt, c=c, mode=mode, relu=relu, res=res, world=world, gres=gres, big=big)


SBN_CASES = [
    _sbn('cnt0_c16', 0, 16), _sbn('cnt1_c32', 1, 32, res=True, gres='write'), _sbn('cnt2_c48', 2, 48), _sbn('cnt255_c64', 255, 64, res=True, gres='acc'),
    _sbn('cnt256_c16', 256, 16, res=True, gres='write'), _sbn('cnt257_c32', 257, 32), _sbn('cnt257_c48_res_acc', 257, 48, res=True, gres='acc'),
    _sbn('cnt257_c48_untracked_plain', 257, 48, mode='untracked', relu=False), _sbn('cnt257_c64_untracked_relu', 257, 64, mode='untracked'),
    _sbn('cnt255_c16_res_norelu', 255, 16, mode='untracked', relu=False, res=True, gres='write'),
    _sbn('cnt257_c64_eval_res', 257, 64, mode='eval', res=True), _sbn('cnt256_c32_eval_plain', 256, 32, mode='eval', relu=False),
    _sbn('cnt255_c32_world2', 255, 32, res=True, world=2, gres='write'), _sbn('cnt257_c16_world2_untracked', 257, 16, mode='untracked', world=2),
    _sbn('cnt1_c64_world2', 1, 64, world=2), _sbn('cnt0_c32_world2', 0, 32, world=2),
    _sbn('big_c64', 9216, 64, res=True, gres='acc', big=True),
]
SBN_BY_NAME = {c['name']: c for c in SBN_CASES}


def sbn_sparse(c):
    s = SBN_BIG if c['big'] else SBN_SET
    d = np.zeros(s['n'] * s['h'] * s['w'], F32)
    d[:c['cnt']] = 1.0
    return d.reshape(s['n'], s['h'], s['w']), 0.5


def make_sbn(c):
    rng = rng_of('sbn/' + c['name'])
    cnt, C = c['cnt'], c['c']
    f = (rng.standard_normal((cnt, C)) * rng.uniform(0.5, 2.0, C) + rng.uniform(-3.0, 3.0, C)).astype(F32)
    d = dict(f=f, gamma=rng.uniform(0.5, 1.5, C).astype(F32) * np.where(np.arange(C) % 5 == 0, -1, 1).astype(F32), beta=rng.uniform(-0.5, 0.5, C).astype(F32),
             res=rng.standard_normal((cnt, C)).astype(F32) if c['res'] else None, g=rng.standard_normal((cnt, C)).astype(F32),
             gres_prev=rng.standard_normal((cnt, C)).astype(F32) if c['gres'] == 'acc' else None, track=None)
    if c['mode'] in ('tracked', 'eval'):
        d['track'] = dict(rm=rng.uniform(-1.0, 1.0, C).astype(F32), rv=rng.uniform(0.5, 2.0, C).astype(F32), nbt=7, repeats=2)
    nudged = 0
    for _ in range(40):
        fw, mag = sbn_reference_fwd(c, d)
        s = fw['y'] if not c['relu'] else (fw['v'] + (0.0 if d['res'] is None else d['res'].reshape(fw['v'].shape)))
        tie = (np.abs(s) <= TIE * mag['y']).reshape(cnt, C) if c['relu'] else np.zeros((cnt, C), bool)
        if not tie.any():
            break
        step = (4.0 * TIE * mag['y'].reshape(cnt, C) * np.where(s.reshape(cnt, C) < 0, -1.0, 1.0))
        if d['res'] is not None:
            d['res'][tie] += step[tie].astype(F32)
        elif cnt <= 2:                           # (x - mean) scale is fixed by the normalisation: only beta moves the pre-activation
            ch = tie.any(0)
            d['beta'][ch] += np.where(tie, step, 0.0).sum(0)[ch].astype(F32)
        else:
            d['f'][tie] += (step / fw['scale'][0])[tie].astype(F32)
        nudged += int(tie.sum())
    else:
        raise AssertionError('ReLU ties left in ' + c['name'])
    d['nudged'] = nudged
    return d


def sbn_reference_fwd(c, d, fault=None):
    fw = A.sbn_forward_ref(d['f'], d['gamma'], d['beta'], train=c['mode'] != 'eval', relu=c['relu'], res=d['res'], track=d['track'], world=c['world'], fault=fault)
    return fw, A.sbn_forward_mags(d['f'], d['gamma'], d['beta'], fw, d['res'], d['track'] if c['mode'] == 'tracked' else None, c['world'])


def sbn_reference_bwd(c, d, fw, fmag, fault=None):
    bw = A.sbn_backward_ref(d['f'], d['g'], fw, d['gamma'], relu=c['relu'], res=d['res'], gres_prev=d['gres_prev'], fault=fault)
    return bw, A.sbn_backward_mags(d['f'], d['g'], fw, fmag, bw, d['gamma'], d['gres_prev'])


def sbn_emulation(c, d):
    fe = A.sbn_forward_emu(d['f'], d['gamma'], d['beta'], train=c['mode'] != 'eval', relu=c['relu'], res=d['res'], track=d['track'], world=c['world'])
    be = None
    if c['mode'] != 'eval':
        be = A.sbn_backward_emu(d['f'], fe['y'], d['g'], fe['st'], d['gamma'], relu=c['relu'], gres_prev=d['gres_prev'], world=c['world'])
    return fe, be


def ratio(got, ref, mag):
    """largest |got - ref| / mag (0 / 0 counts as 0; anything over a zero magnitude as inf)"""
    err = np.abs(np.asarray(got, F64) - ref)
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / mag)
    return float(r.max())


def sbn_ratios(c, fwd_got, bwd_got, ref):
    """fwd_got = dict(y, st[, rm, rv]); bwd_got = dict(gx, dgamma, dbeta) or None -> {quantity: ratio}"""
    fw, fmag, bw, bmag = ref
    out = {'sbn_y': ratio(fwd_got['y'], fw['y'], fmag['y']), 'sbn_st': ratio(fwd_got['st'], fw['st'], fmag['st'])}
    if c['mode'] == 'tracked':
        out['sbn_rm'], out['sbn_rv'] = ratio(fwd_got['rm'], fw['rm'], fmag['rm']), ratio(fwd_got['rv'], fw['rv'], fmag['rv'])
    if bwd_got is not None:
        for q in ('gx', 'dgamma', 'dbeta'):
            out['sbn_' + q] = ratio(bwd_got[q], bw[q], bmag[q])
    return out


# ---- dense kernels ---------------------------------------------------------------------------------------------------------------
POOL_CASES = [dict(name='%dx%d_c%d_acc%d' % (h, w, ch, acc), items=4, h=h, w=w, c=ch, acc=acc)
              for (h, w), ch, acc in zip(((4, 4), (5, 7), (10, 14), (20, 28)), (32, 48, 64, 32), (0, 1, 0, 1))]
POOL_CASES.append(dict(name='grid_cap', items=120, h=20, w=28, c=64, acc=0))           # 4.3 M gradient elements > 16384 x 256


def make_pool(c):
    """Post-ReLU input with planted ties: windows (output pixel) 0: all equal, 1: positions 0 and 7 tie for the maximum, 2: a tie across
    the plane pair (positions 1 and 5), 3: all zeros; and the zeros the ReLU leaves everywhere else.  gy: distinct integers."""
    rng = rng_of('pool/' + c['name'])
    I, H, W, C = c['items'], c['h'], c['w'], c['c']
    x = np.maximum(rng.standard_normal((I, H, W, C)), 0).astype(F32)
    Wo = W // 2
    for io in range(I // 2):
        for k, (yo, xo) in enumerate([(j // Wo, j % Wo) for j in range(min(4, (H // 2) * Wo))]):
            win = x[2 * io:2 * io + 2, 2 * yo:2 * yo + 2, 2 * xo:2 * xo + 2]
            if k == 0:
                win[:] = 1.5
            elif k == 1:
                win[:] = np.minimum(win, 1.0)
                win[0, 0, 0] = win[1, 1, 1] = 2.0
            elif k == 2:
                win[:] = np.minimum(win, 1.0)
                win[0, 0, 1] = win[1, 0, 1] = 2.5
            else:
                win[:] = 0
    Ho = H // 2
    gy = (rng.permutation(I // 2 * Ho * Wo * C) + 1).astype(F32).reshape(I // 2, Ho, Wo, C)
    prev = rng.integers(-1000, 1000, (I, H, W, C)).astype(F32)
    return x, gy, prev


UP_CASES = [dict(name='%s_to_%s_c%d_acc%d' % ('x'.join(map(str, i)), 'x'.join(map(str, o)), ch, acc), frames=2, i=i, o=o, c=ch, acc=acc)
            for i, o, ch, acc in (((2, 2, 3), (4, 5, 7), 80, 0), ((4, 5, 7), (8, 10, 14), 64, 1), ((8, 10, 14), (16, 20, 28), 48, 0),
                                  ((2, 4, 6), (4, 8, 12), 80, 1))]


def make_up(c):
    rng = rng_of('up/' + c['name'])
    x = rng.standard_normal((c['frames'],) + c['i'] + (c['c'],)).astype(F32)
    n = c['frames'] * int(np.prod(c['o'])) * c['c']
    gy = (rng.permutation(n) + 1).astype(F32).reshape((c['frames'],) + c['o'] + (c['c'],))          # all distinct; sums of <= 27 stay below 2^24
    prev = rng.integers(-1000, 1000, x.shape).astype(F32)
    return x, gy, prev


REGRESS_CASES = [dict(name='3x5', n=2, h=3, w=5, z=8.0 / 15), dict(name='1x7', n=1, h=1, w=7, z=0.5)]


def make_regress(c):
    """Costs spread over +-30 (the maximum's subtraction matters), distinct per channel; pixel 0's column 0 is all equal."""
    rng = rng_of('regress/' + c['name'])
    cost = rng.uniform(-30.0, 30.0, (c['n'], 16, c['h'], c['w'], 16)).astype(F32)
    cost[0, :, 0, 0, 0] = 1.25
    cost[0, :, 0, 0, 5] += 3.0 * np.arange(16, dtype=F32)                  # a sharp column
    cost[0, :, 0, 1, :] *= 0.05                                            # a flat pixel: every plane carries weight
    gpred = rng.standard_normal((c['n'], 4 * c['h'], 4 * c['w'])).astype(F32)
    return cost, gpred


ROWS_CASES = [dict(name='d2_c80', n=2, d=2, h=3, w=5, c=80, acc=0), dict(name='d3_c20', n=1, d=3, h=2, w=7, c=20, acc=1)]
FUSION_CASES = [dict(name='p1', n=2, passes=1, h=3, w=5), dict(name='p2', n=1, passes=2, h=5, w=3)]


def make_fusion(c):
    """Pixels with 0, 1 and 2 occupied planes; one voxel whose 16 features are all exactly 0 (it counts as empty); one feature -0.0."""
    rng = rng_of('fusion/' + c['name'])
    N, P, h, w = c['n'], c['passes'], c['h'], c['w']
    feat2d = rng.standard_normal((P * N, h, w, 16)).astype(F32)
    feat3d = np.zeros((N, 16, h, w, 16), F32)
    for n in range(N):
        for y in range(h):
            for x in range(w):
                k = (y * w + x + n) % 3
                for z in rng.choice(16, k, replace=False):
                    feat3d[n, z, y, x] = rng.standard_normal(16)
    feat3d[0, 4, 0, 0] = 0                       # an occupied-looking cell of zeros beside ...
    feat3d[0, 9, 0, 0, 3] = -0.0
    feat3d[0, 11, 1, 1] = 0
    feat3d[0, 11, 1, 1, 15] = 1e-30              # ... one with a single tiny feature
    gvol = rng.standard_normal((N, 16, h, w, 32)).astype(F32)
    return feat2d, feat3d, gvol


PAD_CASES = [dict(name='pt_only', n=2, h=24, w=32, pt=8, pr=0), dict(name='pr_only', n=2, h=16, w=20, pt=0, pr=12),
             dict(name='both', n=2, h=9, w=13, pt=7, pr=3)]


def make_pad(c):
    rng = rng_of('pad/' + c['name'])
    n, h, w = c['n'], c['h'], c['w']
    Hp, Wp = h + c['pt'], w + c['pr']
    image = np.floor(rng.uniform(0, 256, (n, 3, h, w))).astype(F32)
    image[image == 0] = 1.0                      # (so that a normalised in-frame pixel is never the padding's zero)
    sparse = np.where(rng.random((n, h, w)) < 0.3, rng.uniform(0.2, 9.0, (n, h, w)), 0).astype(F32)
    net = rng.standard_normal((2 * n, Hp, Wp)).astype(F32)
    g = rng.standard_normal((n, h, w)).astype(F32)
    return image, sparse, net, g, Hp, Wp


# ---- the emulation's ratios --------------------------------------------------------------------------------------------------------
def conv_geometry(big=False):
    c = CONV_BIG if big else CONV_SET
    sparse = make_conv_set(big)
    coords, feat, fmag = A.levels_ref(sparse, c['z'])
    return sparse, coords, (c['n'], c['h'], c['w'])


def measure():
    """[(op, case, {quantity: the emulation's ratio})]"""
    rows = []
    for c in LEVEL_CASES:
        sp = make_levels(c)
        coords, f, mag = A.levels_ref(sp, c['z'])
        c0 = coords[0]
        emu = A.feature_emu(sp[c0[:, 0], c0[:, 2], c0[:, 3]], c0[:, 1], c['z'])
        rows.append(('levels', c['name'], {'feat': ratio(emu, f, mag)}))
    for big in (False, True):
        sparse, coords, shape = conv_geometry(big)
        for form in (CONV_FORMS[:1] if big else CONV_FORMS):
            k, ci, co, lin, lout = form
            pairs = A.conv_pairs(coords[lin], coords[lout], shape, lin, lout, k)
            x, wk, _ = make_conv(form, len(coords[lin]), len(coords[lout]))
            ref, mag = A.sparse_conv_ref(x, wk, pairs, len(coords[lout]))
            r = {'conv': ratio(A.sparse_conv_emu(x, wk, pairs, len(coords[lout])), ref, mag)}
            gy, wk, prev = make_conv(form, len(coords[lin]), len(coords[lout]), True)
            for acc in (0, 1):
                ref, mag = A.sparse_conv_bwd_ref(gy, wk, pairs, len(coords[lin]), prev if acc else None)
                r['conv_bwd'] = max(r.get('conv_bwd', 0.0), ratio(A.sparse_conv_bwd_emu(gy, wk, pairs, len(coords[lin]), prev if acc else None), ref, mag))
            rows.append(('conv' + ('_big' if big else ''), str(form), r))
    for c in SBN_CASES:
        d = make_sbn(c)
        fw, fmag = sbn_reference_fwd(c, d)
        bw, bmag = sbn_reference_bwd(c, d, fw, fmag)
        fe, be = sbn_emulation(c, d)
        rows.append(('sbn', c['name'], sbn_ratios(c, fe, be, (fw, fmag, bw, bmag))))
    for c in PAD_CASES:
        image, sparse, net, g, Hp, Wp = make_pad(c)
        ref, emu, mag = A.pad_dual_ref(image, Hp, Wp, c['pt'], c['pr'], NORM)
        r2, e2, m2 = A.stage_ref(image, sparse, 2, 16, NORM)
        rows.append(('pad / stage', c['name'], {'norm': max(ratio(emu, ref, mag), ratio(e2, r2, m2))}))
    for c in FUSION_CASES:
        feat2d, feat3d, gvol = make_fusion(c)
        _, mask = A.fusion_fwd_ref(feat2d, feat3d, c['passes'])
        ref, emu, mag = A.fusion_bwd_ref(gvol, mask)
        rows.append(('fusion', c['name'], {'fusion_bwd': ratio(emu, ref, mag)}))
    for c in REGRESS_CASES:
        cost, gpred = make_regress(c)
        ref, emu, mag = A.regress_fwd_ref(cost, c['z'])
        rb, eb, mb = A.regress_bwd_ref(cost, gpred, c['z'])
        rows.append(('regress', c['name'], {'regress': ratio(emu, ref, mag), 'regress_bwd': ratio(eb, rb, mb)}))
    return rows


def worst(rows):
    out = {q: 0.0 for q in QUANTITIES}
    for _, _, r in rows:
        for q, v in r.items():
            out[q] = max(out[q], v)
    return out


def report(rows, gpu=None):
    """The generated part of profiles/costdc_elementwise.txt: the emulation's ratios, TOL = 4 x, and next to each the largest ratio of a GPU
    run (gpu = [(quantity, case, ratio)] read from the test's printed lines; information only)."""
    w = worst(rows)
    big = lambda q: max((r for qq, _, r in gpu or () if qq == q), default=None)
    out = ['quantity      CPU emulation   TOL = 4 x    largest on the GPU (information only, never a bound)']
    for q in QUANTITIES:
        out.append('%-13s %-15.3e %-12.3e %s' % (q, w[q], 4 * w[q], '-' if big(q) is None else '%.3e' % big(q)))
    out += ['', 'Per case, CPU emulation:', '']
    for op, name, r in rows:
        out.append('%-12s %-32s %s' % (op, name, '  '.join('%s %.3e' % (q, v) for q, v in r.items())))
    if gpu:
        out += ['', 'Per comparison, GPU:', ''] + ['%-13s %-44s %.3e' % g for g in gpu]
    return '\n'.join(out) + '\n'


def read_gpu_log(path):
    """The 'costdc <quantity> <case>: largest |error| / magnitude <ratio>' lines tests/test_gpu_costdc_elementwise.py prints (pytest -s)."""
    import re
    out = []
    for line in open(path):
        m = re.search(r'costdc (\w+) (.*?): largest \|error\| / magnitude (\S+)', line)
        if m and m.group(1) in QUANTITIES:
            out.append((m.group(1), m.group(2), float(m.group(3))))
    return out


if __name__ == '__main__':
    import sys
    print(report(measure(), read_gpu_log(sys.argv[1]) if len(sys.argv) > 1 else None), end='')
