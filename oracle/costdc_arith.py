"""CostDCNet's own kernels (csrc/costdc_kernels.hip) on the CPU (test infrastructure): plain numpy references of every operation, float64
where there is arithmetic, an fp32 emulation of the kernels' own order where a bound is needed, the magnitudes the per-element bounds
scale with, and planted wrong arithmetics (`fault=`) that the tests must reject.  Nothing from the library takes part.

Layouts as the kernels have them: voxel features [voxels][channels]; coordinates (frame, plane, y, x) with y, x multiples of the tensor
stride 1 << level; dense volumes NDHWC.  The selection operations (levels, pooling, nearest upsampling, rows, densify, padding) are exact;
sums of a single pair (crop, an accumulated gradient) are the exactly rounded fp32 result.

Semantics of the sparse operations: oracle/minkowski_lite.py (the MinkowskiEngine stand-in, parity unpinned)."""
import numpy as np

from oracle import gbn_arith as GA

F32, F64 = np.float32, np.float64
PLANES = 16
SBN_BLOCKS = 256
SBN_EPS = 1e-5
FAULTS = ('round_half_away', 'keep_plane0', 'clamp16', 'scan_no_carry', 'popc_off_by_one', 'reversed_offsets', 'stride_ts_out',
          'downsample_offgrid', 'transposed_no_ongrid', 'biased_running_var', 'one_running_update', 'mask_pre_residual', 'gres_overwritten',
          'last_max', 'pool_odd_last_row', 'nearest_ceil', 'up_window_narrow', 'shuffle_4j_i', 'rows_d_major', 'fusion_no_plus_one',
          'pad_corners_swapped', 'crop_not_halved')


def fma32(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


# ---- voxel levels ----------------------------------------------------------------------------------------------------------------
def plane_of(d, z_step, fault=None):
    """clip(rint(d / z_step), 0, 15) with the division in fp32 (the choice is discontinuous: the kernel's own operand decides it)."""
    q = np.asarray(d, F32) / F32(z_step)
    r = np.where(q < 0, -np.floor(-q + F32(0.5)), np.floor(q + F32(0.5))) if fault == 'round_half_away' else np.rint(q)
    return np.clip(r, 0, 16 if fault == 'clamp16' else 15).astype(np.int64)


def feature_ref(d, plane, z_step):
    """(d - plane * z_step) / z_step in float64 of the fp32 operands, and the magnitude its fp32 evaluation's error scales with."""
    d, zs = np.asarray(d, F32).astype(F64), float(F32(z_step))
    f = (d - plane * zs) / zs
    return f, (np.abs(d) + np.abs(plane * zs)) / zs + np.abs(f)


def feature_emu(d, plane, z_step):
    d, zs = np.asarray(d, F32), F32(z_step)
    return (d - plane.astype(F32) * zs) / zs


def levels_ref(sparse, z_step, fault=None):
    """sparse [N][H][W] -> [coords of level 0, 1, 2], each int64 [cnt][4] = (frame, plane, y, x) in the order the kernels number them
    (level 0 by (frame, row, column), the coarser levels by (frame, plane, row, column)), and the level-0 feature (float64) with its
    magnitude."""
    z = plane_of(sparse, z_step, fault)
    keep = np.ones_like(z, bool) if fault == 'keep_plane0' else z != 0
    n, y, x = np.nonzero(keep)                                          # row-major: (frame, row, column)
    c0 = np.stack([n, z[n, y, x], y, x], 1)
    f, mag = feature_ref(sparse[n, y, x], c0[:, 1], z_step)
    out = [c0]
    for l in (1, 2):
        ts = 1 << l
        q = c0.copy()
        q[:, 2:] = (q[:, 2:] // ts) * ts
        out.append(np.unique(q, axis=0))                                # lexicographic = (frame, plane, row, column)
    return out, f, mag


def _number(occ, fault):
    """Ids of a [rows][W] occupancy in the kernels' order: row count, exclusive scan in chunks of 1024 rows, rank inside the row from
    ballots over 64 columns.  -> (ids [rows][W] with -1 where empty, total)."""
    rows, W = occ.shape
    cnt = occ.sum(1)
    off = np.cumsum(cnt) - cnt
    total = int(cnt.sum())
    if fault == 'scan_no_carry':
        start = (np.arange(rows) // 1024) * 1024
        off = off - off[start]
        total = int(cnt[(rows - 1) // 1024 * 1024:].sum())
    rank = np.cumsum(occ, 1) - 1
    if fault == 'popc_off_by_one':                                       # mask (1 << (lane + 1)) - 1: every lane counts itself
        rank = rank + 1
    return np.where(occ, off[:, None] + rank, -1), total


def levels_emu(sparse, z_step, fault=None):
    """What the kernels leave behind: [(cnt, coords [cap][4] (rows past cnt unwritten = -9), vol [N][16][H >> l][W >> l])] per level, feat_in."""
    N, H, W = sparse.shape
    cap = N * H * W
    z = plane_of(sparse, z_step, fault)
    occ = np.ones_like(z, bool) if fault == 'keep_plane0' else z != 0
    ids, total = _number(occ.reshape(N * H, W), fault if fault in ('scan_no_carry', 'popc_off_by_one') else None)
    ids = ids.reshape(N, H, W)
    n, y, x = np.nonzero(occ)
    zz = np.minimum(z[n, y, x], 15)                                      # (a plane 16 of the planted clamp would leave the volume)
    coords = np.full((cap + 1, 4), -9, np.int64)
    vol = np.full((N, PLANES, H, W), -1, np.int64)
    feat = np.zeros(cap + 1, F32)
    i = np.minimum(ids[n, y, x], cap)
    coords[i] = np.stack([n, z[n, y, x], y, x], 1)
    feat[i] = feature_emu(sparse[n, y, x], z[n, y, x], z_step)
    vol[n, zz, y, x] = ids[n, y, x]
    levels = [(total, coords[:cap], vol)]
    for l in (1, 2):
        Hc, Wc = H >> l, W >> l
        pc, pcoords = levels[-1][0], levels[-1][1]
        src = pcoords[:min(pc, cap)]
        src = src[src[:, 0] >= 0]
        occ = np.zeros((N, PLANES, Hc, Wc), bool)
        occ[src[:, 0], np.minimum(src[:, 1], 15), src[:, 2] >> l, src[:, 3] >> l] = True
        ids, total = _number(occ.reshape(-1, Wc), fault if fault in ('scan_no_carry', 'popc_off_by_one') else None)
        ids = ids.reshape(N, PLANES, Hc, Wc)
        n, zc, y, x = np.nonzero(occ)
        coords = np.full((cap + 1, 4), -9, np.int64)
        coords[np.minimum(ids[n, zc, y, x], cap)] = np.stack([n, zc, y << l, x << l], 1)
        levels.append((total, coords[:cap], ids))
    return levels, feat[:cap]


def check_levels(levels, sparse, z_step):
    """The sets and the invariants the kernels promise, for a result in the form of levels_emu / CdSparseSet.read: raises AssertionError
    naming the level and what failed."""
    ref, _, _ = levels_ref(sparse, z_step)
    for l, (cnt, coords, vol) in enumerate(levels):
        want = ref[l]
        assert cnt == len(want), 'level %d: %d voxels, reference %d' % (l, cnt, len(want))
        got = np.asarray(coords[:cnt], np.int64)
        as_set = lambda a: a[np.lexsort(a.T[::-1])] if len(a) else a.reshape(0, 4)
        assert np.array_equal(as_set(got), as_set(want)), 'level %d: the coordinate set differs from the reference' % l
        assert not (vol == -2).any(), 'level %d: a marked cell was never numbered' % l
        assert ((vol >= -1) & (vol < cnt)).all(), 'level %d: an id outside -1 .. cnt - 1' % l
        ids = np.sort(vol[vol >= 0])
        assert np.array_equal(ids, np.arange(cnt)), 'level %d: ids are not exactly 0 .. cnt - 1' % l
        if cnt:
            assert np.array_equal(vol[got[:, 0], got[:, 1], got[:, 2] >> l, got[:, 3] >> l], np.arange(cnt)), 'level %d: vol[coords[id]] != id' % l
        filled = np.where(vol >= 0, vol, np.iinfo(np.int64).min)
        run = np.maximum.accumulate(filled, -1)
        assert not ((vol[..., 1:] >= 0) & (vol[..., 1:] <= run[..., :-1])).any(), 'level %d: ids do not increase along a row' % l
        assert np.array_equal(got, want), 'level %d: the numbering is not in the order the kernel file states' % l


# ---- sparse convolution ----------------------------------------------------------------------------------------------------------
def kernel_offsets(ksize, fault=None):
    """[(dz, dy, dx)] by kernel index: the plane axis fastest, k = (dz + 1) + 3 (dy + 1) + 9 (dx + 1)."""
    if ksize == 1:
        return [(0, 0, 0)]
    r = (-1, 0, 1)
    if fault == 'reversed_offsets':
        return [(dz, dy, dx) for dz in r for dy in r for dx in r]
    return [(dz, dy, dx) for dx in r for dy in r for dz in r]


def index_volume(coords, N, H, W, level):
    vol = np.full((N, PLANES, H >> level, W >> level), -1, np.int64)
    vol[coords[:, 0], coords[:, 1], coords[:, 2] >> level, coords[:, 3] >> level] = np.arange(len(coords))
    return vol


def conv_pairs(cin, cout, shape, lin, lout, ksize, fault=None):
    """[(k, output rows u, input rows j)]: output voxel u reads input voxel j = u + off_k * ts_in with kernel element k."""
    N, H, W = shape
    vol = index_volume(cin, N, H, W, lin)
    ts = 1 << (lout if (fault == 'stride_ts_out' and ksize == 3) else lin)
    pairs = []
    if fault == 'downsample_offgrid' and ksize == 1 and lout > lin:      # every input of the output's cell, not only the one on its corner
        tso = 1 << lout
        key = lambda c: ((c[:, 0] * PLANES + c[:, 1]) * H + c[:, 2] // tso * tso) * W + c[:, 3] // tso * tso
        lut = {int(k): u for u, k in enumerate(key(cout))}
        u = np.array([lut[int(k)] for k in key(cin)], np.int64)
        return [(0, u, np.arange(len(cin)))]
    for k, (dz, dy, dx) in enumerate(kernel_offsets(ksize, fault)):
        z, y, x = cout[:, 1] + dz, cout[:, 2] + dy * ts, cout[:, 3] + dx * ts
        ok = (z >= 0) & (z < PLANES) & (y >= 0) & (y < H) & (x >= 0) & (x < W)
        if fault == 'stride_ts_out':
            ok &= (y % (1 << lin) == 0) & (x % (1 << lin) == 0)
        j = np.full(len(cout), -1, np.int64)
        j[ok] = vol[cout[ok, 0], z[ok], y[ok] >> lin, x[ok] >> lin]
        u = np.nonzero(j >= 0)[0]
        pairs.append((k, u, j[u]))
    return pairs


def bwd_pairs_transposed(cin, cout, shape, lin, lout, ksize, fault=None):
    """The same pairs found from the input side, as the transposed kernel finds them: u = j - off_k * ts_in when on the output grid."""
    N, H, W = shape
    vol = index_volume(cout, N, H, W, lout)
    ts, m = 1 << lin, (1 << lout) - 1
    pairs = []
    for k, (dz, dy, dx) in enumerate(kernel_offsets(ksize)):
        z, y, x = cin[:, 1] - dz, cin[:, 2] - dy * ts, cin[:, 3] - dx * ts
        ok = (z >= 0) & (z < PLANES) & (y >= 0) & (y < H) & (x >= 0) & (x < W)
        if fault != 'transposed_no_ongrid':
            ok &= ((y & m) == 0) & ((x & m) == 0)
        u = np.full(len(cin), -1, np.int64)
        u[ok] = vol[cin[ok, 0], z[ok], y[ok] >> lout, x[ok] >> lout]
        j = np.nonzero(u >= 0)[0]
        pairs.append((k, u[j], j))
    return pairs


def sparse_conv_ref(x, Wk, pairs, n_out):
    """float64 out [n_out][Co] and the magnitude sum |x| |W|."""
    x64, W64 = x.astype(F64), Wk.astype(F64)
    out, mag = np.zeros((n_out, Wk.shape[2])), np.zeros((n_out, Wk.shape[2]))
    for k, u, j in pairs:
        np.add.at(out, u, x64[j] @ W64[k])
        np.add.at(mag, u, np.abs(x64[j]) @ np.abs(W64[k]))
    return out, mag


def sparse_conv_emu(x, Wk, pairs, n_out):
    """fp32: sequential fmaf over ci inside k, k ascending (u is unique inside one k)."""
    acc = np.zeros((n_out, Wk.shape[2]), F32)
    for k, u, j in sorted(pairs, key=lambda p: p[0]):
        a = acc[u]
        for ci in range(Wk.shape[1]):
            a = fma32(x[j, ci][:, None], Wk[k, ci][None, :], a)
        acc[u] = a
    return acc


def sparse_conv_bwd_ref(gy, Wk, pairs, n_in, prev=None):
    """The exact transpose: gx[j] = sum over the pairs (k, u, j) of W[k] gy[u]  (+ prev)."""
    g64, W64 = gy.astype(F64), Wk.astype(F64)
    out, mag = np.zeros((n_in, Wk.shape[1])), np.zeros((n_in, Wk.shape[1]))
    for k, u, j in pairs:
        np.add.at(out, j, g64[u] @ W64[k].T)
        np.add.at(mag, j, np.abs(g64[u]) @ np.abs(W64[k]).T)
    if prev is not None:
        out, mag = out + prev.astype(F64), mag + np.abs(prev.astype(F64))
    return out, mag


def sparse_conv_bwd_emu(gy, Wk, pairs, n_in, prev=None):
    acc = np.zeros((n_in, Wk.shape[1]), F32)
    for k, u, j in sorted(pairs, key=lambda p: p[0]):
        a = acc[j]
        for co in range(Wk.shape[2]):
            a = fma32(gy[u, co][:, None], Wk[k, :, co][None, :], a)
        acc[j] = a
    return acc if prev is None else prev.astype(F32) + acc


# ---- BatchNorm over the voxels ---------------------------------------------------------------------------------------------------
def sbn_forward_ref(f, gamma, beta, train=True, relu=True, res=None, track=None, world=1, fault=None):
    """f [cnt][C].  track = dict(rm, rv, nbt, repeats).  -> the dictionary of gbn_arith.forward_ref (fields [1][C], v / y [1][1][cnt][C]) with
    st [4][C] = {scale, shift, mean, inv}; R = max(cnt, 1), over `world` ranks holding the same voxels."""
    x = f.astype(F64)
    cnt, C = x.shape
    R = max(cnt, 1)
    Rg = R * world if cnt > 0 else 1
    if train:
        mean = x.sum(0) / R
        var = np.maximum((x * x).sum(0) / R - mean * mean, 0.0) if cnt == 0 else ((x - mean) ** 2).sum(0) / R
    else:
        mean, var = track['rm'].astype(F64), track['rv'].astype(F64)
    eps = float(F32(SBN_EPS))
    inv = 1.0 / np.sqrt(var + eps)
    scale = gamma.astype(F64) * inv
    shift = beta.astype(F64) - mean * scale
    v = x * scale + shift
    s = v if res is None else v + res.astype(F64)
    out = dict(mean=mean[None], var=var[None], inv=inv[None], scale=scale[None], shift=shift[None], R=R,
               kappa=((mean * mean + var + eps) / (var + eps))[None], rms=np.sqrt(mean * mean + var)[None],
               v=v.reshape(1, 1, cnt, C), y=(np.maximum(s, 0.0) if relu else s).reshape(1, 1, cnt, C))
    out['st'] = np.stack([scale, shift, mean, inv])
    if train and track is not None:
        unb = var * (Rg / (Rg - 1.0) if Rg > 1 and fault != 'biased_running_var' else 1.0)
        rm, rv = track['rm'].astype(F64), track['rv'].astype(F64)
        reps = 1 if fault == 'one_running_update' else track['repeats']
        for _ in range(reps):
            rm, rv = 0.9 * rm + 0.1 * mean, 0.9 * rv + 0.1 * unb
        out.update(rm=rm, rv=rv, nbt=int(track['nbt']) + reps)
    return out


def sbn_forward_mags(f, gamma, beta, fw, res=None, track=None, world=1):
    m = GA.forward_mags(f.reshape(1, 1, *f.shape), gamma, beta, fw, 1, None if res is None else res.reshape(1, 1, *res.shape),
                        track=None if track is None else dict(rm=track['rm'], rv=track['rv']), world=world)
    sc = np.abs(gamma.astype(F64)) * m['inv'][0]
    m['st'] = np.stack([sc, np.abs(beta.astype(F64)) + m['mean'][0] * sc, m['mean'][0], m['inv'][0]])      # {scale, shift, mean, inv}
    return m


def _sbn_partials(a):
    """cd_sbn_stats_kernel's order: block b sums voxels b, b + 256, ... one after the other in fp32 -> [256][C]"""
    cnt, C = a.shape
    K = (cnt + SBN_BLOCKS - 1) // SBN_BLOCKS
    pad = np.zeros((max(K, 1) * SBN_BLOCKS, C), F32)
    pad[:cnt] = a
    s = np.zeros((SBN_BLOCKS, C), F32)
    for k in range(max(K, 1)):
        s = s + pad[k * SBN_BLOCKS:(k + 1) * SBN_BLOCKS]
    return s


def sbn_forward_emu(f, gamma, beta, train=True, relu=True, res=None, track=None, world=1):
    x = f.astype(F32)
    cnt, C = x.shape
    gamma, beta = gamma.astype(F32), beta.astype(F32)
    out = {}
    if train:
        s1, s2 = _sbn_partials(x).astype(F64).sum(0), _sbn_partials(x * x).astype(F64).sum(0)
        R = float(max(cnt, 1))
        if world > 1:
            s1, s2, R = s1 * world, s2 * world, (float(cnt * world) if cnt > 0 else 1.0)
        m = s1 / R
        v = np.maximum(s2 / R - m * m, 0.0)
        mu, var = m.astype(F32), v.astype(F32)
        if track is not None:
            unb = (v * R / (R - 1.0) if R > 1 else v).astype(F32)
            rm, rv = track['rm'].astype(F32), track['rv'].astype(F32)
            for _ in range(track['repeats']):
                rm, rv = F32(0.9) * rm + F32(0.1) * mu, F32(0.9) * rv + F32(0.1) * unb
            out.update(rm=rm, rv=rv)
    else:
        mu, var = track['rm'].astype(F32), track['rv'].astype(F32)
    iv = F32(1) / np.sqrt(var + F32(SBN_EPS))
    sc = gamma * iv
    sh = beta - mu * sc
    y = fma32(x, sc, sh)
    if res is not None:
        y = y + res.astype(F32)
    out.update(st=np.stack([sc, sh, mu, iv]), y=(np.maximum(y, F32(0)) if relu else y).reshape(1, 1, cnt, C))
    return out


def sbn_backward_ref(f, g, fw, gamma, relu=True, res=None, gres_prev=None, fault=None):
    """-> gbn_arith.backward_ref's dictionary (gx, gres [1][1][cnt][C], dgamma, dbeta); the ReLU mask comes from y = bn(f) + res."""
    cnt, C = f.shape
    x4, g4 = f.reshape(1, 1, cnt, C), g.reshape(1, 1, cnt, C)
    r4 = None if res is None else res.reshape(1, 1, cnt, C)
    p4 = None if (gres_prev is None or fault == 'gres_overwritten') else gres_prev.reshape(1, 1, cnt, C)
    R = max(cnt, 1)
    x0 = x4.astype(F64)
    v = x0 * fw['scale'][0] + fw['shift'][0]
    s = v if (r4 is None or fault == 'mask_pre_residual') else v + r4.astype(F64)
    g1 = g4.astype(F64) * (s > 0) if relu else g4.astype(F64)
    xhat = (x0 - fw['mean'][0]) * fw['inv'][0]
    dbeta, dgamma = g1.sum((0, 1, 2)), (g1 * xhat).sum((0, 1, 2))
    c1, c2 = dbeta / R, dgamma / R
    out = dict(g1=g1, gouter=g1, xhat=xhat, c1=c1, c2=c2, dbeta=dbeta, dgamma=dgamma, gx=gamma.astype(F64) * fw['inv'][0] * (g1 - c1 - xhat * c2), v=v)
    out['gres'] = g1 + (0.0 if p4 is None else p4.astype(F64))
    return out


def sbn_backward_mags(f, g, fw, fmag, bw, gamma, gres_prev=None):
    cnt, C = f.shape
    if cnt == 0:
        z = np.zeros((1, 1, 0, C))
        return dict(dbeta=np.zeros(C), dgamma=np.zeros(C), gx=z, gres=z)
    return GA.backward_mags(f.reshape(1, 1, cnt, C), g.reshape(1, 1, cnt, C), fw, fmag, bw, gamma, 1, 'none', None,
                            None if gres_prev is None else gres_prev.reshape(1, 1, cnt, C))


def sbn_backward_emu(f, y, g, st, gamma, relu=True, gres_prev=None, world=1):
    x, yv, gv = f.astype(F32), y.reshape(f.shape).astype(F32), g.astype(F32)
    cnt, C = x.shape
    mu, iv = st[2].astype(F32), st[3].astype(F32)
    g1 = np.where(yv > 0, gv, F32(0)) if relu else gv
    xh = (x - mu) * iv
    s1, s2 = _sbn_partials(g1).astype(F64).sum(0), _sbn_partials(g1 * xh).astype(F64).sum(0)
    R = float(max(cnt, 1))
    gsc = F32(1)
    if world > 1:
        s1, s2, R, gsc = s1 * world, s2 * world, (float(cnt * world) if cnt > 0 else 1.0), F32(1) / F32(world)
    b0, c1, c2 = gamma.astype(F32) * iv, (s1 / R).astype(F32), (s2 / R).astype(F32)
    return dict(dbeta=s1.astype(F32) * gsc, dgamma=s2.astype(F32) * gsc, gx=(b0 * (g1 - c1 - xh * c2)).reshape(1, 1, cnt, C),
                gres=(g1 if gres_prev is None else gres_prev.astype(F32) + g1).reshape(1, 1, cnt, C))


# ---- densify -----------------------------------------------------------------------------------------------------------------------
def densify_ref(f, c2, N, H, W):
    dense = np.zeros((N, PLANES, H >> 2, W >> 2, f.shape[1]), F32)
    dense[c2[:, 0], c2[:, 1], c2[:, 2] >> 2, c2[:, 3] >> 2] = f
    return dense


def densify_bwd_ref(gvol, c2, c0, C):
    return gvol[c2[:, 0], c2[:, 1], c2[:, 2] >> 2, c2[:, 3] >> 2, c0:c0 + C].astype(F32).reshape(len(c2), C)


# ---- padding family, staging, clamp ----------------------------------------------------------------------------------------------
def normalize_ref(v, ch_axis, div, mean, std):
    """(v / div - mean[c]) / std[c] in float64 of the fp32 operands, the fp32 evaluation (three roundings), and the magnitude."""
    shp = [1] * v.ndim
    shp[ch_axis] = 3
    m32, s32 = np.asarray(mean, F32).reshape(shp), np.asarray(std, F32).reshape(shp)
    v64, m, s, d = v.astype(F64), m32.astype(F64), s32.astype(F64), float(F32(div))
    ref = (v64 / d - m) / s
    emu = (v.astype(F32) / F32(div) - m32) / s32
    return ref, emu, (np.abs(v64 / d) + np.abs(m)) / np.abs(s) + np.abs(ref)


def _place(dst, src, pt, pr, fault=None):
    """item 0 pads top / right, item 1 bottom / left: dst [2][N][...][Hp][Wp] <- src [N][...][H][W]"""
    H, W = src.shape[-2:]
    (a, b) = ((0, pr), (pt, 0)) if fault == 'pad_corners_swapped' else ((pt, 0), (0, pr))
    dst[0][..., a[0]:a[0] + H, a[1]:a[1] + W] = src
    dst[1][..., b[0]:b[0] + H, b[1]:b[1] + W] = src
    return dst


def pad_dual_ref(src, Hp, Wp, pt, pr, norm=None, fault=None):
    """src [N][C][H][W] -> [2N][C][Hp][Wp] (float64 with norm = (div, mean, std), else fp32, exact), emulation, magnitude."""
    N, C = src.shape[:2]
    if norm is None:
        return _place(np.zeros((2, N, C, Hp, Wp), F32), src, pt, pr, fault).reshape(2 * N, C, Hp, Wp), None, None
    ref, emu, mag = normalize_ref(src, 1, *norm)
    mk = lambda a, t: _place(np.zeros((2, N, C, Hp, Wp), t), a, pt, pr, fault).reshape(2 * N, C, Hp, Wp)
    return mk(ref, F64), mk(emu, F32), mk(mag, F64)


def crop_avg_ref(net, N, H, W, pt, pr, fault=None):
    """net [2N][Hp][Wp] -> [N][H][W]: one fp32 addition, halved (exact)."""
    s = net[:N, pt:pt + H, :W].astype(F32) + net[N:, :H, pr:pr + W].astype(F32)
    return s if fault == 'crop_not_halved' else s / F32(2)


def scatter_dual_grad_ref(g, Hp, Wp, pt, pr, fault=None):
    N = g.shape[0]
    return _place(np.zeros((2, N, Hp, Wp), F32), F32(0.5) * g.astype(F32), pt, pr, fault).reshape(2 * N, Hp, Wp)


def stage_ref(image, sparse, passes, C, norm=None):
    """image [N][3][H][W], sparse [N][H][W] -> [passes N][H][W][C]: (ref, emulation, magnitude); exact without norm."""
    N, _, H, W = image.shape
    img = np.moveaxis(image, 1, -1)
    if norm is None:
        ref = emu = img.astype(F32)
        mag = np.zeros(img.shape)
    else:
        ref, emu, mag = normalize_ref(img, 3, *norm)
    out = [np.zeros((passes * N, H, W, C), t) for t in (F64, F32, F64)]
    for o, a in zip(out, (ref, emu, mag)):
        o[:N, ..., :3] = a
    for o in out[:2]:
        for p in range(passes):
            o[p * N:(p + 1) * N, ..., 3] = sparse
    return out


def clamp_ref(x, maxd):
    return np.minimum(np.maximum(x, F32(0)), F32(maxd)).astype(F32) if maxd >= 0 else x.astype(F32)


# ---- fusion --------------------------------------------------------------------------------------------------------------------------
def fusion_fwd_ref(feat2d, feat3d, passes, fault=None):
    """feat2d [passes N][h][w][16], feat3d [N][16][h][w][16] -> vol [passes N][16][h][w][32] (one fp32 product per element: exact), mask"""
    N = feat3d.shape[0]
    occ = (feat3d != 0).any(-1).astype(F32)
    m = occ + ((F32(0) if fault == 'fusion_no_plus_one' else F32(1)) - occ.sum(1, keepdims=True, dtype=F32))
    vol = np.zeros((passes * N,) + feat3d.shape[1:4] + (32,), F32)
    for p in range(passes):
        vol[p * N:(p + 1) * N, ..., :16] = feat2d[p * N:(p + 1) * N, None].astype(F32) * m[..., None]
        vol[p * N:(p + 1) * N, ..., 16:] = feat3d
    return vol, m


def fusion_bwd_ref(gvol, mask):
    """gvol [N][16][h][w][32], mask [N][16][h][w] -> (float64 [N][h][w][16], emulation (fmaf over the planes), magnitude)"""
    g, m = gvol[..., :16], mask[..., None]
    ref = (g.astype(F64) * m.astype(F64)).sum(1)
    mag = (np.abs(g.astype(F64)) * np.abs(m.astype(F64))).sum(1)
    acc = np.zeros(ref.shape, F32)
    for d in range(PLANES):
        acc = fma32(g[:, d], m[:, d], acc)
    return ref, acc, mag


# ---- MaxPool3d(2) ----------------------------------------------------------------------------------------------------------------
def _windows(x):
    """x [2 io][H][W][C] -> [io][Ho][Wo][8][C], window position k = 4 plane + 2 row + column"""
    I, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    v = x[:, :2 * Ho, :2 * Wo].reshape(I // 2, 2, Ho, 2, Wo, 2, C)
    return v.transpose(0, 2, 4, 1, 3, 5, 6).reshape(I // 2, Ho, Wo, 8, C)


def pool_fwd_ref(x):
    return _windows(x).max(3)


def pool_bwd_ref(x, gy, prev=None, fault=None):
    """The gradient goes to the FIRST maximum of each window in (plane, row, column) order; odd last rows / columns get none."""
    I, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    w = _windows(x)
    arg = (7 - np.argmax(w[:, :, :, ::-1], 3)) if fault == 'last_max' else np.argmax(w, 3)
    gw = np.zeros(w.shape, F32)
    np.put_along_axis(gw, arg[:, :, :, None], gy[:, :, :, None].astype(F32), 3)
    gx = np.zeros(x.shape, F32)
    gx[:, :2 * Ho, :2 * Wo] = gw.reshape(I // 2, Ho, Wo, 2, 2, 2, C).transpose(0, 3, 1, 4, 2, 5, 6).reshape(I, 2 * Ho, 2 * Wo, C)
    if fault == 'pool_odd_last_row' and H % 2:
        gx[:, H - 1] = gx[:, H - 2]
    return gx if prev is None else prev.astype(F32) + gx


# ---- nearest upsampling ----------------------------------------------------------------------------------------------------------
def nearest_src(n_in, n_out, fault=None):
    """ATen's nearest rule: min(floor(dst * (float)in / out), in - 1), the product in fp32."""
    t = np.arange(n_out, dtype=F32) * (F32(n_in) / F32(n_out))
    return np.minimum((np.ceil(t) if fault == 'nearest_ceil' else np.floor(t)).astype(np.int64), n_in - 1)


def up_fwd_ref(x, Do, Ho, Wo, fault=None):
    """x [frames][Di][Hi][Wi][C]"""
    _, Di, Hi, Wi, _ = x.shape
    return x[:, nearest_src(Di, Do, fault)][:, :, nearest_src(Hi, Ho, fault)][:, :, :, nearest_src(Wi, Wo, fault)]


def up_bwd_ref(gy, Di, Hi, Wi, prev=None, fault=None):
    """gy [frames][Do][Ho][Wo][C] -> the sum over the destinations of each source, float64 (exact on integer-valued gradients)."""
    Fr, Do, Ho, Wo, C = gy.shape
    g = gy.astype(F64)
    for axis, (n_in, n_out) in enumerate(((Di, Do), (Hi, Ho), (Wi, Wo)), 1):
        src = nearest_src(n_in, n_out)
        dst = np.arange(n_out)
        if fault == 'up_window_narrow':                                   # the margin of one destination taken off the quotients where it is added
            keep = (dst >= src * n_out // n_in + 1) & (dst <= (src + 1) * n_out // n_in - 1)
        else:
            keep = np.ones(n_out, bool)
        shp = list(g.shape)
        shp[axis] = n_in
        o = np.zeros(shp)
        idx = [slice(None)] * g.ndim
        for d_ in dst[keep]:
            idx[axis] = d_
            tgt = list(idx)
            tgt[axis] = src[d_]
            o[tuple(tgt)] += g[tuple(idx)]
        g = o
    return g if prev is None else g + prev.astype(F64)


# ---- pixel shuffle + softmax expectation -----------------------------------------------------------------------------------------
def _shuffle(cost, fault=None):
    """cost [N][16][h][w][16] -> [N][16][4h][4w]: pixel (4y + i, 4x + j) reads channel 4i + j"""
    N, D, h, w, _ = cost.shape
    c = cost.reshape(N, D, h, w, 4, 4)
    if fault == 'shuffle_4j_i':
        c = c.transpose(0, 1, 2, 3, 5, 4)
    return c.transpose(0, 1, 2, 4, 3, 5).reshape(N, D, 4 * h, 4 * w)


def regress_fwd_ref(cost, z_step, fault=None):
    """-> (float64 pred [N][4h][4w], fp32 emulation, magnitude)"""
    v = _shuffle(cost, fault)
    v64 = v.astype(F64)
    m = v64.max(1, keepdims=True)
    q = np.exp(v64 - m)
    p = q / q.sum(1, keepdims=True)
    d = np.arange(PLANES, dtype=F64).reshape(1, -1, 1, 1)
    E = (p * d).sum(1)
    zs = float(F32(z_step))
    mag = zs * (1.0 + E + (p * np.abs(d - E[:, None]) * (1.0 + np.abs(v64 - m))).sum(1))
    v32 = v.astype(F32)
    q32 = np.exp(v32 - v32.max(1, keepdims=True))
    s = np.zeros(E.shape, F32)
    e = np.zeros(E.shape, F32)
    for k in range(PLANES):
        s = s + q32[:, k]
        e = e + q32[:, k] * F32(k)
    return E * zs, (e / s) * F32(z_step), mag


def regress_bwd_ref(cost, gpred, z_step, fault=None):
    """-> (float64 gcost [N][16][h][w][16], fp32 emulation, magnitude)"""
    N, D, h, w, _ = cost.shape
    v = _shuffle(cost, fault)
    v64 = v.astype(F64)
    m = v64.max(1, keepdims=True)
    q = np.exp(v64 - m)
    p = q / q.sum(1, keepdims=True)
    d = np.arange(PLANES, dtype=F64).reshape(1, -1, 1, 1)
    E = (p * d).sum(1, keepdims=True)
    zs = float(F32(z_step))
    g = gpred.astype(F64)[:, None] * zs
    ref = g * p * (d - E)
    spread = (p * np.abs(d - E) * (1.0 + np.abs(v64 - m))).sum(1, keepdims=True)
    mag = np.abs(g) * p * ((np.abs(d - E) + 1.0 + E) * (1.0 + np.abs(v64 - m)) + spread)      # (E's own rounding scales with E)
    v32 = v.astype(F32)
    q32 = np.exp(v32 - v32.max(1, keepdims=True))
    s = np.zeros(E.shape[:1] + E.shape[2:], F32)
    e = np.zeros_like(s)
    for k in range(PLANES):
        s = s + q32[:, k]
        e = e + q32[:, k] * F32(k)
    E32 = (e / s)[:, None]
    g32 = (gpred.astype(F32) * F32(z_step))[:, None]
    emu = g32 * (q32 / s[:, None]) * (np.arange(PLANES, dtype=F32).reshape(1, -1, 1, 1) - E32)

    def unshuffle(a):
        a = a.reshape(N, D, h, 4, w, 4).transpose(0, 1, 2, 4, 3, 5)
        if fault == 'shuffle_4j_i':
            a = a.transpose(0, 1, 2, 3, 5, 4)
        return a.reshape(N, D, h, w, 16)
    return unshuffle(ref), unshuffle(emu), unshuffle(mag)


# ---- the heads' rows -----------------------------------------------------------------------------------------------------------------
def rows_fwd_ref(feat, fault=None):
    """feat [N][D][h][w][C] -> rows [N h w][C D], column c D + d"""
    N, D, h, w, C = feat.shape
    t = feat.transpose(0, 2, 3, 1, 4) if fault == 'rows_d_major' else feat.transpose(0, 2, 3, 4, 1)
    return np.ascontiguousarray(t).reshape(N * h * w, C * D)


def rows_bwd_ref(grows, N, D, h, w, C, prev=None, fault=None):
    t = grows.reshape(N, h, w, D, C).transpose(0, 3, 1, 2, 4) if fault == 'rows_d_major' else grows.reshape(N, h, w, C, D).transpose(0, 4, 1, 2, 3)
    t = np.ascontiguousarray(t).astype(F32)
    return t if prev is None else prev.astype(F32) + t
