"""ORACLE -- test infrastructure only.  The MSG_CHN step's first-layer / prediction convolutions (csrc/conv_small.hip), resamplings
(csrc/resample.hip) and loss (csrc/loss.hip) restated per OPERATION in float64 (torch / numpy), and next to each reference a float32
emulation of the kernel's operation order.  The references are what the per-element tests compare the GPU with
(tests/test_gpu_msgchn_elementwise.py); the emulations only size the bounds (tests/msgchn_cases.py: TOL = 4 x their largest error ratio).

Every function returns magnitudes next to its values: the same expression on absolute values, which is what a rounding error scales with.
  convolutions     sum |x| |w| + |bias| + the epilogue operands' magnitudes
  bilinear x2      U |x| + in_size x (the touched taps' |x|) per axis: the fp32 source coordinate scale * dst carries a relative error, i.e.
                   an absolute one that grows with the map size, and moves weight between the two taps
  pooled maps      (sum |d| / k^2) / (count / k^2 + 1e-4)
  loss             see loss_ref()
"""
import numpy as np
import torch
import torch.nn.functional as F

F32, F64 = np.float32, np.float64
EPS_NORM = float(F32(1e-12))          # F.normalize's eps as the fp32 graph holds it
EPS_POOL = float(F32(1e-4))           # the pooled maps' 1e-4 likewise


def bf16_round(a):
    """fp32 -> the nearest bf16-representable fp32 (ties to even)"""
    u = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(F32).reshape(np.shape(a))


def bf16_half_ulp(v):
    """half the spacing of bf16 (8 significant bits) at |v|: 2^(floor(log2 |v|) - 8); 0 at 0"""
    v = np.abs(np.asarray(v, F64))
    with np.errstate(divide='ignore'):
        e = np.floor(np.log2(v))
    return np.where(v > 0, np.exp2(e - 8), 0.0)


def fma32(a, b, c):
    """fl32(a b + c): the product of two fp32 values is exact in float64"""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


# ---- bilinear x2, align_corners=True ---------------------------------------------------------------------------------------------------
def up_scale(n_in, n_out):
    return F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)


def lerp_coef(dst, in_size, scale):
    """csrc/ptta_common.h lerp_coef in float32: (i0, i1, l0, l1) of the destinations `dst`"""
    dst = np.asarray(dst)
    s = (F32(scale) * dst.astype(F32)).astype(F32)
    i0 = np.minimum(s.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    l1 = (s - i0.astype(F32)).astype(F32)
    return i0, i1, (F32(1) - l1).astype(F32), l1


def up2t_weights(i, in_size, scale):
    """csrc/resample.hip up2T_weights: d0 = 2 i - 3 and the seven candidates' weights, float32"""
    i = np.asarray(i, np.int64)
    d0 = 2 * i - 3
    d = d0[:, None] + np.arange(7)
    ok = (d >= 0) & (d < 2 * in_size)
    i0, i1, l0, l1 = lerp_coef(np.clip(d, 0, 2 * in_size - 1), in_size, scale)
    w = np.where(i0 == i[:, None], l0, F32(0)).astype(F32)
    w = (w + np.where(i1 == i[:, None], l1, F32(0)).astype(F32)).astype(F32)
    return d0, np.where(ok, w, F32(0)).astype(F32)


def up2t_window(i, in_size, scale):
    """csrc/resample.hip up2T_window: the first destination of the clamped five-wide window and its five weights"""
    c0, w7 = up2t_weights(i, in_size, scale)
    k0 = np.where(w7[:, 0] == 0, np.where(w7[:, 1] == 0, 2, 1), 0)
    first = np.maximum(np.minimum(c0 + k0, 2 * in_size - 5), 0)
    c = first[:, None] + np.arange(5) - c0[:, None]
    w = np.where((c >= 0) & (c < 7), np.take_along_axis(w7, np.clip(c, 0, 6), 1), F32(0)).astype(F32)
    return first, w


def touching(in_size):
    """Every (destination, source, weight) with a non-zero float32 weight, over ALL destinations of the x2 map (not the candidates)"""
    d = np.arange(2 * in_size)
    i0, i1, l0, l1 = lerp_coef(d, in_size, up_scale(in_size, 2 * in_size))
    same = i0 == i1
    w0 = np.where(same, (l0 + l1).astype(F32), l0)
    dd = np.concatenate([d[w0 != 0], d[(l1 != 0) & ~same]])
    ii = np.concatenate([i0[w0 != 0], i1[(l1 != 0) & ~same]])
    return dd, ii


def up2_matrix(n_in):
    """[2 n, n] float64 weights from exact rational coordinates src = dst (n - 1) / (2 n - 1), and the 0 / 1 matrix of the touched taps"""
    n_out = 2 * n_in
    U, T = np.zeros((n_out, n_in)), np.zeros((n_out, n_in))
    for d in range(n_out):
        num, den = d * (n_in - 1), n_out - 1
        i0 = min(num // den, n_in - 1)
        frac = (num - i0 * den) / den
        i1 = min(i0 + 1, n_in - 1)
        U[d, i0] += 1.0 - frac
        U[d, i1] += frac
        T[d, i0] = T[d, i1] = 1.0
    return U, T


def _sandwich(Ly, x, Lx):
    """x [B, H, W(, C)] -> Ly x Lx^T over (H, W)"""
    x = np.asarray(x, F64)
    y = np.moveaxis(np.tensordot(Ly, x, (1, 1)), 0, 1)               # [B, d, W, ...]
    return np.moveaxis(np.tensordot(Lx, y, (1, 2)), 0, 2)            # [B, d, e, ...]


def up2_ref(x):
    """x [B, H, W(, C)] -> (x2 map, magnitude), float64"""
    H, W = x.shape[1:3]
    (Uy, Ty), (Ux, Tx) = up2_matrix(H), up2_matrix(W)
    a = np.abs(np.asarray(x, F64))
    return _sandwich(Uy, x, Ux), _sandwich(Uy, a, Ux) + W * _sandwich(Uy, a, Tx) + H * _sandwich(Ty, a, Ux)


def up2t_ref(g, add=None):
    """g [B, 2 H, 2 W(, C)] -> (add + U^T g, magnitude)"""
    H, W = g.shape[1] // 2, g.shape[2] // 2
    (Uy, Ty), (Ux, Tx) = up2_matrix(H), up2_matrix(W)
    a = np.abs(np.asarray(g, F64))
    ref = _sandwich(Uy.T, g, Ux.T)
    mag = _sandwich(Uy.T, a, Ux.T) + W * _sandwich(Uy.T, a, Tx.T) + H * _sandwich(Ty.T, a, Ux.T)
    if add is not None:
        ref, mag = ref + np.asarray(add, F64), mag + np.abs(np.asarray(add, F64))
    return ref, mag


def _taps(x, H, W):
    """the four taps and fp32 coefficients of every destination of the x2 map of x [B, H, W(, C)]"""
    iy0, iy1, ly0, ly1 = lerp_coef(np.arange(2 * H), H, up_scale(H, 2 * H))
    ix0, ix1, lx0, lx1 = lerp_coef(np.arange(2 * W), W, up_scale(W, 2 * W))
    sh = (1, 2 * H, 1) + (1,) * (x.ndim - 3)
    sw = (1, 1, 2 * W) + (1,) * (x.ndim - 3)
    g = lambda iy, ix: x[:, iy][:, :, ix]
    return (g(iy0, ix0), g(iy0, ix1), g(iy1, ix0), g(iy1, ix1)), (ly0.reshape(sh), ly1.reshape(sh)), (lx0.reshape(sw), lx1.reshape(sw))


def up2_emu(x):
    """up2_1ch_kernel / the epilogue's skip term: ly.l0 (lx.l0 v00 + lx.l1 v01) + ly.l1 (lx.l0 v10 + lx.l1 v11) in float32"""
    x = np.asarray(x, F32)
    (v00, v01, v10, v11), (ly0, ly1), (lx0, lx1) = _taps(x, x.shape[1], x.shape[2])
    return (ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)).astype(F32)


def up2t_emu(g, ch32, add=None):
    """up2T_1ch_kernel (row sums, then the weighted rows) / up2T_32_kernel (one product of the two weights per tap), float32"""
    g = np.asarray(g, F32)
    Ho, Wo = g.shape[1:3]
    H, W = Ho // 2, Wo // 2
    dy0, wy = up2t_window(np.arange(H), H, up_scale(H, Ho))
    dx0, wx = up2t_window(np.arange(W), W, up_scale(W, Wo))
    ry = dy0[:, None] + np.minimum(np.arange(5), Ho - 1 - dy0[:, None])
    cx = dx0[:, None] + np.minimum(np.arange(5), Wo - 1 - dx0[:, None])
    tail = (1,) * (g.ndim - 3)
    acc = np.zeros((g.shape[0], H, W) + g.shape[3:], F32)
    for ky in range(5):
        rows = g[:, ry[:, ky]]                                  # [B, H, Wo(, C)]
        wyk = wy[:, ky].reshape((1, H, 1) + tail)
        row = np.zeros_like(acc)
        for kx in range(5):
            v = rows[:, :, cx[:, kx]]
            wxk = wx[:, kx].reshape((1, 1, W) + tail)
            if ch32:
                acc = (acc + (wyk * wxk).astype(F32) * v).astype(F32)
            else:
                row = (row + wxk * v).astype(F32)
        if not ch32:
            acc = (acc + wyk * row).astype(F32)
    return acc if add is None else (acc + np.asarray(add, F32)).astype(F32)


# ---- pooled maps -----------------------------------------------------------------------------------------------------------------------
def clamp_ref(s, max_d):
    s = np.asarray(s, F32)
    return np.minimum(np.maximum(s, F32(0)), F32(max_d)) if max_d >= 0 else s.copy()


def prep_ref(sparse, max_d):
    """-> dclamp (exact, fp32), {k: (pooled map, magnitude)} for k = 2, 4: avg_pool(d, k) / (avg_pool(d > 0, k) + 1e-4)"""
    dc = clamp_ref(sparse, max_d)
    t = torch.from_numpy(dc.astype(F64))[:, None]
    out = {}
    for k in (2, 4):
        cnt = F.avg_pool2d((t > 0).double(), k, k)
        out[k] = ((F.avg_pool2d(t, k, k) / (cnt + EPS_POOL))[:, 0].numpy(), (F.avg_pool2d(t.abs(), k, k) / (cnt + EPS_POOL))[:, 0].numpy())
    return dc, out


def prep_emu(sparse, max_d):
    """prep_kernel: the 16 values of a 4 x 4 block summed row by row, the four quadrants on the side, float32"""
    dc = clamp_ref(sparse, max_d)
    N, H, W = dc.shape
    blk = dc.reshape(N, H // 4, 4, W // 4, 4)
    s4, c4 = np.zeros((N, H // 4, W // 4), F32), np.zeros((N, H // 4, W // 4), F32)
    s2, c2 = np.zeros((N, H // 4, W // 4, 2, 2), F32), np.zeros((N, H // 4, W // 4, 2, 2), F32)
    for dy in range(4):
        for dx in range(4):
            d = blk[:, :, dy, :, dx]
            c = (d > 0).astype(F32)
            s4, c4 = (s4 + d).astype(F32), c4 + c
            s2[..., dy >> 1, dx >> 1] = (s2[..., dy >> 1, dx >> 1] + d).astype(F32)
            c2[..., dy >> 1, dx >> 1] += c
    d14 = ((s4 / F32(16)) / (c4 / F32(16) + F32(0.0001))).astype(F32)
    d12 = ((s2 / F32(4)) / (c2 / F32(4) + F32(0.0001))).astype(F32)
    return dc, {2: d12.transpose(0, 1, 3, 2, 4).reshape(N, H // 2, W // 2), 4: d14}


# ---- the first-layer convolution ---------------------------------------------------------------------------------------------------------
def conv_in_weight(weight, cin, cin_first=0, transpose_flip=False):
    """What ptta_pack_conv_in packs, as a cross-correlation weight [32][cin][3][3]: channels cin_first .. of a first layer's weight, or the
    [1][32][3][3] weight of a 32 -> 1 convolution as its input gradient (in / out swapped, taps flipped)"""
    weight = np.asarray(weight)
    if transpose_flip:
        return np.ascontiguousarray(weight[0][:, None, ::-1, ::-1])
    return np.ascontiguousarray(weight[:, cin_first:cin_first + cin])


def conv_out1_weight(weight, src_cin_index=0, from_conv_in=False):
    """What ptta_pack_conv_out1 packs, [1][32][3][3]: a prediction layer's weight, or plane src_cin_index of a first layer's
    [32][cin_total][3][3] weight as the input gradient with respect to that plane"""
    weight = np.asarray(weight)
    if from_conv_in:
        return np.ascontiguousarray(weight[:, src_cin_index][None, :, ::-1, ::-1])
    return weight


def _planes(planes, B, zero_from_b, dt):
    """planes: [(array [nb][H][W], None or (div, mean, std))] -> (x [B][cin][H][W] in dt, |x| magnitude float64)"""
    xs, ms = [], []
    for p, norm in planes:
        v = np.asarray(p, dt)[np.arange(B) % p.shape[0]]
        m = np.abs(v.astype(F64))
        if norm is not None:
            div, mean, std = (dt(F32(t)) for t in norm)
            v = ((v / div - mean) / std).astype(dt)
            m = (m / abs(float(div)) + abs(float(mean))) / abs(float(std))
        xs.append(v)
        ms.append(m)
    x, m = np.stack(xs, 1), np.stack(ms, 1)
    x[zero_from_b:] = 0
    m[zero_from_b:] = 0
    return x, m


def _conv64(x, w):
    return F.conv2d(torch.from_numpy(np.asarray(x, F64)), torch.from_numpy(np.asarray(w, F64)), padding=1).numpy()


def _nhwc(a):
    return np.ascontiguousarray(np.moveaxis(a, 1, -1))


def conv_in_ref(planes, w_eff, B, zero_from_b=1 << 30, bias=None, up=None, mask=None, add1=None):
    """-> dict(raw, sum, mag_raw, mag_sum), NHWC float64: conv + bias + bilinear_x2(up[b % nb]), masked by mask[b % nb] > 0; sum = raw + add1"""
    x, xm = _planes(planes, B, zero_from_b, F64)
    v, m = _nhwc(_conv64(x, w_eff)), _nhwc(_conv64(xm, np.abs(w_eff)))
    idx = lambda t: np.arange(B) % t.shape[0]
    if bias is not None:
        v, m = v + np.asarray(bias, F64), m + np.abs(np.asarray(bias, F64))
    if up is not None:
        u, um = up2_ref(up)
        v, m = v + u[idx(up)], m + um[idx(up)]
    if mask is not None:
        keep = np.asarray(mask)[idx(mask)] > 0
        v, m = np.where(keep, v, 0.0), np.where(keep, m, 0.0)
    out = dict(raw=v, mag_raw=m, sum=v, mag_sum=m)
    if add1 is not None:
        a = np.asarray(add1, F64)[idx(add1)]
        out.update(sum=v + a, mag_sum=m + np.abs(a))
    return out


def conv_in_emu(planes, w_eff, B, zero_from_b=1 << 30, bias=None, up=None, mask=None, add1=None):
    """The kernels' order in float32: one fused multiply-add per k = tap * cin + ci, then + bias, + skip term, mask, + add1"""
    x, _ = _planes(planes, B, zero_from_b, F32)
    cin, H, W = x.shape[1:]
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    acc = np.zeros((B, H, W, 32), F32)
    w = np.asarray(w_eff, F32)
    for tap in range(9):
        for ci in range(cin):
            acc = fma32(xp[:, ci, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W, None], w[None, None, None, :, ci, tap // 3, tap % 3], acc)
    idx = lambda t: np.arange(B) % t.shape[0]
    v = acc if bias is None else (acc + np.asarray(bias, F32)).astype(F32)
    if up is not None:
        v = (v + up2_emu(up)[idx(up)]).astype(F32)
    if mask is not None:
        v = np.where(np.asarray(mask)[idx(mask)] > 0, v, F32(0)).astype(F32)
    return dict(raw=v, sum=v if add1 is None else (v + np.asarray(add1, F32)[idx(add1)]).astype(F32))


def sign_bits(a):
    """One 32-bit word per pixel of an NHWC map: bit c = (channel c > 0)"""
    return ((np.asarray(a) > 0).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


# ---- the prediction convolution ----------------------------------------------------------------------------------------------------------
def conv_out1_ref(x, w_eff, B, bias=None, add=None, relu_in=False):
    """x [in_nb][H][W][32] -> (out [B][H][W], magnitude): conv(relu?(x[b % in_nb])) + bias + add[b % add_nb]"""
    x = np.asarray(x, F64)[np.arange(B) % x.shape[0]]
    x = np.maximum(x, 0) if relu_in else x
    xc = np.moveaxis(x, -1, 1)
    v, m = _conv64(xc, w_eff)[:, 0], _conv64(np.abs(xc), np.abs(w_eff))[:, 0]
    if bias is not None:
        v, m = v + float(bias[0]), m + abs(float(bias[0]))
    if add is not None:
        a = np.asarray(add, F64)[np.arange(B) % add.shape[0]]
        v, m = v + a, m + np.abs(a)
    return v, m


def conv_out1_emu(x, w_eff, B, bias=None, add=None, relu_in=False):
    """conv_out1_lds_kernel: eight lanes per pixel, each four channels over the nine taps by fused multiply-adds, then the three xor-shuffle
    additions (a balanced tree), + bias, + add"""
    x = np.asarray(x, F32)[np.arange(B) % x.shape[0]]
    x = np.maximum(x, F32(0)) if relu_in else x
    H, W = x.shape[1:3]
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    w = np.asarray(w_eff, F32)[0]
    lanes = []
    for q in range(8):
        acc = np.zeros((B, H, W), F32)
        for tap in range(9):
            for j in range(4):
                acc = fma32(xp[:, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W, 4 * q + j], w[4 * q + j, tap // 3, tap % 3], acc)
        lanes.append(acc)
    for step in (1, 2, 4):
        lanes = [(lanes[k] + lanes[k ^ step]).astype(F32) for k in range(8)]
    v = lanes[0]
    if bias is not None:
        v = (v + F32(bias[0])).astype(F32)
    if add is not None:
        v = (v + np.asarray(add, F32)[np.arange(B) % add.shape[0]]).astype(F32)
    return v


# ---- the loss ------------------------------------------------------------------------------------------------------------------------------
def adapt_loss64(image, depth, sparse, validity, emb, ref, w3, max_d):
    """float64 transcription of adapt_loss (sparse-depth consistency, edge-aware smoothness, cosine term with its gate) on torch tensors;
    depth [N][H][W]; emb = ref = None drops the cosine term.  -> (loss, l_sm, l_sd, l_cos, gated w_cos)"""
    w_sd, w_sm, w_cos = (float(F32(t)) for t in w3)
    d, s, im = depth[:, None], sparse[:, None], image
    cs = torch.clamp(s, 0, max_d) if max_d >= 0 else s
    wv = torch.where(s > 0, torch.ones_like(s), s) if validity is None else validity[:, None]
    ex = torch.exp(-(im[..., :-1] - im[..., 1:]).abs().mean(1, keepdim=True))
    ey = torch.exp(-(im[..., :-1, :] - im[..., 1:, :]).abs().mean(1, keepdim=True))
    l_sm = (ex * (d[..., :-1] - d[..., 1:]).abs()).mean() + (ey * (d[..., :-1, :] - d[..., 1:, :]).abs()).mean()
    l_sd = ((wv * (cs - d).abs()).sum((1, 2, 3)) / wv.sum((1, 2, 3))).mean()
    if emb is None:
        return w_sd * l_sd + w_sm * l_sm, l_sm, l_sd, torch.zeros((), dtype=torch.float64), 0.0
    en = emb / emb.norm(dim=-1, keepdim=True).clamp_min(EPS_NORM)
    rn = ref / ref.norm(dim=-1, keepdim=True).clamp_min(EPS_NORM)
    l_cos = (2 - 2 * (en * rn).sum(-1)).mean()
    wc = 0.0 if float(l_cos.detach()) < 0.3 else w_cos
    return w_sd * l_sd + w_sm * l_sm + wc * l_cos, l_sm, l_sd, l_cos, wc


def loss_ref(image, depth, sparse, validity, emb, ref, w3, max_d):
    """Values and gradients by autograd in float64, and their magnitudes.
    info [4] = (loss, l_sm, l_sd, l_cos); rowstats [R][3] = (max(|e|, eps), max(|r|, eps), cos); coef [3 + N] = (-2 w_cos' / R, w_sm / cnt_x,
    w_sm / cnt_y, w_sd / (N sum_w[n])); gdepth, gref.  Magnitudes: sums of absolute values through the same expressions, where
      a ratio num / den carries kappa = sum |w| / |sum w| of its denominator (negative validity weights cancel in it),
      an edge weight exp(-m) carries (1 + m): an error of the exponent is a relative error of the weight."""
    N, H, W = depth.shape
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, F64))
    d = t(depth).requires_grad_(True)
    r = None if ref is None else t(ref).requires_grad_(True)
    loss, l_sm, l_sd, l_cos, wc = adapt_loss64(t(image), d, t(sparse), t(validity), t(emb), r, w3, max_d)
    loss.backward()
    w_sd, w_sm, _ = (float(F32(v)) for v in w3)
    out = dict(info=np.array([float(v.detach()) for v in (loss, l_sm, l_sd, l_cos)]), gdepth=d.grad.numpy(), wc=wc)
    # magnitudes
    D, S, I = np.asarray(depth, F64), np.asarray(sparse, F64), np.asarray(image, F64)
    cs = np.clip(S, 0, max_d) if max_d >= 0 else S
    wv = np.where(S > 0, 1.0, S) if validity is None else np.asarray(validity, F64)
    num, den = (wv * np.abs(cs - D)).sum((1, 2)), wv.sum((1, 2))
    kappa = np.abs(wv).sum((1, 2)) / np.abs(den)
    mag_sd = ((np.abs(wv) * (np.abs(cs) + np.abs(D))).sum((1, 2)) / np.abs(den) + np.abs(num / den) * kappa).mean()
    mx, my = np.abs(I[..., :-1] - I[..., 1:]).mean(1), np.abs(I[..., :-1, :] - I[..., 1:, :]).mean(1)
    ex, ey = np.exp(-mx) * (1 + mx), np.exp(-my) * (1 + my)
    cntx, cnty = N * H * (W - 1), N * (H - 1) * W
    aD = np.abs(D)
    mag_sm = (ex * (aD[..., :-1] + aD[..., 1:])).sum() / cntx + (ey * (aD[..., :-1, :] + aD[..., 1:, :])).sum() / cnty
    sdn = w_sd / (N * den)
    coef = [0.0, w_sm / cntx, w_sm / cnty] + list(sdn)
    mag_coef = [0.0, abs(w_sm) / cntx, abs(w_sm) / cnty] + list(np.abs(sdn) * kappa)
    gx, gy = np.zeros_like(D), np.zeros_like(D)
    sx, sy = np.sign(D[..., :-1] - D[..., 1:]) != 0, np.sign(D[..., :-1, :] - D[..., 1:, :]) != 0
    gx[..., :-1] += ex * sx
    gx[..., 1:] += ex * sx
    gy[..., :-1, :] += ey * sy
    gy[..., 1:, :] += ey * sy
    out['mag_gdepth'] = (np.abs(sdn) * kappa)[:, None, None] * np.abs(wv) * (np.sign(D - cs) != 0) + abs(w_sm) / cntx * gx + abs(w_sm) / cnty * gy
    mag_cos = 0.0
    if emb is not None:
        E, Rf = np.asarray(emb, F64), np.asarray(ref, F64)
        R = E.shape[0]
        ne, nr = np.maximum(np.sqrt((E * E).sum(1)), EPS_NORM), np.maximum(np.sqrt((Rf * Rf).sum(1)), EPS_NORM)
        c, mc = (E * Rf).sum(1) / (ne * nr), (np.abs(E) * np.abs(Rf)).sum(1) / (ne * nr)
        out['rowstats'], out['mag_rowstats'] = np.stack([ne, nr, c], 1), np.stack([ne, nr, mc], 1)
        mag_cos = (2 + 2 * mc).mean()
        coef[0] = mag_coef[0] = -2.0 * wc / R
        out['gref'] = r.grad.numpy()
        proj = np.where(nr > EPS_NORM, mc, 0.0)
        out['mag_gref'] = abs(coef[0]) * (np.abs(E) / ne[:, None] + proj[:, None] * np.abs(Rf) / nr[:, None]) / nr[:, None]
    out['coef'], out['mag_coef'] = np.array(coef), np.abs(np.array(mag_coef))
    out['mag_info'] = np.array([abs(w_sd) * mag_sd + abs(w_sm) * mag_sm + abs(wc) * mag_cos, mag_sm, mag_sd, mag_cos])
    return out


LOSS_PB, LOSS_CB = 256, 1024           # csrc/loss.hip: depth-reduction blocks per sample, cosine-reduction blocks


def _wave_sum(v):
    """wave_sum: the xor butterfly over the last axis (64 lanes), float32"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lane ^ o]).astype(F32)
    return v[..., 0]


def _block_partials(t, nblocks):
    """t [plane] per-pixel terms -> [nblocks] block partials: grid-stride accumulation per thread, butterfly per wave, the four waves in order"""
    n = nblocks * 256
    it = -(-t.size // n)
    a = np.zeros(it * n, F32)
    a[:t.size] = t
    acc = np.zeros(n, F32)
    for k in range(it):
        acc = (acc + a[k * n:(k + 1) * n]).astype(F32)
    w = _wave_sum(acc.reshape(nblocks, 4, 64))
    return (((w[:, 0] + w[:, 1]).astype(F32) + w[:, 2]).astype(F32) + w[:, 3]).astype(F32)


def _edge32(I, axis):
    a, b = (I[..., :-1], I[..., 1:]) if axis == 'x' else (I[..., :-1, :], I[..., 1:, :])
    d = np.abs(a - b).astype(F32)
    m = (((d[:, 0] + d[:, 1]).astype(F32) + d[:, 2]).astype(F32) / F32(3)).astype(F32)
    return np.exp(-m).astype(F32)


def loss_emu(image, depth, sparse, validity, emb, ref, w3, max_d):
    """The kernels' order in float32 (partials per block, double-precision second stage as loss_finalize_block), same keys as loss_ref"""
    N, H, W = depth.shape
    D, S, I = np.asarray(depth, F32), np.asarray(sparse, F32), np.asarray(image, F32)
    w_sd, w_sm, w_cos = (F32(v) for v in w3)
    cs = clamp_ref(S, max_d)
    wv = np.where(S > 0, F32(1), S).astype(F32) if validity is None else np.asarray(validity, F32)
    ex, ey = _edge32(I, 'x'), _edge32(I, 'y')
    t0 = (wv * np.abs(cs - D)).astype(F32)
    t2, t3 = np.zeros_like(D), np.zeros_like(D)
    t2[..., :-1] = ex * np.abs(D[..., :-1] - D[..., 1:])
    t3[..., :-1, :] = ey * np.abs(D[..., :-1, :] - D[..., 1:, :])
    part = np.stack([np.stack([_block_partials(q[n].ravel(), LOSS_PB) for q in (t0, wv, t2, t3)], 1) for n in range(N)]).astype(F64)
    num, den, smx, smy = part[..., 0].sum(1), part[..., 1].sum(1), part[..., 2].sum(), part[..., 3].sum()
    l_sd = (num / den).sum() / N
    sdn = (float(w_sd) / (N * den)).astype(F32)
    cntx, cnty = float(N) * H * (W - 1), float(N) * (H - 1) * W
    l_sm = smx / cntx + smy / cnty
    cx, cy = F32(float(w_sm) / cntx), F32(float(w_sm) / cnty)
    l_cos, wc, coef0 = 0.0, w_cos, F32(0)
    out = {}
    if emb is not None:
        E, Rf = np.asarray(emb, F32), np.asarray(ref, F32)
        R, Dm = E.shape
        pad = (-Dm) % 256
        lanes = lambda a: np.pad(a, ((0, 0), (0, pad))).reshape(R, -1, 64, 4)          # [row][iteration][lane][4]

        def dot(a, b):
            acc = np.zeros((R, 64), F32)
            p = (lanes(a) * lanes(b)).astype(F32)
            for k in range(p.shape[1]):
                acc = (acc + (((p[:, k, :, 0] + p[:, k, :, 1]).astype(F32) + p[:, k, :, 2]).astype(F32) + p[:, k, :, 3]).astype(F32)).astype(F32)
            return _wave_sum(acc)
        ee, rr, er = dot(E, E), dot(Rf, Rf), dot(E, Rf)
        ne, nr = np.maximum(np.sqrt(ee), F32(1e-12)).astype(F32), np.maximum(np.sqrt(rr), F32(1e-12)).astype(F32)
        c = (er / (ne * nr).astype(F32)).astype(F32)
        out['rowstats'] = np.stack([ne, nr, c], 1)
        term = (F32(2) - (F32(2) * c).astype(F32)).astype(F32)
        n = LOSS_CB * 4
        it = -(-R // n)
        a = np.zeros(it * n, F32)
        a[:R] = term
        acc = np.zeros(n, F32)
        for k in range(it):
            acc = (acc + a[k * n:(k + 1) * n]).astype(F32)
        acc = acc.reshape(LOSS_CB, 4)
        cpart = (((acc[:, 0] + acc[:, 1]).astype(F32) + acc[:, 2]).astype(F32) + acc[:, 3]).astype(F32)
        l_cos = cpart.astype(F64).sum() / R
        if F32(l_cos) < F32(0.3):
            wc = F32(0)
        coef0 = F32(-2.0 * float(wc) / R)
        ie, ir = (F32(1) / ne).astype(F32), (F32(1) / nr).astype(F32)
        proj = np.where(nr > F32(1e-12), c, F32(0)).astype(F32)
        out['gref'] = (coef0 * ((E * ie[:, None]).astype(F32) - ((proj[:, None] * Rf).astype(F32) * ir[:, None]).astype(F32)).astype(F32) * ir[:, None]).astype(F32)
    else:
        wc = F32(0)
    out['wc'] = float(wc)
    out['info'] = np.array([float(w_sd) * l_sd + float(w_sm) * l_sm + float(wc) * l_cos, l_sm, l_sd, l_cos]).astype(F32)
    out['coef'] = np.concatenate([[coef0, cx, cy], sdn]).astype(F32)
    sgn = lambda v: np.sign(v).astype(F32)
    v = ((sdn[:, None, None] * wv).astype(F32) * sgn(D - cs)).astype(F32)
    tx, ty = np.zeros_like(D), np.zeros_like(D)
    tx[..., :-1] = (ex * sgn(D[..., :-1] - D[..., 1:])).astype(F32)
    tx[..., 1:] = (tx[..., 1:] - (ex * sgn(D[..., :-1] - D[..., 1:])).astype(F32)).astype(F32)
    ty[..., :-1, :] = (ey * sgn(D[..., :-1, :] - D[..., 1:, :])).astype(F32)
    ty[..., 1:, :] = (ty[..., 1:, :] - (ey * sgn(D[..., :-1, :] - D[..., 1:, :])).astype(F32)).astype(F32)
    out['gdepth'] = ((v + (cx * tx).astype(F32)).astype(F32) + (cy * ty).astype(F32)).astype(F32)
    return out
