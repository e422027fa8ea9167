"""The update half of a step on the CPU (test infrastructure): weight gradients and the optimizer in plain float64, the magnitudes the
per-element bounds scale with, and an fp32 emulation of each operation -- the same operation run in numpy float32 in the kernel's order of
chunks and slices, a matrix-core step modelled as exact products and one rounding of the accumulator (two for the fp32 step: a model, the
instructions' inner roundings are not documented), for the bf16x3 kernels with the three-product split hi*hi + hi*lo + lo*hi.  Nothing from the library takes part.

conv weight gradient   dW[co][ci][ky][kx] = sum_{b,y,x} gy[b][y][x][co] x[b][y+ky-1][x+kx-1][ci] (zero padding), db[co] = sum gy: NHWC maps
                       (csrc/wgrad_adam.hip wgrad32_kernel, csrc/gwgrad_mfma.hip)
Linear weight gradient dW[o][i] = sum_r G'[r][o] X'[r][i], db[o] = sum_r G'[r][o] with the two prologues of csrc/head_train.hip:
                       G' = gscale (G - c1 - (Gh - mean) inv c2) (BatchNorm backward), X' = relu(X xscale + xshift)
Adam                   torch.optim.Adam's single-tensor update as csrc/ptta_kernels.h ptta_adam_update spells it; `rep` updates with one
                       gradient at the step counts (t - 1) rep + 1 .. t rep
EMA                    target = target tau + online (1 - tau)

A magnitude is the float64 sum of the absolute values of the element's terms; where a term is itself a sum (a prologue, Adam's moments
inside the parameter update) its own magnitude is carried through, to first order."""
import numpy as np
import torch

F32, F64 = np.float32, np.float64
U = 2.0 ** -24


# ---- bf16 split (csrc/ptta_common.h split8: hi = RNE(v), lo = RNE(v - hi)) ----------------------------------------------------------------
def bf16_bits(x):
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    return np.where(nan, (u >> 16) | 0x40, (u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_val(bits):
    return (np.asarray(bits).astype(np.uint16).astype(np.uint32) << 16).view(F32)


def through_bf16(x32):
    return bf16_val(bf16_bits(x32))


def split2(x32):
    x32 = np.asarray(x32, F32)
    hi = through_bf16(x32)
    return hi, through_bf16(x32 - hi)


def fma32(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


# ---- conv weight gradient -----------------------------------------------------------------------------------------------------------------
def _conv_w(x, gy):
    """torch.nn.grad.conv2d_weight of NHWC arrays in their own dtype -> (gw [co][ci][3][3], gb [co]: the pixels added one after the other)"""
    xt, gt = torch.from_numpy(np.array(x)).permute(0, 3, 1, 2), torch.from_numpy(np.array(gy)).permute(0, 3, 1, 2)
    gw = torch.nn.grad.conv2d_weight(xt, (gt.shape[1], xt.shape[1], 3, 3), gt, padding=1)
    return gw.numpy(), np.add.reduce(np.asarray(gy).reshape(-1, np.shape(gy)[-1]), 0)


def conv_wgrad_ref(x, gy):
    """float64 reference and magnitudes: ((gw, gb), (the same on |x| and |gy|))"""
    x, gy = np.asarray(x, F64), np.asarray(gy, F64)
    return _conv_w(x, gy), _conv_w(np.abs(x), np.abs(gy))


def mma(acc, a, b):
    """one matrix-core step in float32: acc + a^T b over the leading axis of a [.., k, m] and b [.., k, n], the k products exact (float64
    holds a product of two fp32 values), ONE rounding of the accumulator"""
    return (acc.astype(F64) + np.swapaxes(np.asarray(a, F64), -1, -2) @ np.asarray(b, F64)).astype(F32)


def _taps(x):
    """[b][h][w][c] -> [9][b][h][w][c]: the zero-padded map shifted by (ky - 1, kx - 1), tap = 3 ky + kx"""
    b, h, w, c = x.shape
    xp = np.zeros((b, h + 2, w + 2, c), x.dtype)
    xp[:, 1:-1, 1:-1] = x
    return np.stack([xp[:, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)])


def wgrad32_chunks(pixels):
    """(chunks, pixels per chunk) of ptta_launch_wgrad32: at most 512 chunks of a multiple of 8 pixels"""
    n = min(512, max(1, (pixels + 63) // 64))
    return n, ((pixels + n - 1) // n + 7) & ~7


def wgrad32_emu(x, gy):
    """wgrad32_kernel + wgrad32_reduce_kernel in float32: per chunk the pixels in order, the accumulator rounded after every product (the
    two products of a 32x32x2 fp32 matrix-core step modelled as two chained fused multiply-adds: what the instruction rounds inside is not
    documented, so this approximates it), then the chunks c, c + 8, ... added in order per group and the eight groups in the reducer's tree"""
    x, gy = np.asarray(x, F32), np.asarray(gy, F32)
    P = x.shape[0] * x.shape[1] * x.shape[2]
    n, per = wgrad32_chunks(P)
    g = np.zeros((n * per, 32), F32)
    g[:P] = gy.reshape(P, 32)
    t = np.zeros((9, n * per, 32), F32)
    t[:, :P] = _taps(x).reshape(9, P, 32)
    g, t = g.reshape(n, 1, per, 32), t.reshape(9, n, per, 32).transpose(1, 0, 2, 3)
    acc, bacc = np.zeros((n, 9, 32, 32), F32), np.zeros((n, 32), F32)
    for s in range(per):
        acc = mma(acc, g[:, :, s:s + 1], t[:, :, s:s + 1])
        bacc = bacc + g[:, 0, s]

    def reduce(part):
        grp = []
        for cg in range(8):
            s = np.zeros(part.shape[1:], F32)
            for c in range(cg, n, 8):
                s = s + part[c]
            grp.append(s)
        return ((grp[0] + grp[1]) + (grp[2] + grp[3])) + ((grp[4] + grp[5]) + (grp[6] + grp[7]))
    return reduce(acc).transpose(1, 2, 0).reshape(32, 32, 3, 3), reduce(bacc)


def gwgrad_x3_emu(x, gy):
    """The bf16x3 weight gradient (gwgrad_x3_kernel) in float32: both operands split (hi = RNE(v), lo = RNE(v - hi)), per 16 pixels of a row
    and tap the three matrix-core steps gy_lo x_hi, gy_hi x_lo, gy_hi x_hi with one accumulator rounding each, the items of the map in
    order into one accumulator (the longest chain any grid can have); the bias: the fp32 values added pixel by pixel"""
    x, gy = np.asarray(x, F32), np.asarray(gy, F32)
    b, h, w, ci = x.shape
    co = gy.shape[3]
    (xh, xl), (gh, gl) = split2(x), split2(gy)
    th, tl = _taps(xh), _taps(xl)
    acc = np.zeros((9, co, ci), F32)
    for ib in range(b):
        for y in range(h):
            for x0 in range(0, w, 16):
                sl = (ib, y, slice(x0, x0 + 16))
                for ga, xb in ((gl, th), (gh, tl), (gh, th)):
                    acc = mma(acc, ga[sl][None], xb[(slice(None),) + sl])
    return acc.transpose(1, 2, 0).reshape(co, ci, 3, 3), np.add.reduce(gy.reshape(-1, co), 0)


# ---- Linear weight gradient with the two prologues ------------------------------------------------------------------------------------------
def bn_backward_tables(G, Gh, gamma, eps=1e-5):
    """The per-column constants of the BatchNorm-backward transform from a batch: dH = gscale (G - c1 - xhat c2), xhat = (Gh - mean) inv,
    c1 = mean(G), c2 = mean(G xhat), gscale = gamma inv -- as fp32 tables (what the device holds)"""
    G, Gh = np.asarray(G, F64), np.asarray(Gh, F64)
    mean, var = Gh.mean(0), Gh.var(0)
    inv = 1.0 / np.sqrt(var + eps)
    xh = (Gh - mean) * inv
    return dict(gscale=(np.asarray(gamma, F64) * inv).astype(F32), gc1=G.mean(0).astype(F32), gc2=(G * xh).mean(0).astype(F32),
                gmean=mean.astype(F32), ginv=inv.astype(F32))


def linear_operands_ref(G, X, Gh=None, gt=None, xscale=None, xshift=None):
    """float64 G', X' and their magnitudes (the sum of the absolute addends of each prologue; |value| without one)"""
    G, X = np.asarray(G, F64), np.asarray(X, F64)
    g, gm = G, np.abs(G)
    if Gh is not None:
        gs, c1, c2, mu, iv = (np.asarray(gt[k], F64) for k in ('gscale', 'gc1', 'gc2', 'gmean', 'ginv'))
        Gh = np.asarray(Gh, F64)
        g = gs * (G - c1 - (Gh - mu) * iv * c2)
        gm = np.abs(gs) * (np.abs(G) + np.abs(c1) + (np.abs(Gh) + np.abs(mu)) * np.abs(iv * c2))
    x, xm = X, np.abs(X)
    if xscale is not None:
        xs, xsh = np.asarray(xscale, F64), np.asarray(xshift, F64)
        x = np.maximum(X * xs + xsh, 0.0)
        xm = np.abs(X * xs) + np.abs(xsh)
    return g, gm, x, xm


def linear_wgrad_ref(G, X, Gh=None, gt=None, xscale=None, xshift=None):
    """((dW [O][I], db [O]), (their magnitudes)) in float64"""
    g, gm, x, xm = linear_operands_ref(G, X, Gh, gt, xscale, xshift)
    return (g.T @ x, g.sum(0)), (gm.T @ xm, gm.sum(0))


def linear_wgrad_chunks(R):
    """(chunks, rows per chunk) of ptta_linear_wgrad_chunks: 512-row chunks, at most 64 of them"""
    rc = 512
    if (R + rc - 1) // rc > 64:
        rc = ((R + 63) // 64 + 15) // 16 * 16
    return (R + rc - 1) // rc, rc


def linear_wgrad_emu(G, X, Gh=None, gt=None, xscale=None, xshift=None):
    """linear_wgrad_kernel + wgrad_reduce_kernel in float32: the prologues in the kernel's order of operations, both operands split, per
    row chunk the 16-row slices in order with the three matrix-core steps g_lo x_hi, g_hi x_lo, g_hi x_hi (one accumulator rounding each),
    the bias as the two 8-row halves of every slice added value by value and then to each other, the chunks added in order"""
    g, x = np.asarray(G, F32), np.asarray(X, F32)
    if Gh is not None:
        gs, c1, c2, mu, iv = (np.asarray(gt[k], F32) for k in ('gscale', 'gc1', 'gc2', 'gmean', 'ginv'))
        g = gs * (g - c1 - (np.asarray(Gh, F32) - mu) * iv * c2)
    if xscale is not None:
        x = np.maximum(fma32(x, xscale, xshift), F32(0))
    R, O, I = g.shape[0], g.shape[1], x.shape[1]
    n, rc = linear_wgrad_chunks(R)
    rows = min(rc, (R + 15) // 16 * 16)                     # (the slices past the last row add zeros)

    def chunked(a):
        out = np.zeros((n * rc, a.shape[1]), F32)
        out[:R] = a
        return out.reshape(n, rc, a.shape[1])[:, :rows]
    gc = chunked(g)
    (gh, gl), (xh, xl) = split2(gc), split2(chunked(x))
    acc, bs = np.zeros((n, O, I), F32), np.zeros((n, 2, O), F32)
    for s in range(0, rows, 16):
        for ga, xb in ((gl, xh), (gh, xl), (gh, xh)):
            acc = mma(acc, ga[:, s:s + 16], xb[:, s:s + 16])
        for j in range(8):
            bs = bs + np.stack([gc[:, s + j], gc[:, s + 8 + j]], 1)
    wp, bp = acc, bs[:, 0] + bs[:, 1]
    dW, db = np.zeros((O, I), F32), np.zeros(O, F32)
    for k in range(n):
        dW, db = dW + wp[k], db + bp[k]
    return dW, db


def glinear_wgrad_emu(x, gy):
    """glinear_wgrad_kernel in float32: rows in order, acc = fma(gy, x, acc), the bias a plain running sum"""
    x, gy = np.asarray(x, F32), np.asarray(gy, F32)
    acc, b = np.zeros((gy.shape[1], x.shape[1]), F32), np.zeros(gy.shape[1], F32)
    for r in range(x.shape[0]):
        acc, b = fma32(gy[r][:, None], x[r][None, :], acc), b + gy[r]
    return acc, b


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------------
def hyper32(lr, b1, b2, eps, wd):
    """the hyper-parameter block as the device holds it: five fp32 values"""
    return np.array([lr, b1, b2, eps, wd], F32)


def adam_ref(p, m, v, g, hyper, t, rep=1):
    """float64 Adam from fp32 inputs and the fp32 hyper-parameters widened; t = the step count of THIS update (1 for the first); `rep`
    consecutive updates with the same gradient at the counts (t - 1) rep + 1 .. t rep.  -> ((p, m, v), (magnitudes))"""
    lr, b1, b2, eps, wd = (float(h) for h in np.asarray(hyper, F32))
    p, m, v, g = (np.asarray(a, F64).copy() for a in (p, m, v, g))
    pm, mm, vm = np.abs(p), np.abs(m), np.abs(v)
    for r in range(rep):
        tt = (t - 1) * rep + r + 1
        gg, ggm = g + wd * p, np.abs(g) + abs(wd) * pm
        m, mm = b1 * m + (1.0 - b1) * gg, b1 * mm + (1.0 - b1) * ggm
        v, vm = b2 * v + (1.0 - b2) * gg * gg, b2 * vm + (1.0 - b2) * ggm * ggm
        step, den = lr / (1.0 - b1 ** tt), np.sqrt(v) / np.sqrt(1.0 - b2 ** tt) + eps
        p, pm = p - step * (m / den), pm + step * (mm / den)
    return (p, m, v), (pm, mm, vm)


def adam_emu(p, m, v, g, hyper, t, rep=1):
    """ptta_adam_update in numpy.float32, operation by operation: gg = fma(wd, p, g) (wd != 0); m = fma(b1, m, (1 - b1) gg);
    v = fma(b2, v, ((1 - b2) gg) gg); p = p - step_size (m / (sqrt(v) / bc2s + eps)); bias corrections in double, rounded once"""
    lr, b1, b2, eps, wd = np.asarray(hyper, F32)
    p, m, v, g = (np.asarray(a, F32).copy() for a in (p, m, v, g))
    for r in range(rep):
        tt = (t - 1) * rep + r + 1
        step = F32(float(lr) / (1.0 - float(b1) ** tt))
        bc2s = F32(np.sqrt(1.0 - float(b2) ** tt))
        gg = fma32(wd, p, g) if wd != 0 else g
        m = fma32(b1, m, (F32(1) - b1) * gg)
        v = fma32(b2, v, ((F32(1) - b2) * gg) * gg)
        p = p - step * (m / (np.sqrt(v) / bc2s + eps))
    return p, m, v


def ema32(p, g, tau, omt):
    """fl(fl(p tau) + fl(g omt)) in numpy.float32: ema_multi_kernel's own roundings, so equality is the bound"""
    p, g = np.asarray(p, F32), np.asarray(g, F32)
    return (p * F32(tau)) + (g * F32(omt))


def ema_ref(p, g, tau):
    return float(tau) * np.asarray(p, F64) + (1.0 - float(tau)) * np.asarray(g, F64)
