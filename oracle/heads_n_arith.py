"""The narrow heads of the mixed mode (csrc/heads_n.hip) and head_bwd_finish (csrc/heads_bn.hip) on the CPU (test infrastructure): plain
numpy references of every prologue, epilogue and layout, in float64 with a rounding only where the kernel stores or feeds a narrow value
(operands and outputs to bf16, round to nearest even); an fp32 emulation at the kernel's rounding points where a bound is needed; and the
magnitudes the per-element bounds scale with.  Nothing from the library takes part.

A GEMM is C[r][n] = sum_k A[r][k] W[n][k] (+ bias[n]) with K = N = 512.  The A operand comes from a prologue:
  PRO 1  relu(a scale[k] + shift[k])                    PRO 4  coef (e / |e| - cos r / |r|) / |r| (cos_grad_elem)
  PRO 3  relu((x W0^T + b0) scale + shift)              PRO 5  an fp32 tensor, rounded
and the accumulator goes to an epilogue:
  EPI 0  C = acc + bias, stored bf16                    EPI 1  + per 128-row block column sums of v and v^2 (fp32 values, rows < R)
  EPI 2  + rs[r] = sum_n (stored C)^2                   EPI 5  + (|e|, |c|, cos) per row against E and block partials of sum (2 - 2 cos)
  EPI 3  the data gradient through proj.1's BatchNorm and ReLU and proj.0: mask from the recomputed hidden, two column sums, P [R][32].
Tiled layout of a narrow [R][512] tensor: T[r / 128][k / 32][r % 128][k % 32]; packed weight: Wsl[k / 32][n][8 (c ^ ((n >> 2) & 3)) + k % 8],
c = (k % 32) / 8."""
import numpy as np

F32, F64 = np.float32, np.float64
BM = 128
FLOOR = float(F32(1e-12))
BN_EPS = float(F32(1e-5))
MOMENTUM = float(F32(0.1))
NAN_BITS = 0x7fc0


# ---- bf16 -------------------------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """fp32 -> bf16 bit patterns (uint16), round to nearest even, a NaN kept a NaN: f2bf of csrc/ptta_common.h"""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    return np.where(nan, (u >> 16) | 0x40, (u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_val(bits):
    return (np.asarray(bits).astype(np.uint16).astype(np.uint32) << 16).view(F32)


def round_bf16(x):
    """float64 -> the nearest bf16 value (ties to even) as float64, in one rounding (normal range)"""
    m, e = np.frexp(np.asarray(x, F64))
    return np.ldexp(np.rint(np.ldexp(m, 8)), e - 8)


def ulp_bf16(x):
    m, e = np.frexp(np.asarray(x, F64))
    return np.where(m == 0, 0.0, np.ldexp(1.0, e - 8))


def through_bf16(x32):
    """fp32 -> bf16 -> fp32: what a narrow store keeps"""
    return bf16_val(bf16_bits(x32))


def identity(x):
    return np.asarray(x, F64)


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------
def row_blocks(R):
    return (R + BM - 1) // BM


def tiled_elems(R):
    return row_blocks(R) * BM * 512


def tile(bits, R, pad=NAN_BITS):
    """[R][512] bf16 bit patterns -> the tiled buffer (int16, flat), the padding rows of the last block filled with `pad`"""
    nb = row_blocks(R)
    full = np.full((nb * BM, 512), pad, np.uint16)
    full[:R] = bits
    return np.ascontiguousarray(full.reshape(nb, BM, 16, 32).transpose(0, 2, 1, 3)).reshape(-1).view(np.int16)


def untile(t, R):
    """the tiled buffer -> [blocks * 128][512] bit patterns (uint16), padding rows included"""
    nb = row_blocks(R)
    return np.ascontiguousarray(np.asarray(t).view(np.uint16).reshape(nb, 16, BM, 32).transpose(0, 2, 1, 3)).reshape(nb * BM, 512)


def _pack_index():
    n, k = np.arange(512)[:, None], np.arange(512)[None, :]
    cs = ((k & 31) >> 3) ^ ((n >> 2) & 3)
    return (k >> 5) + 0 * n, n + 0 * k, 8 * cs + (k & 7)


def pack_w(bits):
    """[512 n][512 k] bit patterns -> the slice-major swizzled image [16][512][32] (hn_pack_w_kernel)"""
    out = np.zeros((16, 512, 32), np.uint16)
    out[_pack_index()] = bits
    return out


def unpack_w(image):
    return np.asarray(image).view(np.uint16).reshape(16, 512, 32)[_pack_index()]


# ---- prologues (float64; `rnd` = round_bf16, or identity for the check against torch) ---------------------------------------------------------
def pro1_ref(a, scale, shift, rnd=round_bf16):
    return rnd(np.maximum(a * scale.astype(F64) + shift.astype(F64), 0.0))


def hidden_ref(x, w0, b0):
    """h = x W0^T + b0 from the operands the matrix cores see (x, W0 already bf16 values) and its magnitude"""
    x, w0, b0 = np.asarray(x, F64), np.asarray(w0, F64), np.asarray(b0, F64)
    return x @ w0.T + b0, np.abs(x) @ np.abs(w0).T + np.abs(b0)


def pro3_ref(x, w0, b0, scale, shift, rnd=round_bf16):
    h, _ = hidden_ref(x, w0, b0)
    return rnd(np.maximum(h * scale.astype(F64) + shift.astype(F64), 0.0))


def pro4_ref(e, r, rowstats, coef, rnd=round_bf16):
    """cos_grad_elem: coef (e ie - proj r ir) ir, ie = 1 / |e|, ir = 1 / |r|, proj = cos where |r| > 1e-12 (rowstats [R][3] fp32)"""
    ne, nr, cc = (rowstats[:, j].astype(F64)[:, None] for j in range(3))
    ie, ir = 1.0 / ne, 1.0 / nr
    pj = np.where(rowstats[:, 1:2] > F32(1e-12), cc, 0.0)
    return rnd(float(coef) * (e * ie - pj * r * ir) * ir)


def pro5_ref(af, rnd=round_bf16):
    return rnd(np.asarray(af, F64))


def gemm_ref(A, w):
    """acc = A W^T and sum |a| |w| (W [n][k] already bf16 values)"""
    w = np.asarray(w, F64)
    return A @ w.T, np.abs(A) @ np.abs(w).T


# ---- epilogues --------------------------------------------------------------------------------------------------------------------------
def _blocks(a, R, fill=0.0):
    """[R][...] -> [blocks][128][...], the rows from R on = fill"""
    nb = row_blocks(R)
    out = np.full((nb * BM,) + a.shape[1:], fill, a.dtype)
    out[:R] = a
    return out.reshape((nb, BM) + a.shape[1:])


def epi0_ref(acc, mag, bias):
    """v = acc + bias (the kernel stores its bf16 rounding), magnitude sum |a||w| + |bias| + one bf16 ulp of v"""
    b = 0.0 if bias is None else np.asarray(bias, F64)
    v = acc + b
    return v, mag + np.abs(b) + ulp_bf16(v)


def epi1_ref(v, vmag, R):
    """part [blocks][2][512]: column sums of v and v^2 over the block's rows below R"""
    part = np.stack([_blocks(v, R).sum(1), (_blocks(v, R) ** 2).sum(1)], 1)
    return part, np.stack([_blocks(vmag, R).sum(1), (_blocks(vmag, R) ** 2).sum(1)], 1)


def epi2_ref(stored):
    """rs[r] = sum_n c^2 of the STORED values (float64 of the bf16 values)"""
    rs = (np.asarray(stored, F64) ** 2).sum(1)
    return rs, rs


def epi5_ref(stored, e, rs, R, cpart_n):
    """rowstats [R][3] = (|e|, |c|, cos) and cpart from the stored C, the given E (bf16 values) and rs (fp32), with their magnitudes"""
    c, e = np.asarray(stored, F64), np.asarray(e, F64)
    cc, ce, ace = (c * c).sum(1), (c * e).sum(1), np.abs(c * e).sum(1)
    ne, nr = np.maximum(np.sqrt(np.asarray(rs, F64)), FLOOR), np.maximum(np.sqrt(cc), FLOOR)
    cs = ce / (ne * nr)
    smag = ace / (ne * nr)
    stats, mag = np.stack([ne, nr, cs], 1), np.stack([ne, nr, smag], 1)
    cpart, cmag = np.zeros(cpart_n), np.zeros(cpart_n)
    nb = row_blocks(R)
    cpart[:nb], cmag[:nb] = _blocks(2.0 - 2.0 * cs, R).sum(1), _blocks(2.0 + 2.0 * smag, R).sum(1)
    return dict(stats=stats, cpart=cpart, cc=cc, ce=ce), dict(stats=mag, cpart=cmag)


def epi3_ref(acc, mag, x, w0, b0, escale, eshift, emean, einv, w0t, R, rnd=round_bf16):
    """The ReLU mask from the recomputed hidden, part [blocks][2][512] = (sum g, sum g xhat) over rows < R, P = rnd(g escale) W0t^T [R][32];
    `pre` / `premag`: the mask's pre-activation and its magnitude; gmag: |acc| where masked in, what an ambiguous element moves."""
    esc, esh, emu, eiv = (np.asarray(t, F64) for t in (escale, eshift, emean, einv))
    h, hmag = hidden_ref(x, w0, b0)
    pre, premag = h * esc + esh, hmag * np.abs(esc) + np.abs(esh)
    on = pre > 0
    g, gm = np.where(on, acc, 0.0), np.where(on, mag, 0.0)
    xh = (h - emu) * eiv
    part = np.stack([_blocks(g, R).sum(1), _blocks(g * xh, R).sum(1)], 1)
    pmag = np.stack([_blocks(gm, R).sum(1), _blocks((gm * np.abs(h - emu) + np.abs(g) * (hmag + np.abs(emu))) * np.abs(eiv), R).sum(1)], 1)
    w0t = np.asarray(w0t, F64)
    dy = rnd(g * esc)
    return (dict(part=part, P=dy @ w0t.T, pre=pre, h=h, xh=xh, dy=dy),
            dict(part=pmag, P=(gm * np.abs(esc)) @ np.abs(w0t).T, pre=premag))


def epi3_widen(acc, ref, mag, band, escale, w0t, R):
    """What the elements whose pre-activation lies within band x its magnitude of zero may move: (count mask, d part [blocks][2][512], d P [R][32])"""
    amb = np.abs(ref['pre']) <= band * mag['pre']
    a = np.where(amb, np.abs(acc), 0.0)
    return amb, np.stack([_blocks(a, R).sum(1), _blocks(a * np.abs(ref['xh']), R).sum(1)], 1), (a * np.abs(np.asarray(escale, F64))) @ np.abs(np.asarray(w0t, F64)).T


# ---- the fp32 emulation -----------------------------------------------------------------------------------------------------------------
def f32(x):
    return np.asarray(x, F64).astype(F32)


def fma32(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def mfma_chain(acc, A, B, step=4):
    """acc + A B^T with exact products and one fp32 rounding of the accumulator per `step` products (the finest grain a matrix-core
    instruction of 16 products can have), K in order"""
    A, B = np.asarray(A, F64), np.asarray(B, F64)
    acc = np.broadcast_to(np.asarray(acc, F32), (A.shape[0], B.shape[0])).astype(F32)
    for k in range(0, A.shape[1], step):
        acc = (acc.astype(F64) + A[:, k:k + step] @ B[:, k:k + step].T).astype(F32)
    return acc


def hidden_emu(x, w0, b0):
    """two accumulation chains as the kernel has them: channels 0-15 seeded with b0, channels 16-31 from zero, then one addition"""
    ha = mfma_chain(np.asarray(b0, F32)[None, :], x[:, :16], w0[:, :16])
    hb = mfma_chain(F32(0), x[:, 16:], w0[:, 16:])
    return ha + hb


def pro1_emu(a, scale, shift):
    return through_bf16(np.maximum(fma32(a, scale, shift), F32(0)))


def pro3_emu(x, w0, b0, scale, shift):
    return through_bf16(np.maximum(fma32(hidden_emu(x, w0, b0), scale, shift), F32(0)))


def pro4_emu(e, r, rowstats, coef):
    ne, nr, cc = (rowstats[:, j:j + 1].astype(F32) for j in range(3))
    ie, ir = F32(1) / ne, F32(1) / nr
    pj = np.where(nr > F32(1e-12), cc, F32(0))
    e, r = np.asarray(e, F32), np.asarray(r, F32)
    return through_bf16(F32(coef) * (e * ie - pj * r * ir) * ir)


def pro5_emu(af):
    return through_bf16(np.asarray(af, F32))


def _lane_rows():
    """the rows of a 128-row block in the order a lane half adds them: [h][64]"""
    return np.array([[32 * a + (r & 3) + 8 * (r >> 2) + 4 * h for a in range(4) for r in range(16)] for h in range(2)])


def _colsum_emu(terms, R):
    """column sums over the rows below R of every block, sequential per lane half in fp32, the two halves added: terms = [(a, b)] -> sum of
    fma(a, b, .) (b None: plain addition)"""
    nb = row_blocks(R)
    tb = [(_blocks(np.asarray(a, F32), R), None if b is None else _blocks(np.asarray(b, F32), R)) for a, b in terms]
    ok = _blocks(np.ones(R, bool), R, False)
    out = []
    for a, b in tb:
        halves = []
        for h in range(2):
            s = np.zeros((nb, a.shape[2]), F32)
            for row in _lane_rows()[h]:
                t = (s + a[:, row]) if b is None else fma32(a[:, row], b[:, row], s)
                s = np.where(ok[:, row, None], t, s)
            halves.append(s)
        out.append(halves[0] + halves[1])
    return np.stack(out, 1)


def epi01_emu(acc, bias, R, stats):
    v = acc if bias is None else acc + np.asarray(bias, F32)
    return v, (_colsum_emu([(v, None), (v, v)], R) if stats else None)


def _tree(x):
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def _rowsum_emu(a, b):
    """sum_n a b per row as EPI 2 / 5 add it: four columns in one fp32 expression, the lane's two column tiles, a tree over the eight lanes
    of a row, the eight waves in order"""
    p = (np.asarray(a, F32) * np.asarray(b, F32)).reshape(a.shape[0], 8, 2, 8, 4)
    q = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]
    w = _tree(q[:, :, 0] + q[:, :, 1])
    s = np.zeros(a.shape[0], F32)
    for k in range(8):
        s = s + w[:, k]
    return s


def epi2_emu(stored):
    return _rowsum_emu(stored, stored)


def epi5_emu(stored, e, rs, R, cpart_n):
    cc, ce = _rowsum_emu(stored, stored), _rowsum_emu(stored, e)
    ne, nr = np.maximum(np.sqrt(np.asarray(rs, F32)), F32(1e-12)), np.maximum(np.sqrt(cc), F32(1e-12))
    cs = ce / (ne * nr)
    term = _blocks(F32(2) - F32(2) * cs, R).reshape(row_blocks(R), 2, 64)
    cpart = np.zeros(cpart_n, F32)
    cpart[:row_blocks(R)] = _tree(term)[:, 0] + _tree(term)[:, 1]
    return np.stack([ne, nr, cs], 1), cpart


def epi3_emu(acc, x, w0, b0, escale, eshift, emean, einv, w0t, R):
    esc, esh, emu, eiv = (np.asarray(t, F32) for t in (escale, eshift, emean, einv))
    h = hidden_emu(x, w0, b0)
    v = np.where(fma32(h, esc, esh) > 0, acc, F32(0))
    part = _colsum_emu([(v, None), (v * (h - emu), np.broadcast_to(eiv, v.shape))], R)
    dy = through_bf16(v * esc)
    P = mfma_chain(F32(0), dy[:, :256], np.asarray(w0t)[:, :256]) + mfma_chain(F32(0), dy[:, 256:], np.asarray(w0t)[:, 256:])
    return part, P


# ---- the moments chain ------------------------------------------------------------------------------------------------------------------
def moments_ref(x, w0, b0):
    """mean and biased variance of h = x W0^T + b0 straight from h in float64 (x as the kernel reads it: fp32 or bf16 values; W0 fp32), and
    the magnitudes: of the mean sum |w| E|x| + |b|, of the variance V = sum_ab |w_a| |w_b| (E|x_a x_b| + |m_a| |m_b|) -- what
    C = S / n - m m^T cancels from"""
    x, w0, b0 = np.asarray(x, F64), np.asarray(w0, F64), np.asarray(b0, F64)
    n = x.shape[0]
    mean = np.zeros(512)
    for r in range(0, n, 8192):
        mean += (x[r:r + 8192] @ w0.T + b0).sum(0)
    mean /= n
    var = np.zeros(512)
    for r in range(0, n, 8192):
        var += ((x[r:r + 8192] @ w0.T + b0 - mean) ** 2).sum(0)
    var /= n
    ax, m = np.abs(x), np.abs(x.mean(0))
    aw = np.abs(w0)
    V = np.einsum('ja,ab,jb->j', aw, ax.T @ ax / n + np.outer(m, m), aw)
    return dict(mean=mean, var=var, n=n), dict(mean=aw @ ax.mean(0) + np.abs(b0), var=V)


def moments_part_ref(mom, mag):
    """[2][512] = (sum h, sum h^2) = (n mean, n (var + mean^2)): what value + remainder of `part` add up to"""
    n = mom['n']
    return np.stack([n * mom['mean'], n * (mom['var'] + mom['mean'] ** 2)]), np.stack([n * mag['mean'], n * (mag['var'] + mag['mean'] ** 2)])


def moments_bn_ref(mom, mag, gamma, beta, rm=None, rv=None, eps=BN_EPS, momentum=MOMENTUM):
    """the BatchNorm1d state: inv = 1 / sqrt(var + eps), scale = gamma inv, shift = beta - mean scale, running statistics with the unbiased
    variance (n = 1: the biased one, nothing divided by zero)"""
    n, mean, var = mom['n'], mom['mean'], mom['var']
    g, b = np.asarray(gamma, F64), np.asarray(beta, F64)
    inv = 1.0 / np.sqrt(var + eps)
    imag = 0.5 * inv ** 3 * mag['var'] + inv
    scale, smag = g * inv, np.abs(g) * imag
    out = dict(mean=mean, inv=inv, scale=scale, shift=b - mean * scale)
    m = dict(mean=mag['mean'], inv=imag, scale=smag, shift=np.abs(b) + mag['mean'] * np.abs(scale) + np.abs(mean) * smag)
    if rm is not None:
        f = n / (n - 1.0) if n > 1 else 1.0
        out.update(rm=(1.0 - momentum) * np.asarray(rm, F64) + momentum * mean, rv=(1.0 - momentum) * np.asarray(rv, F64) + momentum * var * f)
        m.update(rm=(1.0 - momentum) * np.abs(rm) + momentum * mag['mean'], rv=(1.0 - momentum) * np.abs(rv) + momentum * mag['var'] * f)
    return out, m


def moments_emu(x, w0, b0):
    """fp32 products summed in fp32 over the 128 rows of a block, float64 across blocks, the covariance rounded to fp32 after the
    subtraction, w . m and w^T C w in fp32 in the kernel's order -> (mean float64, variance float64 clamped at 0, n)"""
    x, w = np.asarray(x, F32), np.asarray(w0, F32)
    n = x.shape[0]
    nb = (n + 127) // 128
    xs = np.zeros((nb * 128, 32), F32)
    xs[:n] = x
    xs = xs.reshape(nb, 128, 32)
    f, fs = np.zeros((nb, 32, 32), F32), np.zeros((nb, 32), F32)
    for r in range(128):
        f = fma32(xs[:, r, :, None], xs[:, r, None, :], f)
        fs = fs + xs[:, r]
    S, s = f.astype(F64).sum(0), fs.astype(F64).sum(0)
    m = s / n
    Cf, mf = (S / n - np.outer(m, m)).astype(F32), m.astype(F32)
    wm, var = [], []
    for hf in range(2):
        a_wm, a_var = np.zeros(512, F32), np.zeros(512, F32)
        for a in range(16 * hf, 16 * hf + 16):
            a_wm = fma32(w[:, a], mf[a], a_wm)
            r4 = [np.zeros(512, F32) for _ in range(4)]
            for q in range(8):
                for i in range(4):
                    r4[i] = fma32(Cf[a, 4 * q + i], w[:, 4 * q + i], r4[i])
            a_var = fma32(w[:, a], (r4[0] + r4[1]) + (r4[2] + r4[3]), a_var)
        wm.append(a_wm)
        var.append(a_var)
    v = var[0] + var[1]
    return dict(mean=(wm[0] + wm[1]).astype(F64) + np.asarray(b0, F32).astype(F64), var=np.maximum(v, F32(0)).astype(F64), n=n)


def moments_part_emu(e):
    n = float(e['n'])
    out = []
    for v in (n * e['mean'], n * (e['var'] + e['mean'] ** 2)):
        hi = v.astype(F32)
        out.append(hi.astype(F64) + (v - hi.astype(F64)).astype(F32).astype(F64))
    return np.stack(out)


def moments_bn_emu(e, gamma, beta, rm=None, rv=None, eps=BN_EPS, momentum=MOMENTUM):
    n, mean, vr = float(e['n']), e['mean'], e['var']
    iv = (1.0 / np.sqrt(vr + eps)).astype(F32)
    m32 = mean.astype(F32)
    sc = np.asarray(gamma, F32) * iv
    out = dict(mean=m32, inv=iv, scale=sc, shift=np.asarray(beta, F32) - m32 * sc)
    if rm is not None:
        unb = (vr * n / (n - 1.0) if n > 1 else vr).astype(F32)
        mo = F32(momentum)
        out.update(rm=(F32(1) - mo) * np.asarray(rm, F32) + mo * m32, rv=(F32(1) - mo) * np.asarray(rv, F32) + mo * unb)
    return out


# ---- head_bwd_finish --------------------------------------------------------------------------------------------------------------------
def finish_ref(P, x, k12, w0):
    """dX = sum of P's halves - x M - u, M[a][c] = sum_j k2_j w_j[a] w_j[c], u[c] = sum_j k1_j w_j[c]  (P [halves][R][32], k12 [2][512])"""
    P, x, k12, w0 = (np.asarray(t, F64) for t in (P, x, k12, w0))
    M, u = (w0 * k12[1][:, None]).T @ w0, k12[0] @ w0
    aM, au = (np.abs(w0) * np.abs(k12[1])[:, None]).T @ np.abs(w0), np.abs(k12[0]) @ np.abs(w0)
    return P.sum(0) - x @ M - u, np.abs(P).sum(0) + np.abs(x) @ aM + au


def finish_emu(P, x, k12, w0, bf16=False):
    P, x = np.asarray(P, F32), np.asarray(x, F32)
    k12, w64 = np.asarray(k12, F64), np.asarray(w0, F32).astype(F64)
    M, u = ((w64 * k12[1][:, None]).T @ w64).astype(F32), (k12[0] @ w64).astype(F32)
    pv = P[0] + P[1] if P.shape[0] == 2 else P[0]
    acc = np.zeros_like(pv)
    for a in range(32):
        acc = fma32(x[:, a:a + 1], M[a][None, :], acc)
    out = (pv - acc) - u
    return through_bf16(out) if bf16 else out
