"""The BatchNorm of the generic engine (csrc/gbn.hip) on the CPU (test infrastructure): a float64 reference of the forward and the
backward with every switch, an fp32 emulation of the kernels' arithmetic, and the magnitudes the per-element bounds scale with.

Everything is numpy, NHWC [B][H][W][C]; nothing from the library takes part.  B images hold `npass` equal slices with their own
statistics; the backward belongs to pass 0.

What the emulation restates: the pixel-to-thread assignment of gbn_stats_kernel (blocks, nsub, pstride, the four-way grouping of the
forward sums, the sequential backward sums), fp32 sums per thread, fp32 over nsub, fp64 over the blocks, the SyncBatchNorm expand's hi +
lo split, inv / scale / shift / c1 / c2 rounded to fp32, the fma apply.  What it cannot state is where the compiler contracts a product
and a sum into one fma, and the library's expm1f / sqrt: the tests allow a factor 4 on the emulation's own error for that.

The cancellation factor of a channel: kappa = (mean^2 + var + eps) / (var + eps) >= 1.  The kernels form var = E[x^2] - mean^2 from fp32
partial sums, so var + eps carries kappa times the fp32 rounding and so does inv, relatively.  In y = scale (x - mean) + beta that error
multiplies |x - mean| only; the plain roundings (the mean's, mean * scale, the fma) multiply |x| + |mean| + rms:
    mag_v = |gamma| inv (kappa |x - mean| + |x| + |mean| + rms) + |beta|,      rms = sqrt(E x^2)."""
import numpy as np

F32, F64 = np.float32, np.float64
BLOCKS = 1024                 # GBN_BLOCKS
FAULTS = ('biased_running_var', 'no_eps', 'shared_stats', 'bwd_pass1_stats', 'drop_tail_pixel', 'drop_block', 'gres_after_inner_mask',
          'dgamma_no_world')


def geometry(C, R):
    """The statistics launch of R pixels per pass and C channels, as the launchers size it."""
    CT = min(C, 256)
    nsub = 256 // CT
    blocks = max(1, min(BLOCKS, (R + nsub - 1) // nsub))
    ps = blocks * nsub
    t = np.arange(ps)
    n = np.where(t < R, (R - t + ps - 1) // ps, 0)                      # pixels per thread
    return dict(CT=CT, nsub=nsub, blocks=blocks, pstride=ps, channel_blocks=(C + CT - 1) // CT, idle_threads=256 - nsub * CT,
                partial_last_channel_block=C > 256 and C % 256 != 0, capped=(R + nsub - 1) // nsub > BLOCKS,
                unrolled_max=int((n // 4).max()), tail_after_unrolled=bool(((n // 4 > 0) & (n % 4 > 0)).any()),
                tail_only=bool(((n // 4 == 0) & (n > 0)).any()), threads_without_pixel=bool((n == 0).any()))


def reducer_loops(nblocks):
    """gbn_sum_partials_block over nblocks partials: (most four-load iterations of a thread, most 256-stride tail iterations)."""
    four = tail = 0
    for t in range(256):
        b, f, k = t, 0, 0
        while b + 768 < nblocks:
            b += 1024; f += 1
        while b < nblocks:
            b += 256; k += 1
        four, tail = max(four, f), max(tail, k)
    return four, tail


def act_fn(v, act):
    if act == 'relu':
        return np.where(v > 0, v, v.dtype.type(0))
    if act == 'lrelu':
        return np.where(v > 0, v, v.dtype.type(0.2) * v)
    if act == 'elu':
        return np.where(v > 0, v, np.expm1(np.minimum(v, v.dtype.type(0))))
    return v


def act_grad(pre, act):
    if act == 'relu':
        return (pre > 0).astype(F64)
    if act == 'lrelu':
        return np.where(pre > 0, 1.0, 0.2)
    if act == 'elu':
        return np.where(pre > 0, 1.0, np.exp(np.minimum(pre, 0.0)))
    return np.ones_like(pre)


def _passes(t, npass):
    """[B][H][W][C] -> [npass][R][C]"""
    return t.reshape(npass, -1, t.shape[-1])


# ---- float64 reference ---------------------------------------------------------------------------------------------------------
def forward_ref(x, gamma, beta, eps, npass=1, act='none', res=None, act_first=False, res_relu=True, track=None, world=1, fault=None,
                drop=None):
    """track = dict(rm, rv, momentum, repeats) for a tracked BatchNorm.  `drop` [R] bool: pixels of every pass left out of the sums (the
    planted faults 'drop_tail_pixel' / 'drop_block').  Returns float64 mean, var, inv, scale, shift [npass][C], the pre-activation v and
    y [B][H][W][C], kappa, rms, and with `track` rm, rv and the eval affine ev = dict(mean, inv, scale, shift) of the updated buffers."""
    xs = _passes(x.astype(F64), npass)
    R, C = xs.shape[1], xs.shape[2]
    gamma, beta, eps = gamma.astype(F64), beta.astype(F64), float(F32(eps))
    if drop is not None:
        mean = (xs * ~drop[None, :, None]).sum(1) / R
        var = np.maximum((xs * xs * ~drop[None, :, None]).sum(1) / R - mean * mean, 0.0)
    else:
        mean = xs.mean(1)
        var = ((xs - mean[:, None]) ** 2).mean(1)
    if fault == 'shared_stats' and npass == 2:
        allx = xs.reshape(-1, C)
        mean = np.broadcast_to(allx.mean(0), (2, C)).copy()
        var = np.broadcast_to(((allx - mean[0]) ** 2).mean(0), (2, C)).copy()
    with np.errstate(divide='ignore', invalid='ignore'):              # (the planted fault 'no_eps' divides by a zero variance)
        inv = 1.0 / np.sqrt(var + (0.0 if fault == 'no_eps' else eps))
        scale = gamma * inv
        shift = beta - mean * scale
        v = (xs - mean[:, None]) * scale[:, None] + beta
    out = dict(mean=mean, var=var, inv=inv, scale=scale, shift=shift, kappa=(mean * mean + var + eps) / (var + eps),
               rms=np.sqrt(mean * mean + var), R=R)
    out['v'] = v.reshape(x.shape)
    out['y'] = _combine(out['v'], None if res is None else res.astype(F64), act, act_first, res_relu)
    if track is not None:
        Rg = R * world
        rm, rv, mom = track['rm'].astype(F64), track['rv'].astype(F64), float(F32(track['momentum']))
        for p in range(npass):
            unb = var[p] * (Rg / (Rg - 1.0) if Rg > 1 and fault != 'biased_running_var' else 1.0)
            for _ in range(track['repeats']):
                rm = (1 - mom) * rm + mom * mean[p]
                rv = (1 - mom) * rv + mom * unb
        out['rm'], out['rv'] = rm, rv
        out['ev'] = eval_affine_ref(gamma, beta, rm, rv, eps)
    return out


def _combine(v, res, act, act_first, res_relu):
    if res is None:
        return act_fn(v, act)
    s = (act_fn(v, act) if act_first else v) + res
    return np.maximum(s, 0.0) if res_relu else s


def eval_affine_ref(gamma, beta, rm, rv, eps):
    inv = 1.0 / np.sqrt(rv.astype(F64) + float(F32(eps)))
    scale = gamma.astype(F64) * inv
    return dict(mean=rm.astype(F64), inv=inv, scale=scale, shift=beta.astype(F64) - rm * scale)


def eval_forward_ref(x, ev, act='none', res=None, act_first=False, res_relu=True):
    v = x.astype(F64) * ev['scale'] + ev['shift']
    return _combine(v, None if res is None else res.astype(F64), act, act_first, res_relu)


def backward_ref(x, g, fw, gamma, npass=1, act='none', res=None, act_first=False, res_relu=True, gx_prev=None, gres_prev=None, world=1,
                 fault=None, drop=None):
    """The gradient of pass 0 given the forward `fw` (forward_ref): g [B / npass][H][W][C] -> dgamma, dbeta [C], gx and, with a residual,
    gres; plus what the magnitudes need (g1 = the gradient at the BatchNorm's output, gouter = at the residual sum, xhat, c1, c2)."""
    sp = 1 if (fault == 'bwd_pass1_stats' and npass == 2) else 0
    with np.errstate(invalid='ignore'):                                # (a forward with the planted fault 'no_eps' holds inf)
        return _backward_ref(x, g, fw, gamma, npass, act, res, act_first, res_relu, gx_prev, gres_prev, world, fault, drop, sp)


def _backward_ref(x, g, fw, gamma, npass, act, res, act_first, res_relu, gx_prev, gres_prev, world, fault, drop, sp):
    n0 = x.shape[0] // npass
    x0 = x[:n0].astype(F64)
    g = g.astype(F64)
    mean, inv, scale, shift = fw['mean'][sp], fw['inv'][sp], fw['scale'][sp], fw['shift'][sp]
    v = (x0 - mean) * scale + (shift + mean * scale)
    if res is None:
        gouter, g1 = g, g * act_grad(v, act)
    else:
        r0 = res[:n0].astype(F64)
        inner = act_fn(v, act) if act_first else v
        gouter = g * ((inner + r0) > 0) if res_relu else g
        g1 = gouter * act_grad(v, act) if act_first else gouter
    xhat = (x0 - mean) * inv
    R = x0.size // x0.shape[-1]
    keep = 1.0 if drop is None else (~drop).astype(F64).reshape(x0.shape[:3] + (1,))
    dbeta = (g1 * keep).sum((0, 1, 2))
    dgamma = (g1 * xhat * keep).sum((0, 1, 2))
    c1, c2 = dbeta / R, dgamma / R
    gx = gamma.astype(F64) * inv * (g1 - c1 - xhat * c2)
    out = dict(g1=g1, gouter=gouter, xhat=xhat, c1=c1, c2=c2, dbeta=dbeta, dgamma=dgamma * (world if fault == 'dgamma_no_world' else 1.0),
               gx=gx + (0.0 if gx_prev is None else gx_prev.astype(F64)), v=v)
    if res is not None:
        gr = g1 if fault == 'gres_after_inner_mask' else gouter
        out['gres'] = gr + (0.0 if gres_prev is None else gres_prev.astype(F64))
    return out


# ---- magnitudes ----------------------------------------------------------------------------------------------------------------
def forward_mags(x, gamma, beta, fw, npass=1, res=None, track=None, world=1):
    """What the forward's bounds scale with: y [B][H][W][C] (mag_v + |res|), v, mean and inv [npass][C], rm and rv [C]."""
    xs = _passes(x.astype(F64), npass)
    g = np.abs(gamma.astype(F64))
    mean, inv, kappa, rms = fw['mean'][:, None], fw['inv'][:, None], fw['kappa'][:, None], fw['rms'][:, None]
    mv = g * inv * (kappa * np.abs(xs - mean) + np.abs(xs) + np.abs(mean) + rms) + np.abs(beta.astype(F64))
    mv = mv.reshape(x.shape)
    out = dict(v=mv, y=mv + (0.0 if res is None else np.abs(res.astype(F64))), mean=np.abs(fw['mean']) + fw['rms'], inv=fw['inv'] * fw['kappa'])
    if track is not None:
        Rg = fw['R'] * world
        eps = (fw['mean'] ** 2 + fw['var']) / fw['kappa'] - fw['var']                           # (kappa's own eps)
        out['rm'] = np.abs(track['rm'].astype(F64)) + out['mean'].max(0)
        out['rv'] = np.abs(track['rv'].astype(F64)) + ((fw['mean'] ** 2 + fw['var'] + eps) * (Rg / max(Rg - 1.0, 1.0))).max(0)
    return out


def eval_mags(x, gamma, beta, ev, mags, eps, res=None):
    """The eval forward from running statistics that carry the errors mags['rm'], mags['rv']."""
    x = x.astype(F64)
    g = np.abs(gamma.astype(F64))
    rel_inv = 1.0 + mags['rv'] / (ev['inv'] ** -2)                     # d inv / inv = d rv / (2 (rv + eps)), plus inv's own rounding
    m = g * ev['inv'] * (np.abs(x - ev['mean']) * rel_inv + mags['rm'] + np.abs(x) + np.abs(ev['mean'])) + np.abs(beta.astype(F64))
    return m + (0.0 if res is None else np.abs(res.astype(F64)))


def backward_mags(x, g, fw, fmag, bw, gamma, npass=1, act='none', gx_prev=None, gres_prev=None):
    """dbeta, dgamma [C], gx and gres [B / npass][H][W][C]."""
    n0 = x.shape[0] // npass
    x0 = x[:n0].astype(F64)
    ga = np.abs(gamma.astype(F64))
    mean, inv, kappa, rms = fw['mean'][0], fw['inv'][0], fw['kappa'][0], fw['rms'][0]
    R = x0.size // x0.shape[-1]
    # ELU's gradient y + 1 = exp(v) carries v's error (slope <= 1); the other activations' gradients are selects
    mg1 = np.abs(g.astype(F64)) * ((1.0 + fmag['v'][:n0]) if act == 'elu' else 1.0)
    mxh = inv * (kappa * np.abs(x0 - mean) + np.abs(x0) + np.abs(mean) + rms)
    g1, xh = np.abs(bw['g1']), np.abs(bw['xhat'])
    mdb = mg1.sum((0, 1, 2))
    mdg = (mg1 * xh + g1 * mxh).sum((0, 1, 2))
    c1, c2 = np.abs(bw['c1']), np.abs(bw['c2'])
    mgx = ga * inv * (kappa * (g1 + c1 + 2 * xh * c2) + mg1 + mdb / R + xh * mdg / R + mxh * c2)
    out = dict(dbeta=mdb, dgamma=mdg, gx=mgx + (0.0 if gx_prev is None else np.abs(gx_prev.astype(F64))))
    out['gres'] = np.abs(bw['gouter']) + (0.0 if gres_prev is None else np.abs(gres_prev.astype(F64)))
    return out


# ---- fp32 emulation ------------------------------------------------------------------------------------------------------------
def _thread_counts(R, ps):
    t = np.arange(ps)
    return np.where(t < R, (R - t + ps - 1) // ps, 0)


def _threads(a, ps):
    """[R][C] -> [K][pstride][C], zero padded: pixel k * pstride + t is the k-th pixel of thread t"""
    R, C = a.shape
    K = (R + ps - 1) // ps
    pad = np.zeros((K * ps, C), F32)
    pad[:R] = a
    return pad.reshape(K, ps, C)


def _over_nsub(s, geo):
    s = s.reshape(geo['blocks'], geo['nsub'], -1)                      # thread t = block * nsub + sub
    a = np.zeros((geo['blocks'], s.shape[2]), F32)
    for k in range(geo['nsub']):
        a = a + s[:, k]
    return a


def stats_partials_emu(xp):
    """gbn_stats_kernel<0> on one pass [R][C] fp32 -> part [blocks][2][C] fp32."""
    R, C = xp.shape
    geo = geometry(C, R)
    ps = geo['pstride']
    xs, n = _threads(xp.astype(F32), ps), _thread_counts(R, ps)
    nun = n // 4
    s1, s2 = np.zeros((ps, C), F32), np.zeros((ps, C), F32)
    for j in range(xs.shape[0] // 4):
        a0, a1, a2, a3 = xs[4 * j], xs[4 * j + 1], xs[4 * j + 2], xs[4 * j + 3]
        m = (nun > j)[:, None]
        s1 = np.where(m, s1 + ((a0 + a1) + (a2 + a3)), s1)
        s2 = np.where(m, s2 + ((a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3)), s2)
    for k in range(xs.shape[0]):
        m = ((k >= 4 * nun) & (k < n))[:, None]
        if m.any():
            s1 = np.where(m, s1 + xs[k], s1)
            s2 = np.where(m, s2 + xs[k] * xs[k], s2)
    return np.stack([_over_nsub(s1, geo), _over_nsub(s2, geo)], 1)


def split_partials(xp, nblocks):
    """Caller-made partials of one pass: the pixels split into nblocks runs, float64 sums rounded to fp32 -> [nblocks][2][C]."""
    x64 = xp.astype(F64)
    edges = np.linspace(0, x64.shape[0], nblocks + 1).astype(np.int64)
    c1 = np.concatenate([np.zeros((1, x64.shape[1])), np.cumsum(x64, 0)])
    c2 = np.concatenate([np.zeros((1, x64.shape[1])), np.cumsum(x64 * x64, 0)])
    return np.stack([c1[edges[1:]] - c1[edges[:-1]], c2[edges[1:]] - c2[edges[:-1]]], 1).astype(F32)


def _block_sums(part, world):
    """fp64 over the blocks; with a SyncBatchNorm exchange the sum comes back as fp32 hi (+ lo when there is a second block)."""
    s = part.astype(F64).sum(0)
    if world > 1:
        v = s * world
        hi = v.astype(F32)
        s = hi.astype(F64) + ((v - hi).astype(F32).astype(F64) if part.shape[0] > 1 else 0.0)
    return s


def _fma(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def _combine32(v, res, act, act_first, res_relu):
    if res is None:
        return act_fn(v, act)
    s = (act_fn(v, act) if act_first else v) + res.astype(F32)
    return np.where(s > 0, s, F32(0)) if res_relu else s


def forward_emu(x, gamma, beta, eps, npass=1, act='none', res=None, act_first=False, res_relu=True, track=None, world=1, parts=None):
    """fp32: st [4][npass][C], y, and with `track` rm, rv, st_eval [4][C].  parts [npass][nblocks][2][C]: caller-made partials."""
    xs = _passes(x.astype(F32), npass)
    R, C = xs.shape[1], xs.shape[2]
    gamma, beta, eps32 = gamma.astype(F32), beta.astype(F32), F32(eps)
    Rg = R * world
    st = np.zeros((4, npass, C), F32)
    rm = rv = None
    if track is not None:
        rm, rv, mom = track['rm'].astype(F32), track['rv'].astype(F32), F32(track['momentum'])
    for p in range(npass):
        s = _block_sums(parts[p] if parts is not None else stats_partials_emu(xs[p]), world)
        m = s[0] / Rg
        var = np.maximum(s[1] / Rg - m * m, 0.0)
        iv = (1.0 / np.sqrt(var + float(eps32))).astype(F32)
        sc = gamma * iv
        mf = m.astype(F32)
        st[0, p], st[1, p], st[2, p], st[3, p] = mf, iv, sc, beta - mf * sc
        if track is not None:
            v2 = np.maximum(1.0 / (iv.astype(F64) ** 2) - float(eps32), 0.0)
            unb = (v2 * Rg / (Rg - 1) if Rg > 1 else v2).astype(F32)
            for _ in range(track['repeats']):
                rm = (F32(1) - mom) * rm + mom * mf
                rv = (F32(1) - mom) * rv + mom * unb
    v = _fma(xs, st[2][:, None], st[3][:, None]).reshape(x.shape)
    out = dict(st=st, v=v, y=_combine32(v, res, act, act_first, res_relu))
    if track is not None:
        iv = F32(1) / np.sqrt(rv + eps32)
        sc = gamma * iv
        out.update(rm=rm, rv=rv, st_eval=np.stack([rm, iv, sc, beta - rm * sc]))
    return out


def backward_emu(x, g, y, st, gamma, npass=1, act='none', has_res=False, act_first=False, res_relu=True, gx_prev=None, gres_prev=None,
                 world=1):
    """fp32 backward of pass 0 from the forward's x, y, st as the kernels read them: dgamma, dbeta, gx, gres (None without a residual)."""
    n0 = x.shape[0] // npass
    C = x.shape[-1]
    x0, y0, g = x[:n0].astype(F32), y[:n0].astype(F32), g.astype(F32)
    mean, inv, sc, sh = st[0, 0], st[1, 0], st[2, 0], st[3, 0]
    rr = bool(has_res and res_relu)
    yless = (not rr) and act == 'relu' and not act_first
    pre = _fma(x0, sc, sh)
    if yless:
        gouter = g1 = np.where(pre > 0, g, F32(0))
    elif rr:
        gouter = np.where(y0 > 0, g, F32(0))
        g1 = np.where(pre > 0, gouter, F32(0)) if act_first else gouter
    elif act == 'relu':
        gouter = g1 = np.where(y0 > 0, g, F32(0))
    elif act == 'lrelu':
        gouter = g1 = np.where(y0 > 0, g, F32(0.2) * g)
    elif act == 'elu':
        gouter = g1 = np.where(y0 > 0, g, g * (y0 + F32(1)))
    else:
        gouter = g1 = g
    R = x0.size // C
    geo = geometry(C, R)
    ps = geo['pstride']
    g1t = _threads(g1.reshape(R, C), ps)
    tt = _threads((g1 * (x0 - mean) * inv).reshape(R, C), ps)
    s1, s2 = np.zeros((ps, C), F32), np.zeros((ps, C), F32)
    for k in range(g1t.shape[0]):                                      # padded pixels add +0
        s1, s2 = s1 + g1t[k], s2 + tt[k]
    s = _block_sums(np.stack([_over_nsub(s1, geo), _over_nsub(s2, geo)], 1), world)
    Rg, gsc = R * world, F32(1) / F32(world)
    out = dict(dbeta=s[0].astype(F32) * gsc, dgamma=s[1].astype(F32) * gsc)
    b0, c1, c2 = gamma.astype(F32) * inv, (s[0] / Rg).astype(F32), (s[1] / Rg).astype(F32)
    d = b0 * (g1 - c1 - ((x0 - mean) * inv) * c2)
    out['gx'] = d if gx_prev is None else d + gx_prev.astype(F32)
    out['gres'] = None if not has_res else (gouter if gres_prev is None else gouter + gres_prev.astype(F32))
    return out
