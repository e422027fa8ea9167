"""Seeded cases of tests/test_inpaint_cases_cpu.py / tests/test_gpu_inpaint_device.py and the numpy restatement of what
ptta_inpaint_biharmonic (csrc/inpaint.hip) computes: the row of a hole in its separable form, built from the 1-D columns, applied
matrix-free, and plain conjugate gradients in fp64.  proxytta/inpaint.py (the host code) is the definition; the expected maps come
from it, once per case."""
import functools

import numpy as np

OFFSETS = [(-2, 0), (-1, -1), (-1, 0), (-1, 1), (0, -2), (0, -1), (0, 0), (0, 1), (0, 2), (1, -1), (1, 0), (1, 1), (2, 0)]


def columns(o, r):
    """Column `o` of the 1-D Laplacian on n = o + 1 + r points with the edge value replicated (scipy 'reflect': the diagonal is -1 at an
    end, -2 inside) and of its square, as arrays of length n."""
    n = o + 1 + r
    L = np.zeros((n, n))
    for i in range(n):
        L[i, i] = -2.0 + (i == 0) + (i == n - 1)
        if i > 0:
            L[i, i - 1] = 1.0
        if i < n - 1:
            L[i, i + 1] = 1.0
    return L[:, o].copy(), (L @ L)[:, o].copy()


def box_row(oy, ry, ox, rx):
    """c_p on the box of a hole `oy` rows / `ox` columns from the box's first row / column, `ry` / `rx` from its last:
    c[y, x] = a2_y[y] [x == px] + 2 a1_y[y] a1_x[x] + [y == py] a2_x[x]."""
    a1y, a2y = columns(oy, ry)
    a1x, a2x = columns(ox, rx)
    c = 2.0 * np.outer(a1y, a1x)
    c[:, ox] += a2y
    c[oy, :] += a2x
    return c


def field(h, w, seed, scale=1.0, offset=0.0):
    """A smooth positive fp32 field with small noise."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    f = 5.0 + 2.0 * np.sin(y / 5.0 + 0.3 * seed) * np.cos(x / 7.0) + 0.05 * y + 0.02 * x + 0.02 * rng.standard_normal((h, w))
    return (offset + scale * f).astype(np.float32)


def _mask(name, h, w, rng):
    m = np.zeros((h, w), bool)
    if name == 'corners_borders':
        m[0:3, 0:3] = True; m[h - 3:, w - 3:] = True                         # two opposite corners
        m[0:2, 10:13] = True; m[h - 2:, 5:8] = True; m[6:9, 0:2] = True; m[7:10, w - 2:] = True     # the four edges
    elif name == 'full_width_stripe':
        m[6:9, :] = True
    elif name == 'full_height_stripe':
        m[:, 10:13] = True
    elif name in ('checkerboard', 'checkerboard48'):
        yy, xx = np.mgrid[0:h, 0:w]
        m = (yy + xx) % 2 == 0
    elif name in ('random30', 'random30_odd'):
        m = rng.random_sample((h, w)) < 0.3
    elif name == 'random90':
        m = rng.random_sample((h, w)) < 0.9
    elif name == 'one_known':
        m[:] = True
        m[5, 9] = False
    elif name == 'big12x18':
        m[2:14, 3:21] = True
    elif name == 'blob32':
        m[8:40, 16:48] = True
    else:
        raise KeyError(name)
    return m


SIZES = {'corners_borders': (16, 24), 'full_width_stripe': (16, 24), 'full_height_stripe': (16, 24), 'checkerboard': (16, 24),
         'random30': (16, 24), 'random90': (16, 24), 'one_known': (16, 24), 'big12x18': (16, 24), 'random30_odd': (17, 23),
         'checkerboard48': (48, 64), 'blob32': (48, 64)}
NAMES = list(SIZES)


@functools.lru_cache(maxsize=None)
def case(name, scale=1.0, offset=0.0):
    """(field, mask, depth = where(mask, 0, field)) of the named case; read-only arrays, shared between the tests."""
    h, w = SIZES[name]
    seed = 1 + NAMES.index(name)
    f = field(h, w, seed, scale, offset)
    m = _mask(name, h, w, np.random.RandomState(100 + seed))
    d = np.where(m, np.float32(0), f).astype(np.float32)
    for a in (f, m, d):
        a.setflags(write=False)
    return f, m, d


@functools.lru_cache(maxsize=None)
def expected(name, scale=1.0, offset=0.0):
    """The host code's result for the case (computed once)."""
    from proxytta.inpaint import inpaint_biharmonic
    _, m, d = case(name, scale, offset)
    out = inpaint_biharmonic(d, m)
    out.setflags(write=False)
    return out


def build_rows(depth, mask):
    """Per hole in raster order: the indices of the 13 places of its row among the holes (-1: known or outside the image), their
    coefficients, and the right-hand side -sum over the known places of c * (double) depth."""
    h, w = depth.shape
    pts = np.argwhere(mask)
    index = -np.ones((h, w), np.int64)
    index[mask] = np.arange(len(pts))
    nbr = -np.ones((len(pts), 13), np.int64)
    coef = np.zeros((len(pts), 13))
    rhs = np.zeros(len(pts))
    for k, (py, px) in enumerate(pts):
        oy, ry, ox, rx = min(py, 2), min(h - 1 - py, 2), min(px, 2), min(w - 1 - px, 2)
        c = box_row(oy, ry, ox, rx)
        for j, (dy, dx) in enumerate(OFFSETS):
            y, x = py + dy, px + dx
            if 0 <= y < h and 0 <= x < w:
                cv = c[oy + dy, ox + dx]
                if index[y, x] >= 0:
                    nbr[k, j], coef[k, j] = index[y, x], cv
                else:
                    rhs[k] -= cv * float(depth[y, x])
    return nbr, coef, rhs


def cg_fill(depth, mask, rtol=1e-12, max_iter=5000):
    """What the kernel computes: (filled fp32 map, iterations, unclipped fp64 solution).  Raises if CG does not converge."""
    nbr, coef, b = build_rows(depth, mask)
    safe = np.where(nbr >= 0, nbr, 0)
    cz = np.where(nbr >= 0, coef, 0.0)

    def apply(v):
        return (cz * v[safe]).sum(axis=1)
    x = np.zeros_like(b)
    r = b.copy()
    p = r.copy()
    rr = float(r @ r)
    tol2 = rtol * rtol * rr
    it = 0
    if rr > 0:
        for it in range(1, max_iter + 1):
            Ap = apply(p)
            pAp = float(p @ Ap)
            assert pAp > 0
            alpha = rr / pAp
            x += alpha * p
            r -= alpha * Ap
            rr_new = float(r @ r)
            if rr_new <= tol2:
                break
            p = r + (rr_new / rr) * p
            rr = rr_new
        else:
            raise RuntimeError('CG did not converge in %d iterations' % max_iter)
    known = depth[~mask]
    out = depth.copy()
    out[mask] = np.clip(x, float(known.min()), float(known.max()))
    return out, it, x


def ulps(a, b):
    """Distance of two fp32 arrays in units in the last place (finite values of one sign or either side of zero)."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))
