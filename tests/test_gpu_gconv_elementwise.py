"""The generic engine's convolution kernels (csrc/gconv_x3_s1.hip, csrc/gconv_x3_strided.hip, csrc/gconv.hip) on their own, through ptta_op_gconv, compared PER
ELEMENT with torch's float64 convolution on the CPU: every launch form, at the sizes, channel counts and switches listed case by case in
tests/gconv_cases.py.  No element is left out of a comparison.

bound = TOL[arithmetic] * (|x| (*) |w| + |bias| + |y_prev|), TOL = 4 x the CPU emulation's largest error ratio (never a GPU figure;
profiles/gconv_elementwise.txt): fp32 (direct form) 3.82e-7, bf16x6 1.39e-7, bf16x3 1.07e-5, hi + lo weights 1.68e-6, one MFMA 2.55e-3
and 1.14e-7 against the float64 convolution of the bf16-rounded operands.  The images of a split batch are compared with their own
arithmetic's bound, so an image on the wrong side of six_B or x1_from_B fails."""
import pytest
import torch

from tests import gconv_cases as G
from tests.util import assert_elementwise

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
_cache = {}


def _expected(c):
    if c['name'] not in _cache:
        _cache.clear()                      # one case at a time: the full-size references are hundreds of MB
        d = G.make(c)
        _cache[c['name']] = (d, G.reference(c, d), G.reference_rounded(c, d) if 'x1' in G.image_ariths(c) else None)
    return _cache[c['name']]


def _device_views(c, d):
    """Device tensors the way the case wants them: dense, or channel slices of wider buffers (ld > C) filled with the sentinel."""
    ho, wo = G.out_size(c)
    x = d['x']
    x0, x1 = x[..., :c['c0']], (x[..., c['c0']:] if c['c1'] else None)

    def put(t, pre, post):
        if t is None:
            return None, None
        if not c['views']:
            return t.contiguous().cuda(), None
        wide = torch.full(t.shape[:3] + (pre + t.shape[3] + post,), SENTINEL)
        wide[..., pre:pre + t.shape[3]] = t
        wide = wide.cuda()
        return wide[..., pre:pre + t.shape[3]], wide
    x0d, _ = put(x0, 8, 8)                  # (16-byte aligned channel offsets, as the engine's slices are)
    x1d, _ = put(x1, 4, 12)
    yinit = d['y_prev'] if d['y_prev'] is not None else torch.full((c['b'], ho, wo, c['co']), SENTINEL)
    yd, ywide = put(yinit, 16, 16)
    return x0d, x1d, yd, ywide


def _run(c, impl):
    from proxytta.engine import op_gconv
    d, (ref, mag), rounded = _expected(c)
    x0d, x1d, yd, ywide = _device_views(c, d)
    form, stats = op_gconv(x0d, d['w'].cuda(), yd, x1=x1d, bias=None if d['bias'] is None else d['bias'].cuda(), k=c['k'], geom=c['geom'],
                           act=c['act'], accumulate=c['acc'], impl=impl, vert=c['vert'], six_b=c['six_b'] if impl == 'mfma' else 0,
                           x1_from_b=c['x1_from_b'], x1_w2=c['x1_w2'], dgrad=c['dgrad'], stat_npass=c['stats'] if impl == 'mfma' else 0)
    got = yd.cpu()
    assert got.shape == ref.shape
    if ywide is not None:                   # channels of the buffer outside the view keep what they were filled with
        w = ywide.cpu()
        assert bool((w[..., :16] == SENTINEL).all()) and bool((w[..., 16 + c['co']:] == SENTINEL).all()), 'wrote outside the output view'
    checked = 0
    for ar, i0, i1 in G.groups(c, impl):
        what = '%s [%s] images %d..%d as %s' % (c['name'], impl, i0, i1 - 1, ar)
        print('%s: largest |error| / magnitude %.3e (TOL %.3e)' % (what, float(((got[i0:i1].double() - ref[i0:i1]).abs() / mag[i0:i1]).max()), G.TOL[ar]))
        assert_elementwise(got[i0:i1], ref[i0:i1], G.TOL[ar] * mag[i0:i1], what)
        if ar == 'x1':
            assert_elementwise(got[i0:i1], rounded[0][i0:i1], G.TOL['x1r'] * rounded[1][i0:i1], what + ' (rounded operands)')
        checked += got[i0:i1].numel()
    assert checked == got.numel()           # the share of elements left out is zero
    return form, stats, got, ref, mag


@pytest.mark.parametrize('name', [c['name'] for c in G.CASES])
def test_gconv_matrix_core_per_element(name):
    c = G.BY_NAME[name]
    form, stats, got, ref, mag = _run(c, 'mfma')
    # the strided launcher took the form this case was written for (a retuned threshold must fail here, not test another kernel)
    assert form == c['form'], (name, form, c['form'])
    if c['stats']:
        # fused BatchNorm sums per pass and channel against float64 sums of the float64 reference; the bound is the elements' bound
        # summed over the pixels (sum y^2: d(y^2) <= (2 |y| + bound) bound), plus the worst case of the fp32 partial sums' own rounding:
        # a tile's sum is 32 additions per lane, one across the lane halves and three across the waves (the tiles are then summed in
        # fp64), under 64 roundings of 2^-24 each relative to the sum of magnitudes = 2^-18
        npass, per = c['stats'], c['b'] // c['stats']
        ar = G.image_ariths(c)
        assert len(set(ar)) == 1
        bnd = G.TOL[ar[0]] * mag
        for p in range(npass):
            r, b_ = ref[p * per:(p + 1) * per], bnd[p * per:(p + 1) * per]
            s1, s2 = r.sum(dim=(0, 1, 2)), (r * r).sum(dim=(0, 1, 2))
            b1 = b_.sum(dim=(0, 1, 2)) + 2.0 ** -18 * r.abs().sum(dim=(0, 1, 2))
            b2 = ((2 * r.abs() + b_) * b_).sum(dim=(0, 1, 2)) + 2.0 ** -18 * s2
            for which, (s, b) in enumerate(((s1, b1), (s2, b2))):
                err = (stats[p, which] - s).abs()
                print('%s pass %d %s: worst |error| / bound %.3f' % (name, p, ('sum y', 'sum y^2')[which], float((err / b).max())))
                assert bool((err <= b).all()), (name, p, which, int((err / b).argmax()), float((err / b).max()))


@pytest.mark.parametrize('name', [c['name'] for c in G.CASES])
def test_gconv_direct_form_per_element(name):
    """The direct fp32 form on the same cases against the same float64 reference, with its own (fp32) bound -- not against the
    matrix-core form."""
    form, _, _, _, _ = _run(G.BY_NAME[name], 'direct')
    assert form is None


def test_gconv_rejects_what_the_launchers_do_not_take():
    from proxytta.engine import op_gconv
    x = torch.zeros(1, 4, 4, 12).cuda()
    w = torch.zeros(8, 12, 3, 3).cuda()
    y = torch.zeros(1, 4, 4, 8).cuda()
    with pytest.raises(RuntimeError, match='-22'):
        op_gconv(x, w, y)                                   # 12 channels: not a multiple of 8
    with pytest.raises(RuntimeError, match='-22'):
        op_gconv(x, w, torch.zeros(1, 3, 4, 8).cuda())      # stride 1 keeps the size
    with pytest.raises(RuntimeError, match='-22'):
        op_gconv(x[..., :8], w, y, k=5)
    op_gconv(x, w, y, impl='direct')                        # the direct form takes any channel count
