"""The ELU form of the affine epilogue of the generic engine's stride-1 matrix-core convolution (csrc/gconv_x3_s1.hip, the ELU
instantiations of gconv_x3_s1_kernel), through ptta_op_gconv_affine with act 4:
    v = fmaf(conv + bias, scale[c], shift[c]);   y = v > 0 ? v : expm1f(v)
-- a BatchNorm3d + ELU of CostDCNet's UNet3D evaluated from constant running statistics, behind its 1x3x3 convolution (frames x planes
images, one source or skip | upsampled) or its 3x1x1 convolution (PTTA_GCONV_VERT: images [D][h w]).

Every case is compared
  * bit for bit with the pair it replaces: ptta_op_gconv (act 0) followed by ptta_op_gbn in mode PTTA_GBN_EVAL with act 4, and
  * per element with a float64 reference built from oracle/gconv_arith.py (convolution, bound magnitude) and oracle/gbn_arith.py (eval
    affine, ELU).
Bound of the float64 comparison, as in tests/test_gpu_gconv_affine.py: the convolution's bf16x3 error is at most TOL['x3'] x (|x| (*) |w| +
|bias|); the epilogue multiplies it by |scale| and adds the fma's rounding (2^-24 |v|) and expm1f's (a few 2^-24 of |expm1 v| <= |v|), two
orders below; ELU is 1-Lipschitz.  So |y - ref| <= TOL['x3'] x ((|x| (*) |w| + |bias|) |scale| + |shift|) per element.  The bf16x6 images of
a case (six_b) are finer than that; what ties them to their arithmetic is the bitwise comparison with the unfused pair, whose convolution
tests/test_gpu_gconv_elementwise.py holds to TOL['x6'].

Shapes: the UNet3D volumes of a 64 x 96 frame (16 planes of 16 x 24 at 32 channels, halved three times to 2 planes of 2 x 3 at 80): the
1x3x3 form over 2 D images, the vertical form over [D][h w] = 2 x 6 (fewer rows than taps), 4 x 24 (less than one 32-pixel tile), 8 x 96 and
16 x 384 (several tiles); 48 and 80 channels leave a half-filled 32-channel tile; the decoder's two-source splits 32 | 48 and 64 | 80.
Channel 0 of every case has zero weights, bias, beta and running mean: its pre-activation is exactly 0."""
import zlib

import numpy as np
import pytest
import torch

from oracle import gbn_arith as B
from oracle import gconv_arith as A
from tests.gconv_cases import TOL

pytestmark = pytest.mark.gpu
EPS = 1e-5
SENTINEL = -777.25


def K(name, b, h, w, c0, c1, co, vert=False, six_b=0, views=False):
    return dict(name=name, b=b, h=h, w=w, c0=c0, c1=c1, co=co, vert=vert, six_b=six_b, views=views)


CASES = [
    # 1x3x3 over frames x planes images
    K('sq_2x3_80', 4, 2, 3, 80, 0, 80),
    K('sq_4x6_64_80_to_64', 8, 4, 6, 64, 80, 64),                     # up2: skip 64 | upsampled 80
    K('sq_8x12_48', 16, 8, 12, 48, 0, 48),
    K('sq_16x24_32_48_to_32', 32, 16, 24, 32, 48, 32),                # up4: skip 32 | upsampled 48
    K('sq_16x24_32_six_views', 32, 16, 24, 32, 0, 32, six_b=16, views=True),     # unet3d.inc: bf16x6 real frames; ldy > co
    K('sq_9x33_48_views', 2, 9, 33, 48, 0, 48, views=True),           # one row / one pixel into the next tile, ldy > co, half-filled tile
    # 3x1x1 as three vertical taps over [D][h w]
    K('v_2x6_80', 2, 2, 6, 80, 0, 80, vert=True),
    K('v_4x24_64', 2, 4, 24, 64, 0, 64, vert=True),
    K('v_8x96_48', 2, 8, 96, 48, 0, 48, vert=True),
    K('v_16x384_32_six', 2, 16, 384, 32, 0, 32, vert=True, six_b=1),
    K('v_9x40_80_views', 2, 9, 40, 80, 0, 80, vert=True, views=True),  # ragged last tile both ways, ldy > co
]


def make(c):
    g = torch.Generator().manual_seed(zlib.crc32(c['name'].encode()))
    cin, co = c['c0'] + c['c1'], c['co']
    taps = 3 if c['vert'] else 9
    shape = (co, cin, 3, 1) if c['vert'] else (co, cin, 3, 3)
    d = dict(x=torch.randn(c['b'], c['h'], c['w'], cin, generator=g),
             w=torch.randn(shape, generator=g) * float(taps * cin) ** -0.5,
             bias=torch.randn(co, generator=g) * 0.5,
             gamma=0.5 + torch.rand(co, generator=g), beta=torch.randn(co, generator=g) * 0.3,
             rm=torch.randn(co, generator=g) * 0.4, rv=0.3 + 2.0 * torch.rand(co, generator=g))
    d['gamma'][::5] *= -1.0              # negative scales too
    d['w'][0] = 0.0                      # channel 0: fmaf(0, scale, 0) = 0 exactly
    d['bias'][0] = 0.0; d['beta'][0] = 0.0; d['rm'][0] = 0.0
    return d


def reference(c, d):
    """float64 output and bound magnitude, NHWC numpy."""
    lin = A.linear_op(3, 's1', c['vert'])
    conv, mag = A.reference(lin, d['x'].permute(0, 3, 1, 2), d['w'], d['bias'])
    conv, mag = conv.permute(0, 2, 3, 1).numpy(), mag.permute(0, 2, 3, 1).numpy()
    ev = B.eval_affine_ref(d['gamma'].numpy(), d['beta'].numpy(), d['rm'].numpy(), d['rv'].numpy(), EPS)
    pre = conv * ev['scale'] + ev['shift']
    return B.eval_forward_ref(conv, ev, act='elu'), mag * np.abs(ev['scale']) + np.abs(ev['shift']), pre


def device_out(c, pad):
    wide = torch.full((c['b'], c['h'], c['w'], c['co'] + 2 * pad), SENTINEL, device='cuda')
    return wide, wide[..., pad:pad + c['co']] if pad else wide


@pytest.mark.parametrize('name', [c['name'] for c in CASES])
def test_elu_epilogue_bitwise_and_elementwise(name):
    from proxytta.engine import op_gbn, op_gconv, op_gconv_affine
    c = {k['name']: k for k in CASES}[name]
    d = make(c)
    dev = {k: v.cuda() for k, v in d.items()}
    x0 = dev['x'][..., :c['c0']]                              # channel slices of one map: ld0 = ld1 = c0 + c1
    x1 = dev['x'][..., c['c0']:] if c['c1'] else None
    pad = 8 if c['views'] else 0
    # unfused: the convolution without an activation, then the eval BatchNorm3d + ELU (which leaves its affine table in st)
    _, raw = device_out(c, 0)
    op_gconv(x0, dev['w'], raw, x1=x1, bias=dev['bias'], vert=c['vert'], six_b=c['six_b'])
    st = torch.zeros(4, c['co'], device='cuda')
    un_wide, un = device_out(c, pad)
    op_gbn('eval', raw, un, st, dev['gamma'], beta=dev['beta'], act='elu', eps=EPS, rm=dev['rm'], rv=dev['rv'])
    # fused, from the same table
    fu_wide, fu = device_out(c, pad)
    op_gconv_affine(x0, dev['w'], fu, st[2], st[3], x1=x1, bias=dev['bias'], act='elu', vert=c['vert'], six_b=c['six_b'])
    torch.cuda.synchronize()
    assert torch.equal(fu_wide, un_wide), 'fused and unfused differ by %.3e' % float((fu_wide - un_wide).abs().max())
    if pad:                                # channels outside the view keep the sentinel
        assert bool((fu_wide[..., :pad] == SENTINEL).all()) and bool((fu_wide[..., pad + c['co']:] == SENTINEL).all())
    ref, mag, pre = reference(c, d)
    out = fu.cpu().double().numpy()
    ratio = float((np.abs(out - ref) / mag.clip(min=1e-300))[..., 1:].max())
    neg = float((pre[..., 1:] < 0).mean())
    print('%s: largest |y - float64| / bound magnitude %.3e (TOL x3 %.3e); %.0f %% negative pre-activations' % (name, ratio, TOL['x3'], 100 * neg))
    assert ratio <= TOL['x3'], ratio
    assert bool((out[..., 0] == 0.0).all()) and bool((ref[..., 0] == 0.0).all())      # the exact zeros: expm1f(0) = 0
    assert 0.25 < neg < 0.75 and float(ref.min()) < -0.5 and float(ref.max()) > 0.5   # both branches, with values that matter


def test_elu_refusals_return_22_before_any_launch():
    from proxytta.engine import op_gconv_affine
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 9, 13, 32, generator=g).cuda()
    w = torch.randn(32, 32, 3, 3, generator=g).cuda()
    tab = torch.ones(2, 32, device='cuda')
    res = torch.zeros(2, 9, 13, 32, device='cuda')

    def refused(**kw):
        y = torch.full((2, kw.pop('ho', 9), kw.pop('wo', 13), 32), SENTINEL, device='cuda')
        args = dict(x0=x, weight=w, y=y, scale=tab[0], shift=tab[1], act='elu')
        args.update(kw)
        with pytest.raises(RuntimeError, match=r'\(-22\)'):
            op_gconv_affine(**args)
        torch.cuda.synchronize()
        assert bool((y == SENTINEL).all()), 'the output was written'

    for vert in (False, True):
        wv = w[:, :, :, :1].contiguous() if vert else w
        refused(weight=wv, vert=vert, res=res)                 # no residual form behind ELU
        refused(weight=wv, vert=vert, accumulate=True)
        refused(weight=wv, vert=vert, stat_npass=1)            # no fused statistics
        refused(weight=wv, vert=vert, impl='direct')           # the direct fp32 kernels have no such epilogue
    refused(geom='s2', ho=5, wo=7)                             # the stride-1 kernels' only
    refused(weight=w[:, :, :1, :1].contiguous(), k=1)
    # and the arguments above are fine when they are right
    y = torch.full((2, 9, 13, 32), SENTINEL, device='cuda')
    op_gconv_affine(x, w, y, tab[0], tab[1], act='elu')
    torch.cuda.synchronize()
    assert bool((y != SENTINEL).all())
