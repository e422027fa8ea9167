"""The per-channel affine epilogue of the generic engine's matrix-core convolutions (csrc/gconv_x3_s1.hip and gconv_x3_strided.hip, GX3Args::scale), through
ptta_op_gconv_affine:   y = act(fmaf(conv + bias, scale[c], shift[c]) [+ res])
-- what the eval forward of NLSPN's meta-only mode runs where a BatchNorm2d with constant statistics follows a convolution.

Every case is compared
  * per element with a float64 restatement written here in numpy, and
  * bit for bit with the unfused pair it replaces: ptta_op_gconv (no activation) followed by ptta_op_gbn in mode PTTA_GBN_EVAL.
Bound of the float64 comparison: the convolution is bf16x3 arithmetic, whose error against float64 the CPU emulation of
tests/gconv_cases.py bounds by TOL['x3'] x (|x| (*) |w| + |bias|); the epilogue multiplies that by |scale| and adds two fp32 roundings (the
fma, the residual add: 2^-24 each, of |v scale + shift| and of the sum), three orders below the first term.  The activations are
1-Lipschitz.  So |y - ref| <= TOL['x3'] x ((|x| (*) |w| + |bias|) |scale| + |shift| + |res|), per element."""
import zlib

import numpy as np
import pytest
import torch

from tests.gconv_cases import TOL

pytestmark = pytest.mark.gpu
EPS = 1e-5
SENTINEL = -777.25


def K(name, b, h, w, ci, co, k=3, geom='s1', act='none', res=False, form=None, views=False):
    return dict(name=name, b=b, h=h, w=w, ci=ci, co=co, k=k, geom=geom, act=act, res=res, form=form, views=views)


# 9 x 13: one row into the second 8-row tile, less than one 32-pixel tile wide; b = 2: more than one block; every channel count of the
# table takes partial or several 32-channel tiles.  Stride 2: 9 x 13 -> 5 x 7 (odd input, the second row of the last row pair outside).
CASES = [
    K('s1_16_64_relu', 2, 9, 13, 16, 64, act='relu'),
    K('s1_64_64_res_relu', 2, 9, 13, 64, 64, act='relu', res=True),                      # BasicBlock bn2: residual, then ReLU
    K('s1_64_64_lrelu', 2, 9, 13, 64, 64, act='lrelu'),                                   # conv_bn_relu's LeakyReLU(0.2)
    K('s1k1_48_48', 2, 9, 13, 48, 48, k=1),
    K('s2_64_128_relu', 2, 9, 13, 64, 128, geom='s2', act='relu', form='nco2'),           # ResNet34's strided 3x3 (conv3.0.conv1)
    K('s2k1_64_128_downsample', 2, 9, 13, 64, 128, k=1, geom='s2', form='plain'),         # its 1x1 downsample: no activation
    K('views_s1_64_40_res', 2, 9, 13, 64, 40, act='relu', res=True, views=True),          # ldy > co and ld_res > co
    # beyond the forms of the list above: the K-split instantiations (1/8 and 1/16-resolution layers) and the decoders' transposed form
    K('s2_ksplit_128_256_relu', 2, 9, 13, 128, 256, geom='s2', act='relu', form='ksplit'),      # conv4.0.conv1
    K('s2k1_ksplit_128_256', 2, 9, 13, 128, 256, k=1, geom='s2', form='ksplit'),               # conv4.0.downsample.0
    K('s2_ksplit_512_512_lrelu', 1, 5, 9, 512, 512, geom='s2', act='lrelu', form='ksplit'),     # conv6
    K('views_s2_64_72_res', 2, 9, 13, 64, 72, geom='s2', act='relu', res=True, views=True, form='plain'),
    K('t2_64_64_lrelu', 2, 5, 7, 64, 64, geom='t2', act='lrelu', form='nco2'),                   # a decoder's ConvTranspose2d + BN + LeakyReLU
]


def out_size(c):
    return {'s1': (c['h'], c['w']), 's2': ((c['h'] + 1) // 2, (c['w'] + 1) // 2), 't2': (2 * c['h'], 2 * c['w'])}[c['geom']]


def make(c):
    g = torch.Generator().manual_seed(zlib.crc32(c['name'].encode()))
    ho, wo = out_size(c)
    taps = c['k'] * c['k']
    shape = (c['ci'], c['co'], c['k'], c['k']) if c['geom'] == 't2' else (c['co'], c['ci'], c['k'], c['k'])
    d = dict(x=torch.randn(c['b'], c['h'], c['w'], c['ci'], generator=g),
             w=torch.randn(shape, generator=g) * float(taps * c['ci']) ** -0.5,
             bias=torch.randn(c['co'], generator=g) * 0.5,
             gamma=0.5 + torch.rand(c['co'], generator=g), beta=torch.randn(c['co'], generator=g) * 0.3,
             rm=torch.randn(c['co'], generator=g) * 0.4, rv=0.3 + 2.0 * torch.rand(c['co'], generator=g),
             res=torch.randn(c['b'], ho, wo, c['co'], generator=g) if c['res'] else None)
    d['gamma'][::5] *= -1.0              # negative scales too
    return d


def conv64(c, x, w):
    """float64 convolution, NHWC, padding k // 2; returns (sum x w, sum |x| |w|)."""
    k, pad = c['k'], c['k'] // 2
    b, h, wd, _ = x.shape
    ho, wo = out_size(c)
    out = [np.zeros((b, ho, wo, c['co'])), np.zeros((b, ho, wo, c['co']))]
    for which, (xx, ww) in enumerate(((x, w), (np.abs(x), np.abs(w)))):
        if c['geom'] == 't2':            # ConvTranspose2d(k, stride 2, padding k // 2, output_padding 1): input (iy, ix) reaches output (2 iy - pad + ky, ..)
            for ky in range(k):
                for kx in range(k):
                    t = xx @ ww[:, :, ky, kx]                                   # [b, h, w, co]
                    for iy in range(h):
                        oy = 2 * iy - pad + ky
                        if not 0 <= oy < ho:
                            continue
                        ox = 2 * np.arange(wd) - pad + kx
                        ok = (ox >= 0) & (ox < wo)
                        out[which][:, oy, ox[ok]] += t[:, iy, ok]
            continue
        s = 1 if c['geom'] == 's1' else 2
        xp = np.zeros((b, h + 2 * pad, wd + 2 * pad, xx.shape[3]))
        xp[:, pad:pad + h, pad:pad + wd] = xx
        for ky in range(k):
            for kx in range(k):
                out[which] += xp[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s] @ ww[:, :, ky, kx].T
    return out


def reference(c, d):
    x, w = d['x'].double().numpy(), d['w'].double().numpy()
    conv, mag = conv64(c, x, w)
    # the eval affine as gbn_eval_affine_kernel forms it, in float64 of the fp32 tables
    inv = 1.0 / np.sqrt(d['rv'].double().numpy() + EPS)
    scale = d['gamma'].double().numpy() * inv
    shift = d['beta'].double().numpy() - d['rm'].double().numpy() * scale
    bias = d['bias'].double().numpy()
    v = (conv + bias) * scale + shift
    m = (mag + np.abs(bias)) * np.abs(scale) + np.abs(shift)
    if d['res'] is not None:
        v = v + d['res'].double().numpy()
        m = m + np.abs(d['res'].double().numpy())
    if c['act'] == 'relu' or d['res'] is not None:
        v = np.maximum(v, 0.0)
    elif c['act'] == 'lrelu':
        v = np.where(v > 0, v, 0.2 * v)
    return v, m


def device_out(c, pad):
    ho, wo = out_size(c)
    wide = torch.full((c['b'], ho, wo, c['co'] + 2 * pad), SENTINEL, device='cuda')
    return wide, wide[..., pad:pad + c['co']] if pad else wide


@pytest.mark.parametrize('name', [c['name'] for c in CASES])
def test_affine_epilogue_elementwise_and_bitwise(name):
    from proxytta.engine import op_gbn, op_gconv, op_gconv_affine
    c = {k['name']: k for k in CASES}[name]
    d = make(c)
    dev = {k: (None if v is None else v.cuda()) for k, v in d.items()}
    pad = 8 if c['views'] else 0          # the output and the residual as the middle channels of maps 16 channels wider
    res = None
    if c['res']:
        rwide, res = device_out(c, pad)
        res.copy_(dev['res'])
    act = 'relu' if c['res'] else c['act']
    # unfused: the convolution without an activation, then the eval BatchNorm (which leaves its affine table in st)
    raw_wide, raw = device_out(c, 0)
    form0, _ = op_gconv(dev['x'], dev['w'], raw, bias=dev['bias'], k=c['k'], geom=c['geom'])
    st = torch.zeros(4, c['co'], device='cuda')
    un_wide, un = device_out(c, pad)
    op_gbn('eval', raw, un, st, dev['gamma'], beta=dev['beta'], res=res, act=act, res_relu=True, eps=EPS, rm=dev['rm'], rv=dev['rv'])
    # fused, from the same table
    fu_wide, fu = device_out(c, pad)
    form = op_gconv_affine(dev['x'], dev['w'], fu, st[2], st[3], bias=dev['bias'], res=res, k=c['k'], geom=c['geom'], act=act)
    torch.cuda.synchronize()
    assert form == c['form'] == form0
    assert torch.equal(fu_wide, un_wide), 'fused and unfused differ by %.3e' % float((fu_wide - un_wide).abs().max())
    if pad:                                # channels outside the view keep the sentinel
        assert bool((fu_wide[..., :pad] == SENTINEL).all()) and bool((fu_wide[..., pad + c['co']:] == SENTINEL).all())
    ref, mag = reference(c, d)
    err = np.abs(fu.cpu().double().numpy() - ref)
    ratio = float((err / mag).max())
    print('%s: largest |y - float64| / bound magnitude %.3e (TOL x3 %.3e)' % (name, ratio, TOL['x3']))
    assert ratio <= TOL['x3'], ratio
    assert float(np.abs(ref).max()) > 0.5          # (the case computes something)


def test_refused_arguments_return_22_before_any_launch():
    from proxytta.engine import op_gconv_affine
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 9, 13, 64, generator=g).cuda()
    w = torch.randn(64, 64, 3, 3, generator=g).cuda()
    tab = torch.ones(2 * 64 + 8, device='cuda')
    scale, shift = tab[:64], tab[64:128]
    res = torch.zeros(1, 9, 13, 64, device='cuda')

    def refused(**kw):
        y = torch.full((1, kw.pop('ho', 9), kw.pop('wo', 13), kw.pop('co', 64)), SENTINEL, device='cuda')
        args = dict(x0=x, weight=w, y=y, scale=scale, shift=shift)
        args.update(kw)
        with pytest.raises(RuntimeError, match=r'\(-22\)'):
            op_gconv_affine(**args)
        torch.cuda.synchronize()
        assert bool((y == SENTINEL).all()), 'the output was written'

    refused(scale=tab[1:65])                                   # 4 bytes off a 16-byte boundary
    refused(shift=tab[65:129])
    refused(res=res, ld_res=0)                                 # a residual without its pixel stride
    refused(ld_res=64)                                         # ... and a stride without a residual
    refused(res=res, ld_res=32)                                # stride below the channel count
    # channel counts the matrix-core forms do not take: multiples of 8 (stride 1) / of 16 (strided) only
    refused(x0=x[..., :12].contiguous(), weight=w[:, :12].contiguous())
    refused(x0=x[..., :24].contiguous(), weight=w[:, :24].contiguous(), geom='s2', ho=5, wo=7)
    refused(impl='direct')                                     # the direct fp32 kernels have no such epilogue
    refused(act='sigmoid')
    refused(accumulate=True)
    # and the arguments above are fine when they are right
    y = torch.full((1, 9, 13, 64), SENTINEL, device='cuda')
    op_gconv_affine(x, w, y, scale, shift, res=res, act='relu')
    torch.cuda.synchronize()
    assert bool((y != SENTINEL).all())
