"""The residual forms and the bf16x6 images of the affine epilogue of the generic engine's matrix-core convolutions (csrc/gconv_x3_s1.hip and gconv_x3_strided.hip,
GX3Args::aff_act_first / aff_res_plain / six_B with GX3Args::scale), through ptta_op_gconv_affine -- what the stage-2 head trainer runs where
a frozen BatchNorm2d follows a convolution (option "head_bn_fused"):
    act        y = act(fmaf(conv + bias, scale[c], shift[c]))
    res_relu   y = relu(fmaf(..) + res)                          a BasicBlock's bn2
    act_first  y = relu(relu(fmaf(..)) + res)                    CostDCNet's ResBlock      PTTA_GCONV_AFF_ACT_FIRST
    res_plain  y = fmaf(..) + res                                the 2layers block          PTTA_GCONV_AFF_RES_PLAIN
each with six_b = 0, 1 and 2 of b = 2 images in bf16x6 (one case: half the batch bf16x6, half bf16x3).

The oracle is the unfused pair: ptta_op_gconv (no activation, the same six_b) followed by ptta_op_gbn in mode PTTA_GBN_EVAL with the same
act / act_first / res_relu.  Both write the same expressions in the same order, so the comparison is torch.equal over the whole buffer, the
channels outside a view included.  No tolerance, and no element left out: make() moves beta of a channel (the inner ReLU) or the residual of
an element (the outer one) until no float64 pre-activation lies within TIE of zero, as tests/gbn_cases.py does, so that a one-ulp
disagreement could not hide behind a ReLU either.

tests/test_gpu_gconv_affine.py holds the float64 restatement of the epilogue's first form; the forms here differ from it by exact
operations only (a select, one fp32 add), and the bf16x6 convolution itself is checked per element by tests/test_gpu_gconv_elementwise.py."""
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
EPS = 1e-5
TIE = 2.0 ** -18
SENTINEL = -777.25
FORMS = ('act', 'res_relu', 'act_first', 'res_plain')


def S(name, h, w, ci, co, k=3, geom='s1', act='relu', form=None, views=False):
    return dict(name=name, b=2, h=h, w=w, ci=ci, co=co, k=k, geom=geom, act=act, form=form, views=views)


# b = 2 everywhere: more than one block.  9 x 40: one row into the second 8-row tile, the second 32-pixel tile 8 wide (W no multiple of 32);
# stride 2: 9 x 40 -> 5 x 20, an odd input height (the second row of the last row pair outside).  48, 96, 16: channel counts that are no
# multiple of 32.  views: the output and the residual are the middle channels of maps 16 channels wider (ldy > co, ld_res > co).
# The last two shapes are beyond the table of the stage-2 layers: no strided layer of that table has the four 32-channel input chunks
# the K-split form needs (ptta_gconv_x3_strided_form), and NLSPN's conv4.0 does.
SHAPES = [
    S('s1_64_64', 9, 40, 64, 64),                                                  # a BasicBlock / ResBlock convolution
    S('s1k1_128_16', 9, 40, 128, 16, k=1, act='none'),                              # Encoder2D's conv2
    S('s2_64_96', 9, 40, 64, 96, geom='s2', form='plain', views=True),              # enc2d.layer2.0.conv1: three channel tiles, one per wave
    S('s2_96_128', 9, 40, 96, 128, geom='s2', form='nco2'),                         # enc2d.layer3.0.conv1: two channel tiles per wave
    S('s2k1_64_96', 9, 40, 64, 96, k=1, geom='s2', act='none', form='plain'),       # enc2d.layer2.0.downsample.0
    S('s1_256_48_views', 9, 40, 256, 48, act='lrelu', views=True),                  # the 2layers block's second convolution into fe1[:, :48]
    S('s1_64_16', 9, 40, 64, 16),                                                   # CostDCNet's 2layers block: 64 -> 16
    S('s2_128_256_ksplit', 9, 40, 128, 256, geom='s2', form='ksplit'),              # conv4.0.conv1: K split over the block's waves
    S('s2k1_128_256_ksplit', 9, 40, 128, 256, k=1, geom='s2', act='none', form='ksplit'),
]
CASES = [(s['name'], f) for s in SHAPES for f in FORMS]


def out_size(c):
    return (c['h'], c['w']) if c['geom'] == 's1' else ((c['h'] + 1) // 2, (c['w'] + 1) // 2)


def switches(c, form):
    """(act, act_first, res_relu, has_res) of the BatchNorm the form stands for"""
    if form == 'act':
        return c['act'], False, True, False
    if form == 'res_relu':
        return 'relu', False, True, True
    if form == 'act_first':
        return 'relu', True, True, True
    return 'none', False, False, True


def make(c, form):
    g = torch.Generator().manual_seed(zlib.crc32((c['name'] + form).encode()))
    ho, wo = out_size(c)
    act, act_first, res_relu, has_res = switches(c, form)
    d = dict(x=torch.randn(c['b'], c['h'], c['w'], c['ci'], generator=g),
             w=torch.randn(c['co'], c['ci'], c['k'], c['k'], generator=g) * float(c['k'] * c['k'] * c['ci']) ** -0.5,
             bias=torch.randn(c['co'], generator=g) * 0.5,
             gamma=0.5 + torch.rand(c['co'], generator=g), beta=torch.randn(c['co'], generator=g) * 0.3,
             rm=torch.randn(c['co'], generator=g) * 0.4, rv=0.3 + 2.0 * torch.rand(c['co'], generator=g),
             res=torch.randn(c['b'], ho, wo, c['co'], generator=g) if has_res else None)
    d['gamma'][::5] *= -1.0              # negative scales too
    # off the ReLU ties, in float64: the inner pre-activation by the channel's beta, the outer one by the element's residual
    conv = F.conv2d(d['x'].double().permute(0, 3, 1, 2), d['w'].double(), d['bias'].double(), stride=1 if c['geom'] == 's1' else 2,
                    padding=c['k'] // 2).permute(0, 2, 3, 1)
    scale = d['gamma'].double() / torch.sqrt(d['rv'].double() + EPS)
    for _ in range(8):
        inner = conv * scale + (d['beta'].double() - d['rm'].double() * scale)
        mag = conv.abs() * scale.abs() + (d['beta'].double().abs() + d['rm'].double().abs() * scale.abs())
        tie_c = ((inner.abs() < TIE * mag).reshape(-1, c['co']).any(0)) if act != 'none' else torch.zeros(c['co'], dtype=torch.bool)
        outer_tie = None
        if has_res and res_relu:
            v = inner.clamp(min=0) if act_first else inner
            outer = v + d['res'].double()
            outer_tie = outer.abs() < TIE * (mag + d['res'].double().abs())
        if not bool(tie_c.any()) and (outer_tie is None or not bool(outer_tie.any())):
            return d
        d['beta'][tie_c] += 2.0 ** -9
        if outer_tie is not None:
            d['res'][outer_tie] += 2.0 ** -9
    raise AssertionError('no tie-free input found for ' + c['name'])


def device_out(c, pad):
    ho, wo = out_size(c)
    wide = torch.full((c['b'], ho, wo, c['co'] + 2 * pad), SENTINEL, device='cuda')
    return wide, wide[..., pad:pad + c['co']] if pad else wide


@pytest.mark.parametrize('name,form', CASES)
def test_forms_equal_the_unfused_pair_bit_for_bit(name, form):
    from proxytta.engine import op_gbn, op_gconv, op_gconv_affine
    c = {s['name']: s for s in SHAPES}[name]
    act, act_first, res_relu, has_res = switches(c, form)
    d = make(c, form)
    dev = {k: (None if v is None else v.cuda()) for k, v in d.items()}
    pad = 8 if c['views'] else 0
    res = None
    if has_res:
        _, res = device_out(c, pad)
        res.copy_(dev['res'])
    outs = {}
    for six_b in (0, 1, 2):
        # unfused: the convolution without an activation, then the eval BatchNorm (which leaves its affine table in st)
        _, raw = device_out(c, 0)
        form0, _ = op_gconv(dev['x'], dev['w'], raw, bias=dev['bias'], k=c['k'], geom=c['geom'], six_b=six_b)
        st = torch.zeros(4, c['co'], device='cuda')
        un_wide, un = device_out(c, pad)
        op_gbn('eval', raw, un, st, dev['gamma'], beta=dev['beta'], res=res, act=act, act_first=act_first, res_relu=res_relu, eps=EPS,
               rm=dev['rm'], rv=dev['rv'])
        # fused, from the same table
        fu_wide, fu = device_out(c, pad)
        got = op_gconv_affine(dev['x'], dev['w'], fu, st[2], st[3], bias=dev['bias'], res=res, k=c['k'], geom=c['geom'], act=act,
                              act_first=form == 'act_first', res_plain=form == 'res_plain', six_b=six_b)
        torch.cuda.synchronize()
        assert got == c['form'] == form0, (got, form0)
        assert torch.equal(fu_wide, un_wide), 'six_b %d: fused and unfused differ by %.3e' % (six_b, float((fu_wide - un_wide).abs().max()))
        if pad:                            # channels outside the view keep the sentinel
            assert bool((fu_wide[..., :pad] == SENTINEL).all()) and bool((fu_wide[..., pad + c['co']:] == SENTINEL).all())
        assert float(fu.abs().max()) > 0.5 and bool(torch.isfinite(fu).all())          # (the case computes something)
        outs[six_b] = fu.clone()
    # the split is per image: image 1 of six_b = 1 is the bf16x3 one, image 0 the bf16x6 one -- and the two arithmetics do differ
    assert torch.equal(outs[1][0], outs[2][0]) and torch.equal(outs[1][1], outs[0][1])
    assert not torch.equal(outs[0], outs[2])


def test_every_strided_launch_form_occurs():
    """one channel tile per wave, two, and K split: a change of ptta_gconv_x3_strided_form cannot silently drop one from the cases above"""
    from proxytta.engine import op_gconv
    want = {s['form'] for s in SHAPES if s['geom'] == 's2'}
    assert want == {'plain', 'nco2', 'ksplit'}
    for c in SHAPES:
        if c['geom'] != 's2':
            continue
        ho, wo = out_size(c)
        x = torch.zeros(c['b'], c['h'], c['w'], c['ci'], device='cuda')
        w = torch.zeros(c['co'], c['ci'], c['k'], c['k'], device='cuda')
        y = torch.zeros(c['b'], ho, wo, c['co'], device='cuda')
        got, _ = op_gconv(x, w, y, k=c['k'], geom='s2')
        assert got == c['form'], (c['name'], got)


def test_refused_combinations_return_22_before_any_launch():
    from proxytta.engine import op_gconv_affine
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 9, 13, 64, generator=g).cuda()
    w = torch.randn(64, 64, 3, 3, generator=g).cuda()
    tab = torch.ones(2 * 64, device='cuda')
    scale, shift = tab[:64], tab[64:]
    res = torch.zeros(2, 9, 13, 64, device='cuda')

    def refused(**kw):
        y = torch.full((2, 9, 13, 64), SENTINEL, device='cuda')
        args = dict(x0=x, weight=w, y=y, scale=scale, shift=shift)
        args.update(kw)
        with pytest.raises(RuntimeError, match=r'\(-22\)'):
            op_gconv_affine(**args)
        torch.cuda.synchronize()
        assert bool((y == SENTINEL).all()), 'the output was written'

    refused(act_first=True, act='relu')                                  # act_first without a residual
    refused(act_first=True, act='lrelu', res=res)                        # ... with an activation that is not ReLU
    refused(act_first=True, act='none', res=res)
    refused(res_plain=True, act='relu', res=res)                         # a plain residual with an activation
    refused(res_plain=True, act='none')                                  # ... without its residual
    refused(act_first=True, res_plain=True, act='relu', res=res)         # both bits
    refused(act_first=True, res_plain=True, act='none', res=res)
    refused(six_b=3, act='relu')                                         # more bf16x6 images than the batch has
    # and each is fine when it is right
    for kw in (dict(act_first=True, act='relu', res=res), dict(res_plain=True, act='none', res=res), dict(six_b=2, act='relu')):
        y = torch.full((2, 9, 13, 64), SENTINEL, device='cuda')
        op_gconv_affine(x, w, y, scale, shift, **kw)
        torch.cuda.synchronize()
        assert bool((y != SENTINEL).all())
