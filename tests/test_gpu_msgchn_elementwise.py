"""The MSG_CHN step's first-layer / prediction convolutions (csrc/conv_small.hip), resamplings (csrc/resample.hip) and loss (csrc/loss.hip)
per element, through the stand-alone hooks (include/ptta.h ptta_op_conv_in, ptta_op_conv_out1, ptta_op_prep, ptta_op_up2*, ptta_op_loss):
every kernel and launch form against the plain float64 references of oracle/msgchn_arith.py on the cases of tests/msgchn_cases.py.

Exact operations are compared with array_equal; arithmetic against the float64 reference within the bound of tests/msgchn_cases.py (4 x the
CPU emulation's own error + the device library's documented error, never a GPU figure), every element, none excluded.  Output buffers start
NaN-filled: a pixel no kernel writes fails.  Each comparison prints its largest ratio; profiles/msgchn_elementwise.txt keeps them."""
import numpy as np
import pytest
import torch

from oracle import msgchn_arith as A
from tests import msgchn_cases as G
from tests.util import assert_elementwise

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
NAN = float('nan')


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, F32)).cuda()


def nans(*shape):
    return torch.full(shape, NAN, device='cuda')


def host(t):
    return None if t is None else t.cpu().numpy()


def as4(a):
    a = np.asarray(a)
    return a.reshape((1,) * (4 - a.ndim) + a.shape) if a.ndim <= 4 else a.reshape((-1,) + a.shape[-3:])


PLANAR = ('conv_out1', 'up2', 'up2t', 'pool', 'gdepth')          # [b][y][x] maps: one channel, so that a failure names the pixel's tile position


def check(name, q, got, ref, mag, narrow=False):
    got, ref, mag = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(mag, F64)
    print('msgchn %s %s: largest |error| / magnitude %.3e (TOL %.3e)' % (q, name, G.ratio(got, ref, mag), G.tol(q)))
    shape = (lambda a: a[..., None]) if q in PLANAR else as4
    assert_elementwise(shape(got), shape(ref), shape(G.bound(q, mag, ref, narrow)), '%s %s' % (q, name))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def refused(fn):
    with pytest.raises(RuntimeError, match=r'\(-22\)'):
        fn()


# ---- the first-layer convolution -----------------------------------------------------------------------------------------------------------
def run_conv_in(c, d, dtype, cap, naive=False):
    from proxytta.engine import op_conv_in
    b, h, w = c['b'], c['h'], c['w']
    float_mask = c['mask'] in ('float', 'both') or (naive and c['mask'])
    bits = None
    if c['mask'] in ('bits', 'both') and not naive:
        bits = torch.from_numpy(A.sign_bits(d['mask']).view(np.int32)).cuda()
    out_raw = nans(b, h, w, 32) if c['want'] in ('raw', 'both') else None
    out_sum = nans(b, h, w, 32) if c['want'] in ('sum', 'both') else None
    a_bits = None
    if c['a_bits_nb'] and dtype == 'fp32' and not naive:
        a_bits = torch.full((b, h, w), -1, dtype=torch.int32, device='cuda')
    form = op_conv_in([(dev(p), norm) for p, norm in d['planes']], dev(d['weight']), b, h, w, bias=dev(d['bias']), cin_total=c['cin_total'],
                      cin_first=c['cin_first'], transpose_flip=c['flip'], up=dev(d['up']), mask=dev(d['mask']) if float_mask else None, mask_bits=bits,
                      add1=dev(d['add1']), out_raw=out_raw, out_sum=out_sum, a_bits=a_bits, a_bits_nb=c['a_bits_nb'] if a_bits is not None else 0,
                      zero_from_b=c['zero_from_b'], dtype=dtype, naive=naive, max_blocks=cap)
    return form, dict(raw=host(out_raw), sum=host(out_sum), bits=host(a_bits))


CONV_IN_PARAMS = [(c, dt) for c in G.CONV_IN_CASES for dt in c['dtypes']]


@pytest.mark.parametrize('c,dtype', CONV_IN_PARAMS, ids=lambda v: v['name'] if isinstance(v, dict) else v)
def test_conv_in(c, dtype):
    """Every pixel of every tile position: exact, ragged and one-pixel tiles, maps smaller than a tile, a block walking the tiles of several
    frames (max_blocks), b % nb planes, the padded K of cin = 2, a sub-weight, the flipped gradient packing, normalised planes whose padding
    must stay zero (a normalised zero is about -2 per channel: a border pixel would miss the reference by whole units), every epilogue."""
    nar = dtype != 'fp32'
    d = G.make_conv_in(c, dtype)
    ref = A.conv_in_ref(**G.conv_in_kwargs(c, d))
    name = '%s %s' % (c['name'], dtype)
    first = None
    for cap in c['caps']:
        form, got = run_conv_in(c, d, dtype, cap)
        assert form == c['form'], (form, c['form'])
        for k in ('raw', 'sum'):
            if got[k] is None:
                continue
            check('%s cap %d %s' % (name, cap, k), 'conv_in', got[k], ref[k], ref['mag_' + k], nar)
            if c['zero_from_b'] < c['b'] and d['up'] is None:
                # a zero-input frame: the accumulator is exactly 0, so the output is the bias (masked), plus the addend in one fp32 addition
                z = np.zeros((c['b'], c['h'], c['w'], 32), F32) + (F32(0) if d['bias'] is None else d['bias'])
                if d['mask'] is not None:
                    z = np.where(d['mask'] > 0, z, F32(0))
                if k == 'sum' and d['add1'] is not None:
                    z = (z + d['add1'][np.arange(c['b']) % d['add1'].shape[0]]).astype(F32)
                z = A.bf16_round(z) if nar else z
                assert np.array_equal(got[k][c['zero_from_b']:], z[c['zero_from_b']:]), name
        if got['bits'] is not None:
            nb = c['a_bits_nb']
            assert np.array_equal(got['bits'][:nb].view(np.uint32), A.sign_bits(got['raw'][:nb])), name         # the words of the stored values
            assert (got['bits'][nb:] == -1).all(), name                                                       # frames beyond a_bits_nb keep their fill
        if first is None:
            first = got
        else:                                               # a capped and an uncapped grid: the same values to the bit
            assert all(first[k] is None or same_bits(first[k], got[k]) for k in ('raw', 'sum')), (name, cap)
            assert first['bits'] is None or np.array_equal(first['bits'], got['bits'])
    if not nar:
        form, got = run_conv_in(c, d, dtype, 0, naive=True)
        assert form == 'naive'
        for k in ('raw', 'sum'):
            if got[k] is not None:
                check('%s naive %s' % (name, k), 'conv_in', got[k], ref[k], ref['mag_' + k])


def test_conv_in_refusals():
    from proxytta.engine import op_conv_in
    b, h, w = 2, 8, 32
    plane, wt = torch.zeros(b, h, w, device='cuda'), torch.zeros(32, 2, 3, 3, device='cuda')
    fmap = torch.ones(b, h, w, 32, device='cuda')
    out, bits = nans(b, h, w, 32), torch.full((b, h, w), -1, dtype=torch.int32, device='cuda')
    go = lambda **kw: (lambda: op_conv_in([(plane, None)], wt, b, h, w, cin_total=2, out_raw=out, **kw))
    refused(go(mask=fmap, dtype='mixed'))                                   # a narrow launch reads its ReLU mask as bit words only
    refused(go(cin_first=2))                                                # past the weight's input channels
    refused(lambda: op_conv_in([(plane, None)], wt, b, 7, w, cin_total=2, out_raw=out, up=fmap))     # bilinear x2 of an odd map
    refused(go(mask_bits=bits, add1=fmap, out_sum=nans(b, h, w, 32)))       # the direct form reads the mask as a map
    refused(go(a_bits=bits, a_bits_nb=1, add1=fmap, out_sum=nans(b, h, w, 32)))   # only the LDS-staged forms write the words
    refused(go(a_bits=bits, a_bits_nb=3))                                   # more frames than the batch
    refused(go(max_blocks=-1))
    small = nans(1, 8, 8, 32)
    refused(lambda: op_conv_in([(torch.zeros(1, 8, 8, device='cuda'), None)], wt, 1, 8, 8, cin_total=2, out_raw=small,
                               up=fmap.reshape(-1)[1:1 + 4 * 4 * 32].reshape(1, 4, 4, 32)))                 # an NHWC operand off its 16-byte alignment
    assert torch.isnan(out).all() and torch.isnan(small).all() and (bits == -1).all()


# ---- the prediction convolution ------------------------------------------------------------------------------------------------------------
CONV_OUT1_PARAMS = [(c, dt) for c in G.CONV_OUT1_CASES for dt in c['dtypes']]


@pytest.mark.parametrize('c,dtype', CONV_OUT1_PARAMS, ids=lambda v: v['name'] if isinstance(v, dict) else v)
def test_conv_out1(c, dtype):
    from proxytta.engine import op_conv_out1
    d = G.make_conv_out1(c, dtype)
    ref, mag = A.conv_out1_ref(**G.conv_out1_kwargs(c, d))
    first = None
    for cap in c['caps']:
        out = nans(c['b'], c['h'], c['w'])
        op_conv_out1(dev(d['x']), dev(d['weight']), out, bias=dev(d['bias']), add=dev(d['add']), relu_in=c['relu'], src_cin_total=2 if c['from_conv_in'] else 0,
                     src_cin_index=1 if c['from_conv_in'] else 0, from_conv_in=c['from_conv_in'], dtype=dtype, max_blocks=cap)
        got = host(out)
        check('%s %s cap %d' % (c['name'], dtype, cap), 'conv_out1', got, ref, mag)         # (the output plane is fp32 in both modes)
        first = got if first is None else first
        assert same_bits(first, got), (c['name'], cap)


def test_conv_out1_refusals():
    from proxytta.engine import op_conv_out1
    x, out = torch.ones(2, 8, 32, 32, device='cuda'), nans(2, 8, 32)
    refused(lambda: op_conv_out1(x, torch.zeros(32, 2, 3, 3, device='cuda'), out, src_cin_total=2, src_cin_index=2, from_conv_in=True))
    refused(lambda: op_conv_out1(torch.ones(3, 8, 32, 32, device='cuda'), torch.zeros(1, 32, 3, 3, device='cuda'), out))      # more input frames than the batch
    refused(lambda: op_conv_out1(x, torch.zeros(1, 32, 3, 3, device='cuda'), out, add=torch.zeros(3, 8, 32, device='cuda')))
    refused(lambda: op_conv_out1(x.reshape(-1)[1:1 + 8 * 32 * 32].reshape(1, 8, 32, 32), torch.zeros(1, 32, 3, 3, device='cuda'), out))      # 16-byte loads
    assert torch.isnan(out).all()


# ---- resampling ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hin,win', G.UP_SIZES, ids=lambda v: str(v))
def test_up2_and_its_transposes(hin, win):
    from proxytta.engine import op_up2
    d = G.make_up(hin, win)
    name = '%dx%d' % (hin, win)
    B = G.UP_B
    ref_u, mag_u = A.up2_ref(d['x'])
    up = host(op_up2(dev(d['x']), nans(B, 2 * hin, 2 * win)))
    check(name, 'up2', up, ref_u, mag_u)
    ref_t, mag_t = A.up2t_ref(d['g'])
    upt = host(op_up2(dev(d['g']), nans(B, hin, win), transposed=True))
    check(name, 'up2t', upt, ref_t, mag_t)
    # the adjoint identity on the GPU's own outputs: <up2(x), g> = <x, up2T(g)> within the two bounds
    lhs, rhs = (up.astype(F64) * d['g']).sum(), (d['x'].astype(F64) * upt).sum()
    slack = (G.bound('up2', mag_u) * np.abs(d['g'])).sum() + (np.abs(d['x']) * G.bound('up2t', mag_t)).sum()
    print('msgchn adjoint %s: |<up2 x, g> - <x, up2T g>| %.3e (allowed %.3e)' % (name, abs(lhs - rhs), slack))
    assert abs(lhs - rhs) <= slack, (name, lhs, rhs, slack)
    for dtype in ('fp32', 'mixed'):
        dn = G.make_up(hin, win, dtype != 'fp32')
        for add in (None, dn['add32']):
            ref, mag = A.up2t_ref(dn['g32'], add)
            got = host(op_up2(dev(dn['g32']), nans(B, hin, win, 32), transposed=True, add=dev(add), dtype=dtype))
            check('%s %s add %d' % (name, dtype, add is not None), 'up2t32', got, ref, mag, dtype != 'fp32')


@pytest.mark.parametrize('c', G.PREP_CASES, ids=lambda c: c['name'])
def test_prep(c):
    from proxytta.engine import op_prep
    s = G.make_prep(c)
    n, h, w = s.shape
    dclamp, d12, d14 = nans(n, h, w), nans(n, h // 2, w // 2), nans(n, h // 4, w // 4)
    op_prep(dev(s), c['max_d'], dclamp, d12, d14)
    dc, ref = A.prep_ref(s, c['max_d'])
    assert np.array_equal(host(dclamp), dc)
    if c['max_d'] < 0:
        assert same_bits(host(dclamp), s)                       # the clamp is off: a copy to the bit
    elif h > 4:
        assert (s > c['max_d']).any() and (s < 0).any()
    for k, t in ((2, d12), (4, d14)):
        got = host(t)
        check('%s 1/%d' % (c['name'], k), 'pool', got, *ref[k])
        empty = ref[k][1] == 0                                  # a block without a valid point: 0 / (0 + 1e-4)
        assert empty.any() and (got[empty] == 0).all()


def test_resampling_refusals():
    from proxytta.engine import op_prep, op_up2
    for h, w in ((6, 8), (8, 6), (2, 8)):
        outs = nans(1, h, w), nans(1, h // 2, w // 2), nans(1, max(h // 4, 1), max(w // 4, 1))
        refused(lambda: op_prep(torch.zeros(1, h, w, device='cuda'), 5.0, *outs))
        assert all(torch.isnan(t).all() for t in outs)
    out = nans(1, 40000, 1)
    refused(lambda: op_up2(torch.zeros(1, 80000, 2, device='cuda'), out, transposed=True))          # more rows than a grid dimension holds
    assert torch.isnan(out).all()


# ---- the loss ----------------------------------------------------------------------------------------------------------------------------------
LOSS_FORMS = [('merged', 'none'), ('nocos', 'none'), ('split', 'none'), ('split_narrow', 'none'), ('merged', 'unfused'), ('split', 'unfused'),
              ('nocos', 'unfused'), ('merged', 'fused'), ('nocos', 'fused'), ('split', 'counted'), ('split_narrow', 'counted')]


@pytest.mark.parametrize('c', G.LOSS_CASES, ids=lambda c: c['name'])
def test_loss_every_launch_form(c):
    """Values, row statistics, coefficients and both gradients of every launch form against autograd in float64; the depth gradient of all
    backward forms bit-identical (csrc/loss.hip claims the same partials, order and expressions for them); gref exactly zero behind a
    closed gate; the gradient exactly zero where every sign function sees a tie."""
    from proxytta.engine import op_loss
    d = G.make_loss(c)
    refs = {cos: A.loss_ref(**G.loss_args(c, d, cos)) for cos in (True, False)}
    assert abs(refs[True]['info'][3] - 0.3) >= G.GATE_MARGIN
    N, H, W, R, D = c['n'], c['h'], c['w'], c['r'], c['d']
    dv = {k: dev(v) for k, v in d.items()}
    gd_first = None
    for fwd, bwd in LOSS_FORMS:
        cos, back = fwd != 'nocos', bwd != 'none'
        ref = refs[cos]
        name = '%s %s/%s' % (c['name'], fwd, bwd)
        info, coef = nans(4), nans(4 + N)
        rowstats = nans(R, 3) if cos else None
        gdepth = nans(N, H, W) if back else None
        gref = nans(R, D) if cos and back else None
        op_loss(fwd, bwd, dv['depth'], dv['image'], dv['sparse'], c['w3'], c['max_d'], validity=dv['validity'], emb=dv['emb'] if cos else None,
                ref=dv['ref'] if cos else None, loss_info=info, rowstats=rowstats, gdepth=gdepth, gref=gref, coef=coef)
        info, coef = host(info), host(coef)
        for k, q in enumerate(G.INFO_Q):
            check(name, q, info[k], ref['info'][k], ref['mag_info'][k])
        check(name, 'coef', coef[:3 + N], ref['coef'], ref['mag_coef'])
        if bwd == 'counted':                             # what loss_cos_coef alone left in the workspace
            check(name + ' cos_coef', 'coef', coef[3 + N], ref['coef'][0], ref['mag_coef'][0])
        else:
            assert np.isnan(coef[3 + N])
        if cos:
            check(name, 'rowstats', host(rowstats), ref['rowstats'], ref['mag_rowstats'])
        if back:
            gd = host(gdepth)
            check(name, 'gdepth', gd, ref['gdepth'], ref['mag_gdepth'])
            assert (gd[ref['gdepth'] == 0] == 0).all() and (ref['gdepth'] == 0).any(), name
            gd_first = gd if gd_first is None else gd_first
            assert same_bits(gd_first, gd), name
        if gref is not None:
            g = host(gref)
            if ref['wc'] == 0:
                assert c['gate'] == 'closed' and (g == 0).all(), name
            else:
                check(name, 'gref', g, ref['gref'], ref['mag_gref'])


def test_loss_refusals():
    from proxytta.engine import op_loss
    n, h, w, r, dm = 1, 8, 12, 5, 16
    depth, image, sparse = torch.ones(n, h, w, device='cuda'), torch.ones(n, 3, h, w, device='cuda'), torch.ones(n, h, w, device='cuda')
    emb = torch.ones(r, dm, device='cuda')
    outs = dict(loss_info=nans(4), rowstats=nans(r, 3), gdepth=nans(n, h, w), gref=nans(r, dm), coef=nans(4 + n))
    go = lambda fwd='merged', bwd='unfused', **kw: (lambda: op_loss(fwd, bwd, depth, image, sparse, (1.0, 2.0, 0.1), 5.0, emb=emb, ref=emb, **outs, **kw))
    refused(go(d=6))                                      # float4 rows
    refused(go(fwd='split_narrow', d=12))                 # narrow rows: eight values per load
    refused(go(shape=(1, 96, 1)))                         # the smoothness counts divide by W - 1 ...
    refused(go(shape=(1, 1, 96)))                         # ... and H - 1
    refused(go(r=0))                                      # a cosine term over no rows
    refused(go(fwd='split', bwd='fused'))                 # no such launch sequence
    refused(go(fwd='merged', bwd='counted'))
    assert all(torch.isnan(t).all() for t in outs.values())
