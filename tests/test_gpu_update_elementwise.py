"""The update half of a step per element, through the stand-alone hooks of csrc/ptta_ops_update.hip (include/ptta.h) against the plain
references of oracle/update_arith.py on the cases of tests/update_cases.py.

Kernels and template instantiations launched here:
  wgrad_adam.hip   wgrad32_kernel<float>, wgrad32_kernel<bf16_t>, wgrad32_reduce_kernel (test_wgrad32); adam_kernel, step_inc_kernel
                   (test_adam_sites_agree, test_adam_in_the_reduction); adam_multi_kernel (test_adam_table, and the two above)
  gwgrad_mfma.hip  gwgrad_x3_kernel<false, true> and <true, true> (32 -> 32, 24 -> 32), <false> and <true> (64 -> 64, 32 -> 128, 128 -> 32),
                   gwgrad_mfma_reduce_kernel without and with GwAdam (test_gwgrad_views, test_adam_in_the_reduction)
  head_train.hip   linear_wgrad_kernel<4, 0, 0>, <4, 0, 1>, <4, 1, 0>, <4, 1, 1>, <1, 0, 0>, <1, 1, 0>, wgrad_reduce_kernel (test_linear_wgrad);
                   ema_multi_kernel (test_ema_table)
  ghead.hip        glinear_wgrad_kernel (test_glinear_wgrad)

Real-valued outputs: every element within TOL x 2^-24 x its scale of the float64 reference, TOL = 4 x the ratio of the CPU emulation on the
SAME case (tests/update_cases.py, tests/update_ratios.py; never a GPU figure).  Exact classes -- the same launch through two hooks, a
strided view against the dense call, bf16 against fp32 gradients holding the same values (gwgrad_x3_kernel widens on load and then runs the same instructions on the same grid, so
bits are the bound), the three sites of ptta_adam_update, the EMA -- with array_equal.  Outputs and everything outside a view start as NaN;
what a launch must not touch must still be NaN afterwards.  Each comparison prints its largest ratio; profiles/update_elementwise.txt keeps
them."""
import numpy as np
import pytest
import torch

from oracle import update_arith as A
from tests import update_cases as G
from tests.util import assert_elementwise

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
NAN16 = 0x7fc0
REFUSED = r'\(-22\)'


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype, order='C')).cuda()          # (a copy: the cases' arrays are read-only)


def dev16(a):
    """fp32 values that are bf16 values -> their bit patterns on the device (int16)"""
    return dev(A.bf16_bits(a).view(np.int16))


def nan(n):
    return torch.full((int(n),), float('nan'), device='cuda')


def host(t):
    return t.cpu().numpy()


def ints(v):
    return torch.tensor([v], dtype=torch.int32, device='cuda')


def as4(a):
    a = np.asarray(a, F64)
    return a.reshape((1,) * (4 - a.ndim) + a.shape)


def check(op, case, q, got, ref, scale, what=''):
    """every element within the CASE's own bound (tests/update_cases.py: 4 x the emulation's ratio on this case x 2^-24 x scale)"""
    got, ref = np.asarray(got, F64).reshape(np.shape(ref)), np.asarray(ref, F64)
    print('update %s %s/%s %s: largest |error| / (2^-24 scale) %.4e (TOL %.4e)' % (q, op, case, what, G.ratio(got, ref, scale), G.tol(op, case, q)))
    assert_elementwise(as4(got), as4(ref), as4(G.bound(op, case, q, scale)), '%s %s/%s %s' % (q, op, case, what))


def same_bits(what, a, b):
    a, b = np.asarray(a), np.asarray(b).reshape(np.shape(a))
    if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
        assert_elementwise(as4(a), as4(b), as4(np.zeros(a.shape)), 'exact ' + what)          # names the worst element
        raise AssertionError('exact %s: bit patterns differ' % what)


def split_pad(t, n):
    """the first n elements of a padded output, after asserting that they are numbers and the padding still NaN"""
    full = host(t)
    assert not np.isnan(full[:n]).any() and np.isnan(full[n:]).all()
    return full[:n]


# ---- wgrad32 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', G.WGRAD32_CASES, ids=lambda c: c['name'])
def test_wgrad32(c):
    from proxytta.engine import op_wgrad32
    b, h, w, cs, grp = c['b'], c['h'], c['w'], c['co_stride'], c['group']
    x, gy, ref, mag = G.wgrad32_data(b, h, w, c['bf16'])
    up = dev16 if c['bf16'] else dev
    gw, gb = nan(32 * cs + G.PAD), nan(32 + G.PAD) if c['bias'] else None
    op_wgrad32(up(x), up(gy), b, h, w, gw[288 * grp:], gb, co_stride=cs, bf16=c['bf16'])
    full = host(gw)
    wfull = full[:32 * cs].reshape(32, cs // 9, 9)
    got = wfull[:, 32 * grp:32 * grp + 32]
    assert not np.isnan(got).any()
    assert np.isnan(np.delete(wfull, np.s_[32 * grp:32 * grp + 32], 1)).all() and np.isnan(full[32 * cs:]).all()       # untouched elements
    check('wgrad32', c['data'], 'wgrad32_w', got, ref[0].reshape(32, 32, 9), mag[0].reshape(32, 32, 9), c['name'])
    if c['bias']:
        check('wgrad32', c['data'], 'wgrad32_b', split_pad(gb, 32), ref[1], mag[1], c['name'])


def test_wgrad32_refuses():
    from proxytta.engine import op_wgrad32
    x, gy = dev(np.zeros((1, 2, 2, 32), F32)), dev(np.zeros((1, 2, 2, 32), F32))
    gw = nan(9216)
    for kw in (dict(co_stride=287), dict(b=0), dict(x=None)):
        a = dict(x=x, gy=gy, b=1, h=2, w=2, gw=gw)
        a.update(kw)
        with pytest.raises(RuntimeError, match=REFUSED):
            op_wgrad32(**a)
    assert np.isnan(host(gw)).all()


# ---- gwgrad on views and with bf16 gradients ----------------------------------------------------------------------------------------------
def _gw_run(c, x, gy, **kw):
    from proxytta.engine import op_gwgrad_view
    nw = c['co'] * c['ci'] * 9
    gw, gb = nan(nw + G.PAD), nan(c['co'] + G.PAD)
    op_gwgrad_view(x, gy, c['b'], c['h'], c['w'], c['ci'], c['co'], gw, gb, **kw)
    return split_pad(gw, nw), split_pad(gb, c['co'])


@pytest.mark.parametrize('c', G.GW_CASES, ids=lambda c: c['name'])
def test_gwgrad_views(c):
    from proxytta.engine import op_gwgrad
    ci, co = c['ci'], c['co']
    x, gyf, gy, ref, mag = G.gwgrad_data(ci, co, c['b'], c['h'], c['w'])
    # full fp32 gradients: the new hook is the launch of ptta_op_gwgrad, and that launch is the float64 gradient within the bound
    w0, b0, _ = op_gwgrad(dev(x), dev(gyf))
    full = _gw_run(c, dev(x), dev(gyf))
    same_bits('gw dense call = ptta_op_gwgrad ' + c['name'], host(w0).reshape(-1), full[0])
    same_bits('gb dense call = ptta_op_gwgrad ' + c['name'], host(b0), full[1])
    check('gwgrad', c['name'], 'gwgrad_w', full[0], ref[0], mag[0])
    check('gwgrad', c['name'], 'gwgrad_b', full[1], ref[1], mag[1])
    # gradients that are bf16 values: the dense fp32 call is what every other form of the call must return
    w0, b0 = _gw_run(c, dev(x), dev(gy))
    xb, xo = G.view_buffer(x, G.X_OFF, G.X_PAD)
    gbuf, go = G.view_buffer(gy, G.G_OFF, G.G_PAD)
    bits = np.full(gy.shape[:-1] + (co + G.G_PAD,), NAN16, np.uint16)
    bits[..., G.G_OFF:G.G_OFF + co] = A.bf16_bits(gy)
    runs = (('strided view', _gw_run(c, dev(xb)[xo:], dev(gbuf)[go:], ldx=ci + G.X_PAD, ldg=co + G.G_PAD)),
            ('bf16 gy', _gw_run(c, dev(x), dev16(gy), gy_bf16=True)),
            ('bf16 gy, strided view', _gw_run(c, dev(xb)[xo:], dev(bits.view(np.int16).reshape(-1))[go:], ldx=ci + G.X_PAD, ldg=co + G.G_PAD, gy_bf16=True)))
    for what, got in runs:
        same_bits('gw %s %s' % (what, c['name']), w0, got[0])
        same_bits('gb %s %s' % (what, c['name']), b0, got[1])


@pytest.mark.parametrize('ci,co', G.GW_REFUSED_BF16)
def test_gwgrad_refuses_bf16_without_a_form(ci, co):
    from proxytta.engine import op_gwgrad_view
    gw, gb = nan(co * ci * 9), nan(co)
    with pytest.raises(RuntimeError, match=REFUSED):
        op_gwgrad_view(dev(np.zeros((1, 4, 4, ci), F32)), dev(np.zeros((1, 4, 4, co), np.int16)), 1, 4, 4, ci, co, gw, gb, gy_bf16=True)
    assert np.isnan(host(gw)).all() and np.isnan(host(gb)).all()


# ---- Adam inside the reduction ------------------------------------------------------------------------------------------------------------
def _state(name, n, gscale):
    return [dev(a) for a in G.adam_state(name, n, gscale)]


@pytest.mark.parametrize('c', G.FUSED_CASES, ids=lambda c: c['name'])
def test_adam_in_the_reduction(c):
    """three sites, one ptta_adam_update: the reduction with Adam inside, adam_multi_kernel and adam_kernel on the gradient the plain
    reduction stored -- the same p, m, v bit for bit, and all of them Adam in float64"""
    from proxytta.engine import op_adam, op_adam_multi, op_gwgrad_view
    ci, co, t0 = c['ci'], c['co'], c['start']
    nw = co * ci * 9
    x, gy, _, _, _ = G.gwgrad_data(ci, co, c['b'], c['h'], c['w'])
    xd, gd = dev(x), dev(gy)
    hy = G.hyper_of(G.FUSED_WD)
    hyper = dev(hy)
    geo = (c['b'], c['h'], c['w'], ci, co)
    before_w, before_b = G.adam_state(c['name'] + '/w', nw, 0.3), G.adam_state(c['name'] + '/b', co, 0.3)
    # A: inside the reduction
    sw, sb = _state(c['name'] + '/w', nw, 0.3), _state(c['name'] + '/b', co, 0.3)
    gw, gb, step, ticket = nan(nw + G.PAD), nan(co + G.PAD), ints(t0), ints(0)
    op_gwgrad_view(xd, gd, *geo, gw, gb, adam=dict(pw=sw[0], mw=sw[1], vw=sw[2], pb=sb[0] if c['bias'] else None, mb=sb[1], vb=sb[2],
                                                    hyper=hyper, step=step, ticket=ticket))
    assert int(step.item()) == t0 + 1 and int(ticket.item()) == 0
    gwA, gbA = split_pad(gw, nw), split_pad(gb, co)
    # B: the plain reduction, then adam_multi on its gw / gb
    gw2, gb2 = nan(nw + G.PAD), nan(co + G.PAD)
    op_gwgrad_view(xd, gd, *geo, gw2, gb2)
    same_bits('gw with and without Adam ' + c['name'], gwA, split_pad(gw2, nw))
    same_bits('gb with and without Adam ' + c['name'], gbA, split_pad(gb2, co))
    mw, mb, step2, ticket2 = _state(c['name'] + '/w', nw, 0.3), _state(c['name'] + '/b', co, 0.3), ints(t0), ints(0)
    op_adam_multi([(*mw, gw2[:nw], 1)] + ([(*mb, gb2[:co], 1)] if c['bias'] else []), hyper, step2, ticket2)
    assert int(step2.item()) == t0 + 1 and int(ticket2.item()) == 0
    # C: adam_kernel per tensor
    kw, kb = _state(c['name'] + '/w', nw, 0.3), _state(c['name'] + '/b', co, 0.3)
    step3 = ints(t0)
    op_adam(*kw, gw2[:nw], hyper, step3)
    assert int(step3.item()) == t0 + 1
    if c['bias']:
        op_adam(*kb, gb2[:co], hyper, ints(t0))
    for j, q in enumerate('pmv'):
        same_bits('%s weight, reduction = adam_multi %s' % (q, c['name']), host(sw[j]), host(mw[j]))
        same_bits('%s weight, reduction = adam %s' % (q, c['name']), host(sw[j]), host(kw[j]))
        same_bits('%s bias, reduction = adam_multi %s' % (q, c['name']), host(sb[j]), host(mb[j]))
        same_bits('%s bias, reduction = adam %s' % (q, c['name']), host(sb[j]), host(kb[j]))
        if not c['bias']:
            same_bits('%s bias untouched %s' % (q, c['name']), host(sb[j]), before_b[j])
    for q, what, got, rf, mg in (G.adam_checks('weight', [host(t) for t in sw], before_w, gwA, hy, t0 + 1, 1) +
                                 (G.adam_checks('bias', [host(t) for t in sb], before_b, gbA, hy, t0 + 1, 1) if c['bias'] else [])):
        check('fused', c['name'], q, got, rf, mg, what)


def test_adam_in_the_reduction_refused_past_one_tile_pair():
    from proxytta.engine import op_gwgrad_view
    ci = co = 64
    nw = co * ci * 9
    sw, sb = [nan(nw) for _ in range(3)], [nan(co) for _ in range(3)]
    gw, gb, step, ticket = nan(nw), nan(co), ints(3), ints(0)
    with pytest.raises(RuntimeError, match=REFUSED):
        op_gwgrad_view(dev(np.zeros((1, 4, 4, ci), F32)), dev(np.zeros((1, 4, 4, co), F32)), 1, 4, 4, ci, co, gw, gb,
                       adam=dict(pw=sw[0], mw=sw[1], vw=sw[2], pb=sb[0], mb=sb[1], vb=sb[2], hyper=dev(G.hyper_of(0.0)), step=step, ticket=ticket))
    assert all(np.isnan(host(t)).all() for t in sw + sb + [gw, gb]) and int(step.item()) == 3 and int(ticket.item()) == 0


# ---- the Adam and EMA tables --------------------------------------------------------------------------------------------------------------
def _padded(a):
    """a device copy with G.PAD NaN behind it -> (the whole buffer, the view of the values)"""
    t = nan(a.size + G.PAD)
    t[:a.size] = dev(a)
    return t, t[:a.size]


@pytest.mark.parametrize('c', G.TABLE_CASES, ids=lambda c: c['name'])
def test_adam_table(c):
    """two launches back to back; each checked on its own against the float64 update of the fp32 state it started from"""
    from proxytta.engine import op_adam_multi
    tab, hy = G.table_data(), G.hyper_of(c['wd'])
    hyper, step, ticket = dev(hy), ints(c['start']), ints(0)
    bufs = [[_padded(a) for a in e[:3]] for e in tab]
    for launch in range(2):
        t = c['start'] + 1 + launch
        before = [[host(view).copy() for _, view in b] for b in bufs]
        grads = [nan(e[0].size) if rep == 0 else dev(e[3 + launch]) for e, rep in zip(tab, c['reps'])]
        op_adam_multi([(b[0][1], b[1][1], b[2][1], g, rep) for b, g, rep in zip(bufs, grads, c['reps'])], hyper, step, ticket)
        assert int(step.item()) == t and int(ticket.item()) == 0
        for k, (e, rep) in enumerate(zip(tab, c['reps'])):
            name = 'tensor %d (%d) launch %d' % (k, e[0].size, launch)
            got = [split_pad(full, e[0].size) if rep else host(full)[:e[0].size] for full, _ in bufs[k]]
            if rep == 0:                                    # listed without a gradient: nothing read, nothing written
                for j, q in enumerate('pmv'):
                    same_bits('%s untouched %s %s' % (q, c['name'], name), got[j], before[k][j])
                assert np.isnan(host(grads[k])).all() and all(np.isnan(host(full)[e[0].size:]).all() for full, _ in bufs[k])
                continue
            for q, nm, gt, rf, mg in G.adam_checks(name, got, before[k], e[3 + launch], hy, t, rep):
                check('adam', c['name'], q, gt, rf, mg, nm)


@pytest.mark.parametrize('k', (0, 4, 6))
@pytest.mark.parametrize('start', (0, 99999))
def test_adam_sites_agree(k, start):
    """adam_kernel and adam_multi_kernel with rep = 1 on one tensor: bit for bit"""
    from proxytta.engine import op_adam, op_adam_multi
    p, m, v, g, _ = G.table_data()[k]
    hyper = dev(G.hyper_of(1e-4))
    a, b = [dev(t) for t in (p, m, v)], [dev(t) for t in (p, m, v)]
    sa, sb, ticket = ints(start), ints(start), ints(0)
    op_adam(*a, dev(g), hyper, sa)
    op_adam_multi([(*b, dev(g), 1)], hyper, sb, ticket)
    assert int(sa.item()) == int(sb.item()) == start + 1 and int(ticket.item()) == 0
    for j, q in enumerate('pmv'):
        same_bits('%s adam = adam_multi, tensor %d' % (q, k), host(a[j]), host(b[j]))


def test_adam_table_refuses():
    from proxytta import _lib
    from proxytta.engine import op_adam, op_adam_multi
    p, m, v, g = nan(8), nan(8), nan(8), nan(8)
    hyper, step, ticket = dev(G.hyper_of(0.0)), ints(2), ints(0)
    with pytest.raises(RuntimeError, match=REFUSED):
        op_adam_multi([(p, m, v, None, 1)], hyper, step, ticket)          # a gradient is required where rep != 0
    with pytest.raises(RuntimeError, match=REFUSED):
        op_adam_multi([(p, m, v, g, -1)], hyper, step, ticket)
    with pytest.raises(RuntimeError, match=REFUSED):
        op_adam(p, m, v, None, hyper, step)
    assert _lib.load().ptta_op_adam_multi(0, None, None, None, None, None, None, None, None, None, None) == -22
    assert _lib.load().ptta_op_ema_multi(0, None, None, None, None, None) == -22
    assert int(step.item()) == 2 and all(np.isnan(host(t)).all() for t in (p, m, v, g))


@pytest.mark.parametrize('tau', G.EMA_TAUS)
def test_ema_table(tau):
    from proxytta.engine import op_ema_multi
    tab = G.table_data()
    tau32, omt32 = F32(tau), F32(1.0 - tau)                  # python doubles -> fp32, as the trainer uploads them
    bufs = [_padded(e[0]) for e in tab]
    online = [dev(e[3]) for e in tab]
    op_ema_multi([(view, g) for (_, view), g in zip(bufs, online)], dev(np.array([tau32, omt32], F32)))
    for k, e in enumerate(tab):
        got = split_pad(bufs[k][0], e[0].size)
        same_bits('EMA tau %g tensor %d (%d)' % (tau, k, e[0].size), got, A.ema32(e[0], e[3], tau32, omt32))
        same_bits('EMA online tensor %d untouched' % k, host(online[k]), e[3])


# ---- linear_wgrad ---------------------------------------------------------------------------------------------------------------------------
def _rows_then_nan(a, extra=16):
    """[R][C] on the device with `extra` rows of NaN behind it: rows from R on must not be read"""
    t = nan((a.shape[0] + extra) * a.shape[1])
    t[:a.size] = dev(a).reshape(-1)
    return t


@pytest.mark.parametrize('c', G.LIN_CASES, ids=lambda c: c['name'])
def test_linear_wgrad(c):
    """every row count against the float64 reference: with GPRO the tail rows of the last 16-row slice are fed Gh = mean, and must add
    nothing to dW and nothing to db (the transformed value of such a row would be -gscale c1, and c1 is of G's own size here)"""
    from proxytta.engine import op_linear_wgrad
    O, I, R = c['O'], c['I'], c['R']
    d = G.linear_data(O, I, R)
    kw = G.linear_args(c, d)
    tables = {}
    if c['gpro']:
        tables.update(Gh=_rows_then_nan(d['Gh']), **{k: dev(v) for k, v in d['gt'].items()})
        assert float(np.abs(d['gt']['gc1'] * d['gt']['gscale']).min()) > 0
    if c['xpro']:
        tables.update(xscale=dev(d['xscale']), xshift=dev(d['xshift']))
    dW, db = nan(O * I + G.PAD), nan(O + G.PAD)
    op_linear_wgrad(_rows_then_nan(d['G']), _rows_then_nan(d['X']), R, O, I, dW, db, **tables)
    ref, mag = A.linear_wgrad_ref(d['G'], d['X'], **kw)
    check('linear', c['name'], 'lin_w', split_pad(dW, O * I), ref[0], mag[0])
    check('linear', c['name'], 'lin_b', split_pad(db, O), ref[1], mag[1])


def test_linear_wgrad_without_bias_gradient():
    from proxytta.engine import op_linear_wgrad
    c = next(c for c in G.LIN_CASES if c['name'] == 'k100_o128_i128_r17')
    d = G.linear_data(c['O'], c['I'], c['R'])
    dW = nan(128 * 128 + G.PAD)
    op_linear_wgrad(dev(d['G']), dev(d['X']), 17, 128, 128, dW, None)
    ref, mag = A.linear_wgrad_ref(d['G'], d['X'])
    check('linear', c['name'], 'lin_w', split_pad(dW, 128 * 128), ref[0], mag[0], 'db NULL')


@pytest.mark.parametrize('c', G.LIN_REFUSED, ids=lambda c: 'o%d_i%d_r%d%s' % (c['O'], c['I'], c['R'], '_xscale' if c.get('xpro') else ''))
def test_linear_wgrad_refuses(c):
    from proxytta.engine import op_linear_wgrad
    O, I = c['O'], c['I']
    dW, db = nan(O * I), nan(O)
    tables = dict(xscale=dev(np.ones(I, F32)), xshift=dev(np.zeros(I, F32))) if c.get('xpro') else {}
    with pytest.raises(RuntimeError, match=REFUSED):
        op_linear_wgrad(dev(np.zeros((16, O), F32)), dev(np.zeros((16, I), F32)), c['R'], O, I, dW, db, **tables)
    assert np.isnan(host(dW)).all() and np.isnan(host(db)).all()


# ---- glinear_wgrad --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', G.GLIN_CASES, ids=lambda c: c['name'])
def test_glinear_wgrad(c):
    from proxytta.engine import op_glinear_wgrad
    I, O, R = c['I'], c['O'], c['R']
    x, gy = G.glinear_data(c)
    (xb, xo), (gbuf, go) = G.view_buffer(x, 1, G.GLIN_PAD[0]), G.view_buffer(gy, 2, G.GLIN_PAD[1])
    ref, mag = A.linear_wgrad_ref(gy, x)
    xd, gd = dev(xb), dev(gbuf)
    for with_gb in (True, False):
        gw, gb = nan(O * I + G.PAD), nan(O + G.PAD)
        op_glinear_wgrad(xd[xo:], I + G.GLIN_PAD[0], I, gd[go:], O + G.GLIN_PAD[1], O, R, gw, gb if with_gb else None)
        check('glinear', c['name'], 'glin_w', split_pad(gw, O * I), ref[0], mag[0])
        if with_gb:
            check('glinear', c['name'], 'glin_b', split_pad(gb, O), ref[1], mag[1])
        else:
            assert np.isnan(host(gb)).all()


def test_glinear_wgrad_refuses():
    from proxytta.engine import op_glinear_wgrad
    x, gy, gw = dev(np.zeros((4, 8), F32)), dev(np.zeros((4, 8), F32)), nan(64)
    for a in (dict(r=0), dict(ldx=7), dict(ldg=7), dict(gw=None)):
        kw = dict(x=x, ldx=8, i=8, gy=gy, ldg=8, o=8, r=4, gw=gw)
        kw.update(a)
        with pytest.raises(RuntimeError, match=REFUSED):
            op_glinear_wgrad(**kw)
    assert np.isnan(host(gw)).all()
