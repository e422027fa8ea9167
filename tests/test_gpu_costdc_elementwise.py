"""CostDCNet's own kernels (csrc/costdc_kernels.hip) per element, through the stand-alone hooks (include/ptta.h ptta_cd_sparse_*,
ptta_op_cd_*): every kernel against the plain references of oracle/costdc_arith.py on the cases of tests/costdc_cases.py.

Selections and exactly rounded single operations are compared with array_equal; arithmetic against the float64 reference within
TOL[quantity] x the element's magnitude (tests/costdc_cases.py: 4 x the CPU emulation's own error, never a GPU figure), every element,
none excluded.  Each comparison prints its largest ratio; profiles/costdc_elementwise.txt keeps them."""
import numpy as np
import pytest
import torch

from oracle import costdc_arith as A
from tests import costdc_cases as G
from tests.util import assert_elementwise

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, F32)).cuda()


def host(t):
    return t.cpu().numpy()


def as4(a):
    a = np.asarray(a)
    return a.reshape((1,) * (4 - a.ndim) + a.shape) if a.ndim <= 4 else a.reshape((-1,) + a.shape[-3:])


def check(name, q, got, ref, mag, tol=None):
    tol = G.TOL[q] if tol is None else tol
    got, ref, mag = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(mag, F64)
    print('costdc %s %s: largest |error| / magnitude %.3e (TOL %.3e)' % (q, name, G.ratio(got, ref, mag), tol))
    assert_elementwise(as4(got), as4(ref), as4(tol * mag), '%s %s' % (q, name))


def sparse_set(sparse, z):
    from proxytta.engine import CdSparseSet
    q = CdSparseSet(*sparse.shape)
    q.build(dev(sparse), z)
    return q


def read_levels(q):
    cnt = q.counts()
    out, feat = [], None
    for l in range(3):
        coords, vol, f = q.read(l)
        out.append((cnt[l], coords.astype(np.int64), vol.astype(np.int64)))
        feat = f if l == 0 else feat
    return out, feat


# ---- voxel levels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', G.LEVEL_CASES, ids=lambda c: c['name'])
def test_voxel_levels(c):
    sp = G.make_levels(c)
    q = sparse_set(sp, c['z'])
    for rebuild in range(2):                           # the second build runs over the first one's volumes
        if rebuild:
            q.build(dev(sp), c['z'])
        levels, feat = read_levels(q)
        A.check_levels(levels, sp, c['z'])
        _, f, mag = A.levels_ref(sp, c['z'])
        check(c['name'], 'feat', feat, f, mag)
    q.close()


def test_sparse_set_refuses_sizes_it_would_index_out_of_bounds():
    from proxytta.engine import CdSparseSet
    for n, h, w in ((1, 6, 8), (1, 8, 6), (1, 9, 8), (0, 8, 8), (1, 0, 8), (1, 2, 2)):
        with pytest.raises(RuntimeError, match=r'\(-22\)'):
            CdSparseSet(n, h, w)


# ---- sparse convolution ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def conv_sets():
    out = {}
    for big in (False, True):
        sparse, coords, shape = G.conv_geometry(big)
        q = sparse_set(sparse, (G.CONV_BIG if big else G.CONV_SET)['z'])
        assert q.counts() == [len(c) for c in coords]
        for l in range(3):
            assert np.array_equal(q.read(l)[0], coords[l])
        out[big] = (q, coords, shape)
    yield out
    for q, _, _ in out.values():
        q.close()


CONV_PARAMS = [(f, False) for f in G.CONV_FORMS] + [(G.CONV_FORMS[0], True)]


@pytest.mark.parametrize('form,big', CONV_PARAMS, ids=lambda v: str(v))
def test_sparse_conv_forward_and_backward(form, big, conv_sets):
    q, coords, shape = conv_sets[big]
    k, ci, co, lin, lout = form
    cin, cout = coords[lin], coords[lout]
    pairs = A.conv_pairs(cin, cout, shape, lin, lout, k)
    name = '%s%s' % (form, ' big' if big else '')
    x, wk, _ = G.make_conv(form, len(cin), len(cout))
    y = torch.full((len(cout), co), float('nan'), device='cuda')
    q.conv(dev(x), dev(wk), y, lin, lout, k)
    ref, mag = A.sparse_conv_ref(x, wk, pairs, len(cout))
    check(name, 'conv', host(y), ref, mag)
    gy, wk, prev = G.make_conv(form, len(cin), len(cout), True)
    for acc in (0, 1):
        gx = dev(prev) if acc else torch.full((len(cin), ci), float('nan'), device='cuda')
        q.conv(dev(gy), dev(wk), gx, lin, lout, k, backward=True, acc=bool(acc))
        ref, mag = A.sparse_conv_bwd_ref(gy, wk, pairs, len(cin), prev if acc else None)
        check('%s acc %d' % (name, acc), 'conv_bwd', host(gx), ref, mag)


def test_sparse_conv_refuses_more_than_64_threads_of_channels(conv_sets):
    q, coords, _ = conv_sets[False]
    x, w, y = torch.zeros(len(coords[0]), 8, device='cuda'), torch.zeros(27, 8, 80, device='cuda'), torch.zeros(len(coords[0]), 80, device='cuda')
    with pytest.raises(RuntimeError, match=r'\(-22\)'):
        q.conv(x, w, y, 0, 0, 3)
    with pytest.raises(RuntimeError, match=r'\(-22\)'):
        q.conv(x, torch.zeros(27, 80, 8, device='cuda'), y, 0, 0, 3, backward=True)
    with pytest.raises(RuntimeError, match=r'\(-22\)'):
        q.conv(x, torch.zeros(27, 8, 8, device='cuda'), x.clone(), 2, 0, 3)


# ---- sparse BatchNorm ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', G.SBN_CASES, ids=lambda c: c['name'])
def test_sparse_batchnorm_forward_and_backward(c):
    d = G.make_sbn(c)
    sparse, z = G.sbn_sparse(c)
    q = sparse_set(sparse, z)
    assert q.counts()[0] == c['cnt']
    cnt, C = c['cnt'], c['c']
    fw, fmag = G.sbn_reference_fwd(c, d)
    pad = max(cnt, 1)                                   # (a zero-voxel tensor still needs a pointer)

    def buf(a=None):
        t = torch.full((pad, C), float('nan'), device='cuda')
        if a is not None and cnt:
            t[:cnt] = dev(a)
        return t
    f, res, out, st = buf(d['f']), (buf(d['res']) if c['res'] else None), buf(), torch.full((4, C), float('nan'), device='cuda')
    gamma, beta = dev(d['gamma']), dev(d['beta'])
    rm = rv = nbt = None
    if d['track'] is not None:
        rm, rv, nbt = dev(d['track']['rm']), dev(d['track']['rv']), torch.tensor([d['track']['nbt']], dtype=torch.int64, device='cuda')
    mode = 'eval' if c['mode'] == 'eval' else 'train'
    q.bn(mode, 0, f, gamma, st, beta=beta, res=res, out=out, rm=rm, rv=rv, nbt=nbt, repeats=2 if c['mode'] == 'tracked' else 1, relu=c['relu'], world=c['world'])
    got = dict(y=host(out)[:cnt].reshape(1, 1, cnt, C), st=host(st))
    if c['mode'] == 'tracked':
        got.update(rm=host(rm), rv=host(rv))
        assert int(nbt.item()) == fw['nbt']
    elif d['track'] is not None:                        # eval leaves the running statistics alone
        assert np.array_equal(host(rm), d['track']['rm']) and np.array_equal(host(rv), d['track']['rv']) and int(nbt.item()) == d['track']['nbt']
    check(c['name'], 'sbn_y', got['y'], fw['y'], fmag['y'])
    check(c['name'], 'sbn_st', got['st'], fw['st'], fmag['st'])
    if c['mode'] == 'tracked':
        check(c['name'], 'sbn_rm', got['rm'], fw['rm'], fmag['rm'])
        check(c['name'], 'sbn_rv', got['rv'], fw['rv'], fmag['rv'])
    if c['mode'] == 'eval':
        q.close()
        return
    bw, bmag = G.sbn_reference_bwd(c, d, fw, fmag)
    g, gx = buf(d['g']), buf()
    gres = None if c['gres'] == 'none' else (buf(d['gres_prev']) if c['gres'] == 'acc' else buf())
    dgamma, dbeta = torch.full((C,), float('nan'), device='cuda'), torch.full((C,), float('nan'), device='cuda')
    q.bn('backward', 0, f, gamma, st, y=out, g=g, gx=gx, gres=gres, acc_res=c['gres'] == 'acc', dgamma=dgamma, dbeta=dbeta, relu=c['relu'], world=c['world'])
    check(c['name'], 'sbn_gx', host(gx)[:cnt].reshape(1, 1, cnt, C), bw['gx'], bmag['gx'])
    check(c['name'], 'sbn_dgamma', host(dgamma), bw['dgamma'], bmag['dgamma'])
    check(c['name'], 'sbn_dbeta', host(dbeta), bw['dbeta'], bmag['dbeta'])
    if gres is not None:
        gr = host(gres)[:cnt].reshape(1, 1, cnt, C)
        if c['gres'] == 'acc':
            check(c['name'], 'gres accumulated', gr, bw['gres'], bmag['gres'], G.TOL_ACC)
        else:
            assert np.array_equal(gr, bw['gres'].astype(F32))                      # a masked copy
    q.close()


def test_sparse_batchnorm_refuses_more_than_64_channels():
    sparse, z = G.sbn_sparse(G.SBN_BY_NAME['cnt2_c48'])
    q = sparse_set(sparse, z)
    t = torch.zeros(4, 128, device='cuda')
    with pytest.raises(RuntimeError, match=r'\(-22\)'):
        q.bn('train', 0, t, torch.ones(128, device='cuda'), torch.zeros(4, 128, device='cuda'), beta=torch.zeros(128, device='cuda'), out=t.clone())
    q.close()


# ---- densify -----------------------------------------------------------------------------------------------------------------------
def test_densify_and_its_gradient(conv_sets):
    q, coords, (N, H, W) = conv_sets[False]
    c2 = coords[2]
    rng = G.rng_of('densify')
    f = rng.standard_normal((len(c2), 16)).astype(F32)
    dense = torch.full((N, 16, H // 4, W // 4, 16), float('nan'), device='cuda')
    q.densify(dev(f), dense, 16)
    assert np.array_equal(host(dense), A.densify_ref(f, c2, N, H, W))
    gvol = rng.standard_normal((N, 16, H // 4, W // 4, 32)).astype(F32)
    g = torch.full((len(c2), 16), float('nan'), device='cuda')
    q.densify(dev(gvol), g, 16, backward=True, ldv=32, c0=16)
    assert np.array_equal(host(g), A.densify_bwd_ref(gvol, c2, 16, 16))
    with pytest.raises(RuntimeError, match=r'\(-22\)'):
        q.densify(dev(gvol), g, 16, backward=True, ldv=24, c0=16)


# ---- dense kernels ---------------------------------------------------------------------------------------------------------------
def dense(op, a, shape, dims, b=None, out_init=None, fpar=(), shape2=None):
    from proxytta.engine import op_cd_dense
    out = dev(out_init) if out_init is not None else torch.full(shape, float('nan'), device='cuda')
    out2 = torch.full(shape2, float('nan'), device='cuda') if shape2 else None
    op_cd_dense(op, dev(a), out, dims, b=dev(b), out2=out2, fpar=fpar)
    return host(out) if out2 is None else (host(out), host(out2))


NORM_F = (G.NORM[0],) + G.NORM[1] + G.NORM[2]


@pytest.mark.parametrize('c', G.PAD_CASES, ids=lambda c: c['name'])
def test_pad_family(c):
    image, sparse, net, g, Hp, Wp = G.make_pad(c)
    n, h, w, pt, pr = c['n'], c['h'], c['w'], c['pt'], c['pr']
    for src, C in ((image, 3), (sparse[:, None], 1)):
        got = dense('pad_dual', src, (2 * n, C, Hp, Wp), (n, C, h, w, Hp, Wp, pt, pr, 0))
        assert np.array_equal(got, A.pad_dual_ref(src, Hp, Wp, pt, pr)[0])
    got = dense('pad_dual', image, (2 * n, 3, Hp, Wp), (n, 3, h, w, Hp, Wp, pt, pr, 1), fpar=NORM_F)
    ref, _, mag = A.pad_dual_ref(image, Hp, Wp, pt, pr, G.NORM)
    check(c['name'] + ' pad_dual', 'norm', got, ref, mag)
    outside = A.pad_dual_ref(np.ones_like(image), Hp, Wp, pt, pr)[0] == 0
    assert outside.any() and (got[outside] == 0).all() and (got[~outside] != 0).all()          # padded pixels exactly zero
    got = dense('crop_avg', net, (n, h, w), (n, h, w, Hp, Wp, pt, pr))
    assert np.array_equal(got, A.crop_avg_ref(net, n, h, w, pt, pr))
    got = dense('scatter_dual_grad', g, (2 * n, Hp, Wp), (n, h, w, Hp, Wp, pt, pr))
    assert np.array_equal(got, A.scatter_dual_grad_ref(g, Hp, Wp, pt, pr))
    from proxytta.engine import op_cd_dense
    with pytest.raises(RuntimeError, match=r'\(-22\)'):                                    # a crop that would read past the padded frame
        op_cd_dense('crop_avg', dev(net), torch.zeros(n, h, w, device='cuda'), (n, h, w, Hp, Wp, pt + 1, pr))
    # staging and clamp on the same frame
    for passes, C, norm in ((1, 4, 0), (2, 16, 0), (2, 4, 1), (1, 16, 1)):
        got = dense('stage', image, (passes * n, h, w, C), (n, passes, h, w, C, norm), b=sparse, fpar=NORM_F)
        ref, _, mag = A.stage_ref(image, sparse, passes, C, G.NORM if norm else None)
        if norm:
            check('%s stage passes %d C %d' % (c['name'], passes, C), 'norm', got, ref, mag)
            assert np.array_equal(got[..., 3:], ref[..., 3:].astype(F32)) and (got[n:, ..., :3] == 0).all()
        else:
            assert np.array_equal(got, ref.astype(F32))
    sp = sparse.copy()
    sp.flat[:4] = (-1.0, 5.0, 5.000001, 1e9)
    for maxd in (5.0, -1.0):
        assert np.array_equal(dense('clamp', sp, sp.shape, (sp.size,), fpar=(maxd,)), A.clamp_ref(sp, maxd))


@pytest.mark.parametrize('c', G.FUSION_CASES, ids=lambda c: c['name'])
def test_fusion(c):
    feat2d, feat3d, gvol = G.make_fusion(c)
    N, P, h, w = c['n'], c['passes'], c['h'], c['w']
    vol, mask = dense('fusion_fwd', feat2d, (P * N, 16, h, w, 32), (N, P, h, w), b=feat3d, shape2=(N, 16, h, w))
    rv, rm = A.fusion_fwd_ref(feat2d, feat3d, P)
    assert np.array_equal(mask, rm) and np.array_equal(vol[..., 16:], rv[..., 16:]) and np.array_equal(vol, rv)
    got = dense('fusion_bwd', gvol, (N, h, w, 16), (N, h, w), b=rm)
    ref, _, mag = A.fusion_bwd_ref(gvol, rm)
    check(c['name'], 'fusion_bwd', got, ref, mag)


@pytest.mark.parametrize('c', G.POOL_CASES, ids=lambda c: c['name'])
def test_pool(c):
    x, gy, prev = G.make_pool(c)
    I, H, W, C = x.shape
    assert np.array_equal(dense('pool_fwd', x, (I // 2, H // 2, W // 2, C), (I // 2, H, W, C)), A.pool_fwd_ref(x))
    got = dense('pool_bwd', x, x.shape, (I, H, W, C, c['acc']), b=gy, out_init=prev if c['acc'] else None)
    assert np.array_equal(got, A.pool_bwd_ref(x, gy, prev if c['acc'] else None))
    from proxytta.engine import op_cd_dense
    with pytest.raises(RuntimeError, match=r'\(-22\)'):                                    # an odd plane count has no partner plane
        op_cd_dense('pool_bwd', dev(x), torch.zeros(x.shape, device='cuda'), (I - 1, H, W, C, 0), b=dev(gy))
    with pytest.raises(RuntimeError, match=r'\(-22\)'):                                    # float4 loads
        op_cd_dense('pool_fwd', dev(x), torch.zeros(I // 2, H // 2, W // 2, C, device='cuda'), (I // 2, H, W, C - 2))


@pytest.mark.parametrize('c', G.UP_CASES, ids=lambda c: c['name'])
def test_up(c):
    x, gy, prev = G.make_up(c)
    fr, ch = c['frames'], c['c']
    got = dense('up_fwd', x, (fr,) + c['o'] + (ch,), (fr,) + c['i'] + c['o'] + (ch,))
    assert np.array_equal(got, A.up_fwd_ref(x, *c['o']))
    got = dense('up_bwd', gy, x.shape, (fr,) + c['i'] + c['o'] + (ch, c['acc']), out_init=prev if c['acc'] else None)
    assert np.array_equal(got.astype(F64), A.up_bwd_ref(gy, *c['i'], prev=prev if c['acc'] else None))


@pytest.mark.parametrize('c', G.REGRESS_CASES, ids=lambda c: c['name'])
def test_regress(c):
    cost, gpred = G.make_regress(c)
    n, h, w = c['n'], c['h'], c['w']
    got = dense('regress_fwd', cost, (n, 4 * h, 4 * w), (n, h, w), fpar=(c['z'],))
    ref, _, mag = A.regress_fwd_ref(cost, c['z'])
    check(c['name'], 'regress', got, ref, mag)
    got = dense('regress_bwd', cost, cost.shape, (n, h, w), b=gpred, fpar=(c['z'],))
    ref, _, mag = A.regress_bwd_ref(cost, gpred, c['z'])
    check(c['name'], 'regress_bwd', got, ref, mag)


@pytest.mark.parametrize('c', G.ROWS_CASES, ids=lambda c: c['name'])
def test_rows(c):
    rng = G.rng_of('rows/' + c['name'])
    n, d, h, w, ch = c['n'], c['d'], c['h'], c['w'], c['c']
    feat = rng.standard_normal((n, d, h, w, ch)).astype(F32)
    rows = dense('rows_fwd', feat, (n * h * w, ch * d), (n, d, h, w, ch))
    assert np.array_equal(rows, A.rows_fwd_ref(feat))
    grows = rng.integers(-1000, 1000, rows.shape).astype(F32)
    prev = rng.integers(-1000, 1000, feat.shape).astype(F32)
    got = dense('rows_bwd', grows, feat.shape, (n, d, h, w, ch, c['acc']), out_init=prev if c['acc'] else None)
    assert np.array_equal(got, A.rows_bwd_ref(grows, n, d, h, w, ch, prev if c['acc'] else None))
