"""The generic engine's BatchNorm (csrc/gbn.hip) on its own, through ptta_op_gbn, compared PER ELEMENT with a float64 reference on the
CPU (oracle/gbn_arith.py): every case of tests/gbn_cases.py forward, then backward on the forward's own statistics.  No element is left
out of a comparison (tests/test_gbn_elementwise_cpu.py asserts that no case has an element on a mask tie).

bound = TOL[quantity] x magnitude, TOL = 4 x the CPU emulation's largest error ratio (never a GPU figure; profiles/gbn_elementwise.txt).
The magnitudes grow with the channel's cancellation factor kappa = (mean^2 + var + eps) / (var + eps): what var = E[x^2] - mean^2 from
fp32 partial sums loses."""
import numpy as np
import pytest
import torch

from oracle import gbn_arith as A
from tests import gbn_cases as G
from tests.util import assert_elementwise

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
_cache = {}


def _expected(c):
    if c['name'] not in _cache:
        _cache.clear()                      # one case at a time
        d = G.make(c)
        _cache[c['name']] = (d, G.reference(c, d))
    return _cache[c['name']]


def _put(c, a, which, fill=None):
    """Device tensor of a: dense, or (views) a channel slice of a wider sentinel-filled buffer with the tensor's own pads
    (G.VIEW_PADS[which]: another row stride for each of the six).  Returns (view, wide or None, pre)."""
    pre, post = G.VIEW_PADS[which]
    t = torch.from_numpy(np.ascontiguousarray(a)) if a is not None else None
    if not c['views']:
        return (t.cuda() if t is not None else torch.full(fill, SENTINEL).cuda()), None, 0
    shape = tuple(t.shape) if t is not None else fill
    wide = torch.full(shape[:3] + (pre + shape[3] + post,), SENTINEL)
    if t is not None:
        wide[..., pre:pre + shape[3]] = t
    wide = wide.cuda()
    return wide[..., pre:pre + shape[3]], wide, pre


def _untouched(wide, pre, ch, what):
    if wide is not None:
        w = wide.cpu()
        assert bool((w[..., :pre] == SENTINEL).all()) and bool((w[..., pre + ch:] == SENTINEL).all()), 'wrote outside the view of ' + what


def _t4(a):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)
    return a.reshape((1,) * (4 - a.ndim) + a.shape)


def _check(name, what, got, ref, mag, tol, report):
    got, ref, mag = _t4(got), _t4(ref), _t4(mag)
    report[what] = float((np.abs(got.astype(np.float64) - ref) / np.maximum(mag, 1e-300)).max())
    print('%s %s: largest |error| / magnitude %.3e (TOL %.3e)' % (name, what, report[what], tol))
    assert_elementwise(got, ref, tol * mag, '%s %s' % (name, what))


def _forward(c, d, world=None):
    """One training forward on the GPU: the device tensors and outputs."""
    from proxytta.engine import op_gbn
    ch, npass = c['c'], c['npass']
    shape = (c['b'], c['h'], c['w'], ch)
    o = dict()
    o['x'], o['xw'], o['xp'] = _put(c, d['x'], 'x')
    o['res'], o['resw'], o['resp'] = _put(c, d['res'], 'res') if c['res'] else (None, None, 0)
    o['y'], o['yw'], o['yp'] = _put(c, None, 'y', fill=shape)
    o['gamma'], o['beta'] = torch.from_numpy(d['gamma']).cuda(), torch.from_numpy(d['beta']).cuda()
    o['st'] = torch.full((4, npass, ch), SENTINEL).cuda()
    kw = {}
    if c['track']:
        t = d['track']
        o['rm'], o['rv'] = torch.from_numpy(t['rm'].copy()).cuda(), torch.from_numpy(t['rv'].copy()).cuda()
        o['nbt'] = torch.tensor([t['nbt']], dtype=torch.int64).cuda()
        o['st_eval'] = torch.full((4, ch), SENTINEL).cuda()
        kw = dict(rm=o['rm'], rv=o['rv'], nbt=o['nbt'], st_eval=o['st_eval'], momentum=t['momentum'], repeats=t['repeats'])
    if d['parts'] is not None:
        kw['part_in'] = torch.from_numpy(d['parts']).cuda()
    op_gbn('train', o['x'], o['y'], o['st'], o['gamma'], o['beta'], res=o['res'], npass=npass, act=c['act'], act_first=c['act_first'],
           res_relu=c['res_relu'], eps=G.EPS, world=c['world'] if world is None else world, **kw)
    return o


def _backward(c, d, o, world=None):
    from proxytta.engine import op_gbn
    ch = c['c']
    shape = (c['b'] // c['npass'], c['h'], c['w'], ch)
    q = dict()
    q['g'], q['gw'], q['gp'] = _put(c, d['g'], 'g')
    q['gx'], q['gxw'], q['gxp'] = _put(c, d['gx_prev'], 'gx', fill=shape)
    q['gres'], q['gresw'], q['gresp'] = _put(c, d['gres_prev'], 'gres', fill=shape) if c['res'] else (None, None, 0)
    if c['views'] and c['res']:          # the six tensors of a residual block: six different row strides
        lds = [t.stride(2) for t in (o['x'], o['res'], o['y'], q['g'], q['gx'], q['gres'])]
        assert len(set(lds)) == 6 and all(ld % 4 == 0 for ld in lds), lds
    q['dgamma'] = None if c['frozen'] else torch.full((ch,), SENTINEL).cuda()
    q['dbeta'] = None if c['frozen'] else torch.full((ch,), SENTINEL).cuda()
    op_gbn('backward', o['x'], o['y'], o['st'], o['gamma'], g=q['g'], gx=q['gx'], gres=q['gres'], npass=c['npass'], act=c['act'],
           act_first=c['act_first'], res_relu=c['res_relu'], acc_gx=c['acc_gx'], acc_gres=c['acc_gres'], dgamma=q['dgamma'], dbeta=q['dbeta'],
           world=c['world'] if world is None else world)
    return q


@pytest.mark.parametrize('name', [c['name'] for c in G.CASES])
def test_gbn_per_element(name):
    c = G.BY_NAME[name]
    d, (fw, fmag, bw, bmag) = _expected(c)
    ch, npass = c['c'], c['npass']
    rep = {}
    # ---- forward ----
    o = _forward(c, d)
    st = o['st'].cpu().numpy()
    _check(name, 'y', o['y'], fw['y'], fmag['y'], G.TOL['y'], rep)
    _check(name, 'mean', st[0], fw['mean'], fmag['mean'], G.TOL['mean'], rep)
    _check(name, 'inv', st[1], fw['inv'], fmag['inv'], G.TOL['inv'], rep)
    _untouched(o['yw'], o['yp'], ch, 'y')
    for k in ('x', 'res'):
        if o.get(k + 'w') is not None:      # the inputs are bitwise what they were
            src = d[k]
            assert np.array_equal(o[k].cpu().numpy(), src) and (_untouched(o[k + 'w'], o[k + 'p'], ch, k) is None)
    o2 = _forward(c, d)
    assert torch.equal(o['y'], o2['y']) and torch.equal(o['st'], o2['st']), 'forward not bitwise reproducible'
    if c['track']:
        t = d['track']
        _check(name, 'rm', o['rm'], fw['rm'], fmag['rm'], G.TOL['rm'], rep)
        _check(name, 'rv', o['rv'], fw['rv'], fmag['rv'], G.TOL['rv'], rep)
        assert int(o['nbt'].item()) == t['nbt'] + npass * t['repeats']
        assert torch.equal(o['rm'], o2['rm']) and torch.equal(o['rv'], o2['rv']) and torch.equal(o['st_eval'], o2['st_eval'])
        # an eval forward from the updated buffers: its affine is the one the training forward left behind, to the two roundings
        # (inv, gamma * inv; beta - mean * scale) the two kernels may order differently
        from proxytta.engine import op_gbn
        ye, yew, yep = _put(c, None, 'y', fill=(c['b'], c['h'], c['w'], ch))
        ste = torch.full((4, ch), SENTINEL).cuda()
        op_gbn('eval', o['x'], ye, ste, o['gamma'], o['beta'], res=o['res'], act=c['act'], act_first=c['act_first'], res_relu=c['res_relu'],
               eps=G.EPS, rm=o['rm'], rv=o['rv'])
        se, sv = ste.cpu().double().numpy(), o['st_eval'].cpu().double().numpy()
        assert np.array_equal(se[0], sv[0]) and np.array_equal(se[0], o['rm'].cpu().double().numpy())
        assert bool((np.abs(se[1:3] - sv[1:3]) <= 2.0 ** -22 * np.abs(se[1:3])).all())
        assert bool((np.abs(se[3] - sv[3]) <= 2.0 ** -22 * (np.abs(d['beta']) + np.abs(se[0] * se[2]))).all())
        ev = fw['ev']
        _check(name, 'eval y', ye, A.eval_forward_ref(d['x'], ev, c['act'], d['res'], c['act_first'], c['res_relu']),
               A.eval_mags(d['x'], d['gamma'], d['beta'], ev, fmag, G.EPS, d['res']), max(G.TOL['y'], G.TOL['rm'], G.TOL['rv']), rep)
        _untouched(yew, yep, ch, 'y (eval)')
    # ---- backward, on the forward's own x, y and statistics ----
    q = _backward(c, d, o)
    _check(name, 'gx', q['gx'], bw['gx'], bmag['gx'], G.TOL['gx'], rep)
    _untouched(q['gxw'], q['gxp'], ch, 'gx')
    if not c['frozen']:
        _check(name, 'dgamma', q['dgamma'], bw['dgamma'], bmag['dgamma'], G.TOL['dgamma'], rep)
        _check(name, 'dbeta', q['dbeta'], bw['dbeta'], bmag['dbeta'], G.TOL['dbeta'], rep)
    if c['res']:
        gres = q['gres'].cpu().numpy()
        if c['acc_gres']:
            _check(name, 'gres', gres, bw['gres'], bmag['gres'], G.TOL_GRES_ACC, rep)
        else:                               # a pure select: g where the float64 outer mask is set, exactly
            assert np.array_equal(gres, bw['gouter'].astype(np.float32)) and np.array_equal(bw['gouter'], np.where(bw['gouter'] != 0, d['g'], 0.0))
        _untouched(q['gresw'], q['gresp'], ch, 'gres')
    q2 = _backward(c, d, o)
    assert torch.equal(q['gx'], q2['gx']) and (c['frozen'] or (torch.equal(q['dgamma'], q2['dgamma']) and torch.equal(q['dbeta'], q2['dbeta'])))
    assert not c['res'] or torch.equal(q['gres'], q2['gres']), 'backward not bitwise reproducible'
    assert torch.equal(o['y'], o2['y']) and torch.equal(o['st'], o2['st'])          # the backward wrote nothing it only reads
    # ---- caller-made partials against the plain statistics pass on the same pixels ----
    if c['nblocks']:
        op = _forward(dict(c, nblocks=0), dict(d, parts=None))
        sp = op['st'].cpu().numpy()
        for k, qn in ((0, 'mean'), (1, 'inv')):
            assert bool((np.abs(st[k].astype(np.float64) - sp[k]) <= 2 * G.TOL[qn] * fmag[qn]).all()), (name, qn)
    # ---- SyncBatchNorm against the one-rank run of the same data ----
    if c['world'] > 1:
        o1 = _forward(c, d, world=1)
        s1 = o1['st'].cpu().numpy()
        for k, qn in ((0, 'mean'), (1, 'inv')):
            err = np.abs(st[k].astype(np.float64) - s1[k]) / fmag[qn]
            print('%s world %d vs 1 %s: largest relative difference %.3e' % (name, c['world'], qn, float(err.max())))
            assert bool((err <= G.TOL_WORLD_STAT).all()), (name, qn, float(err.max()))
        q1 = _backward(c, d, o1, world=1)
        assert_elementwise(o['y'], o1['y'].cpu().double(), G.TOL['y'] * fmag['y'], name + ' y, world 2 vs 1')
        assert_elementwise(q['gx'], q1['gx'].cpu().double(), G.TOL['gx'] * bmag['gx'], name + ' gx, world 2 vs 1')
        assert_elementwise(_t4(q['dgamma']), _t4(q1['dgamma']).astype(np.float64), G.TOL['dgamma'] * _t4(bmag['dgamma']), name + ' dgamma, world 2 vs 1')
    print('%s: largest |error| / bound %.3f' % (name, max(rep[k] / (G.TOL.get(k.split()[-1], G.TOL_GRES_ACC) if k != 'eval y' else max(G.TOL['y'], G.TOL['rm'], G.TOL['rv'])) for k in rep)))
    print('GBN_RATIOS %s %s' % (name, ' '.join('%s=%.3e' % (k.replace(' ', '_'), v) for k, v in rep.items())))


def test_gbn_rejects_what_the_kernels_do_not_take():
    """-22 before any launch: nothing here reaches a kernel.  The switch combinations are refused by the launchers themselves
    (ptta_gbn_switches_ok of csrc/gbn.hip), which the hook calls as the engine does."""
    from proxytta.engine import op_gbn
    z = lambda *s: torch.zeros(*s).cuda()
    wide = z(2, 3, 5, 24)
    gamma, beta, st = torch.ones(8).cuda(), z(8), z(4, 2, 8)

    def train(x, y, **kw):
        op_gbn('train', x, y, kw.pop('st', st), kw.pop('gamma', gamma), kw.pop('beta', beta), **kw)

    def bwd(**kw):
        op_gbn('backward', wide[..., :8], wide[..., 8:16], st, gamma, g=z(2, 3, 5, 8), gx=z(2, 3, 5, 8), **kw)
    train(wide[..., :8], wide[..., 8:16])                                              # what they do take
    bad = [
        lambda: train(z(2, 3, 5, 6), z(2, 3, 5, 6), gamma=torch.ones(6).cuda(), beta=z(6), st=z(4, 1, 6)),     # C = 6
        lambda: train(z(2, 3, 5, 10)[..., :8], wide[..., 8:16]),                       # ld = 10
        lambda: train(wide[..., 2:10], wide[..., 12:20]),                              # 8-byte aligned x
        lambda: train(wide[..., :8], wide[..., 10:18]),                                # ... y
        lambda: train(wide[..., :8], wide[..., 8:16], res=z(2, 3, 5, 9)[..., 1:9]),     # ... res
        lambda: train(wide[..., :8], wide[..., 8:20]),                                 # y with 12 channels
        lambda: train(wide[..., :8], wide[..., 8:16], res=z(2, 3, 5, 4)),              # res with 4
        lambda: train(z(3, 3, 5, 8), z(3, 3, 5, 8), npass=2),                          # 3 images in 2 passes
        lambda: train(wide[..., :8], wide[..., 8:16], gamma=torch.ones(9).cuda()[1:]),  # a misaligned table
        # with a residual and no final ReLU the forward never applies act (act_first = 0) / the backward masks from act(v) + res
        lambda: train(wide[..., :8], wide[..., 8:16], res=z(2, 3, 5, 8), res_relu=False, act='relu'),
        lambda: train(wide[..., :8], wide[..., 8:16], res=z(2, 3, 5, 8), res_relu=False, act='lrelu', act_first=True),
        lambda: train(wide[..., :8], wide[..., 8:16], res=z(2, 3, 5, 8), act='lrelu', act_first=True),      # the inner mask is a ReLU's
        lambda: bwd(gres=z(2, 3, 5, 8), res_relu=False, act='relu'),
        lambda: bwd(gres=z(2, 3, 5, 8), res_relu=False, act='elu', act_first=True),
        lambda: bwd(gres=z(2, 3, 5, 8), act='none', act_first=True),
        lambda: bwd(gres=z(2, 3, 5, 12)[..., 2:10]),
        lambda: op_gbn('eval', wide[..., :8], wide[..., 8:16], z(4, 8), gamma, beta),   # no running statistics
        lambda: op_gbn('eval', wide[..., :8], wide[..., 8:16], z(4, 8), gamma, beta, rm=z(8), rv=torch.ones(8).cuda(), res=z(2, 3, 5, 8),
                       res_relu=False, act='relu'),                                    # the apply launcher's refusal, ahead of the eval affine
    ]
    for k, f in enumerate(bad):
        with pytest.raises(RuntimeError, match='-22'):
            f()
            pytest.fail('case %d accepted' % k)
    bwd(gres=z(2, 3, 5, 8), res_relu=False)                                            # Res_Conv
