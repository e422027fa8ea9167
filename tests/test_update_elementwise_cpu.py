"""CPU-only side of the per-element tests of the update half of a step (tests/test_gpu_update_elementwise.py): the hooks' declarations against
the binding, the references of oracle/update_arith.py against torch in float64 (torch.optim.Adam over several steps, autograd through
BatchNorm + ReLU -> Linear -> BatchNorm1d, conv2d's weight gradient), the fp32 emulations against those references, the tolerances, the
cases the issue lists, and value-only slips planted on the CPU that the bounds must refuse.

A case's tolerance is 4 x the CPU emulation's ratio on that same case (tests/update_ratios.py, profiles/update_elementwise.txt) -- never a
GPU figure."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import update_arith as A
from proxytta import _lib
from tests import update_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
HOOKS = ('ptta_op_wgrad32', 'ptta_op_gwgrad_view', 'ptta_op_adam', 'ptta_op_adam_multi', 'ptta_op_ema_multi', 'ptta_op_linear_wgrad',
         'ptta_op_glinear_wgrad')


def test_hooks_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    sig = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    for name in HOOKS:
        m = re.search(r'^int %s\((.*?)\);' % name, header, re.S | re.M)
        assert m, name
        res, args = sig[name]
        assert res is ctypes.c_int, name
        decl = [a.strip() for a in m.group(1).replace('\n', ' ').split(',')]
        assert len(args) == len(decl), name
        for a, w in zip(args, decl):
            if '*' in w or w.startswith('ptta_stream'):
                assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), (name, w)
            else:
                assert a is {'int': ctypes.c_int, 'long long': ctypes.c_longlong}[re.sub(r'\s+\w+$', '', w)], (name, w)
    for struct, cls in (('ptta_gwgrad_view_args', _lib.GwgradViewArgs), ('ptta_linear_wgrad_args', _lib.LinearWgradArgs)):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct), header, re.S).group(1)
        fields = []
        for decl in body.split(';'):
            decl = decl.strip()
            if decl:
                kind = 'ptr' if '*' in decl else re.match(r'(long long|int)', decl).group(1)
                rest = re.sub(r'^(const\s+)?(long long|int|float|unsigned|void)\s*\*?', '', decl)
                fields += [(n.strip(' *'), kind) for n in rest.split(',')]
        want = {'ptr': ctypes.c_void_p, 'int': ctypes.c_int, 'long long': ctypes.c_longlong}
        assert [(n, want[k]) for n, k in fields] == list(cls._fields_), struct         # the same fields, types and order
    assert re.search(r'#define PTTA_ABI_VERSION 2\b', header) and _lib.PTTA_ABI_VERSION == 2          # a new export changes no ABI version
    src = open(os.path.join(ROOT, 'tta-depth-completion_amd', 'csrc', 'Makefile')).read()
    assert 'ptta_ops_update.hip' in src


# ---- the references are torch in float64 ----------------------------------------------------------------------------------------------------
def _torch_adam(params, grads_per_step, lr, b1, b2, eps, wd):
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in params]
    opt = torch.optim.Adam(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for grads in grads_per_step:
        for p, g in zip(ps, grads):
            p.grad = None if g is None else torch.from_numpy(g.copy())
        opt.step()
    return ps, opt


@pytest.mark.parametrize('wd', (0.0, 1e-4, 0.3))
def test_adam_reference_is_torch_optim_adam(wd):
    rng = G.rng_of('cpu/adam/%g' % wd)
    hy = A.hyper32(1e-3, 0.9, 0.999, 1e-8, wd)
    lr, b1, b2, eps, wdf = (float(h) for h in hy)            # the fp32 values, widened: what the device holds
    n, steps = 300, 5
    p0 = [rng.standard_normal(n), rng.standard_normal(7)]
    grads = [[rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n), rng.standard_normal(7)] for _ in range(steps)]
    ps, _ = _torch_adam(p0, grads, lr, b1, b2, eps, wdf)
    for k in range(2):
        p, m, v = p0[k], np.zeros_like(p0[k]), np.zeros_like(p0[k])
        for t in range(steps):
            (p, m, v), _ = A.adam_ref(p, m, v, grads[t][k], hy, t + 1)
        assert np.allclose(p, ps[k].detach().numpy(), rtol=1e-12, atol=1e-13)
    # a tensor without a gradient is skipped, its step count with it
    ps, _ = _torch_adam(p0, [[g[0], None] for g in grads], lr, b1, b2, eps, wdf)
    assert np.array_equal(ps[1].detach().numpy(), p0[1])


@pytest.mark.parametrize('wd', (0.0, 1e-4))
def test_adam_reference_with_a_parameter_listed_twice(wd):
    """torch.optim.Adam updates a parameter once per occurrence in its list, each with its own step count: rep = 2, 3 of adam_ref"""
    rng = G.rng_of('cpu/adam_rep/%g' % wd)
    hy = A.hyper32(1e-3, 0.9, 0.999, 1e-8, wd)
    lr, b1, b2, eps, wdf = (float(h) for h in hy)
    for rep in (2, 3):
        p0, steps = rng.standard_normal(50), 4
        grads = [rng.standard_normal(50) for _ in range(steps)]
        q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            opt = torch.optim.Adam([{'params': [q] * rep}], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wdf, foreach=False)
        p, m, v = p0, np.zeros(50), np.zeros(50)
        for t in range(steps):
            q.grad = torch.from_numpy(grads[t].copy())
            opt.step()
            (p, m, v), _ = A.adam_ref(p, m, v, grads[t], hy, t + 1, rep)
        assert np.allclose(p, q.detach().numpy(), rtol=1e-12, atol=1e-13), rep
        assert int(opt.state[q]['step']) == steps * rep


def test_linear_reference_is_autograd_through_both_batchnorms():
    """A = relu(BatchNorm(X)) (its affine applied as scale / shift), H = Linear(A), Y = BatchNorm1d(H) in training mode, L = sum(Y Gout):
    dL/dW and dL/db against linear_wgrad_ref with G = Gout, Gh = H and the tables of bn_backward_tables"""
    rng = G.rng_of('cpu/linear')
    R, I, O = 70, 24, 40
    X, W, b = rng.standard_normal((R, I)), rng.standard_normal((O, I)) / 5.0, rng.standard_normal(O)
    xs, xsh = rng.uniform(0.5, 1.5, I), rng.uniform(-0.5, 0.5, I)
    gamma, beta, gout = rng.uniform(0.5, 1.5, O), rng.uniform(-0.5, 0.5, O), rng.standard_normal((R, O))
    t = lambda a: torch.from_numpy(np.asarray(a, F64))
    Wt, bt = t(W).requires_grad_(True), t(b).requires_grad_(True)
    a = torch.relu(t(X) * t(xs) + t(xsh))
    h = torch.nn.functional.linear(a, Wt, bt)
    y = torch.nn.functional.batch_norm(h, None, None, t(gamma), t(beta), training=True, eps=1e-5)
    (y * t(gout)).sum().backward()
    hn = h.detach().numpy()
    mean, inv = hn.mean(0), 1.0 / np.sqrt(hn.var(0) + 1e-5)
    xh = (hn - mean) * inv
    gt = dict(gscale=gamma * inv, gc1=gout.mean(0), gc2=(gout * xh).mean(0), gmean=mean, ginv=inv)            # float64 tables
    (dW, db), (mw, mb) = A.linear_wgrad_ref(gout, X, Gh=hn, gt=gt, xscale=xs, xshift=xsh)
    assert np.allclose(dW, Wt.grad.numpy(), rtol=0, atol=1e-12 * mw.max()) and np.allclose(db, bt.grad.numpy(), rtol=0, atol=1e-12 * mb.max())
    assert (mw >= np.abs(dW)).all() and (mb >= np.abs(db) * (1 - 1e-12)).all()
    # the fp32 tables of bn_backward_tables are those constants
    f = A.bn_backward_tables(gout, hn, gamma)
    assert all(np.allclose(f[k], gt[k], rtol=1e-6, atol=1e-8) for k in gt)
    # each prologue alone, and none
    (dW0, db0), _ = A.linear_wgrad_ref(gout, X)
    assert np.allclose(dW0, gout.T @ X, rtol=0, atol=1e-12) and np.allclose(db0, gout.sum(0), rtol=0, atol=1e-12)


def test_conv_reference_is_conv2d_autograd():
    rng = G.rng_of('cpu/conv')
    x, gy = rng.standard_normal((2, 5, 7, 6)), rng.standard_normal((2, 5, 7, 4))
    w = torch.zeros(4, 6, 3, 3, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(4, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), w, bias, padding=1)
    (y * torch.from_numpy(gy).permute(0, 3, 1, 2)).sum().backward()
    (gw, gb), (mw, mb) = A.conv_wgrad_ref(x, gy)
    assert np.allclose(gw, w.grad.numpy(), rtol=0, atol=1e-12) and np.allclose(gb, bias.grad.numpy(), rtol=0, atol=1e-12)
    assert (mw >= np.abs(gw) - 1e-12).all()
    # the emulations' tap order and padding are the reference's
    x32, g32 = x.astype(F32), gy.astype(F32)
    ew, eb = A.gwgrad_x3_emu(x32, g32)
    assert np.allclose(ew, gw, rtol=0, atol=1e-3 * mw.max()) and np.allclose(eb, gb, rtol=0, atol=1e-5 * mb.max())
    x32, g32 = rng.standard_normal((2, 5, 7, 32)).astype(F32), rng.standard_normal((2, 5, 7, 32)).astype(F32)
    (gw, gb), (mw, mb) = A.conv_wgrad_ref(x32, g32)
    ew, eb = A.wgrad32_emu(x32, g32)
    assert np.allclose(ew, gw, rtol=0, atol=1e-6 * mw.max()) and np.allclose(eb, gb, rtol=0, atol=1e-6 * mb.max())


def test_ema_reference():
    p, g, _, _, _ = (a for a in G.table_data()[4])
    for tau in G.EMA_TAUS:
        want = A.ema_ref(p, g, tau)
        got = A.ema32(p, g, F32(tau), F32(1.0 - tau))
        assert got.dtype == F32 and np.allclose(got, want, rtol=0, atol=4 * A.U * (np.abs(p) + np.abs(g)).max())
    assert not np.array_equal(A.ema32(p, g, F32(0.999), F32(0.001)), A.ema32(p, g, F32(0.001), F32(0.999)))


# ---- the tolerances -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rows():
    return G.measure(big=False)


def _every_case():
    return ({('wgrad32', c['data']) for c in G.WGRAD32_CASES} | {('gwgrad', c['name']) for c in G.GW_CASES} | {('fused', c['name']) for c in G.FUSED_CASES} |
            {('adam', c['name']) for c in G.TABLE_CASES} | {('linear', c['name']) for c in G.LIN_CASES} | {('glinear', c['name']) for c in G.GLIN_CASES})


def test_every_case_has_its_own_ratio_and_it_is_the_emulations(rows):
    """tests/update_ratios.py holds one ratio per case and quantity; the quick pass (everything but the 33,000-row cases at 128 and 512
    columns) recomputes them"""
    assert {(op, name) for op, cases in G.RATIO.items() for name in cases} == _every_case()
    assert len(rows) == len(_every_case()) - 8
    for op, name, r in rows:
        have = G.RATIO[op][name]
        assert set(have) == set(r), (op, name)
        for q, v in r.items():
            assert abs(v - have[q]) <= 1e-3 * v + 1e-12, (op, name, q, v, have[q])
            assert G.tol(op, name, q) == 4.0 * have[q]
    # fp32 arithmetic stays a few roundings of the scale; bf16x3 at the products it drops (lo x lo, 2^-16 of one term) and, at many terms,
    # far below that: the bound of the only case that runs the rchunk formula is below one row's share of the scale
    top = lambda q: max(r[q] for cases in G.RATIO.values() for r in cases.values() if q in r)
    assert max(top(q) for q in ('wgrad32_w', 'wgrad32_b', 'adam_p', 'adam_m', 'adam_v', 'glin_w', 'glin_b', 'lin_b')) < 8
    assert top('gwgrad_b') < 16 and max(top('gwgrad_w'), top('lin_w')) < 2 * 2.0 ** 8
    for c in G.LIN_CASES:
        if c['R'] == 33000:
            assert G.tol('linear', c['name'], 'lin_w') * A.U < 0.1 / 33000, c['name']


def test_profile_holds_the_ratios_next_to_their_bounds():
    text = open(os.path.join(ROOT, 'profiles', 'update_elementwise.txt')).read()
    for op, cases in G.RATIO.items():
        for name, r in cases.items():
            for q, v in r.items():
                assert re.search(r'^%s\s+%s\s+%s\s+%s\s+%s\s' % (op, re.escape(name), q, re.escape('%.4e' % v), re.escape('%.4e' % (4 * v))), text, re.M), (op, name, q)


def test_every_listed_case_is_a_case():
    w = {(c['b'], c['h'], c['w'], c['bf16']) for c in G.WGRAD32_CASES if c['co_stride'] == 288 and c['bias']}
    assert w == {(b, h, ww, bf) for b, h, ww in ((1, 1, 1), (1, 1, 3), (1, 3, 1), (2, 5, 7), (1, 9, 57), (1, 96, 344)) for bf in (False, True)}
    assert {c['group'] for c in G.WGRAD32_CASES if c['co_stride'] == 1152 and not c['bias']} == {0, 1, 2, 3}
    assert A.wgrad32_chunks(33024) == (512, 72) and 459 * 72 > 33024 > 458 * 72 and A.wgrad32_chunks(513) == (9, 64) and A.wgrad32_chunks(70) == (2, 40)
    assert {(c['ci'], c['co'], c['b'], c['h'], c['w']) for c in G.GW_CASES} == {
        p + m for p in ((32, 32), (24, 32), (64, 64), (32, 128), (128, 32)) for m in ((1, 24, 40), (2, 17, 37), (1, 1, 1), (1, 3, 17))}
    assert {(c['ci'], c['co'], c['start'], c['bias']) for c in G.FUSED_CASES} == {(ci, 32, t, b) for ci in (32, 24) for t in (0, 7) for b in (True, False)}
    assert G.TABLE_SIZES == (1, 255, 256, 257, 9216, 32, 70001) and sum(G.TABLE_SIZES) > 65536
    reps = list(G.TABLE_REPS.values())
    assert any(r[0] == 0 for r in reps) and any(r[-1] == 0 for r in reps) and any(0 in r[1:-1] for r in reps) and any(2 in r and 3 in r for r in reps)
    assert {(c['wd'], c['start']) for c in G.TABLE_CASES} == {(wd, t) for wd in (0.0, 1e-4) for t in (0, 1, 99999)}
    lin = {(c['key'], c['O'], c['I'], c['R']) for c in G.LIN_CASES}
    assert lin == ({(k, o, o, r) for k in (100, 101, 110, 111) for o in (512, 128) for r in (1, 15, 16, 17, 512, 513, 33000)} |
                   {(k, 512, 32, r) for k in (0, 10) for r in (1, 15, 16, 17, 512, 513, 33000)})
    assert A.linear_wgrad_chunks(33000) == (63, 528) and A.linear_wgrad_chunks(513) == (2, 512) and A.linear_wgrad_chunks(512) == (1, 512)
    assert {(c['I'], c['O'], c['R']) for c in G.GLIN_CASES} == {(i, o, r) for i, o in ((1, 1), (63, 65), (64, 64), (130, 70)) for r in (1, 15, 17, 1672)}


def test_table_data_holds_what_it_claims():
    for p, m, v, g1, g2 in G.table_data():
        zero = g1 == 0
        assert (m[zero] == 0).all() and (v[zero] == 0).all() and (v >= 0).all()
        if p.size >= 32:
            assert zero.any() and not zero.all()
        if p.size > 1000:
            a = np.abs(g1[~zero])
            assert a.min() < 1e-11 and a.max() > 1e2 and (a < 1e-8).mean() > 0.1 and (a > 1e-8).mean() > 0.1          # far below eps, far above
    d = G.linear_data(128, 128, 17)
    assert float(np.abs(d['gt']['gc1']).min()) > 0 and np.median(np.abs(d['gt']['gc1'])) > 1e-3          # c1 of G's own size
    on = (A.linear_operands_ref(d['G'], d['X'], xscale=d['xscale'], xshift=d['xshift'])[2] > 0).mean()
    assert 0.3 < on < 0.7                                      # about half the ReLUs active


# ---- value-only slips, planted on the CPU ---------------------------------------------------------------------------------------------------
def _outside(op, case, q, got, ref, scale):
    return int((np.abs(np.asarray(got, F64) - ref) > G.bound(op, case, q, scale)).sum())


def test_planted_value_slips_are_outside_the_bounds():
    # wgrad32: clamp-to-edge padding instead of zeros
    x, gy, ref, mag = G.wgrad32_data(2, 5, 7, False)
    ew, eb = A.wgrad32_emu(x, gy)
    assert _outside('wgrad32', '2x5x7_f32', 'wgrad32_w', ew, ref[0], mag[0]) == 0 and _outside('wgrad32', '2x5x7_f32', 'wgrad32_b', eb, ref[1], mag[1]) == 0
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode='edge')
    xt, gt = torch.from_numpy(xp.astype(F64)).permute(0, 3, 1, 2), torch.from_numpy(gy.astype(F64)).permute(0, 3, 1, 2)
    clamped = torch.nn.grad.conv2d_weight(xt, (32, 32, 3, 3), gt, padding=0).numpy()
    assert _outside('wgrad32', '2x5x7_f32', 'wgrad32_w', clamped, ref[0], mag[0]) > 0 and _outside('wgrad32', '2x5x7_f32', 'wgrad32_w', clamped[:, :, 1, 1], ref[0][:, :, 1, 1], mag[0][:, :, 1, 1]) == 0
    # the reducer leaving one of its eight chunk groups out: the chunks 7, 15, ... of the 33,024-pixel map
    x, gy, ref, mag = G.wgrad32_data(1, 96, 344, False)
    n, per = A.wgrad32_chunks(33024)
    g = gy.reshape(-1, 32).astype(F64).copy()
    for c in range(7, n, 8):
        g[c * per:(c + 1) * per] = 0
    assert _outside('wgrad32', '1x96x344_f32', 'wgrad32_b', g.sum(0), ref[1], mag[1]) == 32
    # adam_multi: the step count of a repeated tensor without its + 1
    p, m, v, g1, _ = G.table_data()[4]
    hy = G.hyper_of(0.0)
    (rp, rm, rv), (mp, mm, mv) = A.adam_ref(p, m, v, g1, hy, 1, 2)
    emu = A.adam_emu(p, m, v, g1, hy, 1, 2)
    assert _outside('adam', 'rep23_wd0_t0', 'adam_p', emu[0], rp, mp) == 0 and _outside('adam', 'rep23_wd0_t0', 'adam_m', emu[1], rm, mm) == 0 and _outside('adam', 'rep23_wd0_t0', 'adam_v', emu[2], rv, mv) == 0
    b1, b2, lr, eps = float(hy[1]), float(hy[2]), float(hy[0]), float(hy[3])
    q, mq, vq = p.astype(F64), m.astype(F64), v.astype(F64)
    for tt in (1, 2):                                           # tt = (t - 1) rep + r: one behind (the first would divide by 1 - b^0 = 0; take 1, 2 -> 1, 1)
        mq, vq = b1 * mq + (1 - b1) * g1, b2 * vq + (1 - b2) * g1.astype(F64) ** 2
        q = q - lr / (1 - b1 ** 1) * mq / (np.sqrt(vq) / np.sqrt(1 - b2 ** 1) + eps)
    assert _outside('adam', 'rep23_wd0_t0', 'adam_p', q, rp, mp) > p.size // 2
    # linear_wgrad with GPRO: tail rows of the last slice fed through the transform (Gh = mean, G = 0: -gscale c1 each) move db
    c = next(c for c in G.LIN_CASES if c['name'] == 'k110_o128_i128_r17')
    d = G.linear_data(128, 128, 17)
    ref, mag = A.linear_wgrad_ref(d['G'], d['X'], **G.linear_args(c, d))
    ew, eb = A.linear_wgrad_emu(d['G'], d['X'], **G.linear_args(c, d))
    assert _outside('linear', c['name'], 'lin_w', ew, ref[0], mag[0]) == 0 and _outside('linear', c['name'], 'lin_b', eb, ref[1], mag[1]) == 0
    slip = ref[1] - 15 * d['gt']['gscale'].astype(F64) * d['gt']['gc1'].astype(F64)
    assert _outside('linear', c['name'], 'lin_b', slip, ref[1], mag[1]) == 128
