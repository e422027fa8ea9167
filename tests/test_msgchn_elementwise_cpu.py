"""CPU side of the per-element tests of the MSG_CHN step's first-layer / prediction convolutions, resamplings and loss
(tests/test_gpu_msgchn_elementwise.py): the hooks are declared and bound alike, every float64 reference of oracle/msgchn_arith.py agrees with
an independent formulation (torch operators, autograd, oracle/proxytta_oracle.py), the cases hold what they claim, the tolerances of
tests/msgchn_cases.py are 4 x the float32 emulation's recomputed error and stand in profiles/msgchn_elementwise.txt -- never a GPU figure --
and the five-tap window claim of csrc/resample.hip's up2T_window holds for every map size the step can see."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import msgchn_arith as A
from oracle import proxytta_oracle as O
from proxytta import _lib
from tests import msgchn_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
HOOKS = ('ptta_op_conv_in', 'ptta_op_conv_out1', 'ptta_op_prep', 'ptta_op_up2_1ch', 'ptta_op_up2t_1ch', 'ptta_op_up2t_32', 'ptta_op_loss')
STRUCTS = {'ptta_plane': _lib.PlaneArg, 'ptta_conv_in_args': _lib.ConvInArgs, 'ptta_conv_out1_args': _lib.ConvOut1Args, 'ptta_loss_args': _lib.LossArgs}
CTYPES = {'int': ctypes.c_int, 'float': ctypes.c_float, 'long long': ctypes.c_longlong}


def _ctype_of(decl):
    decl = decl.strip()
    return 'ptr' if '*' in decl or decl.startswith('ptta_stream') else CTYPES[re.sub(r'\s+\w+$', '', decl)]


def test_hooks_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    sig = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    for name in HOOKS:
        m = re.search(r'^int %s\((.*?)\);' % name, header, re.S | re.M)
        assert m, name
        want = [_ctype_of(a) for a in m.group(1).replace('\n', ' ').split(',')]
        res, args = sig[name]
        assert res is ctypes.c_int and len(args) == len(want), name
        for k, (a, w) in enumerate(zip(args, want)):
            is_ptr = a is ctypes.c_void_p or issubclass(a, ctypes._Pointer)
            assert (w == 'ptr' and is_ptr) or a is w, (name, k, a, w)
    for name, cls in STRUCTS.items():
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), header, re.S).group(1)
        fields = []
        for decl in body.split(';'):
            decl = decl.strip()
            if not decl:
                continue
            m = re.match(r'(const\s+)?(long long|int|float|uint32_t|ptta_plane)\s*(.*)', decl)
            for n in m.group(3).split(','):
                n = n.strip()
                kind = 'ptr' if n.startswith('*') else m.group(2)
                fields.append((n.strip('* ').split('[')[0], kind))
        got = [(n, 'ptr' if t is ctypes.c_void_p else {ctypes.c_int: 'int', ctypes.c_float: 'float', ctypes.c_longlong: 'long long'}.get(t, 'ptta_plane'))
               for n, t in cls._fields_]
        assert fields == got, (name, fields, got)            # the same fields, kinds and order
    assert re.search(r'#define PTTA_ABI_VERSION 2\b', header) and _lib.PTTA_ABI_VERSION == 2
    for table, prefix in ((_lib.LOSS_FWD, 'PTTA_LOSS_FWD_'), (_lib.LOSS_BWD, 'PTTA_LOSS_BWD_')):
        for key, val in table.items():
            assert re.search(r'#define %s%s %d\b' % (prefix, key.upper(), val), header), key


# ---- the bounds ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rows():
    return G.measure()


def test_tolerances_are_four_times_the_emulations_error(rows):
    worst = G.worst(rows)
    assert set(worst) == set(G.TOL) == set(G.QUANTITIES)
    for q, r in worst.items():
        assert r > 0 and 4.0 * r <= G.TOL[q] * 1.001 and G.TOL[q] <= 4.0 * r * 1.001, (q, r, G.TOL[q])
    # every bound stays a few fp32 roundings of its magnitude
    assert max(G.tol(q) for q in G.QUANTITIES) < 32 * 2.0 ** -24 and set(G.EXTRA) <= set(G.QUANTITIES)


def test_profile_holds_the_tolerances():
    text = open(os.path.join(ROOT, 'profiles', 'msgchn_elementwise.txt')).read()
    for q, r in G.RATIO.items():
        assert re.search(r'^%s\s+%s\s+\S+\s+%d\s' % (q, re.escape('%.3e' % r), G.EXTRA.get(q, 0)), text, re.M), q


def test_profile_per_case_table_is_the_emulations(rows):
    text = open(os.path.join(ROOT, 'profiles', 'msgchn_elementwise.txt')).read()
    generated = G.report(rows).split('Per case, CPU emulation:')[1]
    assert generated.strip() in text


def test_narrow_bound_is_half_a_bf16_spacing():
    v = np.array([1.0, 1.003, 1.99, 2.0, 0.75, 3e-5, 0.0], F32)
    half = A.bf16_half_ulp(v)
    r = A.bf16_round(v)
    assert np.array_equal(r, torch.from_numpy(v).bfloat16().float().numpy())
    assert (np.abs(r.astype(F64) - v) <= half).all() and (half <= 2.0 ** -8 * np.abs(v)).all() and (half[v > 0] > 2.0 ** -9 * np.abs(v[v > 0]) * 0.999).all()
    assert abs(float(r[1]) - 1.003) > 2.0 ** -9 * 1.003          # why 2^-9 |ref| alone cannot be the bound
    rng = G.rng_of('bf16')
    x = (rng.standard_normal(4096) * np.exp(rng.uniform(-20, 20, 4096))).astype(F32)
    assert np.array_equal(A.bf16_round(x), torch.from_numpy(x).bfloat16().float().numpy())
    assert (np.abs(A.bf16_round(x).astype(F64) - x) <= A.bf16_half_ulp(x)).all()


# ---- the references against independent formulations --------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, F64))


@pytest.mark.parametrize('hin,win', G.UP_SIZES, ids=lambda v: str(v))
def test_bilinear_reference_is_interpolate_and_its_autograd(hin, win):
    d = G.make_up(hin, win)
    x = _t(d['x'])[:, None].requires_grad_(True)
    y = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True)
    assert np.allclose(y.detach().numpy()[:, 0], A.up2_ref(d['x'])[0], rtol=0, atol=1e-13)
    (gx,) = torch.autograd.grad(y, x, _t(d['g'])[:, None])
    assert np.allclose(gx.numpy()[:, 0], A.up2t_ref(d['g'])[0], rtol=0, atol=1e-12)
    x32 = _t(d['add32']).permute(0, 3, 1, 2).requires_grad_(True)
    y32 = F.interpolate(x32, scale_factor=2, mode='bilinear', align_corners=True)
    (g32,) = torch.autograd.grad(y32, x32, _t(d['g32']).permute(0, 3, 1, 2))
    ref, mag = A.up2t_ref(d['g32'], d['add32'])
    assert np.allclose(g32.permute(0, 2, 3, 1).numpy() + d['add32'], ref, rtol=0, atol=1e-12) and (mag >= np.abs(ref) - 1e-12).all()
    U, T = A.up2_matrix(win)
    assert np.allclose(U.sum(1), 1) and ((U > 0) <= (T > 0)).all() and (T.sum(1) <= 2).all()


@pytest.mark.parametrize('c', G.CONV_IN_CASES, ids=lambda c: c['name'])
def test_conv_in_reference_is_conv2d(c):
    """The reference against conv2d on the de-planarised input with the state dict's weight, the flipped packing against autograd through
    the 32 -> 1 convolution and against the explicit transposed-weight formula (conv_transpose2d)."""
    d = G.make_conv_in(c)
    ref = A.conv_in_ref(**G.conv_in_kwargs(c, d))
    B = c['b']
    x = torch.stack([_t(p)[torch.arange(B) % p.shape[0]] for p, _ in d['planes']], 1)
    if c['norm']:
        x = torch.stack([(x[:, k] / float(F32(n[0])) - float(F32(n[1]))) / float(F32(n[2])) for k, (_, n) in enumerate(d['planes'])], 1)
    x[c['zero_from_b']:] = 0
    if c['flip']:
        h32 = torch.zeros(B, 32, c['h'], c['w'], dtype=torch.float64, requires_grad=True)
        out1 = F.conv2d(h32, _t(d['weight']), padding=1)
        (v,) = torch.autograd.grad(out1, h32, x)                                       # x = the gradient of the one-channel output
        assert torch.allclose(v, F.conv_transpose2d(x, _t(d['weight']), padding=1), rtol=0, atol=1e-12)
    else:
        w = _t(d['weight'])[:, c['cin_first']:c['cin_first'] + c['cin']]
        v = F.conv2d(x, w, padding=1)
    v = v.permute(0, 2, 3, 1)
    idx = lambda t: torch.arange(B) % t.shape[0]
    if d['bias'] is not None:
        v = v + _t(d['bias'])
    if d['up'] is not None:
        v = v + F.interpolate(_t(d['up']).permute(0, 3, 1, 2), scale_factor=2, mode='bilinear', align_corners=True).permute(0, 2, 3, 1)[idx(d['up'])]
    if d['mask'] is not None:
        v = torch.where(_t(d['mask']) > 0, v, torch.zeros_like(v))
    assert np.allclose(v.numpy(), ref['raw'], rtol=0, atol=1e-11)
    s = v if d['add1'] is None else v + _t(d['add1'])[idx(d['add1'])]
    assert np.allclose(s.numpy(), ref['sum'], rtol=0, atol=1e-11)
    assert (ref['mag_raw'] >= np.abs(ref['raw']) - 1e-11).all() and (ref['mag_sum'] >= np.abs(ref['sum']) - 1e-11).all()
    if c['norm']:                                        # the padding stays zero: a normalised zero would be about -2 per channel
        assert min(abs((0.0 / n[0] - n[1]) / n[2]) for _, n in d['planes']) > 1.5
    if d['mask'] is not None:
        bits = A.sign_bits(d['mask'])
        assert all(np.array_equal((bits >> np.uint32(ch)) & 1, d['mask'][..., ch] > 0) for ch in (0, 5, 31)) and bits[0, 0, 0] == 0


@pytest.mark.parametrize('c', G.CONV_OUT1_CASES, ids=lambda c: c['name'])
def test_conv_out1_reference_is_conv2d(c):
    """... and the first layer's weight packed as an input gradient against autograd through that layer, with respect to its plane 1"""
    d = G.make_conv_out1(c)
    ref, mag = A.conv_out1_ref(**G.conv_out1_kwargs(c, d))
    B = c['b']
    x = _t(d['x'])[torch.arange(B) % c['in_nb']].permute(0, 3, 1, 2)
    x = F.relu(x) if c['relu'] else x
    if c['from_conv_in']:
        planes = torch.zeros(B, 2, c['h'], c['w'], dtype=torch.float64, requires_grad=True)
        (g,) = torch.autograd.grad(F.conv2d(planes, _t(d['weight']), padding=1), planes, x)
        v = g[:, 1]
        assert torch.allclose(v, F.conv_transpose2d(x, _t(d['weight']), padding=1)[:, 1], rtol=0, atol=1e-11)
    else:
        v = F.conv2d(x, _t(d['weight']), padding=1)[:, 0]
    if d['bias'] is not None:
        v = v + float(d['bias'][0])
    if d['add'] is not None:
        v = v + _t(d['add'])[torch.arange(B) % c['add_nb']]
    assert np.allclose(v.numpy(), ref, rtol=0, atol=1e-11) and (mag >= np.abs(ref) - 1e-11).all()


@pytest.mark.parametrize('c', G.PREP_CASES, ids=lambda c: c['name'])
def test_pooled_reference_is_the_oracles(c):
    s = G.make_prep(c)
    dc, ref = A.prep_ref(s, c['max_d'])
    t = torch.from_numpy(s)[:, None]
    t = torch.clamp(t, 0, c['max_d']) if c['max_d'] >= 0 else t
    assert np.array_equal(t[:, 0].numpy(), dc)
    for k in (2, 4):
        assert np.allclose(O.sparse_pool(t.double(), k)[:, 0].numpy(), ref[k][0], rtol=1e-7, atol=0)
        assert (ref[k][1] == 0).any()                    # a block without a valid point


@pytest.fixture(scope='module')
def loss_refs():
    out = {}
    for c in G.LOSS_CASES:
        d = G.make_loss(c)
        out[c['name']] = (d, A.loss_ref(**G.loss_args(c, d)))
    return out


@pytest.mark.parametrize('c', G.LOSS_CASES, ids=lambda c: c['name'])
def test_loss_reference_is_the_oracles_and_the_cases_hold_their_claims(c, loss_refs):
    d, ref = loss_refs[c['name']]
    t = lambda a: _t(a)[:, None]
    dep = t(d['depth']).requires_grad_(True)
    rf = _t(d['ref']).requires_grad_(True)
    sp = t(d['sparse'])
    val = torch.where(sp > 0, torch.ones_like(sp), sp) if d['validity'] is None else t(d['validity'])
    w3 = [float(F32(v)) for v in c['w3']]
    loss, parts = O.adapt_loss(_t(d['image']), dep, sp, val, _t(d['emb']), rf, *w3, max_input_depth=c['max_d'] if c['max_d'] >= 0 else None)
    loss.backward()
    got = [float(v.detach()) for v in (loss, parts['loss_smooth'], parts['loss_sparse_depth'], parts['loss_cos'])]
    assert np.allclose(got, ref['info'], rtol=1e-9, atol=0)
    assert np.allclose(dep.grad[:, 0].numpy(), ref['gdepth'], rtol=1e-9, atol=1e-15)
    assert np.allclose(rf.grad.numpy(), ref['gref'], rtol=1e-6, atol=1e-15)          # (the zero row's 1 / eps: 1e-12 as fp32 here, as float64 there)
    # the gate, on the side the case names, at a distance no fp32 rounding of l_cos bridges
    l_cos = ref['info'][3]
    assert abs(l_cos - 0.3) >= G.GATE_MARGIN and (l_cos < 0.3) == (c['gate'] == 'closed') and (ref['wc'] == 0) == (c['gate'] == 'closed')
    if c['gate'] == 'closed':
        assert (ref['gref'] == 0).all() and np.isclose(ref['info'][0], w3[0] * ref['info'][2] + w3[1] * ref['info'][1], rtol=1e-12)
    # the planted content
    cs = A.clamp_ref(d['sparse'], c['max_d'])
    wv = np.where(d['sparse'] > 0, 1.0, d['sparse']) if d['validity'] is None else d['validity']
    assert ((d['depth'] == cs) & (wv != 0)).any() and (ref['gdepth'] == 0).any()
    assert (d['depth'][:, :, :-1] == d['depth'][:, :, 1:]).any() and (d['depth'][:, :-1] == d['depth'][:, 1:]).any()
    assert not d['ref'][1].any() and not d['emb'][2].any() and ref['rowstats'][1, 1] == A.EPS_NORM
    assert np.array_equal(A.bf16_round(d['emb']), d['emb']) and np.array_equal(A.bf16_round(d['ref']), d['ref'])
    if c['validity'] is None:
        assert (d['sparse'] < 0).any()
    if c['validity'] == 'given':
        assert (d['validity'] != np.where(d['sparse'] > 0, 1.0, d['sparse'])).any()
    assert (ref['mag_info'] >= np.abs(ref['info']) * (1 - 1e-12)).all() and (ref['mag_gdepth'] >= np.abs(ref['gdepth']) * (1 - 1e-9)).all()


def test_loss_cases_cover_the_loops_and_both_sides_of_the_fused_limit():
    by = G.LOSS_BY_NAME
    assert {c['n'] for c in G.LOSS_CASES} >= {1, 3, 16, 17}
    big = by['n2_260x256_r4100']
    assert big['h'] * big['w'] > 256 * 256 and big['n'] * big['h'] * big['w'] > 512 * 256 and big['r'] > 4 * A.LOSS_CB
    assert any(c['d'] == 8 for c in G.LOSS_CASES) and any(c['gate'] == 'closed' for c in G.LOSS_CASES) and any(c['max_d'] < 0 for c in G.LOSS_CASES)


# ---- the five-tap window of the transposed bilinear ------------------------------------------------------------------------------------------
WINDOW_SIZES = list(range(1, 701)) + [1216, 608, 304, 152, 2432]


def test_up2t_window_holds_every_touching_destination():
    """csrc/resample.hip up2T_window: every destination whose float32 taps touch source index i with a non-zero weight lies among the seven
    candidates 2 i - 3 .. 2 i + 3 AND inside the clamped five-wide window, with the weight the full scan finds -- for every map size the
    gather can meet (1 .. 700 and the benchmark's widths)."""
    for n in WINDOW_SIZES:
        scale = A.up_scale(n, 2 * n)
        dd, ii = A.touching(n)
        first, w5 = A.up2t_window(np.arange(n), n, scale)
        assert (first >= 0).all() and (first + 4 < max(2 * n, 5)).all(), n
        off = dd - first[ii]
        assert ((dd >= 2 * ii - 3) & (dd <= 2 * ii + 3)).all(), n
        assert ((off >= 0) & (off < 5)).all(), (n, int(ii[(off < 0) | (off >= 5)][0]))
        assert (w5[ii, np.clip(off, 0, 4)] != 0).all(), n
        # nothing else carries weight, and the weights of one destination sum to one over the sources
        total = np.zeros(2 * n)
        np.add.at(total, np.clip(first[:, None] + np.arange(5), 0, 2 * n - 1).ravel(), np.where(first[:, None] + np.arange(5) < 2 * n, w5, 0).astype(F64).ravel())
        assert np.allclose(total, 1.0, rtol=0, atol=2e-6) and int((w5 != 0).sum()) == len(dd), n


def test_no_source_is_touched_by_more_than_four_destinations():
    """How much room the five-wide window has: in float32, at every size above, a source collects at most FOUR destinations (the open
    interval of the claim is 4 + 2 / (in - 1) long, and its fifth integer would lie past the map's end), and they start at candidate 2 i - 1
    or at destination 0 -- so a gather narrowed consistently to four taps loses nothing, while one that drops a touching tap does."""
    for n in WINDOW_SIZES:
        dd, ii = A.touching(n)
        lo = np.full(n, 2 * n)
        np.minimum.at(lo, ii, dd)
        assert np.bincount(ii, minlength=n).max() <= 4 and (lo == np.maximum(2 * np.arange(n) - 1, 0)).all(), n
