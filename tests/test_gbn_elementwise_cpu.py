"""CPU-only side of the per-element BatchNorm tests (tests/test_gpu_gbn_elementwise.py): the hook's declaration, the tolerances, the
zero-ambiguity condition of the mask ties, the branches the case list reaches, and planted wrong arithmetics that the bounds reject.

Tolerances (tests/gbn_cases.py TOL) are 4 x the CPU emulation's largest error ratio per quantity over the cases,
profiles/gbn_elementwise.txt -- never a GPU figure."""
import os
import re

import numpy as np
import pytest

from oracle import gbn_arith as A
from proxytta import _lib
from tests import gbn_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c for c in G.CASES if not c['big']]


def test_op_gbn_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    assert re.search(r'int ptta_op_gbn\(const ptta_gbn_args\* a, ptta_stream s\);', header)
    sig = {name: args for name, _, args in _lib.SIGNATURES}
    assert len(sig['ptta_op_gbn']) == 2
    body = re.search(r'typedef struct ptta_gbn_args \{(.*?)\} ptta_gbn_args;', header, re.S).group(1)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names += [n.strip(' *') for n in re.sub(r'^(const\s+)?(long long|ptta_gbn_view|int|float)\s*\*?', '', decl).split(',')]
    assert names == [n for n, _ in _lib.GbnArgs._fields_], names          # the same fields in the same order
    assert [n for n, _ in _lib.GbnView._fields_] == ['p', 'c', 'ld']
    from proxytta.engine import GBN_ACTS, GBN_MODES
    for name, val in (('PTTA_GBN_TRAIN', GBN_MODES['train']), ('PTTA_GBN_EVAL', GBN_MODES['eval']), ('PTTA_GBN_BACKWARD', GBN_MODES['backward'])):
        assert re.search(r'#define %s %d\b' % (name, val), header)
    assert GBN_ACTS == {'none': 0, 'relu': 1, 'lrelu': 2, 'elu': 4}      # GACT_* of csrc/ptta_kernels.h


@pytest.fixture(scope='module')
def rows():
    return G.measure(SMALL)


def test_tolerances_are_four_times_the_emulations_error(rows):
    """The constants against the ratios recomputed here (the one full-size case is left to `python -m tests.gbn_cases`; it holds no
    quantity's largest ratio)."""
    worst = G.worst(rows)
    assert set(worst) == set(G.TOL) == set(G.QUANTITIES)
    for q, r in worst.items():
        assert 4.0 * r <= G.TOL[q] * 1.001 and G.TOL[q] <= 4.0 * r * 1.001, (q, r, G.TOL[q])
    # the nudge's margin is at least the forward bound, and every tolerance stays a few fp32 roundings
    assert G.TOL['y'] <= G.TIE and max(G.TOL.values()) < 16 * 2.0 ** -24


def test_no_element_is_ambiguous(rows):
    """Zero elements within the forward bound of a mask tie in every case; the structured channels survive the nudge."""
    for name, _, _, amb in rows:
        assert amb == 0, name
    assert sum(n for _, _, n, _ in rows) > 0                             # the nudge had something to do
    for name in ('cond_relu', 'cond_npass2_lrelu'):
        x = G.make(G.BY_NAME[name])['x']
        k = G.COND_RATIOS.index('const')
        assert float(np.ptp(x[..., k])) == 0.0, name
        assert float(x[..., G.COND_RATIOS.index('tiny')].var()) < 1e-2 * G.EPS, name


def test_conditioning_channels_are_what_they_claim():
    c = G.BY_NAME['cond_none']
    fw = G.reference(c, G.make(c))[0]
    ratio = np.abs(fw['mean'][0]) / np.sqrt(np.maximum(fw['var'][0], 1e-300))
    for k, want in enumerate(G.COND_RATIOS):
        if want == 'const':
            assert fw['var'][0, k] == 0.0 and fw['kappa'][0, k] > 1e4
        elif want == 'tiny':
            assert fw['var'][0, k] < 1e-2 * G.EPS
        elif want == 0.0:
            assert ratio[k] < 0.2 and fw['kappa'][0, k] < 1.1
        else:
            assert 0.8 * abs(want) < ratio[k] < 1.25 * abs(want), (k, ratio[k])
    assert fw['kappa'][0].max() > 6e4                                     # mean / std = 256: 2^16 of cancellation


def test_every_listed_branch_is_reached():
    """From blocks, nsub and pstride as the launcher computes them (oracle/gbn_arith.geometry)."""
    geo = {c['name']: G.geometry(c) for c in G.CASES}
    by = lambda pred: [c['name'] for c in G.CASES if pred(c, geo[c['name']])]
    # channel geometry
    assert {g['nsub'] for g in geo.values()} >= {64, 32, 5, 4, 1}
    assert by(lambda c, g: c['c'] == 48 and g['idle_threads'] == 16)
    assert by(lambda c, g: g['partial_last_channel_block']) and by(lambda c, g: c['c'] == 512 and g['channel_blocks'] == 2)
    assert by(lambda c, g: c['c'] == 1024 and g['channel_blocks'] == 4 and c['w'] == 1)
    # pixels per pass
    for r in (1, 2, 8):
        assert by(lambda c, g: G.pixels(c) == r), r
    assert by(lambda c, g: G.pixels(c) == 2 and c['b'] == 2 and c['h'] == c['w'] == 1)
    assert by(lambda c, g: G.pixels(c) == 8 and c['c'] == 512)
    assert by(lambda c, g: G.pixels(c) % 2 == 1 and G.pixels(c) < g['nsub'] and g['blocks'] == 1)
    for ch in (256, 64):
        full = lambda c, g: c['c'] == ch and g['blocks'] == A.BLOCKS
        assert by(lambda c, g: full(c, g) and g['unrolled_max'] == 0 and G.pixels(c) == 3 * g['pstride']), ch
        assert by(lambda c, g: full(c, g) and g['unrolled_max'] == 1 and G.pixels(c) == 3 * g['pstride'] + 1), ch
        assert by(lambda c, g: full(c, g) and g['unrolled_max'] == 1 and g['tail_after_unrolled']), ch
    assert by(lambda c, g: g['capped'] and G.pixels(c) % g['pstride'])
    assert by(lambda c, g: g['threads_without_pixel']) and by(lambda c, g: g['tail_only'] and g['unrolled_max'] > 0)
    # the apply kernels' grid-stride loop: exactly the one big case
    assert by(lambda c, g: c['b'] * c['h'] * c['w'] * c['c'] // 4 > 16384 * 256) == [c['name'] for c in G.CASES if c['big']] == ['apply_grid_stride']
    # both loops of gbn_sum_partials_block, for the caller-made partials
    assert sorted(c['nblocks'] for c in G.CASES if c['nblocks']) == [1, 2, 255, 257, 1023, 1024 + 769, 3344]
    loops = {n: A.reducer_loops(n) for n in (1, 2, 255, 257, 1023, 1793, 3344)}
    assert loops[255] == (0, 1) and loops[257] == (0, 2) and loops[1023] == (1, 3) and loops[1793] == (2, 3) and loops[3344] == (3, 2)
    # switches
    combos = {(c['act'], c['res'], c['act_first'], c['res_relu']) for c in G.CASES}
    assert {(a, False, False, True) for a in ('none', 'relu', 'lrelu', 'elu')} <= combos
    assert {('none', True, False, True), ('relu', True, True, True), ('none', True, False, False), ('relu', False, True, True)} <= combos
    assert {(c['acc_gx'], c['acc_gres']) for c in G.CASES if c['res']} == {(False, False), (True, False), (False, True), (True, True)}
    assert by(lambda c, g: c['frozen']) and len(by(lambda c, g: c['views'])) >= 3
    # views: all six tensors of a residual block in one case, every offset a multiple of 4, six different row strides
    assert by(lambda c, g: c['views'] and c['res']) and set(G.VIEW_PADS) == {'x', 'res', 'y', 'g', 'gx', 'gres'}
    assert all(a % 4 == 0 and b % 4 == 0 for a, b in G.VIEW_PADS.values()) and len({a + b for a, b in G.VIEW_PADS.values()}) == 6
    # the inner mask of relu(relu(bn x) + res) under [real | proxy]; an eval forward with a residual, both block forms
    assert by(lambda c, g: c['npass'] == 2 and c['data'] == 'proxy0' and c['res'] and c['act_first'])
    assert by(lambda c, g: c['track'] and c['res'] and c['act_first']) and by(lambda c, g: c['track'] and c['res'] and not c['act_first'])
    assert {(c['npass'], c['repeats']) for c in G.CASES if c['track'] and c['world'] == 1} == {(1, 1), (1, 2), (2, 1), (2, 2)}
    assert by(lambda c, g: c['world'] == 2 and g['blocks'] == 1) and len(by(lambda c, g: c['world'] == 2 and g['blocks'] > 1)) >= 2
    assert by(lambda c, g: c['npass'] == 2 and c['data'] == 'proxy0' and c['act'] == 'relu')
    # no case asks for a combination the launchers refuse
    for c in G.CASES:
        assert not (c['res'] and not c['res_relu'] and c['act'] != 'none') and not (c['res'] and c['res_relu'] and c['act_first'] and c['act'] != 'relu')


def _drop(c, what):
    R, g = G.pixels(c), G.geometry(c)
    d = np.zeros(R, bool)
    if what == 'drop_tail_pixel':
        d[R - 1] = True                                                    # the last pixel of the pass: a tail-loop pixel in these cases
    else:
        d[(np.arange(R) % g['pstride']) // g['nsub'] == 1] = True          # everything block 1 sums
    return d


# fault -> (the cases built for it, the quantities it must push outside the bound)
PLANTED = {
    'biased_running_var': (('track_p1_r1', 'track_p1_r2', 'track_p2_r1', 'track_p2_r2', 'world2_c320_track'), ('rv',)),
    'no_eps': (('cond_none', 'cond_elu'), ('inv', 'y')),
    'shared_stats': (('npass2_proxy_zero', 'npass2_proxy_zero_res', 'npass2_random', 'cond_npass2_lrelu'), ('mean', 'inv', 'y')),
    'bwd_pass1_stats': (('npass2_proxy_zero', 'npass2_proxy_zero_act_first', 'npass2_proxy_zero_res', 'npass2_random', 'cond_npass2_lrelu', 'views_res'), ('gx', 'dgamma')),
    'drop_tail_pixel': (('r4097_c256_unroll1_tail', 'r16385_c64_unroll1_tail', 'r7_below_nsub', 'r3073_c256_unroll1'), ('mean', 'inv', 'dbeta', 'dgamma')),
    'drop_block': (('c4_nsub64', 'c256_nsub1', 'c320_partial_block', 'r12288_c64_unroll0', 'r8_c512_last_map'), ('mean', 'inv', 'dbeta', 'dgamma')),
    'gres_after_inner_mask': (('res_act_first', 'npass2_proxy_zero_act_first', 'res_acc_both', 'views_act_first'), ('gres',)),
    'dgamma_no_world': (('world2_c48_res', 'world2_c320_track', 'world2_single_block'), ('dgamma',)),
}
assert set(PLANTED) == set(A.FAULTS)


@pytest.mark.parametrize('fault', A.FAULTS)
def test_planted_wrong_arithmetic_lands_outside_the_bound(fault):
    """The emulation stands in for a correct GPU result: inside the bound of the true reference, and outside the bound around a
    reference with the fault planted in it, in every quantity named and in every case built for the fault."""
    names, quantities = PLANTED[fault]
    for name in names:
        c = G.BY_NAME[name]
        d = G.make(c)
        fe, be = G.emulation(c, d)
        got = G.emu_quantities(fe, be)
        true = G.reference(c, d)
        drop = _drop(c, fault) if fault.startswith('drop_') else None
        wrong = G.reference(c, d, fault=fault, drop=drop)
        ok = G.ratios(got, true)
        bad = G.ratios(got, (wrong[0], true[1], wrong[2], true[3]))        # the wrong values inside the true bounds' widths
        for q in quantities:
            if q == 'gres':
                width = G.TOL_GRES_ACC * true[3]['gres']
                assert bool((np.abs(be['gres'] - true[2]['gres']) <= width).all()), (fault, name)
                assert not bool((np.abs(be['gres'] - wrong[2]['gres']) <= width).all()), (fault, name)
                continue
            assert ok[q] <= G.TOL[q], (fault, name, q, ok[q])
            assert not bad[q] <= G.TOL[q], (fault, name, q, bad[q], G.TOL[q])
