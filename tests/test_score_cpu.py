"""The run score without a GPU: the numpy restatement of tests/score_cases.py against what the REAL eval_utils gave on the same frames
(tests/golden/run_score.npz, written by tests/golden/make_golden_run_score.py), eval_window, the binding against include/ptta.h, and the
case table the GPU test relies on.

The bound of the comparison with the reference is 2 x `worst_rel` of the fixture: the largest relative difference the generator measured
between the reference's fp32 means and the exact sums of the same fp32 elements, over the committed cases (1.4e-7).  That is the
reference's own fp32 summation error; the elements themselves are bit-equal."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from proxytta import _lib, score
from tests import score_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ('mae', 'rmse', 'imae', 'irmse')


@pytest.fixture(scope='module')
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'run_score.npz'))
    assert list(g['names']) == [c['name'] for c in C.CASES] and list(g['rules']) == [C.ADAPT, C.VALIDATE]
    return g


def within(got, ref, bound):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    finite = np.isfinite(ref)
    return np.array_equal(finite, np.isfinite(got)) and bool(np.all(np.abs(got[finite] - ref[finite]) <= bound * np.abs(ref[finite])))


@pytest.mark.parametrize('index', range(len(C.CASES)), ids=[c['name'] for c in C.CASES])
def test_restatement_against_the_references_results(golden, index):
    c = C.CASES[index]
    out, gt = C.case_frames(c)
    assert C.crc(out, gt) == int(golden['crcs'][index]), 'the frame generator drifted: regenerate tests/golden/run_score.npz'
    bound = 2.0 * float(golden['worst_rel'])
    assert 0.0 < bound < 1e-6
    for j, rule in enumerate((C.ADAPT, C.VALIDATE)):
        r = C.restate_batch(out, gt, c['window'], rule=rule)
        assert r['count'] == int(golden['counts'][index, j]) == int(r['sample_count'].sum())
        assert within(r['metrics'], golden['metrics'][index, j], bound), (rule, r['metrics'], golden['metrics'][index, j])
        np.testing.assert_allclose(r['sample_sums'].sum(axis=0), r['sums'], rtol=1e-14)


def test_run_restatement_against_the_references_bookkeeping(golden):
    batches = C.run_frames()
    assert [C.crc(o, g) for o, g in batches] == [int(v) for v in golden['run_crcs']]
    assert [o.shape[0] for o, _ in batches] == [4, 4, 1] and batches[0][0].shape[2:] == (9, 13)
    bound = 2.0 * float(golden['worst_rel'])
    assert 9 in golden['run_n_samples'] and 0 in golden['run_n_samples']
    for j, rule in enumerate((C.ADAPT, C.VALIDATE)):
        for k, ns in enumerate(int(v) for v in golden['run_n_samples']):
            r = C.restate_run(batches, rule=rule, n_sample=ns)
            assert within([r[m] for m in METRICS], golden['run_metrics'][j, k], bound), (rule, ns)
            assert (r['frames'], r['batches'], r['empty_batches']) == (9, 3, 0)


@pytest.mark.parametrize('name', ['boundary_values', 'boundary_values_aligned'])
def test_the_two_rules_differ_by_exactly_the_pixels_on_a_bound(golden, name):
    c = C.case(name)
    out, gt = C.case_frames(c)
    wy, wx, wh, ww = C.window_of(c)
    g = gt[:, 0, wy:wy + wh, wx:wx + ww]
    on_bound = int((g == C.F(C.LO)).sum() + (g == C.F(C.HI)).sum())
    assert on_bound == sum(C.BOUNDARY_PIXELS) and int((g == C.F(C.LO)).sum()) == C.BOUNDARY_PIXELS[0]
    a, v = C.restate_batch(out, gt, c['window'], rule=C.ADAPT), C.restate_batch(out, gt, c['window'], rule=C.VALIDATE)
    assert a['count'] - v['count'] == on_bound
    i = [x['name'] for x in C.CASES].index(name)
    assert int(golden['counts'][i, 0]) - int(golden['counts'][i, 1]) == on_bound
    plain = C.case('ragged_window')
    o2, g2 = C.case_frames(plain)
    assert C.restate_batch(o2, g2, plain['window'], rule=C.ADAPT)['count'] == C.restate_batch(o2, g2, plain['window'], rule=C.VALIDATE)['count']


def test_all_zero_ground_truth_gives_nan_in_both(golden):
    c = C.case('empty_batch')
    i = [x['name'] for x in C.CASES].index('empty_batch')
    out, gt = C.case_frames(c)
    for j, rule in enumerate((C.ADAPT, C.VALIDATE)):
        r = C.restate_batch(out, gt, c['window'], rule=rule)
        assert r['count'] == 0 and np.isnan(r['metrics']).all() and np.isnan(golden['metrics'][i, j]).all()
    run = C.restate_run([C.case_frames(C.case('full_odd_width')), (out, gt)])
    assert run['empty_batches'] == 1 and all(math.isnan(run[m]) for m in METRICS)
    e = C.case('empty_sample')
    r = C.restate_batch(*C.case_frames(e), e['window'])
    assert list(r['sample_count'] == 0) == [False, True, False] and np.isnan(r['sample_metrics'][1]).all() and np.isfinite(r['metrics']).all()


def test_eval_window():
    assert score.eval_window('vkitti', 375, 1242) == (135, 13, 240, 1216)
    assert score.eval_window('nuscenes', 900, 1600) == (356, 0, 544, 1600)
    assert score.eval_window('vkitti', 240, 1216) == (0, 0, 240, 1216)
    assert score.eval_window('vkitti', 352, 1217) == (112, 0, 240, 1216)
    assert score.eval_window('kitti', 352, 1216) == (0, 0, 352, 1216) and score.eval_window(None, 5, 7) == (0, 0, 5, 7)
    for name, h, w in (('vkitti', 239, 1242), ('vkitti', 375, 1215), ('nuscenes', 543, 1600), ('nuscenes', 900, 1599), ('kitti', 0, 7), ('kitti', 5, 0)):
        with pytest.raises(ValueError):
            score.eval_window(name, h, w)


def test_run_score_refuses_on_the_host():
    with pytest.raises(ValueError):
        score.RunScore(0.0, 100.0, rule='train')
    with pytest.raises(ValueError):
        score.RunScore(0.0, 100.0, window=(0, 0, 5))
    for max_n in (0, _lib.PTTA_SCORE_MAX_N + 1):
        with pytest.raises(ValueError):
            score.RunScore(0.0, 100.0, max_n=max_n)
    rs = score.RunScore(0.0, 100.0)
    with pytest.raises(ValueError):          # no CPU fallback
        rs.update(torch.zeros(1, 1, 5, 7), torch.zeros(1, 1, 5, 7))
    with pytest.raises(ValueError):
        rs.update(torch.zeros(1, 1, 5, 7), torch.zeros(1, 1, 5, 8))


C_TYPES = {'const float*': ctypes.c_void_p, 'float*': ctypes.c_void_p, 'void*': ctypes.c_void_p, 'int32_t*': ctypes.c_void_p,
           'int': ctypes.c_int, 'float': ctypes.c_float}


def test_binding_against_the_header():
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    assert int(re.search(r'#define PTTA_ABI_VERSION (\d+)', header).group(1)) == 2 == _lib.PTTA_ABI_VERSION
    body = re.search(r'typedef struct ptta_score_args \{(.*?)\} ptta_score_args;', header, re.S).group(1)
    fields = []
    for line in re.sub(r'/\*.*?\*/', '', body, flags=re.S).split(';'):
        line = line.strip()
        if line:
            ctype, names = re.match(r'((?:const )?\w+\*?)\s+(.*)', line).groups()
            fields += [(n.strip(), C_TYPES[ctype]) for n in names.split(',')]
    assert fields == list(_lib.ScoreArgs._fields_)
    assert ctypes.sizeof(_lib.ScoreArgs) == 88
    rules = re.search(r'enum \{ PTTA_SCORE_RULE_ADAPT = (\d+), PTTA_SCORE_RULE_VALIDATE = (\d+) \};', header).groups()
    assert (int(rules[0]), int(rules[1])) == (_lib.PTTA_SCORE_RULE_ADAPT, _lib.PTTA_SCORE_RULE_VALIDATE) == (score.RULES['adapt'], score.RULES['validate'])
    assert int(re.search(r'#define PTTA_SCORE_MAX_N (\d+)', header).group(1)) == _lib.PTTA_SCORE_MAX_N
    sig = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    P = ctypes.c_void_p
    assert sig['ptta_score_state_bytes'] == (ctypes.c_int64, [ctypes.c_int])
    assert sig['ptta_score_reset'] == (ctypes.c_int, [P, ctypes.c_int64, P])
    assert sig['ptta_score_accumulate'] == (ctypes.c_int, [ctypes.POINTER(_lib.ScoreArgs), P])
    assert sig['ptta_score_result'] == (ctypes.c_int, [P, ctypes.c_int64, P, P])
    # declared behind ptta_summary_compose and in front of ptta_rotate, in the header and in the table
    order = [header.index('int ptta_summary_compose('), header.index('int64_t ptta_score_state_bytes('), header.index('int ptta_score_reset('),
             header.index('int ptta_score_accumulate('), header.index('int ptta_score_result('), header.index('int ptta_rotate(')]
    assert order == sorted(order)
    names = [name for name, _, _ in _lib.SIGNATURES]
    at = names.index('ptta_summary_compose')
    assert names[at + 1:at + 6] == ['ptta_score_state_bytes', 'ptta_score_reset', 'ptta_score_accumulate', 'ptta_score_result', 'ptta_rotate']


def test_library_refuses_on_the_host_with_a_reason():
    """The refusals that need no device: they return before any HIP call."""
    assert os.path.exists(_lib.LIB_PATH), 'libptta_hip.so not built (run __graft_entry__.build())'
    lib = _lib.load()
    assert lib.ptta_score_state_bytes(1) == 128 + 48 + 64 * 48 and lib.ptta_score_state_bytes(16) == 128 + 16 * (48 + 64 * 48)
    assert lib.ptta_score_state_bytes(16) % 16 == 0
    for max_n in (0, -1, _lib.PTTA_SCORE_MAX_N + 1):
        assert lib.ptta_score_state_bytes(max_n) == -22 and b'max_n' in lib.ptta_last_error(None)
    assert lib.ptta_score_reset(None, 1 << 20, None) == -22 and b'NULL' in lib.ptta_last_error(None)
    assert lib.ptta_score_reset(ctypes.c_void_p(0x1008), 1 << 20, None) == -22 and b'aligned' in lib.ptta_last_error(None)
    assert lib.ptta_score_reset(ctypes.c_void_p(0x1000), lib.ptta_score_state_bytes(1) - 1, None) == -22 and b'state_bytes' in lib.ptta_last_error(None)
    assert lib.ptta_score_accumulate(None, None) == -22 and b'NULL args' in lib.ptta_last_error(None)
    a = _lib.ScoreArgs(n=1, height=5, width=7, win_height=5, win_width=7, min_evaluate_depth=0.0, max_evaluate_depth=100.0)
    assert lib.ptta_score_accumulate(ctypes.byref(a), None) == -22 and b'NULL depth' in lib.ptta_last_error(None)
    assert lib.ptta_score_result(None, 0, None, None) == -22 and b'NULL' in lib.ptta_last_error(None)


def test_case_table_is_what_the_gpu_test_says():
    by = {c['name']: c for c in C.CASES}
    assert len(by) == len(C.CASES)
    for c in C.CASES:
        h, w = c['size']
        wy, wx, wh, ww = C.window_of(c)
        assert 0 <= wy and 0 <= wx and wh >= 1 and ww >= 1 and wy + wh <= h and wx + ww <= w
        assert C.takes_vec_path(c) == (c['path'] == 'vec'), c['name']
    assert by['full_odd_width']['size'] == (5, 7) and by['full_odd_width']['n'] == 1 and by['full_odd_width']['window'] is None
    assert (by['ragged_window']['n'], by['ragged_window']['size'], by['ragged_window']['window']) == (3, (9, 13), (2, 3, 6, 7))
    aw = by['aligned_window']
    assert (aw['n'], aw['size'], aw['window'][1], aw['window'][3]) == (2, (16, 32), 4, 24) and aw['window'][3] < aw['size'][1]
    assert by['several_blocks']['size'] == (72, 128) and by['several_blocks']['n'] == 2
    assert C.blocks_per_sample(by['several_blocks']) == 3 and C.blocks_per_sample(by['several_blocks_scalar']) == 3
    assert C.blocks_per_sample(by['block_cap']) == C.MAX_BLOCKS and 264 * 1024 // 4 > C.MAX_BLOCKS * C.UNITS_PER_BLOCK
    assert all(C.blocks_per_sample(c) == 1 for c in C.CASES if c['name'] not in ('several_blocks', 'several_blocks_scalar', 'block_cap'))
    assert by['one_row']['window'][2] == 1 and by['one_column']['window'][3] == 1
    for name in ('window_at_end', 'window_at_end_ragged'):          # the window's last pixel is the last pixel of the last sample
        (h, w), (wy, wx, wh, ww) = by[name]['size'], by[name]['window']
        assert (wy + wh, wx + ww) == (h, w) and (wy, wx) != (0, 0)
    # but for its base pointer the 'offset' case would take the 16-byte path
    ub = by['unaligned_base']
    assert ub['kind'] == 'offset' and C.takes_vec_path(dict(ub, kind='plain')) and not C.takes_vec_path(ub)
    assert by['empty_sample']['n'] == 3 and by['empty_sample']['kind'] == 'empty_sample' and by['empty_batch']['kind'] == 'empty_batch'
    assert {by['boundary_values']['path'], by['boundary_values_aligned']['path']} == {'scalar', 'vec'}
    # outside a window the frames hold NaN output over valid ground truth
    out, gt = C.case_frames(by['ragged_window'])
    assert np.isnan(out[:, :, 0, 0]).all() and (gt[:, :, 0, 0] == 10.0).all() and np.isfinite(out[:, :, 2:8, 3:10]).all()
    assert C.RUN['batches'] == (4, 4, 1) and C.RUN['size'] == (9, 13) and C.RUN['n_sample'] == 9
