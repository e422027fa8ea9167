"""ptta_score_accumulate / proxytta.score.RunScore on the GPU against the numpy restatement of tests/score_cases.py (itself held to the
REAL eval_utils' results by tests/test_score_cpu.py).

Bounds, none of them taken from what the kernel gives:
  * masked counts: equal;
  * every fp64 sum: |got - exact| <= pixels x 2^-52 x exact.  All terms are non-negative and bit-equal to the restatement's, so this is
    the standard (n - 1) u bound of a sum in ANY order (u = 2^-53), with the factor 2 left for nothing;
  * fp32 outputs: within 1 ulp of the restatement's fp64 metric rounded to fp32 (the fp64 metrics differ in their last bits at most, which
    can move a rounding to the neighbour);
  * the run: the same relative bound with the run's pixels (each batch metric is a quotient and a square root of such sums).
Every output, and the state, is a view inside a sentinel-filled buffer (the `Guarded` pattern of tests/test_gpu_ingest.py); margins are
checked after every call and the inputs compared with what was uploaded."""
import ctypes

import numpy as np
import pytest
import torch

from proxytta import _lib, synth
from proxytta.score import RULES, RunScore
from tests import score_cases as C

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0          # no metric is negative
PAD = 64                     # elements on each side of a view: a view keeps the buffer's 16-byte alignment
U52 = 2.0 ** -52
METRICS = ('mae', 'rmse', 'imae', 'irmse')
ONE = 'meta_selfsup_seq_1layer_ema'


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def upload(a, offset=False):
    """numpy -> device; offset: the tensor starts one float past a 16-byte boundary"""
    if not offset:
        t = torch.from_numpy(a).cuda()
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.zeros(a.size + 4, dtype=torch.float32, device='cuda')
    t = buf[1:1 + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


class Guarded:
    """the state and the three optional outputs as views inside sentinel-filled buffers"""

    def __init__(self, n, max_n=None):
        lib = _lib.load()
        self.n, self.max_n = n, n if max_n is None else max_n
        self.state_bytes = lib.ptta_score_state_bytes(self.max_n)
        assert self.state_bytes > 0 and self.state_bytes % 8 == 0
        self.buf = {'state': torch.full((PAD + self.state_bytes // 8 + PAD,), SENTINEL, dtype=torch.float64, device='cuda'),
                    'batch': torch.full((PAD + 4 + PAD,), SENTINEL, dtype=torch.float32, device='cuda'),
                    'samples': torch.full((PAD + 4 * n + PAD,), SENTINEL, dtype=torch.float32, device='cuda'),
                    'counts': torch.full((PAD + n + PAD,), -12345, dtype=torch.int32, device='cuda')}
        self.size = {'state': self.state_bytes // 8, 'batch': 4, 'samples': 4 * n, 'counts': n}
        self.view = {k: b[PAD:PAD + self.size[k]] for k, b in self.buf.items()}
        assert all(v.data_ptr() % 16 == 0 for v in self.view.values())

    def reset(self):
        rc = _lib.load().ptta_score_reset(_lib.ptr(self.view['state']), self.state_bytes, stream())
        assert rc == 0

    def margins_intact(self):
        torch.cuda.synchronize()
        return all(bool((b[:PAD] == SENTINEL).all()) and bool((b[PAD + self.size[k]:] == SENTINEL).all()) for k, b in self.buf.items())

    def outputs_untouched(self):
        torch.cuda.synchronize()
        return all(bool((self.buf[k] == SENTINEL).all()) for k in ('batch', 'samples', 'counts'))

    def args(self, o, g, window, which, **over):
        n, _, h, w = o.shape
        wy, wx, wh, ww = (0, 0, h, w) if window is None else window
        kw = dict(depth=_lib.ptr(o), ground_truth=_lib.ptr(g), n=n, height=h, width=w, win_y=wy, win_x=wx, win_height=wh, win_width=ww,
                  min_evaluate_depth=C.LO, max_evaluate_depth=C.HI, rule=RULES[which], state=_lib.ptr(self.view['state']),
                  batch_out=_lib.ptr(self.view['batch']), sample_out=_lib.ptr(self.view['samples']), sample_count_out=_lib.ptr(self.view['counts']))
        kw.update(over)
        return _lib.ScoreArgs(**kw)

    def header(self):
        """(sum[4], frames, batches, empty_batches, pixels, last[5], sample[n][5]) of the state"""
        st = self.view['state'].cpu()
        ints = st[4:8].view(torch.int64).tolist()
        return st[:4].numpy(), ints, st[8:13].numpy(), st[16:16 + 6 * self.n].view(self.n, 6)[:, :5].numpy()


def sums_within(got, exact, pixels):
    got, exact = np.asarray(got, np.float64), np.asarray(exact, np.float64)
    return bool(np.all(np.abs(got - exact) <= pixels * U52 * np.abs(exact)))


def within_one_ulp(got32, exact64):
    got32, want = np.asarray(got32, np.float32).ravel(), np.asarray(exact64, np.float64).astype(np.float32).ravel()
    for a, b in zip(got32, want):
        if np.isnan(b):
            if not np.isnan(a):
                return False
        elif not (np.nextafter(b, np.float32(-np.inf)) <= a <= np.nextafter(b, np.float32(np.inf))):
            return False
    return True


@pytest.fixture(scope='module')
def case_data():
    """the frames and both restatements of every case, computed once and left unchanged"""
    data = {}
    for c in C.CASES:
        out, gt = C.case_frames(c)
        data[c['name']] = (out, gt, {rule: C.restate_batch(out, gt, c['window'], rule=rule) for rule in (C.ADAPT, C.VALIDATE)})
    return data


@pytest.mark.parametrize('rule', [C.ADAPT, C.VALIDATE])
@pytest.mark.parametrize('c', C.CASES, ids=[c['name'] for c in C.CASES])
def test_case_table(case_data, c, rule):
    lib = _lib.load()
    out, gt, refs = case_data[c['name']]
    ref, n = refs[rule], c['n']
    o, g = upload(out, c['kind'] == 'offset'), upload(gt, c['kind'] == 'offset')
    gd = Guarded(n)
    gd.reset()
    assert gd.margins_intact() and gd.outputs_untouched()
    a = gd.args(o, g, c['window'], rule)
    assert lib.ptta_score_accumulate(ctypes.byref(a), stream()) == 0
    assert gd.margins_intact()
    assert np.array_equal(o.cpu().numpy(), out, equal_nan=True) and np.array_equal(g.cpu().numpy(), gt)
    sums, (frames, batches, empty, pixels), last, sample = gd.header()
    # counts
    assert gd.view['counts'].cpu().tolist() == ref['sample_count'].tolist()
    assert sample[:, 0].tolist() == ref['sample_count'].tolist() and last[0] == ref['count'] == pixels
    assert (frames, batches, empty) == (n, 1, int(ref['count'] == 0))
    # fp64 sums
    print(c['name'], rule, 'pooled sums', last[1:], 'exact', ref['sums'])
    assert sums_within(last[1:], ref['sums'], ref['count'])
    for s in range(n):
        assert sums_within(sample[s, 1:], ref['sample_sums'][s], int(ref['sample_count'][s])), s
    # fp32 outputs and the run's sums after one batch
    assert within_one_ulp(gd.view['batch'].cpu().numpy(), ref['metrics'])
    assert within_one_ulp(gd.view['samples'].cpu().numpy(), ref['sample_metrics'])
    if ref['count']:
        assert sums_within(sums, ref['metrics'] * n, ref['count'])
    else:
        assert np.isnan(sums).all()
    if c['kind'] == 'empty_sample':
        assert np.isnan(gd.view['samples'].cpu().numpy().reshape(n, 4)[1]).all() and gd.view['counts'].cpu().tolist()[1] == 0
        assert np.isfinite(gd.view['batch'].cpu().numpy()).all()
    # the optional outputs are optional: the same state without them
    gd2 = Guarded(n)
    gd2.reset()
    a2 = gd2.args(o, g, c['window'], rule, batch_out=None, sample_out=None, sample_count_out=None)
    assert lib.ptta_score_accumulate(ctypes.byref(a2), stream()) == 0
    assert gd2.margins_intact() and gd2.outputs_untouched()
    n_head = 16 + 6 * n
    assert torch.equal(gd2.view['state'][:n_head].view(torch.int64), gd.view['state'][:n_head].view(torch.int64))


def test_boundary_pixels_separate_the_two_rules(case_data):
    for name in ('boundary_values', 'boundary_values_aligned'):
        c = C.case(name)
        out, gt, _ = case_data[name]
        o, g = upload(out), upload(gt)
        counts = {}
        for rule in (C.ADAPT, C.VALIDATE):
            rs = RunScore(C.LO, C.HI, rule=rule, window=c['window'], max_n=c['n'])
            rs.update(o, g)
            counts[rule] = rs.result()['pixels']
        assert counts[C.ADAPT] - counts[C.VALIDATE] == sum(C.BOUNDARY_PIXELS)


def run_once(batches, **kw):
    rs = RunScore(C.LO, C.HI, max_n=4, **kw)
    per_sample = [rs.update(o, g, want_samples=True) for o, g in batches]
    return rs, per_sample


def test_run_of_4_4_1():
    host = C.run_frames()
    batches = [(upload(o), upload(g)) for o, g in host]
    for rule in (C.ADAPT, C.VALIDATE):
        rs, _ = run_once(batches, rule=rule)
        for ns in (C.RUN['n_sample'], None):
            got, ref = rs.result(ns), C.restate_run(host, rule=rule, n_sample=ns)
            print(rule, ns, got, ref)
            assert [got[k] for k in ('frames', 'batches', 'empty_batches', 'pixels')] == [ref[k] for k in ('frames', 'batches', 'empty_batches', 'pixels')]
            assert got['frames'] == 9 and got['batches'] == 3
            assert sums_within([got[m] for m in METRICS], [ref[m] for m in METRICS], ref['pixels'])
        # a dataset larger than what the run saw: the sums are divided by n_sample, not by the frames
        assert sums_within([rs.result(12)[m] * 12 for m in METRICS], [rs.result()[m] * 9 for m in METRICS], 4)
        assert sums_within(rs.sums().cpu().numpy(), [rs.result()[m] * 9 for m in METRICS], 2)
    # reset in the middle starts over; two identical runs are bit-equal
    first, samples_first = run_once(batches)
    second = RunScore(C.LO, C.HI, max_n=4)
    second.update(*batches[2])
    second.update(*batches[0])
    second.reset()
    cleared = second.result()
    assert [cleared[k] for k in ('frames', 'batches', 'empty_batches', 'pixels')] == [0, 0, 0, 0] and second.sums().tolist() == [0.0] * 4
    samples_second = [second.update(o, g, want_samples=True) for o, g in batches]
    assert first.result() == second.result() and first.result(9) == second.result(9)
    assert torch.equal(first.sums().view(torch.int64), second.sums().view(torch.int64))
    for a, b in zip(samples_first, samples_second):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_an_empty_batch_stays_in_the_run(case_data):
    plain, empty = case_data['full_odd_width'], case_data['empty_batch']
    rs = RunScore(C.LO, C.HI, max_n=2)
    b0 = rs.update(upload(plain[0]), upload(plain[1]))
    b1, s1, c1 = rs.update(upload(empty[0]), upload(empty[1]), want_samples=True)
    b2 = rs.update(upload(plain[0]), upload(plain[1]))
    r = rs.result()
    assert torch.isfinite(b0).all() and torch.isnan(b1).all() and torch.isnan(s1).all() and c1.tolist() == [0, 0] and torch.equal(b0, b2)
    assert (r['frames'], r['batches'], r['empty_batches'], r['pixels']) == (4, 3, 1, 2 * plain[2][C.ADAPT]['count'])
    assert all(np.isnan(r[m]) for m in METRICS) and torch.isnan(rs.sums()).all()


def test_refusals(case_data):
    """Every refusal returns -22 with a reason before anything is launched: state and outputs keep their bytes."""
    lib = _lib.load()
    out, gt, _ = case_data['ragged_window']
    o, g = upload(out), upload(gt)
    n, _, h, w = out.shape
    win = C.case('ragged_window')['window']
    gd = Guarded(n)
    gd.reset()
    first = gd.args(o, g, win, C.ADAPT, batch_out=None, sample_out=None, sample_count_out=None)
    assert lib.ptta_score_accumulate(ctypes.byref(first), stream()) == 0          # a state with something in it
    torch.cuda.synchronize()
    before = gd.buf['state'].clone()
    small = Guarded(n, max_n=1)
    small.reset()
    state = gd.view['state']
    # an address no state was ever reset at: inside this buffer, 16-byte aligned, and unlike every allocation and every view here not
    # a multiple of 512 (the table of reset states is keyed by address, and a freed state's address may come back from the allocator)
    never = ctypes.c_void_p(state.data_ptr() + 16)
    bad = [dict(depth=None), dict(ground_truth=None), dict(state=None), dict(n=0), dict(n=-1), dict(height=0), dict(width=0),
           dict(win_height=0), dict(win_width=0), dict(win_height=-2), dict(win_y=-1), dict(win_x=-1), dict(win_y=h - win[2] + 1),
           dict(win_x=w - win[3] + 1), dict(win_height=h + 1, win_y=0), dict(win_y=2 ** 31 - 1), dict(win_x=2 ** 31 - 1),
           dict(min_evaluate_depth=C.HI, max_evaluate_depth=C.LO), dict(min_evaluate_depth=float('nan')), dict(max_evaluate_depth=float('inf')),
           dict(min_evaluate_depth=float('-inf')), dict(rule=2), dict(rule=-1),
           dict(state=ctypes.c_void_p(state.data_ptr() + 8)),                    # not 16-byte aligned
           dict(state=_lib.ptr(small.view['state'])),                             # sized for max_n = 1, n = 3
           dict(state=never)]                                                     # never handed to ptta_score_reset
    for over in bad:
        a = gd.args(o, g, win, C.ADAPT, **over)
        assert lib.ptta_score_accumulate(ctypes.byref(a), stream()) == -22, over
        assert len(lib.ptta_last_error(None)) > 10, over
    assert lib.ptta_score_accumulate(None, stream()) == -22
    # reset and result
    assert lib.ptta_score_reset(None, gd.state_bytes, stream()) == -22
    assert lib.ptta_score_reset(ctypes.c_void_p(state.data_ptr() + 8), gd.state_bytes, stream()) == -22
    assert lib.ptta_score_reset(_lib.ptr(state), lib.ptta_score_state_bytes(1) - 16, stream()) == -22 and b'state_bytes' in lib.ptta_last_error(None)
    out8 = torch.full((8,), SENTINEL, dtype=torch.float64, device='cuda')
    assert lib.ptta_score_result(None, 0, _lib.ptr(out8), stream()) == -22 and lib.ptta_score_result(_lib.ptr(state), 0, None, stream()) == -22
    assert lib.ptta_score_result(never, 0, _lib.ptr(out8), stream()) == -22
    torch.cuda.synchronize()
    assert torch.equal(gd.buf['state'].view(torch.int64), before.view(torch.int64)) and gd.outputs_untouched() and gd.margins_intact()
    assert bool((out8 == SENTINEL).all()) and small.margins_intact()
    # the refused state still works
    out8v = torch.full((PAD + 8 + PAD,), SENTINEL, dtype=torch.float64, device='cuda')
    assert lib.ptta_score_result(_lib.ptr(state), 0, _lib.ptr(out8v[PAD:PAD + 8]), stream()) == 0
    torch.cuda.synchronize()
    assert bool((out8v[:PAD] == SENTINEL).all()) and bool((out8v[PAD + 8:] == SENTINEL).all()) and out8v[PAD + 4:PAD + 8].tolist()[:2] == [float(n), 1.0]
    with pytest.raises(RuntimeError, match='max_n'):
        RunScore(C.LO, C.HI, max_n=2).update(o, g)


def test_window_on_the_full_map_equals_the_cropped_copy():
    out, gt = C.frames(2024, 2, 24, 40)
    o, g = upload(out), upload(gt)
    for win in ((5, 6, 17, 30), (4, 8, 16, 24)):          # the one-pixel path and the 16-byte path (rows shorter than the map's)
        wy, wx, wh, ww = win
        ref = C.restate_batch(out, gt, win)
        full, crop, strided = (RunScore(C.LO, C.HI, window=win), RunScore(C.LO, C.HI), RunScore(C.LO, C.HI))
        full.update(o, g)
        oc, gc = o[..., wy:wy + wh, wx:wx + ww], g[..., wy:wy + wh, wx:wx + ww]
        crop.update(oc.contiguous(), gc.contiguous())
        strided.update(oc, gc)                            # a non-contiguous input is copied by the façade
        for rs in (full, crop, strided):
            pooled, sample = (t.cpu().numpy() for t in rs.last_sums())
            assert pooled[0] == ref['count'] and sample[:, 0].tolist() == ref['sample_count'].tolist()
            assert sums_within(pooled[1:], ref['sums'], ref['count'])
        assert torch.equal(crop.sums().view(torch.int64), strided.sums().view(torch.int64))
        assert full.result()['pixels'] == crop.result()['pixels'] == ref['count']


def make_model():
    from proxytta.model import ExternalModel_Adapt
    model = ExternalModel_Adapt('msg_chn', 0.0, 80.0, max_input_depth=80.0, device=torch.device('cuda'))
    model._prepare_head(ONE)
    model.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.formula_state_dict(ONE).items()})
    opt = torch.optim.Adam(model.adapt_parameters(mode='meta'), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    model.model.set_hparams(w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1)
    model.model.bind_optimizer(opt)
    return model, opt


def test_adapt_scores_behind_its_eval_forward():
    """adapt(..., ground_truth, score) on a 32 x 48 MSG_CHN engine: the same depth and loss_info as without the two arguments, and the
    RunScore holds what an update by hand with the returned depth gives."""
    image, sparse = [torch.from_numpy(x).cuda() for x in synth.synthetic_frame(7, 32, 48, 1)]
    gt = upload(C.frames(77, 1, 32, 48)[1])
    plain, _ = make_model()
    scored, _ = make_model()
    rs, by_hand = RunScore(0.0, 80.0), RunScore(0.0, 80.0)
    for _ in range(2):
        d0, i0 = plain.adapt(image, sparse, inner_iter=1)
        d1, i1 = scored.adapt(image, sparse, inner_iter=1, ground_truth=gt, score=rs)
        by_hand.update(d1, gt)
        assert torch.equal(d0, d1) and torch.equal(i0, i1)
    assert rs.result() == by_hand.result() and rs.result()['frames'] == 2 and rs.result()['pixels'] > 0
    assert torch.equal(rs.sums().view(torch.int64), by_hand.sums().view(torch.int64)) and torch.isfinite(rs.sums()).all()
    for kw in (dict(ground_truth=gt), dict(score=rs)):
        with pytest.raises(ValueError):
            scored.adapt(image, sparse, **kw)
