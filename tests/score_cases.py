"""The cases of the run score (include/ptta.h ptta_score_accumulate, proxytta.score.RunScore), a seeded frame generator, and the numpy
restatement of the reference's scoring tails (src/tta_main.py:755-809 adaptation loop, :975-1030 validate()).

Per element the restatement is the reference's own fp32 arithmetic (every product, sum and quotient one float32 operation on float32
arrays); the sums are exact (math.fsum over the float64 values), so they are the value every summation order is measured against.
tests/golden/make_golden_run_score.py records what the REAL eval_utils gives on the same frames; tests/test_score_cpu.py holds the
restatement to that record, tests/test_gpu_score.py holds the library to the restatement."""
import math
import zlib

import numpy as np
import torch

F = np.float32
ADAPT, VALIDATE = 'adapt', 'validate'
LO, HI = 2.0, 50.0           # min / max_evaluate_depth of every case: exact in fp32, so "equal to a bound" means the same in fp32 and fp64

# name, n, (H, W), window (y, x, h, w) or None = the whole frame, kind of frame, the path the kernel takes
#   kinds: 'plain'; 'empty_sample': sample 1 has no valid ground truth; 'empty_batch': no sample has; 'boundary': ground-truth pixels
#   equal to LO and to HI; 'offset': the maps are handed over one float past a 16-byte boundary
CASES = [
    dict(name='full_odd_width', n=1, size=(5, 7), window=None, kind='plain', path='scalar'),
    dict(name='ragged_window', n=3, size=(9, 13), window=(2, 3, 6, 7), kind='plain', path='scalar'),
    dict(name='aligned_window', n=2, size=(16, 32), window=(3, 4, 11, 24), kind='plain', path='vec'),
    dict(name='several_blocks', n=2, size=(72, 128), window=None, kind='plain', path='vec'),
    dict(name='several_blocks_scalar', n=1, size=(37, 61), window=None, kind='plain', path='scalar'),
    dict(name='block_cap', n=1, size=(264, 1024), window=None, kind='plain', path='vec'),
    dict(name='one_row', n=2, size=(6, 16), window=(4, 4, 1, 8), kind='plain', path='vec'),
    dict(name='one_column', n=2, size=(9, 13), window=(1, 5, 7, 1), kind='plain', path='scalar'),
    dict(name='window_at_end', n=2, size=(8, 12), window=(5, 4, 3, 8), kind='plain', path='vec'),
    dict(name='window_at_end_ragged', n=3, size=(7, 11), window=(4, 6, 3, 5), kind='plain', path='scalar'),
    dict(name='unaligned_base', n=2, size=(8, 16), window=(1, 4, 6, 8), kind='offset', path='scalar'),
    dict(name='empty_sample', n=3, size=(6, 8), window=None, kind='empty_sample', path='vec'),
    dict(name='empty_batch', n=2, size=(5, 7), window=None, kind='empty_batch', path='scalar'),
    dict(name='boundary_values', n=2, size=(9, 13), window=(1, 2, 7, 9), kind='boundary', path='scalar'),
    dict(name='boundary_values_aligned', n=1, size=(8, 16), window=None, kind='boundary', path='vec'),
]
BOUNDARY_PIXELS = (3, 4)     # pixels of a 'boundary' frame's window set to LO, and to HI
# the run: batches of N = 4, 4, 1 (a short last batch) at 9 x 13, scored with n_sample = 9 and with the default (the frames seen)
RUN = dict(name='run_4_4_1', batches=(4, 4, 1), size=(9, 13), window=None, n_sample=9)
# block geometry of csrc/score.hip: a workgroup is added per 1024 units (pixels, or groups of 4 pixels on the 16-byte path), 64 at most
UNITS_PER_BLOCK, MAX_BLOCKS = 1024, 64


def case(name):
    return [c for c in CASES if c['name'] == name][0]


def window_of(c):
    h, w = c['size']
    return (0, 0, h, w) if c['window'] is None else c['window']


def takes_vec_path(c):
    """16-byte loads: width, win_x and win_width multiples of 4 on 16-byte-aligned bases (torch allocations are; 'offset' breaks it)"""
    _, wx, _, ww = window_of(c)
    return c['size'][1] % 4 == 0 and wx % 4 == 0 and ww % 4 == 0 and c['kind'] != 'offset'


def blocks_per_sample(c):
    _, _, wh, ww = window_of(c)
    units = wh * (ww // 4 if takes_vec_path(c) else ww)
    return min(MAX_BLOCKS, -(-units // UNITS_PER_BLOCK))


def frames(seed, n, h, w, window=None, kind='plain'):
    """(output_depth, ground_truth): N x 1 x H x W float32 from the CPU torch.Generator.  Ground truth: 30 % holes (0), the rest in
    [0.5, 60) so that some lie below LO and some above HI; output: the ground truth within a few per cent, positive everywhere (where the
    ground truth is a hole too).  Outside a window the output is NaN over VALID ground truth: one pixel read there ruins every sum."""
    g = torch.Generator(device='cpu')
    g.manual_seed(int(seed))
    shape = (n, 1, h, w)
    gt = (0.5 + 59.5 * torch.rand(shape, generator=g, dtype=torch.float32))
    hole = torch.rand(shape, generator=g, dtype=torch.float32) < 0.3
    noise = torch.randn(shape, generator=g, dtype=torch.float32)
    out = (gt * (1.0 + 0.05 * noise) + 0.01).clamp_min(0.05)
    gt = torch.where(hole, torch.zeros_like(gt), gt)
    out, gt = out.numpy().copy(), gt.numpy().copy()
    wy, wx, wh, ww = (0, 0, h, w) if window is None else window
    if kind == 'empty_sample':
        gt[1] = 0.0
    elif kind == 'empty_batch':
        gt[:] = 0.0
    elif kind == 'boundary':
        nlo, nhi = BOUNDARY_PIXELS
        flat = [(y, x) for y in range(wy, wy + wh) for x in range(wx, wx + ww)]
        pick = torch.randperm(len(flat), generator=g)[:nlo + nhi].tolist()
        for k, p in enumerate(pick):
            y, x = flat[p]
            gt[k % n, 0, y, x] = F(LO) if k < nlo else F(HI)
    if window is not None:
        inside = np.zeros((h, w), bool)
        inside[wy:wy + wh, wx:wx + ww] = True
        out[:, :, ~inside] = np.nan
        gt[:, :, ~inside] = F(10.0)
    return out, gt


def case_frames(c):
    h, w = c['size']
    return frames(zlib.crc32(c['name'].encode()), c['n'], h, w, c['window'], c['kind'])


def run_frames():
    h, w = RUN['size']
    return [frames(zlib.crc32(('%s_%d' % (RUN['name'], k)).encode()), n, h, w, RUN['window']) for k, n in enumerate(RUN['batches'])]


def crc(out, gt):
    return zlib.crc32(np.ascontiguousarray(gt).tobytes(), zlib.crc32(np.ascontiguousarray(out).tobytes()))


def mask_of(gt, lo, hi, rule):
    lo, hi = F(lo), F(hi)
    if rule == ADAPT:                    # :776-781: ones where gt > 0, then zeroed where gt < min and where gt > max
        return (gt > 0) & ~(gt < lo) & ~(gt > hi)
    return (gt > 0) & (gt > lo) & (gt < hi)          # :1008-1015


def elements(out, gt):
    """|d|, d^2, |i|, i^2 per pixel in fp32: d = 1000 gt - 1000 out, i = 1 / (0.001 gt + 1e-9) - 1 / (0.001 out + 1e-9)"""
    with np.errstate(all='ignore'):
        d = F(1000.0) * gt - F(1000.0) * out
        i = F(1.0) / (F(0.001) * gt + F(1e-9)) - F(1.0) / (F(0.001) * out + F(1e-9))
        return np.abs(d), d * d, np.abs(i), i * i


def metrics_of(count, sums):
    """MAE, RMSE, iMAE, iRMSE in fp64 from count and the four sums; NaN for an empty mask (0 / 0)"""
    if count == 0:
        return [float('nan')] * 4
    return [sums[0] / count, math.sqrt(sums[1] / count), sums[2] / count, math.sqrt(sums[3] / count)]


def restate_batch(out, gt, window=None, lo=LO, hi=HI, rule=ADAPT):
    """One batch: per-sample and pooled masked counts, exact fp64 sums of the fp32 elements, and the metrics of each"""
    n, _, h, w = out.shape
    wy, wx, wh, ww = (0, 0, h, w) if window is None else window
    o, g = out[:, 0, wy:wy + wh, wx:wx + ww], gt[:, 0, wy:wy + wh, wx:wx + ww]
    assert o.dtype == F and g.dtype == F
    m = mask_of(g, lo, hi, rule)
    el = [e.astype(np.float64) for e in elements(o, g)]
    assert all(e.dtype == np.float64 for e in el)
    sample_count = np.array([int(m[s].sum()) for s in range(n)], dtype=np.int64)
    sample_sums = np.array([[math.fsum(e[s][m[s]].tolist()) for e in el] for s in range(n)], dtype=np.float64)
    count = int(m.sum())
    sums = np.array([math.fsum(e[m].tolist()) for e in el], dtype=np.float64)
    return dict(count=count, sums=sums, metrics=np.array(metrics_of(count, sums)), sample_count=sample_count, sample_sums=sample_sums,
                sample_metrics=np.array([metrics_of(int(c), s) for c, s in zip(sample_count, sample_sums)]).reshape(n, 4))


def restate_run(batches, window=None, lo=LO, hi=HI, rule=ADAPT, n_sample=None):
    """The run bookkeeping (:795-809): metric x batch size added over the batches, divided by n_sample (default: the frames seen)"""
    total, frames_seen, pixels, empty = [0.0] * 4, 0, 0, 0
    for out, gt in batches:
        r = restate_batch(out, gt, window, lo, hi, rule)
        n = out.shape[0]
        total = [t + float(m) * n for t, m in zip(total, r['metrics'])]
        frames_seen, pixels, empty = frames_seen + n, pixels + r['count'], empty + (r['count'] == 0)
    div = n_sample if n_sample else frames_seen
    res = dict(zip(('mae', 'rmse', 'imae', 'irmse'), (t / div if div else float('nan') for t in total)))
    res.update(frames=frames_seen, batches=len(batches), empty_batches=int(empty), pixels=pixels)
    return res
