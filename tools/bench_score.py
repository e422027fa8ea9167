"""Scoring a run on the device (include/ptta.h ptta_score_accumulate, proxytta.score.RunScore; profiles/run_score.txt) beside the host
tail of the reference's adaptation loop and beside proxytta.model.eval_metrics, on one box.  Nothing is asserted about speed: the tool
writes down what it measures.

Workload: output depth and ground truth resident in HBM, N = 1 / 4 / 16, scored
  full    the whole 352 x 1216 frame (the adaptation loop: the inputs were cropped in front of the forward);
  window  the 'vkitti' window (135, 13, 240, 1216) of a 375 x 1242 frame (validate(): the output is cropped): ragged, the one-pixel path.

  host      wall-clock ms per frame of what the reference's tail does (src/tta_main.py:755-798): slice, both maps .to('cpu'), the float
            mask, the masked pixels, four torch reductions, `metric * batch_size / 1000` added to four running sums
            (`--host-repeats` runs of 4 frames).
  metrics   wall-clock ms per frame of eval_metrics on .contiguous() slices with the four floats read back per frame (what a caller of
            ptta_eval_metrics has to do to keep the run's sums).
  update    wall-clock ms per frame of RunScore.update, nothing read back: `--frames` calls, then one synchronisation; and the same
            with a synchronisation after every call (the latency of one scored frame).
  launches  device events around bursts of bare ptta_score_accumulate calls (its two launches), beside the bytes they read:
            2 maps x N x window pixels x 4.

    python tools/bench_score.py [--out FILE] [--repeats 20] [--warmup 3] [--frames 20] [--host-repeats 5]
Fails without a GPU.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tta-depth-completion_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')        # as bench.py: before the HIP runtime exists

LO, HI = 0.0, 100.0


def host_tail(torch, out, gt, window, sums):
    """One frame of a reference-style host tail; `sums` are the four running sums."""
    wy, wx, wh, ww = window
    o = torch.squeeze(out[..., wy:wy + wh, wx:wx + ww].clone().detach()).to(torch.device('cpu'))
    g = torch.squeeze(gt[..., wy:wy + wh, wx:wx + ww]).to(torch.device('cpu'))
    mask = torch.where(g > 0, torch.ones_like(g), torch.zeros_like(g))
    mask[g < LO] = 0.0
    mask[g > HI] = 0.0
    at = mask.nonzero(as_tuple=True)
    o, g = o[at], g[at]
    n = out.shape[0]
    d = 1000.0 * g - 1000.0 * o
    i = 1.0 / (0.001 * g + 1e-9) - 1.0 / (0.001 * o + 1e-9)
    for k, v in enumerate((torch.mean(torch.abs(d)), torch.sqrt(torch.mean(d ** 2)), torch.mean(torch.abs(i)), torch.sqrt(torch.mean(i ** 2)))):
        sums[k] = sums[k] + v * n / 1000
    return sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the printed text to this file')
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--host-repeats', type=int, default=5, help='runs of the host tail (4 frames each, after one warm-up run)')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_score.py measures on a HIP device and there is none')
    from proxytta import _lib
    from proxytta.model import eval_metrics
    from proxytta.score import RunScore, eval_window
    from tests import score_cases as C
    lib = _lib.load()
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def cell(v):
        return '%8.4f [%8.4f .. %8.4f]' % (statistics.median(v), min(v), max(v))

    def wall(frame, sync_each=False, frames=None, repeats=None, warmup=None):
        """ms per frame: `frames` calls of frame() and one synchronisation, `repeats` times after `warmup`"""
        frames, repeats, warmup = frames or a.frames, repeats or a.repeats, a.warmup if warmup is None else warmup
        t = []
        for i in range(warmup + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(frames):
                frame()
                if sync_each:
                    torch.cuda.synchronize()
            torch.cuda.synchronize()
            if i >= warmup:
                t.append(1e3 * (time.perf_counter() - t0) / frames)
        return t

    def events(fn, burst=20):
        t = []
        for i in range(a.warmup + a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(burst):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                t.append(e0.elapsed_time(e1) / burst)
        return t
    say('tools/bench_score.py --repeats %d --warmup %d --frames %d   (%s, torch %s)'
        % (a.repeats, a.warmup, a.frames, torch.cuda.get_device_name(0), torch.__version__))
    say('per line: median [min .. max]; wall-clock figures are ms per frame call over %d calls, device figures ms per accumulate call' % a.frames)
    for label, (h, w), window in (('full frame 352 x 1216', (352, 1216), (0, 0, 352, 1216)),
                                  ("'vkitti' window of 375 x 1242", (375, 1242), eval_window('vkitti', 375, 1242))):
        for n in (1, 4, 16):
            out_np, gt_np = C.frames(1000 + n, n, h, w)
            out, gt = torch.from_numpy(out_np).cuda(), torch.from_numpy(gt_np).cuda()
            wy, wx, wh, ww = window
            nbytes = 2 * n * wh * ww * 4
            say()
            say('%s, N = %d: %.2f MB read per call' % (label, n, nbytes / 1e6))
            sums = [0.0] * 4
            t_host = wall(lambda: host_tail(torch, out, gt, window, sums), frames=4, repeats=a.host_repeats, warmup=1)
            say('  host tail (slice, .to(cpu), mask, four reductions), wall-clock ms per frame:      %s' % cell(t_host))
            t_met = wall(lambda: eval_metrics(out[..., wy:wy + wh, wx:wx + ww].contiguous(), gt[..., wy:wy + wh, wx:wx + ww].contiguous(), LO, HI).tolist())
            say('  eval_metrics on .contiguous() slices + read-back, wall-clock ms per frame:        %s' % cell(t_met))
            rs = RunScore(LO, HI, window=None if window == (0, 0, h, w) else window, max_n=n)
            t_upd = wall(lambda: rs.update(out, gt))
            t_lat = wall(lambda: rs.update(out, gt), sync_each=True)
            say('  RunScore.update, no read-back, wall-clock ms per frame:                           %s   host tail / this = %.0f, eval_metrics / this = %.1f'
                % (cell(t_upd), statistics.median(t_host) / statistics.median(t_upd), statistics.median(t_met) / statistics.median(t_upd)))
            say('  RunScore.update + a synchronisation per frame, wall-clock ms per frame:           %s' % cell(t_lat))
            rs.reset()
            rs.update(out, gt)
            got = rs.result()
            say('  result after one update: mae %.6f rmse %.6f imae %.6f irmse %.6f pixels %d' % (got['mae'], got['rmse'], got['imae'], got['irmse'], got['pixels']))
            if n == 1:
                ref = C.restate_run([(out_np, gt_np)], window=window, lo=LO, hi=HI)
                say('  exact-sum restatement:   mae %.6f rmse %.6f imae %.6f irmse %.6f pixels %d' % (ref['mae'], ref['rmse'], ref['imae'], ref['irmse'], ref['pixels']))
            k = _lib.ScoreArgs(depth=out.data_ptr(), ground_truth=gt.data_ptr(), n=n, height=h, width=w, win_y=wy, win_x=wx, win_height=wh,
                               win_width=ww, min_evaluate_depth=LO, max_evaluate_depth=HI, rule=_lib.PTTA_SCORE_RULE_ADAPT, state=rs._state.data_ptr())
            stream = torch.cuda.current_stream().cuda_stream

            def launch():
                if lib.ptta_score_accumulate(ctypes.byref(k), stream) != 0:
                    raise SystemExit('ptta_score_accumulate failed')
            t_k = events(launch)
            say('  ptta_score_accumulate alone (two launches), device events, ms per call:           %s   %.0f GB/s read'
                % (cell(t_k), nbytes / statistics.median(t_k) / 1e6))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
