"""The price of option "deterministic" (include/ptta.h ptta_set_option): the NLSPN TTA step at 352x1216, N = 1 and 2, fp32 and mixed, with the
propagation gradients' scatters as float atomics (0, the default) and in 64-bit fixed point (1) -- and one propagation sweep's gradient alone
through ptta_op_nl_prop_bwd, form 0 against form 1, on the offsets and affinities of the same frames.  profiles/nlspn_deterministic.txt.

One process per run.  Per configuration: one handle, `--warmup` steps at each setting, then `--blocks` blocks of `--steps` steps per setting,
the two settings alternating block by block (the order swaps every round, so neither setting always runs first); each block is timed with one
pair of hipEvents around its steps.  Reported per setting: the median block's ms / step and the spread (min .. max) over the blocks.  The
sweep is timed by the library (hipEvents around `--sweeps` launches on the stream), one block per form and round, the same alternation.

    python tools/bench_nlspn_deterministic.py [--blocks 7] [--steps 5] [--warmup 3] [--sweeps 50] [--legs 0,1] [--n N] [--dtype fp32|mixed]
                                              [--untouched] [--package DIR]

--legs 0 --untouched   the default leg alone, the option neither set nor read and the sweep hook not called: what a library from before the
                       option runs -- the parent-commit figure
--package DIR          the directory that holds the `proxytta` package to measure (default: this tree's): a build of the parent commit
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _paths(package):
    for p in (ROOT, package or os.path.join(ROOT, 'tta-depth-completion_amd')):
        if p in sys.path:
            sys.path.remove(p)
        sys.path.insert(0, p)


H, W = 352, 1216


def block(eng, frames, steps, first):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        raw, image1, sparse = frames[(first + i) % len(frames)]
        eng.step(image1, sparse, loss_image=raw)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def report(label, legs, t, unit):
    for leg in legs:
        v = t[leg]
        print('%-26s %-4d %10.3f %10.3f .. %-9.3f' % (label, leg, statistics.median(v), min(v), max(v)), flush=True)
    if len(legs) == 2:
        m = [statistics.median(t[leg]) for leg in legs]
        print('%-26s %d vs %d: %+.3f %s (%+.2f %%)' % (label, legs[1], legs[0], m[1] - m[0], unit, 100.0 * (m[1] - m[0]) / m[0]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sweeps', type=int, default=50)
    ap.add_argument('--legs', default='0,1', help="settings of 'deterministic' to time")
    ap.add_argument('--untouched', action='store_true', help='never call set_option or the sweep hook (a library without the option)')
    ap.add_argument('--package', default=None)
    ap.add_argument('--n', type=int, default=None)
    ap.add_argument('--dtype', default=None)
    a = ap.parse_args()
    _paths(a.package)
    import torch
    from tests.test_gpu_nlspn import HP, make_nlspn, nlspn_frame
    legs = [int(v) for v in a.legs.split(',')]
    touch = not a.untouched
    torch.cuda.set_device(0)
    print('device: %s   %d x %d   blocks %d x %d steps, warm-up %d, legs %s' % (torch.cuda.get_device_name(0), H, W, a.blocks, a.steps, a.warmup, legs))
    print('%-26s %-4s %10s %22s' % ('configuration', 'det', 'median', 'spread (min .. max)'))
    for n in ([a.n] if a.n else [1, 2]):
        frames = [[torch.from_numpy(x).cuda() for x in nlspn_frame(i, H, W, n)] for i in range(3)]
        for dtype in ([a.dtype] if a.dtype else ['fp32', 'mixed']):
            eng, _, _ = make_nlspn(n, H, W, hp=dict(HP, dtype=dtype))
            t = {leg: [] for leg in legs}
            for leg in legs:
                if touch:
                    eng.set_option('deterministic', leg)
                block(eng, frames, a.warmup, 0)
            for r in range(a.blocks):
                for leg in (legs if r % 2 == 0 else legs[::-1]):
                    if touch:
                        eng.set_option('deterministic', leg)
                    t[leg].append(block(eng, frames, a.steps, r))
            report('step N %d %-5s  ms/step' % (n, dtype), legs, t, 'ms/step')
            if touch and dtype == 'fp32':
                # one sweep's gradient on this handle's own offsets and affinities (the propagation is fp32 in both dtypes)
                from proxytta.engine import op_nl_prop_bwd
                raw, image1, sparse = frames[0]
                eng.forward_train(image1, sparse)
                off9, aff9 = eng.debug_tensor('off9').view(n, 18, H, W), eng.debug_tensor('aff9').view(n, 9, H, W)
                fix = sparse.clamp(0, HP['max_input_depth']).view(n, H, W).contiguous()
                pred = eng.debug_tensor('pred_init').view(n, H, W)
                pinned = torch.where(fix > 0, fix, pred).contiguous()
                gout = (torch.rand(n, H, W, device='cuda', generator=torch.Generator('cuda').manual_seed(1)) - 0.5).contiguous()
                goff9, gaff9 = torch.zeros_like(off9), torch.zeros_like(aff9)
                ts = {leg: [] for leg in legs}
                for r in range(a.blocks + 1):                              # (the first round warms up)
                    for leg in (legs if r % 2 == 0 else legs[::-1]):
                        us = op_nl_prop_bwd(pinned, fix, off9, aff9, gout, goff9, gaff9, form=leg, reps=a.sweeps)[1]
                        if r:
                            ts[leg].append(us)
                report('sweep N %d  us/sweep' % n, legs, ts, 'us/sweep')
            eng.close()
            del eng
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
