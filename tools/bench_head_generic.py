"""Stage-2 head-trainer step time on the generic engine: NLSPN at 352x1216 and CostDCNet at 480x640, N = 1 and 2, both loss directions, with
option "head_bn_fused" at 1 (every frozen BatchNorm2d of the backbone prefix in its convolution's epilogue) and at 0 (an affine-table launch
and an apply launch per BatchNorm2d) -- include/ptta.h ptta_set_option, profiles/head_bn_fused.txt.

One process per run.  Per configuration: one handle, `--warmup` steps at each setting, then `--blocks` blocks of `--steps` head steps per
setting, the two settings alternating block by block (the order swaps every round, so neither setting always runs first); each block is timed
with one pair of hipEvents around its steps.  Reported per setting: the median block's ms / step and the spread (min .. max) over the blocks.

    python tools/bench_head_generic.py [--blocks 7] [--steps 10] [--warmup 5] [--legs 1,0] [--only nlspn] [--trace-steps K] [--untouched]

--legs 0 --untouched   the separate-launch leg alone and the option neither set nor read: what a library from before the option runs -- the
           parent-commit figure
--trace-steps K   no timing: K head steps of one configuration (--only, --n, --direction) at the setting of --legs, for a
                  `rocprofv3 --kernel-trace` run that counts launches per step
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tta-depth-completion_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from tests.test_gpu_head_trainer import _generic_head_frame, make_generic_head_engine  # noqa: E402

SHAPES = {'nlspn': (352, 1216), 'costdcnet': (480, 640)}
HP = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)


def block(eng, frames, reverse, steps, first):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        eng.head_step(*frames[(first + i) % len(frames)], reverse)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--legs', default='1,0', help="settings of 'head_bn_fused' to time")
    ap.add_argument('--untouched', action='store_true', help='never call set_option / get_option (a library without the option)')
    ap.add_argument('--only', default=None, help='nlspn or costdcnet')
    ap.add_argument('--n', type=int, default=None)
    ap.add_argument('--direction', default=None, help='reverse or forward')
    ap.add_argument('--trace-steps', type=int, default=0)
    a = ap.parse_args()
    legs = [int(v) for v in a.legs.split(',')]
    touch = not a.untouched
    torch.cuda.set_device(0)
    print('device: %s   blocks %d x %d steps, warm-up %d, legs %s' % (torch.cuda.get_device_name(0), a.blocks, a.steps, a.warmup, legs))
    print('%-10s %2s %-8s %-7s %10s %22s %6s' % ('backbone', 'N', 'loss', 'fused', 'ms/step', 'spread (min .. max)', 'count'))
    for backbone in ([a.only] if a.only else ['nlspn', 'costdcnet']):
        h, w = SHAPES[backbone]
        for n in ([a.n] if a.n else [1, 2]):
            eng, sd, _, keep = make_generic_head_engine(backbone, n, h, w, HP, 0.999)
            frames = [[torch.from_numpy(x).cuda() for x in _generic_head_frame(backbone, i, h, w, n)] for i in range(3)]
            for reverse in ([a.direction == 'reverse'] if a.direction else [True, False]):
                if a.trace_steps:
                    if touch:
                        eng.set_option('head_bn_fused', legs[0])
                    for i in range(a.trace_steps):
                        eng.head_step(*frames[i % 3], reverse)
                    torch.cuda.synchronize()
                    continue
                t = {leg: [] for leg in legs}
                count = {}
                for leg in legs:
                    if touch:
                        eng.set_option('head_bn_fused', leg)
                        count[leg] = eng.get_option('head_bn_fused_count')
                    block(eng, frames, reverse, a.warmup, 0)
                for r in range(a.blocks):
                    for leg in (legs if r % 2 == 0 else legs[::-1]):
                        if touch:
                            eng.set_option('head_bn_fused', leg)
                        t[leg].append(block(eng, frames, reverse, a.steps, r))
                for leg in legs:
                    v = t[leg]
                    print('%-10s %2d %-8s %-7d %10.3f %10.3f .. %-9.3f %6s' % (backbone, n, 'reverse' if reverse else 'forward', leg,
                                                                           statistics.median(v), min(v), max(v), count.get(leg, '-')), flush=True)
                if len(legs) == 2:
                    m = [statistics.median(t[leg]) for leg in legs]
                    print('%-10s %2d %-8s %d vs %d: %+.3f ms/step (%.2f %%)' % (backbone, n, 'reverse' if reverse else 'forward', legs[0], legs[1],
                                                                             m[0] - m[1], 100.0 * (m[0] - m[1]) / m[1]), flush=True)
            eng.close()
            del eng, sd, keep, frames
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
