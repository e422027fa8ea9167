"""MSG_CHN's source model at 352x1216, N = 1 (include/ptta.h PTTA_MSGCHN_PLAIN; profiles/msgchn_source.txt): the eval forward of the source
handle against the eval forward of a ProxyTTA 1layer fp32 handle with the same backbone weights -- the same schedule plus the meta
convolution and the re-packing of its adapted weights.

One process.  Per handle `--warmup` calls, then `--blocks` blocks of `--steps` calls, the two handles alternating block by block (the order
swaps every round); each block is timed with one pair of hipEvents around its calls.  Reported per handle: the median block's ms / call and
the spread over the blocks; then the launches per eval forward of both kinds from the profiling leg (ptta_profile_read: every bracketed
launch, by class) and the device memory each handle took (hipMemGetInfo around its creation).

    python tools/bench_msgchn_source.py [--blocks 9] [--steps 20] [--warmup 5] [--size 352x1216]
    python tools/bench_msgchn_source.py --trace source|proxytta [--trace-calls 4]      under `rocprofv3 --kernel-trace --output-format csv`: no timing
    python tools/bench_msgchn_source.py --compare-names <source kernel_trace.csv> <proxytta kernel_trace.csv>      (no GPU)
"""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tta-depth-completion_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

FORMS = ('source eval (PTTA_MSGCHN_PLAIN)', 'ProxyTTA 1layer fp32 eval')
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1, max_input_depth=80.0)


def kernel_names(path):
    names = {}
    for r in csv.DictReader(open(path)):
        k = r['Kernel_Name'].replace('(anonymous namespace)::', '')
        names[k] = names.get(k, 0) + 1
    return names


def compare_names(src, proxy, calls):
    a, b = kernel_names(src), kernel_names(proxy)
    print('kernel names of the source handle\'s trace (%d calls): launches in it / in the ProxyTTA handle\'s' % calls)
    for k, v in sorted(a.items(), key=lambda kv: -kv[1]):
        print('  %5d %5d  %s' % (v, b.get(k, 0), k[:150]))
    new = sorted(set(a) - set(b))
    print('names in the source trace that the ProxyTTA trace lacks: %s' % (new or 'none'))
    print('names in the ProxyTTA trace alone: %s' % ([k[:100] for k in sorted(set(b) - set(a))] or 'none'))
    # (the whole trace: the zero-fills of every allocation and the weight packing at load are in it; a forward's own launches are each row / calls)
    print('launches in the whole trace: source %d, ProxyTTA %d' % (sum(a.values()), sum(b.values())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=9)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--size', default='352x1216')
    ap.add_argument('--trace', default=None, choices=('source', 'proxytta'))
    ap.add_argument('--trace-calls', type=int, default=4)
    ap.add_argument('--compare-names', nargs=2, default=None)
    a = ap.parse_args()
    if a.compare_names:
        return compare_names(a.compare_names[0], a.compare_names[1], a.trace_calls)

    import numpy as np
    import torch
    from proxytta import synth
    from proxytta.engine import ADAPTED, Engine

    h, w = [int(v) for v in a.size.split('x')]
    torch.cuda.set_device(0)
    sd = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in synth.formula_state_dict().items()}
    frames = [[torch.from_numpy(x).cuda() for x in synth.synthetic_frame(i, h, w, 1)] for i in range(3)]

    def make(f):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        eng = Engine(1, h, w, meta='plain' if f == 0 else '1layer', **HP)
        torch.cuda.synchronize()
        took = free0 - torch.cuda.mem_get_info()[0]
        eng.load_state_dict(sd)                      # the stage-3 checkpoint on both: the source handle ignores what _prepare_head added
        keep = [(sd[k].clone(), torch.zeros_like(sd[k]), torch.zeros_like(sd[k])) for k in eng.adapted]
        for k, ts in zip(eng.adapted, keep):
            eng.bind_adapted(k, *ts)
        assert list(eng.adapted) == ([] if f == 0 else list(ADAPTED))
        return eng, keep, took

    def call(eng, i):
        image, sparse = frames[i % len(frames)]
        return eng.forward_eval(image, sparse)

    if a.trace:
        eng, keep, _ = make(0 if a.trace == 'source' else 1)
        for i in range(a.trace_calls):
            call(eng, i)
        torch.cuda.synchronize()
        eng.close()
        return

    engines = [make(0), make(1)]

    def block(f, n, first):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            call(engines[f][0], first + i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    print('device: %s   %dx%d N 1   blocks %d x %d calls, warm-up %d' % (torch.cuda.get_device_name(0), h, w, a.blocks, a.steps, a.warmup))
    t = {0: [], 1: []}
    for f in (0, 1):
        block(f, a.warmup, 0)
    for r in range(a.blocks):
        for f in ((0, 1) if r % 2 == 0 else (1, 0)):
            t[f].append(block(f, a.steps, r))
    for f in (0, 1):
        print('%-34s %8.4f ms / call   (%.4f .. %.4f over the blocks)' % (FORMS[f], statistics.median(t[f]), min(t[f]), max(t[f])), flush=True)
    m = [statistics.median(t[f]) for f in (0, 1)]
    print('%-34s %+8.4f ms (%.2f %%)' % ('  source against ProxyTTA', m[0] - m[1], 100.0 * (m[0] - m[1]) / m[1]), flush=True)
    # launches of one eval forward, by class of the profiling leg (include/ptta.h PTTA_PROF_*)
    for f in (0, 1):
        eng = engines[f][0]
        eng.profile(True)
        call(eng, 0)
        per = [int(eng.profile_read(k)[3]) for k in range(9)]
        eng.profile(False)
        print('%-34s bracketed launches per eval forward %d   by class %s' % (FORMS[f], sum(per), per))
    print('device memory taken at creation: source %.1f MiB, ProxyTTA %.1f MiB (x %.2f)' % (engines[0][2] / 2 ** 20, engines[1][2] / 2 ** 20,
                                                                                            engines[1][2] / max(engines[0][2], 1)))
    d = [call(engines[f][0], 0).clone() for f in (0, 1)]
    print('the two networks\' depths on frame 0 are %.3e relative MAE apart (another network, not another form)' %
          float((d[0] - d[1]).abs().mean() / d[1].abs().mean()))
    for e, _, _ in engines:
        e.close()


if __name__ == '__main__':
    main()
