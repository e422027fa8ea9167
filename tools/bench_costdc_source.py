"""CostDCNet's source model at 480x640, N = 1 (include/ptta.h PTTA_COSTDC_PLAIN | PTTA_ADAPT_META_ONLY; profiles/costdc_source.txt): its eval
forward with every dense BatchNorm in its convolution's epilogue (option "eval_bn_fused" 1) against the same binary with the option at 0
(43 more gbn_apply launches), and against the eval forward of the ProxyTTA handle of the same checkpoint -- the nearest thing the library
offered before: another network (the meta convolution, batch statistics in Encoder2D); and the step of the BatchNorm-adaptation baseline
(PTTA_COSTDC_PLAIN alone) against the ProxyTTA 'meta_bn' step.

One process.  Three handles with the same weights (tests/costdc_source_cases.py, the stage-3 form of the checkpoint); `--warmup` calls per
setting, then `--blocks` blocks of `--steps` calls per setting, the settings of a group (the three eval forwards, the two steps) rotating
block by block (the order reverses every round); each block is timed with one pair of hipEvents around its calls.  Reported per setting: the median block's ms / call and the spread.

    python tools/bench_costdc_source.py [--blocks 9] [--steps 8] [--warmup 4] [--size 480x640]
    python tools/bench_costdc_source.py --trace-calls 6        under `rocprofv3 --kernel-trace --output-format csv`: no timing, 6 calls per setting
    python tools/bench_costdc_source.py --count-launches <kernel_trace.csv>     launches per call of each setting from that trace (no GPU)

`--trace-calls` waits for the device and fills a 7-float tensor (a kernel of torch's own) before every call: the launches of one call are
those between two such fills.
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

FORMS = ('source eval, eval_bn_fused 1', 'source eval, eval_bn_fused 0', 'ProxyTTA handle, eval forward', 'baseline step', "ProxyTTA 'meta_bn' step")
HP = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1)


def count_launches(path, calls):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    # the marker: torch's fill of a 7-element tensor before every call (--trace-calls); the library launches no kernel of torch's
    # (its zero-fills while the handles are set up come before the first marker: the last calls x settings + 1 fills are the markers)
    marks = [i for i, r in enumerate(rows) if 'FillFunctor' in r['Kernel_Name']]
    assert len(marks) >= calls * len(FORMS) + 1, 'expected %d markers in the trace, found %d' % (calls * len(FORMS) + 1, len(marks))
    marks = marks[-(calls * len(FORMS) + 1):]
    for f, form in enumerate(FORMS):
        m = marks[f * calls:(f + 1) * calls + 1]
        per = [b - a - 1 for a, b in zip(m[:-1], m[1:])]
        names = {}
        for r in rows[m[-2] + 1:m[-1]]:
            k = r['Kernel_Name'].replace('(anonymous namespace)::', '').split('(')[0]
            names[k] = names.get(k, 0) + 1
        # the first call of a handle does its one-time work (eval affine tables ...): report the steady calls
        print('%-34s launches per call %s   (steady: %d)' % (form, per, per[-1]))
        for k, v in sorted(names.items(), key=lambda kv: -kv[1]):
            print('      %4d  %s' % (v, k[:110]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=9)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--size', default='480x640')
    ap.add_argument('--trace-calls', type=int, default=0)
    ap.add_argument('--count-launches', default=None)
    a = ap.parse_args()
    if a.count_launches:
        return count_launches(a.count_launches, a.trace_calls or 6)

    import numpy as np
    import torch
    from proxytta.engine import Engine
    from tests.costdc_source_cases import MAX_DEPTH, source_state_dict
    from tests.test_gpu_costdcnet import costdc_frame

    h, w = [int(v) for v in a.size.split('x')]
    torch.cuda.set_device(0)
    sd = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in source_state_dict(stage3=True).items()}
    frames = [[torch.from_numpy(x).cuda() for x in costdc_frame(i, h, w, 1, density=1500.0 / (h * w))] for i in range(3)]

    def make(**kw):
        eng = Engine(1, h, w, backbone='costdcnet', max_predict_depth=MAX_DEPTH, **dict(HP, **kw))
        eng.load_state_dict({k: (v.clone() if k.endswith(('running_mean', 'running_var', 'num_batches_tracked')) else v) for k, v in sd.items()})
        keep = {k: (sd[k].clone().contiguous(), torch.zeros_like(sd[k]), torch.zeros_like(sd[k])) for k in eng.adapted}
        for k in eng.adapted:
            eng.bind_adapted(k, *keep[k])
        return eng, keep

    source, proxy, base = make(meta='plain', adapt_mode='meta'), make(), make(meta='plain')
    print('device: %s   %dx%d N 1   eval_bn_fused_count %d' % (torch.cuda.get_device_name(0), h, w, source[0].get_option('eval_bn_fused_count')))

    def call(f, i):
        raw, image1, sparse = frames[i % len(frames)]
        if f < 2:
            if source[0].get_option('eval_bn_fused') != 1 - f:
                source[0].set_option('eval_bn_fused', 1 - f)
            return source[0].forward_eval(image1, sparse)
        if f == 2:
            return proxy[0].forward_eval(image1, sparse)
        return (base if f == 3 else proxy)[0].step(image1, sparse, loss_image=raw)

    def block(f, n, first):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            call(f, first + i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    if a.trace_calls:
        mark = torch.zeros(7, device='cuda')
        for f in range(len(FORMS)):
            for i in range(a.trace_calls):
                torch.cuda.synchronize()
                mark.fill_(1.0)
                call(f, i)
        torch.cuda.synchronize()
        mark.fill_(2.0)
        torch.cuda.synchronize()
        return
    assert torch.equal(call(0, 0), call(1, 0)), 'fused and unfused eval forwards differ'
    t = {f: [] for f in range(5)}
    for group in ((0, 1, 2), (3, 4)):              # the eval forwards first: the steps move the ProxyTTA handle's weights
        for f in group:
            block(f, a.warmup, 0)
        for r in range(a.blocks):
            for f in (group if r % 2 == 0 else group[::-1]):
                t[f].append(block(f, a.steps, r))
    m = [statistics.median(t[f]) for f in range(5)]
    print('blocks %d x %d calls, warm-up %d' % (a.blocks, a.steps, a.warmup))
    for f in range(5):
        print('%-34s %8.3f ms / call   (%.3f .. %.3f over the blocks)' % (FORMS[f], m[f], min(t[f]), max(t[f])), flush=True)
    print('%-34s %+8.3f ms (%.1f %%)' % ('  fused against unfused', m[0] - m[1], 100.0 * (m[0] - m[1]) / m[1]))
    print('%-34s %+8.3f ms (%.1f %%)' % ('  source against ProxyTTA eval', m[0] - m[2], 100.0 * (m[0] - m[2]) / m[2]))
    print('%-34s %+8.3f ms (%.1f %%)' % ('  baseline against ProxyTTA step', m[3] - m[4], 100.0 * (m[3] - m[4]) / m[4]), flush=True)
    for e, _ in (source, proxy, base):
        e.close()


if __name__ == '__main__':
    main()
