"""Weight-gradient A/B at the wide channel pairs of the 2layers meta block: the engine's launcher (bf16x3, gwgrad_mfma.hip
gwgrad_x3_kernel WIDE) against the fp32-MFMA form (gwgrad_mfma_kernel) it replaces, hipEvent-timed through ptta_op_gwgrad, the two forms
alternating round by round in one process.  NLSPN 352x1216 (48 -> 256, 256 -> 48), CostDCNet 480x640 (16 -> 64), and NLSPN's 1layer
48 -> 48 (already bf16x3) as the precedent.

    python tools/bench_gwgrad_wide.py [--rounds 7] [--reps 10] [--case I] [--forms default]

--case / --forms restrict the run to one shape / one form, e.g. under `rocprofv3 --kernel-trace --stats` to split a call's time between the
weight-gradient kernel and its fixed-order reduction (profiles/gwgrad_wide_kernels.txt).
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

from proxytta.engine import op_gwgrad  # noqa: E402

CASES = [('nlspn 352x1216 48->256', 352, 1216, 48, 256),
         ('nlspn 352x1216 256->48', 352, 1216, 256, 48),
         ('costdcnet 480x640 16->64', 480, 640, 16, 64),
         ('nlspn 352x1216 48->48 (1layer)', 352, 1216, 48, 48)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--case', type=int, default=None, help='index into CASES (default: all)')
    ap.add_argument('--forms', default='default,fp32_mfma', help='comma-separated: default, fp32_mfma')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    print('device: %s' % torch.cuda.get_device_name(0))
    print('%-32s %12s %12s %8s %14s' % ('shape', 'bf16x3 us', 'fp32mfma us', 'speedup', 'max|d|/max|w|'))
    forms = a.forms.split(',')
    for name, h, w, ci, co in (CASES if a.case is None else [CASES[a.case]]):
        g = torch.Generator().manual_seed(ci * 1000 + co)
        x = torch.randn(1, h, w, ci, generator=g).cuda()
        gy = (torch.randn(1, h, w, co, generator=g) * 1e-2).cuda()
        t = {f: [] for f in forms}
        out = {}
        for r in range(a.rounds):
            for impl in (forms if r % 2 == 0 else forms[::-1]):
                gw, _, us = op_gwgrad(x, gy, impl=impl, reps=a.reps)
                t[impl].append(us)
                out[impl] = gw
        if len(forms) == 1:
            print('%-32s %s %12.1f us' % (name, forms[0], statistics.median(t[forms[0]])))
            continue
        d = float((out['default'] - out['fp32_mfma']).abs().max() / out['fp32_mfma'].abs().max())
        m0, m1 = statistics.median(t['default']), statistics.median(t['fp32_mfma'])
        print('%-32s %12.1f %12.1f %7.2fx %14.2e' % (name, m0, m1, m1 / m0, d))
        print('  rounds bf16x3: %s' % ' '.join('%.1f' % v for v in t['default']))
        print('  rounds fp32mfma: %s' % ' '.join('%.1f' % v for v in t['fp32_mfma']))
        del x, gy
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
