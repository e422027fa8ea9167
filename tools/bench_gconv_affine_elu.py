#!/usr/bin/env python3
"""The 28 (convolution, BatchNorm3d + ELU) pairs of CostDCNet's UNet3D at 480x640, N = 1, each run as the two launches of today
(ptta_op_gconv, then ptta_op_gbn in eval mode) and as one launch with the ELU epilogue (ptta_op_gconv_affine, act 4), alternating.
The hooks allocate, pack the weight and synchronise per call, so wall time says nothing here: run it under
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o x -- python tools/bench_gconv_affine_elu.py [reps]
and read the kernel durations with  python tools/bench_gconv_affine_elu.py --read <dir>  (profiles/costdc_source.txt, section C).
The layers under "unet3d.inc" and "unet3d.down1" run bf16x6, as the engine's x6_layers list has them."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tta-depth-completion_amd')]


def layers(h4=120, w4=160):
    """(name, c0, c1, co, D, h, w, six) of every P3D block's 1x3x3 convolution; its 3x1x1 convolution is co -> co on the same volume."""
    f, out = (32, 48, 64, 80), []
    D, h, w = [16, 8, 4, 2], [h4 >> i for i in range(4)], [w4 >> i for i in range(4)]
    out += [('inc.0', 32, 0, 32, 0, True), ('inc.1', 32, 0, 32, 0, True)]
    for i in (1, 2, 3):
        out += [('down%d.0' % i, f[i - 1], 0, f[i - 1], i, i == 1), ('down%d.1' % i, f[i - 1], 0, f[i], i, i == 1)]
    for i in (2, 1, 0):
        out += [('up%d.0' % (4 - i), f[i], f[i + 1], f[i], i, False), ('up%d.1' % (4 - i), f[i], 0, f[i], i, False)]
    return [(n, c0, c1, co, D[l], h[l], w[l], six) for n, c0, c1, co, l, six in out]


def run(reps):
    import torch
    from proxytta.engine import op_gbn, op_gconv, op_gconv_affine
    g = torch.Generator().manual_seed(1)
    for name, c0, c1, co, D, h, w, six in layers():
        for vert in (False, True):
            ci0, ci1 = (co, 0) if vert else (c0, c1)
            shape = (1, D, h * w) if vert else (D, h, w)
            x = torch.randn(*shape, ci0 + ci1, generator=g).cuda()
            x0, x1 = x[..., :ci0], (x[..., ci0:] if ci1 else None)
            wt = (torch.randn(co, ci0 + ci1, 3, 1 if vert else 3, generator=g) * (3 * (1 if vert else 3) * (ci0 + ci1)) ** -0.5).cuda()
            gamma, beta = (0.5 + torch.rand(co, generator=g)).cuda(), torch.randn(co, generator=g).cuda() * 0.3
            rm, rv = torch.randn(co, generator=g).cuda() * 0.4, (0.3 + 2.0 * torch.rand(co, generator=g)).cuda()
            raw, un, fu = (torch.empty(*shape, co, device='cuda') for _ in range(3))
            st = torch.zeros(4, co, device='cuda')
            six_b = shape[0] if six else 0
            for _ in range(reps):
                op_gconv(x0, wt, raw, x1=x1, vert=vert, six_b=six_b)
                op_gbn('eval', raw, un, st, gamma, beta=beta, act='elu', rm=rm, rv=rv)
                op_gconv_affine(x0, wt, fu, st[2], st[3], x1=x1, act='elu', vert=vert, six_b=six_b)
            torch.cuda.synchronize()
            assert torch.equal(un, fu), name
    print('ran %d pairs x %d repetitions, fused == unfused bit for bit' % (2 * len(layers()), reps))


def read(d):
    f = sorted(glob.glob(d + '/**/*kernel_stats.csv', recursive=True))[0]
    rows = [r for r in csv.DictReader(open(f)) if 'gconv_x3_s1_kernel' in r['Name'] or 'gbn_apply_kernel' in r['Name']]
    tot = {'fused': [0.0, 0], 'conv': [0.0, 0], 'apply': [0.0, 0]}
    for r in sorted(rows, key=lambda r: r['Name']):
        args = r['Name'].split('<')[-1].split('>')[0].replace(' ', '').split(',')
        kind = 'apply' if 'gbn_apply' in r['Name'] else ('fused' if len(args) == 6 and args[5] in ('true', '1') else 'conv')
        tot[kind][0] += float(r['TotalDurationNs']); tot[kind][1] += int(r['Calls'])
        print('%-6s %-72s calls %5s total %9.3f ms avg %8.1f us' % (kind, r['Name'][:72], r['Calls'], float(r['TotalDurationNs']) / 1e6, float(r['AverageNs']) / 1e3))
    n = tot['fused'][1] // 28 or 1
    two, one = (tot['conv'][0] + tot['apply'][0]) / n / 1e3, tot['fused'][0] / n / 1e3
    print('per pass over the 28 pairs (%d repetitions): two launches %.1f us (convolutions %.1f + gbn_apply %.1f), fused %.1f us: %.1f us less, %.1f %%'
          % (n, two, tot['conv'][0] / n / 1e3, tot['apply'][0] / n / 1e3, one, two - one, 100 * (two - one) / two))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--read':
        read(sys.argv[2])
    else:
        run(int(sys.argv[1]) if len(sys.argv) > 1 else 10)
