"""Time the CostDCNet TTA step (BASELINE config 5: 1x3x480x640) on one GPU, the 1layer and the 2layers meta layer in the same process.

    python tools/bench_costdcnet.py [H W steps] [--meta 1layer|2layers|both] [--rounds R]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tta-depth-completion_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from bench_nlspn import MEAN, PREPARE, STD, options, timed_rounds
from proxytta import synth
from proxytta.engine import Engine


def make(n, h, w, meta):
    eng = Engine(n, h, w, backbone='costdcnet', meta=meta, max_predict_depth=8.0, lr=3e-3, w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1)
    sd = synth.formula_state_dict_costdcnet(PREPARE[meta])
    sd = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in sd.items()}
    eng.load_state_dict(sd)
    keep = []
    for k in eng.adapted:
        p = sd[k].clone().contiguous()
        keep.append((p, torch.zeros_like(p), torch.zeros_like(p)))
        eng.bind_adapted(k, *keep[-1])
    eng._bench_keep = (keep, sd)
    return eng


def main():
    pos, opt = options(sys.argv[1:])
    h = int(pos[0]) if len(pos) > 0 else 480
    w = int(pos[1]) if len(pos) > 1 else 640
    steps = int(pos[2]) if len(pos) > 2 else 5
    metas = ('1layer', '2layers') if opt.get('meta', 'both') == 'both' else (opt['meta'],)
    n = 1
    image01, sparse = synth.synthetic_frame(0, h, w, n, density=1500.0 / (h * w), dmin=0.3, dmax=7.5)
    image = torch.from_numpy(((np.floor(image01 * 255) / 255 - MEAN) / STD).astype(np.float32)).cuda()
    sparse = torch.from_numpy(sparse).cuda()
    engs = {m: make(n, h, w, m) for m in metas}
    fns = {}
    for m, eng in engs.items():
        fns[m + ' step'] = (lambda e=eng: e.step(image, sparse))
        fns[m + ' eval'] = (lambda e=eng: e.forward_eval(image, sparse))
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    r = timed_rounds(engs, fns, steps, int(opt.get('rounds', 7)))
    print('CostDCNet %dx%d fp32, median of alternating rounds of %d calls:' % (h, w, steps))
    for k, v in r.items():
        print('  %-14s %.3f ms' % (k, v))
    if len(metas) == 2:
        print('  2layers / 1layer step: %.3f' % (r['2layers step'] / r['1layer step']), flush=True)


if __name__ == '__main__':
    main()
