"""Time the NLSPN TTA step (BASELINE config 3: 1x3x352x1216) on one GPU.

    python tools/bench_nlspn.py [H W steps] [--meta 1layer|2layers|both] [--dtype fp32|mixed]

--meta both: the 1layer and the 2layers engines in the same process, timed in alternating rounds (ms per step, median of the rounds)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tta-depth-completion_amd'))
import numpy as np
import torch

from proxytta import synth
from proxytta.engine import Engine

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32).reshape(1, 3, 1, 1)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32).reshape(1, 3, 1, 1)
PREPARE = {'1layer': 'meta_selfsup_seq_1layer_ema', '2layers': 'meta_selfsup_seq_2layers_ema'}


def options(argv):
    """(positional arguments, {option: value}) for --name value pairs"""
    pos, opt, i = [], {}, 0
    while i < len(argv):
        if argv[i].startswith('--'):
            opt[argv[i][2:]] = argv[i + 1]
            i += 2
        else:
            pos.append(argv[i])
            i += 1
    return pos, opt


def make(n, h, w, meta, dtype):
    eng = Engine(n, h, w, backbone='nlspn', meta=meta, dtype=dtype, lr=3e-4, w_sparse_depth=1.0, w_smoothness=0.0, w_cos=0.0,
                 max_input_depth=80.0)
    sd = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in synth.formula_state_dict_nlspn(PREPARE[meta]).items()}
    eng.load_state_dict({k: v for k, v in sd.items() if v.dtype == torch.float32})
    keep = []
    for k in eng.adapted:
        p = sd[k].clone().contiguous()
        keep.append((p, torch.zeros_like(p), torch.zeros_like(p)))
        eng.bind_adapted(k, *keep[-1])
    eng._bench_keep = keep
    return eng


def timed_rounds(engines, fns, steps, rounds):
    """ms per call of every fn, median over `rounds` alternating rounds of `steps` calls (hipEvent timing)"""
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                fn()
            b.record()
            torch.cuda.synchronize()
            res[k].append(a.elapsed_time(b) / steps)
    return {k: float(np.median(v)) for k, v in res.items()}


def main():
    pos, opt = options(sys.argv[1:])
    h = int(pos[0]) if len(pos) > 0 else 352
    w = int(pos[1]) if len(pos) > 1 else 1216
    steps = int(pos[2]) if len(pos) > 2 else 3
    meta, dtype = opt.get('meta', '1layer'), opt.get('dtype', 'fp32')
    n = 1
    image01, sparse = synth.synthetic_frame(0, h, w, n)
    image = torch.from_numpy(((np.floor(image01 * 255) / 255 - MEAN) / STD).astype(np.float32)).cuda()
    sparse = torch.from_numpy(sparse).cuda()
    if meta == 'both':
        engs = {m: make(n, h, w, m, dtype) for m in ('1layer', '2layers')}
        fns = {}
        for m, eng in engs.items():
            fns[m + ' step'] = (lambda e=eng: e.step(image, sparse))
            fns[m + ' eval'] = (lambda e=eng: e.forward_eval(image, sparse))
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        r = timed_rounds(engs, fns, steps, int(opt.get('rounds', 7)))
        print('NLSPN %dx%d %s, median of alternating rounds of %d calls:' % (h, w, dtype, steps))
        for k, v in r.items():
            print('  %-14s %.3f ms' % (k, v))
        print('  2layers / 1layer step: %.3f' % (r['2layers step'] / r['1layer step']), flush=True)
        return
    eng = make(n, h, w, meta, dtype)
    print('alloc GB', torch.cuda.mem_get_info()[0] / 2**30, 'free of', torch.cuda.mem_get_info()[1] / 2**30, flush=True)
    for name, fn in (('step', lambda: eng.step(image, sparse)), ('eval', lambda: eng.forward_eval(image, sparse))):
        fn()
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        print('%s: %.2f ms' % (name, (time.time() - t0) / steps * 1e3), flush=True)
    d = eng.forward_eval(image, sparse)
    print('depth finite', bool(torch.isfinite(d).all()), float(d.min()), float(d.max()))


if __name__ == '__main__':
    main()
