"""Eval-time hole filling on the device (include/ptta.h ptta_inpaint_biharmonic, proxytta.inpaint.inpainting_device;
profiles/inpaint_device.txt) beside the host path it can replace (proxytta.inpaint.inpainting, what NlspnModel_Adapt._fill runs under
fill_holes = True), on one box.

Workload: one 352x1216 frame (N = 1), a smooth positive depth field with a seeded hole pattern: 400 scattered pixels plus square blobs 2, 3,
3, 4, 6, 8 and 12 pixels across -- about 680 unknowns, the order of what a clamped eval output can hold.

  host      wall-clock ms of the whole host path as _fill runs it: the flag read, the map to the CPU, proxytta.inpaint.inpainting, the map
            back to the device; and of inpainting alone.  `--host-repeats` runs, median [min .. max].
  device    a pair of device events around each of `--repeats` calls of the entry point after `--warmup` calls (the map is restored from a
            device copy before each call, outside the events); ms, median [min .. max]; status (= iterations).  And the wall-clock ms
            of inpainting_device, which adds the read-back of the status word.
  forward   the NLSPN eval forward alone at the same size, device events, for scale.
  parity    fp32 units in the last place between the device's and the host's filled values: on the workload, and on every case of
            tests/inpaint_cases.py (what tests/test_gpu_inpaint_device.py asserts), with the iterations each took.
The condition is only that the device path is faster than the host path on the same box; the ratio is printed.

    python tools/bench_inpaint.py [--out FILE] [--repeats 20] [--warmup 3] [--host-repeats 3]
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

H, W = 352, 1216
BLOBS = (2, 3, 3, 4, 6, 8, 12)
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1, max_input_depth=80.0)


def workload(np, seed=0):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f = (20.0 + 8.0 * np.sin(y / 40.0) * np.cos(x / 90.0) + 0.03 * y + 0.05 * rng.standard_normal((H, W))).astype(np.float32)
    m = np.zeros((H, W), bool)
    m.flat[rng.choice(H * W, 400, replace=False)] = True
    for s in BLOBS:
        y0, x0 = rng.randint(0, H - s), rng.randint(0, W - s)
        m[y0:y0 + s, x0:x0 + s] = True
    return np.where(m, np.float32(0), f).astype(np.float32), m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the printed text to this file')
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-repeats', type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_inpaint.py measures on a HIP device and there is none')
    from proxytta import _lib, synth
    from proxytta.engine import Engine
    from proxytta.inpaint import inpainting, inpainting_device
    from tests import inpaint_cases as C
    lib = _lib.load()
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def cell(v):
        return '%9.3f [%9.3f .. %9.3f]' % (statistics.median(v), min(v), max(v))
    say('tools/bench_inpaint.py --repeats %d --warmup %d --host-repeats %d   (%s, torch %s)' % (a.repeats, a.warmup, a.host_repeats, torch.cuda.get_device_name(0),
                                                                                               torch.__version__))
    depth, mask = workload(np)
    say('workload: %dx%d, N = 1, %d unknowns (400 scattered + blobs %s)' % (H, W, int(mask.sum()), ', '.join('%dx%d' % (s, s) for s in BLOBS)))
    pristine = torch.from_numpy(depth).cuda().reshape(1, 1, H, W)

    # ---- host ----
    t_path, t_alone = [], []
    for _ in range(a.host_repeats):
        out = pristine.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if bool((out == 0).any()):
            host = out.cpu().numpy()
            t1 = time.perf_counter()
            host = inpainting(host)
            t2 = time.perf_counter()
            out = torch.from_numpy(host).to(out.device)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        t_path.append(1e3 * (t3 - t0)); t_alone.append(1e3 * (t2 - t1))
    want = out.cpu().numpy()[0, 0]
    say()
    say('host path (fill_holes = True), wall-clock ms, median [min .. max] of %d:' % a.host_repeats)
    say('  flag + map to the CPU + inpainting + map back   %s' % cell(t_path))
    say('  proxytta.inpaint.inpainting alone               %s' % cell(t_alone))

    # ---- device ----
    mu, mi, rtol = 65536, 2000, 1e-12
    size = lib.ptta_inpaint_scratch_bytes(1, H, W, mu)
    scratch = torch.empty((size + 7) // 8, device='cuda', dtype=torch.float64)
    status = torch.zeros(1, device='cuda', dtype=torch.int32)
    work = pristine.clone()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    t_dev = []
    for i in range(a.warmup + a.repeats):
        work.copy_(pristine)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = lib.ptta_inpaint_biharmonic(_lib.ptr(work), 1, H, W, mu, mi, rtol, _lib.ptr(scratch), scratch.numel() * 8, _lib.ptr(status), stream)
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0
        if i >= a.warmup:
            t_dev.append(e0.elapsed_time(e1))
    code = status.cpu().tolist()[0]
    got = work.cpu().numpy()[0, 0]
    t_fac = []
    for i in range(a.warmup + a.repeats):
        work.copy_(pristine)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        inpainting_device(work, mu, mi, rtol)
        t_fac.append(1e3 * (time.perf_counter() - t0))
    t_fac = t_fac[a.warmup:]
    say()
    say('device path (fill_holes = \'device\'), ms, median [min .. max] of %d after %d warm-up calls; max_unknowns %d, max_iter %d, rtol %g, scratch %.1f MB:'
        % (a.repeats, a.warmup, mu, mi, rtol, size / 1e6))
    say('  ptta_inpaint_biharmonic, device events          %s   status %d (iterations)' % (cell(t_dev), code))
    say('  inpainting_device, wall clock with the read-back %s' % cell(t_fac))
    ratio = statistics.median(t_path) / statistics.median(t_fac)
    say('  host path / device path (wall clock, medians): %.0f x  -- the device path is %s' % (ratio, 'FASTER' if ratio > 1 else 'NOT faster'))

    # ---- the eval forward alone ----
    eng = Engine(1, H, W, backbone='nlspn', **dict(HP, lr=3e-4))
    sd = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in synth.formula_state_dict_nlspn().items()}
    eng.load_state_dict({k: v for k, v in sd.items() if v.dtype == torch.float32})
    keep = {k: (sd[k].clone().contiguous(), torch.zeros_like(sd[k]), torch.zeros_like(sd[k])) for k in eng.adapted}
    for k in eng.adapted:
        eng.bind_adapted(k, *keep[k])
    image01, sparse = synth.synthetic_frame(0, H, W, 1, density=0.1)
    mean = np.array([0.485, 0.456, 0.406], dtype=np.float32).reshape(1, 3, 1, 1)
    std = np.array([0.229, 0.224, 0.225], dtype=np.float32).reshape(1, 3, 1, 1)
    image1 = torch.from_numpy(((np.floor(image01 * 255.0).astype(np.float32) / np.float32(255.0) - mean) / std).astype(np.float32)).cuda()
    sparse = torch.from_numpy(sparse).cuda()
    t_fwd = []
    for i in range(a.warmup + a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.forward_eval(image1, sparse)
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            t_fwd.append(e0.elapsed_time(e1))
    eng.close()
    say()
    say('NLSPN eval forward alone, %dx%d, N = 1, device events, ms: %s' % (H, W, cell(t_fwd)))
    say('  device filling / forward = %.2f, host path / forward = %.0f' % (statistics.median(t_dev) / statistics.median(t_fwd),
                                                                       statistics.median(t_path) / statistics.median(t_fwd)))

    # ---- parity ----
    say()
    say('parity with the host code, fp32 units in the last place at the filled pixels (every other pixel: bit-identical or the run stops):')
    assert np.array_equal(got[~mask].view(np.int32), depth[~mask].view(np.int32)) and not (got == 0).any()
    worst = int(C.ulps(got[mask], want[mask]).max())
    say('  %-20s %5d unknowns  %4d iterations  %d ulps' % ('workload %dx%d' % (H, W), int(mask.sum()), code, worst))
    for name in C.NAMES:
        _, m, d = C.case(name)
        t = torch.from_numpy(np.array(d)).cuda().reshape(1, 1, *d.shape)
        inpainting_device(t, mu, mi, rtol)
        out = t.cpu().numpy()[0, 0]
        assert np.array_equal(out[~m].view(np.int32), d[~m].view(np.int32)) and not (out == 0).any()
        u = int(C.ulps(out[m], C.expected(name)[m]).max())
        worst = max(worst, u)
        say('  %-20s %5d unknowns  %4d iterations  %d ulps' % ('%s %dx%d' % ((name,) + d.shape), int(m.sum()), inpainting_device.last_status[0], u))
    say('  maximum over all: %d ulps' % worst)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
