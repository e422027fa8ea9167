"""Raw-frame egress (include/ptta.h ptta_egress_raw, proxytta.sink.RawFrameSink; profiles/egress_raw.txt): what it costs to turn a
prediction into the stored 16-bit frame, on the host thread and on the card, beside the reference-style host tail it replaces.

One process; predictions 352x1216 pasted into 375x1242 at (23, 13), N = 1, 4 and 16 frames per call.

  (a) host tail   what a user writes by hand today, the reference's save_depth up to the encoder: depth.cpu() (a blocking copy of the fp32
                  map from a device that is idle: no compute is waited for), np.uint32(z * 256.0), paste into the zero frame.  Host clock,
                  ms per FRAME on the one host thread; the baseline of this file.
  (b) submit      RawFrameSink.submit alone, depth plane, in a loop of its own: host clock around the call (it enqueues a launch, two event
                  records, a stream wait and one copy; nothing is waited for), then collect() + release(), clocked apart; bytes that cross the
                  link per call, and the slot's device-to-host copy alone by device events on the copy stream.
  (c) kernel      one pair of device events around `--launches` calls of the entry point (through ctypes, arguments prepared once) after a
                  warm-up, for the depth plane and for all three, beside a device-to-device copy_ of as many bytes as the launch reads and
                  writes together (a copy of B bytes reads B and writes B), timed the same way.  A call's buffers fit the 256 MiB Infinity
                  Cache and a run of launches reads and writes the same ones: warm-cache rates, not HBM rates.
  (d) adapt loop  ExternalModel_Adapt.adapt on the MSG_CHN engine, ms per FRAME with sink=None and with a sink (no writer; the oldest slot
                  is collected and released once every slot is unread, as a consumer would), legs alternating, each repeated `--repeats`
                  times: what the sink adds to a frame.

    python tools/bench_egress.py [--out FILE] [--steps 30] [--repeats 3] [--launches 300] [--ns 1,4,16]
    python tools/bench_egress.py --resources       hipcc's kernel-resource-usage remarks for csrc/egress.hip (compiles only: needs no GPU)
The measuring form fails without a GPU.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tta-depth-completion_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')        # as bench.py: before the HIP runtime exists

MODE = 'meta_selfsup_seq_1layer_ema'
(H, W), (h, w), (SY, SX) = (375, 1242), (352, 1216), (23, 13)


def resources():
    """The remarks of `hipcc -Rpass-analysis=kernel-resource-usage` for csrc/egress.hip with csrc/Makefile's flags, one line per kernel."""
    src = os.path.join(ROOT, 'tta-depth-completion_amd', 'csrc', 'egress.hip')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-fPIC', '-std=c++17', '-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', os.devnull],
                       capture_output=True, text=True, check=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            f = re.search(r'egress_raw_kernelILb(\d)ELb(\d)ELb(\d)E', m.group(1))
            cur = {'name': 'egress_raw_kernel<%s>' % ' + '.join(k for k, on in zip(('depth', 'validity', 'image'), f.groups()) if on == '1')}
            rows.append(cur)
        m = re.search(r'(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)', line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    out = ['hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage, csrc/egress.hip (compiled, not run):',
           '  %-50s %5s %5s %8s %10s %10s %9s' % ('kernel', 'VGPR', 'SGPR', 'scratch', 'SGPR spill', 'VGPR spill', 'waves/SIMD')]
    for c in rows:
        out.append('  %-50s %5d %5d %8d %10d %10d %9d' % (c['name'], c['VGPRs'], c['TotalSGPRs'], c['ScratchSize [bytes/lane]'], c['SGPRs Spill'],
                                                        c['VGPRs Spill'], c['Occupancy [waves/SIMD]']))
    out.append('  scratch bytes per lane over all %d kernels: max %d; LDS: %d' % (len(rows), max(c['ScratchSize [bytes/lane]'] for c in rows),
                                                                            max(c['LDS Size [bytes/block]'] for c in rows)))
    return '\n'.join(out)


def cell(v):
    return '%8.3f [%7.3f .. %7.3f]' % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the printed text to this file')
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--launches', type=int, default=300)
    ap.add_argument('--ns', default='1,4,16')
    ap.add_argument('--resources', action='store_true')
    a = ap.parse_args()
    if a.resources:
        print(resources())
        return
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_egress.py measures on a HIP device and there is none (only --resources runs without one)')
    from proxytta import _lib, synth
    from proxytta.egress import PLANES, egress_raw
    from proxytta.model import ExternalModel_Adapt
    from proxytta.sink import RawFrameSink
    lib = _lib.load()
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)
    say('tools/bench_egress.py --steps %d --repeats %d --launches %d   (%s, torch %s)' % (a.steps, a.repeats, a.launches, torch.cuda.get_device_name(0), torch.__version__))
    say('prediction %dx%d pasted into %dx%d at (%d, %d)' % (h, w, H, W, SY, SX))
    ns = [int(v) for v in a.ns.split(',')]

    def prediction(seed, n):
        rng = np.random.default_rng(seed)
        return torch.from_numpy((rng.random((n, 1, h, w)) * 80.0).astype(np.float32)).cuda()

    def events(fn, count, stream=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        for _ in range(count):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / count          # us per call

    # ---- (a) and (b): the host thread ----
    say()
    say('(a) host tail and (b) RawFrameSink.submit, depth plane: host clock, median of %d calls [min .. max], ms per FRAME (ms per call / N); device idle at each call' % (a.steps * a.repeats))
    say('  %3s  %-30s %-30s %-30s %s' % ('N', '(a) .cpu() + uint32(z*256) + paste', '(b) submit()', '(b) collect() + release()',
                                         'MB over the link per call (a) / (b); (b) copy us / call, GB/s'))
    host = {}
    for n in ns:
        depth = prediction(n, n)
        sink = RawFrameSink(n, h, w, H, W)
        st = (torch.full((n,), SY, dtype=torch.int32).cuda(), torch.full((n,), SX, dtype=torch.int32).cuda())
        ta, tb, tc = [], [], []
        for i in range(4 + a.steps * a.repeats):           # (a) in a loop of its own: its arrays sweep the host's caches
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            z = depth.cpu().numpy()
            u = np.uint32(z * 256.0)
            frame = np.zeros((n, H, W), dtype=np.uint32)
            frame[:, SY:SY + h, SX:SX + w] = u[:, 0]
            t1 = time.perf_counter()
            if i >= 4:                                     # (the first calls warm the path up)
                ta.append(1e3 * (t1 - t0) / n)
        for i in range(4 + a.steps * a.repeats):
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            sink.submit(depth=depth, start=st)
            t3 = time.perf_counter()
            got = sink.collect()
            sink.release()
            t4 = time.perf_counter()
            if i == 0:
                assert np.array_equal(np.minimum(frame, 65535).astype(np.uint16), got['depth_u16'])          # the two tails agree
            if i >= 4:
                tb.append(1e3 * (t3 - t2) / n); tc.append(1e3 * (t4 - t3) / n)
        with torch.cuda.stream(sink.copy_stream):
            cus = events(lambda: sink.host[0].copy_(sink.raw[0], non_blocking=True), 20, sink.copy_stream)
        host[n] = (statistics.median(ta), statistics.median(tb), statistics.median(tc), cus)
        say('  %3d  %-30s %-30s %-30s %.2f / %.2f   %8.1f %6.1f' % (n, cell(ta), cell(tb), cell(tc), 4 * n * h * w / 1e6, sink.bytes_per_frame / 1e6, cus,
                                                                   sink.bytes_per_frame / cus / 1e3))
        del sink, depth
    say('  (collect() right behind submit() waits for the launch and the whole copy: the last two columns are that copy alone, by device events on the copy stream)')

    # ---- (c): the launch ----
    say()
    say('(c) kernel: %d launches between two device events, after 20 warm-up launches; GB/s = (bytes read + bytes written) / time; copy = torch copy_ of (read + written) / 2 bytes, device to device' % a.launches)
    say('  %3s %-14s %10s %10s %9s %14s %14s' % ('N', 'planes', 'MB / call', 'us / call', 'GB/s', 'copy us / call', 'launch / copy'))
    for n in ns:
        rng = np.random.default_rng(100 + n)
        d = prediction(n, n)
        v = (d > 40.0).float()
        im = torch.from_numpy(rng.random((n, 3, h, w)).astype(np.float32)).cuda()
        st = (torch.full((n,), SY, dtype=torch.int32).cuda(), torch.full((n,), SX, dtype=torch.int32).cuda())
        for planes, args in (('depth', (d, None, None)), ('all three', (d, v, im))):
            out = egress_raw(*args, dst_size=(H, W), start=st)
            nbytes = sum(t.numel() * 4 for t in args if t is not None) + sum(t.numel() * t.element_size() for t in out.values())
            cargs = ([_lib.ptr(t) for t in args] + [_lib.ptr(out.get(k)) for k in PLANES] + [n, h, w, H, W, _lib.ptr(st[0]), _lib.ptr(st[1]), 256.0, 255.0,
                                                                                              torch.cuda.current_stream().cuda_stream])
            for _ in range(20):
                assert lib.ptta_egress_raw(*cargs) == 0
            us = events(lambda: lib.ptta_egress_raw(*cargs), a.launches)
            src = torch.empty(nbytes // 2 // 16 * 16, dtype=torch.uint8, device='cuda')
            dst = torch.empty_like(src)
            for _ in range(20):
                dst.copy_(src)
            cus = events(lambda: dst.copy_(src), a.launches)
            say('  %3d %-14s %10.2f %10.2f %9.0f %14.2f %14.2f' % (n, planes, nbytes / 1e6, us, nbytes / us / 1e3, cus, us / cus))
            del out, src, dst
        del d, v, im

    # ---- (d): the adapt loop ----
    say()
    say('(d) adapt loop, MSG_CHN (façade defaults), inner_iter = 1, ms per FRAME (ms per call / N): median of %d legs of %d calls [min .. max]; legs alternate' % (a.repeats, a.steps))
    say('  %3s  %-30s %-30s %s' % ('N', 'sink=None', 'sink=RawFrameSink (no writer)', 'sink - none, ms per frame (spread)'))
    loop = {}
    for n in ns:
        model = ExternalModel_Adapt('msg_chn', 0.0, 80.0, max_input_depth=80.0, device=torch.device('cuda'))
        model._prepare_head(MODE)
        model.model.load_state_dict({k: torch.from_numpy(np.asarray(val)) for k, val in synth.formula_state_dict(MODE).items()})
        opt = torch.optim.Adam(model.adapt_parameters(mode='meta'), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
        model.model.set_hparams(w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1)
        model.model.bind_optimizer(opt)
        frames = [[torch.from_numpy(x).cuda() for x in synth.synthetic_frame(s, h, w, n)] for s in range(3)]
        sink = RawFrameSink(n, h, w, H, W)

        def leg(with_sink, count):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(count):
                if with_sink and sink.in_flight() == sink.slots:
                    sink.collect()
                    sink.release()
                model.adapt(*frames[i % 3], inner_iter=1, sink=sink if with_sink else None)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            while sink.in_flight():
                sink.collect()
                sink.release()
            return 1e3 * dt / count / n
        for k in (False, True):
            leg(k, 4)
        res = {False: [], True: []}
        for _ in range(a.repeats):
            for k in (False, True):
                res[k].append(leg(k, a.steps))
        d = statistics.median(res[True]) - statistics.median(res[False])
        spread = max(max(r) - min(r) for r in res.values())
        loop[n] = (d, spread)
        say('  %3d  %-30s %-30s %+.3f (%.3f)' % (n, cell(res[False]), cell(res[True]), d, spread))
        del model, opt, frames, sink
        torch.cuda.empty_cache()
    say()
    say('host-thread time per frame, (b) submit against (a), and what the sink adds to an adapt call (a difference inside the legs\' own spread is called none):')
    for n in ns:
        ha, hb, hc, cus = host[n]
        d, spread = loop[n]
        say('  N=%2d: (a) %.3f ms, (b) submit %.3f ms: submit takes %.1f %% of (a); in the adapt loop the sink adds %s; the slot\'s copy alone is %.3f ms per frame of device time'
            % (n, ha, hb, 100 * hb / ha, 'nothing measurable (%+.3f ms, spread %.3f)' % (d, spread) if abs(d) <= spread else '%+.3f ms per frame (spread %.3f)' % (d, spread),
               cus / 1e3 / n))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
