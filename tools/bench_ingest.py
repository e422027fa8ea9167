"""Raw-frame ingest (include/ptta.h ptta_ingest_raw, proxytta.staging.RawFrameStager; profiles/ingest_raw.txt): what the kernel moves per
second, and what a host-fed adapt loop costs per frame when the frames start out as decoded uint8 / 16-bit arrays.

One process, the MSG_CHN mixed engine as bench.py builds it, seeded raw arrays; sources 375x1242 -> window 352x1216 and 480x640 uncropped,
N = 1, 8 and 16 frames per call.

  kernel     one pair of device events around `--launches` calls of the entry point (through ctypes, arguments prepared once) after a
             warm-up, on the planes RawFrameStager asks for (image + sparse:
             5 bytes read and 16 written per window pixel) and on all of them (7 read, 28 written); bytes read + written over that time,
             beside the 6.29 TB/s a float4 copy reaches on this chip.  The buffers of one call (at most 240 MB) fit the 256 MiB Infinity
             Cache, and a run of launches re-reads and re-writes the same ones: the rate is that of a warm last-level cache, not of HBM.
  host loop  ms per frame of  submit(k+1); acquire(); step(k, next_frame = peek_next); release()  fed three ways, the legs alternating
             and each repeated `--repeats` times (host clock around a leg that ends in a device synchronise):
               (i)   RawFrameStager fed the raw arrays
               (ii)  FrameStager fed fp32 frames made IN the loop from the same raw arrays by the reference's host arithmetic, on the one
                     host thread: np.asarray(image, np.float32) transposed to CHW, z / 256.0 with z[z <= 0] = 0, per sample, then the crop
                     and the collation (src/data_utils.py:150-158, :219-223, src/datasets.py:83-170) -- the path (i) replaces
               (iii) FrameStager fed ready-made fp32 frames (bench.py's from_host_memory figure: the host arithmetic is not in the loop)
             and the same steps on frames resident in HBM, for the gap.

    python tools/bench_ingest.py [--out FILE] [--steps 40] [--repeats 3] [--launches 300] [--ns 1,8,16]
    python tools/bench_ingest.py --resources       hipcc's kernel-resource-usage remarks for csrc/ingest.hip (compiles only: needs no GPU)
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
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1, max_input_depth=80.0)
SHAPES = (((375, 1242), (352, 1216), (23, 13)), ((480, 640), (480, 640), (0, 0)))
COPY_RATE = 6.29e12            # MI355X: float4 copy, measured


def resources():
    """The remarks of `hipcc -Rpass-analysis=kernel-resource-usage` for csrc/ingest.hip with csrc/Makefile's flags, one line per kernel."""
    src = os.path.join(ROOT, 'tta-depth-completion_amd', 'csrc', 'ingest.hip')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-fPIC', '-std=c++17', '-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', os.devnull],
                       capture_output=True, text=True, check=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            f = re.search(r'ingest_raw_kernelILb(\d)ELb(\d)ELb(\d)ELb(\d)E', m.group(1))
            cur = {'name': 'ingest_raw_kernel<%s; %s>' % ('16-byte stores' if f.group(1) == '1' else 'one pixel per lane',
                                                          ' + '.join(k for k, on in zip(('image', 'sparse', 'gt'), f.groups()[1:]) if on == '1'))}
            rows.append(cur)
        m = re.search(r'(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)', line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    out = ['hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage, csrc/ingest.hip (compiled, not run):',
           '  %-62s %5s %5s %8s %10s %10s %9s' % ('kernel', 'VGPR', 'SGPR', 'scratch', 'SGPR spill', 'VGPR spill', 'waves/SIMD')]
    for c in rows:
        out.append('  %-62s %5d %5d %8d %10d %10d %9d' % (c['name'], c['VGPRs'], c['TotalSGPRs'], c['ScratchSize [bytes/lane]'], c['SGPRs Spill'],
                                                        c['VGPRs Spill'], c['Occupancy [waves/SIMD]']))
    out.append('  scratch bytes per lane over all %d kernels: max %d; LDS: %d' % (len(rows), max(c['ScratchSize [bytes/lane]'] for c in rows),
                                                                            max(c['LDS Size [bytes/block]'] for c in rows)))
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the printed text to this file')
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--launches', type=int, default=300)
    ap.add_argument('--ns', default='1,8,16')
    ap.add_argument('--resources', action='store_true')
    a = ap.parse_args()
    if a.resources:
        print(resources())
        return
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_ingest.py measures on a HIP device and there is none (only --resources runs without one)')
    from proxytta import synth
    from proxytta.engine import ADAPTED, Engine
    from proxytta import _lib
    from proxytta.ingest import PLANES, ingest_raw
    from proxytta.staging import FrameStager, RawFrameStager
    lib = _lib.load()
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)
    say('tools/bench_ingest.py --steps %d --repeats %d --launches %d   (%s, torch %s)' % (a.steps, a.repeats, a.launches, torch.cuda.get_device_name(0), torch.__version__))
    ns = [int(v) for v in a.ns.split(',')]

    def raw_set(seed, n, H, W):
        rng = np.random.default_rng(seed)
        image = rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
        sparse = (rng.integers(256, 80 * 256, size=(n, H, W)) * (rng.random((n, H, W)) < 0.05)).astype(np.uint16)
        return image, sparse

    def reference_host_arithmetic(image, sparse, h, w, sy, sx):
        """the loader's per-sample work and the collation, as the reference does them on the host"""
        ims, zs = [], []
        for b in range(image.shape[0]):
            im = np.transpose(np.asarray(image[b], np.float32), (2, 0, 1))
            z = np.array(sparse[b], dtype=np.float32)
            z = z / 256.0
            z[z <= 0] = 0.0
            ims.append(im[:, sy:sy + h, sx:sx + w])
            zs.append(np.expand_dims(z, 0)[:, sy:sy + h, sx:sx + w])
        return np.stack(ims), np.stack(zs)

    # ---- kernel ----
    say()
    say('kernel: %d launches between two device events, after 20 warm-up launches; GB/s = (bytes read + bytes written) / time' % a.launches)
    say('  %-22s %3s %-16s %10s %10s %9s %12s' % ('source -> window', 'N', 'planes', 'MB / call', 'us / call', 'GB/s', '/ 6.29 TB/s'))
    for (H, W), (h, w), (sy, sx) in SHAPES:
        for n in ns:
            image, sparse = raw_set(n, n, H, W)
            im, sp = torch.from_numpy(image).cuda(), torch.from_numpy(sparse.view(np.int16)).cuda()
            st = (torch.full((n,), sy, dtype=torch.int32).cuda(), torch.full((n,), sx, dtype=torch.int32).cuda())
            for planes, args, per_px in (('image + sparse', (im, sp, None), 5 + 16), ('all five', (im, sp, sp), 7 + 28)):
                out = ingest_raw(*args, size=(h, w), start=st)
                if planes == 'image + sparse':
                    del out['validity']
                # the entry point itself, arguments prepared once: the Python wrapper's checks cost more host time than a small call runs
                cargs = ([_lib.ptr(t) for t in args] + [_lib.ptr(out.get(k)) for k in PLANES] + [n, H, W, h, w, _lib.ptr(st[0]), _lib.ptr(st[1]), 256.0,
                                                                                                  torch.cuda.current_stream().cuda_stream])
                for _ in range(20):
                    assert lib.ptta_ingest_raw(*cargs) == 0
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.launches):
                    lib.ptta_ingest_raw(*cargs)
                e1.record()
                torch.cuda.synchronize()
                us = 1e3 * e0.elapsed_time(e1) / a.launches
                nbytes = n * h * w * per_px
                say('  %-22s %3d %-16s %10.2f %10.2f %9.0f %11.1f %%' % ('%dx%d -> %dx%d' % (H, W, h, w), n, planes, nbytes / 1e6, us, nbytes / us / 1e3,
                                                                     100 * nbytes / (us * 1e-6) / COPY_RATE))
            del im, sp, out
    # ---- host-fed loop ----
    say()
    say('host-fed loop, MSG_CHN mixed, ms per FRAME (ms per call / N): median of %d legs of %d calls [min .. max]; legs alternate (i), (ii), (iii), resident' % (a.repeats, a.steps))
    say('  %-22s %3s  %-26s %-26s %-26s %-26s %s' % ('source -> window', 'N', '(i) RawFrameStager', '(ii) host arithmetic + FS', '(iii) ready fp32 + FS', 'resident in HBM',
                                                     'MB sent per call (i) / (ii),(iii)'))
    verdicts = []
    for (H, W), (h, w), (sy, sx) in SHAPES:
        for n in ns:
            eng = Engine(n, h, w, dtype='mixed', **HP)
            sd = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in synth.formula_state_dict(MODE).items()}
            eng.load_state_dict(sd)
            for name in ADAPTED:
                eng.bind_adapted(name, sd[name], torch.zeros_like(sd[name]), torch.zeros_like(sd[name]))
            nsets = 4
            raws = [raw_set(1000 + 16 * i, n, H, W) for i in range(nsets)]
            ready = [reference_host_arithmetic(im, sp, h, w, sy, sx) for im, sp in raws]
            ready = [(np.ascontiguousarray(x), np.ascontiguousarray(z)) for x, z in ready]
            resident = [[torch.from_numpy(x).cuda() for x in fr] for fr in ready]
            raw_st, fs = RawFrameStager(n, H, W, h, w), FrameStager(n, h, w)

            def feed(kind, i):
                im, sp = raws[i % nsets]
                if kind == 'raw':
                    raw_st.submit(im, sp, start=(sy, sx))
                elif kind == 'host':
                    fs.submit(*reference_host_arithmetic(im, sp, h, w, sy, sx))
                else:
                    fs.submit(*ready[i % nsets])

            def leg(kind, count):
                if kind == 'resident':
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(count):
                        eng.step(*resident[i % nsets], next_frame=resident[(i + 1) % nsets])
                    torch.cuda.synchronize()
                    return 1e3 * (time.perf_counter() - t0) / count / n
                st = raw_st if kind == 'raw' else fs
                feed(kind, 0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(count):
                    feed(kind, i + 1)
                    fr = st.acquire()
                    eng.step(fr[0], fr[1], next_frame=st.peek_next(eng.prefix_stream()))
                    st.release()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                st.acquire(); st.release()                         # the frame submitted ahead of the last call
                return 1e3 * dt / count / n
            kinds = ('raw', 'host', 'ready', 'resident')
            for k in kinds:
                leg(k, 4)                                          # warm-up: every shape and path the timed legs use
            res = {k: [] for k in kinds}
            for _ in range(a.repeats):
                for k in kinds:
                    res[k].append(leg(k, a.steps))

            def cell(v):
                return '%7.3f [%6.3f .. %6.3f]' % (statistics.median(v), min(v), max(v))
            say('  %-22s %3d  %-26s %-26s %-26s %-26s %.2f / %.2f' % ('%dx%d -> %dx%d' % (H, W, h, w), n, cell(res['raw']), cell(res['host']), cell(res['ready']),
                                                                    cell(res['resident']), raw_st.bytes_per_frame / 1e6, fs.bytes_per_frame / 1e6))
            verdicts.append(((H, W), n, res))
            eng.close()
            del eng, sd, resident, raw_st, fs
            torch.cuda.empty_cache()
    say()
    say('(i) against (ii), and the gap to the resident rate, from the legs above (a difference inside the legs\' own spread is called none):')
    for (H, W), n, res in verdicts:
        med = {k: statistics.median(v) for k, v in res.items()}

        def spread(*kinds):                                        # the widest min .. max among the legs a statement compares
            return max(max(res[k]) - min(res[k]) for k in kinds)
        d = med['raw'] - med['host']
        word = 'neither slower nor faster than' if abs(d) <= spread('raw', 'host') else ('FASTER than' if d < 0 else 'SLOWER than')
        gap_raw, gap_ready = med['raw'] - med['resident'], med['ready'] - med['resident']
        gs = spread('raw', 'ready', 'resident')
        gword = 'keeps' if abs(gap_raw - gap_ready) <= gs else ('narrows' if gap_raw < gap_ready else 'widens')
        say('  %dx%d N=%2d: (i) - (ii) = %+.3f ms/frame (spread %.3f): (i) is %s (ii); gap to resident: (i) %+.3f, (iii) %+.3f (spread %.3f): raw ingest %s the gap'
            % (H, W, n, d, spread('raw', 'host'), word, gap_raw, gap_ready, gs, gword))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
