"""log_summary's panels composed on the device (include/ptta.h ptta_summary_compose, proxytta.summary, ExternalModel_Adapt.log_summary;
profiles/summary_device.txt) beside the host path the reference's log_summary takes, on one box.  Nothing is asserted about speed: the
tool writes down what it measures.

Workload: N = 4 frames of 352 x 1216 resident in HBM -- one image (0 .. 255, mean/std range), output depth, sparse depth, validity map,
ground truth -- shown with n_image_per_summary 1 and 4: both grids of one call (the image grid, one row; the depth grid, image + output +
sparse + ground-truth rows).

  host      wall-clock ms of a reference-style host path, from the device tensors to the two grid tensors a writer would be handed:
            the max test, the display transform and the error maps in torch, the maps to the CPU, matplotlib's colormaps per sample,
            torch.cat, make_grid (written here from torchvision's documented behaviour).  Twice, as the driver's two call sites do it:
            with the torch arithmetic on the device tensors, and with every tensor moved to the CPU first (the copies inside the timed
            window).  `--host-repeats` runs, median [min .. max].  Needs matplotlib.  The two differ in some elements -- torch's
            division on the device is not the CPU's in the last bit -- and the count is printed; the device path is compared with the CPU form.
  device    wall-clock ms of ExternalModel_Adapt.log_summary with a writer that drops what it is given, image_dtype 'float32' and
            'uint8': uploads nothing (the tensors are resident), the flag launches, two compose launches, one device -> host copy per
            grid.  `--repeats` runs after `--warmup`, median [min .. max].  The grids are compared with the host path's (it says whether they are equal).
  launch    device events around the depth grid's compose launch alone (the larger of the two), both forms, beside a plain
            device-to-device copy of the same number of bytes (torch's copy_ of a tensor of the grid's shape), and around
            ptta_summary_image_flag (its two launches) on the whole N x 3 x H x W image.  Bytes written / time for the compose launch.

    python tools/bench_summary.py [--out FILE] [--repeats 20] [--warmup 3] [--host-repeats 5]
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

N, H, W = 4, 352, 1216
RANGE = [0.485, 0.456, 0.406, 0.229, 0.224, 0.225]
MAXD = 80.0


class NullWriter(object):
    def add_image(self, tag, img, global_step=None, **kw):
        self.last = img

    def add_scalar(self, *a, **k):
        pass

    def add_histogram(self, *a, **k):
        pass


def host_path(torch, np, cmaps, image, maps, nips):
    """A reference-style host path: the two grids as CPU tensors."""
    def colour(t, name):
        a = t.cpu().numpy()[:, 0]
        return torch.from_numpy(np.stack([np.transpose(cmaps[name](a[k])[..., :3], (2, 0, 1)) for k in range(a.shape[0])]).astype(np.float32))

    def grid(panels):
        n, c, ph, pw = panels.shape
        if n == 1:
            return panels[0]
        g = panels.new_zeros((c, ph + 4, n * (pw + 2) + 2))
        for k in range(n):
            g[:, 2:2 + ph, k * (pw + 2) + 2:k * (pw + 2) + 2 + pw] = panels[k]
        return g
    with torch.no_grad():
        if torch.max(image) > 10.0:
            image = image / 255.0
        mean = torch.tensor([-m / s for m, s in zip(RANGE[:3], RANGE[3:])], device=image.device).view(1, 3, 1, 1)
        std = torch.tensor([1 / s for s in RANGE[3:]], device=image.device).view(1, 3, 1, 1)
        shown = ((image - mean) / std)[:nips].cpu()
        row_image = torch.cat([shown, torch.zeros_like(shown)], dim=-1)
        out, sparse, valid, gt = (maps[k][:nips] for k in ('output_depth', 'sparse_depth', 'validity_map', 'ground_truth'))
        left = colour(out / MAXD, 'viridis')
        rows = [row_image, torch.cat([left, torch.zeros_like(left)], dim=3)]
        err = torch.where(valid > 0, torch.abs(out - sparse) / (sparse + 1e-8), valid)
        rows.append(torch.cat([colour(sparse / MAXD, 'viridis'), colour(err / 0.05, 'inferno')], dim=3))
        err = torch.where(gt > 0, (torch.abs(out - gt) + 1e-8) / (gt + 1e-8), torch.zeros_like(gt))
        rows.append(torch.cat([colour(gt / MAXD, 'viridis'), colour(err / 0.05, 'inferno')], dim=3))
        return grid(row_image), grid(torch.cat(rows, dim=2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the printed text to this file')
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-repeats', type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_summary.py measures on a HIP device and there is none')
    import matplotlib
    from proxytta import _lib, summary
    from proxytta.model import ExternalModel_Adapt
    from tests import summary_cases as C
    lib = _lib.load()
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def cell(v):
        return '%9.3f [%9.3f .. %9.3f]' % (statistics.median(v), min(v), max(v))

    def events(fn, burst=20):
        """ms per call by device events around `burst` back-to-back calls of fn() (the queue stays fed: the figure is the launches', not
        the host's), `--repeats` bursts after `--warmup`"""
        t = []
        for i in range(a.warmup + a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(burst):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                t.append(e0.elapsed_time(e1) / burst)
        return t
    say('tools/bench_summary.py --repeats %d --warmup %d --host-repeats %d   (%s, torch %s, matplotlib %s)'
        % (a.repeats, a.warmup, a.host_repeats, torch.cuda.get_device_name(0), torch.__version__, matplotlib.__version__))
    images, maps_np = C.generated_inputs(('bench', N, (H, W), 4, ('raw',), 'osvg'), MAXD)
    image = torch.from_numpy(images[0]).cuda()
    maps = {k: torch.from_numpy(v).cuda() for k, v in maps_np.items()}
    cmaps = {name: matplotlib.colormaps[name] for name in ('viridis', 'inferno')}
    model = object.__new__(ExternalModel_Adapt)              # log_summary reads max_predict_depth and device only: no network is built
    model.max_predict_depth, model.device = MAXD, torch.device('cuda')
    say('workload: N = %d, %d x %d, image 0 .. 255 with a mean/std range, output + sparse + validity + ground truth, all resident' % (N, H, W))
    for nips in (1, 4):
        gh, gw = summary.grid_shape(min(N, nips), H, W, 4)
        ih, iw = summary.grid_shape(min(N, nips), H, W, 1)
        say()
        say('n_image_per_summary = %d: image grid 3 x %d x %d, depth grid 3 x %d x %d (%.1f MB fp32, %.1f MB uint8)'
            % (nips, ih, iw, gh, gw, 12e-6 * gh * gw, 3e-6 * gh * gw))
        t_host, t_cpu, w_last = [], [], {}
        for _ in range(a.host_repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want_dev = host_path(torch, np, cmaps, image, maps, nips)
            t_host.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            want = host_path(torch, np, cmaps, image.cpu(), {k: v.cpu() for k, v in maps.items()}, nips)
            t_cpu.append(1e3 * (time.perf_counter() - t0))
        say('  host path, arithmetic on the device tensors (src/tta_main.py:738-751), wall-clock ms, median [min .. max] of %d:  %s'
            % (a.host_repeats, cell(t_host)))
        say('  host path, tensors moved to the CPU first (src/tta_main.py:637-654), wall-clock ms:                              %s   '
            '(%d elements of its depth grid differ from the line above: torch\'s arithmetic on the device against the CPU\'s)'
            % (cell(t_cpu), int((want[1] != want_dev[1]).sum())))
        for image_dtype in ('float32', 'uint8'):
            w = NullWriter()
            t_dev = []
            for i in range(a.warmup + a.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.log_summary(w, 'bench', i, image=[image], normalized_image_range=RANGE, scalars={}, n_image_per_summary=nips,
                                  image_dtype=image_dtype, **maps)
                t_dev.append(1e3 * (time.perf_counter() - t0))
            t_dev = t_dev[a.warmup:]
            ref = want[1] if image_dtype == 'float32' else (want[1] * 255).clip(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()
            w_last[image_dtype] = w.last
            differ = int((w.last != ref).sum())
            say('  log_summary(image_dtype=%-9r), wall-clock ms, of %d after %d:  %s   host paths / this (medians) = %.1f, %.1f; %s'
                % (image_dtype, a.repeats, a.warmup, cell(t_dev), statistics.median(t_host) / statistics.median(t_dev),
                   statistics.median(t_cpu) / statistics.median(t_dev),
                   'depth grid equal to the CPU host path\'s' if differ == 0 else '%d elements of the depth grid DIFFER from the CPU host path\'s' % differ))
        flag = summary.image_flag(image)
        tables = {name: summary.colormap_table(name) for name in ('viridis', 'inferno')}
        rev = summary.reverse_normalization(RANGE)
        stream = torch.cuda.current_stream().cuda_stream
        for image_dtype, shape, dtype, size in (('float32', (3, gh, gw), torch.float32, 4), ('uint8', (gh, gw, 3), torch.uint8, 1)):
            out, src = torch.empty(shape, dtype=dtype, device='cuda'), torch.zeros(shape, dtype=dtype, device='cuda')
            k = _lib.SummaryArgs()                               # the depth grid's call, built once: the burst below is launches only
            k.n_show, k.height, k.width, k.n_images, k.normalize, k.max_predict_depth = min(N, nips), H, W, 1, 1, MAXD
            k.rows = _lib.PTTA_SUMMARY_ROW_OUTPUT | _lib.PTTA_SUMMARY_ROW_SPARSE | _lib.PTTA_SUMMARY_ROW_GT
            k.out_dtype = _lib.PTTA_SUMMARY_OUT_U8_HWC if image_dtype == 'uint8' else _lib.PTTA_SUMMARY_OUT_F32_CHW
            k.rev_mean[:], k.rev_std[:] = rev
            k.image[0], k.image_div255[0] = image.data_ptr(), flag.data_ptr()
            for name, t in list(maps.items()) + list(tables.items()) + [('out', out)]:
                setattr(k, name, t.data_ptr())

            def launch():
                if lib.ptta_summary_compose(ctypes.byref(k), stream) != 0:
                    raise SystemExit('ptta_summary_compose failed')
            launch()
            if not torch.equal(out.cpu(), w_last[image_dtype]):
                raise SystemExit('the bare launch and log_summary disagree')
            t_k = events(launch)
            t_c = events(lambda: out.copy_(src))
            nbytes = 3 * gh * gw * size
            say('  compose launch alone (%-7s), device events, ms:  %s   %.0f GB/s written;  device-to-device copy of its %.1f MB: %s   compose / copy = %.2f'
                % (image_dtype, cell(t_k), nbytes / statistics.median(t_k) / 1e6, nbytes / 1e6, cell(t_c), statistics.median(t_k) / statistics.median(t_c)))
    t_f = events(lambda: summary.image_flag(image, flag=flag))
    say()
    say('ptta_summary_image_flag on the whole %d x 3 x %d x %d image (%.1f MB read, two launches), device events, ms: %s   %.0f GB/s read'
        % (N, H, W, 4e-6 * image.numel(), cell(t_f), 4 * image.numel() / statistics.median(t_f) / 1e6))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
