"""The augmentation of adapt()'s inner loop (proxytta.augment.StepAugmenter; profiles/augment_loop.txt): the one-launch route
(csrc/augment_fused.hip) beside the staged Transforms calls a caller writes by hand, in one process, alternating, after a warm-up.
Nothing is asserted about speed: the tool writes down what it measures.

Workload: 352 x 1216 frames resident in HBM (raw 0..255 image, sparse depth at 5 %, validity map, ground truth), N = 1 and N = 4, the flags
of bash/adapt/adapt_msgchn_vkitti.sh (horizontal flip, rotation <= 5 degrees, resize-and-crop 1.0-1.5, brightness / contrast / saturation
0.6-1.4) at probability 1.0.  Both routes are given the same seeds, so they make the same draws.

  host     wall-clock us per iteration of draw + apply (staged: geo.transform + pho.transform), nothing synchronised inside the batch:
           the time the launch path is held
  device   us between events recorded around apply (around the two transform calls), per iteration
  counts   of ONE iteration, counted while it runs: library calls and the kernel launches they make (each entry point's launch rule),
           host-to-device copies (Tensor.to / Tensor.copy_ from a host tensor), torch.empty / empty_like allocations
  adapt    wall-clock ms per frame of adapt(inner_iter=1) on the MSG_CHN mixed-mode model of bench.py's headline (N = 1): no augmenter;
           the loop by hand (geo.transform, pho.transform, step, eval forward); adapt(augmenter=) on the fused route

    python tools/bench_augment_loop.py [--out FILE] [--repeats 10] [--warmup 2] [--iters 20] [--frames 10]
Fails without a GPU.
"""
import argparse
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
MODES = ['bilinear', 'nearest', 'nearest', 'nearest']
MODE = 'meta_selfsup_seq_1layer_ema'
SEED = 2024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the printed text to this file')
    ap.add_argument('--repeats', type=int, default=10, help='batches per route (after --warmup), the two routes alternating')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=20, help='iterations per batch')
    ap.add_argument('--frames', type=int, default=10, help='adapt calls per batch')
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_augment_loop.py measures on a HIP device and there is none')
    from proxytta import _lib, synth
    from proxytta.augment import StepAugmenter
    from proxytta.model import CANONICAL_LOSS_TYPE, ExternalModel_Adapt
    from proxytta.transforms import Transforms
    lib = _lib.load()
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def cell(v):
        return '%9.2f [%9.2f .. %9.2f]' % (statistics.median(v), min(v), max(v))

    def flags():
        return (Transforms(random_flip_type=['horizontal'], random_rotate_max=5, random_resize_and_crop=[1.0, 1.5]),
                Transforms(random_brightness=[0.6, 1.4], random_contrast=[0.6, 1.4], random_saturation=[0.6, 1.4]))

    def frame(idx, n):
        image01, sparse = synth.synthetic_frame(idx, H, W, n)
        image = torch.from_numpy(np.floor(image01 * 255.0).astype(np.float32)).cuda()
        sparse = torch.from_numpy(sparse).cuda()
        gt = torch.from_numpy(synth.synthetic_frame(idx + 100, H, W, n, density=1.0)[1]).cuda()
        return image, sparse, torch.where(sparse > 0, torch.ones_like(sparse), sparse), gt

    def seed(k):
        torch.manual_seed(SEED + k)
        np.random.seed(SEED + k)

    class Counts(object):
        """What one iteration asks of the runtime, counted at the Python calls that ask for it."""
        LAUNCHES = {'ptta_crop_flip': 1, 'ptta_rotate': 1, 'ptta_resize_crop': 1}

        def __enter__(self):
            self.calls, self.launches, self.copies, self.allocs = [], 0, 0, 0
            self.saved = {name: getattr(lib, name) for name in ('ptta_crop_flip', 'ptta_rotate', 'ptta_resize_crop', 'ptta_photometric_full', 'ptta_augment_frames')}
            for name, fn in self.saved.items():
                setattr(lib, name, self.counted(name, fn))
            self.to, self.copy_, self.empty, self.empty_like = torch.Tensor.to, torch.Tensor.copy_, torch.empty, torch.empty_like
            me = self

            def to(t, *args, **kw):
                out = me.to(t, *args, **kw)
                me.copies += int(not t.is_cuda and out.is_cuda)
                return out

            def copy_(t, src, *args, **kw):
                me.copies += int(t.is_cuda and not src.is_cuda)
                return me.copy_(t, src, *args, **kw)

            def empty(*args, **kw):
                me.allocs += 1
                return me.empty(*args, **kw)

            def empty_like(*args, **kw):
                me.allocs += 1
                return me.empty_like(*args, **kw)
            torch.Tensor.to, torch.Tensor.copy_, torch.empty, torch.empty_like = to, copy_, empty, empty_like
            return self

        def counted(self, name, fn):
            def call(*args):
                self.calls.append(name)
                if name == 'ptta_photometric_full':         # pass 1, and pass 2 when contrast / gamma / hue / saturation is configured
                    self.launches += 1 + int(any(args[k] is not None and getattr(args[k], 'value', args[k]) for k in (7, 9, 11, 13)))
                elif name == 'ptta_augment_frames':         # the frame-set kernel, and pass 2 when the caller asks for it
                    self.launches += 1 + int(bool(args[0]._obj.pass2 and args[0]._obj.image1))
                else:
                    self.launches += self.LAUNCHES[name]
                return fn(*args)
            return call

        def __exit__(self, *exc):
            for name, fn in self.saved.items():
                setattr(lib, name, fn)
            torch.Tensor.to, torch.Tensor.copy_, torch.empty, torch.empty_like = self.to, self.copy_, self.empty, self.empty_like

    say('tools/bench_augment_loop.py --repeats %d --warmup %d --iters %d --frames %d   (%s, torch %s)'
        % (a.repeats, a.warmup, a.iters, a.frames, torch.cuda.get_device_name(0), torch.__version__))
    say('per line: median [min .. max] over %d batches per route, the routes alternating batch by batch; the spread is the bracket' % a.repeats)

    for n in (1, 4):
        image, sparse, valid, gt = frame(0, n)
        geo_f, pho_f = flags()
        geo_s, pho_s = flags()
        aug = StepAugmenter(geo_f, pho_f, MODES)

        def fused_iter():
            aug.draw(n, H, W, 1.0)
            e0.record()
            out = aug.apply(image, sparse, valid, gt)
            e1.record()
            return out

        def staged_iter():
            # (the events bracket the draws too: transform draws and applies in one call; a draw costs the device nothing)
            e0.record()
            out = geo_s.transform([image, sparse, valid, gt], interpolation_modes=MODES, random_transform_probability=1.0)
            [im1] = pho_s.transform([out[0]], random_transform_probability=1.0)
            e1.record()
            return [im1] + list(out)
        res = {'fused': ([], []), 'staged': ([], [])}
        for rep in range(a.warmup + a.repeats):
            for name, it in (('fused', fused_iter), ('staged', staged_iter)):
                seed(rep)
                host, dev = 0.0, 0.0
                for _ in range(a.iters):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    it()
                    host += time.perf_counter() - t0
                    torch.cuda.synchronize()
                    dev += e0.elapsed_time(e1)
                if rep >= a.warmup:
                    res[name][0].append(1e6 * host / a.iters)
                    res[name][1].append(1e3 * dev / a.iters)
        # the same draws give the same frames on both routes
        seed(0)
        f = [t.clone() for t in fused_iter()]
        seed(0)
        s = staged_iter()
        torch.cuda.synchronize()
        equal = all(torch.equal(x, y) for x, y in zip(f, s))
        say()
        say('N = %d, %d x %d, one iteration = one draw of the vkitti flags + its application to image, sparse depth, validity map, ground truth' % (n, H, W))
        say('  outputs of the two routes for the same draw are bit-identical: %s   (route of the augmenter: %s)' % (equal, aug.path))
        for name in ('fused', 'staged'):
            say('  %-6s host us per iteration (draw + apply, not synchronised): %s' % (name, cell(res[name][0])))
            say('  %-6s device us per iteration (events around apply):          %s' % (name, cell(res[name][1])))
        say('  staged / fused, medians: host %.2f, device %.2f' % (statistics.median(res['staged'][0]) / statistics.median(res['fused'][0]),
                                                                    statistics.median(res['staged'][1]) / statistics.median(res['fused'][1])))
        for name, it in (('fused', fused_iter), ('staged', staged_iter)):
            tally = []
            for k in range(8):                   # the counts depend on the draw (pass 2 runs when contrast or saturation came up)
                seed(100 + k)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with Counts() as c:
                    it()
                tally.append((len(c.calls), c.launches, c.copies, c.allocs))
            torch.cuda.synchronize()
            say('  %-6s over 8 draws: library calls %d..%d, kernel launches %d..%d, host-to-device copies %d..%d, torch.empty allocations %d..%d'
                % ((name,) + tuple(v for col in zip(*tally) for v in (min(col), max(col)))))

    # ---- adapt(inner_iter=1), the headline's model ----
    def make_model():
        model = ExternalModel_Adapt('msg_chn', 0.0, 80.0, max_input_depth=80.0, device=torch.device('cuda'), dtype='mixed')
        model._prepare_head(MODE)
        model.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.formula_state_dict(MODE).items()})
        opt = torch.optim.Adam(model.adapt_parameters(mode='meta'), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
        model.model.set_hparams(w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1)
        model.model.bind_optimizer(opt)
        model.set_image_norm([0, 1])
        return model
    n = 1
    frames = [frame(i, n) for i in range(4)]
    model = make_model()
    geo_s, pho_s = flags()
    aug = StepAugmenter(*flags(), MODES)

    def plain(i):
        image, sparse, valid, gt = frames[i % 4]
        return model.adapt(image, sparse, inner_iter=1, validity_map=valid)

    def by_hand(i):
        image, sparse, valid, gt = frames[i % 4]
        model.train()
        out = geo_s.transform([image, sparse, valid, gt], interpolation_modes=MODES, random_transform_probability=1.0)
        [im1] = pho_s.transform([out[0]], random_transform_probability=1.0)
        info, _ = model.step(im1, out[1], out[2], loss_image=out[0])
        model.eval()
        return model.forward(image, sparse, loss_type=CANONICAL_LOSS_TYPE), info

    def with_augmenter(i):
        image, sparse, valid, gt = frames[i % 4]
        return model.adapt(image, sparse, inner_iter=1, validity_map=valid, augmenter=aug, augmentation_probability=1.0)

    legs = (('no augmenter', plain), ('staged loop by hand', by_hand), ('adapt(augmenter=), the fused route', with_augmenter))
    t = {name: [] for name, _ in legs}
    for rep in range(a.warmup + a.repeats):
        for name, fn in legs:
            seed(rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.frames):
                fn(i)
            torch.cuda.synchronize()
            if rep >= a.warmup:
                t[name].append(1e3 * (time.perf_counter() - t0) / a.frames)
    say()
    say('adapt(inner_iter=1), MSG_CHN mixed mode, N = 1, %d x %d: wall-clock ms per frame over %d frames and one synchronisation' % (H, W, a.frames))
    for name, _ in legs:
        say('  %-36s %s' % (name, cell(t[name])))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
