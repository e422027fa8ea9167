"""Golden vectors of the reference's summary panels: the REAL ExternalModel_Adapt.log_summary (src/external_model_adapt.py:662-909) and the
REAL log_utils.colorize (src/log_utils.py:53-80), imported in place and run on the CPU in the build container, with a recording writer
in place of tensorboard's SummaryWriter.  Nothing of the reference is copied.  Harness-side shims only:
  * `self` is a bare object carrying max_predict_depth (log_summary reads nothing else of it);
  * torchvision is absent from this image: `make_grid` and `normalize` below are stand-ins for torchvision.utils.make_grid and
    torchvision.transforms.functional.normalize, written here from their documented behaviour (make_grid: a single image is returned
    as it is; otherwise a grid of ceil(n / nrow) rows of min(nrow, n) cells, each cell `padding` larger than an image, `padding` more on
    the far edges, filled with pad_value; normalize: (tensor - mean[c]) / std[c] out of place, mean and std converted to the tensor's dtype);
  * log_utils.colorize calls plt.cm.get_cmap, which matplotlib 3.9 removed: the name is pointed at matplotlib.colormaps[...], the
    registry it was an alias of.
The inputs come from tests/summary_cases.py (CASES: each subset of optional inputs that changes the row list, image lists, a maximum above
10, mean/std and [0, 1] ranges, depths on and next to the colormap's bin boundaries, values below 0, above max_predict_depth, NaN, +-inf,
validity 0, validity > 0 over depth 0, ground-truth zeros).  Per case tests/golden/summary_<name>.npz holds the inputs, every add_image
tag and grid, the scalar and histogram tags, and the two 256 x 3 colormap tables (matplotlib's `.colors`).
Usage:  python tests/golden/make_golden_summary.py
"""
import json
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
sys.path.insert(0, ROOT)


def make_grid(tensor, nrow=8, padding=2, pad_value=0.0):
    if tensor.dim() == 4 and tensor.size(1) == 1:
        tensor = torch.cat((tensor, tensor, tensor), 1)
    if tensor.size(0) == 1:
        return tensor.squeeze(0)
    nmaps = tensor.size(0)
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height, width = int(tensor.size(2) + padding), int(tensor.size(3) + padding)
    grid = tensor.new_full((tensor.size(1), height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid[:, y * height + padding:(y + 1) * height, x * width + padding:(x + 1) * width].copy_(tensor[k])
            k += 1
    return grid


def normalize(tensor, mean, std):
    mean = torch.as_tensor(mean, dtype=tensor.dtype).view(-1, 1, 1)
    std = torch.as_tensor(std, dtype=tensor.dtype).view(-1, 1, 1)
    return tensor.clone().sub_(mean).div_(std)


def import_reference():
    import matplotlib
    matplotlib.use('Agg')
    from matplotlib import pyplot as plt
    if not hasattr(plt.cm, 'get_cmap'):
        plt.cm.get_cmap = lambda name: matplotlib.colormaps[name]
    tv = types.ModuleType('torchvision')
    tv.utils = types.ModuleType('torchvision.utils')
    tv.transforms = types.ModuleType('torchvision.transforms')
    tv.transforms.functional = types.ModuleType('torchvision.transforms.functional')
    tv.utils.make_grid = make_grid
    tv.transforms.functional.normalize = normalize
    for name, mod in (('torchvision', tv), ('torchvision.utils', tv.utils), ('torchvision.transforms', tv.transforms),
                      ('torchvision.transforms.functional', tv.transforms.functional)):
        sys.modules.setdefault(name, mod)
    sys.path.insert(0, os.path.join(REF, 'src'))
    import external_model_adapt
    import log_utils
    return external_model_adapt, log_utils


class Recorder(object):
    def __init__(self):
        self.images, self.scalars, self.histograms = [], [], []

    def add_image(self, tag, img, global_step=None):
        self.images.append((tag, img.numpy().copy(), global_step))

    def add_scalar(self, tag, value, global_step=None):
        self.scalars.append((tag, float(value), global_step))

    def add_histogram(self, tag, values, global_step=None):
        self.histograms.append((tag, global_step))


def main():
    import matplotlib
    from tests import summary_cases as C
    ema, log_utils = import_reference()
    tables = {name: np.asarray(matplotlib.colormaps[name].colors, dtype=np.float64) for name in ('viridis', 'inferno')}
    # the tables are what colorize looks values up in: entry k for (k + 0.5) / 256
    probe = torch.from_numpy(((np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(256)).reshape(1, 1, 16, 16))
    for name, table in tables.items():
        got = log_utils.colorize(probe, colormap=name).numpy()[0].reshape(3, 256).T
        assert table.shape == (256, 3) and np.array_equal(got, table.astype(np.float32)), name
    total = 0
    for case in C.CASES:
        images, maps = C.case_inputs(case)
        shim = types.SimpleNamespace(max_predict_depth=case['maxd'])
        rec = Recorder()
        step = 7 + len(case['name'])
        t_images = [torch.from_numpy(a.copy()) for a in images]
        image = None if not t_images else (t_images if case['as_list'] else t_images[0])
        assert case['as_list'] or len(t_images) <= 1
        with np.errstate(all='ignore'):
            ema.ExternalModel_Adapt.log_summary(shim, rec, 'tag-' + case['name'], step, image=image, output_image=None,
                                                normalized_image_range=case['rng_range'], scalars=dict(C.SCALARS),
                                                n_image_per_summary=case['nips'],
                                                **{k: torch.from_numpy(v.copy()) for k, v in maps.items()})
        assert all(s == step for _, _, s in rec.images + rec.scalars) and all(s == step for _, s in rec.histograms)
        meta = dict(case, step=step, tag='tag-' + case['name'], image_tags=[t for t, _, _ in rec.images],
                    scalar_tags=[t for t, _, _ in rec.scalars], scalar_values=[v for _, v, _ in rec.scalars],
                    histogram_tags=[t for t, _ in rec.histograms])
        arrays = {'image%d' % k: a for k, a in enumerate(images)}
        arrays.update(maps)
        arrays.update({'grid%d' % k: g for k, (_, g, _) in enumerate(rec.images)})
        arrays.update(tables)
        for k, (_, g, _) in enumerate(rec.images):
            assert g.dtype == np.float32 and g.ndim == 3 and g.shape[0] == 3, (case['name'], k, g.shape, g.dtype)
        path = C.fixture_path(HERE, case['name'])
        np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
        total += os.path.getsize(path)
        print(case['name'], meta['image_tags'], [g.shape for _, g, _ in rec.images], os.path.getsize(path), 'bytes')
    print(len(C.CASES), 'cases', total, 'bytes')


if __name__ == '__main__':
    main()
