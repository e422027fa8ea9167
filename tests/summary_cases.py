"""The numpy restatement of ptta_summary_compose / log_summary's panels (src/external_model_adapt.py:662-909, src/log_utils.py:53-80,
torchvision.utils.make_grid), the fixture cases tests/golden/make_golden_summary.py records with the REAL reference, and the generated
inputs of the GPU tests.  tests/test_summary_cpu.py holds the restatement to the fixtures with np.array_equal; tests/test_gpu_summary.py
holds the library to both with torch.equal.  Every operation below is one correctly rounded fp32 operation on float32 arrays, as in the
reference's torch expressions."""
import json
import os

import numpy as np

F = np.float32
MEAN_STD = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))

# name, N, (H, W), n_image_per_summary, images, maps given, normalized_image_range, max_predict_depth
#   images: a tuple of image kinds, () = no image; 'unit' = values in [0, 1), 'raw' = 0 .. 255 (maximum above 10), 'late' = above 10 only in the LAST
#   sample (beyond the shown ones), 'nan' = raw with one NaN in the last sample (torch.max gives NaN: not divided); as_list: hand the images over as a list
CASES = [
    dict(name='full_n1_list', n=1, size=(6, 8), nips=1, images=('raw',), as_list=True, maps='osvg', rng_range=MEAN_STD, maxd=8.0),
    dict(name='full_n2_nips2', n=2, size=(5, 7), nips=2, images=('unit',), as_list=False, maps='osvg', rng_range=[0, 1], maxd=5.0),
    dict(name='nips_above_n_list2', n=2, size=(6, 8), nips=4, images=('raw', 'unit'), as_list=True, maps='osvg',
         rng_range=[0.485, 0.456, 0.406, 0.229, 0.224, 0.225], maxd=80.0),
    dict(name='n_above_nips_late_max', n=3, size=(5, 7), nips=2, images=('late',), as_list=False, maps='osvg', rng_range=MEAN_STD, maxd=8.0),
    dict(name='n3_nips3', n=3, size=(6, 8), nips=3, images=('unit',), as_list=True, maps='osvg', rng_range=MEAN_STD, maxd=10.0),
    dict(name='image_only', n=2, size=(6, 8), nips=4, images=('raw',), as_list=False, maps='', rng_range=MEAN_STD, maxd=8.0),
    dict(name='image_list2_only', n=1, size=(5, 7), nips=1, images=('unit', 'raw'), as_list=True, maps='', rng_range=[0, 1], maxd=8.0),
    dict(name='output_only', n=2, size=(5, 7), nips=2, images=(), as_list=False, maps='o', rng_range=[0, 1], maxd=8.0),
    dict(name='image_output', n=2, size=(6, 8), nips=2, images=('unit',), as_list=False, maps='o', rng_range=[0, 1], maxd=5.0),
    dict(name='no_ground_truth', n=2, size=(6, 8), nips=2, images=('raw',), as_list=True, maps='osv', rng_range=MEAN_STD, maxd=8.0),
    dict(name='no_sparse', n=1, size=(6, 8), nips=1, images=('unit',), as_list=True, maps='og', rng_range=MEAN_STD, maxd=8.0),
    dict(name='sparse_without_validity', n=2, size=(5, 7), nips=2, images=('unit',), as_list=False, maps='osg', rng_range=[0, 1], maxd=8.0),
    dict(name='maps_without_output', n=2, size=(5, 7), nips=2, images=('unit',), as_list=False, maps='svg', rng_range=[0, 1], maxd=8.0),
    dict(name='no_image_all_maps', n=1, size=(6, 8), nips=1, images=(), as_list=False, maps='osvg', rng_range=[0, 1], maxd=80.0),
    dict(name='image_nan', n=3, size=(6, 8), nips=2, images=('nan',), as_list=False, maps='o', rng_range=MEAN_STD, maxd=8.0),
]
SCALARS = {'loss': 0.5, 'loss_smooth': 0.125, 'mae': 123.25}
MAP_KEYS = {'o': 'output_depth', 's': 'sparse_depth', 'v': 'validity_map', 'g': 'ground_truth'}


def fixture_path(golden_dir, name):
    return os.path.join(golden_dir, 'summary_%s.npz' % name)


def neighbours(v):
    v = F(v)
    return [np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]


def make_image(rng, kind, n, h, w):
    img = rng.random((n, 3, h, w)).astype(F)
    if kind in ('raw', 'nan'):
        img = np.floor(img * F(256)).astype(F)
        img[0, 0, 0, 0], img[0, 1, 0, 1] = 255.0, 0.0
    elif kind == 'late':
        img[-1, 2, -1, -1] = 200.0                      # above 10 in the last sample only: the WHOLE tensor decides
    else:
        img[0, 0, 0, 0], img[0, 1, 0, 1], img[0, 2, 0, 2] = 0.0, 1.0, 10.0          # exactly 10 is not above 10
    if kind == 'nan':
        img[-1, 1, 2, 3] = np.nan
    return img


def make_maps(rng, n, h, w, maxd):
    """output_depth, sparse_depth, validity_map, ground_truth (N x 1 x H x W float32) with, in sample 0 when it has 32 pixels or more, the
    values the issue lists: depths on and next to the colormap's bin boundaries, below 0, above max_predict_depth, NaN, +-inf, validity 0,
    validity > 0 over sparse depth 0, odd validity values, ground-truth zeros, NaN, negative and infinite ground truth."""
    maxd = F(maxd)
    out = (rng.random((n, 1, h, w)) * 1.1 * float(maxd)).astype(F)
    keep = rng.random((n, 1, h, w)) < 0.45
    sparse = np.where(keep, out * (1 + 0.2 * (rng.random((n, 1, h, w)) - 0.5)), 0).astype(F)
    valid = (sparse > 0).astype(F)
    gt = np.where(rng.random((n, 1, h, w)) < 0.6, out * (1 + 0.1 * (rng.random((n, 1, h, w)) - 0.5)), 0).astype(F)
    if h * w >= 32:
        o, s, v, g = (a[0, 0].reshape(-1) for a in (out, sparse, valid, gt))          # views
        edge = [x for k in (1, 128, 255) for x in neighbours(F(k) / F(256) * maxd)]
        vals = edge + neighbours(maxd)[:2] + [F(-0.5), maxd * F(1.5), F(np.nan), F(np.inf), F(-np.inf), F(0.0), F(-0.0), F(1e-9)]
        o[:len(vals)] = vals                                                          # 19 values
        s[:9], v[:9] = edge, 1.0                                                      # sparse depth on the boundaries, error next to 0
        g[9:18] = edge
        s[19:21], v[19:21] = 0.0, 1.0                                                 # valid over depth 0: |out - 0| / 1e-8
        s[21], v[21] = 3.0, 0.0                                                       # depth without validity
        v[22], v[23], v[24] = -1.0, np.nan, 2.0                                       # where() passes validity itself on when it is not > 0
        s[22], s[23], s[24] = 1.0, 1.0, 1.0
        s[25], v[25] = np.nan, 1.0
        s[26], v[26], o[26] = np.inf, 1.0, 2.0
        g[27], g[28], g[29], g[30] = np.nan, -2.0, np.inf, 0.0
        g[31], o[31] = 2.5, 2.5                                                       # a perfect prediction: 1e-8 / (gt + 1e-8)
        for k, err in enumerate((0.05, 0.025, 0.1)):                                  # relative errors on the error map's scale 0.05
            if 32 + k < h * w:
                g[32 + k], o[32 + k] = 4.0, F(4.0) * F(1 + err)
    return out, sparse, valid, gt


def case_inputs(case):
    """The arrays of one fixture case, from its name alone."""
    rng = np.random.default_rng(sum(case['name'].encode()))
    n, (h, w) = case['n'], case['size']
    images = [make_image(rng, kind, n, h, w) for kind in case['images']]
    out, sparse, valid, gt = make_maps(rng, n, h, w, case['maxd'])
    maps = {key: arr for ch, key, arr in zip('osvg', MAP_KEYS.values(), (out, sparse, valid, gt)) if ch in case['maps']}
    return images, maps


def load_fixture(golden_dir, name):
    """-> (meta dict, arrays dict) of tests/golden/summary_<name>.npz"""
    z = np.load(fixture_path(golden_dir, name))
    return json.loads(str(z['meta'])), {k: z[k] for k in z.files if k != 'meta'}


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def reverse_normalization(normalized_image_range):
    """src/external_model_adapt.py:700-724: None for no transform, else (rev_mean, rev_std) as float32 (torchvision's normalize converts them)"""
    r = normalized_image_range
    if r is None or not (any(isinstance(v, (tuple, list)) for v in r) or len(r) > 2):
        return None
    if len(r) > 2:
        r = [tuple(r[:len(r) // 2]), tuple(r[len(r) // 2:])]
    return np.array([-m / s for m, s in zip(r[0], r[1])], dtype=F), np.array([1 / s for s in r[1]], dtype=F)


def colorize(x, table):
    """log_utils.colorize: matplotlib's Colormap.__call__ on a float32 array, RGB as float32; x: ... -> ... x 3"""
    with np.errstate(all='ignore'):
        t = x.astype(F) * F(256.0)
        nan = np.isnan(t)
        idx = np.trunc(np.clip(np.where(nan, F(0), t), F(0), F(255))).astype(np.int64)          # t < 0 -> 0, t >= 256 -> 255, else trunc(t)
    rgb = np.asarray(table, dtype=np.float64)[idx].astype(F)
    rgb[nan] = 0
    return rgb


def display_image(img, normalized_image_range):
    with np.errstate(all='ignore'):
        if img.max() > 10.0:                          # np.max propagates NaN as torch.max does, and NaN > 10 is false
            img = img / F(255.0)
        rev = reverse_normalization(normalized_image_range)
        if rev is not None:
            img = (img - rev[0].reshape(1, 3, 1, 1)) / rev[1].reshape(1, 3, 1, 1)
    return img.astype(F)


def make_grid(panels, nrow, padding=2):
    """torchvision.utils.make_grid(panels, nrow=nrow) for an ns x 3 x PH x PW array with ns <= nrow"""
    ns, c, ph, pw = panels.shape
    assert ns <= nrow
    if ns == 1:
        return panels[0]
    grid = np.zeros((c, ph + 2 * padding, ns * (pw + padding) + padding), dtype=panels.dtype)
    for i in range(ns):
        grid[:, padding:padding + ph, i * (pw + padding) + padding:i * (pw + padding) + padding + pw] = panels[i]
    return grid


def grid_shape(n_show, h, w, n_rows):
    return (n_rows * h, 2 * w) if n_show == 1 else (n_rows * h + 4, n_show * (2 * w + 2) + 2)


def restate_rows(images, maps, normalized_image_range, max_predict_depth, n_image_per_summary, tables):
    """The panel rows (each ns x 3 x H x 2W float32) in the order of include/ptta.h: one per image, output, sparse, ground truth."""
    maxd = F(max_predict_depth)
    rows = []
    for img in images:
        left = display_image(img, normalized_image_range)[:n_image_per_summary]
        rows.append(np.concatenate([left, np.zeros_like(left)], axis=-1))
    out = maps.get('output_depth')
    if out is None:
        return rows

    def coloured(x, name):
        return np.transpose(colorize(x[:, 0], tables[name]), (0, 3, 1, 2))
    with np.errstate(all='ignore'):
        out = out[:n_image_per_summary].astype(F)
        left = coloured(out / maxd, 'viridis')
        rows.append(np.concatenate([left, np.zeros_like(left)], axis=-1))
        if maps.get('sparse_depth') is not None and maps.get('validity_map') is not None:
            s, v = maps['sparse_depth'][:n_image_per_summary], maps['validity_map'][:n_image_per_summary]
            e = np.where(v > 0, np.abs(out - s) / (s + F(1e-8)), v).astype(F)
            rows.append(np.concatenate([coloured(s / maxd, 'viridis'), coloured(e / F(0.05), 'inferno')], axis=-1))
        if maps.get('ground_truth') is not None:
            g = maps['ground_truth'][:n_image_per_summary]
            e = np.where(g > 0, (np.abs(out - g) + F(1e-8)) / (g + F(1e-8)), F(0)).astype(F)
            rows.append(np.concatenate([coloured(g / maxd, 'viridis'), coloured(e / F(0.05), 'inferno')], axis=-1))
    return rows


def restate_grid(images, maps, normalized_image_range, max_predict_depth, n_image_per_summary, tables):
    """The fp32 3 x GH x GW grid of ptta_summary_compose for these rows"""
    rows = restate_rows(images, maps, normalized_image_range, max_predict_depth, n_image_per_summary, tables)
    return make_grid(np.concatenate(rows, axis=2), n_image_per_summary)


def restate_log_summary(tag, images, maps, normalized_image_range, max_predict_depth, n_image_per_summary, tables):
    """[(tag, grid)] of the add_image calls log_summary issues, in order"""
    calls = []
    text = tag + ('_image' if images else '')
    if images:
        calls.append((tag + '_image', restate_grid(images, {}, normalized_image_range, max_predict_depth, n_image_per_summary, tables)))
    if maps.get('output_depth') is not None:
        text += '_output'
        if maps.get('sparse_depth') is not None and maps.get('validity_map') is not None:
            text += '_sparse-error'
        if maps.get('ground_truth') is not None:
            text += '_groundtruth-error'
    if images or maps.get('output_depth') is not None:
        calls.append((text, restate_grid(images[-1:], maps, normalized_image_range, max_predict_depth, n_image_per_summary, tables)))
    return calls


def to_uint8_hwc(grid):
    """torch.utils.tensorboard.summary.image()'s conversion of a float CHW image: (x * 255).clip(0, 255) truncated to uint8 (NaN -> 0), HWC"""
    with np.errstate(all='ignore'):
        s = grid.astype(F) * F(255.0)
        s = np.where(np.isnan(s), F(0), np.clip(s, F(0), F(255)))
    return np.ascontiguousarray(np.transpose(s.astype(np.uint8), (1, 2, 0)))


# ---- generated inputs of the GPU tests: (name, N, (H, W), n_image_per_summary, image kinds, maps) ----------------------------------
# widths that are and are not multiples of 4, n_show 1, 2, 3 (aligned and 2-float-offset panels), odd heights (GH GW % 4 != 0: the
# one-pixel path), a width that needs more than one wave and one that needs two blocks per span
GENERATED = [
    ('w8_ns1', 1, (6, 8), 1, ('raw',), 'osvg'),
    ('w8_ns2', 2, (6, 8), 2, ('unit',), 'osvg'),
    ('w8_ns3', 3, (6, 8), 3, ('raw',), 'osvg'),
    ('w7_ns1', 2, (6, 7), 1, ('unit',), 'osvg'),
    ('w7_ns2', 2, (6, 7), 2, ('raw',), 'osvg'),
    ('w7_ns3_odd_h', 3, (5, 7), 3, ('unit',), 'osv'),
    ('w10_ns2_list2', 2, (4, 10), 4, ('raw', 'unit'), 'osv'),
    ('w1', 2, (3, 1), 2, ('unit',), 'osvg'),
    ('w3_ns1_odd_rows', 1, (5, 3), 1, (), 'osvg'),
    ('w270_ns2', 2, (4, 270), 2, ('raw',), 'osvg'),
    ('w2100_ns2', 2, (2, 2100), 2, (), 'osvg'),
    ('w2051_ns3', 3, (2, 2051), 3, ('unit',), 'o'),
]
FULL = ('kitti_n4', 4, (352, 1216), 4, ('raw',), 'osvg')


def generated_inputs(entry, maxd=80.0):
    name, n, (h, w), nips, kinds, which = entry
    rng = np.random.default_rng(sum(name.encode()) + 1000)
    images = [make_image(rng, kind, n, h, w) if h >= 3 and w >= 4 else rng.random((n, 3, h, w)).astype(F) for kind in kinds]
    out, sparse, valid, gt = make_maps(rng, n, h, w, maxd)
    maps = {key: arr for ch, key, arr in zip('osvg', MAP_KEYS.values(), (out, sparse, valid, gt)) if ch in which}
    return images, maps
