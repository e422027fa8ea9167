"""The numpy restatement of what ptta_ingest_raw computes and the seeded cases of tests/test_gpu_ingest.py / tests/test_ingest_cpu.py.

The restatement is the reference loader's three expressions plus the window: load_image(normalize=False, 'CHW') = np.asarray(image,
np.float32) transposed (2, 0, 1) (src/data_utils.py:150-158); load_depth = z / multiplier, z[z <= 0] = 0 (:219-223);
load_depth_with_validity_map = v[z > 0] = 1 (:182-188); the crop [sy : sy + h, sx : sx + w] (src/datasets.py:83-170), with the starts
clamped into the sample as ptta_crop_flip clamps them.  tests/golden/ingest_raw.npz holds what the REAL functions return for two small PNGs
(tests/golden/make_golden_ingest.py) and the CPU test holds the restatement to it bit for bit, so `torch.equal` against the restatement
is `torch.equal` against the reference."""
import numpy as np


def clamp_starts(start, n, H, W, h, w):
    sy, sx = (0, 0) if start is None else start
    sy = np.clip(np.broadcast_to(np.asarray(sy, np.int64), (n,)), 0, H - h)
    sx = np.clip(np.broadcast_to(np.asarray(sx, np.int64), (n,)), 0, W - w)
    return sy, sx


def window(a, start, h, w):
    """a: n x H x W (x C) -> n x h x w (x C), per-sample clamped starts"""
    sy, sx = clamp_starts(start, a.shape[0], a.shape[1], a.shape[2], h, w)
    return np.stack([a[b, sy[b]:sy[b] + h, sx[b]:sx[b] + w] for b in range(a.shape[0])])


def restate_image(image_u8, size=None, start=None):
    """n x H x W x 3 uint8 -> n x 3 x h x w float32"""
    h, w = image_u8.shape[1:3] if size is None else size
    return np.stack([np.transpose(np.asarray(im, np.float32), (2, 0, 1)) for im in window(image_u8, start, h, w)])


def restate_depth(z_u16, size=None, start=None, multiplier=256.0):
    """n x H x W 16-bit -> (depth, validity), each n x 1 x h x w float32"""
    h, w = z_u16.shape[1:3] if size is None else size
    z = np.array(window(z_u16, start, h, w), dtype=np.float32)
    z = z / np.float32(multiplier)
    z[z <= 0] = 0.0
    v = z.astype(np.float32)
    v[z > 0] = 1.0
    return z[:, None], v[:, None]


def raw_frames(seed, n, H, W, density=0.3):
    """Seeded decoded frames: uint8 image, 16-bit sparse depth (about `density` of the pixels set) and ground truth (denser)."""
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
    sparse = (rng.integers(1, 65536, size=(n, H, W)) * (rng.random((n, H, W)) < density)).astype(np.uint16)
    gt = (rng.integers(1, 65536, size=(n, H, W)) * (rng.random((n, H, W)) < 0.7)).astype(np.uint16)
    return image, sparse, gt


# name, n, (H, W), (h, w), start (None or (start_y list, start_x list)), what it exercises
CASES = [
    ('scalar_odd', 1, (5, 7), (5, 7), None, 'no vector path at all'),
    ('scalar_ragged', 3, (6, 10), (6, 10), None, 'width not a multiple of 4'),
    ('vector_aligned', 2, (8, 16), (8, 16), None, 'aligned source and output'),
    ('vector_odd_offset', 2, (9, 13), (8, 12), ([1, 0], [1, 0]), 'unaligned source, per-sample starts'),
    ('window_at_end', 1, (7, 9), (3, 8), ([4], [1]), 'the last source byte'),
    ('starts_out_of_range', 3, (9, 13), (4, 8), ([-3, 100, 2], [50, -1, 7]), 'clamped exactly as ptta_crop_flip clamps'),
    ('two_blocks_per_row', 1, (3, 2100), (2, 2048), ([1], [37]), 'a row of 512 lanes: two blocks of 256'),
    ('wide_scalar', 1, (2, 601), (2, 599), ([0], [2]), 'the one-pixel path past one block per row'),
]
FULL = [('kitti_1', 1, (375, 1242), (352, 1216), ([23], [13])), ('kitti_4', 4, (375, 1242), (352, 1216), ([23] * 4, [13] * 4))]
