"""The numpy restatement of what ptta_egress_raw computes and the seeded cases of tests/test_gpu_egress.py / tests/test_egress_cpu.py.

The restatement is the reference writers' three expressions plus the paste: save_depth = np.uint32(z * multiplier) stored as a 16-bit PNG
(src/data_utils.py:236-251), save_validity_map = v > 0 -> 256 (:283-298), save_image = np.uint8(255 * image) transposed to HWC (:29-78);
the window lands at [sy : sy + h, sx : sx + w] of a zero frame, the starts clamped into the frame as ptta_ingest_raw clamps them.  Where
the reference is defined (0 <= z * multiplier < 2^31, 0 <= image * scale < 256) these are its bits: tests/golden/egress_raw.npz holds what
the REAL functions' files decode to (tests/golden/make_golden_egress.py) and the CPU test holds the restatement to it bit for bit.  Outside
that range the project's definition stands: negative, -0 and NaN give 0; at or above the top, +inf included, gives the top."""
import numpy as np

from tests.ingest_cases import clamp_starts


def restate_depth(z, multiplier=256.0):
    """fp32 -> uint16: p = z * multiplier (one fp32 multiply); p > 0 ? min(trunc(p), 65535) : 0"""
    with np.errstate(invalid='ignore', over='ignore'):
        p = np.asarray(z, np.float32) * np.float32(multiplier)
        assert p.dtype == np.float32
        return np.where(p > 0, np.minimum(p, np.float32(65535.0)), np.float32(0.0)).astype(np.uint16)          # (the cast truncates)


def restate_validity(v):
    with np.errstate(invalid='ignore'):
        return np.where(np.asarray(v, np.float32) > 0, 256, 0).astype(np.uint16)


def restate_image(image, image_scale=255.0):
    """n x 3 x h x w fp32 -> n x h x w x 3 uint8: q = image * image_scale; q > 0 ? min(trunc(q), 255) : 0"""
    with np.errstate(invalid='ignore', over='ignore'):
        q = np.asarray(image, np.float32) * np.float32(image_scale)
        assert q.dtype == np.float32
        u8 = np.where(q > 0, np.minimum(q, np.float32(255.0)), np.float32(0.0)).astype(np.uint8)
    return np.ascontiguousarray(np.moveaxis(u8, -3, -1))


def paste(a, dst_size, start):
    """a: n x h x w (x C) -> n x H x W (x C): zeros, the window at the per-sample clamped starts"""
    (H, W), (n, h, w) = dst_size, a.shape[:3]
    sy, sx = clamp_starts(start, n, H, W, h, w)
    out = np.zeros((n, H, W) + a.shape[3:], dtype=a.dtype)
    for b in range(n):
        out[b, sy[b]:sy[b] + h, sx[b]:sx[b] + w] = a[b]
    return out


def restate(depth=None, validity=None, image=None, dst_size=None, start=None, multiplier=256.0, image_scale=255.0):
    """What egress_raw returns for n x 1 x h x w depth / validity and n x 3 x h x w image: a dict of the planes given."""
    ref = {}
    for key, a in (('depth_u16', None if depth is None else restate_depth(depth[:, 0], multiplier)),
                   ('validity_u16', None if validity is None else restate_validity(validity[:, 0])),
                   ('image_u8', None if image is None else restate_image(image, image_scale))):
        if a is not None:
            ref[key] = paste(a, a.shape[1:3] if dst_size is None else dst_size, start)
    return ref


def frames(seed, n, h, w):
    """Seeded predictions: depth with holes, sub-step fractions and some values past the 16-bit range at multiplier 256; a validity map
    with a few negative entries; an image reaching a little below 0 and above 1."""
    rng = np.random.default_rng(seed)
    depth = (rng.random((n, 1, h, w)) * 300.0 * (rng.random((n, 1, h, w)) < 0.7)).astype(np.float32)
    validity = np.where(rng.random((n, 1, h, w)) < 0.1, -1.0, (rng.random((n, 1, h, w)) < 0.5)).astype(np.float32)
    image = (rng.random((n, 3, h, w)) * 1.1 - 0.05).astype(np.float32)
    return depth, validity, image


# name, n, (H, W), (h, w), start (None or (start_y list, start_x list)), what it exercises.  A 16-bit row has 16-byte stores once some lane's
# 8 pixels lie inside it (W >= 8 at least), the image 12-byte stores once W >= 4 and the row's first byte is word-aligned.
CASES = [
    ('odd_no_vector', 1, (5, 3), (3, 2), ([1], [1]), 'odd sizes, no vector path in any plane'),
    ('width_not_multiple_of_8', 3, (6, 21), (4, 10), ([1, 0, 2], [3, 11, 0]), 'head / body / tail of a row, per-sample starts'),
    ('aligned', 2, (8, 32), (4, 16), ([2, 4], [8, 16]), 'aligned rows, window and starts'),
    ('odd_sx', 2, (9, 29), (6, 17), ([2, 1], [5, 3]), 'odd W and sx: rows begin at every alignment mod 16'),
    ('window_at_end', 1, (7, 19), (3, 8), ([4], [11]), 'the window ends on the last output byte'),
    ('starts_out_of_range', 3, (9, 13), (4, 8), ([-3, 100, 2], [50, -1, 7]), 'clamped exactly as ptta_ingest_raw clamps'),
    ('no_border', 2, (6, 24), (6, 24), None, 'h = H and w = W'),
    ('one_by_one', 1, (5, 20), (1, 1), ([2], [9]), 'a 1 x 1 window inside a frame'),
    ('two_blocks_per_row', 1, (3, 2100), (2, 2048), ([1], [37]), 'a row of 525 image lanes: blocks of 256 side by side'),
    ('two_blocks_per_row_16bit', 1, (2, 4100), (1, 4090), ([1], [7]), 'a row of 514 16-bit lanes: blocks of 256 side by side'),
    ('wide_scalar', 1, (2, 601), (2, 599), ([0], [2]), 'a 601-wide row off the word grid: byte stores past one wave'),
    ('rows_past_block_budget', 3, (700, 9), (690, 5), ([4, 0, 10], [2, 4, 0]), 'more than 2,048 rows in all: a block strides over rows'),
]
FULL = [('kitti_1', 1, (375, 1242), (352, 1216), ([23], [13])), ('kitti_4', 4, (375, 1242), (352, 1216), ([23] * 4, [13] * 4))]
COMBOS = [c for c in ((d, v, i) for d in (True, False) for v in (True, False) for i in (True, False)) if any(c)]          # planes present
