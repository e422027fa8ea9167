"""CPU-only: the numpy restatement of ptta_ingest_raw (tests/ingest_cases.py) against the REAL reference's outputs
(tests/golden/ingest_raw.npz), the new entry of the ctypes table against include/ptta.h, and RawFrameStager's slot layout."""
import os
import re

import numpy as np
import pytest

from proxytta import _lib
from proxytta.staging import raw_slot_layout
from tests import ingest_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_reproduces_the_reference_bit_for_bit(golden_dir):
    g = np.load(os.path.join(golden_dir, 'ingest_raw.npz'))
    image, depth = g['image_u8'][None], g['depth_u16'][None]
    assert image.dtype == np.uint8 and depth.dtype == np.uint16 and image.shape == (1, 9, 13, 3)
    assert image.min() == 0 and image.max() == 255 and depth.max() == 65535 and 1 in depth and 0 in depth
    got = C.restate_image(image)
    assert got.dtype == np.float32 and np.array_equal(got[0], g['image'])
    for mult, key in ((256.0, 'depth_256'), (1000.0, 'depth_1000')):
        z, v = C.restate_depth(depth, multiplier=mult)
        assert z.dtype == v.dtype == np.float32 and np.array_equal(z[0], g[key])
        assert np.array_equal(v[0], (g[key] > 0).astype(np.float32))
    z, v = C.restate_depth(depth)
    assert np.array_equal(z[0], g['depth_v']) and np.array_equal(v[0], g['validity'])
    # the window is plain indexing of the reference's arrays, starts clamped into the sample
    z, v = C.restate_depth(depth, (4, 8), ([7], [-2]))
    assert np.array_equal(z[0], g['depth_256'][:, 5:9, 0:8]) and np.array_equal(v[0], g['validity'][:, 5:9, 0:8])
    assert np.array_equal(C.restate_image(image, (8, 12), ([1], [1]))[0], g['image'][:, 1:9, 1:13])
    assert os.path.getsize(os.path.join(golden_dir, 'ingest_raw.npz')) < 16 << 10


def test_case_table_is_what_the_gpu_test_says_it_is():
    for name, n, (H, W), (h, w), start, _ in C.CASES:
        assert h <= H and w <= W and (start is None or all(len(s) == n for s in start)), name
    by = {c[0]: c for c in C.CASES}
    assert by['scalar_odd'][3][1] % 4 and by['scalar_ragged'][3][1] % 4 and by['wide_scalar'][3][1] % 4
    assert by['vector_aligned'][3][1] % 4 == 0 and by['vector_odd_offset'][3][1] % 4 == 0
    n, (H, W), (h, w), (sy, sx) = by['window_at_end'][1], by['window_at_end'][2], by['window_at_end'][3], by['window_at_end'][4]
    assert sy[0] + h == H and sx[0] + w == W and (3 * n * H * W) % 4          # the window ends on the array's last byte, which is not word-aligned
    assert by['two_blocks_per_row'][3][1] // 4 >= 512 and by['wide_scalar'][3][1] >= 512
    a, b, c = C.raw_frames(5, 2, 6, 8)
    a2, b2, c2 = C.raw_frames(5, 2, 6, 8)
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(c, c2) and (b == 0).any() and (b > 0).any()


def test_signature_entry_matches_the_header():
    sig = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    res, args = sig['ptta_ingest_raw']
    assert res is _lib.c_int and len(args) == 17
    assert args == [_lib.c_void_p] * 8 + [_lib.c_int] * 5 + [_lib.c_void_p, _lib.c_void_p, _lib.c_float, _lib.c_void_p]
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    decl = re.search(r'^int ptta_ingest_raw\(([^;]*)\);', header, re.M)
    assert decl and '/*' not in decl.group(1)
    params = [' '.join(p.split()) for p in decl.group(1).split(',')]
    assert len(params) == 17
    kinds = ['p' if '*' in p or p.startswith('ptta_stream') else ('f' if p.startswith('float') else 'i') for p in params]
    assert kinds == ['p'] * 8 + ['i'] * 5 + ['p', 'p', 'f', 'p']
    assert params[0] == 'const uint8_t* image_u8' and params[1] == 'const uint16_t* sparse_u16' and params[15] == 'float multiplier'
    assert header.index('int ptta_crop_flip(') < header.index('int ptta_ingest_raw(') < header.index('int ptta_rotate(')
    assert int(re.search(r'#define PTTA_ABI_VERSION (\d+)', header).group(1)) == _lib.PTTA_ABI_VERSION == 2
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), 'ptta_ingest_raw')


@pytest.mark.parametrize('n,H,W,gt', [(1, 375, 1242, False), (1, 375, 1242, True), (16, 480, 640, False), (3, 5, 7, True), (1, 1, 1, False)])
def test_raw_slot_layout(n, H, W, gt):
    lay = raw_slot_layout(n, H, W, gt)
    px = n * H * W
    sections = [('image', 3 * px), ('sparse', 2 * px)] + ([('gt', 2 * px)] if gt else []) + [('start_y', 4 * n), ('start_x', 4 * n)]
    assert set(lay) == {k for k, _ in sections} | {'bytes'}
    assert lay['image'] == 0
    end = 0
    for (key, size), nxt in zip(sections, sections[1:] + [('bytes', 0)]):
        assert lay[key] >= end, key                                    # no overlap
        end = lay[key] + size
        assert lay[nxt[0]] - end < 16 or nxt[0] == 'start_x', nxt      # no more padding than alignment asks for
    for key in ('image', 'sparse', 'gt', 'start_y'):
        assert key not in lay or lay[key] % 16 == 0, key               # every section on a 16-byte boundary (the starts are ONE section)
    assert lay['start_x'] == lay['start_y'] + 4 * n and lay['bytes'] % 16 == 0 and lay['bytes'] >= lay['start_x'] + 4 * n
    assert lay['bytes'] < (7 if gt else 5) * px + 8 * n + 16 * (len(sections))


def test_raw_slot_layout_figures_and_refusals():
    # the issue's arithmetic for a KITTI frame taken at the window's size: 3 + 2 bytes per pixel against 4 (3 + 1)
    lay = raw_slot_layout(1, 352, 1216)
    assert lay['sparse'] == 3 * 428032 and lay['start_y'] == 5 * 428032 and lay['bytes'] == 5 * 428032 + 16
    assert 4 * (3 + 1) * 428032 / lay['bytes'] > 3.19
    lay = raw_slot_layout(3, 5, 7, True)                                # 315 image bytes -> 320; 210 -> 530 -> 544; 754 -> 768
    assert (lay['sparse'], lay['gt'], lay['start_y'], lay['start_x'], lay['bytes']) == (320, 544, 768, 780, 800)
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0)):
        with pytest.raises(ValueError):
            raw_slot_layout(*bad)
