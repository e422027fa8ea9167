"""CPU-only: the numpy restatement of ptta_egress_raw (tests/egress_cases.py) against what the REAL reference's writers' files decode to
(tests/golden/egress_raw.npz), the restatement's truncation over every 16-bit value, the case table's alignment classes, the new entry of
the ctypes table against include/ptta.h, RawFrameSink's slot layout, and the refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from proxytta import _lib
from proxytta.sink import RawFrameSink, raw_sink_layout
from tests import egress_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_reproduces_the_reference_bit_for_bit(golden_dir):
    path = os.path.join(golden_dir, 'egress_raw.npz')
    g = np.load(path)
    depth, validity, image, image_255 = g['depth'], g['validity'], g['image'], g['image_255']
    assert depth.dtype == validity.dtype == image.dtype == np.float32 and depth.shape == (9, 13) and image.shape == (3, 9, 13)
    # the inputs the fixture promises: the edges of every rule, and nothing the reference leaves undefined
    for v in (0.0, 3.0 / 256.0, np.nextafter(np.float32(1.0), np.float32(0.0)), 255.99609375, 256.0, 300.5, 1e6):
        assert np.float32(v) in depth, v
    assert ((depth > 0) & (depth < 1.0 / 1000.0 + 1e-9)).any() and depth.min() >= 0 and np.isfinite(depth).all() and depth.max() * 1000.0 < 2.0 ** 31
    assert (validity < 0).any() and np.float32(1.0) in image and np.float32(0.0) in image and np.float32(0.999999) in image and np.float32(1.0 / 255.0) in image
    for mult, key in ((256.0, 'depth_256'), (1000.0, 'depth_1000')):
        got = C.restate_depth(depth, mult)
        assert got.dtype == g[key + '_png'].dtype == np.uint16 and np.array_equal(got, g[key + '_png']), key
        assert str(g[key + '_mode']) == 'I;16'
    for v in (255.99609375, 256.0, 300.5, 1e6):
        assert (g['depth_256_png'][depth == np.float32(v)] == 65535).all(), v
    assert np.array_equal(C.restate_validity(validity), g['validity_png']) and str(g['validity_mode']) == 'I;16'
    assert sorted(np.unique(g['validity_png']).tolist()) == [0, 256] and (g['validity_png'][validity < 0] == 0).all()
    got = C.restate_image(image[None], 255.0)[0]
    assert got.dtype == np.uint8 and got.shape == (9, 13, 3) and np.array_equal(got, g['image_png']) and str(g['image_mode']) == 'RGB'
    assert np.array_equal(C.restate_image(image_255[None], 1.0)[0], g['image_255_png']) and str(g['image_255_mode']) == 'RGB'
    # through restate(): planes with their channel axis, no border, and pasted into a frame
    ref = C.restate(depth[None, None], validity[None, None], image[None])
    assert np.array_equal(ref['depth_u16'][0], g['depth_256_png']) and np.array_equal(ref['validity_u16'][0], g['validity_png'])
    assert np.array_equal(ref['image_u8'][0], g['image_png'])
    ref = C.restate(depth[None, None], None, image[None], dst_size=(12, 20), start=([2], [50]))          # sx clamps to 20 - 13
    assert sorted(ref) == ['depth_u16', 'image_u8'] and ref['depth_u16'].shape == (1, 12, 20) and ref['image_u8'].shape == (1, 12, 20, 3)
    assert np.array_equal(ref['depth_u16'][0, 2:11, 7:20], g['depth_256_png']) and np.array_equal(ref['image_u8'][0, 2:11, 7:20], g['image_png'])
    assert ref['depth_u16'].sum() == g['depth_256_png'].sum(dtype=np.uint64) and ref['image_u8'].sum() == g['image_png'].sum(dtype=np.uint64)
    assert os.path.getsize(path) < 16 << 10


def test_truncation_over_all_65536_values():
    k = np.arange(65536)
    assert np.array_equal(C.restate_depth(k.astype(np.float32) / np.float32(256.0), 256.0), k)
    # multiplier 1000: k / 1000 is rounded to fp32, and where it was rounded DOWN the product falls below k and truncates to k - 1.  That
    # is the reference's own np.uint32(z * multiplier); rounding instead would not be what save_depth stores.
    back = C.restate_depth(k.astype(np.float32) / np.float32(1000.0), 1000.0).astype(np.int64)
    assert set(np.unique(back - k).tolist()) == {-1, 0} and int((back == k - 1).sum()) == 739
    # the project's definition outside the reference's range
    odd = np.array([-1.0, -0.0, np.nan, -np.inf, np.inf, 3e38, 2.0 ** 31, 65536.0 / 256.0, 65535.5 / 256.0], dtype=np.float32)
    assert C.restate_depth(odd).tolist() == [0, 0, 0, 0, 65535, 65535, 65535, 65535, 65535]
    assert C.restate_validity(np.array([np.nan, -1.0, -0.0, 1e-30, np.inf], dtype=np.float32)).tolist() == [0, 0, 0, 256, 256]
    q = np.array([-0.1, np.nan, 1.0, 1.004, 2.0, np.inf, 0.999999, 1.0 / 255.0], dtype=np.float32).reshape(1, 1, 1, 8).repeat(3, axis=1)
    assert C.restate_image(q)[0, 0, :, 0].tolist() == [0, 0, 255, 255, 255, 255, 254, 1]


def test_case_table_is_what_the_gpu_test_says_it_is():
    by = {c[0]: c for c in C.CASES}
    assert len(by) == len(C.CASES)
    for name, n, (H, W), (h, w), start, _ in C.CASES + [c + ('',) for c in C.FULL]:
        assert 1 <= h <= H and 1 <= w <= W and (start is None or all(len(s) == n for s in start)), name

    def row_classes(n, H, W):          # the offsets, in pixels, of the 16-bit rows inside a 16-byte line (an aligned base)
        return {(b * H * W + y * W) % 8 for b in range(n) for y in range(H)}

    def image_row_classes(n, H, W):
        return {3 * (b * H * W + y * W) % 4 for b in range(n) for y in range(H)}
    _, n, (H, W), (h, w), start, _ = by['odd_no_vector']
    assert W < 4 and W % 2 and H % 2 and h % 2                                                # no lane holds 8 (or 4) pixels of a row
    _, n, (H, W), (h, w), start, _ = by['width_not_multiple_of_8']
    assert W % 8 and W > 16 and len(row_classes(n, H, W)) > 1 and len(set(start[1])) == n    # a head, a body and a tail
    _, n, (H, W), (h, w), start, _ = by['aligned']
    assert W % 8 == 0 and w % 8 == 0 and all(s % 8 == 0 for s in start[1]) and row_classes(n, H, W) == {0} and image_row_classes(n, H, W) == {0}
    _, n, (H, W), (h, w), start, _ = by['odd_sx']
    assert W % 2 and all(s % 2 for s in start[1]) and row_classes(n, H, W) == set(range(8)) and image_row_classes(n, H, W) == set(range(4))
    _, n, (H, W), (h, w), start, _ = by['window_at_end']
    assert start[0][0] + h == H and start[1][0] + w == W and n == 1
    _, n, (H, W), (h, w), start, _ = by['starts_out_of_range']
    sy, sx = C.clamp_starts(start, n, H, W, h, w)
    assert min(start[0]) < 0 and max(start[0]) > H - h and min(start[1]) < 0 and max(start[1]) > W - w
    assert sy.tolist() == [0, H - h, 2] and sx.tolist() == [W - w, 0, W - w]
    assert by['no_border'][2] == by['no_border'][3] and by['one_by_one'][3] == (1, 1) and by['one_by_one'][2][1] > 8
    W = by['two_blocks_per_row'][2][1]
    assert W == 2100 and (W + 3) // 4 >= 512 and (W + 7) // 8 + 1 < 512                      # image lanes need two blocks and more, 16-bit lanes one
    assert (by['two_blocks_per_row_16bit'][2][1] + 7) // 8 + 1 >= 512
    W = by['wide_scalar'][2][1]
    assert W == 601 and W % 2 and image_row_classes(1, 2, W) == {0, 3}                        # its second image row takes byte stores
    _, n, (H, W), (h, w), start, _ = by['rows_past_block_budget']
    assert n * H > 2048 >= H and len(set(start[0])) == n                                      # (2,048: the launch's block budget, csrc/egress.hip)
    assert C.FULL[0][2:] == ((375, 1242), (352, 1216), ([23], [13])) and [c[1] for c in C.FULL] == [1, 4]
    assert len(C.COMBOS) == 7
    a, b = C.frames(5, 2, 6, 8), C.frames(5, 2, 6, 8)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and (a[0] == 0).any() and (a[0] * 256 > 65536).any() and (a[1] < 0).any()
    assert (a[2] < 0).any() and (a[2] > 1).any()


def test_signature_entry_matches_the_header():
    names = [name for name, _, _ in _lib.SIGNATURES]
    sig = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    res, args = sig['ptta_egress_raw']
    assert res is _lib.c_int and len(args) == 16
    assert args == [_lib.c_void_p] * 6 + [_lib.c_int] * 5 + [_lib.c_void_p, _lib.c_void_p, _lib.c_float, _lib.c_float, _lib.c_void_p]
    assert names.index('ptta_egress_raw') == names.index('ptta_ingest_raw') + 1
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    decl = re.search(r'^int ptta_egress_raw\(([^;]*)\);', header, re.M)
    assert decl and '/*' not in decl.group(1)
    params = [' '.join(p.split()) for p in decl.group(1).split(',')]
    assert len(params) == 16
    kinds = ['p' if '*' in p or p.startswith('ptta_stream') else ('f' if p.startswith('float') else 'i') for p in params]
    assert kinds == ['p'] * 6 + ['i'] * 5 + ['p', 'p', 'f', 'f', 'p']
    assert params[:6] == ['const float* depth', 'const float* validity', 'const float* image', 'uint16_t* depth_u16', 'uint16_t* validity_u16',
                          'uint8_t* image_u8']
    assert params[6:11] == ['int n', 'int height', 'int width', 'int dst_height', 'int dst_width']
    assert params[13:] == ['float multiplier', 'float image_scale', 'ptta_stream s']
    # directly behind ptta_ingest_raw: no other declaration between the two
    between = header[header.index('int ptta_ingest_raw('):header.index('int ptta_egress_raw(')]
    assert len(re.findall(r'^\w[\w\s\*]*\bptta_\w+\(', between, re.M)) == 1
    assert int(re.search(r'#define PTTA_ABI_VERSION (\d+)', header).group(1)) == _lib.PTTA_ABI_VERSION == 2
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), 'ptta_egress_raw')


@pytest.mark.parametrize('n,H,W,planes', [(1, 375, 1242, ('depth',)), (1, 375, 1242, ('depth', 'validity', 'image')), (4, 375, 1242, ('depth', 'image')),
                                          (3, 5, 7, ('image', 'validity')), (1, 1, 1, ('image',)), (2, 3, 3, 'validity')])
def test_raw_sink_layout(n, H, W, planes):
    lay = raw_sink_layout(n, H, W, planes)
    px = n * H * W
    want = [p for p in ('depth', 'validity', 'image') if p in planes]          # the 16-bit planes first, whatever order was asked for
    assert list(lay) == want + ['bytes']
    end = 0
    for key in want:
        assert lay[key] % 16 == 0 and 0 <= lay[key] - end < 16, key                # on a 16-byte boundary, no overlap, no more padding than that
        end = lay[key] + (3 if key == 'image' else 2) * px
    assert lay['bytes'] % 16 == 0 and 0 <= lay['bytes'] - end < 16


def test_raw_sink_layout_figures_and_refusals():
    # one KITTI frame: 2 bytes per pixel against the 4 of the fp32 map; 2 + 2 + 3 against 4 + 4 + 12 with all three planes
    lay = raw_sink_layout(1, 375, 1242, ('depth',))
    assert 2 * 375 * 1242 == 931500 and lay == {'depth': 0, 'bytes': 931504}
    lay = raw_sink_layout(1, 375, 1242, ('depth', 'validity', 'image'))
    assert lay == {'depth': 0, 'validity': 931504, 'image': 1863008, 'bytes': 1863008 + 1397264}
    assert 20 * 465750 / lay['bytes'] > 2.85
    assert raw_sink_layout(3, 5, 7, ('depth', 'image')) == {'depth': 0, 'image': 224, 'bytes': 544}          # 210 -> 224; + 315 = 539 -> 544
    for bad in ((0, 4, 4, ('depth',)), (1, 0, 4, ('depth',)), (1, 4, 0, ('depth',)), (1, 4, 4, ()), (1, 4, 4, ('depth', 'depth')), (1, 4, 4, ('gt',))):
        with pytest.raises(ValueError):
            raw_sink_layout(*bad)


def test_sink_refusals_on_the_host():
    for kw in (dict(n=0), dict(height=0), dict(width=0), dict(dst_height=3), dict(dst_width=5), dict(planes=()), dict(planes=('depth', 'sparse')),
               dict(slots=1), dict(writer='jpeg'), dict(multiplier=0.0), dict(multiplier=float('nan')), dict(image_scale=float('inf')),
               dict(image_scale=-1.0)):
        with pytest.raises(ValueError):
            RawFrameSink(**dict(dict(n=1, height=4, width=6, dst_height=5, dst_width=8), **kw))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            RawFrameSink(1, 4, 6)
        from proxytta.egress import egress_raw
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            egress_raw(depth=torch.zeros(1, 1, 4, 6))


def test_library_refusals_need_no_device():
    """Every refusal returns -22 before any launch and leaves its reason in ptta_last_error(NULL).  The buffers are real (device memory
    where there is a device, host memory otherwise) and large enough for the valid call, which this test never makes."""
    lib = _lib.load()
    n, h, w, H, W = 2, 4, 6, 5, 8
    if torch.cuda.is_available():
        keep = [torch.zeros(n * 3 * H * W, dtype=torch.float32, device='cuda') for _ in range(6)]
        d, v, i, du, vu, iu = (t.data_ptr() for t in keep)
        stream = torch.cuda.current_stream().cuda_stream
    else:
        keep = [ctypes.create_string_buffer(4 * n * 3 * H * W + 16) for _ in range(6)]
        d, v, i, du, vu, iu = ((ctypes.addressof(b) + 15) // 16 * 16 for b in keep)
        stream = None
    ok = dict(d=d, v=v, i=i, du=du, vu=vu, iu=iu, n=n, h=h, w=w, H=H, W=W, m=256.0, s=255.0)
    cases = [(dict(d=None, v=None, i=None, du=None, vu=None, iu=None), 'no input'), (dict(du=None), 'come together'), (dict(v=None), 'come together'),
             (dict(i=None), 'come together'), (dict(iu=None), 'come together'), (dict(n=0), 'n must'), (dict(n=-3), 'n must'),
             (dict(h=0), 'size'), (dict(w=0), 'size'), (dict(H=0, h=0), 'size'), (dict(W=-1), 'size'), (dict(h=H + 1), 'does not fit'),
             (dict(w=W + 1), 'does not fit'), (dict(m=0.0), 'multiplier'), (dict(m=-256.0), 'multiplier'), (dict(m=float('inf')), 'multiplier'),
             (dict(m=float('nan')), 'multiplier'), (dict(s=0.0), 'image_scale'), (dict(s=float('nan')), 'image_scale'),
             (dict(s=float('inf')), 'image_scale'), (dict(du=du + 1), '2-byte aligned'), (dict(vu=vu + 3), '2-byte aligned')]
    for kw, why in cases:
        a = dict(ok, **kw)
        rc = lib.ptta_egress_raw(a['d'], a['v'], a['i'], a['du'], a['vu'], a['iu'], a['n'], a['h'], a['w'], a['H'], a['W'], None, None, a['m'], a['s'], stream)
        said = lib.ptta_last_error(None).decode()
        assert rc == -22 and 'ptta_egress_raw' in said and why in said, (kw, rc, said)
    del keep
