"""StepAugmenter.apply on the one-launch route (csrc/augment_fused.hip) against the staged Transforms.apply calls it replaces, with the same
hand-made draws: all five outputs with torch.equal, no tolerance.  The staged calls are the reference the project already trusts
(tests/golden/transforms_*.npz, tests/test_gpu_staging_augment.py)."""
import ctypes

import numpy as np
import pytest
import torch

from proxytta import _lib
from proxytta.augment import DRAW_DTYPE, StepAugmenter
from proxytta.transforms import Transforms

pytestmark = pytest.mark.gpu

SIZES = [(1, 3, 5), (1, 16, 16), (2, 37, 53), (3, 40, 64)]
MODES = ('bilinear', 'nearest', 'nearest', 'nearest')
KEYS = ('crop', 'hflip', 'vflip', 'rotate', 'resize', 'brightness', 'contrast', 'saturation', 'gamma', 'hue', 'noise', 'crop_pad', 'resize_pad', 'remove')
RANGES = dict(brightness=[0.6, 1.4], contrast=[0.6, 1.4], gamma=[0.8, 1.2], hue=[-0.1, 0.1], saturation=[0.6, 1.4])
FACTORS = dict(brightness=[0.6, 1.4, 1.13], contrast=[1.37, 0.61, 0.9], gamma=[0.8, 1.2, 1.07], hue=[-0.1, 0.1, 0.033], saturation=[0.64, 1.4, 1.21])


def u8(v):
    return torch.tensor(list(v), dtype=torch.uint8)


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32)


_frames = {}


def frames(n, H, W):
    """Three images (fractional, integer-valued, a constant 200.0), sparse depth at 5 % density with its validity map, a dense ground
    truth; made once per size and never written to."""
    if (n, H, W) not in _frames:
        g = torch.Generator().manual_seed(1000 * n + 10 * H + W)
        frac = torch.rand(n, 3, H, W, generator=g) * 255.0
        mask = torch.rand(n, 1, H, W, generator=g) < 0.05
        sparse = torch.where(mask, 1.0 + 79.0 * torch.rand(n, 1, H, W, generator=g), torch.zeros(()))
        gt = 1.0 + 79.0 * torch.rand(n, 1, H, W, generator=g)
        valid = torch.where(sparse > 0, torch.ones_like(sparse), sparse)
        _frames[(n, H, W)] = dict(images={'fractional': frac.cuda(), 'integer': frac.floor().cuda(), 'constant': torch.full((n, 3, H, W), 200.0).cuda()},
                                  sparse=sparse.cuda(), valid=valid.cuda(), gt=gt.cuda())
    return _frames[(n, H, W)]


def geo_draw(n, h, w, hflip=None, vflip=None, angles=None, rotate=None, scale=None, resize=None, crop=None):
    """A geometric draw by hand.  hflip / vflip / rotate / resize: per-sample coins (None = not configured); angles in degrees; scale 1.0 or
    1.5 of the (cropped) size h x w with the largest start offsets; crop = (ch, cw, start_y, start_x)."""
    d = dict.fromkeys(KEYS)
    d['crop'] = None if crop is None else (crop[0], crop[1], i32(crop[2]), i32(crop[3]))
    d['hflip'] = None if hflip is None else u8(hflip)
    d['vflip'] = None if vflip is None else u8(vflip)
    if rotate is not None:
        d['rotate'] = (u8(rotate), torch.tensor(list(angles), dtype=torch.float64))
    if resize is not None:
        rh, rw = (h, w) if scale == 1.0 else (int(scale * h), int(scale * w))
        d['resize'] = (u8(resize), i32([rh] * n), i32([rw] * n), i32([rh - h] * n), i32([rw - w] * n), h, w)
    return d


def pho_draw(n, **coins):
    """A photometric draw by hand: option name -> per-sample coins."""
    d = dict.fromkeys(KEYS)
    for key, do in coins.items():
        d[key] = (u8(do), torch.tensor(FACTORS[key][:n], dtype=torch.float32))
    return d


def pho_object(p):
    return None if p is None else Transforms(**{'random_' + k: RANGES[k] for k in RANGES if p[k] is not None})


def compare(fr, g, p, modes=MODES, scaling=False, kinds=('fractional', 'integer', 'constant'), validity=True, ground_truth=True, moves=False):
    """apply on the fused route against geo.apply + pho.apply, image kind by image kind.  moves: the draw is one that leaves no tensor as
    it was (the comparison is not between two copies of the input)."""
    geo, pho = Transforms(resize_scaling_depth=scaling), pho_object(p)
    aug = StepAugmenter(geo, pho, modes)
    for kind in kinds:
        image = fr['images'][kind]
        maps = [fr['sparse']] + ([fr['valid']] if validity else []) + ([fr['gt']] if ground_truth else [])
        staged = geo.apply([image] + maps, g, modes[:1 + len(maps)])
        image1 = staged[0] if pho is None or not (pho.do_photometric_transforms or pho.do_random_gamma) else pho.apply([staged[0]], p)[0]
        aug.last_draw = (g, p)
        out = aug.apply(image, fr['sparse'], fr['valid'] if validity else None, fr['gt'] if ground_truth else None)
        assert aug.path == 'fused'
        names = ['image1', 'loss_image', 'sparse'] + (['validity'] if validity else []) + (['ground_truth'] if ground_truth else [])
        got = [t for t in out if t is not None]
        assert len(got) == len(names) and (out[3] is None) == (not validity) and (out[4] is None) == (not ground_truth)
        for name, a, b in zip(names, got, [image1] + list(staged)):
            assert a.shape == b.shape and a.dtype == b.dtype
            bad = int((a != b).sum())
            assert torch.equal(a, b), '%s (%s image): %d of %d values differ, largest difference %g' % (name, kind, bad, a.numel(), float((a - b).abs().max()))
        if moves and kind == 'fractional':
            for a, b in zip(got[1:], [image] + maps):
                assert a.shape == b.shape and not torch.equal(a, b) and bool((a != 0).any())
            assert not torch.equal(got[0], got[1])
    return aug


def cycle(values, n):
    return [values[i % len(values)] for i in range(n)]


@pytest.mark.parametrize('size', SIZES)
def test_each_geometric_stage_alone_and_all_together(size):
    n, H, W = size
    fr = frames(*size)
    on, off = [1] * n, [0] * n
    jitter = pho_draw(n, brightness=on, contrast=on, saturation=on)                     # the adapt script's three
    draws = {
        'hflip': geo_draw(n, H, W, hflip=on),
        'vflip': geo_draw(n, H, W, vflip=on),
        'both flips': geo_draw(n, H, W, hflip=on, vflip=on),
        'rotate 5 / -5 / 33': geo_draw(n, H, W, rotate=on, angles=cycle([5.0, -5.0, 33.0], n)),
        'rotate -5 / 33 / 0': geo_draw(n, H, W, rotate=on, angles=cycle([-5.0, 33.0, 0.0], n)),
        'rotate 0': geo_draw(n, H, W, rotate=on, angles=[0.0] * n),
        'resize 1.0': geo_draw(n, H, W, resize=on, scale=1.0),
        'resize 1.5': geo_draw(n, H, W, resize=on, scale=1.5),
        'all': geo_draw(n, H, W, hflip=on, vflip=on, rotate=on, angles=cycle([33.0, 5.0, -5.0], n), resize=on, scale=1.5),
        'all, coins at 0': geo_draw(n, H, W, hflip=off, vflip=off, rotate=off, angles=cycle([33.0, 5.0, -5.0], n), resize=off, scale=1.5),
        'nothing configured': geo_draw(n, H, W),
    }
    for name, g in draws.items():
        for scaling in ((False, True) if g['resize'] is not None else (False,)):
            compare(fr, g, jitter, scaling=scaling, moves=(name == 'all' and H * W > 1000))


@pytest.mark.parametrize('size', SIZES[2:])
def test_per_sample_coins_mixed(size):
    n, H, W = size
    fr = frames(*size)
    alt, rev = cycle([1, 0], n), cycle([0, 1], n)
    g = geo_draw(n, H, W, hflip=alt, vflip=rev, rotate=rev, angles=cycle([5.0, -33.0, 1.25], n), resize=alt, scale=1.5)
    compare(fr, g, pho_draw(n, brightness=rev, contrast=alt, saturation=rev), scaling=True)
    g = geo_draw(n, H, W, hflip=rev, rotate=alt, angles=cycle([-5.0, 33.0, 2.5], n), resize=rev, scale=1.5)
    compare(fr, g, pho_draw(n, brightness=alt, contrast=rev, gamma=alt, hue=rev, saturation=alt))


def test_crop_with_offsets_at_both_ends():
    n, H, W = SIZES[3]
    fr = frames(n, H, W)
    on = [1] * n
    crop = (24, 40, [0, 16, 7], [24, 0, 11])                                            # 40 - 24 = 16 and 64 - 40 = 24 are the last starts
    jitter = pho_draw(n, brightness=on, contrast=on, saturation=on)
    compare(fr, geo_draw(n, 24, 40, crop=crop), jitter)
    compare(fr, geo_draw(n, 24, 40, crop=crop, hflip=[1, 0, 1], vflip=[0, 1, 1]), jitter)
    for scaling in (False, True):
        compare(fr, geo_draw(n, 24, 40, crop=crop, hflip=[1, 0, 1], vflip=[0, 1, 1], rotate=[1, 1, 0], angles=[5.0, -33.0, 5.0], resize=[1, 0, 1], scale=1.5),
                jitter, scaling=scaling)
    compare(fr, geo_draw(n, 24, 40, crop=crop, rotate=on, angles=[0.0, 5.0, -5.0], resize=on, scale=1.0), None)


@pytest.mark.parametrize('size', SIZES)
def test_photometric_options_alone_and_together(size):
    n, H, W = size
    fr = frames(*size)
    on = [1] * n
    g = geo_draw(n, H, W, hflip=on, rotate=on, angles=cycle([5.0, -5.0, 33.0], n), resize=on, scale=1.5)
    for key in RANGES:
        if key == 'gamma':                       # gamma alone is the float branch: with brightness configured (its coin at 0) it is the uint8 one
            compare(fr, g, pho_draw(n, gamma=on, brightness=[0] * n))
        else:
            compare(fr, g, pho_draw(n, **{key: on}))
            compare(fr, g, pho_draw(n, **{key: [0] * n}))                               # configured, not drawn: still truncated to 0..255
    compare(fr, g, pho_draw(n, brightness=on, contrast=on, gamma=on, hue=on, saturation=on))
    compare(fr, g, None)                                                                # no photometric object: image1 is the loss image
    aug = compare(fr, g, dict.fromkeys(KEYS), kinds=('fractional',))                    # an object with nothing configured: likewise
    out = aug.apply(fr['images']['fractional'], fr['sparse'])
    assert out[0] is out[1]


@pytest.mark.parametrize('size', SIZES[1:])
def test_nearest_image(size):
    n, H, W = size
    fr = frames(*size)
    on = [1] * n
    g = geo_draw(n, H, W, hflip=on, vflip=cycle([0, 1], n), rotate=on, angles=cycle([33.0, -5.0, 5.0], n), resize=on, scale=1.5)
    compare(fr, g, pho_draw(n, brightness=on, contrast=on, saturation=on), modes=('nearest',) * 4, scaling=True)
    compare(fr, g, None, modes=(0, 0, 0, 0))


def test_missing_maps_leave_the_other_outputs_unchanged():
    n, H, W = SIZES[2]
    fr = frames(n, H, W)
    on = [1] * n
    g = geo_draw(n, H, W, hflip=on, rotate=on, angles=[5.0, -33.0], resize=on, scale=1.5)
    p = pho_draw(n, brightness=on, contrast=on, saturation=on)
    full = [t.clone() for t in compare(fr, g, p, kinds=('fractional',)).apply(fr['images']['fractional'], fr['sparse'], fr['valid'], fr['gt'])]
    for validity, ground_truth in ((False, False), (True, False), (False, True)):
        aug = compare(fr, g, p, kinds=('fractional',), validity=validity, ground_truth=ground_truth, scaling=False)
        out = aug.apply(fr['images']['fractional'], fr['sparse'], fr['valid'] if validity else None, fr['gt'] if ground_truth else None)
        for a, b in zip(out, full):
            assert a is None or torch.equal(a, b)
        assert (out[3] is None) == (not validity) and (out[4] is None) == (not ground_truth)


def test_grey_sums_of_more_than_256_blocks():
    """258 x 260 pixels are 263 blocks: the last block adds more than one stored sum into a slot, and the contrast mean needs them all."""
    n, H, W = 1, 258, 260
    fr = frames(n, H, W)
    g = geo_draw(n, H, W, hflip=[1], rotate=[1], angles=[5.0], resize=[1], scale=1.5)
    for _ in range(2):                           # twice on one workspace: the arrival counter is back at zero
        compare(fr, g, pho_draw(n, brightness=[1], contrast=[1], saturation=[1]), kinds=('fractional',))


def test_workspace_is_reused_and_a_noise_draw_takes_the_staged_route():
    n, H, W = SIZES[2]
    fr = frames(n, H, W)
    on = [1] * n
    geo = Transforms()
    pho = Transforms(random_brightness=[0.6, 1.4], random_noise_type='gaussian', random_noise_spread=0.1)
    aug = StepAugmenter(geo, pho, MODES)
    g = geo_draw(n, H, W, hflip=on, rotate=on, angles=[5.0, -5.0])
    p = pho_draw(n, brightness=on)
    aug.last_draw = (g, p)
    first = aug.apply(fr['images']['integer'], fr['sparse'], fr['valid'], fr['gt'])
    ptrs = [t.data_ptr() for t in first]
    again = aug.apply(fr['images']['fractional'], fr['sparse'], fr['valid'], fr['gt'])
    assert aug.path == 'fused' and [t.data_ptr() for t in again] == ptrs                # no allocation per call
    noisy = dict(p, noise=(u8(on), [torch.randn(n, 3, H, W, generator=torch.Generator().manual_seed(3))]))
    aug.last_draw = (g, noisy)
    out = aug.apply(fr['images']['fractional'], fr['sparse'], fr['valid'], fr['gt'])
    assert aug.path == 'staged'
    staged = geo.apply([fr['images']['fractional'], fr['sparse'], fr['valid'], fr['gt']], g, MODES)
    image1 = pho.apply([staged[0]], noisy)[0]
    for a, b in zip(out, [image1] + list(staged)):
        assert torch.equal(a, b)
    few = StepAugmenter(geo, pho, MODES[:2])                                            # fewer modes than tensors: the staged calls, as given
    few.last_draw = (geo_draw(n, H, W, hflip=on), p)
    out = few.apply(fr['images']['fractional'], fr['sparse'], fr['valid'], fr['gt'])
    staged = geo.apply([fr['images']['fractional'], fr['sparse'], fr['valid'], fr['gt']], few.last_draw[0], MODES[:2])
    assert few.path == 'staged' and all(torch.equal(a, b) for a, b in zip(out, [pho.apply([staged[0]], p)[0]] + list(staged)))
    with pytest.raises(ValueError, match='hue_factor'):
        aug.last_draw = (g, dict(p, hue=(u8(on), torch.tensor([0.6, 0.0]))))
        aug.apply(fr['images']['fractional'], fr['sparse'])


SENTINEL = -12345.0
PAD = 64


class Direct(object):
    """ptta_augment_frames called directly, every output inside a buffer with sentinel margins."""

    def __init__(self, n, H, W, h, w):
        self.lib = _lib.load()
        self.n, self.h, self.w = n, h, w
        fr = frames(n, H, W)
        self.inputs = [fr['images']['fractional'], fr['sparse'], fr['valid'], fr['gt']]
        self.bufs = [torch.full((PAD + n * c * h * w + PAD,), SENTINEL, device='cuda') for c in (3, 1, 1, 1, 3)]
        self.bytes = int(self.lib.ptta_augment_scratch_bytes(n, h, w))
        self.scratch = torch.zeros(self.bytes // 8, dtype=torch.float64, device='cuda')
        self.records = torch.zeros(n * DRAW_DTYPE.itemsize, dtype=torch.uint8, device='cuda')
        a = _lib.AugmentArgs()
        a.image, a.sparse_depth, a.validity_map, a.ground_truth = [t.data_ptr() for t in self.inputs]
        a.loss_image, a.sparse_depth_out, a.validity_map_out, a.ground_truth_out, a.image1 = [b[PAD:].data_ptr() for b in self.bufs]
        a.draws = self.records.data_ptr()
        a.n, a.height, a.width, a.crop_height, a.crop_width = n, H, W, h, w
        a.image_bilinear, a.scale_depth, a.pass2 = 1, 0, 1
        a.scratch, a.scratch_bytes = self.scratch.data_ptr(), self.bytes
        self.args = a

    def call(self, **changed):
        a = _lib.AugmentArgs()
        ctypes.memmove(ctypes.byref(a), ctypes.byref(self.args), ctypes.sizeof(a))
        for k, v in changed.items():
            setattr(a, k, v)
        rc = self.lib.ptta_augment_frames(ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return all(bool((b == SENTINEL).all()) for b in self.bufs)

    def margins_intact(self):
        return all(bool((b[:PAD] == SENTINEL).all()) and bool((b[-PAD:] == SENTINEL).all()) for b in self.bufs)


def test_argument_errors_return_minus_22_before_any_launch():
    n, H, W = SIZES[2]
    d = Direct(n, H, W, H, W)
    a = d.args
    assert d.bytes >= 8 * 256 * n and d.lib.ptta_augment_scratch_bytes(0, H, W) == -22 and d.lib.ptta_augment_scratch_bytes(65536, H, W) == -22
    refused = [dict(image=None), dict(loss_image=None), dict(draws=None), dict(n=0), dict(n=65536), dict(n=-1), dict(height=0), dict(crop_width=0),
               dict(crop_height=H + 1), dict(crop_width=W + 1), dict(scratch=None), dict(scratch_bytes=d.bytes - 8), dict(scratch_bytes=8 * 256 * n - 8),
               dict(scratch=a.scratch + 4), dict(sparse_depth=None), dict(ground_truth_out=None), dict(validity_map=None),
               dict(loss_image=a.image), dict(image1=a.loss_image), dict(sparse_depth_out=a.sparse_depth), dict(validity_map_out=a.ground_truth_out),
               dict(loss_image=a.image + 4 * (n * 3 * H * W - 1)), dict(image1=a.scratch), dict(ground_truth_out=a.draws)]
    for changed in refused:
        assert d.call(**changed) == -22, changed
        assert d.lib.ptta_last_error(None).decode().startswith('ptta_augment_frames'), changed
        assert d.untouched(), changed
    assert d.lib.ptta_augment_frames(None, None) == -22
    # the same arguments unchanged are accepted; without image1 no scratch is needed
    assert d.call() == 0 and d.margins_intact() and not d.untouched()
    assert d.call(image1=None, scratch=None, scratch_bytes=0) == 0 and d.margins_intact()
    # the wrapper raises on what the library refuses: a crop larger than the frame
    aug = StepAugmenter(Transforms())
    aug.last_draw = (geo_draw(n, H + 1, W, crop=(H + 1, W, [0] * n, [0] * n)), None)
    with pytest.raises(RuntimeError, match='larger than the frame'):
        aug.apply(d.inputs[0], d.inputs[1])
    with pytest.raises(RuntimeError, match='draw first'):
        StepAugmenter(Transforms()).apply(d.inputs[0], d.inputs[1])


@pytest.mark.parametrize('bilinear', [1, 0])
def test_degenerate_records_stay_inside_their_sample(bilinear):
    """Records no draw produces (resize sizes of zero and below, starts far outside, angles that are not finite): every gather index is
    clamped into the cropped window, so the launch completes, writes every output and nothing beside them."""
    n, H, W, h, w = 3, 40, 64, 24, 40
    d = Direct(n, H, W, h, w)
    rec = np.zeros(n, dtype=DRAW_DTYPE)
    rec['flags'] = 511
    rec['crop_y'], rec['crop_x'] = [-5, 10 ** 9, 17], [10 ** 9, -(2 ** 31), 25]
    rec['angle_deg'] = [np.nan, np.inf, 1.0e30]
    rec['resize_height'], rec['resize_width'] = [0, -3, 2 ** 31 - 1], [0, 1, -(2 ** 31)]
    rec['resize_y'], rec['resize_x'] = [-100, 2 ** 30, -(2 ** 31)], [2 ** 31 - 1, -7, 2 ** 30]
    rec['brightness'], rec['contrast'], rec['gamma'], rec['hue'], rec['saturation'] = [np.nan, np.inf, -1.0], [1.0e30, np.nan, 0.0], 1.0, 0.0, [np.inf, 1.0, np.nan]
    d.records.copy_(torch.from_numpy(rec.view(np.uint8)))
    for scale_depth in (0, 1):
        assert d.call(image_bilinear=bilinear, scale_depth=scale_depth) == 0
        assert d.margins_intact()
        assert all(bool((b[PAD:-PAD] != SENTINEL).all()) for b in d.bufs)               # every output value was written
