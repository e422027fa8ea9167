"""The augmentation of one inner-loop iteration (src/tta_main.py:595-604): the geometric transform of [image, sparse depth, validity
map, ground truth], then the photometric transform of the transformed image.  `StepAugmenter.draw` makes the two draws in the reference's
order with `Transforms.draw`; `StepAugmenter.apply` moves the data.

For the draws the adapt scripts enable -- crop to shape, flips, rotation, resize-and-crop, brightness / contrast / gamma / hue /
saturation -- `apply` is ONE host-to-device copy of the packed draw records and one launch (csrc/augment_fused.hip, ptta_augment_frames),
two when contrast / gamma / hue / saturation came up, into a workspace allocated once per shape.  Every output equals the staged
`Transforms.apply` calls bit for bit (tests/test_gpu_augment_fused.py).  Any other draw (noise, crop-and-pad, resize-and-pad, patch removal,
gamma as the only photometric option, an image that is not 3-channel, fewer interpolation modes than tensors, a map that is not sampled
nearest) takes those staged calls: `path` says which route the last call took."""
import ctypes

import numpy as np
import torch

from . import _lib

# include/ptta.h ptta_augment_draw, field by field (52 bytes, no padding)
DRAW_DTYPE = np.dtype([('flags', '<u4'), ('crop_y', '<i4'), ('crop_x', '<i4'), ('angle_deg', '<f4'), ('resize_height', '<i4'), ('resize_width', '<i4'),
                       ('resize_y', '<i4'), ('resize_x', '<i4'), ('brightness', '<f4'), ('contrast', '<f4'), ('gamma', '<f4'), ('hue', '<f4'),
                       ('saturation', '<f4')])
assert DRAW_DTYPE.itemsize == 52

_PHOTO = (('brightness', _lib.PTTA_AUG_BRIGHTNESS), ('contrast', _lib.PTTA_AUG_CONTRAST), ('gamma', _lib.PTTA_AUG_GAMMA), ('hue', _lib.PTTA_AUG_HUE),
          ('saturation', _lib.PTTA_AUG_SATURATION))
_PASS2 = _lib.PTTA_AUG_CONTRAST | _lib.PTTA_AUG_GAMMA | _lib.PTTA_AUG_HUE | _lib.PTTA_AUG_SATURATION
_GEOMETRIC = ('crop', 'hflip', 'vflip', 'rotate', 'resize')
_STAGED_ONLY = ('noise', 'crop_pad', 'resize_pad', 'remove')
_NEAREST, _BILINEAR = ('nearest', 0), ('bilinear', 2)


def _np(t, dtype):
    return np.asarray(t.numpy() if torch.is_tensor(t) else t).astype(dtype)


def pack_draw(geo_draw, pho_draw, n, out=None):
    """The n ptta_augment_draw records of a geometric and a photometric `Transforms.draw` result (pho_draw may be None): a numpy structured
    array of DRAW_DTYPE (written into `out` when given).  A transform that is not configured (None) leaves its fields zero and its flag
    clear; one whose coin is 0 for a sample keeps its values and has its flag clear.  The angle is the fp32 value `Transforms.apply` uploads."""
    rec = np.zeros(n, dtype=DRAW_DTYPE) if out is None else out
    if out is not None:
        rec[...] = np.zeros((), dtype=DRAW_DTYPE)
    flags = np.zeros(n, dtype=np.uint32)
    if geo_draw.get('crop') is not None:
        rec['crop_y'], rec['crop_x'] = _np(geo_draw['crop'][2], np.int32), _np(geo_draw['crop'][3], np.int32)
    for key, bit in (('hflip', _lib.PTTA_AUG_HFLIP), ('vflip', _lib.PTTA_AUG_VFLIP)):
        if geo_draw.get(key) is not None:
            flags |= np.where(_np(geo_draw[key], np.uint8) != 0, np.uint32(bit), np.uint32(0))
    if geo_draw.get('rotate') is not None:
        do, angle = geo_draw['rotate']
        flags |= np.where(_np(do, np.uint8) != 0, np.uint32(_lib.PTTA_AUG_ROTATE), np.uint32(0))
        rec['angle_deg'] = _np(angle.float() if torch.is_tensor(angle) else angle, np.float32)
    if geo_draw.get('resize') is not None:
        do, rh, rw, sy, sx = geo_draw['resize'][:5]
        flags |= np.where(_np(do, np.uint8) != 0, np.uint32(_lib.PTTA_AUG_RESIZE), np.uint32(0))
        for name, v in (('resize_height', rh), ('resize_width', rw), ('resize_y', sy), ('resize_x', sx)):
            rec[name] = _np(v, np.int32)
    if pho_draw is not None:
        for key, bit in _PHOTO:
            if pho_draw.get(key) is not None:
                do, factor = pho_draw[key]
                flags |= np.where(_np(do, np.uint8) != 0, np.uint32(bit), np.uint32(0))
                rec[key] = _np(factor, np.float32)
    rec['flags'] = flags
    return rec


def fused_eligible(geo_draw, pho_draw, interpolation_modes):
    """Whether the one-launch route covers these draws: only crop / flip / rotation / resize-and-crop in the geometric draw, only the five
    photometric options in the photometric one (and not gamma alone: the reference leaves the image float then), one interpolation mode
    for each of [image, sparse depth, validity map, ground truth], 'nearest' or 'bilinear' for the image and 'nearest' for every map."""
    modes = list(interpolation_modes)
    if len(modes) < 4 or modes[0] not in _NEAREST + _BILINEAR or any(m not in _NEAREST for m in modes[1:4]):
        return False
    if any(geo_draw.get(k) is not None for k in _STAGED_ONLY) or any(geo_draw.get(k) is not None for k, _ in _PHOTO):
        return False
    if pho_draw is not None:
        if any(pho_draw.get(k) is not None for k in _STAGED_ONLY + _GEOMETRIC):
            return False
        if pho_draw.get('gamma') is not None and all(pho_draw.get(k) is None for k in ('brightness', 'contrast', 'hue', 'saturation')):
            return False
    return True


class _Workspace(object):
    """Everything one shape of `apply` needs, allocated once: the outputs, the pinned record buffer with its device copy, the scratch."""

    def __init__(self, lib, device, n, h, w, have):
        f32 = dict(device=device, dtype=torch.float32)
        self.loss_image = torch.empty((n, 3, h, w), **f32)
        self.image1 = torch.empty((n, 3, h, w), **f32)
        self.maps = [torch.empty((n, 1, h, w), **f32) if on else None for on in have]
        self.host = torch.zeros(n * DRAW_DTYPE.itemsize, dtype=torch.uint8).pin_memory()
        self.records = self.host.numpy().view(DRAW_DTYPE)
        self.device_records = torch.empty(n * DRAW_DTYPE.itemsize, device=device, dtype=torch.uint8)
        self.scratch_bytes = int(lib.ptta_augment_scratch_bytes(n, h, w))
        if self.scratch_bytes <= 0:
            raise RuntimeError('ptta_augment_scratch_bytes failed (%d)' % self.scratch_bytes)
        self.scratch = torch.zeros(self.scratch_bytes // 8, device=device, dtype=torch.float64)      # the arrival counters start at zero
        self.copied = torch.cuda.Event()
        self.in_flight = False


class StepAugmenter(object):
    """transforms_geometric / transforms_photometric: `proxytta.transforms.Transforms` objects as src/tta_main.py:445-461 builds them (the
    photometric one may be None: image1 is then the geometrically transformed image).  interpolation_modes: one per tensor of [image,
    sparse depth, validity map, ground truth] (src/tta_main.py:471-473).  The route is chosen per call from the draws alone: one launch
    where they allow it (measured faster at N = 1 and N = 4, profiles/augment_loop.txt), the staged calls otherwise."""

    def __init__(self, transforms_geometric, transforms_photometric=None, interpolation_modes=('bilinear', 'nearest', 'nearest', 'nearest')):
        self.geo, self.pho = transforms_geometric, transforms_photometric
        self.interpolation_modes = tuple(interpolation_modes)
        self.last_draw = None
        self.path = None
        self._generator = None
        self._ws = {}

    def draw(self, n, height, width, random_transform_probability, generator=None):
        """The geometric draw, then the photometric one on the size the geometry leaves (the reference's order, src/tta_main.py:595-604:
        the same consumption of torch's generator and of numpy's global state).  Returns and keeps (geo_draw, pho_draw) in `last_draw`."""
        g = self.geo.draw(n, height, width, random_transform_probability, generator, channels=(3, 1, 1, 1))
        self.geo.last_draw = g
        p = None
        if self.pho is not None:
            ph, pw = (g['crop'][0], g['crop'][1]) if g['crop'] is not None else (height, width)
            p = self.pho.draw(n, ph, pw, random_transform_probability, generator, channels=(3,))
            self.pho.last_draw = p
        self.last_draw = (g, p)
        self._generator = generator
        return self.last_draw

    # ---- data movement ----------------------------------------------------------------------------
    def apply(self, image, sparse_depth, validity_map=None, ground_truth=None):
        """The frame through `last_draw`: (image1, loss_image, sparse_depth, validity_map, ground_truth), a None map coming back None.
        On the fused route the outputs live in a workspace allocated once per shape and are valid until the next `apply`."""
        if self.last_draw is None:
            raise RuntimeError('StepAugmenter.apply: call draw first')
        g, p = self.last_draw
        maps = [sparse_depth, validity_map, ground_truth]
        if sparse_depth is None:
            raise ValueError('StepAugmenter.apply: sparse_depth is required')
        for t in [image] + [m for m in maps if m is not None]:
            if not t.is_cuda:
                raise RuntimeError('proxytta.StepAugmenter moves data on the GPU only (no CPU fallback)')
        fused = (fused_eligible(g, p, self.interpolation_modes) and image.ndim == 4 and image.shape[1] == 3 and
                 all(m is None or (m.ndim == 4 and m.shape[1] == 1 and m.shape[0] == image.shape[0] and m.shape[2:] == image.shape[2:]) for m in maps))
        if not fused:
            self.path = 'staged'
            return self._apply_staged(image, maps, g, p)
        self.path = 'fused'
        return self._apply_fused(image, maps, g, p)

    def _apply_staged(self, image, maps, g, p):
        """Today's calls: geo.apply on the tensors that are there, pho.apply on the transformed image."""
        present = [i for i, m in enumerate(maps) if m is not None]
        modes = list(self.interpolation_modes)
        if len(modes) >= 4:                       # one mode per tensor: keep each tensor's own when a map is left out
            modes = [modes[0]] + [modes[1 + i] for i in present]
        out = self.geo.apply([image] + [maps[i] for i in present], g, modes, generator=self._generator)
        loss_image = out[0]
        image1 = loss_image if p is None else self.pho.apply([loss_image], p, generator=self._generator)[0]
        res = [None, None, None]
        for i, t in zip(present, out[1:]):
            res[i] = t
        return (image1, loss_image) + tuple(res)

    def _apply_fused(self, image, maps, g, p):
        lib = _lib.load()
        n, _, H, W = image.shape
        h, w = (int(g['crop'][0]), int(g['crop'][1])) if g['crop'] is not None else (H, W)
        if p is not None and p.get('hue') is not None and bool(((p['hue'][1] < -0.5) | (p['hue'][1] > 0.5)).any()):
            raise ValueError('hue_factor is not in [-0.5, 0.5].')                     # torchvision's adjust_hue, as Transforms.apply
        have = tuple(m is not None for m in maps)
        key = (image.device, n, H, W, h, w, have)
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = _Workspace(lib, image.device, n, h, w, have)
        src = [t if t is None or (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous() for t in [image] + maps]
        if ws.in_flight:
            ws.copied.synchronize()               # the previous call's copy has read the pinned buffer (normally long done)
        rec = pack_draw(g, p, n, out=ws.records)
        photo = p is not None and any(p.get(k) is not None for k, _ in _PHOTO)
        pass2 = photo and bool((rec['flags'] & np.uint32(_PASS2)).any())
        ws.device_records.copy_(ws.host, non_blocking=True)
        ws.copied.record()
        ws.in_flight = True
        modes = self.interpolation_modes
        a = _lib.AugmentArgs()
        a.image, a.sparse_depth, a.validity_map, a.ground_truth = [t.data_ptr() if t is not None else None for t in src]
        a.loss_image = ws.loss_image.data_ptr()
        a.sparse_depth_out, a.validity_map_out, a.ground_truth_out = [t.data_ptr() if t is not None else None for t in ws.maps]
        a.image1 = ws.image1.data_ptr() if photo else None
        a.draws = ws.device_records.data_ptr()
        a.n, a.height, a.width, a.crop_height, a.crop_width = n, H, W, h, w
        a.image_bilinear = int(modes[0] in _BILINEAR)
        a.scale_depth = int(bool(self.geo.resize_scaling_depth))
        a.pass2 = int(pass2)
        a.scratch, a.scratch_bytes = ws.scratch.data_ptr(), ws.scratch_bytes
        rc = lib.ptta_augment_frames(ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError('ptta_augment_frames failed (%d): %s' % (rc, lib.ptta_last_error(None).decode()))
        self._keep = src                          # converted copies stay alive until the next call
        return (ws.image1 if photo else ws.loss_image, ws.loss_image) + tuple(ws.maps)


__all__ = ['StepAugmenter', 'pack_draw', 'fused_eligible', 'DRAW_DTYPE']
