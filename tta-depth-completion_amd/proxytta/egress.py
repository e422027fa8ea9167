"""Raw-frame egress on the device (include/ptta.h ptta_egress_raw), the inverse of proxytta/ingest.py: the reference stores a prediction
with save_depth = np.uint32(z * multiplier) written as a 16-bit PNG (src/data_utils.py:236-251), a validity map with save_validity_map
(:283-298) and an image with save_image (:29-78), each after a copy of the fp32 map to the host -- 4 bytes per pixel across the host link,
multiplied and cast on the host thread that also feeds the step.  Here ONE launch writes the stored frames on the card: the 16-bit map
(and the 8-bit HWC image) pasted into the dst_height x dst_width frame the window was cut from, zeros around it, 2 bytes per pixel to copy.

    planes = egress_raw(depth=depth, dst_size=(375, 1242), start=(sy, sx))
    u16 = planes['depth_u16'].cpu().numpy()             # Image.fromarray(u16[0]).save(path): the file save_depth writes

PyTorch supplies the tensors and the stream (plumbing); no arithmetic happens here, and there is no CPU fallback.
"""
import torch

from . import _lib
from ._lib import ptr
from .ingest import _start_tensor

PLANES = ('depth_u16', 'validity_u16', 'image_u8')
_U16 = (torch.int16, torch.uint16)          # a 16-bit plane is written as unsigned whichever of the two dtypes carries it


def egress_raw(depth=None, validity=None, image=None, dst_size=None, start=None, multiplier=256.0, image_scale=255.0, out=None):
    """depth, validity: N x 1 x h x w fp32; image: N x 3 x h x w fp32 (image_scale = 255 for an image in [0, 1], 1 for one in 0-255); all
    contiguous device tensors, any of them None.  dst_size = (dst_height, dst_width) of the stored frame (default: h x w, no border);
    start = (start_y, start_x), each an int32 device tensor of N entries, a sequence of N ints or one int (ints are uploaded here: keep
    tensors for a hot loop), None = 0: where the window lies in the frame, clamped into it as ptta_ingest_raw clamps.  Returns a dict of
    device tensors, 'depth_u16' and 'validity_u16' N x dst_height x dst_width torch.uint16 and 'image_u8' N x dst_height x dst_width x 3
    uint8, one per input given; with `out` (a dict of preallocated contiguous tensors under those keys, int16 storage allowed for the
    16-bit planes) those are written instead.  Every element is written, zeros outside the window.  Enqueues one launch on the current
    stream; raises RuntimeError with the library's reason for what include/ptta.h lists."""
    lib = _lib.load()
    given = {'depth': depth, 'validity': validity, 'image': image}
    present = [t for t in given.values() if t is not None]
    for name, t in given.items():
        if t is None:
            continue
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError('egress_raw takes device tensors (there is no CPU fallback)')
        channels = 3 if name == 'image' else 1
        if t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != channels or not t.is_contiguous():
            raise TypeError('%s must be a contiguous N x %d x h x w fp32 tensor' % (name, channels))
    n, h, w = (int(present[0].shape[0]), int(present[0].shape[2]), int(present[0].shape[3])) if present else (0, 0, 0)
    for t in present:
        if (int(t.shape[0]), int(t.shape[2]), int(t.shape[3])) != (n, h, w):
            raise ValueError('the inputs must share N, h and w')
    H, W = (h, w) if dst_size is None else (int(dst_size[0]), int(dst_size[1]))
    device = present[0].device if present else torch.device('cuda')
    pairs = (('depth', 'depth_u16'), ('validity', 'validity_u16'), ('image', 'image_u8'))
    if out is None:
        out = {}
        if n >= 1 and h >= 1 and w >= 1 and H >= h and W >= w:          # (sizes the library refuses get no planes: it refuses the call below)
            for src, key in pairs:
                if given[src] is not None:
                    out[key] = (torch.empty((n, H, W, 3), dtype=torch.uint8, device=device) if key == 'image_u8' else
                                torch.empty((n, H, W), dtype=torch.uint16, device=device))
    else:
        unknown = set(out) - set(PLANES)
        if unknown:
            raise KeyError('unknown output plane(s) %s (planes: %s)' % (sorted(unknown), ', '.join(PLANES)))
        out = {k: out[k] for k in PLANES if out.get(k) is not None}
        for k, t in out.items():
            want = (n, H, W, 3) if k == 'image_u8' else (n, H, W)
            ok = t.dtype == torch.uint8 if k == 'image_u8' else t.dtype in _U16
            if not ok or not t.is_cuda or not t.is_contiguous() or (n and tuple(t.shape) != want):
                raise ValueError('out[%r] must be a contiguous device tensor of shape %s, %s' % (k, ' x '.join(map(str, want)), 'uint8' if k == 'image_u8' else '16-bit'))
    sy, sx = (None, None) if start is None else (_start_tensor(start[0], n, device), _start_tensor(start[1], n, device))
    for t in (sy, sx):
        if t is not None and (t.dtype != torch.int32 or not t.is_cuda or t.numel() != n):
            raise ValueError('start_y / start_x must be int32 device tensors of N entries')
    rc = lib.ptta_egress_raw(ptr(depth), ptr(validity), ptr(image), *[ptr(out.get(k)) for k in PLANES], n, h, w, H, W, ptr(sy), ptr(sx),
                             float(multiplier), float(image_scale), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        why = lib.ptta_last_error(None)
        raise RuntimeError('ptta_egress_raw failed (%d)%s' % (rc, ': ' + why.decode() if rc == -22 and why else ''))
    return out
