"""Raw-frame ingest on the device (include/ptta.h ptta_ingest_raw): the reference's loader hands every frame over as fp32 -- an RGB PNG
decoded to uint8 H x W x 3 becomes np.asarray(image, np.float32) transposed to CHW (src/data_utils.py:150-158, src/datasets.py:399-407), a
16-bit depth PNG becomes z / 256.0 with v[z > 0] = 1 (:182-188, :219-223), cropped on the host (src/datasets.py:83-170) -- 16 bytes per
pixel across the host link.  Here the arrays travel as decoded, 5 bytes per pixel, and ONE launch writes the fp32 planes the step,
ptta_outlier_removal, ptta_crop_flip and ptta_set_image_norm (which expects the raw 0-255 image) read.

    planes = ingest_raw(image_u8, sparse_u16, size=(352, 1216), start=(sy, sx))
    engine.step(planes['image'], planes['sparse'], validity=planes['validity'])

PyTorch supplies the tensors and the stream (plumbing); no arithmetic happens here, and there is no CPU fallback.
"""
import torch

from . import _lib
from ._lib import ptr

PLANES = ('image', 'sparse', 'validity', 'gt', 'gt_validity')
_U16 = (torch.int16, torch.uint16)          # a 16-bit plane is read as unsigned whichever of the two dtypes carries it


def _stream_handle(stream):
    if stream is None:
        return torch.cuda.current_stream().cuda_stream
    return stream.cuda_stream if hasattr(stream, 'cuda_stream') else int(stream)


def _start_tensor(v, n, device):
    if v is None or torch.is_tensor(v):
        return v
    return torch.as_tensor([int(v)] * n if isinstance(v, int) else [int(i) for i in v], dtype=torch.int32).to(device)


def ingest_raw(image_u8=None, sparse_u16=None, gt_u16=None, size=None, start=None, multiplier=256.0, out=None, stream=None):
    """image_u8: N x H x W x 3 uint8; sparse_u16, gt_u16: N x H x W int16 / uint16 (read as unsigned); all device tensors, any of them None.
    size = (height, width) of the window (default: the whole source); start = (start_y, start_x), each an int32 device tensor of N
    entries, a sequence of N ints or one int (ints are uploaded here: keep tensors for a hot loop), None = 0; starts are clamped into
    the sample as ptta_crop_flip clamps them.  Returns a dict of fp32 device tensors, N x 3 x height x width for 'image' and
    N x 1 x height x width for 'sparse', 'validity', 'gt', 'gt_validity': every plane of the inputs given, or, with `out` (a dict of
    preallocated contiguous fp32 tensors), exactly the planes `out` names -- e.g. 'sparse' without 'validity'.  Enqueues one launch on
    `stream` (default: the current stream); raises RuntimeError('ptta_ingest_raw failed (-22)') for what include/ptta.h lists."""
    lib = _lib.load()
    given = [t for t in (image_u8, sparse_u16, gt_u16) if t is not None]
    for t in given:
        if not t.is_cuda:
            raise RuntimeError('ingest_raw takes device tensors (there is no CPU fallback)')
    if image_u8 is not None and (image_u8.dtype != torch.uint8 or image_u8.dim() != 4 or image_u8.shape[-1] != 3):
        raise TypeError('image_u8 must be an N x H x W x 3 uint8 tensor')
    for t in (sparse_u16, gt_u16):
        if t is not None and (t.dtype not in _U16 or t.dim() != 3):
            raise TypeError('sparse_u16 / gt_u16 must be N x H x W int16 or uint16 tensors')
    n, H, W = (int(v) for v in given[0].shape[:3]) if given else (0, 0, 0)
    for t in given:
        if tuple(t.shape[:3]) != (n, H, W):
            raise ValueError('the inputs must share N, H and W')
    h, w = (H, W) if size is None else (int(size[0]), int(size[1]))
    device = given[0].device if given else (next(iter(out.values())).device if out else torch.device('cuda'))
    if out is None:
        def plane(channels):
            return torch.empty((n, channels, h, w), dtype=torch.float32, device=device)
        out = {}
        if n >= 1 and h >= 1 and w >= 1:            # (sizes the library refuses get no planes: it refuses the call below)
            if image_u8 is not None:
                out['image'] = plane(3)
            if sparse_u16 is not None:
                out['sparse'], out['validity'] = plane(1), plane(1)
            if gt_u16 is not None:
                out['gt'], out['gt_validity'] = plane(1), plane(1)
    else:
        unknown = set(out) - set(PLANES)
        if unknown:
            raise KeyError('unknown output plane(s) %s (planes: %s)' % (sorted(unknown), ', '.join(PLANES)))
        out = {k: out[k] for k in PLANES if out.get(k) is not None}
        for k, t in out.items():
            if t.dtype != torch.float32 or not t.is_cuda or (n and h > 0 and w > 0 and tuple(t.shape) != (n, 3 if k == 'image' else 1, h, w)):
                raise ValueError("out[%r] must be a contiguous fp32 device tensor of shape N x %d x height x width" % (k, 3 if k == 'image' else 1))
    sy, sx = (None, None) if start is None else (_start_tensor(start[0], n, device), _start_tensor(start[1], n, device))
    for t in (sy, sx):
        if t is not None and (t.dtype != torch.int32 or not t.is_cuda or t.numel() != n):
            raise ValueError('start_y / start_x must be int32 device tensors of N entries')
    rc = lib.ptta_ingest_raw(ptr(image_u8), ptr(sparse_u16), ptr(gt_u16), *[ptr(out.get(k)) for k in PLANES], n, H, W, h, w,
                             ptr(sy), ptr(sx), float(multiplier), _stream_handle(stream))
    if rc != 0:
        raise RuntimeError('ptta_ingest_raw failed (%d)' % rc)
    return out
