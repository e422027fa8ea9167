"""Eval-time hole filling of the NLSPN adapter (src/nlspn_model_adapt.py:124-127 -> src/data_utils.py:327-354 `inpainting`):
pixels whose predicted depth is exactly 0 (the clamp at nlspnmodel_adapt.py:371) are filled by biharmonic inpainting.  The
reference does this on the CPU with scikit-image's `restoration.inpaint_biharmonic` -- a third-party dependency absent from the
reference tree and from this image (PARITY UNPINNED): its published algorithm is restated here on scipy, host-side like the
reference's (the depth map is on its way to the CPU metrics anyway, src/tta_main.py:769).

skimage.restoration.inpaint_biharmonic(image, mask) for a single-channel N-d image:
  * the mask is split into independent regions: connected components (full connectivity) of the mask dilated by one pixel
    (cross-shaped structuring element), restricted to the mask;
  * for every masked point the biharmonic stencil is laplace(laplace(delta)) evaluated on the radius-2 neighbourhood box clipped
    to the image (scipy.ndimage.laplace, 'reflect' boundaries); coefficients on masked points form the unknown matrix, on known
    points the right-hand side;
  * the sparse system is solved directly and the result clipped to [min, max] of the known pixels.
The reference passes each sample as a (1, H, W) array, i.e. a 3-D image one voxel thick: the clipped stencil has extent 1 along
that axis and reduces to the 2-D biharmonic operator.

`inpainting_device` at the end of this file is the same filling on the device (csrc/inpaint.hip); the functions above are its definition
and its fallback.
"""
import ctypes

import numpy as np
import scipy.ndimage as ndi
from scipy import sparse
from scipy.sparse.linalg import spsolve


def _inpaint_region(mask, out, limits):
    pts = np.stack(np.where(mask), axis=-1)
    index = -np.ones(mask.shape, dtype=np.int64)
    index[mask] = np.arange(len(pts))
    shape = np.array(out.shape)
    rows_u, cols_u, vals_u = [], [], []
    rhs = np.zeros(len(pts), dtype=np.float64)
    cache = {}
    for n, pt in enumerate(pts):
        lo, hi = np.maximum(pt - 2, 0), np.minimum(pt + 3, shape)
        key = (tuple(pt - lo), tuple(hi - lo))
        coef = cache.get(key)
        if coef is None:                                  # the stencil depends only on the box and the point's place in it
            delta = np.zeros(hi - lo)
            delta[tuple(pt - lo)] = 1
            coef = ndi.laplace(ndi.laplace(delta))
            cache[key] = coef
        box = tuple(slice(a, b) for a, b in zip(lo, hi))
        idx, known = index[box], out[box]
        nz = coef != 0
        unk = nz & (idx >= 0)
        rows_u += [n] * int(unk.sum()); cols_u += idx[unk].tolist(); vals_u += coef[unk].tolist()
        kn = nz & (idx < 0)
        rhs[n] = -float((coef[kn] * known[kn].astype(np.float64)).sum())
    A = sparse.csr_matrix((vals_u, (rows_u, cols_u)), shape=(len(pts), len(pts)))
    res = np.clip(np.asarray(spsolve(A.tocsc(), rhs)).ravel(), *limits)
    out[mask] = res
    return out


def inpaint_biharmonic(image, mask):
    """image, mask: same-shape arrays (any dimensionality); returns a copy with the masked points filled."""
    image = np.asarray(image)
    mask = np.asarray(mask).astype(bool)
    if image.shape != mask.shape:
        raise ValueError('Input arrays have to be the same shape')
    out = np.copy(image)
    if not mask.any():
        return out
    if mask.all():
        raise ValueError('nothing to inpaint from: every pixel is masked')
    known = image[~mask]
    limits = (float(known.min()), float(known.max()))
    dil = ndi.binary_dilation(mask, structure=ndi.generate_binary_structure(mask.ndim, 1))
    labeled, num = ndi.label(dil, structure=np.ones((3,) * mask.ndim))
    labeled = labeled * mask
    for r in range(1, num + 1):
        region = labeled == r
        if region.any():
            _inpaint_region(region, out, limits)
    return out


def inpainting(depth_map):
    """src/data_utils.py:327-354: depth_map N x 1 x H x W (numpy, modified in place and returned); holes = exact zeros."""
    if not (depth_map == 0).any():
        return depth_map
    for i in range(depth_map.shape[0]):
        depth = depth_map[i, ...]
        depth_map[i] = inpaint_biharmonic(depth, depth == 0)
    return depth_map


_device_buffers = {}


def inpainting_device(depth_tensor, max_unknowns=65536, max_iter=2000, rtol=1e-12):
    """`inpainting` on the device (include/ptta.h ptta_inpaint_biharmonic): depth_tensor is a contiguous N x 1 x H x W fp32 CUDA tensor,
    filled in place on the current stream and returned.  The same system as above, one per sample, solved by conjugate gradients in fp64
    (stop at |r| <= rtol |b|, at most max_iter iterations: 2000 covers holes about 50 pixels across) and clipped and rounded as above: the
    filled values agree with the host's to the last fp32 bit or two.  Only the n status words come back to the host.  A sample the
    device did not fill (status < 0: not converged or a breakdown, more than max_unknowns holes, every pixel a hole) is left as it was by
    the kernel and goes through `inpaint_biharmonic` on the host, which raises ValueError for a sample without a known pixel.
    Returns the tensor; `inpainting_device.last_status` holds the status words of the last call (a list)."""
    import torch
    from . import _lib
    from ._lib import ptr
    lib = _lib.load()
    t = depth_tensor
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] == 1 and t.is_contiguous()):
        raise ValueError('inpainting_device takes a contiguous N x 1 x H x W fp32 CUDA tensor')
    n, _, h, w = t.shape
    key = (t.device, n, h, w, int(max_unknowns))
    if key not in _device_buffers:
        size = lib.ptta_inpaint_scratch_bytes(n, h, w, int(max_unknowns))
        if size < 0:
            raise RuntimeError('ptta_inpaint_scratch_bytes failed (%d)' % size)
        _device_buffers[key] = (torch.empty((size + 7) // 8, device=t.device, dtype=torch.float64), torch.empty(n, device=t.device, dtype=torch.int32))
    scratch, status = _device_buffers[key]
    rc = lib.ptta_inpaint_biharmonic(ptr(t), n, h, w, int(max_unknowns), int(max_iter), float(rtol), ptr(scratch), scratch.numel() * 8, ptr(status),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise RuntimeError('ptta_inpaint_biharmonic failed (%d)' % rc)
    codes = status.cpu().tolist()                              # the one read-back; it also orders the host behind the launches
    inpainting_device.last_status = codes
    for i, code in enumerate(codes):
        if code < 0:
            depth = t[i].cpu().numpy()
            t[i].copy_(torch.from_numpy(inpaint_biharmonic(depth, depth == 0)))
    return t


inpainting_device.last_status = []
