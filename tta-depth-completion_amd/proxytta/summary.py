"""The summary panels of the plugin's log_summary composed on the device (include/ptta.h ptta_summary_compose, csrc/summary.hip): the
reference copies up to five fp32 maps to the host, colours each through a matplotlib colormap in a Python loop (src/log_utils.py:53-80),
and runs torch.cat and make_grid there (src/external_model_adapt.py:662-909).  Here one launch writes the finished grid -- as the fp32
3 x GH x GW tensor the reference hands to summary_writer.add_image, or as the uint8 GH x GW x 3 image the writer would make of it -- and
one copy leaves the card.

    grid = compose_grid(image=[image], output_depth=depth, sparse_depth=sparse, validity_map=validity, max_predict_depth=80.0,
                        n_image_per_summary=4)
    summary_writer.add_image(tag, grid.cpu(), global_step=step)

The two 256 x 3 colormap tables are matplotlib's (`matplotlib.colormaps[name].colors`); `register_colormap` installs a table by name so that
nothing on the GPU path needs matplotlib.  PyTorch supplies the tensors and the stream (plumbing); there is no CPU fallback.
"""
import ctypes

import torch

from . import _lib
from ._lib import ptr

_tables = {}           # name -> 256 x 3 float64 host tensor, as registered
_device_tables = {}    # (name, device) -> 256 x 3 float64 device tensor


def register_colormap(name, table):
    """Install the 256 x 3 table (anything torch.as_tensor takes, float64 RGB in 0..1) that `colormap_table(name)` returns."""
    t = torch.as_tensor(table, dtype=torch.float64)
    if tuple(t.shape) != (256, 3):
        raise ValueError('a colormap table is 256 x 3, got %s' % (tuple(t.shape),))
    _tables[name] = t.contiguous().clone()
    for key in [k for k in _device_tables if k[0] == name]:
        del _device_tables[key]


def colormap_table(name, device=None):
    """The 256 x 3 float64 table of colormap `name` on `device` (default: the current CUDA device), cached per device: the registered
    table, else matplotlib's `matplotlib.colormaps[name].colors`."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    key = (name, device)
    if key not in _device_tables:
        if name not in _tables:
            try:
                import matplotlib
            except ImportError:
                raise RuntimeError("no colormap table registered for %r and matplotlib is not installed: install matplotlib or call "
                                   "proxytta.summary.register_colormap(%r, table) with its 256 x 3 table" % (name, name))
            colors = getattr(matplotlib.colormaps[name], 'colors', None)
            if colors is None or len(colors) != 256:
                raise RuntimeError('matplotlib colormap %r is not a 256-entry listed colormap' % name)
            register_colormap(name, colors)
        _device_tables[key] = _tables[name].to(device)
    return _device_tables[key]


def grid_shape(n_show, height, width, n_rows):
    """(GH, GW) of the grid of n_show panels of n_rows rows (ptta_summary_grid_shape: pure host arithmetic)."""
    gh, gw = ctypes.c_int64(), ctypes.c_int64()
    rc = _lib.load().ptta_summary_grid_shape(int(n_show), int(height), int(width), int(n_rows), ctypes.byref(gh), ctypes.byref(gw))
    if rc != 0:
        raise RuntimeError('ptta_summary_grid_shape failed (%d)' % rc)
    return gh.value, gw.value


def reverse_normalization(normalized_image_range):
    """(rev_mean, rev_std) of the display transform (src/external_model_adapt.py:700-724), or None when the range asks for none: a
    mean/std range -- ((m0, m1, m2), (s0, s1, s2)) or the six numbers in a row -- gives (-m_c / s_c, 1 / s_c) in Python floats, which the
    kernel takes rounded to fp32 as torchvision's normalize does; a two-number range such as [0, 1], or None, gives None."""
    r = normalized_image_range
    if r is None:
        return None
    if not (any(isinstance(v, (tuple, list)) for v in r) or len(r) > 2):
        return None
    if len(r) > 2:
        k = len(r) // 2
        r = [tuple(r[:k]), tuple(r[k:])]
    return tuple(-m / s for m, s in zip(r[0], r[1])), tuple(1 / s for s in r[1])


def _stream_handle():
    return torch.cuda.current_stream().cuda_stream


def _checked(t, what, channels=None):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()):
        raise ValueError('%s must be a contiguous N x C x H x W fp32 device tensor (there is no CPU fallback)' % what)
    if channels is not None and t.shape[1] != channels:
        raise ValueError('%s must have %d channel(s)' % (what, channels))
    return t


def image_flag(image, flag=None):
    """The display transform's `torch.max(image) > 10.0` on the device (ptta_summary_image_flag): returns the int32 buffer whose word 0
    is 1 when some element of the WHOLE tensor is above 10 and none is NaN.  Two launches on the current stream; nothing comes back to the host."""
    _checked(image, 'image')
    if flag is None:
        flag = torch.empty(_lib.PTTA_SUMMARY_FLAG_WORDS, dtype=torch.int32, device=image.device)
    rc = _lib.load().ptta_summary_image_flag(ptr(image), image.numel(), ptr(flag), _stream_handle())
    if rc != 0:
        raise RuntimeError('ptta_summary_image_flag failed (%d)' % rc)
    return flag


def to_host(grid):
    """The grid as a CPU tensor after ONE device -> host copy, into page-locked memory from torch's caching host allocator (a pageable
    destination makes the runtime stage the copy through its own pinned buffer, several times slower for a 165 MB grid).  Each call
    returns a tensor of its own: a writer may keep it."""
    host = torch.empty(grid.shape, dtype=grid.dtype, pin_memory=True)
    with torch.cuda.device(grid.device):
        host.copy_(grid, non_blocking=True)                    # on the current stream, behind the compose launch
        torch.cuda.current_stream().synchronize()
    return host


def compose_grid(image=None, output_depth=None, sparse_depth=None, validity_map=None, ground_truth=None, max_predict_depth=1.0,
                 normalized_image_range=None, n_image_per_summary=4, image_dtype='float32', image_flags=None, tables=None, out=None):
    """One grid of log_summary, on the device.  image: a tensor or a list of N x 3 x H x W fp32 device tensors, one panel row each;
    output_depth / sparse_depth / validity_map / ground_truth: N x 1 x H x W; a depth row appears when its inputs are given (the sparse
    row: output_depth, sparse_depth and validity_map; the ground-truth row: output_depth and ground_truth), as in the reference.
    n_show = min(N, n_image_per_summary) samples are shown.  image_flags: per image the buffer `image_flag` returned (None: computed here,
    over the whole tensor); tables: {'viridis': t, 'inferno': t} device tables (default: colormap_table).  image_dtype 'float32' returns
    3 x GH x GW fp32, 'uint8' GH x GW x 3 uint8; `out` is a preallocated contiguous tensor of that shape and dtype.  Enqueues on the
    current stream; raises RuntimeError('ptta_summary_compose failed (-22)') for what include/ptta.h lists."""
    lib = _lib.load()
    images = [] if image is None else (list(image) if isinstance(image, (list, tuple)) else [image])
    maps = [('output_depth', output_depth), ('sparse_depth', sparse_depth), ('validity_map', validity_map), ('ground_truth', ground_truth)]
    for k, t in enumerate(images):
        _checked(t, 'image[%d]' % k, 3)
    for name, t in maps:
        if t is not None:
            _checked(t, name, 1)
    given = images + [t for _, t in maps if t is not None]
    if image_dtype not in ('float32', 'uint8'):
        raise ValueError("image_dtype is 'float32' or 'uint8'")
    rows = 0
    if output_depth is not None:
        rows |= _lib.PTTA_SUMMARY_ROW_OUTPUT
        if sparse_depth is not None and validity_map is not None:
            rows |= _lib.PTTA_SUMMARY_ROW_SPARSE
        if ground_truth is not None:
            rows |= _lib.PTTA_SUMMARY_ROW_GT
    n_rows = len(images) + bin(rows).count('1')
    if given:
        n, _, h, w = given[0].shape
        for t in given:
            if (t.shape[0], t.shape[2], t.shape[3]) != (n, h, w) or t.device != given[0].device:
                raise ValueError('the inputs must share N, H, W and the device')
        device = given[0].device
    else:
        n, h, w, device = 0, 0, 0, (out.device if out is not None else torch.device('cuda'))
    n_show = min(int(n), int(n_image_per_summary))
    if len(images) > _lib.PTTA_SUMMARY_MAX_IMAGES:
        raise ValueError('at most %d image rows' % _lib.PTTA_SUMMARY_MAX_IMAGES)
    a = _lib.SummaryArgs()
    a.n_show, a.height, a.width, a.n_images, a.rows = n_show, int(h), int(w), len(images), rows
    a.out_dtype = _lib.PTTA_SUMMARY_OUT_U8_HWC if image_dtype == 'uint8' else _lib.PTTA_SUMMARY_OUT_F32_CHW
    a.max_predict_depth = float(max_predict_depth)
    rev = reverse_normalization(normalized_image_range)
    a.normalize = int(rev is not None and bool(images))
    if a.normalize:
        a.rev_mean[:], a.rev_std[:] = rev[0], rev[1]          # (ctypes rounds the Python floats to fp32)
    keep = []
    handle = _stream_handle()
    for k, t in enumerate(images):
        f = image_flags[k] if image_flags is not None and image_flags[k] is not None else image_flag(t)
        keep.append(f)
        a.image[k], a.image_div255[k] = t.data_ptr(), f.data_ptr()
    for name, t in maps:
        setattr(a, name, None if t is None else t.data_ptr())
    if rows:
        tables = tables or {}
        vir = tables.get('viridis') if tables.get('viridis') is not None else colormap_table('viridis', device)
        keep.append(vir)
        a.viridis = vir.data_ptr()
        if rows & (_lib.PTTA_SUMMARY_ROW_SPARSE | _lib.PTTA_SUMMARY_ROW_GT):
            inf = tables.get('inferno') if tables.get('inferno') is not None else colormap_table('inferno', device)
            keep.append(inf)
            a.inferno = inf.data_ptr()
        for t in keep[len(images):]:
            if not (t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (256, 3) and t.is_contiguous()):
                raise ValueError('a colormap table is a contiguous 256 x 3 float64 device tensor')
    gh, gw = grid_shape(n_show, h, w, n_rows) if (n_show >= 1 and n_rows >= 1) else (0, 0)        # (no grid: the library refuses the call below)
    shape, dtype = ((gh, gw, 3), torch.uint8) if image_dtype == 'uint8' else ((3, gh, gw), torch.float32)
    if out is None:
        out = torch.empty(shape, device=device, dtype=dtype)
    elif not (out.is_cuda and out.is_contiguous() and out.dtype == dtype and (gh == 0 or tuple(out.shape) == shape)):
        raise ValueError('out must be a contiguous %s device tensor of shape %s' % (image_dtype, shape))
    a.out = out.data_ptr() if out.numel() else None
    rc = lib.ptta_summary_compose(ctypes.byref(a), handle)
    if rc != 0:
        raise RuntimeError('ptta_summary_compose failed (%d)' % rc)
    return out
