"""HBM -> host staging of the stored frames (the counterpart of proxytta/staging.py, in the other direction): the reference writes a
prediction with save_depth (src/data_utils.py:236-251) after `output_depth.cpu()`: a blocking copy of the fp32 map, 4 bytes per pixel, then
z * multiplier, the cast and the PNG encoder on the host thread that also feeds the step.  Here ptta_egress_raw (proxytta/egress.py)
makes the 16-bit frame on the card, ONE copy of 2 bytes per pixel (2 + 2 + 3 with the validity map and the image) takes it to a pinned slot
on a dedicated copy stream while the next step runs, and, with writer='png', one background thread waits for it and encodes the files.

    sink = RawFrameSink(n, 352, 1216, 375, 1242)          # planes=('depth',)
    depth, info = model.adapt(image, sparse, sink=sink)   # = sink.submit(depth=depth): enqueue only
    planes = sink.collect()                               # host waits for the OLDEST frame; numpy views of its pinned slot
    ...planes['depth_u16']...                             # n x 375 x 1242 uint16: what save_depth's file decodes to
    sink.release()                                        # the slot may be overwritten

PyTorch supplies the pinned memory, streams and events (plumbing); no arithmetic happens here, and there is no CPU fallback.
"""
import queue
import threading

import numpy as np
import torch

PLANES = ('depth', 'validity', 'image')                 # the order of a slot's sections: the 16-bit planes first, then the uint8 image
KEYS = {'depth': 'depth_u16', 'validity': 'validity_u16', 'image': 'image_u8'}


def _round16(v):
    return (v + 15) // 16 * 16


def _planes(planes):
    planes = (planes,) if isinstance(planes, str) else tuple(planes)
    if not planes or len(set(planes)) != len(planes) or any(p not in PLANES for p in planes):
        raise ValueError('planes must be a non-empty selection of %s, each once (got %r)' % (PLANES, planes))
    return tuple(p for p in PLANES if p in planes)


def raw_sink_layout(n, dst_height, dst_width, planes):
    """Byte offsets of the sections of one RawFrameSink slot, the counterpart of staging.raw_slot_layout: the 16-bit planes ('depth', then
    'validity': n x H x W x 2 bytes each) first, then the uint8 image ('image': n x H x W x 3), those of `planes` only.  Every section
    begins on a 16-byte boundary; 'bytes' is the whole slot, which is what one submit copies.  Pure arithmetic."""
    if n < 1 or dst_height < 1 or dst_width < 1:
        raise ValueError('n, dst_height and dst_width must be at least 1')
    px = n * dst_height * dst_width
    lay, end = {}, 0
    for key in _planes(planes):
        lay[key] = _round16(end)
        end = lay[key] + (3 if key == 'image' else 2) * px
    lay['bytes'] = _round16(end)
    return lay


class RawFrameSink:
    """`slots` slots, each ONE device byte buffer (raw_sink_layout) mirrored by one pinned byte buffer.

    submit() runs ptta_egress_raw on the CALLER's current stream -- the engine may overwrite its depth buffer in the next step, so the read
    is ordered in front of whatever the caller enqueues next -- records an event there, has the copy stream wait for it and issue ONE
    device-to-host copy of the slot, and records landed[k].  Nothing waits on the host.  When device slot k is reused the launch is
    ordered behind the earlier copy out of it by a stream wait on landed[k].

    Backpressure: a slot is unread from submit() to release().  Without a writer, submit() raises RuntimeError when all `slots` slots
    are unread (as FrameStager.submit does): collect() / release() one first.  With writer='png', submit() instead WAITS on the host until
    the thread has released the oldest slot; that is the only place the caller's thread blocks.

    collect() waits for the oldest slot's copy and returns numpy views of its pinned buffer, {'depth_u16': n x H x W uint16,
    'validity_u16': the same, 'image_u8': n x H x W x 3 uint8} for the planes the sink has; they are valid until release().

    writer='png': ONE background thread collects each frame, writes a PNG per sample and plane and releases the slot: a 16-bit plane as
    Image.fromarray(u16) (mode 'I;16', what the file save_depth writes decodes to), the image as RGB.  submit(paths=...) names the files:
    {plane: [n paths]}, or just [n paths] for a sink with one plane.  close() drains the queue and joins the thread; an exception in the
    thread is raised from the next submit(), collect() or close().  collect() / release() belong to the thread then."""

    def __init__(self, n, height, width, dst_height=None, dst_width=None, planes=('depth',), slots=3, multiplier=256.0, image_scale=255.0,
                 device=None, copy_stream=None, writer=None):
        dst_height, dst_width = height if dst_height is None else dst_height, width if dst_width is None else dst_width
        if n < 1 or height < 1 or width < 1:
            raise ValueError('n, height and width must be at least 1')
        if not (height <= dst_height and width <= dst_width):
            raise ValueError('the %d x %d window does not fit the %d x %d frame' % (height, width, dst_height, dst_width))
        if slots < 2:
            raise ValueError('slots must be at least 2')
        if writer not in (None, 'png'):
            raise ValueError("writer must be None or 'png'")
        for name, v in (('multiplier', multiplier), ('image_scale', image_scale)):
            if not (v > 0 and np.isfinite(v)):
                raise ValueError('%s must be a positive finite number' % name)
        self.planes = _planes(planes)
        self.layout = lay = raw_sink_layout(n, dst_height, dst_width, self.planes)
        if not torch.cuda.is_available():
            raise RuntimeError('RawFrameSink needs a HIP device (there is no CPU fallback)')
        from . import _lib
        self._lib = _lib.load()
        self.n, self.shape, self.dst_shape = n, (height, width), (n, dst_height, dst_width)
        self.multiplier, self.image_scale, self.slots = float(multiplier), float(image_scale), slots
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        px = n * dst_height * dst_width
        self.host = [torch.empty(lay['bytes'], dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self.host_np = []                                                # views of the pinned slots, section by section
        for hb in self.host:
            b, v = hb.numpy(), {}
            for key in self.planes:
                if key == 'image':
                    v[KEYS[key]] = b[lay[key]:lay[key] + 3 * px].reshape(n, dst_height, dst_width, 3)
                else:
                    v[KEYS[key]] = b[lay[key]:lay[key] + 2 * px].view(np.uint16).reshape(self.dst_shape)
            self.host_np.append(v)
        self.raw = [torch.empty(lay['bytes'], dtype=torch.uint8, device=self.device) for _ in range(slots)]
        self.copy_stream = torch.cuda.Stream(device=self.device) if copy_stream is None else copy_stream
        self.made = [torch.cuda.Event() for _ in range(slots)]           # the egress launch into the slot has finished
        self.landed = [torch.cuda.Event() for _ in range(slots)]         # the copy out of the slot has finished
        self.head = self.tail = 0                                        # submitted / released counters
        self.held = False
        self.bytes_per_frame = lay['bytes']                              # what one submit copies: the whole slot, padding included
        self._starts = (None, None, None)                                # the last uploaded (start, start_y, start_x)
        self._cond = threading.Condition()
        self._error = None
        self._thread = None
        if writer == 'png':
            from PIL import Image                                        # (an absent encoder is an error here, not in the thread)
            self._image = Image
            self._jobs = queue.Queue()
            self._thread = threading.Thread(target=self._write_loop, name='RawFrameSink-png', daemon=True)
            self._thread.start()

    def in_flight(self):
        return self.head - self.tail

    def _raise_thread_error(self):
        if self._error is not None:
            err, self._error = self._error, None
            raise RuntimeError('RawFrameSink: the writer thread failed') from err

    def _start_tensors(self, start):
        if start is None:
            return None, None
        if torch.is_tensor(start[0]) and torch.is_tensor(start[1]):
            return start
        key = tuple(tuple(np.broadcast_to(np.asarray(s, dtype=np.int64), (self.n,)).tolist()) for s in start)
        if self._starts[0] != key:                                       # (uploaded once per distinct value: a fixed window costs nothing per frame)
            sy, sx = (torch.tensor(k, dtype=torch.int32).to(self.device) for k in key)
            self._starts = (key, sy, sx)
        return self._starts[1], self._starts[2]

    def _paths(self, paths):
        if paths is None:
            raise ValueError("a sink with writer='png' needs paths: one per sample and plane")
        if not isinstance(paths, dict):
            if len(self.planes) != 1:
                raise ValueError('paths must be a dict {plane: [n paths]} for a sink with more than one plane')
            paths = {self.planes[0]: paths}
        if set(paths) != set(self.planes) or any(len(paths[p]) != self.n for p in self.planes):
            raise ValueError('paths must name %d file(s) for each of %s' % (self.n, self.planes))
        return {p: [str(f) for f in paths[p]] for p in self.planes}

    def submit(self, depth=None, validity=None, image=None, start=None, paths=None):
        """depth, validity: n x 1 x height x width; image: n x 3 x height x width; contiguous fp32 device tensors, exactly the planes the
        sink was built with.  start = (start_y, start_x): where the window lies in the stored frame, each one int, n ints or an int32
        device tensor of n entries (None = 0), clamped as ptta_ingest_raw clamps.  Enqueues the launch on the current stream and the copy
        on the copy stream; the tensors may be overwritten by anything enqueued on the current stream afterwards."""
        self._raise_thread_error()
        given = {'depth': depth, 'validity': validity, 'image': image}
        if tuple(p for p in PLANES if given[p] is not None) != self.planes:
            raise ValueError('submit takes exactly the planes the sink was built with: %s' % (self.planes,))
        for p in self.planes:
            t = given[p]
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError('RawFrameSink.submit takes device tensors (there is no CPU fallback)')
            if t.dtype != torch.float32 or tuple(t.shape) != (self.n, 3 if p == 'image' else 1) + self.shape or not t.is_contiguous():
                raise ValueError('%s must be a contiguous fp32 tensor of shape %s' % (p, (self.n, 3 if p == 'image' else 1) + self.shape))
        job = self._paths(paths) if self._thread is not None else None
        if self._thread is None and paths is not None:
            raise ValueError("paths goes with writer='png', and only with it")
        with self._cond:
            if self.in_flight() >= self.slots:
                if self._thread is None:
                    raise RuntimeError('all %d sink slots are unread: collect()/release() one first' % self.slots)
                while self.in_flight() >= self.slots and self._thread.is_alive():
                    self._cond.wait(0.05)
                self._raise_thread_error()
                if self.in_flight() >= self.slots:
                    raise RuntimeError('RawFrameSink: the writer thread has ended with every slot unread')
        sy, sx = self._start_tensors(start)
        for t in (sy, sx):
            if t is not None and (t.dtype != torch.int32 or not t.is_cuda or t.numel() != self.n):
                raise ValueError('start_y / start_x must be int32 device tensors of n entries')
        k = self.head % self.slots
        base, lay = self.raw[k].data_ptr(), self.layout
        cur = torch.cuda.current_stream(self.device)
        if self.head >= self.slots:
            cur.wait_event(self.landed[k])           # the earlier copy out of this device slot: a stream wait, not a host wait
        ins = [given[p].data_ptr() if p in self.planes else None for p in PLANES]
        outs = [base + lay[p] if p in self.planes else None for p in PLANES]
        rc = self._lib.ptta_egress_raw(*ins, *outs, self.n, self.shape[0], self.shape[1], self.dst_shape[1], self.dst_shape[2],
                                       None if sy is None else sy.data_ptr(), None if sx is None else sx.data_ptr(), self.multiplier,
                                       self.image_scale, cur.cuda_stream)
        if rc != 0:
            raise RuntimeError('ptta_egress_raw failed (%d): %s' % (rc, (self._lib.ptta_last_error(None) or b'').decode()))
        self.made[k].record(cur)
        self.copy_stream.wait_event(self.made[k])
        with torch.cuda.stream(self.copy_stream):
            self.host[k].copy_(self.raw[k], non_blocking=True)
            self.landed[k].record(self.copy_stream)
        with self._cond:
            self.head += 1
        if job is not None:
            self._jobs.put(job)

    def _collect(self):
        with self._cond:
            if self.held or self.tail >= self.head:
                raise RuntimeError('collect() without a submitted frame (or before release() of the previous one)')
            k = self.tail % self.slots
            self.held = True
        self.landed[k].synchronize()
        return self.host_np[k]

    def _release(self):
        with self._cond:
            if not self.held:
                raise RuntimeError('release() without collect()')
            self.tail += 1
            self.held = False
            self._cond.notify_all()

    def collect(self):
        """Numpy views of the oldest submitted frame's pinned slot, after its copy has landed (the host waits for that copy only)."""
        self._raise_thread_error()
        if self._thread is not None:
            raise RuntimeError("collect() belongs to the writer thread of a sink with writer='png'")
        return self._collect()

    def release(self):
        """The collected slot may be overwritten by a later submit."""
        if self._thread is not None:
            raise RuntimeError("release() belongs to the writer thread of a sink with writer='png'")
        self._release()

    def _write_loop(self):
        while True:
            job = self._jobs.get()
            if job is None:
                return
            try:
                views = self._collect()
                try:
                    if self._error is None:                              # (after a failure the queue is still drained, its slots released)
                        for p in self.planes:
                            for b, path in enumerate(job[p]):
                                # uint16 H x W -> mode 'I;16', uint8 H x W x 3 -> mode 'RGB'
                                self._image.fromarray(views[KEYS[p]][b]).save(path, format='PNG')
                finally:
                    self._release()
            except BaseException as e:          # noqa: B902 -- handed to the caller's thread, whatever it is
                if self._error is None:
                    self._error = e

    def close(self):
        """Drain the writer's queue and join its thread (a sink without a writer has nothing to close); raises what the thread raised."""
        if self._thread is not None and self._thread.is_alive():
            self._jobs.put(None)
            self._thread.join()
        self._raise_thread_error()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
