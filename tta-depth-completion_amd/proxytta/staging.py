"""Host -> HBM staging of the frame stream: the reference moves every batch with a blocking
`in_.to(device)` from pageable memory (src/tta_main.py:519-523), which serialises ~6.8 MB of PCIe traffic per KITTI frame
with the step.  Here frame k+1 is copied into a pinned slot and sent on a dedicated copy stream while the step of frame k
runs.  Slot reuse is ordered by the host waiting on events that are, in steady state, already complete (three slots: the
slot being refilled was consumed two steps ago), which is also the loop's backpressure: the host never runs more than
`slots` frames ahead of the GPU.

The pageable -> pinned copy is a single-threaded numpy copy ON PURPOSE: torch's `Tensor.copy_` fans a 5 MB copy out over
every core it sees (256 on the GPU box) and the spinning OpenMP team exhausts the container's CPU quota (cgroup cpu.max =
16 CPUs) within a few frames -- the process is then throttled for the rest of the 100 ms period, measured as an 80-100 ms
stall every ~5 frames (measured in round 2: 21.8 ms/frame with torch's copy, 2.35 ms/frame with one thread).

    stager.submit(image_k1, sparse_k1)        # host memcpy into pinned slot, async H2D on the copy stream
    image, sparse = stager.acquire()          # host waits for that slot's H2D (submitted a step ago: already there)
    engine.step(image, sparse)                # enqueue only
    stager.release()                          # the slot may be overwritten once the step has consumed it

PyTorch supplies the pinned memory, streams and events (plumbing); no arithmetic happens here.

FrameStager starts from fp32 frames, so its caller has already done the loader's cast, transpose, division and crop on the host and
16 bytes per pixel travel.  RawFrameStager starts from the decoded uint8 / 16-bit arrays: 5 bytes per pixel travel and
ptta_ingest_raw makes the fp32 frame on the device, behind the copy on the copy stream.
"""
import numpy as np
import torch


def _as_numpy(x):
    return x.detach().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


class FrameStager:
    def __init__(self, n, height, width, slots=3, device=None, copy_stream=None):
        if not torch.cuda.is_available():
            raise RuntimeError('FrameStager needs a HIP device (there is no CPU fallback)')
        assert slots >= 2
        self.shape_image, self.shape_sparse = (n, 3, height, width), (n, 1, height, width)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.slots = slots
        self.host = [(torch.empty(self.shape_image, dtype=torch.float32).pin_memory(),
                      torch.empty(self.shape_sparse, dtype=torch.float32).pin_memory()) for _ in range(slots)]
        self.host_np = [(a.numpy(), b.numpy()) for a, b in self.host]          # views of the pinned slots
        self.dev = [(torch.empty(self.shape_image, dtype=torch.float32, device=self.device),
                     torch.empty(self.shape_sparse, dtype=torch.float32, device=self.device)) for _ in range(slots)]
        self.copy_stream = torch.cuda.Stream(device=self.device) if copy_stream is None else copy_stream
        self.ready = [torch.cuda.Event() for _ in range(slots)]          # H2D into the slot has finished
        self.consumed = [torch.cuda.Event() for _ in range(slots)]       # the step that read the slot has finished
        self.head = self.tail = 0                                        # submitted / acquired counters
        self.held = False
        self.bytes_per_frame = 4 * (int(np.prod(self.shape_image)) + int(np.prod(self.shape_sparse)))

    def in_flight(self):
        return self.head - self.tail

    def submit(self, image, sparse):
        """image N x 3 x H x W, sparse N x 1 x H x W: numpy arrays or CPU tensors (any float/uint8 dtype; converted to
        float32 while copying into the pinned slot).  Returns immediately after enqueueing the H2D copy."""
        if self.in_flight() >= self.slots:
            raise RuntimeError('all %d staging slots are in flight: acquire()/release() one first' % self.slots)
        k = self.head % self.slots
        if self.head >= self.slots:
            self.consumed[k].synchronize()         # the step that read this slot (slots frames ago) has finished => so has its H2D
        hi, hs = self.host[k]
        np.copyto(self.host_np[k][0], _as_numpy(image).reshape(self.shape_image), casting='unsafe')
        np.copyto(self.host_np[k][1], _as_numpy(sparse).reshape(self.shape_sparse), casting='unsafe')
        with torch.cuda.stream(self.copy_stream):
            self.dev[k][0].copy_(hi, non_blocking=True)
            self.dev[k][1].copy_(hs, non_blocking=True)
            self.ready[k].record(self.copy_stream)
        self.head += 1

    def acquire(self):
        """Device tensors of the oldest submitted frame, after its copy has landed."""
        if self.held or self.tail >= self.head:
            raise RuntimeError('acquire() without a submitted frame (or before release() of the previous one)')
        k = self.tail % self.slots
        self.ready[k].synchronize()
        self.held = True
        return self.dev[k]

    def peek_next(self, stream=None):
        """Device tensors of the frame AFTER the acquired one (already submitted; None otherwise) for frame pipelining
        (Engine.step(..., next_frame=...)).  No host wait: `stream` (the engine's prefix_stream()) is made to wait for that slot's copy."""
        if not self.held or self.tail + 1 >= self.head:
            return None
        k = (self.tail + 1) % self.slots
        (torch.cuda.current_stream() if stream is None else stream).wait_event(self.ready[k])
        return self.dev[k]

    def release(self):
        """Mark the acquired slot reusable once everything enqueued so far on the current stream has run."""
        if not self.held:
            raise RuntimeError('release() without acquire()')
        self.consumed[self.tail % self.slots].record(torch.cuda.current_stream())
        self.tail += 1
        self.held = False


def _round16(v):
    return (v + 15) // 16 * 16


def raw_slot_layout(n, src_height, src_width, ground_truth=False):
    """Byte offsets of the sections of one RawFrameStager slot: the uint8 image (n x H x W x 3), the 16-bit planes (n x H x W each:
    'sparse', then 'gt' when ground_truth), then the 2n int32 crop starts ('start_y', 'start_x' behind it).  Every section begins on a
    16-byte boundary; 'bytes' is the whole slot, which is what one submit sends (RawFrameStager.bytes_per_frame).  Pure arithmetic."""
    if n < 1 or src_height < 1 or src_width < 1:
        raise ValueError('n, src_height and src_width must be at least 1')
    px = n * src_height * src_width
    lay = {'image': 0}
    end = 3 * px
    for key in ('sparse', 'gt') if ground_truth else ('sparse',):
        lay[key] = _round16(end)
        end = lay[key] + 2 * px
    lay['start_y'] = _round16(end)
    lay['start_x'] = lay['start_y'] + 4 * n
    lay['bytes'] = _round16(lay['start_x'] + 4 * n)
    return lay


class RawFrameStager(FrameStager):
    """FrameStager for frames AS DECODED: uint8 H x W x 3 images and 16-bit depth maps go into the pinned slot and across the link (5
    bytes per pixel, 7 with ground truth, instead of 16 / 28), and ptta_ingest_raw (proxytta/ingest.py) makes the fp32 frames on the device --
    the cast, the transpose, z / multiplier, the validity map and the loader's crop (src/data_utils.py:150-158, :182-188, :219-223,
    src/datasets.py:83-170) leave the one host thread.

    A slot is ONE pinned byte buffer (raw_slot_layout) mirrored by one device byte buffer: one H2D copy per frame set.  submit() does one
    single-threaded np.copyto per plane (the module docstring says why one thread), the copy and the ingest launch on the copy stream,
    then records `ready`: a loop written against FrameStager runs unchanged and acquires fp32 tensors, (image, sparse) or, with
    ground_truth=True, (image, sparse, validity, gt, gt_validity).  acquire / peek_next / release / in_flight are FrameStager's own."""

    def __init__(self, n, src_height, src_width, height=None, width=None, ground_truth=False, slots=3, multiplier=256.0, device=None,
                 copy_stream=None):
        # (FrameStager.__init__ would pin fp32 slots: this class fills in the same fields itself)
        if not torch.cuda.is_available():
            raise RuntimeError('RawFrameStager needs a HIP device (there is no CPU fallback)')
        assert slots >= 2
        from . import _lib
        self._lib = _lib.load()
        height, width = src_height if height is None else height, src_width if width is None else width
        if not (1 <= height <= src_height and 1 <= width <= src_width):
            raise ValueError('the %d x %d window does not fit the %d x %d source' % (height, width, src_height, src_width))
        self.n, self.src_shape, self.ground_truth, self.multiplier = n, (n, src_height, src_width), bool(ground_truth), float(multiplier)
        self.shape_image, self.shape_sparse = (n, 3, height, width), (n, 1, height, width)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.slots = slots
        self.layout = lay = raw_slot_layout(n, src_height, src_width, ground_truth)
        px = n * src_height * src_width
        self.host = [torch.empty(lay['bytes'], dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self.host_np = []                                                # views of the pinned slots, section by section
        for hb in self.host:
            b = hb.numpy()
            v = {'image': b[:3 * px].reshape(n, src_height, src_width, 3), 'start': b[lay['start_y']:lay['start_y'] + 8 * n].view(np.int32).reshape(2, n)}
            for key in ('sparse', 'gt') if ground_truth else ('sparse',):
                v[key] = b[lay[key]:lay[key] + 2 * px].view(np.uint16).reshape(self.src_shape)
            self.host_np.append(v)
        self.raw = [torch.empty(lay['bytes'], dtype=torch.uint8, device=self.device) for _ in range(slots)]
        planes = 5 if ground_truth else 2
        self.dev = [tuple(torch.empty(self.shape_image if i == 0 else self.shape_sparse, dtype=torch.float32, device=self.device)
                          for i in range(planes)) for _ in range(slots)]
        self.copy_stream = torch.cuda.Stream(device=self.device) if copy_stream is None else copy_stream
        self.ready = [torch.cuda.Event() for _ in range(slots)]          # H2D and ingest into the slot have finished
        self.consumed = [torch.cuda.Event() for _ in range(slots)]
        self.head = self.tail = 0
        self.held = False
        self.bytes_per_frame = lay['bytes']                              # what one submit sends: the whole slot, starts and padding included

    def submit(self, image_u8, sparse_u16, ground_truth_u16=None, start=None):
        """image_u8 N x H x W x 3 uint8; sparse_u16 (and ground_truth_u16 when built with ground_truth=True) N x H x W 16-bit integers --
        numpy arrays or CPU tensors; a wider integer array, as an older Pillow decodes a 16-bit PNG, is narrowed while copying, its values
        must fit 16 bits.  start = (start_y, start_x), each one int or N ints (None = 0): the window's corner per sample, clamped into the
        sample on the device.  Returns after enqueueing the copy and the ingest launch."""
        if self.in_flight() >= self.slots:
            raise RuntimeError('all %d staging slots are in flight: acquire()/release() one first' % self.slots)
        if (ground_truth_u16 is not None) != self.ground_truth:
            raise ValueError('ground_truth_u16 goes with RawFrameStager(ground_truth=True), and only with it')
        image_u8 = _as_numpy(image_u8)
        if image_u8.dtype != np.uint8:
            raise TypeError('image_u8 must be uint8 (the decoded image; FrameStager takes float frames)')
        k = self.head % self.slots
        if self.head >= self.slots:
            self.consumed[k].synchronize()         # the step that read this slot (slots frames ago) has finished => so have its H2D and ingest
        v, lay = self.host_np[k], self.layout
        np.copyto(v['image'], image_u8.reshape(v['image'].shape))
        for key, plane in (('sparse', sparse_u16), ('gt', ground_truth_u16)):
            if plane is not None:
                plane = _as_numpy(plane)
                if plane.dtype.kind not in 'ui':
                    raise TypeError('the 16-bit planes are integer arrays (the decoded depth PNG), not %s' % plane.dtype)
                np.copyto(v[key], plane.reshape(self.src_shape), casting='unsafe')
        v['start'][...] = 0 if start is None else np.stack([np.broadcast_to(np.asarray(s, dtype=np.int32), (self.n,)) for s in start])
        base = self.raw[k].data_ptr()
        out = [t.data_ptr() for t in self.dev[k]] + [None] * (5 - len(self.dev[k]))
        with torch.cuda.stream(self.copy_stream):
            self.raw[k].copy_(self.host[k], non_blocking=True)
            rc = self._lib.ptta_ingest_raw(base + lay['image'], base + lay['sparse'], base + lay['gt'] if self.ground_truth else None, *out,
                                           *self.src_shape, self.shape_image[2], self.shape_image[3], base + lay['start_y'],
                                           base + lay['start_x'], self.multiplier, self.copy_stream.cuda_stream)
            if rc != 0:
                raise RuntimeError('ptta_ingest_raw failed (%d)' % rc)
            self.ready[k].record(self.copy_stream)
        self.head += 1
