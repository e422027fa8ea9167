"""Scoring a run on the device (include/ptta.h ptta_score_accumulate, csrc/score.hip): the tail of the reference's drivers that turns a run
into the four numbers of results.txt.  The reference slices output and ground truth to the dataset's window, copies both maps to the host
every frame, masks them there, takes four means, and keeps `metric * batch_size` sums that it divides by n_sample at the end
(src/tta_main.py:755-809; validate() :975-1030 does the same through numpy with another mask).  Here the window is an argument, the sums
live in device memory, and nothing is read back until the result is asked for:

    score = RunScore(min_evaluate_depth, max_evaluate_depth, rule='adapt')
    for image, sparse_depth, ground_truth in frames:
        depth, info = model.adapt(image, sparse_depth, ground_truth=ground_truth, score=score)      # enqueue only
    print(score.result(n_sample=len(dataset)))                                                     # one 64-byte copy

Which loop uses which convention:
  * the reference's adaptation loop crops the INPUTS to the dataset's window before its eval forward (:706-723), so the scored maps are the
    cropped frame already: rule='adapt', window=None (the whole frame);
  * validate() runs the full frame and crops the OUTPUT (:988-999): rule='validate', window=eval_window(dataset_name, height, width), and
    `update` takes the full, uncropped maps -- no cropped copy is made.
The two rules differ on pixels equal to a bound: 'adapt' keeps them (gt > 0, not gt < min, not gt > max), 'validate' drops them (gt > 0,
gt > min, gt < max).  The bounds are compared in fp32, as the reference's fp32 maps compare against a Python number.
PyTorch supplies the tensors and the stream (plumbing); there is no CPU fallback.
"""
import torch

from . import _lib

RULES = {'adapt': _lib.PTTA_SCORE_RULE_ADAPT, 'validate': _lib.PTTA_SCORE_RULE_VALIDATE}
EVAL_CROPS = {'vkitti': (240, 1216), 'nuscenes': (544, 1600)}      # src/tta_main.py:975-986: crop_height, crop_width
METRICS = ('mae', 'rmse', 'imae', 'irmse')
COUNTERS = ('frames', 'batches', 'empty_batches', 'pixels')


def eval_window(dataset_name, height, width):
    """The reference's scoring window (y, x, h, w) inside a height x width frame (src/tta_main.py:988-999): for 'vkitti' (240 x 1216) and
    'nuscenes' (544 x 1600) the bottom rows, start_x = width // 2 - crop_width // 2, 2 (crop_width // 2) columns; any other name gives the
    whole frame.  ValueError for a frame smaller than the window (the reference's slice would silently come out short or empty)."""
    height, width = int(height), int(width)
    if height < 1 or width < 1:
        raise ValueError('eval_window: a frame is at least 1 x 1, got %d x %d' % (height, width))
    if dataset_name not in EVAL_CROPS:
        return (0, 0, height, width)
    ch, cw = EVAL_CROPS[dataset_name]
    if height < ch or width < 2 * (cw // 2) or width // 2 - cw // 2 < 0:
        raise ValueError('eval_window: a %d x %d frame is smaller than the %d x %d window of %r' % (height, width, ch, cw, dataset_name))
    return (height - ch, width // 2 - cw // 2, ch, 2 * (cw // 2))


def _refused(lib, what, rc):
    why = lib.ptta_last_error(None)
    raise RuntimeError('%s failed (%d): %s' % (what, rc, why.decode() if why else ''))


class RunScore(object):
    """The running score of one run.  max_n is the largest batch `update` will be given (it sizes the state: about 3 KB per sample).
    One RunScore is used from one stream at a time."""

    def __init__(self, min_evaluate_depth, max_evaluate_depth, rule='adapt', window=None, max_n=16):
        if rule not in RULES:
            raise ValueError("rule is 'adapt' or 'validate', got %r" % (rule,))
        if window is not None and len(window) != 4:
            raise ValueError('window is (y, x, height, width) or None')
        if not 1 <= int(max_n) <= _lib.PTTA_SCORE_MAX_N:
            raise ValueError('max_n is 1 .. %d' % _lib.PTTA_SCORE_MAX_N)
        self.min_evaluate_depth, self.max_evaluate_depth = float(min_evaluate_depth), float(max_evaluate_depth)
        self.rule, self.window, self.max_n = rule, None if window is None else tuple(int(v) for v in window), int(max_n)
        self._state = None
        self._last_n = 0

    def _stream(self):
        from .engine import _stream
        return _stream()

    def reset(self, device=None):
        """Start the run over (enqueue only).  The state is allocated on the first call, on `device` or the current CUDA device."""
        lib = _lib.load()
        if self._state is None:
            device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
            nbytes = lib.ptta_score_state_bytes(self.max_n)
            if nbytes < 0:
                _refused(lib, 'ptta_score_state_bytes', nbytes)
            self._state = torch.empty(nbytes, device=device, dtype=torch.uint8)
        with torch.cuda.device(self._state.device):
            rc = lib.ptta_score_reset(_lib.ptr(self._state), self._state.numel(), self._stream())
        if rc != 0:
            _refused(lib, 'ptta_score_reset', rc)
        self._last_n = 0

    def update(self, output_depth, ground_truth, want_samples=False):
        """Score one batch: the full, uncropped N x 1 x H x W (or N x H x W, or H x W) fp32 device maps.  Returns the batch's pooled MAE,
        RMSE (mm), iMAE, iRMSE (1/km) as a 4-element device tensor; with want_samples also the N x 4 per-sample tensor (NaN for a sample
        without a masked pixel) and the N int32 masked-pixel counts.  A contiguous input is not copied.  Enqueue only: no synchronisation."""
        lib = _lib.load()
        if output_depth.shape != ground_truth.shape:
            raise ValueError('output_depth %s and ground_truth %s differ in shape' % (tuple(output_depth.shape), tuple(ground_truth.shape)))
        if not (output_depth.is_cuda and ground_truth.is_cuda and output_depth.device == ground_truth.device):
            raise ValueError('RunScore.update takes two tensors of one CUDA device: there is no CPU fallback')
        if output_depth.dtype != torch.float32 or ground_truth.dtype != torch.float32:
            raise ValueError('RunScore.update takes float32 maps')
        shape = tuple(output_depth.shape)
        if len(shape) not in (2, 3, 4) or (len(shape) == 4 and shape[1] != 1):
            raise ValueError('a map is N x 1 x H x W, N x H x W or H x W, got %s' % (shape,))
        n, (h, w) = (1 if len(shape) == 2 else shape[0]), shape[-2:]
        if self._state is None:
            self.reset(output_depth.device)
        if self._state.device != output_depth.device:
            raise ValueError('this RunScore lives on %s, the maps on %s' % (self._state.device, output_depth.device))
        o, g = output_depth.detach().contiguous(), ground_truth.detach().contiguous()
        wy, wx, wh, ww = (0, 0, h, w) if self.window is None else self.window
        batch = torch.empty(4, device=o.device, dtype=torch.float32)
        samples = torch.empty((n, 4), device=o.device, dtype=torch.float32) if want_samples else None
        counts = torch.empty(n, device=o.device, dtype=torch.int32) if want_samples else None
        a = _lib.ScoreArgs(depth=_lib.ptr(o), ground_truth=_lib.ptr(g), n=n, height=h, width=w, win_y=wy, win_x=wx, win_height=wh, win_width=ww,
                           min_evaluate_depth=self.min_evaluate_depth, max_evaluate_depth=self.max_evaluate_depth, rule=RULES[self.rule],
                           state=_lib.ptr(self._state), batch_out=_lib.ptr(batch), sample_out=_lib.ptr(samples), sample_count_out=_lib.ptr(counts))
        with torch.cuda.device(o.device):
            rc = lib.ptta_score_accumulate(_lib.byref(a), self._stream())
        if rc != 0:
            _refused(lib, 'ptta_score_accumulate', rc)
        self._last_n = n
        return (batch, samples, counts) if want_samples else batch

    def result(self, n_sample=None):
        """The run so far, after one 64-byte copy: mae, rmse (mm), imae, irmse (1/km) = sum / n_sample (default: the frames scored,
        src/tta_main.py:806-809), and the counters frames, batches, empty_batches (batches without a masked pixel: each leaves NaN in the
        run, as the reference's mean of an empty tensor does), pixels."""
        lib = _lib.load()
        if self._state is None:
            self.reset()
        out = torch.empty(8, device=self._state.device, dtype=torch.float64)
        with torch.cuda.device(self._state.device):
            rc = lib.ptta_score_result(_lib.ptr(self._state), 0 if n_sample is None else int(n_sample), _lib.ptr(out), self._stream())
        if rc != 0:
            _refused(lib, 'ptta_score_result', rc)
        v = out.cpu().tolist()
        r = dict(zip(METRICS, v[:4]))
        r.update(zip(COUNTERS, (int(x) for x in v[4:])))
        return r

    def sums(self):
        """The run's four fp64 sums (metric x batch size, added over the batches) as a device tensor: a view of the state, for a caller
        that all-reduces them over ranks as src/tta_main.py:823-825 does before dividing by n_sample."""
        if self._state is None:
            self.reset()
        return self._state[:32].view(torch.float64)

    def last_sums(self):
        """(pooled, per_sample) fp64 device tensors of the latest update: count, sum |d|, sum d^2, sum |i|, sum i^2 (5, and N x 5):
        views of the state, overwritten by the next update."""
        if self._state is None or self._last_n == 0:
            raise RuntimeError('RunScore.last_sums: no update since the last reset')
        n = self._last_n
        return self._state[64:104].view(torch.float64), self._state[128:128 + 48 * n].view(torch.float64).view(n, 6)[:, :5]


__all__ = ['RunScore', 'eval_window', 'RULES', 'EVAL_CROPS']
