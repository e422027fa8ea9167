"""Thin Python owner of one libptta_hip handle: device memory, streams and tensors come from
PyTorch-ROCm, all arithmetic of the step runs inside the HIP library."""
import ctypes
from ctypes import byref, c_int, c_int64, c_void_p

import torch

from . import _lib
from ._lib import Hparams, check, ptr

ADAPTED = ('conv1_rgb_meta.weight', 'conv1_rgb_meta.bias')          # 1layer meta layer
_P2 = 'conv1_rgb_meta.conv1_meta.'
ADAPTED_2LAYERS = (_P2 + '0.0.weight', _P2 + '0.1.weight', _P2 + '0.1.bias', _P2 + '1.weight', _P2 + '1.bias',
                   _P2 + '2.weight', _P2 + '2.bias')


HEAD_PARAMS = tuple('%s.%s.%s' % (m, l, t) for m in ('proj', 'pred') for l in ('0', '1', '3') for t in ('weight', 'bias'))
HEAD_TARGETS = tuple('proj_t' + k[4:] for k in HEAD_PARAMS[:6])


def adapted_names(meta='1layer'):
    return ADAPTED_2LAYERS if meta == '2layers' else ADAPTED
_BOUND_SUFFIX = ('running_mean', 'running_var', 'num_batches_tracked')


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def image_norm_constants(normalized_image_range):
    """(divisor, mean[3], std[3]) of `normalized_image_range` as interpreted by
    Transforms.normalize_images (src/transforms.py:681-708)."""
    r = list(normalized_image_range)
    standard = any(isinstance(v, (tuple, list)) for v in r)
    if r == [0, 1]:
        return 255.0, [0.0] * 3, [1.0] * 3
    if standard:
        mean, std = list(r[0]), list(r[1])
        if len(mean) != 3 or len(std) != 3:
            raise ValueError('Unsupported normalization range: {}'.format(normalized_image_range))
        return 255.0, mean, std
    if r == [-1, 1]:
        return 255.0, [0.5] * 3, [0.5] * 3
    if r == [0, 255]:
        return 1.0, [0.0] * 3, [1.0] * 3
    raise ValueError('Unsupported normalization range: {}'.format(normalized_image_range))


class Engine:
    """One (batch, height, width, dtype) instance of the MSG_CHN ProxyTTA step on the current GPU."""

    def __init__(self, n, height, width, dtype='fp32', lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, w_sparse_depth=1.0, w_smoothness=1.0, w_cos=1.0,
                 max_input_depth=None, meta='1layer', backbone='msg_chn', legacy_offset=False, max_predict_depth=None,
                 syncbn_adapted=False, keep=(), options=None, adapt_mode='meta_bn'):
        if not torch.cuda.is_available():
            raise RuntimeError('proxytta needs a HIP device (torch.cuda.is_available() is False); '
                               'there is no CPU fallback')
        self.lib = _lib.load()
        self.n, self.h, self.w = int(n), int(height), int(width)
        self.dtype = dtype
        self.meta = meta
        self.backbone = backbone
        if adapt_mode not in ('meta_bn', 'meta', 'meta_fix'):
            raise ValueError("adapt_mode must be 'meta_bn', 'meta' or 'meta_fix' (src/nlspn_model_adapt.py:302-337)")
        # 'meta' / 'meta_fix' (NLSPN): the meta conv alone adapts, BatchNorm2d evaluates from its loaded running statistics (include/ptta.h PTTA_ADAPT_META_ONLY)
        self.adapt_mode = adapt_mode
        # meta 'none' (NLSPN): the network without the meta layer, one pass, no heads (include/ptta.h PTTA_META_NONE) -- with adapt_mode 'meta_bn'
        # the BatchNorm-adaptation baseline (86 adapted tensors), with 'meta' / 'meta_fix' the source model (nothing adapts, eval forward only)
        # meta 'plain' (CostDCNet): the same for that backbone (include/ptta.h PTTA_COSTDC_PLAIN): 30 adapted tensors / the source model
        # meta 'plain' (MSG_CHN): the source model alone (include/ptta.h PTTA_MSGCHN_PLAIN): nothing adapts, forward_eval and load_state_dict work,
        # every other call raises the library's reason
        if meta not in ('1layer', '2layers', 'none', 'plain'):
            raise ValueError("meta must be '1layer', '2layers', 'none' (NLSPN) or 'plain' (CostDCNet, MSG_CHN)")
        if meta == 'plain' and backbone not in ('costdcnet', 'msg_chn'):
            raise ValueError("meta 'plain' belongs to the CostDCNet and MSG_CHN backbones (NLSPN has 'none')")
        self.emb_dim = 1024 if backbone == 'nlspn' else 512
        if backbone == 'costdcnet' and not max_predict_depth:
            raise ValueError('CostDCNet needs max_predict_depth (the far plane of its cost volume, ExternalModel_Adapt(max_predict_depth))')
        self.adapted = adapted_names(meta)
        self.hp = Hparams(lr, betas[0], betas[1], eps, weight_decay, w_sparse_depth, w_smoothness,
                          w_cos, -1.0 if max_input_depth is None else float(max_input_depth), float(max_predict_depth or 0.0))
        self.handle = c_void_p()
        if dtype not in ('fp32', 'mixed'):
            raise ValueError("dtype must be 'fp32' (fp32 maps, bf16x3 products) or 'mixed' (fp32 / bf16x3 for the real frames' forward, narrow "
                             "bf16 maps and single-MFMA products for the no_grad proxy pass and the backward: include/ptta.h PTTA_DTYPE_MIXED)")
        code = {'fp32': _lib.PTTA_DTYPE_F32, 'mixed': _lib.PTTA_DTYPE_MIXED}[dtype]
        # precision budget only: classes of the mixed mode kept at fp32 / bf16x3 (include/ptta.h PTTA_MIXED_KEEP_*)
        for k in keep:
            code |= {'proxy': 0x100, 'backward': 0x200, 'heads': 0x400, 'bwd_rounded_w': 0x800}[k]
        rc = self.lib.ptta_create(byref(self.handle),
                                  {'nlspn': _lib.PTTA_BACKBONE_NLSPN, 'costdcnet': _lib.PTTA_BACKBONE_COSTDCNET}.get(backbone, _lib.PTTA_BACKBONE_MSG_CHN),
                                  {'2layers': _lib.PTTA_META_2LAYERS, 'none': _lib.PTTA_META_NONE}.get(meta, _lib.PTTA_META_1LAYER) |
                                  (_lib.PTTA_NLSPN_LEGACY_OFFSET if (legacy_offset and backbone == 'nlspn') else 0) |
                                  (_lib.PTTA_SYNCBN_ADAPT if (syncbn_adapted and backbone in ('nlspn', 'costdcnet')) else 0) |
                                  (_lib.PTTA_COSTDC_PLAIN if (meta == 'plain' and backbone == 'costdcnet') else 0) |
                                  (_lib.PTTA_MSGCHN_PLAIN if (meta == 'plain' and backbone == 'msg_chn') else 0) |
                                  (_lib.PTTA_ADAPT_META_ONLY if adapt_mode != 'meta_bn' else 0),
                                  self.n, self.h, self.w, code, byref(self.hp))
        if rc != 0:
            why = {-19: 'no HIP device', -12: 'out of device memory', -22: 'invalid size / argument',
                   -38: 'configuration not on the accelerated path (every backbone runs the 1layer and the 2layers meta layer; '
                        'CostDCNet in fp32 only; the 2layers block not with the SyncBN-adapted set of NLSPN / CostDCNet)'}.get(rc, 'see include/ptta.h')
            said = self.lib.ptta_last_error(None).decode()      # the reason of a refused configuration, where the library states one
            raise RuntimeError('ptta_create failed (%d): %s' % (rc, said if (rc == -38 and said != 'null handle') else why))
        for k, v in (options or {}).items():       # include/ptta.h ptta_set_option
            self.set_option(k, v)
        self.rows = int(self.lib.ptta_embedding_rows(self.handle))
        # adapted tensors in the reference's order, from the library (MSG_CHN 1layer: 2, 2layers: 7, NLSPN meta_bn: 88,
        # src/nlspn_model_adapt.py:322-337)
        names, self.adapted_numel, self.adapted_repeat = [], {}, {}
        for i in range(int(self.lib.ptta_adapted_count(self.handle))):
            n = c_int64(0)
            name = self.lib.ptta_adapted_name(self.handle, i, byref(n)).decode()
            names.append(name)
            self.adapted_numel[name] = int(n.value)
            # entries of the reference's parameter list behind this tensor (CostDCNet's DDP list names four tensors twice: include/ptta.h)
            self.adapted_repeat[name] = int(self.lib.ptta_adapted_repeat(self.handle, i))
        if backbone in ('nlspn', 'costdcnet') or meta == 'plain':
            self.adapted = names
        else:
            assert names == list(self.adapted), (names, self.adapted)
        self._keep = {}           # tensors whose storage the library borrows
        self.device = torch.device('cuda', torch.cuda.current_device())

    def close(self):
        if getattr(self, 'handle', None) and self.handle.value:
            torch.cuda.synchronize()
            self.lib.ptta_destroy(self.handle)
            self.handle = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        check(self.lib, self.handle, rc, what)

    # ---- weights ---------------------------------------------------------------------------
    def load_state_dict(self, state):
        """state: {reference state_dict key: cuda tensor}.  Adapted parameters are skipped (bind
        them with bind_adapted); BatchNorm buffers are bound by pointer and updated in place."""
        for k, t in state.items():
            if k in self.adapted:
                continue
            assert t.is_cuda and t.is_contiguous(), k
            if k.endswith(_BOUND_SUFFIX):
                self._keep[k] = t
            shape = (c_int64 * max(t.dim(), 1))(*([int(x) for x in t.shape] or [1]))
            self._chk(self.lib.ptta_load_weights(self.handle, k.encode(), ptr(t), shape, max(t.dim(), 1),
                                                 _stream()), 'ptta_load_weights(%s)' % k)

    def bind_adapted(self, name, param, exp_avg, exp_avg_sq):
        for t in (param, exp_avg, exp_avg_sq):
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32
        self._keep['adapt/' + name] = (param, exp_avg, exp_avg_sq)
        self._chk(self.lib.ptta_bind_adapted(self.handle, name.encode(), ptr(param), ptr(exp_avg),
                                             ptr(exp_avg_sq)), 'ptta_bind_adapted')

    def set_hparams(self, **kw):
        for k, v in kw.items():
            if k == 'betas':
                self.hp.beta1, self.hp.beta2 = v
            elif k == 'max_input_depth':
                self.hp.max_input_depth = -1.0 if v is None else float(v)
            else:
                setattr(self.hp, k, v)
        self._chk(self.lib.ptta_set_hparams(self.handle, byref(self.hp), _stream()), 'ptta_set_hparams')

    def set_adam_step(self, step):
        self._chk(self.lib.ptta_set_adam_step(self.handle, int(step), _stream()), 'ptta_set_adam_step')

    def adam_step_count(self):
        out = c_int(0)
        self._chk(self.lib.ptta_get_adam_step(self.handle, byref(out), _stream()), 'ptta_get_adam_step')
        return out.value

    # ---- the path ----------------------------------------------------------------------------
    def _f32(self, t, shape):
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == tuple(shape), (t.shape, shape)
        return t.contiguous()

    def forward_train(self, image, sparse, want_emb=True):
        image = self._f32(image, (self.n, 3, self.h, self.w))
        sparse = self._f32(sparse, (self.n, 1, self.h, self.w))
        depth = torch.empty((self.n, 1, self.h, self.w), device=image.device, dtype=torch.float32)
        emb = ref = None
        if want_emb and self.meta not in ('none', 'plain'):       # a handle without heads writes the depth only: (depth, None, None)
            emb = torch.empty((self.rows, self.emb_dim), device=image.device, dtype=torch.float32)
            ref = torch.empty_like(emb)
        self._chk(self.lib.ptta_forward_train(self.handle, ptr(image), ptr(sparse), ptr(depth), ptr(emb),
                                              ptr(ref), _stream()), 'ptta_forward_train')
        return depth, emb, ref

    def forward_eval(self, image, sparse):
        image = self._f32(image, (self.n, 3, self.h, self.w))
        sparse = self._f32(sparse, (self.n, 1, self.h, self.w))
        depth = torch.empty((self.n, 1, self.h, self.w), device=image.device, dtype=torch.float32)
        self._chk(self.lib.ptta_forward_eval(self.handle, ptr(image), ptr(sparse), ptr(depth), _stream()),
                  'ptta_forward_eval')
        return depth

    def loss_forward(self, loss_image, depth, sparse, validity, emb, ref, w_sd, w_sm, w_cos):
        info = torch.empty(4, device=depth.device, dtype=torch.float32)
        rows = 0 if emb is None else emb.shape[0]
        self._chk(self.lib.ptta_loss_forward(self.handle, ptr(loss_image.contiguous()), ptr(depth.contiguous()),
                                             ptr(sparse.contiguous()), ptr(validity.contiguous()),
                                             ptr(None if emb is None else emb.contiguous()),
                                             ptr(None if ref is None else ref.contiguous()), rows,
                                             float(w_sd), float(w_sm), float(w_cos), ptr(info), _stream()),
                  'ptta_loss_forward')
        return info

    def loss_backward(self, loss_image, depth, sparse, validity, emb, ref):
        """Gradients of the LAST loss_forward w.r.t. depth and ref (same inputs must be passed)."""
        gd = torch.empty_like(depth)
        gr = None if ref is None else torch.empty_like(ref)
        rows = 0 if emb is None else emb.shape[0]
        self._chk(self.lib.ptta_loss_backward(self.handle, ptr(loss_image.contiguous()), ptr(depth.contiguous()),
                                              ptr(sparse.contiguous()), ptr(validity.contiguous()),
                                              ptr(None if emb is None else emb.contiguous()),
                                              ptr(None if ref is None else ref.contiguous()), rows,
                                              ptr(gd), ptr(gr), _stream()), 'ptta_loss_backward')
        return gd, gr

    def grad(self, name, like):
        """Gradient of an adapted parameter after backward()/step(), shaped like `like`."""
        out = torch.empty_like(like)
        self._chk(self.lib.ptta_get_grad(self.handle, name.encode(), ptr(out), out.numel(), _stream()), 'ptta_get_grad')
        return out

    def set_grad(self, name, value):
        """Overwrite the stored gradient of an adapted parameter (reduced over ranks) before adam_step()."""
        value = value.contiguous()
        self._chk(self.lib.ptta_set_grad(self.handle, name.encode(), ptr(value), value.numel(), _stream()), 'ptta_set_grad')

    def backward_all(self, grad_depth, grad_ref, params):
        """loss.backward() for any meta layer: returns the gradients of `params` ({name: tensor})."""
        self._chk(self.lib.ptta_backward(self.handle, ptr(grad_depth.contiguous()),
                                         ptr(None if grad_ref is None else grad_ref.contiguous()), None, None, _stream()),
                  'ptta_backward')
        return [self.grad(k, params[k]) for k in self.adapted]

    def backward(self, grad_depth, grad_ref):
        gw = torch.empty((32, 32, 3, 3), device=grad_depth.device, dtype=torch.float32)
        gb = torch.empty((32,), device=grad_depth.device, dtype=torch.float32)
        self._chk(self.lib.ptta_backward(self.handle, ptr(grad_depth.contiguous()),
                                         ptr(None if grad_ref is None else grad_ref.contiguous()),
                                         ptr(gw), ptr(gb), _stream()), 'ptta_backward')
        return gw, gb

    def adam_step(self, gw=None, gb=None):
        self._chk(self.lib.ptta_adam_step(self.handle, ptr(gw), ptr(gb), _stream()), 'ptta_adam_step')

    @staticmethod
    def _frame_key(image, sparse):
        # what identifies a frame's CONTENT on the torch side: the storage and torch's in-place modification counters (a staging slot that is
        # refilled with `copy_` keeps its address and gets a new version)
        # (inference-mode tensors have no version counter and raise on the read: they get a key that never matches, i.e. a fresh token per
        # call -- correct, merely unpipelined; such callers pass explicit tokens)
        try:
            return (image.data_ptr(), image._version, sparse.data_ptr(), sparse._version)
        except RuntimeError:
            return object()

    def step(self, image, sparse, validity=None, loss_image=None, want_depth=False, next_frame=None, frame_token=None, next_token=None):
        """forward + loss + backward + Adam in one enqueue (src/tta_main.py:610-633).
        Returns (loss_info[4] device tensor, depth or None).
        next_frame = (image, sparse) of the frame the NEXT call will pass: the part of its forward upstream of the adapted layer then runs
        beside this step (ptta_step_pipelined, include/ptta.h); same results.  The library recognises the announced frame by a TOKEN, which
        this wrapper derives from the tensors (address + torch's in-place version counter: a refilled staging buffer is a new frame); a
        caller that writes device buffers behind torch's back passes explicit non-zero `frame_token` / `next_token` integers instead."""
        image = self._f32(image, (self.n, 3, self.h, self.w))
        sparse = self._f32(sparse, (self.n, 1, self.h, self.w))
        info = torch.empty(4, device=image.device, dtype=torch.float32)
        depth = torch.empty((self.n, 1, self.h, self.w), device=image.device, dtype=torch.float32) if want_depth else None
        if next_frame is not None:
            nimg = self._f32(next_frame[0], (self.n, 3, self.h, self.w))
            nsp = self._f32(next_frame[1], (self.n, 1, self.h, self.w))
            key, nkey = self._frame_key(image, sparse), self._frame_key(nimg, nsp)
            ann = getattr(self, '_announced', None)
            if frame_token is None:
                frame_token = ann[0] if (ann is not None and ann[1] == key) else self._new_token()
            if next_token is None:
                next_token = frame_token if nkey == key else self._new_token()
            self._announced = (next_token, nkey)
            self._keep['next_frame'] = (nimg, nsp, image, sparse)
            self._chk(self.lib.ptta_step_pipelined(self.handle, ptr(image), ptr(None if loss_image is None else loss_image.contiguous()),
                                                   ptr(sparse), ptr(None if validity is None else validity.contiguous()), int(frame_token),
                                                   ptr(nimg), ptr(nsp), int(next_token), ptr(depth), ptr(info), _stream()), 'ptta_step_pipelined')
            return info, depth
        self._announced = None
        self._chk(self.lib.ptta_step(self.handle, ptr(image), ptr(None if loss_image is None else loss_image.contiguous()),
                                     ptr(sparse), ptr(None if validity is None else validity.contiguous()),
                                     ptr(depth), ptr(info), _stream()), 'ptta_step')
        return info, depth

    def _new_token(self):
        self._token = getattr(self, '_token', 0) + 1
        return self._token

    def forward_eval_last(self):
        """The scored eval forward of the frame the last step(..., next_frame=...) call adapted, reusing that frame's parameter-independent
        prefix (ptta_forward_eval_last)."""
        depth = torch.empty((self.n, 1, self.h, self.w), device=self.device, dtype=torch.float32)
        self._chk(self.lib.ptta_forward_eval_last(self.handle, ptr(depth), _stream()), 'ptta_forward_eval_last')
        return depth

    def prefix_stream(self):
        """torch view of the stream the next frame's prefix runs on (ptta_pipeline_stream): order an asynchronous producer of that frame
        (FrameStager's H2D copy) on it with `.wait_event(...)` before the step call that announces the frame."""
        if getattr(self, '_prefix_stream', None) is None:
            sp = c_void_p()
            self._chk(self.lib.ptta_pipeline_stream(self.handle, byref(sp)), 'ptta_pipeline_stream')
            self._prefix_stream = torch.cuda.ExternalStream(sp.value, device=self.device)
        return self._prefix_stream

    def set_image_norm(self, normalized_image_range):
        """Fuse Transforms.normalize_images (src/transforms.py:668-710) into the first convolution: the
        engine then takes RAW images.  Accepts the reference's `normalized_image_range` values: [0, 1],
        [-1, 1], [0, 255], or [mean, std] with 3-element lists; anything else raises ValueError like the
        reference does."""
        div, mean, std = image_norm_constants(normalized_image_range)
        m = (ctypes.c_float * 3)(*mean)
        s = (ctypes.c_float * 3)(*std)
        self._chk(self.lib.ptta_set_image_norm(self.handle, float(div), m, s), 'ptta_set_image_norm')

    def enable_stat_sync(self, group=None):
        """model.convert_syncbn() for the one-process-per-GPU run (src/tta_main.py:326): train-mode BatchNorm statistics of
        the GLOBAL batch.  The library hands a float64 buffer of partial sums to this callback, which sums it over the ranks
        with torch.distributed (RCCL on ROCm; gloo works too) on the current stream."""
        import torch.distributed as dist
        world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
        if world <= 1:
            self._chk(self.lib.ptta_set_stat_sync(self.handle, None, None, None, 0, 1), 'ptta_set_stat_sync')
            return
        self._stat_sync_how = ('callback', group)
        buf = torch.zeros(self._exchange_numel(), device=self.device, dtype=torch.float64)

        def _allreduce(user, ptr_, count, stream):
            try:
                # the collective must be ordered on the stream the library is enqueuing on (it may be an internal one)
                ext = torch.cuda.ExternalStream(stream) if stream else torch.cuda.current_stream()
                with torch.cuda.stream(ext):
                    dist.all_reduce(buf[:count], op=dist.ReduceOp.SUM, group=group)
                return 0
            except Exception:                       # never raise through the C frame
                import traceback
                traceback.print_exc()
                return -5
        cb = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, ctypes.c_longlong, c_void_p)(_allreduce)
        self._keep['stat_sync'] = (buf, cb)
        self._chk(self.lib.ptta_set_stat_sync(self.handle, ctypes.cast(cb, c_void_p), None, c_void_p(buf.data_ptr()), buf.numel(), world),
                  'ptta_set_stat_sync')

    def enable_rccl_sync(self, comm=None, world=None, stats=True, grads=True):
        """The reference's DDP + SyncBatchNorm run (src/tta_main.py:326-354) on the library's own RCCL communicator: the
        BatchNorm statistics exchange (`stats`) and the mean all-reduce of the adapted gradients between backward and Adam of the
        fused step (`grads`) are enqueued by the library on the step's stream -- no Python frame per collective, and the MSG_CHN
        step keeps replaying its hipGraph.  `comm`: a handle from proxytta.distributed.rccl_communicator() (default: the
        process-wide one).  None/None with no process group = a one-rank communicator (plumbing test)."""
        from . import distributed as D
        if comm is None:
            comm, world = D.rccl_communicator()
        self._keep['rccl'] = comm
        if stats:
            self._stat_sync_how = ('rccl', comm, world)
            buf = torch.zeros(self._exchange_numel(), device=self.device, dtype=torch.float64)
            self._keep['stat_sync'] = (buf, None)
            self._chk(self.lib.ptta_set_stat_sync_rccl(self.handle, c_void_p(comm), c_void_p(buf.data_ptr()), buf.numel(), int(world)), 'ptta_set_stat_sync_rccl')
        if grads:
            self._chk(self.lib.ptta_set_grad_sync_rccl(self.handle, c_void_p(comm)), 'ptta_set_grad_sync_rccl')
        self._rccl_grads = bool(grads)

    def disable_rccl_sync(self):
        self._chk(self.lib.ptta_set_stat_sync_rccl(self.handle, None, None, 0, 1), 'ptta_set_stat_sync_rccl')
        self._chk(self.lib.ptta_set_grad_sync_rccl(self.handle, None), 'ptta_set_grad_sync_rccl')
        self._rccl_grads = False
        self._keep.pop('stat_sync', None)

    def _exchange_numel(self):
        """Length of the statistics exchange buffer: the SyncBatchNorm form of the head trainer averages its twelve gradients through the
        same exchange when no gradient communicator is set, so it gets room for them in ONE message."""
        n = 4 * 2 * 1024
        if getattr(self, '_head_form', 0) == _lib.PTTA_HEAD_FORM_SYNCBN:
            n = max(n, sum(ts[0].numel() for k, ts in self._keep.items() if k.startswith('head/') and len(ts) == 3))
        return n

    def _fit_head_exchange(self):
        """An exchange enabled before the heads were bound (or before the form was chosen) is grown to hold their gradients."""
        kept = self._keep.get('stat_sync')
        if kept is None or kept[0].numel() >= self._exchange_numel():
            return
        how = self._stat_sync_how
        if how[0] == 'callback':
            self.enable_stat_sync(how[1])
        else:
            buf = torch.zeros(self._exchange_numel(), device=self.device, dtype=torch.float64)
            self._keep['stat_sync'] = (buf, None)
            self._chk(self.lib.ptta_set_stat_sync_rccl(self.handle, c_void_p(how[1]), c_void_p(buf.data_ptr()), buf.numel(), int(how[2])),
                      'ptta_set_stat_sync_rccl')

    # ---- stage-2 head trainer (include/ptta.h "Stage-2 head trainer"; src/head_main.py:464-480) ------------
    def set_head_form(self, form):
        """PTTA_HEAD_FORM_PLAIN (0) or PTTA_HEAD_FORM_SYNCBN (1, src/head_main.py:278-279 convert_syncbn() + DDP): before the first
        head step.  An enabled statistics exchange grows to hold the head gradients in one message, whatever the order of the calls."""
        self._chk(self.lib.ptta_head_set_form(self.handle, int(form)), 'ptta_head_set_form')
        self._head_form = int(form)
        self._fit_head_exchange()

    def bind_head(self, name, param, exp_avg=None, exp_avg_sq=None):
        ts = [t for t in (param, exp_avg, exp_avg_sq) if t is not None]
        for t in ts:
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32
        self._keep['head/' + name] = ts
        self._chk(self.lib.ptta_head_bind(self.handle, name.encode(), ptr(param), ptr(exp_avg), ptr(exp_avg_sq)), 'ptta_head_bind')
        self._fit_head_exchange()

    def set_head_hparams(self, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, tau=0.999, adam_step=-1):
        self._chk(self.lib.ptta_head_set_hparams(self.handle, lr, betas[0], betas[1], eps, weight_decay, tau, int(adam_step), _stream()),
                  'ptta_head_set_hparams')

    def head_reload(self):
        self._chk(self.lib.ptta_head_reload(self.handle, _stream()), 'ptta_head_reload')

    def head_forward(self, image, sparse, reverse=True, want=True):
        image = self._f32(image, (self.n, 3, self.h, self.w))
        sparse = self._f32(sparse, (self.n, 1, self.h, self.w))
        emb = ref = None
        if want:
            emb = torch.empty((self.rows, self.emb_dim), device=image.device, dtype=torch.float32)
            ref = torch.empty_like(emb)
        self._chk(self.lib.ptta_head_forward(self.handle, ptr(image), ptr(sparse), int(bool(reverse)), ptr(emb), ptr(ref), _stream()),
                  'ptta_head_forward')
        return emb, ref

    def head_backward(self):
        loss = torch.empty(1, device=self.device, dtype=torch.float32)
        self._chk(self.lib.ptta_head_backward(self.handle, ptr(loss), _stream()), 'ptta_head_backward')
        return loss

    def head_adam_step(self):
        self._chk(self.lib.ptta_head_adam_step(self.handle, _stream()), 'ptta_head_adam_step')

    def head_step(self, image, sparse, reverse=True):
        image = self._f32(image, (self.n, 3, self.h, self.w))
        sparse = self._f32(sparse, (self.n, 1, self.h, self.w))
        loss = torch.empty(1, device=image.device, dtype=torch.float32)
        self._chk(self.lib.ptta_head_step(self.handle, ptr(image), ptr(sparse), int(bool(reverse)), ptr(loss), _stream()), 'ptta_head_step')
        return loss

    def head_grad(self, name, like):
        """Gradient of a head parameter after head_backward(), or None when it is outside the graph (reverse: all of proj)."""
        has = c_int(0)
        out = torch.empty_like(like)
        self._chk(self.lib.ptta_head_get_grad(self.handle, name.encode(), ptr(out), out.numel(), byref(has), _stream()), 'ptta_head_get_grad')
        return out if has.value else None

    def set_graph(self, enable):
        self._chk(self.lib.ptta_set_graph(self.handle, int(bool(enable))), 'ptta_set_graph')

    def set_option(self, key, value):
        """Per-handle switch (include/ptta.h ptta_set_option: graph, aux_stream, thru, fuse_first, fuse_head_bwd, fuse_heads, heads_v2,
        cos_in_gemm, mask_bits, stamps, pair_fuse, tpair_fuse; eval_bn_fused, head_bn_fused on the generic engine's handles, deterministic on
        NLSPN's)."""
        self._chk(self.lib.ptta_set_option(self.handle, key.encode(), int(value)), 'ptta_set_option(%s)' % key)

    def get_option(self, key):
        v = ctypes.c_int(0)
        self._chk(self.lib.ptta_get_option(self.handle, key.encode(), byref(v)), 'ptta_get_option(%s)' % key)
        return v.value

    def profile(self, enable):
        self._chk(self.lib.ptta_profile(self.handle, int(bool(enable))), 'ptta_profile')

    def profile_read(self, klass):
        """(ms_total, algorithmic_bytes, macs, launches) of conv32 kernel class `klass` since profile(True)."""
        ms, by, mc, n = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0), c_int64(0)
        self._chk(self.lib.ptta_profile_read(self.handle, int(klass), byref(ms), byref(by), byref(mc), byref(n), _stream()),
                  'ptta_profile_read')
        return ms.value, by.value, mc.value, n.value

    def debug_tensor(self, name):
        n = c_int64(0)
        self._chk(self.lib.ptta_debug_tensor(self.handle, name.encode(), None, 0, byref(n), _stream()), 'ptta_debug_tensor')
        out = torch.empty(n.value, device=self.device, dtype=torch.float32)
        self._chk(self.lib.ptta_debug_tensor(self.handle, name.encode(), ptr(out), n.value, byref(n), _stream()),
                  'ptta_debug_tensor')
        return out


def op_conv32(x_nhwc, weight, bias, mode, relu_in=False, in_major=False, flip=False, dtype='fp32', naive=False, x3=False):
    """Test hook: run the hot-path 32->32 3x3 kernel on an fp32 NHWC tensor."""
    lib = _lib.load()
    b, h, w, _ = x_nhwc.shape
    ho, wo = {0: (h, w), 1: (h // 2, w // 2), 2: (2 * h, 2 * w)}[mode]
    out = torch.empty((b, ho, wo, 32), device=x_nhwc.device, dtype=torch.float32)
    rc = lib.ptta_op_conv32(ptr(x_nhwc.contiguous()), ptr(weight.contiguous()), ptr(bias), ptr(out), b, h, w, mode,
                            int(relu_in), int(in_major), int(flip), 0 if dtype == 'fp32' else 1, int(bool(naive)) | (2 if x3 else 0), _stream())
    if rc != 0:
        raise RuntimeError('ptta_op_conv32 failed (%d)' % rc)
    return out


def _pv(t):
    """Device pointer value of a tensor for a ctypes struct field (None -> NULL); the tensor must be contiguous."""
    if t is None:
        return None
    assert t.is_contiguous() and t.is_cuda
    return t.data_ptr()


def op_conv_in(planes, weight, b, h, w, bias=None, cin_total=None, cin_first=0, transpose_flip=False, up=None, mask=None, mask_bits=None,
               add1=None, out_raw=None, out_sum=None, a_bits=None, a_bits_nb=0, zero_from_b=1 << 30, dtype='fp32', naive=False, max_blocks=0):
    """Test hook (include/ptta.h ptta_op_conv_in): the 1..3 -> 32 first-layer convolution.  planes: a list of (tensor [nb, h, w], norm) with
    norm None or (div, mean, std); up / mask / add1 fp32 NHWC tensors whose first dimension is their frame count; mask_bits int32 [nb, h, w];
    out_raw / out_sum / a_bits are written in place.  Returns the name of the kernel form that ran (_lib.CONV_IN_FORMS)."""
    lib = _lib.load()
    a = _lib.ConvInArgs()
    a.cin, a.cin_total, a.cin_first, a.transpose_flip = len(planes), (cin_total if cin_total is not None else len(planes)), cin_first, int(transpose_flip)
    a.up_nb = up.shape[0] if up is not None else 1
    a.mask_nb = (mask if mask is not None else mask_bits).shape[0] if (mask is not None or mask_bits is not None) else 1
    a.add1_nb = add1.shape[0] if add1 is not None else 1
    a.a_bits_nb, a.zero_from_b, a.b, a.h, a.w = a_bits_nb, zero_from_b, b, h, w
    a.dtype, a.naive, a.max_blocks = (0 if dtype == 'fp32' else 1), int(naive), max_blocks
    for k, (t, norm) in enumerate(planes):
        a.pl[k].p, a.pl[k].nb, a.pl[k].norm = _pv(t), t.shape[0], int(norm is not None)
        a.pl[k].div, a.pl[k].mean, a.pl[k].stdv = norm if norm is not None else (1.0, 0.0, 1.0)
    a.weight, a.bias, a.up, a.mask, a.mask_bits, a.add1 = _pv(weight), _pv(bias), _pv(up), _pv(mask), _pv(mask_bits), _pv(add1)
    a.out_raw, a.out_sum, a.a_bits = _pv(out_raw), _pv(out_sum), _pv(a_bits)
    form = c_int(-1)
    rc = lib.ptta_op_conv_in(byref(a), byref(form), _stream())
    if rc != 0:
        raise RuntimeError('ptta_op_conv_in failed (%d)' % rc)
    return _lib.CONV_IN_FORMS[form.value]


def op_conv_out1(x_nhwc, weight, out, bias=None, add=None, relu_in=False, src_cin_total=0, src_cin_index=0, from_conv_in=False, dtype='fp32',
                 max_blocks=0):
    """Test hook (include/ptta.h ptta_op_conv_out1): the 32 -> 1 prediction convolution; out [b, h, w] is written in place, x_nhwc holds
    in_nb <= b frames, add [add_nb, h, w]."""
    lib = _lib.load()
    a = _lib.ConvOut1Args()
    a.in_nb, a.src_cin_total, a.src_cin_index, a.from_conv_in = x_nhwc.shape[0], src_cin_total, src_cin_index, int(from_conv_in)
    a.add_nb, a.relu_in, a.dtype = (add.shape[0] if add is not None else 1), int(relu_in), (0 if dtype == 'fp32' else 1)
    a.b, a.h, a.w, a.max_blocks = out.shape[0], out.shape[1], out.shape[2], max_blocks
    setattr(a, 'in', _pv(x_nhwc))
    a.weight, a.bias, a.add, a.out = _pv(weight), _pv(bias), _pv(add), _pv(out)
    rc = lib.ptta_op_conv_out1(byref(a), _stream())
    if rc != 0:
        raise RuntimeError('ptta_op_conv_out1 failed (%d)' % rc)
    return out


def op_prep(sparse, max_input_depth, dclamp, d12, d14):
    """Test hook (include/ptta.h ptta_op_prep): clamp + the 1/2 and 1/4 sparse-aware pooled maps of sparse [n, h, w], written in place."""
    n, h, w = sparse.shape
    rc = _lib.load().ptta_op_prep(ptr(sparse), float(max_input_depth), ptr(dclamp), ptr(d12), ptr(d14), n, h, w, _stream())
    if rc != 0:
        raise RuntimeError('ptta_op_prep failed (%d)' % rc)


def op_up2(x, out, transposed=False, add=None, dtype='fp32'):
    """Test hooks (include/ptta.h ptta_op_up2_1ch / ptta_op_up2t_1ch / ptta_op_up2t_32): bilinear x2 of a planar map [b, hin, win] ->
    out [b, 2 hin, 2 win], or its transpose x [b, 2 hin, 2 win(, 32)] -> out [b, hin, win(, 32)] (+ add, narrow storage: 32 channels only)."""
    lib = _lib.load()
    b, hin, win = (out if transposed else x).shape[:3]
    if x.dim() == 4:
        rc = lib.ptta_op_up2t_32(ptr(x), ptr(add), ptr(out), b, hin, win, 0 if dtype == 'fp32' else 1, _stream())
    elif transposed:
        rc = lib.ptta_op_up2t_1ch(ptr(x), ptr(out), b, hin, win, _stream())
    else:
        rc = lib.ptta_op_up2_1ch(ptr(x), ptr(out), b, hin, win, _stream())
    if rc != 0:
        raise RuntimeError('ptta_op_up2 failed (%d)' % rc)
    return out


def op_loss(fwd, bwd, depth, image, sparse, w3, max_input_depth, validity=None, emb=None, ref=None, loss_info=None, rowstats=None, gdepth=None,
            gref=None, coef=None, shape=None, r=None, d=None):
    """Test hook (include/ptta.h ptta_op_loss): fwd / bwd keys of _lib.LOSS_FWD / _lib.LOSS_BWD; outputs are written in place.  shape / r / d
    override what the tensors say (refusal tests)."""
    lib = _lib.load()
    a = _lib.LossArgs()
    a.fwd, a.bwd = _lib.LOSS_FWD[fwd], _lib.LOSS_BWD[bwd]
    a.n, a.h, a.w = shape if shape is not None else depth.shape
    a.r = r if r is not None else (emb.shape[0] if emb is not None else 0)
    a.d = d if d is not None else (emb.shape[1] if emb is not None else 0)
    a.max_input_depth, (a.w_sd, a.w_sm, a.w_cos) = float(max_input_depth), w3
    for name, t in (('depth', depth), ('image', image), ('sparse', sparse), ('validity', validity), ('emb', emb), ('ref', ref), ('loss_info', loss_info),
                    ('rowstats', rowstats), ('gdepth', gdepth), ('gref', gref), ('coef', coef)):
        setattr(a, name, _pv(t))
    rc = lib.ptta_op_loss(byref(a), _stream())
    if rc != 0:
        raise RuntimeError('ptta_op_loss failed (%d)' % rc)


GWGRAD_IMPLS = {'default': 0, 'fp32_mfma': 1, 'naive': 2}


def op_gwgrad(x_nhwc, gy_nhwc, impl='default', with_bias=True, reps=0):
    """Test / measurement hook: weight (and bias) gradient of a stride-1 3x3 convolution from fp32 NHWC device maps
    x [b, h, w, ci] and gy [b, h, w, co] (include/ptta.h ptta_op_gwgrad).  impl: 'default' (the engine's launcher: bf16x3 wherever a
    form exists), 'fp32_mfma' or 'naive'.  Returns (gw [co, ci, 3, 3], gb [co] or None, microseconds per call of `reps` timed calls)."""
    lib = _lib.load()
    b, h, w, ci = x_nhwc.shape
    co = gy_nhwc.shape[3]
    assert tuple(gy_nhwc.shape[:3]) == (b, h, w)
    x_nhwc, gy_nhwc = x_nhwc.float().contiguous(), gy_nhwc.float().contiguous()
    gw = torch.empty((co, ci, 3, 3), device=x_nhwc.device, dtype=torch.float32)
    gb = torch.empty((co,), device=x_nhwc.device, dtype=torch.float32) if with_bias else None
    us = ctypes.c_float(0.0)
    rc = lib.ptta_op_gwgrad(ptr(x_nhwc), ptr(gy_nhwc), ptr(gw), ptr(gb), b, h, w, ci, co,
                            GWGRAD_IMPLS[impl], int(reps), byref(us), _stream())
    if rc != 0:
        raise RuntimeError('ptta_op_gwgrad failed (%d)' % rc)
    return gw, gb, (us.value if reps > 0 else None)


def _update_rc(rc, what):
    if rc != 0:
        raise RuntimeError('%s failed (%d)' % (what, rc))


def op_wgrad32(x, gy, b, h, w, gw, gb=None, co_stride=288, bf16=False):
    """Test hook (include/ptta.h ptta_op_wgrad32; csrc/wgrad_adam.hip): the 32 -> 32 weight gradient of NHWC maps [b, h, w, 32] (fp32, or
    int16 bf16 bit patterns with bf16) into gw (element (co, ci, tap) at co * co_stride + ci * 9 + tap behind gw's first element) and gb
    [32] or None, in place."""
    _update_rc(_lib.load().ptta_op_wgrad32(ptr(x), ptr(gy), int(bool(bf16)), int(b), int(h), int(w), ptr(gw), ptr(gb), int(co_stride), _stream()),
               'ptta_op_wgrad32')


def op_gwgrad_view(x, gy, b, h, w, ci, co, gw, gb=None, ldx=None, ldg=None, gy_bf16=False, adam=None):
    """Test hook (include/ptta.h ptta_op_gwgrad_view; csrc/gwgrad_mfma.hip): the engine's weight-gradient launcher on strided views.  x, gy:
    tensors whose first element is the view's first channel of pixel 0, pixel strides ldx / ldg elements (default: dense); gy fp32 or int16
    bf16 bit patterns with gy_bf16.  adam: dict(pw, mw, vw, pb, mb, vb, hyper, step, ticket) for the Adam inside the reduction (pb, mb, vb
    may be None)."""
    a = _lib.GwgradViewArgs()
    a.b, a.h, a.w, a.ci, a.co = int(b), int(h), int(w), int(ci), int(co)
    a.ldx, a.ldg, a.gy_bf16 = int(ci if ldx is None else ldx), int(co if ldg is None else ldg), int(bool(gy_bf16))
    for name, t in dict(adam or {}, x=x, gy=gy, gw=gw, gb=gb).items():
        setattr(a, name, _pv(t))
    _update_rc(_lib.load().ptta_op_gwgrad_view(byref(a), _stream()), 'ptta_op_gwgrad_view')


def op_adam(p, m, v, g, hyper, step):
    """Test hook (include/ptta.h ptta_op_adam; adam_kernel): step += 1, then one Adam update of p, m, v with g, in place.  hyper: five device
    floats (lr, beta1, beta2, eps, weight_decay); step: one device int32."""
    _update_rc(_lib.load().ptta_op_adam(ptr(p), ptr(m), ptr(v), ptr(g), p.numel(), ptr(hyper), ptr(step), _stream()), 'ptta_op_adam')


def _host_table(entries, width):
    cols = [(ctypes.c_void_p * len(entries))(*[None if e[j] is None else e[j].data_ptr() for e in entries]) for j in range(width)]
    for e in entries:
        assert all(t is None or (t.is_contiguous() and t.is_cuda) for t in e[:width])
    return cols, (ctypes.c_longlong * len(entries))(*[e[0].numel() for e in entries])


def op_adam_multi(entries, hyper, step, ticket):
    """Test hook (include/ptta.h ptta_op_adam_multi; adam_multi_kernel): entries = [(p, m, v, g, rep)], every tensor updated in ONE launch;
    step (device int32) goes up by one, ticket (device int32, 0) comes back 0."""
    (p, m, v, g), n = _host_table(entries, 4)
    rep = (c_int * len(entries))(*[int(e[4]) for e in entries])
    _update_rc(_lib.load().ptta_op_adam_multi(len(entries), p, m, v, g, n, rep, ptr(hyper), ptr(step), ptr(ticket), _stream()), 'ptta_op_adam_multi')


def op_ema_multi(entries, tau_dev):
    """Test hook (include/ptta.h ptta_op_ema_multi; ema_multi_kernel): entries = [(target, online)], target = target tau + online (1 - tau)
    in place, tau_dev = two device floats (tau, 1 - tau)."""
    (p, g), n = _host_table(entries, 2)
    _update_rc(_lib.load().ptta_op_ema_multi(len(entries), p, g, n, ptr(tau_dev), _stream()), 'ptta_op_ema_multi')


def op_linear_wgrad(G, X, r, o, i, dW, db=None, **tables):
    """Test hook (include/ptta.h ptta_op_linear_wgrad; csrc/head_train.hip): dW [o, i] and db [o] of G [r, o], X [r, i], in place.  tables:
    Gh, gscale, gc1, gc2, gmean, ginv (the BatchNorm-backward transform of G) and xscale, xshift (BatchNorm + ReLU of X)."""
    a = _lib.LinearWgradArgs()
    a.r, a.o, a.i = int(r), int(o), int(i)
    for name, t in dict(tables, G=G, X=X, dW=dW, db=db).items():
        setattr(a, name, _pv(t))
    _update_rc(_lib.load().ptta_op_linear_wgrad(byref(a), _stream()), 'ptta_op_linear_wgrad')


def op_glinear_wgrad(x, ldx, i, gy, ldg, o, r, gw, gb=None):
    """Test hook (include/ptta.h ptta_op_glinear_wgrad; csrc/ghead.hip): gw [o, i] and gb [o] of x [r, ldx] and gy [r, ldg] (views of i and
    o columns), in place."""
    _update_rc(_lib.load().ptta_op_glinear_wgrad(ptr(x), int(ldx), int(i), ptr(gy), int(ldg), int(o), int(r), ptr(gw), ptr(gb), _stream()),
               'ptta_op_glinear_wgrad')


def _nl_scratch(form, b, h, w, device):
    """The fixed-point forms' workspace (include/ptta.h ptta_nl_det_scratch_bytes); form 0 takes none."""
    if not form:
        return None
    return torch.empty(int(_lib.load().ptta_nl_det_scratch_bytes(b, h, w)) // 8, device=device, dtype=torch.int64)


def op_nl_prop_bwd(pinned, fix, off9, aff9, gout, goff9, gaff9, form=0, reps=0):
    """Test / measurement hook (include/ptta.h ptta_op_nl_prop_bwd): one NLSPN propagation sweep's gradient from planar fp32 maps pinned, fix,
    gout [b, h, w], off9 [b, 18, h, w], aff9 [b, 9, h, w].  form 0: the float-atomic kernel, 1: the fixed-point form of option
    'deterministic'.  goff9 / gaff9 are accumulated into in place.  Returns (gfeat [b, h, w], microseconds per sweep of `reps` timed sweeps)."""
    lib = _lib.load()
    b, h, w = gout.shape
    assert tuple(off9.shape) == (b, 18, h, w) == tuple(goff9.shape) and tuple(aff9.shape) == (b, 9, h, w) == tuple(gaff9.shape)
    assert all(t.is_contiguous() and t.dtype == torch.float32 for t in (pinned, fix, off9, aff9, gout, goff9, gaff9))
    gfeat = torch.full((b, h, w), float('nan'), device=gout.device, dtype=torch.float32)
    scratch = _nl_scratch(form, b, h, w, gout.device)
    us = ctypes.c_float(0.0)
    rc = lib.ptta_op_nl_prop_bwd(ptr(pinned), ptr(fix), ptr(off9), ptr(aff9), ptr(gout), ptr(gfeat), ptr(goff9), ptr(gaff9), b, h, w, int(form),
                                 ptr(scratch), int(reps), byref(us), _stream())
    if rc != 0:
        raise RuntimeError('ptta_op_nl_prop_bwd failed (%d)' % rc)
    return gfeat, (us.value if reps > 0 else None)


def op_nl_affinity_bwd(oa, conf, aff_scale, goff9, gaff9, legacy=False, form=0):
    """Test hook (include/ptta.h ptta_op_nl_affinity_bwd): gradient of NLSPN's fused affinity pass.  oa [b, h, w, 24] contiguous NHWC, conf
    [b, h, w], aff_scale a one-element device tensor, goff9 [b, 18, h, w], gaff9 [b, 9, h, w].  Returns (g_oa [b, h, w, 24], gconf [b, h, w])."""
    lib = _lib.load()
    b, h, w, c = oa.shape
    assert c == 24 and tuple(goff9.shape) == (b, 18, h, w) and tuple(gaff9.shape) == (b, 9, h, w) and tuple(conf.shape) == (b, h, w)
    assert all(t.is_contiguous() and t.dtype == torch.float32 for t in (oa, conf, aff_scale, goff9, gaff9))
    goa = torch.full((b, h, w, 24), float('nan'), device=oa.device, dtype=torch.float32)
    gconf = torch.full((b, h, w), float('nan'), device=oa.device, dtype=torch.float32)
    scratch = _nl_scratch(form, b, h, w, oa.device)
    rc = lib.ptta_op_nl_affinity_bwd(ptr(oa), ptr(conf), ptr(aff_scale), int(bool(legacy)), ptr(goff9), ptr(gaff9), ptr(goa), ptr(gconf), b, h, w,
                                     int(form), ptr(scratch), _stream())
    if rc != 0:
        raise RuntimeError('ptta_op_nl_affinity_bwd failed (%d)' % rc)
    return goa, gconf


GCONV_GEOMS = {'s1': 0, 's2': 1, 't2': 2}
GCONV_ACTS = {'none': 0, 'relu': 1, 'lrelu': 2, 'sigmoid': 3}
GCONV_IMPLS = {'mfma': 0, 'direct': 1}
GCONV_FORMS = {-1: None, 0: 'plain', 1: 'nco2', 2: 'ksplit'}


def op_gconv(x0, weight, y, x1=None, bias=None, k=3, geom='s1', act='none', accumulate=False, impl='mfma', vert=False, six_b=0,
             x1_from_b=None, x1_w2=False, dgrad=False, stat_npass=0):
    """Test hook: one convolution of the generic engine (include/ptta.h ptta_op_gconv) on fp32 NHWC device tensors.  x0 [b, hin, win, c0],
    x1 [b, hin, win, c1] or None and y [b, hout, wout, co] may be channel slices of wider tensors (stride(-1) == 1, dense over pixels):
    y is written in place.  weight / bias as the state dict holds them.  Returns (form, stats): the strided launch form ('plain', 'nco2',
    'ksplit'; None for stride 1 and the direct form) and the fused statistics [stat_npass, 2, co] as float64, or None."""
    lib = _lib.load()

    def view(t):
        b, h, w, c = t.shape
        ld = t.stride(2)
        assert t.dtype == torch.float32 and t.stride(3) == 1 and t.stride(1) == w * ld and t.stride(0) == h * w * ld and ld >= c
        return c_void_p(t.data_ptr()), c, ld
    b, hin, win, _ = x0.shape
    hout, wout = y.shape[1], y.shape[2]
    assert y.shape[0] == b and (x1 is None or tuple(x1.shape[:3]) == (b, hin, win))
    p0, c0, ld0 = view(x0)
    p1, c1, ld1 = view(x1) if x1 is not None else (None, 0, 0)
    py, co, ldy = view(y)
    stats = (ctypes.c_double * (stat_npass * 2 * co))() if stat_npass else None
    form = c_int(-1)
    flags = (1 if vert else 0) | (2 if x1_w2 else 0) | (4 if dgrad else 0)
    rc = lib.ptta_op_gconv(p0, c0, ld0, p1, c1, ld1, ptr(weight.contiguous()), ptr(bias), py, co, ldy, b, hin, win, hout, wout, k,
                           GCONV_GEOMS[geom], GCONV_ACTS[act], int(bool(accumulate)), GCONV_IMPLS[impl], flags, int(six_b),
                           (1 << 30) if x1_from_b is None else int(x1_from_b), int(stat_npass), stats, byref(form), _stream())
    if rc != 0:
        raise RuntimeError('ptta_op_gconv failed (%d)' % rc)
    st = torch.tensor(list(stats), dtype=torch.float64).view(stat_npass, 2, co) if stat_npass else None
    return GCONV_FORMS[form.value], st


GCONV_AFFINE_ACTS = dict(GCONV_ACTS, elu=4)      # ELU exists behind the affine only (CostDCNet's BatchNorm3d + ELU)


def op_gconv_affine(x0, weight, y, scale, shift, x1=None, bias=None, res=None, ld_res=None, k=3, geom='s1', act='none', impl='mfma',
                    accumulate=False, act_first=False, res_plain=False, six_b=0, vert=False, stat_npass=0):
    """Test hook: op_gconv with the eval-BatchNorm epilogue of NLSPN's meta-only mode and of the stage-2 head trainer (include/ptta.h
    ptta_op_gconv_affine): y = act(fmaf(conv + bias, scale[c], shift[c]) [+ res]); act_first: relu(relu(fmaf(..)) + res); res_plain:
    fmaf(..) + res.  scale / shift [co] device tensors; res [b, hout, wout, co], possibly a channel slice of a wider tensor; ld_res
    overrides the residual's pixel stride (the argument checks); six_b: the images below it in bf16x6.  act 'elu' (stride 1, k = 3, no
    residual): fmaf, then v > 0 ? v : expm1(v); vert: the three vertical taps of a 3x1x1 Conv3d, weight [co][ci][3][1].  stat_npass: only
    for the argument checks (the epilogue has no fused statistics).  Returns the strided launch form."""
    lib = _lib.load()

    def view(t):
        b, h, w, c = t.shape
        ld = t.stride(2)
        assert t.dtype == torch.float32 and t.stride(3) == 1 and t.stride(1) == w * ld and t.stride(0) == h * w * ld and ld >= c
        return c_void_p(t.data_ptr()), c, ld
    b, hin, win, _ = x0.shape
    hout, wout = y.shape[1], y.shape[2]
    p0, c0, ld0 = view(x0)
    p1, c1, ld1 = view(x1) if x1 is not None else (None, 0, 0)
    py, co, ldy = view(y)
    pr, _, ldr = view(res) if res is not None else (None, 0, 0)
    form = c_int(-1)
    stats = (ctypes.c_double * (stat_npass * 2 * co))() if stat_npass else None
    rc = lib.ptta_op_gconv_affine(p0, c0, ld0, p1, c1, ld1, ptr(weight.contiguous()), ptr(bias), py, co, ldy, b, hin, win, hout, wout, k,
                                  GCONV_GEOMS[geom], GCONV_AFFINE_ACTS[act], int(bool(accumulate)), GCONV_IMPLS[impl],
                                  (_lib.PTTA_GCONV_AFF_ACT_FIRST if act_first else 0) | (_lib.PTTA_GCONV_AFF_RES_PLAIN if res_plain else 0) |
                                  (_lib.PTTA_GCONV_VERT if vert else 0),
                                  int(six_b), 1 << 30, int(stat_npass), stats,
                                  byref(form), ptr(scale), ptr(shift), pr, ldr if ld_res is None else int(ld_res), _stream())
    if rc != 0:
        raise RuntimeError('ptta_op_gconv_affine failed (%d)' % rc)
    return GCONV_FORMS[form.value]


GBN_MODES = {'train': 0, 'eval': 1, 'backward': 2}
GBN_ACTS = {'none': 0, 'relu': 1, 'lrelu': 2, 'elu': 4}


def op_gbn(mode, x, y, st, gamma, beta=None, res=None, g=None, gx=None, gres=None, npass=1, act='none', act_first=False, res_relu=True,
           acc_gx=False, acc_gres=False, eps=1e-5, part_in=None, rm=None, rv=None, nbt=None, momentum=0.1, repeats=1, st_eval=None,
           dgamma=None, dbeta=None, world=1):
    """Test hook: one BatchNorm of the generic engine (include/ptta.h ptta_op_gbn) on fp32 NHWC device tensors, which may be channel
    slices of wider tensors (stride(-1) == 1, dense over pixels).  mode 'train' (x, res -> y, st [4, npass, C]; part_in [npass, nblocks,
    2, C] replaces the statistics pass; rm / rv / nbt / st_eval: a tracked BatchNorm), 'eval' (rm, rv -> st [4, C], y) or 'backward'
    (x, y over all passes, g / gx / gres over pass 0, st -> gx, gres, dgamma, dbeta).  Everything is written in place; raises
    RuntimeError naming the return code otherwise."""
    lib = _lib.load()
    b, h, w, _ = x.shape
    a = _lib.GbnArgs()

    def view(t, images):
        if t is None:
            return _lib.GbnView(None, 0, 0)
        n, hh, ww, c = t.shape
        ld = t.stride(2)
        assert t.dtype == torch.float32 and (n, hh, ww) == (images, h, w), 'views disagree in size'
        assert t.stride(3) == 1 and t.stride(1) == w * ld and t.stride(0) == h * w * ld
        return _lib.GbnView(t.data_ptr(), c, ld)

    def table(t, dtype=torch.float32):
        if t is None:
            return None
        assert t.dtype == dtype and t.is_contiguous()
        return t.data_ptr()
    per = b // npass if mode == 'backward' else b
    a.mode, a.b, a.h, a.w, a.npass = GBN_MODES[mode], b, h, w, int(npass)
    a.act, a.act_first, a.res_relu, a.acc_gx, a.acc_gres = GBN_ACTS[act], int(bool(act_first)), int(bool(res_relu)), int(bool(acc_gx)), int(bool(acc_gres))
    a.world, a.repeats, a.eps, a.momentum = int(world), int(repeats), float(eps), float(momentum)
    a.nblocks_in = int(part_in.shape[1]) if part_in is not None else 0
    a.x, a.y, a.res = view(x, b), view(y, b), view(res, b)
    a.g, a.gx, a.gres = view(g, per), view(gx, per), view(gres, per)
    a.gamma, a.beta, a.part_in, a.st = table(gamma), table(beta), table(part_in), table(st)
    a.rm, a.rv, a.nbt, a.st_eval = table(rm), table(rv), table(nbt, torch.int64), table(st_eval)
    a.dgamma, a.dbeta = table(dgamma), table(dbeta)
    rc = lib.ptta_op_gbn(byref(a), _stream())
    if rc != 0:
        raise RuntimeError('ptta_op_gbn failed (%d)' % rc)


def hn_tiled_elems(r):
    """Elements of a tiled narrow [r, 512] buffer (include/ptta.h): whole 128-row blocks."""
    n = _lib.load().ptta_op_hn_tiled_elems(int(r))
    if n < 0:
        raise RuntimeError('ptta_op_hn_tiled_elems failed (%d)' % n)
    return int(n)


def _hn_fields(a, tensors):
    for name, t in tensors.items():
        if t is not None:
            assert t.is_contiguous() and t.is_cuda, name
            setattr(a, name, t.data_ptr())


def op_hn_gemm(pro, epi, r, x_bf16=False, cpart_n=0, **tensors):
    """Test hook: one GEMM of the mixed mode's narrow heads (include/ptta.h ptta_op_hn_gemm; csrc/heads_n.hip hn_gemm_kernel<pro, epi>) on
    r rows.  `tensors`: the fields of ptta_hn_gemm_args by name -- A, Bref, E, C int16 device tensors of hn_tiled_elems(r) bf16 bit patterns in
    the tiled layout; W [512, 512], W0 [512, 32], W0t [32, 512] fp32 row-major (converted inside the call); X [r, 32] fp32, or int16 bit
    patterns with x_bf16; the tables and the outputs part, rs, rowstats_out, cpart, P fp32; w_image int16 [16, 512, 32] receives the packed
    image of W.  Outputs are written in place; raises RuntimeError naming the return code otherwise."""
    a = _lib.HnGemmArgs()
    a.pro, a.epi, a.x_bf16, a.cpart_n, a.r = int(pro), int(epi), int(bool(x_bf16)), int(cpart_n), int(r)
    _hn_fields(a, tensors)
    rc = _lib.load().ptta_op_hn_gemm(byref(a), _stream())
    if rc != 0:
        raise RuntimeError('ptta_op_hn_gemm failed (%d)' % rc)


def op_hn_moments(x, w0, b0, r, npass=1, x_bf16=False, part=None, bn=False, eps=1e-5, momentum=0.1, **state):
    """Test hook: the moments chain of the narrow heads (include/ptta.h ptta_op_hn_moments; hn_moments_kernel -> hn_moment_reduce_kernel ->
    hn_moment_stats_kernel): the train-mode BatchNorm1d statistics of h = x w0^T + b0 without computing h.  x [npass, r, 32] fp32, or int16
    bf16 bit patterns with x_bf16; part [npass, 2, 2, 512] is written, or with bn the state given in `state` by the names of
    ptta_hn_moments_args: gamma, beta in; mean, inv, scale, shift out; rm, rv, nbt (int64) updated.  Raises RuntimeError naming the return code."""
    a = _lib.HnMomentsArgs()
    a.x_bf16, a.npass, a.bn, a.r, a.eps, a.momentum = int(bool(x_bf16)), int(npass), int(bool(bn)), int(r), float(eps), float(momentum)
    _hn_fields(a, dict(state, X=x, W0=w0, b0=b0, part=part))
    rc = _lib.load().ptta_op_hn_moments(byref(a), _stream())
    if rc != 0:
        raise RuntimeError('ptta_op_hn_moments failed (%d)' % rc)


def op_hn_untile(src_tiled, dst, r):
    """Test hook (include/ptta.h ptta_op_hn_untile; hn_untile_kernel): a tiled narrow tensor (int16 bit patterns) -> dst [r, 512] fp32, in place."""
    rc = _lib.load().ptta_op_hn_untile(ptr(src_tiled), ptr(dst), int(r), _stream())
    if rc != 0:
        raise RuntimeError('ptta_op_hn_untile failed (%d)' % rc)


def op_head_bwd_finish(k12, w0, p, x, r, dx, halves=1, dx_bf16=False):
    """Test hook (include/ptta.h ptta_op_head_bwd_finish; csrc/heads_bn.hip head_bwd_finish_kernel): dx [r, 32] (fp32, or int16 bf16 bit
    patterns with dx_bf16) = P - x M - u from k12 [2, 512] float64, w0 [512, 32], p [halves, r, 32] and x [r, 32] fp32; written in place."""
    assert k12.dtype == torch.float64
    rc = _lib.load().ptta_op_head_bwd_finish(ptr(k12), ptr(w0), ptr(p), ptr(x), int(r), ptr(dx), int(halves), int(bool(dx_bf16)), _stream())
    if rc != 0:
        raise RuntimeError('ptta_op_head_bwd_finish failed (%d)' % rc)


class CdSparseSet:
    """Test hook: the sparse voxel sets of CostDCNet's 3-D encoder (include/ptta.h ptta_cd_sparse) for n frames of h x w pixels, and the
    sparse kernels that run on them.  Feature tensors are fp32 device tensors [voxels of the level][channels], contiguous."""

    def __init__(self, n, h, w):
        self.lib = _lib.load()
        self.h_ = c_void_p()
        rc = self.lib.ptta_cd_sparse_create(byref(self.h_), n, h, w)
        if rc != 0:
            self.h_ = None
            raise RuntimeError('ptta_cd_sparse_create failed (%d)' % rc)
        self.n, self.h, self.w = n, h, w

    def close(self):
        if self.h_:
            self.lib.ptta_cd_sparse_destroy(self.h_)
            self.h_ = None

    __del__ = close

    def build(self, sparse, z_step):
        assert sparse.dtype == torch.float32 and sparse.is_contiguous() and sparse.numel() == self.n * self.h * self.w
        rc = self.lib.ptta_cd_sparse_build(self.h_, ptr(sparse), float(z_step), _stream())
        if rc != 0:
            raise RuntimeError('ptta_cd_sparse_build failed (%d)' % rc)

    def counts(self):
        cnt = (c_int * 3)()
        rc = self.lib.ptta_cd_sparse_read(self.h_, 0, cnt, None, 0, None, None, _stream())
        if rc != 0:
            raise RuntimeError('ptta_cd_sparse_read failed (%d)' % rc)
        return [int(v) for v in cnt]

    def read(self, level):
        """(coords [cnt][4] int32 = (frame, plane, y, x), vol [n][16][h >> level][w >> level] int32, feat_in [cnt] or None) as numpy."""
        import numpy as np
        cnt = self.counts()[level]
        coords = np.zeros((max(cnt, 1), 4), np.int32)
        vol = np.zeros((self.n, 16, self.h >> level, self.w >> level), np.int32)
        feat = np.zeros(max(cnt, 1), np.float32) if level == 0 else None
        rc = self.lib.ptta_cd_sparse_read(self.h_, level, None, coords.ctypes.data_as(c_void_p), max(cnt, 1), vol.ctypes.data_as(c_void_p),
                                          feat.ctypes.data_as(c_void_p) if feat is not None else None, _stream())
        if rc != 0:
            raise RuntimeError('ptta_cd_sparse_read failed (%d)' % rc)
        return coords[:cnt], vol, (feat[:cnt] if feat is not None else None)

    def conv(self, x, wk, y, lin, lout, ksize, backward=False, acc=False):
        """forward: x [cnt[lin]][ci] -> y [cnt[lout]][co]; backward: x = dy [cnt[lout]][co] -> y = dx [cnt[lin]][ci] (added when acc)."""
        k, ci, co = wk.shape
        assert k == ksize ** 3 and x.shape[1] == (co if backward else ci) and y.shape[1] == (ci if backward else co)
        rc = self.lib.ptta_op_cd_sparse_conv(self.h_, ptr(x), ptr(wk), ptr(y), lin, lout, ksize, ci, co, int(bool(backward)), int(bool(acc)), _stream())
        if rc != 0:
            raise RuntimeError('ptta_op_cd_sparse_conv failed (%d)' % rc)

    def bn(self, mode, level, f, gamma, st, beta=None, res=None, out=None, rm=None, rv=None, nbt=None, repeats=1, relu=False, world=1, y=None, g=None,
           gx=None, gres=None, acc_res=False, dgamma=None, dbeta=None):
        a = _lib.CdSbnArgs()
        a.mode, a.level, a.c, a.relu, a.repeats, a.world, a.acc_res = GBN_MODES[mode], level, int(gamma.numel()), int(bool(relu)), int(repeats), int(world), int(bool(acc_res))
        for name, t in (('f', f), ('res', res), ('y', y), ('g', g), ('gamma', gamma), ('beta', beta), ('rm', rm), ('rv', rv), ('nbt', nbt), ('out', out),
                        ('st', st), ('dgamma', dgamma), ('dbeta', dbeta), ('gx', gx), ('gres', gres)):
            if t is not None:
                assert t.is_contiguous() and t.dtype == (torch.int64 if name == 'nbt' else torch.float32)
                setattr(a, name, t.data_ptr())
        rc = self.lib.ptta_op_cd_sbn(self.h_, byref(a), _stream())
        if rc != 0:
            raise RuntimeError('ptta_op_cd_sbn failed (%d)' % rc)

    def densify(self, src, dst, c, backward=False, ldv=0, c0=0):
        rc = self.lib.ptta_op_cd_densify(self.h_, ptr(src), ptr(dst), int(c), int(bool(backward)), int(ldv), int(c0), _stream())
        if rc != 0:
            raise RuntimeError('ptta_op_cd_densify failed (%d)' % rc)


def op_cd_dense(op, a, out, dims, b=None, out2=None, fpar=()):
    """Test hook: one of CostDCNet's dense kernels (include/ptta.h ptta_op_cd_dense; `op` a key of _lib.CD_OPS) on contiguous fp32 device
    tensors; `dims` / `fpar` as the header lists them per op."""
    lib = _lib.load()
    for t in (a, b, out, out2):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    d = (c_int * 12)(*[int(v) for v in dims])
    f = (ctypes.c_float * 8)(*[float(v) for v in fpar])
    rc = lib.ptta_op_cd_dense(_lib.CD_OPS[op], ptr(a), ptr(b), ptr(out), ptr(out2), d, f, _stream())
    if rc != 0:
        raise RuntimeError('ptta_op_cd_dense(%s) failed (%d)' % (op, rc))
