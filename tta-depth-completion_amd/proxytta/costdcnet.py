"""Host-side mirror of src/costdcnet_model_adapt.py (CostDCNetModel_Adapt, the per-backbone adapter the reference selects
with model_name='costdcnet', src/external_model_adapt.py:76-78) on libptta_hip.

On the accelerated path: the canonical TTA flow of bash/adapt/adapt_costdc_*.sh -- prepare_mode
'meta_selfsup_seq_1layer_ema', adapt_mode 'meta_bn', loss_type 'adapt_meta_selfsup_seq_ema_reverse': the reference's own
call sequence forward / compute_loss / loss.backward() / optimizer.step() (src/tta_main.py:610-633), the fused step() and
the eval forward (:729-736).  res = 16 depth planes, up_scale = 4 (src/costdcnet_model_adapt.py:47-52); frame sizes not
divisible by 16 run the reference's dual-corner padding inside the library.  The sparse 3-D encoder's arithmetic lives in
MinkowskiEngine in the reference (absent there, parity unpinned): see csrc/costdc_kernels.hip.
"""
import torch
import torch.nn as nn

from . import synth
from .engine import Engine
from .model import MsgChnModel_Adapt, _ForwardFn, _init_tensor, _Tree

_BUFFERS = ('running_mean', 'running_var', 'num_batches_tracked')


def costdcnet_adapted_names(keys, syncbn=False):
    """adapt_parameters('meta_bn') (src/costdcnet_model_adapt.py:357-378): parameters whose name contains 'meta', then
    weight / bias of every BatchNorm2d in module order = Encoder2D's (BatchNorm3d, BatchNorm1d and the sparse encoder's
    MinkowskiBatchNorm are not BatchNorm2d; ResBlock.norm3 also sits inside `downsample` but a module is visited once).
    syncbn: the list of the reference's DDP run.  convert_syncbn() runs BEFORE adapt_parameters (src/tta_main.py:326,339), every
    BatchNorm is a SyncBatchNorm by then and passes the isinstance test (:364-366): Encoder2D's, the BatchNorm1d inside each
    MinkowskiBatchNorm (`enc3d.<layer>.bn`), UNet3D's BatchNorm3d and the heads' BatchNorm1d -- 116 entries.
    convert_sync_batchnorm builds one new module per visited attribute, so ResBlock.norm3 and its alias downsample[1] are two
    modules around ONE Parameter: enc2d.layer{2,3}.0.norm3.{weight,bias} are listed twice (and stepped twice by Adam).
    2layers: the Res_Conv block's seven parameters come first, its two BatchNorm2d again at the end of the BatchNorm pass (the block is
    registered last): 37 tensors, 41 entries."""
    names = [k for k in keys if 'meta' in k and not k.endswith(_BUFFERS)]
    for k in keys:
        if not k.endswith('.running_mean'):
            continue
        pre = k[:-len('.running_mean')]
        if not syncbn:
            if (k.startswith('enc2d.') and '.downsample.1.' not in k) or k.startswith('conv1_rgb_meta.'):
                names += [pre + '.weight', pre + '.bias']
            continue
        if pre.startswith('enc2d.'):
            pre = pre.replace('.downsample.1', '.norm3')
        names += [pre + '.weight', pre + '.bias']
    return names


def _unique(names):
    seen, out = set(), []
    for k in names:
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out


class _PlainForwardFn(torch.autograd.Function):
    """depth = `_forward`(image, sparse) in training mode on the baseline engine; backward -> gradients of the 30 BatchNorm2d tensors."""

    @staticmethod
    def forward(ctx, eng, image, sparse, *adapted):
        depth, _, _ = eng.forward_train(image, sparse)
        ctx.eng = eng
        ctx.params = dict(zip(eng.adapted, adapted))
        return depth

    @staticmethod
    def backward(ctx, g_depth):
        return (None, None, None) + tuple(ctx.eng.backward_all(g_depth, None, ctx.params))


class CostDCNetModel_Adapt(MsgChnModel_Adapt):
    """Counterpart of src/costdcnet_model_adapt.py:31-556."""

    def __init__(self, device=torch.device('cuda'), max_depth=10.0, max_input_depth=None):
        self.max_predict_depth = max_depth
        self.max_depth = max_depth
        self.max_input_depth = max_input_depth
        self.device = device
        self.dtype = 'fp32'
        self.training = True
        self.prepare_mode = None
        self.model = _Tree()
        for k, s in synth.costdcnet_keys():
            if k.startswith(('proj', 'pred', 'conv1_rgb_meta')) or ('.downsample.1.' in k and k.startswith('enc2d.')):
                continue                                      # heads / meta layer come with _prepare_head; norm3 is one module
            self.model._leaf(k, _init_tensor(k, s), not k.endswith(_BUFFERS))
        self._engines = {}
        self._opt_state = {}
        self._adam_t = 0
        self.sync_bn = False
        self.stats_dropped = False        # adapt_parameters('meta_bn') ran: Encoder2D's BatchNorm2d lost their running statistics
        self._weights_version = 0         # counts the ProxyTTA training calls: see _plain_engine
        self.hparams = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, w_sparse_depth=1.0, w_smoothness=1.0, w_cos=1.0)
        self.total_time = self.train_time = self.eval_time = 0.0
        self.to(device)

    heads_reverse_freezes_proj = False          # stage 2: ref = proj_t(...), proj trains in both directions (csrc/ghead.hip)

    def _state_keys(self):
        return [(k, s) for k, s in synth.costdcnet_keys(self.prepare_mode) if not (k.startswith('enc2d.') and '.downsample.1.' in k)]

    def _prepare_head(self, mode=''):
        """CostDCNet._prepare_head (CostDCNet_adapt.py:426-496)."""
        if 'meta' not in mode or 'selfsup' not in mode or 'ema' not in mode or 'seq' not in mode or \
                ('1layer' not in mode and '2layers' not in mode):
            raise NotImplementedError('hot path covers prepare_mode meta_selfsup_seq_{1layer,2layers}_ema, got %r' % mode)
        self.prepare_mode = mode
        self.meta = '2layers' if '2layers' in mode else '1layer'
        for k, s in synth.costdcnet_keys(mode):
            if k.startswith(('proj', 'pred', 'conv1_rgb_meta')):
                self.model._leaf(k, _init_tensor(k, s).to(self.device), not k.endswith(_BUFFERS))
        self._set_adapted()

    def _set_adapted(self):
        # adapted_listed: the reference's parameter list (duplicates included); adapted: the tensors behind it, as the library binds them
        self.adapted_listed = costdcnet_adapted_names([k for k, _ in synth.costdcnet_keys(self.prepare_mode)], self.sync_bn)
        self.adapted = _unique(self.adapted_listed)
        # proj / pred feed the detached embedding (CD:249): their BatchNorm parameters never get a gradient, torch.optim.Adam skips them
        self._never_stepped = {k for k in self.adapted if k.startswith(('proj.1.', 'pred.1.'))} if self.sync_bn else set()
        self._clear_engines()

    def adapt_parameters(self, mode=None):
        if mode != 'meta_bn':
            raise NotImplementedError("adapt_mode %r: only 'meta_bn' (the CostDCNet scripts' mode) is on the accelerated path" % mode)
        if self.prepare_mode is None:
            # the BatchNorm-adaptation baseline (src/costdcnet_model_adapt.py:357-378 on a model whose head was never prepared): no parameter is
            # called 'meta' yet, so the list is gamma / beta of Encoder2D's 15 BatchNorm2d (30 tensors); forward / step / compute_loss then
            # run on the engine without the meta layer (include/ptta.h PTTA_COSTDC_PLAIN)
            if self.sync_bn:
                raise NotImplementedError('the BatchNorm-adaptation baseline runs on one rank (no SyncBatchNorm form)')
            keys = [k for k, _ in synth.costdcnet_keys() if not k.startswith(('proj', 'pred', 'conv1_rgb_meta'))]
            self.adapted_listed = costdcnet_adapted_names(keys)
            self.adapted = list(self.adapted_listed)
            self._never_stepped = set()
            self._clear_engines()
        elif not self.stats_dropped:
            self._drop_plain_engines()             # a source engine made so far normalised with the statistics this call drops
        self.stats_dropped = True
        params = dict(self.model.named_parameters())
        # the DDP list names four tensors twice: torch.optim.Adam then steps them twice per step(), like the reference's.  The reference
        # pins torch 1.10.1 (README.md:74: one entry at a time, two complete consecutive updates -- what step() does on device); with
        # torch >= 2.0 build the optimizer with foreach=False to get the same from optimizer.step()
        return nn.ParameterList([params[k] for k in self.adapted_listed])

    def convert_syncbn(self, apex=False):
        """SyncBatchNorm.convert_sync_batchnorm (src/costdcnet_model_adapt.py:535-546).  The reference converts BEFORE
        adapt_parameters('meta_bn') (src/tta_main.py:326,339): from here on every BatchNorm of the model is adapted and normalises
        with batch statistics in train AND eval mode (its running statistics are dropped, :364-372) -- the library's
        PTTA_SYNCBN_ADAPT engine, whose sparse encoder has a backward for its BatchNorm gamma / beta."""
        super().convert_syncbn(apex)
        if getattr(self, '_head_syncbn', False):    # stage 2: the head trainer's SyncBatchNorm form, the TTA list unchanged
            return
        if self.prepare_mode is not None:
            self._set_adapted()

    def state_dict(self):
        """The reference's state_dict lists ResBlock.norm3 a second time as downsample.1 (same tensors)."""
        sd = self.model.state_dict()
        out = {}
        for k, _ in synth.costdcnet_keys(self.prepare_mode or 'meta_selfsup_seq_1layer_ema'):
            src = k.replace('.downsample.1.', '.norm3.') if k.startswith('enc2d.') else k
            if src in sd:
                out[k] = sd[src]
        return out

    def load_state_dict(self, state):
        state = {k: v for k, v in state.items() if not (k.startswith('enc2d.') and '.downsample.1.' in k)}
        super().load_state_dict(state)

    def save_model(self, checkpoint_path, step, optimizer, meanvar=None):
        torch.save({'net': self.state_dict(), 'optimizer': optimizer.state_dict() if optimizer else {}, 'train_step': step}, checkpoint_path)

    def _engine(self, image):
        n, _, h, w = image.shape
        key = (n, h, w)
        eng = self._engines.get(key)
        if eng is None:
            if self.prepare_mode is None:
                if self.stats_dropped:             # the baseline model: its only engine is the one without the meta layer
                    return self._plain_engine(image)
                raise RuntimeError('_prepare_head(mode) must be called before forward (tta_main.py:322)')
            eng = Engine(n, h, w, backbone='costdcnet', max_input_depth=self.max_input_depth, max_predict_depth=self.max_depth,
                         syncbn_adapted=self.sync_bn, meta=self.meta, **self.hparams)
            assert all(self.adapted_listed.count(k) == max(eng.adapted_repeat[k], 1) for k in eng.adapted), 'listing counts drifted'
            assert eng.adapted == self.adapted, 'adapted parameter list drifted from the library'
            eng.load_state_dict(self.model.state_dict())      # running statistics are bound by pointer and updated in place
            params = dict(self.model.named_parameters())
            for name in self.adapted:
                p = params[name]
                st = self._opt_state.setdefault(name, {'exp_avg': torch.zeros_like(p.data), 'exp_avg_sq': torch.zeros_like(p.data)})
                eng.bind_adapted(name, p.data, st['exp_avg'], st['exp_avg_sq'])
            if getattr(self, '_image_norm', None) is not None:
                eng.set_image_norm(self._image_norm)
            eng._t = 0
            if self.sync_bn:
                eng.enable_stat_sync()
            self._engines[key] = eng
        return eng

    def _plain_engine(self, image):
        """The engine of `_forward`, the network without the meta layer (include/ptta.h PTTA_COSTDC_PLAIN): the baseline kind once
        adapt_parameters('meta_bn') dropped Encoder2D's running statistics (batch statistics there, its gamma / beta bound to this model's
        parameters), the source kind before (every BatchNorm from the loaded running statistics, eval forward only).  One per shape, beside
        the ProxyTTA engines; the meta layer and the heads of a prepared model are not part of it.
        The source kind COPIES gamma / beta and Encoder2D's statistics and builds its BatchNorm tables once per load, and either kind reads
        BatchNorm3d / sparse buffers that a ProxyTTA engine of the same model updates in place: a plain engine that is older than the last
        ProxyTTA training call (`_weights_version`) loads the model's state again before it runs.  An optimizer outside the library
        (forward -> loss.backward() -> torch.optim.Adam.step) writes gamma / beta after that call: torch counts every in-place write of a
        tensor, so the stamp an engine carries (`_plain_stamp`) holds those counts too, and a 'pretrain' call on either side of
        optimizer.step() sees the parameters as they are."""
        if self.sync_bn:
            raise NotImplementedError("the network without the meta layer runs on one rank (no SyncBatchNorm form of loss_type 'pretrain')")
        n, _, h, w = image.shape
        key = ('plain', n, h, w)
        eng = self._engines.get(key)
        state = lambda: {k: v for k, v in self.model.state_dict().items() if not k.startswith(('proj', 'pred', 'conv1_rgb_meta'))}
        if eng is None:
            baseline = self.stats_dropped
            eng = Engine(n, h, w, backbone='costdcnet', max_input_depth=self.max_input_depth, max_predict_depth=self.max_depth,
                         meta='plain', adapt_mode='meta_bn' if baseline else 'meta', **self.hparams)
            want = [k for k in self.adapted if k.startswith('enc2d.')] if baseline else []
            assert eng.adapted == want and all(eng.adapted_repeat[k] == 1 for k in want), 'adapted parameter list drifted from the library'
            eng.load_state_dict(state())
            params = dict(self.model.named_parameters())
            for name in eng.adapted:
                p = params[name]
                st = self._opt_state.setdefault(name, {'exp_avg': torch.zeros_like(p.data), 'exp_avg_sq': torch.zeros_like(p.data)})
                eng.bind_adapted(name, p.data, st['exp_avg'], st['exp_avg_sq'])
            if getattr(self, '_image_norm', None) is not None:
                eng.set_image_norm(self._image_norm)
            eng._t = 0
            eng._version = self._plain_stamp()
            self._engines[key] = eng
        elif eng._version != self._plain_stamp():
            eng.load_state_dict(state())
            eng._version = self._plain_stamp()
        return eng

    def _plain_stamp(self):
        """What a plain engine's copy of this model was taken at: the ProxyTTA training calls so far (they move buffers and, in the fused step,
        parameters through the library) and torch's write counts of Encoder2D's parameters (an optimizer's in-place updates)."""
        return (self._weights_version, sum(p._version for k, p in self.model.named_parameters() if k.startswith('enc2d.')))

    def _drop_plain_engines(self):
        for key in [k for k in self._engines if k[0] == 'plain']:
            self._engines.pop(key).close()

    def step(self, image, sparse_depth, validity_map=None, loss_image=None, want_depth=False, next_frame=None):
        if self.prepare_mode is not None:
            self._weights_version += 1             # a ProxyTTA step moves what a plain engine of this model copied or tabulated
        return super().step(image, sparse_depth, validity_map, loss_image, want_depth, next_frame)

    def _forward_plain(self, image, sparse_depth, loss_type):
        """`_forward` (CostDCNet_adapt.py:177-205).  Eval: the depth.  Training with 'bn' in the string: (depth, None, None) with autograd edges
        to the 30 BatchNorm2d tensors of the baseline.  Training without 'bn': the reference returns a tensor with autograd into EVERY
        parameter, which is not on the accelerated path."""
        if self.training:
            if 'bn' not in loss_type:
                raise NotImplementedError("loss_type %r in training mode: autograd into every parameter is not on the accelerated path "
                                          "('bn' in the string: the BatchNorm-adaptation baseline)" % loss_type)
            if not self.stats_dropped or self.prepare_mode is not None:
                raise RuntimeError("loss_type %r in training mode follows adapt_parameters('meta_bn') on a model whose head was never prepared "
                                   "(the BatchNorm-adaptation baseline)" % loss_type)
            eng = self._plain_engine(image)
            params = dict(self.model.named_parameters())
            depth = self._timed(lambda: _PlainForwardFn.apply(eng, image, sparse_depth, *[params[k] for k in eng.adapted]), loss_type)
            return depth, None, None
        with torch.no_grad():
            return self._timed(lambda: self._plain_engine(image).forward_eval(image, sparse_depth), loss_type)

    def forward(self, image, sparse_depth, intrinsics=None, crop_mask=None, loss_type='pretrain'):
        if 'pretrain' in loss_type:                # the first test of CostDCNet.forward (CostDCNet_adapt.py:44-54), on a prepared model too
            return self._forward_plain(image, sparse_depth, loss_type)
        if 'head' in loss_type and 'init_meta' not in loss_type and loss_type != 'prepare':       # stage 2 (src/head_main.py:464-468)
            if not self.training:
                raise NotImplementedError('the head forward is a training-mode call (head_main.py:441)')
            return self.head_forward(image, sparse_depth, loss_type)
        if self.training and 'adapt' in loss_type:
            self._weights_version += 1
            params = dict(self.model.named_parameters())
            return self._timed(lambda: _ForwardFn.apply(self, image, sparse_depth, *[params[k] for k in self.adapted]), loss_type)
        with torch.no_grad():
            return self._timed(lambda: self._engine(image).forward_eval(image, sparse_depth), loss_type)
