"""Host-side mirror of src/nlspn_model_adapt.py (NLSPNModel_Adapt, the per-backbone adapter the reference selects
with model_name='nlspn', src/external_model_adapt.py:61-63) on libptta_hip.

What is on the accelerated path: the canonical TTA flow of bash/adapt/adapt_nlspn_*.sh --
prepare_mode 'meta_selfsup_seq_1layer_ema', adapt_mode 'meta_bn', loss_type 'adapt_meta_selfsup_seq_ema_reverse':
the reference's own call sequence ``forward`` / ``compute_loss`` / ``loss.backward()`` / ``optimizer.step()``
(src/tta_main.py:610-633, autograd Functions over ptta_forward_train / ptta_loss_* / ptta_backward), the fused
``step()`` (the same in one library call, Adam on device for the 88 adapted tensors) and the eval ``forward()`` (:729-736).
adapt_mode 'meta' / 'meta_fix' (src/nlspn_model_adapt.py:302-320) run on the same path with two adapted tensors: the meta conv alone
adapts, every BatchNorm2d keeps its loaded running statistics and evaluates from them in the scored eval forward (adapt_parameters below).
The network without the ProxyTTA parts (NLSPNModel_Adapt._forward, nlspnmodel_adapt.py:792-848) runs too: loss_type 'pretrain' in any form
and every string without adapt / selfsup / meta / head go to it, as in the reference (:502-509, :609-616).  In eval mode that is the source
model (the loaded checkpoint, BatchNorm2d from its running statistics); after adapt_parameters('meta_bn') on a model whose head was never
prepared it is the BatchNorm-adaptation baseline (gamma / beta of every BatchNorm2d adapt, 86 tensors, batch statistics in train and eval mode).
Any frame size from 16 x 16 up: encoder maps of odd size make the decoder maps one row / column larger and they are cropped
before each concatenation as in nlspnmodel_adapt.py:474-490 (NYUv2's 228 x 304 is such a size).
The eval path's biharmonic hole filling (src/nlspn_model_adapt.py:124-127, skimage on the CPU) is not applied: exact
zeros of the clamped output are returned as zeros.
"""
import torch
import torch.nn as nn

from . import synth
from .engine import Engine
from .costdcnet import _unique
from .model import MsgChnModel_Adapt, _ForwardFn, _init_tensor, _Tree

_BUFFERS = ('running_mean', 'running_var', 'num_batches_tracked')


def nlspn_meta_names(keys):
    """adapt_parameters('meta') and ('meta_fix') (src/nlspn_model_adapt.py:302-320): the parameters whose name contains 'meta', in
    named_parameters order -- conv1_rgb_meta.weight, conv1_rgb_meta.bias under the 1layer meta conv.  No BatchNorm parameter is listed."""
    return [k for k in keys if 'meta' in k and not k.endswith(_BUFFERS)]


def nlspn_adapted_names(keys, syncbn=False):
    """adapt_parameters('meta_bn') (src/nlspn_model_adapt.py:322-337): parameters whose name contains 'meta', then
    weight / bias of every BatchNorm2d in module order (the heads' BatchNorm1d are not BatchNorm2d).  After
    convert_syncbn() (src/tta_main.py:326 runs it BEFORE adapt_parameters) every BatchNorm is a SyncBatchNorm and the
    isinstance test also matches the heads': proj.1, proj_t.1, pred.1 join the list (94 tensors).
    2layers: the Res_Conv block's seven parameters come first; its two BatchNorm2d are BatchNorm2d too, so their gamma / beta are
    listed a second time, where the block sits in module order (last): 93 tensors, 97 entries."""
    names = [k for k in keys if 'meta' in k and not k.endswith(_BUFFERS)]
    for k in keys:
        if k.endswith('.running_mean') and (syncbn or not k.startswith(('proj', 'pred'))):
            pre = k[:-len('.running_mean')]
            names += [pre + '.weight', pre + '.bias']
    return names


def is_plain_loss_type(loss_type):
    """The strings NLSPNModel_Adapt.forward sends to `_forward`, the network without the meta layer (nlspnmodel_adapt.py:502-509, :609-616)."""
    return 'pretrain' in loss_type or not any(t in loss_type for t in ('adapt', 'selfsup', 'meta', 'head'))


class _PlainForwardFn(torch.autograd.Function):
    """depth = `_forward`(image, sparse) in training mode on the baseline engine; backward -> gradients of the 86 BatchNorm2d tensors."""

    @staticmethod
    def forward(ctx, eng, image, sparse, *adapted):
        depth, _, _ = eng.forward_train(image, sparse)
        ctx.eng = eng
        ctx.params = dict(zip(eng.adapted, adapted))
        return depth

    @staticmethod
    def backward(ctx, g_depth):
        return (None, None, None) + tuple(ctx.eng.backward_all(g_depth, None, ctx.params))


class NlspnModel_Adapt(MsgChnModel_Adapt):
    """Counterpart of src/nlspn_model_adapt.py:13-486."""

    def __init__(self, device=torch.device('cuda'), max_depth=100.0, inpainting=False, use_pretrained=False, dataset_name=None,
                 from_scratch=False, offset=False, max_input_depth=None):
        self.legacy = bool(offset)                            # args.legacy = offset (src/nlspn_model_adapt.py:62)
        self.max_predict_depth = max_depth
        self.max_depth = max_depth
        self.max_input_depth = max_input_depth
        self.device = device
        self.dtype = 'fp32'
        self.training = True
        self.prepare_mode = None
        self.adapt_mode = 'meta_bn'
        self.stats_dropped = False        # adapt_parameters('meta_bn') ran: every BatchNorm2d lost its running statistics
        self.model = _Tree()
        for k, s in synth.nlspn_keys():
            if k.startswith(('proj', 'pred', 'conv1_rgb_meta')):
                continue                                      # come with _prepare_head
            self.model._leaf(k, self._init(k, s), not k.endswith(_BUFFERS))
        self._engines = {}
        self._opt_state = {}
        self._adam_t = 0
        self.sync_bn = False
        self.hparams = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, w_sparse_depth=1.0, w_smoothness=1.0, w_cos=1.0)
        self.total_time = self.train_time = self.eval_time = 0.0
        self.fill_holes = True            # eval forward: biharmonic hole filling like the reference (False: the raw network output)
        self.to(device)

    @staticmethod
    def _init(name, shape):
        if name == 'prop_layer.aff_scale_const':
            return torch.full((1,), 0.5 * 8)
        if name in ('prop_layer.w', 'prop_layer.w_conf'):
            return torch.ones(shape)
        if name == 'prop_layer.b' or name.startswith('prop_layer.conv_offset_aff'):
            return torch.zeros(shape)                         # nlspnmodel_adapt.py:221-222: zero-initialised
        return _init_tensor(name, shape)

    heads_reverse_freezes_proj = False          # stage 2: ref = proj_t(...), proj trains in both directions (csrc/ghead.hip)

    def _state_keys(self):
        return [(k, s) for k, s in synth.nlspn_keys(self.prepare_mode) if not (k.startswith('enc2d.') and '.downsample.1.' in k)]

    def _prepare_head(self, mode=''):
        """NLSPNModel_Adapt._prepare_head (nlspnmodel_adapt.py:1333-1396)."""
        if 'meta' not in mode or 'selfsup' not in mode or 'ema' not in mode or 'seq' not in mode or \
                ('1layer' not in mode and '2layers' not in mode):
            raise NotImplementedError('hot path covers prepare_mode meta_selfsup_seq_{1layer,2layers}_ema, got %r' % mode)
        self.prepare_mode = mode
        self.meta = '2layers' if '2layers' in mode else '1layer'
        for k, s in synth.nlspn_keys(mode):
            if k.startswith(('proj', 'pred', 'conv1_rgb_meta')):
                self.model._leaf(k, _init_tensor(k, s).to(self.device), not k.endswith(_BUFFERS))
        self._set_adapted()

    def _set_adapted(self):
        # adapted_listed: the reference's parameter list (2layers names the block's BatchNorm2d twice); adapted: the tensors behind it
        keys = [k for k, _ in synth.nlspn_keys(self.prepare_mode)]
        self.adapted_listed = nlspn_adapted_names(keys, self.sync_bn) if self.adapt_mode == 'meta_bn' else nlspn_meta_names(keys)
        self.adapted = _unique(self.adapted_listed)
        self._clear_engines()

    def _drop_plain_engines(self):
        for key in [k for k in self._engines if k[0] == 'plain']:
            self._engines.pop(key).close()

    def convert_syncbn(self, apex=False):
        self._drop_plain_engines()                  # one rank only: `_plain_engine` refuses from here on
        super().convert_syncbn(apex)
        if getattr(self, '_head_syncbn', False):    # stage 2: the head trainer's SyncBatchNorm form, the TTA list unchanged
            return
        if self.prepare_mode is not None:           # heads exist: the adapted list grows to the 94 tensors of the DDP run
            self._set_adapted()

    def adapt_parameters(self, mode=None):
        """src/nlspn_model_adapt.py:287-340.  'meta_bn' (the NLSPN scripts' mode): the meta layer + gamma / beta of every BatchNorm2d, which
        lose their running statistics (batch statistics in train and eval mode).  'meta' (the method itself) and 'meta_fix': the meta conv's
        weight and bias only; every BatchNorm2d keeps its loaded buffers with track_running_stats = False -- batch statistics in train-mode
        passes, no buffer written, and the LOADED running statistics and gamma / beta in the scored eval forward.  The two differ in the
        reference only by the requires_grad flags of the frozen BatchNorm parameters, which no optimiser sees: in one process they are
        numerically identical, and both select the same engine mode here (include/ptta.h PTTA_ADAPT_META_ONLY).  The mode holds for the
        engines created afterwards; switching it releases the existing ones, as _prepare_head does."""
        if mode not in ('meta_bn', 'meta', 'meta_fix'):
            raise NotImplementedError("adapt_mode %r: 'meta_bn' (the NLSPN scripts' mode), 'meta' and 'meta_fix' are on the accelerated path" % mode)
        if self.prepare_mode is None:
            if mode != 'meta_bn':
                raise RuntimeError('_prepare_head(mode) must be called before adapt_parameters (tta_main.py:322, :339)')
            # the BatchNorm-adaptation baseline: no parameter is called 'meta' yet, so the list is gamma / beta of every BatchNorm2d (86 tensors);
            # forward / step / compute_loss then run on the engine without the meta layer (include/ptta.h PTTA_META_NONE)
            if self.sync_bn:
                raise NotImplementedError('the BatchNorm-adaptation baseline runs on one rank (no SyncBatchNorm form)')
            keys = [k for k, _ in synth.nlspn_keys() if not k.startswith(('proj', 'pred', 'conv1_rgb_meta'))]
            self.adapt_mode = 'meta_bn'
            self.adapted_listed = nlspn_adapted_names(keys)
            self.adapted = list(self.adapted_listed)
            self.stats_dropped = True
            self._clear_engines()
            params = dict(self.model.named_parameters())
            return nn.ParameterList([params[k] for k in self.adapted_listed])
        if mode != 'meta_bn' and (self.meta == '2layers' or self.sync_bn):
            raise NotImplementedError("adapt_mode %r runs with the 1layer meta conv on one rank (the 2layers block and the SyncBatchNorm "
                                      "form of this mode are not built)" % mode)
        if mode != self.adapt_mode:
            self.adapt_mode = mode
            self._set_adapted()                    # new list; releases the engines of the other mode
        if mode == 'meta_bn' and not self.stats_dropped:
            self.stats_dropped = True
            self._drop_plain_engines()             # a source engine made so far normalised with the statistics this call drops
        params = dict(self.model.named_parameters())
        # 2layers: four tensors listed twice -- torch.optim.Adam steps them twice per step(), as the reference's (torch 1.10.1; with torch >= 2.0
        # on the GPU build the optimizer with foreach=False for the same), and the fused step() does the same on device
        return nn.ParameterList([params[k] for k in self.adapted_listed])

    def _engine(self, image):
        n, _, h, w = image.shape
        key = (n, h, w)
        eng = self._engines.get(key)
        if eng is None:
            if self.prepare_mode is None:
                if self.stats_dropped:             # the baseline model: its only engine is the one without the meta layer
                    return self._plain_engine(image)
                raise RuntimeError('_prepare_head(mode) must be called before forward (tta_main.py:322)')
            eng = self._make_engine(key, n, h, w, self.meta, self.adapt_mode)
        return eng

    def _plain_engine(self, image):
        """The engine of `_forward`, the network without the meta layer: the baseline kind once adapt_parameters('meta_bn') dropped the running
        statistics (batch statistics, gamma / beta of every BatchNorm2d bound to this model's parameters), the source kind before."""
        if self.sync_bn:
            raise NotImplementedError("the network without the meta layer runs on one rank (no SyncBatchNorm form of loss_type 'pretrain')")
        n, _, h, w = image.shape
        key = ('plain', n, h, w)
        eng = self._engines.get(key)
        if eng is None:
            eng = self._make_engine(key, n, h, w, 'none', 'meta_bn' if self.stats_dropped else 'meta')
        return eng

    def _make_engine(self, key, n, h, w, meta, adapt_mode):
        eng = Engine(n, h, w, backbone='nlspn', legacy_offset=self.legacy, max_input_depth=self.max_input_depth,
                     syncbn_adapted=self.sync_bn, meta=meta, adapt_mode=adapt_mode, **self.hparams)
        if meta == 'none':     # the source model adapts nothing; the baseline every BatchNorm2d tensor of this model's list, none twice
            want = [k for k in self.adapted if 'meta' not in k] if adapt_mode == 'meta_bn' else []
            assert eng.adapted == want and all(eng.adapted_repeat[k] == 1 for k in want), 'adapted parameter list drifted from the library'
        else:
            assert all(self.adapted_listed.count(k) == max(eng.adapted_repeat[k], 1) for k in eng.adapted), 'listing counts drifted'
            assert eng.adapted == self.adapted, 'adapted parameter list drifted from the library'
        eng.load_state_dict(self.model.state_dict())     # the heads' BatchNorm1d buffers are bound and updated in place
        params = dict(self.model.named_parameters())
        for name in eng.adapted:
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

    def forward(self, image, sparse_depth, intrinsics=None, crop_mask=None, loss_type='pretrain'):
        if is_plain_loss_type(loss_type):
            return self._forward_plain(image, sparse_depth, loss_type)
        if 'head' in loss_type and 'init_meta' not in loss_type and loss_type != 'prepare':       # stage 2 (src/head_main.py:464-468)
            if not self.training:
                raise NotImplementedError('the head forward is a training-mode call (head_main.py:441)')
            return self.head_forward(image, sparse_depth, loss_type)
        if self.training and 'adapt' in loss_type:
            # (depth, emb, ref) with autograd edges to the 88 adapted tensors: loss.backward() runs ptta_loss_backward +
            # ptta_backward and fills their .grad (src/tta_main.py:610-632)
            params = dict(self.model.named_parameters())
            return self._timed(lambda: _ForwardFn.apply(self, image, sparse_depth, *[params[k] for k in self.adapted]), loss_type)
        with torch.no_grad():
            out = self._timed(lambda: self._engine(image).forward_eval(image, sparse_depth), loss_type)
        return self._fill(out, loss_type)

    def _forward_plain(self, image, sparse_depth, loss_type):
        """`_forward` (nlspnmodel_adapt.py:792-848).  Eval: the depth.  Training with 'bn' in the string: (depth, None, None) with autograd edges
        to the 86 BatchNorm2d tensors of the baseline.  Training without 'bn': the reference returns a tensor with autograd into EVERY
        parameter, which is not on the accelerated path."""
        if self.training:
            if 'bn' not in loss_type:
                raise NotImplementedError("loss_type %r in training mode: autograd into every parameter is not on the accelerated path "
                                          "('bn' in the string: the BatchNorm-adaptation baseline)" % loss_type)
            if not self.stats_dropped:
                raise RuntimeError("loss_type %r in training mode follows adapt_parameters('meta_bn') (the BatchNorm-adaptation baseline)" % loss_type)
            eng = self._plain_engine(image)
            params = dict(self.model.named_parameters())
            depth = self._timed(lambda: _PlainForwardFn.apply(eng, image, sparse_depth, *[params[k] for k in eng.adapted]), loss_type)
            return depth, None, None
        with torch.no_grad():
            out = self._timed(lambda: self._plain_engine(image).forward_eval(image, sparse_depth), loss_type)
        return self._fill(out, loss_type)

    def _fill(self, out, loss_type):
        # Fill in any holes with inpainting (src/nlspn_model_adapt.py:124-127): exact zeros left by the final clamp are filled by
        # biharmonic interpolation on the host, as in the reference (scikit-image there; proxytta/inpaint.py restates it on scipy).
        # One flag comes back first: a map without holes -- the usual case -- never leaves the device.
        if self.fill_holes and 'head' not in loss_type and bool((out == 0).any()):
            from .inpaint import inpainting
            out = torch.from_numpy(inpainting(out.detach().cpu().numpy())).to(out.device)
        return out

    def save_model(self, checkpoint_path, step, optimizer, meanvar=None):
        ckpt = {'net': self.model.state_dict(), 'optimizer': optimizer.state_dict() if optimizer else {}, 'train_step': step}
        if meanvar is not None:
            ckpt['meanvar'] = meanvar                         # src/nlspn_model_adapt.py:473-475
        torch.save(ckpt, checkpoint_path)
