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
The eval path's biharmonic hole filling (src/nlspn_model_adapt.py:124-127, skimage on the CPU) is `_fill` below: `fill_holes` True (the
default) runs it on the host as the reference does, 'device' on the device (include/ptta.h ptta_inpaint_biharmonic), False returns the exact
zeros of the clamped output as zeros.
`deterministic` (default False): True runs the propagation gradients of every training engine without float atomics (include/ptta.h option
'deterministic'), so that repeating a run on the same frames gives the same bits.
"""
import torch

from . import synth
from .engine import Engine
from .model import _BUFFERS, _HEAD_LEAVES, _AdapterBase, _init_tensor, _unique


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


class NlspnModel_Adapt(_AdapterBase):
    """Counterpart of src/nlspn_model_adapt.py:13-486."""

    key_table = staticmethod(synth.nlspn_keys)

    def __init__(self, device=torch.device('cuda'), max_depth=100.0, inpainting=False, use_pretrained=False, dataset_name=None,
                 from_scratch=False, offset=False, max_input_depth=None):
        self.legacy = bool(offset)                            # args.legacy = offset (src/nlspn_model_adapt.py:62)
        self.max_depth = max_depth
        self.adapt_mode = 'meta_bn'
        self.fill_holes = True            # eval forward: biharmonic hole filling like the reference, on the host ('device': on the device; False: the raw network output)
        self._deterministic = False
        super().__init__(max_depth, max_input_depth, device)

    @property
    def deterministic(self):
        """True: every engine that trains runs the propagation gradients without float atomics (include/ptta.h option 'deterministic'): the
        same frames give the same bits on every run.  Holds for the engines created from then on and for the live ones."""
        return self._deterministic

    @deterministic.setter
    def deterministic(self, value):
        self._deterministic = bool(value)
        for eng in self._engines.values():
            if eng.adapted:                       # (the source model has no backward: the library refuses the option there)
                eng.set_option('deterministic', int(self._deterministic))

    @staticmethod
    def _init(name, shape):
        if name == 'prop_layer.aff_scale_const':
            return torch.full((1,), 0.5 * 8)
        if name in ('prop_layer.w', 'prop_layer.w_conf'):
            return torch.ones(shape)
        if name == 'prop_layer.b' or name.startswith('prop_layer.conv_offset_aff'):
            return torch.zeros(shape)                         # nlspnmodel_adapt.py:221-222: zero-initialised
        return _init_tensor(name, shape)

    def _set_adapted(self):
        # adapted_listed: the reference's parameter list (2layers names the block's BatchNorm2d twice; SyncBatchNorm: the 94 tensors of the DDP run)
        keys = [k for k, _ in self._state_keys()]
        self.adapted_listed = nlspn_adapted_names(keys, self.sync_bn) if self.adapt_mode == 'meta_bn' else nlspn_meta_names(keys)
        self.adapted = _unique(self.adapted_listed)
        self._clear_engines()

    def convert_syncbn(self, apex=False):
        self._drop_plain_engines()                  # one rank only: `_plain_engine` refuses from here on
        super().convert_syncbn(apex)

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
            # the BatchNorm-adaptation baseline: gamma / beta of every BatchNorm2d (86 tensors), on the engine of include/ptta.h PTTA_META_NONE
            self._select_baseline(nlspn_adapted_names([k for k, _ in synth.nlspn_keys() if not k.startswith(_HEAD_LEAVES)]))
            return self._listed_parameters()
        if mode != 'meta_bn' and (self.meta == '2layers' or self.sync_bn):
            raise NotImplementedError("adapt_mode %r runs with the 1layer meta conv on one rank (the 2layers block and the SyncBatchNorm "
                                      "form of this mode are not built)" % mode)
        if mode != self.adapt_mode:
            self.adapt_mode = mode
            self._set_adapted()                    # new list; releases the engines of the other mode
        if mode == 'meta_bn' and not self.stats_dropped:
            self.stats_dropped = True
            self._drop_plain_engines()             # a source engine made so far normalised with the statistics this call drops
        # 2layers: four tensors listed twice -- torch.optim.Adam steps them twice per step(), as the reference's (torch 1.10.1; with torch >= 2.0
        # on the GPU build the optimizer with foreach=False for the same), and the fused step() does the same on device
        return self._listed_parameters()

    def _new_engine(self, n, h, w, plain_mode=None):
        """plain_mode: the engine without the meta layer (include/ptta.h PTTA_META_NONE) in that adapt mode."""
        eng = Engine(n, h, w, backbone='nlspn', legacy_offset=self.legacy, max_input_depth=self.max_input_depth, syncbn_adapted=self.sync_bn,
                     meta='none' if plain_mode else self.meta, adapt_mode=plain_mode or self.adapt_mode, **self.hparams)
        if self._deterministic and eng.adapted:
            eng.set_option('deterministic', 1)
        return eng

    def forward(self, image, sparse_depth, intrinsics=None, crop_mask=None, loss_type='pretrain'):
        if is_plain_loss_type(loss_type):
            return self._forward_plain(image, sparse_depth, loss_type)
        if 'head' in loss_type and 'init_meta' not in loss_type and loss_type != 'prepare':       # stage 2 (src/head_main.py:464-468)
            return self.head_forward(image, sparse_depth, loss_type)
        return self._forward_tta(image, sparse_depth, loss_type)    # training: autograd edges to the 88 adapted tensors

    def _require_baseline(self, loss_type):
        if not self.stats_dropped:
            raise RuntimeError("loss_type %r in training mode follows adapt_parameters('meta_bn') (the BatchNorm-adaptation baseline)" % loss_type)

    def _fill(self, out, loss_type):
        # Fill in any holes with inpainting (src/nlspn_model_adapt.py:124-127): exact zeros left by the final clamp are filled by
        # biharmonic interpolation on the host, as in the reference (scikit-image there; proxytta/inpaint.py restates it on scipy).
        # One flag comes back first: a map without holes -- the usual case -- never leaves the device.
        # fill_holes = 'device': the same system solved on the device (proxytta/inpaint.py inpainting_device, include/ptta.h
        # ptta_inpaint_biharmonic); the map stays there and only one status word per sample comes back.  A sample the device could not fill
        # goes through the host code, as under True.
        if self.fill_holes not in (False, True, 'device'):
            raise ValueError("fill_holes is False, True (the host path) or 'device', not %r" % (self.fill_holes,))
        if not self.fill_holes or 'head' in loss_type:
            return out
        if self.fill_holes == 'device':
            from .inpaint import inpainting_device
            return inpainting_device(out.detach().clone(memory_format=torch.contiguous_format))
        if bool((out == 0).any()):
            from .inpaint import inpainting
            out = torch.from_numpy(inpainting(out.detach().cpu().numpy())).to(out.device)
        return out

    def save_model(self, checkpoint_path, step, optimizer, meanvar=None):
        ckpt = {'net': self.model.state_dict(), 'optimizer': optimizer.state_dict() if optimizer else {}, 'train_step': step}
        if meanvar is not None:
            ckpt['meanvar'] = meanvar                         # src/nlspn_model_adapt.py:473-475
        torch.save(ckpt, checkpoint_path)
