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

from . import synth
from .engine import Engine
from .model import _BUFFERS, _HEAD_LEAVES, _AdapterBase, _unique


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


def _is_norm3_alias(k):
    """The reference's state_dict lists ResBlock.norm3 a second time as downsample.1 (same tensors); this model holds it once."""
    return k.startswith('enc2d.') and '.downsample.1.' in k


class CostDCNetModel_Adapt(_AdapterBase):
    """Counterpart of src/costdcnet_model_adapt.py:31-556."""

    key_table = staticmethod(synth.costdcnet_keys)

    def __init__(self, device=torch.device('cuda'), max_depth=10.0, max_input_depth=None):
        self.max_depth = max_depth
        self._weights_version = 0         # counts the ProxyTTA training calls: see _plain_engine
        super().__init__(max_depth, max_input_depth, device)

    def _state_keys(self):
        return [(k, s) for k, s in super()._state_keys() if not _is_norm3_alias(k)]

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
            # the BatchNorm-adaptation baseline (src/costdcnet_model_adapt.py:357-378 on a model whose head was never prepared): gamma / beta of
            # Encoder2D's 15 BatchNorm2d (30 tensors), on the engine of include/ptta.h PTTA_COSTDC_PLAIN
            self._select_baseline(costdcnet_adapted_names([k for k, _ in synth.costdcnet_keys() if not k.startswith(_HEAD_LEAVES)]))
        elif not self.stats_dropped:
            self._drop_plain_engines()             # a source engine made so far normalised with the statistics this call drops
        self.stats_dropped = True
        # the DDP list names four tensors twice: torch.optim.Adam then steps them twice per step(), like the reference's.  The reference
        # pins torch 1.10.1 (README.md:74: one entry at a time, two complete consecutive updates -- what step() does on device); with
        # torch >= 2.0 build the optimizer with foreach=False to get the same from optimizer.step()
        return self._listed_parameters()

    def state_dict(self):
        """The reference's state_dict, with ResBlock.norm3 a second time under its alias."""
        sd = self.model.state_dict()
        out = {}
        for k, _ in synth.costdcnet_keys(self.prepare_mode or 'meta_selfsup_seq_1layer_ema'):
            src = k.replace('.downsample.1.', '.norm3.') if k.startswith('enc2d.') else k
            if src in sd:
                out[k] = sd[src]
        return out

    def load_state_dict(self, state):
        super().load_state_dict({k: v for k, v in state.items() if not _is_norm3_alias(k)})

    def save_model(self, checkpoint_path, step, optimizer, meanvar=None):
        torch.save({'net': self.state_dict(), 'optimizer': optimizer.state_dict() if optimizer else {}, 'train_step': step}, checkpoint_path)

    def _new_engine(self, n, h, w, plain_mode=None):
        """plain_mode: the engine without the meta layer (include/ptta.h PTTA_COSTDC_PLAIN) in that adapt mode.  The ProxyTTA engine takes no
        adapt_mode: 'meta_bn' is this backbone's only one."""
        kind = dict(meta='plain', adapt_mode=plain_mode) if plain_mode else dict(syncbn_adapted=self.sync_bn, meta=self.meta)
        return Engine(n, h, w, backbone='costdcnet', max_input_depth=self.max_input_depth, max_predict_depth=self.max_depth, **kind, **self.hparams)

    def _plain_engine(self, image):
        """The source kind COPIES gamma / beta and Encoder2D's statistics and builds its BatchNorm tables once per load, and either kind reads
        BatchNorm3d / sparse buffers that a ProxyTTA engine of the same model updates in place: a plain engine that is older than the last
        ProxyTTA training call (`_weights_version`) loads the model's state again before it runs.  An optimizer outside the library
        (forward -> loss.backward() -> torch.optim.Adam.step) writes gamma / beta after that call: torch counts every in-place write of a
        tensor, so the stamp an engine carries (`_plain_stamp`) holds those counts too, and a 'pretrain' call on either side of
        optimizer.step() sees the parameters as they are."""
        eng = super()._plain_engine(image)
        stamp = self._plain_stamp()
        if getattr(eng, '_version', stamp) != stamp:          # (a new engine has loaded the state just now)
            eng.load_state_dict(self._plain_state())
        eng._version = stamp
        return eng

    def _plain_state(self):
        return {k: v for k, v in self.model.state_dict().items() if not k.startswith(_HEAD_LEAVES)}

    def _plain_stamp(self):
        """What a plain engine's copy of this model was taken at: the ProxyTTA training calls so far (they move buffers and, in the fused step,
        parameters through the library) and torch's write counts of Encoder2D's parameters (an optimizer's in-place updates)."""
        return (self._weights_version, sum(p._version for k, p in self.model.named_parameters() if k.startswith('enc2d.')))

    def step(self, image, sparse_depth, validity_map=None, loss_image=None, want_depth=False, next_frame=None):
        if self.prepare_mode is not None:
            self._weights_version += 1             # a ProxyTTA step moves what a plain engine of this model copied or tabulated
        return super().step(image, sparse_depth, validity_map, loss_image, want_depth, next_frame)

    def _require_baseline(self, loss_type):
        if not self.stats_dropped or self.prepare_mode is not None:
            raise RuntimeError("loss_type %r in training mode follows adapt_parameters('meta_bn') on a model whose head was never prepared "
                               "(the BatchNorm-adaptation baseline)" % loss_type)

    def forward(self, image, sparse_depth, intrinsics=None, crop_mask=None, loss_type='pretrain'):
        if 'pretrain' in loss_type:                # the first test of CostDCNet.forward (CostDCNet_adapt.py:44-54), on a prepared model too
            return self._forward_plain(image, sparse_depth, loss_type)
        if 'head' in loss_type and 'init_meta' not in loss_type and loss_type != 'prepare':       # stage 2 (src/head_main.py:464-468)
            return self.head_forward(image, sparse_depth, loss_type)
        if self.training and 'adapt' in loss_type:
            self._weights_version += 1             # the training forward moves the BatchNorm buffers a plain engine reads
        return self._forward_tta(image, sparse_depth, loss_type)
