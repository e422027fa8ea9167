"""Host-side mirror of the reference's plugin surface for the ProxyTTA hot path.

``ExternalModel_Adapt`` keeps the method names, argument meaning and return values of
src/external_model_adapt.py:29-660 and of the per-backbone adapter src/msg_chn_model_adapt.py
(forward / compute_loss / _prepare_head / adapt_parameters / parameters / train / eval / to /
restore_model / save_model / convert_syncbn / distributed_data_parallel), so a tta_main-style
driver runs unchanged; underneath, forward, loss, backward and Adam are libptta_hip kernels.
``step()`` and ``adapt()`` are the fused entry points the reference only has inline
(src/tta_main.py:579-636 and :504-804).
``_AdapterBase`` holds what the three per-backbone adapters share (``MsgChnModel_Adapt`` here, proxytta/nlspn.py, proxytta/costdcnet.py);
what a backbone does differently is an override or a class attribute there.
"""
import math

import torch
import torch.nn as nn

from . import _lib, synth
from .engine import HEAD_TARGETS, Engine, adapted_names
from .engine import _BOUND_SUFFIX as _BUFFERS               # the BatchNorm leaves that are buffers, not parameters

CANONICAL_LOSS_TYPE = 'adapt_meta_selfsup_seq_ema_reverse'
_HEAD_LEAVES = ('proj', 'pred', 'conv1_rgb_meta')           # what _prepare_head adds: the heads (proj_t too) and the meta layer


def _unique(names):
    return list(dict.fromkeys(names))


class _Tree(nn.Module):
    """Parameter container with the reference's state_dict keys (no forward of its own)."""

    def __init__(self):
        super().__init__()

    def _leaf(self, dotted, tensor, is_param):
        mod = self
        parts = dotted.split('.')
        for p in parts[:-1]:
            if not hasattr(mod, p):
                mod.add_module(p, _Tree())
            mod = getattr(mod, p)
        if is_param:
            mod.register_parameter(parts[-1], nn.Parameter(tensor))
        else:
            mod.register_buffer(parts[-1], tensor)


def _init_tensor(name, shape):
    """Shape-faithful default init (xavier for the backbone convs with bias 0.01, kaiming fan_out
    for the meta conv, PyTorch defaults for Linear/BatchNorm); real runs restore a checkpoint."""
    if name.endswith('num_batches_tracked'):
        return torch.zeros((), dtype=torch.int64)
    if name.endswith('running_mean'):
        return torch.zeros(shape)
    if name.endswith('running_var'):
        return torch.ones(shape)
    t = torch.empty(shape)
    if len(shape) == 4:
        if 'meta' in name:
            nn.init.kaiming_normal_(t, mode='fan_out', nonlinearity='relu')
        else:
            nn.init.xavier_normal_(t)
    elif len(shape) == 2:
        nn.init.kaiming_uniform_(t, a=math.sqrt(5))
    elif name.endswith('bias'):
        if '.1.' in name and ('proj' in name or 'pred' in name):
            t.zero_()
        elif 'proj' in name or 'pred' in name:
            t.uniform_(-0.04, 0.04)
        else:
            t.fill_(0.01)
    else:
        t.fill_(1.0)
    return t


class _ForwardFn(torch.autograd.Function):
    """(depth, emb, ref) = network(image, sparse); backward -> grads of the adapted parameters."""

    @staticmethod
    def forward(ctx, adapter, image, sparse, *adapted):
        eng = adapter._engine(image)
        depth, emb, ref = eng.forward_train(image, sparse)
        ctx.eng = eng
        ctx.params = dict(zip(eng.adapted, adapted))
        ctx.mark_non_differentiable(emb)
        return depth, emb, ref

    @staticmethod
    def backward(ctx, g_depth, g_emb, g_ref):
        if g_depth is None:
            g_depth = torch.zeros((ctx.eng.n, 1, ctx.eng.h, ctx.eng.w), device=ctx.eng.device)
        grads = ctx.eng.backward_all(g_depth, g_ref, ctx.params)
        return (None, None, None) + tuple(grads)


class _PlainForwardFn(torch.autograd.Function):
    """depth = `_forward`(image, sparse) in training mode on the baseline engine; backward -> gradients of its BatchNorm2d tensors
    (NLSPN: 86, CostDCNet: 30)."""

    @staticmethod
    def forward(ctx, eng, image, sparse, *adapted):
        depth, _, _ = eng.forward_train(image, sparse)
        ctx.eng = eng
        ctx.params = dict(zip(eng.adapted, adapted))
        return depth

    @staticmethod
    def backward(ctx, g_depth):
        return (None, None, None) + tuple(ctx.eng.backward_all(g_depth, None, ctx.params))


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, image, depth, sparse, validity, emb, ref, w_sd, w_sm, w_cos):
        info = eng.loss_forward(image, depth, sparse, validity, emb, ref, w_sd, w_sm, w_cos)
        # the gate and the gradient scalars live on the device until the next loss call
        ctx.eng, ctx.args = eng, (image, depth.detach(), sparse, validity, None if emb is None else emb.detach(),
                                  None if ref is None else ref.detach())
        return info[0].clone(), info

    @staticmethod
    def backward(ctx, g_loss, g_info):
        gd, gr = ctx.eng.loss_backward(*ctx.args)
        gd = gd * g_loss
        if gr is not None:
            gr = gr * g_loss
        return None, None, gd, None, None, None, gr, None, None, None


class _PrepareLossFn(torch.autograd.Function):
    """prepare_loss (src/external_model_adapt.py:524-541) of the last head forward; its backward hands the head parameters
    the gradients ptta_head_backward already produced (parameters outside the graph get None, as in the reference)."""

    @staticmethod
    def forward(ctx, eng, names, *head_params):
        loss = eng.head_backward()
        ctx.grads = [eng.head_grad(k, p) for k, p in zip(names, head_params)]
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g_loss):
        return (None, None) + tuple(None if g is None else g * g_loss for g in ctx.grads)


class _AdapterBase(object):
    """What the per-backbone adapters share: the parameter tree, the per-shape engines and how they are bound, the plain
    (no meta layer) engines of the backbones that have a BatchNorm-adaptation baseline, the stage-2 head trainer and the fused step.
    A backbone states its key table, its Engine keywords (`_new_engine`), its adapted list (`_set_adapted`, `adapt_parameters`)
    and the routing of its `forward`."""

    key_table = None                            # synth.<backbone>_keys: the ordered (key, shape) table of the backbone's state dict
    _init = staticmethod(_init_tensor)
    # whether `reverse` leaves proj without a gradient in stage 2.  NLSPN / CostDCNet: ref = proj_t(...), proj trains in both directions (csrc/ghead.hip)
    heads_reverse_freezes_proj = False
    syncbn_extends_adapted = True               # convert_syncbn: the heads' (and more) BatchNorm join the adapted list, which is rebuilt

    def __init__(self, max_predict_depth, max_input_depth, device, dtype='fp32'):
        self.max_predict_depth = max_predict_depth
        self.max_input_depth = max_input_depth
        self.device = device
        self.dtype = dtype
        self.training = True
        self.prepare_mode = self.meta = None
        # adapted_listed: the reference's parameter list, duplicates included (None: the backbone names no tensor twice); adapted: the tensors behind it
        self.adapted = self.adapted_listed = None
        self.stats_dropped = False        # adapt_parameters('meta_bn') ran: the adapted BatchNorm2d lost their running statistics
        self.model = _Tree()
        for k, s in self._state_keys():
            if not k.startswith(_HEAD_LEAVES):                # heads + meta layer come with _prepare_head
                self.model._leaf(k, self._init(k, s), not k.endswith(_BUFFERS))
        self._engines = {}
        self._opt_state = {}
        self._adam_t = 0              # torch.optim.Adam's state['step'], shared by every per-shape engine
        self._optimizer = None        # bind_optimizer's
        self._never_stepped = set()   # adapted tensors that torch.optim.Adam would leave without a `step` (CostDCNet under SyncBatchNorm)
        self._image_norm = None
        self.sync_bn = False
        self.hparams = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                            w_sparse_depth=1.0, w_smoothness=1.0, w_cos=1.0)
        self.total_time = self.train_time = self.eval_time = 0.0
        # stage 2: set by prepare_parameters / bind_head_optimizer / convert_syncbn / the head calls
        self._head_names = None
        self._head_syncbn = False
        self._head_hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, tau=0.999)
        self._head_opt = None
        self._head_state = {}
        self._head_t = 0
        self._head_mode = self._head_last = None
        self.to(device)

    def _state_keys(self):
        """(key, shape) of this backbone's tensors under the model's prepare mode (never prepared: the table's default, the 1layer one)."""
        return self.key_table(self.prepare_mode) if self.prepare_mode else self.key_table()

    def _clear_engines(self):
        """Release every per-shape engine (workspaces are GBs at full size: do not wait for __del__)."""
        engines, self._engines = self._engines, {}
        for eng in engines.values():
            eng.close()

    def _drop_plain_engines(self):
        for key in [k for k in self._engines if k[0] == 'plain']:
            self._engines.pop(key).close()

    def _timed(self, fn, loss_type):
        """The reference's wall-clock hook: `'time' in loss_type` brackets the network forward with
        torch.cuda.synchronize() + time.time() and accumulates train_time / eval_time / total_time
        (network_exp_msg_chn_adapt.py:338-340,407-414); read back by forward(loss_type='get_time')."""
        if 'time' not in loss_type:
            return fn()
        import time
        torch.cuda.synchronize()
        t0 = time.time()
        out = fn()
        torch.cuda.synchronize()
        dt = time.time() - t0
        if self.training:
            self.train_time += dt
        else:
            self.eval_time += dt
        self.total_time += dt
        return out

    # ---- reference surface -----------------------------------------------------------------
    def _prepare_head(self, mode=''):
        """The network's _prepare_head (network_exp_msg_chn_adapt.py:1022-1087, nlspnmodel_adapt.py:1333-1396, CostDCNet_adapt.py:426-496):
        proj / proj_t / pred and the meta layer join the tree, the adapted list is the new mode's, the engines made so far are released."""
        if 'meta' not in mode or 'selfsup' not in mode or 'ema' not in mode or 'seq' not in mode or \
                ('1layer' not in mode and '2layers' not in mode):
            raise NotImplementedError('hot path covers prepare_mode meta_selfsup_seq_{1layer,2layers}_ema, got %r' % mode)
        self.prepare_mode = mode
        self.meta = '2layers' if '2layers' in mode else '1layer'
        for k, s in self._state_keys():
            if k.startswith(_HEAD_LEAVES):
                self.model._leaf(k, self._init(k, s).to(self.device), not k.endswith(_BUFFERS))
        self._set_adapted()

    def parameters(self):
        return list(self.model.parameters())

    def _select_baseline(self, listed):
        """adapt_parameters('meta_bn') on a model whose head was never prepared, the BatchNorm-adaptation baseline: no parameter is called 'meta'
        yet, so the list is gamma / beta of the backbone's BatchNorm2d alone; forward / step / compute_loss then run on the engine without
        the meta layer (`_plain_engine`)."""
        if self.sync_bn:
            raise NotImplementedError('the BatchNorm-adaptation baseline runs on one rank (no SyncBatchNorm form)')
        self.adapted_listed, self.adapted = listed, list(listed)
        self.stats_dropped = True
        self._clear_engines()

    def _listed_parameters(self):
        params = dict(self.model.named_parameters())
        return nn.ParameterList([params[k] for k in self.adapted_listed])

    # ---- stage 2 (src/head_main.py:259-276, 464-480) ------------------------------------------------------
    def prepare_parameters(self, mode=''):
        """mode containing 'head' (head_main.py:268 passes 'head_selfsup_ema'): the heads are RE-CREATED -- the reference calls
        `_prepare_head(mode)` again here (src/msg_chn_model_adapt.py:295-298), stage 2 trains them from scratch -- and the
        proj / pred parameters without proj_t are returned (:300-304)."""
        if 'head' not in mode or 'selfsup' not in mode or 'ema' not in mode:
            raise NotImplementedError("prepare_parameters(%r): only the head trainer's 'head_selfsup_ema' is on the accelerated path" % mode)
        if self.prepare_mode is None:
            raise RuntimeError('_prepare_head(prepare_mode) first (head_main.py:259)')
        params = dict(self.model.named_parameters())
        with torch.no_grad():
            for k, shape in self._state_keys():
                if k.startswith(('proj.', 'pred.')):
                    t = params.get(k, None)
                    tgt = t if t is not None else self.model.state_dict()[k]
                    tgt.copy_(_init_tensor(k, shape).to(tgt.device))
            state = self.model.state_dict()
            for k in state:
                if k.startswith('proj_t.'):
                    state[k].copy_(state['proj.' + k[len('proj_t.'):]])          # copy.deepcopy(self.proj)
        self._clear_engines()
        self._head_names = [k for k, _ in self.model.named_parameters() if ('proj' in k or 'pred' in k) and '_t' not in k]
        return [params[k] for k in self._head_names]

    def bind_head_optimizer(self, optimizer, tau=0.999):
        """Share Adam state with a torch.optim.Adam built on prepare_parameters(): `head_step` then updates its exp_avg /
        exp_avg_sq / step in place, so optimizer.state_dict() (save_model) stays meaningful."""
        params = dict(self.model.named_parameters())
        g = optimizer.param_groups[0]
        self._head_hp = dict(lr=g['lr'], betas=tuple(g['betas']), eps=g['eps'], weight_decay=g['weight_decay'], tau=tau)
        self._head_opt = optimizer
        self._head_state = {}
        t = 0
        for k in self._head_names:
            st = optimizer.state[params[k]]
            if 'exp_avg' not in st:
                st['step'] = torch.tensor(0.0)
                st['exp_avg'] = torch.zeros_like(params[k].data)
                st['exp_avg_sq'] = torch.zeros_like(params[k].data)
            self._head_state[k] = st
            t = max(t, int(float(st['step'])))
        self._head_t = t
        self._clear_engines()

    def _head_engine(self, image):
        eng = self._engine(image)
        if not eng._heads_bound:
            if self._head_names is None:
                raise RuntimeError('prepare_parameters(\'head_selfsup_ema\') must be called before a head forward (head_main.py:268)')
            if self._head_syncbn:
                eng.set_head_form(_lib.PTTA_HEAD_FORM_SYNCBN)
            params = dict(self.model.named_parameters())
            for k in self._head_names:
                st = self._head_state.get(k) or {'exp_avg': torch.zeros_like(params[k].data), 'exp_avg_sq': torch.zeros_like(params[k].data)}
                self._head_state[k] = st
                eng.bind_head(k, params[k].data, st['exp_avg'], st['exp_avg_sq'])
            for k in HEAD_TARGETS:
                eng.bind_head(k, params[k].data)
            eng.set_head_hparams(adam_step=self._head_t, **self._head_hp)
            eng._head_t = self._head_t
            if self._head_syncbn:
                eng.enable_stat_sync()          # after the binds: its buffer holds the head gradients too (no-op with one rank)
            eng._heads_bound = True
        return eng

    def _sync_head_step(self, eng):
        """Counterpart of _sync_adam_step for the stage-2 heads: every (batch, height, width) engine has its own device-side
        step count, torch.optim.Adam has ONE `step` per parameter -- a second engine (the last short batch of a loader) must
        continue the bias correction where the first one stands."""
        if eng._head_t != self._head_t:
            eng.set_head_hparams(adam_step=self._head_t, **self._head_hp)
            eng._head_t = self._head_t

    def head_forward(self, image, sparse_depth, loss_type):
        """forward(loss_type='head_selfsup_seq_ema[_reverse]') in training mode: (None, embedding, reference)
        (network_exp_msg_chn_adapt.py:610-699); the EMA of proj_t runs first (:682,:691)."""
        if not self.training:
            raise NotImplementedError('the head forward is a training-mode call (head_main.py:441)')
        if 'ema' not in loss_type or 'adapt' in loss_type:
            raise NotImplementedError('loss_type %r is not on the accelerated path' % loss_type)
        eng = self._head_engine(image)
        eng.head_reload()                 # a torch optimizer may have stepped the bound parameters since the last call
        emb, ref = eng.head_forward(image, sparse_depth, 'reverse' in loss_type)
        self._head_last = eng
        return None, emb, ref

    def prepare_loss(self, embedding, reference):
        """compute_loss(loss_type='prepare'): the loss of the LAST head forward (embedding / reference are its outputs)."""
        eng = self._head_last
        if eng is None:
            raise RuntimeError('compute_loss(loss_type=\'prepare\') follows a head forward')
        params = dict(self.model.named_parameters())
        loss = _PrepareLossFn.apply(eng, tuple(self._head_names), *[params[k] for k in self._head_names])
        return loss, {'loss': loss}

    def head_step(self, image, sparse_depth, loss_type):
        """Fused stage-2 step (head_main.py:464-480): EMA, forward, prepare loss, backward, Adam -- one library call."""
        eng = self._head_engine(image)
        # the library keeps ONE step count for the head tensors, torch.optim.Adam one per parameter: in `reverse` mode only
        # `pred` steps, so a run that switches between the two loss types would give proj pred's count -> refused
        rev = 'reverse' in loss_type
        if self.heads_reverse_freezes_proj and self._head_mode not in (None, rev) and self._head_t > 0:
            raise NotImplementedError('head_step: switching between reverse and non-reverse loss types inside one run is not supported '
                                      '(per-parameter Adam step counts would diverge)')
        self._head_mode = rev
        self._sync_head_step(eng)
        loss = eng.head_step(image, sparse_depth, rev)
        self._head_t += 1
        eng._head_t = self._head_t
        live = self._head_names if (not rev or not self.heads_reverse_freezes_proj) else [k for k in self._head_names if k.startswith('pred')]
        for k in live:
            st = self._head_state[k]
            if 'step' in st:
                st['step'] += 1
        return loss

    def train(self):
        self.training = True
        self.model.train()

    train_prepare = train
    train_meta = train

    def eval(self):
        self.training = False
        self.model.eval()

    def to(self, device):
        self.device = device
        self.model.to(device)
        self._clear_engines()

    def data_parallel(self):
        raise NotImplementedError('one process per GPU; use proxytta.distributed')

    def distributed_data_parallel(self, rank):
        """The reference wraps in DDP (msg_chn_model_adapt.py:476-480) and all-reduces every
        gradient; here only the adapted-parameter gradients are reduced: drive the step through
        proxytta.distributed.shared_parameter_step (one flat all-reduce), not through loss.backward()."""
        self.ddp_rank = rank

    def convert_syncbn(self, apex=False):
        """SyncBatchNorm.convert_sync_batchnorm (msg_chn_model_adapt.py:547-556, costdcnet_model_adapt.py:535-546): from now on train-mode
        BatchNorm statistics are those of the GLOBAL batch.  With one rank that is what the engine computes anyway; with
        several ranks the statistics are exchanged inside proxytta.distributed.shared_parameter_step.
        NLSPN / CostDCNet: the reference converts BEFORE adapt_parameters('meta_bn') (src/tta_main.py:326,339), so every BatchNorm of the
        model passes its isinstance test from here on: the adapted list grows (nlspn_adapted_names / costdcnet_adapted_names, syncbn) and the
        engines made afterwards are the library's PTTA_SYNCBN_ADAPT ones.
        After prepare_parameters('head_selfsup_ema') this is stage 2 (src/head_main.py:268, then :278): the head engines take the
        SyncBatchNorm form (include/ptta.h ptta_head_set_form) and the TTA adapted list stays what it is."""
        if self._head_names is not None:
            self._head_syncbn = True
            self._clear_engines()
            return
        self.sync_bn = True
        for key, eng in self._engines.items():
            if key[0] != 'source':                  # (MSG_CHN's `_forward` has no BatchNorm: the source engine stays what it is)
                eng.enable_stat_sync()
        if self.syncbn_extends_adapted and self.prepare_mode is not None:
            self._set_adapted()                     # heads exist: the list of the DDP run, for the engines made from here on

    def restore_model(self, restore_path, optimizer=None):
        ckpt = torch.load(restore_path, map_location=self.device)
        self.load_state_dict(ckpt['net'])
        if optimizer is not None and 'optimizer' in ckpt:
            optimizer.load_state_dict(ckpt['optimizer'])
            if self._optimizer is optimizer:
                self.bind_optimizer(optimizer)      # load_state_dict REPLACED exp_avg / exp_avg_sq / step: rebind them
        return optimizer, ckpt.get('train_step', 0)

    def save_model(self, checkpoint_path, step, optimizer, meanvar=None):
        torch.save({'net': self.model.state_dict(), 'optimizer': optimizer.state_dict() if optimizer else {},
                    'train_step': step}, checkpoint_path)

    def load_state_dict(self, state):
        with torch.no_grad():
            own = self.model.state_dict()
            missing = [k for k in own if k not in state]
            if missing:
                raise KeyError('missing keys: %s' % missing[:5])
            for k, v in own.items():
                v.copy_(torch.as_tensor(state[k]).to(v.device))
        for eng in self._engines.values():
            eng.load_state_dict(self.model.state_dict())

    # ---- engine plumbing --------------------------------------------------------------------
    def _bind_engine(self, key, eng, state, names=None):
        """A new engine takes up this model: `state` loaded (BatchNorm buffers are bound by pointer and updated in place), the parameters
        `names` bound with their Adam moments -- one pair per tensor, shared by every engine of the model -- then the image normalisation,
        the Adam step count and the SyncBatchNorm exchange, and the engine is kept under `key`.  names None: an engine that adapts nothing
        (MSG_CHN's source model), which has no step count to carry and no batch statistics to exchange."""
        eng.load_state_dict(state)
        if names is not None:
            params = dict(self.model.named_parameters())
            for name in names:
                p = params[name]
                st = self._opt_state.setdefault(name, {'exp_avg': torch.zeros_like(p.data), 'exp_avg_sq': torch.zeros_like(p.data)})
                eng.bind_adapted(name, p.data, st['exp_avg'], st['exp_avg_sq'])
        if self._image_norm is not None:
            eng.set_image_norm(self._image_norm)
        if names is not None:
            eng._t = 0
            eng._heads_bound = False
            if self.sync_bn:
                eng.enable_stat_sync()          # no-op with one rank
        self._engines[key] = eng
        return eng

    def _engine(self, image):
        n, _, h, w = image.shape
        key = (n, h, w)
        eng = self._engines.get(key)
        if eng is None:
            if self.prepare_mode is None:
                if self.stats_dropped:             # the baseline model: its only engine is the one without the meta layer
                    return self._plain_engine(image)
                raise RuntimeError('_prepare_head(mode) must be called before forward (tta_main.py:322)')
            eng = self._new_engine(n, h, w)
            if self.adapted_listed is not None:
                assert all(self.adapted_listed.count(k) == max(eng.adapted_repeat[k], 1) for k in eng.adapted), 'listing counts drifted'
                assert eng.adapted == self.adapted, 'adapted parameter list drifted from the library'
            self._bind_engine(key, eng, self.model.state_dict(), self.adapted)
        return eng

    def _plain_engine(self, image):
        """The engine of `_forward`, the network without the meta layer (NLSPN, CostDCNet): the baseline kind once adapt_parameters('meta_bn')
        dropped the running statistics (batch statistics, gamma / beta of the BatchNorm2d bound to this model's parameters), the source kind
        before (every BatchNorm from the loaded running statistics, eval forward only).  One per shape, beside the ProxyTTA engines; the
        meta layer and the heads of a prepared model are not part of it."""
        if self.sync_bn:
            raise NotImplementedError("the network without the meta layer runs on one rank (no SyncBatchNorm form of loss_type 'pretrain')")
        n, _, h, w = image.shape
        key = ('plain', n, h, w)
        eng = self._engines.get(key)
        if eng is None:
            eng = self._new_engine(n, h, w, plain_mode='meta_bn' if self.stats_dropped else 'meta')
            # the source model adapts nothing; the baseline every BatchNorm2d tensor of this model's list, none twice
            want = [k for k in self.adapted if 'meta' not in k] if self.stats_dropped else []
            assert eng.adapted == want and all(eng.adapted_repeat[k] == 1 for k in want), 'adapted parameter list drifted from the library'
            self._bind_engine(key, eng, self._plain_state(), want)
        return eng

    def _plain_state(self):
        """The state a plain engine loads."""
        return self.model.state_dict()

    def _sync_adam_step(self, eng):
        """Every (batch, height, width) has its own engine and device-side step counter; torch.optim.Adam has ONE
        `step` per parameter, so the bias correction must continue across shape changes (last short batch of a
        loader with drop_last=False, src/tta_main.py:281)."""
        if eng._t != self._adam_t:
            eng.set_adam_step(self._adam_t)
            eng._t = self._adam_t

    def set_image_norm(self, normalized_image_range):
        """Take RAW images from now on: Transforms.normalize_images (src/transforms.py:668-710, called at
        src/tta_main.py:454-464,652) is fused into the first convolution's loads.  The loss keeps seeing the
        raw image, as in the reference (tta_main.py:610 vs :620)."""
        from .engine import image_norm_constants
        image_norm_constants(normalized_image_range)        # validate now (raises ValueError like the reference)
        self._image_norm = normalized_image_range
        for eng in self._engines.values():
            eng.set_image_norm(normalized_image_range)

    def set_hparams(self, **kw):
        self.hparams.update({k: v for k, v in kw.items() if k in self.hparams})
        if 'max_input_depth' in kw:
            self.max_input_depth = kw['max_input_depth']
        for eng in self._engines.values():
            eng.set_hparams(**kw)

    def bind_optimizer(self, optimizer):
        """Share Adam state with a torch.optim.Adam built on adapt_parameters(): its exp_avg /
        exp_avg_sq tensors become the buffers the fused step updates, so optimizer.state_dict()
        (save_model) stays meaningful."""
        params = dict(self.model.named_parameters())
        g = optimizer.param_groups[0]
        self.set_hparams(lr=g['lr'], betas=tuple(g['betas']), eps=g['eps'], weight_decay=g['weight_decay'])
        for name in self.adapted:
            p = params[name]
            st = optimizer.state[p]
            if 'exp_avg' not in st:
                st['step'] = torch.tensor(0.0)
                st['exp_avg'] = torch.zeros_like(p.data)
                st['exp_avg_sq'] = torch.zeros_like(p.data)
            self._opt_state[name] = st
        # the library keeps ONE count of optimizer.step() calls; a tensor the list names twice shows twice that in torch's state
        self._adam_t = int(float(optimizer.state[params[self.adapted[0]]]['step']))
        self._clear_engines()
        self._optimizer = optimizer

    # ---- forward / loss -----------------------------------------------------------------------
    def _forward_tta(self, image, sparse_depth, loss_type):
        """The ProxyTTA network.  Training mode with 'adapt' in the string: (depth, emb, ref) with autograd edges to the adapted tensors --
        loss.backward() runs ptta_loss_backward + ptta_backward and fills their .grad (src/tta_main.py:610-632).  Otherwise the eval forward."""
        if self.training and 'adapt' in loss_type:
            params = dict(self.model.named_parameters())
            return self._timed(lambda: _ForwardFn.apply(self, image, sparse_depth, *[params[k] for k in self.adapted]), loss_type)
        with torch.no_grad():
            out = self._timed(lambda: self._engine(image).forward_eval(image, sparse_depth), loss_type)
        return self._fill(out, loss_type)

    def _forward_plain(self, image, sparse_depth, loss_type):
        """`_forward`, the network without the meta layer (nlspnmodel_adapt.py:792-848, CostDCNet_adapt.py:177-205).  Eval: the depth.  Training
        with 'bn' in the string: (depth, None, None) with autograd edges to the BatchNorm2d tensors of the baseline.  Training without 'bn':
        the reference returns a tensor with autograd into EVERY parameter, which is not on the accelerated path."""
        if self.training:
            if 'bn' not in loss_type:
                raise NotImplementedError("loss_type %r in training mode: autograd into every parameter is not on the accelerated path "
                                          "('bn' in the string: the BatchNorm-adaptation baseline)" % loss_type)
            self._require_baseline(loss_type)
            eng = self._plain_engine(image)
            params = dict(self.model.named_parameters())
            depth = self._timed(lambda: _PlainForwardFn.apply(eng, image, sparse_depth, *[params[k] for k in eng.adapted]), loss_type)
            return depth, None, None
        with torch.no_grad():
            out = self._timed(lambda: self._plain_engine(image).forward_eval(image, sparse_depth), loss_type)
        return self._fill(out, loss_type)

    def _fill(self, out, loss_type):
        """What a backbone does to its eval output on the host (NLSPN fills holes)."""
        return out

    def step(self, image, sparse_depth, validity_map=None, loss_image=None, want_depth=False, next_frame=None):
        """The fused step.  next_frame = (image, sparse_depth) of the frame the NEXT call will pass (the data loader's look-ahead): the part of
        its forward upstream of the adapted layer then runs beside this step (Engine.step / ptta_step_pipelined); same results."""
        eng = self._engine(image)
        self._sync_adam_step(eng)
        if next_frame is not None and (eng.backbone != 'msg_chn' or tuple(next_frame[0].shape) != tuple(image.shape)):
            next_frame = None                       # other backbones have nothing upstream of their adapted layers; a new shape is a new engine
        info, depth = eng.step(image, sparse_depth, validity_map, loss_image, want_depth, **({'next_frame': next_frame} if next_frame is not None else {}))
        self._adam_t += 1
        eng._t = self._adam_t
        opt = self._optimizer
        if opt is not None:
            never = self._never_stepped
            skip = {id(p) for k, p in self.model.named_parameters() if k in never} if never else ()
            for p in opt.param_groups[0]['params']:             # as listed: a tensor named twice is stepped twice
                if 'step' in opt.state[p] and id(p) not in skip:
                    opt.state[p]['step'] += 1
        return info, depth


class MsgChnModel_Adapt(_AdapterBase):
    """Counterpart of src/msg_chn_model_adapt.py:11-556 on libptta_hip."""

    key_table = staticmethod(synth.msg_chn_keys)
    heads_reverse_freezes_proj = True           # stage 2: the reference branch of `reverse` is proj itself (network_exp_msg_chn_adapt.py:691-694)
    syncbn_extends_adapted = False              # the adapted list is the meta layer, whatever the BatchNorm modules are: the engines stay

    def __init__(self, max_predict_depth=5.0, inpainting=False, device=torch.device('cuda'), dtype='fp32',
                 max_input_depth=None):
        super().__init__(max_predict_depth, max_input_depth, device, dtype)

    def _prepare_head(self, mode=''):
        if 'meta' not in mode or 'selfsup' not in mode or 'ema' not in mode or 'seq' not in mode:
            raise NotImplementedError('hot path covers prepare_mode meta_selfsup_seq_{1layer}_ema, got %r' % mode)
        if '1layer' not in mode and '2layers' not in mode:
            raise NotImplementedError('meta layer of %r is not on the accelerated path (1layer / 2layers are)' % mode)
        super()._prepare_head(mode)

    def _set_adapted(self):
        self.adapted = adapted_names(self.meta)
        self._clear_engines()

    def adapt_parameters(self, mode=None):
        """mode 'meta': every parameter whose name contains 'meta' (msg_chn_model_adapt.py:392-396)."""
        if mode != 'meta':
            raise NotImplementedError("adapt_mode %r: only 'meta' is on the accelerated path" % mode)
        return nn.ParameterList([p for n, p in self.model.named_parameters() if 'meta' in n])

    def _new_engine(self, n, h, w, plain_mode=None):
        """plain_mode: the source engine, always fp32 (the scored forward of the mixed mode is the fp32 one already)."""
        return Engine(n, h, w, dtype='fp32' if plain_mode else self.dtype, max_input_depth=self.max_input_depth,
                      meta='plain' if plain_mode else self.meta, **self.hparams)

    def _source_engine(self, image):
        """The engine of `network._forward` (network_exp_msg_chn_adapt.py:418-461), the loaded checkpoint without the meta layer, the zero-image
        pass and the heads (include/ptta.h PTTA_MSGCHN_PLAIN): built from this model's backbone tensors beside the ProxyTTA engines, on a
        model that was never prepared too.  Nothing adapts, so it holds no bound parameter: load_state_dict reloads it, _clear_engines drops
        it with the others."""
        n, _, h, w = image.shape
        key = ('source', n, h, w)
        eng = self._engines.get(key)
        if eng is None:
            eng = self._new_engine(n, h, w, plain_mode='meta')
            assert eng.adapted == [] and eng.rows == 0, 'the source handle adapts nothing and has no heads'
            self._bind_engine(key, eng, self.model.state_dict())  # conv1_rgb_meta.*, proj*, pred* of a prepared model: accepted and ignored
        return eng

    def forward(self, image, sparse_depth, intrinsics=None, crop_mask=None, loss_type='pretrain'):
        """network.forward's branches in its own order (network_exp_msg_chn_adapt.py:342-403): 'prepare', 'init_meta', 'head',
        'meta' + 'selfsup', then 'pretrain' in the string -- `_forward`, the source model, on a prepared model too."""
        if loss_type == 'prepare' or 'init_meta' in loss_type:
            raise NotImplementedError('loss_type %r (the stage-1 meta-layer trainer) is not on the accelerated path' % loss_type)
        if 'head' in loss_type:
            return self.head_forward(image, sparse_depth, loss_type)
        if 'meta' in loss_type and 'selfsup' in loss_type:
            return self._forward_tta(image, sparse_depth, loss_type)
        if 'pretrain' not in loss_type:             # the reference leaves `output` unbound here and raises at its return
            raise NotImplementedError('loss_type %r matches no branch of the network\'s forward' % loss_type)
        if self.training:
            # the reference returns three scales with autograd into EVERY parameter of the network
            raise NotImplementedError("loss_type %r in training mode: autograd into every parameter is not on the accelerated path "
                                      "(eval mode runs the source model)" % loss_type)
        with torch.no_grad():                       # output_d11, the scale the eval wrapper returns (src/msg_chn_model_adapt.py:179-181)
            return self._timed(lambda: self._source_engine(image).forward_eval(image, sparse_depth), loss_type)


def eng_is_padded(eng):
    """Frame sizes not divisible by 16 run the dual-corner padding and the plain step (no pipelining state to reuse)."""
    return (eng.h % 16) != 0 or (eng.w % 16) != 0


class ExternalModel_Adapt(object):
    """Counterpart of src/external_model_adapt.py:29 (model_name 'msg_chn', 'nlspn', 'costdcnet')."""

    def __init__(self, model_name, min_predict_depth, max_predict_depth, max_input_depth=None, offset=False,
                 from_scratch=False, dataset_name=None, device=torch.device('cuda'), dtype='fp32'):
        self.model_name = model_name
        self.dataset_name = dataset_name
        self.device = device
        self.max_predict_depth = max_predict_depth
        self.max_input_depth = max_input_depth
        if model_name == 'msg_chn':
            self.model = MsgChnModel_Adapt(device=device, max_predict_depth=max_predict_depth, dtype=dtype,
                                           max_input_depth=max_input_depth)
        elif model_name == 'nlspn':
            from .nlspn import NlspnModel_Adapt
            self.model = NlspnModel_Adapt(device=device, max_depth=max_predict_depth, offset=offset, dataset_name=dataset_name,
                                          from_scratch=from_scratch, max_input_depth=max_input_depth)
        elif 'costdcnet' in model_name:
            from .costdcnet import CostDCNetModel_Adapt
            self.model = CostDCNetModel_Adapt(device=device, max_depth=max_predict_depth, max_input_depth=max_input_depth)
        else:
            raise ValueError('Unsupported depth completion model: {}'.format(model_name))

    def forward(self, image, sparse_depth, crop_mask=None, intrinsics=None, loss_type='pretrain'):
        if loss_type == 'get_time':
            m = self.model
            return [m.total_time, m.train_time, m.eval_time]
        # the clamp of external_model_adapt.py:108 happens inside the library (prep kernel)
        return self.model.forward(image=image, sparse_depth=sparse_depth, intrinsics=intrinsics,
                                  crop_mask=crop_mask, loss_type=loss_type)

    def compute_loss(self, input_rgb=None, output_depth=None, sparse_depth=None, validity_map=None,
                     embedding=None, reference=None, w_loss_sparse_depth=1.0, w_loss_smoothness=1.0,
                     w_loss_cos=1.0, loss_type='adapt', **unused):
        if 'prepare' in loss_type:                  # src/external_model_adapt.py:155-158
            return self.model.prepare_loss(embedding, reference)
        if 'adapt' not in loss_type:
            raise NotImplementedError('loss_type %r is not on the accelerated path' % loss_type)
        eng = self.model._engine(input_rgb)
        loss, info = _LossFn.apply(eng, input_rgb, output_depth, sparse_depth, validity_map, embedding, reference,
                                   w_loss_sparse_depth, w_loss_smoothness, w_loss_cos)
        info = info.detach()
        return loss, {'loss': loss, 'loss_smooth': info[1], 'loss_sparse_depth': info[2], 'loss_cos': info[3]}

    def _prepare_head(self, mode=''):
        self.model._prepare_head(mode=mode)

    def parameters(self):
        return self.model.parameters()

    def adapt_parameters(self, mode=''):
        return self.model.adapt_parameters(mode=mode)

    def prepare_parameters(self, mode=''):
        return self.model.prepare_parameters(mode)

    def bind_head_optimizer(self, optimizer, tau=0.999):
        self.model.bind_head_optimizer(optimizer, tau)

    def head_step(self, image, sparse_depth, loss_type='head_selfsup_seq_ema_reverse'):
        """One stage-2 training step (src/head_main.py:464-480) in one library call; returns the loss (1 device float)."""
        return self.model.head_step(image, sparse_depth, loss_type)

    def train(self, meta=False, prepare=False):
        self.model.train()

    def eval(self):
        self.model.eval()

    def to(self, device):
        self.device = device
        self.model.to(device)

    def data_parallel(self):
        self.model.data_parallel()

    def distributed_data_parallel(self, rank):
        self.model.distributed_data_parallel(rank)

    def restore_model(self, restore_path, optimizer=None, learning_schedule=None, learning_rates=None,
                      n_step_per_epoch=None):
        return self.model.restore_model(restore_path=restore_path, optimizer=optimizer)

    def save_model(self, checkpoint_path, step, optimizer, meanvar=None):
        self.model.save_model(checkpoint_path, step, optimizer, meanvar)

    def convert_syncbn(self, apex=False):
        self.model.convert_syncbn(apex)

    def log_summary(self, summary_writer, tag, step, image=None, output_image=None, sparse_depth=None, output_depth=None,
                    validity_map=None, ground_truth=None, normalized_image_range=None, scalars={}, n_image_per_summary=4,
                    image_dtype='float32'):
        """src/external_model_adapt.py:662-909, keyword for keyword, with the panels composed on the device (proxytta.summary, csrc/summary.hip).
        summary_writer is anything with add_image, add_histogram and add_scalar.  image: an N x 3 x H x W tensor or a list of them; the maps
        N x 1 x H x W; host tensors are uploaded (the driver moves them to the CPU in front of the call, src/tta_main.py:637-640).  The
        calls, tags, order and global_step are the reference's: add_histogram per depth map with the tensor as given, add_scalar per
        entry of `scalars` (device scalars are fetched with ONE stacked copy), add_image with the image grid (tag + '_image') and with
        the depth grid (tag + '_image_output_sparse-error_groundtruth-error' and its shorter forms).  Each grid arrives as a CPU tensor
        after one device -> host copy: bit for bit the reference's 3 x GH x GW fp32 grid, or with image_dtype='uint8' the GH x GW x 3
        uint8 image the writer would make of it, passed with dataformats='HWC' (a quarter of the bytes, the same PNG).
        normalized_image_range=None means "no display transform"; the reference raises TypeError on None[0] there.  output_image is
        not built (no driver passes it and the reference's branch swaps mean and std): anything but None raises NotImplementedError."""
        from . import summary
        if output_image is not None:
            raise NotImplementedError('log_summary(output_image=...) is not built: no driver passes it and the reference normalises it with '
                                      'mean and std swapped (src/external_model_adapt.py:780-783)')
        if image_dtype not in ('float32', 'uint8'):
            raise ValueError("image_dtype is 'float32' or 'uint8'")
        device = self.device if torch.device(self.device).type == 'cuda' else torch.device('cuda')

        def resident(t):
            return None if t is None else t.detach().to(device=device, dtype=torch.float32).contiguous()
        with torch.no_grad():
            images = [] if image is None else [resident(t) for t in (image if isinstance(image, list) else [image])]
            out_d, sparse_d, valid_d, gt_d = (resident(t) for t in (output_depth, sparse_depth, validity_map, ground_truth))
            depth_text = tag + ('_image' if images else '')
            if output_depth is not None:
                depth_text += '_output'
                summary_writer.add_histogram(tag + '_output_depth_distro', output_depth, global_step=step)
                if sparse_depth is not None and validity_map is not None:
                    depth_text += '_sparse-error'
                    summary_writer.add_histogram(tag + '_sparse_depth_distro', sparse_depth, global_step=step)
                if ground_truth is not None:
                    depth_text += '_groundtruth-error'
                    summary_writer.add_histogram(tag + '_ground_truth_distro', ground_truth, global_step=step)
            on_device = [k for k, v in scalars.items() if torch.is_tensor(v) and v.is_cuda]
            fetched = dict(zip(on_device, torch.stack([scalars[k].detach().reshape(()).double() for k in on_device]).cpu().tolist())) if on_device else {}
            for name, value in scalars.items():
                summary_writer.add_scalar(tag + '_' + name, fetched.get(name, value), global_step=step)
            kw = dict(max_predict_depth=self.max_predict_depth, normalized_image_range=normalized_image_range,
                      n_image_per_summary=n_image_per_summary, image_dtype=image_dtype)
            extra = dict(dataformats='HWC') if image_dtype == 'uint8' else {}
            flags = [summary.image_flag(t) for t in images]
            if images:
                grid = summary.compose_grid(image=images, image_flags=flags, **kw)
                summary_writer.add_image(tag + '_image', summary.to_host(grid), global_step=step, **extra)
            if images or output_depth is not None:
                grid = summary.compose_grid(image=images[-1:], image_flags=flags[-1:], output_depth=out_d, sparse_depth=sparse_d,
                                            validity_map=valid_d, ground_truth=gt_d, **kw)
                summary_writer.add_image(depth_text, summary.to_host(grid), global_step=step, **extra)

    # ---- fused entry points -----------------------------------------------------------------
    def set_image_norm(self, normalized_image_range):
        self.model.set_image_norm(normalized_image_range)

    def step(self, image, sparse_depth, validity_map=None, loss_image=None, want_depth=False, next_frame=None):
        """One TTA step (src/tta_main.py:610-633) in one library call; returns (loss_info[4], depth).  next_frame: see the adapter's step."""
        return self.model.step(image, sparse_depth, validity_map, loss_image, want_depth, next_frame=next_frame)

    def adapt(self, image, sparse_depth, inner_iter=1, validity_map=None, loss_image=None, next_frame=None, ground_truth=None, score=None,
              sink=None, sink_paths=None, augmenter=None, augmentation_probability=0.0, generator=None):
        """Per-frame adaptation = inner_iter steps then the scored eval forward
        (src/tta_main.py:579-636 and :729-736).  Returns (depth, loss_info of the last step).
        augmenter (a proxytta.augment.StepAugmenter): the reference's operating mode (src/tta_main.py:581-633).  Every one of the inner_iter
        iterations starts from the frame AS PASSED, draws a fresh geometric and photometric transform at augmentation_probability (from
        `generator`, or torch's global one, and numpy's global state), and steps on the jittered image with the geometrically transformed
        one as the loss image and the transformed sparse depth / validity map.  The scored forward, score and sink see the frame as passed.
        Not together with loss_image (the augmenter makes it) or next_frame (see the message).
        next_frame = (image, sparse_depth) the next call will pass: announced to the LAST step of this frame (frame pipelining).
        ground_truth and score (a proxytta.score.RunScore), given together: score.update(depth, ground_truth) is enqueued behind the scored
        forward on the same stream (src/tta_main.py:769-798 without its copy to the host); the return value is the same.
        sink (a proxytta.sink.RawFrameSink): sink.submit(depth=depth, paths=sink_paths) is enqueued behind the scored forward (behind the
        score's update when there is one): the prediction leaves as the 16-bit map save_depth stores; the return value is the same."""
        if (ground_truth is None) != (score is None):
            raise ValueError('adapt: ground_truth and score are given together or not at all')
        if augmenter is not None:
            if loss_image is not None:
                raise ValueError('adapt: loss_image and augmenter are not given together: the augmenter makes the loss image (the geometrically '
                                 'transformed, not jittered frame)')
            if next_frame is not None:
                raise ValueError('adapt: next_frame and augmenter are not given together: the look-ahead prefix would be computed on the frame as '
                                 'announced, and the next call replaces that frame by its augmented form before it steps')
            depth, info = self._adapt_augmented(image, sparse_depth, inner_iter, validity_map, augmenter, augmentation_probability, generator)
        else:
            depth, info = self._adapt(image, sparse_depth, inner_iter, validity_map, loss_image, next_frame)
        if score is not None:
            score.update(depth, ground_truth)
        if sink is not None:
            sink.submit(depth=depth, paths=sink_paths)
        return depth, info

    def _adapt(self, image, sparse_depth, inner_iter, validity_map, loss_image, next_frame):
        info = None
        self.model.train()
        piped = False
        for it in range(inner_iter):
            if it == inner_iter - 1 and next_frame is not None:
                info, _ = self.step(image, sparse_depth, validity_map, loss_image, next_frame=next_frame)
                piped = type(self.model) is MsgChnModel_Adapt and tuple(next_frame[0].shape) == tuple(image.shape)
                continue
            info, _ = self.model.step(image, sparse_depth, validity_map, loss_image)
        self.model.eval()
        if piped:                    # the scored forward from the adapted frame's own prefix (ptta_forward_eval_last)
            eng = self.model._engine(image)
            if getattr(eng.lib, 'ptta_forward_eval_last', None) is not None and not eng_is_padded(eng):
                return eng.forward_eval_last(), info
        depth = self.model.forward(image, sparse_depth, loss_type=CANONICAL_LOSS_TYPE)
        return depth, info

    def _adapt_augmented(self, image, sparse_depth, inner_iter, validity_map, augmenter, probability, generator):
        info = None
        self.model.train()
        n, _, h, w = image.shape
        for _ in range(inner_iter):                 # each iteration from the originals (src/tta_main.py:581 re-unpacks `inputs`)
            augmenter.draw(n, h, w, probability, generator)
            image1, loss_image, sparse1, validity1, _gt = augmenter.apply(image, sparse_depth, validity_map)
            info, _ = self.model.step(image1, sparse1, validity1, loss_image)
        self.model.eval()
        depth = self.model.forward(image, sparse_depth, loss_type=CANONICAL_LOSS_TYPE)
        return depth, info


ExternalModelAdapt = ExternalModel_Adapt


class OutlierRemoval(object):
    """Counterpart of src/net_utils.py:750-811 on libptta_hip (one fused stencil instead of 6 ATen kernels)."""

    def __init__(self, kernel_size=7, threshold=1.5):
        self.kernel_size = kernel_size
        self.threshold = threshold
        self._scratch = None

    def remove_outliers(self, sparse_depth, validity_map):
        from . import _lib
        from .engine import _stream
        from ._lib import ptr
        lib = _lib.load()
        assert sparse_depth.is_cuda and sparse_depth.dtype == torch.float32 and sparse_depth.shape == validity_map.shape
        n, _, h, w = sparse_depth.shape
        if self._scratch is None or self._scratch.device != sparse_depth.device:
            self._scratch = torch.empty(1024, device=sparse_depth.device, dtype=torch.float32)
        sd, vm = sparse_depth.contiguous(), validity_map.contiguous()
        sd_out, vm_out = torch.empty_like(sd), torch.empty_like(vm)
        rc = lib.ptta_outlier_removal(ptr(sd), ptr(vm), ptr(sd_out), ptr(vm_out), n, h, w, int(self.kernel_size),
                                      float(self.threshold), ptr(self._scratch), _stream())
        if rc != 0:
            raise RuntimeError('ptta_outlier_removal failed (%d)' % rc)
        return sd_out, vm_out


_metric_scratch = {}


def eval_metrics(output_depth, ground_truth, min_evaluate_depth=0.0, max_evaluate_depth=100.0):
    """MAE / RMSE (mm) and iMAE / iRMSE (1/km) of src/tta_main.py:779-798 as a 4-element device tensor."""
    from . import _lib
    from ._lib import ptr
    from .engine import _stream
    lib = _lib.load()
    dev = output_depth.device
    if dev not in _metric_scratch:
        _metric_scratch[dev] = torch.empty(2048, device=dev, dtype=torch.float64)
    out = torch.empty(4, device=dev, dtype=torch.float32)
    o, g = output_depth.contiguous().float(), ground_truth.contiguous().float()
    rc = lib.ptta_eval_metrics(ptr(o), ptr(g), o.numel(), float(min_evaluate_depth), float(max_evaluate_depth),
                               ptr(_metric_scratch[dev]), ptr(out), _stream())
    if rc != 0:
        raise RuntimeError('ptta_eval_metrics failed (%d)' % rc)
    return out
