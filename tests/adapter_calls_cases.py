"""The adapter -> engine call sequence, recorded on the CPU: a fake `Engine` that logs what the three host adapters (proxytta/model.py,
nlspn.py, costdcnet.py) ask of it, and the scenarios that drive them.  tests/golden/make_golden_adapter_calls.py writes the traces to
tests/golden/adapter_engine_calls.json, tests/test_adapter_calls_cpu.py replays the scenarios and compares.  The fixture pins host-side
behaviour only -- which engine is created with which keywords, what is loaded, bound and closed, in which order -- so that the adapters can be
restructured without moving it.  Only the adapters' public names are imported here."""
import contextlib
import hashlib
import json
import types
import warnings

import torch

from proxytta import synth
from proxytta.engine import adapted_names

ONE, TWO = 'meta_selfsup_seq_1layer_ema', 'meta_selfsup_seq_2layers_ema'
TTA = 'adapt_meta_selfsup_seq_ema_reverse'
HEAD = 'head_selfsup_seq_ema_reverse'
BACKBONES = ('msg_chn', 'nlspn', 'costdcnet')
NOT_IN_SOURCE = ('proj', 'pred', 'conv1_rgb_meta')

TRACE = []
LISTS = {}              # '@<digest>': a long list (state-dict keys, bound tensors) that the trace names by its digest
_binds = []             # the run of bind_adapted calls being collected: [engine id, [[name, shape], ...]]


def _flush_binds():
    """Consecutive bind_adapted calls of one engine make ONE entry (NLSPN binds 88 tensors per engine)."""
    if _binds:
        eng, bound = _binds
        del _binds[:]
        log('bind_adapted', eng, bound)


def log(*entry):
    """One trace entry, JSON-plain.  A list of more than sixteen items is entered in LISTS and replaced by its digest: the same 300 state-dict
    keys are loaded dozens of times."""
    _flush_binds()
    entry = json.loads(json.dumps(entry, default=lambda v: list(v) if isinstance(v, (tuple, torch.Size)) else str(v)))
    for i, v in enumerate(entry):
        if isinstance(v, list) and len(v) > 16:
            entry[i] = '@' + hashlib.sha1(json.dumps(v).encode()).hexdigest()[:12]
            LISTS[entry[i]] = v
    TRACE.append(entry)


def _counted(listed):
    names = list(dict.fromkeys(listed))
    return names, {k: listed.count(k) for k in names}


def _adapted_of(backbone, meta, adapt_mode, syncbn):
    """What the library reports for such a handle (Engine.adapted / adapted_repeat), from the adapters' own name functions."""
    from proxytta.costdcnet import costdcnet_adapted_names
    from proxytta.nlspn import nlspn_adapted_names, nlspn_meta_names
    if backbone == 'msg_chn':
        return _counted([] if meta == 'plain' else list(adapted_names(meta)))
    keys_of, names_of = (synth.nlspn_keys, nlspn_adapted_names) if backbone == 'nlspn' else (synth.costdcnet_keys, costdcnet_adapted_names)
    if meta in ('none', 'plain'):
        keys = [k for k, _ in keys_of() if not k.startswith(NOT_IN_SOURCE)]
        return _counted(names_of(keys) if adapt_mode == 'meta_bn' else [])
    keys = [k for k, _ in keys_of(TWO if meta == '2layers' else ONE)]
    if backbone == 'nlspn' and adapt_mode != 'meta_bn':
        return _counted(nlspn_meta_names(keys))
    return _counted(names_of(keys, syncbn))


class FakeEngine:
    """Stands where proxytta.engine.Engine would: no library, no device, CPU tensors back."""
    count = 0

    def __init__(self, n, height, width, **kw):
        FakeEngine.count += 1
        self.id = FakeEngine.count
        self.n, self.h, self.w = int(n), int(height), int(width)
        self.dtype, self.meta, self.backbone = kw.get('dtype', 'fp32'), kw.get('meta', '1layer'), kw.get('backbone', 'msg_chn')
        self.adapt_mode = kw.get('adapt_mode', 'meta_bn')
        self.adapted, self.adapted_repeat = _adapted_of(self.backbone, self.meta, self.adapt_mode, bool(kw.get('syncbn_adapted', False)))
        self.rows = 0 if self.meta in ('none', 'plain') else 4 * self.n
        self.emb_dim = 8
        self.device = torch.device('cpu')
        self.lib = types.SimpleNamespace(ptta_forward_eval_last=True)
        log('create', self.id, self.n, self.h, self.w, sorted(kw.items()))

    def _log(self, what, *args):
        log(what, self.id, *args)

    def _depth(self):
        return torch.ones(self.n, 1, self.h, self.w)

    def close(self):
        self._log('close')

    def load_state_dict(self, state):
        self._log('load_state_dict', list(state.keys()))

    def bind_adapted(self, name, param, exp_avg, exp_avg_sq):
        assert param.shape == exp_avg.shape == exp_avg_sq.shape
        if _binds and _binds[0] != self.id:
            _flush_binds()
        if not _binds:
            _binds.extend([self.id, []])
        _binds[1].append([name, list(param.shape)])

    def set_hparams(self, **kw):
        self._log('set_hparams', sorted(kw.items()))

    def set_adam_step(self, step):
        self._log('set_adam_step', int(step))

    def set_image_norm(self, normalized_image_range):
        self._log('set_image_norm', normalized_image_range)

    def enable_stat_sync(self, group=None):
        self._log('enable_stat_sync')

    def forward_train(self, image, sparse, want_emb=True):
        self._log('forward_train', image.shape)
        emb = ref = None
        if self.rows:
            emb, ref = torch.ones(self.rows, self.emb_dim), torch.ones(self.rows, self.emb_dim)
        return self._depth(), emb, ref

    def forward_eval(self, image, sparse):
        self._log('forward_eval', image.shape, torch.is_grad_enabled())
        return self._depth()

    def forward_eval_last(self):
        self._log('forward_eval_last')
        return self._depth()

    def loss_forward(self, loss_image, depth, sparse, validity, emb, ref, w_sd, w_sm, w_cos):
        self._log('loss_forward', emb is None, ref is None)
        return torch.zeros(4)

    def loss_backward(self, loss_image, depth, sparse, validity, emb, ref):
        self._log('loss_backward')
        return torch.ones_like(depth), None if ref is None else torch.ones_like(ref)

    def backward_all(self, grad_depth, grad_ref, params):
        self._log('backward_all', grad_ref is None, list(params.keys()))
        return [torch.zeros_like(params[k]) for k in self.adapted]

    def step(self, image, sparse, validity=None, loss_image=None, want_depth=False, **kw):
        self._log('step', image.shape, bool(want_depth), sorted(kw))
        return torch.zeros(4), self._depth() if want_depth else None

    # ---- stage 2 ----
    def set_head_form(self, form):
        self._log('set_head_form', int(form))

    def bind_head(self, name, param, exp_avg=None, exp_avg_sq=None):
        self._log('bind_head', name, param.shape, exp_avg is None)

    def set_head_hparams(self, **kw):
        self._log('set_head_hparams', sorted(kw.items()))

    def head_reload(self):
        self._log('head_reload')

    def head_forward(self, image, sparse, reverse=True, want=True):
        self._log('head_forward', image.shape, bool(reverse))
        return torch.ones(4 * self.n, self.emb_dim), torch.ones(4 * self.n, self.emb_dim)

    def head_backward(self):
        self._log('head_backward')
        return torch.zeros(1)

    def head_grad(self, name, like):
        return torch.zeros_like(like)

    def head_step(self, image, sparse, reverse=True):
        self._log('head_step', image.shape, bool(reverse))
        return torch.zeros(1)


@contextlib.contextmanager
def fake_engine():
    """`Engine` of the three adapter modules replaced by the fake, and put back."""
    import proxytta.costdcnet
    import proxytta.model
    import proxytta.nlspn
    mods = (proxytta.model, proxytta.nlspn, proxytta.costdcnet)
    saved = [m.Engine for m in mods]
    for m in mods:
        m.Engine = FakeEngine
    try:
        yield
    finally:
        for m, e in zip(mods, saved):
            m.Engine = e


# ---- what the scenarios are made of --------------------------------------------------------------------------------------------------
def frame(w=64, n=1, h=32):
    return torch.zeros(n, 3, h, w), torch.zeros(n, 1, h, w)


def facade(backbone):
    from proxytta.model import ExternalModel_Adapt
    return ExternalModel_Adapt(backbone, 0.0, 8.0, max_input_depth=6.0, offset=True, device=torch.device('cpu'),
                               dtype='mixed' if backbone == 'msg_chn' else 'fp32')


def adapt_mode(backbone):
    return 'meta' if backbone == 'msg_chn' else 'meta_bn'


def call(label, fn, *a, **kw):
    """One call of the adapter's surface: named in the trace, and what it raised where it refuses."""
    log('call', label)
    try:
        return fn(*a, **kw)
    except (NotImplementedError, RuntimeError, KeyError) as e:
        log('raised', type(e).__name__, str(e))
        return None


def forward(m, image, sparse, loss_type):
    return call('forward ' + loss_type, m.forward, image, sparse, loss_type=loss_type)


def train_pass(m, image, sparse, loss_type):
    """The reference's forward / compute_loss / loss.backward() (src/tta_main.py:610-632)."""
    m.train()
    depth, emb, ref = forward(m, image, sparse, loss_type)
    loss, _ = call('compute_loss', m.compute_loss, input_rgb=image, output_depth=depth, sparse_depth=sparse, validity_map=sparse,
                   embedding=emb, reference=ref)
    call('backward', loss.backward)


def adam(params):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')             # the 2layers lists name four tensors twice
        return torch.optim.Adam(list(params), lr=2e-3, betas=(0.8, 0.9), eps=1e-6)


def log_opt_steps(opt):
    log('opt_steps', [float(opt.state[p]['step']) if 'step' in opt.state[p] else None for p in opt.param_groups[0]['params']])


def prepared(backbone, mode):
    m = facade(backbone)
    call('_prepare_head', m._prepare_head, mode)
    return m


# ---- scenarios -----------------------------------------------------------------------------------------------------------------------
def never_prepared(backbone, mode=None):
    image, sparse = frame()
    m = facade(backbone)
    m.eval()
    forward(m, image, sparse, 'pretrain')
    if backbone == 'msg_chn':                   # no BatchNorm-adaptation baseline on this backbone: its ProxyTTA strings refuse
        forward(m, image, sparse, TTA)
        m.train()
        call('step', m.step, image, sparse)
        return
    call('adapt_parameters', m.adapt_parameters, 'meta_bn')
    train_pass(m, image, sparse, 'pretrain_bn')
    call('step', m.step, image, sparse)
    m.eval()
    forward(m, image, sparse, 'pretrain')
    forward(m, image, sparse, TTA)


def prepared_run(backbone, mode):
    image, sparse = frame()
    m = facade(backbone)
    m.eval()
    forward(m, image, sparse, 'pretrain')
    call('_prepare_head', m._prepare_head, mode)
    call('adapt_parameters', m.adapt_parameters, adapt_mode(backbone))
    call('set_image_norm', m.set_image_norm, [0, 1])
    forward(m, image, sparse, 'pretrain')                   # the plain engine that the last call below finds again, a step later
    train_pass(m, image, sparse, TTA)
    call('step', m.step, image, sparse, want_depth=True)
    call('step 32x96', m.step, *frame(96))                  # a second shape: the Adam step count carries over
    call('step', m.step, image, sparse)
    m.eval()
    forward(m, image, sparse, TTA)
    forward(m, image, sparse, 'pretrain')
    m.train()
    forward(m, image, sparse, 'pretrain')
    forward(m, image, sparse, 'pretrain_bn')


def bound_optimizer(backbone, mode):
    image, sparse = frame()
    m = prepared(backbone, mode)
    opt = adam(call('adapt_parameters', m.adapt_parameters, adapt_mode(backbone)))
    m.eval()
    forward(m, image, sparse, TTA)                          # a live engine: it gets the optimizer's hyper-parameters, then is released
    call('bind_optimizer', m.model.bind_optimizer, opt)
    m.train()
    call('step', m.step, image, sparse)
    call('step', m.step, image, sparse)
    log_opt_steps(opt)
    call('step 32x96', m.step, *frame(96))
    log_opt_steps(opt)
    call('bind_optimizer', m.model.bind_optimizer, opt)     # again (restore_model does it): the count continues from the optimizer's
    call('step', m.step, image, sparse)
    log_opt_steps(opt)


def syncbn_first(backbone, mode):
    image, sparse = frame()
    m = prepared(backbone, mode)
    call('convert_syncbn', m.convert_syncbn)                # src/tta_main.py:326, before adapt_parameters (:339)
    opt = adam(call('adapt_parameters', m.adapt_parameters, adapt_mode(backbone)))
    call('bind_optimizer', m.model.bind_optimizer, opt)
    m.train()
    call('step', m.step, image, sparse)
    log_opt_steps(opt)
    m.eval()
    forward(m, image, sparse, TTA)
    forward(m, image, sparse, 'pretrain')


def syncbn_live(backbone, mode):
    image, sparse = frame()
    m = prepared(backbone, mode)
    call('adapt_parameters', m.adapt_parameters, adapt_mode(backbone))
    m.eval()
    forward(m, image, sparse, TTA)
    forward(m, image, sparse, 'pretrain')
    call('convert_syncbn', m.convert_syncbn)
    forward(m, image, sparse, TTA)
    never = facade(backbone)
    never.eval()
    forward(never, image, sparse, 'pretrain')
    call('convert_syncbn', never.convert_syncbn)
    forward(never, image, sparse, 'pretrain')
    call('adapt_parameters', never.adapt_parameters, adapt_mode(backbone))


def nlspn_mode_switch(backbone='nlspn', mode=ONE):
    image, sparse = frame()
    m = prepared('nlspn', ONE)
    call('adapt_parameters', m.adapt_parameters, 'meta')
    m.eval()
    forward(m, image, sparse, TTA)
    forward(m, image, sparse, 'pretrain')
    train_pass(m, image, sparse, TTA)
    call('step', m.step, image, sparse)
    call('adapt_parameters', m.adapt_parameters, 'meta_fix')        # another mode string: engines released
    call('adapt_parameters', m.adapt_parameters, 'meta_bn')         # drops the running statistics: engines released, plain ones too
    m.eval()
    forward(m, image, sparse, TTA)
    forward(m, image, sparse, 'pretrain')
    call('adapt_parameters', m.adapt_parameters, 'meta_bn')         # nothing changes: nothing released
    call('adapt_parameters', m.adapt_parameters, 'bn')


def next_frame(backbone, mode):
    image, sparse = frame()
    m = prepared(backbone, mode)
    call('adapt_parameters', m.adapt_parameters, adapt_mode(backbone))
    m.train()
    call('step next_frame', m.step, image, sparse, next_frame=frame())
    call('step next_frame 32x96', m.step, image, sparse, next_frame=frame(96))          # another shape is another engine: not announced
    call('model.step next_frame', m.model.step, image, sparse, next_frame=frame())
    call('adapt next_frame', m.adapt, image, sparse, inner_iter=2, next_frame=frame())
    call('adapt next_frame 32x96', m.adapt, image, sparse, inner_iter=1, next_frame=frame(96))
    call('adapt', m.adapt, image, sparse, inner_iter=2)


def lifecycle(backbone, mode):
    image, sparse = frame()
    m = prepared(backbone, mode)
    call('adapt_parameters', m.adapt_parameters, adapt_mode(backbone))
    m.eval()
    forward(m, image, sparse, TTA)
    forward(m, image, sparse, 'pretrain')
    state = m.model.state_dict() if hasattr(m.model, 'state_dict') else m.model.model.state_dict()
    call('load_state_dict', m.model.load_state_dict, dict(state))
    call('load_state_dict short', m.model.load_state_dict, {k: v for k, v in list(state.items())[1:]})
    call('set_hparams', m.model.set_hparams, lr=1e-4, max_input_depth=5.0)
    call('to', m.to, torch.device('cpu'))
    forward(m, image, sparse, TTA)
    call('_clear_engines', m.model._clear_engines)
    call('_prepare_head bad', m._prepare_head, 'meta_selfsup_seq_3layers_ema')
    call('_prepare_head bad', m._prepare_head, 'selfsup_seq_1layer_ema')


def head_trainer(backbone, mode):
    """Stage 2 (src/head_main.py:259-276, :464-480) goes through the same `_engine`."""
    image, sparse = frame(n=2)
    m = facade(backbone)
    call('prepare_parameters', m.prepare_parameters, 'head_selfsup_ema')
    call('_prepare_head', m._prepare_head, mode)
    m.train()
    forward(m, image, sparse, HEAD)                          # before prepare_parameters: refused
    opt = adam(call('prepare_parameters', m.prepare_parameters, 'head_selfsup_ema'))
    _, emb, ref = forward(m, image, sparse, HEAD)            # default hyper-parameters, no optimizer bound
    loss, _ = call('compute_loss prepare', m.compute_loss, embedding=emb, reference=ref, loss_type='prepare')
    call('backward', loss.backward)
    call('bind_head_optimizer', m.bind_head_optimizer, opt, 0.99)
    call('head_step', m.head_step, image, sparse, HEAD)
    call('head_step n=1', m.head_step, *frame(), HEAD)
    call('head_step non-reverse', m.head_step, image, sparse, 'head_selfsup_seq_ema')
    log_opt_steps(opt)
    call('convert_syncbn', m.convert_syncbn)
    call('head_step', m.head_step, image, sparse, HEAD)
    m.eval()
    forward(m, image, sparse, HEAD)


def _scenarios():
    out = {}
    for b in BACKBONES:
        out['never_prepared/' + b] = (never_prepared, b, None)
        for tag, mode in (('1layer', ONE), ('2layers', TWO)):
            for fn in (prepared_run, bound_optimizer, syncbn_first, syncbn_live, next_frame, lifecycle, head_trainer):
                out['%s/%s/%s' % (fn.__name__, b, tag)] = (fn, b, mode)
    out['nlspn_mode_switch'] = (nlspn_mode_switch, 'nlspn', ONE)
    return out


SCENARIOS = _scenarios()


def run(name):
    """The trace of one scenario: a list of JSON-plain entries."""
    fn, backbone, mode = SCENARIOS[name]
    del TRACE[:], _binds[:]
    FakeEngine.count = 0
    torch.manual_seed(0)
    with fake_engine():
        fn(backbone, mode)
    _flush_binds()
    return list(TRACE)
