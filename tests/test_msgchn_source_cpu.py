"""CPU-only: PTTA_MSGCHN_PLAIN in include/ptta.h and the ctypes table; the façade's routing of every loss-type class of network.forward
(network_exp_msg_chn_adapt.py:342-403) with a stub in place of the engine; the training-mode refusal of 'pretrain'; what the source-model
fixtures hold (tests/golden/make_golden_msgchn_source.py)."""
import os
import re

import numpy as np
import pytest
import torch

from proxytta import _lib, synth
from proxytta.model import ExternalModel_Adapt, MsgChnModel_Adapt
from tests.msgchn_source_cases import ONE, PREPARED, SOURCE_EVAL, STAGE3_ONLY, TWO, source_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
TTA = 'adapt_meta_selfsup_seq_ema_reverse'


def test_flag_value_in_the_header_and_the_ctypes_table():
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    m = re.search(r'enum \{ PTTA_MSGCHN_PLAIN = (0x[0-9a-f]+) \};', header)            # an enum of its own
    assert m and int(m.group(1), 16) == _lib.PTTA_MSGCHN_PLAIN == 0x1000
    # one bit, clear of the base modes in the low byte and of every other flag OR-ed into meta_mode
    others = _lib.PTTA_NLSPN_LEGACY_OFFSET | _lib.PTTA_NLSPN_SYNCBN_ADAPT | _lib.PTTA_SYNCBN_ADAPT | _lib.PTTA_ADAPT_META_ONLY | _lib.PTTA_COSTDC_PLAIN
    assert bin(_lib.PTTA_MSGCHN_PLAIN).count('1') == 1 and _lib.PTTA_MSGCHN_PLAIN & (others | 0xff) == 0
    # the two enums other tests read stay as they were, and no entry point was added or changed
    assert re.search(r'PTTA_COSTDC_PLAIN = 0x800 \};', header)
    assert 'enum { PTTA_META_1LAYER = 0, PTTA_META_2LAYERS = 1, PTTA_META_NONE = 2 };' in header
    assert int(re.search(r'#define PTTA_ABI_VERSION (\d+)', header).group(1)) == _lib.PTTA_ABI_VERSION == 2


class _Stub:
    """Stands where an Engine would: records which kind was asked for and what ran on it."""

    def __init__(self, kind, log):
        self.kind, self.log = kind, log

    def forward_eval(self, image, sparse):
        self.log.append((self.kind, 'eval', torch.is_grad_enabled()))
        return torch.full((image.shape[0], 1) + tuple(image.shape[2:]), 1.0 if self.kind == 'source' else 2.0)


def _stubbed(prepared):
    m = MsgChnModel_Adapt(device=torch.device('cpu'))
    if prepared:
        m._prepare_head(ONE)
    log = []
    m._source_engine = lambda image: _Stub('source', log)
    m._engine = lambda image: _Stub('proxytta', log)
    m._timed = lambda fn, loss_type: (log.append(('timed', loss_type)), fn())[1]
    return m, log


@pytest.mark.parametrize('prepared', [False, True])
def test_routing_follows_the_reference_branch_order(prepared):
    image, sparse = torch.zeros(1, 3, 32, 48), torch.zeros(1, 1, 32, 48)
    m, log = _stubbed(prepared)
    m.eval()
    # 'pretrain' in the string, after every other branch failed to match: the source model under no_grad, through the timing hook
    for t in (None, 'pretrain', 'pretrain_time', 'pretrain_bn'):
        del log[:]
        out = m.forward(image, sparse) if t is None else m.forward(image, sparse, loss_type=t)
        assert float(out.mean()) == 1.0 and log == [('timed', t or 'pretrain'), ('source', 'eval', False)], (t, log)
    # 'meta' + 'selfsup' come first: such a string is the ProxyTTA network even with 'pretrain' in it
    for t in ('meta_selfsup_seq_ema', TTA, 'pretrain_meta_selfsup_seq_ema'):
        del log[:]
        assert float(m.forward(image, sparse, loss_type=t).mean()) == 2.0 and log[-1] == ('proxytta', 'eval', False), (t, log)
    # 'prepare' and 'init_meta' are tested before everything else, 'head' before 'meta' + 'selfsup': none of them reaches an engine in eval mode
    for t in ('prepare', 'init_meta_selfsup_seq_ema', 'pretrain_init_meta', 'head_selfsup_seq_ema', 'pretrain_head'):
        del log[:]
        with pytest.raises(NotImplementedError):
            m.forward(image, sparse, loss_type=t)
        assert log == [], (t, log)
    # a string that matches no branch raises, as the reference's unbound `output` does
    for t in ('eval', 'time', 'meta', 'selfsup', 'adapt', ''):
        with pytest.raises(NotImplementedError, match='no branch'):
            m.forward(image, sparse, loss_type=t)
    assert log == []


def test_pretrain_in_training_mode_is_refused_naming_every_parameter():
    image, sparse = torch.zeros(1, 3, 32, 48), torch.zeros(1, 1, 32, 48)
    for prepared in (False, True):
        m, log = _stubbed(prepared)
        m.train()
        for t in (None, 'pretrain', 'pretrain_time'):
            with pytest.raises(NotImplementedError, match='every parameter'):
                m.forward(image, sparse) if t is None else m.forward(image, sparse, loss_type=t)
        assert log == []
    # the façade's own default argument reaches the same branch
    model = ExternalModel_Adapt('msg_chn', 0.0, 80.0, device=torch.device('cpu'))
    model.train()
    with pytest.raises(NotImplementedError, match='every parameter'):
        model.forward(image, sparse)


def test_a_never_prepared_model_holds_the_stage0_keys():
    m = MsgChnModel_Adapt(device=torch.device('cpu'))
    sd = source_state_dict()
    assert list(m.model.state_dict().keys()) == list(sd.keys()) and not [k for k in sd if k.startswith(STAGE3_ONLY)]
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})            # what restore_model does with a stage-0 checkpoint
    for mode in (ONE, TWO):
        stage3 = source_state_dict(mode)
        assert set(stage3) - set(sd) == {k for k in stage3 if k.startswith(STAGE3_ONLY)} and all(np.array_equal(sd[k], stage3[k]) for k in sd)
    assert sd.keys() == synth.formula_state_dict_source().keys()


def test_fixtures_hold_the_stated_sizes():
    gs = [np.load(os.path.join(GOLDEN, n + '.npz')) for n, _, _, _ in SOURCE_EVAL]
    assert [tuple(int(x) for x in g['meta'][:3]) for g in gs] == [(h, w, n) for _, h, w, n in SOURCE_EVAL] == [(32, 48, 1), (32, 48, 2), (36, 52, 1)]
    for g in gs:
        h, w, n = [int(x) for x in g['meta'][:3]]
        assert g['depth_eval'].shape == (n, 1, h, w) and g['depth_eval'].dtype == np.float32 and np.isfinite(g['depth_eval']).all()
        assert float(g['tta_eval_rel_mae']) > 1e-2            # the ProxyTTA network of the same weights is another network
    p = np.load(os.path.join(GOLDEN, PREPARED + '.npz'))
    assert np.array_equal(p['depth_eval'], gs[0]['depth_eval'])              # a prepared model's 'pretrain': bit-equal in the reference
    assert all(os.path.getsize(os.path.join(GOLDEN, n + '.npz')) < 1 << 20 for n in [c[0] for c in SOURCE_EVAL] + [PREPARED])
