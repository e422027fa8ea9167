"""CPU-only: PTTA_META_NONE in include/ptta.h and the ctypes table; the façade's BatchNorm-baseline list and its loss_type routing without an
engine; the names and counts the source-model / baseline fixtures hold (tests/golden/make_golden_nlspn_source.py)."""
import os
import re

import numpy as np
import pytest
import torch

from proxytta import _lib, synth
from proxytta.nlspn import NlspnModel_Adapt, is_plain_loss_type, nlspn_adapted_names
from tests.nlspn_meta_cases import PREPARE, bn2d_prefixes
from tests.nlspn_source_cases import BASELINE_FIRST, BASELINE_SEQ, NOT_IN_SOURCE, SOURCE_EVAL, baseline_names, source_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def test_header_constant_and_signatures_agree():
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    m = re.search(r'enum \{ PTTA_META_1LAYER = (\d+), PTTA_META_2LAYERS = (\d+), PTTA_META_NONE = (\d+) \};', header)
    assert m and [int(v) for v in m.groups()] == [_lib.PTTA_META_1LAYER, _lib.PTTA_META_2LAYERS, _lib.PTTA_META_NONE] == [0, 1, 2]
    # the value lives in the low byte of meta_mode, clear of every flag OR-ed into it
    assert _lib.PTTA_META_NONE & (_lib.PTTA_NLSPN_LEGACY_OFFSET | _lib.PTTA_NLSPN_SYNCBN_ADAPT | _lib.PTTA_ADAPT_META_ONLY) == 0
    assert int(re.search(r'#define PTTA_ABI_VERSION (\d+)', header).group(1)) == _lib.PTTA_ABI_VERSION == 2       # no entry point was added or changed
    for name, _, args in _lib.SIGNATURES:
        decl = re.search(r'^[a-z][\w \*]*\b%s\(([^;]*)\);' % name, header, re.M)
        assert decl, name
        got = decl.group(1).strip()
        assert (0 if got in ('void', '') else len(got.split(','))) == len(args), name


def test_facade_lists_without_a_device():
    m = NlspnModel_Adapt(device=torch.device('cpu'))
    for mode in ('meta', 'meta_fix'):
        with pytest.raises(RuntimeError, match='_prepare_head'):
            m.adapt_parameters(mode)
    assert not m.stats_dropped
    params = m.adapt_parameters('meta_bn')
    named = dict(m.model.named_parameters())
    full = nlspn_adapted_names([k for k, _ in synth.nlspn_keys(PREPARE)])
    want = [k for k in full if not k.startswith('conv1_rgb_meta')]
    assert len(full) == 88 and len(want) == 86 == len(params)
    assert m.adapted == m.adapted_listed == want == baseline_names() and m.stats_dropped and not m._engines
    assert [id(p) for p in params] == [id(named[k]) for k in want]
    assert sum(p.numel() for p in params) == 40048 - 48 * 48 * 9 - 48
    # a prepared model keeps its 88-entry list; the call drops the running statistics there too
    p = NlspnModel_Adapt(device=torch.device('cpu'))
    p._prepare_head(PREPARE)
    assert len(p.adapt_parameters('meta_bn')) == 88 and p.adapted == full and p.stats_dropped


def test_routing_without_a_device():
    # nlspnmodel_adapt.py:502-509, :609-616: 'pretrain' in any form, or a string with none of adapt / selfsup / meta / head
    for t in ('pretrain', 'pretrain_bn', 'pretrain_adapt_meta', 'time', 'bn', 'prepare', 'eval'):
        assert is_plain_loss_type(t), t
    for t in ('adapt_meta_selfsup_seq_ema_reverse', 'head_selfsup_seq_ema', 'selfsup', 'meta', 'adapt', 'selfsup_init_meta_seq_ema'):
        assert not is_plain_loss_type(t), t
    m = NlspnModel_Adapt(device=torch.device('cpu'))
    image, sparse = torch.zeros(1, 3, 32, 64), torch.zeros(1, 1, 32, 64)
    m.train()
    with pytest.raises(NotImplementedError, match='every parameter'):          # the reference's tensor has autograd into all of them
        m.forward(image, sparse)
    with pytest.raises(RuntimeError, match='meta_bn'):                          # 'bn' in the string, but nothing selected the baseline
        m.forward(image, sparse, loss_type='pretrain_bn')
    m.eval()
    with pytest.raises(RuntimeError, match='_prepare_head'):                    # the ProxyTTA strings still need the head
        m.forward(image, sparse, loss_type='adapt_meta_selfsup_seq_ema_reverse')
    m.convert_syncbn()
    with pytest.raises(NotImplementedError, match='one rank'):
        m.forward(image, sparse)


def test_fixtures_hold_the_stated_names_and_counts():
    sd = source_state_dict()
    assert not [k for k in sd if k.startswith(NOT_IN_SOURCE)] and len(bn2d_prefixes(sd)) == 43
    with_head = source_state_dict(with_head=True)
    assert set(with_head) - set(sd) == {k for k in with_head if k.startswith(NOT_IN_SOURCE)} and all(np.array_equal(sd[k], with_head[k]) for k in sd)
    src = [np.load(os.path.join(GOLDEN, n + '.npz')) for n in SOURCE_EVAL]
    assert [tuple(int(x) for x in g['meta'][:3]) for g in src] == [(32, 64, 1), (40, 56, 2)] and [int(g['legacy']) for g in src] == [0, 1]
    stats = [k for k in src[0].files if k.startswith('bn/')]
    assert len(stats) == 86 and not [k for k in src[1].files if k.startswith('bn/')]           # stored once
    for g in src:
        assert float(g['batch_stat_eval_rel_mae']) > 1e-2 and int(g['n_zero_eval']) == int((g['depth_eval'] == 0).sum())
        assert g['depth_eval'].shape == (int(g['meta'][2]), 1, int(g['meta'][0]), int(g['meta'][1]))
    names = baseline_names()
    for name in BASELINE_FIRST + (BASELINE_SEQ,):
        g = np.load(os.path.join(GOLDEN, name + '.npz'))
        steps = int(g['meta'][3])
        assert [str(x) for x in g['adapted_names']] == names and len(names) == 86
        assert float(g['s0/loss_info'][3]) == 0.0
        assert sum(k.startswith('s0/grad/') for k in g.files) == 86 and sum(k.startswith('s%d/param/' % (steps - 1)) for k in g.files) == 86
        for s in range(steps):
            assert int(g['s%d/n_zero_eval' % s]) == int((g['s%d/depth_eval' % s] == 0).sum())
        assert all(g['s0/grad/' + k].shape == sd[k].shape for k in names)
        assert (sum(k.startswith('s0/exp_avg/') for k in g.files) == 86) == (name in BASELINE_FIRST)
    assert steps == 6 and g['alt_rel_mae'].shape == (6,) and float(g['alt_rel_mae'].max()) < 1e-3
    assert all(os.path.getsize(os.path.join(GOLDEN, n + '.npz')) < 1 << 20 for n in SOURCE_EVAL + BASELINE_FIRST + (BASELINE_SEQ,))
