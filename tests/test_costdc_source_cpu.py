"""CPU-only: PTTA_COSTDC_PLAIN in include/ptta.h and the ctypes table; the ELU code of the affine hook; the façade's loss_type routing of
'pretrain' and its 30-entry BatchNorm-baseline list without an engine; what the source-model and baseline fixtures hold
(tests/golden/make_golden_costdc_source.py)."""
import os
import re

import numpy as np
import pytest
import torch

from proxytta import _lib, synth
from proxytta.costdcnet import CostDCNetModel_Adapt, costdcnet_adapted_names
from proxytta.engine import GBN_ACTS, GCONV_ACTS, GCONV_AFFINE_ACTS
from tests.costdc_source_cases import (BASELINE_FIRST, BASELINE_SEQ, PREPARE, SOURCE_EVAL, STAGE3_ONLY, baseline_names, bn_prefixes, canonical,
                                       source_state_dict)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def test_flag_value_in_the_header_and_the_ctypes_table():
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    m = re.search(r'PTTA_COSTDC_PLAIN = (0x[0-9a-f]+) \};', header)
    assert m and int(m.group(1), 16) == _lib.PTTA_COSTDC_PLAIN == 0x800
    # one bit, clear of the base modes in the low byte and of every other flag OR-ed into meta_mode
    others = _lib.PTTA_NLSPN_LEGACY_OFFSET | _lib.PTTA_NLSPN_SYNCBN_ADAPT | _lib.PTTA_SYNCBN_ADAPT | _lib.PTTA_ADAPT_META_ONLY
    assert bin(_lib.PTTA_COSTDC_PLAIN).count('1') == 1 and _lib.PTTA_COSTDC_PLAIN & (others | 0xff) == 0
    assert int(re.search(r'#define PTTA_ABI_VERSION (\d+)', header).group(1)) == _lib.PTTA_ABI_VERSION       # no entry point was added or changed
    assert '"eval_bn_fused_count"' in header


def test_elu_is_an_activation_of_the_affine_hook_only():
    assert GCONV_AFFINE_ACTS == dict(GCONV_ACTS, elu=4) and 'elu' not in GCONV_ACTS and GCONV_AFFINE_ACTS['elu'] == GBN_ACTS['elu']
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    assert 'act 4 (ELU)' in header


def test_facade_lists_without_a_device():
    m = CostDCNetModel_Adapt(device=torch.device('cpu'), max_depth=8.0)
    assert not m.stats_dropped
    params = m.adapt_parameters('meta_bn')
    named = dict(m.model.named_parameters())
    full = costdcnet_adapted_names([k for k, _ in synth.costdcnet_keys(PREPARE)])
    want = [k for k in full if not k.startswith('conv1_rgb_meta')]
    assert len(full) == 32 and len(want) == 30 == len(params)
    assert m.adapted == m.adapted_listed == want == baseline_names() and m.stats_dropped and not m._engines
    assert [id(p) for p in params] == [id(named[k]) for k in want]
    assert sum(p.numel() for p in params) == 5200 - 16 * 16 * 9 - 16
    with pytest.raises(NotImplementedError):
        m.adapt_parameters('meta')
    # a prepared model keeps its 32-entry list; the call drops the running statistics there too
    p = CostDCNetModel_Adapt(device=torch.device('cpu'), max_depth=8.0)
    p._prepare_head(PREPARE)
    assert len(p.adapt_parameters('meta_bn')) == 32 and p.adapted == full and p.stats_dropped


def test_routing_without_a_device():
    m = CostDCNetModel_Adapt(device=torch.device('cpu'), max_depth=8.0)
    image, sparse = torch.zeros(1, 3, 64, 96), torch.zeros(1, 1, 64, 96)
    m.train()
    for t in (None, 'pretrain', 'pretrain_time'):          # CostDCNet_adapt.py:44: 'pretrain' in the string is the first test
        with pytest.raises(NotImplementedError, match='every parameter'):          # the reference's tensor has autograd into all of them
            m.forward(image, sparse) if t is None else m.forward(image, sparse, loss_type=t)
    with pytest.raises(RuntimeError, match='meta_bn'):                          # 'bn' in the string, but nothing selected the baseline
        m.forward(image, sparse, loss_type='pretrain_bn')
    p = CostDCNetModel_Adapt(device=torch.device('cpu'), max_depth=8.0)
    p._prepare_head(PREPARE)
    p.adapt_parameters('meta_bn')
    p.train()
    with pytest.raises(RuntimeError, match='never prepared'):                   # the baseline is the unprepared model's
        p.forward(image, sparse, loss_type='pretrain_bn')
    m.eval()
    with pytest.raises(RuntimeError, match='_prepare_head'):              # the ProxyTTA strings still need the head
        m.forward(image, sparse, loss_type='adapt_meta_selfsup_seq_ema_reverse')
    assert not m._engines


def test_fixtures_hold_the_stated_names_and_counts():
    sd = source_state_dict()
    assert not [k for k in sd if k.startswith(STAGE3_ONLY)]
    pre = {canonical(p) for p in bn_prefixes(sd)}
    assert sum(p.startswith('enc2d.') for p in pre) == 15 and sum(p.startswith('unet3d.') for p in pre) == 28 and sum(p.startswith('enc3d.') for p in pre) == 9
    stage3 = source_state_dict(stage3=True)
    assert set(stage3) - set(sd) == {k for k in stage3 if k.startswith(STAGE3_ONLY)} and all(np.array_equal(sd[k], stage3[k]) for k in sd)
    for k in sd:                               # ResBlock.norm3 and its alias hold one set of values
        if k.startswith('enc2d.') and '.downsample.1.' in k:
            assert np.array_equal(sd[k], sd[k.replace('.downsample.1.', '.norm3.')]), k
    src = [np.load(os.path.join(GOLDEN, n + '.npz')) for n, _, _, _ in SOURCE_EVAL]
    assert [tuple(int(x) for x in g['meta'][:3]) for g in src] == [(h, w, n) for _, h, w, n in SOURCE_EVAL] == [(64, 96, 1), (72, 100, 1), (64, 64, 2)]
    stats = [k for k in src[0].files if k.startswith('bn/')]
    assert len(stats) == 2 * (15 + 28 + 9) and not [k for g in src[1:] for k in g.files if k.startswith('bn/')]           # stored once
    # the loaded buffers are neither (0, 1) nor trivial
    assert all(float(np.abs(src[0][k]).max()) > 1e-3 for k in stats)
    for g in src:
        assert float(g['batch_stat_eval_rel_mae']) > 1e-2
        assert g['depth_eval'].shape == (int(g['meta'][2]), 1, int(g['meta'][0]), int(g['meta'][1]))
    assert all(os.path.getsize(os.path.join(GOLDEN, n + '.npz')) < 1 << 20 for n, _, _, _ in SOURCE_EVAL)


def test_baseline_fixtures_hold_the_stated_names_and_counts():
    sd = source_state_dict()
    names = baseline_names()
    for name, h, w, n in BASELINE_FIRST + [BASELINE_SEQ]:
        g = np.load(os.path.join(GOLDEN, name + '.npz'))
        steps = int(g['meta'][3])
        assert tuple(int(x) for x in g['meta'][:3]) == (h, w, n)
        assert [str(x) for x in g['adapted_names']] == names and len(names) == 30
        assert float(g['s0/loss_info'][3]) == 0.0 and int(g['nbt_step']) == 1
        assert sum(k.startswith('s0/grad/') for k in g.files) == 30 and sum(k.startswith('s%d/param/' % (steps - 1)) for k in g.files) == 30
        assert all(g['s0/grad/' + k].shape == sd[k].shape for k in names)
        bufs = [k[len('s0/buf/'):] for k in g.files if k.startswith('s0/buf/')]
        assert len(bufs) == 2 * (28 + 9) and all(not np.array_equal(g['s0/buf/' + k], sd[k]) for k in bufs)      # every one moved
        assert (sum(k.startswith('s0/grad64/') for k in g.files) == 30) == ((name, h, w, n) in BASELINE_FIRST)
        assert os.path.getsize(os.path.join(GOLDEN, name + '.npz')) < 1 << 20
    assert steps == 6 and g['alt_rel_mae'].shape == (6,) and float(g['alt_rel_mae'].max()) < 1e-3
