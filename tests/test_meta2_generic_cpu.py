"""The 2layers meta block of NLSPN / CostDCNet without a GPU: key tables, adapted lists and fixtures
(tests/golden/make_golden_2layers_generic.py)."""
import os

import numpy as np
import pytest

from proxytta import synth
from proxytta.costdcnet import costdcnet_adapted_names
from proxytta.nlspn import nlspn_adapted_names

TWO = 'meta_selfsup_seq_2layers_ema'
BLOCK = 'conv1_rgb_meta.conv1_meta.'
TWICE = [BLOCK + k for k in ('0.1.weight', '0.1.bias', '2.weight', '2.bias')]
FIXTURES = ['nlspn2l_32x64', 'nlspn2l_32x64_legacy', 'nlspn2l_40x56_n2_legacy', 'nlspn2l_352x1216_legacy', 'nlspn2l_96x320_legacy_seq8',
            'costdcnet2l_64x96', 'costdcnet2l_72x100_pad', 'costdcnet2l_480x640',
            'head_nlspn2l_forward_48x80_n2', 'head_costdcnet2l_forward_64x96_n2']
LISTS = {'nlspn': ('nlspn2l_32x64', synth.nlspn_keys, nlspn_adapted_names, 93),
         'costdcnet': ('costdcnet2l_64x96', synth.costdcnet_keys, costdcnet_adapted_names, 37)}


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + '.npz'))


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_loads_within_the_size_limit(golden_dir, name):
    path = os.path.join(golden_dir, name + '.npz')
    assert os.path.getsize(path) <= 1 << 20
    z = np.load(path)
    assert len(z.files) > 0 and all(z[k].size >= 0 for k in z.files)


@pytest.mark.parametrize('backbone', sorted(LISTS))
def test_listed_order_is_the_references(golden_dir, backbone):
    """adapt_parameters('meta_bn'): the block's seven parameters first, the BatchNorm2d pass after them, the block's two BatchNorm2d a
    second time at its end -- exactly four names twice."""
    name, keys, names_of, n_unique = LISTS[backbone]
    listed = [str(x) for x in _load(golden_dir, name)['adapted_names']]
    mine = names_of([k for k, _ in keys(TWO)])
    assert mine == listed
    assert len(set(listed)) == n_unique and len(listed) == n_unique + 4
    assert sorted(k for k in set(listed) if listed.count(k) == 2) == sorted(TWICE)
    assert listed[-4:] == TWICE and [k for k in listed[:7]] == [k for k, _ in keys(TWO) if k.startswith(BLOCK) and not
                                                                  k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))]


@pytest.mark.parametrize('backbone', sorted(LISTS))
def test_key_table_is_the_references(golden_dir, backbone):
    """The 2layers key table against the names the generator asserted against the reference's state_dict: every tensor the vectors
    name exists in the table, with the block's buffers (running statistics, num_batches_tracked) present."""
    name, keys, _, _ = LISTS[backbone]
    table = dict(keys(TWO))
    z = _load(golden_dir, name)
    named = {str(x) for x in z['adapted_names']}
    for k in z.files:
        for tag in ('/grad/', '/param/', '/exp_avg/'):
            if tag in k:
                named.add(k.split(tag, 1)[1])
    assert named <= set(table)
    for b in ('0.1', '2'):
        for leaf in ('running_mean', 'running_var', 'num_batches_tracked'):
            assert BLOCK + b + '.' + leaf in table
    ch_in, ch_hidden = (48, 256) if backbone == 'nlspn' else (16, 64)
    assert table[BLOCK + '0.0.weight'] == (ch_hidden, ch_in, 3, 3) and BLOCK + '0.0.bias' not in table
    assert table[BLOCK + '1.weight'] == (ch_in, ch_hidden, 3, 3) and table[BLOCK + '1.bias'] == (ch_in,)
    # the 1layer table is what it was
    assert 'conv1_rgb_meta.weight' in dict(keys()) and not any(k.startswith(BLOCK) for k, _ in keys())


def test_facades_list_the_duplicates_without_a_gpu():
    from proxytta.costdcnet import CostDCNetModel_Adapt
    from proxytta.nlspn import NlspnModel_Adapt
    import torch
    for cls, n in ((NlspnModel_Adapt, 97), (CostDCNetModel_Adapt, 41)):
        m = cls(device=torch.device('cpu'))
        m._prepare_head(TWO)
        params = m.adapt_parameters('meta_bn')
        assert len(params) == n and len({id(p) for p in params}) == n - 4
        assert m.meta == '2layers' and len(m.adapted) == n - 4
