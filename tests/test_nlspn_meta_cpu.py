"""CPU-only: the façade's adapt_parameters('meta') / ('meta_fix') list (src/nlspn_model_adapt.py:302-320) from the key table, without an
engine; the flag and the test hook in include/ptta.h and the ctypes table."""
import os
import re

import numpy as np
import pytest
import torch

from proxytta import _lib, synth
from proxytta.nlspn import NlspnModel_Adapt, nlspn_meta_names
from tests.nlspn_meta_cases import META_NAMES, PREPARE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_meta_list_is_the_references_two_names_in_order():
    keys = [k for k, _ in synth.nlspn_keys(PREPARE)]
    assert nlspn_meta_names(keys) == META_NAMES == ['conv1_rgb_meta.weight', 'conv1_rgb_meta.bias']
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'nlspn_meta_32x64.npz'))
    assert [str(x) for x in g['adapted_names']] == META_NAMES                 # what the reference's adapt_parameters('meta') yielded
    m = NlspnModel_Adapt(device=torch.device('cpu'))
    with pytest.raises(RuntimeError, match='_prepare_head'):
        m.adapt_parameters('meta')
    m._prepare_head(PREPARE)
    named = dict(m.model.named_parameters())
    for mode in ('meta', 'meta_fix'):
        params = m.adapt_parameters(mode)
        assert [id(p) for p in params] == [id(named[k]) for k in META_NAMES]
        assert m.adapted == m.adapted_listed == META_NAMES and m.adapt_mode == mode and not m._engines
        assert [tuple(p.shape) for p in params] == [(48, 48, 3, 3), (48,)]
    assert len(m.adapt_parameters('meta_bn')) == 88 and m.adapt_mode == 'meta_bn' and len(m.adapted) == 88
    with pytest.raises(NotImplementedError):
        m.adapt_parameters(None)
    m2 = NlspnModel_Adapt(device=torch.device('cpu'))
    m2._prepare_head('meta_selfsup_seq_2layers_ema')
    with pytest.raises(NotImplementedError, match='1layer'):
        m2.adapt_parameters('meta')


def test_flag_and_hook_are_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    assert int(re.search(r'PTTA_ADAPT_META_ONLY = (0x[0-9a-f]+)', header).group(1), 16) == _lib.PTTA_ADAPT_META_ONLY == 0x400
    assert _lib.PTTA_ADAPT_META_ONLY & (_lib.PTTA_NLSPN_LEGACY_OFFSET | _lib.PTTA_NLSPN_SYNCBN_ADAPT | 0xff) == 0
    sig = {name: args for name, _, args in _lib.SIGNATURES}
    # ptta_op_gconv's arguments, then scale, shift, res, ld_res in front of the stream
    assert sig['ptta_op_gconv_affine'] == sig['ptta_op_gconv'][:-1] + [_lib._P, _lib._P, _lib._P, _lib.c_int, _lib._P]
    decl = re.search(r'int ptta_op_gconv_affine\(([^;]*)\);', header).group(1)
    assert len(decl.split(',')) == len(sig['ptta_op_gconv_affine']) and '"eval_bn_fused"' in header
