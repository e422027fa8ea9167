"""The SyncBatchNorm form of the stage-2 head trainer without a GPU: its fixtures (tests/golden/make_golden_head_syncbn.py) and the ABI."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
NAMES = ['head_syncbn_%s_%s' % (b, c) for b, sizes in (('nlspn', '48x80'), ('costdcnet', '64x96'), ('msg_chn', '32x48'))
         for c in ('forward_' + sizes, 'reverse_' + sizes, 'reverse_' + sizes + '_n2')]


@pytest.mark.parametrize('name', NAMES)
def test_fixture_carries_what_the_gpu_tests_read(name):
    path = os.path.join(GOLD, name + '.npz')
    assert os.path.getsize(path) < 1 << 20
    z = np.load(path)
    h, w, n, steps = (int(v) for v in z['meta'][:4])
    assert (n == 2) == name.endswith('_n2') and 2 <= steps <= 3
    assert len(z['head_names']) == 12 and len(z['hp']) == 6 and int(z['n_syncbn']) > 0
    assert 'before/proj_t.1.running_mean' in z.files and 'before/proj_t.1.running_var' in z.files
    last = 's%d/' % (steps - 1)
    for s in range(steps):
        assert 's%d/loss' % s in z.files
        for k in z['head_names']:
            k = str(k)
            assert 's%d/has_grad/%s' % (s, k) in z.files
            for pre in ('s%d/after/' % s,) + ((last + 'exp_avg/', last + 'exp_avg_sq/') if bool(z['s%d/has_grad/%s' % (s, k)]) else ()):
                assert pre + k in z.files or pre + k + '#rows' in z.files, pre + k
        for b in ('proj.1', 'pred.1', 'proj_t.1'):
            assert 's%d/after/%s.running_mean' % (s, b) in z.files


@pytest.mark.parametrize('backbone,size', [('nlspn', '48x80'), ('costdcnet', '64x96')])
def test_syncbn_form_differs_from_the_plain_form(backbone, size):
    """Same inputs as the plain form's batch-2 reverse vectors (make_golden_head_generic.py): after the conversion proj_t.1 evaluates from its
    running statistics (and on CostDCNet the UNet3D / sparse encoder BatchNorms too), so the loss and proj_t.1's buffers differ."""
    plain = np.load(os.path.join(GOLD, 'head_%s_reverse_%s_n2.npz' % (backbone, size)))
    sync = np.load(os.path.join(GOLD, 'head_syncbn_%s_reverse_%s_n2.npz' % (backbone, size)))
    assert list(plain['meta'][:4]) == list(sync['meta'][:4]) and str(plain['loss_type']) == str(sync['loss_type'])
    assert abs(float(plain['s0/loss']) - float(sync['s0/loss'])) > 1e-4
    rm = 's0/after/proj_t.1.running_mean'
    np.testing.assert_array_equal(sync[rm], sync['before/proj_t.1.running_mean'])          # eval mode: untouched
    assert np.abs(plain[rm] - sync[rm]).max() > 1e-3                                       # train mode: moved


def test_msg_chn_syncbn_vectors_are_the_plain_computation():
    """src/msg_chn_model_adapt.py:435-440: nothing changes on one rank (the plain fixture holds the same reverse loss at n = 2)."""
    sync = np.load(os.path.join(GOLD, 'head_syncbn_msg_chn_reverse_32x48_n2.npz'))
    plain = np.load(os.path.join(GOLD, 'head_reverse_32x48_n2.npz'))
    for s in range(2):
        assert float(sync['s%d/loss' % s]) == pytest.approx(float(plain['s%d/loss' % s]), rel=1e-6, abs=1e-7)


def test_header_declares_the_head_form():
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tta-depth-completion_amd'))
    from proxytta import _lib
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    assert re.search(r'int ptta_head_set_form\(ptta_handle h, int form\);', header)
    assert 'PTTA_HEAD_FORM_PLAIN = 0' in header and 'PTTA_HEAD_FORM_SYNCBN = 1' in header
    assert ('ptta_head_set_form', _lib.c_int, [_lib._P, _lib.c_int]) in [tuple(x) for x in _lib.SIGNATURES]
    assert (_lib.PTTA_HEAD_FORM_PLAIN, _lib.PTTA_HEAD_FORM_SYNCBN) == (0, 1)
