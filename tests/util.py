"""Shared helpers for the GPU parity tests."""
import os

import numpy as np
import torch

from proxytta import synth

ONE = 'meta_selfsup_seq_1layer_ema'


def rel_mae(a, b, floor=1e-4):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float64)
    return float(np.abs(a - b).mean() / max(np.abs(b).mean(), floor))


TWO = 'meta_selfsup_seq_2layers_ema'


def make_engine(n, h, w, dtype='fp32', hp=None, gain=1.0, impl=None, meta='1layer', head_bias=0.0, options=None, keep=()):
    """Engine with formula weights; returns (engine, state dict on device, adapted dict)."""
    from proxytta.engine import Engine, adapted_names
    os.environ.pop('PTTA_CONV_IMPL', None)
    os.environ.pop('PTTA_ARITH', None)
    if impl == 'naive':
        os.environ['PTTA_CONV_IMPL'] = 'naive'
        os.environ['PTTA_ARITH'] = 'exact'
    elif impl == 'exact':
        os.environ['PTTA_ARITH'] = 'exact'
    hp = dict(hp or {})
    eng = Engine(n, h, w, dtype=dtype, meta=meta, options=options, keep=keep, **hp)
    os.environ.pop('PTTA_CONV_IMPL', None)
    os.environ.pop('PTTA_ARITH', None)
    sd = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in synth.formula_state_dict(TWO if meta == '2layers' else ONE, gain, head_bias).items()}
    eng.load_state_dict(sd)
    adapted = {}
    for name in adapted_names(meta):
        p = sd[name]
        adapted[name] = (p, torch.zeros_like(p), torch.zeros_like(p))
        eng.bind_adapted(name, *adapted[name])
    return eng, sd, adapted


def golden_hp(g):
    lr, b1, b2, eps, wd, w_sd, w_sm, w_cos, mid, gain = [float(x) for x in g['hp']]
    return dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, w_sparse_depth=w_sd, w_smoothness=w_sm,
                w_cos=w_cos, max_input_depth=mid), gain


def assert_elementwise(got, ref64, bound, what=''):
    """Every element of `got` (fp32 from the GPU, NHWC) within `bound` (same shape) of the float64 reference `ref64`.  The message names
    the worst element (largest |error| / bound): its index (b, y, x, channel), its place inside the kernels' tile (y mod 8, x mod 32,
    channel mod 32), got / ref / bound, and how many elements fail where -- rows, columns and channels of the failing set."""
    def arr(a):
        return np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    got, ref64, bound = arr(got), arr(ref64), arr(bound)
    assert got.shape == ref64.shape == bound.shape and got.ndim == 4, (got.shape, ref64.shape, bound.shape)
    err = np.abs(got - ref64)
    bad = ~(err <= bound)                      # a NaN fails
    nbad = int(bad.sum())
    if nbad == 0:
        return
    score = np.where(np.isfinite(err), err / np.maximum(bound, 1e-300), np.inf)
    b, y, x, c = np.unravel_index(int(np.argmax(np.where(bad, score, -1.0))), got.shape)
    where = np.argwhere(bad)

    def span(axis):
        v = np.unique(where[:, axis])
        return '%d' % v[0] if v.size == 1 else '%d..%d (%d distinct)' % (v[0], v[-1], v.size)
    raise AssertionError(
        '%s: %d of %d elements outside the bound; worst at (b %d, y %d, x %d, channel %d) = tile position (y mod 8 = %d, x mod 32 = %d, '
        'channel mod 32 = %d): got %.9g ref %.9g |error| %.3g bound %.3g; failing images %s, rows %s, columns %s, channels %s'
        % (what, nbad, got.size, b, y, x, c, y % 8, x % 32, c % 32, got[b, y, x, c], ref64[b, y, x, c], err[b, y, x, c], bound[b, y, x, c],
           span(0), span(1), span(2), span(3)))
