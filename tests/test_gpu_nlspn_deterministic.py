"""Option "deterministic" of the NLSPN engine (include/ptta.h): with it the step holds no float atomic, so the same frames give the same
bits -- between two handles, between direct launches and hipGraph replay, and between the two copies of one frame in a batch -- while the
step stays inside the bounds tests/test_gpu_nlspn.py holds the default step to."""
import os

import numpy as np
import pytest
import torch

from proxytta import synth
from proxytta.engine import Engine
from tests.test_gpu_nlspn import HP, TOL, make_nlspn, nlspn_frame
from tests.util import rel_mae

pytestmark = pytest.mark.gpu


def make(kind, n, h, w):
    """-> (engine with "deterministic" 1, {adapted name: (param, exp_avg, exp_avg_sq)}) of every NLSPN handle kind that trains"""
    if kind == '1layer':
        eng, _, ad = make_nlspn(n, h, w)
    elif kind == 'mixed':
        eng, _, ad = make_nlspn(n, h, w, hp=dict(HP, dtype='mixed'))
    elif kind == '2layers':
        from tests.test_gpu_meta2_generic import make as make2
        eng, _, ad = make2('nlspn', n, h, w, HP)
    elif kind == 'meta':
        from tests.test_gpu_nlspn_meta import make_meta
        eng, _, ad = make_meta(n, h, w, HP)
    else:
        from tests.test_gpu_nlspn_source import make as make_plain
        eng, _, ad = make_plain('baseline', n, h, w, HP)
    assert eng.get_option('deterministic') == 0                             # the default
    eng.set_option('deterministic', 1)
    assert eng.get_option('deterministic') == 1
    return eng, ad


def three_steps(kind, n, h, w, graph=0):
    """three steps on frames 0..2, an eval forward after each -> every quantity the run leaves behind, cloned"""
    eng, ad = make(kind, n, h, w)
    eng.set_option('graph', graph)
    out = {}
    for s in range(3):
        raw, image1, sparse = [torch.from_numpy(x).cuda() for x in nlspn_frame(s, h, w, n)]
        info, depth = eng.step(image1, sparse, loss_image=raw, want_depth=True)
        d_eval = eng.forward_eval(image1, sparse)
        out.update({'s%d/loss_info' % s: info.clone(), 's%d/depth_train' % s: depth.clone(), 's%d/depth_eval' % s: d_eval.clone()})
    torch.cuda.synchronize()
    for k, (p, m, v) in ad.items():
        out.update({'param/' + k: p.clone(), 'exp_avg/' + k: m.clone(), 'exp_avg_sq/' + k: v.clone()})
    eng.close()
    return out


def assert_same_bits(a, b):
    assert a.keys() == b.keys()
    differ = [k for k in a if not torch.equal(a[k], b[k])]
    assert not differ, differ[:8]
    assert all(bool(torch.isfinite(v).all()) for v in a.values())


_RUNS = {}


def first_run(kind, n, h, w):
    """the direct-launch run of a configuration, made once and shared by the run-to-run and the graph tests"""
    key = (kind, n, h, w)
    if key not in _RUNS:
        _RUNS[key] = three_steps(kind, n, h, w)
    return _RUNS[key]


CONFIGS = [('1layer', 1, 32, 64), ('2layers', 1, 32, 64), ('mixed', 1, 32, 64), ('meta', 1, 32, 64), ('baseline', 1, 32, 64),
           ('1layer', 2, 40, 56)]                                           # 40 x 56: not divisible by 16


@pytest.mark.parametrize('kind,n,h,w', CONFIGS)
def test_two_handles_give_the_same_bits(kind, n, h, w):
    assert_same_bits(first_run(kind, n, h, w), three_steps(kind, n, h, w))


@pytest.mark.parametrize('kind', ['1layer', 'mixed'])
def test_graph_replay_gives_the_same_bits(kind):
    """the same three steps with "graph" 1: the second call on replays"""
    assert_same_bits(first_run(kind, 1, 32, 64), three_steps(kind, 1, 32, 64, graph=1))


def test_same_frame_twice_in_a_batch():
    n, h, w = 2, 32, 64
    eng, ad = make('1layer', n, h, w)
    raw, image1, sparse = [torch.from_numpy(np.concatenate((x, x))).cuda() for x in nlspn_frame(0, h, w, 1)]
    eng.step(image1, sparse, loss_image=raw)
    for name in ('goff9', 'gaff9'):
        t = eng.debug_tensor(name).view(2, -1)
        assert float(t.abs().sum()) > 0 and torch.equal(t[0], t[1]), name
    eng.close()


def test_step_matches_golden_with_the_option(golden_dir):
    """tests/test_gpu_nlspn.py test_step_matches_golden on the nlspn_32x64_legacy fixture, its TOL['default'] bounds unchanged"""
    tol = TOL['default']
    g = np.load(os.path.join(golden_dir, 'nlspn_32x64_legacy.npz'))
    h, w, n, steps = [int(x) for x in g['meta']]
    lr, b1, b2, eps, wd, w_sd, w_sm, w_cos, mid = [float(x) for x in g['hp']]
    hp = dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, w_sparse_depth=w_sd, w_smoothness=w_sm, w_cos=w_cos, max_input_depth=mid)
    eng, sd, adapted = make_nlspn(n, h, w, dict(hp, options={'deterministic': 1}), legacy=bool(int(g['legacy'])))       # Engine(options=...) -> set_option
    assert eng.get_option('deterministic') == 1
    names = [str(x) for x in g['adapted_names']]
    assert eng.adapted == names
    for s in range(steps):
        raw, image1, sparse = [torch.from_numpy(x).cuda() for x in nlspn_frame(s, h, w, n)]
        info, depth = eng.step(image1, sparse, loss_image=raw, want_depth=True)
        p = 's%d/' % s
        assert rel_mae(depth, g[p + 'depth_train']) < (tol['depth'] if s == 0 else 1e-3)
        np.testing.assert_allclose(info.cpu().numpy(), g[p + 'loss_info'], rtol=2e-3)
        if s == 0:
            gn = np.array([float(eng.grad(k, adapted[k][0]).double().norm()) for k in names])
            np.testing.assert_allclose(gn, g[p + 'grad_norms'], rtol=tol['gnorm'], atol=1e-6)
            for key in g.files:
                if key.startswith(p + 'grad/'):
                    k = key[len(p + 'grad/'):]
                    assert rel_mae(eng.grad(k, adapted[k][0]), g[key]) < tol['grad'], k
                    assert rel_mae(adapted[k][0], g[p + 'param/' + k]) < tol['param'], k
        d_eval = eng.forward_eval(image1, sparse)
        assert rel_mae(d_eval, g[p + 'depth_eval']) < 1e-3
    eng.close()


def test_refusals_and_range():
    """-38 with a reason where the step has no float atomics or no backward; -22 out of range; get returns what was set"""
    refused = [Engine(1, 32, 48), Engine(1, 64, 96, backbone='costdcnet', max_predict_depth=8.0),
               Engine(1, 32, 64, backbone='nlspn', meta='none', adapt_mode='meta')]
    for eng in refused:
        assert eng.lib.ptta_set_option(eng.handle, b'deterministic', 1) == -38
        assert 'deterministic' in eng.lib.ptta_last_error(eng.handle).decode()
        with pytest.raises(RuntimeError):
            eng.get_option('deterministic')
        eng.close()
    eng = Engine(1, 32, 64, backbone='nlspn', **HP)
    assert eng.lib.ptta_set_option(eng.handle, b'deterministic', 2) == -22 and eng.lib.ptta_set_option(eng.handle, b'deterministic', -1) == -22
    assert 'out of range' in eng.lib.ptta_last_error(eng.handle).decode()
    for v in (0, 1, 1, 0, 1):
        eng.set_option('deterministic', v)
        assert eng.get_option('deterministic') == v
    eng.close()
    eng = Engine(1, 32, 64, backbone='nlspn', syncbn_adapted=True, **HP)               # PTTA_NLSPN_SYNCBN_ADAPT
    eng.set_option('deterministic', 1)
    assert eng.get_option('deterministic') == 1
    eng.close()


def _facade(deterministic):
    from proxytta.model import ExternalModel_Adapt
    model = ExternalModel_Adapt('nlspn', 0.0, 80.0, max_input_depth=80.0, device=torch.device('cuda'))
    model._prepare_head('meta_selfsup_seq_1layer_ema')
    model.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.formula_state_dict_nlspn().items()})
    opt = torch.optim.Adam(model.adapt_parameters(mode='meta_bn'), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    model.model.bind_optimizer(opt)
    model.model.set_hparams(w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1)
    model.model.fill_holes = False
    assert model.model.deterministic is False                                # the default, beside fill_holes
    model.model.deterministic = deterministic
    return model


def _frame(s, h=32, w=64):
    return [torch.from_numpy(x).cuda() for x in nlspn_frame(s, h, w, 1)]


def test_facade_attribute_reaches_the_engines():
    model = _facade(False)
    raw, image1, sparse = _frame(0)
    model.adapt(image1, sparse, loss_image=raw)
    engines = model.model._engines
    assert [e.get_option('deterministic') for e in engines.values()] == [0]
    model.model.deterministic = True                                         # reaches the live engine ...
    assert [e.get_option('deterministic') for e in engines.values()] == [1]
    raw, image1, sparse = _frame(0, 40, 56)
    model.adapt(image1, sparse, loss_image=raw)                              # ... and every engine created from then on
    assert [e.get_option('deterministic') for e in engines.values()] == [1, 1]


def test_facade_runs_are_bitwise_equal():
    """two adapt() runs of two frames with the attribute set: the same depth, bit for bit"""
    runs = []
    for _ in range(2):
        model = _facade(True)
        out = []
        for s in range(2):
            raw, image1, sparse = _frame(s)
            out.append(model.adapt(image1, sparse, loss_image=raw)[0].clone())
        runs.append(out)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
