"""ptta_inpaint_biharmonic (csrc/inpaint.hip), proxytta.inpaint.inpainting_device and NlspnModel_Adapt.fill_holes = 'device' on the GPU
against the host code proxytta/inpaint.py on the cases of tests/inpaint_cases.py (tests/test_inpaint_cases_cpu.py holds the properties
of those cases that the checks below lean on).

Bound on the filled pixels: both sides solve in fp64 and round once to fp32, so they differ by a value that sits next to a rounding
boundary: numpy CG in the kernel's arithmetic is 0 - 1 ulp from the host code on these cases (test_inpaint_cases_cpu.py).  Measured on
MI355X over all cases: 1 ulp (profiles/inpaint_device.txt); asserted: max(2, 2 x measured) = 2 ulps."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import inpaint_cases as C

pytestmark = pytest.mark.gpu

ULP_BOUND = 2
LOSS_TYPE = 'adapt_meta_selfsup_seq_ema_reverse'


def device_fill(depth, max_unknowns=65536, max_iter=2000, rtol=1e-12):
    """depth: N x H x W fp32 numpy -> (filled N x H x W numpy, status list) through the C entry point."""
    from proxytta import _lib
    lib = _lib.load()
    n, h, w = depth.shape
    t = torch.from_numpy(np.array(depth, np.float32)).cuda().reshape(n, 1, h, w)       # a copy: the cases are read-only
    size = lib.ptta_inpaint_scratch_bytes(n, h, w, max_unknowns)
    assert size > 0
    scratch = torch.empty((size + 7) // 8, device='cuda', dtype=torch.float64)
    status = torch.full((n,), 77, device='cuda', dtype=torch.int32)
    rc = lib.ptta_inpaint_biharmonic(_lib.ptr(t), n, h, w, max_unknowns, max_iter, rtol, _lib.ptr(scratch), scratch.numel() * 8, _lib.ptr(status),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return t.cpu().numpy().reshape(n, h, w), status.cpu().tolist()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


@pytest.mark.parametrize('name', C.NAMES)
def test_case_matches_the_host_code(name):
    _, m, d = C.case(name)
    want = C.expected(name)
    out, status = device_fill(d[None])
    out = out[0]
    assert same_bits(out[~m], d[~m])
    assert not (out == 0).any()
    worst = int(C.ulps(out[m], want[m]).max())
    print('inpaint %s: %d unknowns, status %d, %d ulps' % (name, int(m.sum()), status[0], worst))
    assert 0 < status[0] <= 2000
    assert worst <= ULP_BOUND


def test_batch_of_four_takes_limits_and_status_per_sample():
    clean = C.field(16, 24, 40, scale=0.1)
    _, m1, d1 = C.case('random90')
    _, m3, d3 = C.case('big12x18', 10.0, 100.0)
    batch = np.stack([clean, d1, np.zeros((16, 24), np.float32), d3])
    assert clean.max() < d1[~m1].min() and d1[~m1].max() < d3[~m3].min()        # a limit taken over the batch would move random90's clipped values
    out, status = device_fill(batch)
    print('inpaint batch status', status)
    assert status[0] == 0 and status[1] > 0 and status[2] == -2 and status[3] > 0
    assert same_bits(out[0], batch[0]) and same_bits(out[2], batch[2])
    for i, (m, name, args) in ((1, (m1, 'random90', ())), (3, (m3, 'big12x18', (10.0, 100.0)))):
        want = C.expected(name, *args)
        assert same_bits(out[i][~m], batch[i][~m])
        assert int(C.ulps(out[i][m], want[m]).max()) <= ULP_BOUND


def test_not_converged_leaves_the_map_and_the_facade_falls_back_to_the_host():
    from proxytta.inpaint import inpainting_device
    _, m, d = C.case('big12x18')
    out, status = device_fill(d[None], max_iter=5)
    assert status == [-1] and same_bits(out[0], d)
    t = torch.from_numpy(d.copy()).cuda().reshape(1, 1, 16, 24)
    got = inpainting_device(t, max_iter=5)
    assert got is t and inpainting_device.last_status == [-1]
    assert same_bits(t.cpu().numpy()[0, 0], C.expected('big12x18'))


def test_too_many_unknowns_leaves_the_map():
    _, m, d = C.case('random30')
    out, status = device_fill(d[None], max_unknowns=8)
    assert status == [-3] and same_bits(out[0], d)


@pytest.mark.parametrize('name', ['checkerboard48', 'blob32'])
def test_two_runs_are_bit_identical(name):
    _, m, d = C.case(name)
    a, sa = device_fill(d[None])
    b, sb = device_fill(d[None])
    assert sa == sb and sa[0] > 0 and same_bits(a, b)


def test_refused_arguments_touch_nothing():
    from proxytta import _lib
    lib = _lib.load()
    _, m, d = C.case('random30')
    n, h, w, mu = 1, 16, 24, 128
    assert int(m.sum()) <= mu
    t = torch.from_numpy(d.copy()).cuda().reshape(1, 1, h, w)
    size = lib.ptta_inpaint_scratch_bytes(n, h, w, mu)
    scratch = torch.zeros((size + 7) // 8, device='cuda', dtype=torch.float64)
    status = torch.full((n,), 77, device='cuda', dtype=torch.int32)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(depth=_lib.ptr(t), n=n, h=h, w=w, mu=mu, it=100, rtol=1e-12, scratch=_lib.ptr(scratch), bytes=scratch.numel() * 8, status=_lib.ptr(status))
    bad = [dict(depth=None), dict(scratch=None), dict(status=None), dict(n=0), dict(h=4), dict(w=4), dict(mu=0), dict(it=0), dict(rtol=0.0),
           dict(rtol=-1e-12), dict(rtol=math.inf), dict(rtol=math.nan), dict(bytes=size - 1), dict(bytes=0)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.ptta_inpaint_biharmonic(a['depth'], a['n'], a['h'], a['w'], a['mu'], a['it'], a['rtol'], a['scratch'], a['bytes'], a['status'], stream)
        assert rc == -22, change
    torch.cuda.synchronize()
    assert same_bits(t.cpu().numpy()[0, 0], d) and status.cpu().tolist() == [77] and not bool(scratch.any())
    a = good
    assert lib.ptta_inpaint_biharmonic(a['depth'], a['n'], a['h'], a['w'], a['mu'], a['it'], a['rtol'], a['scratch'], a['bytes'], a['status'], stream) == 0
    torch.cuda.synchronize()
    assert status.cpu().tolist()[0] > 0


def test_facade_fills_on_the_device(golden_dir, monkeypatch):
    """The set-up of tests/test_gpu_nlspn.py::test_eval_forward_fills_holes_like_the_reference (same fixture, same frame) with
    fill_holes = 'device': the filled map never passes through the host code."""
    import proxytta.inpaint as inpaint_mod
    from proxytta import synth
    from proxytta.model import ExternalModel_Adapt
    from tests.test_gpu_nlspn import nlspn_frame
    g = np.load(os.path.join(golden_dir, 'nlspn_228x304_legacy.npz'))
    h, w, n, steps = [int(x) for x in g['meta']]
    lr, b1, b2, eps, wd, w_sd, w_sm, w_cos, mid = [float(x) for x in g['hp']]
    model = ExternalModel_Adapt('nlspn', 0.0, 80.0, max_input_depth=mid, offset=True, device=torch.device('cuda'))
    model._prepare_head('meta_selfsup_seq_1layer_ema')
    model.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.formula_state_dict_nlspn().items()})
    params = model.adapt_parameters(mode='meta_bn')
    opt = torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    model.model.bind_optimizer(opt)
    model.model.set_hparams(w_sparse_depth=w_sd, w_smoothness=w_sm, w_cos=w_cos)
    raw, image1, sparse = [torch.from_numpy(x).cuda() for x in nlspn_frame(0, h, w, n)]
    model.train()
    model.step(image1, sparse, loss_image=raw)
    model.eval()
    assert model.model.fill_holes is True                      # the default is the host path
    model.model.fill_holes = False
    d_raw = model.forward(image1, sparse, loss_type=LOSS_TYPE).clone()
    model.model.fill_holes = True
    d_host = model.forward(image1, sparse, loss_type=LOSS_TYPE).clone()
    holes = d_raw == 0
    assert int(holes.sum()) == int(g['s0/n_zero_eval']) >= 1
    assert not bool((d_host == 0).any()) and torch.equal(d_host[~holes], d_raw[~holes])

    def refuse(*a, **k):
        raise AssertionError('the host code ran')
    monkeypatch.setattr(inpaint_mod, 'inpaint_biharmonic', refuse)
    model.model.fill_holes = 'device'
    d_dev = model.forward(image1, sparse, loss_type=LOSS_TYPE)
    monkeypatch.undo()
    assert all(s > 0 for s in inpaint_mod.inpainting_device.last_status)
    assert not bool((d_dev == 0).any())
    assert torch.equal(d_dev[~holes], d_raw[~holes])
    worst = int(C.ulps(d_dev[holes].cpu().numpy(), d_host[holes].cpu().numpy()).max())
    print('inpaint facade 228x304: status %s, %d ulps' % (inpaint_mod.inpainting_device.last_status, worst))
    assert worst <= ULP_BOUND
    model.model.fill_holes = False
    assert torch.equal(model.forward(image1, sparse, loss_type=LOSS_TYPE), d_raw)
