"""Weight gradient of a stride-1 3x3 convolution at the wide channel pairs of the 2layers meta block on NLSPN (48 <-> 256) and
CostDCNet (16 -> 64): the bf16x3 form (gwgrad_mfma.hip gwgrad_x3_kernel, WIDE) through ptta_op_gwgrad against an fp64 torch weight
gradient, against the fp32-MFMA form it replaces, and bitwise across runs (fixed-order reduction, no atomics)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDE = [(16, 64), (48, 256), (256, 48)]
# general multiples of 16 up to 256 with more than one 32 x 32 tile pair: three pairs (one wave of the block idle), a ragged last group
# of four, 256 x 256
GENERAL = [(16, 96), (80, 48), (256, 256)]
MAPS = [(1, 24, 40), (2, 17, 37)]         # batch 2 with odd H and W (a ragged 16-pixel item in every row)


def _ref(x, gy):
    """fp64 weight and bias gradient of Conv2d(ci, co, 3, padding=1) on NHWC maps, on the CPU."""
    xd = x.detach().cpu().double().permute(0, 3, 1, 2)
    gd = gy.detach().cpu().double().permute(0, 3, 1, 2)
    gw = torch.nn.grad.conv2d_weight(xd, (gd.shape[1], xd.shape[1], 3, 3), gd, padding=1)
    return gw, gd.sum(dim=(0, 2, 3))


def _maps(b, h, w, ci, co, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, h, w, ci, generator=g)
    gy = torch.randn(b, h, w, co, generator=g) * 1e-2
    return x.cuda(), gy.cuda()


def _err(got, ref):
    return float((got.cpu().double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize('ci,co', WIDE + GENERAL)
@pytest.mark.parametrize('b,h,w', MAPS)
def test_gwgrad_wide_against_fp64(ci, co, b, h, w):
    from proxytta.engine import op_gwgrad
    x, gy = _maps(b, h, w, ci, co, seed=ci * 1000 + co + h)
    rw, rb = _ref(x, gy)
    gw, gb, _ = op_gwgrad(x, gy)
    fw, fb, _ = op_gwgrad(x, gy, impl='fp32_mfma')
    ew, eb = _err(gw, rw), _err(gb, rb)
    print('%d -> %d %dx%dx%d: bf16x3 weight %.2e bias %.2e, fp32-MFMA weight %.2e' % (ci, co, b, h, w, ew, eb, _err(fw, rw)))
    # bounds ~2x the largest error measured over these cases (bf16x3 weight 5.6e-6, bias 8.9e-8; fp32-MFMA weight 3.1e-7)
    assert ew < 1.2e-5 and eb < 2e-7
    assert _err(fw, rw) < 7e-7
    # the launcher takes the bf16x3 form at these shapes, not the fp32-MFMA one
    assert not torch.equal(gw, fw)


@pytest.mark.parametrize('ci,co', [(48, 256), (256, 48)])
def test_gwgrad_wide_many_items(ci, co):
    """A map with more items than the launch has blocks (each wave loops over items, both register sets of the pipeline in use)."""
    from proxytta.engine import op_gwgrad
    x, gy = _maps(1, 96, 328, ci, co, seed=7 + ci)
    rw, rb = _ref(x, gy)
    gw, gb, _ = op_gwgrad(x, gy)
    ew, eb = _err(gw, rw), _err(gb, rb)
    print('%d -> %d 96x328: bf16x3 weight %.2e bias %.2e' % (ci, co, ew, eb))
    assert ew < 1.2e-5 and eb < 4e-7                 # measured 4.7e-6 / 1.8e-7


@pytest.mark.parametrize('ci,co', WIDE)
def test_gwgrad_wide_bitwise_across_runs(ci, co):
    from proxytta.engine import op_gwgrad
    x, gy = _maps(2, 17, 37, ci, co, seed=3)
    a = op_gwgrad(x, gy)
    b = op_gwgrad(x, gy)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# the narrow bf16x3 forms (gwgrad_x3_kernel without WIDE): one tile pair with one partial per block (the second with a partly empty input
# tile), 2 x 2 pairs, 1 x 4 and 4 x 1
NARROW = [(32, 32), (24, 32), (48, 48), (64, 64), (32, 128), (128, 32)]


@pytest.mark.parametrize('ci,co', NARROW)
@pytest.mark.parametrize('b,h,w', MAPS)
def test_gwgrad_narrow_forms(ci, co, b, h, w):
    from proxytta.engine import op_gwgrad
    x, gy = _maps(b, h, w, ci, co, seed=ci * 1000 + co + h)
    rw, rb = _ref(x, gy)
    gw, gb, _ = op_gwgrad(x, gy)
    gw2, gb2, _ = op_gwgrad(x, gy)
    fw, fb, _ = op_gwgrad(x, gy, impl='fp32_mfma')
    ew, eb = _err(gw, rw), _err(gb, rb)
    print('%d -> %d %dx%dx%d: bf16x3 narrow weight %.2e bias %.2e' % (ci, co, b, h, w, ew, eb))
    # bounds: twice the largest error of its kind over these twelve cases, measured on the build before the launcher was rewritten
    # (profiles/gconv_split.txt: weight 5.824e-6 at 24 -> 32 1x24x40, bias 1.096e-7 at the same case)
    assert ew < 2 * 5.824e-6 and eb < 2 * 1.096e-7
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)
    # the launcher takes a bf16x3 form at these shapes, not the fp32-MFMA one
    assert not torch.equal(gw, fw)


def test_gwgrad_naive_form_agrees():
    """PTTA_CONV_IMPL=naive's direct fp32 weight gradient at a wide pair, through the same entry point."""
    from proxytta.engine import op_gwgrad
    x, gy = _maps(1, 9, 21, 48, 256, seed=11)
    rw, rb = _ref(x, gy)
    nw, nb, _ = op_gwgrad(x, gy, impl='naive')
    assert _err(nw, rw) < 1e-6 and _err(nb, rb) < 1e-6


@pytest.mark.parametrize('ci,co', [(16, 16), (16, 32)])
def test_single_pair_16_channel_shapes_keep_fp32_mfma(ci, co):
    """One 32 x 32 tile pair with 16 input channels (CostDCNet's 1layer Conv2d(16, 16, 3)) stays on the fp32-MFMA form: bitwise the same."""
    from proxytta.engine import op_gwgrad
    x, gy = _maps(1, 20, 36, ci, co, seed=5)
    gw, gb, _ = op_gwgrad(x, gy)
    fw, fb, _ = op_gwgrad(x, gy, impl='fp32_mfma')
    assert torch.equal(gw, fw) and torch.equal(gb, fb)


def test_gwgrad_rejects_bad_arguments():
    from proxytta import _lib
    from proxytta.engine import op_gwgrad
    x, gy = _maps(1, 8, 8, 16, 272, seed=1)
    with pytest.raises(RuntimeError):
        op_gwgrad(x, gy)                  # more than 256 output channels
    lib = _lib.load()
    assert lib.ptta_op_gwgrad(None, None, None, None, 1, 8, 8, 16, 64, 0, 0, None, None) == -22
