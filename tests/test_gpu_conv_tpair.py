"""A transposed 32 -> 32 convolution and the stride-1 convolution behind it as ONE launch (csrc/conv_tpair.hip, option "tpair_fuse").

The one-launch form runs the same products in the same order as the two kernels it replaces, so everything is compared with torch.equal,
never with a tolerance: per pair through ptta_op_conv32_tpair (final map, sum, the first half's map and sign-bit words) in both tile forms
(1 = 4 x 32 one-tile blocks, 2 = persistent 8 x 32 tiles), and the whole step with the option off against on (loss terms, depth, adapted
parameters, both Adam moments).  Every test also asserts that the one-launch form really ran.

Instantiated: the forward's form -- ReLU on both inputs, first half without epilogue operands, second half with zero, one or two skip
addends and map and / or sum output, fp32 (bf16x3) and narrow maps -- and the narrow data gradients' form (hi + lo weights, no ReLU, first
half masked by sign-bit words and summed with an addend, second half reading that SUM and masked).  Every other combination takes the
two launches (fused_host = 0), which the last per-pair test pins down."""
import ctypes

import pytest
import torch

from proxytta import _lib, synth
from tests.util import make_engine

pytestmark = pytest.mark.gpu
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, w_sparse_depth=1.0, w_smoothness=2.0, w_cos=0.1,
          max_input_depth=80.0)
S2, T2 = 1, 2


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _dtype_code(name):
    return {'fp32': 0, 'bf16': 1}[name]                      # PTTA_DTYPE_F32 / any other value: narrow maps


def _tpair(x, w1, b1, w2, b2, up, a1, a2, b, in_nb, dtype, fused, form=0, max_blocks=0, want_raw=True, want_mid=True, mode=T2, relu=True,
           w2form=False, a0=None, m1=None, m2=None):
    lib = _lib.load()
    hin, win = x.shape[1], x.shape[2]
    hm, wm = (2 * hin, 2 * win) if mode == T2 else (hin // 2, win // 2)
    out_raw = torch.full((b, hm, wm, 32), float('nan'), device='cuda') if want_raw else None
    out_sum = torch.full((b, hm, wm, 32), float('nan'), device='cuda') if (a1 is not None or not want_raw) else None
    mid = torch.full((b, hm, wm, 32), float('nan'), device='cuda') if want_mid else None
    mid_sum = torch.full((b, hm, wm, 32), float('nan'), device='cuda') if a0 is not None else None
    bits = torch.full((b, hm, wm), -1, dtype=torch.int32, device='cuda') if dtype == 'fp32' else None
    did = ctypes.c_int(-1)
    rc = lib.ptta_op_conv32_tpair(_ptr(x), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(up), _ptr(a0), _ptr(a1), _ptr(a2), _ptr(m1), _ptr(m2),
                                  _ptr(out_raw), _ptr(out_sum), _ptr(mid), _ptr(mid_sum), _ptr(bits), b, in_nb, hin, win, mode, int(relu),
                                  int(relu), 1 if mode == T2 else 0, 0, _dtype_code(dtype), int(w2form), int(fused), int(form), int(max_blocks),
                                  ctypes.byref(did), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    return {'raw': out_raw, 'sum': out_sum, 'mid': mid, 'mid_sum': mid_sum, 'bits': bits}, did.value


def _operands(hin, win, b, in_nb, nadd, seed, constant=False, up=False, mode=T2):
    g = torch.Generator().manual_seed(seed)
    hm, wm = (2 * hin, 2 * win) if mode == T2 else (hin // 2, win // 2)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).cuda().contiguous()
    x = torch.full((in_nb, hin, win, 32), 0.75).cuda() if constant else rnd(in_nb, hin, win, 32)       # negative values: ReLU bites
    w1, w2 = rnd(32, 32, 3, 3, scale=0.08), rnd(32, 32, 3, 3, scale=0.08)
    b1, b2 = rnd(32, scale=0.3), rnd(32, scale=0.3)
    upm = rnd(b, hm // 2, wm // 2, 32) if up else None
    a1 = rnd(b, hm, wm, 32) if nadd >= 1 else None
    a2 = rnd(b, hm, wm, 32) if nadd >= 2 else None
    return x, w1, b1, w2, b2, upm, a1, a2


def _same(ref, got, what):
    for k in ref:
        if ref[k] is None or got[k] is None:
            continue
        assert not torch.isnan(ref[k]).any() if ref[k].is_floating_point() else True, (what, k, 'the two-launch form left a pixel unwritten')
        assert torch.equal(ref[k], got[k]), (what, k, int((ref[k] != got[k]).sum()), 'elements differ')


# input sizes (the intermediate is twice as large): 2x3 -> 4x6 one partial tile with all four borders inside it; 9x35 -> 18x70 a partial last
# tile row in both tile heights, three tile columns with a seam at 32 and a partial last one, halos recomputed on both sides; 11x38 -> 22x76
# the headline's real 1/16 -> 1/8 map
SIZES = [(2, 3), (9, 35), (11, 38)]

_REF = {}


def _reference(size, nadd, dtype):
    """The two-launch result of a per-pair case: computed once, shared by both forms."""
    key = (size, nadd, dtype)
    if key not in _REF:
        ops = _operands(size[0], size[1], 1, 1, nadd, seed=size[0] * 1000 + size[1] + nadd)
        ref, d0 = _tpair(*ops, 1, 1, dtype, fused=0)
        assert d0 == 0
        _REF[key] = (ops, ref)
    return _REF[key]


@pytest.mark.parametrize('form', [1, 2])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('nadd', [0, 1, 2])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_transposed_pair_fused_equals_two_launches(size, nadd, dtype, form):
    ops, ref = _reference(size, nadd, dtype)
    got, d1 = _tpair(*ops, 1, 1, dtype, fused=1, form=form)
    assert d1 == 1, 'the one-launch form did not run'
    _same(ref, got, (size, nadd, dtype, form))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_persistent_blocks_walk_several_tiles(dtype):
    """18 x 70 intermediate = 3 x 3 tiles of 8 x 32: two blocks walk four and five tiles each, so the next tile's window prefetch and the
    reuse of the LDS region (window + weights, then halo tile) across tiles are exercised; the 4 x 32 form likewise with 15 tiles."""
    ops, ref = _reference((9, 35), 2, dtype)
    for form in (2, 1):
        got, d1 = _tpair(*ops, 1, 1, dtype, fused=1, form=form, max_blocks=2)
        assert d1 == 1
        _same(ref, got, (dtype, form))
    got, d1 = _tpair(*ops, 1, 1, dtype, fused=1, form=0)           # as the step would choose: a small map, the 4 x 32 form
    assert d1 == 1
    _same(ref, got, (dtype, 0))


@pytest.mark.parametrize('form', [1, 2])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_frames_sharing_one_input_frame_sum_only_output_and_unwritten_map(dtype, form):
    """B = 2 frames reading ONE input frame (in_nb = 1) with per-frame addends; the sum-only output form; and the first half's map not
    wanted (the step's default: nothing reads it), where the sign-bit words must still be written.  With the map not wanted the hook itself
    checks that the one-launch form left the map's buffer untouched (its 0xff fill; -14 otherwise), so rc == 0 in _tpair covers that."""
    ops = _operands(9, 35, 2, 1, 2, seed=7)
    for want_raw in (True, False):
        ref, d0 = _tpair(*ops, 2, 1, dtype, fused=0, want_raw=want_raw)
        for want_mid in (True, False):
            got, d1 = _tpair(*ops, 2, 1, dtype, fused=1, form=form, want_raw=want_raw, want_mid=want_mid)
            assert d0 == 0 and d1 == 1
            _same(ref, got, (dtype, want_raw, want_mid))
            if dtype == 'fp32':
                assert torch.equal(ref['bits'], got['bits'])
    assert torch.equal(ref['mid'][0], ref['mid'][1])                    # one input frame ...
    assert not torch.equal(got['sum'][0], got['sum'][1])                # ... different addends per frame: the frames are not copies


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_constant_input_exposes_the_zero_padding_of_the_intermediate(dtype):
    """A constant non-zero input makes the first convolution non-zero OUTSIDE the map too (bias, border taps): the second convolution must
    still see zeros there, not the first one evaluated on out-of-range inputs."""
    for size in ((2, 3), (9, 35)):
        ops = _operands(size[0], size[1], 1, 1, 0, seed=3, constant=True)
        ref, _ = _tpair(*ops, 1, 1, dtype, fused=0)
        for form in (1, 2):
            got, d1 = _tpair(*ops, 1, 1, dtype, fused=1, form=form)
            assert d1 == 1
            _same(ref, got, (dtype, size, form))


def _dg_case(size, b, in_nb):
    hin, win = size
    x, w1, _, w2, _, _, a0, _ = _operands(hin, win, b, in_nb, 1, seed=hin * 77 + win + b)
    g = torch.Generator().manual_seed(hin + 5 * win)
    m1 = torch.randint(-2 ** 31, 2 ** 31 - 1, (b, 2 * hin, 2 * win), generator=g, dtype=torch.int64).to(torch.int32).cuda()
    m2 = torch.randint(-2 ** 31, 2 ** 31 - 1, (b, 2 * hin, 2 * win), generator=g, dtype=torch.int64).to(torch.int32).cuda()
    return (x, w1, None, w2, None, None, None, None, b, in_nb, 'bf16'), dict(relu=False, w2form=True, a0=a0, m1=m1, m2=m2)


@pytest.mark.parametrize('b_in', [(1, 1), (2, 1)], ids=['B1', 'B2_one_input_frame'])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_data_gradient_pair_fused_equals_two_launches(size, b_in):
    """The mixed mode's data gradients: narrow maps, weights as hi + lo, no ReLU; the first half masked by sign-bit words and summed with
    an addend, the second half reading that SUM and masked in turn.  Random mask words (about half of the channels pass) and negative
    values everywhere, so the masks bite; the first half's mask and addend are needed on the halo pixels too.  Both tile forms, and the
    persistent form with two blocks walking all tiles."""
    args, kw = _dg_case(size, *b_in)
    ref, d0 = _tpair(*args, fused=0, **kw)
    assert d0 == 0
    assert float(ref['raw'].abs().max()) > 0 and float((ref['raw'] == 0).float().mean()) > 0.2      # the masks bite
    for form, max_blocks in ((1, 0), (2, 0), (2, 2)):
        got, d1 = _tpair(*args, fused=1, form=form, max_blocks=max_blocks, **kw)
        assert d1 == 1, 'the one-launch form did not run'
        _same(ref, got, (size, b_in, form, max_blocks))


def test_data_gradient_pair_on_a_map_of_more_than_one_tile_per_block_takes_the_two_launches_by_itself():
    """Form 0 is the step's choice: the data gradients' one-launch form measured slower than the two launches where a block walks several
    tiles (more than 480 tiles of 8 x 32; here 13 x 37 = 481), so there the step keeps the two launches; asked for by name it still runs."""
    args, kw = _dg_case((52, 592), 1, 1)
    ref, d0 = _tpair(*args, fused=0, **kw)
    got, d1 = _tpair(*args, fused=1, form=0, **kw)
    assert d0 == 0 and d1 == 0
    _same(ref, got, 'form 0')
    got, d1 = _tpair(*args, fused=1, form=2, **kw)
    assert d1 == 1
    _same(ref, got, 'form 2')


def test_forms_that_are_not_instantiated_take_the_two_launches():
    hin, win = 9, 13
    # ReLU off; a bilinear skip on the second half; a stride-2 first half (conv_pair.hip's, not this hook's)
    cases = [dict(relu=False, up=False, dtype='fp32', mode=T2), dict(relu=True, up=True, dtype='bf16', mode=T2),
             dict(relu=True, up=True, dtype='fp32', mode=S2)]
    for cs in cases:
        h_in, w_in = (hin, win) if cs['mode'] == T2 else (4 * hin, 4 * win)
        ops = _operands(h_in, w_in, 1, 1, 1, seed=11, up=cs['up'], mode=cs['mode'])
        for form in (0, 1, 2):
            ref, d0 = _tpair(*ops, 1, 1, cs['dtype'], fused=0, mode=cs['mode'], relu=cs['relu'])
            got, d1 = _tpair(*ops, 1, 1, cs['dtype'], fused=1, form=form, mode=cs['mode'], relu=cs['relu'])
            assert d0 == 0 and d1 == 0, cs
            _same(ref, got, cs)
    # the data gradients' weights (hi + lo) WITHOUT their masks / sum
    x, w1, _, w2, _, _, _, _ = _operands(hin, win, 1, 1, 0, seed=5)
    args = (x, w1, None, w2, None, None, None, None, 1, 1, 'bf16')
    ref, d0 = _tpair(*args, fused=0, relu=False, w2form=True)
    got, d1 = _tpair(*args, fused=1, form=0, relu=False, w2form=True)
    assert d0 == 0 and d1 == 0
    _same(ref, got, 'hi + lo weights without masks')
    lib = _lib.load()
    assert lib.ptta_op_conv32_tpair(*([None] * 16), 1, 1, 2, 3, T2, 1, 1, 1, 0, 0, 0, 1, 3, 0, None, None) == -22     # form out of range
    assert lib.ptta_op_conv32_tpair(*([None] * 16), 1, 1, 2, 3, T2, 1, 1, 1, 0, 0, 0, 1, 0, -1, None, None) == -22    # max_blocks < 0


def _frames(n, h, w, k=3):
    return [[torch.from_numpy(x).cuda() for x in synth.synthetic_frame(40 + i, h, w, n)] for i in range(k)]


def _run(options, n, h, w, frames, pipelined, dtype, meta='1layer'):
    eng, sd, ad = make_engine(n, h, w, dtype, HP, meta=meta, options=options)
    out, counts = [], []
    for i, (im, sp) in enumerate(frames):
        if pipelined:
            info, depth = eng.step(im, sp, want_depth=True, next_frame=frames[min(i + 1, len(frames) - 1)])
        else:
            info, depth = eng.step(im, sp, want_depth=True)
        out.append((info.clone(), depth.clone()))
        counts.append(eng.get_option('tpair_fuse_count'))
    torch.cuda.synchronize()
    params = {k: [t.clone() for t in v] for k, v in ad.items()}
    eng.close()
    return out, params, counts


def _steps_equal(off, on):
    (o0, p0, c0), (o1, p1, c1) = off, on
    assert all(c == 0 for c in c0), c0
    assert all(c > 0 for c in c1), c1                       # (the comparison cannot pass on the fallback)
    for s, ((i0, d0), (i1, d1)) in enumerate(zip(o0, o1)):
        assert torch.equal(i0, i1) and torch.equal(d0, d1), s
    for k in p0:
        for t0, t1 in zip(p0[k], p1[k]):                    # parameter and both Adam moments
            assert torch.equal(t0, t1), k


# 64x96 and 36x52: every map small (the 4 x 32 form); 136x512: the full-resolution maps take the persistent form (272 tiles of 8 x 32)
@pytest.mark.parametrize('graph', [0, 1])
@pytest.mark.parametrize('pipelined', [False, True])
@pytest.mark.parametrize('dtype', ['fp32', 'mixed'])
@pytest.mark.parametrize('size', [(64, 96), (36, 52), (136, 512)], ids=lambda s: '%dx%d' % s)
def test_whole_step_with_transposed_pairs_fused_equals_the_two_launch_step(size, dtype, pipelined, graph):
    h, w = size
    frames = _frames(1, h, w)
    off = _run({'tpair_fuse': 0, 'graph': graph}, 1, h, w, frames, pipelined, dtype)
    on = _run({'tpair_fuse': 1, 'graph': graph}, 1, h, w, frames, pipelined, dtype)
    _steps_equal(off, on)


def test_whole_step_with_float_masks_still_writes_the_intermediate_map():
    """"mask_bits" 0: the backward masks with the float map, so the one-launch form has to write it."""
    frames = _frames(1, 64, 96)
    off = _run({'tpair_fuse': 0, 'mask_bits': 0}, 1, 64, 96, frames, False, 'fp32')
    on = _run({'tpair_fuse': 1, 'mask_bits': 0}, 1, 64, 96, frames, False, 'fp32')
    _steps_equal(off, on)


def test_whole_step_of_the_2layers_meta_block():
    frames = _frames(1, 64, 96)
    off = _run({'tpair_fuse': 0}, 1, 64, 96, frames, False, 'fp32', meta='2layers')
    on = _run({'tpair_fuse': 1}, 1, 64, 96, frames, False, 'fp32', meta='2layers')
    _steps_equal(off, on)


def test_tpair_fuse_option_keys():
    for dtype in ('fp32', 'mixed'):                          # free on mixed handles
        eng, sd, ad = make_engine(1, 64, 96, dtype, HP)
        assert eng.get_option('tpair_fuse') == 1 and eng.get_option('tpair_fuse_count') == 0
        with pytest.raises(RuntimeError, match='out of range'):
            eng.set_option('tpair_fuse', 2)
        with pytest.raises(RuntimeError, match='out of range'):
            eng.set_option('tpair_fuse', -1)
        with pytest.raises(RuntimeError, match='read-only'):
            eng.set_option('tpair_fuse_count', 1)
        im, sp = _frames(1, 64, 96, 1)[0]
        eng.step(im, sp)
        assert eng.get_option('tpair_fuse_count') > 0
        with pytest.raises(RuntimeError, match='not written'):      # the fused launch kept the map on chip: no stale read
            eng.debug_tensor('u3')
        n_pair = eng.get_option('pair_fuse_count')
        eng.set_option('tpair_fuse', 0)
        assert eng.get_option('tpair_fuse') == 0
        eng.step(im, sp)
        assert eng.get_option('tpair_fuse_count') == 0
        assert eng.debug_tensor('u3').numel() > 0 and eng.debug_tensor('t2').numel() > 0        # written again
        assert eng.get_option('pair_fuse_count') == n_pair       # the two options and their counters are independent
        eng.set_option('tpair_fuse', 1)
        eng.step(im, sp)
        assert eng.get_option('tpair_fuse_count') > 0
        torch.cuda.synchronize()
        eng.close()
