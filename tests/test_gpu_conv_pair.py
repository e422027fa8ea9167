"""A strided 32 -> 32 convolution and the stride-1 convolution behind it as ONE launch on small maps (csrc/conv_pair.hip, option "pair_fuse").

The one-launch form runs the same products in the same order as the two kernels it replaces, so everything is compared with torch.equal,
never with a tolerance: per pair through ptta_op_conv32_pair (final map, sum, the first half's map and sign-bit words), and the whole
step with the option off against on (loss terms, depth, adapted parameters, both Adam moments).

Instantiated today: first half stride 2 with ReLU on load, second half with ReLU on load and the bilinear x2 skip, with zero, one or two
skip addends, fp32 (bf16x3) and narrow maps; and the narrow data gradients' form (hi + lo weights, no ReLU, first half masked and summed
with an addend, second half masked).  The other combinations -- a transposed first half, ReLU off in the forward form, no bilinear skip,
hi + lo weights without the masks -- take the two launches (fused_host = 0), which the last per-pair test pins down so that a later stage
that instantiates one of them has to extend the comparison.  ptta_op_conv32 takes odd stride-2 input sizes (output = floor(size / 2)), so
the 19 x 27 -> 9 x 13 case is in."""
import ctypes

import numpy as np
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
    return {'fp32': 0, 'bf16': 1}[name]                      # PTTA_DTYPE_F32 / any other value: narrow maps (include/ptta.h ptta_op_conv32_pair)


def _pair(x, w1, b1, w2, b2, up, a1, a2, hm, wm, in_nb, b, mode, relu1, relu2, dtype, w2form, fused, want_raw=True, a0=None, m1=None, m2=None):
    lib = _lib.load()
    out_raw = torch.full((b, hm, wm, 32), float('nan'), device='cuda') if want_raw else None
    out_sum = torch.full((b, hm, wm, 32), float('nan'), device='cuda') if (a1 is not None or not want_raw) else None
    mid = torch.full((b, hm, wm, 32), float('nan'), device='cuda')
    mid_sum = torch.full((b, hm, wm, 32), float('nan'), device='cuda') if a0 is not None else None
    bits = torch.full((b, hm, wm), -1, dtype=torch.int32, device='cuda') if dtype == 'fp32' else None
    did = ctypes.c_int(-1)
    hin, win = x.shape[1], x.shape[2]
    rc = lib.ptta_op_conv32_pair(_ptr(x), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(up), _ptr(a0), _ptr(a1), _ptr(a2), _ptr(m1), _ptr(m2),
                                 _ptr(out_raw), _ptr(out_sum), _ptr(mid), _ptr(mid_sum), _ptr(bits), b, in_nb, hin, win, mode, int(relu1),
                                 int(relu2), 1 if mode == T2 else 0, 0, _dtype_code(dtype), int(w2form), int(fused), ctypes.byref(did),
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    return {'raw': out_raw, 'sum': out_sum, 'mid': mid, 'mid_sum': mid_sum, 'bits': bits}, did.value


def _operands(hin, win, hm, wm, b, in_nb, nadd, up, seed, constant=False):
    g = torch.Generator().manual_seed(seed)

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
        if ref[k] is None:
            assert got[k] is None
            continue
        assert not torch.isnan(ref[k]).any() if ref[k].is_floating_point() else True, (what, k, 'the two-launch form left a pixel unwritten')
        assert torch.equal(ref[k], got[k]), (what, k, int((ref[k] != got[k]).sum()), 'elements differ')


# intermediate-map sizes: 3x5 one partial tile with all four borders inside it; 9x13 and 4x6 the odd sizes of the 36x52 padded fixture's
# pyramid; 9x70 three tile rows with a partial last one and three tile columns (a seam at the tile width with halos recomputed on both
# sides, and a partial last column); 22x76 the real 1/16 map.  (hin, win) -> (hm, wm)
SIZES = [((6, 10), (3, 5)), ((18, 26), (9, 13)), ((19, 27), (9, 13)), ((8, 12), (4, 6)), ((18, 140), (9, 70)), ((44, 152), (22, 76))]


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('nadd', [0, 1, 2])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d_to_%dx%d' % (s[0] + s[1]))
def test_stride2_pair_fused_equals_two_launches(size, nadd, dtype):
    (hin, win), (hm, wm) = size
    ops = _operands(hin, win, hm, wm, 1, 1, nadd, True, seed=hin * 1000 + win + nadd)
    ref, d0 = _pair(*ops, hm, wm, 1, 1, S2, True, True, dtype, False, fused=0)
    got, d1 = _pair(*ops, hm, wm, 1, 1, S2, True, True, dtype, False, fused=1)
    assert d0 == 0 and d1 == 1, 'the one-launch form did not run'
    _same(ref, got, (size, nadd, dtype))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_sum_only_output_and_shared_input_frame(dtype):
    """B = 2 frames reading ONE input frame (in_nb = 1, the proxy pass's depth-only tensors), and the z2 = e2_2 + c3 shape: no map output
    of the second half, only the sum."""
    (hin, win), (hm, wm) = (18, 140), (9, 70)
    ops = _operands(hin, win, hm, wm, 2, 1, 1, True, seed=7)
    for want_raw in (True, False):
        ref, d0 = _pair(*ops, hm, wm, 1, 2, S2, True, True, dtype, False, fused=0, want_raw=want_raw)
        got, d1 = _pair(*ops, hm, wm, 1, 2, S2, True, True, dtype, False, fused=1, want_raw=want_raw)
        assert d0 == 0 and d1 == 1
        _same(ref, got, (dtype, want_raw))
    assert torch.equal(got['sum'][0], got['sum'][1]) is False          # (different skip operands per frame: the frames are not copies)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_constant_input_exposes_the_zero_padding_of_the_intermediate(dtype):
    """A constant non-zero input makes the first convolution non-zero OUTSIDE the map too (bias, border taps): the second convolution must
    still see zeros there, not the first one evaluated on out-of-range inputs."""
    for (hin, win), (hm, wm) in (((6, 10), (3, 5)), ((18, 140), (9, 70))):
        ops = _operands(hin, win, hm, wm, 1, 1, 0, True, seed=3, constant=True)
        ref, _ = _pair(*ops, hm, wm, 1, 1, S2, True, True, dtype, False, fused=0)
        got, d1 = _pair(*ops, hm, wm, 1, 1, S2, True, True, dtype, False, fused=1)
        assert d1 == 1
        _same(ref, got, (dtype, hm, wm))


@pytest.mark.parametrize('b_in', [(1, 1), (2, 1)], ids=['B1', 'B2_one_input_frame'])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d_to_%dx%d' % (s[0] + s[1]))
def test_data_gradient_pair_fused_equals_two_launches(size, b_in):
    """The mixed mode's data gradients: narrow maps, weights as hi + lo, no ReLU; the first half masked by sign-bit words and summed with
    an addend, the second half reading that SUM and masked in turn.  Random mask words (about half of the channels pass) and negative
    values everywhere, so the masks bite; the first half's mask and addend are needed on the halo pixels too."""
    (hin, win), (hm, wm) = size
    b, in_nb = b_in
    x, w1, _, w2, _, _, a0, _ = _operands(hin, win, hm, wm, b, in_nb, 1, False, seed=hin * 77 + win + b)
    g = torch.Generator().manual_seed(hin + 5 * win)
    m1 = torch.randint(-2 ** 31, 2 ** 31 - 1, (b, hm, wm), generator=g, dtype=torch.int64).to(torch.int32).cuda()
    m2 = torch.randint(-2 ** 31, 2 ** 31 - 1, (b, hm, wm), generator=g, dtype=torch.int64).to(torch.int32).cuda()
    args = (x, w1, None, w2, None, None, None, None, hm, wm, in_nb, b, S2, False, False, 'bf16', True)
    ref, d0 = _pair(*args, fused=0, a0=a0, m1=m1, m2=m2)
    got, d1 = _pair(*args, fused=1, a0=a0, m1=m1, m2=m2)
    assert d0 == 0 and d1 == 1, 'the one-launch form did not run'
    assert float(ref['raw'].abs().max()) > 0 and float((ref['raw'] == 0).float().mean()) > 0.2      # the masks bite
    _same(ref, got, (size, b_in))


def test_forms_that_are_not_instantiated_take_the_two_launches():
    (hin, win), (hm, wm) = (18, 26), (9, 13)
    cases = [dict(mode=S2, relu1=False, relu2=True, up=True, dtype='fp32', w2=False),       # ReLU off on the first half
             dict(mode=S2, relu1=True, relu2=False, up=True, dtype='bf16', w2=False),       # ... on the second
             dict(mode=S2, relu1=True, relu2=True, up=False, dtype='fp32', w2=False),       # no bilinear skip
             dict(mode=S2, relu1=False, relu2=False, up=False, dtype='bf16', w2=True),      # the data gradients' weights WITHOUT their masks / sum
             dict(mode=T2, relu1=True, relu2=True, up=False, dtype='fp32', w2=False)]       # transposed first half
    for cs in cases:
        h_in, w_in = (hin, win) if cs['mode'] == S2 else (hm // 2, wm // 2)
        h_m, w_m = (hm, wm) if cs['mode'] == S2 else (2 * (hm // 2), 2 * (wm // 2))
        ops = _operands(h_in, w_in, h_m, w_m, 1, 1, 1, cs['up'], seed=11)
        ref, d0 = _pair(*ops, h_m, w_m, 1, 1, cs['mode'], cs['relu1'], cs['relu2'], cs['dtype'], cs['w2'], fused=0)
        got, d1 = _pair(*ops, h_m, w_m, 1, 1, cs['mode'], cs['relu1'], cs['relu2'], cs['dtype'], cs['w2'], fused=1)
        assert d0 == 0 and d1 == 0, cs
        _same(ref, got, cs)


_MID_CACHE = {}


def _two_launch_inputs(b, hm, wm):
    """The operands of one intermediate size (two addends and a skip map, of which a case passes the ones it wants), shared by its twelve cases."""
    if (b, hm, wm) not in _MID_CACHE:
        _MID_CACHE[(b, hm, wm)] = _operands(2 * hm, 2 * wm, hm, wm, b, b, 2, True, seed=hm * 1000 + wm)
    return _MID_CACHE[(b, hm, wm)]


def _skip_ref(up, hm, wm):
    """float64 bilinear skip of the stride-1 epilogue, [b, hm >> 1, wm >> 1, 32] -> [b, hm, wm, 32]: oracle.msgchn_arith.up2_ref on an even
    map; an odd one (9 x 13 from 4 x 6) takes the same align-corners weights src = dst (n_in - 1) / (n_out - 1) in exact rationals, which
    is what the kernels' up_scale(n_in, n_out) rounds to fp32."""
    from oracle import msgchn_arith as A
    if hm % 2 == 0 and wm % 2 == 0:
        return A.up2_ref(up)[0]

    def matrix(n_in, n_out):
        U = np.zeros((n_out, n_in))
        for d in range(n_out):
            num, den = d * (n_in - 1), n_out - 1
            i0 = min(num // den, n_in - 1)
            frac = (num - i0 * den) / den
            U[d, i0] += 1.0 - frac
            U[d, min(i0 + 1, n_in - 1)] += frac
        return U
    return A._sandwich(matrix(hm // 2, hm), up, matrix(wm // 2, wm))


# second term of the bound below: eight fp32 roundings (the interpolation's products and sums, the three additions), 8 x 2^-24
STRIDE1_EPILOGUE_ROUNDINGS = 2.0 ** -21


@pytest.mark.parametrize('size', [(1, 9, 13), (2, 72, 480)], ids=['small_kernel_1x9x13', 'x3_kernel_2x72x480'])
@pytest.mark.parametrize('nadd', [0, 1, 2])
@pytest.mark.parametrize('up', [0, 1])
@pytest.mark.parametrize('relu2', [0, 1])
def test_two_launch_stride1_epilogue_forms(relu2, up, nadd, size):
    """The second launch of the two-launch chain against float64, on both sides of the small-map rule: 1x9x13 is one partial 4x32 tile
    (conv32_s1_small_kernel), 2x72x480 is 2 * 15 * 9 = 270 tiles of 8x32, more than 256 (conv32_s1_x3_kernel).  The reference starts from the
    hook's own first-layer map, so only the second launch is judged:
        conv(relu2 ? relu(mid) : mid, w2) + b2 [+ up2(up)] [+ a1] [+ a2]
    within TOL['x3'] * (|x| (*) |w| + |b|) (tests/test_gpu_parity.py _conv_bound) + 2^-21 * (|conv| + |up2| + |a1| + |a2|)."""
    from tests.gconv_cases import TOL
    from tests.test_gpu_parity import _conv_bound
    from tests.util import assert_elementwise
    b, hm, wm = size
    x, w1, b1, w2, b2, upm, a1, a2 = _two_launch_inputs(b, hm, wm)
    upm, a1, a2 = upm if up else None, a1 if nadd >= 1 else None, a2 if nadd >= 2 else None
    got, did = _pair(x, w1, b1, w2, b2, upm, a1, a2, hm, wm, b, b, S2, True, bool(relu2), 'fp32', False, fused=0)
    assert did == 0
    conv, bound = _conv_bound(got['mid'].cpu(), w2.cpu(), b2.cpu(), 0, bool(relu2), TOL['x3'])
    ref, mag = conv.numpy(), conv.abs().numpy()
    if up:
        u = _skip_ref(upm.cpu().numpy(), hm, wm)
        ref, mag = ref + u, mag + np.abs(u)
    what = 'two-launch stride-1 relu2=%d up=%d nadd=%d %s' % (relu2, up, nadd, size)
    assert_elementwise(got['raw'], ref, bound.numpy() + STRIDE1_EPILOGUE_ROUNDINGS * mag, what + ' out_raw')
    if nadd:
        for a in (a1, a2)[:nadd]:
            ref, mag = ref + a.cpu().double().numpy(), mag + a.cpu().double().abs().numpy()
        assert_elementwise(got['sum'], ref, bound.numpy() + STRIDE1_EPILOGUE_ROUNDINGS * mag, what + ' out_sum')
    else:
        assert got['sum'] is None


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
        counts.append(eng.get_option('pair_fuse_count'))
    torch.cuda.synchronize()
    params = {k: [t.clone() for t in v] for k, v in ad.items()}
    eng.close()
    return out, params, counts


@pytest.mark.parametrize('graph', [0, 1])
@pytest.mark.parametrize('pipelined', [False, True])
@pytest.mark.parametrize('dtype', ['fp32', 'mixed'])
@pytest.mark.parametrize('size', [(64, 96), (36, 52)])
def test_whole_step_with_pairs_fused_equals_the_two_launch_step(size, dtype, pipelined, graph):
    h, w = size
    frames = _frames(1, h, w)
    off, poff, coff = _run({'pair_fuse': 0, 'graph': graph}, 1, h, w, frames, pipelined, dtype)
    on, pon, con = _run({'pair_fuse': 1, 'graph': graph}, 1, h, w, frames, pipelined, dtype)
    assert all(c == 0 for c in coff), coff
    assert all(c > 0 for c in con), con                     # (the comparison cannot pass on the fallback)
    for s, ((i0, d0), (i1, d1)) in enumerate(zip(off, on)):
        assert torch.equal(i0, i1) and torch.equal(d0, d1), s
    for k in poff:
        for t0, t1 in zip(poff[k], pon[k]):                 # parameter and both Adam moments
            assert torch.equal(t0, t1), k


def test_whole_step_of_the_2layers_meta_block():
    frames = _frames(1, 64, 96)
    off, poff, coff = _run({'pair_fuse': 0}, 1, 64, 96, frames, False, 'fp32', meta='2layers')
    on, pon, con = _run({'pair_fuse': 1}, 1, 64, 96, frames, False, 'fp32', meta='2layers')
    assert all(c == 0 for c in coff) and all(c > 0 for c in con), (coff, con)
    for (i0, d0), (i1, d1) in zip(off, on):
        assert torch.equal(i0, i1) and torch.equal(d0, d1)
    for k in poff:
        for t0, t1 in zip(poff[k], pon[k]):
            assert torch.equal(t0, t1), k


def test_pair_fuse_option_keys():
    for dtype in ('fp32', 'mixed'):                          # free on mixed handles
        eng, sd, ad = make_engine(1, 64, 96, dtype, HP)
        assert eng.get_option('pair_fuse') == 1 and eng.get_option('pair_fuse_count') == 0
        with pytest.raises(RuntimeError, match='out of range'):
            eng.set_option('pair_fuse', 2)
        with pytest.raises(RuntimeError, match='out of range'):
            eng.set_option('pair_fuse', -1)
        with pytest.raises(RuntimeError, match='read-only'):
            eng.set_option('pair_fuse_count', 1)
        im, sp = _frames(1, 64, 96, 1)[0]
        eng.step(im, sp)
        assert eng.get_option('pair_fuse_count') > 0
        eng.set_option('pair_fuse', 0)
        assert eng.get_option('pair_fuse') == 0
        eng.step(im, sp)
        assert eng.get_option('pair_fuse_count') == 0
        eng.set_option('pair_fuse', 1)
        eng.step(im, sp)
        assert eng.get_option('pair_fuse_count') > 0
        torch.cuda.synchronize()
        eng.close()
