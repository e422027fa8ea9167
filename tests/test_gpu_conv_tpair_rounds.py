"""The persistent 8 x 32 form of the transposed -> stride-1 pair (csrc/conv_tpair.hip, form 2) where a block walks SEVERAL tiles: the
rounds of the tile loop -- the next window's prefetch, the skip addends requested in front of a row's matrix work, the LDS region that is
window + weights and then halo tile, the first layer's weight pieces fetched again per tile.

Every output element is compared bit for bit (torch.equal) with the two-launch form of the same library (fused = 0): the second map, its
sum, the first layer's map (and its sum, the data gradients' form) and the sign-bit words.  The fp32 and narrow forward cases are also
checked per element against the float64 convolution pair of oracle/gconv_arith.py, at the bound of that file's tests
(tests/gconv_cases.py TOL: 4 x the emulation's own error ratio, times the magnitude |x| (*) |w| + |bias| + |addends|), carried through
the pair: the first layer's bound e1 = TOL mag1 reaches the second layer's output through ReLU (slope <= 1) and |w2|, so
bound = TOL mag2 + |w2| (*) e1.  Narrow maps (one MFMA per product, TOL['x1']) also round what they store to bf16, relative 2^-9 per
rounding: the input and the stored intermediate (2 x 2^-9 mag1 more in e1), the addends and the stored output (2 x 2^-9 mag2 more).

The grid of form 2 is min(tiles, 480, max_blocks) blocks (conv_tpair.hip launch_tpair_t, kTpairBlocks; ptta_conv32_tpair_pays does not
limit the forward's form, and form 2 is asked for by name), tile t = (t % tile rows, t / tile rows): y fastest, block k walks tiles
k, k + blocks, ...  The cases, as input size -> intermediate size, tiles, blocks, tiles per block:
  51 x 577 -> 102 x 1154   13 x 37 = 481 tiles, 480 blocks: block 0 walks two tiles, every other block one -- the real grid with a partial
                           second round; the last tile row has 6 rows, the last tile column 2 pixels
  13 x 35  ->  26 x 70     4 x 3 = 12 tiles, max_blocks 5: blocks 0, 1 walk three tiles, blocks 2 - 4 two (partial third round)
  13 x 16  ->  26 x 32     4 x 1 tiles, the width exactly one tile, max_blocks 1: one block walks four VERTICAL neighbours top to bottom
   3 x 35  ->   6 x 70     1 x 3 tiles, one (partial) tile high -- top and bottom padding in the same tile; max_blocks 2: two tiles and one
each with zero, one and two skip addends (fp32); the 26 x 70 case once more with narrow maps, forward and data-gradient form."""
import pytest
import torch
import torch.nn.functional as F

from oracle import gconv_arith as A
from tests.gconv_cases import TOL
from tests.test_gpu_conv_tpair import _dg_case, _operands, _same, _tpair
from tests.util import assert_elementwise

pytestmark = pytest.mark.gpu
K_BLOCKS = 480                                               # conv_tpair.hip kTpairBlocks

# (input rows, input columns, max_blocks, expected tiles, expected blocks, expected tiles of the busiest and the idlest block)
CASES = {
    'real_grid_481_tiles': (51, 577, 0, 481, 480, 2, 1),
    'three_rounds_partial_last': (13, 35, 5, 12, 5, 3, 2),
    'one_tile_wide_vertical_walk': (13, 16, 1, 4, 1, 4, 4),
    'one_tile_high': (3, 35, 2, 3, 2, 2, 1),
}


def _grid(hin, win, max_blocks, b=1):
    hm, wm = 2 * hin, 2 * win
    tiles = b * ((wm + 31) // 32) * ((hm + 7) // 8)
    blocks = min(tiles, K_BLOCKS)
    if max_blocks > 0:
        blocks = min(blocks, max_blocks)
    return tiles, blocks, -(-tiles // blocks), tiles // blocks


def test_the_cases_make_blocks_walk_several_tiles():
    for name, (hin, win, mb, tiles, blocks, most, least) in CASES.items():
        assert _grid(hin, win, mb) == (tiles, blocks, most, least), name
        assert most >= 2, name
    assert any(c[5] != c[6] for c in CASES.values())          # a partial last round


_REF, _ORACLE = {}, {}


def _reference(name, nadd, dtype):
    """Operands and the two-launch result of a case: computed once."""
    key = (name, nadd, dtype)
    if key not in _REF:
        hin, win = CASES[name][:2]
        ops = _operands(hin, win, 1, 1, nadd, seed=hin * 1000 + win)          # (the same x, weights and biases for every nadd of a case)
        ref, d0 = _tpair(*ops, 1, 1, dtype, fused=0)
        assert d0 == 0
        _REF[key] = (ops, ref)
    return _REF[key]


def _nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2).contiguous()


def _oracle(name, ops):
    """float64 reference of both layers without the addends, and the magnitudes the bound scales with (NCHW, CPU); once per case."""
    if name not in _ORACLE:
        x, w1, b1, w2, b2 = ops[:5]
        t2, s1 = A.linear_op(3, 't2'), A.linear_op(3, 's1')
        mid, mag1 = A.reference(t2, _nchw(x).clamp(min=0), w1.cpu(), b1.cpu())
        out, mag2 = A.reference(s1, mid.clamp(min=0), w2.cpu().double(), b2.cpu())
        _ORACLE[name] = (mid, mag1, out, mag2, F.conv2d(mag1, w2.cpu().double().abs(), padding=1))
    return _ORACLE[name]


def _check_oracle(name, ops, got, tol, store):
    """tol: the arithmetic's TOL; store: the relative rounding of a stored value (0 for fp32 maps)."""
    mid, mag1, out, mag2, w2mag1 = _oracle(name, ops)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    if got['mid'] is not None:
        assert_elementwise(got['mid'], nhwc(mid), nhwc((tol + 2 * store) * mag1), name + ' first layer')
    add, addmag = torch.zeros_like(out), torch.zeros_like(out)
    for a in ops[6:8]:
        if a is not None:
            add, addmag = add + _nchw(a).double(), addmag + _nchw(a).double().abs()
    bound = (tol + 2 * store) * (mag2 + addmag) + (tol + 2 * store) * w2mag1
    if got['raw'] is not None:
        assert_elementwise(got['raw'], nhwc(out), nhwc((tol + 2 * store) * mag2 + (tol + 2 * store) * w2mag1), name + ' second layer')
    if got['sum'] is not None:
        assert_elementwise(got['sum'], nhwc(out + add), nhwc(bound), name + ' sum')


@pytest.mark.parametrize('nadd', [0, 1, 2])
@pytest.mark.parametrize('name', list(CASES))
def test_rounds_of_the_persistent_form_equal_the_two_launches(name, nadd):
    ops, ref = _reference(name, nadd, 'fp32')
    got, d1 = _tpair(*ops, 1, 1, 'fp32', fused=1, form=2, max_blocks=CASES[name][2])
    assert d1 == 1, 'the one-launch form did not run'
    _same(ref, got, (name, nadd))
    assert torch.equal(ref['bits'], got['bits'])
    _check_oracle(name, ops, got, TOL['x3'], 0.0)


@pytest.mark.parametrize('nadd', [0, 2])
def test_rounds_without_the_first_layers_map(nadd):
    """The step's default: nothing reads the first layer's map, the launch writes its sign-bit words only; sum-only output."""
    name = 'three_rounds_partial_last'
    ops, ref = _reference(name, nadd, 'fp32')
    got, d1 = _tpair(*ops, 1, 1, 'fp32', fused=1, form=2, max_blocks=CASES[name][2], want_mid=False)
    assert d1 == 1
    _same(ref, got, (name, nadd, 'no map'))
    assert torch.equal(ref['bits'], got['bits'])


def test_rounds_of_the_narrow_forward_form():
    name = 'three_rounds_partial_last'
    ops, ref = _reference(name, 2, 'bf16')
    got, d1 = _tpair(*ops, 1, 1, 'bf16', fused=1, form=2, max_blocks=CASES[name][2])
    assert d1 == 1
    _same(ref, got, (name, 'bf16'))
    _check_oracle(name, ops, got, TOL['x1'], 2.0 ** -9)


def test_rounds_of_the_narrow_data_gradient_form():
    """Hi + lo weights: the first layer's fragments are fetched per tile as in the fp32 form; its SUM output is compared too."""
    hin, win, mb = CASES['three_rounds_partial_last'][:3]
    args, kw = _dg_case((hin, win), 1, 1)
    ref, d0 = _tpair(*args, fused=0, **kw)
    got, d1 = _tpair(*args, fused=1, form=2, max_blocks=mb, **kw)
    assert d0 == 0 and d1 == 1
    assert ref['mid_sum'] is not None and got['mid_sum'] is not None
    _same(ref, got, 'data gradients')
