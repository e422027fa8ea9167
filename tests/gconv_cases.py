"""The cases of tests/test_gpu_gconv_elementwise.py and tests/test_gconv_elementwise_cpu.py, their seeded inputs, the arithmetic every
image of a case is computed with, and the tolerances.

TOL[arithmetic] = 4 x the largest error ratio |emulation - float64| / (|x| (*) |w| + |bias| + |y_prev|) of the CPU emulation
(oracle/gconv_arith.py) over the cases below -- never a figure from a GPU run.  `python -m tests.gconv_cases` recomputes the ratios and
prints the table kept in profiles/gconv_elementwise.txt; the CPU test checks the constants against the recomputed ratios."""
import zlib

import torch

from oracle import gconv_arith as A

# 4 x the ratios of profiles/gconv_elementwise.txt (python -m tests.gconv_cases)
RATIO = {'x1r': 1.142e-07, 'fp32': 3.821e-07, 'x6': 1.388e-07, 'x3': 1.073e-05, 'w2': 1.680e-06, 'x1': 2.553e-03}
TOL = {a: 4.0 * r for a, r in RATIO.items()}
NEXT_COARSER = {'x6': 'x3', 'x3': 'w2', 'w2': 'x1'}


def C(name, b, h, w, c0, c1, co, k=3, geom='s1', act='none', bias=False, acc=False, vert=False, six_b=0, x1_from_b=None, x1_w2=False,
      dgrad=False, out_hw=None, xexact=False, views=False, stats=0, form=None, big=False, discriminates=True):
    return dict(name=name, b=b, h=h, w=w, c0=c0, c1=c1, co=co, k=k, geom=geom, act=act, bias=bias, acc=acc, vert=vert, six_b=six_b,
                x1_from_b=x1_from_b, x1_w2=x1_w2, dgrad=dgrad, out_hw=out_hw, xexact=xexact, views=views, stats=stats, form=form, big=big,
                discriminates=discriminates)


CASES = [
    # ---- stride 1: sizes around the 8-row x 32-pixel tile, channel counts from the networks and at the launcher's edges ----
    C('s1_1x1_c8_co8', 1, 1, 1, 8, 0, 8),                                       # one pixel: only halo around it; c0 = 8: 3/4 of the first chunk empty, co = 8
    C('s1_7x31_c24_co40', 2, 7, 31, 24, 0, 40, act='lrelu', bias=True),         # one short of a tile both ways; half-empty second sub-chunk; 8 of 32 channels in the last tile
    C('s1_8x32_c40_c8_co72', 3, 8, 32, 40, 8, 72, act='relu', bias=True),       # exactly one tile; the source boundary inside the chunk sequence (40 = 32 + 8, then 8)
    C('s1_9x33_nlspn_head1', 1, 9, 33, 64, 64, 64),                             # NLSPN id/gd_dec1 (fd2 | fe2 -> 64): one row and one column into the second tile
    C('s1_17x65_nlspn_gd_dec0', 2, 17, 65, 64, 64, 8, bias=True),               # NLSPN gd_dec0 (gd1 | fe1 -> 8): third tile row / column of one pixel
    C('s1_17x33_nlspn_cf_dec0', 1, 17, 33, 32, 64, 1, act='sigmoid', bias=True),     # NLSPN cf_dec0 (cf1 | fe1 -> 1, sigmoid): Cy = 1 takes the scalar epilogue
    C('s1_9x31_nlspn_offset_aff', 2, 9, 31, 8, 0, 24, bias=True),               # NLSPN prop_layer.conv_offset_aff 8 -> 24
    C('s1_9x33_costdc_16_64', 2, 9, 33, 16, 0, 64),                             # CostDCNet 2layers block 16 -> 64 ...
    C('s1_8x65_costdc_64_16', 2, 8, 65, 64, 0, 16, bias=True),                  # ... and 64 -> 16
    C('s1_9x31_nlspn_48_256', 1, 9, 31, 48, 0, 256),                            # NLSPN 2layers block 48 -> 256 ...
    C('s1_7x33_nlspn_256_48', 1, 7, 33, 256, 0, 48, bias=True),                 # ... and 256 -> 48
    C('s1_1x65_c8_co40_lrelu', 3, 1, 65, 8, 0, 40, act='lrelu'),                # a single row
    C('s1_17x1_c24_c24_relu', 2, 17, 1, 24, 24, 72, act='relu'),                # a single column; both sources with a half-empty sub-chunk
    C('s1k1_9x33_costdc_128_16', 2, 9, 33, 128, 0, 16, k=1),                    # CostDCNet enc2d.conv2, 1x1 128 -> 16
    C('s1k1_1x65_c24_co40', 3, 1, 65, 24, 0, 40, k=1, bias=True, act='relu'),
    C('s1k1_17x31_c40_c8_co72', 1, 17, 31, 40, 8, 72, k=1, bias=True),
    C('s1k1_8x32_heads_512_1024', 1, 8, 32, 512, 0, 1024, k=1),                 # NLSPN heads' Linear 512 -> 1024 over the rows
    C('s1_acc_9x33', 2, 9, 33, 40, 8, 40, act='relu', bias=True, acc=True),     # accumulate (a gradient buffer's second writer), ReLU after the sum
    C('s1_acc_sigmoid_8x31', 1, 8, 31, 16, 0, 8, act='sigmoid', acc=True),      # accumulate + sigmoid: the scalar epilogue
    C('s1k1_acc_7x65', 2, 7, 65, 64, 0, 24, k=1, acc=True),
    C('s1_views_9x33_48_48', 2, 9, 33, 48, 0, 48, bias=True, views=True),       # NLSPN conv1_rgb_meta -> the fe1_rgb slice of fe1: ld > C for input and output
    C('s1_views_17x31_two_src', 1, 17, 31, 24, 40, 40, act='lrelu', views=True, acc=True),
    C('s1k1_views_8x33', 2, 8, 33, 16, 0, 72, k=1, views=True),
    C('s1_vert_9x65_32', 2, 9, 65, 32, 0, 32, vert=True),                       # CostDCNet P3D conv2 (3x1x1) as three vertical taps over [D][H*W]
    C('s1_vert_17x33_64_six', 2, 17, 33, 64, 0, 64, vert=True, six_b=1, bias=True),
    C('s1_six_all_9x33', 2, 9, 33, 16, 0, 64, six_b=2),                         # bf16x6 for the whole batch (an eval forward) ...
    C('s1_six_half_9x33', 2, 9, 33, 16, 0, 64, six_b=1, bias=True),             # ... and for the real frame of [real | proxy]
    C('s1_six_17x31_c24_c8', 3, 17, 31, 24, 8, 40, six_b=2, act='lrelu'),       # (the split is six_B, not B / 2: two of three images)
    C('s1k1_six_half_8x33', 2, 8, 33, 128, 0, 16, k=1, six_b=1),
    C('s1_x1_half_9x33', 2, 9, 33, 64, 64, 64, x1_from_b=1),                    # mixed mode: the proxy frame with one MFMA per product
    C('s1_x1_all_7x31', 3, 7, 31, 24, 0, 40, x1_from_b=0, act='lrelu', bias=True),
    C('s1_x1_one_of_three_8x32', 3, 8, 32, 16, 0, 16, x1_from_b=2),
    C('s1_six_x1_9x33', 2, 9, 33, 16, 0, 64, six_b=1, x1_from_b=1),             # [real: bf16x6 | proxy: one MFMA], the mixed mode of an x6 layer
    C('s1k1_x1_half_9x33', 2, 9, 33, 64, 0, 24, k=1, x1_from_b=1),
    C('s1_w2_half_9x33', 2, 9, 33, 16, 0, 64, x1_from_b=1, x1_w2=True, xexact=True),     # hi + lo weights for the second image
    C('s1_w2_all_8x31', 2, 8, 31, 24, 0, 40, x1_from_b=0, x1_w2=True, xexact=True),
    C('s1_stats_9x33', 2, 9, 33, 64, 0, 64, stats=1),                           # fused BatchNorm sums, one pass
    C('s1_stats2_17x65', 4, 17, 65, 16, 0, 40, stats=2),                        # two passes ([real | proxy]), partly empty channel tile
    C('s1_stats2_lrelu_7x31', 2, 7, 31, 24, 8, 72, stats=2, act='lrelu', bias=True),
    C('s1k1_stats_8x33', 2, 8, 33, 64, 0, 24, k=1, stats=1),
    C('s1_stats_acc_9x31', 2, 9, 31, 16, 0, 40, stats=1, acc=True),             # statistics out of the scalar epilogue
    C('s1_full_176x608', 2, 176, 608, 16, 0, 96, act='lrelu', bias=True, big=True),      # the 1/2-resolution map of a 352 x 1216 frame: 2508 blocks
    # ---- stride 2 (output ceil(in / 2)): every launch form, k 3 and 1, odd and even inputs, widths around 32 output pixels ----
    C('s2_plain_9x33', 2, 9, 33, 32, 0, 72, geom='s2', form='plain', bias=True),                # odd tile count -> one channel tile per wave; 17 output pixels
    C('s2_plain_six_8x64', 2, 8, 64, 16, 0, 16, geom='s2', form='plain', six_b=1),              # exactly 32 output pixels
    C('s2_nco2_8x66', 1, 8, 66, 16, 16, 64, geom='s2', form='nco2', act='relu'),                # two sources; 33 output pixels
    C('s2_nco2_six_7x62', 2, 7, 62, 64, 0, 128, geom='s2', form='nco2', six_b=2),               # NLSPN conv3.0.conv1 64 -> 128; odd rows: the second row of the last pair is outside
    C('s2_ksplit_7x31', 2, 7, 31, 128, 0, 40, geom='s2', form='ksplit', bias=True),             # K over the waves, partly empty channel tile
    C('s2_ksplit_six_4x64', 2, 4, 64, 128, 0, 64, geom='s2', form='ksplit', six_b=1),
    C('s2_ksplit_nlspn_conv6', 1, 5, 9, 512, 0, 512, geom='s2', form='ksplit'),                 # NLSPN conv6 512 -> 512 at 1/16 resolution
    C('s2k1_plain_9x65', 1, 9, 65, 64, 0, 128, k=1, geom='s2', form='plain'),                   # NLSPN conv3.0.downsample 64 -> 128, 1x1
    C('s2k1_ksplit_8x62', 2, 8, 62, 128, 0, 256, k=1, geom='s2', form='ksplit', six_b=1),       # NLSPN conv4.0.downsample 128 -> 256
    C('s2k1_below_threshold', 5, 76, 256, 128, 0, 512, k=1, geom='s2', form='ksplit', big=True),     # 380 items x 16 tiles: 95 * 16 = 1520 < 1536 ...
    C('s2k1_above_threshold', 5, 80, 256, 128, 0, 512, k=1, geom='s2', form='plain', big=True),      # ... 400 items: 100 * 16 = 1600, everything else equal
    C('s2_x1_half_9x33', 2, 9, 33, 32, 0, 64, geom='s2', form='nco2', x1_from_b=1),
    C('s2_full_176x608', 1, 176, 608, 64, 0, 128, geom='s2', form='nco2', big=True),
    # ---- transposed stride 2 (output 2 x in): every launch form, widths around 32 input pixels ----
    C('t2_plain_5x17', 2, 5, 17, 32, 0, 72, geom='t2', form='plain', bias=True),
    C('t2_plain_six_4x32', 2, 4, 32, 16, 0, 16, geom='t2', form='plain', six_b=1),
    C('t2_nco2_4x33', 1, 4, 33, 16, 16, 64, geom='t2', form='nco2', act='lrelu'),
    C('t2_nco2_six_7x31', 2, 7, 31, 64, 0, 128, geom='t2', form='nco2', six_b=2),
    C('t2_ksplit_nlspn_dec4', 1, 3, 5, 256, 512, 128, geom='t2', form='ksplit'),               # NLSPN dec4 (fd5 | fe5 -> 128): the widest decoder concatenation
    C('t2_ksplit_six_4x33', 2, 4, 33, 128, 0, 40, geom='t2', form='ksplit', six_b=1, bias=True),
    C('t2k1_plain_9x33', 1, 9, 33, 64, 0, 128, k=1, geom='t2', form='plain'),
    C('t2k1_ksplit_4x31', 2, 4, 31, 128, 0, 64, k=1, geom='t2', form='ksplit', six_b=1),
    C('t2_x1_half_5x33', 2, 5, 33, 32, 0, 64, geom='t2', form='nco2', x1_from_b=1),
    C('t2_full_nlspn_dec2_88x304', 1, 88, 304, 64, 128, 64, geom='t2', form='nco2', big=True),  # NLSPN dec2 (fd3 | fe3 -> 64) up to the 1/2-resolution map
    # ---- data gradients as GNet's backward sweep runs them: c0 = the forward OUTPUT channels, co = the forward input's ----
    C('dgrad_s1_9x33', 2, 9, 33, 48, 0, 64, dgrad=True),                                        # stride 1 with flipped, transposed weights
    C('dgrad_s1_w2_9x33', 2, 9, 33, 48, 0, 64, dgrad=True, x1_from_b=0, x1_w2=True, xexact=True),    # ... in the mixed mode: hi + lo weights
    C('dgrad_s1_x1_9x33', 2, 9, 33, 48, 0, 64, dgrad=True, x1_from_b=0),                        # ... with one MFMA (option bwd_w2 = 0)
    C('dgrad_s2_odd_5x17', 2, 5, 17, 128, 0, 64, geom='s2', dgrad=True, out_hw=(9, 33), form='ksplit'),      # a stride-2 conv over an odd 9 x 33 map: transposed run, output 2 in - 1
    C('dgrad_s2_w2_4x16', 1, 4, 16, 128, 0, 64, geom='s2', dgrad=True, out_hw=(8, 32), form='ksplit', x1_from_b=0, x1_w2=True, xexact=True),
    C('dgrad_t2_8x34', 2, 8, 34, 32, 0, 64, geom='t2', dgrad=True, out_hw=(4, 17), form='nco2'),           # a transposed conv's gradient: stride-2 run
    C('dgrad_t2_w2_8x66', 1, 8, 66, 64, 0, 128, geom='t2', dgrad=True, out_hw=(4, 33), form='nco2', x1_from_b=0, x1_w2=True, xexact=True),
    C('dgrad_s1k1_8x33', 2, 8, 33, 24, 0, 64, k=1, dgrad=True),
]
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def out_size(c):
    if c['dgrad']:
        return c['out_hw'] if c['out_hw'] else (c['h'], c['w'])
    return {'s1': (c['h'], c['w']), 's2': ((c['h'] + 1) // 2, (c['w'] + 1) // 2), 't2': (2 * c['h'], 2 * c['w'])}[c['geom']]


def make(c):
    """Seeded inputs of a case, NHWC fp32 (the layout the hook takes); the weight in the state dict's layout."""
    g = torch.Generator().manual_seed(zlib.crc32(c['name'].encode()))
    cin = c['c0'] + c['c1']
    ho, wo = out_size(c)
    x = torch.randn(c['b'], c['h'], c['w'], cin, generator=g)
    if c['xexact']:
        x = A.bf16(x)                       # bf16-exact activations: the weight's lo term is then the leading error term (see TOL notes)
    wi, wo_ = (c['co'], c['c0']) if c['dgrad'] else (cin, c['co'])              # the FORWARD convolution's (in, out) channels
    taps = 3 if c['vert'] else c['k'] * c['k']
    shape = (wi, wo_, c['k'], c['k']) if c['geom'] == 't2' else ((wo_, wi, 3, 1) if c['vert'] else (wo_, wi, c['k'], c['k']))
    w = torch.randn(shape, generator=g) * float(taps * wi) ** -0.5
    bias = torch.randn(c['co'], generator=g) * 0.5 if c['bias'] else None
    y_prev = torch.randn(c['b'], ho, wo, c['co'], generator=g) if c['acc'] else None
    return dict(x=x, w=w, bias=bias, y_prev=y_prev)


def lin_of(c):
    return A.linear_op(c['k'], c['geom'], c['vert'], c['dgrad'], out_size(c))


def image_ariths(c, impl='mfma'):
    """The arithmetic of every image of the batch (GX3Args: six_B, x1_from_B, x1_w2)."""
    if impl == 'direct':
        return ['fp32'] * c['b']
    x1f = c['b'] if c['x1_from_b'] is None else c['x1_from_b']
    return [('w2' if c['x1_w2'] else 'x1') if i >= x1f else ('x6' if i < c['six_b'] else 'x3') for i in range(c['b'])]


def groups(c, impl='mfma'):
    """[(arithmetic, first image, one past the last)]: runs of images with one arithmetic."""
    ar = image_ariths(c, impl)
    out, i0 = [], 0
    for i in range(1, len(ar) + 1):
        if i == len(ar) or ar[i] != ar[i0]:
            out.append((ar[i0], i0, i))
            i0 = i
    return out


def nchw(t):
    return None if t is None else t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def reference(c, d):
    """float64 reference and bound magnitude, NHWC."""
    ref, mag = A.reference(lin_of(c), nchw(d['x']), d['w'], d['bias'], nchw(d['y_prev']), c['act'])
    return nhwc(ref), nhwc(mag)


def reference_rounded(c, d):
    """The one-MFMA images' second reference: the float64 convolution of the bf16-ROUNDED operands, which that arithmetic equals up to
    its fp32 accumulation (tolerance TOL['x1r']).  Against it an image computed with a finer arithmetic is 2^-9 off: an image on the wrong
    side of x1_from_B fails whichever side it is on."""
    return reference(c, dict(d, x=A.bf16(d['x']), w=A.bf16(d['w'])))


def emulation(c, d, arith, i0=0, i1=None):
    yp = nchw(d['y_prev'])
    return nhwc(A.emulate(arith, lin_of(c), nchw(d['x'])[i0:i1], d['w'], d['bias'], None if yp is None else yp[i0:i1], c['act']))


def measure(cases):
    """Per case and image group: (case, arithmetic, its ratio, the next coarser arithmetic's ratio on the same images); and fp32 over
    the whole batch."""
    rows = []
    for c in cases:
        d = make(c)
        ref, mag = reference(c, d)
        rows.append((c['name'], 'fp32', A.error_ratio(emulation(c, d, 'fp32'), ref, mag), None))
        for ar, i0, i1 in groups(c):
            r = A.error_ratio(emulation(c, d, ar, i0, i1), ref[i0:i1], mag[i0:i1])
            nx = NEXT_COARSER.get(ar)
            rows.append((c['name'], ar, r, A.error_ratio(emulation(c, d, nx, i0, i1), ref[i0:i1], mag[i0:i1]) if nx else None))
            if ar == 'x1':
                rr, rmag = reference_rounded(c, d)
                rows.append((c['name'], 'x1r', A.error_ratio(emulation(c, d, 'x1', i0, i1), rr[i0:i1], rmag[i0:i1]),
                             A.error_ratio(emulation(c, d, 'x3', i0, i1), rr[i0:i1], rmag[i0:i1])))
    return rows


def worst(rows):
    out = {}
    for _, ar, r, _ in rows:
        out[ar] = max(out.get(ar, 0.0), r)
    return out


if __name__ == '__main__':
    torch.set_num_threads(16)
    rows = measure(CASES)
    print('%-34s %-5s %-12s %s' % ('case', 'arith', 'ratio', 'next coarser arithmetic on the same images'))
    for name, ar, r, rn in rows:
        print('%-34s %-5s %-12.3e %s' % (name, ar, r, '' if rn is None else '%.3e%s' % (rn, '' if 0.5 * rn > TOL[ar] else '   (< 2 x TOL: not discriminated)')))
    print()
    for ar, r in sorted(worst(rows).items(), key=lambda kv: (A.ARITHS + ('x1r',)).index(kv[0])):
        print('%-5s largest ratio %.3e  -> TOL = 4 x = %.3e' % (ar, r, 4 * r))
