"""CPU emulations of the arithmetics of the generic engine's convolution kernels (test infrastructure; DESIGN.md section 3 and the
GX3Args comments of csrc/ptta_kernels.h), the float64 reference they are measured against and the componentwise error bound.

An arithmetic is a way to form the products of a convolution; every one of them accumulates in fp32:
  fp32   the direct form (gconv.hip): fp32 operands
  x6     bf16x6: x = h + m + l, w = h + m + l by three round-to-nearest-even bf16 conversions, the six products down to 2^-16
         (l.h, h.l, m.m, m.h, h.m, h.h)
  x3     bf16x3: x = h + m, w = h + m; m.h + h.m + h.h
  w2     hi + lo weights: h.m + h.h (the activation rounded to bf16, the weight kept to 16 bits)
  x1     one MFMA: h.h
What an emulation cannot state is the ORDER of the fp32 accumulation inside and across the matrix instructions; the tests allow
a factor 4 on the emulation's own error for it (tests/gconv_cases.py).

Everything here is NCHW torch on the CPU; nothing from the library takes part."""
import torch
import torch.nn.functional as F

ARITHS = ('fp32', 'x6', 'x3', 'w2', 'x1')            # fine to coarse; the matrix-core chain is x6 < x3 < w2 < x1


def bf16(t):
    """Round to nearest even to bf16, returned as fp32 (torch's conversion, the same as the kernels' gsplit2 / gsplit3 / f2bf)."""
    return t.to(torch.bfloat16).to(torch.float32)


def split3(t):
    h = bf16(t)
    m = bf16(t - h)
    return h, m, bf16((t - h) - m)


def linear_op(k, geom, vert=False, dgrad=False, out_hw=None):
    """The convolution as a function lin(x, w) that is linear in both, in the dtype of its arguments.  geom 's1' / 's2' / 't2' (stride 2
    transposed, output_padding 1); vert: w [co][ci][3][1], three vertical taps.  dgrad: x is the gradient of the forward OUTPUT, w the
    forward weight, the result the gradient of the forward input, of size out_hw (a stride-2 convolution's input may be odd)."""
    pad = (1, 0) if vert else (k // 2, k // 2)
    if not dgrad:
        if geom == 's1':
            return lambda x, w: F.conv2d(x, w, padding=pad)
        if geom == 's2':
            return lambda x, w: F.conv2d(x, w, stride=2, padding=pad)
        return lambda x, w: F.conv_transpose2d(x, w, stride=2, padding=pad, output_padding=1)
    if geom == 's1':
        return lambda g, w: F.conv_transpose2d(g, w, padding=pad)
    if geom == 't2':
        return lambda g, w: F.conv2d(g, w, stride=2, padding=pad)

    def s2_grad(g, w):
        op = (out_hw[0] - ((g.shape[2] - 1) * 2 - 2 * pad[0] + k), out_hw[1] - ((g.shape[3] - 1) * 2 - 2 * pad[1] + k))
        return F.conv_transpose2d(g, w, stride=2, padding=pad, output_padding=op)
    return s2_grad


def activation(v, act):
    if act == 'relu':
        return v.clamp(min=0)
    if act == 'lrelu':
        return torch.where(v > 0, v, 0.2 * v)
    if act == 'sigmoid':
        return torch.sigmoid(v)
    return v


def emulate(arith, lin, x, w, bias=None, y_prev=None, act='none'):
    """fp32 tensors in, the fp32 result of the arithmetic: the small products first, as the kernels issue them."""
    x, w = x.float(), w.float()
    if arith == 'fp32':
        y = lin(x, w)
    else:
        xh, xm, xl = split3(x)
        wh, wm, wl = split3(w)
        y = None
        terms = {'x6': ((xl, wh), (xh, wl), (xm, wm), (xm, wh), (xh, wm), (xh, wh)), 'x3': ((xm, wh), (xh, wm), (xh, wh)),
                 'w2': ((xh, wm), (xh, wh)), 'x1': ((xh, wh),)}[arith]
        for a, b in terms:
            t = lin(a, b)
            y = t if y is None else y + t
    if bias is not None:
        y = y + bias.float().view(1, -1, 1, 1)
    if y_prev is not None:
        y = y + y_prev.float()
    return activation(y, act)


def reference(lin, x, w, bias=None, y_prev=None, act='none'):
    """float64 reference and the magnitude the bound scales with: |x| (*) |w| + |bias| + |y_prev| (the pre-activation value's; every
    activation here has slope <= 1)."""
    x, w = x.double(), w.double()
    y, mag = lin(x, w), lin(x.abs(), w.abs())
    if bias is not None:
        y = y + bias.double().view(1, -1, 1, 1)
        mag = mag + bias.double().abs().view(1, -1, 1, 1)
    if y_prev is not None:
        y = y + y_prev.double()
        mag = mag + y_prev.double().abs()
    return activation(y, act), mag


def error_ratio(emu, ref, mag):
    """Largest |emulation - reference| / magnitude: the number a tolerance is 4 x of."""
    return float(((emu.double() - ref).abs() / mag.clamp(min=1e-300)).max())
