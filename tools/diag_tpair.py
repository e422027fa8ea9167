#!/usr/bin/env python3
"""In-kernel phase stamps of conv32_tpair_kernel<float, 8, ADD> (library built with `make DIAG=1`): the headline's full-resolution pair
(176 x 608 -> 352 x 1216, two skip addends, sum output, the first half's map not written) through ptta_op_conv32_tpair; the stamped
instantiation prints per-tile cycle counts of every wave of two blocks.  python tools/diag_tpair.py [batch] [hin] [win]"""
import ctypes, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tta-depth-completion_amd'))
import torch
from proxytta import _lib
from proxytta._lib import ptr
lib = _lib.load()
b = int(sys.argv[1]) if len(sys.argv) > 1 else 1
hin, win = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (176, 608)
hm, wm = 2 * hin, 2 * win
x = torch.randn(b, hin, win, 32, device='cuda')
w1, w2 = torch.randn(32, 32, 3, 3, device='cuda') * 0.08, torch.randn(32, 32, 3, 3, device='cuda') * 0.08
b1, b2 = torch.randn(32, device='cuda') * 0.3, torch.randn(32, device='cuda') * 0.3
a1, a2 = torch.randn(b, hm, wm, 32, device='cuda'), torch.randn(b, hm, wm, 32, device='cuda')
out = torch.empty(b, hm, wm, 32, device='cuda')
bits = torch.empty(b, hm, wm, dtype=torch.int32, device='cuda')
did = ctypes.c_int(-1)
for rep in range(2):          # (the second call: weights and addends as warm as the step leaves them)
    rc = lib.ptta_op_conv32_tpair(ptr(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2), None, None, ptr(a1), ptr(a2), None, None, None, ptr(out), None, None, ptr(bits),
                                  b, b, hin, win, 2, 1, 1, 1, 0, 0, 0, 1, 2, 0, ctypes.byref(did), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    print('call', rep, 'rc', rc, 'one-launch form ran', did.value)
