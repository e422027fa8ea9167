"""CPU-only: the wide weight-gradient diagnostic is declared in include/ptta.h and bound by the ctypes table with its full argument list."""
import os
import re

from proxytta import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_op_gwgrad_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'ptta.h')).read()
    m = re.search(r'int ptta_op_gwgrad\(([^)]*)\);', header)
    assert m, 'ptta_op_gwgrad not declared'
    nargs = len([a for a in m.group(1).split(',') if a.strip()])
    sig = {name: args for name, _, args in _lib.SIGNATURES}
    assert 'ptta_op_gwgrad' in sig and len(sig['ptta_op_gwgrad']) == nargs == 13


def test_op_gwgrad_python_forms():
    from proxytta.engine import GWGRAD_IMPLS
    assert GWGRAD_IMPLS == {'default': 0, 'fp32_mfma': 1, 'naive': 2}
