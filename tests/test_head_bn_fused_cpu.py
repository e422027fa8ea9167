"""CPU-only: the flags of ptta_op_gconv_affine's residual forms and the "head_bn_fused" option keys, as include/ptta.h declares them and
as the ctypes binding carries them."""
import os
import re

from proxytta import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'ptta.h')).read()


def _define(name):
    return int(re.search(r'^#define %s (\d+)\b' % name, HEADER, re.M).group(1))


def test_gconv_flag_constants_equal_the_headers_defines():
    names = ('PTTA_GCONV_VERT', 'PTTA_GCONV_X1_W2', 'PTTA_GCONV_DGRAD', 'PTTA_GCONV_AFF_ACT_FIRST', 'PTTA_GCONV_AFF_RES_PLAIN')
    values = [_define(n) for n in names]
    assert values == [getattr(_lib, n) for n in names]
    # the next free bits behind PTTA_GCONV_DGRAD, each its own
    assert values == [1, 2, 4, 8, 16]
    assert _define('PTTA_ABI_VERSION') == _lib.PTTA_ABI_VERSION == 2          # nothing existing changed meaning


def test_option_keys_are_in_the_headers_option_table():
    table = HEADER[HEADER.index('key             default  meaning of 0'):HEADER.index('int ptta_set_option(')]
    settable, read_only = table.split('Read-only keys')
    assert re.search(r'^ \*   "head_bn_fused"\s+1\s', settable, re.M)
    assert re.search(r'^ \*   "head_bn_fused_count"\s', read_only, re.M) and '"head_bn_fused_count"' not in settable
