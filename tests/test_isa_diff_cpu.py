"""tools/isa_diff.py on small hand-written assembly listings: kernels that move between files and change their function index compare
equal; a changed instruction, a missing kernel and a kernel defined twice are each reported."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'isa_diff.py')


def _kernel(sym, n, body='\tv_add_f32_e32 v0, v1, v2'):
    """one kernel as the compiler lists it, as the n-th function of its file"""
    return '\n'.join(['\t.protected\t%s ; -- Begin function %s' % (sym, sym), '\t.globl\t%s' % sym, '%s:' % sym,
                      '\ts_cbranch_execz .LBB%d_2' % n, '.LBB%d_1:%s; =>This Loop Header: Depth=1' % (n, ' ' * (30 - len(str(n)))),
                      body, '\ts_cbranch_scc1 .LBB%d_1' % n, '.LBB%d_2:' % n, '\ts_endpgm', '\t.amdhsa_kernel %s' % sym, '\t\t.amdhsa_next_free_vgpr 3',
                      '\t.end_amdhsa_kernel', '.Lfunc_end%d:' % n, '\t.size\t%s, .Lfunc_end%d-%s' % (sym, n, sym), '\t; -- End function', ''])


def _run(tmp_path, before, after):
    for side, files in (('a', before), ('b', after)):
        os.makedirs(tmp_path / side)
        for name, text in files.items():
            (tmp_path / side / name).write_text(text)
    r = subprocess.run([sys.executable, TOOL, str(tmp_path / 'a'), str(tmp_path / 'b')], stdout=subprocess.PIPE, text=True)
    return r.returncode, r.stdout


def test_kernels_that_move_to_other_files_compare_equal(tmp_path):
    before = {'one.s': _kernel('k0', 0) + _kernel('k1', 1) + _kernel('k2', 12)}
    after = {'x.s': _kernel('k2', 0), 'y.s': _kernel('k0', 3) + _kernel('k1', 0)}
    rc, out = _run(tmp_path, before, after)
    assert rc == 0, out
    assert 'kernels on both sides: 3, with differing text: 0' in out and 'one.s' in out and 'y.s' in out


def test_differences_are_reported(tmp_path):
    before = {'one.s': _kernel('k0', 0) + _kernel('k1', 1) + _kernel('gone', 2)}
    after = {'x.s': _kernel('k0', 0, body='\tv_sub_f32_e32 v0, v1, v2') + _kernel('k1', 1), 'y.s': _kernel('k1', 0) + _kernel('new', 1)}
    rc, out = _run(tmp_path, before, after)
    assert rc == 1
    assert 'symbols only before: 1' in out and 'gone (one.s)' in out
    assert 'symbols only after: 1' in out and 'new (y.s)' in out
    assert 'more than one file of a side: 1' in out and 'after: k1 in x.s, y.s' in out
    assert 'with differing text: 1' in out and 'v_sub_f32_e32' in out
