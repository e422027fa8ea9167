#!/usr/bin/env python3
"""Compare the device code of two trees kernel by kernel, as text.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only FILE.hip -o DIR/FILE.s      (every touched file, both trees)
    python tools/isa_diff.py DIR_BEFORE DIR_AFTER

Every *.s of a directory is split per kernel symbol: the function from its `-- Begin function` line to its `-- End function` line,
which holds the body, the `.amdhsa_kernel ... .end_amdhsa_kernel` descriptor and the resource `.set` lines.  The only tokens that depend
on where in a translation unit a function stands are normalised: the function index of the block labels `.LBB<n>_<m>` (and of the
`BB<n>_<m>` in the compiler's loop comments) and of `.Lfunc_end<n>`; runs of blanks count as one (the comment column
behind a label moves with the label's length).  Reported: symbols on one side only, symbols defined in more than
one file of a side, symbols whose text differs (with the first differing line), and the kernel count of every file.  A file may move its kernels to other files: symbols are matched across
the whole directory.  Exit status 0 when the two sides hold the same symbols, each once, with the same text."""
import glob
import os
import re
import sys

BEGIN = re.compile(r';\s*-- Begin function (\S+)')
END = re.compile(r';\s*-- End function')
LABEL = re.compile(r'(\.L|\b)BB\d+_(\d+)')           # `.LBB<n>_<m>` labels and the `BB<n>_<m>` of the loop comments
FUNC_END = re.compile(r'\.Lfunc_end\d+')
BLANKS = re.compile(r'[ \t]+')               # the comment column behind a label moves with the label's length


def kernels_of(path):
    """{symbol: normalised text} of the kernels (functions with a kernel descriptor) of one assembly file"""
    out, sym, buf = {}, None, []
    with open(path, errors='replace') as f:
        for line in f:
            if sym is None:
                m = BEGIN.search(line)
                if m:
                    sym, buf = m.group(1), [line]
                continue
            buf.append(line)
            if END.search(line):
                text = ''.join(buf)
                if '.amdhsa_kernel ' + sym in text:
                    out[sym] = BLANKS.sub(' ', FUNC_END.sub('.Lfunc_end#', LABEL.sub(r'\1BB#_\2', text)))
                sym = None
    return out


def side(directory):
    where, text, per_file = {}, {}, {}
    for path in sorted(glob.glob(os.path.join(directory, '*.s'))):
        ks = kernels_of(path)
        per_file[os.path.basename(path)] = len(ks)
        for sym, t in ks.items():
            where.setdefault(sym, []).append(os.path.basename(path))
            text.setdefault(sym, t)
    return where, text, per_file


def first_difference(a, b):
    la, lb = a.split('\n'), b.split('\n')
    for n, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            return 'line %d of the function: %r | %r' % (n + 1, x.strip()[:90], y.strip()[:90])
    return 'length: %d | %d lines' % (len(la), len(lb))


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    (wa, ta, fa), (wb, tb, fb) = side(argv[1]), side(argv[2])
    for name, files in (('before', fa), ('after', fb)):
        print('%s (%s): %d kernels in %d files' % (name, argv[1 if name == 'before' else 2], sum(files.values()), len(files)))
        for f, n in files.items():
            print('    %-24s %4d' % (f, n))
    only_a, only_b = sorted(set(ta) - set(tb)), sorted(set(tb) - set(ta))
    dup = [(n, s, w[s]) for n, w in (('before', wa), ('after', wb)) for s in sorted(w) if len(w[s]) > 1]
    differ = [s for s in sorted(set(ta) & set(tb)) if ta[s] != tb[s]]
    print('symbols only before: %d' % len(only_a))
    for s in only_a:
        print('    %s (%s)' % (s, wa[s][0]))
    print('symbols only after: %d' % len(only_b))
    for s in only_b:
        print('    %s (%s)' % (s, wb[s][0]))
    print('symbols defined in more than one file of a side: %d' % len(dup))
    for n, s, files in dup:
        print('    %s: %s in %s' % (n, s, ', '.join(files)))
    print('kernels on both sides: %d, with differing text: %d' % (len(set(ta) & set(tb)), len(differ)))
    for s in differ:
        print('    %s (%s -> %s)\n        %s' % (s, wa[s][0], wb[s][0], first_difference(ta[s], tb[s])))
    return 1 if (only_a or only_b or dup or differ) else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
