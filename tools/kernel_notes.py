"""vgpr / sgpr / scratch / LDS of the kernels inside a BUILT library (the notes of its gfx950 code object: seconds, no recompilation).

    python tools/kernel_notes.py <lib.so> [substring of the mangled kernel name]
    python tools/kernel_notes.py <parent.so> --against <branch.so>     both side by side; exit status 1 if a kernel of the parent got worse

The rule of --against: for every kernel name of the parent, vgpr, scratch and LDS of the branch are <= the parent's (a missing kernel is worse)."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = '/opt/rocm/lib/llvm/bin'


def kernel_notes(so):
    with tempfile.TemporaryDirectory() as td:
        import shutil
        shutil.copy(so, os.path.join(td, 'lib.so'))
        subprocess.check_call([os.path.join(LLVM, 'llvm-objdump'), '--offloading', os.path.join(td, 'lib.so')], stdout=subprocess.DEVNULL, cwd=td)
        co = [f for f in os.listdir(td) if 'gfx950' in f][0]
        notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', os.path.join(td, co)], capture_output=True, text=True, check=True).stdout
    res = {}
    for blk in re.split(r'\n\s+- \.agpr_count:', notes)[1:]:
        g = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        res[re.search(r'\.name:\s+(\S+)', blk).group(1)] = dict(vgpr=g('vgpr_count'), sgpr=g('sgpr_count'), scratch=g('private_segment_fixed_size'),
                                                                 lds=g('group_segment_fixed_size'))
    return res


def short_name(mangled):
    """name<template arguments> of a kernel template in the anonymous namespace (bools as 0 / 1); anything else stays mangled"""
    m = re.match(r'_ZN12_GLOBAL__N_1(\d+)', mangled)
    name = mangled[m.end():m.end() + int(m.group(1))] if m else ''
    args = re.match(r'I((?:L[a-z]n?\d+E)+)E', mangled[m.end() + len(name):]) if m else None
    if not args:
        return mangled
    return '%s<%s>' % (name, ','.join(a.replace('n', '-') for a in re.findall(r'L[a-z](n?\d+)E', args.group(1))))


def compare(parent_so, branch_so):
    """Prints the side-by-side table (the format of profiles/*_kernel_notes.txt); returns the number of parent kernels that got worse."""
    a, b = kernel_notes(parent_so), kernel_notes(branch_so)
    keys = ('vgpr', 'scratch', 'lds')
    worse = [k for k in a if k not in b or any(b[k][f] > a[k][f] for f in keys)]
    cols = lambda r: '%3s %5s %6s' % tuple(r[f] if r else '-' for f in keys)
    print("kernel resources, parent commit | this commit (tools/kernel_notes.py on both libraries, gfx950): vgpr / scratch bytes / LDS bytes")
    print('rule: for every kernel name of the parent, vgpr, scratch and LDS of this commit are <= the parent\'s; "new" = a kernel the parent does not have')
    print("%d kernels in the parent, %d here; kernels of the parent that got worse: %d\n" % (len(a), len(b), len(worse)))
    for k in sorted(a) + sorted(set(b) - set(a)):
        mark = '  WORSE' if k in worse else '' if k in a else '  new'
        print("%-52.52s %s | %s%s" % (short_name(k), cols(a.get(k)), cols(b.get(k)), mark))
    return len(worse)


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[2] == '--against':
        sys.exit(1 if compare(sys.argv[1], sys.argv[3]) else 0)
    pat = sys.argv[2] if len(sys.argv) > 2 else ''
    for name, r in sorted(kernel_notes(sys.argv[1]).items()):
        if pat in name:
            print("%-90s vgpr %3d sgpr %3d scratch %4d lds %6d" % (name[:90], r['vgpr'], r['sgpr'], r['scratch'], r['lds']))
