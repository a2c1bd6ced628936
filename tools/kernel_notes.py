"""vgpr / sgpr / scratch / LDS of the kernels inside a BUILT library (the notes of its gfx950 code object: seconds, no recompilation).

    python tools/kernel_notes.py <lib.so> [substring of the mangled kernel name]
    python tools/kernel_notes.py <parent.so> --against <branch.so>     both side by side; exit status 1 if a kernel of the parent got worse
    python tools/kernel_notes.py <parent.so> --identical <branch.so>   the exact comparison, with sgpr and code size; exit status 1 if a kernel
                                                                       of the parent differs in any figure or a new kernel uses scratch

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


def kernel_notes_with_size(so):
    """kernel name -> (vgpr, sgpr, LDS bytes, scratch bytes, code bytes): the notes, and the size of the kernel's symbol in the code object"""
    with tempfile.TemporaryDirectory() as td:
        import shutil
        shutil.copy(so, os.path.join(td, 'lib.so'))
        subprocess.check_call([os.path.join(LLVM, 'llvm-objdump'), '--offloading', os.path.join(td, 'lib.so')], stdout=subprocess.DEVNULL, cwd=td)
        co = os.path.join(td, [f for f in os.listdir(td) if 'gfx950' in f][0])
        syms = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--symbols', '--wide', co], capture_output=True, text=True, check=True).stdout
    size = {}
    for line in syms.splitlines():
        p = line.split()
        if len(p) >= 8 and p[3] == 'FUNC':
            size[p[7]] = int(p[2], 0)
    return {k: (r['vgpr'], r['sgpr'], r['lds'], r['scratch'], size.get(k, -1)) for k, r in kernel_notes(so).items()}


def compare_identical(parent_so, branch_so):
    """The exact comparison (the format of profiles/step_vs_kernel_notes.txt): every kernel of the parent has identical figures in the
    branch, and no new kernel uses scratch.  Returns the number of kernels that break the rule."""
    a, b = kernel_notes_with_size(parent_so), kernel_notes_with_size(branch_so)
    diff = [k for k in a if a[k] != b.get(k)]
    new = sorted(set(b) - set(a))
    print("kernel resources from the metadata of the gfx950 code object (llvm-readelf --notes; code size: the kernel symbol's size, llvm-readelf --symbols)")
    print("of the main library, parent commit | this commit: vgpr / sgpr / LDS bytes / scratch bytes / code bytes")
    print("rule: every kernel symbol of the parent is in this commit's code object with IDENTICAL figures; \"new\" = a kernel the parent does not have, and it uses no scratch")
    print("%d kernels in the parent, %d here; kernels of the parent whose figures differ: %d; new kernels: %d, of them with scratch: %d\n"
          % (len(a), len(b), len(diff), len(new), sum(1 for k in new if b[k][3])))
    fmt = lambda r: '%3d %3d %6d %5d %6d' % r if r else '  -   -      -     -      -'
    for k in sorted(a) + new:
        mark = '  DIFFERS' if k in diff else '' if k in a else '  new'
        print("%-56.56s %s | %s%s" % (short_name(k), fmt(a.get(k)), fmt(b.get(k)), mark))
    return len(diff) + sum(1 for k in new if b[k][3])


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[2] == '--against':
        sys.exit(1 if compare(sys.argv[1], sys.argv[3]) else 0)
    if len(sys.argv) == 4 and sys.argv[2] == '--identical':
        sys.exit(1 if compare_identical(sys.argv[1], sys.argv[3]) else 0)
    pat = sys.argv[2] if len(sys.argv) > 2 else ''
    for name, r in sorted(kernel_notes(sys.argv[1]).items()):
        if pat in name:
            print("%-90s vgpr %3d sgpr %3d scratch %4d lds %6d" % (name[:90], r['vgpr'], r['sgpr'], r['scratch'], r['lds']))
