#!/usr/bin/env python3
"""Compare the gfx950 ISA of named kernels between two `hipcc --save-temps` assembly files (the device .s).

    tools/isa_diff.py OLD.s NEW.s detout_class_kernel detout_tile_class_kernel detout_merge_kernel \\
        '--rename=ssd::detout_tile_class_kernel<0>=ssd::detout_tile_class_kernel'

A kernel is every symbol whose demangled name (without `void ` and the parameter list; --rename=NEW=OLD maps a kernel that
became a template instantiation onto its old name) contains one of the patterns.  Its body is the instructions from the
symbol's label to its last s_endpgm: the kernel descriptor after it (name, kernarg size) is not compared.  Basic-block
labels are renumbered (their function index moves when a file gains a kernel) and comment lines dropped.  Prints one line
per kernel and exits 1 on a difference or a kernel missing from NEW."""
import re
import subprocess
import sys


def bodies(path):
    out, name, lines = {}, None, []
    for ln in open(path, errors='replace'):
        m = re.match(r'^(_Z\w+):', ln)
        if m and name is None:
            name, lines = m.group(1), []
            continue
        if name is not None:
            if ln.startswith('.Lfunc_end'):
                last = max((i for i, x in enumerate(lines) if x.strip() == 's_endpgm'), default=len(lines) - 1)
                out[name] = lines[:last + 1]
                name = None
                continue
            s = ln.split(';')[0].rstrip()
            if s.strip():
                lines.append(re.sub(r'\.LBB\d+_', '.LBB_', s))
    return out


def demangled(table, renames):
    names = sorted(table)
    dem = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    out = {}
    for n, d in zip(names, dem):
        d = re.sub(r'^void ', '', d).split('(')[0]
        out[renames.get(d, d)] = table[n]
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--rename=')]
    renames = dict(a.split('=', 2)[1:] for a in sys.argv[1:] if a.startswith('--rename='))
    old, new, pats = demangled(bodies(args[0]), {}), demangled(bodies(args[1]), renames), args[2:]
    bad = 0
    for n in sorted(set(old) | set(new)):
        d = n
        if not any(p in d for p in pats):
            continue
        if n not in old or n not in new:
            print(('only in new: ' if n in new else 'only in old: ') + d)
            bad += n not in new
            continue
        same = old[n] == new[n]
        bad += not same
        print(f'{"identical" if same else "DIFFERENT"}  {len(new[n])} lines  {d}')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
