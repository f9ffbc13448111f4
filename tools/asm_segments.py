#!/usr/bin/env python3
"""Instruction counts of one kernel per barrier segment, from the compiler's assembly listing
(hipcc -O3 -std=c++17 --offload-arch=gfx950 -I../include --cuda-device-only -S csrc/<file>.hip).

    tools/asm_segments.py LISTING.s 'trk_corr_kernelILi4ELi0E' [--dump FIRST,LAST]

A segment is the straight run of instructions between two s_barrier in listing order (the kernels
this is meant for are straight-line code per channel).  Columns: vector ALU instructions, of
which v_mov, s_nop (and the wait states they add up to), LDS instructions, scalar ALU, s_waitcnt,
global memory.  --dump prints the instructions of segments FIRST..LAST instead.  A record for
profiles/, not a test: nothing in the suite reads instruction text."""
import argparse
import collections
import re


def body(path, name):
    lines = open(path).read().split('\n')
    start = next(i for i, l in enumerate(lines) if re.match(r'^_Z\S*' + name + r'\S*:', l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
    out = []
    for l in lines[start + 1:end]:
        s = l.split(';')[0].strip()
        if not s or s.startswith(('.', '//')) or s.endswith(':'):
            continue
        out.append(s)
    return lines[start].rstrip(':'), out


def kind(op):
    if op.startswith('v_'):
        return 'valu'
    if op.startswith('ds_'):
        return 'lds'
    if op.startswith(('global_', 'buffer_', 'flat_', 'scratch_')):
        return 'vmem'
    if op in ('s_nop', 's_waitcnt'):
        return op
    return 'salu'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('listing')
    ap.add_argument('kernel', help='part of the mangled name, e.g. trk_corr_kernelILi4ELi0E')
    ap.add_argument('--dump', help='FIRST,LAST: print the instructions of these segments')
    a = ap.parse_args()
    name, ins = body(a.listing, a.kernel)
    segs = collections.defaultdict(collections.Counter)
    seg = 0
    dump = [int(x) for x in a.dump.split(',')] if a.dump else None
    for l in ins:
        op = l.split()[0]
        if op == 's_barrier':
            seg += 1
            continue
        if dump:
            if dump[0] <= seg <= dump[1]:
                print(seg, l)
            continue
        c = segs[seg]
        c[kind(op)] += 1
        if op.startswith('v_mov_b'):
            c['v_mov'] += 1
        if op == 's_nop':
            c['nop_states'] += int(l.split()[1]) + 1
    if dump:
        return
    cols = ('valu', 'v_mov', 's_nop', 'nop_states', 'lds', 'salu', 's_waitcnt', 'vmem')
    print(name)
    print('| segment | ' + ' | '.join(cols) + ' |')
    print('|---|' + '---|' * len(cols))
    tot = collections.Counter()
    for s in sorted(segs):
        tot.update(segs[s])
        print(f'| {s} | ' + ' | '.join(str(segs[s][k]) for k in cols) + ' |')
    print('| all | ' + ' | '.join(str(tot[k]) for k in cols) + ' |')


if __name__ == '__main__':
    main()
