#!/usr/bin/env python3
"""The kernels' resource table and the CU budget of a replay step, from the
compiler's resource remarks: the Makefile keeps them per source file in
gps-sdr-receiver_amd/build/<name>.resources.  No GPU and no instructions are read: registers, LDS,
scratch and occupancy are what the code object's metadata says.

    tools/cu_budget.py                 the table of the budget's kernels and the rule, term by term
    tools/cu_budget.py --all           every kernel of the library
    tools/cu_budget.py --build         run make first (needs hipcc)

The rule, for C = the batch form of the code-phase correlation and every kernel R that a replay
step runs beside it (three workgroups of C per CU, one wave of R per SIMD beside them):
    registers   3 a(C) + a(R) <= 512                a(K) = the registers a wave of K is handed
    LDS         3 l(LDS_C) + l(LDS_R) <= 163840     l(b) = b rounded up to LDS_GRANULE
    scratch     0 for all of them

What a wave is handed is not only what the kernel uses: a kernel that can have at most w < 8 waves
on a SIMD (by its LDS, its launch bounds or an amdgpu_waves_per_eu attribute; the remarks'
"Occupancy") is given at least the registers that keep a (w + 1)-th wave out, 8 floor(512 / (w + 1) / 8)
+ 1, whatever it uses, and everything goes in eights: acq_corr_kernel<0> uses 62 and is handed
104, which is what rocprofv3 reports for its dispatches (in units of two).
"""
import glob
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'gps-sdr-receiver_amd')
BUILD = os.path.join(PKG, 'build')

SIMD_VGPRS = 512            # per lane: the unified register file of a gfx950 SIMD
VGPR_GRANULE = 8            # registers are allocated in eights (gfx90a and later)
CU_LDS = 163840             # bytes of LDS per CU
# LDS is handed out in blocks of 128 dwords: rocprofv3 reports 40448 B per dispatch for the
# correlation's 40192 and 5632 for the epilogue's 5376 (profiles/cu_budget/)
LDS_GRANULE = 512
CORR_PER_CU = 3             # workgroups of the code-phase correlation a CU holds

CORR = ('trk_corr_kernel<4, 0>', 'trk_corr_kernel<4, 1>')
RESIDENTS = ('trk_epilogue8_kernel<32>', 'trk_epilogue8_kernel<16>', 'trk_epilogue8_kernel<8>',
             'acq_corr_kernel<0>', 'acq_spectrum_kernel<1, 0>', 'acq_spectrum_kernel<1, 1>')
LEFT_OUT = ()               # kernels held to the LDS and scratch terms only: none

FIELDS = {'VGPRs': 'vgpr', 'AGPRs': 'agpr', 'ScratchSize [bytes/lane]': 'scratch',
          'Occupancy [waves/SIMD]': 'waves', 'LDS Size [bytes/block]': 'lds'}


def round_up(v, g):
    return (v + g - 1) // g * g


def min_vgprs_for_waves(w):
    """The least a kernel of at most w waves per SIMD is handed (see the module docstring)."""
    return 0 if w >= 8 else SIMD_VGPRS // (w + 1) // VGPR_GRANULE * VGPR_GRANULE + 1


def allocated_vgprs(k):
    """Registers a wave of this kernel takes from its SIMD: vector registers up to a multiple of
    four, accumulation registers behind them, at least what its waves per SIMD imply, in eights."""
    used = round_up(k['vgpr'], 4) + k['agpr']
    return round_up(max(used, min_vgprs_for_waves(k['waves'])), VGPR_GRANULE)


def cxxfilt():
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    for c in (os.path.join(os.path.dirname(os.path.realpath(hipcc)), '..', 'llvm', 'bin', 'llvm-cxxfilt'),
              '/opt/rocm/llvm/bin/llvm-cxxfilt', shutil.which('llvm-cxxfilt'), shutil.which('c++filt')):
        if c and os.path.exists(c):
            return c
    return None


def short_name(demangled):
    """'void gpsmi::trk_corr_kernel<4, 0>(void const*, ...)' -> 'trk_corr_kernel<4, 0>'"""
    s = demangled.replace('void ', '', 1) if demangled.startswith('void ') else demangled
    depth = 0
    for i, ch in enumerate(s):
        depth += ch == '<'
        depth -= ch == '>'
        if ch == '(' and depth == 0:
            s = s[:i]
            break
    return s.replace('gpsmi::', '')


def parse(paths=None):
    """{short kernel name: {'vgpr', 'agpr', 'scratch', 'waves', 'lds', 'file'}} of the remark files."""
    paths = sorted(glob.glob(os.path.join(BUILD, '*.resources'))) if paths is None else paths
    raw = []
    for p in paths:
        cur = None
        for line in open(p):
            m = re.search(r'remark:\s+(.*?):\s+(\S+)\s+\[-Rpass-analysis=kernel-resource-usage\]', line)
            if not m:
                continue
            key, val = m.group(1).strip(), m.group(2)
            if key == 'Function Name':
                cur = {'mangled': val, 'file': os.path.basename(p)}
                raw.append(cur)
            elif cur is not None and key in FIELDS:
                cur[FIELDS[key]] = int(val)
    filt = cxxfilt()
    names = [k['mangled'] for k in raw]
    if filt and names:
        names = subprocess.run([filt], input='\n'.join(names) + '\n', capture_output=True, text=True,
                               check=True).stdout.splitlines()
    return {short_name(n): k for n, k in zip(names, raw)}


def table(kernels, names):
    rows = ['| kernel | VGPRs used | handed to a wave | LDS B | LDS allocated | scratch B/lane | waves/SIMD |',
            '|---|---|---|---|---|---|---|']
    for n in names:
        k = kernels[n]
        rows.append(f"| `{n}` | {k['vgpr'] + k['agpr']} | {allocated_vgprs(k)} | {k['lds']} | "
                    f"{round_up(k['lds'], LDS_GRANULE)} | {k['scratch']} | {k['waves']} |")
    return '\n'.join(rows)


def check(kernels, residents=RESIDENTS, left_out=LEFT_OUT):
    """The rule term by term: [(text, holds)]."""
    out = []
    for c in CORR:
        kc = kernels[c]
        for r in residents + left_out:
            kr = kernels[r]
            if r in residents:
                v = CORR_PER_CU * allocated_vgprs(kc) + allocated_vgprs(kr)
                out.append((f'registers  3 x {allocated_vgprs(kc)} ({c}) + {allocated_vgprs(kr)} ({r}) = {v} '
                            f'<= {SIMD_VGPRS}', v <= SIMD_VGPRS))
            lds = CORR_PER_CU * round_up(kc['lds'], LDS_GRANULE) + round_up(kr['lds'], LDS_GRANULE)
            out.append((f'LDS        3 x {round_up(kc["lds"], LDS_GRANULE)} ({c}) + '
                        f'{round_up(kr["lds"], LDS_GRANULE)} ({r}) = {lds} <= {CU_LDS}', lds <= CU_LDS))
    for n in CORR + residents + left_out:
        out.append((f'scratch    {n}: {kernels[n]["scratch"]} B/lane', kernels[n]['scratch'] == 0))
    return out


def main():
    if '--build' in sys.argv:
        subprocess.check_call(['make', '-C', PKG, '-j4'])
    kernels = parse()
    if not kernels:
        sys.exit(f'no resource remarks under {BUILD}: build the library first (make -C gps-sdr-receiver_amd)')
    if '--all' in sys.argv:
        print(table(kernels, sorted(kernels)))
        return
    print(table(kernels, CORR + RESIDENTS + LEFT_OUT))
    print(f'\nVGPR granule {VGPR_GRANULE}, LDS granule {LDS_GRANULE} B, {SIMD_VGPRS} VGPRs per SIMD lane, '
          f'{CU_LDS} B of LDS per CU\n')
    bad = 0
    for text, ok in check(kernels):
        print(('ok    ' if ok else 'FAILS ') + text)
        bad += not ok
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
