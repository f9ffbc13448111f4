"""The window rule of cancellation, signatures and profiles (csrc/gpsmi_windows.h)
without a GPU: tests/host/windows_check.cpp is a program of its own around the header, built here with
the host compiler under AddressSanitizer + UBSan into a temporary directory and run as a child process
(nothing is loaded into Python and nothing is preloaded).  The starts it prints are held to the numpy
restatements: sig_ref.sig_windows, profile_ref.prof_windows and cancel_ref.cancel_windows."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cancel_ref as CR
import profile_ref as PR
import sig_ref as SR
from test_submit_host import INC, PROBE, ROOT, STATIC

SRC = os.path.join(ROOT, 'tests', 'host', 'windows_check.cpp')
SANITIZE = 'address,undefined'
L1 = 1575.42e6


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('windows_check'))
    probe = os.path.join(tmp, 'probe.cpp')
    with open(probe, 'w') as f:
        f.write(PROBE)
    why = 'neither g++ nor clang++ found'
    for cxx in ('g++', 'clang++'):
        if not shutil.which(cxx):
            continue
        # (the header's `#pragma clang fp contract` is for hipcc: x86-64 without -march has no fused multiply-add)
        flags = [cxx, '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', f'-fsanitize={SANITIZE}',
                 '-Wno-unknown-pragmas'] + STATIC.get(cxx, {}).get(SANITIZE, [])
        r = subprocess.run(flags + [probe, '-o', os.path.join(tmp, 'probe')], capture_output=True, text=True, timeout=120)
        if r.returncode:                # (no runtime to link: the next compiler may have one)
            why = f'{cxx} does not link -fsanitize={SANITIZE}: {r.stderr.strip()[-200:]}'
            continue
        out = os.path.join(tmp, 'windows_check')
        r = subprocess.run(flags + ['-Wall', '-Wextra', '-Werror', '-I', INC, SRC, '-o', out],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f'{cxx} -fsanitize={SANITIZE}:\n{r.stderr}'
        return out
    pytest.skip(why)


def run(exe, cases):
    """cases: [[word, number, ...]] -> the program's lines, one list of ints per case."""
    args = [a.hex() if isinstance(a, float) else str(a) for c in cases for a in c]
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    for word in ('AddressSanitizer', 'runtime error'):
        assert word not in r.stdout, r.stdout[-4000:]
    assert r.returncode == 0, r.stdout[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == 'windows_check ok' and len(lines) == len(cases) + 1, r.stdout[-4000:]
    for line, c in zip(lines, cases):
        assert line.split()[0] == c[0], line
    return [[int(v) for v in line.split()[1:]] for line in lines[:-1]]


def records(cs):
    """(f_hz, tau, f_offset, carrier_hz, n) -- tau negative, zero and many periods ahead, half-sample
    ties (f_hz = f_offset: Tc = cs exactly, so every start of the record is one), f_hz - f_offset of
    either sign, a small carrier (the code Doppler a thousand times L1's)."""
    n = 9 * cs + 333
    out = [(f, tau, off, car, n) for f, off, car in ((0.0, 0.0, L1), (4200.0, 0.0, L1), (-3700.0, 1500.0, L1),
                                                     (2500.0, 2500.0, L1), (900.0, -800.0, 1.0e6), (-900.0, 0.0, 1.0e6))
           for tau in (0.0, -0.5, 0.5, 10.5, 11.5, 7.49, 8.0, 8.5, 31.5, 32.0, -700.3, cs - 0.25, float(cs),
                       -40.0 * cs + 3.5, -3.0e9 * cs - 0.5, 5.0 * cs + 100.25)]
    return out + [(0.0, 60.0 * cs + 1.5, 0.0, L1, 70 * cs), (1000.0, 0.5 * cs, 0.0, L1, cs + cs // 4)]  # the last: no window


@pytest.mark.parametrize('cs', [2048, 16368])
def test_signature_windows(exe, cs):
    rec = records(cs)
    cases = [['starts', cs, n, f, tau, car, off, 0, 0, n_ms] for f, tau, off, car, n in rec for n_ms in (0, 3)]
    got = run(exe, cases + [['pad', 1]])
    want = [SR.sig_windows(n, cs, f, tau, n_ms, car, off) for f, tau, off, car, n in rec for n_ms in (0, 3)]
    assert got[:-1] == want
    assert [] in want and max(map(len, want)) >= 10 and sum(len(w) == 3 for w in want) >= len(rec) - 2
    # the table: every record's starts, 0 behind them
    most = max(map(len, want))
    assert got[-1] == [most] + [j for w in want for j in w + [0] * (most - len(w))]
    # cancellation cuts the same periods: its windows that lie whole inside iq start where these do
    for (f, tau, off, car, n), w in zip(rec, want[::2]):
        assert w == [j for _, _, j in CR.cancel_windows(n, cs, f, tau, car, off) if j >= 0 and j + cs <= n]


@pytest.mark.parametrize('cs', [2048, 16368])
def test_ends_of_the_input(exe, cs):
    """Tc = cs: the last window ends exactly at n, and with one sample less it is gone; a start that
    rounds exactly onto the guard is kept, one below it is not."""
    for guard in (0, 8, 32):
        n = 5 + 4 * cs + guard
        a, b, c, d = run(exe, [['starts', cs, n, 0.0, 5.0 - cs, L1, 0.0, guard, 0, 0],
                               ['starts', cs, n - 1, 0.0, 5.0 - cs, L1, 0.0, guard, 0, 0],
                               ['starts', cs, n, 0.0, guard + 0.5, L1, 0.0, guard, 0, 0],
                               ['starts', cs, n, 0.0, guard - 0.51, L1, 0.0, guard, 0, 0]])
        first = 5 if guard <= 5 else 5 + cs
        assert a == list(range(first, 5 + 3 * cs + 1, cs)) and a[-1] + cs + guard == n and b == a[:-1]
        assert c[0] == guard and d[0] == guard - 1 + cs                # (guard + 0.5 ties down to the even guard)
        assert a == PR.prof_windows(n, cs, 0.0, 5.0 - cs, guard, 0, 1).ravel().tolist() if guard else \
            a == SR.sig_windows(n, cs, 0.0, 5.0 - cs)


@pytest.mark.parametrize('cs', [2048, 16368])
def test_profile_windows(exe, cs):
    """Every skip_ms, at guards 8 and 32, runs of 3 windows, n_runs 0 and 2; then all of records() at
    skip_ms 0 and 7."""
    n = 30 * cs + 77
    some = [(4200.0, -700.3, 0.0, L1, n), (-3700.0, 7.5, 1500.0, L1, n)]
    sets = [(r, Lh, skip, n_runs) for r in some for Lh in (8, 32) for skip in range(20) for n_runs in (0, 2)]
    sets += [(r, 12, skip, 0) for r in records(cs) for skip in (0, 7)]
    coh = 3
    cases = [['starts', cs, n_, f, tau, car, off, Lh, skip, n_runs * coh] for (f, tau, off, car, n_), Lh, skip, n_runs in sets]
    got = run(exe, cases + [['pad', coh]])
    want = [PR.prof_windows(n_, cs, f, tau, Lh, skip, coh, n_runs, car, off) for (f, tau, off, car, n_), Lh, skip, n_runs in sets]
    for g, w, s in zip(got, want, sets):
        assert g[:w.size] == w.ravel().tolist() and len(g) - w.size < coh, s
    assert {len(w) for w in want} >= {0, 2, 3, 9}          # no run, the n_runs asked for, (29 - 19) // 3, 29 // 3
    most = max(len(w) for w in want)
    assert got[-1] == [most] + [j for w in want for j in w.ravel().tolist() + [0] * (coh * (most - len(w)))]


@pytest.mark.parametrize('cs', [2048, 16368])
def test_cancel_edges(exe, cs):
    """ceil and rint of the one edge function against cancellation's restatement: the windows tile
    [0, n) between the ceilings, the replica is laid from the rounded start."""
    rec = [r for r in records(cs) if abs(r[1]) < 1e6 * cs]
    cases, wins = [], []
    for f, tau, off, car, n in rec:
        w = CR.cancel_windows(n, cs, f, tau, car, off)
        Tc = cs / (1.0 + (f - off) / car)
        k0 = int(np.rint((w[0][2] - tau) / Tc))
        assert int(np.rint(tau + float(k0) * Tc)) == w[0][2]
        cases.append(['edges', cs, n, f, tau, car, off, k0, len(w) + 1])
        wins.append(w)
    for g, w, (f, tau, off, car, n) in zip(run(exe, cases), wins, rec):
        ceil, rint = g[0::2], g[1::2]
        assert [(min(max(lo, 0), n), min(hi, n), j) for lo, hi, j in zip(ceil, ceil[1:], rint)] == w
        assert w[0][0] == 0 and w[-1][1] == n and all(a[1] == b[0] for a, b in zip(w, w[1:]))


def test_refusals_name_the_caller(exe):
    """The record's checks: the text is "<entry point>: <reason>" whatever stage asks."""
    def refused(f, tau, car, off, cs=2048):
        args = ['starts', cs, 4096, f, tau, car, off, 0, 0, 0]
        r = subprocess.run([exe] + [a.hex() if isinstance(a, float) else str(a) for a in args],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert r.returncode == 0, r.stdout
        return r.stdout.splitlines()[0]
    assert refused(0.0, 0.0, -1.0, 0.0) == 'refused -1 windows_check: carrier_hz must be positive (0: L1)'
    assert refused(0.0, 0.0, 0.0, float('inf')) == 'refused -1 windows_check: f_offset_hz must be finite'
    assert refused(0.0, 0.0, 0.0, 0.0, cs=4096) == 'refused -5 windows_check: code_samples 2048 and 16368 only (4096)'
    assert refused(1024000.0, 0.0, 0.0, 0.0) == 'refused -1 windows_check: f_hz out of range'
    assert refused(0.0, 1e15, 0.0, 0.0) == 'refused -1 windows_check: tau out of range'
    assert refused(900000.0, 0.0, 1.0e7, 0.0) == 'refused -1 windows_check: f_hz - f_offset_hz beyond 1 % of carrier_hz'
