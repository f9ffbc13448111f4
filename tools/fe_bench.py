"""Device time of the front-end stage (gpsmi_fe_push_dev) for configurations A, B and
C of tests/fe_ref.py: one 1-s batch and one 32-ms block of input, already in device memory.  Prints
the median over --reps calls, input Msamples/s, x real time and FMA/s (outputs x taps x FMAs per tap:
two dot products over complex samples, 4 per tap).

    python tools/fe_bench.py [--reps 20] [--configs A,B,C] [--json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'gps-sdr-receiver_amd'))

CONFIGS = {   # (format, fs_in, IF / offset) -> 2.048 Msps
    'A': ('sc16', 4_000_000, 0.0),
    'B': ('r8', 16_368_000, 4_092_000.0),
    'C': ('r8', 38_192_000, 9_548_000.0),
}
FMA_PER_TAP = 4


def bench(name, reps):
    from gpsmi import _lib
    from gpsmi.engine import DeviceBuffer
    from gpsmi.frontend import FORMATS, FrontEnd
    fmt, fs_in, if_hz = CONFIGS[name]
    _, dt, per = FORMATS[fmt]
    fe = FrontEnd(None, fs_in, fmt, if_hz)
    lib = _lib.load()
    rng = np.random.default_rng(1)
    res = {'config': name, 'format': fmt, 'fs_in': fs_in, 'if_hz': if_hz, 'taps': fe.n_taps, 'phases': fe.n_phases}
    for label, seconds in (('batch_1s', 1.0), ('block_32ms', 0.032)):
        n = int(round(seconds * fs_in))
        info = np.iinfo(dt)
        x = rng.integers(info.min // 4, info.max // 4, size=n * per).astype(dt)
        d_in = DeviceBuffer(x.nbytes)
        d_in.upload(x)
        cap = int(n * 2_048_000 // fs_in) + 16
        d_out = DeviceBuffer(cap * 8)
        got = C.c_size_t(0)
        ms, outs = [], []
        for r in range(reps + 2):
            _lib.check(lib.gpsmi_fe_push_dev(fe.h, d_in.ptr, n, d_out.ptr, cap, C.byref(got)), 'gpsmi_fe_push_dev')
            if r >= 2:
                ms.append(fe.last_ms())
                outs.append(got.value)
        med = float(np.median(ms))
        n_out = int(np.median(outs))
        res[label] = {'input_samples': n, 'outputs': n_out, 'device_ms': round(med, 4),
                      'min_ms': round(float(np.min(ms)), 4),
                      'msps_in': round(n / med / 1e3, 1), 'x_realtime': round(seconds * 1e3 / med, 1),
                      'gfma_per_s': round(n_out * fe.n_taps * FMA_PER_TAP / med / 1e6, 1)}
        d_in.free()
        d_out.free()
    fe.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--configs', default='A,B,C')
    ap.add_argument('--json', action='store_true')
    a = ap.parse_args()
    rows = [bench(n, a.reps) for n in a.configs.split(',')]
    if a.json:
        print(json.dumps({'fe_bench': rows}))
        return
    for r in rows:
        for label in ('batch_1s', 'block_32ms'):
            b = r[label]
            print(f"{r['config']} {r['format']:5s} {r['fs_in'] / 1e6:7.3f} Msps {r['taps']:4d} taps x {r['phases']:3d} "
                  f"phases  {label:10s} {b['device_ms']:8.4f} ms  {b['msps_in']:8.1f} Msps in  "
                  f"{b['x_realtime']:8.1f} x real time  {b['gfma_per_s']:8.1f} GFMA/s")


if __name__ == '__main__':
    main()
