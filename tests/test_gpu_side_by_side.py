"""The results of a replay step do not depend on who shares a CU with the code-phase correlation.

In the step of bench.py the previous batch's epilogue and the acquisition search run beside the
batch form of the code-phase correlation (the CU budget: three of its
workgroups leave a CU registers and LDS for them).  Here the same batch runs alone (replay_run,
nothing else on the device) and then 20 times in bench.py's order with a 32 SV x 41 bins x 1 ms
search beside it; every step must return the bytes of the run alone, every search the peak table
of a synchronous search.

9 blocks (the XCD map's batch branch starts at 8: one remainder block), 13 channels (the last
group of four holds one), N_CYC 32, complex64 and raw uint16 input (the search reads the same
format).  The state table is drawn the way tests/test_gpu_trk_corr.py draws its own.

Each input format is one GPU step: a child process of its own under a time limit; the second does
not start when the first has failed, and nothing is tried twice."""
import os
import subprocess
import sys

import numpy as np
import pytest

NB, NCH, N_CYC, CORR_AVG = 9, 13, 32, 8
STEPS = 20
STEP_LIMIT_S = 120          # a child takes a few seconds: the scene, 22 batches, 21 searches
PRNS = list(range(1, 33))
FREQS = [-5000.0 + 250.0 * i for i in range(41)]
ACQ_N = 2048                # 1 ms


def run_case(fmt):
    """One input format, in this process: run alone, then side by side.  Raises on any difference."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import conftest  # noqa: F401  (the package paths)
    import test_gpu_trk_corr as tc
    from gpsmi.engine import (AcqEngine, Config, DeviceBuffer, PinnedArray, TrkEngine, OUT_DTYPE,
                              PEAK_DTYPE)
    u8 = fmt == 'u8'
    blocks, raws = tc._scene_blocks(N_CYC)
    src = raws if u8 else blocks
    table, forced = tc._draw_table(np.random.default_rng([NB, NCH, N_CYC]), NB, NCH, tc._template_row())
    rows = np.arange(NB) % tc.N_DISTINCT
    eng = TrkEngine(Config(n_cyc=N_CYC, corr_avg=CORR_AVG, corr_min=tc.CORR_MIN), max_ch=NCH)
    assert tc._force_cg(eng, 4, 'option') == 4              # the batch form, whatever the job count
    eng.set_input_format(u8)
    acq = AcqEngine()
    acq.set_input_format(u8)
    buf = DeviceBuffer(NB * src[0].nbytes)
    for i in range(NB):
        buf.upload(src[rows[i]], i * src[0].nbytes)
    pins = [PinnedArray((NB, NCH), OUT_DTYPE) for _ in range(2)]
    apins = [PinnedArray((len(FREQS), len(PRNS)), PEAK_DTYPE) for _ in range(2)]

    # alone
    eng.replay_load(NB, table, forced)
    eng.replay_run(buf.ptr, NB)
    alone = eng.replay_fetch(np.zeros((NB, NCH), dtype=OUT_DTYPE)).copy()
    assert (alone['prn'] == table['prn']).all()
    assert (alone['delay'] >= 0).any() and (alone['delay'] < 0).any()      # both sides of CORR_MIN
    want = acq.search((buf.ptr, ACQ_N), PRNS, FREQS, 1).copy()
    assert np.isfinite(want['peak']).all() and (want['peak'] > 0).all()

    def same(got, ref, what):
        names = [k for k in ref.dtype.names
                 if np.ascontiguousarray(got[k]).tobytes() != np.ascontiguousarray(ref[k]).tobytes()]
        assert not names, (fmt, what, names)
        assert got.tobytes() == ref.tobytes(), (fmt, what, 'bytes between the fields')

    # side by side, bench.py's order
    for k in range(STEPS):
        if k > 0:
            acq.wait()
            same(apins[(k - 1) & 1].array, want, ('search', k - 1))
        pins[k & 1].array.view(np.uint8)[:] = 0xAB
        apins[k & 1].array.view(np.uint8)[:] = 0xCD
        acq.after(eng)
        eng.replay_run_async(buf.ptr, NB)
        acq.search_async(buf.ptr, ACQ_N, PRNS, FREQS, 1, apins[k & 1].array)
        eng.replay_fetch_async(pins[k & 1].array)
        eng.wait_prev()
        if k > 0:
            same(pins[(k - 1) & 1].array, alone, ('batch', k - 1))
    acq.wait()
    eng.wait()
    same(apins[(STEPS - 1) & 1].array, want, ('search', STEPS - 1))
    same(pins[(STEPS - 1) & 1].array, alone, ('batch', STEPS - 1))
    buf.free()
    for p in pins + apins:
        p.free()
    acq.close()
    eng.close()
    print(f'side by side ok: {fmt}, {STEPS} steps of {NB} x {NCH} jobs')


@pytest.mark.gpu
def test_results_do_not_depend_on_who_shares_a_cu():
    for fmt in ('c64', 'u8'):
        cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), fmt]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=STEP_LIMIT_S)
        print(r.stdout[-3000:])
        assert r.returncode == 0 and f'side by side ok: {fmt}' in r.stdout, (fmt, r.returncode)


if __name__ == '__main__':
    run_case(sys.argv[1])
