"""Record tests/golden/windows_pin.npz: what cancellation, the signatures and the profiles return on
the inputs of tests/test_gpu_windows_pin.py, for both code lengths and both input formats; the host and
the `_dev` entry points must agree, and one set is kept for both.  Run it on an MI355X with the library
of the commit whose results are to be pinned (GPSMI_LIB_PATH names a library other than
lib/libgpsmi.so):

    python tools/record_windows_pin.py

Arrays of more than 4 KiB are stored as their SHA-256; everything else as it comes back."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import conftest  # noqa: E402  (puts the package on the path)
import test_gpu_windows_pin as t  # noqa: E402
from gpsmi.engine import AcqEngine, Config  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(conftest.GOLDEN, 'windows_pin.npz')
pin = {}
for cs in (2048, 16368):
    for raw in (False, True):
        e = AcqEngine(Config(**t.CFG[cs]), prns=sorted({s[0] for s in t.CANCEL_SATS + t.PROF_SATS}))
        e.set_input_format(raw)
        for dev in (False, True):
            for k, v in t.run_combo(e, cs, raw, dev).items():
                held = pin.setdefault(f'{t.tag(cs, raw)}_{k}', v)
                assert np.array_equal(held, v), f'{k}: the host and the _dev entry point differ'
        e.close()
np.savez_compressed(out, **pin)
print(out, os.path.getsize(out), 'bytes;', len(pin), 'arrays')
