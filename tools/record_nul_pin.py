"""Record tests/golden/nul_pin.npz: what null steering, its space-time form and the beams return on the
inputs of tests/test_gpu_nul_pin.py, for both input formats; the host and the `_dev` entry points (for
the beams: the host entry, beams_dev on packed rows and beams_dev on strided rows) must agree, and one
set is kept for all of them.  Run it on an MI355X with the library of the commit whose results are to
be pinned (GPSMI_LIB_PATH names a library other than lib/libgpsmi.so):

    python tools/record_nul_pin.py

Arrays of more than 4 KiB are stored as their SHA-256; everything else as it comes back."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import conftest  # noqa: E402  (puts the package on the path)
import test_gpu_nul_pin as t  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(conftest.GOLDEN, 'nul_pin.npz')
pin = {}


def keep(tag, arrays):
    for k, v in arrays.items():
        first = pin.setdefault(f'{tag}_{k}', v)
        assert first.dtype == v.dtype and np.array_equal(first, v), f'{tag}_{k}: the entry points differ'


for A, T, raw, dev in t.WEIGHT_CASES:
    keep(t.weights_tag(A, T, raw), t.run_weights(A, T, raw, dev))
for A, raw, entry in t.BEAM_CASES:
    keep(t.beams_tag(A, raw), t.run_beams(A, raw, entry))
keep('none', t.run_no_weights())
for k in sorted(pin):
    if k.endswith('_flags'):
        print(k, pin[k].tolist())
np.savez_compressed(out, **pin)
print(out, os.path.getsize(out), 'bytes;', len(pin), 'arrays')
