"""Record tests/golden/epilogue_pin.npz: the records and next-state rows of the wave-per-job batch
epilogue (option "epilogue_form" = 0) on the inputs of
tests/test_gpu_trk.py::test_batch_epilogue_forms_agree_on_random_states, N_CYC = 32 / 16 / 8.
Run it on an MI355X with the library of the commit whose arithmetic is to be pinned:

    python tools/record_epilogue_pin.py [blocks]

`blocks`: how many leading blocks of each run to keep (default: all of them).  Drift-list entries
past df_len are not the epilogue's to write and are stored as zero."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import conftest  # noqa: E402  (puts the package on the path)
import test_gpu_trk as t  # noqa: E402

keep = int(sys.argv[1]) if len(sys.argv) > 1 else None
r = t._run_closed_loop(conftest.load_golden('ref_default.npz'), 'default')
pin = {}
for n_cyc in (32, 16, 8):
    rec, st = t.random_state_runs(r, n_cyc)[0]
    rec, st = rec[:keep].copy(), st[:keep].copy()
    for idx in np.ndindex(st.shape):
        st[idx]['df'][int(st[idx]['df_len']):] = 0
    pin[f'rec{n_cyc}'], pin[f'st{n_cyc}'] = rec, st
r[0].close()
out = os.path.join(conftest.GOLDEN, 'epilogue_pin.npz')
np.savez_compressed(out, **pin)
print(out, os.path.getsize(out), 'bytes;', len(pin['rec32']), 'blocks of each run')
