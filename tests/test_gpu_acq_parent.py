"""GPU: every acquisition search against the tables the parent of the kernel consolidation
(csrc/gpsmi_acq_search.h) wrote, byte for byte: peak records (argmax, peak, mean, std) and neighbour
tables of the coherent, non-coherent and deep searches at both code lengths, complex64 and raw
input, including a search whose bins take two launches.

tests/golden/acq_parent_tables.npz holds this project's own outputs, recorded on an MI355X from the
commit before the consolidation by running this file as a script against that commit's library
(`GPSMI_LIB_PATH=<the parent's libgpsmi.so> python tests/test_gpu_acq_parent.py OUT.npz`).  It must
never be re-recorded from a build whose kernels are under test.  The inputs are seeded noise;
their sha256 is part of the fixture and is asserted before anything is compared, so a drift of the
generator cannot pass as a kernel change."""
import hashlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'acq_parent_tables.npz')
CFG = {2048: dict(code_samples=2048, n_cyc=32), 16368: dict(code_samples=16368, n_cyc=8)}
L1_HZ = 1575.42e6

PRNS = [3, 17, 30]
BINS = [-4000.0, -250.0, 0.0, 1750.0, 5000.0]
COH_2048 = [1, 3, 4, 10]            # G = 1; G = 4 dealt evenly; G = 4 dealt 3 / 3 / 2 / 2
COH_NBR = (1, 4)                    # ... of which these ask for the neighbours
SEG_2048 = [(1, 2), (4, 3), (5, 2)]
SEG_16368 = [(2, 3)]
# deep: bins around an offset of 1 MHz, so that 1 ms of code slides by more than a sample
DEEP_OFFSET = 1.0e6
DEEP_BINS = [1.0e6, 0.0, 2.0e6, -2.0e6, 4.0e6]
# second chunk: 512 MiB of scratch / (n_seg * cs * 8 bytes) = 64 bins a launch, bins 64 .. 69 in a second
BIG_PRNS = [5, 22]
BIG_BINS = [-3450.0 + 100.0 * i for i in range(70)]
BIG_SEG = {2048: 512, 16368: 64}
BIG_DEEP_OFFSET = 2.0e4


def deep_shifts(freqs, f_offset, n_coh, n_seg, cs):
    """deep_shift of csrc/gpsmi_acq.hip, restated: [bin][segment] in 0 .. cs - 1."""
    out = np.zeros((len(freqs), n_seg), np.int64)
    for b, f in enumerate(freqs):
        for s in range(n_seg):
            m = np.rint(-(np.float64(f) - f_offset) / L1_HZ * np.float64(s) * np.float64(n_coh) * np.float64(cs))
            out[b, s] = int(np.fmod(m, cs)) % cs
    return out


def inputs(cs, raw, big):
    """(key, samples): seeded uint16 noise, as it is or decoded as the recorder's samples are."""
    from gpsmi.synth import raw_to_c64
    n = BIG_SEG[cs] * cs if big else 12 * cs
    rng = np.random.default_rng(20260 + cs + (1 if big else 0))
    data = rng.integers(0, 65536, n, dtype=np.uint16)
    if not raw:
        data = np.ascontiguousarray(raw_to_c64(data))
    key = f"sha_{cs}_{'u8' if raw else 'c64'}_{'big' if big else 'small'}"
    return key, data


def run_cases(cs, raw, check_input=lambda key, data: None):
    """Every case of one code length and input format: {name: table or neighbours}."""
    from gpsmi.engine import AcqEngine, Config
    tag = f"{cs}_{'u8' if raw else 'c64'}"
    out = {}
    key, data = inputs(cs, raw, False)
    check_input(key, data)
    key_big, data_big = inputs(cs, raw, True)
    check_input(key_big, data_big)
    e = AcqEngine(Config(**CFG[cs]), prns=PRNS + BIG_PRNS)
    try:
        e.set_input_format(raw)
        for n_avg in (COH_2048 if cs == 2048 else [2]):
            if n_avg in COH_NBR or cs != 2048:
                out[f'{tag}_coh{n_avg}_tab'], out[f'{tag}_coh{n_avg}_nbr'] = e.search_ex(data, PRNS, BINS, n_avg)
            if n_avg not in COH_NBR:
                out[f'{tag}_coh{n_avg}_plain'] = e.search(data, PRNS, BINS, n_avg)
        for n_coh, n_seg in (SEG_2048 if cs == 2048 else SEG_16368):
            name = f'{tag}_{n_coh}x{n_seg}'
            out[f'{name}_nc_tab'], out[f'{name}_nc_nbr'] = e.search_noncoherent(data, PRNS, BINS, n_coh, n_seg,
                                                                               nbr=True)
            out[f'{name}_deep_tab'], out[f'{name}_deep_nbr'] = e.search_deep(
                data, PRNS, DEEP_BINS, n_coh, n_seg, f_offset=DEEP_OFFSET, nbr=True)
        n_seg = BIG_SEG[cs]
        out[f'{tag}_big_nc_tab'], out[f'{tag}_big_nc_nbr'] = e.search_noncoherent(data_big, BIG_PRNS, BIG_BINS, 1,
                                                                                 n_seg, nbr=True)
        out[f'{tag}_big_deep_tab'], out[f'{tag}_big_deep_nbr'] = e.search_deep(
            data_big, BIG_PRNS, BIG_BINS, 1, n_seg, f_offset=BIG_DEEP_OFFSET, nbr=True)
    finally:
        e.close()
    return out


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope='module')
def parent():
    if not os.path.exists(FIXTURE):
        pytest.skip('tests/golden/acq_parent_tables.npz has not been recorded yet: record it from the '
                    'PARENT commit\'s build on an MI355X (see this module\'s docstring)')
    return np.load(FIXTURE, allow_pickle=False)


def test_deep_cases_hold_the_three_kinds_of_shift():
    """No shift, a small one, and one above 1792 (the rotated read wraps in the last 256-lane row),
    in every deep case of the 2048 path; the second chunk's bins shift too."""
    for n_coh, n_seg in SEG_2048:
        m = deep_shifts(DEEP_BINS, DEEP_OFFSET, n_coh, n_seg, 2048)[:, 1:]
        assert (m[0] == 0).all() and (m[1:] != 0).all()
        assert ((m > 0) & (m <= 16)).any() and (m > 1792).any()
    m = deep_shifts(BIG_BINS, BIG_DEEP_OFFSET, 1, BIG_SEG[2048], 2048)
    assert m[64:].all(axis=0)[1:].any()


@pytest.mark.parametrize('raw', [False, True])
@pytest.mark.parametrize('cs', [2048, 16368])
def test_tables_are_the_parents(parent, cs, raw):
    def check_input(key, data):
        assert _sha(data) == str(parent[key]), f'{key}: the generated input is not the recorded one'

    got = run_cases(cs, raw, check_input)
    tag = f"{cs}_{'u8' if raw else 'c64'}_"
    assert sorted(got) == sorted(k for k in parent.files if k.startswith(tag))
    for name, a in got.items():
        ref = parent[name]
        assert a.dtype == ref.dtype and a.shape == ref.shape, name
        assert a.tobytes() == ref.tobytes(), name


if __name__ == '__main__':          # record the fixture (from the parent's build only: see above)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'gps-sdr-receiver_amd'))
    rec = {}
    for cs_ in (2048, 16368):
        for raw_ in (False, True):
            rec.update(run_cases(cs_, raw_, lambda key, data: rec.__setitem__(key, np.array(_sha(data)))))
    np.savez_compressed(sys.argv[1], **rec)
    print(f'{len(rec)} arrays written to {sys.argv[1]}')
