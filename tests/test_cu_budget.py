"""The CU budget of a replay step, without a GPU: three workgroups of the
batch code-phase correlation per CU must leave registers and LDS for one wave per SIMD of every
kernel the step runs beside it, and none of them may use scratch.  The figures are the compiler's
resource remarks that the Makefile keeps in gps-sdr-receiver_amd/build/<name>.resources
(tools/cu_budget.py parses them); only that metadata is read, no instructions."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import cu_budget as cb  # noqa: E402

NEEDED = ('gpsmi_trk.resources', 'gpsmi_acq.resources')


@pytest.fixture(scope='module')
def kernels():
    """The parsed remark files: reused when the build left them, made otherwise."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    have = all(os.path.exists(os.path.join(cb.BUILD, n)) for n in NEEDED)
    if not os.path.exists(hipcc):
        if not have:
            pytest.skip('no hipcc and no resource remarks from an earlier build')
    else:                                     # (nothing to do when the objects are up to date)
        r = subprocess.run(['make', '-C', cb.PKG, '-j4'] + ['build/' + n.replace('.resources', '.o') for n in NEEDED],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
    if cb.cxxfilt() is None:
        pytest.skip('no c++filt to read the kernel names with')
    k = cb.parse([os.path.join(cb.BUILD, n) for n in NEEDED])
    print('\n' + cb.table(k, cb.CORR + cb.RESIDENTS + cb.LEFT_OUT))
    return k


def test_every_budget_kernel_is_in_the_remarks(kernels):
    for n in cb.CORR + cb.RESIDENTS + cb.LEFT_OUT:
        assert n in kernels, (n, sorted(kernels)[:40])
        assert set(cb.FIELDS.values()) <= set(kernels[n]), (n, kernels[n])


def test_granules_and_rounding():
    assert cb.VGPR_GRANULE == 8 and cb.LDS_GRANULE == 512
    assert cb.allocated_vgprs({'vgpr': 142, 'agpr': 0, 'waves': 3}) == 144
    assert cb.allocated_vgprs({'vgpr': 122, 'agpr': 0, 'waves': 3}) == 136     # three waves: 129 at least
    assert cb.allocated_vgprs({'vgpr': 76, 'agpr': 0, 'waves': 6}) == 80
    assert cb.allocated_vgprs({'vgpr': 62, 'agpr': 0, 'waves': 4}) == 104      # what rocprofv3 shows as 52 x 2
    assert cb.allocated_vgprs({'vgpr': 62, 'agpr': 6, 'waves': 8}) == 72       # 64 + 6 in eights
    assert cb.round_up(40192, cb.LDS_GRANULE) == 40448 and cb.round_up(5376, cb.LDS_GRANULE) == 5632


def test_three_correlation_workgroups_leave_room_for_every_resident(kernels):
    """Registers and LDS, every batch form of the correlation against every kernel a replay step
    runs beside it (none is left out: cu_budget.LEFT_OUT is empty)."""
    lines = cb.check(kernels)
    print('\n' + '\n'.join(('ok    ' if ok else 'FAILS ') + t for t, ok in lines))
    bad = [t for t, ok in lines if not ok and not t.startswith('scratch')]
    assert not bad, bad
    n_res, n_all = len(cb.RESIDENTS), len(cb.RESIDENTS + cb.LEFT_OUT)
    assert sum(t.startswith('registers') for t, _ in lines) == len(cb.CORR) * n_res
    assert sum(t.startswith('LDS') for t, _ in lines) == len(cb.CORR) * n_all
    assert n_res == 6 and n_all == 6


def test_correlation_is_compiled_for_three_workgroups_per_cu(kernels):
    """The factor 3 of the rule is what the compiler reports for the correlation's waves per SIMD
    (a workgroup of 256 threads is one wave on each of the four SIMDs)."""
    for n in cb.CORR:
        assert kernels[n]['waves'] == cb.CORR_PER_CU, (n, kernels[n])


def test_no_scratch(kernels):
    for n in cb.CORR + cb.RESIDENTS + cb.LEFT_OUT:
        assert kernels[n]['scratch'] == 0, (n, kernels[n])
