"""Per-satellite beams on the GPU (gpsmi_nul_beams*, csrc/gpsmi_nul_beam.h) against
the float64 restatement (tests/beam_ref.py): the case matrix of test_gpu_nulling.py's blocks, the
bit-for-bit properties of the contract, and snapshot.measure(..., beams=True) on the four-antenna
spoofed second."""
import numpy as np
import pytest

import beam_ref as B
import nul_ref as R
from test_gpu_nulling import JN_DB, SIGMA, _case_blocks, _cfg, _four_blocks

pytestmark = pytest.mark.gpu

PIVOT_MIN = 0.1                 # the constraints of the matrix: far from the dependence check's 1 / 64


def _beams_for(A, nbeam, seed):
    """nbeam steering vectors, min(A - 1, 4) null vectors and masks that cycle through 0, 1 and
    A - 1 (at most 4) nulls; every beam's Gram pivots >= PIVOT_MIN."""
    rng = np.random.default_rng(seed)
    nnull = min(A - 1, 4)
    while True:
        nulls = np.stack([R.cgauss(rng, A) * (0.5 + q) for q in range(nnull)])
        if min(B.gram_pivots(list(nulls))) >= PIVOT_MIN:
            break
    kinds = [0, 1 << (nnull - 1), (1 << nnull) - 1]
    steer, mask = [], []
    for b in range(nbeam):
        mk = kinds[b % 3]
        while True:
            s = R.cgauss(rng, A) * (1.0 + 0.25 * b)
            if min(B.gram_pivots([s] + [nulls[q] for q in range(nnull) if (mk >> q) & 1])) >= PIVOT_MIN:
                break
        steer.append(s), mask.append(mk)
    return np.stack(steer), nulls, np.array(mask, dtype=np.uint32)


def _compare(tag, x, n, A, nb, steer, nulls, mask, y, flags, gain, w):
    """Flags exact; weights, gain_db and output within four times what beam_ref.plain deviates from
    the restatement on the same case."""
    xc = (R.decode(x) if x.dtype == np.uint16 else x).reshape(A, nb, n)
    y_r, f_r, g_r, w_r = B.BeamRef(n, A).run(x, steer, nulls, mask)
    pl = [B.plain(xc[:, b], n, steer, nulls, mask) for b in range(nb)]
    assert [p[1].tolist() for p in pl] == f_r.tolist()
    y = y.reshape(len(steer), nb, n)
    fin = np.isfinite(g_r)
    g_p = np.stack([p[2] for p in pl])
    assert np.array_equal(g_p[~fin], g_r[~fin]) and np.array_equal(gain[~fin], g_r[~fin])      # (-inf: an all-zero block)
    tol_y = 4.0 * max(np.abs(p[0] - y_r[:, b]).max() for b, p in enumerate(pl))
    tol_g = 4.0 * np.abs(g_p.astype(np.float64)[fin] - g_r.astype(np.float64)[fin]).max(initial=0.0)
    tol_w = 4.0 * max(np.abs(p[3] - w_r[b]).max() for b, p in enumerate(pl))
    dev_y = np.abs(y - y_r).max()
    dev_g = np.abs(gain.astype(np.float64)[fin] - g_r.astype(np.float64)[fin]).max(initial=0.0)
    dev_w = np.abs(w - w_r).max()
    print(f'beam-matrix {tag} flags={sorted(set(f_r.ravel().tolist()))} gain_db {np.round(g_r[fin].min(initial=0), 2)} .. '
          f'{np.round(g_r[fin].max(initial=0), 2)} dev_w={dev_w:.3g} tol_w={tol_w:.3g} dev_g={dev_g:.3g} tol_g={tol_g:.3g} '
          f'dev_y={dev_y:.3g} tol_y={tol_y:.3g}')
    assert np.array_equal(flags, f_r), (flags, f_r)
    assert dev_g <= tol_g and dev_w <= tol_w and dev_y <= tol_y
    return f_r


CASES = [(A, n, raw_u8, nb) for A in (2, 3, 5, 8) for n in (2048, 4096 + 32) for raw_u8 in (False, True) for nb in (1, 3)]
CASES.append((4, 130944, True, 1))


@pytest.mark.parametrize('A,n,raw_u8,nb', CASES,
                         ids=[f'A{A}-n{n}-{"u8" if u else "c64"}-nb{nb}' for A, n, u, nb in CASES])
def test_case_matrix_against_the_reference(A, n, raw_u8, nb):
    """The blocks of test_gpu_nulling.py's matrix (0, 1 and A - 1 jammers, an all-zero block, a block
    of identical rows), 1, 3 or 16 beams whose masks carry 0, 1 and A - 1 (at most 4) nulls."""
    from gpsmi.nulling import NullSteer
    x = _case_blocks(A, n, nb, raw_u8)
    nbeam = (1, 3, 16)[(CASES.index((A, n, raw_u8, nb)) + nb) % 3]
    steer, nulls, mask = _beams_for(A, nbeam, 17 * A + nb)
    ns = NullSteer(_cfg(n), antennas=A, raw_u8=raw_u8)
    y = ns.beams(x, steer, nulls, mask)
    flags, gain, w = ns.last_beam_flags.copy(), ns.last_beam_gain_db.copy(), ns.last_beam_weights.copy()
    ns.close()
    f_r = _compare(f'A={A} n={n} {"u8" if raw_u8 else "c64"} nb={nb} B={nbeam}', x, n, A, nb, steer, nulls, mask, y,
                   flags, gain, w)
    if nb == 3 and not raw_u8 and n == 2048:
        assert 0 in f_r                                  # (the all-zero block: the quiescent beam)
        b = int(np.flatnonzero(f_r[:, 0] == 0)[0])
        assert not y.reshape(nbeam, nb, n)[:, b].any()
        for k in range(nbeam):
            cols = [steer[k]] + [nulls[q] for q in range(len(nulls)) if (int(mask[k]) >> q) & 1]
            G = np.stack(cols, axis=1)
            e0 = np.eye(G.shape[1])[0]
            assert np.abs(w[b, k] - G @ np.linalg.solve(G.conj().T @ G, e0)).max() < 1e-12 * np.abs(w[b, k]).max()


def _results(ns):
    return ns.last_beam_flags.tobytes() + ns.last_beam_gain_db.tobytes() + ns.last_beam_weights.tobytes()


def _per_block(res_flags, res_gain, res_w):
    return b''.join(np.concatenate(r).tobytes() for r in (res_flags, res_gain, res_w))


def test_the_bits_of_a_beam_depend_on_the_beam_and_its_block_alone():
    from gpsmi._lib import EngineError
    from gpsmi.engine import DeviceBuffer
    from gpsmi.nulling import NullSteer
    A, n, nb, nbeam = 3, 4096 + 32, 4, 5
    cfg = _cfg(n)
    raw = _four_blocks(A, n, True)
    x = R.decode(raw)
    steer, nulls, mask = _beams_for(A, nbeam, 3)
    assert sorted(set(mask.tolist())) == [0, 2, 3]
    a, b, u = NullSteer(cfg, antennas=A), NullSteer(cfg, antennas=A), NullSteer(cfg, antennas=A, raw_u8=True)
    # gpsmi_nul_apply before ...
    z4 = a.apply(x).tobytes()
    apply_res = a.last_flags.tobytes() + a.last_gain_db.tobytes() + a.last_weights.tobytes()
    y = a.beams(x, steer, nulls, mask)
    res, w_all = _results(a), a.last_beam_weights.copy()
    assert a.last_beam_flags.tolist() == [[1] * nbeam] * nb
    # ... and after, on the same handle: its old bytes, and its results were left alone by beams()
    assert a.last_flags.tobytes() + a.last_gain_db.tobytes() + a.last_weights.tobytes() == apply_res
    assert a.apply(x).tobytes() == z4
    assert a.last_flags.tobytes() + a.last_gain_db.tobytes() + a.last_weights.tobytes() == apply_res
    assert a.beams(x, steer, nulls, mask).tobytes() == y.tobytes() and _results(a) == res
    # a beam alone equals the beam among others, also with only its own nulls handed in
    for k in range(nbeam):
        yk = a.beams(x, steer[k:k + 1], nulls, mask[k:k + 1])
        assert yk.tobytes() == y[k].tobytes() and np.array_equal(a.last_beam_weights[:, 0], w_all[:, k])
        own = [q for q in range(len(nulls)) if (int(mask[k]) >> q) & 1]
        yk = a.beams(x, steer[k:k + 1], nulls[own] if own else None, [(1 << len(own)) - 1])
        assert yk.tobytes() == y[k].tobytes()
    # one call of 4 blocks equals 4 calls of 1
    singles, rf, rg, rw = [], [], [], []
    for k in range(nb):
        singles.append(a.beams(np.ascontiguousarray(x[:, k * n:(k + 1) * n]), steer, nulls, mask))
        rf.append(a.last_beam_flags.copy()), rg.append(a.last_beam_gain_db.copy()), rw.append(a.last_beam_weights.copy())
    assert np.concatenate(singles, axis=1).tobytes() == y.tobytes() and _per_block(rf, rg, rw) == res
    # two handles in one process agree; raw u8 equals complex64 of its decode
    assert b.beams(x, steer, nulls, mask).tobytes() == y.tobytes() and _results(b) == res
    assert u.beams(raw, steer, nulls, mask).tobytes() == y.tobytes() and _results(u) == res
    # host equals dev in both formats, packed and with strides; the samples between the rows stay untouched
    for h, src in ((b, x), (u, raw)):
        row = nb * n
        d_in, d_out = DeviceBuffer(src.nbytes), DeviceBuffer(nbeam * row * 8)
        d_in.upload(src)
        h.beams_dev(d_in.ptr, d_out.ptr, nb, steer, nulls, mask)
        assert d_out.download(np.complex64, nbeam * row).tobytes() == y.tobytes() and _results(h) == res
        gi, go = 64, 34                                  # (even: the rows keep their alignment)
        wide = np.zeros((A, row + gi), dtype=src.dtype)
        wide[:, :row] = src
        wide[:, row:] = src[:, :gi]                      # (whatever stands between the rows is not read as a block)
        s_in, s_out = DeviceBuffer(wide.nbytes), DeviceBuffer(nbeam * (row + go) * 8)
        s_in.upload(wide)
        fill = np.full(nbeam * (row + go), np.complex64(7.0 - 3.0j))
        s_out.upload(fill)
        h.beams_dev(s_in.ptr, s_out.ptr, nb, steer, nulls, mask, in_stride=row + gi, out_stride=row + go)
        got = s_out.download(np.complex64, nbeam * (row + go)).reshape(nbeam, row + go)
        assert np.ascontiguousarray(got[:, :row]).tobytes() == y.tobytes() and _results(h) == res
        assert np.array_equal(got[:, row:], fill.reshape(nbeam, row + go)[:, row:])
        # refusals on a live handle leave it usable
        with pytest.raises(EngineError, match='overlap'):
            h.beams_dev(d_in.ptr, d_in.ptr, 1, steer, nulls, mask)
        with pytest.raises(EngineError, match='overlap'):
            h.beams_dev(d_in.ptr, d_in.at((A * n - 8) * src.itemsize), 1, steer, nulls, mask)    # (the tail of a call of 1)
        with pytest.raises(EngineError, match='aligned'):
            h.beams_dev(d_in.ptr, d_out.at(8), 1, steer, nulls, mask)
        with pytest.raises(EngineError, match='aligned'):
            h.beams_dev(d_in.ptr, d_out.ptr, 1, steer, nulls, mask, in_stride=row + 1)
        with pytest.raises(EngineError, match='aligned'):
            h.beams_dev(d_in.ptr, d_out.ptr, 1, steer, nulls, mask, out_stride=n + 1)
        with pytest.raises(EngineError, match='stride'):
            h.beams_dev(d_in.ptr, d_out.ptr, 2, steer, nulls, mask, out_stride=n)
        with pytest.raises(EngineError, match='stride'):
            h.beams_dev(d_in.ptr, d_out.ptr, 2, steer, nulls, mask, in_stride=-2)
        for bad in (0, -1):
            with pytest.raises(EngineError, match='nb out of range'):
                h.beams_dev(d_in.ptr, d_out.ptr, bad, steer, nulls, mask)
        with pytest.raises(EngineError, match='dependent'):
            h.beams_dev(d_in.ptr, d_out.ptr, 1, steer[:1], steer[:1] * 2.0, [1])
        h.beams_dev(d_in.ptr, d_out.ptr, nb, steer, nulls, mask)
        assert d_out.download(np.complex64, nbeam * row).tobytes() == y.tobytes() and _results(h) == res
        assert h.last_ms() > 0 and min(h.last_beam_kernel_ms()) > 0
        for d in (d_in, d_out, s_in, s_out):
            d.free()
    for h in (a, b, u):
        h.close()


def test_space_time_handle_refuses_beams():
    from gpsmi._lib import EngineError
    from gpsmi.nulling import NullSteer
    A, n = 3, 2048
    st = NullSteer(_cfg(n), antennas=A, taps=3)
    x = _four_blocks(A, n)[:, :n].copy()
    with pytest.raises(EngineError, match=r'\(-3\)'):                # GPSMI_E_STATE
        st.beams(x, np.ones((1, A)))
    assert st.apply(x).shape == (n,)                     # (still usable)
    st.close()


def test_e0_beam_is_power_inversion():
    """steer = e0 without nulls: gpsmi_nul_apply's output wherever its flag is 1, within four times
    what the two restatements differ by."""
    from gpsmi.nulling import NullSteer
    A, n, nb = 3, 4096 + 32, 4
    x = _four_blocks(A, n)
    ns = NullSteer(_cfg(n), antennas=A)
    z = ns.apply(x).reshape(nb, n)
    on = ns.last_flags.copy()
    w_apply = ns.last_weights.copy()
    y = ns.beams(x, np.eye(A)[:1]).reshape(nb, n)
    w = ns.last_beam_weights[:, 0].copy()
    ns.close()
    assert on.tolist() == [1, 0, 1, 1]
    y_r, _, _, w_r = B.BeamRef(n, A).run(x, np.eye(A)[:1])
    z_r, _, _, wz_r = R.NullRef(n, A).run(x)
    for b in np.flatnonzero(on):
        tol_w = 4.0 * np.abs(w_r[b, 0] - wz_r[b]).max()
        tol_y = 4.0 * np.abs(y_r[0, b] - z_r[b]).max()
        print(f'block {b}: |w - w_apply| {np.abs(w[b] - w_apply[b]).max():.3g} (tol {tol_w:.3g}), '
              f'|y - apply| {np.abs(y[b] - z[b]).max():.3g} (tol {tol_y:.3g})')
        assert np.abs(w[b] - w_apply[b]).max() <= tol_w and np.abs(y[b] - z[b]).max() <= tol_y


def test_a_beam_without_weights_is_zeros():
    """Flag -1: M = Z^H Z underflows to zero -- samples of 1e30 under a steering vector of 1e-150 --
    and the beam's block is +0.0 while the beam beside it is formed as ever."""
    from gpsmi.nulling import NullSteer
    A, n = 2, 2048
    rng = np.random.default_rng(9)
    x = (1.0e30 * R.cgauss(rng, (A, 2 * n))).astype(np.complex64)
    x[:, n:] = R.noisy_block(rng, A, n, 1, JN_DB, SIGMA)
    steer = np.stack([R.cgauss(rng, A) * 1.0e-150, R.cgauss(rng, A)])
    ns = NullSteer(_cfg(n), antennas=A)
    y = ns.beams(x, steer).reshape(2, 2, n)
    flags, gain, w = ns.last_beam_flags.copy(), ns.last_beam_gain_db.copy(), ns.last_beam_weights.copy()
    ns.close()
    y_r, f_r, g_r, w_r = B.BeamRef(n, A).run(x, steer)
    assert f_r.tolist() == [[-1, 1], [1, 1]] and flags.tolist() == f_r.tolist()
    assert y[0, 0].tobytes() == np.zeros(n, np.complex64).tobytes() and not w[0, 0].any() and gain[0, 0] == 0
    for b in (0, 1):
        assert np.allclose(w[b, 1], w_r[b, 1], rtol=1e-12, atol=0.0)
        assert np.abs(y[1, b] - y_r[1, b]).max() <= 1e-5 * np.abs(y_r[1, b]).max()       # (y: [beam][block])


# ---- the spoofed second -----------------------------------------------------------------------------

# cn0_dbhz against the CPU-restated rise (test_beams.RESTATED): test_gpu_acq_refine.py holds a record's
# cn0_dbhz to a window of +- 2 dB.  (The GPU's signatures span the whole second, the restated ones 64 ms:
# both lie within 0.999 of the steering vectors, 0.01 dB of beam gain.)
CN0_MARGIN_DB = 2.0


def test_snapshot_beams_on_the_spoofed_second():
    import sig_ref as SR
    import spoof_truth as ST
    from gpsmi import snapshot as S
    from gpsmi.acquisition import Acquisition
    from test_beams import RESTATED, gains_on_parts
    from test_snapshot_signature import is_added
    _, info, _ = ST.spoofed()
    rows = SR.snapshot_raw('spoofed')
    acq = Acquisition(raw_u8=True)
    try:
        kw = dict(prns=sorted(info['ephs']), source='refine', spoof=True, antennas=SR.SNAP_ANTENNAS)
        off, _ = S.measure(acq, rows, **kw)
        st = {}
        meas, rep = S.measure(acq, rows, beams=True, stats=st, **kw)
        # with the option off: the existing call's bytes, which are the records as they were
        assert st['before_beams'].tobytes() == off.tobytes()
        assert acq.engine.raw_u8                                          # (the input format is back)
        tracked, _ = S.measure(acq, rows, beams=True, **dict(kw, source='track'))
    finally:
        acq.engine.close()
    before, beams, plan = st['before_beams'], st['beams'], st['beam_plan']
    assert len(meas) == len(before) == len(beams) == 16 and meas['prn'].tolist() == before['prn'].tolist()
    added = [bool(is_added(r)) for r in before]
    # the restated plan (test_beams.RESTATED, from the chain on the CPU): the same set, the same masks
    assert plan['set'] == [i for i, a in enumerate(added) if a] and len(plan['set']) == 8
    assert sorted(set(before['prn'].tolist())) == sorted(RESTATED)
    mask = np.array([int(b['null']) for b in beams])
    assert mask.tolist() == [0 if a else RESTATED[int(p)][0] for p, a in zip(before['prn'], added)]
    # every record confirmed on its beam, every block adaptive
    assert all(b['confirmed'] and b['flags'] == [1] for b in beams), beams
    # the two conditions, from the weights the call returned (block 0 on the scene's separate parts)
    w0 = np.stack([b['weights'][0] for b in beams])
    gain, copy = gains_on_parts(before, added, w0, mask)
    rise = meas['cn0_dbhz'] - before['cn0_dbhz']
    for i, b in enumerate(beams):
        print('PRN %2d %-9s null %d  gain_db %.2f  signal over noise against antenna 0 %+.2f dB  other copy %s  '
              'cn0_dbhz %.2f -> %.2f (%+.2f)' % (b['prn'], 'added' if added[i] else 'authentic', mask[i], b['gain_db'], gain[i],
                                                'n/a' if np.isnan(copy[i]) else '%.1f dB' % copy[i], before['cn0_dbhz'][i],
                                                meas['cn0_dbhz'][i], rise[i]))
    print('beams %.3f ms on the device, kernels (covariance, solve, apply) %s ms' % (st['beams_ms'], st['beam_kernel_ms']))
    assert gain.min() >= 10.0 * np.log10(SR.SNAP_ANTENNAS) - 3.0, gain
    assert (copy[mask == 1] < -S.SPOOF_REL_DB).all(), copy
    auth = np.array([not a for a in added])
    assert (rise[auth] > 0).all(), rise
    want = np.array([RESTATED[int(p)][2 if a else 1] for p, a in zip(before['prn'], added)])
    print('cn0_dbhz rise against the restated one: largest difference %.3f dB' % np.abs(rise - want).max())
    assert (np.abs(rise[auth] - want[auth]) <= CN0_MARGIN_DB).all(), (rise, want)
    assert tracked['prn'].tolist() == meas['prn'].tolist() and (tracked['source'] == b'track').all()
