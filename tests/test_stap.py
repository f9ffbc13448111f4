"""Space-time null steering without a GPU: the restatement of the contract (tests/stap_ref.py, what
gpsmi_nul_* with taps = 3, 5, 7 is held to) against the one-weight restatement and a plain numpy
evaluation, the argument errors of the C ABI, and what the taps buy on two antennas whose channels
are 0.3 samples apart: the restatement followed by the oracle's acquisition sweep."""
import ctypes as C

import numpy as np
import pytest

import nul_ref as R
import stap_ref as S

# what the sweep finds on the single-antenna scene without a jammer: PRN -> (bin, code phase)
CLEAN = {4: (-2000.0, 143), 6: (1200.0, 1023), 15: (-3200.0, 638), 17: (2600.0, 1963),
         24: (-2800.0, 150), 27: (-3800.0, 1305), 28: (-2000.0, 1876), 32: (-2200.0, 1714)}
MATRIX = ((2, 3, 2048, 1), (3, 5, 4128, 2), (5, 7, 2080, 4), (8, 3, 2048, 7), (8, 7, 4128, 3))


def test_one_tap_is_the_one_weight_restatement_byte_for_byte():
    rng = np.random.default_rng(4)
    for A, n, J in ((2, 2048, 1), (5, 4128, 4), (8, 8192 + 2048, 3), (3, 4128, 0)):
        x = R.noisy_block(rng, A, n, J).astype(np.complex64)
        y_r, f_r, g_r, w_r = R.NullRef(n, A).process(x)
        for taps in (1, 0):
            y, f, g, w = S.StapRef(n, A, taps).process(x)
            assert w.shape == (A, 1) and f == f_r == (J > 0)
            assert y.tobytes() == y_r.tobytes() and w[:, 0].tobytes() == w_r.tobytes()
            assert np.float32(g).tobytes() == np.float32(g_r).tobytes()
    x = np.zeros((3, 2048), dtype=np.complex64)                      # no Cholesky factor
    assert S.StapRef(2048, 3, 1).process(x)[1:3] == R.NullRef(2048, 3).process(x)[1:3] == (0, 0.0)
    assert S.combine(x, np.ones(3)).tobytes() == R.combine(x, np.ones(3)).tobytes()


@pytest.mark.parametrize('A,T,n,J', MATRIX)
def test_matrix_from_the_lags_is_the_gram_matrix_of_the_shifted_rows(A, T, n, J):
    rng = np.random.default_rng(100 * A + T)
    x = S.stap_block(rng, A, n, J).astype(np.complex64)
    Z = S.shifted_rows(x, T)
    G = Z @ Z.conj().T / n
    for mode in ('f64', 'ext'):
        r = S.lag_sums(x, T, mode)
        assert not r[0].imag.diagonal().any() and np.array_equal(r[0], r[0].conj().T)
        M = S.lag_matrix(r, n)
        assert np.abs(M - G).max() <= 1e-13 * np.abs(G).max()
        assert np.array_equal(M, M.conj().T)                         # Hermitian to the bit
        for t in range(T - 1):                                       # block-Toeplitz to the bit
            assert np.array_equal(M[t::T, t::T][:, :], M[t + 1::T, t + 1::T])
        ev = np.linalg.eigvalsh(M)
        assert ev.min() >= -1e-12 * np.trace(M).real, ev.min()
    # the two evaluations of the sums agree to float64 rounding
    assert np.abs(S.lag_sums(x, T, 'f64') - S.lag_sums(x, T, 'ext')).max() <= 1e-13 * np.abs(G).max() * n


@pytest.mark.parametrize('A,T,n,J', MATRIX)
def test_restatement_against_plain_numpy(A, T, n, J):
    rng = np.random.default_rng(200 * A + T)
    x = S.stap_block(rng, A, n, J).astype(np.complex64)
    c = (T - 1) // 2
    yp, fp, gp, wp = S.plain(x, n, T)
    for mode in ('f64', 'ext'):
        y, flag, g, w = S.StapRef(n, A, T).process(x, mode)
        assert flag == fp == 1 and abs(float(g) - float(gp)) < 1e-4 and g > 15.0
        assert w[0, c] == 1.0 and np.abs(w - wp).max() < 1e-9
        assert np.abs(y - yp).max() < 1e-5 * np.abs(x).max()
        assert not y[:c].any() and not y[n - c:].any() and y[c:n - c].all()
        assert y.tobytes() == S.combine(x, w).tobytes()
    # the predicted output power holds the inner samples' (and the edges' and the loading's): the gain
    # measured on the inner samples is at least the predicted one, less the ratio of the two counts
    out = S.filt(x.astype(np.complex128), w)
    measured = 10 * np.log10(np.mean(np.abs(x[0].astype(np.complex128)) ** 2) / np.mean(np.abs(out) ** 2))
    assert measured >= float(g) - 10 * np.log10(n / (n - 2 * c)) - 1e-3 and measured < float(g) + 1.0


def test_degenerate_blocks_pass_through_or_null_deeply():
    n, A, T = 2048, 3, 5
    ref = S.StapRef(n, A, T)
    e = np.zeros((A, T))
    e[0, 2] = 1.0
    y, flag, g, w = ref.process(np.zeros((A, n), dtype=np.complex64))
    assert flag == 0 and g == 0 and not y.any() and np.array_equal(w, e)
    rng = np.random.default_rng(2)
    x = S.stap_block(rng, A, n, 0).astype(np.complex64)               # noise alone: antenna 0 bit for bit
    y, flag, g, w = ref.process(x)
    assert flag == 0 and 0.0 < g < 1.0 and y.tobytes() == x[0].tobytes() and np.array_equal(w, e)
    x = np.tile(R.cgauss(rng, n).astype(np.complex64), (A, 1))        # exact copies: singular but for the loading
    y, flag, g, w = ref.process(x)
    assert flag == 1 and g > 50.0 and np.abs(y).max() < 1e-3 * np.abs(x).max()


def _nul_cfg(n=65536, A=4, taps=0):
    from gpsmi import _lib
    return _lib.NulCfg(n, A, 0.0, 0.0, 0, taps)


def test_abi_taps_argument_needs_no_gpu():
    from gpsmi import _lib
    lib = _lib.load()
    assert lib.gpsmi_abi_sizeof(21) == C.sizeof(_lib.NulCfg) == 24
    assert _lib.NulCfg.taps.offset == 20 and _nul_cfg(taps=5).taps == 5
    for taps in (-1, 2, 4, 6, 8, 9):
        for A in (2, 8):
            h = C.c_void_p(0xDEAD)
            assert lib.gpsmi_nul_create(C.byref(_nul_cfg(A=A, taps=taps)), C.byref(h)) == -1 and h.value is None
            assert b'taps' in lib.gpsmi_last_error()
    for taps in (0, 1, 3, 5, 7):                      # accepted: whatever follows is not an argument error
        h = C.c_void_p(None)
        rc = lib.gpsmi_nul_create(C.byref(_nul_cfg(A=8, taps=taps)), C.byref(h))
        assert rc != -1 and (rc == 0) == (h.value is not None)
        if rc == 0:
            assert lib.gpsmi_nul_destroy(h) == 0


def test_python_wrapper_refuses_bad_taps_without_a_gpu():
    from gpsmi.engine import Config, EngineError
    from gpsmi.nulling import NullSteer
    for taps in (-1, 2, 4, 6, 8, 9):
        with pytest.raises(EngineError, match=r'\(-1\)'):
            NullSteer(Config(), antennas=2, taps=taps)


def test_default_channel_changes_nothing_and_a_channel_renders_alone():
    from gpsmi import synth_array as SA
    old = R.array_scene()                                            # the existing four-antenna scene
    new = SA.ArrayScene(old.scene, old.steering, old.jammers, channel=None)
    assert new.scale == old.scale and np.array_equal(new.block_raw(2, 4096), old.block_raw(2, 4096))
    arr = S.stap_scene('a')
    sat, noise, jam = arr.parts(1, 4096)
    plain_scene = SA.ArrayScene(arr.scene, arr.steering, arr.jammers, scale=arr.scale)
    sat0, noise0, jam0 = plain_scene.parts(1, 4096)
    assert np.array_equal(noise, noise0)                             # the receiver noise is not filtered
    assert np.array_equal(sat[0], sat0[0]) and np.array_equal(jam[0], jam0[0])    # antenna 0 has no channel
    assert not np.allclose(jam[1], jam0[1], atol=0.01 * np.abs(jam0).max())
    # antenna 1 of the jammer is antenna 0's waveform through the delay and the steering phase
    h = SA.delay_fir(S.DELAY)
    assert abs(h.sum() - 1.0) < 1e-12 and len(h) == 2 * SA.SINC_HALF + 1
    full = arr.parts(1)
    assert np.array_equal(full[2][:, :4096], jam) and np.array_equal(full[0][:, :4096], sat)
    assert np.array_equal(arr.block_raw(1, 4096), arr.block_raw(1)[:, :4096])
    assert np.allclose(arr.sat_components(1, 4096).sum(axis=0), sat, atol=1e-15)
    with pytest.raises(ValueError, match='per antenna'):
        SA.ArrayScene(arr.scene, arr.steering, [], channel=[None])
    with pytest.raises(ValueError, match='odd'):
        SA.ArrayScene(arr.scene, arr.steering, [], channel=[None, [1.0, 0.5]])


def _snr_rows(arr, w, b=0):
    """Per satellite: (SNR behind the weights against the unjammed antenna 0 in dB, lag of the peak of
    the cross-correlation with antenna 0's copy, its loss against a perfect copy in dB)."""
    n = arr.ngps
    T = w.shape[1]
    c = (T - 1) // 2
    _, noise, jam = arr.parts(b)
    rest = np.mean(np.abs(S.filt(noise + jam, w)) ** 2)
    rows = []
    for comp in arr.sat_components(b):
        out = S.filt(comp, w)
        snr = (np.mean(np.abs(out) ** 2) / rest) / (np.mean(np.abs(comp[0]) ** 2) / np.mean(np.abs(noise[0]) ** 2))
        ref0 = comp[0]
        xc = [abs(np.vdot(ref0[c + 4 + l:n - c - 4 + l], out[4:n - 2 * c - 4])) for l in range(-3, 4)]
        lag = int(np.argmax(xc)) - 3
        loss = max(xc) ** 2 / (np.sum(np.abs(out[4:n - 2 * c - 4]) ** 2) * np.sum(np.abs(ref0[c + 4:n - c - 4]) ** 2))
        rows.append((round(float(10 * np.log10(snr)), 1), lag, round(float(10 * np.log10(loss)), 2)))
    return rows


@pytest.mark.parametrize('kind,raw_u8', [('a', False), ('a', True), ('b', False), ('b', True)],
                         ids=['white-c64', 'white-u8', 'tones-c64', 'tones-u8'])
def test_what_the_taps_buy(kind, raw_u8):
    """Scene (a): one white jammer through channels 0.3 samples apart; scene (b): three tones from three
    directions.  One weight per antenna acquires strictly fewer satellites than five taps, and five
    taps acquire at the clean scene's bin (or its neighbour) and code phase +-1.  The figures are in
    DESIGN.md 4.2o."""
    arr = S.stap_scene(kind, raw_u8)
    n = arr.ngps
    blocks = {}

    def blk(b):
        if b not in blocks:
            blocks[b] = arr.block(b) if raw_u8 else S.block_c64(arr, b)
        return blocks[b]

    found = {}
    for T in (1, 3, 5):
        ref, res = S.StapRef(n, S.A2, T), {}

        def out(b):
            if b not in res:
                res[b] = ref.process(blk(b))
            return res[b][0]

        found[T] = S.oracle_sweep(out)
        y, flag, g, w = res[0]
        print(f'stap-scene {kind} {"u8" if raw_u8 else "c64"} T={T} flag={flag} gain_db={float(g):.2f} '
              f'found={dict(sorted(found[T].items()))}')
        if flag:
            print('   per satellite (SNR against unjammed antenna 0 dB, peak lag, loss dB):',
                  dict(zip([s.prn for s in arr.scene.sats], _snr_rows(arr, w))))
    assert len(found[1]) < len(found[5]) and set(found[1]) <= set(found[5])
    assert len(found[5]) >= 6 and found[5] == S.FOUND[kind, raw_u8, 5] and found[1] == S.FOUND[kind, raw_u8, 1]
    for s, (f, d) in found[5].items():
        assert abs(f - CLEAN[s][0]) <= 200.0, (s, f, d)
        dd = abs(d - CLEAN[s][1])
        assert min(dd, 2048 - dd) <= 1, (s, f, d)


def test_clean_scene_passes_antenna_0_through_at_every_tap_count():
    clean = S.stap_scene('clean')
    assert S.oracle_sweep(lambda b: clean.block(b)[0]) == CLEAN
    n = clean.ngps
    x = clean.block(0)
    for T in (1, 3, 5, 7):
        for b in range(2):
            xb = clean.block(b)
            y, flag, g, w = S.StapRef(n, S.A2, T).process(xb)
            assert flag == 0 and g < 1.0 and y.tobytes() == xb[0].tobytes()
            assert w[0, (T - 1) // 2] == 1.0 and np.abs(w).sum() == 1.0
    raw = clean.block_raw(0)
    y, flags, _, _ = S.StapRef(n, S.A2, 5).run(raw)
    assert not flags.any() and y[0].tobytes() == R.decode(raw[0]).tobytes() == x[0].tobytes()
