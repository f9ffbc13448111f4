"""Thin Python objects over the C ABI: device buffers, the acquisition engine and
the tracking engine.  All arithmetic happens in libgpsmi.so on the GPU; these
classes only marshal numpy arrays and keep handles alive."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib, codes
from ._lib import (CANCEL_OUT_DTYPE, CANCEL_SAT_DTYPE, EngineError, OUT_DTYPE, PEAK_DTYPE,  # noqa: F401
                   REFINE_HIT_DTYPE, REFINE_OUT_DTYPE, STATE_DTYPE, WTRK_BIT_DTYPE, WTRK_STATE_DTYPE, check, ptr)


@dataclass
class Config:
    """The gpsglob.py constants the path depends on (reference
    src/gpsglob.py:35-131)."""
    code_samples: int = 2048
    n_cyc: int = 32
    corr_avg: int = 8
    sweep_corr_avg: int = 4
    corr_min: float = 8.0
    min_freq: float = -5000.0
    max_freq: float = 5000.0
    step_freq: float = 200
    it_sweep: int = 40
    it_sweep_all: int = 10
    max_sat: int = 11
    device: int = 0

    @property
    def ngps(self):
        return self.code_samples * self.n_cyc

    @property
    def sample_rate(self):
        return 1000 * self.code_samples

    def c_struct(self):
        return _lib.Cfg(self.code_samples, self.n_cyc, self.corr_avg,
                        self.sweep_corr_avg, self.corr_min, self.min_freq,
                        self.max_freq, self.device)


def set_default(key, value):
    """Process-wide default of a create-time / tuning option (gpsmi_set_default, gpsmi.h)."""
    check(_lib.load().gpsmi_set_default(key.encode(), int(value)), 'gpsmi_set_default')


def clear_default(key):
    check(_lib.load().gpsmi_clear_default(key.encode()), 'gpsmi_clear_default')


def device_count():
    n = C.c_int(0)
    check(_lib.load().gpsmi_device_count(C.byref(n)), 'gpsmi_device_count')
    return n.value


def device_name(device=0):
    buf = C.create_string_buffer(256)
    check(_lib.load().gpsmi_device_name(device, buf, 256), 'gpsmi_device_name')
    return buf.value.decode()


class DeviceBuffer:
    """A block of HBM owned by Python (IQ kept resident between calls)."""

    def __init__(self, nbytes, device=0):
        self.lib = _lib.load()
        self.device = device
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(self.lib.gpsmi_dev_alloc(device, self.nbytes, C.byref(p)),
              'gpsmi_dev_alloc')
        self.ptr = p

    def upload(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        if offset + arr.nbytes > self.nbytes:
            raise ValueError('upload exceeds the buffer')
        dst = C.c_void_p(self.ptr.value + offset)
        check(self.lib.gpsmi_dev_upload(self.device, dst, ptr(arr), arr.nbytes),
              'gpsmi_dev_upload')

    def download(self, dtype, count, offset=0):
        return self.download_into(np.empty(count, dtype=dtype), offset)

    def download_into(self, out, offset=0):
        """Fills `out` (C-contiguous, e.g. page-locked) from the buffer; -> out."""
        if offset + out.nbytes > self.nbytes:
            raise ValueError('download exceeds the buffer')
        src = C.c_void_p(self.ptr.value + offset)
        check(self.lib.gpsmi_dev_download(self.device, ptr(out), src,
                                          out.nbytes), 'gpsmi_dev_download')
        return out

    def at(self, offset):
        return C.c_void_p(self.ptr.value + int(offset))

    def free(self):
        if self.ptr:
            check(self.lib.gpsmi_dev_free(self.device, self.ptr),
                  'gpsmi_dev_free')
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PinnedArray:
    """numpy array over page-locked host memory (hipHostMalloc)."""

    def __init__(self, shape, dtype):
        self.lib = _lib.load()
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        check(self.lib.gpsmi_host_alloc(max(n, 1), C.byref(p)),
              'gpsmi_host_alloc')
        self._p = p
        buf = (C.c_char * n).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=dtype).reshape(shape)

    def free(self):
        if self._p:
            self.array = None
            check(self.lib.gpsmi_host_free(self._p), 'gpsmi_host_free')
            self._p = None


def unpack_u8iq(d_out, d_raw, n, device=0):
    """raw uint16 (Q<<8|I) -> complex64 on the device (gpsrecv.py:170-172)."""
    check(_lib.load().gpsmi_dev_unpack_u8iq(device, d_out, d_raw, n),
          'gpsmi_dev_unpack_u8iq')


def sync(device=0):
    check(_lib.load().gpsmi_dev_sync(device), 'gpsmi_dev_sync')


def collective_grid(n_e=1, n_n=1, n_t=1, pool=1, e0=0.0, n0=0.0, t0=0.0, d_e=0.0, d_n=0.0, d_t=0.0):
    """The grid of a collective search (gpsmi_collective_grid): n_e x n_n x n_t points from
    (e0, n0, t0) in steps (d_e, d_n, d_t), clock lags in steps of `pool` samples."""
    return _lib.CollectiveGrid(int(n_e), int(n_n), int(n_t), int(pool), float(e0), float(n0),
                               float(t0), float(d_e), float(d_n), float(d_t))


def collective_plan(code_samples, nsv_rows, nbins, sats, grid):
    """gpsmi_acq_collective_plan: the argument checks of AcqEngine.collective without a GPU.
    -> (scratch_bytes, workgroups); EngineError where the call would refuse."""
    sats = np.ascontiguousarray(sats, dtype=_lib.COLLECTIVE_SAT_DTYPE)
    g = grid if isinstance(grid, _lib.CollectiveGrid) else collective_grid(**grid)
    scratch, wgs = C.c_size_t(), C.c_int()
    check(_lib.load().gpsmi_acq_collective_plan(
        int(code_samples), int(nsv_rows), int(nbins), ptr(sats), len(sats), C.byref(g),
        C.byref(scratch), C.byref(wgs)), 'gpsmi_acq_collective_plan')
    return scratch.value, wgs.value


PEAKS_PICK_DTYPE = _lib.PEAKS_PICK_DTYPE
MAX_PEAK_ROWS = _lib.MAX_PRN + 1          # kPeaksMaxRows


def peaks_cfg(nbins, k=4, guard_lags=-1, bins=None):
    """The options of AcqEngine.peaks (gpsmi_peaks_cfg).  bins: the inclusive window (lo, hi), by
    default the whole row."""
    lo, hi = (0, int(nbins) - 1) if bins is None else bins
    return _lib.PeaksCfg(int(k), int(guard_lags), int(lo), int(hi))


def peaks_plan(code_samples, nsv_rows, nbins, k=4, guard_lags=-1, bins=None):
    """gpsmi_acq_peaks_plan: the argument checks of AcqEngine.peaks without a GPU.
    -> (scratch_bytes, workgroups); EngineError where the call would refuse."""
    c = peaks_cfg(nbins, k, guard_lags, bins)
    scratch, wgs = C.c_size_t(), C.c_int()
    check(_lib.load().gpsmi_acq_peaks_plan(int(code_samples), int(nsv_rows), int(nbins), C.byref(c),
                                           C.byref(scratch), C.byref(wgs)), 'gpsmi_acq_peaks_plan')
    return scratch.value, wgs.value


def search_array_plan(code_samples, n, antennas, nbins, n_coh, n_seg, f_offset=0.0, carrier_hz=1575.42e6):
    """gpsmi_acq_search_array_plan: the argument checks of AcqEngine.search_array that need no
    handle, without a GPU, for rows of `n` samples.  -> (scratch_bytes of a launch, bins a launch
    takes); EngineError where the call would refuse."""
    scratch, nbc = C.c_size_t(), C.c_int()
    check(_lib.load().gpsmi_acq_search_array_plan(
        int(code_samples), int(n), int(antennas), int(nbins), int(n_coh), int(n_seg), float(carrier_hz),
        float(f_offset), C.byref(scratch), C.byref(nbc)), 'gpsmi_acq_search_array_plan')
    return scratch.value, nbc.value


def _records(sats, dtype):
    """Refined records as the table a stage takes: (prn, f_hz, tau), or (prn, skip_ms, f_hz, tau)
    where the stage has a second int32 (CANCEL_SAT_DTYPE, SIG_SAT_DTYPE and PROF_SAT_DTYPE are one
    layout; the field is `reserved`, 0, in the first two)."""
    s_a = np.zeros(len(sats), dtype=dtype)
    for i, s in enumerate(sats):
        prn, second, f_hz, tau = s if len(s) == 4 else (s[0], 0, s[1], s[2])
        s_a[i] = (int(prn), int(second), float(f_hz), float(tau))
    return s_a


def _sig_cfg(antennas, n_ms, f_offset, carrier_hz):
    return _lib.SigCfg(int(antennas), int(n_ms), float(carrier_hz), float(f_offset))


def _prof_cfg(half_taps, coh_ms, n_runs, f_offset, carrier_hz):
    return _lib.ProfCfg(int(half_taps), int(coh_ms), int(n_runs), 0, float(carrier_hz), float(f_offset))


def _counts_plan(lib, name, code_samples, n, s_a, cfg, n_extra):
    """A `_plan` export that writes a count per record and n_extra ints behind them -> (counts int32
    [R], the ints...)."""
    counts = np.zeros(max(len(s_a), 1), np.int32)
    extra = [C.c_int(0) for _ in range(n_extra)]
    check(getattr(lib, name)(int(code_samples), int(n), ptr(s_a), len(s_a), C.byref(cfg), ptr(counts),
                             *map(C.byref, extra)), name)
    return (counts[:len(s_a)], *(e.value for e in extra))


def signature_plan(code_samples, n, sats, antennas, n_ms=0, f_offset=0.0, carrier_hz=1575.42e6):
    """gpsmi_acq_signature_plan: the argument checks of AcqEngine.signatures without a GPU, for
    rows of `n` samples.  -> (n_win int32 [R], max_windows); EngineError where the call would
    refuse."""
    return _counts_plan(_lib.load(), 'gpsmi_acq_signature_plan', code_samples, n, _records(sats, _lib.SIG_SAT_DTYPE),
                        _sig_cfg(antennas, n_ms, f_offset, carrier_hz), 1)


def profiles_plan(code_samples, n, sats, half_taps=0, coh_ms=0, n_runs=0, f_offset=0.0, carrier_hz=1575.42e6):
    """gpsmi_acq_profile_plan: the argument checks of AcqEngine.profiles without a GPU, for `n`
    samples.  sats: [(prn, skip_ms, f_hz, tau)].  -> (n_runs int32 [R], max_runs, taps K);
    EngineError where the call would refuse."""
    return _counts_plan(_lib.load(), 'gpsmi_acq_profile_plan', code_samples, n, _records(sats, _lib.PROF_SAT_DTYPE),
                        _prof_cfg(half_taps, coh_ms, n_runs, f_offset, carrier_hz), 2)


def _iq_dtype(raw_u8):
    """What a handle's input format holds per sample: the recorder's uint16 (Q << 8 | I) or complex64."""
    return np.uint16 if raw_u8 else np.complex64


def _host_block(a, raw_u8, what):
    """A host array handed to a handle, C-contiguous, in its input format (a silent cast would
    turn one format into garbage of the other)."""
    a = np.asarray(a)
    if a.dtype != _iq_dtype(raw_u8):
        raise TypeError(f'{what} dtype {a.dtype} does not match the input format '
                        f'({np.dtype(_iq_dtype(raw_u8)).name}; see set_input_format)')
    return np.ascontiguousarray(a)


def _spectrum_c64(prn, cs):
    return np.ascontiguousarray(codes.replica_spectrum(prn, cs)
                                .astype(np.complex64))


class AcqEngine:
    """Search surface of gpsrecv.sweepAllSats (reference gpsrecv.py:241-274)."""

    def __init__(self, cfg=None, prns=range(1, 38)):
        self.cfg = cfg or Config()
        self.lib = _lib.load()
        h = C.c_void_p()
        cs = self.cfg.c_struct()
        check(self.lib.gpsmi_acq_create(C.byref(cs), C.byref(h)),
              'gpsmi_acq_create')
        self.h = h
        self._have_time = set()        # PRNs whose GPSCacode a 2048 handle holds (refine)
        for p in prns:
            if self.cfg.code_samples == 2048:
                spec = _spectrum_c64(p, self.cfg.code_samples)
                check(self.lib.gpsmi_acq_set_replica(self.h, p, ptr(spec)),
                      'gpsmi_acq_set_replica')
            else:                      # time-domain correlation for other code lengths
                rep = np.ascontiguousarray(
                    codes.code_replica(p, self.cfg.code_samples).astype(np.float32))
                check(self.lib.gpsmi_acq_set_replica_time(self.h, p, ptr(rep)),
                      'gpsmi_acq_set_replica_time')

    raw_u8 = False

    def set_input_format(self, raw_u8):
        """raw_u8 = True: the iq of the searches that follow is the recorder's uint16
        (Q << 8 | I) samples (gpsrecv.py:162-173), decoded inside the wipe-off kernel."""
        check(self.lib.gpsmi_acq_set_input_format(self.h, 1 if raw_u8 else 0),
              'gpsmi_acq_set_input_format')
        self.raw_u8 = bool(raw_u8)

    def _host_iq(self, iq):
        return _host_block(iq, self.raw_u8, 'iq')

    def _input(self, iq, nbr=False, lead=None):
        """iq of any entry point -> (pointer, n, host?): a host array in the input format, or a
        (c_void_p, n) device pair as it is (the neighbours `nbr` come back for host input only).
        lead: the shape a host array must have in front of its n samples -- () for one row, (A,) for
        one row per antenna; None: any shape, n all its samples."""
        if isinstance(iq, tuple):
            if nbr:
                raise ValueError('nbr is returned for host input only')
            return iq[0], int(iq[1]), False
        iq = self._host_iq(iq)
        if lead is None:
            return ptr(iq), iq.size, True          # (the pointer keeps the array alive)
        if iq.ndim != len(lead) + 1 or iq.shape[:-1] != lead:
            raise ValueError('data must be ' + (f'[{lead[0]}][n], one row per antenna' if lead else
                                                'one row of samples'))
        return ptr(iq), iq.shape[-1], True

    @staticmethod
    def _tables(prns, freqs, nbr=False):
        """The tables of a search -> (the four arguments that name the PRNs and the bins, the
        PEAK_DTYPE table [nbins, nsv] it fills, the neighbours float32 [nbins, nsv, 2] or None)."""
        prn_a = np.ascontiguousarray(prns, dtype=np.int32)
        f_a = np.ascontiguousarray(freqs, dtype=np.float64)
        out = np.zeros((len(f_a), len(prn_a)), dtype=PEAK_DTYPE)
        nb = np.zeros((len(f_a), len(prn_a), 2), dtype=np.float32) if nbr else None
        return (ptr(prn_a), len(prn_a), ptr(f_a), len(f_a)), out, nb

    def _export(self, name, host):
        """The entry point `name` for host input, its `_dev` twin for device input -> (function, its name)."""
        name = name if host else name + '_dev'
        return getattr(self.lib, name), name

    def search(self, iq, prns, freqs, n_avg, out_dev=None):
        """iq: complex64 numpy array (host; uint16 after set_input_format(True)) or a
        (c_void_p, n) device pair.
        Returns a structured array [nbins, nsv] of (argmax, peak, mean, std)."""
        tab, out, _ = self._tables(prns, freqs)
        d_iq, n, host = self._input(iq)
        fn, name = self._export('gpsmi_acq_search', host)
        check(fn(self.h, d_iq, n, *tab, n_avg, ptr(out), *(() if host else (out_dev,))), name)
        return out

    def search_noncoherent(self, iq, prns, freqs, n_coh, n_seg, out_dev=None, nbr=False):
        """Non-coherent search (gpsmi_acq_search_nc): per cell the mean of the correlation
        magnitudes of n_seg consecutive segments of n_coh code periods, each segment searched as
        search() does with n_avg = n_coh.  iq: host array in the input format, or a
        (c_void_p, n) device pair.  Returns the PEAK_DTYPE table [nbins, nsv] of that mean
        surface, and with nbr=True also its values left / right of every argmax
        (float32 [nbins, nsv, 2]; host input only)."""
        tab, out, nb = self._tables(prns, freqs, nbr)
        d_iq, n, host = self._input(iq, nbr)
        fn, name = self._export('gpsmi_acq_search_nc', host)
        check(fn(self.h, d_iq, n, *tab, int(n_coh), int(n_seg), ptr(out), ptr(nb) if host else out_dev), name)
        return (out, nb) if nbr else out

    L1_HZ = 1575.42e6

    def search_deep(self, iq, prns, freqs, n_coh, n_seg, f_offset=0.0, carrier_hz=L1_HZ,
                    out_dev=None, nbr=False, rows=None):
        """Deep search (gpsmi_acq_search_deep): search_noncoherent with the code Doppler
        compensated, for spans of seconds.  The magnitudes of segment s of bin f are added at the
        lag they had at the start of iq: rotated by rint(-(f - f_offset) / carrier_hz * s * n_coh *
        code_samples) samples.  f_offset: what the bin frequencies differ from the true Doppler
        by (a tuner's frequency error).  Arguments and returns otherwise as search_noncoherent;
        the argmax is the code phase at the start of iq.
        rows: a DeviceBuffer of at least nsv * nbins * code_samples * 4 bytes that receives the
        surface of every cell, float32 [nsv][nbins][code_samples] (gpsmi_acq_search_deep_rows_dev;
        host input is uploaded first; not together with nbr).  The table is the same bytes."""
        tab, out, nb = self._tables(prns, freqs, nbr)
        if rows is not None:
            if nbr:
                raise ValueError('nbr is not returned together with rows')
            need = out.size * self.cfg.code_samples * 4
            if rows.nbytes < need:
                raise ValueError(f'rows holds {rows.nbytes} bytes, the surfaces need {need}')
        d_iq, n, host = self._input(iq, nbr)
        held = None
        if rows is not None and host:              # the rows entry point reads device memory alone
            nbytes = n * np.dtype(_iq_dtype(self.raw_u8)).itemsize
            held = DeviceBuffer(max(nbytes, 1), self.cfg.device)
            check(self.lib.gpsmi_dev_upload(held.device, held.ptr, d_iq, nbytes), 'gpsmi_dev_upload')
            d_iq, host = held.ptr, False
        name = 'gpsmi_acq_search_deep' + ('' if host else '_dev' if rows is None else '_rows_dev')
        last = (ptr(nb),) if host else (out_dev,) if rows is None else (out_dev, rows.ptr)
        try:
            check(getattr(self.lib, name)(self.h, d_iq, n, *tab, int(n_coh), int(n_seg), float(carrier_hz),
                                          float(f_offset), ptr(out), *last), name)
        finally:
            if held is not None:
                held.free()
        return (out, nb) if nbr else out

    def search_array(self, data, antennas, prns, freqs, n_coh, n_seg, f_offset=0.0, carrier_hz=L1_HZ,
                     out_dev=None, nbr=False, rows=None):
        """Array search (gpsmi_acq_search_array): search_deep over `antennas` = 2 .. 4 rows at once,
        the complex correlations of the rows combined per lag,
            T = (sum_s sum_a |c_a|^2 + 2 sum_{a<b} |sum_s c_a conj(c_b)|) / (antennas n_seg),
        so that a satellite no single row shows stands out by the gain of the array.  data: [A][n]
        on the host in the input format, antenna 0 first, or a (c_void_p, n) device pair of such
        rows of n samples.  Arguments and returns otherwise as search_deep; the table holds the
        records of T, a power.  rows: a DeviceBuffer that receives T of every cell, float32
        [nsv][nbins][code_samples] (host input is uploaded first; not together with nbr)."""
        A = int(antennas)
        tab, out, nb = self._tables(prns, freqs, nbr)
        if rows is not None:
            if nbr:
                raise ValueError('nbr is not returned together with rows')
            need = out.size * self.cfg.code_samples * 4
            if rows.nbytes < need:
                raise ValueError(f'rows holds {rows.nbytes} bytes, the surfaces need {need}')
        d_iq, n, host = self._input(data, nbr, lead=None if isinstance(data, tuple) else (A,))
        held = None
        if rows is not None and host:              # only the device entry point keeps rows
            nbytes = A * n * np.dtype(_iq_dtype(self.raw_u8)).itemsize
            held = DeviceBuffer(max(nbytes, 1), self.cfg.device)
            check(self.lib.gpsmi_dev_upload(held.device, held.ptr, d_iq, nbytes), 'gpsmi_dev_upload')
            d_iq, host = held.ptr, False
        fn, name = self._export('gpsmi_acq_search_array', host)
        last = (ptr(nb),) if host else (out_dev, None if rows is None else rows.ptr)
        try:
            check(fn(self.h, d_iq, n, A, *tab, int(n_coh), int(n_seg), float(carrier_hz), float(f_offset),
                     ptr(out), *last), name)
        finally:
            if held is not None:
                held.free()
        return (out, nb) if nbr else out

    def collective(self, rows, sats, grid, nsv_rows=None, nbins=None):
        """Collective detection (gpsmi_acq_collective_dev) over the surfaces `rows` that
        search_deep(..., rows=) left: a DeviceBuffer of float32 [nsv_rows][nbins][code_samples].
        sats: COLLECTIVE_SAT_DTYPE records (row, bin_lo, bin_hi, lag0, g_e, g_n, g_t); grid: a dict
        or _lib.CollectiveGrid of n_e, n_n, n_t, pool, e0, n0, t0, d_e, d_n, d_t.  nsv_rows and
        nbins describe the rows; by default the largest row and bin the satellites name, plus one.
        Returns the cell map, COLLECTIVE_CELL_DTYPE [n_t, n_n, n_e]: per grid point the best
        clock lag and its score."""
        sats = np.ascontiguousarray(sats, dtype=_lib.COLLECTIVE_SAT_DTYPE)
        g = grid if isinstance(grid, _lib.CollectiveGrid) else collective_grid(**grid)
        if nsv_rows is None:
            nsv_rows = int(sats['row'].max()) + 1 if len(sats) else 1
        if nbins is None:
            nbins = int(sats['bin_hi'].max()) + 1 if len(sats) else 1
        need = int(nsv_rows) * int(nbins) * self.cfg.code_samples * 4
        if rows.nbytes < need:
            raise ValueError(f'rows holds {rows.nbytes} bytes, [{nsv_rows}][{nbins}] surfaces are {need}')
        shape = (max(g.n_t, 0), max(g.n_n, 0), max(g.n_e, 0))
        cells = shape[0] * shape[1] * shape[2]
        out = np.zeros(shape if 0 < cells <= _lib.COLLECTIVE_MAX_CELLS else (1, 1, 1),
                       dtype=_lib.COLLECTIVE_CELL_DTYPE)
        check(self.lib.gpsmi_acq_collective_dev(
            self.h, rows.ptr, int(nsv_rows), int(nbins), ptr(sats), len(sats), C.byref(g), ptr(out),
            None), 'gpsmi_acq_collective_dev')
        return out

    def peaks_plan(self, nsv_rows, nbins, k=4, guard_lags=-1, bins=None):
        """peaks_plan at the engine's code length."""
        return peaks_plan(self.cfg.code_samples, nsv_rows, nbins, k, guard_lags, bins)

    def peaks(self, d_rows, nsv_rows, nbins, k=4, guard_lags=-1, bins=None, cols=True, out_dev=None,
              cols_dev=None):
        """Auxiliary peaks (gpsmi_acq_peaks_dev) over the surfaces `d_rows` that
        search_deep(..., rows=) left: a DeviceBuffer of float32 [nsv_rows][nbins][code_samples].
        Per satellite the k largest values of z = (S - mean) / std over the bins of the window
        `bins` (inclusive (lo, hi), by default all), more than guard_lags apart (circular; -1: two
        chips).  Returns (picks, cols): PEAKS_PICK_DTYPE [nsv_rows, k] (lag, bin, z, s; -1, -1, 0, 0
        where there is no pick) and, with cols=True, float32 [nsv_rows, k, 2, nbins]: S and z down
        the bins at every picked lag (else None).  out_dev / cols_dev: device pointers that receive
        the same bytes."""
        c = peaks_cfg(nbins, k, guard_lags, bins)
        need = int(nsv_rows) * int(nbins) * self.cfg.code_samples * 4
        if need > 0 and d_rows.nbytes < need:
            raise ValueError(f'rows holds {d_rows.nbytes} bytes, [{nsv_rows}][{nbins}] surfaces are {need}')
        ok = 0 < int(nsv_rows) <= MAX_PEAK_ROWS and 0 < int(nbins) <= 4096 and 0 < c.k <= _lib.PEAKS_MAX_K
        shape = (int(nsv_rows), c.k) if ok else (1, 1)        # (a refused call writes nothing)
        picks = np.zeros(shape, dtype=PEAKS_PICK_DTYPE)
        col = np.zeros(shape + (2, int(nbins) if ok else 1), np.float32) if cols else None
        check(self.lib.gpsmi_acq_peaks_dev(self.h, d_rows.ptr, int(nsv_rows), int(nbins), C.byref(c), ptr(picks),
                                           out_dev, ptr(col), cols_dev), 'gpsmi_acq_peaks_dev')
        return picks, col

    def refine(self, iq, hits, n_ms, df_step=2.0, df_half=120.0, tap_samples=0, f_offset=0.0,
               carrier_hz=L1_HZ, min_ratio=2.5, want_grid=False, want_prompts=False):
        """Refinement of weak / deep hits (gpsmi_acq_refine): per hit (prn, freq, delay) -- the SV,
        the bin and the argmax a non-coherent or deep search returned for the start of iq -- the
        fine Doppler, the bit edge, a sub-sample code phase, C/N0 and a detection ratio from n_ms
        milliseconds (a multiple of 20) of 1-ms prompts summed coherently over each data bit.
        iq as in search_deep.  Returns a REFINE_OUT_DTYPE array [nhits]; with want_grid /
        want_prompts a tuple with the grid float32 [nhits, n_df, 20] and / or the prompts
        complex64 [nhits, 3, n_ms] (early, prompt, late) behind it."""
        cs = self.cfg.code_samples
        h_a = np.zeros(len(hits), dtype=REFINE_HIT_DTYPE)
        for i, (prn, freq, delay) in enumerate(hits):
            h_a[i] = (int(prn), int(delay), float(freq))
        self._need_time_replicas(h_a['prn'])   # the FFT searches never needed GPSCacode itself
        cfg = _lib.RefineCfg(int(n_ms), int(tap_samples), float(df_step), float(df_half),
                             float(carrier_hz), float(f_offset), float(min_ratio), 0)
        d_iq, n, host = self._input(iq)
        n_df = C.c_int(0)
        check(self.lib.gpsmi_acq_refine_plan(cs, n, ptr(h_a), len(h_a), C.byref(cfg),
                                             C.byref(n_df)), 'gpsmi_acq_refine_plan')
        out = np.zeros(len(h_a), dtype=REFINE_OUT_DTYPE)
        grid = np.zeros((len(h_a), n_df.value, 20), np.float32) if want_grid else None
        prompts = np.zeros((len(h_a), 3, int(n_ms)), np.complex64) if want_prompts else None
        fn, name = self._export('gpsmi_acq_refine', host)
        check(fn(self.h, d_iq, n, ptr(h_a), len(h_a), C.byref(cfg), ptr(out), ptr(grid), ptr(prompts)), name)
        extra = [a for a in (grid, prompts) if a is not None]
        return (out, *extra) if extra else out

    def _need_time_replicas(self, prns):
        """A 2048 handle holds GPSCacode only for the PRNs refine / track_weak have met."""
        cs = self.cfg.code_samples
        if cs != 2048:
            return
        for p in sorted({int(x) for x in prns} - self._have_time):
            if 1 <= p <= 37:
                rep = np.ascontiguousarray(codes.code_replica(p, cs).astype(np.float32))
                check(self.lib.gpsmi_acq_set_replica_time(self.h, p, ptr(rep)),
                      'gpsmi_acq_set_replica_time')
                self._have_time.add(p)

    def track_weak(self, iq, states, n_bits, first_sample=0, tap_samples=0, pll_bw=0.0, fll_bw=0.0,
                   dll_bw=0.0, pull_in_bits=0, f_offset=0.0, carrier_hz=L1_HZ):
        """Bit-synchronous tracking of refined hits (gpsmi_acq_track): every channel of `states`
        (WTRK_STATE_DTYPE, from acquisition.open_weak_channels or an earlier call) is tracked over
        up to n_bits 20-ms data bits of iq, whose first sample has stream index first_sample.
        Bandwidths of 0 take the defaults; a negative pll_bw / fll_bw switches that term off.  iq
        as in search_deep.  Returns (records WTRK_BIT_DTYPE [nhits, n_bits], states): the records
        past a channel's last bit are zero, and states['bit_no'] tells how far each channel got."""
        st = np.array(states, dtype=WTRK_STATE_DTYPE, ndmin=1, copy=True)
        st = np.ascontiguousarray(st)
        self._need_time_replicas(st['prn'])
        cfg = _lib.WtrkCfg(int(n_bits), int(tap_samples), float(pll_bw), float(fll_bw), float(dll_bw),
                           float(carrier_hz), float(f_offset), int(first_sample), int(pull_in_bits), 0)
        d_iq, n, host = self._input(iq)
        check(self.lib.gpsmi_acq_track_plan(self.cfg.code_samples, n, ptr(st), len(st), C.byref(cfg)),
              'gpsmi_acq_track_plan')
        bits = np.zeros((len(st), int(n_bits)), dtype=WTRK_BIT_DTYPE)
        fn, name = self._export('gpsmi_acq_track', host)
        check(fn(self.h, d_iq, n, ptr(st), len(st), C.byref(cfg), ptr(bits)), name)
        return bits, st

    def cancel(self, data, sats, out=None, f_offset=0.0, coef=False, carrier_hz=L1_HZ, min_window=0):
        """Cancellation of strong satellites (gpsmi_acq_cancel): every satellite
        of `sats` -- (prn, f_hz, tau) with the Doppler to a few Hz and tau any of its code starts in
        samples from the first sample, to half a sample -- is projected out of the samples code
        period by code period, in the order given (the strongest first).  data: a host array in
        the input format, or a (device pointer, n) pair.  out: where the complex64 result goes --
        host data: an optional complex64 array [n]; device data: a device pointer to complex64
        [n], None = in place (complex64 input only).  Returns (out, records CANCEL_OUT_DTYPE
        [nsat]), and with coef=True the windows' coefficients complex64 [nsat, max_windows, 3]
        behind them."""
        s_a = _records(sats, CANCEL_SAT_DTYPE)
        self._need_time_replicas(s_a['prn'])
        cfg = _lib.CancelCfg(float(carrier_hz), float(f_offset), int(min_window), 0)
        d_iq, n, host = self._input(data)
        max_w = C.c_int(0)
        check(self.lib.gpsmi_acq_cancel_plan(self.cfg.code_samples, n, ptr(s_a), len(s_a), C.byref(cfg),
                                             C.byref(max_w)), 'gpsmi_acq_cancel_plan')
        rec = np.zeros(len(s_a), dtype=CANCEL_OUT_DTYPE)
        co = np.zeros((len(s_a), max_w.value, 3), np.complex64) if coef else None
        if host:
            if out is None:
                out = np.empty(n, np.complex64)
            if out.dtype != np.complex64 or out.size != n or not out.flags['C_CONTIGUOUS']:
                raise TypeError('out must be a C-contiguous complex64 array of the length of data')
        elif out is None:
            if self.raw_u8:
                raise ValueError('raw input cannot be cancelled in place: pass a complex64 device buffer')
            out = d_iq
        fn, name = self._export('gpsmi_acq_cancel', host)
        check(fn(self.h, d_iq, n, ptr(s_a), len(s_a), C.byref(cfg), ptr(out) if host else out, ptr(rec), ptr(co)),
              name)
        return (out, rec, co) if coef else (out, rec)

    def signatures(self, data, sats, antennas, n_ms=0, f_offset=0.0, carrier_hz=L1_HZ, prompts=False):
        """Spatial signatures over several coherent antennas (gpsmi_acq_signature):
        per record of `sats` -- (prn, f_hz, tau) as in cancel; a PRN may appear more than once --
        the 1-ms prompts of every antenna at the record's code starts and their covariance over the
        antennas.  data: a host array [antennas][n] in the input format, or a (device pointer, n)
        pair with the rows n samples apart.  n_ms: the windows taken per record (0: all that fit).
        Returns (cov complex128 [R][A][A], n_win int32 [R]) and with prompts=True the prompts
        complex64 [R][A][max_windows] behind them (zero past a record's last window)."""
        A = int(antennas)
        return self._cov_stage('gpsmi_acq_signature', data, (A,), _records(sats, _lib.SIG_SAT_DTYPE),
                               _sig_cfg(A, n_ms, f_offset, carrier_hz), A, prompts)

    def _cov_stage(self, name, data, lead, s_a, cfg, D, sums):
        """signatures and profiles behind their arguments: the `_plan` export sizes the results (the
        width of the sums, and behind it the order D of the covariances where D is None), then the
        call.  -> (cov complex128 [R][D][D], counts int32 [R]) and with `sums` the sums complex64
        [R][D][width] behind them."""
        self._need_time_replicas(s_a['prn'])
        d_iq, n, host = self._input(data, lead=lead)
        counts, width, *order = _counts_plan(self.lib, name + '_plan', self.cfg.code_samples, n, s_a, cfg,
                                             2 if D is None else 1)
        D = order[0] if D is None else D
        cov = np.zeros((len(s_a), D, D), np.complex128)
        sm = np.zeros((len(s_a), D, width), np.complex64) if sums else None
        fn, name = self._export(name, host)
        check(fn(self.h, d_iq, n, ptr(s_a), len(s_a), C.byref(cfg), ptr(cov), ptr(counts), ptr(sm)), name)
        return (cov, counts, sm) if sums else (cov, counts)

    def profiles(self, data, sats, half_taps=0, coh_ms=0, n_runs=0, f_offset=0.0, carrier_hz=L1_HZ, sums=False):
        """Multi-tap correlation profiles on one antenna (gpsmi_acq_profile): per
        record of `sats` -- (prn, skip_ms, f_hz, tau), f_hz and tau as in signatures, skip_ms the
        windows dropped up to the bit edge; a PRN may appear more than once -- the correlation at
        the whole-sample lags -half_taps .. +half_taps around the code start, summed coherently over
        runs of coh_ms windows, and the covariance of those sums over the taps.  data: a host array
        of n samples in the input format, or a (device pointer, n) pair.  0 for an option: its
        default (8 taps either side at 2048, 32 at 16368; 20 ms; every run that fits).
        Returns (cov complex128 [R][K][K], n_runs int32 [R]) and with sums=True the sums complex64
        [R][K][max_runs] behind them (zero past a record's last run)."""
        return self._cov_stage('gpsmi_acq_profile', data, (), _records(sats, _lib.PROF_SAT_DTYPE),
                               _prof_cfg(half_taps, coh_ms, n_runs, f_offset, carrier_hz),
                               None, sums)

    def search_async(self, d_iq, n, prns, freqs, n_avg, out, out_dev=None):
        """Enqueue a search on device-resident iq; `out` is a pinned PEAK_DTYPE
        array [nbins, nsv] filled when wait() returns."""
        prn_a = np.ascontiguousarray(prns, dtype=np.int32)
        f_a = np.ascontiguousarray(freqs, dtype=np.float64)
        check(self.lib.gpsmi_acq_search_dev_async(
            self.h, d_iq, n, ptr(prn_a), len(prn_a), ptr(f_a), len(f_a), n_avg,
            ptr(out), out_dev), 'gpsmi_acq_search_dev_async')

    def wait(self):
        check(self.lib.gpsmi_acq_wait(self.h), 'gpsmi_acq_wait')

    def after(self, trk_engine):
        """Later searches start when the TrkEngine's enqueued work is done."""
        check(self.lib.gpsmi_acq_after_trk(self.h, trk_engine.h), 'gpsmi_acq_after_trk')

    def search_ex(self, iq, prns, freqs, n_avg):
        """search() plus corr[argmax-1], corr[argmax+1] per cell: (table, nbr)."""
        tab, out, nbr = self._tables(prns, freqs, True)
        d_iq, n, _ = self._input(self._host_iq(iq))      # (host input only)
        check(self.lib.gpsmi_acq_search_ex(self.h, d_iq, n, *tab, n_avg, ptr(out), ptr(nbr)), 'gpsmi_acq_search_ex')
        return out, nbr

    def last_ms(self):
        ms = C.c_float(0)
        check(self.lib.gpsmi_acq_last_ms(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            self.lib.gpsmi_acq_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TrkEngine:
    """All tracking channels of one GPU (numeric part of SatStream.process,
    reference gpslib.py:1141-1210)."""

    def __init__(self, cfg=None, max_ch=12, prns=range(1, 38), streams=1):
        """streams > 1: that many independent receivers (IQ streams) share the handle and
        every launch (gpsmi_trk_set_streams); a channel is then addressed as (ch, stream)."""
        self.cfg = cfg or Config()
        self.max_ch = max_ch
        self.streams = 1
        self.lib = _lib.load()
        h = C.c_void_p()
        cs = self.cfg.c_struct()
        check(self.lib.gpsmi_trk_create(C.byref(cs), max_ch, C.byref(h)),
              'gpsmi_trk_create')
        self.h = h
        if streams != 1:
            check(self.lib.gpsmi_trk_set_streams(self.h, int(streams)), 'gpsmi_trk_set_streams')
            self.streams = int(streams)
        for p in prns:
            rep = np.ascontiguousarray(
                codes.code_replica(p, self.cfg.code_samples).astype(np.float32))
            spec = _spectrum_c64(p, self.cfg.code_samples)
            check(self.lib.gpsmi_trk_set_replica(self.h, p, ptr(rep), ptr(spec)),
                  'gpsmi_trk_set_replica')

    raw_u8 = False

    def _row(self, ch, stream):
        if self.streams == 1 and stream == 0:
            return ch                         # (the library checks the range itself)
        if not (0 <= ch < self.max_ch and 0 <= stream < self.streams):
            raise ValueError('channel / stream out of range')
        return stream * self.max_ch + ch

    def open(self, ch, prn, freq, delay, stream=0):
        check(self.lib.gpsmi_trk_open(self.h, self._row(ch, stream), prn, float(freq), int(delay)),
              'gpsmi_trk_open')

    def close_channel(self, ch, stream=0):
        check(self.lib.gpsmi_trk_close(self.h, self._row(ch, stream)), 'gpsmi_trk_close')

    def get_state(self, ch, stream=0):
        st = np.zeros(1, dtype=STATE_DTYPE)
        check(self.lib.gpsmi_trk_get_state(self.h, self._row(ch, stream), ptr(st)),
              'gpsmi_trk_get_state')
        return st[0]

    def set_state(self, ch, st, stream=0):
        a = np.zeros(1, dtype=STATE_DTYPE)
        a[0] = st
        check(self.lib.gpsmi_trk_set_state(self.h, self._row(ch, stream), ptr(a)),
              'gpsmi_trk_set_state')

    def erase_prev(self, ch, stream=0):
        check(self.lib.gpsmi_trk_erase_prev(self.h, self._row(ch, stream)), 'gpsmi_trk_erase_prev')

    def process(self, iq, want_out=True):
        """One closed-loop block for every open channel.  iq: complex64[NGPS]
        on the host, or a c_void_p to a device-resident block.  With streams > 1:
        [streams, NGPS] (one block per stream, back to back); out is [streams, max_ch]."""
        shape = self.max_ch if self.streams == 1 else (self.streams, self.max_ch)
        out = np.zeros(shape, dtype=OUT_DTYPE) if want_out else None
        if isinstance(iq, C.c_void_p):
            check(self.lib.gpsmi_trk_process_dev(self.h, iq, self.streams * self.cfg.ngps,
                                                 ptr(out)),
                  'gpsmi_trk_process_dev')
        else:
            iq = _host_block(iq, self.raw_u8, 'block')
            if out is None:
                out = np.zeros(shape, dtype=OUT_DTYPE)
            check(self.lib.gpsmi_trk_process(self.h, ptr(iq), iq.size, ptr(out)),
                  'gpsmi_trk_process')
        return out

    def process_stream(self, iq, out=None):
        """One closed-loop block (per stream) from host memory without waiting for it
        (gpsmi_trk_process_stream): the call returns once the step of the call before last is
        complete, i.e. the host runs at most two steps ahead.  iq: a C-contiguous array in the
        handle's input format, ideally a PinnedArray's, untouched until two later calls (or
        wait()) have returned; out: optional pinned OUT_DTYPE array, valid from the same moment."""
        n = self.streams * self.cfg.ngps
        if iq.size != n or iq.dtype != _iq_dtype(self.raw_u8):
            raise TypeError('block size or dtype does not match the handle')
        if not iq.flags.c_contiguous:
            raise ValueError('the block must be C-contiguous (its address is handed to the device)')
        check(self.lib.gpsmi_trk_process_stream(self.h, ptr(iq), n, ptr(out)),
              'gpsmi_trk_process_stream')

    def process_stream_ptr(self, iq_ptr, out_ptr):
        """process_stream with the two addresses already as ctypes pointers (a caller that cycles
        through a fixed ring of page-locked buffers converts them once): no checks here, the
        library checks the sample count and refuses what it cannot read."""
        rc = self.lib.gpsmi_trk_process_stream(self.h, iq_ptr, self.streams * self.cfg.ngps, out_ptr)
        if rc:
            check(rc, 'gpsmi_trk_process_stream')

    def replay(self, d_iq, nb, table, delay_used=None):
        """nb device-resident blocks, states at block start [nb, max_ch]."""
        table = np.ascontiguousarray(table, dtype=STATE_DTYPE)
        if table.shape != (nb, self.max_ch):
            raise ValueError('table must be [nb, max_ch]')
        if delay_used is not None:
            delay_used = np.ascontiguousarray(delay_used, dtype=np.int32)
            if delay_used.shape != (nb, self.max_ch):
                raise ValueError('delay_used must be [nb, max_ch]')
        out = np.zeros((nb, self.max_ch), dtype=OUT_DTYPE)
        check(self.lib.gpsmi_trk_replay(self.h, d_iq, nb, ptr(table),
                                        ptr(delay_used), ptr(out)),
              'gpsmi_trk_replay')
        return out

    def replay_load(self, nb, table, delay_used=None):
        table = np.ascontiguousarray(table, dtype=STATE_DTYPE)
        if table.shape != (nb, self.max_ch):
            raise ValueError('table must be [nb, max_ch]')
        if delay_used is not None:
            delay_used = np.ascontiguousarray(delay_used, dtype=np.int32)
            if delay_used.shape != (nb, self.max_ch):
                raise ValueError('delay_used must be [nb, max_ch]')
        check(self.lib.gpsmi_trk_replay_load(self.h, nb, ptr(table),
                                             ptr(delay_used)),
              'gpsmi_trk_replay_load')

    def replay_run(self, d_iq, nb):
        check(self.lib.gpsmi_trk_replay_run(self.h, d_iq, nb),
              'gpsmi_trk_replay_run')

    def replay_run_async(self, d_iq, nb):
        check(self.lib.gpsmi_trk_replay_run_async(self.h, d_iq, nb),
              'gpsmi_trk_replay_run_async')

    def replay_fetch_async(self, out):
        check(self.lib.gpsmi_trk_replay_fetch_async(self.h, ptr(out), out.size),
              'gpsmi_trk_replay_fetch_async')

    def wait(self):
        check(self.lib.gpsmi_trk_wait(self.h), 'gpsmi_trk_wait')

    def after(self, acq_engine):
        """Later work of this handle starts when the AcqEngine's enqueued work is done."""
        check(self.lib.gpsmi_trk_after_acq(self.h, acq_engine.h), 'gpsmi_trk_after_acq')

    def set_input_format(self, raw_u8):
        """raw_u8 = True: the blocks handed to process / replay are the recorder's uint16
        (Q << 8 | I) samples (gpsrecv.py:162-173), decoded inside the kernels that read IQ."""
        check(self.lib.gpsmi_trk_set_input_format(self.h, 1 if raw_u8 else 0),
              'gpsmi_trk_set_input_format')
        self.raw_u8 = bool(raw_u8)

    def set_option(self, key, value):
        """A tuning option of this handle (gpsmi_trk_set_option; the keys are listed in gpsmi.h)."""
        check(self.lib.gpsmi_trk_set_option(self.h, key.encode(), int(value)), 'gpsmi_trk_set_option')

    def get_option(self, key):
        v = C.c_longlong(0)
        check(self.lib.gpsmi_trk_get_option(self.h, key.encode(), C.byref(v)), 'gpsmi_trk_get_option')
        return v.value

    def set_timing(self, on):
        """Kernel-timing events for the launches that follow (see gpsmi.h)."""
        check(self.lib.gpsmi_trk_set_timing(self.h, 2 if on == 2 else int(bool(on))), 'gpsmi_trk_set_timing')

    def wait_prev(self):
        """The run before the latest one, and its read-back, are done."""
        check(self.lib.gpsmi_trk_wait_prev(self.h), 'gpsmi_trk_wait_prev')

    def replay_fetch(self, out):
        """out: C-contiguous OUT_DTYPE array (ideally from pinned_array)."""
        check(self.lib.gpsmi_trk_replay_fetch(self.h, ptr(out), out.size),
              'gpsmi_trk_replay_fetch')
        return out

    def replay_states(self, nb):
        st = np.zeros((nb, self.max_ch), dtype=STATE_DTYPE)
        check(self.lib.gpsmi_trk_replay_states(self.h, ptr(st), st.size),
              'gpsmi_trk_replay_states')
        return st

    def last_ms(self):
        a, b = C.c_float(0), C.c_float(0)
        check(self.lib.gpsmi_trk_last_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_codephase_ms(self):
        a = C.c_float(0)
        check(self.lib.gpsmi_trk_last_codephase_ms(self.h, C.byref(a)))
        return a.value

    def close(self):
        if self.h:
            self.lib.gpsmi_trk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dumps_of(rec):
    """complex64 prompt dumps of one gpsmi_trk_out record."""
    n = int(rec['n_dumps'])
    d = rec['dumps']
    return (d[0:2 * n:2] + 1j * d[1:2 * n:2]).astype(np.complex64)
