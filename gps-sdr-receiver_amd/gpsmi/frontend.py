"""Recordings of other SDR front ends -> complex64 blocks at the engine's rate (gpsmi_fe_*, gpsmi.h).

On the GPU, ``FrontEnd`` decodes one of several sample formats, mixes a given IF or tuner offset
down to 0 Hz, band-limits and resamples from any whole-Hz input rate to ``cfg.sample_rate``
(1000 * CODE_SAMPLES).  Its output goes straight into acquisition, excision and tracking, in their
complex64 format (``pipeline.Receiver(raw_u8=False)``).  DESIGN.md 4.2c.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr
from .engine import Config, PinnedArray

# name -> (GPSMI_FE_* code, numpy dtype of one stored value, values per sample)
FORMATS = {
    'c64': (0, np.complex64, 1),
    'u8iq': (1, np.uint16, 1),
    'sc8': (2, np.int8, 2),
    'sc16': (3, np.int16, 2),
    'r8': (4, np.int8, 1),
}


def fe_cfg(fs_in, fs_out, fmt, if_hz=0.0, conjugate=False, passband_hz=None, atten_db=60.0, max_out=1,
           device=0):
    """The gpsmi_fe_cfg of a configuration (fmt: a FORMATS name)."""
    if fmt not in FORMATS:
        raise ValueError(f'unknown sample format {fmt!r}: one of {sorted(FORMATS)}')
    return _lib.FeCfg(int(fs_in), int(fs_out), float(if_hz), float(passband_hz or 0.0), float(atten_db or 0.0),
                      FORMATS[fmt][0], 1 if conjugate else 0, int(max_out), int(device))


def design(fs_in, fs_out, fmt, if_hz=0.0, conjugate=False, passband_hz=None, atten_db=60.0):
    """The filter gpsmi_fe_create would use, computed on the host (no GPU): (n_taps, n_phases,
    table float32 [n_phases + 1, n_taps]); EngineError for a configuration the stage refuses."""
    lib = _lib.load()
    c = fe_cfg(fs_in, fs_out, fmt, if_hz, conjugate, passband_hz, atten_db)
    k, ph = C.c_int(0), C.c_int(0)
    check(lib.gpsmi_fe_design(C.byref(c), C.byref(k), C.byref(ph), None), 'gpsmi_fe_design')
    table = np.zeros((ph.value + 1, k.value), dtype=np.float32)
    check(lib.gpsmi_fe_design(C.byref(c), C.byref(k), C.byref(ph), ptr(table)), 'gpsmi_fe_design')
    return k.value, ph.value, table


class FrontEnd:
    """One streaming front-end handle: input at fs_in (whole Hz) in format `fmt`, complex64 out at
    cfg.sample_rate.  if_hz: the IF of real input ('r8') or the tuner offset of complex input, its
    sign the sideband; conjugate mirrors complex input.  passband_hz None: 0.44 min(fs_in, fs_out).
    A configuration the stage cannot filter to spec raises EngineError (GPSMI_E_UNSUPPORTED)."""

    def __init__(self, cfg=None, fs_in=None, fmt='c64', if_hz=0.0, conjugate=False, passband_hz=None,
                 atten_db=60.0, max_out=None):
        self.cfg = cfg or Config()
        self.lib = _lib.load()
        self.fs_in = int(fs_in if fs_in is not None else self.cfg.sample_rate)
        self.fs_out = int(self.cfg.sample_rate)
        self.fmt = fmt
        if fmt not in FORMATS:
            raise ValueError(f'unknown sample format {fmt!r}: one of {sorted(FORMATS)}')
        _, self.dtype, self.per_sample = FORMATS[fmt]
        self.max_out = int(max_out or 4 * self.cfg.ngps)
        c = fe_cfg(self.fs_in, self.fs_out, fmt, if_hz, conjugate, passband_hz, atten_db, self.max_out,
                   self.cfg.device)
        h = C.c_void_p()
        check(self.lib.gpsmi_fe_create(C.byref(c), C.byref(h)), 'gpsmi_fe_create')
        self.h = h
        self.n_taps, self.n_phases, _ = design(self.fs_in, self.fs_out, fmt, if_hz, conjugate, passband_hz,
                                               atten_db)
        # largest input piece of one call whose outputs fit max_out (ceil(n fs_out / fs_in) + 1 at most)
        self.max_in = max(1, ((self.max_out - 2) * self.fs_in) // self.fs_out)
        self._out = PinnedArray((self.max_out,), np.complex64)
        self._block = None
        self._fill = 0

    def _samples(self, chunk):
        x = np.asarray(chunk)
        if x.dtype != self.dtype:
            raise TypeError(f'chunk dtype {x.dtype} does not match the format {self.fmt!r} '
                            f'({np.dtype(self.dtype).name})')
        x = np.ascontiguousarray(x).reshape(-1)
        if x.size % self.per_sample:
            raise ValueError(f'{self.fmt!r} chunks hold {self.per_sample} values per sample')
        return x, x.size // self.per_sample

    def _push_into(self, chunk):
        """-> outputs in the page-locked scratch, valid until the next call (a view)."""
        x, n = self._samples(chunk)
        got, pos, parts = C.c_size_t(0), 0, []
        while True:                 # (pieces of max_in samples: the same bits as one call)
            m = min(self.max_in, n - pos)
            piece = x[pos * self.per_sample:(pos + m) * self.per_sample]
            check(self.lib.gpsmi_fe_push(self.h, ptr(piece), m, ptr(self._out.array), self.max_out,
                                         C.byref(got)), 'gpsmi_fe_push')
            pos += m
            v = self._out.array[:got.value]
            if pos >= n:
                parts.append(v)
                break
            parts.append(v.copy())
        return parts[0] if len(parts) == 1 else np.concatenate(parts)

    def push(self, chunk):
        """Input samples (numpy array of the format's dtype; sc8 / sc16 interleaved I, Q) -> the
        complex64 outputs they complete (a new array)."""
        return np.array(self._push_into(chunk), dtype=np.complex64, copy=True)

    def blocks(self, chunk):
        """Generator of the complete cfg.ngps-sample blocks the chunk completes, each in the same
        page-locked buffer (use it before the next one); the remainder is kept for the next call."""
        if self._block is None:
            self._block = PinnedArray((self.cfg.ngps,), np.complex64)
        out = self._push_into(chunk)
        n, pos = self.cfg.ngps, 0
        while pos < len(out):
            m = min(n - self._fill, len(out) - pos)
            self._block.array[self._fill:self._fill + m] = out[pos:pos + m]
            self._fill += m
            pos += m
            if self._fill == n:
                self._fill = 0
                yield self._block.array

    def flush(self):
        """End of stream: the outputs up to the last input sample (zeros taken past it)."""
        got = C.c_size_t(0)
        check(self.lib.gpsmi_fe_flush(self.h, ptr(self._out.array), self.max_out, C.byref(got)),
              'gpsmi_fe_flush')
        return self._out.array[:got.value].copy()

    def reset(self):
        """Input index := 0, carry := 0, no partial block: as after creation."""
        check(self.lib.gpsmi_fe_reset(self.h), 'gpsmi_fe_reset')
        self._fill = 0

    def last_ms(self):
        ms = C.c_float(0.0)
        check(self.lib.gpsmi_fe_last_ms(self.h, C.byref(ms)), 'gpsmi_fe_last_ms')
        return ms.value

    def close(self):
        if getattr(self, 'h', None):
            check(self.lib.gpsmi_fe_destroy(self.h), 'gpsmi_fe_destroy')
            self.h = None
        for a in ('_out', '_block'):
            p = getattr(self, a, None)
            if p is not None:
                p.free()
                setattr(self, a, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
