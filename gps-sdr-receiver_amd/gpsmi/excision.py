"""Narrowband interference excision ahead of acquisition and tracking (gpsmi_ifx_*, gpsmi.h).

A continuous-wave tone some 30 dB above the noise defeats the C/A code's processing gain. On
the GPU, ``Excision`` finds such tones in the spectrum of each block and zeroes their bins in
overlapping Hann frames. The output is complex64 and goes straight into the acquisition and
tracking engines, in their complex64 format. Opt-in: nothing else changes when it is not used
(``pipeline.Receiver(excise=...)``).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr
from .engine import Config

MASK_WORDS = 64                 # 2048 bins, bit k % 32 of word k // 32


class Excision:
    """One excision handle over blocks of cfg.ngps samples (cfg: engine.Config; its code_samples *
    n_cyc must be a multiple of 1024 and >= 4096, else EngineError with GPSMI_E_UNSUPPORTED).
    raw_u8: the input is the recorder's uint16 (Q << 8 | I), decoded on the GPU; the output is
    complex64 either way."""

    def __init__(self, cfg=None, thresh_db=6.0, dilate=2, max_bins=256, raw_u8=False):
        self.cfg = cfg or Config()
        self.lib = _lib.load()
        self.n = self.cfg.ngps
        self.raw_u8 = bool(raw_u8)
        c = _lib.IfxCfg(self.n, float(thresh_db), int(dilate), int(max_bins), self.cfg.device)
        h = C.c_void_p()
        check(self.lib.gpsmi_ifx_create(C.byref(c), C.byref(h)), 'gpsmi_ifx_create')
        self.h = h
        if self.raw_u8:
            check(self.lib.gpsmi_ifx_set_input_format(self.h, 1), 'gpsmi_ifx_set_input_format')
        self.last_counts = None         # int32 [nb] of the last call: bins removed, -1 wideband
        self.last_masks = None          # uint32 [nb, 64] of the last call: the bins removed
        self._psd_nb = 0                # blocks of the last call that ran (rows of last_psd)

    def _results(self, nb):
        self.last_counts = np.zeros(nb, dtype=np.int32)
        self.last_masks = np.zeros((nb, MASK_WORDS), dtype=np.uint32)
        return self.last_counts, self.last_masks

    def apply(self, blocks, out=None):
        """Host blocks in (one block [n] or consecutive blocks [nb, n]; complex64, or uint16 with
        raw_u8), complex64 of the same shape out (into `out` when given, e.g. page-locked memory)."""
        want = np.uint16 if self.raw_u8 else np.complex64
        x = np.asarray(blocks)
        if x.dtype != want:
            raise TypeError(f'blocks dtype {x.dtype} does not match the input format '
                            f'({np.dtype(want).name})')
        if x.size == 0 or x.size % self.n:
            raise ValueError(f'blocks of {self.n} samples expected, got {x.shape}')
        x = np.ascontiguousarray(x)
        nb = x.size // self.n
        if out is None:
            out = np.empty(x.shape, dtype=np.complex64)
        elif out.dtype != np.complex64 or out.size != x.size or not out.flags['C_CONTIGUOUS']:
            raise ValueError('out must be a C-contiguous complex64 array of the input size')
        counts, masks = self._results(nb)
        check(self.lib.gpsmi_ifx_apply(self.h, ptr(x), ptr(out), nb, ptr(counts), ptr(masks)),
              'gpsmi_ifx_apply')
        self._psd_nb = nb
        return out

    def apply_dev(self, d_in, d_out, nb):
        """nb consecutive blocks from device memory (c_void_p or int) to device memory (complex64)."""
        counts, masks = self._results(int(nb))
        check(self.lib.gpsmi_ifx_apply_dev(self.h, d_in, d_out, int(nb), ptr(counts), ptr(masks)),
              'gpsmi_ifx_apply_dev')
        self._psd_nb = int(nb)

    def reset(self):
        """Carry := 0, as after creation (the block before the next one is taken as silence)."""
        check(self.lib.gpsmi_ifx_reset(self.h), 'gpsmi_ifx_reset')

    def last_ms(self):
        ms = C.c_float(0.0)
        check(self.lib.gpsmi_ifx_last_ms(self.h, C.byref(ms)), 'gpsmi_ifx_last_ms')
        return ms.value

    def last_psd(self):
        """float32 [nb, 2048]: the P[k] that the mask pass of the last call thresholded, bit for bit
        (a diagnostic; EngineError with GPSMI_E_STATE before the first call)."""
        psd = np.zeros((max(self._psd_nb, 1), 2048), dtype=np.float32)
        check(self.lib.gpsmi_ifx_last_psd(self.h, ptr(psd)), 'gpsmi_ifx_last_psd')
        return psd

    def close(self):
        if getattr(self, 'h', None):
            check(self.lib.gpsmi_ifx_destroy(self.h), 'gpsmi_ifx_destroy')
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
