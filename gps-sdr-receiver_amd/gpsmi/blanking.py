"""Pulse blanking ahead of acquisition and tracking (gpsmi_pb_*, gpsmi.h).

Pulsed emitters (radar) and swept "privacy" jammers are strong but short in time: a chirp sweeping
+-8 MHz crosses a 2 MHz front end as a burst every few microseconds.  On the GPU, ``PulseBlanker``
takes a robust noise floor per block (the lower median of the sample powers), zeroes every sample far
above it plus a short guard around it and passes every other sample bit for bit.  It works in the time
domain, at any block length.  Opt-in: nothing else changes when it is not used
(``pipeline.Receiver(blank=...)``).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr
from .engine import Config


def default_guard(code_samples):
    """Guard samples on each side of a detection: 2 at 2.048 Msps, 16 at 16.368 Msps."""
    return max(2, int(round(2 * code_samples / 2048)))


class PulseBlanker:
    """One blanking handle over blocks of cfg.ngps samples (cfg: engine.Config, any code length).
    thresh_db: a sample is a detection when its power exceeds the block's lower median by this much;
    pre / post: samples blanked before / after each detection (None: default_guard); max_frac: a block
    with more blanked samples than this fraction passes through (count -1).  raw_u8: the input is the
    recorder's uint16 (Q << 8 | I), decoded on the GPU; the output is complex64 either way."""

    def __init__(self, cfg=None, thresh_db=10.0, pre=None, post=None, max_frac=0.5, raw_u8=False):
        self.cfg = cfg or Config()
        self.lib = _lib.load()
        self.n = self.cfg.ngps
        self.raw_u8 = bool(raw_u8)
        g = default_guard(self.cfg.code_samples)
        self.pre = g if pre is None else int(pre)
        self.post = g if post is None else int(post)
        c = _lib.PbCfg(self.n, float(thresh_db), self.pre, self.post, float(max_frac), self.cfg.device)
        h = C.c_void_p()
        check(self.lib.gpsmi_pb_create(C.byref(c), C.byref(h)), 'gpsmi_pb_create')
        self.h = h
        if self.raw_u8:
            check(self.lib.gpsmi_pb_set_input_format(self.h, 1), 'gpsmi_pb_set_input_format')
        self.last_counts = None         # int32 [nb] of the last call: samples blanked, -1 passed through
        self.last_floors = None         # float32 [nb]: the lower median of the powers
        self.last_masks = None          # uint32 [nb, n / 32]: the samples blanked

    def _results(self, nb):
        self.last_counts = np.zeros(nb, dtype=np.int32)
        self.last_floors = np.zeros(nb, dtype=np.float32)
        self.last_masks = np.zeros((nb, self.n // 32), dtype=np.uint32)
        return self.last_counts, self.last_floors, self.last_masks

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
        counts, floors, masks = self._results(nb)
        check(self.lib.gpsmi_pb_apply(self.h, ptr(x), ptr(out), nb, ptr(counts), ptr(floors), ptr(masks)),
              'gpsmi_pb_apply')
        return out

    def apply_dev(self, d_in, d_out, nb):
        """nb consecutive blocks from device memory (c_void_p or int) to device memory (complex64)."""
        counts, floors, masks = self._results(int(nb))
        check(self.lib.gpsmi_pb_apply_dev(self.h, d_in, d_out, int(nb), ptr(counts), ptr(floors),
                                          ptr(masks)), 'gpsmi_pb_apply_dev')

    def reset(self):
        """Carry := 0, as after creation (nothing of the block before reaches the next one)."""
        check(self.lib.gpsmi_pb_reset(self.h), 'gpsmi_pb_reset')

    def last_ms(self):
        ms = C.c_float(0.0)
        check(self.lib.gpsmi_pb_last_ms(self.h, C.byref(ms)), 'gpsmi_pb_last_ms')
        return ms.value

    def close(self):
        if getattr(self, 'h', None):
            check(self.lib.gpsmi_pb_destroy(self.h), 'gpsmi_pb_destroy')
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
