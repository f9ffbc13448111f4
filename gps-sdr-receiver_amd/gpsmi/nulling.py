"""Null steering over several coherent antennas, ahead of everything else (gpsmi_nul_*, gpsmi.h).

A jammer that is wide in frequency and continuous in time (band-limited noise, a slow sweep, a dense
tone field) leaves nothing for the excision or the blanker to grip: in one antenna it differs from
the satellites only in its direction of arrival.  With A sample-aligned antennas (a coherent
multi-channel recorder writes one file per channel) ``NullSteer`` minimises, per block and on the
GPU, the output power with the gain of antenna 0 held at one (power inversion): up to A - 1 spatial
nulls land on whatever is far above the noise, without calibration, antenna positions or satellite
directions.  A block in which that would gain less than ``min_gain_db`` passes antenna 0 through bit
for bit.  Opt-in: nothing else changes when it is not used (``pipeline.Receiver(null=...)``).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ptr
from .conditioning import BlockFilter


class NullSteer(BlockFilter):
    """One null-steering handle over blocks of cfg.ngps samples of `antennas` antennas (2..8).
    load: diagonal loading relative to the mean antenna power (0: 1e-6); min_gain_db: a block whose
    predicted gain (antenna 0's power over the output power) is below it passes through (0: 3 dB).
    raw_u8: the input is the recorder's uint16 (Q << 8 | I), decoded on the GPU; the output is
    complex64 either way.  Input of a call: [antennas][nb * n], every antenna's blocks contiguous.
    taps: 0 or 1: one complex weight per antenna.  3, 5 or 7: space-time, a filter of that many taps
    per antenna, y[i] = sum_a sum_t conj(w[a][t]) x_a[i + c - t] with c = (taps - 1) / 2 and the
    centre tap of antenna 0 held at one.  It absorbs delay and filter mismatch between the channels
    and nulls more than antennas - 1 narrowband interferers; the output stays aligned with antenna 0,
    and its first and last c samples of a block are zero (a tap would reach outside the block)."""
    PREFIX = 'nul'

    def __init__(self, cfg=None, antennas=4, load=0.0, min_gain_db=0.0, raw_u8=False, taps=1):
        super().__init__(cfg, raw_u8)
        self.antennas = int(antennas)
        self.taps = int(taps)
        self._create(_lib.NulCfg(self.n, self.antennas, float(load), float(min_gain_db), self.cfg.device,
                                 self.taps))
        self.last_flags = None          # int32 [nb] of the last call: 1 nulled, 0 passed through
        self.last_gain_db = None        # float32 [nb]: the predicted gain
        self.last_weights = None        # complex128 [nb, antennas] (taps <= 1) or [nb, antennas, taps]: w
        #                                 (the unit vector of antenna 0's centre tap for a pass-through block)

    def _results(self, nb):
        self.last_flags = np.zeros(nb, dtype=np.int32)
        self.last_gain_db = np.zeros(nb, dtype=np.float32)
        shape = (nb, self.antennas) if self.taps <= 1 else (nb, self.antennas, self.taps)
        self.last_weights = np.zeros(shape, dtype=np.complex128)
        return self.last_flags, self.last_gain_db, self.last_weights

    def apply(self, blocks, out=None):
        """Host blocks in ([antennas, n], [antennas, nb * n] or [antennas, nb, n]; complex64, or
        uint16 with raw_u8), complex64 out ([n] for one block, else [nb, n]; into `out` when given)."""
        want = np.uint16 if self.raw_u8 else np.complex64
        x = np.asarray(blocks)
        if x.dtype != want:
            raise TypeError(f'blocks dtype {x.dtype} does not match the input format '
                            f'({np.dtype(want).name})')
        if x.ndim < 2 or x.shape[0] != self.antennas or x.size == 0 or (x.size // self.antennas) % self.n:
            raise ValueError(f'{self.antennas} antennas of blocks of {self.n} samples expected, got {x.shape}')
        x = np.ascontiguousarray(x)
        nb = x.size // self.antennas // self.n
        shape = (self.n,) if x.shape[1:] == (self.n,) else (nb, self.n)
        if out is None:
            out = np.empty(shape, dtype=np.complex64)
        elif out.dtype != np.complex64 or out.size != nb * self.n or not out.flags['C_CONTIGUOUS']:
            raise ValueError('out must be a C-contiguous complex64 array of one antenna\'s size')
        self._call('apply', self.h, ptr(x), ptr(out), nb, *map(ptr, self._results(nb)))
        self.last_nb = nb
        return out

    def reset(self):
        """Nothing to reset: every block is worked on alone."""

    def last_kernel_ms(self):
        """Device time of the last call's three kernels: (covariance, solve, apply) in ms."""
        ms = (C.c_float * 3)()
        self._call('last_kernel_ms', self.h, ms)
        return tuple(float(v) for v in ms)
