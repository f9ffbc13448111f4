"""Null steering over several coherent antennas, ahead of everything else (gpsmi_nul_*, gpsmi.h).

A jammer that is wide in frequency and continuous in time (band-limited noise, a slow sweep, a dense
tone field) leaves nothing for the excision or the blanker to grip: in one antenna it differs from
the satellites only in its direction of arrival.  With A sample-aligned antennas (a coherent
multi-channel recorder writes one file per channel) ``NullSteer`` minimises, per block and on the
GPU, the output power with the gain of antenna 0 held at one (power inversion): up to A - 1 spatial
nulls land on whatever is far above the noise, without calibration, antenna positions or satellite
directions.  A block in which that would gain less than ``min_gain_db`` passes antenna 0 through bit
for bit.  Opt-in: nothing else changes when it is not used (``pipeline.Receiver(null=...)``).

``NullSteer.beams`` forms per-satellite beams on the same handle (gpsmi_nul_beams): a
given steering vector held at one, given null vectors held at zero, the output power minimised under
those constraints; many beams from one read of the antennas (``snapshot.measure(..., beams=True)``).
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
        self.last_beam_flags = None     # int32 [nb, nbeam] of the last beams call: 1, 0 quiescent, -1 none
        self.last_beam_gain_db = None   # float32 [nb, nbeam]
        self.last_beam_weights = None   # complex128 [nb, nbeam, antennas]

    def _results(self, nb):
        self.last_flags = np.zeros(nb, dtype=np.int32)
        self.last_gain_db = np.zeros(nb, dtype=np.float32)
        shape = (nb, self.antennas) if self.taps <= 1 else (nb, self.antennas, self.taps)
        self.last_weights = np.zeros(shape, dtype=np.complex128)
        return self.last_flags, self.last_gain_db, self.last_weights

    def _input(self, blocks):
        """Host blocks of every antenna, checked against the input format -> (C-contiguous array, nb)."""
        want = np.uint16 if self.raw_u8 else np.complex64
        x = np.asarray(blocks)
        if x.dtype != want:
            raise TypeError(f'blocks dtype {x.dtype} does not match the input format '
                            f'({np.dtype(want).name})')
        if x.ndim < 2 or x.shape[0] != self.antennas or x.size == 0 or (x.size // self.antennas) % self.n:
            raise ValueError(f'{self.antennas} antennas of blocks of {self.n} samples expected, got {x.shape}')
        return np.ascontiguousarray(x), x.size // self.antennas // self.n

    def _kernel_ms(self, name):
        ms = (C.c_float * 3)()
        self._call(name, self.h, ms)
        return tuple(float(v) for v in ms)

    def apply(self, blocks, out=None):
        """Host blocks in ([antennas, n], [antennas, nb * n] or [antennas, nb, n]; complex64, or
        uint16 with raw_u8), complex64 out ([n] for one block, else [nb, n]; into `out` when given)."""
        x, nb = self._input(blocks)
        shape = (self.n,) if x.shape[1:] == (self.n,) else (nb, self.n)
        if out is None:
            out = np.empty(shape, dtype=np.complex64)
        elif out.dtype != np.complex64 or out.size != nb * self.n or not out.flags['C_CONTIGUOUS']:
            raise ValueError('out must be a C-contiguous complex64 array of one antenna\'s size')
        self._call('apply', self.h, ptr(x), ptr(out), nb, *map(ptr, self._results(nb)))
        self.last_nb = nb
        return out

    # ---- per-satellite beams (gpsmi_nul_beams*) ---------------------------------------------------

    def _beam_args(self, nb, steer, nulls, mask):
        """The beam description as the ABI takes it, and fresh last_beam_* arrays for nb blocks."""
        A = self.antennas
        s = np.ascontiguousarray(np.asarray(steer, dtype=np.complex128).reshape(-1, A))
        u = None if nulls is None else np.ascontiguousarray(np.asarray(nulls, dtype=np.complex128).reshape(-1, A))
        nnull = 0 if u is None else len(u)
        if mask is None:                                # every beam carries every null
            mask = np.full(len(s), (1 << nnull) - 1)
        m = np.ascontiguousarray(np.asarray(mask, dtype=np.uint32))
        if m.shape != (len(s),):
            raise ValueError(f'one mask word per beam expected, got {m.shape} for {len(s)} beams')
        rows = max(nb, 0)                               # (a bad nb is the library's to refuse)
        self.last_beam_flags = np.zeros((rows, len(s)), dtype=np.int32)
        self.last_beam_gain_db = np.zeros((rows, len(s)), dtype=np.float32)
        self.last_beam_weights = np.zeros((rows, len(s), A), dtype=np.complex128)
        self._beam_keep = (s, u, m)
        return (len(s), ptr(s), nnull, None if u is None else ptr(u), ptr(m), ptr(self.last_beam_flags),
                ptr(self.last_beam_gain_db), ptr(self.last_beam_weights))

    def beams(self, blocks, steer, nulls=None, mask=None, out=None):
        """Host blocks in as for apply() -> complex64 [nbeam, nb * n]: beam b holds steer[b]
        (complex [nbeam, antennas]) at one, holds the rows of nulls (complex [nnull <= 4, antennas])
        that its mask word names (bit q: null q; None: all of them) at zero and minimises the output
        power under those constraints, per block.  last_beam_flags [nb, nbeam] (1 adaptive, 0
        quiescent, -1 no weights: zeros out), last_beam_gain_db and last_beam_weights
        [nb, nbeam, antennas] describe the call.  One weight per antenna only (taps <= 1)."""
        x, nb = self._input(blocks)
        args = self._beam_args(nb, steer, nulls, mask)
        if out is None:
            out = np.empty((args[0], nb * self.n), dtype=np.complex64)
        elif out.dtype != np.complex64 or out.size != args[0] * nb * self.n or not out.flags['C_CONTIGUOUS']:
            raise ValueError('out must be a C-contiguous complex64 array of nbeam rows of one antenna\'s size')
        self._call('beams', self.h, ptr(x), ptr(out), nb, *args)
        return out

    def beams_dev(self, d_in, d_out, nb, steer, nulls=None, mask=None, in_stride=0, out_stride=0):
        """The same from device memory to device memory (c_void_p or int).  in_stride / out_stride:
        samples from one antenna's / one beam's row to the next; 0 means nb * n."""
        self._call('beams_dev', self.h, d_in, int(in_stride), d_out, int(out_stride), int(nb),
                   *self._beam_args(int(nb), steer, nulls, mask))

    def last_beam_kernel_ms(self):
        """Device time of the last beams call's three kernels: (covariance, solve, apply) in ms."""
        return self._kernel_ms('last_beam_kernel_ms')

    def reset(self):
        """Nothing to reset: every block is worked on alone."""

    def last_kernel_ms(self):
        """Device time of the last call's three kernels: (covariance, solve, apply) in ms."""
        return self._kernel_ms('last_kernel_ms')
