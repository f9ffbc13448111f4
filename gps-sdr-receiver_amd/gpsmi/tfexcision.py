"""Time-frequency (sweep) excision ahead of acquisition and tracking (gpsmi_tfx_*, gpsmi.h).

A swept or chirp jammer is continuous in time and wide in a block's mean spectrum: the tone excision
sees no line and the blanker a constant envelope.  In a short-time Fourier transform it is narrow in
every frame.  On the GPU, ``SweepExcision`` takes the cells of the time-frequency plane far above the
block's lower median, zeroes them (10-30 % of the plane for the usual jammers) and transforms back;
the satellites' spread-spectrum signal lives on in the rest.  It works at any block length that is a
multiple of 128, the 16.368 Msps configurations among them.  Opt-in: nothing else changes when it is
not used (``pipeline.Receiver(sweep=...)``).
"""
import numpy as np

from . import _lib
from ._lib import ptr
from .conditioning import BlockFilter

FRAMES = (32, 64, 128, 256)


def default_frame(code_samples):
    """64 samples at 2.048 Msps; 32 at 16.368 Msps, where the +-8 MHz / 20 us chirp crosses a bin of
    longer frames in less than a frame."""
    return 64 if code_samples <= 4096 else 32


class SweepExcision(BlockFilter):
    """One handle over blocks of cfg.ngps samples (cfg: engine.Config; ngps a multiple of 128, else
    EngineError with GPSMI_E_UNSUPPORTED).  frame: L, 32 / 64 / 128 / 256 (None: default_frame);
    thresh_db: a cell is a detection when its power exceeds the block's lower median by this much;
    dilate: bins flagged on each side of a detection, inside its frame; max_frac: a block with more
    of its plane flagged passes through (count -1); keep_power: last_power() may be called.  raw_u8:
    the input is the recorder's uint16 (Q << 8 | I), decoded on the GPU; the output is complex64
    either way."""
    PREFIX = 'tfx'

    def __init__(self, cfg=None, frame=None, thresh_db=12.0, dilate=1, max_frac=0.5, keep_power=False,
                 raw_u8=False):
        super().__init__(cfg, raw_u8)
        self.frame = default_frame(self.cfg.code_samples) if frame is None else int(frame)
        self.keep_power = bool(keep_power)
        # (the ABI's zeros mean "the default": a threshold of 0 dB or max_frac 0 is asked for as the
        # smallest positive float32)
        tiny = float(np.finfo(np.float32).tiny)
        self._create(_lib.TfxCfg(self.n, self.frame, float(thresh_db) or tiny, int(dilate), float(max_frac) or tiny,
                                 int(self.keep_power), self.cfg.device, 0))
        self.nf = self.n // (self.frame // 2)
        self.last_counts = None         # int32 [nb] of the last call: cells flagged, -1 passed through
        self.last_floors = None         # float32 [nb]: the lower median of the cell powers
        self.last_masks = None          # uint32 [nb, nf * frame / 32]: the cells zeroed

    def _results(self, nb):
        self.last_counts = np.zeros(nb, dtype=np.int32)
        self.last_floors = np.zeros(nb, dtype=np.float32)
        self.last_masks = np.zeros((nb, self.nf * self.frame // 32), dtype=np.uint32)
        return self.last_counts, self.last_floors, self.last_masks

    def last_power(self):
        """float32 [nb, nf, frame]: the cell powers P of the last call, bit for bit what its floors,
        masks and counts were made from (EngineError with GPSMI_E_STATE without keep_power or before
        the first call)."""
        P = np.zeros((max(self.last_nb, 1), self.nf, self.frame), dtype=np.float32)
        self._call('last_power', self.h, ptr(P))
        return P
