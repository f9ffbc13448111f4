"""Pulse blanking ahead of acquisition and tracking (gpsmi_pb_*, gpsmi.h).

Pulsed emitters (radar) and swept "privacy" jammers are strong but short in time: a chirp sweeping
+-8 MHz crosses a 2 MHz front end as a burst every few microseconds.  On the GPU, ``PulseBlanker``
takes a robust noise floor per block (the lower median of the sample powers), zeroes every sample far
above it plus a short guard around it and passes every other sample bit for bit.  It works in the time
domain, at any block length.  Opt-in: nothing else changes when it is not used
(``pipeline.Receiver(blank=...)``).
"""
import numpy as np

from . import _lib
from .conditioning import BlockFilter


def default_guard(code_samples):
    """Guard samples on each side of a detection: 2 at 2.048 Msps, 16 at 16.368 Msps."""
    return max(2, int(round(2 * code_samples / 2048)))


class PulseBlanker(BlockFilter):
    """One blanking handle over blocks of cfg.ngps samples (cfg: engine.Config, any code length).
    thresh_db: a sample is a detection when its power exceeds the block's lower median by this much;
    pre / post: samples blanked before / after each detection (None: default_guard); max_frac: a block
    with more blanked samples than this fraction passes through (count -1).  raw_u8: the input is the
    recorder's uint16 (Q << 8 | I), decoded on the GPU; the output is complex64 either way."""
    PREFIX = 'pb'

    def __init__(self, cfg=None, thresh_db=10.0, pre=None, post=None, max_frac=0.5, raw_u8=False):
        super().__init__(cfg, raw_u8)
        g = default_guard(self.cfg.code_samples)
        self.pre = g if pre is None else int(pre)
        self.post = g if post is None else int(post)
        self._create(_lib.PbCfg(self.n, float(thresh_db), self.pre, self.post, float(max_frac), self.cfg.device))
        self.last_counts = None         # int32 [nb] of the last call: samples blanked, -1 passed through
        self.last_floors = None         # float32 [nb]: the lower median of the powers
        self.last_masks = None          # uint32 [nb, n / 32]: the samples blanked

    def _results(self, nb):
        self.last_counts = np.zeros(nb, dtype=np.int32)
        self.last_floors = np.zeros(nb, dtype=np.float32)
        self.last_masks = np.zeros((nb, self.n // 32), dtype=np.uint32)
        return self.last_counts, self.last_floors, self.last_masks
