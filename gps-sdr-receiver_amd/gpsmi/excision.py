"""Narrowband interference excision ahead of acquisition and tracking (gpsmi_ifx_*, gpsmi.h).

A continuous-wave tone some 30 dB above the noise defeats the C/A code's processing gain. On
the GPU, ``Excision`` finds such tones in the spectrum of each block and zeroes their bins in
overlapping Hann frames. The output is complex64 and goes straight into the acquisition and
tracking engines, in their complex64 format. Opt-in: nothing else changes when it is not used
(``pipeline.Receiver(excise=...)``).
"""
import numpy as np

from . import _lib
from ._lib import ptr
from .conditioning import BlockFilter

MASK_WORDS = 64                 # 2048 bins, bit k % 32 of word k // 32


class Excision(BlockFilter):
    """One excision handle over blocks of cfg.ngps samples (cfg: engine.Config; its code_samples *
    n_cyc must be a multiple of 1024 and >= 4096, else EngineError with GPSMI_E_UNSUPPORTED).
    raw_u8: the input is the recorder's uint16 (Q << 8 | I), decoded on the GPU; the output is
    complex64 either way."""
    PREFIX = 'ifx'

    def __init__(self, cfg=None, thresh_db=6.0, dilate=2, max_bins=256, raw_u8=False):
        super().__init__(cfg, raw_u8)
        self._create(_lib.IfxCfg(self.n, float(thresh_db), int(dilate), int(max_bins), self.cfg.device))
        self.last_counts = None         # int32 [nb] of the last call: bins removed, -1 wideband
        self.last_masks = None          # uint32 [nb, 64] of the last call: the bins removed

    def _results(self, nb):
        self.last_counts = np.zeros(nb, dtype=np.int32)
        self.last_masks = np.zeros((nb, MASK_WORDS), dtype=np.uint32)
        return self.last_counts, self.last_masks

    def last_psd(self):
        """float32 [nb, 2048]: the P[k] that the mask pass of the last call thresholded, bit for bit
        (a diagnostic; EngineError with GPSMI_E_STATE before the first call)."""
        psd = np.zeros((max(self.last_nb, 1), 2048), dtype=np.float32)
        self._call('last_psd', self.h, ptr(psd))
        return psd
