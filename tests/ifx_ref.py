"""numpy restatement of the narrowband interference excision (gpsmi_ifx_*, include/gpsmi.h),
float64 throughout: the contract the HIP kernels of csrc/gpsmi_ifx.hip are tested against.

One block of n complex samples (n % 1024 == 0, n >= 4096) is cut into frames of L = 2048 samples
at hop H = 1024: frame m = 0 .. n/H - 1 covers block samples [m H - H, m H + H), frame 0 taking
its first H samples from the carry (the previous block's last H input samples, zero after a
reset).  Window: periodic Hann w[i] = sin^2(pi i / L); the last frame uses w[i] for i < H and 1
for i >= H, so the frames sum to 1 at every output sample without reading the next block.

Detection: P[k] = mean over frames 0 .. n/H - 2 of |FFT(w x_m)|^2; floor = median(P); a bin is
flagged when P[k] > floor 10^(thresh_db / 10), then widened by +-dilate bins circularly.  More
than max_bins flagged bins: the block passes through unchanged, count -1, empty mask.  Apply:
every frame is transformed, the flagged bins zeroed, transformed back and overlap-added.
"""
import numpy as np

L = 2048
H = 1024


def window():
    i = np.arange(L)
    return np.sin(np.pi * i / L) ** 2


def check_block(n):
    return n % H == 0 and n >= 4 * H


class ExcisionRef:
    def __init__(self, n, thresh_db=6.0, dilate=2, max_bins=256):
        if not check_block(n):
            raise ValueError('block length must be a multiple of 1024 and >= 4096')
        self.n, self.thresh_db, self.dilate, self.max_bins = n, thresh_db, dilate, max_bins
        self.w = window()
        self.w_last = self.w.copy()
        self.w_last[H:] = 1.0
        self.reset()

    def reset(self):
        self.carry = np.zeros(H, dtype=np.complex128)

    def frames(self, x):
        """[n/H, L] windowed frames of block x (complex128) behind the current carry."""
        ext = np.concatenate([self.carry, x])
        nf = self.n // H
        fr = np.stack([ext[m * H:m * H + L] for m in range(nf)])
        fr = fr * self.w[None, :]
        fr[-1] = ext[(nf - 1) * H:(nf - 1) * H + L] * self.w_last
        return fr

    def detect(self, spectra):
        """(P, threshold, mask bool[L], count) from the frame spectra [n/H, L]."""
        P = np.mean(np.abs(spectra[:-1]) ** 2, axis=0)
        thr = np.median(P) * 10.0 ** (self.thresh_db / 10.0)
        raw = P > thr
        mask = raw.copy()
        for d in range(1, self.dilate + 1):
            mask |= np.roll(raw, d) | np.roll(raw, -d)
        count = int(mask.sum())
        if count > self.max_bins:
            return P, thr, np.zeros(L, dtype=bool), -1
        return P, thr, mask, count

    def process(self, x):
        """One block -> (y complex128 [n], count, mask bool[L], P, threshold); advances the carry."""
        x = np.asarray(x).astype(np.complex128)
        assert x.shape == (self.n,)
        spectra = np.fft.fft(self.frames(x), axis=1)
        P, thr, mask, count = self.detect(spectra)
        y = x.copy() if count < 0 else self._overlap_add(spectra, mask)
        self.carry = x[-H:].copy()
        return y, count, mask, P, thr

    def excise_with(self, x, mask):
        """Block x with a given mask applied, behind the current carry, which is left as it is (the
        filter is linear for a fixed mask: what a jammed block's mask leaves of the tone alone)."""
        x = np.asarray(x).astype(np.complex128)
        return self._overlap_add(np.fft.fft(self.frames(x), axis=1), mask)

    def _overlap_add(self, spectra, mask):
        spectra = spectra.copy()
        spectra[:, mask] = 0
        back = np.fft.ifft(spectra, axis=1)
        y = np.zeros(self.n + H, dtype=np.complex128)      # (index 0: carry sample 0)
        for m in range(back.shape[0]):
            y[m * H:m * H + L] += back[m]
        return y[H:]


def mask_words(mask):
    """bool[2048] -> uint32[64], bin k in bit k % 32 of word k // 32 (the ABI's layout)."""
    bits = np.asarray(mask, dtype=np.uint32).reshape(64, 32)
    return (bits << np.arange(32, dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint32)


def words_to_mask(words):
    w = np.asarray(words, dtype=np.uint32)
    return ((w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(bool).reshape(-1)


def add_tone(x, jn_db, freq_hz, fs, first_sample=0, noise_power=None, phase=0.3):
    """x + a CW tone whose power over `noise_power` (default: the scene's total noise power,
    sigma^2) is jn_db; sample k of the block is absolute sample first_sample + k."""
    amp = np.sqrt(noise_power * 10.0 ** (jn_db / 10.0))
    k = np.arange(len(x), dtype=np.float64) + first_sample
    return x + amp * np.exp(1j * (2.0 * np.pi * freq_hz * k / fs + phase))


def quantise(x):
    """complex128 -> the recorder's uint16 (Q << 8 | I), as synth.Scene.block_raw does."""
    i = np.clip(np.rint((x.real + 1.0) * 127.5), 0, 255).astype(np.uint16)
    q = np.clip(np.rint((x.imag + 1.0) * 127.5), 0, 255).astype(np.uint16)
    return (q << 8) | i
