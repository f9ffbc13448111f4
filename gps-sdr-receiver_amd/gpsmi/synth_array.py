"""A synth.Scene seen by several coherent antennas, with wideband jammers, for the null steering
(gpsmi.nulling).

Narrowband model: satellite s and jammer j reach antenna a with a fixed complex factor (a phase),
``steering[a][s]`` and ``Jammer.steering[a]``; the receiver noise is independent per antenna.  Like
synth.py the generator is counter-based: noise and jammer waveforms are hashes of the absolute sample
index, so any block of any antenna can be rendered on its own with the same bits.  Antenna 0 of a
scene with unit steering and no jammer is the synth.Scene itself.

Optionally every antenna has a channel response of its own (``channel``): a short complex FIR, or a
fractional delay rendered as a windowed sinc -- cables and filters that are not matched, which one
complex weight per antenna cannot undo (gpsmi.nulling, taps).  It acts on what arrives through the
antenna, satellites and jammers, not on the receiver noise behind it.  The filter reads the same
counter-based waveforms at the neighbouring sample indices, so a block still renders alone.

Everything is scaled by one factor (``scale``) before the 8-bit rendering, chosen so that the total
power per antenna leaves the quantiser clipping fewer than 1e-3 of the samples
(``clip_fraction`` counts them).
"""
from dataclasses import dataclass, field, replace
from typing import List

import numpy as np

from . import synth

_MAX_POWER = 0.16       # per complex sample: sigma 0.283 per component, P(|N| > 1) = 4e-4
SINC_HALF = 8           # a fractional delay is a Hamming-windowed sinc of 2 * SINC_HALF + 1 taps


def delay_fir(delay, half=SINC_HALF):
    """The centred FIR [2 half + 1] of a delay of `delay` samples (|delay| < 1): a Hamming-windowed
    sinc, unit gain at zero frequency."""
    m = np.arange(-half, half + 1, dtype=np.float64)
    h = np.sinc(m - delay) * (0.54 + 0.46 * np.cos(np.pi * (m - delay) / (half + 1.0)))
    return (h / h.sum()).astype(np.complex128)


def _gauss(seed, stream, idx):
    """Complex unit-power Gaussian, a pure function of (seed, stream, idx)."""
    u1 = synth._uniform(seed, stream, idx)
    u2 = synth._uniform(seed, stream + 1, idx)
    r = np.sqrt(-2.0 * np.log(u1))
    a = 2.0 * np.pi * u2
    return (r * np.cos(a) + 1j * r * np.sin(a)) / np.sqrt(2.0)


def ula_steering(antennas, sines, spacing=0.5):
    """Phase factors [antennas][len(sines)] of a uniform line of antennas `spacing` wavelengths apart
    for arrivals whose direction has the sine `sines` against broadside (antenna 0: 1)."""
    a = np.arange(antennas, dtype=np.float64)[:, None]
    return np.exp(2j * np.pi * spacing * a * np.asarray(sines, dtype=np.float64)[None, :])


@dataclass
class Jammer:
    steering: object                 # complex [antennas]
    jn_db: float = 30.0              # power over the noise of one antenna
    kind: str = 'white'              # 'white': complex Gaussian noise; 'tones': a sum of carriers
    tones: object = None             # 'tones': the frequencies in Hz (equal amplitudes)
    stream: int = 500                # hash stream of the waveform (and of the tone phases)


@dataclass
class ArrayScene:
    scene: synth.Scene
    steering: object                 # complex [antennas][satellites]
    jammers: List[Jammer] = field(default_factory=list)
    scale: float = None              # None: as large as the clipping limit allows, at most 1
    channel: object = None           # None, or per antenna: None (none), a delay in samples (float) or
    #                                  the taps of a centred complex FIR (odd length):
    #                                  out[k] = sum_m h[m] in[k + (len(h) - 1) / 2 - m]

    def __post_init__(self):
        self.steering = np.asarray(self.steering, dtype=np.complex128)
        if self.steering.ndim != 2 or self.steering.shape[1] != len(self.scene.sats):
            raise ValueError('steering must be [antennas][satellites]')
        for j in self.jammers:
            if len(np.atleast_1d(j.steering)) != self.antennas:
                raise ValueError('a jammer needs one steering factor per antenna')
        self._sats = [replace(self.scene, sats=[s], noise_sigma=0.0, _rep=self.scene._rep)
                      for s in self.scene.sats]
        self._fir = None
        if self.channel is not None:
            if len(self.channel) != self.antennas:
                raise ValueError('channel needs one entry per antenna')
            firs = [np.ones(1, dtype=np.complex128) if c is None else
                    delay_fir(float(c)) if np.ndim(c) == 0 else np.asarray(c, dtype=np.complex128)
                    for c in self.channel]
            if any(h.ndim != 1 or len(h) % 2 == 0 for h in firs):
                raise ValueError('a channel FIR needs an odd number of taps (it is centred)')
            half = max(len(h) for h in firs) // 2
            self._fir = np.zeros((self.antennas, 2 * half + 1), dtype=np.complex128)
            for a, h in enumerate(firs):
                self._fir[a, half - len(h) // 2:half + len(h) // 2 + 1] = h
        if self.scale is None:
            self.scale = min(1.0, float(np.sqrt(_MAX_POWER / self.power())))

    @property
    def antennas(self):
        return self.steering.shape[0]

    @property
    def ngps(self):
        return self.scene.ngps

    def noise_power(self):
        return self.scene.noise_sigma ** 2

    def jammer_power(self, j):
        return self.noise_power() * 10.0 ** (j.jn_db / 10.0)

    def power(self):
        """Expected power per antenna before scaling."""
        return (self.noise_power() + sum(s.amp ** 2 for s in self.scene.sats)
                + sum(self.jammer_power(j) for j in self.jammers))

    def _index(self, block_no, n):
        n = self.ngps if n is None else n
        return np.arange(n, dtype=np.int64) + int(block_no) * self.ngps

    def sat_parts(self, block_no, n=None):
        """complex128 [satellites][n]: every satellite alone, as antenna 0 would see it unscaled."""
        return np.stack([s.block_float(block_no, n) for s in self._sats]) if self._sats \
            else np.zeros((0, len(self._index(block_no, n))), dtype=np.complex128)

    def noise_parts(self, block_no, n=None):
        """complex128 [antennas][n]; antenna 0's is the synth.Scene's own noise."""
        k = self._index(block_no, n)
        return np.stack([self.scene.noise_sigma * _gauss(self.scene.seed, 1000 * a + 1, k)
                         for a in range(self.antennas)])

    def jammer_parts(self, block_no, n=None):
        """complex128 [jammers][n]: every jammer's waveform at unit steering."""
        return self._jammers_at(self._index(block_no, n))

    def _jammers_at(self, k):
        out = []
        for j in self.jammers:
            amp = np.sqrt(self.jammer_power(j))
            if j.kind == 'white':
                z = _gauss(self.scene.seed, j.stream, k)
            elif j.kind == 'tones':
                f = np.asarray(j.tones, dtype=np.float64)
                ph0 = 2.0 * np.pi * synth._uniform(self.scene.seed, j.stream, np.arange(len(f)))
                t = (k.astype(np.float64) + 1.0) / self.scene.sample_rate
                z = np.exp(1j * (2.0 * np.pi * f[:, None] * t[None, :] + ph0[:, None])).sum(axis=0)
                z /= np.sqrt(len(f))
            else:
                raise ValueError(f'unknown jammer kind {j.kind!r}')
            out.append(amp * z)
        return np.stack(out) if out else np.zeros((0, len(k)), dtype=np.complex128)

    def parts(self, block_no, n=None):
        """(satellites, noise, jammers) as every antenna receives them, scaled:
        complex128 [antennas][n] each; their sum is block_float."""
        js = np.array([np.atleast_1d(j.steering) for j in self.jammers],
                      dtype=np.complex128).reshape(len(self.jammers), self.antennas)
        if self._fir is None:
            sat = self.steering @ self.sat_parts(block_no, n)
            jam = js.T @ self.jammer_parts(block_no, n)
        else:
            sat = self._through(self.steering @ self._sats_around(block_no, n))
            k = self._index(block_no, n)
            half = self._fir.shape[1] // 2
            jam = self._through(js.T @ self._jammers_at(np.arange(k[0] - half, k[-1] + half + 1, dtype=np.int64)))
        return self.scale * sat, self.scale * self.noise_parts(block_no, n), self.scale * jam

    def sat_components(self, block_no, n=None):
        """complex128 [satellites][antennas][n]: every satellite alone as every antenna receives it,
        scaled; their sum over the satellites is parts()[0]."""
        if self._fir is None:
            sp = self.sat_parts(block_no, n)
            return self.scale * self.steering.T[:, :, None] * sp[:, None, :]
        sp = self._sats_around(block_no, n)
        return self.scale * np.stack([self._through(self.steering[:, s][:, None] * sp[s][None, :])
                                      for s in range(len(self._sats))])

    def _sats_around(self, block_no, n):
        """sat_parts of the block's samples and of the channel filters' reach either side of them
        (the tail of the block before, the head of the one after)."""
        n = self.ngps if n is None else n
        half = self._fir.shape[1] // 2
        here = min(n + half, self.ngps)
        parts = [self.sat_parts(block_no - 1)[:, self.ngps - half:], self.sat_parts(block_no, here)]
        if n + half > here:
            parts.append(self.sat_parts(block_no + 1, n + half - here))
        return np.concatenate(parts, axis=1)

    def _through(self, x):
        """[antennas][n + 2 half] -> [antennas][n]: every antenna's row through its channel FIR."""
        return np.stack([np.convolve(x[a], self._fir[a], mode='valid') for a in range(self.antennas)])

    def block_float(self, block_no, n=None):
        """complex128 [antennas][n] before quantisation."""
        sat, noise, jam = self.parts(block_no, n)
        return sat + noise + jam

    def block_raw(self, block_no, n=None):
        """uint16 [antennas][n] raw samples (Q << 8 | I), one row per channel file."""
        x = self.block_float(block_no, n)
        i = np.clip(np.rint((x.real + 1.0) * 127.5), 0, 255).astype(np.uint16)
        q = np.clip(np.rint((x.imag + 1.0) * 127.5), 0, 255).astype(np.uint16)
        return (q << 8) | i

    def block(self, block_no, n=None):
        """complex64 [antennas][n] as the decode hands them on."""
        return synth.raw_to_c64(self.block_raw(block_no, n))

    def clip_fraction(self, block_no, n=None):
        """Fraction of the components of block_raw that the 8-bit range cut off."""
        x = self.block_float(block_no, n)
        v = np.concatenate([x.real.ravel(), x.imag.ravel()])
        r = np.rint((v + 1.0) * 127.5)
        return float(np.mean((r < 0) | (r > 255)))
