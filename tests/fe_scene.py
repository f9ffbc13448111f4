"""The satellites of a synth.Scene rendered as another front end records them: any input rate, IF or
tuner offset and sample format (tests of the front-end stage, gpsmi_fe_*).

Input sample i sits at the scene's output-sample time k = i fs_out / fs_in.  Each satellite is
rectangular 1.023 Mchip/s chips at its true code position (Sat.pos_poly, or the linear delay model
of synth.Scene.block_float) with the scene's data bits, on the carrier IF + Doppler (the phase of
block_float plus 2 pi IF i / fs_in); real input carries A cos(.), complex input A exp(j .).  Noise has
the scene's density (noise_sigma^2 / fs_out), hashed from the input index; the samples are scaled so
that the rms is 1/5 of full scale (int8 clips at 5 sigma) and quantised."""
import numpy as np

from gpsmi import codes, synth

import fe_ref as R


def signal(scene, fs_in, if_hz, real, i0, n):
    """complex128 (real input: float64 as complex) samples [i0, i0 + n) before quantisation."""
    cs, fs = scene.code_samples, scene.sample_rate
    i = np.arange(i0, i0 + n, dtype=np.float64)
    k = i * (fs / fs_in)
    x = np.zeros(n, dtype=np.float64 if real else np.complex128)
    w_if = 2.0 * np.pi * if_hz / fs_in * i
    for s in scene.sats:
        rate = (-s.doppler / 1575.42e6) if s.delay_rate is None else s.delay_rate
        if s.pos_poly is not None:
            coefs, k0, ks = s.pos_poly
            pos = np.polyval(coefs, (k - k0) / ks)
        else:
            pos = k - (s.delay + rate * k)
        period = np.floor(pos / cs)
        chip = np.floor((pos - period * cs) * (1023.0 / cs)).astype(np.int64)
        code = codes.ca_chips(s.prn).astype(np.float64)[np.clip(chip, 0, 1022)]
        if s.nav_bits is not None:
            bit_no = np.floor(period / 20.0).astype(np.int64)
            nav = np.asarray(s.nav_bits)
            code = code * (2.0 * nav[bit_no % len(nav)] - 1.0)
        elif s.data_bits:
            bit_no = np.floor(period / 20.0).astype(np.int64)
            h = synth._mix64((bit_no + (1 << 40)).astype(np.uint64) ^ np.uint64(scene.seed * 1000 + s.prn))
            code = code * (1.0 - 2.0 * (h & np.uint64(1)).astype(np.float64))
        t = (k + 1.0) / fs
        ph = 2.0 * np.pi * (s.doppler * t + 0.5 * s.doppler_rate * t * t) + s.phase0 + w_if
        x += s.amp * code * (np.cos(ph) if real else np.exp(1j * ph))
    if scene.noise_sigma > 0:
        g1, g2 = synth.gaussian_pair(scene.seed + 991, i.astype(np.int64))
        sig = scene.noise_sigma * np.sqrt(fs_in / fs)
        x = x + (0.5 * sig * g1 if real else (sig / np.sqrt(2.0)) * (g1 + 1j * g2))
    return x


def scale(scene, fs_in, real):
    """Quantiser gain: rms per stored component -> 0.2 of full scale."""
    p = sum(s.amp ** 2 for s in scene.sats) / 2.0
    nv = scene.noise_sigma ** 2 * fs_in / scene.sample_rate
    rms = np.sqrt(p + (nv / 4.0 if real else nv / 2.0))
    return 0.2 / rms


def render(scene, fs_in, fmt, if_hz, i0, n):
    """Stored samples [i0, i0 + n) in `fmt` (numpy array of the format's dtype)."""
    real = fmt == 'r8'
    return R.add_quantise(signal(scene, fs_in, if_hz, real, i0, n), fmt, scale(scene, fs_in, real))


def write(path, scene, fs_in, fmt, if_hz, seconds, chunk=1 << 21):
    n = int(round(seconds * fs_in))
    with open(path, 'wb') as f:
        for a in range(0, n, chunk):
            render(scene, fs_in, fmt, if_hz, a, min(chunk, n - a)).tofile(f)
    return n
