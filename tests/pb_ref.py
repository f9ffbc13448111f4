"""numpy restatement of the pulse blanking (gpsmi_pb_*, include/gpsmi.h): the contract the HIP kernels
of csrc/gpsmi_pb.hip must equal bit for bit, and the jammer scenes of the tests.

Every step is exact in float32 or in integers: p = re*re + im*im (numpy float32, never fused), the
floor m = np.partition(p, (n-1)//2)[(n-1)//2], T = float32(m) * float32(10^(thresh_db/10)), detections
p > T, sample i blanked when a detection j of the block has i - post <= j <= i + pre or when i < carry
(carry = max(0, j + post - n + 1) over the previous block's detections), more than
floor(max_frac * n) blanked: the block passes through with count -1 and an empty mask.
"""
import numpy as np


def f_of(thresh_db):
    """10^(thresh_db / 10) in double, rounded to float32 (thresh_db as the ABI's float32)."""
    return np.float32(10.0 ** (float(np.float32(thresh_db)) / 10.0))


def power(x):
    x = np.asarray(x, dtype=np.complex64)
    return x.real * x.real + x.imag * x.imag


def lower_median(p):
    k = (len(p) - 1) // 2
    return np.partition(p, k)[k]


def default_guard(code_samples):
    return max(2, int(round(2 * code_samples / 2048)))


class BlankerRef:
    def __init__(self, n, thresh_db=10.0, pre=2, post=2, max_frac=0.5):
        self.n, self.pre, self.post = n, pre, post
        self.f = f_of(thresh_db)
        self.limit = int(np.floor(float(np.float32(max_frac)) * n))
        self.reset()

    def reset(self):
        self.carry = 0

    def process(self, x):
        """One block (complex64 [n]) -> (y complex64, count, floor float32, blank bool [n]); advances
        the carry."""
        x = np.asarray(x, dtype=np.complex64)
        n = self.n
        assert x.shape == (n,)
        p = power(x)
        m = lower_median(p)
        with np.errstate(invalid='ignore', over='ignore'):
            T = np.float32(m * self.f)
            det = p > T
        c = np.concatenate([[0], np.cumsum(det)])
        i = np.arange(n)
        hi = np.minimum(i + self.pre, n - 1)
        lo = np.maximum(i - self.post, 0)
        blank = ((c[hi + 1] - c[lo]) > 0) | (i < self.carry)
        js = np.flatnonzero(det)
        self.carry = max(0, int(js[-1]) + self.post - n + 1) if len(js) else 0
        count = int(blank.sum())
        if count > self.limit:
            return x.copy(), -1, m, np.zeros(n, dtype=bool)
        y = np.where(blank, np.complex64(0), x).astype(np.complex64)
        return y, count, m, blank

    def run(self, blocks):
        """Consecutive blocks [nb, n] -> (y [nb, n], counts int32 [nb], floors float32 [nb], masks uint32
        [nb, n/32])."""
        ys, cs, fs, ms = [], [], [], []
        for x in blocks:
            y, c, m, b = self.process(x)
            ys.append(y)
            cs.append(c)
            fs.append(m)
            ms.append(mask_words(b))
        return np.stack(ys), np.array(cs, dtype=np.int32), np.array(fs, dtype=np.float32), np.stack(ms)


def mask_words(blank):
    """bool [n] -> uint32 [n / 32], sample i in bit i % 32 of word i // 32."""
    return np.packbits(np.asarray(blank, dtype=bool).reshape(-1, 32), axis=1,
                       bitorder='little').view('<u4').reshape(-1).astype(np.uint32)


def words_to_mask(words):
    w = np.asarray(words, dtype=np.uint32).reshape(-1)
    return ((w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(bool).reshape(-1)


# ---- scenes ------------------------------------------------------------------------------------

def _cgauss(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


def add_pulses(x, noise_power, seed, jn_db=30.0, width=8, duty=0.15):
    """x + bursts of complex Gaussian noise `width` samples wide at about `duty` of the samples, each
    jn_db above noise_power; burst starts from a seeded RNG.  -> (y, bool mask of the burst samples)."""
    n = len(x)
    rng = np.random.default_rng(seed)
    starts = rng.choice(n // width, size=int(round(duty * n / width)), replace=False) * width
    on = np.zeros(n, dtype=bool)
    for s in starts:
        on[s:s + width] = True
    amp = np.sqrt(noise_power * 10.0 ** (jn_db / 10.0))
    y = np.asarray(x, dtype=np.complex128).copy()
    y[on] += amp * _cgauss(rng, int(on.sum()))
    return y, on


def chirp(first_sample, n, fs, jn_db, noise_power, sweep_hz=8e6, period_s=20e-6, over=16, taps=None):
    """A linear chirp sweeping -sweep_hz .. +sweep_hz every period_s, rendered at over * fs as a
    function of absolute time (blocks join up), low-passed to +-0.9 MHz with a float64 Hamming-windowed
    sinc and decimated to fs; samples first_sample .. first_sample + n.  Its power in band is jn_db
    above noise_power during a burst."""
    fh = over * fs
    if taps is None:
        taps = 16 * over + 1
    half = taps // 2
    k = np.arange((first_sample * over) - half, (first_sample + n) * over + half, dtype=np.float64)
    t = k / fh
    tau = np.mod(t, period_s)
    rate = 2.0 * sweep_hz / period_s
    ph = 2.0 * np.pi * (-sweep_hz * tau + 0.5 * rate * tau * tau)
    z = np.exp(1j * ph)
    m = np.arange(taps) - half
    fc = 0.9e6 / fh
    h = 2.0 * fc * np.sinc(2.0 * fc * m) * np.hamming(taps)
    h /= h.sum()
    y = np.convolve(z, h, mode='valid')[::over][:n]
    amp = np.sqrt(noise_power * 10.0 ** (jn_db / 10.0))
    return amp * y
