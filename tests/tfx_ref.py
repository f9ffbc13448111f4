"""numpy restatement of the time-frequency (sweep) excision (gpsmi_tfx_*, include/gpsmi.h), float64
throughout: the contract the HIP kernels of csrc/gpsmi_tfx.hip are tested against.

One block of n complex samples (n % 128 == 0, n >= 1024) is cut into frames of L = 32 / 64 / 128 /
256 samples at hop H = L / 2: frame f = 0 .. nf - 1 (nf = n / H) covers block samples [f H - H,
f H + H), frame 0 taking its first H samples from the carry (the previous block's last H input
samples, zero after a reset).  Window: periodic Hann w[i] = 0.5 - 0.5 cos(2 pi i / L); the last frame
uses w[i] for i < H and 1 for i >= H, so the frames sum to 1 at every output sample without reading
the next block.

Detection: P[f][k] = |FFT(w x_f)[k]|^2; floor = the lower median (rank (m - 1) // 2) of the
m = (nf - 1) L values of all frames but the last; T = floor 10^(thresh_db / 10), the last frame's
threshold T 11/6 (its window carries 11/6 of Hann's power); a cell is a detection when P > T, and
every detection is widened by +-dilate bins circularly inside its frame.  More than
floor(max_frac nf L) flagged cells: the block passes through unchanged, count -1, empty mask.  Apply:
the flagged cells are zeroed, every frame is transformed back and the frames are overlap-added.
"""
import numpy as np

FRAMES = (32, 64, 128, 256)
LAST_GAIN = 11.0 / 6.0          # sum(w_last^2) / sum(w^2) = (3/16 + 1/2) / (3/8)


def window(L):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L) / L)


def check_block(n):
    return n % 128 == 0 and n >= 1024


def limit_of(max_frac, nf, L):
    """floor(max_frac nf L) with max_frac the float32 the ABI carries, the product in double."""
    return int(np.floor(float(np.float32(max_frac)) * float(nf) * float(L)))


def widen(raw, dilate):
    """bool [nf, L] -> the same with every True spread over +-dilate bins, circularly per frame."""
    mask = raw.copy()
    for d in range(1, dilate + 1):
        mask |= np.roll(raw, d, axis=1) | np.roll(raw, -d, axis=1)
    return mask


class SweepRef:
    def __init__(self, n, L=64, thresh_db=12.0, dilate=1, max_frac=0.5):
        if not check_block(n) or L not in FRAMES:
            raise ValueError('block length: a multiple of 128 >= 1024; frame: 32, 64, 128 or 256')
        self.n, self.L, self.H, self.nf = n, L, L // 2, n // (L // 2)
        self.thresh_db, self.dilate, self.max_frac = thresh_db, dilate, max_frac
        self.limit = limit_of(max_frac, self.nf, L)
        self.w = window(L)
        self.w_last = self.w.copy()
        self.w_last[self.H:] = 1.0
        self.reset()

    def reset(self):
        self.carry = np.zeros(self.H, dtype=np.complex128)

    def frames(self, x):
        """[nf, L] windowed frames of block x (complex128) behind the current carry."""
        H, L, nf = self.H, self.L, self.nf
        ext = np.concatenate([self.carry, x])
        fr = np.lib.stride_tricks.sliding_window_view(ext, L)[::H][:nf].copy()
        fr[:-1] *= self.w[None, :]
        fr[-1] *= self.w_last
        return fr

    def detect(self, P):
        """(floor, T, mask bool [nf, L], count) from the cell powers [nf, L]."""
        vals = np.sort(P[:-1].ravel())
        floor = vals[(len(vals) - 1) // 2]
        with np.errstate(invalid='ignore', over='ignore'):
            T = floor * 10.0 ** (self.thresh_db / 10.0)
            raw = P > T
            raw[-1] = P[-1] > T * LAST_GAIN
        mask = widen(raw, self.dilate)
        count = int(mask.sum())
        if count > self.limit:
            return floor, T, np.zeros_like(mask), -1
        return floor, T, mask, count

    def process(self, x):
        """One block -> (y complex128 [n], count, mask bool [nf, L], P, floor, T); advances the carry."""
        x = np.asarray(x).astype(np.complex128)
        assert x.shape == (self.n,)
        spectra = np.fft.fft(self.frames(x), axis=1)
        P = spectra.real ** 2 + spectra.imag ** 2
        floor, T, mask, count = self.detect(P)
        y = x.copy() if count < 0 else self._overlap_add(spectra, mask)
        self.carry = x[-self.H:].copy()
        return y, count, mask, P, floor, T

    def excise_with(self, x, mask):
        """Block x with a given mask applied, behind the current carry, which is left as it is."""
        x = np.asarray(x).astype(np.complex128)
        return self._overlap_add(np.fft.fft(self.frames(x), axis=1), mask)

    def _overlap_add(self, spectra, mask):
        H = self.H
        back = np.fft.ifft(np.where(mask, 0.0, spectra), axis=1)
        y = np.zeros(self.n + H, dtype=np.complex128)          # (index 0: carry sample 0)
        y[:self.n] += back[:, :H].ravel()
        y[H:] += back[:, H:].ravel()
        return y[H:]

    def run(self, xs):
        """Consecutive blocks -> (y [nb, n], counts, masks bool [nb, nf, L], floors)."""
        out = [self.process(x) for x in xs]
        return (np.stack([o[0] for o in out]), np.array([o[1] for o in out]), np.stack([o[2] for o in out]),
                np.array([o[4] for o in out]))


def mask_words(mask):
    """bool [..., L] (or any length % 32 == 0) -> uint32 [size / 32], cell c of the flattened plane in bit
    c % 32 of word c // 32 (the ABI's layout: frame f's words are f L / 32 ..)."""
    bits = np.asarray(mask, dtype=np.uint32).reshape(-1, 32)
    return (bits << np.arange(32, dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint32)


def words_to_mask(words, L):
    w = np.asarray(words, dtype=np.uint32).reshape(-1)
    return ((w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(bool).reshape(-1, L)


def sweep(first_sample, n, fs, jn_db, noise_power, span_hz, period_s, phase=0.3):
    """A linear sweep from -span_hz to +span_hz every period_s, jn_db above noise_power, over the
    absolute samples [first_sample, first_sample + n): phase 2 pi (-S tau + r tau^2 / 2), tau = t mod
    period_s, r = 2 S / period_s, t absolute, so that consecutive blocks join and the wrap is inside."""
    amp = np.sqrt(noise_power * 10.0 ** (jn_db / 10.0))
    t = (np.arange(n, dtype=np.float64) + float(first_sample)) / fs
    tau = np.mod(t, period_s)
    r = 2.0 * span_hz / period_s
    return amp * np.exp(1j * (2.0 * np.pi * (-span_hz * tau + 0.5 * r * tau * tau) + phase))


def comb(n, L, every=3, level=1.0):
    """Tones on every `every`-th bin of the L-point transform, equal amplitudes: with the Hann window's
    three-bin main lobe they fill the plane of every frame."""
    k = np.arange(n, dtype=np.float64)
    x = np.zeros(n, dtype=np.complex128)
    for b in range(0, L, every):
        x += level * np.exp(2j * np.pi * ((b * k) % L) / L + 1j * b)
    return x


def quantise(x):
    """complex128 -> the recorder's uint16 (Q << 8 | I), as synth.Scene.block_raw does."""
    i = np.clip(np.rint((x.real + 1.0) * 127.5), 0, 255).astype(np.uint16)
    q = np.clip(np.rint((x.imag + 1.0) * 127.5), 0, 255).astype(np.uint16)
    return (q << 8) | i


def raw_to_c64(raw):
    """uint16 (Q << 8 | I) -> complex64, as gpsmi.synth.raw_to_c64 and the kernels' decode."""
    im, re = np.divmod(raw, 256)
    return np.asarray(re + 1j * im, dtype=np.complex64) / 127.5 - (1 + 1j)


# --------------------------------------------------------------------------------------------
# Select / threshold / widen / count restated in float32 on a given P, a float32 oracle of the whole
# filter, and the case table of tests/test_tfx_ref.py (CPU) and tests/test_gpu_tfx_ref.py (GPU).

def detect_from_power(P32, thresh_db=12.0, dilate=1, max_frac=0.5):
    """tfx_select_kernel and tfx_mask_kernel on a given float32 P [nf, L], operation for operation:
    the floor is the order statistic (m - 1) // 2 of the float32 values of the frames but the last,
    T = floor * float32(10^(thresh_db / 10)) and T * float32(11 / 6) in float32, the comparison is a
    strict >, the widening wraps inside the frame, and a count above floor(max_frac nf L) gives -1 and
    an empty mask.  -> (floor float32, mask bool [nf, L], count)."""
    P = np.asarray(P32)
    assert P.dtype == np.float32 and P.ndim == 2
    nf, L = P.shape
    vals = np.sort(P[:-1].ravel())
    floor = vals[(len(vals) - 1) // 2]
    with np.errstate(over='ignore', invalid='ignore'):
        f = np.float32(10.0 ** (float(np.float32(thresh_db)) / 10.0))
        T = np.float32(floor * f)
        TL = np.float32(T * np.float32(LAST_GAIN))
        raw = P > T
        raw[-1] = P[-1] > TL
    mask = widen(raw, dilate)
    count = int(mask.sum())
    if count > limit_of(max_frac, nf, L):
        return floor, np.zeros_like(mask), -1
    return floor, mask, count


class Oracle32:
    """The filter in float32, as a careful float32 implementation other than the kernel's would do it:
    complex64 samples, the float32 window, complex64 transforms (scipy.fft keeps the type), re^2 +
    im^2 in float32, overlap-add in complex64.  Its distance from SweepRef is what float32 costs; the
    kernels are held to a small multiple of it."""

    def __init__(self, n, L):
        assert check_block(n) and L in FRAMES
        self.n, self.L, self.H, self.nf = n, L, L // 2, n // (L // 2)
        self.w = window(L).astype(np.float32)
        self.w_last = self.w.copy()
        self.w_last[self.H:] = 1.0
        self.carry = np.zeros(self.H, dtype=np.complex64)

    def spectra(self, x):
        import scipy.fft
        assert x.dtype == np.complex64 and x.shape == (self.n,)
        ext = np.concatenate([self.carry, x])
        fr = np.lib.stride_tricks.sliding_window_view(ext, self.L)[::self.H][:self.nf].copy()
        fr[:-1] *= self.w[None, :]
        fr[-1] *= self.w_last
        assert fr.dtype == np.complex64
        sp = scipy.fft.fft(fr, axis=1)
        assert sp.dtype == np.complex64, sp.dtype
        return sp

    @staticmethod
    def power(sp):
        P = sp.real * sp.real + sp.imag * sp.imag
        assert P.dtype == np.float32
        return P

    def overlap_add(self, sp, mask):
        import scipy.fft
        H = self.H
        back = scipy.fft.ifft(np.where(mask, np.complex64(0), sp), axis=1)
        assert back.dtype == np.complex64, back.dtype
        y = np.empty(self.n, dtype=np.complex64)
        y[:self.n - H] = (back[:-1, H:] + back[1:, :H]).ravel()
        y[self.n - H:] = back[-1, H:]
        return y


def rms(x):
    return float(np.sqrt(np.mean(np.abs(np.asarray(x).astype(np.complex128)) ** 2)))


def power_metric(P, P64):
    """max over the cells of |P - P64| / sqrt(P64 mean(P64)): the error of |X|^2 is 2 |X| delta, with
    delta set by the plane's mean energy.  (Cells with P64 == 0 are held to equality.)"""
    P64 = np.asarray(P64, dtype=np.float64)
    d = np.abs(np.asarray(P, dtype=np.float64) - P64)
    if P64.mean() == 0:
        return 0.0 if not d.any() else np.inf
    den = np.sqrt(P64 * P64.mean())
    return float(np.max(np.where(den > 0, d / np.where(den > 0, den, 1.0), np.where(d > 0, np.inf, 0.0))))


SIGMA = 0.35                    # noise per complex sample, as synth.Scene
NOISE_POWER = SIGMA ** 2
BORDERLINE_CAP = 16             # cells per block whose P64 may lie within the power bound of the threshold


def noise(seed, count):
    rng = np.random.default_rng(seed)
    return (SIGMA / np.sqrt(2.0)) * (rng.standard_normal(count) + 1j * rng.standard_normal(count))


def tone(jn_db, cycles_per_sample, first, count, phase=0.3):
    amp = np.sqrt(NOISE_POWER * 10.0 ** (jn_db / 10.0))
    k = np.arange(first, first + count, dtype=np.float64)
    return amp * np.exp(1j * (2.0 * np.pi * np.mod(cycles_per_sample * k, 1.0) + phase))


def pulses(seed, count, width, every, jn_db):
    """Bursts of `width` samples every `every` samples (jittered), jn_db above the noise: wider than a
    frame, so that whole frames are flagged."""
    rng = np.random.default_rng(seed)
    x = np.zeros(count, dtype=np.complex128)
    amp = np.sqrt(NOISE_POWER * 10.0 ** (jn_db / 10.0))
    for s in range(every // 2, count - width, every):
        s += int(rng.integers(0, every // 4))
        x[s:s + width] = amp * np.exp(2j * np.pi * rng.random(width))
    return x


NB = 3                          # blocks per case, chained behind a reset
SHAPES = tuple((n, L) for n in (1024, 4096, 130944) for L in FRAMES if n >= 8 * L)
INPUTS = ('sweep', 'tone', 'pulses', 'noise')
# (seed offsets of cases whose float32 oracle has more than BORDERLINE_CAP cells within the power bound of
# the threshold: the seed is moved, the cap stays; none needed so far)
RESEED = {}


def case_name(n, L, fmt, kind):
    return f'{kind}-{n}-L{L}-{fmt}'


def _build(n, L, fmt, kind, seed):
    """complex128 [NB, n].  Raw u8 clips at +-1: the whole scene is scaled so that the jammer's
    amplitude stays inside (every jammed kind by 0.05: the 30 dB jammers then peak at 0.55)."""
    count = NB * n
    x = noise(seed, count)
    fs = 2.048e6
    if kind == 'sweep':                                     # one sweep of +-0.8 MHz per 1 ms, 30 dB up
        x = x + sweep(0, count, fs, 30.0, NOISE_POWER, 0.8e6, 1e-3)
    elif kind == 'tone':                                    # between two bins of every L
        x = x + tone(30.0, 0.1137, 0, count)
    elif kind == 'pulses':
        x = x + pulses(seed + 1, count, 3 * L, max(n // 3, 12 * L), 30.0)
    if fmt == 'u8':
        x = x * (0.05 if kind != 'noise' else 1.0)
    return x.reshape(NB, n)


CASES = {}
for _i, (_n, _L) in enumerate(SHAPES):
    for _j, _kind in enumerate(INPUTS):
        for _k, _fmt in enumerate(('c64', 'u8')):
            _name = case_name(_n, _L, _fmt, _kind)
            _seed = 5000 + 100 * _i + 10 * _j + _k + RESEED.get(_name, 0)
            CASES[_name] = dict(n=_n, L=_L, fmt=_fmt, kind=_kind, seed=_seed,
                                params=dict(thresh_db=12.0, dilate=1, max_frac=0.5))

_MEMO = {}


def case_input(name):
    """(x complex64 [NB, n]: what the filter sees; raw uint16 [NB, n] or None: what a raw-u8 handle is
    given).  Memoised; callers leave both unchanged."""
    key = ('in', name)
    if key not in _MEMO:
        c = CASES[name]
        x = _build(c['n'], c['L'], c['fmt'], c['kind'], c['seed'])
        if c['fmt'] == 'u8':
            raw = quantise(x)
            _MEMO[key] = (raw_to_c64(raw), raw)
        else:
            _MEMO[key] = (x.astype(np.complex64), None)
        for a in _MEMO[key]:
            if a is not None:
                a.setflags(write=False)
    return _MEMO[key]


def reference(name):
    """The float64 reference and the float32 oracle over the blocks of a case, chained behind a reset.
    One record per block: carry (complex128, before the block), y, count, mask, P, floor, T of SweepRef;
    pow_dev and out_dev: the oracle's distance from them in the tests' two metrics (out_dev with the
    reference's mask; None where the block passes through); P32: the oracle's P."""
    key = ('ref', name)
    if key not in _MEMO:
        c = CASES[name]
        x = case_input(name)[0]
        ref, orc = SweepRef(c['n'], c['L'], **c['params']), Oracle32(c['n'], c['L'])
        recs = []
        for b in range(NB):
            carry = ref.carry.copy()
            y, count, mask, P, floor, T = ref.process(x[b])
            sp = orc.spectra(x[b])
            P32 = orc.power(sp)
            rec = dict(carry=carry, y=y, count=count, mask=mask, P=P, floor=floor, T=T, P32=P32,
                       pow_dev=power_metric(P32, P), out_dev=None)
            if count >= 0:
                rec['out_dev'] = float(np.abs(orc.overlap_add(sp, mask) - y).max()) / rms(x[b])
            orc.carry = x[b, -orc.H:].copy()
            recs.append(rec)
        _MEMO[key] = recs
    return _MEMO[key]


def oracle_worst(name):
    """(power, out): the oracle's worst deviations over the blocks of a case."""
    recs = reference(name)
    return (max(r['pow_dev'] for r in recs),
            max([r['out_dev'] for r in recs if r['out_dev'] is not None], default=None))


def borderline(rec, pow_bound):
    """bool [nf, L]: the cells of a block whose P64 lies within the power bound (the metric's bound turned
    back into an absolute error at the cell) of their threshold, before the widening: float32 may put
    them on either side."""
    P = rec['P']
    thr = np.full(P.shape, rec['T'])
    thr[-1] = rec['T'] * LAST_GAIN
    with np.errstate(invalid='ignore'):
        return np.abs(P - thr) <= pow_bound * np.sqrt(P * P.mean())
