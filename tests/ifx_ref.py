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


# --------------------------------------------------------------------------------------------
# The mask pass restated in float32, a float32 oracle of the whole filter, and the case table of
# tests/test_ifx_ref.py (CPU) and tests/test_gpu_excision_ref.py (GPU).

def detect_from_psd(P32, thresh_db, dilate, max_bins):
    """ifx_mask_kernel on a given float32 P, operation for operation: the threshold is
    float32(0.5) * (s[1023] + s[1024]) * float32(10^(thresh_db / 10)) on the ascending sort, the
    comparison is a strict >, the widening wraps, and a count above max_bins gives -1 and an empty
    mask.  -> (mask bool[L], count, threshold float32)."""
    P = np.asarray(P32)
    assert P.dtype == np.float32 and P.shape == (L,)
    s = np.sort(P)
    with np.errstate(over='ignore', invalid='ignore'):
        scale = np.float32(10.0 ** (float(np.float32(thresh_db)) / 10.0))
        thr = np.float32(0.5) * (s[L // 2 - 1] + s[L // 2]) * scale
        raw = P > thr
    mask, count = widen_and_count(raw, dilate, max_bins)
    return mask, count, thr


def widen_and_count(raw, dilate, max_bins):
    """The flagged bins widened circularly by +-dilate, then the count and the wideband rule."""
    mask = raw.copy()
    for d in range(1, dilate + 1):
        mask |= np.roll(raw, d) | np.roll(raw, -d)
    count = int(mask.sum())
    if count > max_bins:
        return np.zeros(L, dtype=bool), -1
    return mask, count


class Oracle32:
    """The filter in float32, as a careful float32 implementation other than the kernel's would do
    it: complex64 samples, the float32 window, complex64 transforms (scipy.fft keeps the type),
    |X|^2 summed over frames ascending within groups of 8 and then over the groups, overlap-add in
    complex64.  Its distance from ExcisionRef is what float32 costs; the kernels are held to a small
    multiple of it."""
    GROUP = 8

    def __init__(self, n):
        assert check_block(n)
        self.n = n
        self.w = window().astype(np.float32)
        self.w_last = self.w.copy()
        self.w_last[H:] = 1.0
        self.carry = np.zeros(H, dtype=np.complex64)

    def spectra(self, x):
        import scipy.fft
        assert x.dtype == np.complex64 and x.shape == (self.n,)
        ext = np.concatenate([self.carry, x])
        nf = self.n // H
        fr = np.stack([ext[m * H:m * H + L] for m in range(nf)])
        fr[:-1] *= self.w[None, :]
        fr[-1] *= self.w_last
        assert fr.dtype == np.complex64
        sp = scipy.fft.fft(fr, axis=1)
        assert sp.dtype == np.complex64, sp.dtype
        return sp

    def psd(self, sp):
        a = sp.real * sp.real + sp.imag * sp.imag
        assert a.dtype == np.float32
        nfp = sp.shape[0] - 1
        total = np.zeros(L, dtype=np.float32)
        for g in range(0, nfp, self.GROUP):
            acc = np.zeros(L, dtype=np.float32)
            for f in range(g, min(g + self.GROUP, nfp)):
                acc += a[f]
            total += acc
        return total / np.float32(nfp)

    def overlap_add(self, sp, mask):
        import scipy.fft
        sp = sp.copy()
        sp[:, mask] = 0
        back = scipy.fft.ifft(sp, axis=1)
        assert back.dtype == np.complex64, back.dtype
        y = np.empty(self.n, dtype=np.complex64)
        nf = sp.shape[0]
        for s in range(nf - 1):
            y[s * H:s * H + H] = back[s, H:] + back[s + 1, :H]
        y[(nf - 1) * H:] = back[nf - 1, H:]
        return y


def rms(x):
    return float(np.sqrt(np.mean(np.abs(np.asarray(x).astype(np.complex128)) ** 2)))


def psd_metric(P, P64):
    """max_k |P_k - P64_k| / sqrt(P64_k mean(P64)): the error of |X_k|^2 is 2 |X_k| delta, with delta
    set by the frame's total energy."""
    P64 = np.asarray(P64, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(P, dtype=np.float64) - P64) / np.sqrt(P64 * P64.mean())))


SIGMA = 0.35                    # noise per complex sample, as synth.Scene
NOISE_POWER = SIGMA ** 2
TONE_BIN = -2717.3 / 1000.0     # the CW tone of tests/test_gpu_excision.py, in bins of 1 kHz
DEFAULT = dict(thresh_db=6.0, dilate=2, max_bins=256)


def noise(seed, count):
    rng = np.random.default_rng(seed)
    return (SIGMA / np.sqrt(2.0)) * (rng.standard_normal(count) + 1j * rng.standard_normal(count))


def tone(jn_db, bin_, first, count, phase=0.3):
    """A CW tone jn_db above the noise power at `bin_` (in bins of the 2048-point transform, any
    real number) over absolute samples [first, first + count): the phase runs on across blocks."""
    amp = np.sqrt(NOISE_POWER * 10.0 ** (jn_db / 10.0))
    k = np.arange(first, first + count, dtype=np.float64)
    return amp * np.exp(1j * (2.0 * np.pi * ((bin_ * k) % L) / L + phase))


def wideband(seed, n):
    """Interference over a quarter of the band, as test_unsupported_config_and_wideband_pass_through
    builds it: flat over n/4 bins of the block's own spectrum, random phases."""
    spec = np.zeros(n, dtype=np.complex128)
    lo, wd = n // 16, n // 4
    spec[lo:lo + wd] = np.exp(2j * np.pi * np.random.default_rng(seed).random(wd))
    return np.fft.ifft(spec) * np.sqrt(n) * 3.0


def _chain(seed, n, nb, jn_db, bins):
    x = noise(seed, nb * n)
    for b in bins:
        x = x + tone(jn_db, b, 0, nb * n)
    return x.reshape(nb, n)


def _period(seed, n, jn_db=35.0, jn2_db=12.0):
    """The 7 distinct blocks of the run-length cases: five jammed (a tone of jn_db at -5 cycles per
    block, so that the tiling keeps its phase; a tone of jn2_db at 603 cycles per block on top of
    blocks 1 and 3), one of noise only, one wideband."""
    x = noise(seed, 7 * n).reshape(7, n)
    for b in range(5):
        x[b] += tone(jn_db, -5 * float(L) / n, 0, n)
    for b in (1, 3):
        x[b] += tone(jn2_db, 603 * float(L) / n, 0, n)
    x[6] += wideband(seed + 1, n)
    return x


# name -> n, nb, format, parameters, input builder, expected class of outcome per block ('+': count
# > 0, '0', '-': -1) of the blocks that are held to float64 (all of them, or the first 14)
CASES = {}


def _case(name, n, nb, build, fmt='c64', classes=None, held=None, **params):
    CASES[name] = dict(n=n, nb=nb, fmt=fmt, build=build, classes=classes, held=held or nb,
                       params=dict(DEFAULT, **params))


SHAPES = (4096, 5120, 9216, 10240, 16384, 32768, 65536)
for _i, _n in enumerate(SHAPES):
    # (a) 35 dB tone in complex64; 3 dB in raw u8 (amplitude 0.5: the format clips at +-1)
    _case(f'shape-{_n}-c64', _n, 3, lambda n=_n, s=100 + _i: _chain(s, n, 3, 35.0, [TONE_BIN]),
          classes='-++' if _n <= 5120 else '+++')
    _case(f'shape-{_n}-u8', _n, 3, lambda n=_n, s=200 + _i: _chain(s, n, 3, 3.0, [TONE_BIN]), fmt='u8',
          classes='+++')

# (b) run lengths: name -> n, nb, format; the period tiled to nb blocks, the first 14 held to float64
RUNS = {'run-S2': (5120, 820, 'c64'), 'run-S4': (5120, 1639, 'c64'), 'run-S8': (20480, 820, 'c64'),
        'run-S8-clipped': (4096, 4096, 'u8'), 'run-S1-under': (4096, 1023, 'c64')}
RUN_S = {'run-S2': 2, 'run-S4': 4, 'run-S8': 8, 'run-S8-clipped': 8, 'run-S1-under': 1}


def run_length(n, nb):
    """S of ifx_run: output segments per apply workgroup."""
    segs = nb * (n // H)
    return 8 if segs >= 16384 else 4 if segs >= 8192 else 2 if segs >= 4096 else 1


def _tiled(seed, n, fmt):
    """Two periods: the blocks held to float64 (raw u8 clips at +-1: a 3 dB tone there, and the whole
    period scaled by 0.4)."""
    p = _period(seed, n) if fmt == 'c64' else 0.4 * _period(seed, n, 3.0, -3.0)
    return np.tile(p, (2, 1))


def tile_to(blocks, nb):
    """The first 7 blocks of a run-length case's input, repeated to nb blocks."""
    return np.ascontiguousarray(np.tile(blocks[:7], ((nb + 6) // 7, 1))[:nb])


# (c) parameters and bin edges at n = 16384: two chained blocks, 10 dB tones on exact bins
PARAM_N = 16384
# (a tone on bin k fills k - 1 .. k + 1 under the Hann window: on bins 0 and 2047 the flagged bins
# straddle the end of the spectrum already, and a widening that clamped would give the same mask;
# on bins 1 and 2046 only the widening crosses it)
EDGE_BINS = {'bin0': [0], 'bin2047': [2047], 'bin1024': [1024], 'bins31-32': [31, 32],
             'bins63-64': [63, 64], 'bins255-256': [255, 256], 'bin1': [1], 'bin2046': [2046]}
EDGE_DILATES = {'bin0': (0, 1, 2, 64), 'bin2047': (0, 1, 2, 64), 'bins31-32': (0, 1, 2, 64),
                'bin1': (1, 64), 'bin2046': (1, 64)}
for _i, (_k, _bins) in enumerate(EDGE_BINS.items()):
    for _d in EDGE_DILATES.get(_k, (2,)):
        _case(f'edge-{_k}-d{_d}', PARAM_N, 2, lambda s=300 + _i, b=_bins: _chain(s, PARAM_N, 2, 10.0, b),
              classes='++', dilate=_d, max_bins=2048 if _d == 64 else 256)
# (thresh_db 0 and no widening: exactly the 1024 bins above the mean of the two middle values)
_case('param-t0-d0-m2048', PARAM_N, 2, lambda: _chain(310, PARAM_N, 2, 15.0, [TONE_BIN]), classes='++',
      thresh_db=0.0, dilate=0, max_bins=2048)
for _t, _mb, _cl in ((0.0, 2048, '++'), (3.0, 2048, '++'), (12.0, 256, '++'), (-np.inf, 2048, '++'),
                     (6.0, 0, '--'), (6.0, 2048, '++')):
    _case(f'param-t{_t:g}-m{_mb}', PARAM_N, 2, lambda: _chain(310, PARAM_N, 2, 15.0, [TONE_BIN]),
          classes=_cl, thresh_db=_t, max_bins=_mb)
_case('param-noise-m0', PARAM_N, 2, lambda: _chain(311, PARAM_N, 2, -np.inf, [0]), classes='00', max_bins=0)
MAXBINS_BASE = 'param-t6-m2048'          # max_bins = c against c - 1, c its block 1's count


def maxbins_pair():
    """The two cases around the wideband rule: max_bins = c (count c) and c - 1 (count -1), with c
    the reference's count of block 1 of MAXBINS_BASE."""
    c = reference(MAXBINS_BASE)[1]['count']
    for mb in (c, c - 1):
        name = f'param-maxbins-{mb}'
        if name not in CASES:
            _case(name, PARAM_N, 2, CASES[MAXBINS_BASE]['build'], classes=None, max_bins=mb)
    return c, f'param-maxbins-{c}', f'param-maxbins-{c - 1}'


# (d) edges


def _zero_then_jammed():
    x = _chain(320, PARAM_N, 2, 35.0, [TONE_BIN])
    x[0] = 0
    return x


WIDE_N = 32768


def _wideband_in_the_middle(jn_db, scale=1.0):
    x = _chain(321, WIDE_N, 3, jn_db, [TONE_BIN])
    x[1] += wideband(322, WIDE_N)
    return x * scale


_case('edge-zero-then-jammed', PARAM_N, 2, _zero_then_jammed, classes='0+')
_case('edge-wideband-middle-c64', WIDE_N, 3, lambda: _wideband_in_the_middle(35.0), classes='+-+')
_case('edge-wideband-middle-u8', WIDE_N, 3, lambda: _wideband_in_the_middle(3.0, 0.4), fmt='u8',
      classes='+-+')
_case('edge-format-switch', PARAM_N, 2, lambda: raw_to_c64(quantise(_chain(323, PARAM_N, 2, 3.0, [TONE_BIN]))),
      classes='++')
_case('edge-1-plus-3', PARAM_N, 4, lambda: _chain(324, PARAM_N, 4, 35.0, [TONE_BIN]), classes='++++')

# (block 0 stands behind a reset, block 7 behind the wideband block; the noise-only block behind a 35
# dB tone takes the tone's end in its frame 0: wideband at the short lengths, a wide mask at 20480)
_RUN_CLASSES = {'run-S2': '-++++---++++--', 'run-S4': '-++++---++++--', 'run-S8': '++++++--+++++-',
                'run-S8-clipped': '++++++--+++++-', 'run-S1-under': '-++++---++++--'}
for _i, (_k, (_n, _nb, _fmt)) in enumerate(RUNS.items()):
    _case(_k, _n, _nb, lambda s=400 + _i, n=_n, f=_fmt: _tiled(s, n, f),
          fmt=_fmt, held=14, classes=_RUN_CLASSES.get(_k))


def raw_to_c64(raw):
    """uint16 (Q << 8 | I) -> complex64, as gpsmi.synth.raw_to_c64 and the kernels' decode."""
    im, re = np.divmod(raw, 256)
    return np.asarray(re + 1j * im, dtype=np.complex64) / 127.5 - (1 + 1j)


_MEMO = {}


def case_input(name):
    """(x complex64 [held, n]: what the filter sees; raw uint16 [held, n] or None: what a raw-u8
    handle is given).  held = nb, but for the run-length cases: their first 14 blocks, which
    tile_to repeats.  Memoised; callers leave both unchanged."""
    key = ('in', name)
    if key not in _MEMO:
        c = CASES[name]
        x = c['build']()
        assert x.shape == (c['held'], c['n'])
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
    """The float64 reference and the float32 oracle over the held blocks of a case, chained behind a
    reset.  One record per block: carry (complex128, before the block), y, count, mask, P, thr of
    ExcisionRef; psd_dev and out_dev: the oracle's distance from them in the tests' two metrics
    (out_dev with the reference's mask; None where the block passes through or is all zero)."""
    key = ('ref', name)
    if key not in _MEMO:
        c = CASES[name]
        x = case_input(name)[0]
        ref, orc = ExcisionRef(c['n'], **c['params']), Oracle32(c['n'])
        recs = []
        for b in range(c['held']):
            carry = ref.carry.copy()
            y, count, mask, P, thr = ref.process(x[b])
            sp = orc.spectra(x[b])
            rec = dict(carry=carry, y=y, count=count, mask=mask, P=P, thr=thr, psd_dev=None, out_dev=None)
            if P.min() > 0:
                rec['psd_dev'] = psd_metric(orc.psd(sp), P)
                if count >= 0:
                    rec['out_dev'] = float(np.abs(orc.overlap_add(sp, mask) - y).max()) / rms(x[b])
            orc.carry = x[b, -H:].copy()
            recs.append(rec)
        _MEMO[key] = recs
    return _MEMO[key]


def oracle_worst(name):
    """(psd, out): the oracle's worst deviations over the held blocks of a case."""
    recs = reference(name)
    return (max(r['psd_dev'] for r in recs if r['psd_dev'] is not None),
            max([r['out_dev'] for r in recs if r['out_dev'] is not None], default=None))


def class_of(count):
    return '-' if count < 0 else '0' if count == 0 else '+'


def borderline(rec, psd_bound):
    """Bins of a block whose P is within the PSD bound (the metric's bound turned back into an
    absolute error at bin k) of the reference's threshold: float32 may put them on either side."""
    P = rec['P']
    if rec['psd_dev'] is None:              # (an all-zero block: P and the threshold are exactly 0)
        return np.zeros(L, dtype=bool)
    return np.abs(P - rec['thr']) <= psd_bound * np.sqrt(P * P.mean())
