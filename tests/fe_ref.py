"""float64 numpy restatement of the front-end stage (csrc/gpsmi_fe.hip, gpsmi.h gpsmi_fe_*): decode,
mix with the integer phase, and resample with the tap table gpsmi_fe_design returns.  numpy only."""
import numpy as np

FMT = {'c64': 0, 'u8iq': 1, 'sc8': 2, 'sc16': 3, 'r8': 4}

# the named configurations of the tests: format, fs_in, IF / offset, fs_out, passband (None: default)
CONFIGS = {
    'A': dict(fmt='sc16', fs_in=4_000_000, if_hz=0.0, fs_out=2_048_000, passband_hz=None),
    'B': dict(fmt='r8', fs_in=16_368_000, if_hz=4_092_000.0, fs_out=2_048_000, passband_hz=None),
    'C': dict(fmt='r8', fs_in=38_192_000, if_hz=9_548_000.0, fs_out=2_048_000, passband_hz=None),
    'D': dict(fmt='sc8', fs_in=2_500_000, if_hz=25_000.0, fs_out=2_048_000, passband_hz=None),
    'E': dict(fmt='u8iq', fs_in=2_000_000, if_hz=0.0, fs_out=2_048_000, passband_hz=None),
    'F': dict(fmt='r8', fs_in=16_368_000, if_hz=4_092_000.0, fs_out=16_368_000, passband_hz=3_000_000.0),
}


def passband(c):
    return c['passband_hz'] or 0.44 * min(c['fs_in'], c['fs_out'])


def stop_edge(c):
    """The nearest frequency from which anything aliases (or, real input, images) into |f| <= p."""
    fi, p = c['fs_in'], passband(c)
    s = min(fi, c['fs_out']) - p
    if c['fmt'] == 'r8':
        ifr = c['if_hz'] - fi * np.floor(c['if_hz'] / fi + 0.5)
        s = min(s, abs(ifr), 0.5 * fi - abs(ifr))
    return s


def ratio(fs_in, fs_out):
    g = np.gcd(int(fs_in), int(fs_out))
    return int(fs_in) // g, int(fs_out) // g


def decode(x, fmt):
    """Input samples -> complex128 of full scale 1 (real input times 2)."""
    x = np.asarray(x)
    if fmt == 'c64':
        return x.astype(np.complex128)
    if fmt == 'u8iq':
        im, re = np.divmod(x, 256)
        c64 = np.asarray(re + 1j * im, dtype=np.complex64) / 127.5 - (1 + 1j)      # synth.raw_to_c64
        return c64.astype(np.complex128)
    if fmt == 'sc8':
        v = x.reshape(-1, 2).astype(np.float64) / 128.0
        return v[:, 0] + 1j * v[:, 1]
    if fmt == 'sc16':
        v = x.reshape(-1, 2).astype(np.float64) / 32768.0
        return v[:, 0] + 1j * v[:, 1]
    if fmt == 'r8':
        return 2.0 * x.astype(np.float64) / 128.0 + 0j
    raise ValueError(fmt)


def phase_inc(if_hz, fs_in):
    f = if_hz / float(fs_in)
    f -= np.floor(f)
    inc = int(np.ldexp(f, 64))
    return 0 if inc >= 1 << 64 else inc


def mix(x, if_hz, fs_in, i0=0, conjugate=False):
    """x[k] exp(-j 2 pi if_hz (i0 + k) / fs_in) with the stage's phase: top 24 bits of (i inc mod 2^64)."""
    if conjugate:
        x = np.conj(x)
    inc = np.uint64(phase_inc(if_hz, fs_in))
    i = np.arange(len(x), dtype=np.uint64) + np.uint64(i0)
    with np.errstate(over='ignore'):
        ph = i * inc
    top = (ph.view(np.int64) >> np.int64(40)).astype(np.float64) * 2.0 ** -23
    return x * np.exp(-1j * np.pi * top)


def resample(xm, K, L, table, P, Q, n0, n1, chunk=2048):
    """Outputs n0 .. n1 - 1 from the mixed input xm (sample 0 = index 0; zeros outside)."""
    T = np.asarray(table, dtype=np.float64)
    out = np.empty(n1 - n0, dtype=np.complex128)
    pad = K
    xp = np.concatenate([np.zeros(pad, np.complex128), xm, np.zeros(pad, np.complex128)])
    m = np.arange(K)
    for a in range(n0, n1, chunk):
        n = np.arange(a, min(a + chunk, n1), dtype=np.int64)
        num = n * P
        I, r = num // Q, num % Q
        rl = r * L
        j, mu = rl // Q, (rl % Q).astype(np.float64) / Q
        idx = (I - K // 2 + 1)[:, None] + m[None, :] + pad
        xs = xp[idx]
        a0 = np.einsum('nk,nk->n', xs, T[j])
        a1 = np.einsum('nk,nk->n', xs, T[j + 1])
        out[a - n0:a - n0 + len(n)] = a0 + mu * (a1 - a0)
    return out


def complete(K, P, Q, total):
    """Outputs whose support is in once `total` input samples are: n with floor(n P / Q) + K/2 <= total - 1."""
    M = total - 1 - K // 2
    if M < 0:
        return 0
    return -(-((M + 1) * Q) // P)


def run(x, c, K, L, table, n_out=None):
    """The stage over a whole input (its complete outputs, or the first n_out)."""
    P, Q = ratio(c['fs_in'], c['fs_out'])
    xm = mix(decode(x, c['fmt']), c['if_hz'], c['fs_in'], 0, c.get('conjugate', False))
    n = complete(K, P, Q, len(xm)) if n_out is None else n_out
    return resample(xm, K, L, table, P, Q, 0, n)


def response(table, K, L, fs_in, f_hz):
    """Frequency response of the interpolated prototype (the piecewise-linear h on the 1/L grid) at
    f_hz: y_n = sum_i x_i h(t_n - i), so a tone e^{j 2 pi f i / fs_in} leaves as H(f) e^{j 2 pi f t_n}
    plus images at f + k fs_in weighted H(f + k fs_in)."""
    T = np.asarray(table, dtype=np.float64)
    # grid sample q / L (q = j + L (K/2 - 1 - m)) from rows j = 0 .. L - 1
    j, m = np.meshgrid(np.arange(L), np.arange(K), indexing='ij')
    q = (j + L * (K // 2 - 1 - m)).ravel()
    g = T[:L].ravel()
    u = np.asarray(f_hz, dtype=np.float64) / (L * fs_in)          # cycles per grid step
    out = np.empty(u.shape, dtype=np.complex128)
    for a in range(0, u.size, 256):
        uu = u.ravel()[a:a + 256]
        out.ravel()[a:a + 256] = (np.exp(-2j * np.pi * np.outer(uu, q)) @ g) / L * np.sinc(uu) ** 2
    return out


def add_quantise(x, fmt, scale):
    """complex128 (or real, for r8) signal -> the stored samples of `fmt` at `scale` of full scale."""
    if fmt == 'r8':
        return np.clip(np.rint(x.real * scale * 128.0), -127, 127).astype(np.int8)
    if fmt == 'sc8':
        v = np.stack([x.real, x.imag], -1) * scale * 128.0
        return np.clip(np.rint(v), -127, 127).astype(np.int8).ravel()
    if fmt == 'sc16':
        v = np.stack([x.real, x.imag], -1) * scale * 32768.0
        return np.clip(np.rint(v), -32767, 32767).astype(np.int16).ravel()
    if fmt == 'u8iq':
        i = np.clip(np.rint((x.real * scale + 1.0) * 127.5), 0, 255).astype(np.uint16)
        q = np.clip(np.rint((x.imag * scale + 1.0) * 127.5), 0, 255).astype(np.uint16)
        return (q << 8) | i
    if fmt == 'c64':
        return (x * scale).astype(np.complex64)
    raise ValueError(fmt)
