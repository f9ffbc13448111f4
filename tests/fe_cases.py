"""The pinned cases of the front-end stage (csrc/gpsmi_fe.hip) beside the named configurations A-F of
tests/fe_ref.py: small shapes at atten_db 20, where the outer taps carry 2-4 % of the largest one, every
class of the planner (workgroups of 256, 128 and 64 outputs, LDS below and above 64 KiB), every
format and flag, both sidebands, an IF beyond fs_in and ratios whose phase row advances irregularly.
The case table, the input builders, the planner's workgroup rule restated, the error bound of one
output and the call cuts of tests/test_frontend_cases.py (CPU) and tests/test_gpu_frontend_cases.py
(GPU).  numpy only."""
import numpy as np

import fe_ref

FS_OUT = 2_048_000
LDS_BUDGET = 64 * 1024          # preferred dynamic LDS of a workgroup
LDS_MAX = 160 * 1024            # LDS of one CU: workgroups of 64 outputs may take it

# name -> configuration (fe_ref's keys, plus conjugate and atten_db) and the class the case is there
# for: R outputs per workgroup, LDS above 64 KiB or not, outer: the least share of the largest tap that
# the first and the last tap must reach (None: the case is not about them)
CASES = {
    'lo': dict(fmt='c64', fs_in=4_000_000, if_hz=0.0, conjugate=False, passband_hz=None, atten_db=20.0,
               R=256, lds_hi=False, outer=0.01),
    'conj': dict(fmt='c64', fs_in=4_000_000, if_hz=-312_500.0, conjugate=True, passband_hz=None, atten_db=20.0,
                 R=256, lds_hi=False, outer=0.01),
    'wrap': dict(fmt='sc16', fs_in=4_000_000, if_hz=4_312_500.0, conjugate=False, passband_hz=None,
                 atten_db=20.0, R=256, lds_hi=False, outer=0.01),
    'near1': dict(fmt='sc16', fs_in=2_047_999, if_hz=-300_000.0, conjugate=False, passband_hz=None,
                  atten_db=20.0, R=256, lds_hi=False, outer=None),
    'odd': dict(fmt='sc8', fs_in=5_000_011, if_hz=1_234_567.0, conjugate=False, passband_hz=None,
                atten_db=20.0, R=256, lds_hi=False, outer=0.01),
    # (beside the eleven cases above and below: `odd` as complex64 at IF 0, the one unit-impulse case whose
    # outputs fall between two phase rows, mu != 0; with Q = 64 or 1 dividing r L the others read one row)
    'oddc': dict(fmt='c64', fs_in=5_000_011, if_hz=0.0, conjugate=False, passband_hz=None, atten_db=20.0,
                 R=256, lds_hi=False, outer=0.01),
    'up': dict(fmt='u8iq', fs_in=1_100_000, if_hz=0.0, conjugate=False, passband_hz=None, atten_db=20.0,
               R=256, lds_hi=False, outer=None),
    'negif': dict(fmt='r8', fs_in=16_368_000, if_hz=-4_092_000.0, conjugate=False, passband_hz=None,
                  atten_db=20.0, R=256, lds_hi=False, outer=0.01),
    'r128': dict(fmt='sc8', fs_in=60_000_000, if_hz=0.0, conjugate=False, passband_hz=None, atten_db=20.0,
                 R=128, lds_hi=False, outer=None),
    'r64': dict(fmt='c64', fs_in=131_072_000, if_hz=0.0, conjugate=False, passband_hz=None, atten_db=20.0,
                R=64, lds_hi=False, outer=None),
    'lds_hi': dict(fmt='c64', fs_in=4_000_000, if_hz=0.0, conjugate=False, passband_hz=1_015_000.0,
                   atten_db=20.0, R=64, lds_hi=True, outer=None),
    'lds_hi60': dict(fmt='c64', fs_in=4_000_000, if_hz=0.0, conjugate=False, passband_hz=1_000_000.0,
                     atten_db=60.0, R=64, lds_hi=True, outer=None),
}
for _c in CASES.values():
    _c['fs_out'] = FS_OUT

# the configuration the planner must refuse: no workgroup size fits the LDS of one CU
REFUSED = dict(fmt='c64', fs_in=2_048_000, if_hz=0.0, conjugate=False, passband_hz=1_000_000.0, atten_db=120.0,
               fs_out=FS_OUT)

IMPULSE_CASES = ('lo', 'oddc', 'r64', 'lds_hi', 'lds_hi60')          # c64 at IF 0: a 1.0 passes the mix exactly


def plan_shape(K, L, P, Q):
    """The end of fe_plan: (outputs per workgroup, dynamic LDS bytes), None where nothing fits.  The
    table [(L + 1) K] float32 padded to an even count, then the input span of R consecutive outputs,
    (R - 1) P // Q + 1 + K complex64; the largest of R = 256, 128, 64 within 64 KiB, R = 64 within
    160 KiB.  The library exposes neither R nor the LDS bytes: keep this in step with the loop over R at
    the end of fe_plan (csrc/gpsmi_fe.hip), or the cases drift out of their classes unnoticed."""
    tab_floats = ((L + 1) * K + 1) & ~1
    for r in (256, 128, 64):
        lds = 4 * tab_floats + 8 * ((r - 1) * P // Q + 1 + K)
        if lds <= LDS_BUDGET or (r == 64 and lds <= LDS_MAX):
            return r, lds
    return None


def bound(x_mixed, K, L, T, P, Q, n0, n1):
    """Per-output bound on |float32 kernel - float64 restatement| for outputs n0 .. n1 - 1:
    B_n = (K + 16) 2^-24 sum_m max(|T[j, m]|, |T[j + 1, m]|) |x_m| over the indices of fe_ref.resample.
    K 2^-24 sum |h| |x| is the running-sum bound of one thread's ascending float32 sum of K products;
    the 16 covers the float32 sincospif, the three roundings of the complex mix, the rounding of mu and
    the three roundings of a0 + mu (a1 - a0)."""
    A = np.abs(np.asarray(T, dtype=np.float64))
    A = np.maximum(A[:-1], A[1:])                       # row j: max(|T[j]|, |T[j + 1]|)
    xa = np.concatenate([np.zeros(K), np.abs(x_mixed), np.zeros(K)])
    n = np.arange(n0, n1, dtype=np.int64)
    num = n * P
    I, r = num // Q, num % Q
    j = (r * L) // Q
    idx = (I - K // 2 + 1)[:, None] + np.arange(K)[None, :] + K
    return (K + 16) * 2.0 ** -24 * np.einsum('nk,nk->n', xa[idx], A[j])


def ratio(c):
    return fe_ref.ratio(c['fs_in'], c['fs_out'])


def samples(c, x):
    """Input samples held by the stored array x (sc8 / sc16: two values a sample)."""
    return len(x) // (2 if c['fmt'] in ('sc8', 'sc16') else 1)


def cut(c, x, a, b):
    """Samples a .. b - 1 of the stored array x."""
    per = 2 if c['fmt'] in ('sc8', 'sc16') else 1
    return x[a * per:b * per]


def n_input(K, P, Q, R):
    """The smallest input that completes 3 R + 5 outputs and K samples past them."""
    return -(-(3 * R + 5) * P // Q) + K


def noise_input(name, K, R):
    """Seeded Gaussian at 0.25 of full scale in the case's format (real for r8), n_input samples."""
    c = CASES[name]
    P, Q = ratio(c)
    n = n_input(K, P, Q, R)
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return fe_ref.add_quantise(x, c['fmt'], 0.25)


def impulse_positions(K, P, Q, R):
    """Input indices of the unit impulse: the first sample, either side of the centre tap of output 0,
    and the sample under the middle output of the second workgroup."""
    return [0, K // 2 - 1, K // 2, (R + R // 2) * P // Q]


def impulse_expected(K, L, T, P, Q, i0, n_out):
    """Outputs 0 .. n_out - 1 for a 1.0 at input index i0 and zeros elsewhere, straight from (n, i0):
    T[j, m] + mu (T[j + 1, m] - T[j, m]) with m = i0 - floor(n P / Q) + K/2 - 1 (tap m weighs input
    floor(t_n) - K/2 + 1 + m), 0 outside 0 <= m < K (float64; hit: the outputs whose support holds the
    impulse)."""
    T = np.asarray(T, dtype=np.float64)
    out = np.zeros(n_out)
    hit = np.zeros(n_out, dtype=bool)
    for n in range(n_out):
        I, r = divmod(n * P, Q)
        m = i0 - I + K // 2 - 1
        if 0 <= m < K:
            j, rem = divmod(r * L, Q)
            mu = rem / Q
            out[n] = T[j, m] + mu * (T[j + 1, m] - T[j, m])
            hit[n] = True
    return out, hit


def _advance(K, P, Q, taken, emitted, want):
    """The fewest further input samples after which at least `want` more outputs are complete."""
    m = 0
    while fe_ref.complete(K, P, Q, taken + m) - emitted < want:
        m += 1
    return m


def cuts_by_outputs(K, P, Q, R, n_in):
    """Call lengths over n_in samples among which successive calls emit exactly 0, 1, R - 1, R, R + 1
    outputs, then the rest -> (lengths, outputs of each call, positions of those five calls in the
    lists).  Where one input sample can complete two outputs (P < Q) a wanted number may be out of reach
    from where the stream stands; one-sample calls are put in front of that call until it is in reach."""
    lens, outs, at, taken, emitted = [K // 2], [0], [0], K // 2, 0
    assert fe_ref.complete(K, P, Q, taken) == 0
    for want in (1, R - 1, R, R + 1):
        while True:
            m = _advance(K, P, Q, taken, emitted, want)
            e = fe_ref.complete(K, P, Q, taken + m) - emitted
            hit = e == want
            if hit:
                at.append(len(lens))
            else:                                       # (out of reach: move on by one sample)
                assert P < Q
                m, e = 1, fe_ref.complete(K, P, Q, taken + 1) - emitted
            lens.append(m)
            outs.append(e)
            taken, emitted = taken + m, emitted + e
            if hit:
                break
    assert taken < n_in and len(at) == 5
    lens.append(n_in - taken)
    outs.append(fe_ref.complete(K, P, Q, n_in) - emitted)
    return lens, outs, at


def cuts_by_length(K, n_in):
    """A zero-length call, one call shorter than the filter, forty one-sample calls, a zero-length call
    in mid-stream, the rest."""
    lens = [0, K - 1] + [1] * 40 + [0]
    assert sum(lens) < n_in
    return lens + [n_in - sum(lens)]
