"""Float64 numpy restatement of the prompt correlate-and-dump of tracking (trk_span_kernel,
trk_span8_kernel, trk_stream_kernel with trk_partial_reduce_kernel, and the window part of the
epilogue; decodeData of the reference, gpslib.py:1400-1420), shared by test_dump_ref.py (CPU) and
test_gpu_trk_dumps.py (GPU).  Written from include/gpsmi.h and the header comments of
csrc/gpsmi_trk_stream.h and csrc/gpsmi_trk_span.h; nothing of the oracle's float32 path is used.

For one block x (complex64 [N_CYC * CS], or the recorder's uint16 decoded by the unpack formula),
one state row (prn, freq, omega0, phase, nps, prev_sum_re / im) and the job's delay_used d, with
fs = 1000 * CS:
    om      = omega0 if it is non-zero, else float32(float32(2 pi) * freq): the float32 the kernels
              wipe off with -- an input of the operation, not an error of it
    y[k]    = roll(GPSCacode(prn, CS), d)[k mod CS] x[k] exp(-j (phase + om (k + 1) / fs))
    ends    : n1 = nps + d, or CS if that is 0; then + CS while n1 <= N_CYC CS + nps -- the window
              ends, counted from the start of the carry (nps samples in front of the block)
    dump[0] = (prev_sum + sum y[0 : n1 - nps]) / n1        prev_sum = 0 where nps = 0: no carry
    dump[i] = sum y[ends[i-1] - nps : ends[i] - nps] / CS
    tail    = sum y[ends[-1] - nps :], the next prev_sum;  next nps = N_CYC CS + nps - ends[-1]
    first_len = ends[0]
everything in float64 / complex128 with exact k."""
import numpy as np

import corr_ref as cr

MAX_DUMPS = 33

DUMP_DTYPE = np.dtype([
    ('n_dumps', np.int32), ('first_len', np.int32), ('nps', np.int32),
    ('dumps', np.complex128, (MAX_DUMPS,)),       # 0 past n_dumps
    ('carry', np.complex128),                     # the tail sum: the next prev_sum
    ('rms', np.float64)])                         # sqrt(mean |x|^2): what deviations are scaled by

_CODE = {}


def replica(prn, cs):
    """GPSCacode(prn, CS) in float64 (the replica the engine is given, before its rounding)."""
    if (prn, cs) not in _CODE:
        from gpsmi import codes
        _CODE[prn, cs] = np.asarray(codes.code_replica(int(prn), cs), np.float64)
    return _CODE[prn, cs]


def _c64(block):
    x = np.asarray(block)
    return cr.decode_u8(x) if x.dtype == np.uint16 else x


def window_ends(nps, d, cs, n_cyc):
    """decodeData's window ends, counted from the start of the carry."""
    n1 = int(nps) + int(d)
    if n1 == 0:
        n1 = cs
    ends = []
    while n1 <= n_cyc * cs + nps:
        ends.append(n1)
        n1 += cs
    return ends


def _rms(x):
    return float(np.sqrt(np.mean(np.abs(x.astype(np.complex128)) ** 2)))


def wipe(block, state, cs, n_cyc):
    """complex128 [N_CYC * CS]: x[k] exp(-j (phase + om (k + 1) / fs)), the part of y that does not
    depend on the delay."""
    x = _c64(block)
    assert x.shape == (n_cyc * cs,)
    om = float(cr.omega_f32(state['freq'], state['omega0']))
    k = np.arange(n_cyc * cs, dtype=np.float64)
    arg = float(np.float32(state['phase'])) + om * ((k + 1.0) / (1000.0 * cs))
    return x.astype(np.complex128) * np.exp(-1j * arg)


def prefix(block, state, d, cs, n_cyc, wiped=None):
    """(running sums of y, complex128 [N_CYC * CS + 1] with p[b] - p[a] = sum y[a:b]; rms of x): what
    a job's windows, and the shifted ones of the sensitivity condition, are cut from.  (The
    rounding of the running sums, some 1e-13 of a dump, is far below anything compared here.)
    wiped: the job's wipe(), where the caller has it already."""
    wiped = wipe(block, state, cs, n_cyc) if wiped is None else wiped
    y = np.tile(np.roll(replica(int(state['prn']), cs), int(d)), n_cyc) * wiped
    return np.concatenate([[0j], np.cumsum(y)]), _rms(_c64(block))


def _record(pre, state, ends, divisors, cs, n_cyc):
    """The DUMP_DTYPE record of a job's prefix() and window ends; divisors[i] divides window i."""
    run, rms = pre
    nps = int(state['nps'])
    r = np.zeros((), DUMP_DTYPE)
    prev = complex(float(state['prev_sum_re']), float(state['prev_sum_im'])) if nps > 0 else 0j
    cut = np.array([0] + [e - nps for e in ends])
    assert cut[0] <= cut[1] and (np.diff(cut[1:]) > 0).all() and cut[-1] <= n_cyc * cs, cut
    sums = np.diff(run[cut])
    sums[0] += prev
    r['dumps'][:len(ends)] = sums / np.asarray(divisors, np.float64)
    r['n_dumps'] = len(ends)
    r['first_len'] = divisors[0]
    r['nps'] = n_cyc * cs - cut[-1]
    r['carry'] = run[-1] - run[cut[-1]]
    r['rms'] = rms
    return r


def dump_ref(block, state, d, cs, n_cyc, pre=None, wiped=None):
    """One job: block, one state row (any record with prn, freq, omega0, phase, nps,
    prev_sum_re, prev_sum_im), the job's delay_used and the configuration -> DUMP_DTYPE record.
    pre / wiped: the job's prefix() / wipe(), where the caller has one already."""
    ends = window_ends(state['nps'], d, cs, n_cyc)
    pre = prefix(block, state, d, cs, n_cyc, wiped) if pre is None else pre
    return _record(pre, state, ends, [ends[0]] + [cs] * (len(ends) - 1), cs, n_cyc)


def shifted(block, state, d, cs, n_cyc, boundary, by, pre=None):
    """dump_ref with window end number `boundary` moved by `by` samples: the replica roll, every
    other end and every divisor as they were -- what a correlator gives that closes one window a
    position early or late.  (The sensitivity condition of test_dump_ref.py is its only use.)"""
    ends = window_ends(state['nps'], d, cs, n_cyc)
    divisors = [ends[0]] + [cs] * (len(ends) - 1)
    ends[boundary] += by
    pre = prefix(block, state, d, cs, n_cyc) if pre is None else pre
    return _record(pre, state, ends, divisors, cs, n_cyc)


def oracle_wipe(block, state, cs, n_cyc):
    """complex64 [N_CYC * CS]: the oracle's demod_doppler of the block (float32 carrier argument).
    FREQ is a Python float where the state carries omega0 (float32(2 pi FREQ) of the float64
    product) and a float32 where it does not, as in the oracle's own closed loop."""
    import gps_oracle as orc
    if np.float32(state['omega0']) != 0:
        freq = float(np.float64(state['omega0']) / (2 * np.pi))
        assert np.float32(2 * np.pi * freq) == np.float32(state['omega0'])
    else:
        freq = np.float32(state['freq'])
    ss = _oracle_stream(int(state['prn']), cs, n_cyc)
    wiped, _ = orc.demod_doppler(_c64(block), freq, np.float32(state['phase']), ss.p.ngps, ss.t)
    assert wiped.dtype == np.complex64
    return wiped


def oracle_record(block, state, d, cs, n_cyc, wiped=None):
    """The same record from the project's float32 oracle (oracle_wipe, then
    SatStream.decode_data), with a carry array of nps samples whose sum is prev_sum: what the tests
    measure their bounds with.  wiped: the job's oracle_wipe(), where the caller has it already."""
    wiped = oracle_wipe(block, state, cs, n_cyc) if wiped is None else wiped
    ss = _oracle_stream(int(state['prn']), cs, n_cyc)
    nps = int(state['nps'])
    carry = np.zeros(nps, np.complex128)
    if nps:
        carry[0] = complex(float(state['prev_sum_re']), float(state['prev_sum_im']))
    ss.prev_samples = carry
    ss.phase_locked = False                                # (no edge scan: it reads no dump)
    dumps = ss.decode_data(wiped, int(d))
    r = np.zeros((), DUMP_DTYPE)
    r['n_dumps'] = len(dumps)
    r['dumps'][:len(dumps)] = dumps
    n1 = nps + int(d)
    r['first_len'] = n1 if n1 else cs
    r['nps'] = len(ss.prev_samples)
    r['carry'] = np.sum(ss.prev_samples)
    r['rms'] = _rms(_c64(block))
    return r


_STREAMS = {}


def _oracle_stream(prn, cs, n_cyc):
    import gps_oracle as orc
    key = (prn, cs, n_cyc)
    if key not in _STREAMS:
        _STREAMS[key] = orc.SatStream(prn, 0.0, orc.Params(code_samples=cs, n_cyc=n_cyc))
    return _STREAMS[key]


def kernel_records(out, nxt):
    """gpsmi_trk_out records and the next-state rows of the same jobs (TrkEngine.replay and
    replay_states) as DUMP_DTYPE records (rms left 0)."""
    r = np.zeros(out.shape, DUMP_DTYPE)
    r['n_dumps'], r['first_len'], r['nps'] = out['n_dumps'], out['first_len'], out['nps']
    d = np.asarray(out['dumps'], np.float64)
    r['dumps'] = d[..., 0:2 * MAX_DUMPS:2] + 1j * d[..., 1:2 * MAX_DUMPS:2]
    r['carry'] = np.asarray(nxt['prev_sum_re'], np.float64) + 1j * np.asarray(nxt['prev_sum_im'], np.float64)
    return r


# ---- deviations of a float32 realisation (the oracle, a kernel) from the float64 records

METRICS = ('dumps', 'carry')           # the fields that get a bound
REPORTED = ('dumps', 'dump0', 'carry')
INTS = ('n_dumps', 'first_len', 'nps')


def deviations(got, ref):
    """Per job, how far `got` (DUMP_DTYPE records) is from the float64 records `ref`, as absolute
    errors over the rms of the block's samples: 'dumps' max |dump - ref| over all n_dumps dumps (and
    over the unused slots, which are 0 on both sides), 'carry' the next prev_sum, and for the reports
    'dump0', the first dump alone (the one the carry enters).  dump0 is one of the dumps and is held
    to their bound, not to one of its own: the oracle's error is that of its float32 carrier
    argument, which is next to nothing in the first samples of a block, so its deviation there says
    nothing about the rounding of a float32 window sum.  Returns a dict of float64 arrays shaped
    like ref."""
    e = np.abs(np.asarray(got['dumps']) - ref['dumps'])
    return {'dumps': np.max(e, axis=-1) / ref['rms'],
            'dump0': e[..., 0] / ref['rms'],
            'carry': np.abs(np.asarray(got['carry']) - ref['carry']) / ref['rms']}
