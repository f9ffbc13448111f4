"""The pinned cases of the pulse blanking (csrc/gpsmi_pb.hip) beside the workload's own blocks: block
lengths whose word count is no multiple of four and whose last slice is partial, guards from 0 to the
limit of 1024 with detections placed where the guard comparison, the words, the slices and the block
end decide, and sample powers the radix select has not seen from noise (a few ulp apart, two
values, ties at the rank, NaN / Inf, subnormals).  Builders, an independent brute-force restatement
of the contract in tests/pb_ref.py's docstring, and the case matrix of tests/test_blanking_cases.py
(CPU) and tests/test_gpu_blanking_cases.py (GPU).  numpy only."""
import numpy as np

import ifx_ref

# block length -> (words, what it is there for)
LENGTHS = {
    2048: (64, 'the minimum: one slice, shorter than the large slice'),
    2080: (65, 'words % 4 = 1: one full small slice and one word'),
    4128: (129, 'the last small slice is one word long'),
    10272: (321, 'two large slices, the second partial; six small slices'),
}
GUARDS = [(0, 0), (1, 0), (0, 1), (31, 33), (32, 32), (1024, 0), (0, 1024), (1024, 1024)]
# a middle large slice with a full halo on both sides: 256 + 2 * 32 detection words, all the kernel holds
WIDE_N, WIDE_GUARD = 3 * 8192 + 32, (1024, 1024)
GEOMETRY = [(n, g) for n in LENGTHS for g in GUARDS] + [(WIDE_N, WIDE_GUARD)]
GEO_THRESH_DB, GEO_MAX_FRAC = 10.0, 1.0                # (max_frac 1: the large guards never pass through)
SIGMA_U8 = 0.03                                         # under 4 LSB: a few dozen distinct powers, ties at the rank


# ---- floors ------------------------------------------------------------------------------------

def unit(n, seed):
    """exp(j phi), seeded phi, as complex64: float32 powers within a few ulp of 1 (at most two values
    of the top 21 bits), so the last pass of the select decides."""
    phi = np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, n)
    return np.exp(1j * phi).astype(np.complex64)


def gauss(n, seed, sigma=1.0):
    rng = np.random.default_rng(seed)
    return (sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)).astype(np.complex64)


def u8(n, seed):
    """The recorder's uint16 (Q << 8 | I) of Gaussian noise: at most 2^16 distinct samples, many ties."""
    rng = np.random.default_rng(seed)
    return ifx_ref.quantise(SIGMA_U8 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)))


def plant(x, positions, amp=40):
    """A copy of x with single-sample spikes (complex64: the value amp; uint16: amp is the raw word)."""
    y = np.array(x, copy=True)
    for p in positions:
        y[p] = amp
    return y


# ---- the contract, by brute force --------------------------------------------------------------

def brute(x, thresh_db, pre, post, max_frac, carry):
    """One block of the contract with explicit loops over the detections, a sort for the lower median
    and no cumulative sums -> (y complex64, count, floor float32, blank bool [n], carry out)."""
    x = np.asarray(x, dtype=np.complex64)
    n = len(x)
    re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        p = (re * re).astype(np.float32) + (im * im).astype(np.float32)
        m = np.sort(p)[(n - 1) // 2]                    # (NaN sorts last, above +inf)
        f = np.float32(10.0 ** (float(np.float32(thresh_db)) / 10.0))
        T = np.float32(np.float32(m) * f)
        det = [j for j in range(n) if p[j] > T]
    blank = np.zeros(n, dtype=bool)
    blank[:min(carry, n)] = True
    out_carry = 0
    for j in det:                                       # i - post <= j <= i + pre
        blank[max(0, j - pre):min(n, j + post + 1)] = True
        out_carry = max(out_carry, j + post - n + 1)
    count = int(np.count_nonzero(blank))
    if count > int(np.floor(float(np.float32(max_frac)) * n)):
        return x.copy(), -1, m, np.zeros(n, dtype=bool), out_carry
    y = x.copy()
    y[blank] = 0
    return y, count, m, blank, out_carry


def brute_run(blocks, thresh_db, pre, post, max_frac, carry=0):
    """Consecutive blocks -> what BlankerRef.run returns (masks as bool [nb, n]) and the last carry."""
    ys, cs, fs, bs = [], [], [], []
    for x in blocks:
        y, c, m, b, carry = brute(x, thresh_db, pre, post, max_frac, carry)
        ys.append(y)
        cs.append(c)
        fs.append(m)
        bs.append(b)
    return np.stack(ys), np.array(cs, dtype=np.int32), np.array(fs, dtype=np.float32), np.stack(bs), carry


# ---- geometry ----------------------------------------------------------------------------------

PAIR_AT = 5             # first spike of the spaced pairs (odd: not on a word or slice boundary)


def position_sets(n, pre, post):
    """[(label, spikes of a block, follow)]: one block each; follow: a clean block comes after it.
    Sets that do not fit the block are left out."""
    sets = [('first', [0], False), ('words', [31, 32], False)]
    for a in (2047, 8191):                              # the last / first sample of a small / large slice
        if a + 1 < n:
            sets.append((f'slice{a + 1}', [a, a + 1], False))
    # spikes d apart leave max(0, d - pre - post - 1) samples between them untouched: pre + post and
    # pre + post + 1 leave none, pre + post + 2 is the first to leave one
    for d in (pre + post, pre + post + 1, pre + post + 2):
        if PAIR_AT + d < n:
            sets.append((f'pair{d - pre - post}', sorted({PAIR_AT, PAIR_AT + d}), False))
    if post > 0:
        sets.append(('carry1', [n - post], True))       # reaches one sample into the next block
        sets.append(('carry0', [n - post - 1], True))   # ends with the block
    sets.append(('last', [n - 1], True))                # carry = post
    return sets


def geometry_blocks(n, pre, post):
    """The blocks of one (n, guards): every position set on a unit floor, a clean unit block behind
    the sets that look at the carry, padded with clean blocks to whole triples and so that a block
    with a follow-up is never the last of its triple: the triples run as calls of their own, and a
    carry must not end with the call that made it -> (blocks complex64 [3 k, n], planted: the spike
    list of every block, labels)."""
    blocks, planted, labels = [], [], []
    for i, (label, spikes, follow) in enumerate(position_sets(n, pre, post)):
        if follow and len(blocks) % 3 == 2:             # (a block and its follow-up stay in one triple)
            blocks.append(unit(n, 3000 + len(blocks)))
            planted.append([])
            labels.append('pad')
        blocks.append(plant(unit(n, 1000 + i), spikes))
        planted.append(list(spikes))
        labels.append(label)
        if follow:
            blocks.append(unit(n, 2000 + i))
            planted.append([])
            labels.append(label + '+clean')
    while len(blocks) % 3:
        blocks.append(unit(n, 3000 + len(blocks)))
        planted.append([])
        labels.append('pad')
    return np.stack(blocks), planted, labels


def carries_of(labels, post):
    """[(index in the triple, carry)] of the blocks of a triple whose carry the next block must show."""
    want = {'carry1': 1, 'carry0': 0, 'last': post}
    return [(i, want[label]) for i, label in enumerate(labels) if label in want]


def spread16(triple, seed):
    """A 16-block call with the three blocks at positions 0, 7 and 15 and seeded unit blocks between
    (a carry out of position 0 or 7 lands in the clean block behind it)."""
    n = triple.shape[1]
    out = np.stack([unit(n, seed + b) for b in range(16)])
    for b, x in zip((0, 7, 15), triple):
        out[b] = x
    return out


# ---- raw input ---------------------------------------------------------------------------------

RAW_LENGTHS = (2080, 10272)
RAW_GUARDS = [(31, 33), (1024, 1024)]
RAW_TIE_GUARDS = [(0, 0)] + RAW_GUARDS                  # (0, 0): the mask is the detections themselves


def raw_blocks(n, spiked):
    """Three uint16 blocks of quantised noise; spiked: 0xFFFF samples (power 2) planted at the block
    ends, a word boundary and mid-block."""
    blocks = []
    for b in range(3):
        x = u8(n, 50 + b)
        if spiked:
            x = plant(x, [[0, 31, 32, n // 2 + 7], [n - 1], [2047, 2048, n - 34]][b], 0xFFFF)
        blocks.append(x)
    return np.stack(blocks)


# ---- select ------------------------------------------------------------------------------------

SELECT_N = 2080
SELECT_THRESH_DB = (13.0, 3.0)                          # (3 dB: a quarter of a Gaussian block is detected)
SELECT_GUARD = (3, 5)
SELECT_LABELS = ('unit', 'gauss', 'two values', 'nan and inf', 'subnormal')


def two_values(n, seed, lo=0.5, hi=1.0):
    """Exactly two powers, (n - 1) // 2 + 1 samples of the lower: the lower median is the last element
    of the lower group."""
    k = (n - 1) // 2 + 1
    x = np.full(n, hi, dtype=np.complex64)
    x[np.random.default_rng(seed).permutation(n)[:k]] = lo
    return x


def nonfinite(n, seed):
    """Gaussian with three NaN, one +Inf and one -Inf component: the floor stays finite."""
    x = gauss(n, seed).copy()
    v = x.view(np.float32)
    v[2 * 3] = np.nan
    v[2 * 1000 + 1] = np.nan
    v[2 * (n - 1)] = np.nan
    v[2 * 64 + 1] = np.inf
    v[2 * 1500] = -np.inf
    return x


def select_blocks():
    n = SELECT_N
    sub = (gauss(n, 14).astype(np.complex128) * 2.0 ** -70).astype(np.complex64)
    return np.stack([unit(n, 11), gauss(n, 12), two_values(n, 13), nonfinite(n, 15), sub])


# ---- carry out of a block that passed through ---------------------------------------------------

CARRY = dict(n=2048, thresh_db=10.0, pre=0, post=1024, max_frac=0.5)


def carry_blocks():
    """Block 0: spikes at 0, 1025 and n - 1 blank all of it under post 1024: over the limit, it passes
    through, and its last spike still reaches 1024 samples into the clean block 1."""
    n = CARRY['n']
    return np.stack([plant(unit(n, 21), [0, 1025, n - 1]), unit(n, 22)])


# ---- chunking ----------------------------------------------------------------------------------

CHUNK = dict(n=10272, thresh_db=10.0, pre=1024, post=1024, max_frac=1.0, nb=16)


def chunk_blocks():
    n = CHUNK['n']
    return np.stack([plant(unit(n, 30 + b), [n - 1]) for b in range(CHUNK['nb'])])
