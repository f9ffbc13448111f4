"""float64 restatement of the per-satellite beams (gpsmi_nul_beams*, include/gpsmi.h): the contract
the kernels of csrc/gpsmi_nul_beam.h are held to, every operation in the header's order, on top of
nul_ref's covariance, Cholesky arithmetic and combine; `plain`, the same formulas as one would write
them in numpy (w = R^-1 G (G^H R^-1 G)^-1 e0), the yardstick of the tolerances; and `gram_pivots`,
the dependence check of the argument errors.
"""
import numpy as np

import nul_ref as R
from nul_ref import _conj, _div, _mul, _sub, f32


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1])


def _abs2(a):
    return a[0] * a[0] + a[1] * a[1]


def _c(v):
    return (float(v.real), float(v.imag))


def cholesky(Rm, m):
    """Lower triangle Rm[i][j] (tuples) -> (L, ok), column by column as the header states it."""
    L = [[None] * m for _ in range(m)]
    ok = True
    with np.errstate(all='ignore'):
        for j in range(m):
            d = Rm[j][j][0]
            for k in range(j):
                d -= L[j][k][0] * L[j][k][0] + L[j][k][1] * L[j][k][1]
            if not (d > 0.0) or not (d < np.inf):
                ok = False
            l = float(np.sqrt(np.float64(d)))
            L[j][j] = (l, 0.0)
            for i in range(j + 1, m):
                v = Rm[i][j]
                for k in range(j):
                    v = _sub(v, _mul(L[i][k], _conj(L[j][k])))
                L[i][j] = _div(v, l)
    return L, ok


def solve_e0(K, m):
    """K K^H q = e0: forward, then backward, as nul_ref.solve does for R u = e0."""
    y, q = [None] * m, [None] * m
    y[0] = (1.0 / K[0][0][0], 0.0)
    for i in range(1, m):
        v = (0.0, 0.0)
        for k in range(i):
            v = _sub(v, _mul(K[i][k], y[k]))
        y[i] = _div(v, K[i][i][0])
    for i in range(m - 1, -1, -1):
        v = y[i]
        for k in range(i + 1, m):
            v = _sub(v, _mul(_conj(K[k][i]), q[k]))
        q[i] = _div(v, K[i][i][0])
    return q


def factor(C, n, load=0.0):
    """C [A][A] of a block of n samples -> (L, flag, tr): R = C / n + delta I = L L^H; L = I and
    flag 0 when a pivot is not positive and finite."""
    A = C.shape[0]
    load = f32(1e-6) if f32(load) == 0.0 else f32(load)
    dn = float(n)
    Rm = [[(float(C[a, b].real) / dn, 0.0 if a == b else float(C[a, b].imag) / dn) for b in range(a + 1)]
          for a in range(A)]
    tr = 0.0
    for a in range(A):
        tr += Rm[a][a][0]
    delta = load * tr / float(A)
    for a in range(A):
        Rm[a][a] = (Rm[a][a][0] + delta, 0.0)
    L, ok = cholesky(Rm, A)
    if not ok:
        L = [[(1.0 if i == j else 0.0, 0.0) for j in range(A)] for i in range(A)]
    return L, int(ok), tr


def column(L, g):
    """z = L^-1 g, forward."""
    A = len(g)
    z = [None] * A
    for i in range(A):
        v = _c(g[i])
        for k in range(i):
            v = _sub(v, _mul(L[i][k], z[k]))
        z[i] = _div(v, L[i][i][0])
    return z


def beam(L, flag, tr, s, us):
    """One beam of a factored block: steering vector s, its null vectors us (in ascending q) ->
    (w complex128 [A], flag, gain_db float32)."""
    A = len(s)
    Z = [column(L, s)] + [column(L, u) for u in us]
    m = len(Z)
    M = [[None] * m for _ in range(m)]
    for i in range(m):
        for j in range(i + 1):
            if i == j:
                acc = 0.0
                for a in range(A):
                    acc += _abs2(Z[i][a])
                M[i][i] = (acc, 0.0)
            else:
                acc = (0.0, 0.0)
                for a in range(A):
                    acc = _add(acc, _mul(_conj(Z[i][a]), Z[j][a]))
                M[i][j] = acc
    K, ok = cholesky(M, m)
    if not ok:
        return np.zeros(A, dtype=np.complex128), -1, np.float32(0.0)
    with np.errstate(all='ignore'):
        q = solve_e0(K, m)
        t = []
        for a in range(A):
            acc = (0.0, 0.0)
            for j in range(m):
                acc = _add(acc, _mul(Z[j][a], q[j]))
            t.append(acc)
        w = [None] * A
        for i in range(A - 1, -1, -1):
            v = t[i]
            for k in range(i + 1, A):
                v = _sub(v, _mul(_conj(L[k][i]), w[k]))
            w[i] = _div(v, L[i][i][0])
        s2 = 0.0
        for a in range(A):
            s2 += _abs2(_c(s[a]))
        gdb = np.float32(10.0 * np.log10(np.float64(tr) / np.float64(s2 * q[0][0])))
    return np.array([complex(*v) for v in w]), flag, gdb


def _columns(steer, nulls, mask, b):
    nulls = np.zeros((0, steer.shape[1])) if nulls is None else nulls
    return [nulls[q] for q in range(len(nulls)) if mask is not None and (int(mask[b]) >> q) & 1]


class BeamRef:
    def __init__(self, n, antennas, load=0.0):
        self.n, self.A, self.load = n, antennas, load

    def weights(self, x, steer, nulls=None, mask=None):
        """One block (complex64 [A][n]) -> (w complex128 [B][A], flags int32 [B], gain_db float32 [B])."""
        steer = np.asarray(steer, dtype=np.complex128)
        L, flag, tr = factor(R.covariance(x), self.n, self.load)
        res = [beam(L, flag, tr, steer[b], _columns(steer, nulls, mask, b)) for b in range(len(steer))]
        return (np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.int32),
                np.array([r[2] for r in res], dtype=np.float32))

    def run(self, x, steer, nulls=None, mask=None):
        """[A][nb * n] complex64 (or uint16: decoded first) -> (y [B][nb][n], flags [nb][B], gain_db
        [nb][B], weights complex128 [nb][B][A])."""
        x = np.asarray(x)
        if x.dtype == np.uint16:
            x = R.decode(x)
        x = x.reshape(self.A, -1, self.n)
        nb, B = x.shape[1], len(steer)
        y = np.zeros((B, nb, self.n), dtype=np.complex64)
        ws, fs, gs = [], [], []
        for b in range(nb):
            w, f, g = self.weights(x[:, b], steer, nulls, mask)
            for k in range(B):
                if f[k] >= 0:
                    y[k, b] = R.combine(x[:, b], w[k])
            ws.append(w), fs.append(f), gs.append(g)
        return y, np.stack(fs), np.stack(gs), np.stack(ws)


def plain(x, n, steer, nulls=None, mask=None, load=0.0):
    """The header's formulas in idiomatic numpy, no order kept.  One block [A][n] -> (y [B][n], flags,
    gain_db, w [B][A]).  Its distance from BeamRef is what float64 and float32 leave open."""
    x = np.asarray(x, dtype=np.complex64)
    steer = np.asarray(steer, dtype=np.complex128)
    A, B = x.shape[0], len(steer)
    load = f32(1e-6) if f32(load) == 0.0 else f32(load)
    X = x.astype(np.complex128)
    C = X @ X.conj().T / n
    tr = np.trace(C).real
    Rm = C + load * tr / A * np.eye(A)
    flag = 1
    with np.errstate(all='ignore'):
        try:
            np.linalg.cholesky(Rm)
        except np.linalg.LinAlgError:
            Rm, flag = np.eye(A, dtype=np.complex128), 0
        ys, fs, gs, ws = [], [], [], []
        for b in range(B):
            G = np.stack([steer[b]] + _columns(steer, nulls, mask, b), axis=1)
            RG = np.linalg.solve(Rm, G)
            M = G.conj().T @ RG
            e0 = np.zeros(G.shape[1], dtype=np.complex128)
            e0[0] = 1.0
            try:
                np.linalg.cholesky(M)
                q = np.linalg.solve(M, e0)
            except np.linalg.LinAlgError:
                ys.append(np.zeros(x.shape[1], dtype=np.complex64)), fs.append(-1)
                gs.append(np.float32(0.0)), ws.append(np.zeros(A, dtype=np.complex128))
                continue
            w = RG @ q
            g = np.float32(10.0 * np.log10(tr / (np.vdot(steer[b], steer[b]).real * q[0].real)))
            ys.append((np.conj(w.astype(np.complex64))[:, None] * x).sum(axis=0, dtype=np.complex64))
            fs.append(flag), gs.append(g), ws.append(w)
    return np.stack(ys), np.array(fs, dtype=np.int32), np.array(gs, dtype=np.float32), np.stack(ws)


def gram_pivots(cols):
    """The pivots (the values under the square roots) of the float64 Cholesky of the Gram matrix of
    the unit-normalised columns: the argument check wants every one >= 1 / 64."""
    U = np.stack([np.asarray(c, dtype=np.complex128) / np.linalg.norm(c) for c in cols], axis=1)
    G = U.conj().T @ U
    m = G.shape[0]
    L = np.zeros((m, m), dtype=np.complex128)
    piv = []
    for j in range(m):
        d = G[j, j].real - np.sum(np.abs(L[j, :j]) ** 2)
        piv.append(float(d))
        L[j, j] = np.sqrt(max(d, 0.0))
        for i in range(j + 1, m):
            L[i, j] = (G[i, j] - np.sum(L[i, :j] * np.conj(L[j, :j]))) / L[j, j] if d > 0 else 0.0
    return piv
