"""Inputs and references for the tests of libawelu's block-tridiagonal kernels (btd_factor_kernel,
btd_apply_kernel): matrix families T[nb, 3, m, m] (host float64; slot 0 the sub-diagonal block L_k,
1 the diagonal block D_k, 2 the super-diagonal block U_k), the block recursion and a dense solve in
numpy.longdouble (80-bit) as the references, an exact float64 model of one block of the kernel's
Gauss-Jordan loop, the bounds of the GPU tests and their shape tables (test_btd_model.py asserts
that the tables straddle every edge of the kernels' tiling and of the solve's chunking).

The slots that the kernels ignore (L_0 and U_{nb-1}) hold random numbers in sym and perm_noise, so
that a kernel reading them is noticed."""
from fractions import Fraction

import numpy as np
import torch

import awelu_cases as ac

F64 = torch.float64
LD = np.longdouble
EPS = 2.0 ** -52

# ---- shape tables of the GPU tests ------------------------------------------------------------
# the Gauss-Jordan loop's tiles: 3 rows per lane, 12 rows per wave, 9 columns per lane (16 column
# groups over [D' | U | I]), the smallest and the largest block
BTD_M_EDGES = (1, 2, 3, 4, 8, 9, 10, 11, 12, 13, 18, 19, 24, 25, 27, 28, 36, 37, 47, 48)
BTD_FACTOR_NB, BTD_FACTOR_BATCH = 3, 2
BTD_LONG_CHAIN = (41, 46)                                                 # (nb, m)
BTD_MODEL_MAX_M = 25                                                      # gj_model: a block well under a second
BTD_PIVOT_RULE_M = (13, 25)
BTD_INERTIA_M, BTD_INERTIA_NB = (12, 13, 48), 5
BTD_ALTERNATING = (3, 13)                                                 # (nb, m)
BTD_ISOLATION_M = (13, 48)
# (batch, nb, m, nrhs): chunk widths 1, 2 (150 chunks), 2 (ragged), 19 (ragged), 64, 33 (ragged)
BTD_SOLVE_SHAPES = ((1, 3, 13, 5), (1, 2, 48, 300), (4, 3, 25, 65), (40, 2, 12, 129), (256, 2, 7, 64),
                    (300, 2, 7, 65))
BTD_SOLVE_WIDTHS = (1, 2, 2, 19, 64, 33)
BTD_SOLVE_TARGET_WGS = 256                                # the literal in awelu_btd_solve_batched


def btd_tiles(c):
    """(rows per wave, rows per lane, columns per lane) of btd_factor_kernel<kThreads, kBtdMaxM>."""
    waves = c["kThreads"] // 64
    rows_wave = c["kBtdMaxM"] // waves
    return rows_wave, rows_wave // 4, 3 * c["kBtdMaxM"] // 16


def btd_chunk_width(c, batch, nrhs):
    """awelu_btd_solve_batched's right-hand sides per workgroup."""
    chunks = min(nrhs, max(-(-nrhs // c["kBtdMaxRhs"]), -(-BTD_SOLVE_TARGET_WGS // batch)))
    return -(-nrhs // chunks)


# ---- matrix families ---------------------------------------------------------------------------
def _scaled(A, norm):
    return A * (norm / torch.linalg.matrix_norm(A, 2).item())


def _ints(m, g):
    return torch.randint(-3, 4, (m, m), generator=g).to(F64)


def _signed_perm(m, g):
    """A signed permutation matrix times powers of two in 2^-3 .. 2^3, and the row of every column's
    entry."""
    p = torch.randperm(m, generator=g)
    v = (2 * torch.randint(0, 2, (m,), generator=g) - 1).to(F64) * 2.0 ** torch.randint(-3, 4, (m,), generator=g).to(F64)
    D = torch.zeros(m, m, dtype=F64)
    D[torch.arange(m), p] = v
    return D, torch.argsort(p)


def sym(nb, m, member=0):
    """Symmetric T: D_k = Q diag(+-d) Q^T with d in [2, 4], random signs and Q orthogonal; U_k
    Gaussian with 2-norm 0.5; L_k = U_{k-1}^T.  |L_k W_{k-1}| stays below the smallest |eigenvalue|
    of D_k (|W_{k-1}| <= 0.5 / 1.8), so every pivot block is regular: measured kappa_inf(D'_k) <= 45
    and kappa_inf(T) <= 63 over the tests' shapes, and the smallest |eigenvalue| of T is about 1.8.
    member: another draw, for a batch."""
    g = ac._gen(21, nb, m, member)
    T = torch.randn(nb, 3, m, m, generator=g, dtype=F64)
    for k in range(nb):
        Q = torch.linalg.qr(torch.randn(m, m, generator=g, dtype=F64))[0]
        d = (2.0 + 2.0 * torch.rand(m, generator=g, dtype=F64)) * (2 * torch.randint(0, 2, (m,), generator=g) - 1)
        D = Q @ torch.diag(d) @ Q.T
        T[k, 1] = 0.5 * (D + D.T)
        if k < nb - 1:
            T[k, 2] = _scaled(torch.randn(m, m, generator=g, dtype=F64), 0.5)
            T[k + 1, 0] = T[k, 2].T
    return T


def alternating(nb, m, member=0):
    """Symmetric T whose pivot blocks' inertia comes from the update alone: every D_k is positive
    definite (Q diag(d) Q^T, d in [2, 4]) and U_k = 5 Q' with Q' orthogonal, L_k = U_{k-1}^T.  Then
    D'_1 = D_1 - U_0^T D_0^-1 U_0 has its eigenvalues in [2 - 12.5, 4 - 6.25]: negative definite;
    D'_2 = D_2 + 25 Q'^T |D'_1|^-1 Q' is positive definite again, eigenvalues in [4.3, 15.2].  For
    nb <= 3 (later blocks are indefinite and can come close to singular): T has m negative
    eigenvalues at nb = 3, the D_k none."""
    assert nb <= 3
    g = ac._gen(27, nb, m, member)
    T = torch.randn(nb, 3, m, m, generator=g, dtype=F64)
    for k in range(nb):
        Q = torch.linalg.qr(torch.randn(m, m, generator=g, dtype=F64))[0]
        D = Q @ torch.diag(2.0 + 2.0 * torch.rand(m, generator=g, dtype=F64)) @ Q.T
        T[k, 1] = 0.5 * (D + D.T)
        if k < nb - 1:
            T[k, 2] = 5.0 * torch.linalg.qr(torch.randn(m, m, generator=g, dtype=F64))[0]
            T[k + 1, 0] = T[k, 2].T
    return T


def perm_noise(nb, m, member=0):
    """D_k a signed permutation matrix times powers of two in 2^-3 .. 2^3 plus 2^-20 N(0, 1) dense
    noise; U_k and L_k Gaussian with 2-norm 0.25.  In D_0 only the column maximum is a usable pivot
    (every other entry of the column is noise), and it usually lies in another wave's rows.
    member: another draw, for a batch."""
    g = ac._gen(22, nb, m, member)
    T = torch.randn(nb, 3, m, m, generator=g, dtype=F64)
    for k in range(nb):
        T[k, 1] = _signed_perm(m, g)[0] + 2.0 ** -20 * torch.randn(m, m, generator=g, dtype=F64)
        if k < nb - 1:
            T[k, 2] = _scaled(torch.randn(m, m, generator=g, dtype=F64), 0.25)
            T[k + 1, 0] = _scaled(torch.randn(m, m, generator=g, dtype=F64), 0.25)
    return T


def perm_exact(m):
    """nb = 1: the signed, power-of-two-scaled permutation alone and an integer U in -3 .. 3.  Every
    operation of the elimination is exact.  Returns (T, Dinv, W) with the exact D^-1 and D^-1 U."""
    g = ac._gen(23, m)
    D = _signed_perm(m, g)[0]
    U = _ints(m, g)
    Dinv = torch.where(D.T != 0, 1.0 / D.T, torch.zeros_like(D))        # powers of two: exact
    return torch.stack([torch.zeros(m, m, dtype=F64), D, U]).unsqueeze(0), Dinv, Dinv @ U


def hadamard(m):
    """nb = 1: Sylvester's Hadamard matrix (every pivot search an exact tie) and the same integer U.
    Gauss-Jordan with the lowest row on ties is exact on it (pivots are powers of two, numerators
    have at most 6 bits).  Returns (T, Dinv, W) = (T, H / m, H U / m)."""
    H = ac.hadamard(m)[0]
    U = _ints(m, ac._gen(24, m))
    return torch.stack([torch.zeros(m, m, dtype=F64), H, U]).unsqueeze(0), H / m, (H @ U) / m


def with_tail(T):
    """T with one more block row (L = 0, D = I, U = 0).  The kernel forms no W for the last block
    row, so a one-block case whose W is wanted gets this tail: D'_0 = D_0 and W_0 = D_0^-1 U_0 as
    for nb = 1, D' = I exactly for the tail."""
    m = T.shape[-1]
    tail = torch.zeros(1, 3, m, m, dtype=F64)
    tail[0, 1] = torch.eye(m, dtype=F64)
    return torch.cat([T, tail])


def pivot_rule(m):
    """nb = 1: perm_noise's D with a second copy (random sign) of every column's pivot entry in a row
    of another wave, 13 rows lower (m = 13: in row 12, the only row of the second wave, or row 0),
    redrawn until kappa_inf <= 1e3; and a Gaussian U of norm 0.25.  The noise leaves the two copies
    alone, so column 0's search is an exact tie between two waves (the first elimination step
    spreads the noise over the other copies: gj_model reports no later tie)."""
    rows_wave = 12
    for draw in range(100):
        g = ac._gen(25, m, draw)
        P, row_of = _signed_perm(m, g)
        D = P + 2.0 ** -20 * torch.randn(m, m, generator=g, dtype=F64)
        for c in range(m):
            r = int(row_of[c])
            r2 = (r + 13) % m if m > 13 else (12 if r < 12 else 0)
            assert r2 // rows_wave != r // rows_wave
            s = 1.0 if int(torch.randint(0, 2, (1,), generator=g)) else -1.0
            D[r, c] = P[r, c]
            D[r2, c] = s * P[r, c]
        U = _scaled(torch.randn(m, m, generator=g, dtype=F64), 0.25)
        if np.linalg.cond(D.numpy(), np.inf) <= 1e3:
            return torch.stack([torch.zeros(m, m, dtype=F64), D, U]).unsqueeze(0)
    raise AssertionError("no regular pivot-rule matrix")


def dense(T):
    """The dense [nb m, nb m] matrix of T [nb, 3, m, m] (numpy, T's dtype)."""
    T = np.asarray(T)
    nb, _, m, _ = T.shape
    A = np.zeros((nb * m, nb * m), dtype=T.dtype)
    for k in range(nb):
        for s, dk in ((0, -1), (1, 0), (2, 1)):
            if 0 <= k + dk < nb:
                A[k * m:(k + 1) * m, (k + dk) * m:(k + dk + 1) * m] = T[k, s]
    return A


# ---- the long-double references ----------------------------------------------------------------
def _gauss_jordan(A, B):
    """A^-1 B by Gauss-Jordan with partial pivoting, in A's dtype."""
    n = A.shape[0]
    M = np.concatenate([A, B], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        if p != c:
            M[[c, p]] = M[[p, c]]
        M[c] = M[c] / M[c, c]
        f = M[:, c].copy()
        f[c] = 0
        M -= f[:, None] * M[c][None, :]
    return M[:, n:]


def _norm_inf(A):
    return float(np.abs(A).sum(axis=1).max())


def sweep_reference(T):
    """The block recursion in numpy.longdouble: D'_k = D_k - L_k W_{k-1},
    [W_k | Dinv_k] = D'_k^-1 [U_k | I].  Returns (Dp, W, Dinv) [nb, m, m] long double (W's last block
    is zero: the recursion has no use for it) and kappa [nb] float: the largest
    kappa_inf(D'_j) over j <= k, the factor bound's condition number."""
    assert np.finfo(LD).eps < 2.0 ** -60, "the reference needs an extended-precision long double"
    Tl = np.asarray(T, dtype=np.float64).astype(LD)
    nb, _, m, _ = Tl.shape
    Dp, W, Dinv = (np.zeros((nb, m, m), dtype=LD) for _ in range(3))
    kappa = np.zeros(nb)
    for k in range(nb):
        Dp[k] = Tl[k, 1] - (Tl[k, 0] @ W[k - 1] if k > 0 else 0)
        S = _gauss_jordan(Dp[k], np.concatenate([Tl[k, 2], np.eye(m, dtype=LD)], axis=1))
        if k < nb - 1:
            W[k] = S[:, :m]
        Dinv[k] = S[:, m:]
        kappa[k] = max(_norm_inf(Dp[k]) * _norm_inf(Dinv[k]), kappa[k - 1] if k > 0 else 0.0)
    return Dp, W, Dinv, kappa


def solve_reference(T, X, max_n=240):
    """T^-1 X by a long-double Gauss-Jordan solve of the assembled dense matrix; X [nb, m, nrhs].
    Returns (x [nb, m, nrhs] long double, kappa_inf(T)).  nb m <= 240 keeps it to a fraction of a
    second (the GPU tests stay there; test_btd_model.py pays a second for two larger ones)."""
    assert np.finfo(LD).eps < 2.0 ** -60
    nb, _, m, _ = T.shape
    assert nb * m <= max_n
    A = dense(np.asarray(T, dtype=np.float64))
    x = _gauss_jordan(A.astype(LD), np.asarray(X, dtype=np.float64).astype(LD).reshape(nb * m, -1))
    return x.reshape(nb, m, -1), float(np.linalg.cond(A, np.inf))


# ---- the bounds of the GPU tests (and, at a quarter, of the float64 restatement) ---------------
def factor_excess(got, ref, kappa):
    """The largest max|B_k - ref_k| / (m eps kappa_k max|ref_k|) over the blocks of one factor output
    (D', W or Dinv; got [nb', m, m], ref its long-double reference): at most 1 within the bound."""
    m = ref.shape[-1]
    worst = 0.0
    for k in range(got.shape[0]):
        scale = float(np.abs(ref[k]).max())
        err = float(np.abs(np.asarray(got[k], dtype=np.float64).astype(LD) - ref[k]).max())
        if scale == 0.0:
            assert err == 0.0
            continue
        worst = max(worst, err / (m * EPS * kappa[k] * scale))
    return worst


def solve_excess(got, ref, kappa_T):
    """max|x - ref| / (4 eps kappa_inf(T) max|ref|)."""
    err = float(np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref).max())
    return err / (4 * EPS * kappa_T * float(np.abs(ref).max()))


# ---- the exact model of one block ---------------------------------------------------------------
def _fnma(f, p, a):
    """fma(-f, p, a), correctly rounded (Python 3.10 has no math.fma)."""
    if f == 0.0 or p == 0.0:
        return a - f * p                                  # an exact zero product
    return float(Fraction(a) - Fraction(f) * Fraction(p))


def gj_model(D, U, rows_wave=12, highest_wave_on_ties=False):
    """An exact float64 model of one block of btd_factor_kernel's Gauss-Jordan loop on [D | U | I]
    (nb = 1, where D' = D).  The pivot of column c is the largest |a[r][c]| over the unused rows,
    the lowest row on ties: every wave (rows_wave rows) proposes its lowest such row, and the lowest
    wave wins ties (highest_wave_on_ties: the broken rule `kw >= kb`, for the tests of the tests).
    rp = 1 / a[p][c];  pr = a[p][.] rp, a plain product;  a[r][.] = fma(-a[r][c], pr, a[r][.]) for
    r != p, the compiler's contraction of the kernel's a - f pr;  row p becomes pr;  output row c is
    row piv[c].  Returns (W, Dinv) float64 tensors, piv, and the columns whose choice was an exact
    tie between two waves."""
    m = D.shape[0]
    assert m <= BTD_MODEL_MAX_M
    a = [[float(x) for x in D[r]] + [float(x) for x in U[r]] + [1.0 if j == r else 0.0 for j in range(m)]
         for r in range(m)]
    used, piv, ties = [False] * m, [], []
    for c in range(m):
        cand = []                                         # (key, row) of every wave with an unused row
        for w0 in range(0, m, rows_wave):
            best, bi = -1.0, -1
            for r in range(w0, min(m, w0 + rows_wave)):
                if not used[r] and abs(a[r][c]) > best:
                    best, bi = abs(a[r][c]), r
            if bi >= 0:
                cand.append((best, bi))
        kb, p = cand[0]
        for kw, r in cand[1:]:
            if kw > kb or (highest_wave_on_ties and kw == kb):
                kb, p = kw, r
        if sum(k == kb for k, _ in cand) > 1:
            ties.append(c)
        used[p] = True
        piv.append(p)
        rp = 1.0 / a[p][c]
        pr = [x * rp for x in a[p]]
        for r in range(m):
            if r != p:
                f = a[r][c]
                if f != 0.0:
                    a[r] = [_fnma(f, pr[j], a[r][j]) for j in range(3 * m)]
        a[p] = pr
    out = torch.tensor([a[piv[c]] for c in range(m)], dtype=F64)
    assert bool(torch.isfinite(out).all())
    return out[:, m:2 * m].contiguous(), out[:, 2 * m:].contiguous(), piv, ties


# ---- a bordered separator system for btd.BorderedBtd --------------------------------------------
def bordered_case(nb=4, m=13, n_border=3, unused=((1, 4), (3, 12))):
    """A symmetric bordered block-tridiagonal system in btd.BorderedBtd's input form: sym(nb, m) with
    the rows and columns of two unused block positions taken out, a border of 3 unknowns (Gaussian
    couplings of norm 0.5, a diagonal-dominant indefinite corner), the separators in a random order;
    every fifth entry is split in two duplicates (two terms, so their sum does not depend on the
    order), and two entries point past the last separator (BorderedBtd drops them).
    Returns (stage_of, pos_of, rows, cols, vals, S): S [n_S, n_S] the assembled matrix."""
    g = ac._gen(26, nb, m)
    A = torch.tensor(dense(sym(nb, m).numpy()))
    slots = [(k, i) for k in range(nb) for i in range(m) if (k, i) not in unused]
    n_t, n_s = len(slots), len(slots) + n_border
    S = torch.zeros(n_s, n_s, dtype=F64)
    idx = torch.tensor([k * m + i for k, i in slots])
    S[:n_t, :n_t] = A[idx][:, idx]
    E = _scaled(torch.randn(n_t, n_border, generator=g, dtype=F64), 0.5)
    S[:n_t, n_t:] = E
    S[n_t:, :n_t] = E.T
    S[n_t:, n_t:] = torch.diag(torch.tensor([3.0, -2.5, 2.0], dtype=F64)[:n_border])
    order = torch.randperm(n_s, generator=g)               # separator q is row order[q] of the above
    S = S[order][:, order].contiguous()
    stage = [slots[int(o)][0] if int(o) < n_t else -1 for o in order]
    pos = [slots[int(o)][1] if int(o) < n_t else 0 for o in order]
    rows, cols, vals = [], [], []
    for n, (r, c) in enumerate(torch.nonzero(S).tolist()):
        v = float(S[r, c])
        parts = (0.25 * v, v - 0.25 * v) if n % 5 == 0 else (v,)
        for part in parts:
            rows.append(r)
            cols.append(c)
            vals.append(part)
    rows += [n_s, 0]
    cols += [0, n_s]
    vals += [7.0, 7.0]
    shuffle = torch.randperm(len(rows), generator=g).tolist()
    rows, cols, vals = ([x[i] for i in shuffle] for x in (rows, cols, vals))
    S_sum = torch.zeros(n_s + 1, n_s + 1, dtype=F64)
    S_sum.index_put_((torch.tensor(rows), torch.tensor(cols)), torch.tensor(vals, dtype=F64), accumulate=True)
    return np.array(stage), np.array(pos), np.array(rows), np.array(cols), torch.tensor(vals, dtype=F64), \
        S_sum[:n_s, :n_s].contiguous()
