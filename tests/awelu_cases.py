"""Inputs for the libawelu tests (LU, solve, inertia): matrix families whose inertia is known by
construction, the eigenvalue reference with a check that it is unambiguous, the dispatch
constants of batched_lu.hip, and the shape tables of the GPU tests (test_inertia_model.py asserts
that the tables straddle every dispatch threshold).

All matrices are host float64 tensors from a seeded torch.Generator; every family returns
(A, (positive, negative, zero))."""
import os
import re

import torch

F64 = torch.float64
ZTOL = 1e-11
HIP_SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "awebox_amd", "csrc",
                          "batched_lu.hip")

# ---- shape tables of the GPU tests ------------------------------------------------------------
LU_EDGE_BATCH = 3
LU_EDGE_SIZES = (2, 15, 16, 32, 33, 128, 129, 255, 256, 257, 1024)        # kNB, kThreads, kMaxN edges
LU_SMALL_BATCH = 1100                                                     # = kLuSmallMinBatch
LU_SMALL_SIZES = (126, 128, 17, 1, 129)                                   # 129 stays on <256>
LU_HADAMARD_SIZES = (16, 64, 512)
LU_REJECTED_N = 1025
SOLVE_SHAPES = ((2, 1024, 5), (1, 60, 17), (1, 60, 33), (300, 126, 3))    # (batch, n, nrhs)
SOLVE_COLUMN_SHAPES = ((1, 60, 33), (3, 1000, 40))
INERTIA_SIZES = (1, 2, 3, 63, 64, 65, 126, 199, 200, 201, 255, 256, 257, 640)
INERTIA_NARROW = ((800, 410), (1290, 640))                                # saddle (n1, m): nb = 15, 9
INERTIA_REJECTED_N = 4801


def read_constants(path=HIP_SOURCE):
    """The integer dispatch constants of batched_lu.hip (constexpr <type> kName = <int products>;)."""
    with open(path) as f:
        src = f.read()
    out = {}
    for name, expr in re.findall(r"constexpr\s+(?:int|long|size_t)\s+(k\w+)\s*=\s*([0-9][0-9\s*]*);", src):
        v = 1
        for factor in expr.split("*"):
            v *= int(factor)
        out[name] = v
    return out


def solve_chunk_width(c, batch, n, nrhs):
    """awelu_solve_batched's balanced chunk width (right-hand sides per workgroup) and the LDS cap."""
    cap = c["kSolveLds"] // 8 // n - c["kNB"]
    want = max(1, -(-c["kSolveTargetWgs"] // batch))
    w = min(max(c["kSolveMinChunk"], -(-nrhs // want)), cap)
    nchunks = -(-nrhs // w)
    return -(-nrhs // nchunks), cap


def inertia_panel_width(c, n):
    """awelu_sym_inertia_batched's panel width nb for n rows (fewer than 4: the size is rejected)."""
    return min(c["kSyNB"], c["kSyLds"] // 8 // max(n, 1))


# ---- matrix families ---------------------------------------------------------------------------
def _gen(*key):
    seed = 12345
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def saddle(n1, m, dup=0, perm=0):
    """[[H, J^T], [J, 0]]: H a diagonal of integers in 1..3 (n1 rows), J m x n1 with entries in
    {-1, 0, 1} and full row rank; dup copies row 0 of J into its last row, perm applies a symmetric
    random permutation.  H > 0, so the inertia is (n1, rank J, m - rank J): (n1, m, 0), and
    (n1, m - 1, 1) with dup and m > 1.

    Up to 32 columns J is dense (redrawn until it has full rank).  Beyond, J is sparse, as a KKT
    Jacobian is: every row has a +-1 in a column of its own, which gives the rank by construction,
    and +-1 in two random columns that no row owns (none if m = n1).  The reason is the eigenvalue
    reference, not the kernel: eigvalsh returns an exact zero eigenvalue as a few eps ||A||_2,
    whatever the size, and inertia_reference wants it below 1e-14 max|A| = 1e-14 max H.  A dense J
    has ||A||_2 about sqrt(n) and lands on either side of that bound by chance from about 600 rows on
    (0.3e-14 .. 1.8e-14 max|A| over the seeds at 1930 rows).  Three entries a row keep ||A||_2 below
    4.9 = 1.6 max|A|, and H in 1..3 allows no less than 1.0.  Measured |ev| / max|A| of the zero
    eigenvalue with 1, 4, 8 and 16 LAPACK threads, over every dup case of the tests (perm both
    ways): at most 1.9e-15 up to 640 rows, 2.1e-15 at 1210 rows and 4.1e-15 at 1930 rows (0.6e-15 to
    4.1e-15 over the four thread counts there), so 2.4 times inside the bound at the worst.  That is
    eigvalsh's floor, about 4 eps ||A||_2: two entries a row (||A||_2 = 4.3) measured up to
    3.0e-15, so a still sparser J buys no wider margin."""
    assert 0 <= m <= n1
    g = _gen(1, n1, m)
    h = torch.randint(1, 4, (n1,), generator=g).to(F64)
    if n1 <= 32:
        while True:
            J = torch.randint(-1, 2, (m, n1), generator=g).to(F64)
            if m == 0 or int(torch.linalg.matrix_rank(J)) == m:
                break
    else:
        cols = torch.randperm(n1, generator=g)
        own, free = cols[:m], cols[m:]
        rows = torch.arange(m)
        J = torch.zeros(m, n1, dtype=F64)
        J[rows, own] = (2 * torch.randint(0, 2, (m,), generator=g) - 1).to(F64)
        for _ in range(2 if len(free) else 0):
            c = free[torch.randint(0, len(free), (m,), generator=g)]
            J[rows, c] = (2 * torch.randint(0, 2, (m,), generator=g) - 1).to(F64)
    rank = m
    if dup and m > 1:
        J[m - 1] = J[0]
        rank = m - 1
    n = n1 + m
    A = torch.zeros(n, n, dtype=F64)
    A[:n1, :n1] = torch.diag(h)
    A[n1:, :n1] = J
    A[:n1, n1:] = J.T
    if perm:
        p = torch.randperm(n, generator=_gen(2, n1, m))
        A = A[p][:, p].contiguous()
    return A, (n1, rank, m - rank)


def antidiag(n):
    """2 x 2 blocks [[0, 1], [1, 0]] down the diagonal, a trailing -1 when n is odd: the diagonal is
    zero and |a(k+1, k)| = |a(k, k+1)| exactly, so every Bunch-Kaufman test is an exact tie and every
    pivot is 2 x 2 without an interchange."""
    A = torch.zeros(n, n, dtype=F64)
    for k in range(0, n - 1, 2):
        A[k, k + 1] = A[k + 1, k] = 1.0
    if n % 2:
        A[n - 1, n - 1] = -1.0
    return A, (n // 2, n // 2 + n % 2, 0)


def zero(n):
    return torch.zeros(n, n, dtype=F64), (0, 0, n)


def diagonal(n):
    """diag(2, -1, 0, 2, -1, 0, ...)."""
    d = torch.tensor([2.0, -1.0, 0.0], dtype=F64).repeat(n // 3 + 1)[:n]
    return torch.diag(d), (int((d > 0).sum()), int((d < 0).sum()), int((d == 0).sum()))


def congruence(n):
    """U diag(linspace(-3, 2, n - 2)) U^T with a Gaussian n x (n - 2) U: two zero eigenvalues (and the
    signs of the diagonal, by Sylvester's law), n > 2."""
    assert n > 2
    g = _gen(3, n)
    U = torch.randn(n, n - 2, generator=g, dtype=F64)
    d = torch.linspace(-3, 2, n - 2, dtype=F64)
    d[d.abs() < 1e-12] = 0.0                              # the grid point at 0 (n = 5 i + 3), exactly
    A = U @ torch.diag(d) @ U.T
    A = 0.5 * (A + A.T)
    return A, (int((d > 0).sum()), int((d < 0).sum()), 2 + int((d == 0).sum()))


def hadamard(n):
    """Sylvester's Hadamard matrix, n a power of two: symmetric, H^2 = n I, trace 0 for n > 1."""
    assert n >= 1 and n & (n - 1) == 0
    H = torch.ones(1, 1, dtype=F64)
    while H.shape[0] < n:
        H = torch.cat([torch.cat([H, H], 1), torch.cat([H, -H], 1)], 0)
    return H, ((1, 0, 0) if n == 1 else (n // 2, n // 2, 0))


def inertia_families(n):
    """Every family at total size n (saddle with n1 about 2 n / 3, dup and perm both ways):
    (names, A [members, n, n], expected [members, 3] int32)."""
    m = n // 3
    cases = [(f"saddle(dup={dup},perm={perm})", saddle(n - m, m, dup, perm)) for dup in (0, 1) for perm in (0, 1)]
    cases += [("antidiag", antidiag(n)), ("zero", zero(n)), ("diagonal", diagonal(n))]
    if n > 2:
        cases.append(("congruence", congruence(n)))
    if n & (n - 1) == 0:
        cases.append(("hadamard", hadamard(n)))
    names = [c[0] for c in cases]
    A = torch.stack([c[1][0] for c in cases])
    want = torch.tensor([c[1][1] for c in cases], dtype=torch.int32)
    return names, A, want


def inertia_reference(A, ztol=ZTOL):
    """sym_inertia_host's counts of A ([n, n] or [batch, n, n]), after asserting that they are
    unambiguous: every eigenvalue counted non-zero is at least 1e3 ztol max|A| in magnitude and every
    one counted zero at most 1e-3 ztol max|A|.  This is a condition on the input (a matrix that
    breaks it is a bad test case), not a tolerance on the code under test."""
    from awebox_amd.batched_lu import sym_inertia_host
    A3 = A if A.dim() == 3 else A.unsqueeze(0)
    ev = torch.linalg.eigvalsh(0.5 * (A3 + A3.transpose(-1, -2)))
    scale = A3.abs().amax(dim=(-1, -2)).unsqueeze(-1)
    is_zero = ev.abs() <= ztol * scale.clamp(min=1e-300)
    far = (ev.abs() >= 1e3 * ztol * scale) & ~is_zero
    tiny = (ev.abs() <= 1e-3 * ztol * scale) & is_zero
    bad = ~(far | tiny)
    assert not bool(bad.any()), ("ambiguous reference: |ev| / max|A| =",
                                 (ev.abs() / scale.clamp(min=1e-300))[bad].tolist())
    counts = sym_inertia_host(A3, ztol=ztol)
    return counts if A.dim() == 3 else counts[0]
