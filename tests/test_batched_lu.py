"""The batched LU kernel (libawelu.so) against torch.linalg on an MI355X: P A = L U, and
torch.linalg.lu_solve on its output solves A x = b (relative residual <= 1e-12).  The shapes sit on
the host dispatch's boundaries (awelu_cases.py; test_inertia_model.py checks that they still do):
the panel width, the workgroup size, the largest n, the two-wave instantiation for small blocks in
large batches, the solve's LDS cap and its chunks of right-hand sides."""
import pytest

import awelu_cases as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test on a machine without a visible GPU")
    from awebox_amd.build import LIB_LU, build_one
    build_one(LIB_LU)
    return torch


def _pivots_in_range(torch, piv):
    """LAPACK's convention: 1-based, step k exchanges row k with a row at or below it."""
    n = piv.shape[-1]
    k = torch.arange(n, device=piv.device, dtype=piv.dtype)
    return bool(((piv >= k + 1) & (piv <= n)).all())


def _check_definition(torch, A, LU, piv, g):
    n = A.shape[-1]
    assert _pivots_in_range(torch, piv)
    P, L, U = torch.lu_unpack(LU, piv)
    assert torch.allclose(P @ L @ U, A, rtol=0, atol=1e-11 * A.abs().max().item() * n)
    rhs = torch.randn(A.shape[0], n, 3, dtype=torch.float64, device="cuda", generator=g)
    x = torch.linalg.lu_solve(LU, piv, rhs)
    res = (A @ x - rhs).abs().max() / (A.abs().max() * x.abs().max() + rhs.abs().max())
    assert res.item() < 1e-12
    # partial pivoting: every multiplier is bounded by 1 in magnitude (the pivot sequence itself may
    # differ from LAPACK's where rounding flips a near-tie; then all later choices differ too)
    assert L.abs().max().item() <= 1.0 + 1e-12


def _gaussian(torch, batch, n, g):
    A = torch.randn(batch, n, n, dtype=torch.float64, device="cuda", generator=g)
    A[:, :, 0] *= 1e-3                                    # forces row interchanges
    return A


# the second row: the panel width (16) and the workgroup size (256) from both sides, and the largest n
@pytest.mark.parametrize("batch,n", [(1, 1), (3, 17), (40, 268), (20, 640), (2, 1000)] +
                         [(ac.LU_EDGE_BATCH, n) for n in ac.LU_EDGE_SIZES])
def test_lu_factor_matches_definition(gpu, batch, n):
    torch = gpu
    from awebox_amd.batched_lu import lu_factor
    g = torch.Generator(device="cuda").manual_seed(n)
    A = _gaussian(torch, batch, n, g)
    LU, piv = lu_factor(A)
    _check_definition(torch, A, LU, piv, g)


@pytest.mark.parametrize("n", ac.LU_SMALL_SIZES)
def test_lu_two_wave_instantiation_same_bits(gpu, n):
    """lu_batched_kernel<128> (n <= 128 in batches from 1100: the MPC's interval blocks) returns the
    bits of <256>, which splits the trailing columns into a different number of row chunks: the
    batch in one call against its halves and against the batch less one member (all on <256>; at
    n = 129 every call is)."""
    torch = gpu
    from awebox_amd.batched_lu import lu_factor
    batch = ac.LU_SMALL_BATCH
    g = torch.Generator(device="cuda").manual_seed(1000 + n)
    A = _gaussian(torch, batch, n, g)
    LU, piv = lu_factor(A)
    _check_definition(torch, A, LU, piv, g)
    for lo, hi in ((0, batch // 2), (batch // 2, batch), (0, batch - 1)):
        LUp, pivp = lu_factor(A[lo:hi])
        assert torch.equal(pivp, piv[lo:hi]), (lo, hi)
        assert torch.equal(LUp, LU[lo:hi]), (lo, hi)


@pytest.mark.parametrize("n", ac.LU_HADAMARD_SIZES)
def test_lu_exact_ties_lowest_row(gpu, n):
    """Sylvester's Hadamard matrix: every pivot search is an exact tie among all remaining rows and
    every intermediate value an integer of magnitude <= n, so the arithmetic is exact in any order
    and only the tie rule (lowest row, per thread, per wave and across waves) decides the factors:
    LAPACK's (first maximum) bit for bit."""
    torch = gpu
    from awebox_amd.batched_lu import lu_factor
    H = ac.hadamard(n)[0]
    LU_ref, piv_ref = torch.linalg.lu_factor(H)
    assert torch.equal(LU_ref, LU_ref.round()) and LU_ref.abs().max().item() <= n
    LU, piv = lu_factor(torch.stack([H, H]).cuda())
    for b in range(2):
        assert torch.equal(piv[b].cpu(), piv_ref)
        assert torch.equal(LU[b].cpu(), LU_ref)


@pytest.mark.parametrize("n1,m", [(84, 42), (430, 210)])
def test_lu_saddle_point_blocks(gpu, n1, m):
    """KKT-like blocks [[H, J^T], [J, 0]] under symmetric permutations: zero diagonal entries and
    columns of equal-magnitude entries: interchanges forced by exact zeros and decided by exact ties."""
    torch = gpu
    from awebox_amd.batched_lu import lu_factor
    K = ac.saddle(n1, m, perm=1)[0]
    gh = torch.Generator().manual_seed(n1)
    members = [K]
    for _ in range(3):
        p = torch.randperm(n1 + m, generator=gh)
        members.append(K[p][:, p])
    A = torch.stack(members).cuda()
    LU, piv = lu_factor(A)
    _check_definition(torch, A, LU, piv, torch.Generator(device="cuda").manual_seed(n1))


@pytest.mark.parametrize("n", [40, 268])
def test_lu_members_are_isolated(gpu, n):
    """A zero matrix and a matrix with NaNs in a batch: a zero pivot is no error (its member's
    factors are non-finite), every pivot stays in range (NaN never wins the search, a lane without
    rows proposes the diagonal), and the finite members get the bits of their solo factorisation
    and of their solo solve."""
    torch = gpu
    from awebox_amd.batched_lu import lu_factor, lu_solve
    g = torch.Generator(device="cuda").manual_seed(3 * n)
    A = _gaussian(torch, 5, n, g)
    A[2] = 0.0
    A[3, :, 7] = float("nan")
    A[3, n // 2, n - 1] = float("nan")
    rhs = torch.randn(5, n, 3, dtype=torch.float64, device="cuda", generator=g)
    LU, piv = lu_factor(A)
    x = lu_solve(LU, piv, rhs)
    assert _pivots_in_range(torch, piv)
    good = [0, 1, 4]
    _check_definition(torch, A[good], LU[good], piv[good], g)
    for b in good:
        LU1, piv1 = lu_factor(A[b:b + 1])
        assert torch.equal(piv1[0], piv[b]) and torch.equal(LU1[0], LU[b]), b
        assert torch.equal(lu_solve(LU1, piv1, rhs[b:b + 1])[0], x[b]), b
        assert bool(torch.isfinite(x[b]).all())


def test_lu_rejects_n_beyond_the_panel_budget(gpu):
    """n = 1025: ValueError from the wrapper, return code 1 with a message from the library, and in
    both cases no launch (the buffers keep their contents)."""
    import ctypes
    torch = gpu
    from awebox_amd.batched_lu import load_library, lu_factor
    n = ac.LU_REJECTED_N
    A = torch.full((1, n, n), 2.0, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        lu_factor(A)
    piv = torch.full((1, n), -7, dtype=torch.int32, device="cuda")
    lib = load_library()
    rc = lib.awelu_factor_batched(n, 1, ctypes.c_void_p(A.data_ptr()), ctypes.c_void_p(piv.data_ptr()),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 1 and len(lib.awelu_last_error()) > 0
    torch.cuda.synchronize()
    assert bool((A == 2.0).all()) and bool((piv == -7).all())


@pytest.mark.parametrize("batch,n,nrhs", [(1, 1, 1), (5, 17, 3), (256, 60, 1), (64, 126, 22), (16, 463, 1),
                                          (3, 1000, 40)] + list(ac.SOLVE_SHAPES))
def test_lu_solve_matches_torch(gpu, batch, n, nrhs):
    """awelu_solve_batched (LDS-resident right-hand sides, chunked when n (16 + nrhs) doubles exceed
    the LDS budget, as for n = 1000, nrhs = 40) against torch.linalg.lu_solve on the same factors.
    (2, 1024, 5): the cap is 2 columns per workgroup; (1, 60, 17) and (1, 60, 33): one more than
    the smallest chunk, split in 2 and 3; (300, 126, 3): more matrices than target workgroups."""
    torch = gpu
    from awebox_amd.batched_lu import lu_factor, lu_solve
    g = torch.Generator(device="cuda").manual_seed(7 * n + nrhs)
    A = torch.randn(batch, n, n, dtype=torch.float64, device="cuda", generator=g)
    A[:, :, 0] *= 1e-3
    rhs = torch.randn(batch, n, nrhs, dtype=torch.float64, device="cuda", generator=g)
    LU, piv = lu_factor(A)
    x = lu_solve(LU, piv, rhs)
    x_ref = torch.linalg.lu_solve(LU, piv, rhs)
    assert (x - x_ref).abs().max().item() <= 1e-10 * x_ref.abs().max().item()
    res = (A @ x - rhs).abs().max() / (A.abs().max() * x.abs().max() + rhs.abs().max())
    assert res.item() < 1e-12


@pytest.mark.parametrize("batch,n,nrhs", ac.SOLVE_COLUMN_SHAPES)
def test_lu_solve_column_invariance(gpu, batch, n, nrhs):
    """A right-hand-side column gets the same bits alone as in any chunk of any launch: the first
    and last column, and the two either side of the first chunk boundary (w, the host code's
    balanced chunk width); and a strided right-hand side gets the bits of its contiguous copy."""
    torch = gpu
    from awebox_amd.batched_lu import lu_factor, lu_solve
    w, cap = ac.solve_chunk_width(ac.read_constants(), batch, n, nrhs)
    assert 1 <= w < nrhs and w <= cap
    g = torch.Generator(device="cuda").manual_seed(11 * n + nrhs)
    A = _gaussian(torch, batch, n, g)
    wide = torch.randn(batch, n, 2 * nrhs, dtype=torch.float64, device="cuda", generator=g)
    rhs = wide[:, :, ::2]                                 # not contiguous
    assert not rhs.is_contiguous()
    wide0 = wide.clone()
    LU, piv = lu_factor(A)
    x = lu_solve(LU, piv, rhs)
    assert torch.equal(x, lu_solve(LU, piv, rhs.contiguous()))
    assert torch.equal(wide, wide0) and x.is_contiguous()  # the caller's tensor is left alone
    for j in sorted({0, w - 1, w, nrhs - 1}):
        xj = lu_solve(LU, piv, rhs[:, :, j:j + 1])
        assert torch.equal(xj[:, :, 0], x[:, :, j]), j


@pytest.mark.parametrize("batch,nb,m,nrhs", [(1, 1, 1, 1), (4, 5, 7, 2), (256, 21, 22, 1), (3, 9, 32, 8),
                                            (1, 81, 23, 30), (2, 41, 46, 70), (8, 41, 46, 1), (1, 7, 48, 3)])
def test_btd_solve_matches_dense(gpu, batch, nb, m, nrhs):
    """awelu_btd_factor_batched + awelu_btd_solve_batched (chunked beyond 64 right-hand sides, as
    for nrhs = 70) against a dense solve of the assembled block-tridiagonal matrix;
    KKT-like blocks (indefinite diagonal blocks with a zero-ish corner) exercise the in-block
    pivoting."""
    torch = gpu
    from awebox_amd.batched_lu import btd_dense, btd_factor, btd_solve
    g = torch.Generator(device="cuda").manual_seed(nb * m + nrhs)
    T = torch.randn(batch, nb, 3, m, m, dtype=torch.float64, device="cuda", generator=g)
    T[:, :, 1] += 4.0 * torch.eye(m, dtype=torch.float64, device="cuda")
    T[:, :, 1, : m // 2, : m // 2] *= 1e-6
    X = torch.randn(batch, nb, m, nrhs, dtype=torch.float64, device="cuda", generator=g)
    F, Dinv = btd_factor(T)
    x = btd_solve(F, Dinv, X)
    assert torch.equal(btd_solve(F, Dinv, X), x)          # the factors are reusable
    A = btd_dense(T).cpu()                               # host LAPACK as the independent reference
    b = X.reshape(batch, nb * m, nrhs).cpu()
    xs = x.reshape(batch, nb * m, nrhs).cpu()
    x_ref = torch.linalg.solve(A, b)
    scale = A.abs().amax(dim=(1, 2)) * xs.abs().amax(dim=(1, 2)) + b.abs().amax(dim=(1, 2))
    res = ((A @ xs - b).abs().amax(dim=(1, 2)) / scale).max().item()
    # backward error of the block sweep: explicit pivot-block inverses with one refinement step per
    # block solve, and no interchanges between block rows (1e-11 measured on the 256 random systems)
    assert res < 1e-10
    cond = torch.linalg.cond(A)                          # forward error: cond x eps x block growth
    fwd = ((xs - x_ref).abs().amax(dim=(1, 2)) / x_ref.abs().amax(dim=(1, 2)))
    assert bool((fwd <= 1e-13 * cond + 1e-10).all())
