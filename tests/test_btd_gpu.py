"""btd_factor_kernel and btd_apply_kernel (libawelu.so) on an MI355X, block by block: the three
outputs of the factorisation (D'_k, W_k, Dinv_k) and the solution against the long-double references
of btd_cases.py, at the edges of the Gauss-Jordan loop's tiling and of the solve's chunking
(test_btd_model.py checks that the tables still sit there, and that the inputs allow the bounds).

Bounds, eps = 2^-52, against the long-double reference only:
    a factor block B_k:  max|B_k - ref_k| <= m eps max_{j<=k} kappa_inf(D'_j) max|ref_k|
    a solution:          max|x - ref|     <= 4 eps kappa_inf(T) max|ref|
Every test prints its share of the bound before it asserts.  Measured on an MI355X, the worst share
over the cases: factor outputs 0.56 at m = 1 (two roundings against a bound of 2 (eps / 2) there),
0.22 from m = 2 on and 0.007 on the long chain; solutions 0.031; the pivot-rule matrices agree with
the exact model in every entry.  The whole file takes 4 s, no test more than 0.2 s.

A one-block case (nb = 1) gets no W from the kernel (the last block row's U is not read), so where
W_0 = D_0^-1 U_0 is wanted the case runs a second time with btd_cases.with_tail's identity block row."""
import numpy as np
import pytest

import awelu_cases as ac
import btd_cases as bc

pytestmark = pytest.mark.gpu

FAMILIES = {"sym": bc.sym, "perm_noise": bc.perm_noise}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test on a machine without a visible GPU")
    from awebox_amd.build import LIB_LU, build_one
    build_one(LIB_LU)
    return torch


def _bits(torch, a, b):
    """Equal bit for bit (NaNs and signed zeros included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _factor(torch, T):
    """btd_factor of host T [batch, nb, 3, m, m]: (F, Dinv) on the host, after checking that the
    input and the slots the kernel has no business with come back bit for bit."""
    from awebox_amd.batched_lu import btd_factor
    Td = T.cuda()
    F, Dinv = btd_factor(Td)
    torch.cuda.synchronize()
    F, Dinv = F.cpu(), Dinv.cpu()
    assert _bits(torch, Td.cpu(), T)
    assert _bits(torch, F[:, :, 0], T[:, :, 0]) and _bits(torch, F[:, -1, 2], T[:, -1, 2])
    return F, Dinv


def _factor_shares(F, Dinv, T):
    """Shares of the factor bound of (D', W, Dinv), the worst over the batch."""
    shares = np.zeros(3)
    for b in range(T.shape[0]):
        Dp_ref, W_ref, Dinv_ref, kappa = bc.sweep_reference(T[b])
        got = (F[b, :, 1].numpy(), F[b, :-1, 2].numpy(), Dinv[b].numpy())
        ref = (Dp_ref, W_ref[:-1], Dinv_ref)
        shares = np.maximum(shares, [bc.factor_excess(g, r, kappa) for g, r in zip(got, ref)])
    return shares


@pytest.mark.parametrize("m", bc.BTD_M_EDGES)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_btd_factor_outputs_match_the_reference(gpu, family, m):
    """D'_k, W_k and Dinv_k of two members with three block rows at every tiling edge of m.
    Measured shares of the bound: at m = 1 sym 0.56 and perm_noise 0.44, at m = 2 sym 0.22 and
    perm_noise 0.11, from m = 8 on at most 0.05 (sym) and 0.02 (perm_noise)."""
    torch = gpu
    nb = bc.BTD_FACTOR_NB
    T = torch.stack([FAMILIES[family](nb, m, member=b) for b in range(bc.BTD_FACTOR_BATCH)])
    F, Dinv = _factor(torch, T)
    shares = _factor_shares(F, Dinv, T)
    print(f"factor {family}({nb}, {m}): share of the bound D' {shares[0]:.3f} W {shares[1]:.3f} Dinv {shares[2]:.3f}")
    assert shares.max() <= 1.0


def test_btd_factor_long_chain(gpu):
    """41 block rows of 46: the bound's condition number is the running maximum over the chain.
    Measured share of the bound: 0.007 (Dinv; W 0.004, D' below 0.001)."""
    torch = gpu
    nb, m = bc.BTD_LONG_CHAIN
    T = bc.sym(nb, m).unsqueeze(0)
    F, Dinv = _factor(torch, T)
    shares = _factor_shares(F, Dinv, T)
    print(f"factor sym({nb}, {m}): share of the bound D' {shares[0]:.3f} W {shares[1]:.3f} Dinv {shares[2]:.3f}")
    assert shares.max() <= 1.0


def _exact_case(torch, T, Dinv_want, W_want):
    """One block whose elimination is exact: Dinv and W as numbers equal the exact answers (a zero
    may carry either sign: 0 times a negative reciprocal), alone and with the identity tail."""
    m = T.shape[-1]
    eye = torch.eye(m, dtype=torch.float64)
    F, Dinv = _factor(torch, T.unsqueeze(0))
    assert torch.equal(Dinv[0, 0], Dinv_want) and torch.equal(F[0, 0, 1], T[0, 1])
    F, Dinv = _factor(torch, bc.with_tail(T).unsqueeze(0))
    assert torch.equal(Dinv[0, 0], Dinv_want) and torch.equal(F[0, 0, 2], W_want)
    assert torch.equal(F[0, :, 1], torch.stack([T[0, 1], eye])) and torch.equal(Dinv[0, 1], eye)


@pytest.mark.parametrize("m", [1, 2, 4, 8, 16, 32])
def test_btd_factor_exact_on_hadamard(gpu, m):
    """Every pivot search is an exact tie among all unused rows, within a lane, a wave and across the
    waves; with the lowest row winning, the elimination is exact: Dinv = H / m, W = H U / m."""
    _exact_case(gpu, *bc.hadamard(m))


def test_btd_factor_exact_on_scaled_permutations(gpu):
    """A signed permutation matrix times powers of two, at every m: the one non-zero of a column is
    the pivot wherever it lies (any lane, any wave), every multiplier is an exact zero and the final
    scatter through pivrow is the inverse permutation: Dinv = D^-1 and W = D^-1 U exactly."""
    for m in range(1, ac.read_constants()["kBtdMaxM"] + 1):
        _exact_case(gpu, *bc.perm_exact(m))


@pytest.mark.parametrize("m", bc.BTD_PIVOT_RULE_M)
def test_btd_factor_pivot_rule(gpu, m):
    """Column 0's maximum sits, bit for bit, in two rows of different waves: the lowest row must win.
    Dinv and W equal the exact float64 model of the loop (btd_cases.gj_model: the kernel's pivot
    rule, rp = 1 / pivot, pr = row rp, a = fma(-f, pr, a)) as numbers, so any other pivot order, and
    any other rounding, fails (test_btd_model.py: the highest wave on ties gives other factors).
    Measured: every entry equal, so the build contracts a - f pr to the fused operation the model
    assumes; a scratch build with `kw >= kb` in the cross-wave choice fails both cases."""
    torch = gpu
    T = bc.pivot_rule(m)
    W, Dinv, piv, ties = bc.gj_model(T[0, 1], T[0, 2])
    assert 0 in ties
    F, Dinv_gpu = _factor(torch, bc.with_tail(T).unsqueeze(0))
    shares = _factor_shares(F, Dinv_gpu, bc.with_tail(T).unsqueeze(0))
    print(f"pivot_rule({m}): share of the bound W {shares[1]:.3f} Dinv {shares[2]:.3f}; entries that differ from "
          f"the model: Dinv {int((Dinv_gpu[0, 0] != Dinv).sum())} W {int((F[0, 0, 2] != W).sum())}")
    assert shares.max() <= 1.0
    assert torch.equal(Dinv_gpu[0, 0], Dinv) and torch.equal(F[0, 0, 2], W)
    assert torch.equal(_factor(torch, T.unsqueeze(0))[1][0, 0], Dinv)


@pytest.mark.parametrize("family,nb,m", [("sym", bc.BTD_INERTIA_NB, m) for m in bc.BTD_INERTIA_M] +
                         [("alternating",) + bc.BTD_ALTERNATING])
def test_btd_inertia_from_the_stored_pivot_blocks(gpu, family, nb, m):
    """Haynsworth additivity, as BorderedBtd.inertia() uses it: the inertia kernel's counts of the
    stored D'_k, summed over k, are the eigenvalue counts of the assembled matrix.  sym's update
    L_k W_{k-1} is smaller than the gaps of D_k's spectrum, so D_k and D'_k have the same counts;
    in alternating the counts come from the update alone (every D_k is positive definite), so a
    block stored before its update is counted wrong."""
    torch = gpu
    from awebox_amd.batched_lu import btd_factor, sym_inertia
    T = torch.stack([getattr(bc, family)(nb, m, member=b) for b in range(2)])
    want = torch.stack([ac.inertia_reference(torch.tensor(bc.dense(T[b].numpy()))) for b in range(2)])
    assert bool((want[:, 2] == 0).all()) and bool((want[:, :2] > 0).all())      # indefinite, regular
    F, _ = btd_factor(T.cuda())
    counts = sym_inertia(F[:, :, 1].reshape(2 * nb, m, m), ztol=ac.ZTOL).view(2, nb, 3).sum(1)
    assert torch.equal(counts.cpu().to(torch.int32), want.to(torch.int32))


def test_bordered_btd_on_the_device(gpu):
    """btd.BorderedBtd on the device (the fused kernels): m = 13, nb = 4, a border of 3 unknowns, two
    unused block positions, duplicate entries.  .inertia() against the eigenvalues of the assembled
    matrix; .solve() against host LAPACK on it, within 8 eps kappa_inf(S) max|x|: the solve bound
    for the device path and as much again for LAPACK's own error (the bound is set by this
    reasoning, not by the measured share, 0.008)."""
    torch = gpu
    from awebox_amd.btd import BorderedBtd
    stage, pos, rows, cols, vals, S = bc.bordered_case()
    want = ac.inertia_reference(S)
    bt = BorderedBtd(stage, pos, 4, 13, rows, cols, "cuda")
    bt.factor(vals.cuda())
    assert bt.fused and bt.n_unused == 2 and bt.nG == 3
    assert torch.equal(bt.inertia()[0].cpu(), want.to(torch.int64))
    r = torch.randn(len(stage), generator=ac._gen(33), dtype=torch.float64)
    x_ref = torch.linalg.solve(S, r)
    bound = 8 * bc.EPS * np.linalg.cond(S.numpy(), np.inf) * x_ref.abs().max().item()
    err = (bt.solve(r.cuda()).cpu() - x_ref).abs().max().item()
    print(f"bordered: share of the bound {err / bound:.3f}")
    assert err <= bound


@pytest.mark.parametrize("m", bc.BTD_ISOLATION_M)
def test_btd_members_are_isolated(gpu, m):
    """A member with a zero D_0 and one with a NaN in D_1 (no finite pivot candidate: the waves
    publish their lowest unused row, key -1, or no row, key -2): both calls return, and the other
    members get the bits of their solo factorisation and solve."""
    torch = gpu
    from awebox_amd.batched_lu import btd_factor, btd_solve
    nb = 3
    T = torch.stack([bc.sym(nb, m, member=b) for b in range(5)])
    T[1, 0, 1] = 0.0
    T[3, 1, 1, m // 2, m - 1] = float("nan")
    X = torch.randn(5, nb, m, 3, generator=ac._gen(34, m), dtype=torch.float64).cuda()
    Td = T.cuda()
    F, Dinv = btd_factor(Td)
    x = btd_solve(F, Dinv, X)
    torch.cuda.synchronize()
    assert _bits(torch, Td.cpu(), T)
    assert not bool(torch.isfinite(Dinv[1, 0]).all()) and not bool(torch.isfinite(Dinv[3, 1]).all())
    assert bool(torch.isfinite(Dinv[3, 0]).all())         # the NaN's own member, the block before it
    for b in (0, 2, 4):
        F1, Dinv1 = btd_factor(Td[b:b + 1])
        assert _bits(torch, F1[0], F[b]) and _bits(torch, Dinv1[0], Dinv[b]), b
        assert _bits(torch, btd_solve(F1, Dinv1, X[b:b + 1])[0], x[b]), b
        assert bool(torch.isfinite(x[b]).all()) and bool(torch.isfinite(Dinv[b]).all())
    good = [0, 2, 4]
    assert _factor_shares(F[good].cpu(), Dinv[good].cpu(), T[good]).max() <= 1.0


@pytest.mark.parametrize("batch,nb,m,nrhs", bc.BTD_SOLVE_SHAPES)
def test_btd_solve_matches_the_reference(gpu, batch, nb, m, nrhs):
    """The solution of the first and the last member against the long-double dense solve, and the
    batch invariance the apply kernel promises: a column alone, a member alone
    (another chunk width: test_btd_model.py) and a repeat return the same bits.
    Measured share of the bound: at most 0.031 (0.007 to 0.031 over the six shapes)."""
    torch = gpu
    from awebox_amd.batched_lu import btd_factor, btd_solve
    w = bc.btd_chunk_width(ac.read_constants(), batch, nrhs)
    assert w == bc.BTD_SOLVE_WIDTHS[bc.BTD_SOLVE_SHAPES.index((batch, nb, m, nrhs))]
    T = torch.stack([bc.sym(nb, m, member=b) for b in range(batch)])
    X = torch.randn(batch, nb, m, nrhs, generator=ac._gen(35, batch, nrhs), dtype=torch.float64)
    Td, Xd = T.cuda(), X.cuda()
    F, Dinv = btd_factor(Td)
    x = btd_solve(F, Dinv, Xd)
    assert _bits(torch, btd_solve(F, Dinv, Xd), x) and _bits(torch, Xd.cpu(), X)
    xh = x.cpu()
    share = 0.0
    for b in sorted({0, batch - 1}):
        x_ref, kappa_T = bc.solve_reference(T[b], X[b])
        share = max(share, bc.solve_excess(xh[b].numpy(), x_ref, kappa_T))
    print(f"solve {(batch, nb, m, nrhs)}: chunk width {w}, share of the bound {share:.3f}")
    assert share <= 1.0
    for j in sorted({0, w - 1, min(w, nrhs - 1), nrhs - 1}):
        xj = btd_solve(F, Dinv, Xd[:, :, :, j:j + 1])
        assert _bits(torch, xj[..., 0], x[..., j]), j
    b = batch - 1
    F1, Dinv1 = btd_factor(Td[b:b + 1])
    assert _bits(torch, F1[0], F[b]) and _bits(torch, Dinv1[0], Dinv[b])
    assert _bits(torch, btd_solve(F1, Dinv1, Xd[b:b + 1])[0], x[b])


def test_btd_rejects_bad_arguments(gpu):
    """m = 49, nb = 0 and float32 raise without a launch; a valid call afterwards still works."""
    torch = gpu
    from awebox_amd.batched_lu import btd_factor, btd_solve
    mmax = ac.read_constants()["kBtdMaxM"]
    T, Dinv_want, _ = bc.perm_exact(4)
    F, Dinv = btd_factor(T.unsqueeze(0).cuda())
    f64 = torch.float64
    for bad in (torch.zeros(1, 1, 3, mmax + 1, mmax + 1, dtype=f64), torch.zeros(1, 0, 3, 4, 4, dtype=f64),
                T.unsqueeze(0).to(torch.float32)):
        with pytest.raises((ValueError, RuntimeError)):
            btd_factor(bad.cuda())
    with pytest.raises((ValueError, RuntimeError)):
        btd_solve(F, Dinv, torch.zeros(1, 1, 4, 2, dtype=torch.float32, device="cuda"))
    with pytest.raises((ValueError, RuntimeError)):
        btd_solve(F, Dinv, torch.zeros(1, 1, 5, 2, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    F, Dinv = btd_factor(T.unsqueeze(0).cuda())
    assert torch.equal(Dinv[0, 0].cpu(), Dinv_want)
    X = torch.ones(1, 1, 4, 2, dtype=torch.float64)
    assert torch.equal(btd_solve(F, Dinv, X.cuda()).cpu()[0, 0], Dinv_want @ X[0, 0])
