"""CPU checks behind the GPU tests of libawelu's block-tridiagonal kernels (test_btd_gpu.py).

The bounds of the GPU tests are conditions the inputs must allow: a float64 restatement of the
sweep and of the apply (numpy, the kernels' recursion with the apply's refinement step) stays
within a quarter of them against the long-double reference, so a kernel beyond a bound is wrong and
not unlucky.  Measured shares of the bounds over the shapes below: factor 0.039 (sym) and 0.003
(perm_noise), solve 0.022 (sym) and 0.001 (perm_noise).  The exact model of the Gauss-Jordan loop
(btd_cases.gj_model) meets the same bound, returns the exact answers on the exact families, and
tells the lowest-row tie rule from the broken one on the pivot-rule matrices.  And the shape tables
straddle every edge of the kernels' tiling and of the solve's chunking."""
import numpy as np
import pytest
import torch

import awelu_cases as ac
import btd_cases as bc

SHAPES = [(5, 7), (9, 13), (21, 22), (7, 48)]
FAMILIES = [bc.sym, bc.perm_noise]


def sweep_f64(T):
    """btd_factor_kernel's recursion in float64: (D', W, Dinv)."""
    T = np.asarray(T)
    nb, _, m, _ = T.shape
    Dp, W, Dinv = (np.zeros((nb, m, m)) for _ in range(3))
    for k in range(nb):
        Dp[k] = T[k, 1] - T[k, 0] @ W[k - 1] if k > 0 else T[k, 1]
        S = bc._gauss_jordan(Dp[k], np.concatenate([T[k, 2], np.eye(m)], axis=1))
        if k < nb - 1:
            W[k] = S[:, :m]
        Dinv[k] = S[:, m:]
    return Dp, W, Dinv


def apply_f64(T, Dp, W, Dinv, X):
    """btd_apply_kernel's two sweeps in float64, with its one refinement step per block solve."""
    T, X = np.asarray(T), np.asarray(X)
    nb = T.shape[0]
    Y = np.zeros_like(X)
    for k in range(nb):
        Z = X[k] - T[k, 0] @ Y[k - 1] if k > 0 else X[k]
        Y[k] = Dinv[k] @ Z
        Y[k] = Y[k] + Dinv[k] @ (Z - Dp[k] @ Y[k])
    for k in range(nb - 2, -1, -1):
        Y[k] = Y[k] - W[k] @ Y[k + 1]
    return Y


@pytest.fixture(scope="module")
def references():
    out = {}
    for family in FAMILIES:
        for nb, m in SHAPES:
            T = family(nb, m)
            out[family.__name__, nb, m] = (T, bc.sweep_reference(T))
    return out


@pytest.mark.parametrize("nb,m", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_float64_sweep_within_a_quarter_of_the_factor_bound(references, family, nb, m):
    T, (Dp_ref, W_ref, Dinv_ref, kappa) = references[family.__name__, nb, m]
    Dp, W, Dinv = sweep_f64(T.numpy())
    shares = [bc.factor_excess(got, ref, kappa) for got, ref in ((Dp, Dp_ref), (W[:-1], W_ref[:-1]), (Dinv, Dinv_ref))]
    print(f"{family.__name__}({nb}, {m}): share of the factor bound D' {shares[0]:.3f} W {shares[1]:.3f} "
          f"Dinv {shares[2]:.3f}, kappa {kappa[-1]:.1f}")
    assert max(shares) <= 0.25


@pytest.mark.parametrize("nb,m", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_float64_apply_within_a_quarter_of_the_solve_bound(references, family, nb, m):
    T, _ = references[family.__name__, nb, m]
    X = torch.randn(nb, m, 3, generator=ac._gen(31, nb, m), dtype=torch.float64)
    x_ref, kappa_T = bc.solve_reference(T, X, max_n=21 * 22)
    x = apply_f64(T.numpy(), *sweep_f64(T.numpy()), X.numpy())
    share = bc.solve_excess(x, x_ref, kappa_T)
    print(f"{family.__name__}({nb}, {m}): share of the solve bound {share:.3f}, kappa_inf(T) {kappa_T:.1f}")
    assert share <= 0.25


def test_solve_reference_agrees_with_the_sweep_reference():
    """The two long-double references are independent algorithms (dense elimination, block
    recursion): the recursion's solution from its own factors matches the dense one far inside the
    float64 bound.  Each carries about n eps_ld kappa with eps_ld = 2^-11 eps and n = 35, which is
    n 2^-11 / 4 = 0.004 of 4 eps kappa: 2^-6 for the two."""
    T = bc.sym(5, 7)
    X = torch.randn(5, 7, 2, generator=ac._gen(32), dtype=torch.float64)
    x_ref, kappa_T = bc.solve_reference(T, X)
    Dp, W, Dinv, _ = bc.sweep_reference(T)
    Tl, Y = T.numpy().astype(bc.LD), X.numpy().astype(bc.LD)
    for k in range(5):
        Y[k] = Dinv[k] @ (Y[k] - Tl[k, 0] @ Y[k - 1] if k > 0 else Y[k])
    for k in range(3, -1, -1):
        Y[k] = Y[k] - W[k] @ Y[k + 1]
    assert bc.solve_excess(Y, x_ref, kappa_T) <= 2.0 ** -6


@pytest.mark.parametrize("m", [1, 7, 13, bc.BTD_MODEL_MAX_M])
@pytest.mark.parametrize("family", FAMILIES)
def test_gj_model_within_the_factor_bound(family, m):
    """Measured: at most 0.023 of the bound from m = 7 on."""
    T = bc.with_tail(family(1, m))
    _, W_ref, Dinv_ref, kappa = bc.sweep_reference(T)
    W, Dinv, piv, _ = bc.gj_model(T[0, 1], T[0, 2])
    assert sorted(piv) == list(range(m))
    shares = (bc.factor_excess(W[None].numpy(), W_ref[:1], kappa), bc.factor_excess(Dinv[None].numpy(), Dinv_ref[:1], kappa))
    print(f"gj_model on {family.__name__}(1, {m}): share of the factor bound W {shares[0]:.3f} Dinv {shares[1]:.3f}")
    # m = 1: W = U (1 / D) is two roundings, up to 2 (eps / 2) |W|, which is the whole bound
    # (m = kappa = 1); no float64 code has a quarter of it to spare there (measured 0.44)
    assert max(shares) <= (1.0 if m == 1 else 0.25)


@pytest.mark.parametrize("m", [1, 2, 4, 8, 16])
def test_gj_model_exact_on_hadamard(m):
    T, Dinv, W = bc.hadamard(m)
    Wm, Dm, piv, ties = bc.gj_model(T[0, 1], T[0, 2])
    assert torch.equal(Dm, Dinv) and torch.equal(Wm, W)
    assert torch.equal(Dinv @ T[0, 1], torch.eye(m, dtype=torch.float64))
    assert m <= 12 or ties                                # beyond one wave's rows the waves tie


@pytest.mark.parametrize("m", [1, 2, 12, 13, bc.BTD_MODEL_MAX_M])
def test_gj_model_exact_on_perm_exact(m):
    T, Dinv, W = bc.perm_exact(m)
    Wm, Dm, piv, _ = bc.gj_model(T[0, 1], T[0, 2])
    assert torch.equal(Dm, Dinv) and torch.equal(Wm, W)
    assert torch.equal(Dinv @ T[0, 1], torch.eye(m, dtype=torch.float64))
    assert torch.equal(T[0, 1] @ W, T[0, 2])


@pytest.mark.parametrize("m", bc.BTD_PIVOT_RULE_M)
def test_pivot_rule_matrices_tell_the_tie_rules_apart(m):
    """Column 0's maximum sits in two rows of different waves, bit for bit; the model sees exact
    cross-wave ties, and with the highest wave winning them it returns other factors: a kernel with
    that rule fails the GPU test's bitwise comparison.  Both rules stay within the factor bound (the
    bound alone cannot tell them apart)."""
    T = bc.pivot_rule(m)
    D = T[0, 1]
    top = torch.nonzero(D[:, 0].abs() == D[:, 0].abs().max()).flatten().tolist()
    assert len(top) == 2 and top[0] // 12 != top[1] // 12
    W, Dinv, piv, ties = bc.gj_model(D, T[0, 2])
    W2, Dinv2, piv2, _ = bc.gj_model(D, T[0, 2], highest_wave_on_ties=True)
    assert 0 in ties and piv[0] == top[0] and piv2[0] == top[1]
    assert not torch.equal(Dinv, Dinv2) and not torch.equal(W, W2)
    _, W_ref, Dinv_ref, kappa = bc.sweep_reference(bc.with_tail(T))
    assert kappa[0] <= 1e3
    for Wx, Dx in ((W, Dinv), (W2, Dinv2)):
        assert bc.factor_excess(Wx[None].numpy(), W_ref[:1], kappa) <= 0.25
        assert bc.factor_excess(Dx[None].numpy(), Dinv_ref[:1], kappa) <= 0.25
    print(f"pivot_rule({m}): kappa {kappa[0]:.1f}, exact cross-wave ties at columns {ties}")


def test_families_are_reproducible():
    for family in FAMILIES:
        assert torch.equal(family(3, 13), family(3, 13))
        assert not torch.equal(family(3, 13)[0], family(4, 13)[0])
    for family in (bc.perm_exact, bc.hadamard):
        assert all(torch.equal(a, b) for a, b in zip(family(8), family(8)))
    assert torch.equal(bc.pivot_rule(13), bc.pivot_rule(13))
    c1, c2 = bc.bordered_case(), bc.bordered_case()
    assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(c1, c2))


@pytest.mark.parametrize("nb,m", [(5, 12), (5, 13), (5, 48), (3, 1), (9, 25)])
def test_sym_inertia_is_unambiguous(nb, m):
    """sym's dense matrix passes inertia_reference's test (smallest |eigenvalue| about 1.8), and the
    reference sweep's pivot blocks add up to the same counts (Haynsworth additivity)."""
    from awebox_amd.batched_lu import sym_inertia_host
    T = bc.sym(nb, m)
    A = torch.tensor(bc.dense(T.numpy()))
    assert torch.equal(A, A.T)
    want = ac.inertia_reference(A)
    assert int(want[2]) == 0 and torch.linalg.eigvalsh(A).abs().min().item() > 1.0
    Dp = torch.tensor(bc.sweep_reference(T)[0].astype(np.float64))
    assert torch.equal(sym_inertia_host(Dp).sum(0), want)


def test_alternating_inertia_comes_from_the_update():
    """alternating's D_k are all positive definite, its pivot blocks are positive, negative and
    positive definite: the counts of the D_k (a factorisation that stored the block before its
    update) miss the matrix's, the reference sweep's D'_k give them.  Both members of the GPU test."""
    from awebox_amd.batched_lu import sym_inertia_host
    nb, m = bc.BTD_ALTERNATING
    for member in range(2):
        T = bc.alternating(nb, m, member=member)
        want = ac.inertia_reference(torch.tensor(bc.dense(T.numpy())))
        assert want.tolist() == [2 * m, m, 0]
        assert sym_inertia_host(T[:, 1]).sum(0).tolist() == [nb * m, 0, 0]
        Dp, _, _, kappa = bc.sweep_reference(T)
        Dp = torch.tensor(Dp.astype(np.float64))
        assert sym_inertia_host(Dp).tolist() == [[m, 0, 0], [0, m, 0], [m, 0, 0]]
        ev = torch.linalg.eigvalsh(0.5 * (Dp + Dp.transpose(1, 2)))
        assert kappa[-1] <= 10 and 2.0 <= ev.abs().min().item() and ev.abs().max().item() <= 15.2


def test_bordered_case_on_the_host():
    """The BorderedBtd case of the GPU test through the host path (LAPACK blocks): its inertia is
    unambiguous and equals BorderedBtd's, and the solve matches the dense one.  So the case itself
    is sound where the device path is compared with the same references."""
    from awebox_amd.btd import BorderedBtd
    stage, pos, rows, cols, vals, S = bc.bordered_case()
    assert int((stage < 0).sum()) == 3 and len(stage) == 4 * 13 - 2 + 3
    assert len(set(zip(rows.tolist(), cols.tolist()))) < len(rows)       # duplicates
    assert torch.equal(S, S.T)
    want = ac.inertia_reference(S)
    bt = BorderedBtd(stage, pos, 4, 13, rows, cols, "cpu")
    assert bt.n_unused == 2
    bt.factor(vals)
    assert torch.equal(bt.inertia()[0], want.to(torch.int64))
    r = torch.randn(len(stage), generator=ac._gen(33), dtype=torch.float64)
    x_ref = torch.linalg.solve(S, r)
    kappa = np.linalg.cond(S.numpy(), np.inf)
    assert (bt.solve(r) - x_ref).abs().max().item() <= 8 * bc.EPS * kappa * x_ref.abs().max().item()


def test_gpu_shape_tables_straddle_the_tiling_edges():
    """If the tiling of btd_factor_kernel or the chunking of awelu_btd_solve_batched is retuned, this
    says which GPU cases to move."""
    c = ac.read_constants()
    for name in ("kThreads", "kBtdMaxM", "kBtdMaxRhs"):
        assert name in c, name
    from awebox_amd.batched_lu import BTD_MAX_M
    mmax, wmax = c["kBtdMaxM"], c["kBtdMaxRhs"]
    assert BTD_MAX_M == mmax
    rows_wave, rows_lane, cols_lane = bc.btd_tiles(c)
    assert (rows_wave, rows_lane, cols_lane) == (12, 3, 9)               # gj_model's rows_wave, pivot_rule's 13
    edges = set(bc.BTD_M_EDGES)
    assert max(edges) == mmax and {1, 2, mmax - 1} <= edges
    # a lane's rows, a wave's rows (one, two and three waves full, and one row more), the pivot
    # columns of one to four column groups and one column more
    assert {rows_lane, rows_lane + 1} <= edges
    assert {q * rows_wave + d for q in (1, 2, 3) for d in (0, 1)} | {rows_wave - 1} <= edges
    assert {q * cols_lane + d for q in (1, 2, 3, 4) for d in (0, 1)} | {cols_lane - 1} <= edges
    # 3 m columns over tiles of 9: blocks whose [D' | U | I] ends inside a lane's tile or leaves
    # whole column groups empty, and U and I starting inside a tile
    assert any(3 * m % cols_lane for m in edges) and any(m % cols_lane for m in edges)
    assert any(3 * m <= 15 * cols_lane for m in edges) and 3 * mmax == 16 * cols_lane
    nb, m = bc.BTD_LONG_CHAIN
    assert nb > 9 and 3 * rows_wave < m < mmax and m % cols_lane and m not in edges
    assert all(m <= bc.BTD_MODEL_MAX_M and m - 1 in (rows_wave, 2 * rows_wave) for m in bc.BTD_PIVOT_RULE_M)
    assert {rows_wave, rows_wave + 1, mmax} == set(bc.BTD_INERTIA_M)
    assert {rows_wave + 1, mmax} == set(bc.BTD_ISOLATION_M)

    # the solve: w = 1, 1 < w < kBtdMaxRhs, w = kBtdMaxRhs, a ragged last chunk, more than one pass
    # of 64, a batch beyond the target workgroup count, and the solo call on another width
    widths = [bc.btd_chunk_width(c, b, nrhs) for b, nb, m, nrhs in bc.BTD_SOLVE_SHAPES]
    assert tuple(widths) == bc.BTD_SOLVE_WIDTHS
    assert 1 in widths and wmax in widths and any(1 < w < wmax for w in widths)
    assert any(nrhs % w for (b, nb, m, nrhs), w in zip(bc.BTD_SOLVE_SHAPES, widths))
    assert any(nrhs > wmax and b == 1 for b, nb, m, nrhs in bc.BTD_SOLVE_SHAPES)
    assert any(b > bc.BTD_SOLVE_TARGET_WGS for b, nb, m, nrhs in bc.BTD_SOLVE_SHAPES)
    assert any(m == mmax for b, nb, m, nrhs in bc.BTD_SOLVE_SHAPES)
    for (b, nb, m, nrhs), w in zip(bc.BTD_SOLVE_SHAPES, widths):
        assert nb * m <= 240 and b <= 300
        assert b == 1 or bc.btd_chunk_width(c, 1, nrhs) != w
