"""CPU checks behind the GPU tests of libawelu's inertia kernels.

tools/bk_blocked_model.py, the host model of sym_inertia_kernel's delayed-update Bunch-Kaufman
scheme, returns the eigenvalue counts on the structured matrix families of awelu_cases.py at panel
widths 4, 7 and 16: on these inputs (zero diagonal blocks, exact ties, exact zero columns) the
algorithm itself is right, so a GPU miscount on them is a kernel bug.  And the shape tables of the
GPU tests straddle every dispatch threshold of batched_lu.hip."""
import pytest
import torch

import awelu_cases as ac
from tools.bk_blocked_model import inertia_blocked

NB = (4, 7, 16)


def _check(A, want):
    ref = ac.inertia_reference(A, ac.ZTOL)
    assert tuple(ref.tolist()) == want                   # the construction and the eigenvalues agree
    for nb in NB:
        assert inertia_blocked(A.numpy(), ztol=ac.ZTOL, nb=nb) == want, nb


@pytest.mark.parametrize("n1,m", [(2, 1), (2, 2), (40, 23), (84, 42), (130, 69), (171, 86)])
@pytest.mark.parametrize("dup", [0, 1])
@pytest.mark.parametrize("perm", [0, 1])
def test_model_counts_saddle(n1, m, dup, perm):
    A, want = ac.saddle(n1, m, dup, perm)
    assert want == ((n1, m - 1, 1) if dup and m > 1 else (n1, m, 0))
    _check(A, want)


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65])
@pytest.mark.parametrize("family", [ac.antidiag, ac.zero, ac.diagonal])
def test_model_counts_ties_and_zeros(family, n):
    _check(*family(n))


@pytest.mark.parametrize("n", [2, 16, 64])
def test_model_counts_hadamard(n):
    _check(*ac.hadamard(n))


def test_families_are_reproducible_and_symmetric():
    for n in (3, 65):
        names, A, want = ac.inertia_families(n)
        assert torch.equal(A, ac.inertia_families(n)[1])
        assert torch.equal(A, A.transpose(1, 2))
        assert torch.equal(ac.inertia_reference(A), want), names


def test_reference_rejects_an_ambiguous_matrix():
    A = torch.diag(torch.tensor([1.0, 1e-12], dtype=torch.float64))      # neither zero nor non-zero
    with pytest.raises(AssertionError):
        ac.inertia_reference(A, ac.ZTOL)


def test_gpu_shape_tables_straddle_the_dispatch_thresholds():
    """If a threshold of batched_lu.hip is retuned, this says which GPU cases to move."""
    c = ac.read_constants()
    for name in ("kNB", "kThreads", "kLuSmallN", "kLuSmallMinBatch", "kMaxN", "kSyNB", "kSyLds", "kSyBlockedMinN",
                 "kSolveLds", "kSolveTargetWgs", "kSolveMinChunk"):
        assert name in c, name
    nb, nt, nmax = c["kNB"], c["kThreads"], c["kMaxN"]
    from awebox_amd.batched_lu import MAX_N
    assert MAX_N == nmax

    # LU panels: one panel less a column, exactly one, two, two plus a column; the thread count
    # (one trailing column per thread) from both sides; the largest size and the first rejected one
    lu = set(ac.LU_EDGE_SIZES)
    assert {nb - 1, nb, 2 * nb, 2 * nb + 1, nt - 1, nt, nt + 1, nmax} <= lu
    assert ac.LU_REJECTED_N == nmax + 1
    # lu_batched_kernel<128>: n at and beyond kLuSmallN at the smallest batch that selects it; the
    # halves and the batch less one stay on <256>
    sm = set(ac.LU_SMALL_SIZES)
    assert ac.LU_SMALL_BATCH == c["kLuSmallMinBatch"] and ac.LU_SMALL_BATCH // 2 < c["kLuSmallMinBatch"]
    assert {c["kLuSmallN"], c["kLuSmallN"] + 1} <= sm and min(sm) == 1
    assert any(n % nb and n < c["kLuSmallN"] for n in sm)
    assert all(n <= nmax for n in lu | sm | set(ac.LU_HADAMARD_SIZES))
    assert any(n > nt for n in ac.LU_HADAMARD_SIZES) and nb in ac.LU_HADAMARD_SIZES

    # solve: the LDS cap binds at kMaxN (cap < nrhs, several chunks of one launch); a single chunk
    # of exactly kSolveMinChunk + 1 columns and two chunks; a batch beyond kSolveTargetWgs
    widths = {s: ac.solve_chunk_width(c, *s) for s in ac.SOLVE_SHAPES + ac.SOLVE_COLUMN_SHAPES}
    assert all(1 <= w <= cap for w, cap in widths.values())
    assert any(n == nmax and cap < nrhs and w == cap for (b, n, nrhs), (w, cap) in widths.items())
    assert any(nrhs == c["kSolveMinChunk"] + 1 and w < nrhs for (b, n, nrhs), (w, cap) in widths.items())
    assert any(b > c["kSolveTargetWgs"] for b, n, nrhs in ac.SOLVE_SHAPES)
    for s in ac.SOLVE_COLUMN_SHAPES:                     # column w - 1 and column w are in two chunks
        assert widths[s][0] < s[2]

    # inertia: both kernels at their common boundary, the wave and workgroup sizes, narrow panels
    sy = set(ac.INERTIA_SIZES)
    lim = c["kSyBlockedMinN"]
    assert {lim - 1, lim, lim + 1, 63, 64, 65, nt - 1, nt, nt + 1} <= sy
    assert min(sy) == 1 and max(sy) > 2 * nt
    assert all(ac.inertia_panel_width(c, n) == c["kSyNB"] for n in sy)
    narrow = [ac.inertia_panel_width(c, n1 + m) for n1, m in ac.INERTIA_NARROW]
    assert len(set(narrow)) == len(narrow) > 1 and all(4 <= w < c["kSyNB"] for w in narrow)
    assert ac.inertia_panel_width(c, ac.INERTIA_REJECTED_N) < 4 <= ac.inertia_panel_width(c, ac.INERTIA_REJECTED_N - 1)
