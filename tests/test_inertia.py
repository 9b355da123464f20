"""Inertia of the structured KKT matrix (IPOPT's inertia correction, ipm.IpmOptions(inertia="exact")).

CPU: StructuredKKT.inertia (Haynsworth additivity over the interval blocks and the dense or
block-tridiagonal separator system) equals the eigenvalue counts of the assembled K.
GPU: the Bunch-Kaufman kernel (awelu_sym_inertia_batched) equals symmetric eigenvalue counts on
random indefinite and rank-deficient matrices, and the structured counts on the device equal the
host ones; both inertia kernels equal the eigenvalue counts on the structured families of
awelu_cases.py (saddle points, exact ties, exact zeros) at the sizes where the host dispatch changes
kernel or panel width, alone as in a batch, reading the lower triangle only."""
import functools

import numpy as np
import pytest
import torch

import awelu_cases as ac
from awebox_amd import homotopy as hm
from awebox_amd import problem as pb
from awebox_amd.initial_guess import initial_guess


def _case(device, evaluator, n_k=5, d=3, shift=0.0):
    from awebox_amd.ipm import DeviceNlp, StructuredKKT, _dense_A
    consts = pb.build_constants(pb.Ap2Config(n_k=n_k, d=d))
    lay = pb.NlpLayout(n_k, d)
    v0 = initial_guess(consts, lay)
    st = hm.schedule(consts, lay, v0)[0]
    lbg, ubg = lay.g_bounds()
    nlp = DeviceNlp(evaluator(consts), pb.pack_p(lay, consts, v0, step=st.cost_step), st.lbx, st.ubx,
                    lbg, ubg, device)
    sk = StructuredKKT(nlp, lay, device, separators="btd")
    gen = torch.Generator().manual_seed(2)
    f64 = dict(dtype=torch.float64)
    hv = torch.randn(len(nlp.h_keep), generator=gen, **f64).to(device)
    jv = torch.randn(len(nlp.j_row), generator=gen, **f64).to(device)
    diag = (torch.rand(nlp.ny, generator=gen, **f64) + shift).to(device)
    N, ny = sk.N, nlp.ny
    K = torch.zeros(N, N, dtype=torch.float64, device=device)
    K[nlp.h_r, nlp.h_c] = hv
    K[nlp.h_c[nlp.h_offdiag], nlp.h_r[nlp.h_offdiag]] = hv[nlp.h_offdiag]
    i = torch.arange(ny, device=device)
    K[i, i] += diag
    _dense_A(nlp, jv, ny, K)
    return nlp, sk, hv, jv, diag, K


def _eig_counts(K):
    ev = torch.linalg.eigvalsh(K.cpu())
    tol = 1e-10 * ev.abs().max()
    return int((ev > tol).sum()), int((ev < -tol).sum()), int(((ev >= -tol) & (ev <= tol)).sum())


@pytest.mark.parametrize("btd,shift", [(False, 0.0), (True, 0.0), (False, 50.0), (True, 50.0)])
def test_structured_inertia_matches_eigenvalues(btd, shift):
    from oracle.cpu_device import CpuDeviceEvaluator
    nlp, sk, hv, jv, diag, K = _case("cpu", CpuDeviceEvaluator, shift=shift)
    sk.force_btd = btd
    sk.factor(hv, diag, jv, 0.0, nlp.mI)
    assert sk.use_btd == btd
    assert sk.inertia() == _eig_counts(K)


@pytest.mark.gpu
def test_bunch_kaufman_inertia_kernel():
    from awebox_amd.batched_lu import sym_inertia, sym_inertia_host
    gen = torch.Generator().manual_seed(3)
    for n, b in ((1, 3), (7, 5), (46, 41), (268, 8), (500, 2)):
        A = torch.randn(b, n, n, generator=gen, dtype=torch.float64)
        A = A + A.transpose(1, 2)
        if n > 2:                                   # rank-deficient members: zero eigenvalues
            U = torch.randn(n, n - 2, generator=gen, dtype=torch.float64)
            A[0] = U @ torch.diag(torch.linspace(-3, 2, n - 2, dtype=torch.float64)) @ U.T
        c = sym_inertia(A.cuda(), ztol=1e-11).cpu()
        ref = sym_inertia_host(A, ztol=1e-11)
        assert torch.equal(c, ref), (n, c, ref)


@functools.lru_cache(maxsize=None)
def _families_once(n):
    names, A, want = ac.inertia_families(n)
    ref = ac.inertia_reference(A, ac.ZTOL)
    assert torch.equal(ref, want), (n, names, ref, want)   # the construction and the eigenvalues agree
    return tuple(names), A, ref


def _families(n):
    """awelu_cases' families at size n with the eigenvalue reference, computed once; every caller
    gets copies of its own, so an in-place edit in one test cannot reach another's inputs."""
    names, A, ref = _families_once(n)
    return names, A.clone(), ref.clone()


def _wrong(names, got, ref):
    return [(nm, g.tolist(), r.tolist()) for nm, g, r in zip(names, got, ref) if not torch.equal(g, r)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", ac.INERTIA_SIZES)
def test_inertia_structured_families(n):
    """Saddle points (zero diagonal blocks: 2 x 2 pivots; a duplicated constraint: an exact zero
    eigenvalue), exact ties, exact zero columns and a rank-deficient congruence in one batch, so the
    workgroups of one launch take different pivot paths; sizes around the wave, the workgroup and
    the unblocked / blocked boundary (199, 200)."""
    from awebox_amd.batched_lu import sym_inertia
    names, A, ref = _families(n)
    got = sym_inertia(A.cuda(), ztol=ac.ZTOL).cpu()
    assert not _wrong(names, got, ref), n


@pytest.mark.gpu
@pytest.mark.parametrize("n", ac.INERTIA_SIZES)
def test_inertia_member_alone_as_in_batch(n):
    from awebox_amd.batched_lu import sym_inertia
    names, A, ref = _families(n)
    Ad = A.cuda()
    got = torch.cat([sym_inertia(Ad[b:b + 1], ztol=ac.ZTOL) for b in range(len(names))]).cpu()
    assert torch.equal(got, sym_inertia(Ad, ztol=ac.ZTOL).cpu())
    assert not _wrong(names, got, ref), n


@pytest.mark.gpu
@pytest.mark.parametrize("n1,m", ac.INERTIA_NARROW)
def test_inertia_narrow_panels(n1, m):
    """Beyond 1200 rows the blocked kernel's panel has fewer than 16 columns (15 at 1210 rows, 9 at
    1930): its `j < nb - 1` loop bound and the two free slots of a 2 x 2 pivot with nb != 16."""
    from awebox_amd.batched_lu import sym_inertia
    cases = [ac.saddle(n1, m, dup, 1) for dup in (0, 1)]
    A = torch.stack([c[0] for c in cases])
    ref = ac.inertia_reference(A, ac.ZTOL)
    assert ref.tolist() == [list(c[1]) for c in cases]
    got = sym_inertia(A.cuda(), ztol=ac.ZTOL).cpu()
    assert torch.equal(got, ref), (got, ref)


@pytest.mark.gpu
def test_inertia_large_grid_same_counts():
    from awebox_amd.batched_lu import sym_inertia
    A, want = ac.saddle(84, 42, 1, 1)
    assert tuple(ac.inertia_reference(A, ac.ZTOL).tolist()) == want
    got = sym_inertia(A.unsqueeze(0).repeat(300, 1, 1).cuda(), ztol=ac.ZTOL).cpu()
    assert torch.equal(got, torch.tensor(want, dtype=torch.int32).expand(300, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [126, 268])
def test_inertia_reads_the_lower_triangle_only(n):
    """NaN in the strict upper triangle changes nothing (both kernels), and the caller's tensor is
    left as it was."""
    from awebox_amd.batched_lu import sym_inertia
    names, A, ref = _families(n)
    upper = torch.triu(torch.ones(n, n, dtype=torch.bool), diagonal=1)
    Ad = A.clone().masked_fill_(upper, float("nan")).cuda()
    before = Ad.clone()
    got = sym_inertia(Ad, ztol=ac.ZTOL).cpu()
    assert torch.equal(Ad.view(torch.int64), before.view(torch.int64))
    assert not _wrong(names, got, ref), n


@pytest.mark.gpu
def test_inertia_rejects_n_beyond_the_panel_budget():
    from awebox_amd.batched_lu import sym_inertia
    n = ac.INERTIA_REJECTED_N
    A = torch.ones(1, n, n, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match=r"1 <= n <= 4800"):
        sym_inertia(A, ztol=ac.ZTOL)
    torch.cuda.synchronize()
    assert bool((A == 1.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0.0, 50.0])
def test_structured_inertia_on_gpu(shift):
    from awebox_amd.evaluator import Ap2Evaluator
    nlp, sk, hv, jv, diag, K = _case("cuda", lambda c: Ap2Evaluator(c, batch=1), shift=shift)
    ref = _eig_counts(K)
    for sep in ("btd", "dense"):
        sk.btd_off = sep == "dense"
        sk.factor(hv, diag, jv, 0.0, nlp.mI)
        assert sk.inertia() == ref, sep
