"""The reference-window kernel (awempc.hip: mpc_ref_window_kernel) on the MI355X.

The kernel and ``mpc.reference_window_cpu`` run the same core (csrc/ref_pp.hpp): the same IEEE operations
in the same order, contraction off and explicit fma's on both sides, so they are compared bitwise.  Then:
a loop's window does not depend on the batch, a NaN start time stays in its loop, a window written into
P in place leaves the rest of P alone; the closed loop tracking ``from_simulation`` on aligned phases
reproduces the ``simulate_reference`` mode step by step, and between the nodes (spline) it runs on past the
stored trajectory's former end.
"""
import numpy as np
import pytest
import torch

from awebox_amd import kite3 as k3
from awebox_amd import mpc
from awebox_amd.reference import PeriodicTrajectory
from awebox_amd.rti import BatchedRti
from test_reference_interp import KINDS, TRAJ_GRIDS, aligned_loop, close, consts_lay, perturbed_circle, time_list

pytestmark = pytest.mark.gpu
GPU_SHAPES = ((3, 2), (20, 4))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from awebox_amd.build import build
    build()
    return torch.device("cuda:0")


_EVALUATORS = {}


def evaluator(shape, B):
    if (shape, B) not in _EVALUATORS:
        c, lay = consts_lay(*shape)
        _EVALUATORS[shape, B] = (c, lay, mpc.MpcEvaluator(c, batch=B))
    return _EVALUATORS[shape, B]


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("grid", TRAJ_GRIDS)
@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_kernel_equals_host_core_bitwise(gpu, kind, grid, shape):
    for B in (130, 3):
        c, lay, ev = evaluator(shape, B)
        tab = perturbed_circle(c, *grid).tables(kind)
        ev.set_reference(tab)
        times = time_list(tab["period"])
        if B == 130:
            batches = [np.concatenate([times, np.random.default_rng(1).uniform(0, 2 * tab["period"], B - len(times))])]
        else:
            batches = [np.resize(times[i:i + B], B) for i in range(0, len(times), B)]
        for t0 in batches:
            got = ev.reference_window(torch.tensor(t0, device=gpu)).cpu().numpy()
            want = mpc.reference_window_cpu(tab, t0, lay, c)
            diff = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
            assert len(diff) == 0, (B, len(diff), diff[:4], float(np.abs(got - want).max()))


def test_window_is_independent_of_the_batch(gpu):
    shape = (20, 4)
    c, lay, ev = evaluator(shape, 130)
    _, _, ev1 = evaluator(shape, 1)
    tab = perturbed_circle(c, 12, 4).tables("spline")
    ev.set_reference(tab), ev1.set_reference(tab)
    t0 = torch.tensor(np.random.default_rng(2).uniform(0, 3 * tab["period"], 130), device=gpu)
    R = ev.reference_window(t0).cpu().numpy()
    for i in (0, 63, 64, 129):
        assert same_bits(R[i], ev1.reference_window(t0[i:i + 1].clone()).cpu().numpy()[0])
    t_nan = t0.clone()
    t_nan[64] = float("nan")
    Rn = ev.reference_window(t_nan).cpu().numpy()
    keep = np.arange(130) != 64
    assert same_bits(Rn[keep], R[keep])
    assert np.isnan(Rn[64, lay.x(0)]).all() and np.isnan(Rn[64, lay.coll_x(19, 3)]).all()


def test_window_written_into_p_in_place(gpu):
    c, lay, ev = evaluator((20, 4), 130)
    tab = perturbed_circle(c, 5, 3).tables("poly")
    ev.set_reference(tab)
    t0 = torch.tensor(np.random.default_rng(4).uniform(0, tab["period"], 130), device=gpu)
    P = torch.randn(130, lay.n_p, dtype=torch.float64, device=gpu)
    P0 = P.clone()
    ev.reference_window(t0, out=P, ld=lay.n_p, off=lay.p_ref)
    ref = slice(lay.p_ref, lay.p_ref + lay.n_v)
    assert same_bits(P[:, ref].cpu().numpy().copy(), ev.reference_window(t0).cpu().numpy())
    P0[:, ref] = P[:, ref]
    assert same_bits(P.cpu().numpy(), P0.cpu().numpy())
    assert ev.last_ref_ms() > 0.0


def _gpu_loop(c, B):
    return BatchedRti(c, B, device="cuda")


def test_closed_loop_on_aligned_phases_equals_the_simulated_mode(gpu):
    """(N, d, B) = (10, 4, 8), ts = 0.125, poly: V and x0 after each of 10 steps."""
    n_nodes = 22
    _, a = aligned_loop(_gpu_loop, n_nodes, n_k=10, d=4, B=8)
    c, b = aligned_loop(_gpu_loop, n_nodes, n_k=10, d=4, B=8)
    lay = b.lay
    b.track(PeriodicTrajectory.from_simulation(b), "poly", t0=np.zeros(8))
    assert close(b.V.cpu().numpy(), a.V.cpu().numpy())
    for s in range(10):
        a.step(), b.step()
        va, vb = a.V.cpu().numpy(), b.V.cpu().numpy()
        xa, xb = a.P[:, :k3.NX].cpu().numpy(), b.P[:, :k3.NX].cpu().numpy()
        print("step", s, "V gap", float(np.abs(va - vb).max()), "x0 gap", float(np.abs(xa - xb).max()))
        assert close(vb, va) and close(xb, xa), s


def test_closed_loop_between_the_nodes(gpu):
    """The same loops started 0.37 ts after the nodes, spline: 25 steps, past the stored trajectory's end."""
    n_nodes = 22
    c, b = aligned_loop(_gpu_loop, n_nodes, n_k=10, d=4, B=8)
    b.track(PeriodicTrajectory.from_simulation(b), "spline", t0=np.full(8, 0.37 * 0.125))
    for s in range(25):
        out = b.step()
        print("step", s, "eq", float(out["eq_residual"].max()), "plant", float(out["plant_residual"].max()))
        assert torch.isfinite(out["eq_residual"]).all() and bool(out["plant_converged"].all()), s
