"""The tracking MPC's reference generator on the host (awebox_amd/reference.py, csrc/ref_pp.hpp).

``mpc.reference_window_cpu`` runs the core the HIP kernel runs (piecewise polynomials from
``PeriodicTrajectory.tables``); ``PeriodicTrajectory.window_host`` restates the windows with scipy's
interpolators and never touches the tables.  Checked here:

* window parity of the two at the project's parity tolerance (1e-9 |b| + 1e-11 max |b|);
* the order of accuracy against the analytic circle: halving the interval cuts the error by at least
  2^d (poly; theory 2^(d+1)) and 8 (spline; theory 16);
* node exactness on a grid of binary fractions, zero channels, a NaN start time, a refused table, files;
* the closed loop on the oracle-backed evaluator: ``track(from_simulation(r), "poly")`` on aligned phases
  reproduces the ``simulate_reference`` mode, and runs past the stored trajectory's end.
"""
import numpy as np
import pytest
import torch

from awebox_amd import kite3 as k3
from awebox_amd import mpc
from awebox_amd.nlp_binding import AwegpuError
from awebox_amd.reference import PeriodicTrajectory
from awebox_amd.rti import BatchedRti, orbit_states

KINDS = ("poly", "spline")
TRAJ_GRIDS = ((5, 3), (12, 4))
MPC_SHAPES = ((3, 2), (10, 4))


def close(a, b):
    """The parity tolerance of DESIGN section 3, entry by entry."""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all(np.abs(a - b) <= 1e-9 * np.abs(b) + 1e-11 * np.abs(b).max()))


def circle(c):
    orbit = k3.CircularOrbit(c.cfg)
    return orbit, lambda t: orbit_states(orbit, np.asarray(t)) / c.scaling[:k3.NX]


def perturbed_circle(c, n_k, d, seed=7):
    """The circle plus a seeded smooth periodic perturbation of every x, z and u channel (none constant)."""
    orbit, fn = circle(c)
    T = orbit.period
    rng = np.random.default_rng(seed)

    def smooth(n):
        amp, ph = 0.05 * rng.standard_normal((3, n)), rng.uniform(0, 2 * np.pi, (3, n))
        return lambda t: sum(amp[m] * np.sin(2 * np.pi * (m + 1) * np.asarray(t)[:, None] / T + ph[m]) for m in range(3))

    px, pz, pu = smooth(k3.NX), smooth(k3.NZ), smooth(k3.NU)
    traj = PeriodicTrajectory.from_function(lambda t: fn(t) + px(t), T, n_k, d)
    tn = (np.arange(n_k)[:, None] + traj.tau[None, 1:]) * (T / n_k)
    z = 1.0 + pz(tn.reshape(-1)).reshape(n_k, d, k3.NZ)
    u = pu(np.arange(n_k) * (T / n_k))
    return PeriodicTrajectory(T, traj.x, z, u)


def time_list(T, seed=3):
    rng = np.random.default_rng(seed)
    return np.concatenate([[0.0, T, 3 * T, np.nextafter(T, 0), 1e3 * T + 0.37], rng.uniform(0, 2 * T, 20)])


def consts_lay(N, d, ts=0.1):
    c = k3.build_constants(k3.Kite3Config(n_k=N, d=d, ts=ts))
    return c, k3.MpcLayout(N, d)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("grid", TRAJ_GRIDS)
@pytest.mark.parametrize("shape", MPC_SHAPES)
def test_window_parity_with_scipy(kind, grid, shape):
    c, lay = consts_lay(*shape)
    traj = perturbed_circle(c, *grid)
    t0 = time_list(traj.T)
    got = mpc.reference_window_cpu(traj.tables(kind), t0, lay, c)
    want = traj.window_host(kind, t0, lay, c)
    assert np.abs(want).min(axis=0)[lay.coll_z(0, 0)[0]] > 0.0          # z is tracked, not a zero channel
    assert close(got, want), float(np.abs(got - want).max())


def _max_error(c, lay, kind, n_k, d, t):
    orbit, fn = circle(c)
    traj = PeriodicTrajectory.from_function(fn, orbit.period, n_k, d)
    R = mpc.reference_window_cpu(traj.tables(kind), t, lay, c)
    return float(np.abs(R[:, lay.x(0)] - fn(t)).max())


@pytest.mark.parametrize("kind,d,factor", [("poly", 2, 4.0), ("poly", 3, 8.0), ("poly", 4, 16.0),
                                           ("spline", 2, 8.0), ("spline", 3, 8.0), ("spline", 4, 8.0)])
def test_order_of_accuracy(kind, d, factor):
    """Against the analytic circle at 4,000 random times, n_k = 6 -> 12 -> 24."""
    c, lay = consts_lay(3, 2)
    T = k3.CircularOrbit(c.cfg).period
    t = np.random.default_rng(11).uniform(0, T, 4000)
    e = [_max_error(c, lay, kind, n_k, d, t) for n_k in (6, 12, 24)]
    print(kind, d, e, e[0] / e[1], e[1] / e[2])
    assert e[0] / e[1] >= factor and e[1] / e[2] >= factor, e


def binary_grid_trajectory(n, d, ts=0.125, seed=5):
    """What ``from_simulation`` yields in shape: n intervals of length ts = 0.125, so breakpoints and
    sampling times are exact binary fractions; the node values are random, the states continuous from
    one interval to the next as an integrator leaves them."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d + 1, k3.NX))
    x[1:, 0] = x[:-1, -1]
    return PeriodicTrajectory(n * ts, x, rng.standard_normal((n, d, k3.NZ)),
                              rng.standard_normal((n, k3.NU)), xdot0=rng.standard_normal((n, k3.NX)),
                              z0=rng.standard_normal((n, k3.NZ)))


def test_nodes_are_reproduced_on_a_binary_grid():
    N, d, n, ts = 3, 2, 8, 0.125
    c, lay = consts_lay(N, d, ts)
    traj = binary_grid_trajectory(n, d, ts)
    starts = np.array([0, 2, 4])
    R = mpc.reference_window_cpu(traj.tables("poly"), starts * ts, lay, c)
    scale = max(np.abs(traj.x).max(), np.abs(traj.z).max(), np.abs(traj.u).max())
    ok = lambda a, b: bool(np.all(np.abs(a - b) <= 1e-9 * np.abs(b) + 1e-11 * scale))   # noqa: E731
    for i, s in enumerate(starts):
        for k in range(N + 1):
            assert ok(R[i, lay.x(k)], traj.x[s + k, 0])
        for k in range(N):
            assert ok(R[i, lay.u(k)[3:]], traj.u[s + k, 3:])
            assert ok(R[i, lay.xdot(k)], traj.xdot0[s + k]) and ok(R[i, lay.z(k)], traj.z0[s + k])
            for j in range(d):
                assert ok(R[i, lay.coll_x(k, j)], traj.x[s + k, j + 1])
                assert ok(R[i, lay.coll_z(k, j)], traj.z[s + k, j])
    assert np.array_equal(R[:, lay.theta()], np.tile(np.array([c.cfg.diam_t, N * ts]) / c.scaling[-2:], (3, 1)))
    assert not R[:, lay.phi()].any() and not R[:, lay.xi()].any()


@pytest.mark.parametrize("kind", KINDS)
def test_zero_and_fictitious_channels_are_exactly_zero(kind):
    c, lay = consts_lay(3, 2)
    traj = perturbed_circle(c, 5, 3)
    traj.x[:, :, 9] = 0.0                                     # dl_t: an all-zero state channel
    traj.u[:, :3] = 0.3                                       # fictitious forces: zero whatever is stored
    for tr in (traj, PeriodicTrajectory(traj.T, traj.x, 0.0 * traj.z, traj.u)):
        R = mpc.reference_window_cpu(tr.tables(kind), time_list(tr.T), lay, c)
        for k in range(lay.n_k):
            assert not R[:, lay.u(k)[:3]].any() and not R[:, lay.xdot(k)].any() and not R[:, lay.z(k)].any()
            assert not R[:, lay.x(k)[9]].any() and not R[:, lay.coll_x(k, 1)[9]].any()
    assert not R[:, lay.coll_z(1, 0)].any()                   # the second trajectory's z is all zero
    assert R[:, lay.coll_x(1, 0)[0]].all()


@pytest.mark.parametrize("kind", KINDS)
def test_nan_start_time_stays_in_its_loop(kind):
    c, lay = consts_lay(3, 2)
    tab = perturbed_circle(c, 5, 3).tables(kind)
    good = mpc.reference_window_cpu(tab, np.array([1.0, 5.0, 2.0]), lay, c)
    for bad_t in (np.nan, np.inf):
        bad = mpc.reference_window_cpu(tab, np.array([1.0, bad_t, 2.0]), lay, c)
        assert np.array_equal(bad[0], good[0]) and np.array_equal(bad[2], good[2])
        assert np.isnan(bad[1, lay.x(0)]).all() and np.isnan(bad[1, lay.coll_x(2, 1)]).all()


def test_window_written_in_place_leaves_the_rest():
    c, lay = consts_lay(3, 2)
    tab = perturbed_circle(c, 5, 3).tables("spline")
    t0 = np.array([0.3, 40.0])
    P = np.random.default_rng(0).standard_normal((2, lay.n_p))
    P0 = P.copy()
    mpc.reference_window_cpu(tab, t0, lay, c, out=P, off=lay.p_ref)
    assert np.array_equal(P[:, lay.p_ref:lay.p_ref + lay.n_v], mpc.reference_window_cpu(tab, t0, lay, c))
    assert np.array_equal(P[:, :lay.p_ref], P0[:, :lay.p_ref]) and np.array_equal(P[:, lay.p_u_ref:], P0[:, lay.p_u_ref:])


def test_oversize_table_is_refused():
    c, lay = consts_lay(3, 2)
    tab = perturbed_circle(c, 5, 3).tables("poly")
    gx = tab["grids"]["x"]
    gx["coef"] = np.concatenate([gx["coef"], np.zeros(gx["coef"].shape[:2] + (8 - gx["degree"],))], axis=2)
    with pytest.raises(AwegpuError, match="degree"):
        mpc.reference_window_cpu(tab, np.zeros(1), lay, c)
    n = 2100
    tab = perturbed_circle(c, 5, 3).tables("poly")
    tab["grids"]["u"] = {"breaks": np.linspace(0.0, tab["period"], n + 1), "degree": 0,
                         "coef": np.zeros((n, mpc.REF_CHANNELS["u"], 1))}
    with pytest.raises(AwegpuError, match="staging"):
        mpc.reference_window_cpu(tab, np.zeros(1), lay, c)


def test_save_load_round_trip(tmp_path):
    traj = binary_grid_trajectory(6, 3)
    traj.save(tmp_path / "traj.npz")
    back = PeriodicTrajectory.load(tmp_path / "traj.npz")
    assert (back.T, back.n_k, back.d, back.diam_t) == (traj.T, traj.n_k, traj.d, traj.diam_t)
    for name in ("x", "z", "u", "xdot0", "z0"):
        assert np.array_equal(getattr(back, name), getattr(traj, name))
    assert back.closure_gap == traj.closure_gap == float(np.abs(traj.x[-1, -1] - traj.x[0, 0]).max())


# ------------------------------------------------------------------ closed loop -----------------
def aligned_loop(make, n_nodes, ts=0.125, n_k=3, d=2, B=2):
    """A loop whose B members all start at phase 0 (their perturbations kept), with a simulated
    reference of ``n_nodes`` sampling times: every member's stored trajectory is then the same one."""
    c = k3.build_constants(k3.Kite3Config(n_k=n_k, d=d, ts=ts))
    r = make(c, B)
    r.start(x0_entries=(6, 7, 10))
    lay = r.lay
    ref = slice(lay.p_ref, lay.p_ref + lay.n_v)
    new = torch.as_tensor(r.reference(np.zeros(B)), device=r.dev)
    delta = new - r.P[:, ref]
    r.P[:, lay.p_x0:lay.p_x0 + k3.NX] += delta[:, lay.x(0)]
    r.V[:, lay.v_intervals:] += delta[:, lay.v_intervals:]
    r.P[:, ref] = new
    r.simulate_reference(n_nodes)
    return c, r


def _oracle_loop(c, B):
    from test_rti import OracleBatchEval          # tests/ is on sys.path
    return BatchedRti(c, B, device="cpu", evaluator=OracleBatchEval(c, k3.MpcLayout(c.cfg.n_k, c.cfg.d)))


def test_track_reproduces_the_simulated_reference_mode():
    """Aligned phases, ts = 0.125, poly: the kernel core's windows equal the stored ones, so two RTIs give
    the same V; the tracking loop then runs on past the stored trajectory's former end."""
    n_nodes = 6
    _, a = aligned_loop(_oracle_loop, n_nodes)
    c, b = aligned_loop(_oracle_loop, n_nodes)
    lay = b.lay
    traj = PeriodicTrajectory.from_simulation(b)
    assert traj.T == n_nodes * 0.125 and (traj.n_k, traj.d) == (n_nodes, lay.d)
    b.track(traj, "poly", t0=np.zeros(b.B))
    ref = slice(lay.p_ref, lay.p_ref + lay.n_v)
    assert close(b.P[:, ref].numpy(), a.P[:, ref].numpy())
    assert close(b.V.numpy(), a.V.numpy())
    for _ in range(2):
        a.step(), b.step()
        assert close(b.P[:, ref].numpy(), a.P[:, ref].numpy())
    print("V gap after two RTIs", float((a.V - b.V).abs().max()))
    assert close(b.V.numpy(), a.V.numpy())
    assert close(b.P[:, :k3.NX].numpy(), a.P[:, :k3.NX].numpy())
    for _ in range(n_nodes - lay.n_k - 2):
        a.step(), b.step()
    with pytest.raises(ValueError, match="ends before"):
        a.step()
    out = b.step()                                            # window n_nodes - n_k + 1: wraps round the period
    assert torch.isfinite(out["x0"]).all() and torch.isfinite(b.V).all()
