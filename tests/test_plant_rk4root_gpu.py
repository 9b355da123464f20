"""The fused rk4root plant on the GPU (awempc.hip: mpc_plant_rk4root_kernel, one lane per loop): against the
same core on the host, its independence of the batch, the isolation of a NaN, the existing host-loop plant
``BatchedRti._rk4root`` in closed loop, and the open-loop simulation built on it."""
import numpy as np
import pytest
import torch

from awebox_amd import kite3 as k3
from awebox_amd import mpc
from awebox_amd.rti import BatchedRti

pytestmark = pytest.mark.gpu
B130 = 130          # two full wavefronts and a partial one


def parity(a, b):
    """The project's parity tolerance: |a - b| <= 1e-9 |b| + 1e-11 max |b|."""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all(np.abs(a - b) <= 1e-9 * np.abs(b) + 1e-11 * np.abs(b).max()))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from awebox_amd.build import build
    build()
    return torch.device("cuda:0")


def small_loop(batch, **kw):
    c = k3.build_constants(k3.Kite3Config(n_k=3, d=2))
    r = BatchedRti(c, batch, device="cuda", **kw)
    r.start(x0_entries=(6, 7, 10))
    return c, r


class Case:
    """130 loops' plant inputs (from BatchedRti.start at n_k = 3, d = 2) with two controls each, and the
    kernel's outputs for (n_fe, n_steps) = (4, 2), computed once and left unchanged."""

    def __init__(self):
        self.c, self.r = small_loop(B130)
        self.ev = self.r.ev
        self.x0, self.z0, self.par = self.r._plant_inputs()
        u0 = self.r.V[:, self.r.u0_idx]
        rng = np.random.default_rng(11)
        du = torch.tensor(0.01 * rng.standard_normal((B130, k3.NU)), device="cuda")
        self.u = torch.stack([u0, u0 + du], dim=1).contiguous()
        self.ts = self.c.cfg.ts
        self.out = self.run()
        torch.cuda.synchronize()

    def run(self, x0=None, n_fe=4, n_steps=2):
        return self.ev.plant_rk4root(self.x0 if x0 is None else x0, self.u[:, :n_steps].contiguous(), self.z0, self.par,
                                     self.ts, n_fe, n_steps)

    def host(self, n_fe, n_steps):
        return mpc.plant_rk4root_cpu(self.c, self.x0.cpu().numpy(), self.u[:, :n_steps].cpu().numpy(),
                                     self.z0.cpu().numpy(), self.par.cpu().numpy(), self.ts, n_fe, n_steps)


@pytest.fixture(scope="module")
def case(gpu):
    return Case()


@pytest.mark.parametrize("n_fe,n_steps", [(4, 2), (1, 1)])
def test_kernel_matches_host_core(case, n_fe, n_steps):
    """The kernel against awempc_plant_rk4root_cpu, the same core compiled for the host: the two differ
    in contraction and libm only."""
    xf, zf, qf, res = case.out if (n_fe, n_steps) == (4, 2) else case.run(n_fe=n_fe, n_steps=n_steps)
    ref = case.host(n_fe, n_steps)
    print("max diff", {k: float(np.abs(v.cpu().numpy() - ref[n]).max())
                       for k, v, n in (("xf", xf, "xf"), ("zf", zf, "zf"), ("qf", qf, "qf"))},
          "res", float(res.max()), ref["res"].max())
    assert float(res.max()) < 1e-10 and ref["res"].max() < 1e-10
    assert parity(xf.cpu().numpy(), ref["xf"])
    assert parity(zf.cpu().numpy(), ref["zf"])
    assert parity(qf.cpu().numpy(), ref["qf"])


def test_result_does_not_depend_on_the_batch(case):
    """Loops 0, 63, 64 and 129 of the 130-loop call are bitwise the one-loop calls on their inputs, and
    two identical calls agree bitwise."""
    again = case.run()
    for a, b in zip(case.out, again):
        assert torch.equal(a, b)
    ev1 = mpc.MpcEvaluator(case.c, batch=1)
    for i in (0, 63, 64, 129):
        one = ev1.plant_rk4root(case.x0[i:i + 1].contiguous(), case.u[i:i + 1].contiguous(),
                                case.z0[i:i + 1].contiguous(), case.par[i:i + 1].contiguous(), case.ts, 4, 2)
        for a, b in zip(case.out, one):
            assert torch.equal(a[i:i + 1], b), i


def test_nan_stays_in_its_loop(case):
    """A NaN in one loop's x0: the call returns, that loop reports a non-finite residual, every other
    loop is bitwise what it was."""
    bad = 70
    x0 = case.x0.clone()
    x0[bad, 3] = float("nan")
    out = case.run(x0=x0)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(out[3][bad]))
    keep = torch.arange(B130, device="cuda") != bad
    for a, b in zip(case.out, out):
        assert torch.equal(a[keep], b[keep])
    assert bool(torch.isfinite(out[3][keep]).all())


def test_fused_plant_matches_host_loop_plant(gpu):
    """_rk4root_fused against _rk4root from the same state over two closed-loop steps at (n_k, d, B) =
    (3, 2, 65), five RK4 steps per sampling time."""
    c, r = small_loop(65, plant="rk4root_fused", n_fe=5)
    r.simulate_reference(2 + c.cfg.n_k + 1)
    for _ in range(2):
        r.iterate()
        x_f, res_f = r._rk4root_fused()
        x_o, res_o = r._rk4root()
        torch.cuda.synchronize()
        print("x1 diff", float((x_f - x_o).abs().max()), "res", float(res_f.max()), float(res_o.max()))
        assert float(res_f.max()) < 1e-9 and float(res_o.max()) < 1e-9
        assert parity(x_f.cpu().numpy(), x_o.cpu().numpy())
        r._shift(x_o)
        r.step_count += 1


def test_fused_rk4root_plant_full_configuration(gpu):
    """test_rk4root_plant_on_gpu's assertions with the fused plant: the full configuration, 256 loops
    tracking trajectories of the model from x0 perturbed on the invariant-free states, per loop against
    the collocation plant from the same state and control over three closed-loop steps."""
    c = k3.build_constants()
    r = BatchedRti(c, 256, device="cuda", plant="rk4root_fused")
    r.start(x0_entries=(6, 7, 10))
    r.simulate_reference(3 + c.cfg.n_k + 1)
    for _ in range(3):
        r.iterate()
        x0 = r.P[:, :k3.NX].clone()
        x_c, res_c = r._plant()
        x_r, res_r = r._rk4root_fused()
        torch.cuda.synchronize()
        assert torch.isfinite(x_r).all()
        assert float(res_r.max()) < 1e-9 and float(res_c.max()) < 1e-9
        step = (x_c - x0).abs().amax(dim=1)
        gap = (x_c - x_r).abs().amax(dim=1)
        print("gap / step", float((gap / step).max()))
        assert bool((gap <= 1e-8 * step).all()), float((gap / step).max())
        r._shift(x_r)
        r.step_count += 1
    out = r.step()
    assert torch.isfinite(out["x0"]).all() and bool(out["plant_converged"].all())


def test_open_loop_is_the_chained_plant(gpu):
    """simulate_open_loop over 3 sampling times is three _rk4root_fused calls chained (x1 -> x0, (xdot, z)
    at x1 -> the next guess), bitwise, and leaves the loops as they were."""
    c, r = small_loop(65, plant="rk4root_fused", n_fe=3)
    rng = np.random.default_rng(3)
    u_seq = r.V[:, r.u0_idx].unsqueeze(1) + torch.tensor(0.01 * rng.standard_normal((65, 3, k3.NU)), device="cuda")
    V0, P0 = r.V.clone(), r.P.clone()
    sim = r.simulate_open_loop(u_seq)
    assert torch.equal(r.V, V0) and torch.equal(r.P, P0)
    assert sim["x"].shape == (65, 3, k3.NX) and sim["q"].shape == (65, 3)
    for s in range(3):
        r.V[:, r.u0_idx] = u_seq[:, s]
        x1, res = r._rk4root_fused()
        assert torch.equal(x1, sim["x"][:, s]) and torch.equal(r.plant_q, sim["q"][:, s])
        assert float(res.max()) < 1e-9
        r.P[:, r.lay.p_x0:r.lay.p_x0 + k3.NX] = x1
        r.V[:, r.rk_cols] = r.plant_z
    assert torch.equal(r.plant_z, sim["z"])
    assert not torch.equal(sim["x"][:, 0], sim["x"][:, 2]) and float(sim["residual"].max()) < 1e-9
