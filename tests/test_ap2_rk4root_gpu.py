"""The fused AP2 rk4root on the GPU (awegpu.hip: ap2_rk4root_kernel, one lane per integration task): against
the same core on the host, its independence of the batch, the isolation of a NaN, ``integrators.reintegrate``
against the host-loop ``IntervalIntegrator.rk4root`` on the HIP evaluator for every (instance, interval), and
``integrators.simulate_open_loop``."""
import numpy as np
import pytest
import torch

from awebox_amd import evaluator as evm
from awebox_amd import homotopy as hm
from awebox_amd import problem as pb
from awebox_amd.integrators import IntervalIntegrator, reintegrate, simulate_open_loop
from test_ap2_rk4root import Start, parity          # tests/ is on sys.path

pytestmark = pytest.mark.gpu
N130 = 130          # two full wavefronts and a partial one


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from awebox_amd.build import build
    build()
    return torch.device("cuda:0")


class Case:
    """130 tasks: the intervals of 44 perturbed instances at (n_k, d) = (3, 2) (test_ap2_rk4root.Start), each
    with three controls and its own sampling time, and the kernel's outputs for (n_fe, n_steps) = (2, 3),
    computed once and left unchanged."""

    def __init__(self):
        self.s = s = Start(n_inst=44, seed=11)
        parts = [s.task(k) for k in range(s.lay.n_k)]
        x0, u1, y0, par = (np.concatenate([p[i] for p in parts])[:N130] for i in range(4))
        rng = np.random.default_rng(12)
        u = np.repeat(u1, 3, axis=1)
        u[:, 1:, 6:] += 0.05 * rng.standard_normal((N130, 2, 4))
        ts = 0.1 * (1.0 + 0.25 * rng.random(N130))      # n_fe = 2: steps below 0.0625 s, inside RK4's stability range
        self.host_in = (x0, u, y0, par, ts)
        self.ev = evm.Ap2Evaluator(s.c, batch=1)
        self.dev_in = tuple(torch.tensor(a, device="cuda") for a in self.host_in)
        self.out = self.run()
        torch.cuda.synchronize()

    def run(self, sel=None, n_fe=2, n_steps=3, x0=None):
        """The kernel on the tasks ``sel`` (an index tensor; default all) in this order."""
        a = list(self.dev_in)
        if x0 is not None:
            a[0] = x0
        if sel is not None:
            a = [t[sel] for t in a]
        a[1] = a[1][:, :n_steps]
        return self.ev.integrate_rk4root(*(t.contiguous() for t in a), n_fe, n_steps)

    def host(self, n, n_fe, n_steps):
        x0, u, y0, par, ts = (a[:n] for a in self.host_in)
        return evm.integrate_rk4root_cpu(self.s.c, x0, np.ascontiguousarray(u[:, :n_steps]), y0, par, ts, n_fe, n_steps)


@pytest.fixture(scope="module")
def case(gpu):
    return Case()


@pytest.mark.parametrize("n", [N130, 1])
@pytest.mark.parametrize("n_fe,n_steps", [(4, 1), (2, 3)])
def test_kernel_matches_host_core(case, n, n_fe, n_steps):
    """The kernel against awe_integrate_rk4root_cpu, the same core compiled for the host: the two differ in
    contraction and libm only."""
    if (n, n_fe, n_steps) == (N130, 2, 3):
        xf, yf, qf, res = case.out
    else:
        xf, yf, qf, res = case.run(torch.arange(n, device="cuda"), n_fe, n_steps)
    ref = case.host(n, n_fe, n_steps)
    diff = {k: float(np.abs(v.cpu().numpy() - ref[k]).max()) for k, v in (("xf", xf), ("yf", yf), ("qf", qf))}
    print("max diff", diff, "res", float(res.max()), ref["res"].max())
    assert float(res.max()) < 1e-10 and ref["res"].max() < 1e-10
    assert parity(xf.cpu().numpy(), ref["xf"])
    assert parity(yf.cpu().numpy(), ref["yf"])
    assert parity(qf.cpu().numpy(), ref["qf"])


def test_result_does_not_depend_on_the_batch(case):
    """Task 5 at positions 0, 63, 64 and 129 of a batch of 130 and alone: bitwise the same results."""
    sel = torch.arange(N130, device="cuda")
    for pos in (0, 63, 64, 129):
        sel[pos] = 5
    many = case.run(sel)
    alone = case.run(torch.tensor([5], device="cuda"))
    for a, m, o in zip(alone, many, case.out):
        for pos in (0, 63, 64, 129):
            assert torch.equal(m[pos], a[0])
        assert torch.equal(o[5], a[0])
        assert torch.equal(m[7], o[7])


def test_nan_task_is_isolated(case):
    """A NaN in one task's state: that task ends with a non-finite residual, every other task's bits unchanged."""
    x0 = case.dev_in[0].clone()
    x0[70, 7] = float("nan")
    out = case.run(x0=x0)
    keep = torch.ones(N130, dtype=torch.bool, device="cuda")
    keep[70] = False
    assert not bool(torch.isfinite(out[3][70]))
    for a, b in zip(out, case.out):
        assert torch.equal(a[keep], b[keep])
    assert bool(torch.isfinite(case.out[3]).all())


def test_reintegrate_matches_the_host_loop_on_every_interval(gpu):
    """reintegrate on the device at (n_k, d) = (3, 2), B = 3, n_fe = 8 against IntervalIntegrator.rk4root on
    the HIP evaluator for the same interval with the same n_steps, max_newton and tol: x_end, z_end and the
    energy of every (instance, interval) within the project's parity tolerance -- a wrong interval-to-task
    mapping, sampling time or theta0 row shows here."""
    s = Start(n_inst=3, seed=21)
    s.P[1, s.lay.p_theta0 + pb.THETA0_OFF["wind.u_ref"][0]] = 8.5       # the instances' theta0 rows differ
    s.V[2, s.lay.theta()[1]] = 1.5                                       # and their interval lengths
    ev = evm.Ap2Evaluator(s.c, batch=3)
    V, P = torch.tensor(s.V, device="cuda"), torch.tensor(s.P, device="cuda")
    r = reintegrate(ev, s.lay, s.c, V, P, n_fe=8, device="cuda", max_newton=20, tol=1e-12)
    assert tuple(r["x"].shape) == (3, s.lay.n_k) and float(r["residual"].max()) < 1e-10
    h = V[:, int(s.lay.theta()[1])] * s.c.scaling[pb.W_TH0 + 1] / s.lay.n_k
    for k in range(s.lay.n_k):
        ref = IntervalIntegrator(ev, s.lay, s.c.scaling, k=k, device="cuda").rk4root(
            V, P, hm.power_integrand(s.c), h, n_steps=8, max_newton=20, tol=1e-12)
        print(k, "x", float((r["x_end"][:, k] - ref["x_end"]).abs().max()), "z",
              float((r["z_end"][:, k] - ref["z_end"]).abs().max()), "q", r["q_end"][:, k].tolist(), ref["q"].tolist())
        assert float(ref["residual"].max()) < 1e-10
        for b in range(3):
            assert parity(r["x_end"][b, k].cpu().numpy(), ref["x_end"][b].cpu().numpy()), (b, k)
            assert parity(r["z_end"][b, k].cpu().numpy(), ref["z_end"][b].cpu().numpy()), (b, k)
        assert parity(r["q_end"][:, k].cpu().numpy(), ref["q"].cpu().numpy()), k
        exp = V[:, torch.as_tensor(s.lay.x(k + 1), device="cuda")]
        err = (ref["x_end"] - exp).abs().amax(dim=1) / exp.abs().amax(dim=1)
        assert torch.allclose(r["x"][:, k], err, rtol=1e-6, atol=1e-12)


def test_open_loop_is_chained_single_steps(case):
    """simulate_open_loop over three sampling times equals three chained single-step calls, bitwise."""
    c = case.s.c
    x0, u, y0, par, ts = (t[:N130] for t in case.dev_in)
    th = torch.tensor(case.s.V[:1, case.s.lay.theta()], device="cuda").expand(N130, 2)
    kw = dict(n_fe=2, theta=th, gamma=torch.ones(N130, dtype=torch.float64, device="cuda"))
    one = simulate_open_loop(case.ev, c, x0, u, ts, y0=y0, **kw)
    x, y = x0, y0
    for s in range(3):
        o = simulate_open_loop(case.ev, c, x, u[:, s:s + 1], ts, y0=y, **kw)
        x, y = o["x"][:, 0].contiguous(), o["y"]
        assert torch.equal(o["x"][:, 0], one["x"][:, s]) and torch.equal(o["q"][:, 0], one["q"][:, s])
    assert torch.equal(y, one["y"])
    assert float(one["residual"].max()) < 1e-10 and bool(torch.isfinite(one["x"]).all())
    # the same tasks as the case's kernel run: the wrapper packs what the direct call was given
    assert torch.equal(one["x"], case.out[0])
