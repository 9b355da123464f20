"""The fused rk4root plant on the host (no GPU): the generated rootfinder node code
(csrc/kite3_noderoot.gen.hpp, written by csrc/gen/kite3_rootgen.cpp) against the dual-number model, and
the integrator core (csrc/plant_rk4root.hpp through awempc_plant_rk4root_cpu) against the existing
oracle-driven plant ``BatchedRti._rk4root``, its own order of convergence, chaining and argument checks.

The reference's plant is sim.py:72-78 -> rk4root (tools/integrator_routines.py:32-96): n_fe RK4 steps per
sampling time with a Newton rootfinder for (xdot, z) at every stage and once more at the end."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from awebox_amd import build as B
from awebox_amd import kite3 as k3
from awebox_amd import mpc
from awebox_amd.nlp_binding import AwegpuError
from awebox_amd.rti import BatchedRti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "awebox_amd", "csrc")


def parity(a, b):
    """The project's parity tolerance: |a - b| <= 1e-9 |b| + 1e-11 max |b|."""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all(np.abs(a - b) <= 1e-9 * np.abs(b) + 1e-11 * np.abs(b).max()))


@pytest.fixture(scope="module", autouse=True)
def library():
    B.generate()
    B.build_one(B.LIB_MPC)


# ---- generated code ---------------------------------------------------------------------------------
def test_committed_root_header_is_current():
    """kite3_noderoot.gen.hpp in the tree is what gen/kite3_rootgen.cpp writes for the current model."""
    before = open(B.K3_ROOT_HEADER).read()
    B.generate(force=True)
    assert open(B.K3_ROOT_HEADER).read() == before, "kite3_noderoot.gen.hpp is stale: run python -m awebox_amd.build"


@pytest.fixture(scope="module")
def root_checker(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("k3root")
    exe = str(tmp / "check_k3root")
    subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(CSRC, "gen", "check_kite3_root.cpp"), "-o", exe],
                   check=True)
    return tmp, exe


@pytest.mark.parametrize("k,seed", [(0, 0), (9, 1), (19, 2)])
def test_generated_root_code_matches_dual_model(root_checker, k, seed):
    """The 12 rows and every entry of the 12 x 12 block d eq / d(xdot, z) against one dual-number pass of
    kite3_node per unknown (csrc/gen/check_kite3_root.cpp), at the perturbed nodes and with the
    thresholds of test_generated_kite3_jacobian_matches_dual_model; every slot is a pattern entry and the
    block has full rank."""
    tmp, exe = root_checker
    c = k3.build_constants()
    lay = k3.MpcLayout(20, 4)
    V, p = k3.batch_instance(c, lay, k, 8)
    rng = np.random.default_rng(seed)
    w = np.concatenate([V[lay.x(k)], V[lay.xdot(k)], V[lay.u(k)], V[lay.z(k)], V[lay.theta()], V[lay.phi()][:1]])
    w = w * (1 + 0.05 * rng.standard_normal(w.shape)) + 0.01 * rng.standard_normal(w.shape)
    np.savetxt(str(tmp / "consts.txt"), c.consts)
    np.savetxt(str(tmp / "w.txt"), w)
    u_ref = 4.0 + 4.0 * rng.random()
    out = subprocess.run([exe, str(tmp / "consts.txt"), str(tmp / "w.txt"), repr(u_ref)], check=True,
                         capture_output=True, text=True)
    r = json.loads(out.stdout)
    assert r["entries"] == r["n_slots"] == r["entry_table"], "every slot is a pattern entry, both tables agree"
    assert r["value_rel"] < 1e-14, r
    assert r["entry_rel"] < 1e-12, r
    assert r["entry_max"] > 1.0
    block = np.array(r["block"]).reshape(12, 12)
    assert np.linalg.matrix_rank(block) == 12, np.linalg.svd(block, compute_uv=False)


# ---- the integrator core on the host ------------------------------------------------------------------
class Start:
    """The consistent start of the CPU tests: (n_k, d, B) = (3, 2, 2), the oracle as the evaluator
    (tests/test_rti.py), start(x0_entries=(6, 7, 10)), n_fe = 2."""

    def __init__(self):
        from test_rti import OracleBatchEval          # tests/ is on sys.path
        self.c = c = k3.build_constants(k3.Kite3Config(n_k=3, d=2))
        self.lay = lay = k3.MpcLayout(3, 2)
        self.r = r = BatchedRti(c, 2, device="cpu", evaluator=OracleBatchEval(c, lay), plant="rk4root", n_fe=2)
        r.start(x0_entries=(6, 7, 10))
        self.x0, self.z0, self.par = (t.numpy().copy() for t in r._plant_inputs())
        self.u = r.V[:, r.u0_idx].numpy().copy().reshape(2, 1, k3.NU)
        self.ts = c.cfg.ts

    def core(self, n_fe, n_steps=1, u=None, x0=None, z0=None, **kw):
        return mpc.plant_rk4root_cpu(self.c, self.x0 if x0 is None else x0, self.u if u is None else u,
                                     self.z0 if z0 is None else z0, self.par, self.ts, n_fe, n_steps, **kw)


@pytest.fixture(scope="module")
def start():
    return Start()


def restated_rk4root(r, max_newton=6, tol=1e-11):
    """``BatchedRti._rk4root``'s loop written out again on the same evaluator, with what it does not
    return: the power integrand lambda l_t dl_t (SI, dynamics.py:318-330) at each stage's own state and z,
    integrated with the RK4 weights (the convention of integrators.py::rk4root), and the rootfinder at
    the end state, which gives (xdot, z) there."""
    n, nb = r.n_rk, r.B
    s = torch.tensor(r.consts.scaling)
    h = r.consts.cfg.ts / r.n_fe
    Vp = r.V.clone()
    x = r.P[:, r.lay.p_x0:r.lay.p_x0 + k3.NX].clone()
    worst = torch.zeros(nb, dtype=torch.float64)

    def ode(xs):
        nonlocal worst
        Vp[:, r.x_idx[0]] = xs
        for it in range(max_newton + 1):
            r.ev.eval_nlp_device(Vp, r.P, r.f, r.g, r.grad, r.jac)
            rows = r.g[:, r.rk_rows]
            res = rows.abs().amax(dim=1)
            if it == max_newton or float(res.max()) < tol:
                break
            A = torch.zeros(nb, n * n, dtype=torch.float64)
            A[:, r.rk_dst] = r.jac[:, r.rk_keep]
            Vp[:, r.rk_cols] -= torch.linalg.solve(A.view(nb, n, n), rows.unsqueeze(-1)).squeeze(-1)
        worst = torch.maximum(worst, res)
        y = Vp[:, r.rk_cols]
        p = (y[:, k3.NX] * s[2 * k3.NX + k3.NU]) * (xs[:, 8] * s[8]) * (xs[:, 9] * s[9])
        return Vp[:, r.xdot_idx] * r.rk_ratio, p

    q = torch.zeros(nb, dtype=torch.float64)
    for _ in range(r.n_fe):
        k1, p1 = ode(x)
        k2, p2 = ode(x + 0.5 * h * k1)
        k3_, p3 = ode(x + 0.5 * h * k2)
        k4, p4 = ode(x + h * k3_)
        x = x + h * (k1 + 2.0 * k2 + 2.0 * k3_ + k4) / 6.0
        q = q + h * (p1 + 2.0 * p2 + 2.0 * p3 + p4) / 6.0
    ode(x)
    return x.numpy(), Vp[:, r.rk_cols].numpy().copy(), q.numpy(), worst.numpy()


def test_host_core_matches_oracle_driven_plant(start):
    """awempc_plant_rk4root_cpu against BatchedRti._rk4root from the same start: x1 to the project's
    parity tolerance, both residuals below 1e-10; (xdot, z) at x1 and the power integral against the
    restatement of that loop (which reproduces _rk4root's x1)."""
    r = start.r
    x_old, res_old = r._rk4root()
    out = start.core(n_fe=2)
    print("x1 diff", np.abs(out["xf"][:, 0] - x_old.numpy()).max(), "res", out["res"].max(), float(res_old.max()))
    assert out["res"].max() < 1e-10 and float(res_old.max()) < 1e-10
    assert parity(out["xf"][:, 0], x_old.numpy())
    x_re, y_re, q_re, res_re = restated_rk4root(r)
    print("zf diff", np.abs(out["zf"] - y_re).max(), "qf", out["qf"][:, 0], q_re)
    assert parity(x_re, x_old.numpy()) and res_re.max() < 1e-10
    assert parity(out["zf"], y_re)
    assert parity(out["qf"][:, 0], q_re)
    assert np.abs(q_re).min() > 0.0


def test_order_of_convergence(start):
    """Classical RK4: against the core's own n_fe = 64 the error of n_fe = 2, 4, 8 falls by a factor in
    [8, 32] per halving of the step (16 for order 4)."""
    ref = start.core(n_fe=64)["xf"][:, 0]
    err = [np.abs(start.core(n_fe=n)["xf"][:, 0] - ref).max() for n in (2, 4, 8)]
    print("errors", err, "factors", err[0] / err[1], err[1] / err[2],
          "step", np.abs(ref - start.x0).max())
    for a, b in zip(err, err[1:]):
        assert 8.0 <= a / b <= 32.0, err


def test_chained_calls_equal_one_call(start):
    """n_steps = 3 in one call is three n_steps = 1 calls chained (xf -> x0, zf -> z0), bitwise."""
    rng = np.random.default_rng(5)
    u = start.u + 0.01 * rng.standard_normal((2, 3, k3.NU))
    one = start.core(n_fe=3, n_steps=3, u=u)
    x, z = start.x0, start.z0
    for s in range(3):
        o = start.core(n_fe=3, n_steps=1, u=np.ascontiguousarray(u[:, s:s + 1]), x0=x, z0=z)
        x, z = np.ascontiguousarray(o["xf"][:, 0]), o["zf"]
        assert np.array_equal(o["xf"][:, 0], one["xf"][:, s])
        assert np.array_equal(o["qf"][:, 0], one["qf"][:, s])
    assert np.array_equal(z, one["zf"])
    assert np.isfinite(one["xf"]).all() and one["res"].max() < 1e-10
    assert not np.array_equal(one["xf"][:, 0], one["xf"][:, 1])


@pytest.mark.parametrize("kw,word", [({"n_fe": 0}, "n_fe"), ({"n_fe": 2, "n_steps": 0}, "n_steps"),
                                     ({"n_fe": 2, "max_newton": -1}, "max_newton")])
def test_bad_arguments_are_errors(start, kw, word):
    with pytest.raises(AwegpuError, match=word):
        start.core(**kw)


def test_constants_of_another_structure_are_refused(start):
    """The generated code is for a fixed tether element count (kNElements); other constants, or a
    vector of another length, are an error with a message."""
    c = start.c.consts.copy()
    c[23] += 1.0                                        # K3_C_N_ELEMENTS
    with pytest.raises(AwegpuError, match="tether elements"):
        mpc.plant_rk4root_cpu(c, start.x0, start.u, start.z0, start.par, start.ts, 2)
    with pytest.raises(AwegpuError, match="constants"):
        mpc.plant_rk4root_cpu(c[:-1], start.x0, start.u, start.z0, start.par, start.ts, 2)
    with pytest.raises(ValueError):
        mpc.plant_rk4root_cpu(start.c, start.x0[:, :-1], start.u, start.z0, start.par, start.ts, 2)
