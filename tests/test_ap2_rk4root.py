"""The fused AP2 rk4root on the host (no GPU): the generated rootfinder node code
(csrc/ap2_noderoot.gen.hpp, written by csrc/gen/ap2_rootgen.cpp) against the dual-number model and its
structured Newton step against a dense 24 x 24 one, and the integrator core (csrc/plant_rk4root.hpp through
awe_integrate_rk4root_cpu) against the independent host loop ``IntervalIntegrator.rk4root``, its own order of
convergence, chaining, NaN isolation, argument checks and ``integrators.reintegrate``.

The reference's integrator is tools/integrator_routines.py:32-96 (n_fe RK4 steps with a Newton rootfinder for
(xdot, z) at every stage and once more at the end), as test/reg/test_discretization.py:20-193 runs it over
an interval of a solved trajectory."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from awebox_amd import build as B
from awebox_amd import evaluator as evm
from awebox_amd import homotopy as hm
from awebox_amd import problem as pb
from awebox_amd.initial_guess import initial_guess
from awebox_amd.integrators import IntervalIntegrator, reintegrate
from awebox_amd.nlp_binding import AwegpuError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "awebox_amd", "csrc")
# the Newton step of the structured solve against the dense 24 x 24 LU, relative to the largest step entry:
# 8.3e-15 observed over the three points below, asserted with one decimal order of margin
STEP_BOUND = 8.3e-14


def parity(a, b):
    """The project's parity tolerance: |a - b| <= 1e-9 |b| + 1e-11 max |b|."""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all(np.abs(a - b) <= 1e-9 * np.abs(b) + 1e-11 * np.abs(b).max()))


@pytest.fixture(scope="module", autouse=True)
def library():
    B.generate()
    B.build_one(B.LIB)


class Start:
    """The point of these tests: (n_k, d, B) = (3, 2, 2), the initial guess with a deterministic
    perturbation of omega, delta and dl_t (states) and of the surface and winch controls; q, dq and r keep
    the tether and DCM invariants.  The guess's own period (21.7 s, 7.2 s per interval) is far outside the
    stability region of four RK4 steps (the Baumgarte poles at -10 /s alone ask for a step below 0.28 s: the
    host loop returns NaN there), so the point's t_f is 1.2 s: 0.4 s per interval, 0.1 s per step."""

    T_F = 1.2

    def __init__(self, n_inst=2, seed=7):
        self.c = c = pb.build_constants(pb.Ap2Config(n_k=3, d=2))
        self.lay = lay = pb.NlpLayout(3, 2)
        v0 = initial_guess(c, lay)
        P1 = pb.pack_p(lay, c, v0, step="power1")
        rng = np.random.default_rng(seed)
        V = np.stack([v0] * n_inst)
        V[:, lay.theta()[1]] = self.T_F
        for b in range(n_inst):
            nodes = [lay.x(k) for k in range(lay.n_k + 1)] + [lay.coll_x(k, j) for k in range(lay.n_k)
                                                              for j in range(lay.d)]
            for idx in nodes:       # the collocation states too: the interval's energy is not zero then
                for name in ("omega10", "delta10", "dl_t"):
                    o, sz = pb.W_OFF[("x", name)]
                    V[b, idx[o:o + sz]] += 0.05 * rng.standard_normal(sz)
            for k in range(lay.n_k):
                V[b, lay.u(k)[6:]] += 0.05 * rng.standard_normal(4)          # ddelta10, ddl_t
        self.V, self.P = V, np.stack([P1] * n_inst)
        self.h = V[:, lay.theta()[1]] * c.scaling[pb.W_TH0 + 1] / lay.n_k

    def task(self, k):
        """(x0, u [B, 1, 10], y0, par) of interval k of every instance."""
        V, P, lay = self.V, self.P, self.lay
        par = evm.rk4root_par(V[:, lay.theta()], V[:, lay.phi("gamma")], P[:, lay.p_theta0:lay.p_theta0 + pb.NTHETA0])
        return (V[:, lay.x(k)].copy(), V[:, lay.u(k)][:, None, :].copy(),
                np.concatenate([V[:, lay.xdot(k)], V[:, lay.z(k)]], axis=1), par)

    def core(self, n_fe, k=1, ts=None, n_steps=1, consts=None, x0=None, u=None, y0=None, par=None, **kw):
        """The host core on interval k's task; any input replaced, ts a number for every task (default: the
        instances' own interval lengths)."""
        t = self.task(k)
        x0, u, y0, par = (t[i] if a is None else a for i, a in enumerate((x0, u, y0, par)))
        ts = self.h if ts is None else np.full(len(x0), ts)
        return evm.integrate_rk4root_cpu(self.c if consts is None else consts, x0, u, y0, par, ts, n_fe, n_steps, **kw)


@pytest.fixture(scope="module")
def start():
    return Start()


def test_library_exports_and_binds_the_rk4root_header():
    """libawegpu.so exports what include/awegpu_rk4root.h declares, and the binding's table has every
    prototype with as many argtypes as it has parameters (tests/test_library.py does this for awegpu.h)."""
    import re
    text = open(os.path.join(ROOT, "include", "awegpu_rk4root.h")).read()
    protos = re.findall(r"^int\s+(awe_\w+)\(([^)]*)\)\s*;", text, re.M)
    assert {n for n, _ in protos} == set(evm.RK4ROOT_SYMBOLS) == set(re.findall(r"^int\s+(awe_\w+)\(", text, re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", B.LIB], capture_output=True, text=True, check=True).stdout
    assert set(evm.RK4ROOT_SYMBOLS) <= set(re.findall(r"\bT (awe_\w+)", out))
    lib = evm.load_library()
    for name, params in protos:
        assert len(getattr(lib, name).argtypes) == params.count(",") + 1, name


# ---- generated code ---------------------------------------------------------------------------------
def test_committed_root_header_is_current():
    """ap2_noderoot.gen.hpp in the tree is what gen/ap2_rootgen.cpp writes for the current model."""
    before = open(B.AP2_ROOT_HEADER).read()
    B.generate(force=True)
    assert open(B.AP2_ROOT_HEADER).read() == before, "ap2_noderoot.gen.hpp is stale: run python -m awebox_amd.build"


@pytest.fixture(scope="module")
def root_checker(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ap2root")
    exe = str(tmp / "check_ap2root")
    subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(CSRC, "gen", "check_ap2_root.cpp"), "-o", exe], check=True)
    return tmp, exe


@pytest.mark.parametrize("k,seed", [(0, 0), (1, 1), (2, 2)])
def test_generated_root_code_matches_dual_model(root_checker, start, k, seed):
    """The 24 rows, every emitted tangent and the power integrand against one dual-number pass of ap2_node
    per unknown (csrc/gen/check_ap2_root.cpp) with the bounds of test_codegen.py, at perturbed nodes; every
    slot is a pattern entry; the partition is the expected one (17 explicit rows, K = 7, found from the
    tape); the structured Newton step equals the dense 24 x 24 LU step of that Jacobian to rounding."""
    tmp, exe = root_checker
    c, lay, V = start.c, start.lay, start.V[0]
    rng = np.random.default_rng(seed)
    w = np.concatenate([V[lay.x(k)], V[lay.xdot(k)], V[lay.u(k)], V[lay.z(k)], V[lay.theta()], V[lay.phi()][:1]])
    w = w * (1 + 0.05 * rng.standard_normal(w.shape)) + 0.01 * rng.standard_normal(w.shape)
    th = c.theta0.copy()
    th[pb.THETA0_OFF["wind.u_ref"][0]] = 6.0 + 6.0 * rng.random()
    for name, a in (("consts", c.consts), ("w", w), ("th", th)):
        np.savetxt(str(tmp / f"{name}.txt"), a)
    out = subprocess.run([exe] + [str(tmp / f"{n}.txt") for n in ("consts", "w", "th")], check=True,
                         capture_output=True, text=True)
    r = json.loads(out.stdout)
    print(r)
    assert r["entries"] == r["n_slots"] == r["entry_table"], "every slot is a pattern entry, both tables agree"
    assert (r["K"], r["explicit"]) == (7, 17)
    assert r["value_rel"] < 1e-14, r
    assert r["integrand_rel"] < 1e-14, r
    assert r["entry_rel"] < 1e-12, r
    assert r["entry_max"] > 1.0 and r["step_max"] > 1e-3
    assert r["step_rel"] < STEP_BOUND, r


# ---- the integrator core on the host ------------------------------------------------------------------
def test_host_core_matches_independent_host_loop(start):
    """awe_integrate_rk4root_cpu against IntervalIntegrator.rk4root on the CPU port of the NLP, 2 instances,
    interval 1, n_fe = 4: every rootfinder of both sides below 1e-10 (the host loop alone first), then x_end,
    (xdot, z) at the end and the energy within the project's parity tolerance."""
    from oracle.cpu_device import CpuDeviceEvaluator
    c, lay, k = start.c, start.lay, 1
    integ = IntervalIntegrator(CpuDeviceEvaluator(c), lay, c.scaling, k=k, device="cpu")
    Vt, Pt = torch.tensor(start.V), torch.tensor(start.P)
    ref = integ.rk4root(Vt, Pt, hm.power_integrand(c), torch.tensor(start.h), n_steps=4)
    assert float(ref["residual"].max()) < 1e-10, ref["residual"]
    # (xdot, z) at the end: the loop's last rootfinder ran at x_end from the state the loop left in its copy
    # of V, which it does not return; one more call from x_end with zero steps' worth of motion restates it
    Vend = Vt.clone()
    Vend[:, integ.x_idx] = ref["x_end"]
    Vend[:, integ.xdot_idx], Vend[:, integ.z_idx] = torch.tensor(start.V[:, lay.xdot(k)]), ref["z_end"]
    res_end = integ._newton(Vend, Pt, integ.rk, 20, 1e-12)
    assert float(res_end.max()) < 1e-10
    y_ref = torch.cat([Vend[:, integ.xdot_idx], Vend[:, integ.z_idx]], dim=1).numpy()
    out = start.core(n_fe=4)
    print("res", out["res"], ref["residual"].numpy(), "x diff", np.abs(out["xf"][:, 0] - ref["x_end"].numpy()).max(),
          "y diff", np.abs(out["yf"] - y_ref).max(), "q", out["qf"][:, 0], ref["q"].numpy())
    assert out["res"].max() < 1e-10
    assert parity(out["xf"][:, 0], ref["x_end"].numpy())
    assert parity(out["yf"], y_ref)
    assert parity(out["qf"][:, 0], ref["q"].numpy())
    assert np.abs(ref["q"].numpy()).min() > 0.0
    assert np.abs(out["xf"][:, 0] - start.V[:, lay.x(k)]).max() > 1e-3, "the state moved"


def test_order_of_convergence(start):
    """Classical RK4: against the core's own n_fe = 64 the error of n_fe = 2, 4, 8 falls by a factor between
    12 and 20 per halving of the step (16 for order 4).  The sampling time is 0.05 s: the fastest poles of the
    model are the Baumgarte ones at -10 /s, and the coarsest step (n_fe = 2, 0.025 s) has to sit at
    |h lambda| = 0.25, well inside the asymptotic range, for the ratio to be the order's."""
    ref = start.core(n_fe=64, ts=0.05)["xf"][:, 0]
    err = [np.abs(start.core(n_fe=n, ts=0.05)["xf"][:, 0] - ref).max() for n in (2, 4, 8)]
    print("errors", err, "factors", err[0] / err[1], err[1] / err[2])
    for a, b in zip(err, err[1:]):
        assert 12.0 <= a / b <= 20.0, err


def test_chained_calls_equal_one_call(start):
    """n_steps = 3 in one call is three n_steps = 1 calls chained (xf -> x0, yf -> y0), bitwise."""
    rng = np.random.default_rng(5)
    x0, u1, y0, par = start.task(1)
    u = np.repeat(u1, 3, axis=1)
    u[:, :, 6:] += 0.05 * rng.standard_normal((2, 3, 4))
    one = start.core(n_fe=3, n_steps=3, u=u)
    x, y = x0, y0
    for s in range(3):
        o = start.core(n_fe=3, u=np.ascontiguousarray(u[:, s:s + 1]), x0=x, y0=y)
        x, y = np.ascontiguousarray(o["xf"][:, 0]), o["yf"]
        assert np.array_equal(o["xf"][:, 0], one["xf"][:, s])
        assert np.array_equal(o["qf"][:, 0], one["qf"][:, s])
    assert np.array_equal(y, one["yf"])
    assert np.isfinite(one["xf"]).all() and one["res"].max() < 1e-10
    assert not np.array_equal(one["xf"][:, 0], one["xf"][:, 1])


def test_nan_task_is_isolated(start):
    """A task with a NaN in its state runs to the end with a non-finite residual; the other tasks' bits are
    those of the call without it."""
    x0, u, y0, par = start.task(1)
    three = lambda a: np.ascontiguousarray(np.concatenate([a, a[:1]]))   # noqa: E731
    x3 = three(x0)
    x3[1, 7] = np.nan
    clean = start.core(n_fe=4)
    out = start.core(n_fe=4, x0=x3, u=three(u), y0=three(y0), par=three(par), ts=start.h[0])
    assert not np.isfinite(out["res"][1])
    for name in ("xf", "yf", "qf", "res"):
        assert np.array_equal(out[name][0], clean[name][0]) and np.array_equal(out[name][2], clean[name][0]), name


@pytest.mark.parametrize("kw,word", [({"n_fe": 0}, "n_fe"), ({"n_fe": 2, "n_steps": 0}, "n_steps"),
                                     ({"n_fe": 2, "max_newton": -1}, "max_newton")])
def test_bad_arguments_are_errors(start, kw, word):
    with pytest.raises(AwegpuError, match=word):
        start.core(**kw)


def test_constants_of_another_structure_are_refused(start):
    """The generated code is for a fixed tether element count and fixed stability-table lengths; other
    constants, or a vector of another length, are an error with a message."""
    c = start.c.consts.copy()
    c[pb.CONST_IDX["n_elements"]] += 1.0
    with pytest.raises(AwegpuError, match="tether elements"):
        start.core(n_fe=2, consts=c)
    c = start.c.consts.copy()
    c[pb.CONST_IDX["sd_len0"] + 1] += 1.0
    with pytest.raises(AwegpuError, match="stability-table"):
        start.core(n_fe=2, consts=c)
    with pytest.raises(AwegpuError, match="constants"):
        start.core(n_fe=2, consts=start.c.consts[:-1])
    with pytest.raises(ValueError):
        start.core(n_fe=2, x0=start.task(1)[0][:, :-1])


def test_reintegrate_on_the_host(start):
    """reintegrate(device="cpu"): n_k rows per instance, finite residuals, task (b, k) is interval k of
    instance b (its end state is the core's for that interval alone) and its x error is taken against
    V.x[k + 1]."""
    lay = start.lay
    r = reintegrate(None, lay, start.c, start.V, start.P, n_fe=4, device="cpu")
    for name in ("x", "z", "q", "residual"):
        assert tuple(r[name].shape) == (2, lay.n_k) and bool(torch.isfinite(r[name]).all()), name
    assert float(r["residual"].max()) < 1e-10
    for k in range(lay.n_k):
        alone = start.core(n_fe=4, k=k)
        assert np.array_equal(r["x_end"][:, k].numpy(), alone["xf"][:, 0])
        assert np.array_equal(r["q_end"][:, k].numpy(), alone["qf"][:, 0])
        exp = start.V[:, lay.x(k + 1)]
        err = np.abs(alone["xf"][:, 0] - exp).max(axis=1) / np.abs(exp).max(axis=1)
        assert np.allclose(r["x"][:, k].numpy(), err, rtol=1e-12, atol=0.0)
        e_q = np.array([hm.interval_energy(start.c, lay, start.V[b], k) for b in range(2)])
        assert np.allclose(r["q"][:, k].numpy(), np.abs(alone["qf"][:, 0] - e_q) / np.abs(e_q), rtol=1e-9, atol=0.0)
