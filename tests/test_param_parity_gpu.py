"""Every kernel family against the oracle with every entry of P moved (tests/param_cases.py), on an
MI355X: each family stages P, indexes the costs and weights and runs its finalize pass in code of its
own, and the other parity tests move V generously but P hardly (u_ref, three schedule steps, the MPC's
Q).  tests/test_param_reach.py shows on the CPU that at these inputs every entry the model reads moves
some output by at least 10 tolerances, so a family that reads a wrong entry fails here.

Tolerances are those of tests/test_gpu_parity.py (1e-9 |b| + 1e-11 max|b|, per column for J_g, relative
1e-12 for f), imported, not restated.  Shapes are the smallest that reach each branch; the oracle's
outputs of a shape are computed once and shared."""
import numpy as np
import pytest

from awebox_amd import problem as pb
from awebox_amd.initial_guess import initial_guess

import param_cases as pc
from test_gpu_parity import ATOL_REL, RTOL, _close, _close_hess, _close_jac, _oracle_all

pytestmark = pytest.mark.gpu

AP2_SHAPES = [(3, 2), (2, 5)]
AP2_PATHS = ["colour", "generated", "soa"]
_CACHE = {}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test on a machine without a visible GPU")
    from awebox_amd.build import build
    build()
    return torch


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- AP2 ----------------------------------------------------------------------------------------------
class Ap2Case:
    """B instances of ap2_full_p at (n_k, d), seeds 0..B-1, and the oracle's outputs of ``members``."""

    def __init__(self, n_k, d, B, members):
        from oracle.ap2_oracle import from_problem
        self.consts = pb.build_constants(pb.Ap2Config(n_k=n_k, d=d))
        self.lay = lay = pb.NlpLayout(n_k, d)
        v0 = initial_guess(self.consts, lay)
        cases = [pc.ap2_full_p(self.consts, lay, v0, seed=b) for b in range(B)]
        self.V, self.P = np.stack([c.V for c in cases]), np.stack([c.P for c in cases])
        self.B, self.members = B, members
        self.orc = from_problem(self.consts, n_k=n_k, d=d)
        self.ref = {b: _oracle_all(self.orc, lay, self.V[b], self.P[b]) for b in members}
        self.dead = pc.ap2_dead_entries(self.consts, lay)
        rng = np.random.default_rng(100 * n_k + d)
        self.sigma = np.array([1.3, 0.0, 0.6] + [1.0] * (B - 3))[:B]
        self.lam = rng.standard_normal((B, lay.n_g))
        self._hess = {}

    def hess_ref(self, b):
        if b not in self._hess:
            self._hess[b] = self.orc.nlp_hess_l(self.V[b], self.P[b], self.sigma[b], self.lam[b], self.lay,
                                                pb.THETA0_OFF, pb.COST_NAMES, pb.PHI_NAMES)
        return self._hess[b]

    def evaluator(self):
        from awebox_amd.evaluator import Ap2Evaluator
        return Ap2Evaluator(self.consts, batch=self.B)

    def check(self, ev, out, what):
        for b in self.members:
            f, g, grad, J = self.ref[b]
            assert out["f"][b] == pytest.approx(f, rel=1e-12), f"{what}: f[{b}]"
            _close(out["g"][b], g, f"{what}: g[{b}]")
            _close(out["grad_f"][b], grad, f"{what}: grad_f[{b}]")
            _close_jac(ev.jac_csc(out["jac"][b]), J, f"{what}: J[{b}]")


def _ap2(n_k, d, B=3, members=(0, 1, 2)):
    return _cached(("ap2", n_k, d, B), lambda: Ap2Case(n_k, d, B, members))


@pytest.mark.parametrize("path", AP2_PATHS)
@pytest.mark.parametrize("n_k,d", AP2_SHAPES)
def test_ap2_first_order_matches_oracle(gpu, n_k, d, path):
    """f, g, grad f and J_g of three instances, each with its own weights, costs, theta0 and p.ref, on the
    colour kernel, the node + gather path and the instance-minor path."""
    case = _ap2(n_k, d)
    ev = case.evaluator()
    ev.path = path
    assert ev.path == path
    case.check(ev, ev.eval_nlp(case.V, case.P), path)


@pytest.mark.parametrize("n_k,d", AP2_SHAPES)
def test_ap2_value_only_kernel_matches_oracle(gpu, n_k, d):
    """eval_f and eval_g (the value-only kernel: its own staging of P and its own objective sum)."""
    case = _ap2(n_k, d)
    ev = case.evaluator()
    f, g = ev.eval_f(case.V, case.P), ev.eval_g(case.V, case.P)
    for b in case.members:
        assert f[b] == pytest.approx(case.ref[b][0], rel=1e-12), f"f[{b}]"
        _close(g[b], case.ref[b][1], f"g[{b}]")


def _device_eval(torch, ev, V, P, inputs_im):
    """One call with instance-minor outputs: awe_eval_nlp_imv with instance-minor V and P (alloc_inputs),
    else awe_eval_nlp_im; outputs pre-filled with NaN."""
    B = ev.batch
    nan = lambda *s: torch.full(s, np.nan, dtype=torch.float64, device="cuda")   # noqa: E731
    Vt, Pt = torch.tensor(V, device="cuda"), torch.tensor(P, device="cuda")
    if inputs_im:
        Vi, Pi = ev.alloc_inputs("cuda")
        Vi.copy_(Vt)
        Pi.copy_(Pt)
        Vt, Pt = Vi, Pi
    f, g = nan(B), nan(B, ev.n_g)
    gr, jac = ev.alloc_grad("cuda", instance_minor=True), ev.alloc_jac("cuda", instance_minor=True)
    gr.fill_(np.nan)
    jac.fill_(np.nan)
    ev.eval_nlp_device(Vt, Pt, f, g, gr, jac)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in (("f", f), ("g", g), ("grad_f", gr), ("jac", jac))}


def test_ap2_instance_minor_block_and_ragged_lane(gpu):
    """(3, 2) with B = 65, one full block of 64 lanes and a ragged one, through awe_eval_nlp_im and
    awe_eval_nlp_imv: instances 0, 63 and 64 against the oracle, all 65 against the node + gather path."""
    torch = gpu
    case = _ap2(3, 2, 65, (0, 63, 64))
    ev = case.evaluator()
    ev.path = "generated"
    ref = ev.eval_nlp(case.V, case.P)
    case.check(ev, ref, "node + gather")
    ev.path = "soa"
    for inputs_im in (False, True):
        what = "imv" if inputs_im else "im"
        out = _device_eval(torch, ev, case.V, case.P, inputs_im)
        assert all(np.isfinite(a).all() for a in out.values()), what
        case.check(ev, out, what)
        for b in range(case.B):
            assert out["f"][b] == pytest.approx(ref["f"][b], rel=1e-12), f"{what}: f[{b}]"
            for k in ("g", "grad_f", "jac"):
                _close(out[k][b], ref[k][b], f"{what}: {k}[{b}] vs node + gather")


@pytest.mark.parametrize("hess", ["hyperdual", "generated"])
@pytest.mark.parametrize("n_k,d", AP2_SHAPES)
def test_ap2_hessian_matches_oracle(gpu, n_k, d, hess):
    """nlp_hess_l of three instances with their own sigma (one of them 0) and multipliers on both Hessian
    kernels; the instance-minor output equals the per-instance one bitwise."""
    torch = gpu
    case = _ap2(n_k, d)
    ev = case.evaluator()
    ev.hess_path = hess
    assert ev.hess_path == hess and 0.0 in case.sigma
    H = ev.eval_hess(case.V, case.P, case.sigma, case.lam)
    for b in case.members:
        _close_hess(ev.hess_csc(H[b]), case.hess_ref(b), f"{hess}: H[{b}]")
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda")   # noqa: E731
    Him = ev.alloc_hess()
    ev.eval_hess_device_im(dev(case.V), dev(case.P), dev(case.sigma), dev(case.lam), Him)
    torch.cuda.synchronize()
    assert np.array_equal(Him.cpu().numpy(), H)


@pytest.mark.parametrize("hess", ["hyperdual", "generated"])
def test_ap2_hessian_tf_tf_entry_carries_the_time_cost(gpu, hess):
    """H[t_f, t_f] differs from the same call with cost["t_f"] = 0 by 2 sigma cost_tf.  Both calls share
    every other term of the entry, each is within the parity tolerance of its exact value, so the
    difference is within twice that tolerance (RTOL |H_tt| + ATOL_REL max|H|)."""
    case = _ap2(3, 2)
    lay = case.lay
    ev = case.evaluator()
    ev.hess_path = hess
    i_tf = int(lay.theta()[1])
    i_c = lay.p_cost + pb.COST_NAMES.index("t_f")
    P0 = case.P.copy()
    P0[:, i_c] = 0.0
    H = ev.eval_hess(case.V, case.P, case.sigma, case.lam)
    H0 = ev.eval_hess(case.V, P0, case.sigma, case.lam)
    for b in range(case.B):
        A, A0 = ev.hess_csc(H[b]), ev.hess_csc(H0[b])
        want = 2.0 * case.sigma[b] * case.P[b, i_c]
        tol = 2.0 * (RTOL * abs(A[i_tf, i_tf]) + ATOL_REL * abs(A).max())
        print(hess, b, "H_tt", A[i_tf, i_tf], "without", A0[i_tf, i_tf], "want", want, "tol", tol)
        assert abs((A[i_tf, i_tf] - A0[i_tf, i_tf]) - want) <= tol
        assert tol < 1e-3 * 2.0 * pc.LO                       # the check can see the term (cost_tf >= LO)
        D = (A - A0).tolil()
        D[i_tf, i_tf] = 0.0
        assert abs(D.tocsc()).max() == 0.0, "cost.t_f reaches no other entry"


def test_ap2_dead_entries_are_not_read(gpu):
    """The entries of P that the model does not have (param_cases.ap2_dead_entries) overwritten with
    distinct large values: every output of every path is bitwise the one from before."""
    case = _ap2(3, 2)
    Q = pc.with_dead_overwritten(case.P, case.dead)
    assert not np.array_equal(Q, case.P)
    ev = case.evaluator()
    for path in AP2_PATHS:
        ev.path = path
        a, b = ev.eval_nlp(case.V, case.P), ev.eval_nlp(case.V, Q)
        for k in a:
            assert np.array_equal(a[k], b[k]), (path, k)
    assert np.array_equal(ev.eval_f(case.V, case.P), ev.eval_f(case.V, Q))
    assert np.array_equal(ev.eval_g(case.V, case.P), ev.eval_g(case.V, Q))
    for hess in ("hyperdual", "generated"):
        ev.hess_path = hess
        assert np.array_equal(ev.eval_hess(case.V, case.P, case.sigma, case.lam),
                              ev.eval_hess(case.V, Q, case.sigma, case.lam)), hess


def test_ap2_rk4root_parameter_rows_with_full_theta0(gpu):
    """awe_integrate_rk4root against awe_integrate_rk4root_cpu with every theta0 entry of every task
    moved by a multiplier of its own (param_cases: the zeros of geometry.j filled too); the other rk4root
    tests differ in wind.u_ref only.  Shape and tolerance of test_ap2_rk4root_gpu.py's smallest case
    (n_fe = 4, one sampling time; parity, rootfinder residuals below 1e-10), nine tasks: the three
    intervals of three instances."""
    torch = gpu
    from awebox_amd import evaluator as evm
    from test_ap2_rk4root import Start, parity
    s = Start(n_inst=3, seed=31)
    for b in range(3):
        s.P[b, s.lay.p_theta0:] = pc.theta0_block(s.c.theta0, np.random.default_rng([2, b]))[0]
    parts = [s.task(k) for k in range(s.lay.n_k)]
    x0, u, y0, par = (np.ascontiguousarray(np.concatenate([p[i] for p in parts])) for i in range(4))
    assert len(np.unique(par[:, 3:], axis=0)) == 3 and len(x0) == 9
    ts = np.tile(s.h, s.lay.n_k)
    ref = evm.integrate_rk4root_cpu(s.c, x0, u, y0, par, ts, 4, 1)
    ev = evm.Ap2Evaluator(s.c, batch=1)
    xf, yf, qf, res = ev.integrate_rk4root(*(torch.tensor(a, device="cuda") for a in (x0, u, y0, par, ts)), 4, 1)
    torch.cuda.synchronize()
    print("res", float(res.max()), ref["res"].max())
    assert float(res.max()) < 1e-10 and ref["res"].max() < 1e-10
    assert parity(xf.cpu().numpy(), ref["xf"])
    assert parity(yf.cpu().numpy(), ref["yf"])
    assert parity(qf.cpu().numpy(), ref["qf"])


# ---- dual kites ---------------------------------------------------------------------------------------
class DualCase:
    """B instances of dual_full_p at (n_k, d) in one layout, and the oracle's outputs of three of them (J_g
    by one jacfwd of the whole g at d < 4, by per-interval blocks at d = 4, where the former takes 8 s)."""

    def __init__(self, n_k, d, B, phase_fix):
        from awebox_amd import dual as du
        from oracle import multikite_oracle as mo
        self.mc = du.build_constants(du.MultiConfig(n_k=n_k, d=d, phase_fix=phase_fix))
        self.lay = lay = du.layout_for(self.mc)
        V0 = du.initial_guess(self.mc, lay)
        cases = [pc.dual_full_p(self.mc, lay, V0, seed=b) for b in range(B)]
        self.V, self.P = np.stack([c.V for c in cases]), np.stack([c.P for c in cases])
        self.B, self.members = B, sorted({0, B // 2, B - 1})
        orc = mo.from_constants(self.mc, lay)
        self.ref = {}
        for b in self.members:
            th = mo.theta0_dict(self.P[b, lay.p_theta0:])
            self.ref[b] = (float(orc.nlp_f(self.V[b], self.P[b], lay, th, pb.COST_NAMES, pb.PHI_NAMES)),
                           orc.nlp_g(self.V[b], self.P[b], lay, th).numpy(),
                           orc.nlp_grad_f(self.V[b], self.P[b], lay, th, pb.COST_NAMES, pb.PHI_NAMES).numpy(),
                           (orc.nlp_jac_g_sparse if d >= 4 else orc.nlp_jac_g)(self.V[b], self.P[b], lay, th))


def _dual_eval(torch, ev, V, P, instance_minor):
    """The colour kernel (contiguous outputs) or the generated node code (instance-minor outputs)."""
    B = ev.batch
    f = torch.full((B,), np.nan, dtype=torch.float64, device="cuda")
    g = torch.full((B, ev.n_g), np.nan, dtype=torch.float64, device="cuda")
    gr, jac = ev.alloc_grad("cuda", instance_minor=instance_minor), ev.alloc_jac("cuda", instance_minor=instance_minor)
    gr.fill_(np.nan)
    jac.fill_(np.nan)
    ev.eval_nlp_device(torch.tensor(V, device="cuda"), torch.tensor(P, device="cuda"), f, g, gr, jac)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (f, g, gr, jac)]


@pytest.mark.parametrize("n_k,d,B,phase_fix", [(5, 3, 3, "single_reelout"), (5, 4, 65, "single_reelout"),
                                               (5, 3, 3, "simple"), (5, 4, 2, "simple")])
def test_dual_paths_match_oracle(gpu, n_k, d, B, phase_fix):
    """The colour kernel and, where it exists (the generated node code is instantiated for d = 4 only), the
    generated path at dual_full_p: three instances against the oracle, the generated path against the
    colour kernel for all; ``single_reelout`` with its two t_f (B = 65: a full block of lanes and a ragged
    one) and the plain layout with one; then the model's dead entries overwritten, bitwise on every path."""
    torch = gpu
    from awebox_amd.dual_evaluator import DualEvaluator
    case = _cached(("dual", n_k, d, B, phase_fix), lambda: DualCase(n_k, d, B, phase_fix))
    lay = case.lay
    assert lay.single_reelout == (phase_fix == "single_reelout") and lay.n_tf_rows == (2 if lay.single_reelout else 0)
    ev = DualEvaluator(case.mc, batch=B)
    assert ev.generated_available == (d == 4)
    paths = (False, True) if d == 4 else (False,)
    out = {im: _dual_eval(torch, ev, case.V, case.P, im) for im in paths}
    for im in paths:
        what = "generated" if im else "colour"
        fk, gk, grk, jk = out[im]
        assert all(np.isfinite(a).all() for a in out[im]), what
        for b in case.members:
            f, g, grad, J = case.ref[b]
            assert abs(fk[b] - f) <= 1e-12 * abs(f), f"{what}: f[{b}]"
            _close(gk[b], g, f"{what}: g[{b}]")
            _close(grk[b], grad, f"{what}: grad_f[{b}]")
            _close_jac(ev.jac_csc(jk[b]), J, f"{what}: J[{b}]")
    if True in paths:
        assert np.allclose(out[True][0], out[False][0], rtol=1e-12, atol=0)
        for b in range(B):
            for k, name in ((1, "g"), (2, "grad_f"), (3, "jac")):
                _close(out[True][k][b], out[False][k][b], f"{name}[{b}] vs colour")
    Q = pc.with_dead_overwritten(case.P, pc.dual_dead_entries(case.mc, lay))
    for im in paths:
        for a, b in zip(out[im], _dual_eval(torch, ev, case.V, Q, im)):
            assert np.array_equal(a, b), "dead entries read on the %s path" % ("generated" if im else "colour")


# ---- MPC ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_k,d,B", [(3, 2, 3), (5, 3, 65)])
def test_mpc_paths_and_hessian_match_oracle(gpu, n_k, d, B):
    """The dual-number kernel, the generated instance-minor path and the Hessian at mpc_full_p (x0, ref,
    u_ref, Q, R and the terminal P all drawn per instance): three instances against the oracle, the
    generated path against the dual-number kernel for all."""
    torch = gpu
    from awebox_amd import kite3 as k3
    from awebox_amd.mpc import MpcEvaluator
    from oracle.kite3_oracle import from_constants
    c = k3.build_constants(k3.Kite3Config(n_k=n_k, d=d))
    lay = k3.MpcLayout(n_k, d)
    orc = from_constants(c, lay)
    cases = [pc.mpc_full_p(c, lay, 13 * b, 64, seed=b) for b in range(B)]
    V, P = np.stack([x.V for x in cases]), np.stack([x.P for x in cases])
    ev = MpcEvaluator(c, batch=B)
    assert ev.generated_available
    out = {im: _dual_eval(torch, ev, V, P, im) for im in (False, True)}
    members = sorted({0, B // 2, B - 1})
    ref = {b: (float(orc.nlp_f(V[b], P[b], lay)), orc.nlp_g(V[b], P[b], lay).numpy(),
               orc.nlp_grad_f(V[b], P[b], lay).numpy(), orc.nlp_jac_g(V[b], P[b], lay)) for b in members}
    for im, what in ((False, "dual-number"), (True, "generated")):
        fk, gk, grk, jk = out[im]
        assert all(np.isfinite(a).all() for a in out[im]), what
        for b in members:
            f, g, grad, J = ref[b]
            assert abs(fk[b] - f) <= 1e-12 * abs(f), f"{what}: f[{b}]"
            _close(gk[b], g, f"{what}: g[{b}]")
            _close(grk[b], grad, f"{what}: grad_f[{b}]")
            _close_jac(ev.jac_csc(jk[b]), J, f"{what}: J[{b}]")
    assert np.allclose(out[True][0], out[False][0], rtol=1e-13, atol=0)
    for b in range(B):
        for k, name in ((1, "g"), (2, "grad_f"), (3, "jac")):
            _close(out[True][k][b], out[False][k][b], f"{name}[{b}] vs dual-number")
    rng = np.random.default_rng(3)
    sig, lam = rng.uniform(0.5, 2.0, B), rng.standard_normal((B, lay.n_g))
    sig[1] = 0.0
    H = ev.eval_hess(V, P, sig, lam)
    for b in members:
        _close_hess(ev.hess_csc(H[b]), orc.nlp_hess_l(V[b], P[b], sig[b], lam[b], lay), f"H[{b}]")
