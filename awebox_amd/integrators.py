"""DAE integrators over one shooting interval, on the HIP evaluator.

The reference re-integrates a solved trajectory with the DAE integrators of its multiple-shooting
discretisation to check the direct-collocation solution (test/reg/test_discretization.py:20-193):

* ``collocation``: CasADi's collocation integrator with the NLP's own scheme (radau, d = 4) and one
  step per interval (``nlp.integrator.num_steps_overwrite = 1``).  Its equations over one interval
  are the direct-collocation rows of that interval, so it reproduces ``V.x[k+1]`` to the NLP
  tolerance (the reference asserts 1e-7 relative);
* ``rk4root``: awebox's own RK4 with a rootfinder for the algebraic variables at every stage
  (``tools/integrator_routines.py:32-96``), 30 steps per interval in the test (2e-2 relative).

The awebox DAE treats the state derivatives as algebraic variables (``dae.fill_in_dae_variables``:
x = states, z = [xdot, z], p = [u, theta, params]): ode x' = xdot, alg 0 = F(x, xdot, u, z).  Both
integrators here solve exactly those rows with the HIP evaluator's values and Jacobian blocks:

* collocation: Newton on interval k's shooting-node rows and collocation rows in its interior
  unknowns (xdot[k], z[k], and the collocation states and algebraics), from V's values;
* rk4root: RK4 on x' = xdot(x) where xdot(x), z(x) solve the shooting-node rows at the stage state
  (Newton, warm-started from the previous stage); the quadrature (the power integral output,
  ``dynamics.py:318-330``) is integrated by the same RK4 stages.

All arithmetic is float64 on the evaluator's device; the small Newton systems (24 and 120 unknowns
for the AP2 kite) are dense solves.  ``integrand(x, z)`` returns the quadrature integrand per
instance from scaled states x [B, n_x] and algebraic variables z [B, n_z].

``IntervalIntegrator`` is the host loop: every Newton iteration of every stage evaluates the whole NLP.
``reintegrate`` and ``simulate_open_loop`` run rk4root fused instead -- one lane per (instance, interval)
or per instance, the whole integrator in one launch (``Ap2Evaluator.integrate_rk4root``) -- and are held to
``IntervalIntegrator.rk4root`` by the tests.
"""
from __future__ import annotations

import numpy as np
import torch


class IntervalIntegrator:
    """Integrators of interval ``k`` of a collocation NLP on the evaluator ``ev`` (batch B)."""

    def __init__(self, ev, lay, scaling, k: int = 0, device="cuda"):
        self.ev, self.lay, self.k = ev, lay, k
        self.dev = torch.device(device)
        t = lambda a: torch.tensor(np.asarray(a, dtype=np.int64), device=self.dev)  # noqa: E731
        colind, row = ev.sparsity_jac()
        jcol = np.repeat(np.arange(ev.n_v), np.diff(colind))
        d = lay.d
        nx = len(lay.x(k))

        def block(rows, cols):
            rsel = {int(r): i for i, r in enumerate(rows)}
            csel = {int(c): i for i, c in enumerate(cols)}
            if len(rsel) != len(csel):
                raise ValueError("rows and unknowns do not form a square system")
            keep = np.where(np.isin(row, rows) & np.isin(jcol, cols))[0]
            dst = np.array([rsel[int(row[e])] * len(rsel) + csel[int(jcol[e])] for e in keep], dtype=np.int64)
            return t(rows), t(cols), t(keep), t(dst), len(rsel)

        shoot_rows = lay.g_shooting(k)
        shoot_cols = np.concatenate([lay.xdot(k), lay.z(k)])
        self.rk = block(shoot_rows, shoot_cols)
        coll_rows = np.concatenate([shoot_rows] + [lay.g_coll(k, j) for j in range(d)])
        coll_cols = np.concatenate([shoot_cols] + [np.concatenate([lay.coll_x(k, j), lay.coll_z(k, j)])
                                                   for j in range(d)])
        self.co = block(coll_rows, coll_cols)
        self.x_idx = t(lay.x(k))
        self.xdot_idx = t(lay.xdot(k))
        self.xcol_idx = [t(lay.coll_x(k, j)) for j in range(d)]
        self.z_idx = t(lay.z(k))
        self.zcol_idx = [t(lay.coll_z(k, j)) for j in range(d)]
        s = np.asarray(scaling, dtype=np.float64)
        self.ratio = torch.tensor(s[nx:2 * nx] / s[:nx], device=self.dev)   # xdot_scaled -> d(x_scaled)/dt
        from .collocation import coefficients
        tau, C, D, w = coefficients(d, "radau")
        self.D = [float(v) for v in np.asarray(D, dtype=float)]
        self.w = [float(v) for v in np.asarray(w, dtype=float)]
        self._B = None

    def _buffers(self, B):
        if self._B != B:
            f64 = dict(dtype=torch.float64, device=self.dev)
            ev = self.ev
            self.f, self.g = torch.zeros(B, **f64), torch.zeros(B, ev.n_g, **f64)
            self.grad, self.jac = torch.zeros(B, ev.n_v, **f64), torch.zeros(B, ev.nnz, **f64)
            self._B = B

    def _newton(self, V, P, blk, max_newton, tol, damped=False):
        """Newton on the rows of ``blk`` in its unknowns, in place in V; with ``damped`` the step is
        halved until the max-norm residual decreases (per instance).  Returns the final residual."""
        rows, cols, keep, dst, n = blk
        B = V.shape[0]
        self._buffers(B)
        self.ev.eval_nlp_device(V, P, self.f, self.g, self.grad, self.jac)
        r = self.g[:, rows].clone()
        res = r.abs().amax(dim=1)
        for it in range(max_newton):
            if float(res.max()) < tol:
                break
            A = torch.zeros(B, n * n, dtype=torch.float64, device=self.dev)
            A[:, dst] = self.jac[:, keep]
            step = torch.linalg.solve(A.view(B, n, n), r.unsqueeze(-1)).squeeze(-1)
            base = V[:, cols].clone()
            a = torch.ones(B, 1, dtype=torch.float64, device=self.dev)
            for _ in range(30 if damped else 1):
                V[:, cols] = base - a * step
                self.ev.eval_nlp_device(V, P, self.f, self.g, self.grad, self.jac)
                r_t = self.g[:, rows]
                res_t = r_t.abs().amax(dim=1)
                bad = ~(res_t < res) & (res >= tol)
                if not damped or not bool(bad.any()):
                    break
                a = torch.where(bad.unsqueeze(1), 0.5 * a, a)
            r, res = r_t.clone(), res_t
        return res

    def collocation(self, V, P, integrand, h, x0=None, max_newton=30, tol=1e-12, warm=False):
        """One radau collocation step over the interval (length h [s] per instance, tensor [B]) from
        x0 (default: V.x[k]).  The Newton iteration starts from CasADi's collocation-integrator
        guess -- x0 and the shooting node's z at every collocation point -- unless ``warm`` (V's
        own collocation values).  Returns dict(x_end, z_end, q, residual, V) with the collocation
        unknowns solved in a copy of V."""
        Vp = V.clone()
        if x0 is not None:
            Vp[:, self.x_idx] = x0
        if not warm:
            for j in range(len(self.xcol_idx)):
                Vp[:, self.xcol_idx[j]] = Vp[:, self.x_idx]
                Vp[:, self.zcol_idx[j]] = Vp[:, self.z_idx]
        res = self._newton(Vp, P, self.co, max_newton, tol, damped=True)
        x_end = sum(self.D[r] * (Vp[:, self.x_idx] if r == 0 else Vp[:, self.xcol_idx[r - 1]])
                    for r in range(len(self.D)))
        q = sum(h * self.w[j] * integrand(Vp[:, self.xcol_idx[j]], Vp[:, self.zcol_idx[j]])
                for j in range(len(self.w)))
        z_end = Vp[:, self.zcol_idx[-1]]
        return {"x_end": x_end, "z_end": z_end, "q": q, "residual": res, "V": Vp}

    def rk4root(self, V, P, integrand, h, n_steps=30, x0=None, max_newton=20, tol=1e-12):
        """n_steps RK4 steps over the interval (length h [s], tensor [B]) with the stage rootfinder.
        Returns dict(x_end, z_end, q, residual) (z_end from the rootfinder at x_end)."""
        Vp = V.clone()
        x = (Vp[:, self.x_idx] if x0 is None else x0).clone()
        dt = (h / n_steps).unsqueeze(-1)
        worst = torch.zeros(V.shape[0], dtype=torch.float64, device=self.dev)

        def ode(xs):
            nonlocal worst
            Vp[:, self.x_idx] = xs
            res = self._newton(Vp, P, self.rk, max_newton, tol)
            worst = torch.maximum(worst, res)
            return Vp[:, self.xdot_idx] * self.ratio, integrand(xs, Vp[:, self.z_idx])

        q = torch.zeros(V.shape[0], dtype=torch.float64, device=self.dev)
        for _ in range(n_steps):
            k1, p1 = ode(x)
            k2, p2 = ode(x + 0.5 * dt * k1)
            k3, p3 = ode(x + 0.5 * dt * k2)
            k4, p4 = ode(x + dt * k3)
            x = x + dt * (k1 + 2.0 * k2 + 2.0 * k3 + k4) / 6.0
            q = q + dt[:, 0] * (p1 + 2.0 * p2 + 2.0 * p3 + p4) / 6.0
        ode(x)
        z_end = Vp[:, self.z_idx]
        return {"x_end": x, "z_end": z_end, "q": q, "residual": worst}


# ---- the fused rk4root: one lane per integration task (csrc/plant_rk4root.hpp on the generated node code) ----
def _as_torch(a, dev):
    return (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a), dtype=torch.float64)).to(
        device=dev, dtype=torch.float64)


def _run_rk4root(ev, consts, x0, u, y0, par, ts, n_fe, n_steps, max_newton, tol, device):
    """Both back ends behind one call on torch tensors: the kernel (``ev.integrate_rk4root``) on a CUDA
    device, the host core (``evaluator.integrate_rk4root_cpu``) with ``device="cpu"`` (``ev`` unused)."""
    args = [t.contiguous() for t in (x0, u, y0, par, ts)]
    if torch.device(device).type == "cpu":
        from .evaluator import integrate_rk4root_cpu
        o = integrate_rk4root_cpu(consts, *(t.numpy() for t in args), n_fe, n_steps, max_newton, tol)
        return tuple(torch.from_numpy(o[k]) for k in ("xf", "yf", "qf", "res"))
    return ev.integrate_rk4root(*args, n_fe, n_steps, max_newton, tol)


def reintegrate(ev, lay, consts, V, P, n_fe=30, device="cuda", max_newton=20, tol=1e-12):
    """The reference's rk4root check of a direct-collocation solution (test/reg/test_discretization.py:
    20-193) over ALL n_k intervals of every instance of V [B, n_v], P [B, n_p] in one launch: task
    (b, k) starts at x0 = V.x[k] with the control V.u[k] held, the rootfinder's guess (V.xdot[k], V.z[k])
    and takes n_fe RK4 steps over the interval t_f / n_k.  Returns a dict of [B, n_k] tensors: the three
    relative errors test_discretization.error defines, max |found - expected| / max |expected|, of

    * ``x``: the end state against V.x[k+1],
    * ``z``: the end algebraic variable against V.coll_z[k, d-1],
    * ``q``: the interval's energy against ``homotopy.interval_energy(k)``,

    the largest rootfinder ``residual``, and what was found: ``x_end`` [B, n_k, 23], ``z_end`` [B, n_k, 1],
    ``q_end`` [B, n_k].  ``device="cpu"`` runs the host core (``ev`` may then be None)."""
    from . import problem as pb
    from .evaluator import rk4root_par
    dev = torch.device(device)
    V, P = _as_torch(V, dev), _as_torch(P, dev)
    if V.dim() == 1:
        V, P = V[None], P[None]
    B, n_k, d = V.shape[0], lay.n_k, lay.d
    idx = lambda f: torch.as_tensor(np.stack([f(k) for k in range(n_k)]), device=dev)   # noqa: E731
    rows = lambda i: V[:, i].reshape(B * n_k, -1)                                       # noqa: E731
    x0, u = rows(idx(lay.x)), rows(idx(lay.u))
    y0 = torch.cat([rows(idx(lay.xdot)), rows(idx(lay.z))], dim=1)
    per_task = lambda a: a.repeat_interleave(n_k, dim=0)                                # noqa: E731
    th = V[:, torch.as_tensor(lay.theta(), device=dev)]
    par = rk4root_par(per_task(th), per_task(V[:, int(lay.phi("gamma"))]),
                      per_task(P[:, lay.p_theta0:lay.p_theta0 + pb.NTHETA0]))
    s = torch.as_tensor(np.asarray(consts.scaling), device=dev)
    t_f = th[:, 1] * s[pb.W_TH0 + 1]
    xf, yf, qf, res = _run_rk4root(ev, consts, x0, u.reshape(B * n_k, 1, pb.NU), y0, par, per_task(t_f / n_k),
                                   n_fe, 1, max_newton, tol, dev)
    x_end, z_end, q_end = xf.reshape(B, n_k, pb.NX), yf[:, pb.NX:].reshape(B, n_k, pb.NZ), qf.reshape(B, n_k)
    x_exp = V[:, idx(lambda k: lay.x(k + 1))]
    z_exp = V[:, idx(lambda k: lay.coll_z(k, d - 1))]
    # homotopy.interval_energy for every (instance, interval)
    w = torch.as_tensor(np.asarray(pb.collocation(d)[3], dtype=float), device=dev)
    o_l, o_dl, o_lam = pb.W_OFF[("x", "l_t")][0], pb.W_OFF[("x", "dl_t")][0], pb.W_OFF[("z", "lambda10")][0]
    q_exp = torch.zeros(B, n_k, dtype=torch.float64, device=dev)
    for j in range(d):
        cx = V[:, idx(lambda k: lay.coll_x(k, j))]
        lam = V[:, idx(lambda k: lay.coll_z(k, j))][..., 0]
        q_exp = q_exp + (t_f / n_k)[:, None] * w[j] * lam * s[o_lam] * cx[..., o_l] * s[o_l] * cx[..., o_dl] * s[o_dl]
    rel = lambda a, b: (a - b).abs().amax(dim=-1) / b.abs().amax(dim=-1)                # noqa: E731
    return {"x": rel(x_end, x_exp), "z": rel(z_end, z_exp), "q": (q_end - q_exp).abs() / q_exp.abs(),
            "residual": res.reshape(B, n_k), "x_end": x_end, "z_end": z_end, "q_end": q_end}


def simulate_open_loop(ev, consts, x0, u_seq, ts, n_fe=20, y0=None, theta=None, gamma=None, theta0=None,
                       max_newton=20, tol=1e-12, device="cuda"):
    """The reference's open-loop simulation (sim.py:72-78, 'open_loop': the integrator run forward on the
    trial's model under given controls) of the 6-DOF kite for B instances and ``n_steps =
    u_seq.shape[1]`` sampling times in one launch, without the host in the loop: x0 [B, 23] and u_seq
    [B, n_steps, 10] scaled, ts the length of a sampling time [s] (a number or [B]).  y0 [B, 24] is the
    rootfinder's first guess for (xdot, z) (default: xdot = 0, lambda = 1 scaled); theta [B, 2] (default: the
    fixed diameter), gamma [B] (default 0: no fictitious forces) and theta0 [B, NTHETA0] (default: the
    constants' own) complete the model.  Returns dict(x [B, n_steps, 23], y [B, 24] at the last state,
    q [B, n_steps] energy per sampling time [J], residual [B])."""
    from . import problem as pb
    from .evaluator import RK_NUNK, rk4root_par
    dev = torch.device(device)
    x0, u_seq = _as_torch(x0, dev), _as_torch(u_seq, dev)
    B, n_steps = x0.shape[0], u_seq.shape[1]
    f64 = dict(dtype=torch.float64, device=dev)
    if y0 is None:
        y0 = torch.zeros(B, RK_NUNK, **f64)
        y0[:, pb.NX:] = 1.0
    if theta is None:
        theta = torch.tensor([consts.cfg.diam_t_fixed / consts.scaling[pb.W_TH0], 0.0], **f64).expand(B, 2)
    gamma = torch.zeros(B, **f64) if gamma is None else _as_torch(gamma, dev)
    theta0 = torch.as_tensor(consts.theta0, **f64).expand(B, pb.NTHETA0) if theta0 is None else _as_torch(theta0, dev)
    ts = torch.as_tensor(ts, **f64).expand(B) if not isinstance(ts, torch.Tensor) or ts.dim() == 0 else ts.to(**f64)
    par = rk4root_par(_as_torch(theta, dev), gamma, theta0)
    xf, yf, qf, res = _run_rk4root(ev, consts, x0, u_seq, _as_torch(y0, dev), par, ts, n_fe, n_steps, max_newton,
                                   tol, dev)
    return {"x": xf, "y": yf, "q": qf, "residual": res}
