"""Periodic reference trajectories of the 3-DOF model and their interpolation into the tracking MPC's
reference windows.

The reference's ``Pmpc`` tracks an optimised periodic trajectory: ``__create_reference_interpolator``
and ``get_reference`` (pmpc.py:408-550) turn the periodic solution ``V_opt`` into the V-shaped
reference of the horizon starting at any time t (taken modulo the period), by one of two interpolators
(``mpc.ref_interpolator``): ``'poly'`` evaluates the collocation polynomial of the interval t falls in
(ocp/collocation.py:146-183, struct_operations.py:473-499), ``'spline'`` a spline through the node
values (pmpc.py:432-474; what examples/mpc_closed_loop.py:67 selects).

``PeriodicTrajectory`` holds such a trajectory on its own grid (n_k intervals of d Radau nodes over the
period T, independent of the MPC's horizon, degree and sampling time).  ``tables(kind)`` describes either
interpolant as piecewise polynomials -- the one form the HIP kernel and its host twin evaluate
(csrc/ref_pp.hpp, ``MpcEvaluator.reference_window``, ``mpc.reference_window_cpu``) -- and
``window_host`` restates the windows with scipy's interpolators, without the tables: the yardstick of
the tests.

Window contents (get_reference, pmpc.py:492-550): theta = (diam_t, N ts), phi = xi = 0; x[k] at
t0 + k ts; the collocation x and z at t0 + (k + tau_j) ts; u[k] at t0 + k ts; the shooting node's xdot and
z are what the trajectory holds for them, zero (as get_reference leaves them) unless it comes from
``from_simulation``, whose source windows carry the plant's values.  Times are reduced as
t - T floor(t / T).

Where this departs from the reference, on purpose:

* the spline's knots.  The reference feeds CasADi's ``bspline`` interpolant with the values and time
  grid of ``viz_tools.merge_x_values`` / ``merge_z_values``, helpers its tree does not contain; the
  knots here are 0 and every collocation time (Radau's tau_d = 1 supplies the interior shooting times
  and T), the period closed as pmpc.py:450,456 do (the last value placed at 0), and the spline is the
  not-a-knot cubic through them;
* the controls are held over their interval in both kinds.  The reference's spline mode splines a
  sampled staircase of the controls on its plot grid; that is not reproduced.

A time on a breakpoint is read from the piece it opens (``calculate_kdx``: tau = 0), except at the
collocation nodes, which are read from the piece they close: Radau's last node is an interval's end, and
``calculate_kdx`` would read its z from the next interval's polynomial, extrapolated to tau = 0.  With the
closing rule a window aligned with the trajectory's grid reproduces the stored nodes, z included.  At an
exact breakpoint of a general grid the held control is defined only to within an ulp of t, here as in
``calculate_kdx``; on grids of binary fractions it is exact.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import kite3 as k3
from .collocation import coefficients

KINDS = ("poly", "spline")
N_FICT = 3                        # the fictitious forces lead u (kite3.U_VARS)


def reduce_time(t, T):
    """t - T floor(t / T), the reduction every implementation of the window uses."""
    t = np.asarray(t, dtype=np.float64)
    return t - T * np.floor(t / T)


def _not_a_knot(knots: np.ndarray, y: np.ndarray) -> np.ndarray:
    """Coefficients [pieces, channels, 4] in s = (t - b_i) / h_i of the not-a-knot cubic spline through
    (knots, y [n + 1, channels]): the second derivatives M from the continuity of S' at the interior
    knots and of S''' at the second and the last-but-one."""
    n = len(knots) - 1
    if n < 3:
        raise ValueError("a not-a-knot cubic needs at least four knots")
    h = np.diff(knots)
    A = np.zeros((n + 1, n + 1))
    rhs = np.zeros((n + 1, y.shape[1]))
    slope = np.diff(y, axis=0) / h[:, None]
    for i in range(1, n):
        A[i, i - 1:i + 2] = h[i - 1], 2.0 * (h[i - 1] + h[i]), h[i]
        rhs[i] = 6.0 * (slope[i] - slope[i - 1])
    A[0, :3] = h[1], -(h[0] + h[1]), h[0]
    A[n, n - 2:] = h[n - 1], -(h[n - 2] + h[n - 1]), h[n - 2]
    M = np.linalg.solve(A, rhs)
    h2 = (h * h)[:, None]
    c = np.empty((n, y.shape[1], 4))
    c[:, :, 0] = y[:-1]
    c[:, :, 1] = (y[1:] - y[:-1]) - h2 * (2.0 * M[:-1] + M[1:]) / 6.0
    c[:, :, 2] = h2 * M[:-1] / 2.0
    c[:, :, 3] = h2 * (M[1:] - M[:-1]) / 6.0
    return c


@dataclass
class PeriodicTrajectory:
    """One period of a trajectory of the 3-DOF model on n_k intervals of d Radau nodes, scaled as V is:
    x [n_k, d + 1, NX] (shooting node, then the Radau nodes), z [n_k, d, NZ], u [n_k, NU]; diam_t [m].
    ``xdot0`` [n_k, NX] and ``z0`` [n_k, NZ] are the shooting nodes' xdot and z, zero by default."""
    T: float
    x: np.ndarray
    z: np.ndarray
    u: np.ndarray
    diam_t: float = k3.Kite3Config.diam_t
    xdot0: np.ndarray | None = None
    z0: np.ndarray | None = None
    n_k: int = field(init=False)
    d: int = field(init=False)

    def __post_init__(self):
        self.x = np.array(self.x, dtype=np.float64)
        self.n_k, self.d = self.x.shape[0], self.x.shape[1] - 1
        self.z = np.array(self.z, dtype=np.float64).reshape(self.n_k, self.d, k3.NZ)
        self.u = np.array(self.u, dtype=np.float64).reshape(self.n_k, k3.NU)
        self.xdot0 = np.zeros((self.n_k, k3.NX)) if self.xdot0 is None else np.array(self.xdot0, dtype=np.float64)
        self.z0 = np.zeros((self.n_k, k3.NZ)) if self.z0 is None else np.array(self.z0, dtype=np.float64)
        if self.x.shape != (self.n_k, self.d + 1, k3.NX) or self.d < 1 or self.n_k < 1:
            raise ValueError(f"x must be [n_k, d + 1, {k3.NX}]")
        if self.xdot0.shape != (self.n_k, k3.NX) or self.z0.shape != (self.n_k, k3.NZ):
            raise ValueError("xdot0 / z0 must be [n_k, NX] / [n_k, NZ]")
        if not (self.T > 0.0 and np.isfinite(self.T)):
            raise ValueError("the period must be positive and finite")
        self.T, self.diam_t = float(self.T), float(self.diam_t)
        self.tau = coefficients(self.d, "radau")[0]            # [0, tau_1 .. tau_d = 1]

    # ------------------------------------------------------------------ constructors ----
    @classmethod
    def from_v(cls, lay: k3.MpcLayout, V, period: float, diam_t: float = k3.Kite3Config.diam_t):
        """An ``MpcLayout``-shaped V (scaled) read as one period of ``period`` seconds: its n_k
        intervals' shooting states, collocation x and z, and held controls."""
        V = np.asarray(V, dtype=np.float64).ravel()
        if V.size != lay.n_v:
            raise ValueError(f"V has {V.size} entries, the layout {lay.n_v}")
        x = np.stack([np.stack([V[lay.x(k)]] + [V[lay.coll_x(k, j)] for j in range(lay.d)]) for k in range(lay.n_k)])
        z = np.stack([np.stack([V[lay.coll_z(k, j)] for j in range(lay.d)]) for k in range(lay.n_k)])
        u = np.stack([V[lay.u(k)] for k in range(lay.n_k)])
        return cls(period, x, z, u, diam_t)

    @classmethod
    def from_simulation(cls, rti, loop: int = 0):
        """The trajectory ``BatchedRti.simulate_reference`` stored for ``loop`` (``sim_blocks``,
        ``sim_xs``), with period n_nodes ts.  It is not periodic (see ``closure_gap``): windows that
        reach across the period's end jump there.  The shooting nodes' xdot and z are kept, as the
        windows of ``simulate_reference`` carry them."""
        if rti.sim_blocks is None:
            raise ValueError("no simulated reference: call simulate_reference first")
        lay = rti.lay
        blocks = rti.sim_blocks[loop].cpu().numpy()
        n, d, nx, nu, nz = blocks.shape[0], lay.d, k3.NX, k3.NU, k3.NZ
        c0 = 2 * nx + nu + nz
        coll = blocks[:, c0:].reshape(n, d, nx + nz)
        x = np.concatenate([blocks[:, None, :nx], coll[:, :, :nx]], axis=1)
        return cls(n * rti.consts.cfg.ts, x, coll[:, :, nx:], blocks[:, nx:nx + nu], rti.consts.cfg.diam_t,
                   xdot0=blocks[:, nx + nu:2 * nx + nu], z0=blocks[:, 2 * nx + nu:c0])

    @classmethod
    def from_function(cls, fn, T: float, n_k: int, d: int, z=1.0, u=None, diam_t: float = k3.Kite3Config.diam_t):
        """Samples ``fn(t [n]) -> x [n, NX]`` (scaled states; e.g. ``rti.orbit_states`` over the state
        scaling) at the grid's nodes; z is constant (the circle's scaled 1) and u zero unless given."""
        tau = coefficients(d, "radau")[0]
        t = (np.arange(n_k)[:, None] + tau[None, :]) * (T / n_k)
        x = np.asarray(fn(t.reshape(-1)), dtype=np.float64).reshape(n_k, d + 1, k3.NX)
        return cls(T, x, np.full((n_k, d, k3.NZ), float(z)), np.zeros((n_k, k3.NU)) if u is None else u, diam_t)

    # ------------------------------------------------------------------ files ------------
    ARRAYS = ("T", "x", "z", "u", "diam_t", "xdot0", "z0")

    def save(self, path):
        """An ``.npz`` of plain arrays (``ARRAYS``; INTEGRATION.md names them): data only."""
        with open(path, "wb") as fh:
            np.savez(fh, **{n: np.asarray(getattr(self, n), dtype=np.float64) for n in self.ARRAYS})

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as f:
            opt = {n: f[n] for n in ("xdot0", "z0") if n in f.files}
            return cls(float(f["T"]), f["x"], f["z"], f["u"], float(f["diam_t"]), **opt)

    # ------------------------------------------------------------------ description ------
    @property
    def closure_gap(self) -> float:
        """max |x(T) - x(0)|: reported, not enforced."""
        return float(np.abs(self.x[-1, -1] - self.x[0, 0]).max())

    def _held(self):
        """[n_k, NU + NX + NZ]: what an interval holds -- u (fictitious forces zero, pmpc.py:461), then
        the shooting node's xdot and z."""
        held = np.concatenate([self.u, self.xdot0, self.z0], axis=1)
        held[:, :N_FICT] = 0.0
        return held

    def _spline_knots(self):
        h = self.T / self.n_k
        knots = np.concatenate([[0.0], ((np.arange(self.n_k)[:, None] + self.tau[None, 1:]) * h).reshape(-1)])
        knots[-1] = self.T
        xv = np.concatenate([self.x[-1:, -1], self.x[:, 1:].reshape(-1, k3.NX)])
        zv = np.concatenate([self.z[-1:, -1], self.z.reshape(-1, k3.NZ)])
        return knots, xv, zv

    def tables(self, kind: str = "spline") -> dict:
        """The interpolant as piecewise polynomials: dict(period, diam_t, kind, grids) with grids "x",
        "z" and "u" (the held one: u, then the shooting node's xdot and z), each dict(breaks [pieces +
        1] ascending from 0 to T, degree, coef [pieces, channels, degree + 1]) in the local variable s =
        (t - b_i) / (b_{i+1} - b_i), lowest power first.  A channel whose values are all zero, and the
        fictitious forces, are identically zero (pmpc.py:453,461)."""
        if kind not in KINDS:
            raise ValueError(f"unknown interpolator {kind!r}: one of {KINDS}")
        edges = np.arange(self.n_k + 1) * (self.T / self.n_k)
        edges[-1] = self.T
        if kind == "poly":
            # monomial coefficients of the Lagrange polynomials: x through [0, tau_1 .. tau_d], z
            # through tau_1 .. tau_d (the reference's coeff_fun and coeff_fun_u)
            vx = np.vander(self.tau, increasing=True)
            vz = np.vander(self.tau[1:], increasing=True)
            cx = np.linalg.solve(vx[None], self.x).transpose(0, 2, 1)
            cz = np.linalg.solve(vz[None], self.z).transpose(0, 2, 1)
            gx, gz = (edges, cx), (edges, cz)
        else:
            knots, xv, zv = self._spline_knots()
            gx, gz = (knots, _not_a_knot(knots, xv)), (knots, _not_a_knot(knots, zv))
        grids = {}
        for name, (b, c) in (("x", gx), ("z", gz), ("u", (edges, self._held()[:, :, None]))):
            grids[name] = {"breaks": np.ascontiguousarray(b), "degree": c.shape[2] - 1,
                           "coef": np.ascontiguousarray(c)}
        return {"period": self.T, "diam_t": self.diam_t, "kind": kind, "grids": grids}

    # ------------------------------------------------------------------ yardstick --------
    def _eval_host(self, kind, t, closing=False):
        """(x [n, NX], z [n, NZ], held [n, NU + NX + NZ]) at reduced times t, by scipy's interpolators.
        ``closing``: a time on an interval's end is read from that interval (tau = 1), not the next."""
        from scipy.interpolate import BarycentricInterpolator, make_interp_spline
        n_k = self.n_k
        q = n_k * t / self.T
        kdx = (np.ceil(q) - 1.0 if closing else np.floor(q)).astype(np.int64)    # calculate_kdx
        kdx = np.clip(kdx, 0, n_k - 1)                           # kdx == n_k: the last interval, tau = 1
        tau = t / self.T * n_k - kdx
        held = self._held()[kdx]
        if kind == "spline":
            knots, xv, zv = self._spline_knots()
            return make_interp_spline(knots, xv, k=3)(t), make_interp_spline(knots, zv, k=3)(t), held
        x, z = np.zeros((len(t), k3.NX)), np.zeros((len(t), k3.NZ))
        for k in np.unique(kdx):
            m = kdx == k
            x[m] = BarycentricInterpolator(self.tau, self.x[k])(tau[m])
            z[m] = BarycentricInterpolator(self.tau[1:], self.z[k])(tau[m])
        return x, z, held

    def window_host(self, kind: str, t0, lay: k3.MpcLayout, consts: k3.Kite3Constants) -> np.ndarray:
        """The windows [B, n_v] starting at t0 [B], restated with numpy and scipy
        (``BarycentricInterpolator`` per interval for 'poly', ``make_interp_spline(k=3)`` for 'spline')
        and never through ``tables``."""
        if kind not in KINDS:
            raise ValueError(f"unknown interpolator {kind!r}: one of {KINDS}")
        t0 = np.atleast_1d(np.asarray(t0, dtype=np.float64))
        B, nk, d, ts, s = len(t0), lay.n_k, lay.d, consts.cfg.ts, consts.scaling
        tau = coefficients(d, "radau")[0]
        ts_x = t0[:, None] + np.arange(nk + 1)[None, :] * ts
        ts_c = t0[:, None] + ((np.arange(nk)[:, None] + tau[None, 1:]) * ts).reshape(-1)[None, :]
        ts_u = t0[:, None] + np.arange(nk)[None, :] * ts

        def ev(tt, closing=False):
            return self._eval_host(kind, reduce_time(tt.reshape(-1), self.T), closing)

        xs = ev(ts_x)[0].reshape(B, nk + 1, k3.NX)
        xc, zc, _ = ev(ts_c, closing=True)
        xc, zc = xc.reshape(B, nk, d, k3.NX), zc.reshape(B, nk, d, k3.NZ)
        held = ev(ts_u)[2].reshape(B, nk, -1)
        zero_x = ~np.any(self.x != 0.0, axis=(0, 1))             # all-zero channels are identically zero
        zero_z = ~np.any(self.z != 0.0, axis=(0, 1))
        xs[:, :, zero_x], xc[:, :, :, zero_x], zc[:, :, :, zero_z] = 0.0, 0.0, 0.0
        R = np.zeros((B, lay.n_v))
        R[:, lay.theta()] = np.array([self.diam_t, nk * ts]) / s[2 * k3.NX + k3.NU + k3.NZ:]
        for k in range(nk + 1):
            R[:, lay.x(k)] = xs[:, k]
            if k < nk:
                R[:, lay.u(k)[0]:lay.z(k)[-1] + 1] = held[:, k]
                for j in range(d):
                    R[:, lay.coll_x(k, j)] = xc[:, k, j]
                    R[:, lay.coll_z(k, j)] = zc[:, k, j]
        return R
