"""Python side of the tracking-MPC boundary: ctypes binding of ``libawempc.so`` (include/awempc.h).

``MpcEvaluator`` exposes the NLP oracle surface the MPC's IPOPT solver reaches through
``ct.nlpsol('solver', 'ipopt', {'x': V, 'p': p, 'f': f, 'g': g})`` in ``awebox/pmpc.py:193-217``
(``nlp_f`` / ``nlp_g`` / ``nlp_grad_f`` / ``nlp_jac_g``, with x = V and p = the MPC parameter struct
``[x0, ref, u_ref, Q, R, P]``), plus the batched device path used for many MPC instances at once
(``nlp_binding.NlpEvaluator``).

There is no CPU fallback: a missing library or device raises ``AwegpuUnavailable``.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import kite3 as k3
from . import nlp_binding as nb
from .nlp_binding import DP, FP, IP, VP, H, I

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libawempc.so")
PREFIX = "awempc_"
SIGNATURES = {
    "hess_init": [H, IP],
    "gen_status": [H, IP],
    "last_kernel_ms_im": [H] + [FP] * 3,
    # x0, u, z0, par | ts, n_fe, n_steps, max_newton, tol | xf, zf, qf, res
    "plant_rk4root": [H] + [VP] * 4 + [ctypes.c_double, I, I, I, ctypes.c_double] + [VP] * 4 + [VP],
    "plant_rk4root_cpu": [DP, I, I] + [DP] * 4 + [ctypes.c_double, I, I, I, ctypes.c_double] + [DP] * 4,
    "last_plant_ms": [H, FP],
    # period, offs, head, pieces, degree, brk, coef
    "ref_set": [H, ctypes.c_double, DP, DP, IP, IP, DP, DP],
    "ref_window": [H, VP, VP, nb.Z, nb.Z, VP],
    "ref_window_cpu": [I, I, I, ctypes.c_double, DP, DP, IP, IP, DP, DP, DP, DP, nb.Z, nb.Z],
    "last_ref_ms": [H, FP],
}
REF_GRIDS = ("x", "z", "u")       # the grids of a reference table, in the library's order
REF_CHANNELS = {"x": k3.NX, "z": k3.NZ, "u": k3.NU + k3.NX + k3.NZ}
PLANT_NUNK = k3.NX + k3.NZ        # the rootfinder's unknowns: xdot (11), z.lambda
PLANT_NPAR = 4                    # theta.diam_t, theta.t_f, phi.gamma (scaled), u_ref
EXPORTED_SYMBOLS = nb.exported(PREFIX, SIGNATURES)


def load_library(path: str = _LIB_PATH):
    return nb.load(path, PREFIX, SIGNATURES)


def _n_v(consts):
    return k3.MpcLayout(consts.cfg.n_k, consts.cfg.d).n_v


def sparsity_jac_static(consts: k3.Kite3Constants):
    """CCS pattern (colind, row) of the MPC J_g, derived on the CPU (no device)."""
    return nb.static_sparsity(load_library(), PREFIX, "jac", consts, _n_v(consts))


def sparsity_hess_static(consts: k3.Kite3Constants):
    """Upper-triangular CCS pattern (colind, row) of the MPC nlp_hess_l, derived on the CPU."""
    return nb.static_sparsity(load_library(), PREFIX, "hess", consts, _n_v(consts))


def plant_rk4root_cpu(consts, x0, u, z0, par, ts, n_fe, n_steps=1, max_newton=6, tol=1e-11):
    """The rk4root plant (``MpcEvaluator.plant_rk4root``) on the host, no device: ``consts`` are the
    model constants (``Kite3Constants`` or their vector), x0 [B, 11], u [B, n_steps, 6], z0 [B, 12],
    par [B, 4] numpy arrays.  Returns dict(xf [B, n_steps, 11], zf [B, 12], qf [B, n_steps], res [B])."""
    lib = load_library()
    c = np.ascontiguousarray(getattr(consts, "consts", consts), dtype=np.float64)
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    B = x0.shape[0] if x0.ndim == 2 else 0
    arrs = [x0] + [np.ascontiguousarray(a, dtype=np.float64) for a in (u, z0, par)]
    if B >= 1 and n_steps >= 1:
        for a, shape in zip(arrs, ((B, k3.NX), (B, n_steps, k3.NU), (B, PLANT_NUNK), (B, PLANT_NPAR))):
            if a.shape != shape:
                raise ValueError(f"expected an array of shape {shape}, got {a.shape}")
    out = {"xf": np.zeros((max(B, 0), max(n_steps, 0), k3.NX)), "zf": np.zeros((max(B, 0), PLANT_NUNK)),
           "qf": np.zeros((max(B, 0), max(n_steps, 0))), "res": np.zeros(max(B, 0))}
    rc = lib.awempc_plant_rk4root_cpu(nb._dptr(c), c.size, B, *(nb._dptr(a) for a in arrs), float(ts), int(n_fe),
                                      int(n_steps), int(max_newton), float(tol), *(nb._dptr(a) for a in out.values()))
    if rc != nb.AWE_OK:
        raise nb.AwegpuError(f"awempc error {rc}: {nb.last_error(lib, PREFIX)}")
    return out


def reference_points(lay: k3.MpcLayout, consts: k3.Kite3Constants, diam_t: float):
    """What a reference window needs beside the trajectory's tables: the time offsets of its points
    from the window's start -- x[k] at k ts, the collocation nodes at (k + tau_j) ts (interval-major),
    u[k] at k ts (pmpc.py:413-419, the MPC trial's time grids) -- and its leading entries theta =
    (diam_t, N ts) scaled, phi = xi = 0 (pmpc.py:518-524)."""
    from .collocation import coefficients
    ts, s = consts.cfg.ts, consts.scaling
    tau = coefficients(lay.d, "radau")[0]
    k = np.arange(lay.n_k, dtype=np.float64)
    offs = np.concatenate([np.arange(lay.n_k + 1, dtype=np.float64) * ts,
                           ((k[:, None] + tau[None, 1:]) * ts).reshape(-1), k * ts])
    head = np.zeros(lay.v_intervals)
    head[lay.theta()] = np.array([diam_t, lay.n_k * ts]) / s[2 * k3.NX + k3.NU + k3.NZ:]
    return offs, head


def _reference_args(tables, lay, consts):
    """A table of ``reference.PeriodicTrajectory.tables`` as the library takes it."""
    pieces, degree, brk, coef = [], [], [], []
    for name in REF_GRIDS:
        g = tables["grids"][name]
        b = np.asarray(g["breaks"], dtype=np.float64)
        c = np.asarray(g["coef"], dtype=np.float64)
        if b.ndim != 1 or c.ndim != 3 or c.shape[:2] != (len(b) - 1, REF_CHANNELS[name]):
            raise ValueError(f"grid {name!r}: coef must be [pieces, {REF_CHANNELS[name]}, degree + 1]")
        pieces.append(len(b) - 1)
        degree.append(c.shape[2] - 1)
        brk.append(b)
        coef.append(c.reshape(-1))
    offs, head = reference_points(lay, consts, float(tables["diam_t"]))
    arrs = [np.ascontiguousarray(a) for a in (offs, head, np.array(pieces, dtype=np.int32),
                                              np.array(degree, dtype=np.int32), np.concatenate(brk),
                                              np.concatenate(coef))]
    ptrs = [nb._dptr(arrs[0]), nb._dptr(arrs[1]), nb._iptr(arrs[2]), nb._iptr(arrs[3]), nb._dptr(arrs[4]),
            nb._dptr(arrs[5])]
    return float(tables["period"]), arrs, ptrs


def reference_window_cpu(tables, t0, lay, consts, out=None, ld=None, off=0):
    """``MpcEvaluator.reference_window`` on the host, no device: the windows [B, n_v] of the loops
    starting at times ``t0`` [B] from a table of ``PeriodicTrajectory.tables``; with ``out`` (a
    contiguous float64 array of B rows of length ``ld``) they are written at ``out[b, off:off + n_v]``
    and nothing else of ``out`` is touched."""
    lib = load_library()
    t0 = np.ascontiguousarray(np.atleast_1d(t0), dtype=np.float64)
    B = t0.shape[0]
    if out is None:
        out, ld = np.zeros((B, lay.n_v)), lay.n_v
    ld = out.shape[1] if ld is None else ld
    if out.dtype != np.float64 or not out.flags.c_contiguous or out.size != B * ld:
        raise ValueError("out must be a contiguous float64 array of B rows of length ld")
    period, arrs, ptrs = _reference_args(tables, lay, consts)
    rc = lib.awempc_ref_window_cpu(lay.n_k, lay.d, B, period, *ptrs, nb._dptr(t0), nb._dptr(out), int(ld), int(off))
    if rc != nb.AWE_OK:
        raise nb.AwegpuError(f"awempc error {rc}: {nb.last_error(lib, PREFIX)}")
    return out


class MpcEvaluator(nb.GeneratedPathMixin, nb.NlpEvaluator):
    """HIP evaluator of the 3-DOF tracking-MPC NLP for ``batch`` (V, p) instances.
    ``eval_nlp_device`` runs the dual-number kernel on contiguous grad_f / jac and the generated node
    code on instance-minor ones, which ``alloc_jac`` / ``alloc_grad`` hand out when the generated
    path serves the handle and B > 1; the Hessian tables are built on first use (awempc_hess_init)."""

    PREFIX, LIBNAME = PREFIX, "awempc"
    INSTANCE_MINOR = None
    BATCH1_CONTIGUOUS = True
    HESS_NNZ = "hess_init"
    N_IM_TIMES = 3          # input transposition, node kernels, finalize
    _load = staticmethod(load_library)
    _default_constants = staticmethod(k3.build_constants)

    @staticmethod
    def _layout(consts):
        return k3.MpcLayout(consts.cfg.n_k, consts.cfg.d)

    def plant_rk4root(self, x0, u, z0, par, ts, n_fe, n_steps=1, max_newton=6, tol=1e-11, stream=None):
        """The reference's simulation plant (sim.py:72-78 -> rk4root) for all ``batch`` loops in one
        launch: ``n_steps`` sampling times of length ``ts`` [s], ``n_fe`` RK4 steps each, the control
        u[:, s] held over sampling time s, a Newton rootfinder for (xdot, z) at every stage and at the end
        of every sampling time.  Contiguous float64 CUDA tensors x0 [B, 11], u [B, n_steps, 6] (scaled),
        z0 [B, 12] (rootfinder guess: xdot, lambda), par [B, 4] (theta.diam_t, theta.t_f, phi.gamma,
        u_ref).  Returns (xf [B, n_steps, 11], zf [B, 12] at the last xf, qf [B, n_steps] power integral
        of each sampling time, res [B] largest rootfinder residual)."""
        import torch
        B = self.batch
        for t, shape in ((x0, (B, k3.NX)), (u, (B, max(n_steps, 0), k3.NU)), (z0, (B, PLANT_NUNK)),
                         (par, (B, PLANT_NPAR))):
            if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError(f"expected a contiguous float64 CUDA tensor of shape {shape}")
        f64 = dict(dtype=torch.float64, device=x0.device)
        xf, zf = torch.empty(B, max(n_steps, 0), k3.NX, **f64), torch.empty(B, PLANT_NUNK, **f64)
        qf, res = torch.empty(B, max(n_steps, 0), **f64), torch.empty(B, **f64)
        self._call("plant_rk4root", x0.data_ptr(), u.data_ptr(), z0.data_ptr(), par.data_ptr(), float(ts), int(n_fe),
                   int(n_steps), int(max_newton), float(tol), xf.data_ptr(), zf.data_ptr(), qf.data_ptr(),
                   res.data_ptr(), self._stream(stream))
        return xf, zf, qf, res

    def set_reference(self, tables):
        """Upload a periodic trajectory's tables (``reference.PeriodicTrajectory.tables``) for
        ``reference_window``; a degree or piece count beyond the kernel's staging raises AwegpuError."""
        period, arrs, ptrs = _reference_args(tables, self.layout, self.consts)
        self._call("ref_set", period, *ptrs)

    def reference_window(self, t0, out=None, ld=None, off=0, stream=None):
        """Pmpc's reference windows (pmpc.py:492-550) of all ``batch`` loops in one launch: loop b's
        window starts at ``t0[b]`` (a float64 CUDA tensor [B]; any time, reduced modulo the period).
        Returns [B, n_v]; with ``out`` (a contiguous float64 CUDA tensor of B rows of length ``ld``) the
        windows are written at ``out[b, off:off + n_v]`` -- ``out=P, off=lay.p_ref`` writes the MPC
        parameter in place -- and nothing else of ``out`` is touched."""
        import torch
        B = self.batch
        if t0.dtype != torch.float64 or not t0.is_cuda or not t0.is_contiguous() or tuple(t0.shape) != (B,):
            raise ValueError(f"t0 must be a contiguous float64 CUDA tensor of shape ({B},)")
        if out is None:
            out, ld = torch.empty(B, self.n_v, dtype=torch.float64, device=t0.device), self.n_v
        ld = out.shape[1] if ld is None else ld
        if out.dtype != torch.float64 or not out.is_cuda or not out.is_contiguous() or out.numel() != B * ld:
            raise ValueError("out must be a contiguous float64 CUDA tensor of B rows of length ld")
        self._call("ref_window", t0.data_ptr(), out.data_ptr(), int(ld), int(off), self._stream(stream))
        return out

    def last_ref_ms(self):
        """HIP-event time of the last ``reference_window`` kernel, ms."""
        a, = nb._floats(1)
        self._call("last_ref_ms", ctypes.byref(a))
        return a.value

    def last_plant_ms(self):
        """HIP-event time of the last ``plant_rk4root`` kernel, ms."""
        a, = nb._floats(1)
        self._call("last_plant_ms", ctypes.byref(a))
        return a.value
