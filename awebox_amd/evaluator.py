"""Python side of the drop-in boundary: ctypes binding of ``libawegpu.so`` (include/awegpu.h).

``Ap2Evaluator`` exposes the NLP oracle surface IPOPT reaches through ``casadi.nlpsol`` in the
reference (awebox/opti/preparation.py:366-400): ``nlp_f``, ``nlp_g``, ``nlp_grad_f`` and
``nlp_jac_g`` with CasADi's argument meaning (x = V, p = P) and output convention (J_g in CCS,
column-major).  It also provides the batched device-pointer path used by the sweep / MPC drivers
and by ``bench.py``.  What it shares with the other two evaluators lives in ``nlp_binding``.

There is no CPU fallback: if the shared library is missing or no HIP device is visible, every
constructor raises ``AwegpuUnavailable``.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import nlp_binding as nb
from . import problem as pb
from .nlp_binding import (AWE_ERR_ARG, AWE_ERR_HIP, AWE_ERR_NODEVICE, AWE_ERR_NONFINITE, AWE_OK,  # noqa: F401
                          FP, IP, VP, AwegpuError, AwegpuUnavailable, H, I, Z, _dptr)

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libawegpu.so")
PREFIX = "awe_"
SIGNATURES = {
    "eval_nlp_im": [H] + [VP] * 6 + [I, VP],           # ldj is an int here, a size_t in the other two
    "eval_nlp_imv": [H, VP, VP, I] + [VP] * 4 + [I, VP],
    "instance_ld": [H, IP],
    "eval_g": [H] + [VP] * 4,
    "eval_f": [H] + [VP] * 4,
    "eval_f_host": [H] + [nb.DP] * 3,
    "eval_g_host": [H] + [nb.DP] * 3,
    "device_count": [],
    "hess_nnz": [H, IP],
    "eval_hess_im": [H] + [VP] * 5 + [Z, VP],
    "set_eval_path": [H, I],
    "get_eval_path": [H, IP],
    "set_hess_path": [H, I],
    "get_hess_path": [H, IP],
    "last_kernel_ms_gen": [H, FP, FP],
    "last_kernel_ms_soa": [H, FP],
}
EXPORTED_SYMBOLS = nb.exported(PREFIX, SIGNATURES)
# the rk4root re-integration, declared in include/awegpu_rk4root.h beside awegpu.h
RK4ROOT_SIGNATURES = {
    "integrate_rk4root": [H, I] + [VP] * 5 + [I, I, I, ctypes.c_double] + [VP] * 5,
    "integrate_rk4root_cpu": [nb.DP, I, I] + [nb.DP] * 5 + [I, I, I, ctypes.c_double] + [nb.DP] * 4,
    "rk4root_par_layout": [IP, IP],
    "last_integrate_ms": [H, FP],
}
RK4ROOT_SYMBOLS = [PREFIX + name for name in RK4ROOT_SIGNATURES]

PATH_COLOUR, PATH_GENERATED, PATH_SOA = 0, 1, 2


def load_library(path: str = _LIB_PATH):
    lib = nb.load(path, PREFIX, SIGNATURES)
    for name, sig in RK4ROOT_SIGNATURES.items():
        fn = getattr(lib, PREFIX + name)
        fn.argtypes, fn.restype = sig, I
    return lib


def _n_v(consts):
    return pb.NlpLayout(consts.cfg.n_k, consts.cfg.d).n_v


def sparsity_jac_static(consts: pb.Ap2Constants):
    """CCS pattern (colind, row) of J_g derived on the CPU -- no device needed."""
    return nb.static_sparsity(load_library(), PREFIX, "jac", consts, _n_v(consts))


def sparsity_hess_static(consts: pb.Ap2Constants):
    """Upper-triangular CCS pattern (colind, row) of nlp_hess_l derived on the CPU."""
    return nb.static_sparsity(load_library(), PREFIX, "hess", consts, _n_v(consts))


RK_NUNK = pb.NX + pb.NZ      # the rootfinder's unknowns y = (xdot, z)


def rk4root_par_layout():
    """Sources of a task's parameter row (awe_rk4root_par_layout, include/awegpu_rk4root.h): entry < 1000 is
    node variable i (57 theta.diam_t, 58 theta.t_f, 59 phi.gamma), entry >= 1000 theta0 entry i - 1000."""
    lib = load_library()
    n = ctypes.c_int()
    lib.awe_rk4root_par_layout(ctypes.byref(n), None)
    src = np.zeros(n.value, dtype=np.int32)
    lib.awe_rk4root_par_layout(ctypes.byref(n), nb._iptr(src))
    return src


def rk4root_par(theta, gamma, theta0):
    """Parameter rows [n, n_par] of n integration tasks from theta [n, 2] (scaled diam_t, t_f), phi.gamma
    [n] and theta0 [n, NTHETA0] (P's tail): numpy arrays or torch tensors, the result of the same kind."""
    src = rk4root_par_layout()
    node = np.concatenate([theta, gamma[:, None]], axis=1) if isinstance(theta, np.ndarray) else None
    if node is None:
        import torch
        node = torch.cat([theta, gamma[:, None]], dim=1)
        cat = lambda a, b: torch.cat([a, b], dim=1)   # noqa: E731
    else:
        cat = lambda a, b: np.concatenate([a, b], axis=1)   # noqa: E731
    n_in = int((src < 1000).sum())
    return cat(node[:, (src[:n_in] - pb.W_TH0).tolist()], theta0[:, (src[n_in:] - 1000).tolist()])


def _rk4root_shapes(n, n_steps):
    return ((n, pb.NX), (n, n_steps, pb.NU), (n, RK_NUNK), (n, len(rk4root_par_layout())), (n,))


def integrate_rk4root_cpu(consts, x0, u, y0, par, ts, n_fe, n_steps=1, max_newton=20, tol=1e-12):
    """``Ap2Evaluator.integrate_rk4root`` on the host, no device: ``consts`` are the model constants
    (``Ap2Constants`` or their vector); numpy arrays x0 [n, 23], u [n, n_steps, 10], y0 [n, 24], par
    [n, n_par] (``rk4root_par``), ts [n].  Returns dict(xf [n, n_steps, 23], yf [n, 24], qf [n, n_steps],
    res [n])."""
    lib = load_library()
    c = np.ascontiguousarray(getattr(consts, "consts", consts), dtype=np.float64)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (x0, u, y0, par, ts)]
    n = arrs[0].shape[0] if arrs[0].ndim == 2 else 0
    if n >= 1 and n_steps >= 1:
        for a, shape in zip(arrs, _rk4root_shapes(n, n_steps)):
            if a.shape != shape:
                raise ValueError(f"expected an array of shape {shape}, got {a.shape}")
    n, m = max(n, 0), max(n_steps, 0)
    out = {"xf": np.zeros((n, m, pb.NX)), "yf": np.zeros((n, RK_NUNK)), "qf": np.zeros((n, m)), "res": np.zeros(n)}
    rc = lib.awe_integrate_rk4root_cpu(nb._dptr(c), c.size, arrs[0].shape[0] if arrs[0].ndim == 2 else 0,
                                       *(nb._dptr(a) for a in arrs), int(n_fe), int(n_steps), int(max_newton),
                                       float(tol), *(nb._dptr(a) for a in out.values()))
    if rc != AWE_OK:
        raise AwegpuError(f"awegpu error {rc}: {nb.last_error(lib, PREFIX)}")
    return out


class Ap2Evaluator(nb.NlpEvaluator):
    """HIP evaluator of the AP2 direct-collocation NLP for ``batch`` (V, P) instances."""

    PREFIX, LIBNAME = PREFIX, "awegpu"
    INSTANCE_MINOR = True
    BATCH1_CONTIGUOUS = True
    has_eval_paths = True
    _load = staticmethod(load_library)
    _default_constants = staticmethod(pb.build_constants)

    def __init__(self, consts: pb.Ap2Constants | None = None, batch: int = 1):
        super().__init__(consts, batch)
        self._hess_pattern()

    @staticmethod
    def _layout(consts):
        return pb.NlpLayout(consts.cfg.n_k, consts.cfg.d)

    def _before_create(self):
        if self._lib.awe_device_count() <= 0:
            raise AwegpuUnavailable("no HIP device visible: the evaluator has no CPU fallback")

    # ---------------------------------------------- device path (torch CUDA tensors) ---
    def _inputs_instance_minor(self, V, P):
        """V and P from ``alloc_inputs``: eval_nlp_device then runs awe_eval_nlp_imv."""
        if self.batch == 1:
            return False
        ld = self.instance_ld
        return (tuple(V.shape) == (self.batch, self.n_v) and V.stride() == (1, ld)
                and tuple(P.shape) == (self.batch, self.n_p) and P.stride() == (1, ld))

    @property
    def instance_ld(self):
        """Leading dimension of the handle's instance-minor buffers (awe_instance_ld)."""
        v = ctypes.c_int()
        self._call("instance_ld", ctypes.byref(v))
        return v.value

    def alloc_inputs(self, device="cuda"):
        """(V, P) value tensors [B, n_v], [B, n_p] stored instance-minor (the transposed views of
        contiguous [n, instance_ld] tensors): eval_nlp_device then runs awe_eval_nlp_imv, which reads
        them in place instead of transposing per-instance inputs (instance-minor path only)."""
        import torch
        ld = self.instance_ld
        return (torch.zeros(self.n_v, ld, dtype=torch.float64, device=device).t()[:self.batch],
                torch.zeros(self.n_p, ld, dtype=torch.float64, device=device).t()[:self.batch])

    def alloc_hess(self, device="cuda", instance_minor=True):
        """A Hessian value tensor [B, nnz_h], instance-minor unless asked otherwise."""
        return super().alloc_hess(device, instance_minor)

    def eval_g_device(self, V, P, g, stream=None):
        self._call("eval_g", V.data_ptr(), P.data_ptr(), g.data_ptr(), self._stream(stream))

    def eval_f_device(self, V, P, f, stream=None):
        self._call("eval_f", V.data_ptr(), P.data_ptr(), f.data_ptr(), self._stream(stream))

    def eval_hess_device_im(self, V, P, sigma, lam_g, H, stream=None):
        """As eval_hess_device with H instance-minor: the transposed view ``x.t()`` of a contiguous
        [nnz_h, ld] tensor, ld >= B (awe_eval_hess_im; ``alloc_hess``)."""
        import torch
        self._check_hess_inputs((V, self.n_v), (P, self.n_p), (sigma, 1), (lam_g, self.n_g))
        if H.dtype != torch.float64 or not H.is_cuda or tuple(H.shape) != (self.batch, self.nnz_h) or \
                H.stride(0) != 1 or H.stride(1) < self.batch:
            raise ValueError("H must be an instance-minor [batch, nnz_h] float64 view (strides (1, ld))")
        self._call("eval_hess_im", V.data_ptr(), P.data_ptr(), sigma.data_ptr(), lam_g.data_ptr(), H.data_ptr(),
                   int(H.stride(1)), self._stream(stream))

    # ---------------------------------------------- rk4root re-integration -------------
    def integrate_rk4root(self, x0, u, y0, par, ts, n_fe, n_steps=1, max_newton=20, tol=1e-12, stream=None):
        """The reference's rk4root (tools/integrator_routines.py:32-96) for n integration tasks in one
        launch, one lane per task (n is free: it is not the evaluator's batch): ``n_steps`` sampling
        times of length ts[t] [s], ``n_fe`` RK4 steps each, the control u[t, s] held over sampling time s,
        a Newton rootfinder for y = (xdot, z) at every stage and at the end of every sampling time.
        Contiguous float64 CUDA tensors x0 [n, 23], u [n, n_steps, 10] (scaled), y0 [n, 24] (the
        rootfinder's guess), par [n, n_par] (``rk4root_par``), ts [n].  Returns (xf [n, n_steps, 23],
        yf [n, 24] at the last xf, qf [n, n_steps] energy of each sampling time [J], res [n] the largest
        rootfinder residual)."""
        import torch
        n = x0.shape[0] if x0.dim() == 2 else 0
        for t, shape in zip((x0, u, y0, par, ts), _rk4root_shapes(n, max(n_steps, 0))):
            if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError(f"expected a contiguous float64 CUDA tensor of shape {shape}")
        f64 = dict(dtype=torch.float64, device=x0.device)
        xf, yf = torch.empty(n, max(n_steps, 0), pb.NX, **f64), torch.empty(n, RK_NUNK, **f64)
        qf, res = torch.empty(n, max(n_steps, 0), **f64), torch.empty(n, **f64)
        self._call("integrate_rk4root", n, x0.data_ptr(), u.data_ptr(), y0.data_ptr(), par.data_ptr(), ts.data_ptr(),
                   int(n_fe), int(n_steps), int(max_newton), float(tol), xf.data_ptr(), yf.data_ptr(), qf.data_ptr(),
                   res.data_ptr(), self._stream(stream))
        return xf, yf, qf, res

    def last_integrate_ms(self):
        """Kernel time of the last ``integrate_rk4root`` (HIP events), ms."""
        a, = nb._floats(1)
        self._call("last_integrate_ms", ctypes.byref(a))
        return a.value

    # ---------------------------------------------- kernel selection -------------------
    HESS_PATHS = {"hyperdual": 0, "generated": 1, "follow": 2}

    @property
    def hess_path(self):
        """'generated' or 'hyperdual': the Hessian kernel the next call runs (include/awegpu.h)."""
        p = ctypes.c_int()
        self._call("get_hess_path", ctypes.byref(p))
        return {0: "hyperdual", 1: "generated"}[p.value]

    @hess_path.setter
    def hess_path(self, name):
        self._call("set_hess_path", self.HESS_PATHS[name])
        self._hess_mode = name

    @property
    def hess_mode(self):
        """The Hessian selection as set: 'follow' (the default: the kernel follows the evaluation
        path, resolved on every call), 'generated' or 'hyperdual'.  ``hess_path`` returns what the
        next call resolves to.  A solver that reads ``hess_instance_minor`` once to pick the H layout
        (ipm.DeviceNlp.h_im) only picks a layout: the C side dispatches the kernel on every call and
        both entry points (awe_eval_hess / awe_eval_hess_im) handle either kernel."""
        return getattr(self, "_hess_mode", "follow")

    @property
    def hess_instance_minor(self):
        """The generated Hessian kernel writes H instance-minor (eval_hess_device_im)."""
        return self.hess_path == "generated"

    # evaluation path of eval_nlp (include/awegpu.h): "soa" (the default: one lane per instance,
    # the build-time generated sparse-Jacobian code storing straight into J_g), "generated" (one
    # thread per collocation node, tangents gathered by a second kernel) or "colour" (compressed
    # forward mode)
    PATHS = {"colour": PATH_COLOUR, "generated": PATH_GENERATED, "soa": PATH_SOA}

    @property
    def path(self):
        p = ctypes.c_int()
        self._call("get_eval_path", ctypes.byref(p))
        return {v: k for k, v in self.PATHS.items()}[p.value]

    @path.setter
    def path(self, name):
        self._call("set_eval_path", self.PATHS[name])

    # ---------------------------------------------- timers -----------------------------
    def last_kernel_ms_soa(self):
        """HIP-event times of the last instance-minor call (ms): input transpose (0 with
        instance-minor inputs); the node launch (shooting and Radau tiles, the Radau workgroups'
        interval pass); the finalize kernel; 0 (once the finalize kernel's slot: there is no
        separate interval kernel); output transpose (0 with instance-minor outputs)."""
        ms = (ctypes.c_float * 5)()
        self._call("last_kernel_ms_soa", ms)
        return [float(x) for x in ms]

    def last_kernel_ms_gen(self):
        """(node kernel ms, assembly kernel ms) of the last eval_nlp on the generated path."""
        a, b = nb._floats(2)
        self._call("last_kernel_ms_gen", ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    # ---------------------------------------------- value-only kernels (nlp_f / nlp_g) -
    def eval_f(self, V, P):
        """Host arrays in: f [B] from the value-only kernel (no derivatives)."""
        f = np.zeros(self.batch)
        V, P = self._host(V, self.n_v), self._host(P, self.n_p)
        self._call("eval_f_host", _dptr(V), _dptr(P), _dptr(f))
        return f

    def eval_g(self, V, P):
        """Host arrays in: g [B, n_g] from the value-only kernel (no derivatives)."""
        g = np.zeros((self.batch, self.n_g))
        V, P = self._host(V, self.n_v), self._host(P, self.n_p)
        self._call("eval_g_host", _dptr(V), _dptr(P), _dptr(g))
        return g
