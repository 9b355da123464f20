"""What the ctypes bindings of the three model libraries share (include/awegpu.h, awedual.h, awempc.h).

The libraries export one NLP oracle surface under three prefixes (``awe_``, ``adl_``, ``awempc_``):
``load`` declares its entry points from one signature table, ``static_sparsity`` serves the
``*_sparsity_*_static`` queries, and ``NlpEvaluator`` is the handle-owning base class of
``Ap2Evaluator``, ``DualEvaluator`` and ``MpcEvaluator``, which state only what differs.

There is no CPU fallback: a missing library or device raises ``AwegpuUnavailable``.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

AWE_OK, AWE_ERR_ARG, AWE_ERR_HIP, AWE_ERR_NONFINITE, AWE_ERR_NODEVICE = 0, 1, 2, 3, 4


class AwegpuUnavailable(RuntimeError):
    """The HIP evaluator cannot run here (library not built or no MI355X visible)."""


class AwegpuError(RuntimeError):
    pass


I, Z, VP, H = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p
DP, IP, FP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)
_STATIC = [I, I, DP, I, IP, IP, IP]       # n_k, d, consts, n_consts, nnz, colind, row

# entry-point suffix -> argtypes (restype int), or (argtypes, restype); the model modules add theirs
COMMON_SIGNATURES = {
    "create": [I, I, DP, I, I, ctypes.POINTER(H)],
    "destroy": [H],
    "last_error": ([], ctypes.c_char_p),
    "sizes": [H, IP, IP, IP, IP],
    "sparsity_jac": [H, IP, IP],
    "sparsity_jac_static": _STATIC,
    "eval_nlp": [H] + [VP] * 7,
    "eval_nlp_host": [H] + [DP] * 6,
    "eval_nlp_im": [H] + [VP] * 6 + [Z, VP],
    "last_kernel_ms": [H, FP, FP],
    "sparsity_hess": [H, IP, IP],
    "sparsity_hess_static": _STATIC,
    "eval_hess": [H] + [VP] * 6,
    "eval_hess_host": [H] + [DP] * 5,
    "last_hess_ms": [H, FP],
}

_LIBS: dict = {}


def exported(prefix: str, extra: dict) -> list:
    """The symbols a library exports: the common entry points and the model's own."""
    return [prefix + name for name in {**COMMON_SIGNATURES, **extra}]


def load(path: str, prefix: str, extra: dict):
    """The model library of ``prefix`` with every entry point's argtypes / restype declared.  The
    first one loaded serves the process: a tool that loads a variant build first gets it everywhere."""
    if prefix not in _LIBS:
        if not os.path.exists(path):
            raise AwegpuUnavailable(f"{path} not built; run `python -m awebox_amd.build`")
        lib = ctypes.CDLL(path)
        for name, sig in {**COMMON_SIGNATURES, **extra}.items():
            fn = getattr(lib, prefix + name)
            fn.argtypes, fn.restype = sig if isinstance(sig, tuple) else (sig, I)
        _LIBS[prefix] = lib
    return _LIBS[prefix]


def _dptr(a: np.ndarray):
    return a.ctypes.data_as(DP)


def _iptr(a: np.ndarray):
    return a.ctypes.data_as(IP)


def last_error(lib, prefix: str) -> str:
    return getattr(lib, prefix + "last_error")().decode()


def _consts_args(consts):
    c = np.ascontiguousarray(consts.consts, dtype=np.float64)
    return c, (consts.cfg.n_k, consts.cfg.d, _dptr(c), c.size)


def static_sparsity(lib, prefix: str, which: str, consts, n_v: int):
    """CCS pattern (colind, row) of J_g (``which`` = "jac") or of the upper triangle of nlp_hess_l
    ("hess"), derived on the CPU -- no device needed."""
    fn = getattr(lib, f"{prefix}sparsity_{which}_static")
    c, args = _consts_args(consts)
    nnz = ctypes.c_int()
    if fn(*args, ctypes.byref(nnz), None, None) != AWE_OK:
        raise AwegpuError(last_error(lib, prefix))
    colind = np.zeros(n_v + 1, dtype=np.int32)
    row = np.zeros(nnz.value, dtype=np.int32)
    if fn(*args, ctypes.byref(nnz), _iptr(colind), _iptr(row)) != AWE_OK:
        raise AwegpuError(last_error(lib, prefix))
    return colind, row


def _floats(n):
    return [ctypes.c_float() for _ in range(n)]


def solver_tensors(ev, B, n_v, device, hess=True):
    """(grad f [B, n_v], J_g [B, nnz], H [B, nnz_h] or None, whether H is instance-minor) for a solver
    that drives ``ev`` through the device path, in the evaluator's own layouts.  The solvers accept
    any object with the minimal device surface (sizes, ``sparsity_*``, ``eval_*_device``: the CPU
    and oracle adapters of the tests); the optional members are defaulted here, in one place: no
    ``alloc_*`` means per-instance tensors, no ``hess_instance_minor`` means a per-instance H."""
    import torch

    def alloc(what, n, **kw):
        fn = getattr(ev, "alloc_" + what, None)
        return fn(device, **kw) if fn else torch.zeros(B, n, dtype=torch.float64, device=device)

    h_im = bool(getattr(ev, "hess_instance_minor", False))
    H = alloc("hess", ev.nnz_h, instance_minor=h_im) if hess else None
    return alloc("grad", n_v), alloc("jac", ev.nnz), H, h_im


_BATCH_SHAPE = "device tensors must be contiguous float64 CUDA tensors of the batch shape"
_ONE_INSTANCE = "the oracle-named entry points evaluate one instance (batch=1)"


class NlpEvaluator:
    """HIP evaluator of one NLP for ``batch`` (V, P) instances: the oracle surface IPOPT reaches
    through ``casadi.nlpsol`` in the reference (``nlp_f``, ``nlp_g``, ``nlp_grad_f``, ``nlp_jac_g``,
    ``nlp_hess_l`` with x = V, p = P and J_g in CCS), the batched host path (numpy) and the batched
    device path (torch CUDA tensors).  A subclass names its library and layout:

    * ``PREFIX`` / ``LIBNAME``: symbol prefix and the name in error messages;
    * ``_load()``: the library; ``_default_constants()`` and ``_layout(consts)``;
    * ``INSTANCE_MINOR``: layout of ``alloc_jac`` / ``alloc_grad`` when not asked for one -- True,
      False, or None: instance-minor iff ``batch > 1 and generated_available``;
    * ``BATCH1_CONTIGUOUS``: a single instance always takes the contiguous entry point;
    * ``HESS_NNZ``: the entry point that returns nnz_h (and builds the Hessian tables if need be).
    """

    PREFIX = LIBNAME = None
    INSTANCE_MINOR = False
    BATCH1_CONTIGUOUS = False
    HESS_NNZ = "hess_nnz"
    has_eval_paths = False           # whether ``path`` / ``hess_path`` select among kernels (AP2)
    hess_instance_minor = False      # whether the solver should hold H instance-minor (alloc_hess)

    def __init__(self, consts=None, batch: int = 1):
        self._hess = None
        self.consts = consts or self._default_constants()
        self.layout = self._layout(self.consts)
        self.batch = int(batch)
        self._lib = self._load()
        self._before_create()
        c, args = _consts_args(self.consts)
        handle = ctypes.c_void_p()
        self._check(self._fn("create")(*args, self.batch, ctypes.byref(handle)))
        self._h = handle
        sizes = [ctypes.c_int() for _ in range(4)]
        self._call("sizes", *(ctypes.byref(x) for x in sizes))
        self.n_v, self.n_g, self.n_p, self.nnz = (x.value for x in sizes)
        assert (self.n_v, self.n_g, self.n_p) == (self.layout.n_v, self.layout.n_g, self.layout.n_p)
        self._colind = np.zeros(self.n_v + 1, dtype=np.int32)
        self._row = np.zeros(self.nnz, dtype=np.int32)
        self._call("sparsity_jac", _iptr(self._colind), _iptr(self._row))

    def _before_create(self):
        pass

    # ---------------------------------------------- handle and errors ------------------
    def _fn(self, name):
        return getattr(self._lib, self.PREFIX + name)

    def _check(self, rc):
        if rc != AWE_OK:
            msg = last_error(self._lib, self.PREFIX)
            if rc == AWE_ERR_NODEVICE:
                raise AwegpuUnavailable(msg)
            raise AwegpuError(f"{self.LIBNAME} error {rc}: {msg}")

    def _call(self, name, *args):
        """An entry point on this handle; a closed evaluator passes NULL, which the library refuses."""
        self._check(self._fn(name)(getattr(self, "_h", None), *args))

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------- patterns ---------------------------
    def sparsity_jac(self):
        """CCS pattern of J_g: (colind[n_v+1], row[nnz]) -- nlp_jac_g's output sparsity."""
        return self._colind.copy(), self._row.copy()

    def _hess_pattern(self):
        """(colind, row) of the Hessian's upper triangle, queried on first use."""
        if self._hess is None:
            n = ctypes.c_int()
            self._call(self.HESS_NNZ, ctypes.byref(n))
            colind = np.zeros(self.n_v + 1, dtype=np.int32)
            row = np.zeros(n.value, dtype=np.int32)
            self._call("sparsity_hess", _iptr(colind), _iptr(row))
            self._hess = (colind, row)
        return self._hess

    @property
    def nnz_h(self):
        return len(self._hess_pattern()[1])

    def sparsity_hess(self):
        """Upper-triangular CCS pattern of nlp_hess_l: (colind[n_v+1], row[nnz_h])."""
        colind, row = self._hess_pattern()
        return colind.copy(), row.copy()

    def jac_csc(self, values):
        import scipy.sparse as sp
        return sp.csc_matrix((np.asarray(values), self._row, self._colind), shape=(self.n_g, self.n_v))

    def hess_csc(self, values, full=True):
        """scipy matrix from upper-triangular values; full=True adds the strict lower triangle."""
        import scipy.sparse as sp
        colind, row = self._hess_pattern()
        U = sp.csc_matrix((np.asarray(values), row, colind), shape=(self.n_v, self.n_v))
        return (U + sp.triu(U, 1).T).tocsc() if full else U

    # ---------------------------------------------- device path (torch CUDA tensors) ---
    @staticmethod
    def _stream(stream):
        import torch
        return ctypes.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)

    def _inputs_instance_minor(self, V, P):
        return False

    def eval_nlp_device(self, V, P, f, g, grad_f, jac, stream=None):
        """f, g, grad f, J_g for all instances; float64 CUDA tensors V [B, n_v], P [B, n_p], f [B],
        g [B, n_g] (contiguous) and grad_f [B, n_v], jac [B, nnz]: both contiguous (``*_eval_nlp``),
        or both instance-minor views ``x_t.t()`` of contiguous [n, ld] tensors with one ld >= B
        (``*_eval_nlp_im``, the layout the batched solver reads; ``alloc_grad`` / ``alloc_jac``)."""
        import torch
        vin_im = self._inputs_instance_minor(V, P)
        for t, n in ((V, self.n_v), (P, self.n_p), (f, 1), (g, self.n_g)):
            if t.dtype != torch.float64 or not t.is_cuda or t.numel() != self.batch * n or \
                    not (t.is_contiguous() or (vin_im and (t is V or t is P))):
                raise ValueError(_BATCH_SHAPE + (" (V and P may be instance-minor views from alloc_inputs)"
                                                 if self.has_eval_paths else ""))
        for t, n, name in ((jac, self.nnz, "jac"), (grad_f, self.n_v, "grad_f")):
            if t.dtype != torch.float64 or not t.is_cuda or tuple(t.shape) != (self.batch, n):
                raise ValueError(f"{name} must be a float64 CUDA tensor of shape [batch, {n}]")
        im = lambda t: t.stride(0) == 1 and t.stride(1) >= self.batch   # noqa: E731
        both_im = im(jac) and im(grad_f) and jac.stride(1) == grad_f.stride(1)
        outs = (f.data_ptr(), g.data_ptr(), grad_f.data_ptr(), jac.data_ptr())
        if vin_im:
            if not both_im:
                raise ValueError("instance-minor V and P need instance-minor jac and grad_f")
            self._call("eval_nlp_imv", V.data_ptr(), P.data_ptr(), int(V.stride(1)), *outs, int(jac.stride(1)),
                       self._stream(stream))
        elif (self.BATCH1_CONTIGUOUS and self.batch == 1) or (jac.is_contiguous() and grad_f.is_contiguous()):
            self._call("eval_nlp", V.data_ptr(), P.data_ptr(), *outs, self._stream(stream))
        elif both_im:
            self._call("eval_nlp_im", V.data_ptr(), P.data_ptr(), *outs, int(jac.stride(1)), self._stream(stream))
        else:
            raise ValueError("jac and grad_f must both be contiguous or both instance-minor views "
                             "(strides (1, ld), one ld)")

    def _check_hess_inputs(self, *pairs):
        import torch
        for t, n in pairs:
            if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.numel() != self.batch * n:
                raise ValueError(_BATCH_SHAPE)

    def eval_hess_device(self, V, P, sigma, lam_g, H, stream=None):
        """Upper-triangular CCS values of the Hessian of sigma f + lam_g^T g for all instances:
        contiguous float64 CUDA tensors V [B, n_v], P [B, n_p], sigma [B], lam_g [B, n_g], H [B, nnz_h]."""
        self._check_hess_inputs((V, self.n_v), (P, self.n_p), (sigma, 1), (lam_g, self.n_g), (H, self.nnz_h))
        self._call("eval_hess", V.data_ptr(), P.data_ptr(), sigma.data_ptr(), lam_g.data_ptr(), H.data_ptr(),
                   self._stream(stream))

    def _alloc(self, n, device, instance_minor):
        import torch
        if instance_minor is None:
            instance_minor = self.INSTANCE_MINOR
        if instance_minor is None:
            instance_minor = self.batch > 1 and self.generated_available
        if instance_minor:
            return torch.zeros(n, self.batch, dtype=torch.float64, device=device).t()
        return torch.zeros(self.batch, n, dtype=torch.float64, device=device)

    def alloc_jac(self, device="cuda", instance_minor=None):
        """A J_g value tensor [B, nnz]: instance-minor (the transposed view of [nnz, B], which the
        instance-minor kernels write with coalesced stores) or per instance; None: the class's own
        choice (``INSTANCE_MINOR``)."""
        return self._alloc(self.nnz, device, instance_minor)

    def alloc_grad(self, device="cuda", instance_minor=None):
        """A grad f tensor [B, n_v] in the layout of ``alloc_jac``."""
        return self._alloc(self.n_v, device, instance_minor)

    def alloc_hess(self, device="cuda", instance_minor=False):
        """A Hessian value tensor [B, nnz_h], per instance unless asked otherwise."""
        return self._alloc(self.nnz_h, device, bool(instance_minor))

    def last_kernel_ms(self):
        a, b = _floats(2)
        self._call("last_kernel_ms", ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    def last_hess_ms(self):
        a, = _floats(1)
        self._call("last_hess_ms", ctypes.byref(a))
        return a.value

    # ---------------------------------------------- host path (numpy) ------------------
    def _host(self, a, n):
        return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(self.batch, n))

    def eval_nlp(self, V, P):
        """Host arrays in, host arrays out: dict(f [B], g [B, n_g], grad_f [B, n_v], jac [B, nnz])."""
        V, P = self._host(V, self.n_v), self._host(P, self.n_p)
        out = {"f": np.zeros(self.batch), "g": np.zeros((self.batch, self.n_g)),
               "grad_f": np.zeros((self.batch, self.n_v)), "jac": np.zeros((self.batch, self.nnz))}
        self._call("eval_nlp_host", _dptr(V), _dptr(P), *(_dptr(a) for a in out.values()))
        return out

    def eval_hess(self, V, P, sigma, lam_g):
        """Host arrays in, host array out: H [B, nnz_h] (upper triangle, CCS)."""
        H = np.zeros((self.batch, self.nnz_h))
        V, P, lam = self._host(V, self.n_v), self._host(P, self.n_p), self._host(lam_g, self.n_g)
        sig = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (self.batch,)))
        self._call("eval_hess_host", _dptr(V), _dptr(P), _dptr(sig), _dptr(lam), _dptr(H))
        return H

    def eval_f(self, V, P):
        """Host arrays in: f [B] (from the derivative kernel unless the model has a value-only one)."""
        return self.eval_nlp(V, P)["f"]

    def eval_g(self, V, P):
        """Host arrays in: g [B, n_g] (from the derivative kernel unless the model has a value-only one)."""
        return self.eval_nlp(V, P)["g"]

    # ---- CasADi nlpsol oracle names (one instance) ------------------------------------
    def _single(self, fn, *arrays):
        if self.batch != 1:
            raise ValueError(_ONE_INSTANCE)
        return fn(*(np.asarray(a).reshape(1, -1) for a in arrays))

    def nlp_f(self, x, p):
        return float(self._single(self.eval_f, x, p)[0])

    def nlp_g(self, x, p):
        return self._single(self.eval_g, x, p)[0]

    def nlp_grad_f(self, x, p):
        out = self._single(self.eval_nlp, x, p)
        return float(out["f"][0]), out["grad_f"][0]

    def nlp_jac_g(self, x, p):
        out = self._single(self.eval_nlp, x, p)
        return out["g"][0], self.jac_csc(out["jac"][0])

    def nlp_hess_l(self, x, p, lam_f, lam_g):
        """CasADi nlp_hess_l: Hessian of lam_f f + lam_g^T g (upper triangle, CCS values)."""
        return self._single(lambda x, p, lam: self.eval_hess(x, p, lam_f, lam), x, p, lam_g)[0]


class GeneratedPathMixin:
    """The dual-kite and MPC libraries: a generated instance-minor path beside the main kernel."""

    N_IM_TIMES = 0

    @property
    def generated_available(self) -> bool:
        """Whether the generated instance-minor path (``*_eval_nlp_im``) serves these constants."""
        ok = ctypes.c_int()
        self._call("gen_status", ctypes.byref(ok))
        return bool(ok.value)

    def last_kernel_ms_im(self):
        """HIP-event times of the stages of the last instance-minor evaluation, ms."""
        v = _floats(self.N_IM_TIMES)
        self._call("last_kernel_ms_im", *(ctypes.byref(x) for x in v))
        return tuple(x.value for x in v)
