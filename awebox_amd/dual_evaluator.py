"""ctypes binding of ``libawedual.so`` (include/awedual.h): the multi-kite NLP oracle surface.

``DualEvaluator`` serves ``nlp_f`` / ``nlp_g`` / ``nlp_grad_f`` / ``nlp_jac_g`` / ``nlp_hess_l`` for the dual-kite
power-cycle NLP (config 3) with CasADi's argument meaning (x = V, p = P) and J_g in CCS
(awebox/opti/preparation.py:366-400), plus the batched device-pointer path used by the sweep
driver and ``bench.py`` (``nlp_binding.NlpEvaluator``).  No CPU fallback: a missing library or
device raises ``AwegpuUnavailable``.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import dual as du
from . import nlp_binding as nb
from .nlp_binding import AWE_OK, DP, FP, IP, AwegpuError, H, I, _dptr

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libawedual.so")
PREFIX = "adl_"
SIGNATURES = {
    "colour_counts": [I, I, DP, I, IP, IP, IP, IP],
    "node_eval_host": [DP, DP, DP, I, DP, DP],
    "hess_nnz": [H, IP],
    "gen_status": [H, IP],
    "last_kernel_ms_im": [H] + [FP] * 4,
}
EXPORTED_SYMBOLS = nb.exported(PREFIX, SIGNATURES)


def load_library(path: str = _LIB_PATH):
    return nb.load(path, PREFIX, SIGNATURES)


def sparsity_jac_static(consts: du.MultiConstants):
    """CCS pattern (colind, row) of J_g derived on the CPU -- no device needed."""
    return nb.static_sparsity(load_library(), PREFIX, "jac", consts, du.layout_for(consts).n_v)


def sparsity_hess_static(consts: du.MultiConstants):
    """Upper-triangular CCS pattern (colind, row) of nlp_hess_l derived on the CPU."""
    return nb.static_sparsity(load_library(), PREFIX, "hess", consts, du.layout_for(consts).n_v)


def colour_counts(consts: du.MultiConstants):
    """(colours at the shooting node, at a Radau node, tangent entries of each) -- CPU only."""
    lib = load_library()
    c = np.ascontiguousarray(consts.consts, dtype=np.float64)
    out = [ctypes.c_int() for _ in range(4)]
    if lib.adl_colour_counts(consts.cfg.n_k, consts.cfg.d, _dptr(c), c.size, *[ctypes.byref(o) for o in out]) != AWE_OK:
        raise AwegpuError(nb.last_error(lib, PREFIX))
    return tuple(o.value for o in out)


def node_eval_host(w: np.ndarray, theta0: np.ndarray, consts: du.MultiConstants):
    """Diagnostics (CPU): values [75] and Jacobian [75, 127] of one node of the HIP model's
    source, evaluated on the host in dual arithmetic (the kernel's model code, not the oracle)."""
    lib = load_library()
    w = np.ascontiguousarray(w, dtype=np.float64)
    th = np.ascontiguousarray(theta0, dtype=np.float64)
    c = np.ascontiguousarray(consts.consts, dtype=np.float64)
    val = np.zeros(75)
    jac = np.zeros((75, 127))
    if lib.adl_node_eval_host(_dptr(w), _dptr(th), _dptr(c), c.size, _dptr(val), _dptr(jac)) != AWE_OK:
        raise AwegpuError(nb.last_error(lib, PREFIX))
    return val, jac


class DualEvaluator(nb.GeneratedPathMixin, nb.NlpEvaluator):
    """HIP evaluator of the dual-kite direct-collocation NLP for ``batch`` (V, P) instances.
    ``eval_nlp_device`` runs the colour kernel on contiguous grad_f / jac and the generated node code
    on instance-minor ones; the Hessian is exact (dual_hess_kernel)."""

    PREFIX, LIBNAME = PREFIX, "awedual"
    N_IM_TIMES = 4          # input transposition, node kernel, interval kernel, finalize
    _load = staticmethod(load_library)
    _default_constants = staticmethod(du.build_constants)
    _layout = staticmethod(du.layout_for)
