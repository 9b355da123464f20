"""Python side of the tracking-MPC boundary: ctypes binding of ``libawempc.so`` (include/awempc.h).

``MpcEvaluator`` exposes the NLP oracle surface the MPC's IPOPT solver reaches through
``ct.nlpsol('solver', 'ipopt', {'x': V, 'p': p, 'f': f, 'g': g})`` in ``awebox/pmpc.py:193-217``
(``nlp_f`` / ``nlp_g`` / ``nlp_grad_f`` / ``nlp_jac_g``, with x = V and p = the MPC parameter struct
``[x0, ref, u_ref, Q, R, P]``), plus the batched device path used for many MPC instances at once
(``nlp_binding.NlpEvaluator``).

There is no CPU fallback: a missing library or device raises ``AwegpuUnavailable``.
"""
from __future__ import annotations

import os

from . import kite3 as k3
from . import nlp_binding as nb
from .nlp_binding import FP, IP, H

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libawempc.so")
PREFIX = "awempc_"
SIGNATURES = {
    "hess_init": [H, IP],
    "gen_status": [H, IP],
    "last_kernel_ms_im": [H] + [FP] * 3,
}
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
