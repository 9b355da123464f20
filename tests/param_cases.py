"""Inputs for the parameter-reach tests (test_param_reach.py, test_param_parity_gpu.py): (V, P) pairs
in which every entry of P that a model reads is distinct from its neighbours and far enough from any
other value that a kernel reading the wrong entry, or none, changes an output by much more than the
parity tolerance.  The schedule's own P cannot do this: half of its costs are 0, its 59 weights take
8 values spread over 12 decades, p.ref is the initial guess with V's own diam_t (theta regularisation
and the t_f cost vanish) and geometry.j is symmetric with four zeros.

Every builder returns a ``Case``: V, P and ``dP``, the amount by which the builder moved each entry of P's
weights, cost and theta0 blocks (zero elsewhere, and zero for an entry it left at 0).  The census of
test_param_reach.py changes one entry back by ``dP`` and asks that an output moves by 10 parity
tolerances at least:

* theta0: the entry times its own multiplier ``s``, |s| in [0.02, 0.10] with a random sign; for the
  four filled zeros of geometry.j the whole value;
* weights and costs: ``gap(n)``, the smallest gap two of the block's n entries can have -- the smallest
  error that reading a neighbour's value in place of one's own can make.

All draws come from numpy Generators seeded by (model tag, seed), so no two instances of a batch share
a value or a multiplier."""
from collections import namedtuple

import numpy as np

from awebox_amd import problem as pb

Case = namedtuple("Case", "V P dP")

SIGMA = 0.03                     # noise of V and p.ref: 0.01 leaves seven higher-order stability
#                                  derivatives within 45..900 tolerances (alpha stays too small)
S_MIN, S_MAX = 0.02, 0.10        # |multiplier - 1| of a theta0 entry
LO, HI = 0.5, 2.0                # range of the weights and costs
J_FILL = 0.3                     # the zeros of geometry.j
DEAD_FILL = 1e6                  # dead entry i is overwritten with DEAD_FILL * (i + 1)


def distinct(rng, n, lo=LO, hi=HI):
    """n values in [lo, hi], in random order, any two at least ``gap(n, lo, hi)`` apart: a jittered grid."""
    step = (hi - lo) / n
    return rng.permutation(lo + step * (np.arange(n) + 0.5 + rng.uniform(-0.25, 0.25, n)))


def gap(n, lo=LO, hi=HI):
    return 0.5 * (hi - lo) / n


def multipliers(rng, n):
    """s [n] with |s| in [S_MIN, S_MAX] and a random sign."""
    return rng.choice([-1.0, 1.0], n) * rng.uniform(S_MIN, S_MAX, n)


def theta0_block(theta0, rng):
    """(theta0 perturbed, dP of the block): zeros of geometry.j filled, then every entry times 1 + s."""
    th = theta0.copy()
    o, n = pb.THETA0_OFF["geometry.j"]
    zeros = o + np.flatnonzero(th[o:o + n] == 0.0)
    th[zeros] = J_FILL + 0.02 * (rng.permutation(len(zeros)) - 0.5 * (len(zeros) - 1))
    s = multipliers(rng, th.size)
    d = th * s
    th = th + d
    d[zeros] = th[zeros]
    return th, d


def _ap2_like(lay, nw, V, ref, theta0, rng):
    """P = [ref, weights, cost, theta0] of the AP2 and multi-kite layouts, and its dP."""
    P, dP = np.zeros(lay.n_p), np.zeros(lay.n_p)
    P[lay.p_ref:lay.p_ref + lay.n_v] = ref
    P[lay.p_weights:lay.p_weights + nw] = distinct(rng, nw)
    dP[lay.p_weights:lay.p_weights + nw] = gap(nw)
    P[lay.p_cost:lay.p_cost + pb.NCOST] = distinct(rng, pb.NCOST)
    dP[lay.p_cost:lay.p_cost + pb.NCOST] = gap(pb.NCOST)
    P[lay.p_theta0:], dP[lay.p_theta0:] = theta0_block(theta0, rng)
    return Case(V, P, dP)


def ap2_full_p(consts, lay, v0, seed, sigma=SIGMA):
    """AP2: V is batch member 2 seed and p.ref member 2 seed + 1 (noise ``sigma``), with diam_t moved up
    by 10..30 % in V and down by 10..20 % in p.ref and V's t_f up by 2..5 %, so theta regularisation and
    the t_f cost are active; all 59 weights and 20 costs distinct in [0.5, 2]; theta0 as in the
    module's docstring."""
    from awebox_amd.initial_guess import batch_member
    rng = np.random.default_rng([1, seed])
    V = batch_member(v0, lay, 2 * seed, sigma=sigma)
    ref = batch_member(v0, lay, 2 * seed + 1, sigma=sigma)
    V[lay.theta()[0]] *= 1.0 + rng.uniform(0.1, 0.3)
    ref[lay.theta()[0]] *= 1.0 - rng.uniform(0.1, 0.2)
    V[lay.theta()[1]] *= 1.0 + rng.uniform(0.02, 0.05)
    return _ap2_like(lay, pb.NW, V, ref, consts.theta0, rng)


def _dead_costs_and_theta0(sd_len, lay):
    """P indices of the cost and theta0 entries no model here reads, from names and sd_len: the costs of
    terms a power-cycle objective does not have and P_max, the atmosphere and wind entries of other
    atmosphere and wind models, the two rotation bounds the yaw constraint does not use and the
    stability-derivative slots beyond each table's length."""
    dead = [lay.p_cost + pb.COST_NAMES.index(n) for n in
            ("power_derivative", "nominal_landing", "compromised_battery", "transition", "P_max")]
    for n in ("atmosphere.gamma", "atmosphere.p_ref", "atmosphere.mu_ref", "atmosphere.c_sutherland",
              "wind.log_wind.z0_air"):
        dead.append(lay.p_theta0 + pb.THETA0_OFF[n][0])
    o = lay.p_theta0 + pb.THETA0_OFF["model_bounds.rot_angles"][0]
    dead += [o, o + 1]
    o = lay.p_theta0 + pb.THETA0_OFF["aero.stab_derivs"][0]
    sd_len = np.asarray(sd_len).reshape(-1)
    dead += [o + t * pb.SD_MAXLEN + l for t in range(sd_len.size) for l in range(int(sd_len[t]), pb.SD_MAXLEN)]
    return dead


def ap2_dead_entries(consts, lay):
    """P indices that the AP2 model does not read: _dead_costs_and_theta0 and the weight of t_f, which is
    not regularised."""
    dead = _dead_costs_and_theta0(consts.sd_len, lay) + [lay.p_weights + pb.W_OFF[("theta", "t_f")][0]]
    return np.array(sorted(dead))


def with_dead_overwritten(P, dead):
    """P (one row or a batch) with dead entry i set to DEAD_FILL * (i + 1): large, finite, distinct."""
    P = np.array(P, dtype=np.float64)
    P[..., dead] = DEAD_FILL * (np.arange(len(dead)) + 1.0)
    return P


def entry_name(lay, i, w_names=None):
    """A readable name of P entry i of an AP2-like layout."""
    if i < lay.p_weights:
        return f"p.ref[{i}]"
    if i < lay.p_cost:
        return f"weights[{i - lay.p_weights}]" + (f" {w_names[i - lay.p_weights]}" if w_names else "")
    if i < lay.p_theta0:
        return "cost." + pb.COST_NAMES[i - lay.p_cost]
    t = i - lay.p_theta0
    for name, (o, n) in pb.THETA0_OFF.items():
        if o <= t < o + n:
            if name == "aero.stab_derivs":
                tab, l = divmod(t - o, pb.SD_MAXLEN)
                return f"theta0.aero.{pb.SD_COEFFS[tab // len(pb.SD_INPUTS)]}.{pb.SD_INPUTS[tab % len(pb.SD_INPUTS)]}[{l}]"
            return f"theta0.{name}[{t - o}]"
    raise IndexError(i)


AP2_W_NAMES = [f"{vt}.{n}[{i}]" for vt, ents in pb.VAR_TYPES for n, s in ents for i in range(s)]


# ---- dual kites ---------------------------------------------------------------------------------------
def dual_full_p(mc, lay, V0, seed, sigma=SIGMA):
    """Dual kites (``single_reelout`` with its two t_f, or the plain layout: whatever ``lay`` is): V and
    p.ref two batch members with diam_t moved apart as in ap2_full_p and every t_f of V up by a factor of
    its own (2..5 %), so the period differs from the reference's; l_s and diam_s differ through the noise;
    weights, costs and theta0 as in the module's docstring."""
    from awebox_amd import dual as du
    rng = np.random.default_rng([3, seed])
    V = du.batch_member(V0, lay, 2 * seed, sigma=sigma)
    ref = du.batch_member(V0, lay, 2 * seed + 1, sigma=sigma)
    i_d = lay.theta_index("diam_t")
    V[i_d] *= 1.0 + rng.uniform(0.1, 0.3)
    ref[i_d] *= 1.0 - rng.uniform(0.1, 0.2)
    for i in sorted({lay.tf_index(0), lay.tf_index(lay.n_k - 1)}):
        V[i] *= 1.0 + rng.uniform(0.02, 0.05)
    return _ap2_like(lay, mc.model.nw, V, ref, mc.theta0, rng)


def dual_dead_entries(mc, lay):
    """As ap2_dead_entries for the multi-kite model: the same costs and theta0 entries, the weight of t_f."""
    dead = _dead_costs_and_theta0(mc.sd_len, lay) + [lay.p_weights + mc.model.off[("theta", "t_f")][0]]
    return np.array(sorted(dead))


def dual_w_names(mc):
    return [f"{vt}.{n}[{i}]" for vt, ents in mc.model.groups for n, s in ents for i in range(s)]


# ---- MPC ----------------------------------------------------------------------------------------------
def mpc_full_p(c, lay, i, batch, seed, sigma=SIGMA):
    """The tracking MPC: kite3.batch_instance(i, batch) with x0, ref, u_ref, Q, R and the terminal P all
    drawn: ref is the reference window plus noise of its own (so V - ref is not V's noise alone), u_ref
    in [4, 8], Q, R and P distinct in [0.5, 2] across all three (one jittered grid of 28 values).
    ``dP`` is the grid's smallest gap for Q, R and P and 2 % for u_ref."""
    from awebox_amd import kite3 as k3
    rng = np.random.default_rng([5, seed])
    V, p = k3.batch_instance(c, lay, i, batch, sigma=sigma, seed=99 + 1000 * seed)
    free = np.ones(lay.n_v, dtype=bool)
    free[:lay.v_intervals] = False
    p[lay.p_ref:lay.p_ref + lay.n_v][free] += sigma * rng.standard_normal(int(free.sum()))
    p[lay.p_x0:lay.p_x0 + k3.NX] += sigma * rng.standard_normal(k3.NX)
    p[lay.p_u_ref] = rng.uniform(4.0, 8.0)
    n = lay.n_p - lay.p_Q
    p[lay.p_Q:] = distinct(rng, n)
    dP = np.zeros(lay.n_p)
    dP[lay.p_Q:] = gap(n)
    dP[lay.p_u_ref] = S_MIN * p[lay.p_u_ref]
    return Case(V, p, dP)
