"""The interval/separator partition (awebox_amd/kkt_partition.py) that ipm.StructuredKKT and
rti.BatchedRti build their index tables from: a hand-sized pattern with every edge the tables can
get wrong, rebuilt to the dense matrix entry for entry; the owner rule against the layouts' own
index maps; the sub-block picker against the dictionary loop it replaced."""
import numpy as np
import pytest

from awebox_amd import dual as du
from awebox_amd import kite3 as k3
from awebox_amd import problem as pb
from awebox_amd.kkt_partition import IntervalPartition, block_entries, column_owner, group_positions, row_owner

# 12 unknowns, interleaved: interiors of sizes 3 / 2 / 3 (interval 1's block is padded) and four
# separators: A (1, interval 0 only), B (4, shared by intervals 0 and 1), a global G (9, both) and C
# (11, coupled to separators only).  Interval 2 couples to no separator.
OWNER = np.array([0, -1, 1, 0, -1, 2, 1, 0, 2, -1, 2, -1])
A, B, G, C = 1, 4, 9, 11
UPPER = [(0, 3), (3, 7), (2, 6), (5, 8), (8, 10), (5, 10),          # inside the interiors
         (0, A), (3, B), (7, G), (2, B), (6, B), (6, G),            # interior - separator
         (A, B), (B, G), (C, G)]                                    # separator - separator


def _pattern(extra=()):
    """COO of the symmetric pattern, both orientations and the diagonal, in a shuffled value order."""
    up = UPPER + list(extra)
    P = np.array([p for p, q in up] + [q for p, q in up] + list(range(len(OWNER))))
    Q = np.array([q for p, q in up] + [p for p, q in up] + list(range(len(OWNER))))
    order = np.random.default_rng(3).permutation(len(P))
    return P[order], Q[order]


@pytest.fixture(scope="module")
def case():
    P, Q = _pattern()
    M = np.random.default_rng(4).standard_normal((len(OWNER),) * 2)
    vals = (M + M.T)[P, Q]                       # symmetric: the mirrored entries carry one value
    return P, Q, vals, IntervalPartition(OWNER, P, Q, 3)


def test_sizes_and_floor(case):
    _, _, _, part = case
    assert (part.nI, part.nS, part.L, part.n_k) == (3, 4, 3, 3)
    assert part.counts.tolist() == [3, 2, 3]
    assert part.sep.tolist() == part.sep_p.tolist() == [A, B, G, C]
    assert part.lsep_arr.tolist() == [[0, 1, 2], [1, 2, 4], [4, 4, 4]]     # padding: nS
    # nothing coupled anywhere: L rests on its floor
    lone = IntervalPartition(OWNER, np.arange(12), np.arange(12), 3)
    assert lone.L == 1 and (lone.lsep_arr == lone.nS).all() and len(lone.is_) == 0


def test_every_entry_is_in_exactly_one_class(case):
    P, Q, _, part = case
    cls = np.concatenate([part.ii, part.is_, part.ss])
    assert len(np.unique(cls)) == len(cls)
    # what is left are the mirrors K_SI of the K_IS entries, which neither solve stores
    rest = np.setdiff1d(np.arange(len(P)), cls)
    assert ((OWNER[P[rest]] < 0) & (OWNER[Q[rest]] >= 0)).all()
    assert sorted(zip(Q[rest], P[rest])) == sorted(zip(P[part.is_], Q[part.is_]))
    for sel in (part.ii, part.is_, part.ss):
        assert (np.diff(sel) > 0).all()


def test_loc_is_a_bijection_in_ascending_order(case):
    _, _, _, part = case
    for k in range(3):
        mine = np.where(OWNER == k)[0]
        assert part.loc[mine].tolist() == list(range(part.counts[k]))
    assert (part.loc[OWNER < 0] == -1).all() and (part.sep_id[OWNER >= 0] == -1).all()
    assert part.sep_id[part.sep].tolist() == list(range(part.nS))
    assert part.int_p.tolist() == np.where(OWNER >= 0)[0].tolist()
    assert (part.int_flat == OWNER[part.int_p] * part.nI + part.loc[part.int_p]).all()


def test_group_positions():
    pos, counts = group_positions(np.array([2, 0, 2, 1, 0]), 4)
    assert pos.tolist() == [0, 0, 1, 0, 1] and counts.tolist() == [2, 1, 2, 0]


def test_lpos_inverts_lsep(case):
    _, _, _, part = case
    hit = np.zeros_like(part.lpos, dtype=bool)
    for k in range(3):
        for i, s in enumerate(part.lsep_arr[k]):
            if s < part.nS:
                assert part.lpos[k, s] == i
                hit[k, s] = True
    assert (part.lpos[~hit] == -1).all()


def test_schur_pairs(case):
    _, _, _, part = case
    L = part.L
    assert part.r_idx.shape == part.c_idx.shape == (3, L, L)
    assert (part.r_idx == part.lsep_arr[:, :, None]).all() and (part.c_idx == part.lsep_arr[:, None, :]).all()
    # the shared separator B: intervals 0 and 1 both add to S[B, B]
    b = part.sep_id[B]
    both = (part.r_idx == b) & (part.c_idx == b)
    assert both.reshape(3, -1).sum(1).tolist() == [1, 1, 0]


def test_blocks_rebuild_the_dense_matrix(case):
    P, Q, vals, part = case
    N, n_k, nI, nS, L = len(OWNER), 3, part.nI, part.nS, part.L
    K = np.zeros((N, N))
    K[P, Q] = vals
    # assemble as the solves do: the blocks of one instance, ones on the padding diagonal
    KII = np.zeros(n_k * nI * nI)
    KII[part.dst_ii] = vals[part.ii]
    assert len(np.unique(part.dst_ii)) == len(part.dst_ii)
    assert part.pad.tolist() == [1 * nI * nI + 2 * nI + 2] and (KII[part.pad] == 0.0).all()
    KII[part.pad] = 1.0
    KIS = np.zeros(n_k * nI * L)
    KIS[part.dst_is] = vals[part.is_]
    assert len(np.unique(part.dst_is)) == len(part.dst_is)
    KII, KIS = KII.reshape(n_k, nI, nI), KIS.reshape(n_k, nI, L)
    R = np.zeros((N, N))
    for k in range(n_k):
        mine = part.int_p[OWNER[part.int_p] == k]                   # by position: loc ascends
        c = len(mine)
        R[np.ix_(mine, mine)] = KII[k, :c, :c]                      # the padding ones stay behind
        assert (KII[k, c:, :c] == 0.0).all() and (KII[k, :c, c:] == 0.0).all()
        real = part.lsep_arr[k] < nS
        cols = part.sep[part.lsep_arr[k, real]]
        R[np.ix_(mine, cols)] = KIS[k][:c][:, real]
        R[np.ix_(cols, mine)] = KIS[k][:c][:, real].T                # K_SI: the mirror, not stored
        assert (KIS[k][:, ~real] == 0.0).all() and (KIS[k, c:] == 0.0).all()
    assert (P[part.ss] == part.sep[part.ss_r]).all() and (Q[part.ss] == part.sep[part.ss_c]).all()
    R[P[part.ss], Q[part.ss]] = vals[part.ss]
    assert np.array_equal(R, K)


def test_coupled_interiors_are_refused():
    P, Q = _pattern(extra=[(0, 2)])                                 # interval 0 with interval 1
    with pytest.raises(ValueError, match="couples the interiors"):
        IntervalPartition(OWNER, P, Q, 3)


# ------------------------------------------------------------------------------- owner rule
def _dual_layout():
    return du.layout_for(du.build_constants(du.MultiConfig(n_k=2, d=1)))


def _g_coll(lay, k, j):
    if hasattr(lay, "g_coll"):
        return lay.g_coll(k, j)
    n_eq = len(lay.g_shooting(k))                                   # the dual layout names no g_coll
    b = lay.g_path(k)[-1] + 1 + j * n_eq
    return np.arange(b, b + n_eq)


def _g_continuity(lay, k):
    if hasattr(lay, "g_continuity"):
        return lay.g_continuity(k)
    b = _g_coll(lay, k, lay.d - 1)[-1] + 1
    return np.arange(b, b + lay.nx)


@pytest.mark.parametrize("make", [lambda: pb.NlpLayout(2, 1), lambda: k3.MpcLayout(2, 1), _dual_layout],
                         ids=["ap2", "mpc", "dual"])
def test_owner_rule_against_the_layout(make):
    lay = make()
    col = np.full(lay.n_v, -1)
    row = np.full(lay.n_g, -1)
    for k in range(lay.n_k):
        coll = [f(k, j) for j in range(lay.d) for f in (lay.coll_x, lay.coll_z)]
        for idx in [lay.u(k), lay.xdot(k), lay.z(k)] + coll:
            col[idx] = k
        for idx in [lay.g_shooting(k), lay.g_path(k)] + [_g_coll(lay, k, j) for j in range(lay.d)]:
            row[idx] = k
    assert np.array_equal(column_owner(np.arange(lay.n_v), lay), col)
    assert np.array_equal(row_owner(np.arange(lay.n_g), lay), row)
    # the separators, by name: shooting states, globals, x[n_k]; continuity rows, rows outside the intervals
    seps = np.concatenate([lay.x(k) for k in range(lay.n_k + 1)] + [np.arange(lay.v_intervals)])
    assert (col[seps] == -1).all() and (col >= 0).sum() == lay.n_v - len(seps)
    cont = np.concatenate([_g_continuity(lay, k) for k in range(lay.n_k)])
    g0 = getattr(lay, "g_int0", 0)
    outside = np.concatenate([np.arange(g0), np.arange(g0 + lay.n_k * lay.rows_per_interval, lay.n_g)])
    assert len(outside) > 0
    assert (row[cont] == -1).all() and (row[outside] == -1).all()
    assert (row >= 0).sum() == lay.n_g - len(cont) - len(outside)
    # a subset in any order gives the same owners
    pick = np.random.default_rng(0).permutation(lay.n_v)[:lay.n_v // 2]
    assert np.array_equal(column_owner(pick, lay), col[pick])


def test_more_leading_rows_than_states_are_refused():
    lay = k3.MpcLayout(2, 1)
    lay.g_int0 = lay.nx + 1
    with pytest.raises(ValueError, match="leading rows"):
        row_owner(np.arange(3), lay)


# ------------------------------------------------------------------------------- block_entries
def test_block_entries_match_the_dictionary_loop():
    from awebox_amd.mpc import sparsity_jac_static
    lay = k3.MpcLayout(2, 1)
    colind, row = sparsity_jac_static(k3.build_constants(k3.Kite3Config(n_k=2, d=1)))
    jcol = np.repeat(np.arange(lay.n_v), np.diff(colind))
    blocks = [(np.concatenate([lay.g_shooting(0)] + [lay.g_coll(0, j) for j in range(lay.d)]),
               np.concatenate([lay.xdot(0), lay.z(0)] + [np.concatenate([lay.coll_x(0, j), lay.coll_z(0, j)])
                                                         for j in range(lay.d)])),
              (lay.g_shooting(0), np.concatenate([lay.xdot(0), lay.z(0)])),
              (lay.g_continuity(1)[::-1], lay.x(2))]                # rows in another order
    for rows, cols in blocks:
        rsel = {int(r): i for i, r in enumerate(rows)}
        csel = {int(c): i for i, c in enumerate(cols)}
        pk = [e for e in range(len(row)) if int(row[e]) in rsel and int(jcol[e]) in csel]
        dst = [rsel[int(row[e])] * len(rsel) + csel[int(jcol[e])] for e in pk]
        keep, got = block_entries(row, jcol, rows, cols)
        assert len(rows) == len(cols) and len(pk) > 0
        assert keep.tolist() == pk and got.tolist() == dst
