"""The interval/separator partition of a collocation KKT pattern: which unknowns are interior to
which interval, where they sit in that interval's block, which separators each interval couples
to, and where every pattern entry lands in K_II, K_IS or K_SS.  ipm.StructuredKKT and
rti.BatchedRti both build their index tables from it; the stage order of the separators, the
assembly of the values and the algebra stay with each solve.  Index arithmetic only (numpy)."""
from __future__ import annotations

import numpy as np

from . import problem as pb


def _fields(lay):
    """What the owner rule reads from a layout (nx: states per shooting node; g_int0: rows in front
    of interval 0's, the MPC NLP's initial-condition rows)."""
    return (lay.n_k, lay.interval_stride, lay.v_intervals, lay.rows_per_interval,
            getattr(lay, "nx", pb.NX), getattr(lay, "g_int0", 0))


def layout_key(lay):
    """The layout as the owner rule sees it: two evaluators whose layouts agree here (and whose NLPs
    have the same patterns) share one KKT structure."""
    return (type(lay).__name__,) + _fields(lay)


def column_owner(cols, lay):
    """The interval that owns each V column, -1 for a separator: u[k], xdot[k], z[k] and the
    collocation variables belong to interval k; x[k] (the first nx of the interval's stride), the
    globals in front of the intervals and x[n_k] behind them are separators."""
    n_k, stride, v0, _, nx, _ = _fields(lay)
    cols = np.asarray(cols, dtype=np.int64)
    k, o = np.divmod(cols - v0, stride)
    return np.where((cols >= v0) & (k < n_k) & (o >= nx), k, -1)


def row_owner(rows, lay):
    """The interval that owns each g row, -1 for a separator: the node, path and collocation rows
    belong to interval k; its last nx rows (continuity: an interval has more rows than interior
    unknowns, x[k] and x[k+1] close the count) and the rows outside the intervals are separators."""
    n_k, _, _, per, nx, g0 = _fields(lay)
    if g0 > nx:
        raise ValueError("more leading rows than states per node")
    r = np.asarray(rows, dtype=np.int64) - g0
    return np.where((r >= 0) & (r < n_k * per) & (r % per < per - nx), r // per, -1)


def block_entries(row, col, rows, cols):
    """The COO entries (row[e], col[e]) inside the dense block rows x cols: (keep, dst) with keep the
    entry indices in ascending order and dst their row-major positions in the block."""
    row, col, rows, cols = (np.asarray(a, dtype=np.int64) for a in (row, col, rows, cols))
    rpos = np.full(max(row.max(), rows.max()) + 1, -1, dtype=np.int64)
    cpos = np.full(max(col.max(), cols.max()) + 1, -1, dtype=np.int64)
    rpos[rows] = np.arange(len(rows))
    cpos[cols] = np.arange(len(cols))
    keep = np.where((rpos[row] >= 0) & (cpos[col] >= 0))[0]
    return keep, rpos[row[keep]] * len(cols) + cpos[col[keep]]


def group_positions(group, n):
    """(pos, counts): the position of every element among the elements of its group (0 .. n - 1), in
    ascending element order, and the group sizes."""
    counts = np.bincount(group, minlength=n).astype(np.int64)
    order = np.argsort(group, kind="stable")
    pos = np.empty(len(group), dtype=np.int64)
    pos[order] = np.arange(len(group)) - (np.cumsum(counts) - counts)[group[order]]
    return pos, counts


class IntervalPartition:
    """``owner[p]``: the interval of unknown p, -1 for a separator; (P, Q): the KKT pattern in COO,
    in the caller's value order.  With nI the largest interior, nS the separators and L the longest
    coupled-separator list (at least 1):

    sep, sep_id     the separators, and unknown -> separator number (-1 for interiors)
    loc, counts     unknown -> position in its interval's block (ascending unknown order), block sizes
    int_p, int_flat the interior unknowns and their slots k nI + loc in [n_k, nI]; sep_p = sep
    ii, is_, ss     the entries of K_II, K_IS and K_SS (entry indices, ascending)
    lsep_arr, lpos  [n_k, L] each interval's coupled separators, ascending, padded with nS, and
                    its inverse [n_k, nS + 1] (-1 where not coupled)
    dst_ii, dst_is  the entries' positions in [n_k, nI, nI] and [n_k, nI, L] of one instance
    ss_r, ss_c      the K_SS entries' separator numbers
    pad             the diagonal positions in [n_k, nI, nI] behind the interiors of short blocks
    r_idx, c_idx    [n_k, L, L] separator numbers of interval k's Schur block K_SI K_II^-1 K_IS
    """

    def __init__(self, owner, P, Q, n_k):
        owner, P, Q = (np.asarray(a, dtype=np.int64) for a in (owner, P, Q))
        N = len(owner)
        self.owner, self.n_k = owner, n_k
        self.sep = self.sep_p = sep = np.where(owner < 0)[0]
        self.nS = nS = len(sep)
        self.sep_id = sep_id = np.full(N, -1, dtype=np.int64)
        sep_id[sep] = np.arange(nS)
        self.int_p = ip = np.where(owner >= 0)[0]
        self.loc = loc = np.full(N, -1, dtype=np.int64)
        loc[ip], self.counts = group_positions(owner[ip], n_k)
        self.nI = nI = int(self.counts.max())
        self.int_flat = owner[ip] * nI + loc[ip]
        oP, oQ = owner[P], owner[Q]
        if ((oP >= 0) & (oQ >= 0) & (oP != oQ)).any():
            raise ValueError("KKT couples the interiors of two intervals")
        self.ii = ii = np.where((oP >= 0) & (oP == oQ))[0]
        self.is_ = isi = np.where((oP >= 0) & (oQ < 0))[0]
        self.ss = ss = np.where((oP < 0) & (oQ < 0))[0]
        # every interval's coupled separators: the distinct (interval, separator) pairs, sorted
        pk, ps = np.divmod(np.unique(oP[isi] * (nS + 1) + sep_id[Q[isi]]), nS + 1)
        pi, n_l = group_positions(pk, n_k)
        self.L = L = max(1, int(n_l.max()))
        self.lsep_arr = np.full((n_k, L), nS, dtype=np.int64)           # padding -> dummy separator
        self.lpos = np.full((n_k, nS + 1), -1, dtype=np.int64)
        self.lsep_arr[pk, pi] = ps
        self.lpos[pk, ps] = pi
        self.dst_ii = oP[ii] * nI * nI + loc[P[ii]] * nI + loc[Q[ii]]
        self.dst_is = oP[isi] * nI * L + loc[P[isi]] * L + self.lpos[oP[isi], sep_id[Q[isi]]]
        self.ss_r, self.ss_c = sep_id[P[ss]], sep_id[Q[ss]]
        k_, j_ = np.nonzero(np.arange(nI)[None, :] >= self.counts[:, None])   # padding rows, by interval
        self.pad = k_ * nI * nI + j_ * nI + j_
        self.r_idx = self.lsep_arr[:, :, None].repeat(L, axis=2)
        self.c_idx = self.lsep_arr[:, None, :].repeat(L, axis=1)
