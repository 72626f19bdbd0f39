"""Helper (not a test): an independent restatement, in plain loops over numpy arrays, of the reference routines the device
path of discrete networks replaces - written from the cited lines, not from pybnesian_amd/factors.py.

- joint_counts: factors/discrete/discrete_indices.cpp:134-150 over the rows the combined bitmap keeps (a row with a null in
  any variable of the family is dropped);
- logprob: learning/parameters/mle_DiscreteFactor.cpp:14-38;
- row_logl: factors/discrete/DiscreteFactor.cpp:91-119 (NaN where the combined bitmap is unset);
- network_logl: models/BayesianNetwork.hpp:960-994, the nodes added one at a time in node order;
- slogl_exact: DiscreteFactor.cpp:133-158 summed EXACTLY (math.fsum), with the sum of magnitudes the error bounds need.

Codes are int32 arrays, -1 = null.  A family is (variable, [parents...]) over column indices; its table has the variable
fastest and the parents in the order given."""
import math

import numpy as np


def strides_of(cards, family):
    cols = [family[0]] + list(family[1])
    strides, s = [], 1
    for c in cols:
        strides.append(s)
        s *= int(cards[c])
    return cols, strides, s


def joint_index(codes, cards, family):
    """(index per row, valid per row)."""
    cols, strides, _ = strides_of(cards, family)
    n = len(codes[cols[0]]) if cols else 0
    index = np.zeros(n, dtype=np.int64)
    valid = np.ones(n, dtype=bool)
    for c, s in zip(cols, strides):
        col = np.asarray(codes[c], dtype=np.int64)
        valid &= col >= 0
        index += np.where(col >= 0, col, 0) * s
    return index, valid


def joint_counts(codes, cards, family):
    _, _, cells = strides_of(cards, family)
    index, valid = joint_index(codes, cards, family)
    counts = np.zeros(cells, dtype=np.int64)
    for i in index[valid]:
        counts[i] += 1
    return counts


def joint_counts_fast(codes, cards, family):
    """The same table through numpy.bincount, for tables of many rows (checked against joint_counts in the CPU tier)."""
    _, _, cells = strides_of(cards, family)
    index, valid = joint_index(codes, cards, family)
    return np.bincount(index[valid], minlength=cells).astype(np.int64)


def logprob(counts, card):
    out = np.zeros(len(counts), dtype=np.float64)
    for k in range(len(counts) // card):
        block = counts[k * card: (k + 1) * card]
        total = int(block.sum())
        for i in range(card):
            if total == 0:
                out[k * card + i] = math.log(1.0 / card)
            else:
                out[k * card + i] = (math.log(float(block[i])) if block[i] > 0 else -math.inf) - math.log(float(total))
    return out


def row_logl(codes, cards, family, lp):
    index, valid = joint_index(codes, cards, family)
    out = np.full(len(index), np.nan)
    out[valid] = np.asarray(lp, dtype=np.float64)[index[valid]]
    return out


def network_logl(codes, cards, families, lps):
    out = None
    for family, lp in zip(families, lps):
        ll = row_logl(codes, cards, family, lp)
        out = ll if out is None else out + ll
    return out


def slogl_exact(codes, cards, family, lp):
    """(exact sum of logprob over the valid rows, exact sum of their magnitudes = sum over the cells of |count x logprob|,
    cells); -inf when a row falls on a cell of probability zero."""
    _, _, cells = strides_of(cards, family)
    index, valid = joint_index(codes, cards, family)
    values = np.asarray(lp, dtype=np.float64)[index[valid]].tolist()
    return math.fsum(values), math.fsum(abs(v) for v in values), cells


def slogl_bound(cells, magnitude):
    """One rounding per product and recursive summation over the cells: (cells + 1) 2^-53 sum |count x logprob|."""
    return (cells + 1) * 2.0 ** -53 * magnitude
