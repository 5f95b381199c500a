"""The numpy restatement of the curve-based ensemble statistics, written from the contract of include/esim.h and
from nothing in the package: over a stack [members, rows, cols] of keys (uint32 in the store's order, or int32 for the signed
kinds -- numpy compares either as the numbers they are) the depth numerators, their totals, and the central region with its
envelope.  brute_depth enumerates the pairs themselves, for the tests that check the counting rule."""
import itertools

import numpy as np


def pairs(m):
    return int(m) * (int(m) - 1) // 2


def depth(stack):
    """uint64 [members, cols]: per member and column the sum over the rows of C(M, 2) - C(below, 2) - C(above, 2)."""
    x = np.asarray(stack)
    m = x.shape[0]
    out = np.zeros((m, x.shape[2]), np.uint64)
    for i in range(m):
        below = (x < x[i]).sum(axis=0).astype(np.int64)
        above = (x > x[i]).sum(axis=0).astype(np.int64)
        out[i] = (pairs(m) - below * (below - 1) // 2 - above * (above - 1) // 2).sum(axis=0)
    return out


def brute_depth(stack):
    """The same by enumeration: the pairs {j, k}, j < k, of the members whose band holds member i's key, cell by cell."""
    x = np.asarray(stack).astype(np.int64)
    m = x.shape[0]
    out = np.zeros((m, x.shape[2]), np.uint64)
    for i in range(m):
        for j, k in itertools.combinations(range(m), 2):
            inside = (np.minimum(x[j], x[k]) <= x[i]) & (x[i] <= np.maximum(x[j], x[k]))
            out[i] += inside.sum(axis=0).astype(np.uint64)
    return out


def total(stack):
    """uint64 [members]: depth summed over the columns."""
    return depth(stack).sum(axis=1, dtype=np.uint64)


def band(stack, need, pooled):
    """{"lo", "hi", "median": [rows, cols] in the stack's dtype, "deepest", "n_in": uint32 [cols], "inside": bool [members, cols]}.
    Per column the need-th largest depth is the threshold and every member at or above it is in; pooled: the same with the totals,
    one set for all columns.  deepest: the smallest index among the members of the largest depth."""
    x = np.asarray(stack)
    m, _, cols = x.shape
    assert 1 <= need <= m
    d = depth(x)
    if pooled:
        d = np.repeat(d.sum(axis=1, dtype=np.uint64)[:, None], cols, axis=1)
    thr = np.sort(d, axis=0)[m - need]
    inside = d >= thr[None, :]
    deepest = np.argmax(d, axis=0)                                   # (the first of equals)
    big, small = (np.iinfo(x.dtype).max, np.iinfo(x.dtype).min)
    lo = np.where(inside[:, None, :], x, big).min(axis=0).astype(x.dtype)
    hi = np.where(inside[:, None, :], x, small).max(axis=0).astype(x.dtype)
    median = np.take_along_axis(x, np.broadcast_to(deepest[None, None, :], (1,) + x.shape[1:]), axis=0)[0]
    return {"lo": lo, "hi": hi, "median": median, "deepest": deepest.astype(np.uint32), "n_in": inside.sum(axis=0).astype(np.uint32), "inside": inside}
