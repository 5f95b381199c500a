"""The numpy reference of the ensemble quantile maps and their rank rules, written from the definitions and from
nothing in the package: order statistics by a full sort over the member stack, exceedance by counting, the inverted-CDF rank by
a search over exact fractions."""
import fractions

import numpy as np

NEVER = 0xFFFFFFFF
TOP = 0x80000000


def order_statistics(stack, ranks):
    """[len(ranks), ...]: the ranks[q]-th smallest (0-based) over axis 0 of the [members, ...] stack, in the stack's own order
    (unsigned for uint32, signed for int32)."""
    ordered = np.sort(np.asarray(stack), axis=0)
    return np.stack([ordered[int(r)] for r in ranks])


def exceedance(stack, thresholds, never=False):
    """uint32 [len(thresholds), ...]: the members with x >= t, compared in int64 so that any threshold may be asked; with
    never=True a member at NEVER is >= every threshold."""
    x = np.asarray(stack).astype(np.int64)
    at_never = (np.asarray(stack) == NEVER) if never else np.zeros(x.shape, bool)
    return np.stack([((x >= int(t)) | at_never).sum(axis=0) for t in thresholds]).astype(np.uint32)


def to_key(signed):
    """int32 values as the keys the store holds: the top bit flipped, so that unsigned order is signed order."""
    return np.asarray(signed, np.int32).view(np.uint32) ^ np.uint32(TOP)


def from_key(key):
    return (np.asarray(key, np.uint32) ^ np.uint32(TOP)).view(np.int32)


def nearest_rank(p, m):
    """The inverted CDF by its definition: among m sorted members the smallest 0-based rank r such that the r + 1 members up to
    it are at least p * m, p an exact fraction; rank 0 for p = 0."""
    p = fractions.Fraction(p)
    for r in range(m):
        if r + 1 >= p * m:
            return r
    raise AssertionError((p, m))


def linear_quantile(stack, p):
    """numpy's default definition over axis 0, float64."""
    return np.quantile(np.asarray(stack).astype(np.float64), float(p), axis=0)
