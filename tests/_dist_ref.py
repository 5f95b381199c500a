"""Plain numpy for the pairwise distances of esim_dist.h and a brute-force k-medoids, what the distance tests compare with.
Member i is compared with all members at once in int64, so that 256 members x 1000 cells stay small."""
import itertools

import numpy as np

NEVER = 0xFFFFFFFF
METRICS = {"l1": 0, "differ": 1}


def substitute(planes, never_as=None):
    """The keys with NEVER replaced by never_as (None: as they are), uint32."""
    x = np.asarray(planes)
    if x.dtype == np.int32:                                         # a signed store: its keys differ as its values do
        return (x.astype(np.int64) + (1 << 31)).astype(np.uint32)
    x = x.astype(np.uint32)
    return x if never_as is None else np.where(x == NEVER, np.uint32(never_as), x)


def distances(planes, metric, never_as=None):
    """uint64 [m, m] for planes [m, ...]: every axis behind the first is summed over."""
    x = substitute(planes, never_as)
    m = x.shape[0]
    x = x.reshape(m, -1).astype(np.int64)
    out = np.zeros((m, m), np.uint64)
    for i in range(m):
        if metric in ("l1", 0):
            out[i] = np.abs(x - x[i]).sum(axis=1, dtype=np.uint64) if x.shape[1] else 0
        elif metric in ("differ", 1):
            out[i] = (x != x[i]).sum(axis=1, dtype=np.uint64)
        else:
            raise ValueError(metric)
    return out


def live_cells(zero, never, first, n):
    """The cells of [first, first + n) that the skip tables do not settle (members_trivial)."""
    live = np.ones(n, bool)
    if never is not None:
        live &= never[first:first + n] != 0
    if zero is not None:
        live &= zero[first:first + n] != 0
    return int(live.sum())


def cost_of(d, medoid):
    """(cost, labels) of a set of medoids: every member to its nearest medoid, ties to the first in `medoid`."""
    d = np.asarray(d)
    sub = d[:, list(medoid)]
    label = sub.argmin(axis=1)
    return int(sum(int(sub[i, label[i]]) for i in range(d.shape[0]))), label


def best_medoids(d, k):
    """The smallest cost over all C(M, k) sets of medoids, by brute force."""
    m = np.asarray(d).shape[0]
    return min(cost_of(d, c)[0] for c in itertools.combinations(range(m), k))
