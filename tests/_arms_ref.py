"""Plain numpy for the policy grids of esim_arms.h: the definition that the arms tests compare with.  The members are read as
replicates of arms, slot = replicate * n_arms + arm.  Keys are below 2^32 and there are at most 256 members, so a sum over the
replicates stays below 2^40; the totals over the cells are summed in uint64, which holds 2^32 cells of such keys."""
import numpy as np

NEVER = 0xFFFFFFFF
KEYS = ("best", "sole", "regret", "sum", "totals")


def arms(x, n_arms, maximize=False, never_as=None, has_never=True):
    """For planes x [M, ...] (every axis behind the first is a cell axis and keeps its shape): {"best", "sole": uint32 [A, ...],
    "regret", "sum": uint64 [A, ...], "totals": uint64 [S, A]} with S = M / A.  never_as replaces NEVER first where the store
    can hold it (has_never); None leaves it."""
    x = np.asarray(x)
    assert x.dtype == np.uint32 and n_arms >= 1 and x.shape[0] % n_arms == 0
    if has_never and never_as is not None:
        x = np.where(x == NEVER, np.uint32(never_as), x)
    a, s = int(n_arms), x.shape[0] // int(n_arms)
    k = x.astype(np.int64).reshape((s, a) + x.shape[1:])            # [S, A, ...]
    b = k.max(axis=1, keepdims=True) if maximize else k.min(axis=1, keepdims=True)
    eq = k == b
    alone = eq & (eq.sum(axis=1, keepdims=True) == 1)
    cells = tuple(range(2, k.ndim))
    return {"best": eq.sum(axis=0).astype(np.uint32), "sole": alone.sum(axis=0).astype(np.uint32), "regret": np.abs(k - b).sum(axis=0).astype(np.uint64),
            "sum": k.sum(axis=0).astype(np.uint64), "totals": k.astype(np.uint64).sum(axis=cells, dtype=np.uint64).reshape(s, a)}


def live_cells(zero, never, first, n):
    """The cells of [first, first + n) that the skip tables do not settle (members_trivial)."""
    live = np.ones(n, bool)
    if never is not None:
        live &= never[first:first + n] != 0
    if zero is not None:
        live &= zero[first:first + n] != 0
    return int(live.sum())
