"""The marshalling rules every binding of libesim shares, as pure functions: the ctypes pointer of an array, zeroed output
arrays by key, the code of a `where`, the default number of rows of a series, the two-call sizing protocol and the rate of two
count tables.  Nothing here loads the library or knows a Simulator (of _lib only the constants are used);
what needs a simulator's state (_n_cols, _last, ...) is a method of Simulator."""
import ctypes as C

import numpy as np

from . import _lib

_POINTER = {np.dtype(d): C.POINTER(t) for d, t in ((np.uint8, C.c_uint8), (np.uint16, C.c_uint16), (np.uint32, C.c_uint32), (np.int32, C.c_int32),
                                                   (np.uint64, C.c_uint64), (np.int64, C.c_int64), (np.float64, C.c_double))}
PLACES = {"current": _lib.AREA_CURRENT, "home": _lib.AREA_HOME, "group": _lib.BY_GROUP, "setting": _lib.BY_SETTING, "all": _lib.BY_ALL}
STATUS = {"susceptible": _lib.SUSCEPTIBLE, "exposed": _lib.EXPOSED, "infected": _lib.INFECTED, "recovered": _lib.RECOVERED, "vaccinated": _lib.VACCINATED}


def ptr(a):
    """The ctypes pointer of a contiguous numpy array, typed by its dtype; None for None, TypeError for a dtype no call takes."""
    if a is None:
        return None
    if a.dtype not in _POINTER:
        raise TypeError("no libesim call takes an array of %s" % a.dtype)
    return a.ctypes.data_as(_POINTER[a.dtype])


def zeros(keys, shape, u64=(), u8=()):
    """{key: zeroed array of `shape`} in the order of `keys`: uint32, but uint64 for the keys in `u64` and uint8 for those in
    `u8` -- so *(ptr(out[k]) for k in keys) are the output arguments of a call in its own order."""
    return {k: np.zeros(shape, np.uint64 if k in u64 else np.uint8 if k in u8 else np.uint32) for k in keys}


def place_code(where, names):
    """`where` as its code.  names: the space-separated names this call takes, out of current home group setting all; another
    string raises ValueError before the library is touched.  A code passes through: the library refuses what it does not take
    (every call that counts by area refuses "current" unless its docstring offers it)."""
    if isinstance(where, str):
        if where not in names.split():
            raise ValueError("where must be one of %s, got %r" % (", ".join(repr(n) for n in names.split()), where))
        return PLACES[where]
    return int(where)


def default_rows(first, stride, last, lowest):
    """The rows of a series from step `first` in strides up to step `last` -- what n_rows=None means; 0 where there is none
    (stride 0, first below `lowest`, which is 1 for the rows of a status and 0 where step 0 is the cohort of the index cases,
    or first beyond last)."""
    return (last - int(first)) // int(stride) + 1 if stride and lowest <= first <= last else 0


def sized(call, make_arrays, empty_ok=False):
    """The two-call protocol of the outputs whose length only the library knows.  call(pointers, cap, byref(n)) is made with
    null pointers and cap 0 for the number of entries n, then with those of make_arrays(n) -- a list or dict of arrays -- only
    where the first answered ESIM_ERANGE: buffers are needed, or the arguments are refused, which the second call says again.
    empty_ok: ESIM_ERANGE with n == 0 is no error and no second call is made.  Returns (the last code, the arrays)."""
    n = C.c_uint32(0)
    code = call([None] * len(make_arrays(0)), 0, C.byref(n))
    arrays = make_arrays(n.value)
    if code == _lib.ESIM_ERANGE and empty_ok and not n.value:
        return _lib.ESIM_OK, arrays
    if code == _lib.ESIM_ERANGE:
        code = call([ptr(a) for a in (arrays.values() if isinstance(arrays, dict) else arrays)], n.value, C.byref(n))
    return code, arrays


def rate(num, den):
    """num / den as float64, NaN where den == 0."""
    n, d = np.asarray(num, np.float64), np.asarray(den, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(d > 0, n / d, np.nan)
