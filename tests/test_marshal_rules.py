"""The pure functions of epidemicsimulator_amd/_marshal.py on their own: pointers by dtype, zeroed outputs by key, the code of a
`where`, the default rows of a series, the two-call sizing protocol and the rate."""
import ctypes as C

import numpy as np
import pytest

from epidemicsimulator_amd import _lib


def test_the_pure_rules_of_marshal():
    from epidemicsimulator_amd import _marshal as m
    for dtype, ctype in ((np.uint8, C.c_uint8), (np.uint16, C.c_uint16), (np.uint32, C.c_uint32), (np.int32, C.c_int32), (np.uint64, C.c_uint64),
                         (np.int64, C.c_int64), (np.float64, C.c_double)):
        a = np.arange(3).astype(dtype)
        p = m.ptr(a)
        assert isinstance(p, C.POINTER(ctype)) and C.addressof(p.contents) == a.ctypes.data and p[2] == 2
    assert m.ptr(None) is None
    for bad in (np.float32, np.int16, bool):
        with pytest.raises(TypeError):
            m.ptr(np.zeros(2, bad))
    out = m.zeros(("a", "b", "c"), (2, 3), u64=("b",), u8=("c",))
    assert list(out) == ["a", "b", "c"] and [v.dtype for v in out.values()] == [np.uint32, np.uint64, np.uint8]
    assert all(v.shape == (2, 3) and not v.any() for v in out.values())
    assert [m.place_code(w, "current home group setting all") for w in ("current", "home", "group", "setting", "all")] == \
        [_lib.AREA_CURRENT, _lib.AREA_HOME, _lib.BY_GROUP, _lib.BY_SETTING, _lib.BY_ALL]
    assert m.place_code(np.int64(7), "home") == 7 and type(m.place_code(np.int64(7), "home")) is int
    for where, names in (("all", "current home"), ("", "home"), ("hom", "home"), ("areas", "current home group setting all")):
        with pytest.raises(ValueError):
            m.place_code(where, names)
    assert [m.default_rows(*a) for a in ((1, 1, 100, 1), (0, 1, 100, 1), (0, 24, 100, 0), (100, 7, 100, 1), (101, 7, 100, 1), (3, 0, 100, 1), (5, 7, 40, 0))] == \
        [100, 0, 5, 1, 0, 0, 6]
    assert np.array_equal(m.rate([1, 0, 3], [2, 0, 4]), [0.5, np.nan, 0.75], equal_nan=True)


def test_sized_calls_again_only_on_erange():
    from epidemicsimulator_amd._marshal import sized
    for first, n, empty_ok, calls, code in ((_lib.ESIM_ERANGE, 3, False, 2, _lib.ESIM_OK), (_lib.ESIM_OK, 0, False, 1, _lib.ESIM_OK),
                                            (_lib.ESIM_ERANGE, 0, False, 2, _lib.ESIM_ERANGE), (_lib.ESIM_ERANGE, 0, True, 1, _lib.ESIM_OK),
                                            (-2, 0, True, 1, -2)):
        seen = []

        def call(ptrs, cap, ref):
            seen.append((list(ptrs), cap))
            ref._obj.value = n
            return first if len(seen) == 1 or not n else _lib.ESIM_OK
        got, arrays = sized(call, lambda k: [np.zeros(k, np.uint32), np.zeros(k, np.uint8)], empty_ok)
        assert got == code and len(seen) == calls and seen[0] == ([None, None], 0) and [a.shape for a in arrays] == [(n,), (n,)]
        if calls == 2:
            assert seen[1][1] == n and all(p is not None for p in seen[1][0])
