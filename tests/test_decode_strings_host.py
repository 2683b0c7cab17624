"""The packed string-literal decode's entry point on the host: exported, bound with the right arity, its three
status values numbered as include/hpk.h states them, and refusing bad arguments before they touch a device (no
GPU needed: the argument checks come first)."""

import ctypes
import os
import re

from loona_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_export_and_argtypes():
    L = _lib.lib()
    assert "hpk_decode_strings_packed" in _lib.EXPORTS
    assert hasattr(L, "hpk_decode_strings_packed")
    assert len(L.hpk_decode_strings_packed.argtypes) == 13 and L.hpk_decode_strings_packed.restype is ctypes.c_int


def test_status_values():
    assert (_lib.HPK_PREFIX_TOO_MANY_OCTETS, _lib.HPK_PREFIX_NOT_ENOUGH_OCTETS, _lib.HPK_STRING_NOT_ENOUGH_OCTETS) == (6, 7, 8)
    assert _lib.HPK_BAD_OFFSETS == 5
    src = open(os.path.join(REPO, "include", "hpk.h")).read()
    for name, value in (("HPK_BAD_OFFSETS", 5), ("HPK_PREFIX_TOO_MANY_OCTETS", 6), ("HPK_PREFIX_NOT_ENOUGH_OCTETS", 7),
                        ("HPK_STRING_NOT_ENOUGH_OCTETS", 8)):
        assert re.search(rf"\b{name} = {value}\b", src), name
    assert "v1" in _lib.lib().hpk_version().decode() and "string-literal decode" in _lib.lib().hpk_version().decode()


def _bufs():
    b = (ctypes.c_uint8 * 64)()
    return b, (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 4)(), \
        (ctypes.c_uint32 * 4)(), (ctypes.c_uint8 * 4)()


def test_null_context():
    L = _lib.lib()
    b, so, se, oo, ol, co, st = _bufs()
    for flags in (_lib.HPK_PTR_DEVICE, _lib.HPK_PTR_HOST):
        assert L.hpk_decode_strings_packed(None, b, 64, so, se, 1, b, 64, oo, ol, co, st, flags) == _lib.HPK_E_INVAL
        assert L.hpk_decode_strings_packed(None, b, 64, so, None, 1, b, 64, oo, ol, None, st, flags) == _lib.HPK_E_INVAL


def test_null_arguments():
    """(the checks come before the context is used: any non-null address stands in for one)"""
    L = _lib.lib()
    b, so, se, oo, ol, co, st = _bufs()
    ctx = (ctypes.c_uint8 * 4096)()
    for flags in (_lib.HPK_PTR_DEVICE, _lib.HPK_PTR_HOST):
        call = lambda *a: L.hpk_decode_strings_packed(ctx, *a, flags)  # noqa: E731
        assert call(b, 64, None, se, 1, b, 64, oo, ol, co, st) == _lib.HPK_E_INVAL
        assert call(b, 64, so, se, 1, b, 64, None, ol, co, st) == _lib.HPK_E_INVAL
        assert call(b, 64, so, se, 1, b, 64, oo, None, co, st) == _lib.HPK_E_INVAL
        assert call(b, 64, so, se, 1, b, 64, oo, ol, co, None) == _lib.HPK_E_INVAL
        assert b"null argument" in L.hpk_last_error(None)
        assert call(b, 64, so, se, 0, b, 64, None, ol, co, st) == _lib.HPK_E_INVAL  # n == 0 too
        assert call(None, 64, so, se, 1, b, 64, oo, ol, co, st) == _lib.HPK_E_INVAL
        assert b"null blob" in L.hpk_last_error(None)
        assert call(b, 64, so, se, 1, None, 64, oo, ol, co, st) == _lib.HPK_E_INVAL
        assert call(b, 64, so, se, 0x7FFFFFFF, b, 64, oo, ol, co, st) == _lib.HPK_E_INVAL
