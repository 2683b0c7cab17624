"""Host side of the packed output form (no GPU): the three new entry points are exported and bound, refuse
a NULL context, and the pack kernel's geometry is sane."""

import ctypes

from loona_amd import _lib

NEW = ("hpk_decode_batch_packed", "hpk_pack_batch", "hpk_test_pack_geometry")


def test_symbols_exported_and_bound():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    assert len(L.hpk_decode_batch_packed.argtypes) == len(L.hpk_decode_batch_compact.argtypes) == 11
    assert len(L.hpk_pack_batch.argtypes) == 10


def test_null_context_is_invalid():
    L = _lib.lib()
    off = (ctypes.c_uint32 * 2)(0, 0)
    ln = (ctypes.c_uint32 * 1)(0)
    st = (ctypes.c_uint8 * 1)(0)
    for flags in (_lib.HPK_PTR_DEVICE, _lib.HPK_PTR_DEVICE | _lib.HPK_ASYNC, _lib.HPK_PTR_HOST):
        assert L.hpk_decode_batch_packed(None, None, 0, off, 1, None, 0, off, ln, st, flags) == _lib.HPK_E_INVAL
        assert L.hpk_pack_batch(None, None, 0, off, ln, 1, None, 0, off, flags) == _lib.HPK_E_INVAL


def test_pack_geometry():
    L = _lib.lib()
    t, l = ctypes.c_uint32(0), ctypes.c_uint32(0)
    assert L.hpk_test_pack_geometry(ctypes.byref(t), ctypes.byref(l)) == _lib.HPK_E_OK
    assert t.value > 0 and t.value % 16 == 0
    assert l.value > 0
    assert L.hpk_test_pack_geometry(None, None) == _lib.HPK_E_INVAL
