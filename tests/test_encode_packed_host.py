"""The packed encode's two entry points on the host: exported, bound with the right arity, and refusing bad
arguments before they touch a device (no GPU needed: the argument checks come first)."""

import ctypes

from loona_amd import _lib


def test_exports_and_argtypes():
    L = _lib.lib()
    assert "hpk_encoded_len_batch" in _lib.EXPORTS and "hpk_encode_batch_packed" in _lib.EXPORTS
    assert len(L.hpk_encoded_len_batch.argtypes) == 7 and L.hpk_encoded_len_batch.restype is ctypes.c_int
    assert len(L.hpk_encode_batch_packed.argtypes) == 11 and L.hpk_encode_batch_packed.restype is ctypes.c_int


def _bufs():
    b = (ctypes.c_uint8 * 64)()
    o = (ctypes.c_uint32 * 4)()
    return b, o, (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 4)(), (ctypes.c_uint8 * 4)()


def test_null_context():
    L = _lib.lib()
    b, io, oo, ol, st = _bufs()
    dev = _lib.HPK_PTR_DEVICE
    assert L.hpk_encoded_len_batch(None, b, 64, io, 1, ol, dev) == _lib.HPK_E_INVAL
    assert L.hpk_encode_batch_packed(None, b, 64, io, 1, b, 64, oo, ol, st, dev) == _lib.HPK_E_INVAL


def test_host_pointer_flags_and_null_offsets():
    """(the checks come before the context is used: any non-null address stands in for one)"""
    L = _lib.lib()
    b, io, oo, ol, st = _bufs()
    ctx = (ctypes.c_uint8 * 4096)()
    dev = _lib.HPK_PTR_DEVICE
    for flags in (_lib.HPK_PTR_HOST, _lib.HPK_PTR_HOST | _lib.HPK_ASYNC):
        assert L.hpk_encoded_len_batch(ctx, b, 64, io, 1, ol, flags) == _lib.HPK_E_INVAL
        assert b"device pointers only" in L.hpk_last_error(None)
        assert L.hpk_encode_batch_packed(ctx, b, 64, io, 1, b, 64, oo, ol, st, flags) == _lib.HPK_E_INVAL
        assert b"device pointers only" in L.hpk_last_error(None)
    assert L.hpk_encoded_len_batch(ctx, b, 64, None, 1, ol, dev) == _lib.HPK_E_INVAL
    assert L.hpk_encoded_len_batch(ctx, b, 64, io, 1, None, dev) == _lib.HPK_E_INVAL
    assert L.hpk_encode_batch_packed(ctx, b, 64, None, 1, b, 64, oo, ol, st, dev) == _lib.HPK_E_INVAL
    assert L.hpk_encode_batch_packed(ctx, b, 64, io, 1, b, 64, None, ol, st, dev) == _lib.HPK_E_INVAL
    assert L.hpk_encode_batch_packed(ctx, b, 64, io, 1, b, 64, oo, None, st, dev) == _lib.HPK_E_INVAL
    assert L.hpk_encode_batch_packed(ctx, b, 64, io, 1, b, 64, oo, ol, None, dev) == _lib.HPK_E_INVAL
    assert L.hpk_encode_batch_packed(ctx, b, 64, io, 0, b, 64, None, ol, st, dev) == _lib.HPK_E_INVAL  # n == 0 too
