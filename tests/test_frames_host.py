"""The frame scan's entry points on the host: exported, bound with the right arity, their records the sizes hpk.h
states, and refusing bad arguments before they touch a device (no GPU needed: the argument checks come first)."""

import ctypes
import os
import re

import frames_cases as fc
from loona_amd import _lib, batch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hpk_scan_frames", "hpk_frame_blocks", "hpk_ctx_set_frame_scan", "hpk_test_frmscan_geometry")


def test_exports_and_argtypes():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and getattr(L, name).restype is ctypes.c_int, name
    assert len(L.hpk_scan_frames.argtypes) == 18 and len(L.hpk_frame_blocks.argtypes) == 12
    assert (_lib.HPK_FRAME_SCAN_HOST, _lib.HPK_FRAME_SCAN_DEVICE) == (0, 1)
    src = open(os.path.join(REPO, "include", "hpk.h")).read()
    assert re.search(r"#define HPK_FRAME_SCAN_HOST 0\b", src) and re.search(r"#define HPK_FRAME_SCAN_DEVICE 1\b", src)
    assert batch.FCONN_DTYPE.itemsize == 32 and batch.FBLOCK_DTYPE.itemsize == 16
    assert batch.FCONN_DTYPE == fc.FCONN_DTYPE and batch.FBLOCK_DTYPE == fc.FBLOCK_DTYPE
    assert "frame scan v1" in L.hpk_version().decode()


def test_null_context_and_geometry():
    L = _lib.lib()
    b = (ctypes.c_uint8 * 64)()
    o = (ctypes.c_uint32 * 4)()
    for flags in (_lib.HPK_PTR_DEVICE, _lib.HPK_PTR_DEVICE | _lib.HPK_ASYNC, _lib.HPK_PTR_HOST):
        assert L.hpk_scan_frames(None, b, 64, o, 1, b, b, 1, o, o, o, 1, o, o, o, 1, o, flags) == _lib.HPK_E_INVAL
        assert L.hpk_frame_blocks(None, b, 64, o, o, 1, b, 1, b, 64, o, flags) == _lib.HPK_E_INVAL
    assert L.hpk_ctx_set_frame_scan(None, _lib.HPK_FRAME_SCAN_DEVICE) == _lib.HPK_E_INVAL
    assert L.hpk_test_frmscan_geometry(None) == _lib.HPK_E_INVAL
    w = ctypes.c_uint32(0)
    assert L.hpk_test_frmscan_geometry(ctypes.byref(w)) == _lib.HPK_E_OK and w.value % 64 == 0 and w.value >= 64


def test_read_frames_without_a_context_is_the_host_path():
    """no context: the device frame scan is never asked, whatever a context elsewhere has selected"""
    from loona_amd import h2

    c = h2.Connection()
    r = h2.read_frames([c], [h2.frame(0x1, 0x4, 1, fc.B)], None)
    assert r.errors == [None] and r.consumed == [26] and len(r.blocks) == 1
