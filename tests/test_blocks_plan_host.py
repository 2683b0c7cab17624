"""The block plan's entry points on the host: exported, bound with the right arity, bad arguments refused before
they touch a device, the testing-only hash, and hpk_henc_table_size (no GPU needed: the argument checks come first)."""

import ctypes
import os
import re

import numpy as np

from hpk_util import hpack_ref
from loona_amd import _lib, batch, hpack

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hpk_plan_blocks", "hpk_test_plan_calls", "hpk_ctx_set_block_plan", "hpk_test_blkplan_geometry", "hpk_test_blkplan_hash", "hpk_henc_table_size")


def test_exports_and_argtypes():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and getattr(L, name).restype is (ctypes.c_uint64 if name == "hpk_test_plan_calls" else ctypes.c_int), name
    assert L.hpk_test_plan_calls(None) == 0
    assert len(L.hpk_plan_blocks.argtypes) == 22
    assert (_lib.HPK_PLAN_NONE, _lib.HPK_PLAN_INDEXED, _lib.HPK_PLAN_NAME_INDEXED, _lib.HPK_PLAN_NEW_NAME) == (0, 1, 2, 3)
    src = open(os.path.join(REPO, "include", "hpk.h")).read()
    assert re.search(r"HPK_PLAN_NONE = 0, HPK_PLAN_INDEXED = 1, HPK_PLAN_NAME_INDEXED = 2,\s+HPK_PLAN_NEW_NAME = 3", src)
    assert batch.HREP_DTYPE.itemsize == 16 and batch.HREP_DTYPE.fields["prefix"][1] == 8
    assert "block plan v1" in L.hpk_version().decode()


def test_null_context_and_geometry():
    L = _lib.lib()
    b = (ctypes.c_uint8 * 256)()
    for flags in (_lib.HPK_PTR_DEVICE, _lib.HPK_PTR_DEVICE | _lib.HPK_ASYNC, _lib.HPK_PTR_HOST):
        assert L.hpk_plan_blocks(None, b, 256, 0, 0, 0, b, b, 1, 1, b, b, b, 1, b, b, 1, b, b, b, b, flags) == _lib.HPK_E_INVAL
    assert L.hpk_ctx_set_block_plan(None, 1) == _lib.HPK_E_INVAL
    assert (_lib.HPK_BLOCK_PLAN_HOST, _lib.HPK_BLOCK_PLAN_DEVICE) == (0, 1)
    r, c, w, g = (ctypes.c_uint32() for _ in range(4))
    assert L.hpk_test_blkplan_geometry(ctypes.byref(r), ctypes.byref(c), ctypes.byref(w), ctypes.byref(g)) == _lib.HPK_E_OK
    assert r.value in (128, 256, 512, 1024, 2048) and c.value == 64 and w.value >= 1 and g.value == 64
    assert L.hpk_test_blkplan_geometry(None, ctypes.byref(c), ctypes.byref(w), ctypes.byref(g)) == _lib.HPK_E_INVAL


def hashes(strs):
    blob = np.frombuffer(b"".join(strs) or b"\0", np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(s) for s in strs])]).astype(np.uint32)
    out = np.zeros(max(len(strs), 1), np.uint32)
    assert _lib.lib().hpk_test_blkplan_hash(blob.ctypes.data, off.ctypes.data, len(strs), out.ctypes.data) == _lib.HPK_E_OK
    return out[: len(strs)].tolist()


def test_hash_is_deterministic_and_of_the_bytes_alone():
    strs = [b"", b"a", b"b", b"ab", b"ba", b":method", b"x" * 300, b"a", b""]
    h = hashes(strs)
    assert h == hashes(strs) and h[1] == h[7] and h[0] == h[8]  # the same bytes, wherever they lie
    assert len(set(h[:7])) == 7
    assert hashes([b"zz" + s for s in strs]) != h
    L = _lib.lib()
    assert L.hpk_test_blkplan_hash(None, None, 0, None) == _lib.HPK_E_OK
    assert L.hpk_test_blkplan_hash(None, None, 1, None) == _lib.HPK_E_INVAL
    off = np.array([4, 2], np.uint32)  # decreasing
    assert L.hpk_test_blkplan_hash(off.ctypes.data, off.ctypes.data, 1, off.ctypes.data) == _lib.HPK_E_INVAL


def test_henc_table_size():
    e, ref = hpack.Encoder(), hpack_ref.Encoder()
    assert e.table_size() == (0, 0, 4096)
    headers = [(b":method", b"GET"), (b"x-a", b"1"), (b"x-bb", b"22"), (b"x-a", b"1"), (b"x-a", b"2")]
    assert e.encode(headers) == ref.encode(headers)
    assert e.table_size() == (36 + 38, 2, 4096) == (ref.dynamic.size, len(ref.dynamic.table), 4096)
    e.set_max_table_size(40)
    assert e.table_size() == (38, 1, 40)  # the oldest entry went
    e.set_max_table_size(0)
    assert e.table_size() == (0, 0, 0)
    L = _lib.lib()
    assert L.hpk_henc_table_size(None, None, None, None) == _lib.HPK_E_INVAL
    assert L.hpk_henc_table_size(e._h, None, None, None) == _lib.HPK_E_OK
