"""The block apply's entry points on the host: exported, bound with the right arity, the static table as the oracle
has it, and bad arguments refused before they touch a device (no GPU needed: the argument checks come first)."""

import ctypes
import os
import re

import blocks_apply_cases as ac
from loona_amd import _lib, batch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hpk_apply_blocks", "hpk_static_table", "hpk_ctx_set_block_apply", "hpk_test_blkapply_geometry")


def test_exports_and_argtypes():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and getattr(L, name).restype is ctypes.c_int, name
    assert len(L.hpk_apply_blocks.argtypes) == 20
    assert (_lib.HPK_BLOCK_APPLY_HOST, _lib.HPK_BLOCK_APPLY_DEVICE, _lib.HPK_BLK_DEFERRED) == (0, 1, 10) and ac.E_DEFERRED == 10
    src = open(os.path.join(REPO, "include", "hpk.h")).read()
    assert re.search(r"#define HPK_BLK_DEFERRED 10\b", src) and re.search(r"#define HPK_DTAB_NO_LIMIT 0xFFFFFFFFu", src)
    assert batch.DTAB_DTYPE.itemsize == 32 and batch.HEADER_DTYPE.itemsize == 16 and batch.RESULT_DTYPE.itemsize == 16
    assert "block apply v1" in L.hpk_version().decode()


def test_static_table_is_the_oracles():
    text, ent = batch.static_table()
    got = [(text[e["name_off"] : e["name_off"] + e["name_len"]], text[e["value_off"] : e["value_off"] + e["value_len"]]) for e in ent]
    assert got == ac.static_table() and len(got) == 61
    assert len(text) == sum(len(n) + len(v) for n, v in got)  # end to end
    assert _lib.lib().hpk_static_table(None, None, None) == _lib.HPK_E_OK


def test_null_context_and_geometry():
    L = _lib.lib()
    b = (ctypes.c_uint8 * 256)()
    for flags in (_lib.HPK_PTR_DEVICE, _lib.HPK_PTR_DEVICE | _lib.HPK_ASYNC, _lib.HPK_PTR_HOST):
        assert L.hpk_apply_blocks(None, b, b, 1, b, b, b, 0, 0, 0, b, b, 1, b, b, 1, b, 1, b, flags) == _lib.HPK_E_INVAL
    assert L.hpk_ctx_set_block_apply(None, 1) == _lib.HPK_E_INVAL
    r, c, w = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    assert L.hpk_test_blkapply_geometry(ctypes.byref(r), ctypes.byref(c), ctypes.byref(w)) == _lib.HPK_E_OK
    assert r.value in (128, 256, 512, 1024, 2048) and c.value == 64 and w.value >= 1
    assert L.hpk_test_blkapply_geometry(None, ctypes.byref(c), ctypes.byref(w)) == _lib.HPK_E_INVAL
