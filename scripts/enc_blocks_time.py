#!/usr/bin/env python3
"""Wall time of hpk_henc_encode_blocks through a device context, the C call alone (arrays marshalled once, fresh
encoders per call): `python scripts/enc_blocks_time.py [scale] [reps] [rounds]`. The header lists are the
interop stories' (tests/golden/interop.json.gz), `scale` copies of them over 64 Huffman-coding encoders. One
JSON line per round; the first call's blocks are hashed so two builds (HPK_LIB) can be compared byte for byte.
The call is host-bound: compare ranges over rounds, not single figures."""
import ctypes
import gzip
import hashlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from loona_amd import HuffmanCodec, _lib  # noqa: E402


def main():
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    with gzip.open(os.path.join(REPO, "tests", "golden", "interop.json.gz")) as f:
        inter = json.load(f)
    lists = [[(k.encode(), v.encode()) for k, v in c["headers"]] for enc in sorted(inter) for st in inter[enc]
             for c in st["cases"]] * scale
    parts, off, hoff = [], [0], [0]
    for hs in lists:
        for name, value in hs:
            for x in (name, value):
                parts.append(x)
                off.append(off[-1] + len(x))
        hoff.append(hoff[-1] + len(hs))
    fields = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    off32, hoff32 = np.asarray(off, np.uint32), np.asarray(hoff, np.uint32)
    n, k = len(lists), 64
    L = _lib.lib()
    codec = HuffmanCodec(0)

    def call(keep=False):
        hs = [L.hpk_henc_create(1) for _ in range(k)]
        encs = (ctypes.c_void_p * n)(*[hs[i % k] for i in range(n)])
        out = _lib.HencOut()
        t0 = time.perf_counter()
        rc = L.hpk_henc_encode_blocks(codec._h, encs, fields.ctypes.data, off32.ctypes.data, hoff32.ctypes.data, n,
                                      ctypes.byref(out))
        dt = time.perf_counter() - t0
        _lib.check(rc, "hpk_henc_encode_blocks")
        res = (hashlib.sha256(ctypes.string_at(out.bytes, out.len)).hexdigest(), out.len) if keep else None
        L.hpk_henc_out_free(ctypes.byref(out))
        for h in hs:
            L.hpk_henc_destroy(h)
        return dt, res

    _, (digest, nbytes) = call(keep=True)
    call()
    for r in range(rounds):
        ts = sorted(call()[0] for _ in range(reps))
        print(json.dumps({"blocks": n, "fields_bytes": int(fields.size), "block_bytes": nbytes, "sha256": digest[:16],
                          "round": r, "reps": reps, "min_ms": round(ts[0] * 1e3, 2),
                          "median_ms": round(ts[len(ts) // 2] * 1e3, 2), "max_ms": round(ts[-1] * 1e3, 2),
                          "lib": os.path.basename(os.environ.get("HPK_LIB", "libhpk.so"))}), flush=True)


if __name__ == "__main__":
    main()
