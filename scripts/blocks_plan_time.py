#!/usr/bin/env python3
"""Wall time of hpk_henc_encode_blocks through a device context with the table logic on the host or on the device
(hpk_ctx_set_block_plan), the C call alone (arrays marshalled once, fresh encoders per call):
`python scripts/blocks_plan_time.py [host|device|split|alone] [encoders] [scale] [reps] [rounds]`. The header lists are
scripts/enc_blocks_time.py's corpus: the interop stories' (tests/golden/interop.json.gz), `scale` copies of them dealt
round-robin over `encoders` Huffman-coding encoders. One JSON line per round; the first call's blocks are hashed so
that two settings or two builds (HPK_LIB; a build without the setting runs `host` only) can be compared byte for byte.
`split` is `device` under HPK_HENC_TIMING: the library waits for the stream after each pass of the device path and
prints the passes' wall times to stderr, which this script catches and gives back as one JSON line per timed call.
`alone` times hpk_plan_blocks by itself on device-resident inputs, empty tables, and then the same call holding only
its longest encoder's list, which bounds the call from below. Compare ranges over rounds, not single figures."""
import ctypes
import gzip
import hashlib
import json
import os
import re
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from loona_amd import HuffmanCodec, _lib  # noqa: E402


def corpus(scale):
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
    return len(lists), b"".join(parts), np.asarray(off, np.uint32), np.asarray(hoff, np.uint32)


def stats(ts):
    ts = sorted(ts)
    return {"min_ms": round(ts[0] * 1e3, 3), "median_ms": round(ts[len(ts) // 2] * 1e3, 3), "max_ms": round(ts[-1] * 1e3, 3)}


def encode(setting, k, scale, reps, rounds):
    split = setting == "split"
    if split:  # (read by the library, so set before its first call; its lines go to a file that stands in for stderr)
        os.environ["HPK_HENC_TIMING"] = "1"
        setting = "device"
        caught = tempfile.TemporaryFile()
        sys.stderr.flush()
        os.dup2(caught.fileno(), 2)
    n, text, off32, hoff32 = corpus(scale)
    fields = np.frombuffer(text, dtype=np.uint8).copy()
    L = _lib.lib()
    codec = HuffmanCodec(0)
    if hasattr(L, "hpk_ctx_set_block_plan"):
        codec.set_block_plan(setting)
    elif setting != "host":
        raise SystemExit("this build has no block plan setting")

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
    if split:
        caught.seek(0, os.SEEK_END)
        at = caught.tell()  # (the two calls above grew the scratch: their lines are left out)
        for _ in range(reps * rounds):
            call()
        caught.seek(at)
        for text_line in caught.read().decode().splitlines():
            us = {key: int(v) for key, v in re.findall(r"(\w+) (\d+) us", text_line)}
            if us:
                print(json.dumps({"what": "device path per-pass wall time, the stream waited for after each pass (HPK_HENC_TIMING)",
                                  "encoders": k, "blocks": n, "sha256": digest[:16], "us": us}), flush=True)
        return
    for r in range(rounds):
        line = {"what": "hpk_henc_encode_blocks", "setting": setting, "encoders": k, "blocks": n, "headers": int(hoff32[-1]),
                "fields_bytes": int(fields.size), "block_bytes": nbytes, "sha256": digest[:16], "round": r, "reps": reps}
        line.update(stats([call()[0] for _ in range(reps)]))
        line["lib"] = os.path.basename(os.environ.get("HPK_LIB", "libhpk.so"))
        print(json.dumps(line), flush=True)


def alone(k, scale, reps, rounds):
    import torch

    from loona_amd import batch

    n, text, off32, hoff32 = corpus(scale)
    stext, _ = batch.static_table()
    nh = int(hoff32[-1])
    head = stext + text
    head += bytes(-len(head) % 4)
    arena0 = torch.from_numpy(np.frombuffer(head + bytes(4 * nh), np.uint8).copy()).cuda()
    L = _lib.lib()
    g = [ctypes.c_uint32() for _ in range(4)]
    L.hpk_test_blkplan_geometry(*[ctypes.byref(x) for x in g])
    ring = g[0].value
    codec = HuffmanCodec(0, stream=torch.cuda.current_stream())
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()  # noqa: E731

    def run(lists_of, label):
        ne = len(lists_of)
        eoff = np.concatenate([[0], np.cumsum([len(x) for x in lists_of])]).astype(np.uint32)
        eblk = np.concatenate(lists_of).astype(np.uint32)
        tabs0 = np.zeros(ne, batch.DTAB_DTYPE)
        tabs0["ent"], tabs0["cap"], tabs0["max_size"] = np.arange(ne) * 128, 128, 4096
        d = dict(foff=i32(off32), hoff=i32(hoff32), eoff=i32(eoff), eblk=i32(eblk), flags=torch.ones(ne, dtype=torch.uint8, device="cuda"),
                 ent=torch.zeros(16 * 128 * ne, dtype=torch.uint8, device="cuda"))
        outs = None
        heads = [int((hoff32[x + 1].astype(np.int64) - hoff32[x]).sum()) for x in lists_of]
        for r in range(rounds):
            ts = []
            for _ in range(reps):
                arena = arena0.clone()
                tabs = torch.from_numpy(tabs0.view(np.uint8).copy()).cuda()
                d["ent"].zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs = codec.plan_blocks(arena, 0, len(stext), len(head), d["foff"], d["hoff"], d["eoff"], d["eblk"], d["flags"], tabs,
                                         d["ent"], *(outs or ()), sync=True)
                ts.append(time.perf_counter() - t0)
                assert (tabs.cpu().numpy().view(batch.DTAB_DTYPE)["applied"] == np.diff(eoff)).all()
            line = {"what": "hpk_plan_blocks alone", "which": label, "encoders": ne, "blocks": int(eoff[-1]), "headers_of_call": nh,
                    "headers_listed": int(sum(heads)), "longest_encoder_headers": int(max(heads)), "ring": ring, "round": r, "reps": reps}
            line.update(stats(ts))
            print(json.dumps(line), flush=True)
        return heads

    lists_of = [np.arange(e, n, k) for e in range(k)]
    heads = run(lists_of, "all encoders")
    run([lists_of[int(np.argmax(heads))]], "the longest encoder only")


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "host"
    k, scale, reps, rounds = (int(sys.argv[i]) if len(sys.argv) > i else v for i, v in ((2, 64), (3, 4), (4, 5), (5, 5)))
    if what == "alone":
        alone(k, scale, reps, rounds)
    else:
        encode(what, k, scale, reps, rounds)


if __name__ == "__main__":
    main()
