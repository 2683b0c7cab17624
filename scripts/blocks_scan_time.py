#!/usr/bin/env python3
"""Config 4's corpus (bench.py's run_config4: the interop stories' header blocks replicated to >= 1M Huffman
literals, one hpk_hdec per connection) through ONE hpk_hdec_decode_blocks call on the host-scan path and on the
device-scan path (hpk_ctx_set_block_scan), alternating in the same process: three warm-up calls per leg, then
`calls` calls per leg, wall clock, with the per-pass split each call prints under HPK_HDEC_TIMING. Then
hpk_scan_blocks alone on the same blocks, device-resident, by events on one stream. One JSON line.
  usage: blocks_scan_time.py [calls=5]"""
import ctypes
import gzip
import json
import os
import re
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HOST_RE = re.compile(r"(\d+) threads, scan (\d+) us, batch issue (\d+) us, apply (\d+) us, join (\d+) us")
DEV_RE = re.compile(r"(\d+) threads, device scan (\d+) us, strings (\d+) us, bytes back (\d+) us, apply (\d+) us, join (\d+) us")


def child(calls):
    sys.path.insert(0, REPO)
    import numpy as np
    import torch

    from loona_amd import HuffmanCodec, _lib

    gold = os.path.join(REPO, "tests", "golden")
    with gzip.open(os.path.join(gold, "interop.json.gz"), "rt") as f:
        inter = json.load(f)
    with open(os.path.join(gold, "interop_digest.json")) as f:
        dig = json.load(f)
    stories = [[bytes.fromhex(c["wire"]) for c in st["cases"]] for enc in sorted(inter) for st in inter[enc]]
    reps = -(-1_000_000 // dig["huffman_literals"])
    L = _lib.lib()
    blocks, owners = [], []
    for r in range(reps):
        for si, st in enumerate(stories):
            for b in st:
                blocks.append(b)
                owners.append(r * len(stories) + si)
    nconn = reps * len(stories)
    off = np.zeros(len(blocks) + 1, np.int64)
    np.cumsum([len(b) for b in blocks], out=off[1:])
    blob = np.frombuffer(b"".join(blocks), np.uint8).copy()
    off32 = off.astype(np.uint32)
    codec = HuffmanCodec(0)

    def call(kind):
        codec.set_block_scan(kind)
        decs = [L.hpk_hdec_create() for _ in range(nconn)]
        arr = (ctypes.c_void_p * len(blocks))(*[decs[o] for o in owners])
        out = _lib.BlocksOut()
        sys.stderr.write(f"leg {kind}\n")
        sys.stderr.flush()
        t0 = time.perf_counter()
        rc = L.hpk_hdec_decode_blocks(codec._h, arr, blob.ctypes.data, off32.ctypes.data, len(blocks), ctypes.byref(out))
        dt = time.perf_counter() - t0
        _lib.check(rc, "hpk_hdec_decode_blocks")
        errs = sum(1 for b in range(len(blocks)) if out.blocks[b].error)
        res = (dt, errs, out.n_headers, out.arena_len)
        L.hpk_blocks_out_free(ctypes.byref(out))
        for d in decs:
            L.hpk_hdec_destroy(d)
        return res

    legs = ("host", "device")
    for _ in range(3):
        for kind in legs:
            call(kind)
    sys.stderr.write("timed\n")
    times = {k: [] for k in legs}
    same = {}
    for _ in range(calls):
        for kind in legs:
            dt, *rest = call(kind)
            times[kind].append(dt)
            same[kind] = rest
    assert same["host"] == same["device"], same
    codec.set_block_scan("host")
    # the scan alone, device-resident
    db = torch.from_numpy(blob).cuda()
    do = torch.from_numpy(off32.view(np.int32)).cuda()
    codec.set_stream(torch.cuda.current_stream())
    outs = codec.scan_blocks(db, do, sync=True)
    nf, ns = int(outs[1][-1].item()), int(outs[4][-1].item())
    kw = dict(fields=outs[0], field_off=outs[1], str_off=outs[2], str_end=outs[3], str_blk_off=outs[4], status=outs[5])
    ev = []
    for _ in range(3 + 10):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        codec.scan_blocks(db, do, **kw)
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    scan_us = [a.elapsed_time(b) * 1e3 for a, b in ev[3:]]
    print(json.dumps({
        "lib": os.path.basename(os.environ.get("HPK_LIB", "libhpk.so")), "version": L.hpk_version().decode()[:8],
        "header_blocks": len(blocks), "block_bytes": int(blob.size), "connections": nconn, "fields": nf, "strings": ns,
        "headers": same["host"][1], "block_errors": same["host"][0],
        "host_scan_ms": round(statistics.median(times["host"]) * 1e3, 2),
        "device_scan_ms": round(statistics.median(times["device"]) * 1e3, 2),
        "device_over_host": round(statistics.median(times["host"]) / statistics.median(times["device"]), 3),
        "calls_ms": {k: [round(x * 1e3, 2) for x in v] for k, v in times.items()},
        "scan_blocks_alone_us": {"median": round(statistics.median(scan_us), 1), "min": round(min(scan_us), 1),
                                 "max": round(max(scan_us), 1), "calls": len(scan_us)},
        "scan_blocks_alone_gb_per_s": round(blob.size / statistics.median(scan_us) / 1e3, 2)}))


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    if os.environ.get("_BST_CHILD"):
        return child(calls)
    env = dict(os.environ, _BST_CHILD="1", HPK_HDEC_TIMING="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(calls)], env=env, capture_output=True, text=True,
                       timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-3000:])
        raise SystemExit(p.returncode)
    line = json.loads(p.stdout.strip().splitlines()[-1])
    err = p.stderr[p.stderr.index("timed\n"):]
    host = [[int(x) for x in m.groups()] for m in HOST_RE.finditer(err)]
    dev = [[int(x) for x in m.groups()] for m in DEV_RE.finditer(err)]
    med = lambda rows, names: dict(zip(names, [statistics.median(r[i] for r in rows) for i in range(len(names))]))  # noqa: E731
    line["pass_median_us"] = {
        "host": med(host, ("threads", "scan", "batch_issue", "apply", "join")) if host else None,
        "device": med(dev, ("threads", "upload_count_scans_totals", "emit_strings_arrays_back", "bytes_back", "apply", "join"))
        if dev else None}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
