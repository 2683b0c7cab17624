#!/usr/bin/env python3
"""Config 4's corpus (bench.py's run_config4: the interop stories' header blocks replicated to >= 1M Huffman
literals, one hpk_hdec per connection) through ONE hpk_hdec_decode_blocks call under each of the three settings:
the host scan, the device scan (hpk_ctx_set_block_scan) and the device apply (hpk_ctx_set_block_apply). The legs
alternate in the same process: three warm-up calls per leg, then `calls` calls per leg, wall clock, with the
per-pass split each call prints under HPK_HDEC_TIMING. Then hpk_apply_blocks alone on the same blocks, every input
device-resident (scan_blocks' and decode_strings' outputs, fresh tables before every call), by events on one
stream. The whole measurement runs in `procs` processes, one after the other; each appends one JSON line to
profiles/blocks_apply/blocks_apply_time.jsonl and prints it.
HPK_LIB selects another build of the library for the host-scan and device-scan legs (one without the apply has no
third leg).
  usage: blocks_apply_time.py [calls=5] [procs=2]"""
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
OUT = os.path.join(REPO, "profiles", "blocks_apply", "blocks_apply_time.jsonl")

HOST_RE = re.compile(r"(\d+) threads, scan (\d+) us, batch issue (\d+) us, apply (\d+) us, join (\d+) us")
DEV_RE = re.compile(r"(\d+) threads, device scan (\d+) us, strings (\d+) us, bytes back (\d+) us, apply (\d+) us, join (\d+) us")
APP_RE = re.compile(r"device apply, (\d+) decoders, tables out (\d+) us, device scan (\d+) us, strings (\d+) us, "
                    r"apply and results back (\d+) us, outputs and tables in (\d+) us")


def child(calls):
    sys.path.insert(0, REPO)
    import numpy as np
    import torch

    from loona_amd import HuffmanCodec, _lib, batch

    gold = os.path.join(REPO, "tests", "golden")
    with gzip.open(os.path.join(gold, "interop.json.gz"), "rt") as f:
        inter = json.load(f)
    with open(os.path.join(gold, "interop_digest.json")) as f:
        dig = json.load(f)
    stories = [[bytes.fromhex(c["wire"]) for c in st["cases"]] for enc in sorted(inter) for st in inter[enc]]
    reps = -(-1_000_000 // dig["huffman_literals"])
    L = _lib.lib()
    has_apply = hasattr(L, "hpk_apply_blocks")
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
        codec.set_block_scan("device" if kind == "device_scan" else "host")
        if has_apply:
            codec.set_block_apply("device" if kind == "device_apply" else "host")
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
        emitted = sum(out.blocks[b].n_headers for b in range(len(blocks)))
        sizes = []
        a, n, m = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        for d in decs[:: max(1, nconn // 64)]:
            L.hpk_hdec_table_size(d, ctypes.byref(a), ctypes.byref(n), ctypes.byref(m))
            sizes.append((a.value, n.value, m.value))
        res = (dt, errs, emitted, sizes)
        L.hpk_blocks_out_free(ctypes.byref(out))
        for d in decs:
            L.hpk_hdec_destroy(d)
        return res

    legs = ("host_scan", "device_scan") + (("device_apply",) if has_apply else ())
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
    assert all(same[k] == same["host_scan"] for k in legs), "the settings disagree"
    med = {k: statistics.median(v) for k, v in times.items()}
    line = {
        "lib": os.path.basename(os.environ.get("HPK_LIB", "libhpk.so")), "version": L.hpk_version().decode()[:8],
        "header_blocks": len(blocks), "block_bytes": int(blob.size), "connections": nconn,
        "headers": same["host_scan"][1], "block_errors": same["host_scan"][0],
        "call_ms": {k: round(v * 1e3, 2) for k, v in med.items()},
        "calls_ms": {k: [round(x * 1e3, 2) for x in v] for k, v in times.items()}}
    if has_apply:
        line["device_scan_over_device_apply"] = round(med["device_scan"] / med["device_apply"], 3)
        line["host_scan_over_device_apply"] = round(med["host_scan"] / med["device_apply"], 3)
        # the apply alone, device-resident: the scan's and the string decode's outputs as they stand, empty tables
        codec.set_block_scan("host")
        codec.set_block_apply("host")
        codec.set_stream(torch.cuda.current_stream())
        ring, chunk, wgd = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        L.hpk_test_blkapply_geometry(ctypes.byref(ring), ctypes.byref(chunk), ctypes.byref(wgd))
        db = torch.from_numpy(blob).cuda()
        do = torch.from_numpy(off32.view(np.int32)).cuda()
        fields, foff, so, se, sbo, _ = codec.scan_blocks(db, do, sync=True)
        nf, ns = int(foff[-1].item()), int(sbo[-1].item())
        _, oo, ol, _, st = codec.decode_strings(db, so[:ns], se[:ns], sync=True)
        order = np.argsort(np.asarray(owners), kind="stable").astype(np.uint32)
        counts = np.bincount(np.asarray(owners), minlength=nconn)
        dbo = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32).view(np.int32)).cuda()
        dbl = torch.from_numpy(order.view(np.int32)).cuda()
        cap = 128
        tabs0 = np.zeros(nconn, dtype=batch.DTAB_DTYPE)
        tabs0["ent"] = np.arange(nconn, dtype=np.uint32) * cap
        tabs0["cap"], tabs0["max_size"], tabs0["max_allowed"] = cap, 4096, 0xFFFFFFFF
        t0 = torch.from_numpy(tabs0.view(np.uint8)).cuda()
        tabs = torch.empty_like(t0)
        ent = torch.zeros(16 * cap * nconn, dtype=torch.uint8, device="cuda")
        headers = torch.empty(16 * nf, dtype=torch.uint8, device="cuda")
        results = torch.empty(16 * len(blocks), dtype=torch.uint8, device="cuda")
        text, _ = batch.static_table()
        ev = []
        for _ in range(3 + 10):
            tabs.copy_(t0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            codec.apply_blocks(fields[: 16 * nf], foff, oo, ol, st, ns, len(text), 0, dbo, dbl, tabs, ent, headers=headers,
                               results=results)
            b.record()
            ev.append((a, b))
        torch.cuda.synchronize()
        codec.check()
        r = results.cpu().numpy().view(batch.RESULT_DTYPE)
        assert int(r["n_headers"].sum()) == same["host_scan"][1] and int((r["error"] != 0).sum()) == same["host_scan"][0]
        us = [a.elapsed_time(b) * 1e3 for a, b in ev[3:]]
        line.update({"fields": nf, "strings": ns, "ring_entries": ring.value,
                     "apply_blocks_alone_us": {"median": round(statistics.median(us), 1), "min": round(min(us), 1),
                                               "max": round(max(us), 1), "calls": len(us)},
                     "apply_blocks_alone_mfields_per_s": round(nf / statistics.median(us), 1)})
    print(json.dumps(line))


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    procs = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    if os.environ.get("_BAT_CHILD"):
        return child(calls)
    env = dict(os.environ, _BAT_CHILD="1", HPK_HDEC_TIMING="1")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    for k in range(procs):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), str(calls)], env=env, capture_output=True, text=True,
                           timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            raise SystemExit(p.returncode)
        line = json.loads(p.stdout.strip().splitlines()[-1])
        err = p.stderr[p.stderr.index("timed\n"):]

        def med(rx, names):
            rows = rx.findall(err)
            return dict(zip(names, [statistics.median(int(r[i]) for r in rows) for i in range(len(names))])) if rows else None

        line["process"] = k
        line["pass_median_us"] = {
            "host_scan": med(HOST_RE, ("threads", "scan", "batch_issue", "apply", "join")),
            "device_scan": med(DEV_RE, ("threads", "upload_count_scans_totals", "emit_strings_arrays_back", "bytes_back", "apply",
                                        "join")),
            "device_apply": med(APP_RE, ("decoders", "tables_out", "upload_count_scans_totals", "emit_strings",
                                         "apply_kernel_results_back", "outputs_and_tables_in"))}
        with open(OUT, "a") as f:
            f.write(json.dumps(line) + "\n")
        print(json.dumps(line))


if __name__ == "__main__":
    main()
