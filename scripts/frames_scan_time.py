#!/usr/bin/env python3
"""The interop connections' wires (tests/h2_cases.interop_connections: every interop story as HEADERS + CONTINUATION
frames on a connection of its own, replicated `reps` times) measured two ways, in one process:
  * hpk_scan_frames + hpk_frame_blocks on the wires device-resident, by events on one stream (10 calls after 3);
  * ONE hpk_h2_read_frames call over all connections with the default framing and with the opt-in device framing
    (hpk_ctx_set_frame_scan), alternating, fresh connections per call: one warm-up round, then `rounds` rounds, wall
    clock, ranges reported.
One JSON line.
  usage: frames_scan_time.py [rounds=5] [reps=8]"""
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import numpy as np
    import torch

    import h2_cases
    from loona_amd import HuffmanCodec, _lib, batch

    wires, _ = h2_cases.interop_connections(0)
    wires = wires * reps
    nconn = len(wires)
    off = np.zeros(nconn + 1, np.int64)
    np.cumsum([len(w) for w in wires], out=off[1:])
    blob = np.frombuffer(b"".join(wires), np.uint8).copy()
    off32 = off.astype(np.uint32)
    L = _lib.lib()
    codec = HuffmanCodec(0)

    def frames_of(w):  # the frames of a wire: the walk's serial steps
        k, pos = 0, 0
        while len(w) - pos >= 9:
            pos += 9 + int.from_bytes(w[pos : pos + 3], "big")
            k += 1
        return k

    most_frames = max(frames_of(w) for w in wires[: nconn // reps])

    def call(kind):
        codec.set_frame_scan(kind)
        conns = [L.hpk_h2conn_create() for _ in range(nconn)]
        arr = (ctypes.c_void_p * nconn)(*conns)
        out = _lib.H2Out()
        t0 = time.perf_counter()
        rc = L.hpk_h2_read_frames(codec._h, arr, blob.ctypes.data, off32.ctypes.data, nconn, ctypes.byref(out))
        dt = time.perf_counter() - t0
        _lib.check(rc, "hpk_h2_read_frames")
        res = (out.hb.n_blocks, out.hb.n_headers, out.hb.arena_len, sum(out.conn_consumed[c] for c in range(nconn)),
               sum(1 for c in range(nconn) if out.conn_error[c]))
        L.hpk_h2_out_free(ctypes.byref(out))
        for c in conns:
            L.hpk_h2conn_destroy(c)
        return dt, res

    legs = ("host", "device")
    for kind in legs:
        call(kind)
    times = {k: [] for k in legs}
    same = {}
    for _ in range(rounds):
        for kind in legs:
            dt, res = call(kind)
            times[kind].append(dt)
            same[kind] = res
    assert same["host"] == same["device"], same
    codec.set_frame_scan("host")
    # the two device calls alone, device-resident
    codec.set_stream(torch.cuda.current_stream())
    db = torch.from_numpy(blob).cuda()
    do = torch.from_numpy(off32.view(np.int32)).cuda()
    st = np.zeros(nconn, batch.FCONN_DTYPE)
    st["max_frame_size"] = 16384
    fresh = torch.from_numpy(st.view(np.uint8).reshape(-1)).cuda()
    dconns = fresh.clone()
    outs = codec.scan_frames(db, do, dconns, sync=True)
    nb, nf = int(outs[1][-1].item()), int(outs[4][-1].item())
    kw = dict(blocks=outs[0], conn_blk_off=outs[1], frag_off=outs[2], frag_len=outs[3], conn_frag_off=outs[4], open_off=outs[5],
              open_len=outs[6], conn_open_off=outs[7])
    blk = torch.empty(blob.size, dtype=torch.uint8, device="cuda")
    boff = torch.empty(nb + 1, dtype=torch.int32, device="cuda")
    ev = []
    for _ in range(3 + 10):
        dconns.copy_(fresh)
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        a.record()
        codec.scan_frames(db, do, dconns, **kw)
        b.record()
        codec.frame_blocks(db, outs[2][:nf], outs[3][:nf], outs[0], nblocks=nb, out_blob=blk, block_off=boff)
        c.record()
        ev.append((a, b, c))
    torch.cuda.synchronize()
    codec.check()
    scan_us = [a.elapsed_time(b) * 1e3 for a, b, _ in ev[3:]]
    gather_us = [b.elapsed_time(c) * 1e3 for _, b, c in ev[3:]]
    rng = lambda v: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1), "calls": len(v)}  # noqa: E731
    ms = lambda v: {"median": round(statistics.median(v) * 1e3, 2), "min": round(min(v) * 1e3, 2), "max": round(max(v) * 1e3, 2)}  # noqa: E731
    print(json.dumps({
        "lib": os.path.basename(os.environ.get("HPK_LIB", "libhpk.so")), "version": L.hpk_version().decode()[:8],
        "connections": nconn, "wire_bytes": int(blob.size), "longest_connection_bytes": max(len(w) for w in wires),
        "most_frames_in_a_connection": most_frames,
        "header_blocks": nb, "fragments": nf, "block_bytes": int(boff[-1].item()), "headers": same["host"][1],
        "scan_frames_us": rng(scan_us), "frame_blocks_us": rng(gather_us),
        "scan_frames_gb_per_s": round(blob.size / statistics.median(scan_us) / 1e3, 2),
        "scan_frames_us_per_frame_of_the_longest": round(statistics.median(scan_us) / most_frames, 3),
        "read_frames_host_ms": ms(times["host"]), "read_frames_device_ms": ms(times["device"]),
        "device_over_host": round(statistics.median(times["host"]) / statistics.median(times["device"]), 3),
        "rounds_ms": {k: [round(x * 1e3, 2) for x in v] for k, v in times.items()}}))


if __name__ == "__main__":
    main()
