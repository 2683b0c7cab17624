#!/usr/bin/env python3
"""The interop corpus' header blocks (tests/frames_write_cases.interop_blocks, repeated to tens of MB) measured two
ways, in one process:
  * device-resident, by events on one stream (10 calls after 3, the legs alternating), at each frame size M of 16384
    (one frame a block: the real case), 1024 and 16 (header density): hpk_write_frames; hpk_pack_batch moving the same
    blocks' windows (the same bytes without headers); a device-to-device copy of the wire total;
  * ONE hpk_h2_write_headers call over the corpus' header lists (`hreps` times, an encoder per story and repetition)
    with the default host framing and with HPK_FRAME_WRITE_DEVICE on the same context, alternating, fresh encoders per
    call: one warm-up round, then `rounds` rounds, wall clock.
One JSON line.
  usage: frames_write_time.py [rounds=5] [target_mb=32] [hreps=4]"""
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    target = (int(sys.argv[2]) if len(sys.argv) > 2 else 32) << 20
    hreps = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import numpy as np
    import torch

    import frames_write_cases as wc
    from hpk_util import load
    from loona_amd import HuffmanCodec, _lib

    L = _lib.lib()
    codec = HuffmanCodec(0, stream=torch.cuda.current_stream())
    blocks = wc.interop_blocks()
    once = sum(len(b) for b in blocks)
    reps = max(1, target // once)
    lens = np.array([len(b) for b in blocks] * reps, np.int64)
    n = len(lens)
    blob = np.frombuffer(b"".join(blocks) * reps, np.uint8)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    db = torch.from_numpy(blob.copy()).cuda()
    doff = torch.from_numpy(off.astype(np.uint32).view(np.int32)).cuda()
    dlen = torch.from_numpy(lens.astype(np.uint32).view(np.int32)).cuda()
    dsid = torch.from_numpy((2 * np.arange(n, dtype=np.int64) % 2**31 + 1).astype(np.uint32).view(np.int32)).cuda()
    rng = lambda v: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1), "calls": len(v)}  # noqa: E731
    cases = {}
    for m in (16384, 1024, 16):
        total = int((lens + 9 * np.maximum(-(-lens // m), 1)).sum())
        dmf = torch.full((n,), m, dtype=torch.int32, device="cuda")
        out = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
        woff = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        st = torch.empty(n, dtype=torch.uint8, device="cuda")
        pk = torch.empty(blob.size + 64, dtype=torch.uint8, device="cuda")
        pkoff = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        src = torch.empty(total, dtype=torch.uint8, device="cuda")
        dst = torch.empty(total, dtype=torch.uint8, device="cuda")
        ev = []
        for _ in range(3 + 10):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            codec.write_frames(db, doff, dsid, dmf, out_blob=out, wire_off=woff, status=st)
            e[1].record()
            codec.pack(db, doff[:n], dlen, dst_blob=pk, dst_off=pkoff)
            e[2].record()
            dst.copy_(src)
            e[3].record()
            ev.append(e)
        torch.cuda.synchronize()
        codec.check()
        assert int(woff[n].item()) & 0xFFFFFFFF == total and not bool(st.any().item())
        w = [e[0].elapsed_time(e[1]) * 1e3 for e in ev[3:]]
        p = [e[1].elapsed_time(e[2]) * 1e3 for e in ev[3:]]
        c = [e[2].elapsed_time(e[3]) * 1e3 for e in ev[3:]]
        cases[str(m)] = {"wire_bytes": total, "frames": int(np.maximum(-(-lens // m), 1).sum()), "write_frames_us": rng(w),
                         "pack_us": rng(p), "copy_us": rng(c), "write_over_pack": round(statistics.median(w) / statistics.median(p), 3),
                         "write_over_copy": round(statistics.median(w) / statistics.median(c), 3),
                         "write_gb_per_s": round(total / statistics.median(w) / 1e3, 1)}
    # one hpk_h2_write_headers call on both framing paths
    inter = load("interop.json.gz")
    stories = [[[(a.encode(), v.encode()) for a, v in c["headers"]] for c in story["cases"]] for enc in sorted(inter) for story in inter[enc]]
    stories = stories * hreps
    parts, foff, hoff, which = [], [0], [0], []
    for k, s in enumerate(stories):
        for hl in s:
            for name, value in hl:
                for x in (name, value):
                    parts.append(x)
                    foff.append(foff[-1] + len(x))
            hoff.append(hoff[-1] + len(hl))
            which.append(k)
    fields = np.frombuffer(b"".join(parts), np.uint8).copy()
    foff32, hoff32 = np.asarray(foff, np.uint32), np.asarray(hoff, np.uint32)
    nb = len(which)
    sid = (2 * np.arange(nb, dtype=np.int64) % 2**31 + 1).astype(np.uint32)
    mf = np.full(nb, 16384, np.uint32)

    def call(kind):
        codec.set_frame_write(kind)
        encs = [L.hpk_henc_create(1) for _ in stories]
        arr = (ctypes.c_void_p * nb)(*[encs[k] for k in which])
        out = _lib.HencOut()
        before = L.hpk_test_frame_write_calls(codec._h)
        t0 = time.perf_counter()
        rc = L.hpk_h2_write_headers(codec._h, arr, fields.ctypes.data, foff32.ctypes.data, hoff32.ctypes.data, nb, sid.ctypes.data,
                                    mf.ctypes.data, ctypes.byref(out))
        dt = time.perf_counter() - t0
        _lib.check(rc, "hpk_h2_write_headers")
        assert L.hpk_test_frame_write_calls(codec._h) - before == (kind == "device")
        res = (int(out.len), ctypes.string_at(out.bytes, min(out.len, 4096)))
        L.hpk_henc_out_free(ctypes.byref(out))
        for e in encs:
            L.hpk_henc_destroy(e)
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
    assert same["host"] == same["device"]
    codec.set_frame_write("host")
    ms = lambda v: {"median": round(statistics.median(v) * 1e3, 2), "min": round(min(v) * 1e3, 2), "max": round(max(v) * 1e3, 2)}  # noqa: E731
    print(json.dumps({
        "lib": os.path.basename(os.environ.get("HPK_LIB", "libhpk.so")), "version": L.hpk_version().decode()[:8],
        "blocks": n, "block_bytes": int(blob.size), "by_max_frame": cases,
        "write_headers": {"blocks": nb, "encoders": len(stories), "field_bytes": int(fields.size), "wire_bytes": same["host"][0],
                          "host_ms": ms(times["host"]), "device_ms": ms(times["device"]),
                          "host_over_device": round(statistics.median(times["host"]) / statistics.median(times["device"]), 3),
                          "rounds_ms": {k: [round(x * 1e3, 2) for x in v] for k, v in times.items()}}}))


if __name__ == "__main__":
    main()
