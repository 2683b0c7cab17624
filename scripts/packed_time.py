#!/usr/bin/env python3
"""Device time of the output forms of one synthetic workload (device-generated, device-resident), the
legs alternating in one process after warm-up: `python scripts/packed_time.py config5 [reps] [rounds]`.
  (a) region decode (hpk_decode_batch)
  (b) hpk_decode_batch_compact
  (c) hpk_decode_batch_compact followed by the torch shard.compact: the decoded bytes end to end, in
      literal order, by the only means there was before the packed form
  (d) hpk_decode_batch_packed: the same bytes from one call
  (e) hpk_pack_batch alone on (a)'s output
Each round times every leg once (`reps` calls between two events); per leg the rounds' least, median and
greatest. (d)'s result is checked once against (c)'s, and its out_off[n] against the sum of out_len. One
JSON line."""
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from loona_amd import HuffmanCodec, _lib, shard, synth  # noqa: E402
from loona_amd.batch import compact_capacity, decode_offsets_torch  # noqa: E402


def main():
    wl = sys.argv[1] if len(sys.argv) > 1 else "config5"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    codec = HuffmanCodec(0)
    gens = {"config3": synth.device_config3, "config5": lambda c: synth.device_config5_shard(c, 0)}
    w = gens[wl](codec)
    n, dev = w.n, "cuda"
    L = _lib.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    fl = _lib.HPK_PTR_DEVICE | _lib.HPK_ASYNC

    # (a) region form
    doff = decode_offsets_torch(w.enc_off)
    out_a = torch.empty(int(doff[-1].item()) + 16, dtype=torch.uint8, device=dev)
    ol = torch.empty(n, dtype=torch.int32, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    codec.decode_into(w.enc_blob, w.enc_off, out_a, doff, ol, st, device=True)  # binds the stream, checks args
    torch.cuda.synchronize()
    synth.check_decoded(w, out_a, doff, ol, st)
    total = int(ol.to(torch.int64).sum().item())
    # (b) compacted form
    out_b = torch.empty(compact_capacity(w.enc_blob.numel(), n), dtype=torch.uint8, device=dev)
    off_b = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ol_b, st_b = torch.empty_like(ol), torch.empty_like(st)
    # (d) packed form
    out_d = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    off_d = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ol_d, st_d = torch.empty_like(ol), torch.empty_like(st)
    # (e) the pack alone
    out_e = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    off_e = torch.empty(n + 1, dtype=torch.int32, device=dev)

    def batch_args(out, off, ln, stt):
        return (codec._h, vp(w.enc_blob), w.enc_blob.numel(), vp(w.enc_off), ctypes.c_uint32(n), vp(out), out.numel(),
                vp(off), vp(ln), vp(stt), fl)

    args_a, args_b, args_d = batch_args(out_a, doff, ol, st), batch_args(out_b, off_b, ol_b, st_b), batch_args(out_d, off_d, ol_d, st_d)
    args_e = (codec._h, vp(out_a), out_a.numel(), vp(doff), vp(ol), ctypes.c_uint32(n), vp(out_e), out_e.numel(), vp(off_e), fl)

    def leg_c():
        assert L.hpk_decode_batch_compact(*args_b) == 0
        return shard.compact(out_b, off_b, ol_b, n, total)

    legs = {
        "a_region": lambda: L.hpk_decode_batch(*args_a),
        "b_compact": lambda: L.hpk_decode_batch_compact(*args_b),
        "c_compact_torch_gather": leg_c,
        "d_packed": lambda: L.hpk_decode_batch_packed(*args_d),
        "e_pack_alone": lambda: L.hpk_pack_batch(*args_e),
    }
    # once, checked: (d) == (c) == (e), out_off[n] == the sum of out_len
    ref = leg_c()
    for k in ("d_packed", "e_pack_alone"):
        assert legs[k]() == 0, _lib.last_error()
    torch.cuda.synchronize()
    codec.check()
    total_d = int(off_d[n].item()) & 0xFFFFFFFF
    ok = (total_d == total and int(ol_d.to(torch.int64).sum().item()) == total and torch.equal(out_d[:total], ref)
          and torch.equal(out_e[:total], ref) and torch.equal(off_d, off_e) and torch.equal(ol_d, ol) and torch.equal(st_d, st))
    del ref
    s = torch.cuda.current_stream()
    for _ in range(int(os.environ.get("HPK_WARM", "3"))):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(reps):
                f()
            e1.record(s)
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    res = {k: {"min_us": round(min(v), 1), "median_us": round(statistics.median(v), 1), "max_us": round(max(v), 1)}
           for k, v in times.items()}
    # (e)'s algorithmic traffic: the decoded bytes read and written, 12 bytes of offsets per literal
    traffic = 2 * total + 12 * n
    e_us = res["e_pack_alone"]["median_us"]
    print(json.dumps({"workload": wl, "literals": n, "encoded_bytes": w.enc_bytes, "decoded_bytes": total,
                      "packed_out_off_n": total_d, "checked": bool(ok), "reps": reps, "rounds": rounds, "legs": res,
                      "pack_traffic_bytes": traffic, "pack_TB_s": round(traffic / e_us / 1e6, 3),
                      "d_over_c": round(res["d_packed"]["median_us"] / res["c_compact_torch_gather"]["median_us"], 4),
                      "src_sha16": __import__("bench").source_hash()}), flush=True)
    assert ok, "the packed result differs"


if __name__ == "__main__":
    main()
