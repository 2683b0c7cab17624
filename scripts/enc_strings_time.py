#!/usr/bin/env python3
"""Device time of the packed string-literal encode next to the packed encode, on one synthetic workload
(device-generated strings): `python scripts/enc_strings_time.py config3 [reps] [rounds]`.

Legs, timed in alternating rounds with events on one stream, `reps` calls each, one JSON line per round:
  a  encode_packed (the Huffman bytes alone: what this call adds to);
  b  encode_strings under HPK_STR_AUTO (prefix, H bit, Huffman where strictly shorter);
  c  encode_strings under HPK_STR_RAW (every literal raw behind its prefix);
  d  a device copy of as many bytes as (c) writes: (c)'s ceiling.
(b)'s result is checked once before anything is timed: its offsets are the exclusive sum of its lengths, every
literal the workload's own encoding Huffman-codes shorter carries the H bit, and the Huffman payloads of the
first literals equal the workload's encoding."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from loona_amd import HuffmanCodec, synth  # noqa: E402


def timed(fn, reps):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / reps, 1)


def main():
    wl = sys.argv[1] if len(sys.argv) > 1 else "config3"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    codec = HuffmanCodec(0)
    w = {"config2": synth.device_config2, "config3": synth.device_config3}[wl](codec)
    n = w.n
    doff = w.dec_off.to(torch.int32)
    cap = max(w.enc_bytes, w.dec_bytes) + 6 * n + 16
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    src = torch.empty(cap, dtype=torch.uint8, device="cuda")
    ol = torch.empty(n, dtype=torch.int32, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    ooff = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    raw = torch.ones(n, dtype=torch.uint8, device="cuda")

    def leg_a():
        codec.encode_packed(w.dec_blob, doff, out_blob=out, out_off=ooff, out_len=ol, status=st)

    def leg_b():
        codec.encode_strings(w.dec_blob, doff, None, out_blob=out, out_off=ooff, out_len=ol, status=st)

    def leg_c():
        codec.encode_strings(w.dec_blob, doff, raw, out_blob=out, out_off=ooff, out_len=ol, status=st)

    leg_c()
    torch.cuda.synchronize()
    raw_total = int(ooff[n].item()) & 0xFFFFFFFF

    def leg_d():
        out[:raw_total].copy_(src[:raw_total])

    # (b) against the workload's own encoding
    leg_b()
    torch.cuda.synchronize()
    assert not st.any().item()
    o = ooff.to(torch.int64) & 0xFFFFFFFF
    ln = ol.to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(o[1:] - o[:-1], ln) and int(o[0].item()) == 0, "offsets"
    auto_total = int(o[n].item())
    dl = (w.dec_off[1:] - w.dec_off[:-1]).to(torch.int64)
    el = (w.enc_off[1:] - w.enc_off[:-1]).to(torch.int64)
    hbit = (out[o[:-1].clamp(max=cap - 1)] & 0x80) != 0
    assert torch.equal(hbit, (el < dl) & (dl > 0)), "the H bit is set exactly where the Huffman form is shorter"
    for i in range(min(n, 200)):
        if bool(hbit[i].item()):
            p = int(el[i].item())
            k = 1 if p < 127 else 2 if p - 127 < 128 else 3
            a, b = int(o[i].item()) + k, int(w.enc_off[i].item())
            assert torch.equal(out[a : a + p], w.enc_blob[b : b + p]), f"payload of literal {i}"
    for r in range(rounds):
        line = {"workload": wl, "literals": n, "decoded_bytes": w.dec_bytes, "encoded_bytes": w.enc_bytes,
                "auto_bytes": auto_total, "raw_bytes": raw_total, "round": r, "reps": reps,
                "a_encode_packed_us": timed(leg_a, reps), "b_strings_auto_us": timed(leg_b, reps),
                "c_strings_raw_us": timed(leg_c, reps), "d_copy_us": timed(leg_d, reps), "results_checked": True,
                "lib": os.path.basename(os.environ.get("HPK_LIB", "libhpk.so"))}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
