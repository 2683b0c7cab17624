#!/usr/bin/env python3
"""Device time of the packed encode against the two-step way to the same result, on one synthetic workload
(device-generated strings): `python scripts/enc_packed_time.py config3 [reps] [rounds]`.

Legs, timed in alternating rounds with events on one stream, `reps` calls each, one JSON line per round:
  A  encode_device into bound-sized regions, then pack (what a caller had before the packed form);
  B  encode_packed (skipped when the library has no hpk_encode_batch_packed: an older build under HPK_LIB);
  C  the region encode_device alone.
Every leg's result is checked once against the workload's own encoding before anything is timed."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from loona_amd import HuffmanCodec, _lib, synth  # noqa: E402
from loona_amd.batch import encode_offsets_torch  # noqa: E402


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
    eoff = encode_offsets_torch(doff)
    region = torch.empty(int(eoff[-1].item()) + 16, dtype=torch.uint8, device="cuda")
    ol = torch.empty(n, dtype=torch.int32, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    packed = torch.empty(w.enc_bytes + 16, dtype=torch.uint8, device="cuda")
    poff = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    has_b = hasattr(_lib.lib(), "hpk_encode_batch_packed")
    want_off = w.enc_off.to(torch.int64)

    def leg_c():
        codec.encode_into(w.dec_blob, doff, region, eoff, ol, st, device=True)

    def leg_a():
        leg_c()
        codec.pack(region, eoff, ol, dst_blob=packed, dst_off=poff)

    def leg_b():
        codec.encode_packed(w.dec_blob, doff, out_blob=packed, out_off=poff, out_len=ol, status=st)

    def verify(leg):
        packed.zero_()
        leg()
        torch.cuda.synchronize()
        assert not st.any().item()
        assert torch.equal(poff.to(torch.int64) & 0xFFFFFFFF, want_off), "offsets"
        assert torch.equal(packed[: w.enc_bytes], w.enc_blob[: w.enc_bytes]), "bytes"

    verify(leg_a)
    if has_b:
        verify(leg_b)
    for r in range(rounds):
        line = {"workload": wl, "literals": n, "decoded_bytes": w.dec_bytes, "encoded_bytes": w.enc_bytes, "round": r,
                "reps": reps, "A_region_then_pack_us": timed(leg_a, reps)}
        if has_b:
            line["B_encode_packed_us"] = timed(leg_b, reps)
        line["C_region_encode_us"] = timed(leg_c, reps)
        line["results_checked"] = True
        line["lib"] = os.path.basename(os.environ.get("HPK_LIB", "libhpk.so"))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
