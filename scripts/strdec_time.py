#!/usr/bin/env python3
"""Device time of the packed string-literal decode next to the packed decode, on one synthetic workload
(device-generated strings, framed by encode_strings): `python scripts/strdec_time.py config3 [reps] [rounds] [legs]`
(legs: the letters of the legs to time, e.g. `a` alone under a kernel trace; default all).

Legs, timed in alternating rounds with events on one stream, `reps` calls each, one JSON line per round:
  a  decode_strings on the AUTO framing (prefix, H bit, Huffman where strictly shorter), mirror form;
  b  decode_packed on the same strings' gathered Huffman payloads: the floor, (a) does strictly more;
  c  decode_strings on an all-raw framing of the same bytes;
  d  decode_packed on the workload's own encoding (every literal Huffman-coded), and
  e  pack on that result's region layout: the two existing calls, for runs of two libraries on one box
     (HPK_LIB=<an older libhpk.so> runs d and e alone when the library has no string-literal decode).
(a)'s and (c)'s results are checked once before anything is timed: status all 0, out_off the exclusive sum of
out_len, consumed the encoder's out_len, and the bytes the workload's plaintext. Every line carries the sha256
of the library's sources (loona_amd/csrc, include/hpk.h) as the working tree has them."""
import glob
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from loona_amd import HuffmanCodec, _lib, synth  # noqa: E402


def source_hash():
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(REPO, "loona_amd", "csrc", "*.h")) + glob.glob(os.path.join(REPO, "loona_amd", "csrc", "*.hip")) +
                   glob.glob(os.path.join(REPO, "loona_amd", "csrc", "*.cpp")) + [os.path.join(REPO, "include", "hpk.h")])
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0" + open(f, "rb").read())
    return h.hexdigest()[:16]


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
    have = hasattr(_lib.lib(), "hpk_decode_strings_packed")
    w = {"config2": synth.device_config2, "config3": synth.device_config3}[wl](codec)
    n = w.n
    doff = w.dec_off.to(torch.int32)
    eoff = w.enc_off.to(torch.int32)
    cap = max(w.enc_bytes, w.dec_bytes) + 6 * n + 16
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    ol = torch.empty(n, dtype=torch.int32, device="cuda")
    co = torch.empty(n, dtype=torch.int32, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    ooff = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    line0 = {"workload": wl, "literals": n, "decoded_bytes": w.dec_bytes, "encoded_bytes": w.enc_bytes}
    legs = {}

    # d, e: the existing calls
    def leg_d():
        codec.decode_packed(w.enc_blob, eoff, out_blob=out, out_off=ooff, out_len=ol, status=st)

    rb, ro, rl, rs = codec.decode_device(w.enc_blob, eoff, sync=True)
    pdst = torch.empty(w.dec_bytes + 16, dtype=torch.uint8, device="cuda")
    poff = torch.empty(n + 1, dtype=torch.int32, device="cuda")

    def leg_e():
        codec.pack(rb, ro, rl[:n], dst_blob=pdst, dst_off=poff)

    legs["d_decode_packed_all_us"] = leg_d
    legs["e_pack_us"] = leg_e
    if have:
        auto = codec.encode_strings(w.dec_blob, doff, None, sync=True)
        rawp = torch.ones(n, dtype=torch.uint8, device="cuda")
        raw = codec.encode_strings(w.dec_blob, doff, rawp, sync=True)
        # the AUTO framing's Huffman payloads, gathered: the workload's own encoding where it is strictly shorter
        dl = (w.dec_off[1:] - w.dec_off[:-1]).to(torch.int64)
        el = (w.enc_off[1:] - w.enc_off[:-1]).to(torch.int64)
        hl = torch.where((el < dl) & (dl > 0), el, torch.zeros_like(el)).to(torch.int32)
        hblob, hoff = codec.pack(w.enc_blob, eoff, hl, sync=True)
        line0.update(auto_bytes=int(auto[0].numel()), raw_bytes=int(raw[0].numel()), huffman_payload_bytes=int(hblob.numel()),
                     huffman_strings=int((hl > 0).sum().item()))

        def leg_a():
            codec.decode_strings(auto[0], auto[1], out_blob=out, out_off=ooff, out_len=ol, consumed=co, status=st)

        def leg_b():
            codec.decode_packed(hblob, hoff, out_blob=out, out_off=ooff, out_len=ol, status=st)

        def leg_c():
            codec.decode_strings(raw[0], raw[1], out_blob=out, out_off=ooff, out_len=ol, consumed=co, status=st)

        for leg, enc in ((leg_a, auto), (leg_c, raw)):
            leg()
            torch.cuda.synchronize()
            assert not st.any().item(), "status"
            o = ooff.to(torch.int64) & 0xFFFFFFFF
            assert int(o[0].item()) == 0 and torch.equal(o[1:] - o[:-1], ol.to(torch.int64)), "offsets"
            assert torch.equal(ol.to(torch.int64), dl) and torch.equal(co, enc[2][:n]), "lengths"
            assert torch.equal(out[: w.dec_bytes], w.dec_blob[: w.dec_bytes]), "bytes"
        legs = {"a_strings_auto_us": leg_a, "b_decode_packed_huffman_us": leg_b, "c_strings_raw_us": leg_c, **legs}
    if len(sys.argv) > 4:
        legs = {k: v for k, v in legs.items() if k[0] in sys.argv[4]}
    for leg in legs.values():
        leg()
    torch.cuda.synchronize()
    src = source_hash()
    for r in range(rounds):
        line = dict(line0, round=r, reps=reps)
        for name, leg in legs.items():
            line[name] = timed(leg, reps)
        line.update(results_checked=have, lib=os.path.basename(os.environ.get("HPK_LIB", "libhpk.so")),
                    version=_lib.lib().hpk_version().decode().split(" gfx950")[0], source_sha256=src)
        print(json.dumps(line), flush=True)
    codec.check()


if __name__ == "__main__":
    main()
