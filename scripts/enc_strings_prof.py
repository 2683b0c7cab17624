#!/usr/bin/env python3
"""Diagnostics for the string-literal emit kernel (not part of the product): cycles per phase, summed over
waves, of one launch of the packed encode's kernel and of the string-literal emit kernel under HPK_STR_AUTO and
HPK_STR_RAW, from the diagnostic library's HPK_ENCODE_CFG=9 variants (the phases are hpk_encode2's):
`python scripts/enc_strings_prof.py config3`. One JSON line per kernel, millions of cycles per phase."""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("HPK_LIB", os.path.join(REPO, "loona_amd", "libhpk_diag.so"))
os.environ["HPK_ENCODE_CFG"] = "9"

import numpy as np  # noqa: E402
import torch  # noqa: E402

from loona_amd import HuffmanCodec, _lib, synth  # noqa: E402

PHASES = ["top", "meta_fits", "setup", "pass1", "scan", "pass2", "finalize", "writeback", "split", "unused9",
          "unused10", "barrier_waits"]


def main():
    wl = sys.argv[1] if len(sys.argv) > 1 else "config3"
    codec = HuffmanCodec(0)
    w = {"config2": synth.device_config2, "config3": synth.device_config3}[wl](codec)
    n = w.n
    doff = w.dec_off.to(torch.int32)
    out = torch.empty(max(w.enc_bytes, w.dec_bytes) + 6 * n + 16, dtype=torch.uint8, device="cuda")
    ol = torch.empty(n, dtype=torch.int32, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    ooff = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    raw = torch.ones(n, dtype=torch.uint8, device="cuda")
    L = _lib.lib()
    L.hpk_debug_encode_prof.argtypes = [ctypes.c_void_p]
    legs = {"encode_packed": lambda: codec.encode_packed(w.dec_blob, doff, out_blob=out, out_off=ooff, out_len=ol, status=st),
            "strings_auto": lambda: codec.encode_strings(w.dec_blob, doff, None, out_blob=out, out_off=ooff, out_len=ol,
                                                         status=st),
            "strings_raw": lambda: codec.encode_strings(w.dec_blob, doff, raw, out_blob=out, out_off=ooff, out_len=ol,
                                                        status=st)}
    for name, leg in legs.items():
        for _ in range(3):
            leg()
        torch.cuda.synchronize()
        buf = np.zeros(16, np.uint64)
        assert L.hpk_debug_encode_prof(buf.ctypes.data) == 0
        print(json.dumps({"workload": wl, "kernel": name, "Mcycles_total": round(float(buf[:12].sum()) / 1e6, 1),
                          "Mcycles": {p: round(float(buf[i]) / 1e6, 1) for i, p in enumerate(PHASES)}}), flush=True)


if __name__ == "__main__":
    main()
