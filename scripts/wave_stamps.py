#!/usr/bin/env python3
"""Per-wave phase stamps of the v25 wave-fill decode kernel (diagnostic build, HPK_DEBUG_MODE=3,
HPK_DECODE_KERNEL=wave): `python scripts/wave_stamps.py [config5|c2_4m|config2]`. One JSON line: mean
cycles per wave in each phase and its share of the wave's total, the lane loop split into its body rounds
and its tails, and the per-fill figures (cycles, rounds, fills per wave). Since decode v40 "queue" holds the
queue reads ("prefetch_issue_qread" the prefetch issue and the first literal's load only), and "write_back" the
issue of the image's read-out before the sort plus the stores after it; a stamp waits for every LDS
operation in flight, so the stamped build does not run the sort under the read-out as the product does."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("HPK_LIB", os.path.join(REPO, "loona_amd", "libhpk_diag.so"))
os.environ["HPK_DEBUG_MODE"] = "3"
os.environ.setdefault("HPK_DECODE_KERNEL", "wave")
from loona_amd import HuffmanCodec, _lib, synth  # noqa: E402
from loona_amd.batch import decode_offsets_torch  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "config5"
codec = HuffmanCodec(0)
gens = {"config2": synth.device_config2, "c2_4m": lambda c: synth.device_config2(c, n=4_000_000),
        "config5": lambda c: synth.device_config5_shard(c, 0)}
w = gens[wl](codec)
doff = decode_offsets_torch(w.enc_off)
out = torch.empty(int(doff[-1].item()) + 16, dtype=torch.uint8, device="cuda")
ol = torch.empty(w.n, dtype=torch.int32, device="cuda")
st = torch.empty(w.n, dtype=torch.uint8, device="cuda")
for _ in range(3):
    codec.decode_into(w.enc_blob, w.enc_off, out, doff, ol, st, device=True, sync=True)
synth.check_decoded(w, out, doff, ol, st)
L = _lib.lib()
L.hpk_debug_stamps.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
buf = np.zeros(256 * 16 * 16, np.uint64)
got = L.hpk_debug_stamps(buf.ctypes.data, buf.size)
s = buf[:got].reshape(-1, 16).astype(np.int64)
names = ["total", "offsets_wait", "write_back", "queue", "window", "prefetch_issue_qread", "lane_tails",
         "byte_path_results", "fills", "loop_rounds", "long_phase", "before_first_fill", "lane_body"]
tot = s[:, 0].mean()
res = {"workload": wl, "kernel": os.environ["HPK_DECODE_KERNEL"], "waves": int(s.shape[0])}
for i, nm in enumerate(names):
    res[nm] = {"mean": round(float(s[:, i].mean()), 1), "max": int(s[:, i].max()), "min": int(s[:, i].min())}
    if i not in (0, 8, 9):
        res[nm]["share"] = round(float(s[:, i].mean() / tot), 4)
# the lane loop is its body rounds (stamp 12) and its tails (stamp 6); per fill, with the rounds per fill
body, tails, fills = s[:, 12].mean(), s[:, 6].mean(), max(float(s[:, 8].mean()), 1.0)
res["lane_loop"] = {"mean": round(float(body + tails), 1), "share": round(float((body + tails) / tot), 4),
                    "tail_share_of_loop": round(float(tails / max(body + tails, 1.0)), 4)}
res["per_fill"] = {"total": round(float(tot / fills), 1), "lane_body": round(float(body / fills), 1),
                   "lane_tails": round(float(tails / fills), 1), "rounds": round(float(s[:, 9].mean() / fills), 3),
                   "fills_per_wave": round(fills, 2)}
print(json.dumps(res), flush=True)
