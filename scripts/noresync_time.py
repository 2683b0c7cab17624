#!/usr/bin/env python3
"""The huge-literal phase's worst case next to its usual one: a 1 MiB literal that is '0' repeated (no walk that
starts off a code boundary finds its way back, so the truth moves one piece per fix round: 1,023 rounds, the phase
is serial) against the 1 MiB text literal of tests/test_gpu.py::test_large_literals. Synchronous device-resident
calls, the two alternating in one process, every result checked against the oracle. One JSON line per literal
and round, then one with the medians and their ratio: `python scripts/noresync_time.py [rounds] [reps]`."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hpk_util import compare_batches, oracle_decode_batch, pack  # noqa: E402  (the checker)
from loona_amd import HuffmanCodec, huffman_encode  # noqa: E402


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    nb = 1 << 20
    rng = np.random.default_rng(4096)
    text = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789-_=;,/.:ABCDEFGHIJ ", np.uint8)
    lits = {"text": huffman_encode(rng.choice(text, nb + nb // 3).tobytes())[:nb], "zeros": huffman_encode(b"0" * (8 * nb // 5))}
    assert len(lits["zeros"]) == nb
    codec = HuffmanCodec(0, stream=torch.cuda.current_stream())
    bufs = {}
    for name, lit in lits.items():
        blob, off = pack([lit])
        ref = oracle_decode_batch(blob, off)
        db, do = torch.from_numpy(blob).cuda(), torch.from_numpy(off.astype(np.int32)).cuda()
        out, oo, ol, st = codec.decode_device(db, do, sync=True)
        compare_batches((out.cpu().numpy(), oo.cpu().numpy().astype(np.uint32), ol[:1].cpu().numpy().astype(np.uint32),
                         st[:1].cpu().numpy()), ref, name)
        bufs[name] = (db, do, out, oo, ol, st)
    times = {name: [] for name in lits}
    for r in range(rounds):
        for name in lits:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                codec.decode_into(*bufs[name], device=True, sync=True)
            us = (time.perf_counter() - t0) / reps * 1e6
            times[name].append(us)
            print(json.dumps({"literal": name, "round": r, "encoded_bytes": nb, "device_sync_call_us": round(us, 1)}), flush=True)
    med = {name: statistics.median(v) for name, v in times.items()}
    print(json.dumps({"encoded_bytes": nb, "text_us_median": round(med["text"], 1), "text_us_min_max": [round(min(times["text"]), 1),
                      round(max(times["text"]), 1)], "zeros_us_median": round(med["zeros"], 1),
                      "zeros_us_min_max": [round(min(times["zeros"]), 1), round(max(times["zeros"]), 1)],
                      "ratio": round(med["zeros"] / med["text"], 1), "rounds": rounds, "reps": reps}), flush=True)
    codec.close()


if __name__ == "__main__":
    main()
