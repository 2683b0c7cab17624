"""bench.py's --dump-outputs writer and its plain / --full switch (CPU: the writer takes any torch
tensors, here the oracle's decode of a small config-2 batch)."""

import os
import sys

import numpy as np
import pytest

from hpk_util import REPO, oracle_decode_batch

torch = pytest.importorskip("torch")
sys.path.insert(0, REPO)
import bench  # noqa: E402
from loona_amd import synth  # noqa: E402


def _entries(w):
    out, oo, ol, st = oracle_decode_batch(w.enc_blob, w.enc_off)
    return [("shard0", w.n, torch.from_numpy(out), torch.from_numpy(oo.astype(np.int64)).to(torch.int32),
             torch.from_numpy(ol.astype(np.int32)), torch.from_numpy(st))]


def test_dump_outputs_sample_and_sums(tmp_path, monkeypatch):
    w = synth.config2(n=50_000)
    ent = _entries(w)
    monkeypatch.setattr(bench, "DUMP_CHUNK", 20_000)  # three checksum rows, the last one short
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, ent)
    bench.dump_outputs(b, ent)
    names = sorted(os.listdir(a))
    assert names == sorted(f"shard0_{k}.npy" for k in ("literals", "out_off", "out_len", "status", "bytes", "sums"))
    total = 0
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype in (np.float32, np.float64)
        assert np.array_equal(x, y), f  # the same literals, run after run
        total += x.nbytes
    # the benchmark's 8 launches of a step stay under the 64 MB a dump may take
    assert 8 * total <= 64 * 2**20
    lit = np.load(os.path.join(a, "shard0_literals.npy")).astype(np.int64)
    rows = np.load(os.path.join(a, "shard0_bytes.npy"))
    lens = np.load(os.path.join(a, "shard0_out_len.npy"))
    assert rows.shape == (bench.DUMP_SAMPLE, bench.DUMP_WIDTH) and not np.load(os.path.join(a, "shard0_status.npy")).any()
    doff = np.asarray(w.dec_off, dtype=np.int64)
    dec = np.asarray(w.dec_blob)
    for k in range(0, len(lit), 97):
        want = dec[doff[lit[k]] : doff[lit[k] + 1]]
        assert lens[k] == len(want)
        assert np.array_equal(rows[k, : len(want)], want) and (rows[k, len(want) :] == -1).all()
    sums = np.load(os.path.join(a, "shard0_sums.npy"))
    assert sums.shape == (3, 4)
    cuts = [0, 20_000, 40_000, 50_000]
    for r, (x, y) in enumerate(zip(cuts[:-1], cuts[1:])):
        part = dec[doff[x] : doff[y]].astype(np.int64)
        assert sums[r, 0] == part.sum()
        assert sums[r, 1] == (part * (np.arange(part.size) % 65521 + 1)).sum()
        assert sums[r, 2] == doff[y] - doff[x] and sums[r, 3] == 0


def test_dump_outputs_sees_a_changed_byte(tmp_path):
    w = synth.config2(n=2_000)  # (the checksums cover every literal, sampled or not)
    ent = _entries(w)
    bench.dump_outputs(str(tmp_path / "a"), ent)
    tag, n, out, oo, ol, st = ent[0]
    out = out.clone()
    out[int(oo[n - 1])] ^= 1  # first byte of the last literal
    bench.dump_outputs(str(tmp_path / "b"), [(tag, n, out, oo, ol, st)])
    sa, sb = (np.load(str(tmp_path / d / "shard0_sums.npy")) for d in ("a", "b"))
    assert abs(sa[0, 0] - sb[0, 0]) == 1 and sa[0, 1] != sb[0, 1]


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    args = bench.parse()
    assert args.steps == 3 and args.warmup == 1 and not args.full and args.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full and args.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
