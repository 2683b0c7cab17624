"""Block generators shared by the block decoder's tests: tests/test_hpack.py runs them through the library, and the
stand-alone host driver (tests/host_cases.py, tests/test_host_sanitizers.py) decodes the same blocks under the host
sanitizers."""

import random

from hpk_util import hpack_ref


def churn_streams(seed=4096, streams=6, blocks=120):
    """[[block]] per stream: long runs of insertions, lookups, evictions and size updates (tests/test_hpack.py's churn):
    the decoder's entry ring grows past its first 64 slots and its byte buffer is compacted many times"""
    rng = random.Random(seed)
    out = []
    for _ in range(streams):
        entries = 0
        mine = []
        for _ in range(blocks):
            blk = bytearray()
            if rng.random() < 0.15:  # dynamic table size update (decoder.rs:538-554)
                blk += hpack_ref.encode_integer(rng.choice([0, 100, 4096, 20000, 60000]), 5, 0x20)
            for _ in range(rng.randrange(1, 24)):
                op = rng.random()
                if op < 0.55:  # literal with incremental indexing, new name
                    nl = rng.choice([0, 1, 5, 12, 40, rng.randrange(0, 300)])
                    vl = rng.choice([0, 3, 20, 100, rng.randrange(0, 5000)])
                    blk += b"\x40" + hpack_ref.encode_integer(nl, 7, 0) + bytes(rng.randrange(97, 123) for _ in range(nl))
                    blk += hpack_ref.encode_integer(vl, 7, 0) + bytes(rng.randrange(32, 127) for _ in range(vl))
                    entries += 1
                elif op < 0.75:  # literal with incremental indexing, indexed name
                    idx = rng.randrange(1, 62) if rng.random() < 0.7 else rng.randrange(62, 65)
                    vl = rng.randrange(0, 60)
                    blk += hpack_ref.encode_integer(idx, 6, 0x40)
                    blk += hpack_ref.encode_integer(vl, 7, 0) + bytes(rng.randrange(32, 127) for _ in range(vl))
                    entries += 1
                else:  # indexed field, sometimes past the table
                    hi = 62 + min(entries, 400) + 3 if rng.random() < 0.05 else 65
                    blk += hpack_ref.encode_integer(rng.randrange(1, hi), 7, 0x80)
            mine.append(bytes(blk))
        out.append(mine)
    return out
