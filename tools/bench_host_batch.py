"""Whole-call times of the four host batch operations on every staging path.

hec_host_encode_batch, hec_host_reconstruct_batch (stripe s has lost s % 5
shards, bench.py's erasure_masks), hec_host_reconstruct_some_batch (the first
lost shard of each stripe wanted) and hec_host_verify_batch on one
[stripes, 14, shard_len] tensor of RS(10,4) stripes, in pinned and in pageable
memory, each with zero copy on and off: the direct view, the two pinned slots
and the copy pipeline from either kind of memory. 256 stripes of 1 MiB are 43
chunks of 6 stripes. Median of --reps timed calls after --warmup, in-process;
the library comes from HEC_LIB_PATH when set. Prints one JSON line.
python tools/bench_host_batch.py [--stripes 256] [--shard-len 1048576]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=256)
    ap.add_argument("--shard-len", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    from bench import erasure_masks
    S, L = args.stripes, args.shard_len
    rs = H.ReedSolomon(10, 4)
    by_count = [erasure_masks(S, 0, e).view(np.uint32) for e in range(5)]
    masks = np.array([by_count[s % 5][s] for s in range(S)], dtype=np.uint32)
    lost = ~masks & 0x3FFF
    wants = (lost & -lost.astype(np.int64)).astype(np.uint32)  # lowest lost shard, 0 where none is lost
    pageable = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (S, 14, L), dtype=np.uint8))
    B.host_encode_batch(rs, pageable)
    legs = {}
    ok = True
    for memory, t in (("pinned", pageable.pin_memory()), ("pageable", pageable)):
        for zc in (1, 0):
            assert H.lib.hec_set_host_zero_copy(zc) == 0
            assert B.host_zero_copy(t) == (memory == "pinned" and zc == 1)
            ops = {"encode": lambda: B.host_encode_batch(rs, t),
                   "reconstruct": lambda: B.host_reconstruct_batch(rs, t, masks),
                   "reconstruct_some": lambda: B.host_reconstruct_some_batch(rs, t, masks, wants),
                   "verify": lambda: B.host_verify_batch(rs, t)}
            for op, call in ops.items():
                times = []
                for i in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    r = call()
                    times.append(time.perf_counter() - t0)
                ok = ok and (r is None or not np.any(r))  # no stripe skipped, no mismatch word set
                legs[f"{op}/{memory}/zero_copy_{'on' if zc else 'off'}"] = round(
                    statistics.median(times[args.warmup:]) * 1e3, 3)
    H.lib.hec_set_host_zero_copy(1)
    print(json.dumps({"lib": os.environ.get("HEC_LIB_PATH", "product"), "stripes": S, "shard_len": L,
                      "reps": args.reps, "median_ms": legs, "clean": bool(ok)}), flush=True)


if __name__ == "__main__":
    main()
