#!/usr/bin/env python3
"""What naming the corrupt shard costs over the scrub alone.

tools/bench_verify.py's method on bench.py's own batch (4096 x 1 MiB-shard
stripes, 64 KiB shard pad, device resident, data from fill_stripes_splitmix,
parity from encode_batch): one process, warm-up, then the legs alternate with
the order flipped each round, HIP-event times, medians.

  (v)   verify_batch on the clean batch;
  (l0)  locate_corrupt_batch on the clean batch: pass 1 is the same verify,
        pass 2 reads one word per (stripe, 4 KiB chunk) and no shard;
  (l1)  locate_corrupt_batch on a copy with 1 stripe holding one flipped byte;
  (l64) the same with 64 such stripes: pass 2 reads 14 MiB per flagged stripe.

The number that matters is l0 / v. After the clock: the clean words are all 0,
and the suspects of the two dirty batches equal the seeded flips (one bit per
flipped stripe). Prints one JSON line; --out writes it to a file
(profiles/locate/bench_locate.json).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED_BASE = 0x5EED0000


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--shard-len", type=int, default=1 << 20)
    ap.add_argument("--shard-pad", type=int, default=64 << 10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    if args.rounds < 7:
        ap.error("--rounds must be at least 7")

    import torch
    import helyim_amd as H
    import helyim_amd.batch as B

    S, L = args.stripes, args.shard_len
    if S < 64:
        ap.error("--stripes must be at least 64")
    rs = H.ReedSolomon(10, 4)
    t = B.empty_stripes(S, 14, L, shard_pad=args.shard_pad)
    B.fill_stripes_splitmix(t, 10, SEED_BASE)
    B.encode_batch(rs, t)
    torch.cuda.synchronize()
    mis = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    sus = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()

    # the dirty legs run on the one batch: their flips are put in before each
    # timed call and taken out after it, outside the events
    rng = np.random.default_rng(SEED_BASE)
    order = rng.permutation(S)[:64]
    flips = [(int(s), int(rng.integers(14)), int(rng.integers(L)), int(rng.integers(1, 256))) for s in order]

    def toggle(n):
        for s, i, p, v in flips[:n]:
            t[s, i, p] ^= v

    def verify():
        B.verify_batch(rs, t, mismatch=mis)

    def locate():
        B.locate_corrupt_batch(rs, t, mismatch=mis, suspects=sus)

    legs = {"v": (verify, 0), "l0": (locate, 0), "l1": (locate, 1), "l64": (locate, 64)}
    for _ in range(args.warmup):
        for fn, _n in legs.values():
            fn()
    torch.cuda.synchronize()

    times = {k: [] for k in legs}
    checks = {}
    for r in range(args.rounds):
        keys = list(legs) if r % 2 == 0 else list(legs)[::-1]
        for k in keys:
            fn, n = legs[k]
            toggle(n)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
            if r == args.rounds - 1 and k != "v":  # after the clock of this call
                got = sus.cpu().numpy().view(np.uint32)
                want = np.zeros(S, dtype=np.uint32)
                for s, i, _p, _v in flips[:n]:
                    want[s] = 1 << i
                flagged = mis.cpu().numpy() != 0
                checks[k] = bool((got == want).all()) and bool((flagged == (want != 0)).all())
            toggle(n)
    torch.cuda.synchronize()
    clean_again = B.verify_batch(rs, t).cpu().numpy()
    restored = bool((clean_again == 0).all())

    def stats(v):
        return {"ms_median": round(float(np.median(v)), 4), "ms_min": round(float(np.min(v)), 4),
                "ms_max": round(float(np.max(v)), 4), "ms_rounds": [round(float(x), 4) for x in v]}

    med = {k: float(np.median(v)) for k, v in times.items()}
    nbytes = 14 * L * S
    result = {
        "tool": "tools/bench_locate.py", "lib": os.path.basename(H.LIB_PATH), "version": H.version(),
        "device": torch.cuda.get_device_name(0),
        "stripes": S, "shard_len": L, "shard_pad": args.shard_pad, "rounds": args.rounds,
        "verify_kernel": B.verify_kernel_name(L),
        "verify": dict(stats(times["v"]), GiBps_14_shards_read=round(nbytes / (med["v"] * 1e-3) / 2**30, 1)),
        "locate_clean": stats(times["l0"]),
        "locate_1_dirty_stripe": stats(times["l1"]),
        "locate_64_dirty_stripes": stats(times["l64"]),
        "ratio_locate_clean_over_verify_median": round(med["l0"] / med["v"], 4),
        "ratio_locate_clean_over_verify_rounds": [round(a / b, 4) for a, b in zip(times["l0"], times["v"])],
        "ms_added_by_1_dirty_stripe_median": round(med["l1"] - med["l0"], 4),
        "ms_added_by_64_dirty_stripes_median": round(med["l64"] - med["l0"], 4),
        "suspects_equal_seeded_flips": checks,
        "batch_restored_clean": restored,
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if restored and all(checks.get(k) for k in ("l0", "l1", "l64")) else 1


if __name__ == "__main__":
    sys.exit(main())
