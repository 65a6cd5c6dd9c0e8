#!/usr/bin/env python3
"""What the degraded scrub's masked verify costs, against the bit-sliced full
verify and against the only route a degraded batch had before it.

tools/bench_locate.py's method on bench.py's own batch (4096 x 1 MiB-shard
stripes, 64 KiB shard pad, device resident, data from fill_stripes_splitmix,
parity from encode_batch): one process, warm-up, then the legs alternate with
the order flipped each round, HIP-event times, medians and ranges.

  (v)    verify_batch: the bit-sliced scrub of all 14 shards, the ceiling;
  (c0)   verify_present_batch with full masks: the table kernel on 14 shards;
  (c1..c3) verify_present_batch with 1, 2, 3 shards of every stripe marked
         absent, positions varied from stripe to stripe: 13, 12, 11 shards read;
  (rv1..rv3) reconstruct_batch with the same masks, then verify_batch: what a
         caller had to run on such a batch before (and it rebuilds on faith).

The batch is clean throughout (the reconstruct rewrites the absent shards with
the bytes they held), so after the clock every check word must be 0. Rates
are bytes READ per second: (present shards) x shard_len x stripes over the
median time, also as a fraction of 8 TB/s. Prints one JSON line; --out writes
it to a file (profiles/degraded/bench_check.json).
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
PEAK_BYTES_PER_S = 8e12


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
    rs = H.ReedSolomon(10, 4)
    t = B.empty_stripes(S, 14, L, shard_pad=args.shard_pad)
    B.fill_stripes_splitmix(t, 10, SEED_BASE)
    B.encode_batch(rs, t)
    torch.cuda.synchronize()
    mis = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    chk = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    unchecked = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()

    rng = np.random.default_rng(SEED_BASE)
    masks = {}
    for f in range(4):
        m = np.full(S, 0x3FFF, dtype=np.int64)
        for s in range(S):
            for i in rng.choice(14, size=f, replace=False):
                m[s] &= ~(1 << int(i))
        masks[f] = torch.tensor(m.astype(np.int32), device="cuda")

    def verify():
        B.verify_batch(rs, t, mismatch=mis)

    def check(f):
        return lambda: B.verify_present_batch(rs, t, masks[f], check=chk, unchecked=unchecked)

    def rebuild_then_verify(f):
        def run():
            B.reconstruct_batch(rs, t, masks[f])
            B.verify_batch(rs, t, mismatch=mis)
        return run

    legs = {"v": verify}
    for f in range(4):
        legs["c%d" % f] = check(f)
    for f in (1, 2, 3):
        legs["rv%d" % f] = rebuild_then_verify(f)
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()

    times = {k: [] for k in legs}
    words_zero = {}
    for r in range(args.rounds):
        keys = list(legs) if r % 2 == 0 else list(legs)[::-1]
        for k in keys:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            legs[k]()
            e1.record(stream)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
            if r == args.rounds - 1:  # after the clock of this call
                words_zero[k] = bool(((chk if k.startswith("c") else mis).cpu().numpy() == 0).all())
    torch.cuda.synchronize()
    none_unchecked = int(unchecked.item()) == 0

    def stats(v, shards_read=None):
        d = {"ms_median": round(float(np.median(v)), 4), "ms_min": round(float(np.min(v)), 4),
             "ms_max": round(float(np.max(v)), 4), "ms_rounds": [round(float(x), 4) for x in v]}
        if shards_read:
            rate = shards_read * L * S / (float(np.median(v)) * 1e-3)
            d.update(shards_read=shards_read, TBps_read=round(rate / 1e12, 3),
                     fraction_of_8TBps=round(rate / PEAK_BYTES_PER_S, 3))
        return d

    result = {
        "tool": "tools/bench_check.py", "lib": os.path.basename(H.LIB_PATH), "version": H.version(),
        "device": torch.cuda.get_device_name(0),
        "stripes": S, "shard_len": L, "shard_pad": args.shard_pad, "rounds": args.rounds,
        "verify_kernel": B.verify_kernel_name(L), "check_kernel": B.check_kernel_name(L),
        "decode_kernel": H.lib.hec_decode_kernel_name(L).decode(),
        "verify_batch": stats(times["v"], 14),
    }
    for f in range(4):
        result["check_%d_erased" % f] = stats(times["c%d" % f], 14 - f)
    for f in (1, 2, 3):
        c, rv = times["c%d" % f], times["rv%d" % f]
        result["reconstruct_then_verify_%d_erased" % f] = stats(rv)
        result["ratio_check_over_reconstruct_then_verify_%d_erased_rounds" % f] = [round(a / b, 4) for a, b in zip(c, rv)]
        result["check_faster_every_round_%d_erased" % f] = bool(all(a < b for a, b in zip(c, rv)))
    result["ratio_check_full_mask_over_verify_median"] = round(
        float(np.median(times["c0"])) / float(np.median(times["v"])), 4)
    result["words_all_zero"] = words_zero
    result["no_stripe_unchecked"] = none_unchecked
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if none_unchecked and all(words_zero.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
