#!/usr/bin/env python3
"""What naming two wrong shards per byte column costs over naming one.

tools/bench_locate.py's method and batch (4096 x 1 MiB-shard stripes, 64 KiB
shard pad, device resident, data from fill_stripes_splitmix, parity from
encode_batch): one process, warm-up, then the legs alternate with the order
flipped each round, HIP-event times, medians and min..max.

  (v)    verify_batch on the clean batch;
  (l0)   locate_corrupt_batch on the clean batch;
  (p0)   locate_corrupt_pairs_batch on the clean batch: the same code up to the
         first ballot, so a difference from l0 would be the pair code's cost in
         occupancy or prologue;
  (l64)  locate_corrupt_batch with 64 stripes holding one flipped byte;
  (p64)  locate_corrupt_pairs_batch with the same 64 flips: the pair search is
         behind a ballot no wave passes;
  (pp64) locate_corrupt_pairs_batch with 64 stripes where two shards carry a
         corrupted 4 KiB run at the same offset: four waves per stripe run the
         pair search on every byte.

The criterion is relative: the median of p0 must lie within l0's own min..max
over the rounds. p64 against l64, and pp64, carry no threshold. After the
clock: the words of each leg equal the seeded construction, pp64's words under
the existing locate are bit 31, and the batch verifies clean again. Prints one
JSON line; --out writes it to a file
(profiles/locate_pairs/bench_locate_pairs.json).
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
RUN = 4096
UNEXPLAINED = 0x80000000


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--shard-len", type=int, default=1 << 20)
    ap.add_argument("--shard-pad", type=int, default=64 << 10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    if args.rounds < 9:
        ap.error("--rounds must be at least 9")

    import torch
    import helyim_amd as H
    import helyim_amd.batch as B

    S, L = args.stripes, args.shard_len
    if S < 64 or L < RUN:
        ap.error("--stripes must be at least 64 and --shard-len at least 4096")
    rs = H.ReedSolomon(10, 4)
    t = B.empty_stripes(S, 14, L, shard_pad=args.shard_pad)
    B.fill_stripes_splitmix(t, 10, SEED_BASE)
    B.encode_batch(rs, t)
    torch.cuda.synchronize()
    mis = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    sus = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()

    # the dirty legs run on the one batch: their corruption is XORed in before
    # each timed call and out again after it, outside the events
    rng = np.random.default_rng(SEED_BASE)
    order = [int(s) for s in rng.permutation(S)[:64]]
    flips = [(s, int(rng.integers(14)), int(rng.integers(L)), int(rng.integers(1, 256))) for s in order]
    runs = []
    for s in order:
        a, b = sorted(int(c) for c in rng.choice(14, 2, replace=False))
        off = int(rng.integers(0, L - RUN + 1)) // 16 * 16
        pats = [torch.from_numpy(rng.integers(1, 256, RUN, dtype=np.uint8)).cuda() for _ in range(2)]  # no zero byte
        runs.append((s, a, b, off, pats))

    def toggle(kind):
        if kind == "flips":
            for s, i, p, v in flips:
                t[s, i, p] ^= v
        elif kind == "runs":
            for s, a, b, off, (pa, pb) in runs:
                t[s, a, off:off + RUN] ^= pa
                t[s, b, off:off + RUN] ^= pb

    def want_words(kind):
        want = np.zeros(S, dtype=np.uint32)
        if kind == "flips":
            for s, i, _p, _v in flips:
                want[s] = 1 << i
        elif kind == "runs":
            for s, a, b, _off, _pats in runs:
                want[s] = (1 << a) | (1 << b)
        return want

    def verify():
        B.verify_batch(rs, t, mismatch=mis)

    def locate():
        B.locate_corrupt_batch(rs, t, mismatch=mis, suspects=sus)

    def pairs():
        B.locate_corrupt_pairs_batch(rs, t, mismatch=mis, suspects=sus)

    legs = {"v": (verify, None), "l0": (locate, None), "p0": (pairs, None), "l64": (locate, "flips"),
            "p64": (pairs, "flips"), "pp64": (pairs, "runs")}
    for _ in range(args.warmup):
        for fn, kind in legs.values():
            toggle(kind)
            fn()
            toggle(kind)
    torch.cuda.synchronize()

    times = {k: [] for k in legs}
    checks = {}
    for r in range(args.rounds):
        keys = list(legs) if r % 2 == 0 else list(legs)[::-1]
        for k in keys:
            fn, kind = legs[k]
            toggle(kind)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
            if r == args.rounds - 1 and k != "v":  # after the clock of this call
                got = sus.cpu().numpy().view(np.uint32)
                want = want_words(kind)
                flagged = mis.cpu().numpy() != 0
                checks[k] = bool((got == want).all()) and bool((flagged == (want != 0)).all())
            toggle(kind)
    torch.cuda.synchronize()
    # the existing locate on pp64's corruption: every dirty stripe is bit 31 and nothing else
    toggle("runs")
    locate()
    torch.cuda.synchronize()
    got = sus.cpu().numpy().view(np.uint32)
    want = np.where(want_words("runs") != 0, np.uint32(UNEXPLAINED), np.uint32(0))
    checks["pp64_under_existing_locate_is_bit_31"] = bool((got == want).all())
    toggle("runs")
    torch.cuda.synchronize()
    restored = bool((B.verify_batch(rs, t).cpu().numpy() == 0).all())

    def stats(v):
        return {"ms_median": round(float(np.median(v)), 4), "ms_min": round(float(np.min(v)), 4),
                "ms_max": round(float(np.max(v)), 4), "ms_rounds": [round(float(x), 4) for x in v]}

    med = {k: float(np.median(v)) for k, v in times.items()}
    within = bool(min(times["l0"]) <= med["p0"] <= max(times["l0"]))
    result = {
        "tool": "tools/bench_locate_pairs.py", "lib": os.path.basename(H.LIB_PATH), "version": H.version(),
        "device": torch.cuda.get_device_name(0),
        "stripes": S, "shard_len": L, "shard_pad": args.shard_pad, "rounds": args.rounds, "run_bytes": RUN,
        "verify_kernel": B.verify_kernel_name(L),
        "v": stats(times["v"]), "l0": stats(times["l0"]), "p0": stats(times["p0"]), "l64": stats(times["l64"]),
        "p64": stats(times["p64"]), "pp64": stats(times["pp64"]),
        "ratio_p0_over_l0_median": round(med["p0"] / med["l0"], 4),
        "ratio_p64_over_l64_median": round(med["p64"] / med["l64"], 4),
        "ms_pp64_minus_p0_median": round(med["pp64"] - med["p0"], 4),
        "p0_median_within_l0_min_max": within,
        "words_equal_seeded_construction": checks,
        "batch_restored_clean": restored,
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ok = restored and within and all(checks.get(k) for k in ("l0", "p0", "l64", "p64", "pp64",
                                                            "pp64_under_existing_locate_is_bit_31"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
