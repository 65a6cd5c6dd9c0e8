#!/usr/bin/env python3
"""What correcting in place costs, against locating and against the repair.

tools/bench_locate_pairs.py's method and batch (4096 x 1 MiB-shard stripes, 64
KiB shard pad, device resident, data from fill_stripes_splitmix, parity from
encode_batch): one process, warm-up, then the legs alternate with the order
flipped each round, HIP-event times, medians and min..max. Correct and repair
change their input, so every corrupted leg XORs its seeded corruption in
before each timed call, outside the events; the call itself takes it out.

  (l0)    locate_corrupt_batch on the clean batch;
  (c0)    correct_batch on the clean batch: pass 1 and the walk are the same code;
  (r64)   repair_batch with 64 stripes holding one flipped byte;
  (c64)   correct_batch with the same 64 flips;
  (cp64)  correct_batch(pairs=True) with 64 stripes where two shards carry a
          corrupted 4 KiB run at the same offset;
  (rfull) repair_batch with 64 stripes whose shard 3 is wrong throughout;
  (cfull) correct_batch with the same;
  (c5)    correct_batch with 64 stripes where five shards carry one flipped
          byte each at five offsets; repair_batch leaves such stripes alone,
          and how many it left is reported (once, untimed).

The criterion is relative: the median of c0 must lie within l0's own min..max
over the rounds. No other time is fixed in advance. After every timed call of
the last round the words and counters equal the seeded construction; after the
clock the 64 stripes every leg touched equal their saved originals byte for
byte and the whole batch verifies clean. Prints one JSON line; --out writes it
to a file (profiles/correct/bench_correct.json).
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
FULL_SHARD = 3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--shard-len", type=int, default=1 << 20)
    ap.add_argument("--shard-pad", type=int, default=64 << 10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
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
    masks = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    left = torch.zeros(1, dtype=torch.int32, device="cuda")
    unc = torch.zeros(1, dtype=torch.int32, device="cuda")
    nbytes = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream()

    rng = np.random.default_rng(SEED_BASE)
    order = [int(s) for s in rng.permutation(S)[:64]]
    saved = {s: t[s].clone() for s in order}  # every leg damages these 64 stripes and no other
    flips = [(s, int(rng.integers(14)), int(rng.integers(L)), int(rng.integers(1, 256))) for s in order]
    runs = []
    for s in order:
        a, b = sorted(int(c) for c in rng.choice(14, 2, replace=False))
        off = int(rng.integers(0, L - RUN + 1)) // 16 * 16
        pats = [torch.from_numpy(rng.integers(1, 256, RUN, dtype=np.uint8)).cuda() for _ in range(2)]  # no zero byte
        runs.append((s, a, b, off, pats))
    full = torch.from_numpy(rng.integers(1, 256, L, dtype=np.uint8)).cuda()  # no zero byte
    fives = []
    for s in order:
        shards = [int(c) for c in rng.choice(14, 5, replace=False)]
        offs = [int(o) for o in rng.choice(L, 5, replace=False)]
        fives.append((s, [(c, o, int(rng.integers(1, 256))) for c, o in zip(shards, offs)]))

    def apply(kind):
        if kind == "flips":
            for s, i, p, v in flips:
                t[s, i, p] ^= v
        elif kind == "runs":
            for s, a, b, off, (pa, pb) in runs:
                t[s, a, off:off + RUN] ^= pa
                t[s, b, off:off + RUN] ^= pb
        elif kind == "full":
            for s in order:
                t[s, FULL_SHARD] ^= full
        elif kind == "fives":
            for s, hits in fives:
                for c, o, v in hits:
                    t[s, c, o] ^= v

    def want(kind):
        """-> (suspects words, bytes a correct changes)."""
        w = np.zeros(S, dtype=np.uint32)
        if kind == "flips":
            for s, i, _p, _v in flips:
                w[s] = 1 << i
            return w, 64
        if kind == "runs":
            for s, a, b, _off, _pats in runs:
                w[s] = (1 << a) | (1 << b)
            return w, 64 * 2 * RUN
        if kind == "full":
            w[order] = 1 << FULL_SHARD
            return w, 64 * L
        if kind == "fives":
            for s, hits in fives:
                w[s] = sum(1 << c for c, _o, _v in hits)
            return w, 64 * 5
        return w, 0

    def locate():
        B.locate_corrupt_batch(rs, t, mismatch=mis, suspects=sus)

    def repair():
        B.repair_batch(rs, t, mismatch=mis, suspects=sus, present_masks=masks, unrepaired=left)

    def correct():
        B.correct_batch(rs, t, mismatch=mis, suspects=sus, uncorrected=unc, corrected_bytes=nbytes)

    def correct_pairs():
        B.correct_batch(rs, t, mismatch=mis, suspects=sus, uncorrected=unc, corrected_bytes=nbytes, pairs=True)

    legs = {"l0": (locate, None), "c0": (correct, None), "r64": (repair, "flips"), "c64": (correct, "flips"),
            "cp64": (correct_pairs, "runs"), "rfull": (repair, "full"), "cfull": (correct, "full"),
            "c5": (correct, "fives")}
    for _ in range(args.warmup):
        for fn, kind in legs.values():
            apply(kind)
            fn()
    torch.cuda.synchronize()

    times = {k: [] for k in legs}
    checks = {}
    for r in range(args.rounds):
        keys = list(legs) if r % 2 == 0 else list(legs)[::-1]
        for k in keys:
            fn, kind = legs[k]
            apply(kind)
            unc.zero_()
            nbytes.zero_()
            left.zero_()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
            if r == args.rounds - 1:  # after the clock of this call
                words, changed = want(kind)
                ok = bool((sus.cpu().numpy().view(np.uint32) == words).all())
                ok = ok and bool(((mis.cpu().numpy() != 0) == (words != 0)).all())
                if k.startswith("c"):
                    ok = ok and int(unc.item()) == 0 and int(nbytes.item()) == changed
                elif k.startswith("r"):
                    ok = ok and int(left.item()) == 0
                checks[k] = ok
    torch.cuda.synchronize()
    # what the repair does with c5's damage: the stripes it leaves alone (untimed)
    apply("fives")
    left.zero_()
    repair()
    torch.cuda.synchronize()
    c5_left_by_repair = int(left.item())
    correct()  # takes the damage out again
    torch.cuda.synchronize()
    restored = all(bool(torch.equal(t[s], saved[s])) for s in order)
    clean = bool((B.verify_batch(rs, t).cpu().numpy() == 0).all())

    def stats(v):
        return {"ms_median": round(float(np.median(v)), 4), "ms_min": round(float(np.min(v)), 4),
                "ms_max": round(float(np.max(v)), 4), "ms_rounds": [round(float(x), 4) for x in v]}

    med = {k: float(np.median(v)) for k, v in times.items()}
    within = bool(min(times["l0"]) <= med["c0"] <= max(times["l0"]))
    result = {
        "tool": "tools/bench_correct.py", "lib": os.path.basename(H.LIB_PATH), "version": H.version(),
        "device": torch.cuda.get_device_name(0),
        "stripes": S, "shard_len": L, "shard_pad": args.shard_pad, "rounds": args.rounds, "run_bytes": RUN,
        "verify_kernel": B.verify_kernel_name(L),
        **{k: stats(times[k]) for k in legs},
        "ratio_c0_over_l0_median": round(med["c0"] / med["l0"], 4),
        "ratio_c64_over_r64_median": round(med["c64"] / med["r64"], 4),
        "ratio_cfull_over_rfull_median": round(med["cfull"] / med["rfull"], 4),
        "ms_cp64_minus_c0_median": round(med["cp64"] - med["c0"], 4),
        "ms_c5_minus_c0_median": round(med["c5"] - med["c0"], 4),
        "c5_stripes_left_by_repair": c5_left_by_repair,
        "c0_median_within_l0_min_max": within,
        "words_and_counters_equal_seeded_construction": checks,
        "damaged_stripes_equal_their_originals": restored,
        "batch_verifies_clean": clean,
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ok = restored and clean and within and c5_left_by_repair == 64 and all(checks.get(k) for k in legs)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
