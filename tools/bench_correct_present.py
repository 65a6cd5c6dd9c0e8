#!/usr/bin/env python3
"""What correcting a degraded batch in place costs, against locating in it and
against the checked reconstruct.

tools/bench_correct.py's method and batch (4096 x 1 MiB-shard stripes, 64 KiB
shard pad, device resident, data from fill_stripes_splitmix, parity from
encode_batch): one process, warm-up, then the legs alternate with the order
flipped each round, HIP-event times, medians and min..max. One seeded shard of
every stripe is erased (its bit is clear in the present mask) in every leg.
The correcting legs change their input, so every corrupted leg XORs its seeded
corruption into present shards before each timed call, outside the events; the
call itself takes it out.

  (lp0)     locate_corrupt_present_batch on the clean batch;
  (cp0)     correct_present_batch on the clean batch: pass 1 and the walk are the same code;
  (rc64)    reconstruct_checked_batch with 64 stripes holding one flipped byte;
  (rcc64)   reconstruct_corrected_batch with the same 64 flips;
  (cc5)     reconstruct_corrected_batch with 64 stripes where five survivors
            carry one flipped byte each at five offsets; reconstruct_checked_batch
            leaves such stripes alone, and how many it left is reported (once,
            untimed);
  (rcfull)  reconstruct_checked_batch with 64 stripes with one survivor wrong throughout;
  (rccfull) reconstruct_corrected_batch with the same.

The criterion is relative: the median of cp0 must lie within lp0's own min..max
over the rounds. No other time is fixed in advance. After every timed call of
the last round the words, use masks and counters equal the seeded construction;
after the clock the 64 stripes every leg touched equal their saved originals
byte for byte and the whole batch verifies clean. Prints one JSON line; --out
writes it to a file (profiles/correct_present/bench_correct_present.json).
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
ALL = 0x3FFF


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
    if S < 64 or L < 16:
        ap.error("--stripes must be at least 64 and --shard-len at least 16")
    rs = H.ReedSolomon(10, 4)
    t = B.empty_stripes(S, 14, L, shard_pad=args.shard_pad)
    B.fill_stripes_splitmix(t, 10, SEED_BASE)
    B.encode_batch(rs, t)
    torch.cuda.synchronize()
    chk = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    sus = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    use = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    left = torch.zeros(1, dtype=torch.int32, device="cuda")
    unc = torch.zeros(1, dtype=torch.int32, device="cuda")
    nbytes = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream()

    rng = np.random.default_rng(SEED_BASE)
    erased = rng.integers(14, size=S)
    present = (ALL & ~(1 << erased)).astype(np.uint32)
    masks = torch.tensor(present.view(np.int32), device="cuda")
    order = [int(s) for s in rng.permutation(S)[:64]]
    saved = {s: t[s].clone() for s in order}  # every leg damages these 64 stripes and no other

    def survivors(s, n):
        ids = [i for i in range(14) if i != int(erased[s])]
        return [ids[int(j)] for j in rng.choice(13, n, replace=False)]

    flips = [(s, survivors(s, 1)[0], int(rng.integers(L)), int(rng.integers(1, 256))) for s in order]
    full_shard = {s: survivors(s, 1)[0] for s in order}
    full = torch.from_numpy(rng.integers(1, 256, L, dtype=np.uint8)).cuda()  # no zero byte
    fives = []
    for s in order:
        offs = [int(o) for o in rng.choice(L, 5, replace=False)]
        fives.append((s, [(c, o, int(rng.integers(1, 256))) for c, o in zip(survivors(s, 5), offs)]))

    def apply(kind):
        if kind == "flips":
            for s, i, p, v in flips:
                t[s, i, p] ^= v
        elif kind == "full":
            for s in order:
                t[s, full_shard[s]] ^= full
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
        if kind == "full":
            for s in order:
                w[s] = 1 << full_shard[s]
            return w, 64 * L
        if kind == "fives":
            for s, hits in fives:
                w[s] = sum(1 << c for c, _o, _v in hits)
            return w, 64 * 5
        return w, 0

    def locate():
        B.locate_corrupt_present_batch(rs, t, masks, check=chk, suspects=sus)

    def correct():
        B.correct_present_batch(rs, t, masks, check=chk, suspects=sus, uncorrected=unc, corrected_bytes=nbytes)

    def checked():
        B.reconstruct_checked_batch(rs, t, masks, check=chk, suspects=sus, use_masks=use, unrepaired=left)

    def corrected():
        B.reconstruct_corrected_batch(rs, t, masks, check=chk, suspects=sus, use_masks=use, unrepaired=left,
                                      corrected_bytes=nbytes)

    legs = {"lp0": (locate, None), "cp0": (correct, None), "rc64": (checked, "flips"), "rcc64": (corrected, "flips"),
            "cc5": (corrected, "fives"), "rcfull": (checked, "full"), "rccfull": (corrected, "full")}
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
                ok = ok and bool(((chk.cpu().numpy() != 0) == (words != 0)).all())
                if fn is correct:
                    ok = ok and int(unc.item()) == 0 and int(nbytes.item()) == changed
                elif fn is checked:  # the named survivor is dropped and rebuilt with the hole
                    ok = ok and int(left.item()) == 0
                    ok = ok and bool((use.cpu().numpy().view(np.uint32) == (present & ~words)).all())
                elif fn is corrected:  # nothing is dropped
                    ok = ok and int(left.item()) == 0 and int(nbytes.item()) == changed
                    ok = ok and bool((use.cpu().numpy().view(np.uint32) == present).all())
                checks[k] = ok
    torch.cuda.synchronize()
    # what the checked reconstruct does with cc5's damage: the stripes it leaves alone (untimed)
    apply("fives")
    left.zero_()
    checked()
    torch.cuda.synchronize()
    cc5_left_by_checked = int(left.item())
    corrected()  # takes the damage out again
    torch.cuda.synchronize()
    restored = all(bool(torch.equal(t[s], saved[s])) for s in order)
    clean = bool((B.verify_batch(rs, t).cpu().numpy() == 0).all())

    def stats(v):
        return {"ms_median": round(float(np.median(v)), 4), "ms_min": round(float(np.min(v)), 4),
                "ms_max": round(float(np.max(v)), 4), "ms_rounds": [round(float(x), 4) for x in v]}

    med = {k: float(np.median(v)) for k, v in times.items()}
    within = bool(min(times["lp0"]) <= med["cp0"] <= max(times["lp0"]))
    result = {
        "tool": "tools/bench_correct_present.py", "lib": os.path.basename(H.LIB_PATH), "version": H.version(),
        "device": torch.cuda.get_device_name(0),
        "stripes": S, "shard_len": L, "shard_pad": args.shard_pad, "rounds": args.rounds, "erased_per_stripe": 1,
        "check_kernel": B.check_kernel_name(L),
        **{k: stats(times[k]) for k in legs},
        "ratio_cp0_over_lp0_median": round(med["cp0"] / med["lp0"], 4),
        "ratio_rcc64_over_rc64_median": round(med["rcc64"] / med["rc64"], 4),
        "ratio_rccfull_over_rcfull_median": round(med["rccfull"] / med["rcfull"], 4),
        "ms_cc5_minus_rcc64_median": round(med["cc5"] - med["rcc64"], 4),
        "cc5_stripes_left_by_checked_reconstruct": cc5_left_by_checked,
        "cp0_median_within_lp0_min_max": within,
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
    ok = restored and clean and within and cc5_left_by_checked == 64 and all(checks.get(k) for k in legs)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
