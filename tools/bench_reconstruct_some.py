#!/usr/bin/env python3
"""What rebuilding only the wanted shards saves against the full decode.

The bench's batch (4096 x 1 MiB-shard stripes, 64 KiB shard pad, device
resident, data from fill_stripes_splitmix, parity from encode_batch) with four
seeded erasures per stripe. One process, warm-up, then the legs alternate with
the order flipped each round, HIP-event times, medians and min..max.

  (full)  reconstruct_batch;
  (all)   reconstruct_some_batch with every want bit set;
  (w3, w2, w1)  reconstruct_some_batch wanting 3, 2, 1 of the 4 erased shards
          (a seeded choice per stripe).

A stripe moves (10 + w) shard lengths and does w rows of GF math, so w1 moves
11 units against the full decode's 14. The criterion is relative: the median
of w1 lies below the minimum of full's rounds. `all` against `full` is
reported as a ratio, with whether its median lies inside full's min..max; no
threshold (existing callers do not take that path).

After the clock every leg runs once more on a batch whose erased shards hold
other bytes (the true bytes XOR 0xA5): on the device every wanted shard must
equal the encoded batch's and every unwanted erased shard what it held, and 16
seeded stripes per leg are brought back and their wanted shards compared with
the C oracle's reconstruct of the survivors. Prints one JSON line; --out writes
it to a file (profiles/reconstruct_some/bench_reconstruct_some.json).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED_BASE = 0x50FE0000
ALL = 0x3FFF
POISON = 0xA5


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
    from oracle import corc

    S, L = args.stripes, args.shard_len
    if S < 16 or L < 16:
        ap.error("--stripes and --shard-len must be at least 16")
    rs = H.ReedSolomon(10, 4)
    t = B.empty_stripes(S, 14, L, shard_pad=args.shard_pad)
    B.fill_stripes_splitmix(t, 10, SEED_BASE)
    B.encode_batch(rs, t)
    torch.cuda.synchronize()
    truth = t.clone()
    stream = torch.cuda.current_stream()

    rng = np.random.default_rng(SEED_BASE)
    erased = np.stack([rng.permutation(14)[:4] for _ in range(S)])  # seeded order: the first w are wanted
    present = np.full(S, ALL, dtype=np.uint32)
    for q in range(4):
        present &= ~(np.uint32(1) << erased[:, q].astype(np.uint32))
    masks = torch.tensor(present.view(np.int32), device="cuda")

    def want_words(w):
        words = np.zeros(S, dtype=np.uint32)
        for q in range(w):
            words |= np.uint32(1) << erased[:, q].astype(np.uint32)
        return words

    wants = {"all": np.full(S, 0xFFFFFFFF, dtype=np.uint32), "w3": want_words(3), "w2": want_words(2),
             "w1": want_words(1)}
    dwants = {k: torch.tensor(v.view(np.int32), device="cuda") for k, v in wants.items()}
    wanted = {"full": want_words(4), "all": want_words(4), **{k: wants[k] for k in ("w3", "w2", "w1")}}

    def leg(k):
        if k == "full":
            B.reconstruct_batch(rs, t, masks)
        else:
            B.reconstruct_some_batch(rs, t, masks, dwants[k])

    legs = ["full", "all", "w3", "w2", "w1"]
    for _ in range(args.warmup):
        for k in legs:
            leg(k)
    torch.cuda.synchronize()

    times = {k: [] for k in legs}
    for r in range(args.rounds):
        for k in (legs if r % 2 == 0 else legs[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            leg(k)
            e1.record(stream)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    torch.cuda.synchronize()

    # after the clock: every erased shard holds other bytes, then each leg once more
    rows = {j: torch.tensor(np.flatnonzero(((present >> j) & 1) == 0), device="cuda") for j in range(14)}
    oracle = corc.CReedSolomon(10, 4)
    sample = [int(s) for s in rng.permutation(S)[:16]]
    checks = {}
    for k in legs:
        for j in range(14):
            t[rows[j], j] = truth[rows[j], j] ^ POISON
        leg(k)
        torch.cuda.synchronize()
        ok_wanted = ok_unwanted = True
        for j in range(14):
            is_w = ((wanted[k] >> j) & 1) == 1
            gone = ((present >> j) & 1) == 0
            w_rows = torch.tensor(np.flatnonzero(gone & is_w), device="cuda")
            u_rows = torch.tensor(np.flatnonzero(gone & ~is_w), device="cuda")
            if len(w_rows):
                ok_wanted = ok_wanted and bool(torch.equal(t[w_rows, j], truth[w_rows, j]))
            if len(u_rows):
                ok_unwanted = ok_unwanted and bool(torch.equal(t[u_rows, j], truth[u_rows, j] ^ POISON))
        ok_present = all(bool(torch.equal(t[s][[j for j in range(14) if (present[s] >> j) & 1]],
                                          truth[s][[j for j in range(14) if (present[s] >> j) & 1]])) for s in sample)
        ok_oracle = True
        for s in sample:
            got = t[s].cpu().numpy()
            pr = [bool((present[s] >> j) & 1) for j in range(14)]
            bufs = [got[j].copy() for j in range(14)]
            assert oracle.reconstruct(bufs, pr) == 0
            for j in range(14):
                if (wanted[k][s] >> j) & 1:
                    ok_oracle = ok_oracle and bool(np.array_equal(got[j], bufs[j]))
        checks[k] = {"wanted_equal_encoded_batch": ok_wanted, "unwanted_erased_keep_their_bytes": ok_unwanted,
                     "sampled_survivors_unchanged": ok_present, "sampled_wanted_equal_c_oracle": ok_oracle}

    def stats(k):
        v = times[k]
        w = 4 if k in ("full", "all") else int(k[1])
        return {"ms_median": round(float(np.median(v)), 4), "ms_min": round(float(np.min(v)), 4),
                "ms_max": round(float(np.max(v)), 4), "ms_rounds": [round(float(x), 4) for x in v],
                "shard_lengths_moved_per_stripe": 10 + w,
                "gib_per_s_moved_at_median": round((10 + w) * S * L / 2**30 / (float(np.median(v)) / 1e3), 1)}

    med = {k: float(np.median(v)) for k, v in times.items()}
    result = {
        "tool": "tools/bench_reconstruct_some.py", "lib": os.path.basename(H.LIB_PATH), "version": H.version(),
        "device": torch.cuda.get_device_name(0),
        "stripes": S, "shard_len": L, "shard_pad": args.shard_pad, "rounds": args.rounds, "erased_per_stripe": 4,
        "decode_kernel": H.lib.hec_decode_kernel_name(L).decode(),
        "some_kernel": B.reconstruct_some_kernel_name(L),
        **{k: stats(k) for k in legs},
        "ratio_w1_over_full_median": round(med["w1"] / med["full"], 4),
        "ratio_w2_over_full_median": round(med["w2"] / med["full"], 4),
        "ratio_w3_over_full_median": round(med["w3"] / med["full"], 4),
        "ratio_all_over_full_median": round(med["all"] / med["full"], 4),
        "w1_median_below_full_min": bool(med["w1"] < min(times["full"])),
        "all_median_within_full_min_max": bool(min(times["full"]) <= med["all"] <= max(times["full"])),
        "checks_after_the_clock": checks,
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(all(c.values()) for c in checks.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
