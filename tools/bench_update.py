#!/usr/bin/env python3
"""What folding a few changed shards into the parity saves against re-encoding.

The bench's batch (4096 x 1 MiB-shard stripes, 64 KiB shard pad, device
resident, data from fill_stripes_splitmix, parity from encode_batch) and a
second arena of new data shards. One process, warm-up, then the legs alternate
with the order flipped each round, HIP-event times, medians and min..max.

  (encode)              encode_batch of the whole batch: 14 shard lengths a stripe;
  (old_u1, old_u2, old_u3)   update_batch_sep with the old arena, 1, 2, 3 changed
                        shards a stripe (a seeded choice per stripe): 2|U| + 8;
  (new_u1, new_u5, new_u10)  update_batch_sep without an old arena: |U| + 8.

The expectation from bytes alone is 10/14 of the encode's time for old_u1. The
criterion is relative: the median of old_u1 lies below the minimum of encode's
rounds. Nothing else is a threshold.

After the clock the parity is encoded afresh and every update leg runs once
more; 16 seeded stripes per leg are brought back and their parity compared with
the C oracle's encode of the old data XOR its encode of the masked delta, and
the data arenas of those stripes with what they held. Prints one JSON line;
--out writes it to a file (profiles/update/bench_update.json).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED_BASE = 0x0DA7E000
K, M = 10, 4


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
    rs = H.ReedSolomon(K, M)
    t = B.empty_stripes(S, K + M, L, shard_pad=args.shard_pad)
    B.fill_stripes_splitmix(t, K, SEED_BASE)
    new = B.empty_stripes(S, K, L, shard_pad=args.shard_pad)
    B.fill_stripes_splitmix(new, K, SEED_BASE + 0x1000)
    B.encode_batch(rs, t)
    torch.cuda.synchronize()
    old, parity = t[:, :K], t[:, K:]
    stream = torch.cuda.current_stream()

    rng = np.random.default_rng(SEED_BASE)
    order = np.stack([rng.permutation(K) for _ in range(S)])  # seeded order: the first |U| shards change

    def mask_words(u):
        words = np.zeros(S, dtype=np.uint32)
        for q in range(u):
            words |= np.uint32(1) << order[:, q].astype(np.uint32)
        return words

    legs = ["encode", "old_u1", "old_u2", "old_u3", "new_u1", "new_u5", "new_u10"]
    changed = {k: int(k.split("_u")[1]) for k in legs[1:]}
    words = {k: mask_words(u) for k, u in changed.items()}
    dwords = {k: torch.tensor(v.view(np.int32), device="cuda") for k, v in words.items()}
    units = {"encode": K + M, **{k: (2 * u if k.startswith("old") else u) + 2 * M for k, u in changed.items()}}

    def leg(k):
        if k == "encode":
            B.encode_batch(rs, t)
        else:
            B.update_batch_sep(rs, old if k.startswith("old") else None, new, parity, dwords[k])

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

    # after the clock: a fresh parity, each update leg once, sampled stripes against the C oracle
    sample = sorted(int(s) for s in rng.permutation(S)[:16])
    h_old = np.ascontiguousarray(old[sample].cpu().numpy())
    h_new = np.ascontiguousarray(new[sample].cpu().numpy())
    fresh = corc.encode_stripes(h_old)
    checks = {}
    for k in legs[1:]:
        B.encode_batch(rs, t)
        leg(k)
        torch.cuda.synchronize()
        sel = ((words[k][sample][:, None] >> np.arange(K)[None, :]) & 1).astype(bool)[:, :, None]
        delta = np.where(sel, (h_old ^ h_new) if k.startswith("old") else h_new, np.uint8(0))
        want = fresh ^ corc.encode_stripes(np.ascontiguousarray(delta))
        checks[k] = {"sampled_parity_equals_c_oracle": bool(np.array_equal(parity[sample].cpu().numpy(), want)),
                     "sampled_old_and_new_data_unchanged": bool(np.array_equal(old[sample].cpu().numpy(), h_old) and
                                                                np.array_equal(new[sample].cpu().numpy(), h_new))}

    def stats(k):
        v = times[k]
        return {"ms_median": round(float(np.median(v)), 4), "ms_min": round(float(np.min(v)), 4),
                "ms_max": round(float(np.max(v)), 4), "ms_rounds": [round(float(x), 4) for x in v],
                "shard_lengths_moved_per_stripe": units[k],
                "tb_per_s_moved_at_median": round(units[k] * S * L / 1e12 / (float(np.median(v)) / 1e3), 3)}

    med = {k: float(np.median(v)) for k, v in times.items()}
    result = {
        "tool": "tools/bench_update.py", "lib": os.path.basename(H.LIB_PATH), "version": H.version(),
        "device": torch.cuda.get_device_name(0),
        "stripes": S, "shard_len": L, "shard_pad": args.shard_pad, "rounds": args.rounds,
        "encode_kernel": H.lib.hec_encode_kernel_name(L).decode(),
        "update_kernel": B.update_kernel_name(L),
        **{k: stats(k) for k in legs},
        **{f"ratio_{k}_over_encode_median": round(med[k] / med["encode"], 4) for k in legs[1:]},
        "expected_ratio_old_u1_from_bytes": round(10 / 14, 4),
        "old_u1_median_below_encode_min": bool(med["old_u1"] < min(times["encode"])),
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
