#!/usr/bin/env python3
"""Scrub rate of the fused verify against what a caller did before it.

On bench.py's own batch (4096 x 1 MiB-shard stripes, 64 KiB shard pad, device
resident, data from fill_stripes_splitmix, parity from encode_batch), in one
process and after warm-up, three legs alternate, the order flipped each round:

  (a) verify_batch: 14 shards read, one word per stripe written;
  (b) the caller's scrub without it: encode_batch_sep into a scratch parity
      tensor, then torch.equal against the stored parity (10 read + 4 written,
      then 8 read);
  (c) encode_batch, for reference (10 read + 4 written).

Timed with HIP events. After the clock: every word of the clean batch is 0,
and a batch with a seeded set of flipped bytes yields exactly the C oracle's
words (the flipped stripes and a seeded sample of clean ones go through the
oracle; the rest must be 0). Prints one JSON line; --out writes it to a file
(profiles/verify/).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes/s, MI355X datasheet
SEED_BASE = 0x5EED0000


def oracle_word(host14):
    """host14 [14, L] uint8 -> mismatch word of the stripe by the C oracle."""
    from oracle import corc
    L = host14.shape[1]
    bufs = [np.ascontiguousarray(host14[i]).copy() for i in range(10)] + [np.zeros(L, np.uint8) for _ in range(4)]
    corc.CReedSolomon(10, 4).encode(bufs)
    return sum(1 << j for j in range(4) if (bufs[10 + j] != host14[10 + j]).any())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--shard-len", type=int, default=1 << 20)
    ap.add_argument("--shard-pad", type=int, default=64 << 10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--flips", type=int, default=48)
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
    data, stored = t[:, :10], t[:, 10:]
    scratch = B.empty_stripes(S, 4, L, shard_pad=args.shard_pad)
    words = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()
    equal = [None]

    def leg_a():
        B.verify_batch(rs, t, mismatch=words)

    def leg_b():
        B.encode_batch_sep(rs, data, scratch)
        equal[0] = torch.equal(scratch, stored)

    def leg_c():
        B.encode_batch(rs, t)

    legs = {"a": leg_a, "b": leg_b, "c": leg_c}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()

    times = {k: [] for k in legs}
    for r in range(args.rounds):
        order = "abc" if r % 2 == 0 else "cba"
        for k in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            legs[k]()
            e1.record(stream)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    assert equal[0] is True, "leg (b) found the clean batch unequal"

    # ---- after the clock ----------------------------------------------------
    clean_words = words.cpu().numpy().view(np.uint32)
    clean_ok = bool((clean_words == 0).all())
    rng = np.random.default_rng(SEED_BASE)
    flips = sorted({(int(rng.integers(S)), int(rng.integers(14)), int(rng.integers(L))) for _ in range(args.flips)})
    for s, i, p in flips:
        t[s, i, p] ^= int(rng.integers(1, 256))
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = B.verify_batch(rs, t, mismatch=words, bad_stripes=bad).cpu().numpy().view(np.uint32)
    flipped = sorted({s for s, _, _ in flips})
    sample = sorted(set(flipped) | {int(s) for s in rng.integers(S, size=32)})
    want = np.zeros(S, dtype=np.uint32)
    for s in sample:
        want[s] = oracle_word(t[s].cpu().numpy())
    flips_ok = bool((got == want).all()) and int(bad.item()) == int((want != 0).sum())

    nbytes = 14 * L * S
    def stats(v):
        return {"ms_median": round(float(np.median(v)), 4), "ms_min": round(float(np.min(v)), 4),
                "ms_max": round(float(np.max(v)), 4), "ms_rounds": [round(float(x), 4) for x in v]}
    a_med = float(np.median(times["a"]))
    result = {
        "tool": "tools/bench_verify.py", "lib": os.path.basename(H.LIB_PATH), "version": H.version(),
        "device": torch.cuda.get_device_name(0),
        "stripes": S, "shard_len": L, "shard_pad": args.shard_pad, "rounds": args.rounds,
        "kernel": B.verify_kernel_name(L),
        "verify": dict(stats(times["a"]), GiBps_14_shards_read=round(nbytes / (a_med * 1e-3) / 2**30, 1),
                       fraction_of_8TBps=round(nbytes / (a_med * 1e-3) / HBM_PEAK, 4)),
        "encode_then_equal": stats(times["b"]),
        "encode": dict(stats(times["c"]),
                       GiBps_14_shards_moved=round(nbytes / (float(np.median(times["c"])) * 1e-3) / 2**30, 1)),
        "verify_faster_than_encode_then_equal_every_round": bool(all(a < b for a, b in zip(times["a"], times["b"]))),
        "ratio_b_over_a_median": round(float(np.median(times["b"])) / a_med, 3),
        "ratio_a_over_c_median": round(a_med / float(np.median(times["c"])), 3),
        "clean_words_all_zero": clean_ok,
        "seeded_flips": {"flips": len(flips), "stripes_flipped": len(flipped), "oracle_stripes": len(sample),
                         "words_equal_oracle": flips_ok, "bad_stripes": int(bad.item())},
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ok = clean_ok and flips_ok and result["verify_faster_than_encode_then_equal_every_round"]
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
