#!/usr/bin/env python3
"""What the ragged scrub costs against the strided scrub on the same bytes.

tools/bench_check.py's method: one process, bench.py's batch (4096 x 1 MiB-shard
stripes, 64 KiB shard pad, device resident, data from fill_stripes_splitmix,
parity from encode_batch), warm-up, then the legs alternate with the order
flipped each round, HIP-event times around each call, medians and ranges. The
yardstick of every ragged leg is the strided call on the same stripes in the
same process:

  (v)    verify_batch, bit-sliced;
  (rv)   verify_ragged, the same stripes as descriptors with full masks (the
         bit-sliced pick);
  (c1)   verify_present_batch with one shard of every stripe marked absent,
         positions varied from stripe to stripe;
  (rc1)  verify_ragged with the same masks (the table pick);
  (l64)  locate_corrupt_batch, 64 of the stripes holding one flipped byte;
  (rl64) locate_corrupt_ragged on the same stripes, full masks;
  (mix)  verify_ragged alone on a config-5 batch: 2048 stripes, shard lengths
         log-uniform in 64 KiB..4 MiB (multiples of 16), 0..3 shards of each
         marked absent; reported as bytes READ per second.

The 64 flipped bytes are in the batch from the start, so every leg sees the
same bytes; after the clock the words of every leg are compared with what the
seeded construction implies (a flipped data shard sets every spare bit, a
flipped spare shard its own, an absent one nothing; the mixed batch is clean).
A ragged call's time includes building and uploading its workgroup map, as a
caller pays it; host_call_ms is how long the call kept the host, the map
included (the event clock starts before it). Criterion (as for the earlier
scrub kernels): the ragged median lies inside the min..max of its strided
partner over the rounds. Prints one JSON line; --out writes it to a file
(profiles/ragged_scrub/bench_ragged_scrub.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED_BASE = 0x5EED0000
PEAK_BYTES_PER_S = 8e12
ALL = 0x3FFF
PAIRS = (("rv", "v"), ("rc1", "c1"), ("rl64", "l64"))


def spare_bits(mask):
    ids = [i for i in range(14) if mask >> i & 1]
    return ids[10:]


def expected_check(mask, flipped):
    """Check word (bits by shard index) of a stripe whose shard `flipped` holds one wrong byte."""
    if flipped is None or not mask >> flipped & 1:
        return 0
    E = spare_bits(mask)
    return 1 << flipped if flipped in E else sum(1 << e for e in E)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--shard-len", type=int, default=1 << 20)
    ap.add_argument("--shard-pad", type=int, default=64 << 10)
    ap.add_argument("--mix-stripes", type=int, default=2048)
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
    rng = np.random.default_rng(SEED_BASE)

    # the strided batch, in a buffer the descriptors can address
    shard = L + args.shard_pad
    buf = torch.empty(S * 14 * shard, dtype=torch.uint8, device="cuda")
    t = buf.as_strided((S, 14, L), (14 * shard, shard, 1))
    B.fill_stripes_splitmix(t, 10, SEED_BASE)
    B.encode_batch(rs, t)
    flipped = {}
    for s in rng.choice(S, size=min(64, S), replace=False):
        c, pos = int(rng.integers(14)), int(rng.integers(L))
        flipped[int(s)] = c
        t[int(s), c, pos] ^= 1
    one_lost = np.array([ALL & ~(1 << int(rng.integers(14))) for _ in range(S)], dtype=np.uint32)
    masks1 = torch.tensor(one_lost.view(np.int32), device="cuda")

    def descs_of(masks):
        d = np.zeros(S, dtype=B.desc_dtype())
        d["offset"] = np.arange(S, dtype=np.uint64) * np.uint64(14 * shard)
        d["shard_stride"], d["shard_len"], d["present_mask"] = shard, L, masks
        return d

    d_full, d_one = descs_of(np.full(S, ALL, dtype=np.uint32)), descs_of(one_lost)

    # the mixed batch: stripes back to back, 256-byte aligned, clean
    M = args.mix_stripes
    lens = np.exp(rng.uniform(np.log(64 << 10), np.log(4 << 20), M)).astype(np.int64) // 16 * 16
    lens = lens.clip(64 << 10, 4 << 20)
    strides = (lens + 255) // 256 * 256
    offs = np.concatenate([[0], np.cumsum(14 * strides)[:-1]])
    mix_masks = np.array([ALL & ~sum(1 << int(i) for i in rng.choice(14, size=int(rng.integers(4)), replace=False))
                          for _ in range(M)], dtype=np.uint32)
    d_mix = np.zeros(M, dtype=B.desc_dtype())
    d_mix["offset"], d_mix["shard_stride"], d_mix["shard_len"], d_mix["present_mask"] = offs, strides, lens, mix_masks
    mix = torch.empty(int(14 * strides.sum()), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(mix.view(1, -1), mix.numel(), SEED_BASE + 1)
    B.encode_ragged(rs, mix, d_mix)
    mix_read = int(sum(int(n) * bin(int(m)).count("1") for n, m in zip(lens, mix_masks)))
    torch.cuda.synchronize()

    def stale(n):
        return torch.full((n,), -1, dtype=torch.int32, device="cuda")

    out = {k: (stale(S), stale(S)) for k in ("v", "rv", "c1", "rc1", "l64", "rl64")}
    out["mix"] = (stale(M), stale(M))
    unchecked = torch.zeros(1, dtype=torch.int32, device="cuda")
    legs = {
        "v": lambda: B.verify_batch(rs, t, mismatch=out["v"][0]),
        "rv": lambda: B.verify_ragged(rs, buf, d_full, check=out["rv"][0], unchecked=unchecked),
        "c1": lambda: B.verify_present_batch(rs, t, masks1, check=out["c1"][0], unchecked=unchecked),
        "rc1": lambda: B.verify_ragged(rs, buf, d_one, check=out["rc1"][0], unchecked=unchecked),
        "l64": lambda: B.locate_corrupt_batch(rs, t, mismatch=out["l64"][0], suspects=out["l64"][1]),
        "rl64": lambda: B.locate_corrupt_ragged(rs, buf, d_full, check=out["rl64"][0], suspects=out["rl64"][1],
                                                unchecked=unchecked),
        "mix": lambda: B.verify_ragged(rs, mix, d_mix, check=out["mix"][0], unchecked=unchecked),
    }
    stream = torch.cuda.current_stream()
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()

    times = {k: [] for k in legs}
    host = {k: [] for k in legs}  # how long the call itself kept the host (a ragged call builds its map in it)
    for r in range(args.rounds):
        keys = list(legs) if r % 2 == 0 else list(legs)[::-1]
        for k in keys:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            h0 = time.perf_counter()
            legs[k]()
            host[k].append((time.perf_counter() - h0) * 1e3)
            e1.record(stream)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    torch.cuda.synchronize()

    # after the clock: every leg's words against the seeded construction
    def got(k, i):
        return out[k][i].cpu().numpy().view(np.uint32).tolist()

    full_chk = [expected_check(ALL, flipped.get(s)) for s in range(S)]
    one_chk = [expected_check(int(one_lost[s]), flipped.get(s)) for s in range(S)]
    sus = [1 << flipped[s] if s in flipped else 0 for s in range(S)]
    words_ok = {
        "v": got("v", 0) == [w >> 10 for w in full_chk],
        "rv": got("rv", 0) == full_chk,
        "c1": got("c1", 0) == one_chk,
        "rc1": got("rc1", 0) == one_chk,
        "l64": got("l64", 0) == [w >> 10 for w in full_chk] and got("l64", 1) == sus,
        "rl64": got("rl64", 0) == full_chk and got("rl64", 1) == sus,
        "mix": got("mix", 0) == [0] * M,
    }
    none_unchecked = int(unchecked.item()) == 0

    def stats(v, bytes_read, h):
        rate = bytes_read / (float(np.median(v)) * 1e-3)
        return {"host_call_ms_median": round(float(np.median(h)), 4), "ms_median": round(float(np.median(v)), 4),
                "ms_min": round(float(np.min(v)), 4),
                "ms_max": round(float(np.max(v)), 4), "ms_rounds": [round(float(x), 4) for x in v],
                "TBps_read": round(rate / 1e12, 3), "fraction_of_8TBps": round(rate / PEAK_BYTES_PER_S, 3)}

    read = {"v": 14 * L * S, "rv": 14 * L * S, "c1": 13 * L * S, "rc1": 13 * L * S, "l64": 14 * L * S,
            "rl64": 14 * L * S, "mix": mix_read}
    result = {
        "tool": "tools/bench_ragged_scrub.py", "lib": os.path.basename(H.LIB_PATH), "version": H.version(),
        "device": torch.cuda.get_device_name(0),
        "stripes": S, "shard_len": L, "shard_pad": args.shard_pad, "rounds": args.rounds, "flipped_stripes": len(flipped),
        "mix_stripes": M, "mix_bytes_read": mix_read,
        "kernels": {"v": B.verify_kernel_name(L), "c1": B.check_kernel_name(L), "rv": B.ragged_scrub_kernel_name(d_full),
                    "rc1": B.ragged_scrub_kernel_name(d_one), "mix": B.ragged_scrub_kernel_name(d_mix)},
        "legs": {k: stats(times[k], read[k], host[k]) for k in legs},
    }
    for ragged, strided in PAIRS:
        med = float(np.median(times[ragged]))
        result["ratio_%s_over_%s_median" % (ragged, strided)] = round(med / float(np.median(times[strided])), 4)
        result["%s_median_inside_%s_range" % (ragged, strided)] = bool(
            min(times[strided]) <= med <= max(times[strided]))
    result["words_match_construction"] = words_ok
    result["no_stripe_unchecked"] = none_unchecked
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if none_unchecked and all(words_ok.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
