#!/usr/bin/env python3
"""What the ragged correct costs against the ragged locate, and against the
strided masked correct on the same bytes.

tools/bench_ragged_scrub.py's method: one process, bench.py's batch (4096 x 1
MiB-shard stripes, 64 KiB shard pad, device resident, data from
fill_stripes_splitmix, parity from encode_batch), one shard of every stripe
marked absent (positions varied), warm-up, then the legs alternate with the
order flipped each round, HIP-event times around each call, medians and
ranges. 64 stripes can hold one flipped byte in a present shard; before each
leg, outside the clock, those 64 bytes are set to what the leg is measured on
(their originals for a clean leg, flipped for a dirty one), so a correct leg,
which restores them, sees them wrong again next round.

  (lc)   locate_corrupt_ragged, clean batch;
  (cc)   correct_ragged, clean batch;
  (l64)  locate_corrupt_ragged, the 64 dirty stripes;
  (c64)  correct_ragged, the same;
  (s64)  correct_present_batch on the same bytes;
  (rr64) reconstruct_corrected_ragged, the same;
  (rb64) reconstruct_corrected_batch, the same;
  (mix)  reconstruct_corrected_ragged on a config-5 batch: 2048 clean stripes,
         shard lengths log-uniform in 64 KiB..4 MiB (multiples of 16), 0..3
         shards of each marked absent; bytes moved per second (the scrub's
         reads, the decode's reads and its writes).

After the clock every leg's words are compared with what the seeded
construction implies, and verify_batch on the whole batch must be clean after
a last correct. A ragged call's time includes building and uploading its
maps. Criterion (as for the earlier correct kernels): the clean-batch
correct_ragged median lies inside the min..max of locate_corrupt_ragged over
the rounds. Prints one JSON line; --out writes it to a file
(profiles/ragged_correct/bench_ragged_correct.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_ragged_scrub import ALL, PEAK_BYTES_PER_S, SEED_BASE, expected_check  # noqa: E402

PAIRS = (("cc", "lc"), ("c64", "l64"), ("c64", "s64"), ("rr64", "rb64"))
DIRTY = ("l64", "c64", "s64", "rr64", "rb64")


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

    shard = L + args.shard_pad
    buf = torch.empty(S * 14 * shard, dtype=torch.uint8, device="cuda")
    t = buf.as_strided((S, 14, L), (14 * shard, shard, 1))
    B.fill_stripes_splitmix(t, 10, SEED_BASE)
    B.encode_batch(rs, t)
    one_lost = np.array([ALL & ~(1 << int(rng.integers(14))) for _ in range(S)], dtype=np.uint32)
    masks1 = torch.tensor(one_lost.view(np.int32), device="cuda")
    flipped = {}
    for s in rng.choice(S, size=min(64, S), replace=False):
        present = [i for i in range(14) if int(one_lost[s]) >> i & 1]
        flipped[int(s)] = (present[int(rng.integers(13))], int(rng.integers(L)))
    fs = torch.tensor(sorted(flipped), device="cuda")
    fc = torch.tensor([flipped[s][0] for s in sorted(flipped)], device="cuda")
    fp = torch.tensor([flipped[s][1] for s in sorted(flipped)], device="cuda")
    originals = t[fs, fc, fp].clone()

    def set_bytes(dirty):
        t[fs, fc, fp] = originals ^ 1 if dirty else originals

    d_one = np.zeros(S, dtype=B.desc_dtype())
    d_one["offset"] = np.arange(S, dtype=np.uint64) * np.uint64(14 * shard)
    d_one["shard_stride"], d_one["shard_len"], d_one["present_mask"] = shard, L, one_lost

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
    pop = [bin(int(m)).count("1") for m in mix_masks]
    mix_moved = int(sum(int(n) * (p + (0 if p == 14 else 10 + 14 - p)) for n, p in zip(lens, pop)))
    torch.cuda.synchronize()

    def stale(n):
        return torch.full((n,), -1, dtype=torch.int32, device="cuda")

    out = {k: (stale(S), stale(S), stale(S)) for k in ("lc", "cc", "l64", "c64", "s64", "rr64", "rb64")}
    out["mix"] = (stale(M), stale(M), stale(M))
    nbytes = {k: torch.zeros(1, dtype=torch.int64, device="cuda") for k in out}
    left = {k: torch.zeros(1, dtype=torch.int32, device="cuda") for k in out}

    def ragged_locate(k):
        return lambda: B.locate_corrupt_ragged(rs, buf, d_one, check=out[k][0], suspects=out[k][1])

    def ragged_correct(k):
        return lambda: B.correct_ragged(rs, buf, d_one, 2, check=out[k][0], suspects=out[k][1], uncorrected=left[k],
                                        corrected_bytes=nbytes[k])

    legs = {
        "lc": ragged_locate("lc"),
        "cc": ragged_correct("cc"),
        "l64": ragged_locate("l64"),
        "c64": ragged_correct("c64"),
        "s64": lambda: B.correct_present_batch(rs, t, masks1, 2, check=out["s64"][0], suspects=out["s64"][1],
                                               uncorrected=left["s64"], corrected_bytes=nbytes["s64"]),
        "rr64": lambda: B.reconstruct_corrected_ragged(rs, buf, d_one, 2, check=out["rr64"][0],
                                                       suspects=out["rr64"][1], use_masks=out["rr64"][2],
                                                       unrepaired=left["rr64"], corrected_bytes=nbytes["rr64"]),
        "rb64": lambda: B.reconstruct_corrected_batch(rs, t, masks1, 2, check=out["rb64"][0],
                                                      suspects=out["rb64"][1], use_masks=out["rb64"][2],
                                                      unrepaired=left["rb64"], corrected_bytes=nbytes["rb64"]),
        "mix": lambda: B.reconstruct_corrected_ragged(rs, mix, d_mix, 2, check=out["mix"][0], suspects=out["mix"][1],
                                                      use_masks=out["mix"][2], unrepaired=left["mix"],
                                                      corrected_bytes=nbytes["mix"]),
    }
    stream = torch.cuda.current_stream()
    calls = {k: 0 for k in legs}

    def run(k):
        set_bytes(k in DIRTY)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        h0 = time.perf_counter()
        legs[k]()
        h = (time.perf_counter() - h0) * 1e3
        e1.record(stream)
        e1.synchronize()
        calls[k] += 1
        return e0.elapsed_time(e1), h

    for _ in range(args.warmup):
        for k in legs:
            run(k)
    times = {k: [] for k in legs}
    host = {k: [] for k in legs}
    for r in range(args.rounds):
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            ms, h = run(k)
            times[k].append(ms)
            host[k].append(h)
    torch.cuda.synchronize()

    # after the clock: every leg's words and counters against the seeded construction
    def got(k, i):
        return out[k][i].cpu().numpy().view(np.uint32).tolist()

    zero = [0] * S
    chk64 = [expected_check(int(one_lost[s]), flipped[s][0]) if s in flipped else 0 for s in range(S)]
    sus64 = [1 << flipped[s][0] if s in flipped else 0 for s in range(S)]
    use = [int(m) for m in one_lost]
    n64 = len(flipped)
    words_ok = {
        "lc": got("lc", 0) == zero and got("lc", 1) == zero,
        "cc": got("cc", 0) == zero and got("cc", 1) == zero and int(nbytes["cc"].item()) == 0,
        "l64": got("l64", 0) == chk64 and got("l64", 1) == sus64,
        "mix": got("mix", 0) == [0] * M and got("mix", 2) == [int(m) for m in mix_masks] and
        int(nbytes["mix"].item()) == 0 and int(left["mix"].item()) == 0,
    }
    for k in ("c64", "s64", "rr64", "rb64"):
        words_ok[k] = (got(k, 0) == chk64 and got(k, 1) == sus64 and int(nbytes[k].item()) == n64 * calls[k] and
                       int(left[k].item()) == 0 and (k[0] != "r" or got(k, 2) == use))
    set_bytes(True)
    legs["c64"]()
    restored = bool((B.verify_batch(rs, t) == 0).all().item()) and bool((t[fs, fc, fp] == originals).all().item())

    def stats(v, h):
        return {"host_call_ms_median": round(float(np.median(h)), 4), "ms_median": round(float(np.median(v)), 4),
                "ms_min": round(float(np.min(v)), 4), "ms_max": round(float(np.max(v)), 4),
                "ms_rounds": [round(float(x), 4) for x in v]}

    result = {
        "tool": "tools/bench_ragged_correct.py", "lib": os.path.basename(H.LIB_PATH), "version": H.version(),
        "device": torch.cuda.get_device_name(0),
        "stripes": S, "shard_len": L, "shard_pad": args.shard_pad, "rounds": args.rounds, "flipped_stripes": n64,
        "mix_stripes": M, "mix_bytes_moved": mix_moved,
        "kernels": {"pass1": B.ragged_scrub_kernel_name(d_one), "pass1_mix": B.ragged_scrub_kernel_name(d_mix),
                    "strided_pass1": B.check_kernel_name(L)},
        "legs": {k: stats(times[k], host[k]) for k in legs},
    }
    rate = mix_moved / (float(np.median(times["mix"])) * 1e-3)
    result["legs"]["mix"].update(TBps_moved=round(rate / 1e12, 3), fraction_of_8TBps=round(rate / PEAK_BYTES_PER_S, 3))
    for a, b in PAIRS:
        med = float(np.median(times[a]))
        result["ratio_%s_over_%s_median" % (a, b)] = round(med / float(np.median(times[b])), 4)
        result["%s_median_inside_%s_range" % (a, b)] = bool(min(times[b]) <= med <= max(times[b]))
    result["words_match_construction"] = words_ok
    result["batch_clean_after_last_correct"] = restored
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if restored and all(words_ok.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
