#!/usr/bin/env python3
"""What the ragged update costs over the strided one, and what it saves
against a ragged re-encode.

One process, warm-up, then the legs of a group alternate with the order flipped
each round, HIP-event times (the workgroup map's upload included), medians and
min..max.

Uniform batch -- the bench's batch (4096 x 1 MiB-shard stripes, 64 KiB shard
pad), a second arena of new data, the old arena given, one changed shard a
stripe (a seeded choice per stripe):
  (strided)  update_batch_sep, the reference leg;
  (ragged)   update_ragged on the same bytes.
The ratio of the medians is recorded, and whether the ragged median lies inside
the strided leg's own min..max over the rounds.

Mixed batch -- config 5: 2048 stripes, shard lengths log-uniform in 64 KiB..
4 MiB (multiples of 16), in place, and a second arena of new data:
  (encode)                  encode_ragged, the reference leg: 14 shard lengths;
  (old_u1, old_u2, old_u3)  update_ragged with the old arena: 2|U| + 8;
  (new_u1)                  update_ragged without: |U| + 8.
The criterion, set before the first run: the median of old_u1 lies below the
minimum of encode's rounds (the bytes say 10/14). Nothing else is a threshold.

Host batch -- 1024 updates of 4 KiB shards with one changed shard, wall clock:
  (per_call)  1024 hec_rs_update calls, the reference leg;
  (batch)     one hec_rs_update_batch.

After the clock every update leg runs once more over a fresh parity; 16 seeded
stripes per leg are brought back and their parity compared with the C oracle's
encode of the old data XOR its encode of the masked delta. Prints one JSON
line; --out writes it to a file (profiles/update_ragged/bench_update_ragged.json).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED_BASE = 0x0DA7F000
K, M = 10, 4


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--shard-len", type=int, default=1 << 20)
    ap.add_argument("--shard-pad", type=int, default=64 << 10)
    ap.add_argument("--mix-stripes", type=int, default=2048)
    ap.add_argument("--mix-min", type=int, default=64 << 10)
    ap.add_argument("--mix-max", type=int, default=4 << 20)
    ap.add_argument("--host-updates", type=int, default=1024)
    ap.add_argument("--host-len", type=int, default=4096)
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

    rs = H.ReedSolomon(K, M)
    stream = torch.cuda.current_stream()
    rng = np.random.default_rng(SEED_BASE)

    def mask_words(order, u):
        words = np.zeros(len(order), dtype=np.uint32)
        for q in range(u):
            words |= np.uint32(1) << order[:, q].astype(np.uint32)
        return words

    def alternate(legs, run, clock):
        for _ in range(args.warmup):
            for k in legs:
                run(k)
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for r in range(args.rounds):
            for k in (legs if r % 2 == 0 else legs[::-1]):
                times[k].append(clock(lambda: run(k)))
        torch.cuda.synchronize()
        return times

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def wall_ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def stats(v, moved_bytes=None, units=None):
        out = {"ms_median": round(float(np.median(v)), 4), "ms_min": round(float(np.min(v)), 4),
               "ms_max": round(float(np.max(v)), 4), "ms_rounds": [round(float(x), 4) for x in v]}
        if units is not None:
            out["shard_lengths_moved_per_stripe"] = units
        if moved_bytes is not None:
            out["tb_per_s_moved_at_median"] = round(moved_bytes / 1e12 / (float(np.median(v)) / 1e3), 3)
        return out

    def oracle_parity(h_old, h_new, words, with_old):
        """Per sampled stripe ([10, L] arrays): the old data's parity XOR the encode of the masked delta."""
        out = []
        for o, w, m in zip(h_old, h_new, words):
            sel = ((int(m) >> np.arange(K)) & 1).astype(bool)[:, None]
            delta = np.where(sel, (o ^ w) if with_old else w, np.uint8(0))
            out.append(corc.encode_stripes(np.ascontiguousarray(o[None]))[0] ^
                       corc.encode_stripes(np.ascontiguousarray(delta[None]))[0])
        return out

    # ---- uniform batch ---------------------------------------------------------------
    S, L = args.stripes, args.shard_len
    if S < 16 or L < 16:
        ap.error("--stripes and --shard-len must be at least 16")
    shard = L + args.shard_pad
    buf = torch.empty(S * (K + M) * shard, dtype=torch.uint8, device="cuda")
    t = buf.as_strided((S, K + M, L), ((K + M) * shard, shard, 1))
    B.fill_stripes_splitmix(t, K, SEED_BASE)
    nbuf = torch.empty(S * K * shard, dtype=torch.uint8, device="cuda")
    new = nbuf.as_strided((S, K, L), (K * shard, shard, 1))
    B.fill_stripes_splitmix(new, K, SEED_BASE + 0x1000)
    B.encode_batch(rs, t)
    torch.cuda.synchronize()
    old, parity = t[:, :K], t[:, K:]
    order = np.stack([rng.permutation(K) for _ in range(S)])
    words_u = mask_words(order, 1)
    dwords_u = torch.tensor(words_u.view(np.int32), device="cuda")
    descs_u = np.zeros(S, dtype=B.desc_dtype())
    descs_u["offset"], descs_u["shard_stride"], descs_u["shard_len"] = np.arange(S) * (K + M) * shard, shard, L
    ndescs_u = np.zeros(S, dtype=B.desc_dtype())
    ndescs_u["offset"], ndescs_u["shard_stride"], ndescs_u["shard_len"] = np.arange(S) * K * shard, shard, L
    rows_u = B.update_descs_in_place(descs_u, ndescs_u, words_u)

    def uniform(k):
        if k == "strided":
            B.update_batch_sep(rs, old, new, parity, dwords_u)
        else:
            B.update_ragged(rs, buf, nbuf, buf, rows_u)

    t_uni = alternate(["strided", "ragged"], uniform, event_ms)
    sample = sorted(int(s) for s in rng.permutation(S)[:16])
    h_old = [old[s].cpu().numpy() for s in sample]
    h_new = [new[s].cpu().numpy() for s in sample]
    want = oracle_parity(h_old, h_new, words_u[sample], True)
    checks = {}
    for k in ("strided", "ragged"):
        B.encode_batch(rs, t)
        uniform(k)
        torch.cuda.synchronize()
        checks["uniform_" + k] = {"sampled_parity_equals_c_oracle": bool(all(
            np.array_equal(parity[s].cpu().numpy(), w) for s, w in zip(sample, want)))}
    uni_bytes = 10 * S * L
    med_s, med_r = float(np.median(t_uni["strided"])), float(np.median(t_uni["ragged"]))
    uniform_result = {
        "stripes": S, "shard_len": L, "shard_pad": args.shard_pad, "changed_shards_per_stripe": 1, "old_arena": True,
        "strided_kernel": B.update_kernel_name(L), "ragged_kernel": B.update_ragged_kernel_name(True),
        "strided": stats(t_uni["strided"], uni_bytes, 10), "ragged": stats(t_uni["ragged"], uni_bytes, 10),
        "ratio_ragged_over_strided_median": round(med_r / med_s, 4),
        "ragged_median_inside_strided_min_max": bool(min(t_uni["strided"]) <= med_r <= max(t_uni["strided"])),
    }
    del t, new, old, parity, buf, nbuf
    torch.cuda.empty_cache()

    # ---- mixed batch (config 5) ------------------------------------------------------
    MS = args.mix_stripes
    lens = np.exp(rng.uniform(np.log(args.mix_min), np.log(args.mix_max), MS)).astype(np.int64) // 16 * 16
    lens = lens.clip(args.mix_min, args.mix_max)
    strides = (lens + 255) // 256 * 256
    d_mix = np.zeros(MS, dtype=B.desc_dtype())
    d_mix["offset"] = np.concatenate([[0], np.cumsum((K + M) * strides)[:-1]])
    d_mix["shard_stride"], d_mix["shard_len"], d_mix["present_mask"] = strides, lens, 0x3FFF
    n_mix = np.zeros(MS, dtype=B.desc_dtype())
    n_mix["offset"] = np.concatenate([[0], np.cumsum(K * strides)[:-1]])
    n_mix["shard_stride"], n_mix["shard_len"] = strides, lens
    mix = torch.empty(int((K + M) * strides.sum()), dtype=torch.uint8, device="cuda")
    mix_new = torch.empty(int(K * strides.sum()), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(mix.view(1, -1), mix.numel(), SEED_BASE + 1)
    B.fill_splitmix(mix_new.view(1, -1), mix_new.numel(), SEED_BASE + 2)
    B.encode_ragged(rs, mix, d_mix)
    torch.cuda.synchronize()
    order_m = np.stack([rng.permutation(K) for _ in range(MS)])
    mix_legs = ["encode", "old_u1", "old_u2", "old_u3", "new_u1"]
    changed = {k: int(k.split("_u")[1]) for k in mix_legs[1:]}
    words_m = {k: mask_words(order_m, u) for k, u in changed.items()}
    rows_m = {k: B.update_descs_in_place(d_mix, n_mix, words_m[k]) for k in changed}
    units = {"encode": K + M, **{k: (2 * u if k.startswith("old") else u) + 2 * M for k, u in changed.items()}}

    def mixed(k):
        if k == "encode":
            B.encode_ragged(rs, mix, d_mix)
        else:
            B.update_ragged(rs, mix if k.startswith("old") else None, mix_new, mix, rows_m[k])

    t_mix = alternate(mix_legs, mixed, event_ms)
    sample_m = sorted(int(s) for s in rng.permutation(MS)[:16])

    def rows_of(tensor, off, stride, ln, shards):
        return np.stack([tensor[off + i * stride: off + i * stride + ln].cpu().numpy() for i in range(shards)])

    m_old = [rows_of(mix, int(d_mix["offset"][s]), int(strides[s]), int(lens[s]), K) for s in sample_m]
    m_new = [rows_of(mix_new, int(n_mix["offset"][s]), int(strides[s]), int(lens[s]), K) for s in sample_m]
    for k in mix_legs[1:]:
        B.encode_ragged(rs, mix, d_mix)
        mixed(k)
        torch.cuda.synchronize()
        want = oracle_parity(m_old, m_new, words_m[k][sample_m], k.startswith("old"))
        got = [rows_of(mix, int(d_mix["offset"][s]) + K * int(strides[s]), int(strides[s]), int(lens[s]), M)
               for s in sample_m]
        still = all(np.array_equal(rows_of(mix, int(d_mix["offset"][s]), int(strides[s]), int(lens[s]), K), o)
                    for s, o in zip(sample_m, m_old))
        checks["mixed_" + k] = {"sampled_parity_equals_c_oracle": bool(all(np.array_equal(g, w)
                                                                           for g, w in zip(got, want))),
                                "sampled_old_data_unchanged": bool(still)}
    total_len = int(lens.sum())
    med_m = {k: float(np.median(v)) for k, v in t_mix.items()}
    mixed_result = {
        "stripes": MS, "shard_len_min": int(lens.min()), "shard_len_max": int(lens.max()),
        "shard_len_sum": total_len, "encode_kernel": B.ragged_kernel_name(d_mix, False),
        **{k: stats(t_mix[k], units[k] * total_len, units[k]) for k in mix_legs},
        **{f"ratio_{k}_over_encode_median": round(med_m[k] / med_m["encode"], 4) for k in mix_legs[1:]},
        "expected_ratio_old_u1_from_bytes": round(10 / 14, 4),
        "old_u1_median_below_encode_min": bool(med_m["old_u1"] < min(t_mix["encode"])),
    }
    del mix, mix_new
    torch.cuda.empty_cache()

    # ---- host batch ------------------------------------------------------------------
    HS, HL = args.host_updates, args.host_len
    hrng = np.random.default_rng(SEED_BASE + 3)
    h_shards = [[hrng.integers(0, 256, HL, dtype=np.uint8) for _ in range(K + M)] for _ in range(HS)]
    which = hrng.integers(0, K, HS)
    h_news = [[hrng.integers(0, 256, HL, dtype=np.uint8) if c == which[s] else None for c in range(K)]
              for s in range(HS)]
    pristine = [[p.copy() for p in sh[K:]] for sh in h_shards]
    # the C ABI itself, the pointer arrays built once: the clock sees the library, not the Python mirror
    import ctypes
    n = K + M
    each = [((ctypes.c_void_p * n)(*[a.ctypes.data for a in sh]), (ctypes.c_size_t * n)(*([HL] * n)),
             (ctypes.c_void_p * K)(*[None if w is None else w.ctypes.data for w in nw]))
            for sh, nw in zip(h_shards, h_news)]
    all_ptrs = (ctypes.c_void_p * (HS * n))(*[a.ctypes.data for sh in h_shards for a in sh])
    all_lens = (ctypes.c_size_t * (HS * n))(*([HL] * (HS * n)))
    all_news = (ctypes.c_void_p * (HS * K))(*[None if w is None else w.ctypes.data for nw in h_news for w in nw])

    def host(k):
        if k == "per_call":
            for p, ln, nw in each:
                H.errors.check(H.lib.hec_rs_update(rs.handle, p, ln, nw, n))
        else:
            H.errors.check(H.lib.hec_rs_update_batch(rs.handle, all_ptrs, all_lens, all_news, HS, None))

    t_host = alternate(["per_call", "batch"], host, wall_ms)
    sample_h = sorted(int(s) for s in hrng.permutation(HS)[:16])
    for k in ("per_call", "batch"):
        for sh, par in zip(h_shards, pristine):
            for j in range(M):
                sh[K + j][:] = par[j]
        host(k)
        want = []
        for s in sample_h:
            sel = (np.arange(K) == which[s])[:, None]
            delta = np.where(sel, np.stack(h_shards[s][:K]) ^ np.stack([w if w is not None else np.zeros(HL, np.uint8)
                                                                        for w in h_news[s]]), np.uint8(0))
            want.append(np.stack(pristine[s]) ^ corc.encode_stripes(np.ascontiguousarray(delta[None]))[0])
        checks["host_" + k] = {"sampled_parity_equals_c_oracle": bool(all(
            np.array_equal(np.stack(h_shards[s][K:]), w) for s, w in zip(sample_h, want)))}
    host_result = {
        "updates": HS, "shard_len": HL, "changed_shards_per_update": 1, "clock": "wall (time.perf_counter)",
        "per_call": stats(t_host["per_call"]), "batch": stats(t_host["batch"]),
        "ratio_batch_over_per_call_median": round(float(np.median(t_host["batch"])) /
                                                  float(np.median(t_host["per_call"])), 4),
        "us_per_update_per_call": round(float(np.median(t_host["per_call"])) * 1e3 / HS, 2),
        "us_per_update_batch": round(float(np.median(t_host["batch"])) * 1e3 / HS, 2),
    }

    result = {
        "tool": "tools/bench_update_ragged.py", "lib": os.path.basename(H.LIB_PATH), "version": H.version(),
        "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
        "uniform": uniform_result, "mixed": mixed_result, "host": host_result,
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
