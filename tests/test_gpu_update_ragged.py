"""Ragged update on the GPU (include/hec.h hec_gpu_update_ragged,
hec_rs_update_batch) against tests/update_ragged_model.py, bit for bit. The
device cases run on whole arenas of seeded random bytes -- slack up to the
stride, gaps, a parity that is no codeword's -- and compare every byte of every
arena with an expected image (tests/footprint.py): the old and new arenas
unchanged, the parity arena different only in [0, shard_len) of the parity
shards of the stripes whose mask names a shard."""
import ctypes
from typing import NamedTuple, Optional

import numpy as np
import pytest

import footprint as F
import update_model
import update_ragged_model as R

pytestmark = pytest.mark.gpu

K, MP = 10, 4
HIGH = 0xFFFFFC00  # mask bits that mean nothing
# every mask: 1024 stripes of two lengths alternating (two column ranges, the
# second partial, and one partial range); stripe s has mask (s + 512) % 1024, so
# the stripe without a workgroup sits in the middle of the batch
EVERY_S, EVERY_LENS = 1 << K, (4096 + 48, 1000)
LENGTHS = (1, 15, 16, 17, 4095, 4096, 4097, 4096 + 48, 8192 + 5, 12288)
OLD = pytest.mark.parametrize("has_old", [True, False], ids=["old", "no old"])


def every_mask_batch():
    lens = [EVERY_LENS[s % 2] for s in range(EVERY_S)]
    masks = [(s + EVERY_S // 2) % EVERY_S for s in range(EVERY_S)]
    return lens, masks


def map_entries(lens, masks):
    """Workgroup map entries hec_gpu_update_ragged builds: one per 4 KiB column
    range of every stripe with U non-empty."""
    return sum(-(-ln // 4096) for ln, m in zip(lens, masks) if m & 0x3FF)


class Batch(NamedTuple):
    arenas: list           # numpy arenas, seeded random bytes
    old: Optional[int]     # arena indices
    new: int
    par: int
    rows: list             # descriptor rows (R.FIELDS)
    stripes: list          # F.Stripe per stripe: its shards in every arena
    first_par: int         # index of parity shard 0 among a stripe's locs


def seeded_masks(rng, S):
    """1 to 10 bits a stripe."""
    out = []
    for _ in range(S):
        bits = rng.permutation(K)[: int(rng.integers(1, K + 1))]
        out.append(int(sum(1 << int(b) for b in bits)))
    return out


def build(kind, lens, masks, rng, has_old, slack=None):
    """A batch on fresh arenas. kind: "in place" (old data and parity in one
    arena of 14-shard stripes, hec_stripe_desc's layout, through
    update_descs_in_place), "separate" (three arenas, three different strides),
    "permuted" (the new and old arenas in other stripe orders than the parity
    arena) or "gaps" (bytes between the stripes of every arena)."""
    import helyim_amd.batch as B
    S = len(lens)
    slack = slack or [16 * (1 + (7 * s) % 17) for s in range(S)]  # 16 to 272 bytes up to the stride
    lead = F.SLACK
    if kind == "in place":
        a = R.arena_layout(lens, 14, slack, lead=lead)
        n = R.arena_layout(lens, K, [s + 16 for s in slack], lead=lead)
        descs = np.array([(a[0][s], a[1][s], lens[s], 0x3FFF) for s in range(S)], dtype=B.desc_dtype())
        rows = B.update_descs_in_place(descs, [(n[0][s], n[1][s], lens[s], 0) for s in range(S)], masks)
        rows = [tuple(int(x) for x in r) for r in rows]
        sizes = [a[2] + F.SLACK, n[2] + F.SLACK]
        stripes = [F.Stripe(lens[s], tuple((0, a[0][s] + i * a[1][s]) for i in range(14)) +
                            tuple((1, n[0][s] + c * n[1][s]) for c in range(K))) for s in range(S)]
        arenas = [F.random_arena(sz, rng) for sz in sizes]
        if not has_old:
            rows = [r[:4] + (0, 0) + r[6:] for r in rows]
        return Batch(arenas, 0 if has_old else None, 1, 0, rows, stripes, K)
    order_new = order_old = None
    gap = 0
    if kind == "permuted":
        order_new, order_old = [int(x) for x in rng.permutation(S)], [int(x) for x in rng.permutation(S)]
    elif kind == "gaps":
        gap = 4096 + 112
    else:
        assert kind == "separate", kind
    p = R.arena_layout(lens, MP, slack, gap=gap, lead=lead)
    n = R.arena_layout(lens, K, [s + 32 for s in slack], order=order_new, gap=gap and 208, lead=lead)
    o = R.arena_layout(lens, K, [s + 64 for s in slack], order=order_old, gap=gap and 48, lead=lead)
    rows = R.desc_rows(lens, masks, p[:2], n[:2], o[:2] if has_old else None)
    sizes = [p[2] + F.SLACK, n[2] + F.SLACK] + ([o[2] + F.SLACK] if has_old else [])
    stripes = []
    for s in range(S):
        locs = tuple((1, n[0][s] + c * n[1][s]) for c in range(K))
        if has_old:
            locs += tuple((2, o[0][s] + c * o[1][s]) for c in range(K))
        stripes.append(F.Stripe(lens[s], locs + tuple((0, p[0][s] + j * p[1][s]) for j in range(MP))))
    arenas = [F.random_arena(sz, rng) for sz in sizes]
    return Batch(arenas, 2 if has_old else None, 1, 0, rows, stripes, len(stripes[0].locs) - MP)


def plan_of(b: Batch):
    """Expected image: the arenas as they are, the parity arena the model's."""
    plan = F.Plan(b.arenas, b.stripes)
    plan.expected[b.par] = R.updated(b.arenas[b.par], None if b.old is None else b.arenas[b.old], b.arenas[b.new], b.rows)
    for s, r in enumerate(b.rows):
        if r[7] & 0x3FF:
            for j in range(MP):
                plan.roles[s][b.first_par + j] = F.OUTPUT
    return plan


def launch(rs, b: Batch, devs, rows=None):
    import helyim_amd.batch as B
    B.update_ragged(rs, None if b.old is None else devs[b.old], devs[b.new], devs[b.par], b.rows if rows is None else rows)


def check(b: Batch, note, rows=None):
    """One call, every byte of every arena against the plan."""
    import helyim_amd as H
    rs = H.ReedSolomon(K, MP)
    plan = plan_of(b)
    devs = F.to_device(b.arenas)
    launch(rs, b, devs, rows)
    F.assert_footprint(plan, F.to_host(devs), note)
    return plan


@OLD
def test_lengths_across_lane_tail_and_range_edges_in_one_batch(gpu, has_old):
    rng = np.random.default_rng(0x7A60 + has_old)
    lens = list(LENGTHS)
    slack = [16, 272, 32, 48, 64, 256, 80, 96, 112, 128]  # bytes up to the stride, poisoned like everything else
    b = build("separate", lens, seeded_masks(rng, len(lens)), rng, has_old, slack=slack)
    assert [r[1] - R.round16(r[6]) for r in b.rows] == slack
    plan = check(b, "mixed lengths")
    assert (plan.expected[b.par] != b.arenas[b.par]).any()


@OLD
def test_every_mask(gpu, has_old):
    """All 1024 mask words over two lengths; the stripe with the empty word owns
    no workgroup, so its neighbours' first_block does not count it."""
    rng = np.random.default_rng(0x7A70 + has_old)
    lens, masks = every_mask_batch()
    assert sorted(masks) == list(range(EVERY_S)) and masks[EVERY_S // 2] == 0
    b = build("in place", lens, masks, rng, has_old, slack=[16 + 16 * (s % 3) for s in range(EVERY_S)])
    plan = check(b, "every mask")
    # the expected image moves every stripe's parity but the one with the empty mask
    for s in (0, 1, EVERY_S // 2 - 1, EVERY_S // 2, EVERY_S // 2 + 1, EVERY_S - 1):
        moved = any((plan.shard(plan.expected, s, b.first_par + j) != plan.shard(b.arenas, s, b.first_par + j)).any()
                    for j in range(MP))
        assert moved == (s != EVERY_S // 2), s


def test_bits_from_ten_up_are_ignored(gpu):
    rng = np.random.default_rng(0x7A80)
    lens = [4096 + 48, 1000, 17, 4099, 64, 8192]
    masks = seeded_masks(rng, len(lens))
    masks[2] = 0
    b = build("separate", lens, masks, rng, True)
    noisy = [r[:7] + (r[7] | HIGH,) for r in b.rows]
    assert noisy[2][7] == HIGH
    check(b, "high mask bits", rows=noisy)  # the plan is the plain masks'


@OLD
@pytest.mark.parametrize("kind", ["in place", "separate", "permuted", "gaps"])
def test_layouts_and_footprint(gpu, kind, has_old):
    rng = np.random.default_rng(0x7A90 + 2 * ["in place", "separate", "permuted", "gaps"].index(kind) + has_old)
    lens = [4096 + 48, 1000, 17, 4099, 8192, 33]
    masks = seeded_masks(rng, len(lens))
    masks[4] = 0
    b = build(kind, lens, masks, rng, has_old)
    strides = {(r[1], r[3], r[5]) for r in b.rows}
    if kind != "in place":
        assert all(len({p, n, o}) == 3 for p, n, o in strides)  # three different strides a stripe
    check(b, kind)


def ragged_arena(lens, rng, slack=48):
    """An in-place ragged arena (hec_stripe_desc rows) of random bytes."""
    import helyim_amd.batch as B
    a = R.arena_layout(lens, 14, [slack] * len(lens), gap=32, lead=F.SLACK)
    descs = np.array([(a[0][s], a[1][s], lens[s], 0x3FFF) for s in range(len(lens))], dtype=B.desc_dtype())
    return F.random_arena(a[2] + F.SLACK, rng), descs


def test_progressive_encode_over_zeroed_parity(gpu):
    """Three calls without d_old over a partition of 0..9 per stripe, the new
    arena being the stripes' own data shards: hec_gpu_encode_ragged's bytes."""
    import torch

    import helyim_amd as H
    import helyim_amd.batch as B
    rng = np.random.default_rng(0x7AA0)
    rs = H.ReedSolomon(K, MP)
    lens = [1000, 4096, 4096 + 48, 17, 12288 + 5]
    arena, descs = ragged_arena(lens, rng)
    for d in descs:  # zeroed parity inside the shards; the slack keeps its random bytes
        for j in range(MP):
            at = int(d["offset"]) + (K + j) * int(d["shard_stride"])
            arena[at: at + int(d["shard_len"])] = 0
    owner = rng.integers(0, 3, (len(lens), K))
    want = torch.from_numpy(arena).cuda()
    B.encode_ragged(rs, want, descs)
    got = torch.from_numpy(arena).cuda()
    for part in range(3):
        masks = [int(sum(1 << c for c in range(K) if owner[s][c] == part)) for s in range(len(lens))]
        rows = B.update_descs_in_place(descs, descs, masks)  # new data = the arena's own data shards
        B.update_ragged(rs, None, got, got, rows)
    torch.cuda.synchronize()
    assert (want.cpu().numpy() != arena).any()
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())


def test_round_trip_with_the_scrub(gpu):
    """Update, commit on the host, verify_ragged: zero words. A delta byte
    flipped between the update and the commit shows."""
    import torch

    import helyim_amd as H
    import helyim_amd.batch as B
    rng = np.random.default_rng(0x7AB0)
    rs = H.ReedSolomon(K, MP)
    lens = [1000, 4096 + 48, 17, 8192, 4099, 100]
    S = len(lens)
    arena, descs = ragged_arena(lens, rng)
    n = R.arena_layout(lens, K, [16] * S, lead=F.SLACK)
    new = F.random_arena(n[2] + F.SLACK, rng)
    masks = seeded_masks(rng, S)
    masks[3] = 0
    dev = torch.from_numpy(arena).cuda()
    B.encode_ragged(rs, dev, descs)
    rows = B.update_descs_in_place(descs, [(n[0][s], n[1][s], lens[s], 0) for s in range(S)], masks)
    B.update_ragged(rs, dev, torch.from_numpy(new).cuda(), dev, rows)
    torch.cuda.synchronize()
    after = dev.cpu().numpy()

    def commit(image, new_bytes):
        out = image.copy()
        for s in range(S):
            for c in range(K):
                if (masks[s] >> c) & 1:
                    to, frm = int(descs["offset"][s]) + c * int(descs["shard_stride"][s]), n[0][s] + c * n[1][s]
                    out[to: to + lens[s]] = new_bytes[frm: frm + lens[s]]
        return out

    words = B.verify_ragged(rs, torch.from_numpy(commit(after, new)).cuda(), descs)
    assert not words.cpu().numpy().any()
    # the caller commits other bytes than it folded in: stripe 1's first changed shard, one byte
    flipped = new.copy()
    c = (masks[1] & -masks[1]).bit_length() - 1
    flipped[n[0][1] + c * n[1][1] + 4100] ^= 0x40
    words = B.verify_ragged(rs, torch.from_numpy(commit(after, flipped)).cuda(), descs).cpu().numpy()
    assert words[1] != 0 and not np.delete(words, 1).any()


def test_six_calls_back_to_back_pass_the_metadata_slots(gpu):
    """More calls than the four metadata slots on one stream with no
    synchronise between them, every call another batch; then one check."""
    import helyim_amd as H
    rs = H.ReedSolomon(K, MP)
    rng = np.random.default_rng(0x7AC0)
    kinds = ["separate", "in place", "gaps", "permuted", "separate", "in place"]
    batches, plans, devs = [], [], []
    for i, kind in enumerate(kinds):
        lens = [int(x) for x in rng.choice([17, 1000, 4096, 4099, 8192 + 5, 4096 + 48], size=3 + i)]
        b = build(kind, lens, seeded_masks(rng, len(lens)), rng, has_old=i % 2 == 0)
        batches.append(b)
        plans.append(plan_of(b))
        devs.append(F.to_device(b.arenas))
    for b, d in zip(batches, devs):
        launch(rs, b, d)
    for i, (plan, d) in enumerate(zip(plans, devs)):
        F.assert_footprint(plan, F.to_host(d), f"call {i}")


@OLD
def test_nothing_to_do_writes_nothing(gpu, has_old):
    import helyim_amd as H
    rs = H.ReedSolomon(K, MP)
    rng = np.random.default_rng(0x7AD0 + has_old)
    one = build("separate", [4096 + 48], [0x204], rng, has_old)
    check(one, "one stripe")
    lens = [1000, 4096 + 48, 17]
    for masks, rows_of in (([0, HIGH, 0], lambda b: b.rows), ([1, 2, 4], lambda b: [])):
        b = build("separate", lens, masks, rng, has_old)
        devs = F.to_device(b.arenas)
        launch(rs, b, devs, rows_of(b))
        F.assert_unchanged(b.arenas, F.to_host(devs), b.stripes, "all masks empty" if rows_of(b) else "empty batch")


# ---- hec_rs_update_batch ---------------------------------------------------------------
HOST_S = 64
HOST_LENS = (1, 100, 1000, 4096, 4099, 65536 + 7)


def host_stripes(rng, k, m, S=HOST_S, lens=HOST_LENS):
    """[(shards, new_data)]: seeded lengths, 0 to 3 changed shards a stripe, the
    stripes without a change interleaved; random parity (no codeword's)."""
    out = []
    for s in range(S):
        ln = int(lens[int(rng.integers(0, len(lens)))])
        n_changed = 0 if s % 5 == 2 else int(rng.integers(1, min(3, k) + 1))
        which = set(int(c) for c in rng.permutation(k)[:n_changed])
        shards = [rng.integers(0, 256, ln, dtype=np.uint8) for _ in range(k + m)]
        news = [rng.integers(0, 256, ln, dtype=np.uint8) if c in which else None for c in range(k)]
        out.append((shards, news))
    return out


def copy_of(stripes):
    return [([a.copy() for a in sh], [None if w is None else w.copy() for w in nw]) for sh, nw in stripes]


def check_host_batch(k, m, seed, lens=HOST_LENS):
    import helyim_amd as H
    rs = H.ReedSolomon(k, m)
    rng = np.random.default_rng(seed)
    before = host_stripes(rng, k, m, lens=lens)
    assert sum(all(w is None for w in nw) for _sh, nw in before) >= HOST_S // 5
    assert {sum(w is not None for w in nw) for _sh, nw in before} == set(range(min(3, k) + 1))
    batched, single = copy_of(before), copy_of(before)
    rs.update_batch(batched)
    for sh, nw in single:
        rs.update(sh, nw)
    for s, ((sh0, nw0), (sh1, nw1), (sh2, _nw2)) in enumerate(zip(before, batched, single)):
        mask = sum(1 << c for c in range(k) if nw0[c] is not None)
        ln = sh0[0].size
        old = np.stack(sh0[:k])[None]
        new = np.stack([w if w is not None else np.zeros(ln, np.uint8) for w in nw0])[None]
        want = update_model.updated_parity(np.stack(sh0[k:])[None], old, new, [mask], k, m)[0]
        for j in range(m):
            assert np.array_equal(sh1[k + j], want[j]), (s, j, ln, hex(mask))
            assert np.array_equal(sh1[k + j], sh2[k + j]), (s, j, ln, hex(mask))
        for c in range(k):  # old, new and untouched shards: as they were
            assert np.array_equal(sh1[c], sh0[c]), (s, c)
            assert nw0[c] is None or np.array_equal(nw1[c], nw0[c]), (s, c)


def test_host_batch_against_per_call_updates_and_the_model(gpu):
    check_host_batch(K, MP, 0x7AE0)


def test_host_batch_through_copies(gpu):
    import helyim_amd as H
    assert H.lib.hec_set_host_zero_copy(0) == 0
    try:
        check_host_batch(K, MP, 0x7AE1)
    finally:
        assert H.lib.hec_set_host_zero_copy(1) == 0


@pytest.mark.parametrize("k,m", [(5, 5), (3, 2)])
def test_host_batch_other_codecs_loop(gpu, k, m):
    check_host_batch(k, m, 0x7AE2 + k, lens=(1, 100, 1000, 4099))


def test_host_batch_of_one_stripe_and_bad_index(gpu):
    """One active stripe (its descriptor rides in the kernel arguments), and a
    failing stripe behind valid ones: nothing written, its index reported."""
    import helyim_amd as H
    rs = H.ReedSolomon(K, MP)
    rng = np.random.default_rng(0x7AF0)
    before = host_stripes(rng, K, MP, S=3, lens=(4099,))
    before[0] = (before[0][0], [None] * K)
    before[2] = (before[2][0], [None] * K)
    assert any(w is not None for w in before[1][1])
    got, single = copy_of(before), copy_of(before)
    rs.update_batch(got)
    rs.update(*single[1])
    for s in range(3):
        for i in range(K + MP):
            assert np.array_equal(got[s][0][i], single[s][0][i]), (s, i)
    assert any((got[1][0][K + j] != before[1][0][K + j]).any() for j in range(MP))
    bad = copy_of(before)
    bad[2][0][K + 1] = np.zeros(4098, np.uint8)
    with pytest.raises(H.IncorrectShardSize) as e:
        rs.update_batch(bad)
    assert e.value.stripe == 2
    for s in range(2):
        for i in range(K + MP):
            assert np.array_equal(bad[s][0][i], before[s][0][i]), (s, i)
