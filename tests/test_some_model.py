"""tests/some_model.py checked against a stand-in reconstruct some (the C
oracle, no GPU): the clean stand-in matches the model byte for byte, and each
planted fault is caught and named."""
import numpy as np
import pytest

import footprint as F
import some_model as M
from oracle import corc

K, MP, N = 10, 4, 14
L = 100
FULL = (1 << N) - 1


def _mask(*erased):
    m = FULL
    for i in erased:
        m &= ~(1 << i)
    return m


# stripe: (present mask, want word)
CASES = [
    (_mask(2, 5, 11, 13), 1 << 5),                      # one of four
    (_mask(0, 12), (1 << 0) | (1 << 12)),               # all of two
    (_mask(3, 7, 9), (1 << 9) | (1 << 4) | (1 << 20)),  # one of three, plus a present shard's bit and a stray one
    (_mask(1, 6, 8, 10), 0),                            # W empty by an empty word
    (_mask(4), 1 << 2),                                 # W empty: only a present shard is named
    (FULL, M.ALL),                                      # all present
    (_mask(0, 1, 2, 3, 4), 1 << 3),                     # 9 present, W non-empty: counted
    (_mask(5, 6, 7, 8, 9), 1 << 0),                     # 9 present, W empty: a no-op, not counted
    (_mask(2, 5, 11, 13), M.ALL),                       # every want bit
]


def _setup(seed=11):
    rng = np.random.default_rng(seed)
    lay = F.stripe_major(N, L, len(CASES), F.r16(L) + 16, 48)
    stripes = F.stripes_of(lay)
    arenas = [F.random_arena(sz, rng) for sz in F.arena_sizes(stripes)]
    present = [F.present_flags(m, N) for m, _ in CASES]
    wants = [w for _, w in CASES]
    return arenas, stripes, present, wants


def stand_in(arenas, stripes, present, wants, fault=None):
    """A reconstruct some built from the oracle's full reconstruct. fault:
    "unwanted written" stores every erased shard; "wanted unwritten" leaves the
    last wanted shard of a stripe out; "other row" stores the first unwanted
    erased shard's bytes in a wanted slot; "noop counted" counts every stripe
    with fewer than k present. Returns the counter."""
    rs = corc.CReedSolomon(K, MP)
    counted = 0
    for s, st in enumerate(stripes):
        pr = present[s]
        w = M.wanted_erased(pr, wants[s])
        if sum(pr) < K:
            counted += 1 if (w or fault == "noop counted") else 0
            continue
        if sum(pr) == N or not w:
            continue
        view = lambda i: arenas[st.locs[i][0]][st.locs[i][1]:st.locs[i][1] + st.L]
        bufs = [view(i).copy() for i in range(N)]
        assert rs.reconstruct(bufs, pr) == 0
        unwanted = [i for i in range(N) if not pr[i] and i not in w]
        store = list(w)
        if fault == "unwanted written":
            store += unwanted
        if fault == "wanted unwritten":
            store = store[:-1]
        for i in store:
            view(i)[:] = bufs[unwanted[0]] if fault == "other row" and unwanted and i == w[0] else bufs[i]
    return counted


def test_clean_stand_in_matches_the_model():
    arenas, stripes, present, wants = _setup()
    plan = M.plan_reconstruct_some(arenas, stripes, K, MP, present, wants)
    assert plan.n_bad == 1 and plan.n_noop_short == 1
    assert plan.roles[0][5] == F.OUTPUT and plan.roles[0][2] == M.UNWANTED and plan.roles[0][0] == F.PRESENT
    assert plan.roles[3] == [M.NOOP] * N and plan.roles[7] == [M.NOOP] * N and plan.roles[6] == [F.SKIPPED] * N
    before = [a.copy() for a in arenas]
    counted = stand_in(arenas, stripes, present, wants)
    F.assert_footprint(plan, arenas)
    M.assert_counted(plan, counted)
    # the image differs from the input exactly in the wanted erased shards
    changed = {(s, i) for s in range(len(stripes)) for i in range(N)
               if not np.array_equal(plan.shard(before, s, i), plan.shard(plan.expected, s, i))}
    assert changed == {(0, 5), (1, 0), (1, 12), (2, 9), (8, 2), (8, 5), (8, 11), (8, 13)}


def test_every_want_bit_is_the_full_reconstruct():
    arenas, stripes, present, _ = _setup()
    some = M.plan_reconstruct_some(arenas, stripes, K, MP, present, [M.ALL] * len(stripes))
    full = F.plan_reconstruct(arenas, stripes, K, MP, present)
    assert all(np.array_equal(a, b) for a, b in zip(some.expected, full.expected))
    assert some.n_bad == full.n_bad == 2 and some.n_noop_short == 0


def _planted(fault):
    arenas, stripes, present, wants = _setup()
    plan = M.plan_reconstruct_some(arenas, stripes, K, MP, present, wants)
    counted = stand_in(arenas, stripes, present, wants, fault)
    return plan, arenas, counted


def test_planted_unwanted_slot_written():
    plan, arenas, _ = _planted("unwanted written")
    v = plan.verdict(arenas)
    assert v is not None and v.kind == M.UNWANTED and (v.stripe, v.shard) == (0, 2)
    assert "unwanted erased shard (stripe 0 shard 2" in str(v)


def test_planted_wanted_slot_left_unwritten():
    plan, arenas, _ = _planted("wanted unwritten")
    v = plan.verdict(arenas)
    assert v is not None and v.kind == F.OUTPUT and (v.stripe, v.shard) == (0, 5)
    assert "stripe 0 shard 5 at byte" in str(v)


def test_planted_wanted_slot_holds_another_row():
    plan, arenas, _ = _planted("other row")
    v = plan.verdict(arenas)
    assert v is not None and v.kind == F.OUTPUT and (v.stripe, v.shard) == (0, 5)


def test_planted_noop_stripe_counted():
    plan, arenas, counted = _planted("noop counted")
    F.assert_footprint(plan, arenas)  # the bytes are right; only the counter is not
    with pytest.raises(AssertionError, match="no-op stripe counted"):
        M.assert_counted(plan, counted)


def test_every_pair_count():
    pairs = M.every_pair()
    assert len(pairs) == len(set(pairs)) == 19320
    assert all(10 <= bin(m).count("1") <= 13 and w & m == 0 for m, w in pairs)
