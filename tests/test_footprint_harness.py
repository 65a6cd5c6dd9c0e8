"""The write-footprint helper (tests/footprint.py) checked against itself on
the CPU: the stand-in for the product is the C oracle writing straight into a
numpy arena. An unplanted run is clean; every planted fault, taken alone, is
found and classified."""
import numpy as np
import pytest

import footprint as F
from oracle import corc

K, M, N = 10, 4, 14


def _arenas(stripes, seed, slack=F.SLACK):
    rng = np.random.default_rng(seed)
    return [F.random_arena(n, rng) for n in F.arena_sizes(stripes, slack)]


def _views(arenas, st):
    return [arenas[a][o:o + st.L] for a, o in st.locs]


def oracle_encode(arenas, stripes, k=K, m=M, out_locs=None):
    """The stand-in product: parity of every stripe written into the arena in
    place. out_locs(s, j) -> (arena, offset) overrides where parity j of
    stripe s lands (a planted address fault)."""
    rs = corc.CReedSolomon(k, m)
    for s, st in enumerate(stripes):
        par = [np.zeros(st.L, np.uint8) for _ in range(m)]
        rs.encode([v.copy() for v in _views(arenas, st)[:k]] + par)
        for j in range(m):
            a, o = out_locs(s, j) if out_locs else st.locs[k + j]
            arenas[a][o:o + st.L] = par[j]


def oracle_reconstruct(arenas, stripes, present, k=K, m=M, data_only=False):
    rs = corc.CReedSolomon(k, m)
    for st, pr in zip(stripes, present):
        rs.reconstruct(_views(arenas, st), pr, data_only=data_only)  # writes the erased views in place


def _present(rows):
    return [[i not in erased for i in range(N)] for erased in rows]


# ---- layouts of the self-test ------------------------------------------------
L, S = 17, 3                    # a 1-byte tail after one full 16-byte vector
A = F.stripe_major(N, L, S, shard_stride=F.r16(L) + 16, gap=4096 + 32)   # padded, extra stripe gap
DATA = F.stripe_major(K, L, S, shard_stride=F.r16(L) + 48, gap=16)      # C: data stripe-major ...
PAR = F.shard_major(M, L, S, stripe_stride=F.r16(L) + 16, pad2=48, arena=1)  # ... parity shard-major, 2nd arena
ERASED = [(0, 3, 11), (1, 2, 4, 6, 12), (), (5, 13)]  # stripe 1: 9 present (skipped); stripe 2: all present
A4 = A._replace(S=4)


def test_layout_addresses_and_arena_sizes():
    assert A.off(2, 5) == F.SLACK + 2 * (14 * 48 + 4128) + 5 * 48
    assert PAR.off(1, 2) == F.SLACK + 1 * 48 + 2 * (3 * 48 + 48)
    assert A.sub(K, M).off(1, 0) == A.off(1, K) and A.sub(K, M).shards == M
    st = F.stripes_of(DATA, PAR)
    assert st[1].locs[0] == (0, DATA.off(1, 0)) and st[1].locs[K + 3] == (1, PAR.off(1, 3))
    assert F.arena_sizes(st) == [DATA.end + F.SLACK, PAR.end + F.SLACK]
    with pytest.raises(AssertionError, match="overlaps"):   # shard stride below L: the layout itself is wrong
        F.Plan(_arenas(st, 0), F.stripes_of(F.stripe_major(N, L, S, shard_stride=L - 1)))
    with pytest.raises(AssertionError, match="slack"):
        F.Plan(_arenas(st, 0), F.stripes_of(F.stripe_major(N, L, S, shard_stride=32, base=100)))


@pytest.mark.parametrize("k,m", [(10, 4), (3, 2)])
def test_unplanted_encode_is_clean(k, m):
    for lay in ([F.stripe_major(k + m, L, S, F.r16(L) + 16, gap=16)],
                [F.shard_major(k + m, 4099, S, 4099 + 3, pad2=5, base=F.SLACK + 3)],
                [F.stripe_major(k, L, S, F.r16(L) + 48), F.shard_major(m, L, S, F.r16(L), pad2=16, arena=1)]):
        st = F.stripes_of(*lay)
        arenas = _arenas(st, 1)
        plan = F.plan_encode(arenas, st, k, m)
        assert plan.verdict(arenas) is not None  # random parity slots are not the oracle's parity
        oracle_encode(arenas, st, k, m)
        F.assert_footprint(plan, arenas)
        assert all(r == [F.PRESENT] * k + [F.OUTPUT] * m for r in plan.roles)


@pytest.mark.parametrize("data_only", [False, True])
def test_unplanted_reconstruct_is_clean(data_only):
    st = F.stripes_of(A4)
    arenas = _arenas(st, 2)
    before = [a.copy() for a in arenas]
    plan = F.plan_reconstruct(arenas, st, K, M, _present(ERASED), data_only=data_only)
    assert plan.n_bad == 1
    assert plan.roles[1] == [F.SKIPPED] * N and plan.roles[2] == [F.PRESENT] * N
    assert plan.roles[0][11] == (F.DATA_ONLY_PARITY if data_only else F.OUTPUT) and plan.roles[0][3] == F.OUTPUT
    oracle_reconstruct(arenas, st, _present(ERASED), data_only=data_only)
    F.assert_footprint(plan, arenas)
    # only erased ranges of the two decodable stripes differ from the input
    changed = np.flatnonzero(arenas[0] != before[0])
    kinds = {plan.classify(0, int(o))[0] for o in changed}
    assert kinds == {F.OUTPUT}
    # the decode read the first ten present shards only: garbage in a surplus
    # survivor (stripe 3: shards 0..4, 6..10 are read; 11, 12 are surplus) changes nothing
    again = [a.copy() for a in before]
    plan.shard(again, 3, 12)[:] ^= 0xFF
    plan2 = F.plan_reconstruct(again, st, K, M, _present(ERASED), data_only=data_only)
    assert np.array_equal(plan2.shard(plan2.expected, 3, 5), plan.shard(plan.expected, 3, 5))
    if not data_only:
        assert np.array_equal(plan2.shard(plan2.expected, 3, 13), plan.shard(plan.expected, 3, 13))


def _encoded(seed=3):
    st = F.stripes_of(A)
    arenas = _arenas(st, seed)
    plan = F.plan_encode(arenas, st, K, M)
    oracle_encode(arenas, st)
    F.assert_footprint(plan, arenas)
    return plan, arenas


def test_planted_byte_past_the_end_of_an_output_shard():
    plan, arenas = _encoded()
    arenas[0][A.off(1, 11) + L] ^= 0x01        # between parity 1 and parity 2 of stripe 1
    v = plan.verdict(arenas)
    assert (v.kind, v.arena, v.offset) == (F.SHARD_GAP, 0, A.off(1, 11) + L), str(v)
    plan, arenas = _encoded()
    arenas[0][A.off(1, 13) + L] ^= 0x01        # after the stripe's last shard: between stripes 1 and 2
    v = plan.verdict(arenas)
    assert (v.kind, v.offset) == (F.STRIPE_GAP, A.off(1, 13) + L), str(v)
    assert "stripe gap" in str(v) and str(A.off(1, 13) + L) in str(v)


def test_planted_full_vector_store_at_a_tail():
    """L = 17: the second 16-byte vector of a shard owes one byte. A full
    store there leaves byte 16 right and changes the 15 bytes after the shard."""
    plan, arenas = _encoded()
    o = A.off(2, 10)
    arenas[0][o + 16:o + 32] = np.concatenate([arenas[0][o + 16:o + 17], np.full(15, 0, np.uint8)])
    before = plan.expected[0][o + 17:o + 32]
    assert before.any()  # the planted zeros differ from the random gap somewhere
    first = o + 17 + int(np.flatnonzero(before != 0)[0])
    v = plan.verdict(arenas)
    assert (v.kind, v.offset) == (F.SHARD_GAP, first), str(v)


def test_planted_output_strides_swapped():
    """Parity j of stripe s stored at s * shard_stride + j * stripe_stride:
    (0, 0) lands right; the slot of parity 1 of stripe 0 receives parity 0 of
    stripe 1 instead, which is the lowest offset that differs."""
    st = F.stripes_of(A)
    arenas = _arenas(st, 4, slack=3 * F.SLACK)  # room for the misplaced stores
    plan = F.plan_encode(arenas, st, K, M)
    par = A.sub(K, M)
    room = [len(a) for a in arenas]
    assert par.base + (S - 1) * par.shard_stride + (M - 1) * par.stripe_stride + L <= room[0]
    oracle_encode(arenas, st, out_locs=lambda s, j: (0, par.base + s * par.shard_stride + j * par.stripe_stride))
    v = plan.verdict(arenas)
    assert (v.kind, v.stripe, v.shard, v.byte) == (F.OUTPUT, 0, K + 1, 0), str(v)
    assert "stripe 0 shard 11 at byte 0" in str(v)


def test_planted_parity_written_with_the_data_strides():
    """Data stripe-major (pitch 80, stripes 816 apart), parity shard-major in a
    second arena (stripes 48 apart): parity stored with the data strides puts
    (0, 0) right and leaves (1, 0), 48 bytes on, unwritten."""
    st = F.stripes_of(DATA, PAR)
    arenas = _arenas(st, 5)
    plan = F.plan_encode(arenas, st, K, M)
    assert PAR.base + (S - 1) * DATA.stripe_stride + (M - 1) * DATA.shard_stride + L <= len(arenas[1])
    oracle_encode(arenas, st,
                  out_locs=lambda s, j: (1, PAR.base + s * DATA.stripe_stride + j * DATA.shard_stride))
    v = plan.verdict(arenas)
    assert (v.arena, v.kind, v.stripe, v.shard, v.byte) == (1, F.OUTPUT, 1, K, 0), str(v)


def _reconstructed(data_only=False, seed=6):
    st = F.stripes_of(A4)
    arenas = _arenas(st, seed)
    plan = F.plan_reconstruct(arenas, st, K, M, _present(ERASED), data_only=data_only)
    return plan, arenas, st


def test_planted_present_shard_rewritten():
    plan, arenas, st = _reconstructed()
    oracle_reconstruct(arenas, st, _present(ERASED))
    arenas[0][A4.off(3, 7) + 9] ^= 0x80
    v = plan.verdict(arenas)
    assert (v.kind, v.stripe, v.shard, v.byte) == (F.PRESENT, 3, 7, 9), str(v)
    assert str(v).startswith(f"arena 0 offset {A4.off(3, 7) + 9}: present shard (stripe 3 shard 7 at byte 9)")


def test_planted_skipped_stripe_touched():
    """Stripe 1 has 9 present: a product that 'rebuilds' it anyway (here: its
    erased slot 2 zeroed) is caught on that slot, as are its present shards."""
    plan, arenas, st = _reconstructed()
    oracle_reconstruct(arenas, st, _present(ERASED))
    F.assert_footprint(plan, arenas)
    keep = arenas[0][A4.off(1, 2):A4.off(1, 2) + L].copy()
    arenas[0][A4.off(1, 2):A4.off(1, 2) + L] = 0
    first = int(np.flatnonzero(keep != 0)[0])
    v = plan.verdict(arenas)
    assert (v.kind, v.stripe, v.shard, v.byte) == (F.SKIPPED, 1, 2, first), str(v)
    assert "skipped stripe (stripe 1 shard 2" in str(v)


def test_planted_all_present_stripe_touched():
    plan, arenas, st = _reconstructed()
    oracle_reconstruct(arenas, st, _present(ERASED))
    arenas[0][A4.off(2, 13) + L - 1] ^= 0x55  # stripe 2: every shard present, a no-op
    v = plan.verdict(arenas)
    assert (v.kind, v.stripe, v.shard, v.byte) == (F.PRESENT, 2, 13, L - 1), str(v)


def test_planted_missing_parity_written_under_data_only():
    """The plan is data_only, the stand-in runs a full reconstruct: stripe 0's
    erased parity 11 gets rebuilt where it had to stay as it was."""
    plan, arenas, st = _reconstructed(data_only=True)
    before = arenas[0][A4.off(0, 11):A4.off(0, 11) + L].copy()
    oracle_reconstruct(arenas, st, _present(ERASED), data_only=False)
    after = arenas[0][A4.off(0, 11):A4.off(0, 11) + L]
    first = int(np.flatnonzero(before != after)[0])
    v = plan.verdict(arenas)
    assert (v.kind, v.stripe, v.shard, v.byte) == (F.DATA_ONLY_PARITY, 0, 11, first), str(v)
    assert "data_only parity (stripe 0 shard 11" in str(v)


@pytest.mark.parametrize("where", ["leading", "last leading", "first trailing", "trailing"])
def test_planted_slack_byte(where):
    plan, arenas = _encoded()
    o = {"leading": 0, "last leading": A.base - 1, "first trailing": A.end, "trailing": len(arenas[0]) - 1}[where]
    arenas[0][o] ^= 0xFF
    v = plan.verdict(arenas)
    assert (v.kind, v.offset, v.stripe) == (F.SLACK_KIND, o, None), str(v)
    with pytest.raises(AssertionError, match=f"arena 0 offset {o}: slack"):
        F.assert_footprint(plan, arenas)


def test_failed_call_must_leave_the_arena_unchanged():
    st = F.stripes_of(A)
    arenas = _arenas(st, 7)
    before = [a.copy() for a in arenas]
    F.assert_unchanged(before, arenas, st)
    arenas[0][A.off(0, 12)] ^= 1
    with pytest.raises(AssertionError, match="present shard \\(stripe 0 shard 12 at byte 0\\)"):
        F.assert_unchanged(before, arenas, st)


def test_first_difference_is_the_lowest_offset_of_the_lowest_arena():
    st = F.stripes_of(DATA, PAR)
    arenas = _arenas(st, 8)
    plan = F.plan_encode(arenas, st, K, M)
    oracle_encode(arenas, st)
    F.assert_footprint(plan, arenas)
    arenas[1][5] ^= 1
    arenas[0][DATA.off(2, 9) + 4] ^= 1
    arenas[0][DATA.off(1, 0) + 3] ^= 1
    v = plan.verdict(arenas)
    assert (v.arena, v.kind, v.stripe, v.shard, v.byte) == (0, F.PRESENT, 1, 0, 3), str(v)
