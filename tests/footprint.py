"""Whole-arena write-footprint checks -- TEST INFRASTRUCTURE ONLY.

The parity tests prove that the bytes a coding call is meant to produce are
right. This module proves they are the ONLY bytes it touches: a call runs on
shards laid out inside one flat byte arena (or two: data and parity apart)
filled with seeded random bytes everywhere -- gaps, slack, erased slots,
outputs -- and the arena after the call must equal, byte for byte, an expected
image built from the arena's own input bytes with the C oracle.

    plan = footprint.plan_encode(arenas, stripes, k, m)        # before the call
    ... the product codes the arena(s) ...
    footprint.assert_footprint(plan, actual_arenas)            # every byte

A stripe is a ``Stripe(L, locs)``: shard i holds L bytes at ``locs[i] =
(arena index, byte offset)``. ``Layout`` describes the strided batches of
include/hec.h (shard (s, i) at base + s * stripe_stride + i * shard_stride) and
turns into stripes; ragged descriptors and per-call shard pointers are stripes
directly. On a mismatch the verdict names the first differing offset as slack,
shard gap, stripe gap, an output ("stripe s shard i at byte b"), a present
shard, a skipped stripe or a parity slot ``data_only`` must leave alone.
"""
from __future__ import annotations

import bisect
import ctypes
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from oracle import corc

SLACK = 4096  # least untouched bytes before the first and after the last byte of any layout

# what a shard's bytes are to the call under test
OUTPUT = "output"                 # the call must write exactly the oracle's bytes
PRESENT = "present shard"         # read (or ignored), never written
SKIPPED = "skipped stripe"        # fewer than k present: nothing of the stripe is written
DATA_ONLY_PARITY = "data_only parity"  # erased parity under data_only: left as it was
SLACK_KIND, SHARD_GAP, STRIPE_GAP = "slack", "shard gap", "stripe gap"


def r16(x: int) -> int:
    return (x + 15) // 16 * 16


class Stripe(NamedTuple):
    L: int
    locs: Tuple[Tuple[int, int], ...]  # per shard: (arena index, byte offset)


class Layout(NamedTuple):
    """hec.h's strided batch: shard (s, i) at base + s*stripe_stride + i*shard_stride."""
    base: int
    stripe_stride: int
    shard_stride: int
    L: int
    S: int
    shards: int
    arena: int = 0

    def off(self, s: int, i: int) -> int:
        return self.base + s * self.stripe_stride + i * self.shard_stride

    @property
    def end(self) -> int:
        return self.off(self.S - 1, self.shards - 1) + self.L

    def sub(self, first: int, count: int) -> "Layout":
        """Shards [first, first + count) of every stripe (an in-place batch's data or parity)."""
        return self._replace(base=self.base + first * self.shard_stride, shards=count)

    def moved(self, base: int, arena: int = None) -> "Layout":
        return self._replace(base=base, arena=self.arena if arena is None else arena)


def stripe_major(shards: int, L: int, S: int, shard_stride: int, gap: int = 0, base: int = SLACK,
                 arena: int = 0) -> Layout:
    """[S][shards][shard_stride] plus `gap` more bytes between stripes."""
    return Layout(base, shards * shard_stride + gap, shard_stride, L, S, shards, arena)


def shard_major(shards: int, L: int, S: int, stripe_stride: int, pad2: int = 0, base: int = SLACK,
                arena: int = 0) -> Layout:
    """[shards][S][stripe_stride] plus `pad2` more bytes between shards."""
    return Layout(base, stripe_stride, S * stripe_stride + pad2, L, S, shards, arena)


def stripes_of(*layouts: Layout) -> List[Stripe]:
    """Stripes whose shards are the layouts' shards side by side (data layout
    then parity layout; one layout for an in-place batch)."""
    S, L = layouts[0].S, layouts[0].L
    assert all(la.S == S and la.L == L for la in layouts)
    return [Stripe(L, tuple((la.arena, la.off(s, i)) for la in layouts for i in range(la.shards)))
            for s in range(S)]


def arena_sizes(stripes: Sequence[Stripe], slack: int = SLACK) -> List[int]:
    """Bytes each arena needs: the last byte any shard touches plus `slack`."""
    n = 1 + max(a for st in stripes for a, _ in st.locs)
    ends = [0] * n
    for st in stripes:
        for a, o in st.locs:
            ends[a] = max(ends[a], o + st.L)
    return [e + slack for e in ends]


def random_arena(nbytes: int, rng: np.random.Generator) -> np.ndarray:
    """Seeded random bytes everywhere: a constant poison would hide a stale or
    shifted copy of poison."""
    return rng.integers(0, 256, nbytes, dtype=np.uint8)


class Verdict(NamedTuple):
    arena: int
    offset: int
    kind: str
    stripe: Optional[int]
    shard: Optional[int]
    byte: Optional[int]
    got: int
    want: int

    def __str__(self):
        where = f"arena {self.arena} offset {self.offset}: "
        at = f"stripe {self.stripe} shard {self.shard} at byte {self.byte}"
        if self.kind == OUTPUT:
            what = at
        elif self.stripe is not None:
            what = f"{self.kind} ({at})"
        else:
            what = self.kind
        return f"{where}{what}; got 0x{self.got:02x}, expected 0x{self.want:02x}"


class Plan:
    """Stripes, what each shard is to the call, and the expected image."""

    def __init__(self, arenas: Sequence[np.ndarray], stripes: Sequence[Stripe], slack: int = SLACK):
        self.stripes = list(stripes)
        self.roles = [[PRESENT] * len(st.locs) for st in self.stripes]
        self.expected = [np.array(a, dtype=np.uint8, copy=True) for a in arenas]
        self.n_bad = 0
        # per arena: shard ranges sorted by offset; they must not overlap and
        # must leave the slack free, or the layout under test is itself wrong
        self.ranges = [[] for _ in arenas]
        for s, st in enumerate(self.stripes):
            for i, (a, o) in enumerate(st.locs):
                self.ranges[a].append((o, o + st.L, s, i))
        for a, rr in enumerate(self.ranges):
            rr.sort()
            for x, y in zip(rr, rr[1:]):
                assert x[1] <= y[0], f"arena {a}: stripe {x[2]} shard {x[3]} overlaps stripe {y[2]} shard {y[3]}"
            if rr:
                assert rr[0][0] >= slack and rr[-1][1] + slack <= len(arenas[a]), f"arena {a}: slack below {slack}"
        self.starts = [[r[0] for r in rr] for rr in self.ranges]

    def shard(self, arenas: Sequence[np.ndarray], s: int, i: int) -> np.ndarray:
        """View of stripe s shard i inside `arenas`."""
        a, o = self.stripes[s].locs[i]
        return arenas[a][o:o + self.stripes[s].L]

    def classify(self, arena: int, offset: int):
        """-> (kind, stripe, shard, byte) of one arena offset."""
        rr = self.ranges[arena]
        j = bisect.bisect_right(self.starts[arena], offset) - 1
        if j >= 0 and offset < rr[j][1]:
            _, _, s, i = rr[j]
            return self.roles[s][i], s, i, offset - rr[j][0]
        if j < 0 or j + 1 >= len(rr):
            return SLACK_KIND, None, None, None
        # between two shards: of one stripe, or of two
        return (SHARD_GAP if rr[j][2] == rr[j + 1][2] else STRIPE_GAP), None, None, None

    def verdict(self, actual: Sequence[np.ndarray]) -> Optional[Verdict]:
        """None when every byte of every arena equals the expected image, else
        the first differing offset (lowest arena, lowest offset), classified."""
        assert len(actual) == len(self.expected)
        for a, (got, want) in enumerate(zip(actual, self.expected)):
            got = np.asarray(got)
            assert got.dtype == np.uint8 and got.shape == want.shape, f"arena {a}: shape or dtype changed"
            diff = np.flatnonzero(got != want)
            if diff.size:
                o = int(diff[0])
                return Verdict(a, o, *self.classify(a, o), int(got[o]), int(want[o]))
        return None


def plan_encode(arenas: Sequence[np.ndarray], stripes: Sequence[Stripe], k: int, m: int) -> Plan:
    """Expected image of an encode: the arenas as they are, with exactly the
    parity ranges (shards k..k+m of every stripe) overwritten by the C oracle's
    encode of the data ranges."""
    plan = Plan(arenas, stripes)
    rs = corc.CReedSolomon(k, m)
    for s, st in enumerate(plan.stripes):
        assert len(st.locs) == k + m
        bufs = [plan.shard(arenas, s, i).copy() for i in range(k)] + [np.zeros(st.L, np.uint8) for _ in range(m)]
        rs.encode(bufs)
        for j in range(m):
            plan.shard(plan.expected, s, k + j)[:] = bufs[k + j]
            plan.roles[s][k + j] = OUTPUT
    return plan


def present_flags(mask: int, n: int) -> List[bool]:
    """hec.h present masks: bit i set = shard i present; bits from n up are ignored."""
    return [bool((int(mask) >> i) & 1) for i in range(n)]


def plan_reconstruct(arenas: Sequence[np.ndarray], stripes: Sequence[Stripe], k: int, m: int,
                     present: Sequence[Sequence[bool]], data_only: bool = False) -> Plan:
    """Expected image of a reconstruct: the arenas as they are, with exactly
    the erased shard ranges overwritten by the C oracle's reconstruct of the
    same shard bytes and presence flags (it reads the first k present shards;
    surplus survivors hold whatever the arena holds and come back unchanged).
    Stripes with every shard present, or with fewer than k present (counted in
    plan.n_bad), contribute no change; with data_only, erased parity neither."""
    plan = Plan(arenas, stripes)
    rs = corc.CReedSolomon(k, m)
    n = k + m
    for s, st in enumerate(plan.stripes):
        pr = [bool(p) for p in present[s]]
        assert len(st.locs) == n and len(pr) == n
        if sum(pr) == n:
            continue
        if sum(pr) < k:
            plan.n_bad += 1
            plan.roles[s] = [SKIPPED] * n
            continue
        bufs = [plan.shard(arenas, s, i).copy() for i in range(n)]
        assert rs.reconstruct(bufs, pr, data_only=data_only) == 0
        for i in range(n):
            if pr[i]:
                continue
            if data_only and i >= k:
                plan.roles[s][i] = DATA_ONLY_PARITY
                continue
            plan.shard(plan.expected, s, i)[:] = bufs[i]
            plan.roles[s][i] = OUTPUT
    return plan


def assert_footprint(plan: Plan, actual: Sequence[np.ndarray], note=None) -> None:
    v = plan.verdict(actual)
    assert v is None, f"{v}" + (f"  [{note}]" if note is not None else "")


def assert_unchanged(before: Sequence[np.ndarray], actual: Sequence[np.ndarray], stripes: Sequence[Stripe],
                     note=None) -> None:
    """A call that failed by contract: no byte of any arena differs."""
    assert_footprint(Plan(before, stripes), actual, note)


# ---- device and host arenas of the GPU suites -------------------------------------
def present_of(masks, n):
    return [present_flags(mk, n) for mk in masks]


def to_device(arenas):
    import torch
    devs = [torch.from_numpy(a).cuda() for a in arenas]
    assert all(d.data_ptr() % 256 == 0 for d in devs)  # the layout's own offsets decide the alignment
    return devs


def to_host(devs):
    import torch
    torch.cuda.synchronize()
    return [d.cpu().numpy() for d in devs]


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream


HOST_ARENA = 3 << 20
HOST_PATHS = ("pinned zero copy", "pageable pinned slots", "pageable copy2d")


class HostArenas:
    """Two pinned and two pageable buffers (64-byte aligned) the host cases
    carve their arenas from."""

    def __init__(self):
        import torch
        self.pinned_t = [torch.empty(HOST_ARENA, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.pinned = [t.numpy() for t in self.pinned_t]
        self.raw = [np.empty(HOST_ARENA + 64, np.uint8) for _ in range(2)]
        self.pageable = [r[(-r.ctypes.data) % 64:][:HOST_ARENA] for r in self.raw]

    def take(self, path, stripes, rng):
        """Arenas for `stripes` on this path, filled with seeded random bytes;
        -> (live arenas the call works on, a copy of them before the call)."""
        bufs = self.pinned if path == HOST_PATHS[0] else self.pageable
        live = []
        for sz, b in zip(arena_sizes(stripes), bufs):
            assert sz <= HOST_ARENA and b.ctypes.data % 64 == 0
            b[:sz] = random_arena(sz, rng)
            live.append(b[:sz])
        return live, [a.copy() for a in live]


class host_path:
    """Select one of the three host paths; the setting is restored on exit."""

    def __init__(self, path):
        self.path = path

    def __enter__(self):
        import helyim_amd as H
        assert H.lib.hec_set_host_zero_copy(0 if self.path == HOST_PATHS[2] else 1) == 0
        return self

    def __exit__(self, *exc):
        import helyim_amd as H
        H.lib.hec_set_host_zero_copy(1)

    def check_view(self, live, lay):
        """The pinned arena is coded zero-copy, everything else is staged."""
        import helyim_amd as H
        z = ctypes.c_int(7)
        p = live[lay.arena].ctypes.data + lay.base
        assert H.lib.hec_host_zero_copy_view(p, lay.end - lay.base, ctypes.byref(z)) == 0
        assert z.value == (1 if self.path == HOST_PATHS[0] else 0), (self.path, lay)
