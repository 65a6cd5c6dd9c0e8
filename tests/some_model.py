"""Expected image of a reconstruct-some call -- TEST INFRASTRUCTURE ONLY.

include/hec.h (hec_gpu_reconstruct_some_batch) is the contract: per stripe,
with E the erased shards and W = want & E, exactly the shards of W get the
bytes a full reconstruct gives them; an erased shard outside W, a survivor and
a gap keep theirs; a stripe with W empty is a no-op that is not counted, even
with fewer than k shards present; a stripe with fewer than k present and W
non-empty is skipped and counted.

The image is built as tests/footprint.py builds its own -- from the arena's
bytes with the C oracle -- by starting from ``footprint.plan_reconstruct`` (every
erased shard an output) and putting every erased slot outside W back to the
bytes the arena held. The roles are marked, so a verdict names an "unwanted
erased shard" or a "no-op stripe" instead of an output.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

import footprint as F

UNWANTED = "unwanted erased shard"  # erased, not in W: left as it was
NOOP = "no-op stripe"               # W empty: nothing of the stripe is read, written or counted

ALL = 0xFFFFFFFF


def wanted_erased(present: Sequence[bool], want: int) -> List[int]:
    """W: the erased shards the want word names, ascending."""
    return [i for i, p in enumerate(present) if not p and (int(want) >> i) & 1]


def plan_reconstruct_some(arenas: Sequence[np.ndarray], stripes: Sequence[F.Stripe], k: int, m: int,
                          present: Sequence[Sequence[bool]], wants: Sequence[int]) -> F.Plan:
    """plan_reconstruct narrowed to W. plan.n_bad counts the stripes with fewer
    than k present and W non-empty; plan.n_noop_short the ones with fewer than
    k present and W empty, which a call must NOT count."""
    assert len(wants) == len(stripes)
    plan = F.plan_reconstruct(arenas, stripes, k, m, present)
    plan.n_noop_short = 0
    n = k + m
    for s in range(len(plan.stripes)):
        pr = [bool(p) for p in present[s]]
        w = wanted_erased(pr, wants[s])
        if sum(pr) == n:
            continue
        if not w:
            if sum(pr) < k:
                plan.n_bad -= 1
                plan.n_noop_short += 1
            for i in range(n):
                if not pr[i]:
                    plan.shard(plan.expected, s, i)[:] = plan.shard(arenas, s, i)
            plan.roles[s] = [NOOP] * n
            continue
        if sum(pr) < k:
            continue  # footprint's SKIPPED, counted
        for i in range(n):
            if not pr[i] and i not in w:
                plan.shard(plan.expected, s, i)[:] = plan.shard(arenas, s, i)
                plan.roles[s][i] = UNWANTED
    return plan


def assert_counted(plan: F.Plan, counted: int, note=None) -> None:
    """The call's bad-stripe counter against the model's."""
    tail = f"  [{note}]" if note is not None else ""
    if counted == plan.n_bad:
        return
    if plan.n_noop_short and counted == plan.n_bad + plan.n_noop_short:
        raise AssertionError(f"no-op stripe counted: {counted} counted, {plan.n_bad} have fewer than k shards "
                             f"present and want an erased shard ({plan.n_noop_short} more want none){tail}")
    raise AssertionError(f"{counted} stripes counted, expected {plan.n_bad}{tail}")


def every_pair(n: int = 14, max_erased: int = 4):
    """Every (present mask, W) with 1 to max_erased erasures and every subset W
    of the erased shards, the empty one included: 19,320 pairs for n = 14."""
    from itertools import combinations
    out = []
    full = (1 << n) - 1
    for e in range(1, max_erased + 1):
        for erased in combinations(range(n), e):
            mask = full
            for i in erased:
                mask &= ~(1 << i)
            for sub in range(1 << e):
                w = 0
                for q in range(e):
                    if (sub >> q) & 1:
                        w |= 1 << erased[q]
                out.append((mask, w))
    return out
