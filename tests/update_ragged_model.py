"""The ragged update in numpy -- TEST INFRASTRUCTURE ONLY.

include/hec.h (hec_gpu_update_ragged) is the contract: per stripe exactly
hec_gpu_update_batch's, with that stripe's own length, its place in three flat
arenas and U = update_mask & 0x3FF. The model cuts every stripe out of the
arenas by its descriptor and hands it, as a batch of one, to
update_model.updated_parity; nothing here repeats the arithmetic.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

import update_model

K, M = 10, 4
FIELDS = ("parity_offset", "parity_stride", "new_offset", "new_stride", "old_offset", "old_stride", "shard_len",
          "update_mask")


def shard_rows(arena: np.ndarray, offset: int, stride: int, length: int, shards: int) -> np.ndarray:
    """The [shards, length] bytes of one stripe of a flat arena (a copy)."""
    offset, stride, length = int(offset), int(stride), int(length)
    return np.stack([arena[offset + i * stride: offset + i * stride + length] for i in range(shards)])


def updated(parity: np.ndarray, old: Optional[np.ndarray], new: np.ndarray, descs) -> np.ndarray:
    """The flat parity arena after the call: parity / old (None: zero) / new are
    flat uint8 arenas, descs rows carry FIELDS. Only bytes [0, shard_len) of the
    four parity shards of stripes with U non-empty differ from ``parity``."""
    out = parity.copy()
    for d in descs:
        named = getattr(getattr(d, "dtype", None), "names", None)  # a structured row, or a plain tuple
        po, ps, no, ns, oo, os_, ln, mask = (int(d[f]) for f in FIELDS) if named else (int(x) for x in d)
        if mask & 0x3FF == 0:
            continue
        par = shard_rows(parity, po, ps, ln, M)[None]
        nw = shard_rows(new, no, ns, ln, K)[None]
        od = None if old is None else shard_rows(old, oo, os_, ln, K)[None]
        after = update_model.updated_parity(par, od, nw, [mask & 0x3FF])[0]
        for j in range(M):
            out[po + j * ps: po + j * ps + ln] = after[j]
    return out


def in_place_descs(descs, new_descs, masks):
    """What helyim_amd.batch.update_descs_in_place must give, written out per
    stripe: rows of FIELDS for stripes (offset, shard_stride, shard_len, _) of an
    in-place 14-shard arena and of a ten-shard arena of new data."""
    rows = []
    for d, nd, m in zip(descs, new_descs, masks):
        off, stride, ln = int(d[0]), int(d[1]), int(d[2])
        rows.append((off + 10 * stride, stride, int(nd[0]), int(nd[1]), off, stride, ln, int(m)))
    return rows


def round16(x: int) -> int:
    return (int(x) + 15) // 16 * 16


def arena_layout(lens, shards: int, slack, order=None, gap: int = 0, lead: int = 0):
    """Stripes of `shards` shards each laid out in a flat arena in `order`
    (default: index order), stripe s with stride round16(lens[s]) + slack[s],
    `gap` bytes between stripes and `lead` before the first -> (offsets,
    strides, arena bytes). Everything stays 16-byte aligned when slack, gap and
    lead are multiples of 16."""
    S = len(lens)
    off, strides, at = [0] * S, [0] * S, int(lead)
    for s in (range(S) if order is None else order):
        strides[s] = round16(lens[s]) + int(slack[s])
        off[s] = at
        at += shards * strides[s] + int(gap)
    return off, strides, at


def desc_rows(lens, masks, par, new, old=None):
    """Rows of FIELDS from (offsets, strides) pairs of the three arenas; without
    an old arena its fields are 0."""
    S = len(lens)
    oo, os_ = old if old is not None else ([0] * S, [0] * S)
    return [(par[0][s], par[1][s], new[0][s], new[1][s], oo[s], os_[s], int(lens[s]), int(masks[s])) for s in range(S)]
