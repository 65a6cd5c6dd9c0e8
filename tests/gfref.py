"""Batched plain GF(2^8) reference and the every-present-mask image -- TEST
INFRASTRUCTURE ONLY.

ref_encode is the parity of a whole batch in numpy: the parity rows of
rs_oracle.build_matrix through rs_oracle.mul_rows (one 256-entry table lookup
per coefficient) over the flattened batch. torch_encode is the same lookup in
torch, for batches that live on the device and are too large to copy back: the
oracle's 256 x 256 product table indexed with the data bytes, XORed over the
inputs, a chunk of stripes at a time. device_codewords is a batch of seeded
random stripes with torch_encode's parity, built on the device.

all_masks_case builds the image the every-mask sweeps share: 2^(k+m) stripes,
stripe s with present mask s. It needs no reconstruct oracle: upstream (and
include/hec.h) decode from the first k present shards in index order only, so
in every decodable stripe the erased slots are poisoned, every surplus
survivor (a present shard after the first k present ones) is overwritten with
garbage, and the expected image has the erased slots back at their codeword
bytes and the garbage untouched. A kernel that reads any other survivor, or
the wrong plan of one mask, fails on that stripe. tests/test_gfref.py pins
ref_encode, torch_encode and this construction against the C oracle on the CPU.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from oracle import rs_oracle as O

POISON = 0xA5
SLACK = 4096  # garbage kept before and after a sweep's image on the device


@functools.lru_cache(maxsize=None)
def parity_rows(k: int, m: int) -> np.ndarray:
    rows = O.build_matrix(k, k + m)[k:]
    rows.setflags(write=False)
    return rows


def ref_encode(k: int, m: int, data: np.ndarray) -> np.ndarray:
    """data[S, k, L] -> parity[S, m, L] (numpy, rs_oracle's matrix and tables)."""
    S, kk, L = data.shape
    assert kk == k and data.dtype == np.uint8
    flat = [np.ascontiguousarray(data[:, i]).reshape(-1) for i in range(k)]
    outs = O.mul_rows(parity_rows(k, m), flat)
    return np.stack([o.reshape(S, L) for o in outs], axis=1)


def torch_encode(k: int, m: int, data, out=None, max_index_bytes: int = 1 << 29):
    """data[S, k, L] (uint8 torch tensor, any strides, any device) ->
    parity[S, m, L], written into `out` when given (any strides). The int64
    index tensor of a chunk of stripes stays at or below max_index_bytes."""
    import torch
    S, kk, L = data.shape
    assert kk == k and data.dtype == torch.uint8
    if out is None:
        out = torch.empty((S, m, L), dtype=torch.uint8, device=data.device)
    assert tuple(out.shape) == (S, m, L) and out.dtype == torch.uint8
    rows = parity_rows(k, m)
    # tabs[i][r] = the 256 products of coefficient (r, i)
    tabs = torch.from_numpy(np.ascontiguousarray(O.MUL_TABLE[rows.T])).to(data.device)  # [k, m, 256]
    step = max(1, max_index_bytes // (8 * max(L, 1)))
    for s0 in range(0, S, step):
        s1 = min(S, s0 + step)
        acc = torch.zeros((m, s1 - s0, L), dtype=torch.uint8, device=data.device)
        for i in range(k):
            idx = data[s0:s1, i].to(torch.int64)
            acc ^= tabs[i][:, idx]
            del idx
        out[s0:s1] = acc.permute(1, 0, 2)
        del acc
    return out


def device_codewords(k: int, m: int, S: int, L: int, seed: int):
    """[S, k + m, L] uint8 on the current device: seeded random data shards
    and torch_encode's parity (batches too large to encode on the host)."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.empty((S, k + m, L), dtype=torch.uint8, device="cuda")
    t[:, :k] = torch.randint(0, 256, (S, k, L), dtype=torch.uint8, device="cuda", generator=g)
    torch_encode(k, m, t[:, :k], out=t[:, k:])
    return t


class MaskTables(NamedTuple):
    masks: np.ndarray      # [S] int32, stripe s -> s
    present: np.ndarray    # [S, n] bool
    decodable: np.ndarray  # [S] bool: k <= popcount < n
    erased: np.ndarray     # [S, n] bool: absent shards of the decodable stripes
    surplus: np.ndarray    # [S, n] bool: present shards after the first k present, decodable stripes
    n_bad: int             # stripes with popcount < k


@functools.lru_cache(maxsize=None)
def mask_tables(k: int, m: int) -> MaskTables:
    n = k + m
    S = 1 << n
    masks = np.arange(S, dtype=np.int32)
    present = ((masks[:, None] >> np.arange(n)[None, :]) & 1).astype(bool)
    pc = present.sum(axis=1)
    decodable = (pc >= k) & (pc < n)
    rank = np.cumsum(present, axis=1)  # 1-based rank of a present shard among the present ones
    erased = ~present & decodable[:, None]
    surplus = present & (rank > k) & decodable[:, None]
    # the first k present shards precede any surplus one, so a data shard never is surplus
    assert not surplus[:, :k].any()
    assert ((present & ~surplus).sum(axis=1)[decodable] == k).all()
    for a in (masks, present, decodable, erased, surplus):
        a.setflags(write=False)
    return MaskTables(masks, present, decodable, erased, surplus, int((pc < k).sum()))


class MaskCase(NamedTuple):
    start: object     # [S, n, pitch] uint8: what the call is given
    expected: object  # [S, n, pitch] uint8: what it must leave
    tables: MaskTables
    raw: object       # the seeded random image the case was composed from


def all_masks_case(k: int, m: int, L: int, pitch: int, seed: int, image: np.ndarray = None) -> MaskCase:
    """The every-mask image in numpy. `image` [2^n, n, pitch]: the seeded
    random bytes to compose from (drawn from `seed` when not given): the data
    shards are its data bytes, the surplus garbage and the pitch bytes past L
    its own bytes."""
    n = k + m
    tb = mask_tables(k, m)
    S = 1 << n
    assert pitch >= L > 0
    if image is None:
        image = np.random.default_rng(seed).integers(0, 256, (S, n, pitch), dtype=np.uint8)
    assert image.shape == (S, n, pitch) and image.dtype == np.uint8
    parity = ref_encode(k, m, image[:, :k, :L])
    expected = image.copy()
    keep = tb.surplus[:, k:, None]  # surplus survivors (parity shards only) keep the image's random bytes
    expected[:, k:, :L] = np.where(keep, image[:, k:, :L], parity)
    start = expected.copy()
    start[:, :, :L] = np.where(tb.erased[:, :, None], np.uint8(POISON), expected[:, :, :L])
    return MaskCase(start, expected, tb, image)


def all_masks_case_torch(k: int, m: int, L: int, pitch: int, seed: int, device, image=None) -> MaskCase:
    """all_masks_case composed in torch on `device`, parity from torch_encode:
    for images too large to build in numpy and copy over."""
    import torch
    n = k + m
    tb = mask_tables(k, m)
    S = 1 << n
    assert pitch >= L > 0
    if image is None:
        g = torch.Generator(device=device).manual_seed(seed)
        image = torch.randint(0, 256, (S, n, pitch), dtype=torch.uint8, device=device, generator=g)
    assert tuple(image.shape) == (S, n, pitch) and image.dtype == torch.uint8
    expected = image.clone()
    parity = torch_encode(k, m, image[:, :k, :L])
    keep = torch.from_numpy(tb.surplus[:, k:, None].copy()).to(image.device)
    expected[:, k:, :L] = torch.where(keep, image[:, k:, :L], parity)
    del parity
    start = expected.clone()
    erased = torch.from_numpy(tb.erased[:, :, None].copy()).to(image.device)
    start[:, :, :L] = torch.where(erased, torch.full((), POISON, dtype=torch.uint8, device=image.device),
                                  expected[:, :, :L])
    return MaskCase(start, expected, tb, image)


def describe_first_difference(got, want, tb: MaskTables, L: int, first: int = 0) -> str:
    """First differing byte of two [S, n, pitch] images (numpy or torch), by
    what it is to the call (tb None: no mask tables, plain positions). `first`:
    the batch index of the images' stripe 0."""
    import torch
    if isinstance(got, torch.Tensor):
        S = got.shape[0]
        step = max(1, (1 << 28) // max(1, got.shape[1] * got.shape[2]))
        for s0 in range(0, S, step):
            if not torch.equal(got[s0:s0 + step], want[s0:s0 + step]):
                return describe_first_difference(got[s0:s0 + step].cpu().numpy(), want[s0:s0 + step].cpu().numpy(),
                                                 tb, L, first + s0)
        return "no difference"
    diff = np.argwhere(got != want)
    if not len(diff):
        return "no difference"
    r, i, b = (int(x) for x in diff[0])
    s = first + r
    mask = None if tb is None else int(tb.masks[s])
    if b >= L:
        role = "pitch byte past the shard"
    elif tb is None:
        role = "shard"
    elif tb.erased[s, i]:
        role = "erased slot (output)"
    elif tb.surplus[s, i]:
        role = "surplus survivor (must not be read or written)"
    elif not tb.decodable[s]:
        role = "shard of a skipped or complete stripe"
    else:
        role = "one of the first k present shards"
    where = "" if mask is None else f" (present mask {mask:#x})"
    return f"stripe {s}{where} shard {i} byte {b}: {role}; got {int(got[r, i, b]):#04x}, " \
           f"expected {int(want[r, i, b]):#04x}"
