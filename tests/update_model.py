"""The update in numpy -- TEST INFRASTRUCTURE ONLY.

include/hec.h (hec_gpu_update_batch) is the contract: per stripe, with U the
data shards its mask names (bits 0..k-1; the other bits mean nothing),

    parity ^= P[:, U] * (old[U] ^ new[U])

The model is independent of the code under test: the parity before the call
XOR gfref.ref_encode (rs_oracle's matrix and tables) of the delta with the
shards outside U zeroed. It holds for any parity before the call, codeword or
not. tests/test_update_model.py pins it against the C oracle's encode.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

import gfref


def changed(masks, k: int) -> np.ndarray:
    """masks [S] -> bool [S, k]: data shard c of stripe s is in U."""
    m = np.asarray(masks).astype(np.int64) & ((1 << k) - 1)
    return ((m[:, None] >> np.arange(k)[None, :]) & 1).astype(bool)


def updated_parity(parity: np.ndarray, old: Optional[np.ndarray], new: np.ndarray, masks, k: int = 10,
                   m: int = 4) -> np.ndarray:
    """parity[S, m, L] before the call, old[S, k, L] (None: zero), new[S, k, L]
    and one mask word per stripe -> the parity after the call. Shards outside U
    may hold anything: they take no part."""
    S, mm, L = parity.shape
    assert mm == m and new.shape == (S, k, L) and (old is None or old.shape == new.shape)
    delta = new if old is None else old ^ new
    delta = np.where(changed(masks, k)[:, :, None], delta, np.uint8(0))
    return parity ^ gfref.ref_encode(k, m, np.ascontiguousarray(delta))


def merged(old: np.ndarray, new: np.ndarray, masks, k: int = 10) -> np.ndarray:
    """The data after the caller commits: new where the mask names the shard, old elsewhere."""
    return np.where(changed(masks, k)[:, :, None], new, old)
