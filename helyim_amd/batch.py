"""Device-resident stripe batches over torch tensors (ROCm).

PyTorch is plumbing here: it owns the HBM allocation and the HIP stream; the
arithmetic is libhec's gfx950 kernels (hec_gpu_encode_batch /
hec_gpu_reconstruct_batch). Layout: a uint8 tensor ``[S, total, L]`` (stripe
major, shard, byte) -- a small row of the reference's .dat layout is exactly
10 contiguous L-byte blocks, so a run of rows lands here with one copy.
"""
from __future__ import annotations

import torch

from . import _lib
from .errors import check
from .rs import ReedSolomon

lib = _lib.lib
check_status = check  # for the calls that have a result tensor named `check`


def _stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


def _check_device(t: torch.Tensor):
    # libhec works on the calling thread's current device (hec.h): a tensor
    # on another GPU would be addressed through the wrong device's page tables
    if t.device.index != torch.cuda.current_device():
        raise ValueError(f"tensor on {t.device}, current device is cuda:{torch.cuda.current_device()}")


def _check_stripes(t: torch.Tensor, rs: ReedSolomon, shards: int = None):
    if t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 3:
        raise TypeError("expected a uint8 CUDA tensor [stripes, shards, L]")
    if t.stride(2) != 1:
        raise ValueError("shard bytes must be contiguous")
    want = rs.total_shard_count() if shards is None else shards
    if t.shape[1] != want:
        raise ValueError(f"expected {want} shards per stripe, got {t.shape[1]}")
    _check_device(t)


def _layout(rs: ReedSolomon, stripes: torch.Tensor):
    """In-place ``stripes[S, total, L]``, checked -> (the six data / parity
    layout arguments of the C calls, S, L): the parity is shards data..total."""
    _check_stripes(stripes, rs)
    S, n, L = stripes.shape
    st, sh = stripes.stride(0), stripes.stride(1)
    base = stripes.data_ptr()
    return (base, st, sh, base + rs.data_shard_count() * sh, st, sh), S, L


def _layout_sep(rs: ReedSolomon, data: torch.Tensor, parity: torch.Tensor):
    """_layout of data[S, k, L] and parity[S, m, L] in separate buffers."""
    _check_stripes(data, rs, rs.data_shard_count())
    _check_stripes(parity, rs, rs.parity_shard_count())
    S, k, L = data.shape
    if parity.shape[0] != S or parity.shape[2] != L:
        raise ValueError(f"parity {tuple(parity.shape)} does not match data {tuple(data.shape)}")
    return (data.data_ptr(), data.stride(0), data.stride(1), parity.data_ptr(), parity.stride(0),
            parity.stride(1)), S, L


def _encode(rs, layout, stream):
    lay, S, L = layout
    check(lib.hec_gpu_encode_batch(rs.handle, *lay, L, S, _stream_ptr(stream)))


def encode_batch(rs: ReedSolomon, stripes: torch.Tensor, stream=None) -> None:
    """Parity of every stripe of ``stripes[S, total, L]`` into shards data..total."""
    _encode(rs, _layout(rs, stripes), stream)


def encode_batch_sep(rs: ReedSolomon, data: torch.Tensor, parity: torch.Tensor, stream=None) -> None:
    """data[S, k, L] -> parity[S, m, L] (separate buffers)."""
    _encode(rs, _layout_sep(rs, data, parity), stream)


def reconstruct_batch(rs: ReedSolomon, stripes: torch.Tensor, present_masks: torch.Tensor,
                      bad_stripes: torch.Tensor = None, stream=None) -> None:
    """Rebuild erased shards in place; present_masks int32 [S] (bit i = shard i present)."""
    _check_stripes(stripes, rs)
    S, n, L = stripes.shape
    if not (present_masks.is_cuda and present_masks.dtype == torch.int32 and present_masks.numel() == S
            and present_masks.is_contiguous()):
        raise ValueError("present_masks must be a contiguous int32 CUDA tensor with one word per stripe")
    _check_device(present_masks)
    if bad_stripes is not None:
        if not (bad_stripes.is_cuda and bad_stripes.dtype in (torch.int32, torch.uint32)
                and bad_stripes.numel() >= 1):
            raise ValueError("bad_stripes must be a 32-bit CUDA tensor")
        _check_device(bad_stripes)
    bad = bad_stripes.data_ptr() if bad_stripes is not None else None
    check(lib.hec_gpu_reconstruct_batch(rs.handle, stripes.data_ptr(), stripes.stride(0),
                                        stripes.stride(1), L, S, present_masks.data_ptr(), bad,
                                        _stream_ptr(stream)))


def reconstruct_some_batch(rs: ReedSolomon, stripes: torch.Tensor, present_masks: torch.Tensor,
                           want_masks: torch.Tensor, bad_stripes: torch.Tensor = None, stream=None) -> None:
    """Rebuild, in place, only the erased shards named in want_masks (int32
    [S], bit i = shard i is worth rebuilding); the other erased shards are
    neither computed nor written, and a stripe that wants none of its erased
    shards is not read (hec_gpu_reconstruct_some_batch, RS(10,4))."""
    _check_stripes(stripes, rs)
    S, n, L = stripes.shape
    for name, t in (("present_masks", present_masks), ("want_masks", want_masks)):
        if not (t.is_cuda and t.dtype in (torch.int32, torch.uint32) and t.numel() == S and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous 32-bit CUDA tensor with one word per stripe")
        _check_device(t)
    check(lib.hec_gpu_reconstruct_some_batch(rs.handle, stripes.data_ptr(), stripes.stride(0), stripes.stride(1),
                                             L, S, present_masks.data_ptr(), want_masks.data_ptr(),
                                             _counter_arg(bad_stripes, "bad_stripes"), _stream_ptr(stream)))


def reconstruct_some_kernel_name(L: int) -> str:
    """Kernel an aligned reconstruct_some_batch of shard length L runs."""
    return lib.hec_reconstruct_some_kernel_name(L).decode()


def _update(rs, old, new, parity, update_masks, stream):
    """old / new: (pointer, stripe stride, shard stride) of data arenas indexed
    by shard id; parity: the checked [S, m, L] tensor."""
    S, _m, L = parity.shape
    if update_masks is None:
        raise ValueError("update_masks is required")
    masks = _words_arg(S, update_masks, "update_masks")
    check(lib.hec_gpu_update_batch(rs.handle, *old, *new, parity.data_ptr(), parity.stride(0), parity.stride(1), L, S,
                                   masks.data_ptr(), _stream_ptr(stream)))


def update_batch(rs: ReedSolomon, stripes: torch.Tensor, new_data: torch.Tensor, update_masks: torch.Tensor,
                 stream=None) -> None:
    """Fold changed data shards into the stored parity of ``stripes[S, 14, L]``
    in place (hec_gpu_update_batch, RS(10,4)): update_masks 32-bit ``[S]``, bit
    c = data shard c changed from ``stripes[s, c]`` (old) to ``new_data[s, c]``
    (``new_data[S, 10, L]``). Only the four parity shards of stripes with a
    non-empty mask are written; only the shards a mask names are read. The
    new data is not copied over the old. Asynchronous on the stream."""
    _check_stripes(stripes, rs)
    k = rs.data_shard_count()
    update_batch_sep(rs, stripes[:, :k], new_data, stripes[:, k:], update_masks, stream)


def update_batch_sep(rs: ReedSolomon, old: torch.Tensor, new: torch.Tensor, parity: torch.Tensor,
                     update_masks: torch.Tensor, stream=None) -> None:
    """update_batch of old[S, k, L] -> new[S, k, L] into parity[S, m, L]
    (separate buffers). ``old`` may be None: old is zero, and the parity
    accumulates the coded new shards (over zeroed parity, any partition of the
    data shards into calls gives encode_batch's bytes)."""
    _layout_sep(rs, new, parity)
    old_arg = (None, 0, 0)
    if old is not None:
        _layout_sep(rs, old, parity)
        old_arg = (old.data_ptr(), old.stride(0), old.stride(1))
    _update(rs, old_arg, (new.data_ptr(), new.stride(0), new.stride(1)), parity, update_masks, stream)


def update_kernel_name(L: int) -> str:
    """Kernel an aligned update_batch of shard length L runs (hec_update_kernel_name)."""
    return lib.hec_update_kernel_name(L).decode()


def _words_arg(S: int, t: torch.Tensor, name: str) -> torch.Tensor:
    """A per-stripe result tensor (mismatch, suspects, present_masks): allocated when not given."""
    if t is None:
        t = torch.empty(S, dtype=torch.int32, device="cuda")
    elif not (t.is_cuda and t.dtype in (torch.int32, torch.uint32) and t.is_contiguous() and t.numel() >= S):
        raise ValueError(f"{name} must be a contiguous 32-bit CUDA tensor with at least one word per stripe")
    _check_device(t)
    return t


def _counter_arg(t: torch.Tensor, name: str):
    """An optional accumulated device word (bad_stripes, unrepaired) -> its pointer or None."""
    if t is None:
        return None
    if not (t.is_cuda and t.dtype in (torch.int32, torch.uint32) and t.numel() >= 1):
        raise ValueError(f"{name} must be a 32-bit CUDA tensor")
    _check_device(t)
    return t.data_ptr()


def _verify_args(S: int, mismatch: torch.Tensor, bad_stripes: torch.Tensor):
    """Result tensors of a device verify -> (mismatch, bad_stripes pointer)."""
    return _words_arg(S, mismatch, "mismatch"), _counter_arg(bad_stripes, "bad_stripes")


def _verify(rs, layout, mismatch, bad_stripes, stream):
    lay, S, L = layout
    mismatch, bad = _verify_args(S, mismatch, bad_stripes)
    check(lib.hec_gpu_verify_batch(rs.handle, *lay, L, S, mismatch.data_ptr(), bad, _stream_ptr(stream)))
    return mismatch


def verify_batch(rs: ReedSolomon, stripes: torch.Tensor, mismatch: torch.Tensor = None,
                 bad_stripes: torch.Tensor = None, stream=None) -> torch.Tensor:
    """Scrub ``stripes[S, total, L]`` on the device (hec_gpu_verify_batch): word s
    of the returned int32 ``[S]`` tensor (``mismatch``, allocated when not
    given) has bit j set when parity shard j of stripe s differs from the
    parity of its data shards; 0 = clean. bad_stripes (32-bit CUDA word,
    accumulated): plus one per stripe with a non-zero word. Nothing else is
    written. Asynchronous on the stream."""
    return _verify(rs, _layout(rs, stripes), mismatch, bad_stripes, stream)


def verify_batch_sep(rs: ReedSolomon, data: torch.Tensor, parity: torch.Tensor, mismatch: torch.Tensor = None,
                     bad_stripes: torch.Tensor = None, stream=None) -> torch.Tensor:
    """verify_batch of data[S, k, L] against the stored parity[S, m, L] (separate buffers)."""
    return _verify(rs, _layout_sep(rs, data, parity), mismatch, bad_stripes, stream)


def _locate(call, rs, layout, mismatch, suspects, bad_stripes, stream):
    lay, S, L = layout
    mismatch, bad = _verify_args(S, mismatch, bad_stripes)
    suspects = _words_arg(S, suspects, "suspects")
    check(call(rs.handle, *lay, L, S, mismatch.data_ptr(), suspects.data_ptr(), bad, _stream_ptr(stream)))
    return mismatch, suspects


def _repair(call, rs, stripes, mismatch, suspects, present_masks, unrepaired, stream):
    _check_stripes(stripes, rs)
    S, n, L = stripes.shape
    mismatch = _words_arg(S, mismatch, "mismatch")
    left = _counter_arg(unrepaired, "unrepaired")
    suspects = _words_arg(S, suspects, "suspects")
    present_masks = _words_arg(S, present_masks, "present_masks")
    check(call(rs.handle, stripes.data_ptr(), stripes.stride(0), stripes.stride(1), L, S, mismatch.data_ptr(),
               suspects.data_ptr(), present_masks.data_ptr(), left, _stream_ptr(stream)))
    return mismatch, suspects, present_masks


def locate_corrupt_batch(rs: ReedSolomon, stripes: torch.Tensor, mismatch: torch.Tensor = None,
                         suspects: torch.Tensor = None, bad_stripes: torch.Tensor = None, stream=None):
    """verify_batch that also names the corrupt shard (hec_gpu_locate_corrupt_batch,
    RS(10,4) only). Returns ``(mismatch, suspects)``, int32 ``[S]`` tensors
    (allocated when not given): mismatch as verify_batch's; bit c of
    suspects[s] set = shard c alone explains a byte column of stripe s (data
    shards 0..9, parity shard j at bit 10 + j), ``helyim_amd.SUSPECT_UNEXPLAINED`` (bit
    31) = a column no single shard explains; 0 = clean. With at most 3 wrong
    shards in a column no intact shard is ever named. Nothing else is written.
    Asynchronous on the stream."""
    return _locate(lib.hec_gpu_locate_corrupt_batch, rs, _layout(rs, stripes), mismatch, suspects, bad_stripes,
                   stream)


def locate_corrupt_batch_sep(rs: ReedSolomon, data: torch.Tensor, parity: torch.Tensor,
                             mismatch: torch.Tensor = None, suspects: torch.Tensor = None,
                             bad_stripes: torch.Tensor = None, stream=None):
    """locate_corrupt_batch of data[S, k, L] against the stored parity[S, m, L] (separate buffers)."""
    return _locate(lib.hec_gpu_locate_corrupt_batch, rs, _layout_sep(rs, data, parity), mismatch, suspects,
                   bad_stripes, stream)


def locate_corrupt_pairs_batch(rs: ReedSolomon, stripes: torch.Tensor, mismatch: torch.Tensor = None,
                               suspects: torch.Tensor = None, bad_stripes: torch.Tensor = None, stream=None):
    """locate_corrupt_batch that also names two wrong shards of a byte column
    (hec_gpu_locate_corrupt_pairs_batch, RS(10,4) only): the same arguments
    and result shape. A column one shard explains sets its bit as before; a
    column that shards a and b together explain sets bits a and b; bit 31 = a
    column no one or two shards explain. At most 2 wrong shards in a column
    are named exactly; 3 wrong shards never name a single intact shard but
    may name an intact pair (include/hec.h) -- locate_corrupt_batch keeps the
    stricter promise. Asynchronous on the stream."""
    return _locate(lib.hec_gpu_locate_corrupt_pairs_batch, rs, _layout(rs, stripes), mismatch, suspects, bad_stripes,
                   stream)


def locate_corrupt_pairs_batch_sep(rs: ReedSolomon, data: torch.Tensor, parity: torch.Tensor,
                                   mismatch: torch.Tensor = None, suspects: torch.Tensor = None,
                                   bad_stripes: torch.Tensor = None, stream=None):
    """locate_corrupt_pairs_batch of data[S, k, L] against the stored parity[S, m, L] (separate buffers)."""
    return _locate(lib.hec_gpu_locate_corrupt_pairs_batch, rs, _layout_sep(rs, data, parity), mismatch, suspects,
                   bad_stripes, stream)


def repair_batch(rs: ReedSolomon, stripes: torch.Tensor, mismatch: torch.Tensor = None,
                 suspects: torch.Tensor = None, present_masks: torch.Tensor = None,
                 unrepaired: torch.Tensor = None, stream=None):
    """Locate, then rebuild in place the shards locate names (hec_gpu_repair_batch,
    RS(10,4) only). Returns ``(mismatch, suspects, present_masks)``, int32
    ``[S]`` tensors (allocated when not given): a stripe whose suspects word
    names 1 to 4 shards with bit 31 clear has them rebuilt from the others
    (present mask ``0x3FFF & ~suspects``); any other stripe is left byte for
    byte (mask ``0x3FFF``) and, when its word is non-zero, counted into
    unrepaired (32-bit CUDA word, accumulated). Run verify_batch afterwards
    for proof. Asynchronous on the stream."""
    return _repair(lib.hec_gpu_repair_batch, rs, stripes, mismatch, suspects, present_masks, unrepaired, stream)


def repair_pairs_batch(rs: ReedSolomon, stripes: torch.Tensor, mismatch: torch.Tensor = None,
                       suspects: torch.Tensor = None, present_masks: torch.Tensor = None,
                       unrepaired: torch.Tensor = None, stream=None):
    """repair_batch over locate_corrupt_pairs_batch's words
    (hec_gpu_repair_pairs_batch): the same arguments and results; a stripe with
    two shards wrong in one column is repaired too, as long as its columns
    name at most four shards in all and bit 31 is clear. Whole shards per
    stripe. Asynchronous on the stream."""
    return _repair(lib.hec_gpu_repair_pairs_batch, rs, stripes, mismatch, suspects, present_masks, unrepaired, stream)


def _bytes_counter_arg(t: torch.Tensor, name: str):
    """An optional accumulated 64-bit device word (corrected_bytes) -> its pointer or None."""
    if t is None:
        return None
    if not (t.is_cuda and t.dtype in (torch.int64, torch.uint64) and t.numel() >= 1):
        raise ValueError(f"{name} must be a 64-bit CUDA tensor")
    _check_device(t)
    return t.data_ptr()


def _correct(rs, layout, mismatch, suspects, bad_stripes, uncorrected, corrected_bytes, pairs, stream):
    lay, S, L = layout
    mismatch, bad = _verify_args(S, mismatch, bad_stripes)
    suspects = _words_arg(S, suspects, "suspects")
    call = lib.hec_gpu_correct_pairs_batch if pairs else lib.hec_gpu_correct_batch
    check(call(rs.handle, *lay, L, S, mismatch.data_ptr(), suspects.data_ptr(), bad,
               _counter_arg(uncorrected, "uncorrected"), _bytes_counter_arg(corrected_bytes, "corrected_bytes"),
               _stream_ptr(stream)))
    return mismatch, suspects


def correct_batch(rs: ReedSolomon, stripes: torch.Tensor, mismatch: torch.Tensor = None,
                  suspects: torch.Tensor = None, bad_stripes: torch.Tensor = None, uncorrected: torch.Tensor = None,
                  corrected_bytes: torch.Tensor = None, pairs: bool = False, stream=None):
    """Locate, and fix in place every byte column one shard explains
    (hec_gpu_correct_batch, RS(10,4) only; ``pairs=True``: also the columns two
    shards explain, hec_gpu_correct_pairs_batch). Returns ``(mismatch,
    suspects)`` as locate_corrupt_batch (locate_corrupt_pairs_batch), of the
    bytes as they were before the call. Only wrong bytes of explained columns
    change; a column that sets bit 31 keeps its bytes while the stripe's other
    columns are still fixed. uncorrected (32-bit CUDA word, accumulated): plus
    one per stripe with bit 31; corrected_bytes (64-bit CUDA word,
    accumulated): the bytes changed. Unlike repair_batch this also restores a
    stripe whose columns name five or more shards. Asynchronous on the
    stream."""
    return _correct(rs, _layout(rs, stripes), mismatch, suspects, bad_stripes, uncorrected, corrected_bytes, pairs,
                    stream)


def correct_batch_sep(rs: ReedSolomon, data: torch.Tensor, parity: torch.Tensor, mismatch: torch.Tensor = None,
                      suspects: torch.Tensor = None, bad_stripes: torch.Tensor = None,
                      uncorrected: torch.Tensor = None, corrected_bytes: torch.Tensor = None, pairs: bool = False,
                      stream=None):
    """correct_batch of data[S, k, L] and the stored parity[S, m, L] (separate buffers, both fixed in place)."""
    return _correct(rs, _layout_sep(rs, data, parity), mismatch, suspects, bad_stripes, uncorrected, corrected_bytes,
                    pairs, stream)


def _masks_arg(S: int, present_masks: torch.Tensor) -> torch.Tensor:
    if not (present_masks.is_cuda and present_masks.dtype in (torch.int32, torch.uint32)
            and present_masks.numel() == S and present_masks.is_contiguous()):
        raise ValueError("present_masks must be a contiguous 32-bit CUDA tensor with one word per stripe")
    _check_device(present_masks)
    return present_masks


def _present_args(rs, stripes, present_masks, **words):
    """The masked calls' shared preparation -> (the C arguments up to the
    masks, the per-stripe result tensors named in words, allocated when None)."""
    _check_stripes(stripes, rs)
    S, n, L = stripes.shape
    masks = _masks_arg(S, present_masks)
    lead = (rs.handle, stripes.data_ptr(), stripes.stride(0), stripes.stride(1), L, S, masks.data_ptr())
    return lead, [_words_arg(S, t, name) for name, t in words.items()]


def verify_present_batch(rs: ReedSolomon, stripes: torch.Tensor, present_masks: torch.Tensor,
                         check: torch.Tensor = None, bad_stripes: torch.Tensor = None,
                         unchecked: torch.Tensor = None, stream=None) -> torch.Tensor:
    """Scrub degraded ``stripes[S, 14, L]`` (hec_gpu_verify_present_batch, RS(10,4)
    only): present_masks as reconstruct_batch's. Of a stripe's p >= 11 present
    shards the ten lowest are decoded from and the other p - 10 compared: bit e
    (shard index) of the returned int32 ``[S]`` word is set when present shard
    e differs from what those ten imply; with the full mask that is
    verify_batch's word shifted left by 10. Stripes with p <= 10 give 0, are
    not read and are counted into unchecked; bad_stripes counts the non-zero
    words (32-bit CUDA words, accumulated). Absent shards are never read and
    nothing but the words is written. Asynchronous on the stream."""
    lead, (check,) = _present_args(rs, stripes, present_masks, check=check)
    check_status(lib.hec_gpu_verify_present_batch(
        *lead, check.data_ptr(), _counter_arg(bad_stripes, "bad_stripes"), _counter_arg(unchecked, "unchecked"),
        _stream_ptr(stream)))
    return check


def locate_corrupt_present_batch(rs: ReedSolomon, stripes: torch.Tensor, present_masks: torch.Tensor,
                                 check: torch.Tensor = None, suspects: torch.Tensor = None,
                                 bad_stripes: torch.Tensor = None, unchecked: torch.Tensor = None, stream=None):
    """verify_present_batch that also names the corrupt survivor
    (hec_gpu_locate_corrupt_present_batch). Returns ``(check, suspects)``: bit c
    of suspects[s] = present shard c alone explains a byte column of stripe s,
    ``helyim_amd.SUSPECT_UNEXPLAINED`` = a column no single shard explains. With
    1 or 2 shards lost one corrupt survivor is named; with 3 lost it is only
    detected (bit 31); with 2 lost, two wrong shards in one column may name an
    intact shard (include/hec.h has the table). With the full mask the words
    are locate_corrupt_batch's (check = mismatch << 10)."""
    lead, (check, suspects) = _present_args(rs, stripes, present_masks, check=check, suspects=suspects)
    check_status(lib.hec_gpu_locate_corrupt_present_batch(
        *lead, check.data_ptr(), suspects.data_ptr(), _counter_arg(bad_stripes, "bad_stripes"),
        _counter_arg(unchecked, "unchecked"), _stream_ptr(stream)))
    return check, suspects


def reconstruct_checked_batch(rs: ReedSolomon, stripes: torch.Tensor, present_masks: torch.Tensor,
                              check: torch.Tensor = None, suspects: torch.Tensor = None,
                              use_masks: torch.Tensor = None, bad_stripes: torch.Tensor = None,
                              unrepaired: torch.Tensor = None, stream=None):
    """reconstruct_batch that checks its survivors first
    (hec_gpu_reconstruct_checked_batch). Returns ``(check, suspects, use_masks)``:
    a clean or uncheckable stripe is rebuilt from present_masks as
    reconstruct_batch would; a stripe whose suspects word names shards (bit 31
    clear, at least 10 others present) has them rebuilt too (use mask =
    present & ~suspects); any other dirty stripe is left byte for byte, holes
    included (use mask 0x3FFF), and counted into unrepaired. bad_stripes is
    reconstruct_batch's count. Only shards outside a stripe's use mask are
    written. Run verify_batch afterwards for proof."""
    lead, (check, suspects, use_masks) = _present_args(rs, stripes, present_masks, check=check, suspects=suspects,
                                                       use_masks=use_masks)
    check_status(lib.hec_gpu_reconstruct_checked_batch(
        *lead, check.data_ptr(), suspects.data_ptr(), use_masks.data_ptr(), _counter_arg(bad_stripes, "bad_stripes"),
        _counter_arg(unrepaired, "unrepaired"), _stream_ptr(stream)))
    return check, suspects, use_masks


def correct_present_batch(rs: ReedSolomon, stripes: torch.Tensor, present_masks: torch.Tensor, min_spares: int = 2,
                          check: torch.Tensor = None, suspects: torch.Tensor = None,
                          bad_stripes: torch.Tensor = None, unchecked: torch.Tensor = None,
                          uncorrected: torch.Tensor = None, corrected_bytes: torch.Tensor = None, stream=None):
    """locate_corrupt_present_batch that also fixes, in place, every byte column
    one present shard explains (hec_gpu_correct_present_batch). Returns
    ``(check, suspects)`` of the bytes as they were before the call. Only
    stripes with min_spares (2, 3 or 4) or more spare shards are written; only
    wrong bytes of explained columns change, a column that sets bit 31 keeps
    its bytes, absent shards are never touched. With two spares, two wrong
    shards in one column may be taken for an intact one, which is then
    written (include/hec.h has the rates); min_spares=3 rules that out.
    uncorrected (32-bit CUDA word, accumulated): plus one per stripe left
    inconsistent (bit 31, or dirty with fewer spares); corrected_bytes (64-bit
    CUDA word, accumulated): the bytes changed. Asynchronous on the stream."""
    lead, (check, suspects) = _present_args(rs, stripes, present_masks, check=check, suspects=suspects)
    check_status(lib.hec_gpu_correct_present_batch(
        *lead, int(min_spares), check.data_ptr(), suspects.data_ptr(), _counter_arg(bad_stripes, "bad_stripes"),
        _counter_arg(unchecked, "unchecked"), _counter_arg(uncorrected, "uncorrected"),
        _bytes_counter_arg(corrected_bytes, "corrected_bytes"), _stream_ptr(stream)))
    return check, suspects


def reconstruct_corrected_batch(rs: ReedSolomon, stripes: torch.Tensor, present_masks: torch.Tensor,
                                min_spares: int = 2, check: torch.Tensor = None, suspects: torch.Tensor = None,
                                use_masks: torch.Tensor = None, bad_stripes: torch.Tensor = None,
                                unrepaired: torch.Tensor = None, corrected_bytes: torch.Tensor = None, stream=None):
    """Correct the survivors, then rebuild the lost shards from them
    (hec_gpu_reconstruct_corrected_batch). Returns ``(check, suspects,
    use_masks)``: correct_present_batch's words; a clean or uncheckable stripe,
    and a dirty one with min_spares or more spare shards whose columns were all
    corrected (bit 31 clear), is rebuilt from its present shards (use mask =
    present mask: no survivor is dropped); any other dirty stripe keeps its
    holes (use mask 0x3FFF) and is counted into unrepaired. Unlike
    reconstruct_checked_batch this also restores a stripe whose columns name
    many different shards; a survivor that is wrong throughout is cheaper as
    an erasure there. Run verify_batch afterwards for proof."""
    lead, (check, suspects, use_masks) = _present_args(rs, stripes, present_masks, check=check, suspects=suspects,
                                                       use_masks=use_masks)
    check_status(lib.hec_gpu_reconstruct_corrected_batch(
        *lead, int(min_spares), check.data_ptr(), suspects.data_ptr(), use_masks.data_ptr(),
        _counter_arg(bad_stripes, "bad_stripes"), _counter_arg(unrepaired, "unrepaired"),
        _bytes_counter_arg(corrected_bytes, "corrected_bytes"), _stream_ptr(stream)))
    return check, suspects, use_masks


def check_kernel_name(L: int) -> str:
    """The kernel an aligned verify_present_batch of this shard length runs (hec_check_kernel_name)."""
    return lib.hec_check_kernel_name(L).decode()


def verify_kernel_name(L: int) -> str:
    """The kernel an aligned RS(10,4) verify_batch of this shard length runs (hec_verify_kernel_name)."""
    return lib.hec_verify_kernel_name(L).decode()


def _check_host(t: torch.Tensor, rs: ReedSolomon):
    if t.dtype != torch.uint8 or t.is_cuda or t.dim() != 3 or t.stride(2) != 1:
        raise TypeError("expected a host uint8 tensor [stripes, shards, L] with contiguous shards")
    if t.shape[1] != rs.total_shard_count():
        raise ValueError(f"expected {rs.total_shard_count()} shards per stripe, got {t.shape[1]}")


def _device_list(devices):
    """devices -> (ctypes int array, count) for the *_multi calls."""
    import ctypes
    ds = [int(d) for d in devices]
    if not ds:
        raise ValueError("empty device list")
    return (ctypes.c_int * len(ds))(*ds), len(ds)


def _host_layout(rs: ReedSolomon, stripes: torch.Tensor):
    """Check host stripes[S, total, L] -> (S, L, shards, parity): the (address,
    stripe stride, shard stride) of the whole arena, and of its parity shards."""
    _check_host(stripes, rs)
    S, _n, L = stripes.shape
    st, sh = stripes.stride(0), stripes.stride(1)
    base = stripes.data_ptr()
    return S, L, (base, st, sh), (base + rs.data_shard_count() * sh, st, sh)


def _host_masks(S: int, masks, name: str):
    """masks -> a contiguous uint32 numpy array of one word per stripe."""
    import numpy as np
    m = np.ascontiguousarray(np.asarray(masks, dtype=np.uint32))
    if m.size != S:
        raise ValueError(f"{m.size} {name} masks for {S} stripes")
    return m


def _host_call(name: str, rs: ReedSolomon, devices, *args) -> None:
    """lib.<name> on the current device, or with a device list lib.<name>_multi."""
    if devices is None:
        check(getattr(lib, name)(rs.handle, *args))
        return
    arr, nd = _device_list(devices)
    check(getattr(lib, name + "_multi")(rs.handle, arr, nd, *args))


def host_encode_batch(rs: ReedSolomon, stripes: torch.Tensor, devices=None) -> None:
    """Host-memory stripes[S, total, L] (pin_memory() for full PCIe rate):
    parity computed on the GPU, pipelined H2D -> kernel -> D2H. devices (a
    list of GPU ids, repeats allowed): contiguous stripe ranges, one per entry,
    coded concurrently (hec_host_encode_batch_multi); None = the current
    device."""
    S, L, shards, parity = _host_layout(rs, stripes)
    _host_call("hec_host_encode_batch", rs, devices, *shards, *parity, L, S)


def host_reconstruct_batch(rs: ReedSolomon, stripes: torch.Tensor, present_masks, devices=None) -> int:
    """Host-memory in-place reconstruct; returns the number of skipped stripes
    (fewer than data_shards present). devices: as host_encode_batch
    (hec_host_reconstruct_batch_multi)."""
    import ctypes
    S, L, shards, _parity = _host_layout(rs, stripes)
    m = _host_masks(S, present_masks, "present")
    bad = ctypes.c_uint32(0)
    _host_call("hec_host_reconstruct_batch", rs, devices, *shards, L, S, m.ctypes.data, ctypes.byref(bad))
    return int(bad.value)


def host_reconstruct_some_batch(rs: ReedSolomon, stripes: torch.Tensor, present_masks, want_masks) -> int:
    """host_reconstruct_batch of the erased shards named in want_masks only
    (hec_host_reconstruct_some_batch, RS(10,4)): only those come back over
    PCIe. Returns the number of skipped stripes (fewer than 10 shards present
    and an erased shard wanted)."""
    import ctypes
    S, L, shards, _parity = _host_layout(rs, stripes)
    m = _host_masks(S, present_masks, "present")
    w = _host_masks(S, want_masks, "want")
    bad = ctypes.c_uint32(0)
    _host_call("hec_host_reconstruct_some_batch", rs, None, *shards, L, S, m.ctypes.data, w.ctypes.data,
               ctypes.byref(bad))
    return int(bad.value)


def host_update_batch(rs: ReedSolomon, delta: torch.Tensor, parity: torch.Tensor, update_masks) -> None:
    """Fold host-memory deltas into host-memory parity on the GPU
    (hec_host_update_batch, RS(10,4)): ``delta[S, 10, L]`` holds old ^ new of
    each changed data shard (or the new shard where the parity has not seen it
    yet), ``parity[S, 4, L]`` is updated in place, update_masks one word per
    stripe (bit c = data shard c changed). Only the named deltas and the parity
    of the stripes with a non-empty mask cross PCIe. Synchronous."""
    k, m = rs.data_shard_count(), rs.parity_shard_count()
    for t, n, name in ((delta, k, "delta"), (parity, m, "parity")):
        if t.dtype != torch.uint8 or t.is_cuda or t.dim() != 3 or t.stride(2) != 1:
            raise TypeError(f"{name}: expected a host uint8 tensor [stripes, shards, L] with contiguous shards")
        if t.shape[1] != n:
            raise ValueError(f"{name}: expected {n} shards per stripe, got {t.shape[1]}")
    S, _k, L = delta.shape
    if parity.shape[0] != S or parity.shape[2] != L:
        raise ValueError(f"parity {tuple(parity.shape)} does not match delta {tuple(delta.shape)}")
    w = _host_masks(S, update_masks, "update")
    _host_call("hec_host_update_batch", rs, None, delta.data_ptr(), delta.stride(0), delta.stride(1),
               parity.data_ptr(), parity.stride(0), parity.stride(1), L, S, w.ctypes.data)


def host_verify_batch(rs: ReedSolomon, stripes: torch.Tensor):
    """Scrub host-memory stripes[S, total, L] on the GPU (hec_host_verify_batch):
    returns the uint32 ``[S]`` numpy array of mismatch words (verify_batch's
    contract). Only the words come back over PCIe; the stripes are not written."""
    import numpy as np
    S, L, shards, parity = _host_layout(rs, stripes)
    words = np.zeros(max(S, 1), dtype=np.uint32)
    _host_call("hec_host_verify_batch", rs, None, *shards, *parity, L, S, words.ctypes.data, None)
    return words[:S]


DESC_DTYPE = None


def desc_dtype():
    """numpy dtype of include/hec.h ``hec_stripe_desc`` (24 bytes)."""
    import numpy as np
    global DESC_DTYPE
    if DESC_DTYPE is None:
        DESC_DTYPE = np.dtype([("offset", "<u8"), ("shard_stride", "<u8"), ("shard_len", "<u4"),
                               ("present_mask", "<u4")])
    return DESC_DTYPE


def _desc_array(descs, base: torch.Tensor, shards: int):
    """descs: a ``desc_dtype()`` array, or rows of (offset, shard_stride,
    shard_len, present_mask). Every stripe's bytes [offset, offset +
    (shards-1)*stride + len) must lie inside ``base`` (checked here: the C ABI
    only sees a pointer)."""
    import numpy as np
    dt = desc_dtype()
    if isinstance(descs, np.ndarray) and descs.dtype == dt:
        d = np.ascontiguousarray(descs)
    else:
        d = np.array([tuple(int(x) for x in r) for r in descs], dtype=dt)
    if base.dtype != torch.uint8 or not base.is_cuda or not base.is_contiguous():
        raise TypeError("base must be a contiguous uint8 CUDA tensor")
    _check_device(base)
    if len(d):
        off, stride, ln = d["offset"], d["shard_stride"], d["shard_len"].astype(np.uint64)
        limit = np.uint64(base.numel())
        # no wrap-around: every term is checked against the buffer before summing
        bad = (off > limit) | (stride > limit) | (ln > limit)
        end = off + np.uint64(shards - 1) * np.minimum(stride, limit) + ln
        bad |= end > limit
        bad |= (ln > 0) & (stride < ln)
        if bad.any():
            i = int(np.argmax(bad))
            raise ValueError(f"stripe {i} (offset {int(off[i])}, stride {int(stride[i])}, len {int(ln[i])}) "
                             f"overlaps itself or runs past base ({base.numel()} bytes)")
    return d


def encode_ragged(rs: ReedSolomon, base: torch.Tensor, descs, stream=None) -> None:
    """RS(10,4) encode of stripes of mixed lengths in one launch; descs rows are
    (byte offset of shard 0 in base, shard stride, shard length, unused)."""
    d = _desc_array(descs, base, rs.total_shard_count())
    check(lib.hec_gpu_encode_ragged(rs.handle, base.data_ptr(), d.ctypes.data, len(d), _stream_ptr(stream)))


def reconstruct_ragged(rs: ReedSolomon, base: torch.Tensor, descs, bad_stripes: torch.Tensor = None,
                       stream=None) -> None:
    """Reconstruct stripes of mixed lengths and patterns in place, one launch;
    descs rows are (offset, shard stride, shard length, present mask)."""
    d = _desc_array(descs, base, rs.total_shard_count())
    bad = bad_stripes.data_ptr() if bad_stripes is not None else None
    check(lib.hec_gpu_reconstruct_ragged(rs.handle, base.data_ptr(), d.ctypes.data, len(d), bad,
                                         _stream_ptr(stream)))


def reconstruct_some_ragged(rs: ReedSolomon, base: torch.Tensor, descs, want_masks,
                            bad_stripes: torch.Tensor = None, stream=None) -> None:
    """reconstruct_ragged of the erased shards named in want_masks only (one
    host word per stripe, bit i = shard i is worth rebuilding); a stripe that
    wants none of its erased shards launches nothing
    (hec_gpu_reconstruct_some_ragged)."""
    import numpy as np
    d = _desc_array(descs, base, rs.total_shard_count())
    w = np.ascontiguousarray(np.asarray(want_masks, dtype=np.uint32))
    if w.size != len(d):
        raise ValueError(f"{w.size} want masks for {len(d)} stripes")
    check(lib.hec_gpu_reconstruct_some_ragged(rs.handle, base.data_ptr(), d.ctypes.data, w.ctypes.data, len(d),
                                              _counter_arg(bad_stripes, "bad_stripes"), _stream_ptr(stream)))


UPDATE_DESC_DTYPE = None


def update_desc_dtype():
    """numpy dtype of include/hec.h ``hec_update_desc`` (56 bytes)."""
    import numpy as np
    global UPDATE_DESC_DTYPE
    if UPDATE_DESC_DTYPE is None:
        UPDATE_DESC_DTYPE = np.dtype([("parity_offset", "<u8"), ("parity_stride", "<u8"), ("new_offset", "<u8"),
                                      ("new_stride", "<u8"), ("old_offset", "<u8"), ("old_stride", "<u8"),
                                      ("shard_len", "<u4"), ("update_mask", "<u4")])
    return UPDATE_DESC_DTYPE


def _update_arena(t, name: str):
    if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous uint8 CUDA tensor")
    _check_device(t)


def _update_desc_array(descs, old, new: torch.Tensor, parity: torch.Tensor):
    """descs: an ``update_desc_dtype()`` array, or rows of its eight fields in
    order. As _desc_array, every stripe's bytes must lie inside its arenas: the
    four parity shards in ``parity``, the ten data shards in ``new`` and, when
    given, ``old`` (checked here: the C ABI only sees pointers)."""
    import numpy as np
    dt = update_desc_dtype()
    if isinstance(descs, np.ndarray) and descs.dtype == dt:
        d = np.ascontiguousarray(descs)
    else:
        rows = [tuple(int(x) for x in r) for r in descs]
        if any(len(r) != len(dt.names) for r in rows):
            raise ValueError(f"an update descriptor has {len(dt.names)} fields: {', '.join(dt.names)}")
        d = np.array(rows, dtype=dt)
    arenas = [("parity", parity, 4), ("new", new, 10)] + ([("old", old, 10)] if old is not None else [])
    for name, t, shards in arenas:
        _update_arena(t, name)
        if not len(d):
            continue
        off, stride, ln = d[name + "_offset"], d[name + "_stride"], d["shard_len"].astype(np.uint64)
        limit = np.uint64(t.numel())
        # no wrap-around: every term is checked against the buffer before summing
        bad = (off > limit) | (stride > limit) | (ln > limit)
        end = off + np.uint64(shards - 1) * np.minimum(stride, limit) + ln
        bad |= end > limit
        bad |= (ln > 0) & (stride < ln)
        if bad.any():
            i = int(np.argmax(bad))
            raise ValueError(f"stripe {i} ({name} offset {int(off[i])}, stride {int(stride[i])}, len {int(ln[i])}) "
                             f"overlaps itself or runs past the {name} arena ({t.numel()} bytes)")
    return d


def update_ragged(rs: ReedSolomon, old, new: torch.Tensor, parity: torch.Tensor, descs, stream=None) -> None:
    """update_batch_sep over stripes of mixed lengths in one launch
    (hec_gpu_update_ragged, RS(10,4)): ``old`` (or None: old is zero), ``new``
    and ``parity`` are flat uint8 arenas, descs rows are (parity offset, parity
    stride, new offset, new stride, old offset, old stride, shard length, update
    mask). ``parity`` may be the tensor ``old`` is (the in-place ragged arena,
    update_descs_in_place). Only bytes [0, shard length) of the four parity
    shards of stripes with a non-empty mask are written. Asynchronous."""
    d = _update_desc_array(descs, old, new, parity)
    check(lib.hec_gpu_update_ragged(rs.handle, old.data_ptr() if old is not None else None, new.data_ptr(),
                                    parity.data_ptr(), d.ctypes.data, len(d), _stream_ptr(stream)))


def update_descs_in_place(descs, new_descs, masks):
    """Update descriptors of an in-place ragged arena: ``descs`` (desc_dtype
    rows) place every stripe's 14 shards in the arena passed as both ``old``
    and ``parity``; ``new_descs`` (desc_dtype rows; the mask field is not read)
    place its ten new data shards in the ``new`` arena; masks: one update mask
    per stripe."""
    import numpy as np
    dt = desc_dtype()

    def as_descs(x):
        if isinstance(x, np.ndarray) and x.dtype == dt:
            return x
        return np.array([tuple(int(v) for v in r) for r in x], dtype=dt)

    d, nd = as_descs(descs), as_descs(new_descs)
    m = np.asarray(masks, dtype=np.uint32).reshape(-1)
    if not (len(d) == len(nd) == m.size):
        raise ValueError(f"{len(d)} stripes, {len(nd)} new-data descriptors, {m.size} masks")
    if (d["shard_len"] != nd["shard_len"]).any():
        i = int(np.argmax(d["shard_len"] != nd["shard_len"]))
        raise ValueError(f"stripe {i}: shard length {int(d['shard_len'][i])} against {int(nd['shard_len'][i])} "
                         "of its new data")
    out = np.zeros(len(d), dtype=update_desc_dtype())
    out["parity_offset"] = d["offset"] + np.uint64(10) * d["shard_stride"]
    out["parity_stride"] = d["shard_stride"]
    out["new_offset"] = nd["offset"]
    out["new_stride"] = nd["shard_stride"]
    out["old_offset"] = d["offset"]
    out["old_stride"] = d["shard_stride"]
    out["shard_len"] = d["shard_len"]
    out["update_mask"] = m
    return out


def update_ragged_kernel_name(with_old: bool) -> str:
    """Kernel update_ragged runs with an old arena or without (hec_update_ragged_kernel_name)."""
    return lib.hec_update_ragged_kernel_name(1 if with_old else 0).decode()


def _ragged_args(rs, base, descs, **words):
    """The ragged scrub calls' shared preparation -> (the descriptor array,
    the per-stripe result tensors named in words, allocated when None)."""
    d = _desc_array(descs, base, rs.total_shard_count())
    return d, [_words_arg(len(d), t, name) for name, t in words.items()]


def verify_ragged(rs: ReedSolomon, base: torch.Tensor, descs, check: torch.Tensor = None,
                  bad_stripes: torch.Tensor = None, unchecked: torch.Tensor = None, stream=None) -> torch.Tensor:
    """Scrub stripes of mixed lengths and present masks in one pass
    (hec_gpu_verify_ragged, RS(10,4) only); descs as reconstruct_ragged's.
    Returns the int32 ``[S]`` check words (``check``, allocated when not
    given), verify_present_batch's contract stripe by stripe: bit e (shard
    index) set when spare present shard e differs from what the stripe's ten
    lowest present shards imply over its own shard length. Stripes with ten
    or fewer shards present give 0, are not read and are counted into
    unchecked; bad_stripes counts the non-zero words (32-bit CUDA words,
    accumulated). Nothing but the words is written. Asynchronous on the
    stream."""
    d, (check,) = _ragged_args(rs, base, descs, check=check)
    check_status(lib.hec_gpu_verify_ragged(
        rs.handle, base.data_ptr(), d.ctypes.data, len(d), check.data_ptr(), _counter_arg(bad_stripes, "bad_stripes"),
        _counter_arg(unchecked, "unchecked"), _stream_ptr(stream)))
    return check


def locate_corrupt_ragged(rs: ReedSolomon, base: torch.Tensor, descs, check: torch.Tensor = None,
                          suspects: torch.Tensor = None, bad_stripes: torch.Tensor = None,
                          unchecked: torch.Tensor = None, stream=None):
    """verify_ragged that also names the corrupt shard
    (hec_gpu_locate_corrupt_ragged). Returns ``(check, suspects)``,
    locate_corrupt_present_batch's words stripe by stripe: bit c of
    suspects[s] = present shard c alone explains a byte column of stripe s,
    ``helyim_amd.SUSPECT_UNEXPLAINED`` = a column no single shard explains (every
    dirty column of a stripe with one spare shard). To repair, clear the named
    bits in the stripe's present mask and call reconstruct_ragged; verify_ragged
    with the original masks is the proof."""
    d, (check, suspects) = _ragged_args(rs, base, descs, check=check, suspects=suspects)
    check_status(lib.hec_gpu_locate_corrupt_ragged(
        rs.handle, base.data_ptr(), d.ctypes.data, len(d), check.data_ptr(), suspects.data_ptr(),
        _counter_arg(bad_stripes, "bad_stripes"), _counter_arg(unchecked, "unchecked"), _stream_ptr(stream)))
    return check, suspects


def correct_ragged(rs: ReedSolomon, base: torch.Tensor, descs, min_spares: int = 2, check: torch.Tensor = None,
                   suspects: torch.Tensor = None, bad_stripes: torch.Tensor = None, unchecked: torch.Tensor = None,
                   uncorrected: torch.Tensor = None, corrected_bytes: torch.Tensor = None, stream=None):
    """locate_corrupt_ragged that also fixes, in place, every byte column one
    present shard explains (hec_gpu_correct_ragged): correct_present_batch's
    contract stripe by stripe, each stripe with its own length and present
    mask. Returns ``(check, suspects)`` of the bytes as they were before the
    call. Only stripes with min_spares (2, 3 or 4) or more spare shards are
    written; a column that sets bit 31 keeps its bytes; absent shards, bytes
    at or past a stripe's length and the gaps between stripes are never
    touched. uncorrected, corrected_bytes: as correct_present_batch's.
    Asynchronous on the stream."""
    d, (check, suspects) = _ragged_args(rs, base, descs, check=check, suspects=suspects)
    check_status(lib.hec_gpu_correct_ragged(
        rs.handle, base.data_ptr(), d.ctypes.data, len(d), int(min_spares), check.data_ptr(), suspects.data_ptr(),
        _counter_arg(bad_stripes, "bad_stripes"), _counter_arg(unchecked, "unchecked"),
        _counter_arg(uncorrected, "uncorrected"), _bytes_counter_arg(corrected_bytes, "corrected_bytes"),
        _stream_ptr(stream)))
    return check, suspects


def reconstruct_corrected_ragged(rs: ReedSolomon, base: torch.Tensor, descs, min_spares: int = 2,
                                 check: torch.Tensor = None, suspects: torch.Tensor = None,
                                 use_masks: torch.Tensor = None, bad_stripes: torch.Tensor = None,
                                 unrepaired: torch.Tensor = None, corrected_bytes: torch.Tensor = None, stream=None):
    """Correct the survivors of a ragged batch, then rebuild the lost shards
    from them, in one call (hec_gpu_reconstruct_corrected_ragged):
    reconstruct_corrected_batch's steps stripe by stripe. Returns ``(check,
    suspects, use_masks)``: a clean or uncheckable stripe, and a dirty one
    with min_spares or more spare shards whose columns were all corrected, is
    rebuilt from its present shards (use mask = present mask); any other dirty
    stripe keeps its holes (use mask 0x3FFF) and is counted into unrepaired.
    bad_stripes counts the stripes with fewer than ten shards. Run
    verify_ragged with full masks afterwards for proof."""
    d, (check, suspects, use_masks) = _ragged_args(rs, base, descs, check=check, suspects=suspects,
                                                   use_masks=use_masks)
    check_status(lib.hec_gpu_reconstruct_corrected_ragged(
        rs.handle, base.data_ptr(), d.ctypes.data, len(d), int(min_spares), check.data_ptr(), suspects.data_ptr(),
        use_masks.data_ptr(), _counter_arg(bad_stripes, "bad_stripes"), _counter_arg(unrepaired, "unrepaired"),
        _bytes_counter_arg(corrected_bytes, "corrected_bytes"), _stream_ptr(stream)))
    return check, suspects, use_masks


def host_zero_copy(t: torch.Tensor) -> bool:
    """True when host batches on t's bytes are coded zero-copy on the current
    device (hec_host_zero_copy_view): t is one pinned, GPU-addressable range."""
    import ctypes
    z = ctypes.c_int(0)
    span = (t.numel() and (sum((n - 1) * st for n, st in zip(t.shape, t.stride())) + 1)) * t.element_size()
    check(lib.hec_host_zero_copy_view(t.data_ptr(), span, ctypes.byref(z)))
    return bool(z.value)


def ragged_kernel_name(descs, decode: bool) -> str:
    """The kernel (and workgroup order) encode_ragged / reconstruct_ragged runs
    on these descriptors (hec_ragged_kernel_name: the
    launch's own choice)."""
    import numpy as np
    d = descs if isinstance(descs, np.ndarray) and descs.dtype == desc_dtype() else \
        np.array([tuple(int(x) for x in r) for r in descs], dtype=desc_dtype())
    d = np.ascontiguousarray(d)
    return lib.hec_ragged_kernel_name(d.ctypes.data if len(d) else None, len(d), int(bool(decode))).decode()


def ragged_scrub_kernel_name(descs) -> str:
    """The pass-1 kernel verify_ragged / locate_corrupt_ragged runs on these
    descriptors (hec_ragged_scrub_kernel_name: the launch's own choice)."""
    import numpy as np
    d = descs if isinstance(descs, np.ndarray) and descs.dtype == desc_dtype() else \
        np.array([tuple(int(x) for x in r) for r in descs], dtype=desc_dtype())
    d = np.ascontiguousarray(d)
    return lib.hec_ragged_scrub_kernel_name(d.ctypes.data if len(d) else None, len(d)).decode()


def fill_splitmix(t: torch.Tensor, bytes_per_stripe: int, seed_base: int, stream=None) -> None:
    """Fill the first bytes_per_stripe bytes of each t[s] with splitmix64(seed_base + s)."""
    if t.dtype != torch.uint8 or not t.is_cuda or t.dim() < 1:
        raise TypeError("expected a uint8 CUDA tensor")
    _check_device(t)
    S = t.shape[0]
    room = t.untyped_storage().nbytes() - t.storage_offset()
    if S and (bytes_per_stripe > t.stride(0) and S > 1 or (S - 1) * t.stride(0) + bytes_per_stripe > room):
        raise ValueError(f"{S} rows of {bytes_per_stripe} bytes at pitch {t.stride(0)} do not fit the tensor")
    check(lib.hec_gpu_fill_splitmix(t.data_ptr(), t.stride(0), bytes_per_stripe, S, seed_base,
                                    _stream_ptr(stream)))


_GOLDEN = 0x9E3779B97F4A7C15
SHARD_PAD = 64 << 10


def empty_stripes(n_stripes: int, total: int, shard_len: int, shard_pad: int = SHARD_PAD,
                  base_align: int = 0) -> torch.Tensor:
    """An uninitialised ``[S, total, L]`` batch in one HBM allocation on the
    current device, shard stride ``L + shard_pad`` (stripe stride ``total``
    times that). Speed only: the kernels take any shard stride. With 1 MiB
    shards a 64 KiB pad runs encode and decode ~1.5% faster than packed shards
    inside the same allocation (DESIGN.md "Data layout in HBM").
    base_align (a power of two, 0 = the allocator's own base): over-allocate
    by that much and start the batch at the first multiple of it (measurement:
    VERDICT r04 item 1(c), profiles/r05/INDEX.md)."""
    if n_stripes < 0 or total < 1 or shard_len < 0 or shard_pad < 0 or base_align < 0:
        raise ValueError("negative geometry")
    if base_align & (base_align - 1):
        raise ValueError("base_align must be a power of two")
    shard = shard_len + shard_pad
    buf = torch.empty(n_stripes * total * shard + base_align, dtype=torch.uint8, device="cuda")
    off = (-buf.data_ptr()) % base_align if base_align else 0
    return buf.as_strided((n_stripes, total, shard_len), (total * shard, shard, 1), off)


def address_alignment(ptr: int) -> int:
    """Largest power of two dividing ptr (capped at 2^40)."""
    return min(ptr & -ptr, 1 << 40) if ptr else 1 << 40


def shard_seed(seed_base: int, shard: int, shard_len: int) -> int:
    """Seed under which hec_gpu_fill_splitmix writes shard ``shard`` of a
    stripe seeded ``seed_base`` on its own: word n of the stripe stream is
    mix(seed + (n + 1) * gamma), so the stream from word shard * L / 8 on is
    the stream of seed + shard * (L / 8) * gamma (L a multiple of 8)."""
    if shard_len % 8:
        raise ValueError("shard_len must be a multiple of 8")
    return (seed_base + shard * (shard_len // 8) * _GOLDEN) & ((1 << 64) - 1)


def fill_stripes_splitmix(t: torch.Tensor, data_shards: int, seed_base: int, stream=None) -> None:
    """The data shards of ``t[S, total, L]`` get exactly the bytes
    ``fill_splitmix`` writes into a packed batch (stripe s = one splitmix64
    stream of data_shards * L bytes), whatever the shard stride: shard i of a
    stripe is that stream from word i * L / 8 on, i.e. the same generator with
    its seed advanced by i * L / 8 golden-ratio steps (hec.h)."""
    if t.dim() != 3 or t.stride(2) != 1 or data_shards > t.shape[1]:
        raise ValueError("expected [stripes, shards, L] with contiguous shards")
    L = t.shape[2]
    if t.stride(1) == L:
        fill_splitmix(t, data_shards * L, seed_base, stream)
        return
    if L % 8:
        raise ValueError("a padded batch needs shard_len % 8 == 0 (the generator emits 8-byte words)")
    for i in range(data_shards):
        fill_splitmix(t[:, i], L, shard_seed(seed_base, i, L), stream)
