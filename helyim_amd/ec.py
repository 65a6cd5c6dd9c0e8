"""helyim_ec crate surface for the hot path (GPU-backed).

Constants mirror /root/reference/helyim-ec/src/lib.rs:44-50 and ``to_ext``
lib.rs:84-86; ``write_ec_files`` / ``rebuild_ec_files`` mirror
encoder.rs:39-50 (called by helyim-store/src/server.rs:468 and :497).
Errors are ``helyim_amd.errors.EcShardError`` subclasses, with RS errors
wrapped as ``ErasureCoding`` like errors.rs:58-59.
"""
from __future__ import annotations

import ctypes
from typing import List

from . import _lib
from .errors import check, check_ec

lib = _lib.lib

DATA_SHARDS_COUNT = 10
PARITY_SHARDS_COUNT = 4
TOTAL_SHARDS_COUNT = DATA_SHARDS_COUNT + PARITY_SHARDS_COUNT
ERASURE_CODING_LARGE_BLOCK_SIZE = 1024 * 1024 * 1024
ERASURE_CODING_SMALL_BLOCK_SIZE = 1024 * 1024


def to_ext(ec_idx: int) -> str:
    return ".ec%02d" % ec_idx


def ec_shard_filename(collection: str, dir: str, volume_id: int) -> str:
    """Base path of a volume's shard files (shard.rs:51-57): ``dir/vid`` or
    ``dir/collection_vid``; append ``to_ext(shard_id)`` for one shard."""
    return "%s/%d" % (dir, volume_id) if not collection else "%s/%s_%d" % (dir, collection, volume_id)


def ec_shard_base_filename(collection: str, volume_id: int) -> str:
    """Directory-less base name (shard.rs:59-65)."""
    return "%d" % volume_id if not collection else "%s_%d" % (collection, volume_id)


def write_ec_files(base_filename: str) -> None:
    """base.dat -> base.ec00 .. base.ec13 (encoder.rs:39-46)."""
    check_ec(lib.hec_write_ec_files(base_filename.encode()))


def generate_ec_files(base_filename: str, buf_size: int, large_block_size: int,
                      small_block_size: int) -> None:
    """encoder.rs:52-71 with explicit geometry (tests shrink the blocks)."""
    check_ec(lib.hec_write_ec_files_ex(base_filename.encode(), buf_size, large_block_size,
                                       small_block_size))


def rebuild_ec_files(base_filename: str) -> List[int]:
    """Recreate missing .ecNN files; returns the rebuilt shard ids (encoder.rs:48-50)."""
    ids = (ctypes.c_uint32 * TOTAL_SHARDS_COUNT)()
    n = ctypes.c_size_t(0)
    check_ec(lib.hec_rebuild_ec_files(base_filename.encode(), ids, ctypes.byref(n)))
    return [int(ids[i]) for i in range(n.value)]


class _ScrubBad(ctypes.Structure):
    """include/hec.h ``hec_scrub_bad``."""
    _fields_ = [("offset", ctypes.c_uint64), ("length", ctypes.c_uint32), ("parity_mask", ctypes.c_uint32)]


def verify_ec_files(base_filename: str, block_size: int = 0, cap: int = 1024):
    """Scrub base.ec00 .. base.ec13 on the GPU (hec_verify_ec_files): the files
    are checked as 14 byte streams in column blocks of ``block_size`` bytes
    (0 = 1 MiB). Returns ``(n_blocks, n_bad, bad)``: blocks checked, blocks
    whose stored parity differs from their data's (the total), and the first
    ``min(cap, n_bad)`` of them as ``(offset, length, parity_mask)`` in
    ascending offset (bit j of the mask = .ec(10+j) differs). Reads only."""
    if cap < 0:
        raise ValueError("negative cap")
    bad = (_ScrubBad * cap)() if cap else None
    n_bad, n_blocks = ctypes.c_size_t(0), ctypes.c_uint64(0)
    check_ec(lib.hec_verify_ec_files(base_filename.encode(), block_size, bad, cap, ctypes.byref(n_bad),
                                     ctypes.byref(n_blocks)))
    got = min(cap, n_bad.value)
    return (int(n_blocks.value), int(n_bad.value),
            [(int(bad[i].offset), int(bad[i].length), int(bad[i].parity_mask)) for i in range(got)])


class _ScrubSuspect(ctypes.Structure):
    """include/hec.h ``hec_scrub_suspect``."""
    _fields_ = [("offset", ctypes.c_uint64), ("length", ctypes.c_uint32), ("parity_mask", ctypes.c_uint32),
                ("suspects", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


def _locate_files(call, base_filename: str, block_size: int, cap: int):
    """One of the two full-volume file locates -> (n_blocks, n_bad, entries)."""
    if cap < 0:
        raise ValueError("negative cap")
    bad = (_ScrubSuspect * cap)() if cap else None
    n_bad, n_blocks = ctypes.c_size_t(0), ctypes.c_uint64(0)
    check_ec(call(base_filename.encode(), block_size, bad, cap, ctypes.byref(n_bad), ctypes.byref(n_blocks)))
    got = min(cap, n_bad.value)
    return (int(n_blocks.value), int(n_bad.value),
            [(int(bad[i].offset), int(bad[i].length), int(bad[i].parity_mask), int(bad[i].suspects))
             for i in range(got)])


def locate_corrupt_ec_files(base_filename: str, block_size: int = 0, cap: int = 1024):
    """verify_ec_files that also names the corrupt file of each bad block
    (hec_locate_corrupt_ec_files). Returns ``(n_blocks, n_bad, bad)`` with
    entries ``(offset, length, parity_mask, suspects)``: bit c of suspects =
    ``.ec(c)`` alone explains a byte column of the block, bit 31 = a column no
    single file explains. Reads only: to repair, delete the named ``.ecNN``
    and call ``rebuild_ec_files``."""
    return _locate_files(lib.hec_locate_corrupt_ec_files, base_filename, block_size, cap)


def locate_corrupt_pairs_ec_files(base_filename: str, block_size: int = 0, cap: int = 1024):
    """locate_corrupt_ec_files that also names two files per byte column
    (hec_locate_corrupt_pairs_ec_files): the same result shape; a column that
    ``.ec(a)`` and ``.ec(b)`` together explain sets bits a and b, bit 31 = a
    column no one or two files explain. Reads only: when the named files
    number at most four over all blocks and bit 31 is clear everywhere, delete
    them and call ``rebuild_ec_files``. Three wrong files in one column may
    name an intact pair (include/hec.h); the stricter call is
    locate_corrupt_ec_files."""
    return _locate_files(lib.hec_locate_corrupt_pairs_ec_files, base_filename, block_size, cap)


def correct_ec_files(base_filename: str, block_size: int = 0, cap: int = 1024, pairs: bool = False):
    """locate_corrupt_ec_files that also fixes what it explains, in the files
    (hec_correct_ec_files; ``pairs=True``: hec_correct_pairs_ec_files, which
    also fixes columns two files explain). The same result shape, with the
    words from before the correction. Of each bad block only the files its
    suspects word names are rewritten, at the block's offset; a column that
    sets bit 31 keeps its bytes. A file that cannot be opened for writing
    raises ``Io`` before any device work."""
    call = lib.hec_correct_pairs_ec_files if pairs else lib.hec_correct_ec_files
    return _locate_files(call, base_filename, block_size, cap)


def _scrub_present(call, head, cap):
    """One of the degraded file scrubs: call(*head, bad, cap, &n_bad, &n_blocks,
    &present_mask) -> (n_blocks, n_bad, bad, present_mask)."""
    if cap < 0:
        raise ValueError("negative cap")
    bad = (_ScrubSuspect * cap)() if cap else None
    n_bad, n_blocks, present = ctypes.c_size_t(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    check_ec(call(*head, bad, cap, ctypes.byref(n_bad), ctypes.byref(n_blocks), ctypes.byref(present)))
    got = min(cap, n_bad.value)
    return (int(n_blocks.value), int(n_bad.value),
            [(int(bad[i].offset), int(bad[i].length), int(bad[i].parity_mask), int(bad[i].suspects))
             for i in range(got)], int(present.value))


def locate_corrupt_ec_files_present(base_filename: str, block_size: int = 0, cap: int = 1024):
    """locate_corrupt_ec_files for a degraded volume
    (hec_locate_corrupt_ec_files_present): missing ``.ecNN`` files are erased
    shards. Returns ``(n_blocks, n_bad, bad, present_mask)``; entries are
    ``(offset, length, check, suspects)`` with bits by file index 0..13 (the
    masked verify's and locate's words). Needs 11 or more files
    (``ErasureCoding(TooFewShardsPresent)`` below that, ``ShardNotFound`` with none). Reads
    only. To repair: when blocks name files and bit 31 is clear everywhere,
    delete the named files too (at most four missing in all), call
    ``rebuild_ec_files``, scrub again; ``correct_ec_files_present`` heals
    scattered damage in the survivors in place instead."""
    return _scrub_present(lib.hec_locate_corrupt_ec_files_present, (base_filename.encode(), block_size), cap)


def correct_ec_files_present(base_filename: str, block_size: int = 0, min_spares: int = 2, cap: int = 1024):
    """locate_corrupt_ec_files_present that also fixes what it explains, in the
    present files (hec_correct_ec_files_present). The same result shape, with
    the words from before the correction. Of each bad block only the present
    files its suspects word names are rewritten, at the block's offset; a
    column that sets bit 31 keeps its bytes; a missing file is not created.
    min_spares (2, 3 or 4): a volume with fewer spare files is only located
    (with two spares, two wrong files in one byte column may be taken for an
    intact one, which is then written: include/hec.h has the rates; 3 rules
    that out). A present file that cannot be opened for writing raises ``Io``
    before any device work. The recipe for a degraded volume: this call, then
    ``rebuild_ec_files`` when bit 31 is clear everywhere, then scrub again."""
    return _scrub_present(lib.hec_correct_ec_files_present, (base_filename.encode(), block_size, min_spares), cap)


# --- EC volume files around the shards (helyim-ec host-side byte formats) ---

def write_sorted_file_from_index(base_filename: str, ext: str = ".ecx") -> None:
    """.idx -> sorted .ecx (encoder.rs:21-37). Raises Io like EcVolumeError::Io."""
    check(lib.hec_write_sorted_file_from_index(base_filename.encode(), ext.encode()))


def rebuild_ecx_file(base_filename: str) -> None:
    """Apply .ecj tombstones to .ecx, delete .ecj (lib.rs:95-133)."""
    check(lib.hec_rebuild_ecx_file(base_filename.encode()))


def save_volume_info(filename: str, version: int) -> None:
    """.vif as the generate RPC writes it (server.rs:470-475)."""
    check(lib.hec_save_volume_info(filename.encode(), version))


def find_data_filesize(base_filename: str) -> int:
    """decoder.rs:46-66."""
    out = ctypes.c_uint64(0)
    check(lib.hec_find_data_filesize(base_filename.encode(), ctypes.byref(out)))
    return int(out.value)


def write_data_file(base_filename: str, data_filesize: int) -> None:
    """.ec00-.ec09 -> .dat (decoder.rs:142-180)."""
    check(lib.hec_write_data_file(base_filename.encode(), data_filesize))


def write_index_file_from_ec_index(base_filename: str) -> None:
    """.ecx + .ecj -> .idx (decoder.rs:22-44)."""
    check(lib.hec_write_index_file_from_ec_index(base_filename.encode()))


def volume_ec_shards_generate(base_filename: str, version: int) -> None:
    """The body of the VolumeEcShardsGenerate RPC (helyim-store/src/server.rs:466-475):
    .ecx, then .ec00-.ec13, then .vif."""
    write_sorted_file_from_index(base_filename, ".ecx")
    write_ec_files(base_filename)
    save_volume_info(base_filename + ".vif", version)


def volume_ec_shards_rebuild(base_filename: str) -> List[int]:
    """The body of the VolumeEcShardsRebuild RPC for one location (server.rs:497-498)."""
    ids = rebuild_ec_files(base_filename)
    rebuild_ecx_file(base_filename)
    return ids


# ---- needle reads (locate + degraded read), SURVEY §8f rank 3 ----------------

class Interval(ctypes.Structure):
    """helyim_ec::locate::Interval (helyim-ec/src/locate.rs:3-27)."""
    _fields_ = [("block_index", ctypes.c_uint64), ("inner_block_offset", ctypes.c_uint64),
                ("size", ctypes.c_uint64), ("large_block_rows", ctypes.c_uint64),
                ("is_large_block", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def shard_id(self) -> int:
        return int(lib.hec_interval_shard_id(ctypes.byref(self)))

    def offset(self, large_block_size: int, small_block_size: int) -> int:
        return int(lib.hec_interval_offset(ctypes.byref(self), large_block_size, small_block_size))

    def as_tuple(self):
        return (self.block_index, self.inner_block_offset, self.size, bool(self.is_large_block),
                self.large_block_rows)


def locate_data(large_block_len: int, small_block_len: int, data_size: int, offset: int,
                size: int) -> List[Interval]:
    """locate_data (locate.rs:29-72)."""
    n = ctypes.c_size_t(0)
    rc = lib.hec_locate_data(large_block_len, small_block_len, data_size, offset, size, None, 0, ctypes.byref(n))
    if rc and n.value == 0:
        check(rc)
    out = (Interval * max(n.value, 1))()
    check(lib.hec_locate_data(large_block_len, small_block_len, data_size, offset, size, out, n.value,
                              ctypes.byref(n)))
    return list(out[:n.value])


def find_needle_from_ecx(base_filename: str, needle_id: int):
    """EcVolume::find_needle_from_ecx (volume/mod.rs:153-155): (offset, size) as stored."""
    off, size = ctypes.c_uint32(0), ctypes.c_int32(0)
    check_ec(lib.hec_find_needle_from_ecx(base_filename.encode(), needle_id, ctypes.byref(off), ctypes.byref(size)))
    return off.value, size.value


def read_ec_data(base_filename: str, ranges, large_block_size: int = ERASURE_CODING_LARGE_BLOCK_SIZE,
                 small_block_size: int = ERASURE_CODING_SMALL_BLOCK_SIZE) -> bytes:
    """read_ec_shard_intervals over [(offset, size), ...] of the volume's data,
    from the local base.ecNN files; intervals of missing shards are rebuilt on
    the GPU in one batch. Returns the ranges' bytes back to back."""
    ranges = list(ranges)
    n = len(ranges)
    offs = (ctypes.c_uint64 * max(n, 1))(*[r[0] for r in ranges])
    sizes = (ctypes.c_uint64 * max(n, 1))(*[r[1] for r in ranges])
    out = ctypes.create_string_buffer(max(sum(r[1] for r in ranges), 1))
    check_ec(lib.hec_read_ec_data(base_filename.encode(), large_block_size, small_block_size, offs, sizes, n, out))
    return out.raw[:sum(r[1] for r in ranges)]


def read_ec_needle(base_filename: str, needle_id: int, large_block_size: int = ERASURE_CODING_LARGE_BLOCK_SIZE,
                   small_block_size: int = ERASURE_CODING_SMALL_BLOCK_SIZE) -> bytes:
    """read_ec_shard_needle's data path (erasure_coding/mod.rs:129-171): the
    needle record's actual_size bytes (parse with the needle format)."""
    n = ctypes.c_size_t(0)
    name = base_filename.encode()
    rc = lib.hec_read_ec_needle_ex(name, large_block_size, small_block_size, needle_id, None, 0, ctypes.byref(n))
    if rc and n.value == 0:
        check_ec(rc)
    out = ctypes.create_string_buffer(max(n.value, 1))
    check_ec(lib.hec_read_ec_needle_ex(name, large_block_size, small_block_size, needle_id, out, n.value,
                                       ctypes.byref(n)))
    return out.raw[:n.value]


def read_ec_needles(base_filename: str, needle_ids, large_block_size: int = ERASURE_CODING_LARGE_BLOCK_SIZE,
                    small_block_size: int = ERASURE_CODING_SMALL_BLOCK_SIZE):
    """Many needle reads in one call (one GPU batch for every lost interval).
    Returns one entry per id: the needle's bytes, or the exception the single
    read would raise (``Io`` not in .ecx, ``NeedleNotFound`` deleted)."""
    from .errors import _EC
    ids = list(needle_ids)
    n = len(ids)
    c_ids = (ctypes.c_uint64 * max(n, 1))(*ids)
    offs = (ctypes.c_uint64 * (n + 1))()
    st = (ctypes.c_int * max(n, 1))()
    name = base_filename.encode()
    rc = lib.hec_read_ec_needles(name, large_block_size, small_block_size, c_ids, n, None, 0, offs, st)
    if rc and not (n and offs[n] > 0):
        check_ec(rc)
    out = ctypes.create_string_buffer(max(offs[n], 1))
    check_ec(lib.hec_read_ec_needles(name, large_block_size, small_block_size, c_ids, n, out, offs[n], offs, st))
    raw = out.raw
    res = []
    for i in range(n):
        if st[i]:
            res.append(_EC[st[i]]("Needle %d: %s" % (ids[i], _lib.strerror(st[i]))))
        else:
            res.append(raw[offs[i]:offs[i + 1]])
    return res


class EcVolume:
    """A mounted EC volume (EcVolume, helyim-ec/src/volume/mod.rs:30-171):
    .ecx / .ecj held open, every local base.ecNN mounted, so a stream of needle
    reads pays the lookup and the preads only. ``open`` follows EcVolume::new
    (a missing or file-less .vif is written with version 2)."""

    def __init__(self, base_filename: str, large_block_size: int = ERASURE_CODING_LARGE_BLOCK_SIZE,
                 small_block_size: int = ERASURE_CODING_SMALL_BLOCK_SIZE):
        h = ctypes.c_void_p()
        check_ec(lib.hec_ec_volume_open_ex(base_filename.encode(), large_block_size, small_block_size,
                                           ctypes.byref(h)))
        self._h = h

    def close(self) -> None:
        if self._h:
            lib.hec_ec_volume_close(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def version(self) -> int:
        return int(lib.hec_ec_volume_version(self._h))

    def shard_ids(self) -> List[int]:
        bits = lib.hec_ec_volume_shard_bits(self._h)
        return [i for i in range(TOTAL_SHARDS_COUNT) if (bits >> i) & 1]

    def find_needle_from_ecx(self, needle_id: int):
        off, size = ctypes.c_uint32(0), ctypes.c_int32(0)
        check_ec(lib.hec_ec_volume_find_needle(self._h, needle_id, ctypes.byref(off), ctypes.byref(size)))
        return off.value, size.value

    def delete_needle_from_ecx(self, needle_id: int) -> None:
        check_ec(lib.hec_ec_volume_delete_needle(self._h, needle_id))

    def read_needle(self, needle_id: int) -> bytes:
        n = ctypes.c_size_t(0)
        rc = lib.hec_ec_volume_read_needle(self._h, needle_id, None, 0, ctypes.byref(n))
        if rc and n.value == 0:
            check_ec(rc)
        out = ctypes.create_string_buffer(max(n.value, 1))
        check_ec(lib.hec_ec_volume_read_needle(self._h, needle_id, out, n.value, ctypes.byref(n)))
        return out.raw[:n.value]

    def read_needles(self, needle_ids):
        """As read_ec_needles: one entry per id, bytes or the exception."""
        from .errors import _EC
        ids = list(needle_ids)
        n = len(ids)
        c_ids = (ctypes.c_uint64 * max(n, 1))(*ids)
        offs = (ctypes.c_uint64 * (n + 1))()
        st = (ctypes.c_int * max(n, 1))()
        rc = lib.hec_ec_volume_read_needles(self._h, c_ids, n, None, 0, offs, st)
        if rc and not (n and offs[n] > 0):
            check_ec(rc)
        out = ctypes.create_string_buffer(max(offs[n], 1))
        check_ec(lib.hec_ec_volume_read_needles(self._h, c_ids, n, out, offs[n], offs, st))
        raw = out.raw
        return [_EC[st[i]]("Needle %d: %s" % (ids[i], _lib.strerror(st[i]))) if st[i] else raw[offs[i]:offs[i + 1]]
                for i in range(n)]
