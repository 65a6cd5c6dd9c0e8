"""The ragged update entry points without a GPU: the symbols, the descriptor's
layout, and every argument and codec check that precedes device work, in the
order include/hec.h states (fake non-null pointers are never touched)."""
import ctypes
import os
import re

import numpy as np
import pytest

from abi_util import L, P, c_parameters, codes, has_gpu
from conftest import ROOT

C = codes()
INVALID_ARGUMENT, EMPTY_SHARD, NO_DEVICE, HIP = (C["HEC_ERR_INVALID_ARGUMENT"], C["HEC_ERR_EMPTY_SHARD"],
                                                 C["HEC_ERR_NO_DEVICE"], C["HEC_ERR_HIP"])
NEW = ("hec_gpu_update_ragged", "hec_rs_update_batch", "hec_update_ragged_kernel_name")
Q, O = P + (1 << 30), P + (2 << 30)  # two more fake arenas
FIELDS = ("parity_offset", "parity_stride", "new_offset", "new_stride", "old_offset", "old_stride", "shard_len",
          "update_mask")


def eight(**change):
    """Eight valid stripes; change = {"<field><stripe>": value}, e.g. shard_len3=0."""
    import helyim_amd.batch as B
    rows = []
    for s in range(8):
        ln = (L, 1000, 17, 4097)[s % 4]
        stride = (ln + 15) // 16 * 16 + 16
        rows.append(dict(parity_offset=s * 4 * 8192, parity_stride=stride, new_offset=s * 10 * 8192, new_stride=stride,
                         old_offset=s * 10 * 8192, old_stride=stride, shard_len=ln, update_mask=1 << s))
    for key, value in change.items():
        field, s = key[:-1], int(key[-1])
        assert field in FIELDS, key
        rows[s][field] = value
    return np.array([tuple(r[f] for f in FIELDS) for r in rows], dtype=B.update_desc_dtype())


def ragged(rs, old=O, new=Q, par=P, descs="eight", n=None, **change):
    import helyim_amd as H
    d = eight(**change) if isinstance(descs, str) else descs
    return H.lib.hec_gpu_update_ragged(rs, old, new, par, None if d is None else d.ctypes.data,
                                       (0 if d is None else len(d)) if n is None else n, None)


def test_symbols_and_signatures():
    import helyim_amd as H
    from helyim_amd import _lib, batch
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hec.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "hec-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert hasattr(H.lib, name), name
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(c_parameters(header, name)), name
        assert "pub fn %s(" % name in rust, name
    assert c_parameters(header, NEW[0]) == ["const hec_rs_t* rs", "const uint8_t* d_old", "const uint8_t* d_new",
                                            "uint8_t* d_parity", "const hec_update_desc* descs", "uint32_t n_stripes",
                                            "void* stream"]
    assert c_parameters(header, NEW[1]) == ["const hec_rs_t* rs", "uint8_t* const* shards", "const size_t* lens",
                                            "const uint8_t* const* new_data", "size_t n_stripes", "size_t* bad_index"]
    assert c_parameters(header, NEW[2]) == ["int with_old"]
    assert "pub struct hec_update_desc" in rust
    for name in ("update_desc_dtype", "update_ragged", "update_descs_in_place", "update_ragged_kernel_name"):
        assert callable(getattr(batch, name)), name
    assert callable(H.ReedSolomon.update_batch)
    assert "pub fn update_batch(" in open(os.path.join(ROOT, "rust", "helyim-ec-hip", "src", "lib.rs")).read()


def test_descriptor_layout():
    """hec_update_desc as the header declares it: 56 bytes, six 64-bit words and two 32-bit ones."""
    import helyim_amd.batch as B
    header = open(os.path.join(ROOT, "include", "hec.h")).read()
    body = re.search(r"typedef struct hec_update_desc \{(.*?)\} hec_update_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for ctype, names in re.findall(r"(uint64_t|uint32_t)\s+([^;]+);", body):
        declared += [(n.strip(), ctype) for n in names.split(",")]
    assert [n for n, _ in declared] == list(FIELDS)

    class Desc(ctypes.Structure):
        _fields_ = [(n, ctypes.c_uint64 if t == "uint64_t" else ctypes.c_uint32) for n, t in declared]

    assert ctypes.sizeof(Desc) == 56
    assert [getattr(Desc, n).offset for n in FIELDS] == [0, 8, 16, 24, 32, 40, 48, 52]
    dt = B.update_desc_dtype()
    assert dt.itemsize == 56 and dt.names == FIELDS
    assert [dt.fields[n][1] for n in FIELDS] == [0, 8, 16, 24, 32, 40, 48, 52]


def test_device_call_errors_before_device_work_in_order():
    import helyim_amd as H
    codec = H.ReedSolomon(10, 4)  # kept alive: the handle dies with it
    rs = codec.handle
    other = H.ReedSolomon(10, 2)
    assert ragged(rs, n=0) == 0
    assert ragged(rs, descs=None) == 0   # no stripes, no list
    # 1. the nulls, also with no stripes
    assert ragged(None) == INVALID_ARGUMENT
    for pointer in ("new", "par"):
        assert ragged(rs, **{pointer: None}) == INVALID_ARGUMENT, pointer
        assert "null" in H._lib.last_detail()
        assert ragged(rs, n=0, **{pointer: None}) == INVALID_ARGUMENT, pointer
    assert ragged(rs, descs=None, n=3) == INVALID_ARGUMENT and "null" in H._lib.last_detail()
    # a null pointer wins over the codec
    assert ragged(other.handle, new=None) == INVALID_ARGUMENT and "null" in H._lib.last_detail()
    assert ragged(other.handle, descs=None, n=2) == INVALID_ARGUMENT and "null" in H._lib.last_detail()
    # 2. the codec wins over an empty shard
    assert ragged(other.handle, shard_len0=0) == INVALID_ARGUMENT and "RS(10,4) only" in H._lib.last_detail()
    # 3. per descriptor in index order: stripe 3's empty shard wins over stripe 5's misalignment
    assert ragged(rs, shard_len3=0, new_offset5=8) == EMPTY_SHARD and "stripe 3" in H._lib.last_detail()
    assert ragged(rs, new_offset3=8, shard_len5=0) == INVALID_ARGUMENT and "stripe 3" in H._lib.last_detail()
    assert ragged(rs, shard_len3=0, update_mask3=0) == EMPTY_SHARD    # whether U is empty or not
    assert ragged(rs, new_stride6=8, update_mask6=0) == INVALID_ARGUMENT and "stripe 6" in H._lib.last_detail()
    # within a descriptor the empty shard comes first
    assert ragged(rs, shard_len2=0, parity_offset2=4) == EMPTY_SHARD and "stripe 2" in H._lib.last_detail()
    for arena in ("parity", "new", "old"):
        assert ragged(rs, **{arena + "_offset4": 8}) == INVALID_ARGUMENT, arena
        assert "stripe 4" in H._lib.last_detail()
        assert ragged(rs, **{arena + "_stride4": 24}) == INVALID_ARGUMENT, arena       # misaligned
        assert ragged(rs, **{arena + "_stride1": 992}) == INVALID_ARGUMENT, arena      # aligned, below shard_len 1000
        assert "stripe 1" in H._lib.last_detail()
        # the extent wraps 64 bits: offset + shards * stride
        shards = 4 if arena == "parity" else 10
        top = ((1 << 64) // shards + 15) // 16 * 16
        assert ragged(rs, **{arena + "_stride7": top}) == INVALID_ARGUMENT, arena
        assert ragged(rs, **{arena + "_offset7": (1 << 64) - 4096}) == INVALID_ARGUMENT, arena
    for pointer in ("old", "new", "par"):  # a misaligned base
        assert ragged(rs, **{pointer: P + 8}) == INVALID_ARGUMENT, pointer
        assert "stripe 0" in H._lib.last_detail()
    # 4. more than 2^32 column ranges in total: 4096 stripes of 2^32 - 16 bytes own 2^32 ranges, one more is too many
    import helyim_amd.batch as B
    big = np.zeros(4097, dtype=B.update_desc_dtype())
    for arena in ("parity", "new", "old"):
        big[arena + "_stride"] = 1 << 32
    big["shard_len"], big["update_mask"] = (1 << 32) - 16, 1
    assert ragged(rs, descs=big) == INVALID_ARGUMENT and "2^32" in H._lib.last_detail()
    # a broken descriptor in front of the one that passes the limit wins; stripes with U empty own no range
    big["shard_len"][4000] = 0
    assert ragged(rs, descs=big) == EMPTY_SHARD and "stripe 4000" in H._lib.last_detail()
    big["shard_len"][4000], big["new_stride"][4096] = 16, 8
    assert ragged(rs, descs=big) == INVALID_ARGUMENT and "stripe 4096" in H._lib.last_detail()


def test_old_arena_fields_are_ignored_without_an_old_arena():
    import helyim_amd as H
    codec = H.ReedSolomon(10, 4)
    rs = codec.handle
    junk = dict(old_offset2=7, old_stride2=3, old_offset5=(1 << 64) - 1, old_stride5=(1 << 64) - 1)
    assert ragged(rs, **junk) == INVALID_ARGUMENT and "stripe 2" in H._lib.last_detail()
    # without d_old they mean nothing: the call gets as far as the device (every mask empty, so
    # that a machine with a GPU launches nothing over the fake pointers)
    empty = {"update_mask%d" % s: 0xFC00 for s in range(8)}
    rc = ragged(rs, old=None, **junk, **empty)
    assert rc in ((0,) if has_gpu() else (NO_DEVICE, HIP)), rc
    assert ragged(rs, **junk, **empty) == INVALID_ARGUMENT
    # the other arenas are still checked
    assert ragged(rs, old=None, new_offset2=8, **junk) == INVALID_ARGUMENT


@pytest.mark.parametrize("k,m", [(5, 5), (10, 2), (10, 6)])
def test_other_codecs_are_refused_by_the_device_call(k, m):
    import helyim_amd as H
    codec = H.ReedSolomon(k, m)
    rs = codec.handle
    assert ragged(rs) == INVALID_ARGUMENT and "RS(10,4) only" in H._lib.last_detail()
    assert ragged(rs, n=0) == INVALID_ARGUMENT and "RS(10,4) only" in H._lib.last_detail()
    assert ragged(rs, old=None) == INVALID_ARGUMENT
    assert ragged(rs, par=None) == INVALID_ARGUMENT and "null" in H._lib.last_detail()


def host_batch(rs, k, m, stripes, bad=True, null_array=None, n=None):
    """hec_rs_update_batch on real host buffers. stripes: dicts with changed
    (data shards with a new_data entry), null (shard slots passed as NULL), lens
    (per-slot lengths) and n_bytes -> (status, *bad_index, the buffers)."""
    import helyim_amd as H
    total = k + m
    bufs, news, ptrs, lens, nws = [], [], [], [], []
    for st in stripes:
        nb = st.get("n_bytes", 64)
        b = [np.full(nb, 0x11 * (i + 1) & 0xFF, dtype=np.uint8) for i in range(total)]
        w = [np.full(nb, 0xC3, dtype=np.uint8) for _ in range(k)]
        bufs.append(b)
        news.append(w)
        ptrs += [None if i in st.get("null", ()) else x.ctypes.data for i, x in enumerate(b)]
        lens += list(st.get("lens") or [nb] * total)
        nws += [w[c].ctypes.data if c in st.get("changed", ()) else None for c in range(k)]
    S = len(stripes)
    a_ptrs = (ctypes.c_void_p * max(1, S * total))(*ptrs)
    a_lens = (ctypes.c_size_t * max(1, S * total))(*lens)
    a_news = (ctypes.c_void_p * max(1, S * k))(*nws)
    arrays = [None if null_array == i else a for i, a in enumerate((a_ptrs, a_lens, a_news))]
    out = ctypes.c_size_t(12345)
    rc = H.lib.hec_rs_update_batch(rs.handle, *arrays, S if n is None else n, ctypes.byref(out) if bad else None)
    return rc, out.value, bufs


def untouched(bufs):
    return all((b == (0x11 * (i + 1) & 0xFF)).all() for st in bufs for i, b in enumerate(st))


@pytest.mark.parametrize("k,m", [(10, 4), (5, 3)])
def test_host_batch_validation_in_order(k, m):
    import helyim_amd as H
    rs, n = H.ReedSolomon(k, m), k + m
    good = dict(changed=())
    assert H.lib.hec_rs_update_batch(None, None, None, None, 0, None) == INVALID_ARGUMENT
    for i in range(3):
        assert host_batch(rs, k, m, [good], null_array=i)[0] == INVALID_ARGUMENT
        assert "null" in H._lib.last_detail()
    # no stripes: fine with null arrays, and *bad_index = n_stripes = 0
    assert H.lib.hec_rs_update_batch(rs.handle, None, None, None, 0, None) == 0
    rc, bad, _ = host_batch(rs, k, m, [], n=0)
    assert (rc, bad) == (0, 0)
    # per stripe hec_rs_update's order: the pointers before the lengths
    zero = [0] * n
    rc, bad, bufs = host_batch(rs, k, m, [good, good, dict(changed=(1,), null=(1,), lens=zero), dict(lens=zero)])
    assert (rc, bad) == (INVALID_ARGUMENT, 2) and "old buffer" in H._lib.last_detail() and untouched(bufs)
    rc, bad, _ = host_batch(rs, k, m, [good, dict(changed=(1,), null=(n - 1,), lens=zero)])
    assert (rc, bad) == (INVALID_ARGUMENT, 1) and "parity" in H._lib.last_detail()
    rc, bad, _ = host_batch(rs, k, m, [dict(changed=(), null=(k,))])   # the parity is required even for a no-op
    assert (rc, bad) == (INVALID_ARGUMENT, 0)
    # the lengths in use: the changed shards' old slots and the parity
    lens = [64] * n
    lens[1] = 0
    rc, bad, _ = host_batch(rs, k, m, [good, good, good, dict(changed=(1,), lens=lens)])
    assert (rc, bad) == (EMPTY_SHARD, 3) and "stripe 3" in H._lib.last_detail()
    lens[1], lens[k] = 64, 65
    rc, bad, _ = host_batch(rs, k, m, [dict(changed=(1,), lens=lens), dict(changed=(1,), null=(1,))])
    assert (rc, bad) == (C["HEC_ERR_INCORRECT_SHARD_SIZE"], 0)   # the first failing stripe, not the worst
    lens[k], lens[n - 1] = 64, 63
    rc, bad, _ = host_batch(rs, k, m, [good, dict(changed=(), lens=lens)])
    assert (rc, bad) == (C["HEC_ERR_INCORRECT_SHARD_SIZE"], 1)
    # an empty shard wins over the length limit; the limit is an invalid argument
    if ctypes.sizeof(ctypes.c_size_t) == 8:
        huge = [1 << 32] * n
        rc, bad, _ = host_batch(rs, k, m, [good, dict(changed=(0,), lens=huge)])
        assert (rc, bad) == (INVALID_ARGUMENT, 1) and "2^32" in H._lib.last_detail()
        huge[k] = 0
        assert host_batch(rs, k, m, [dict(changed=(0,), lens=huge)])[0] == EMPTY_SHARD
    # the optional index may be null
    assert host_batch(rs, k, m, [dict(changed=(1,), null=(1,))], bad=False)[0] == INVALID_ARGUMENT


@pytest.mark.parametrize("k,m", [(10, 4), (5, 3)])
def test_host_batch_without_a_changed_shard_needs_no_device(k, m):
    import helyim_amd as H
    rs = H.ReedSolomon(k, m)
    # lengths and pointers of unused old slots are ignored
    lens = [0, 7, 9] + [5] * (k - 3) + [64] * m
    rc, bad, bufs = host_batch(rs, k, m, [dict(changed=(), lens=lens, null=(0, 2)), dict(changed=()), dict(changed=())])
    assert (rc, bad) == (0, 3) and untouched(bufs)


def test_kernel_names():
    import helyim_amd as H
    from helyim_amd import batch
    with_old, without = batch.update_ragged_kernel_name(True), batch.update_ragged_kernel_name(False)
    assert with_old.startswith("rs104_ragged_update_kernel<HAS_OLD=true>") and "XCD eighths" in with_old
    assert without.startswith("rs104_ragged_update_kernel<HAS_OLD=false>") and "XCD eighths" in without
    assert H.lib.hec_update_ragged_kernel_name(7).decode() == with_old


def test_python_mirror_checks_its_arguments():
    import torch

    import helyim_amd as H
    from helyim_amd import batch
    rs = H.ReedSolomon(10, 4)
    host = torch.zeros(1 << 16, dtype=torch.uint8)
    row = (0, 64, 0, 64, 0, 64, 64, 1)
    with pytest.raises(TypeError):   # host tensors are not device arenas
        batch.update_ragged(rs, None, host, host, [row])
    with pytest.raises(ValueError):  # seven fields
        batch.update_ragged(rs, None, host, host, [row[:7]])
    with pytest.raises(ValueError):
        batch.update_descs_in_place([(0, 64, 64, 0x3FFF)], [(0, 64, 64, 0)], [1, 2])
    with pytest.raises(ValueError):
        rs.update_batch([([np.zeros(8, np.uint8)] * 14, [None] * 9)])
    with pytest.raises(ValueError):
        rs.update_batch([([np.zeros(8, np.uint8)] * 14, [np.zeros(9, np.uint8)] + [None] * 9)])
    with pytest.raises(H.TooFewShards) as e:
        rs.update_batch([([np.zeros(8, np.uint8)] * 14, [None] * 10), ([np.zeros(8, np.uint8)] * 13, [None] * 10)])
    assert e.value.stripe == 1
    with pytest.raises(H.IncorrectShardSize) as e:   # the library's error carries the stripe
        shards = [np.zeros(8, np.uint8) for _ in range(14)]
        odd = [np.zeros(8, np.uint8) for _ in range(13)] + [np.zeros(9, np.uint8)]
        rs.update_batch([(shards, [None] * 10), (odd, [None] * 10)])
    assert e.value.stripe == 1
    rs.update_batch([])
    rs.update_batch([([None] * 10 + [np.zeros(8, np.uint8)] * 4, [None] * 10)])  # nothing changed: no device needed


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU error path")
def test_no_device_is_an_error_not_a_fallback():
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    assert ragged(rs.handle) in (NO_DEVICE, HIP)
    assert ragged(rs.handle, old=None) in (NO_DEVICE, HIP)
    for k, m in ((10, 4), (5, 3)):
        rc, bad, bufs = host_batch(H.ReedSolomon(k, m), k, m, [dict(changed=()), dict(changed=(0, k - 1))])
        assert rc in (NO_DEVICE, HIP) and untouched(bufs)
