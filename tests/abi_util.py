"""What the per-feature test_*_abi.py modules share -- TEST INFRASTRUCTURE ONLY
(not collected): the status codes of include/hec.h by name, the header's
parameter lists, fake-pointer calls of the device entry points by argument-list
family, and the empty shard files the file checks run on. No call made here
touches a device: the pointers are fake, and the checks under test come first."""
import os
import re

import numpy as np

from conftest import ROOT, has_gpu  # noqa: F401  (has_gpu: for the modules' skipif marks)

HEADER = open(os.path.join(ROOT, "include", "hec.h")).read()
CODES = dict((k, int(v)) for k, v in re.findall(r"\b(HEC_(?:OK|ERR_\w+))\s*=\s*(\d+)", HEADER))
INVALID_ARGUMENT, NO_DEVICE, IO = CODES["HEC_ERR_INVALID_ARGUMENT"], CODES["HEC_ERR_NO_DEVICE"], CODES["HEC_ERR_IO"]
EMPTY_SHARD, TOO_FEW_PRESENT = CODES["HEC_ERR_EMPTY_SHARD"], CODES["HEC_ERR_TOO_FEW_SHARDS_PRESENT"]
EC_SHARD_SIZE, SHARD_NOT_FOUND = CODES["HEC_ERR_UNEXPECTED_EC_SHARD_SIZE"], CODES["HEC_ERR_SHARD_NOT_FOUND"]

P, L, FULL = 0x1000, 4096, 0x3FFF  # a fake non-null pointer, the default shard length, all 14 shards present


def codes():
    return CODES


def c_parameters(header, name):
    m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, header, flags=re.S)
    assert m, name
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


# ---- fake-pointer calls ------------------------------------------------------------
SPLIT = dict(data=P, ds=14 * L, dsh=L, par=P + 10 * L, ps=14 * L, psh=L, length=L, n=2)   # data and parity apart
IN_PLACE = dict(shards=P, st=14 * L, sh=L, length=L, n=2)                                 # 14 shards, one base
# entry point -> (leading arguments, the arguments after them: fake pointers but for spares = 2,
#                 trailing counters and stream passed as null)
STRIDED = {
    "hec_gpu_verify_batch": (SPLIT, ("res",), 2),
    "hec_host_verify_batch": (SPLIT, ("res",), 1),
    "hec_gpu_locate_corrupt_batch": (SPLIT, ("res", "sus"), 2),
    "hec_gpu_locate_corrupt_pairs_batch": (SPLIT, ("res", "sus"), 2),
    "hec_gpu_correct_batch": (SPLIT, ("res", "sus"), 4),
    "hec_gpu_correct_pairs_batch": (SPLIT, ("res", "sus"), 4),
    "hec_gpu_repair_batch": (IN_PLACE, ("res", "sus", "masks"), 2),
    "hec_gpu_repair_pairs_batch": (IN_PLACE, ("res", "sus", "masks"), 2),
    "hec_gpu_verify_present_batch": (IN_PLACE, ("masks", "res"), 3),
    "hec_gpu_locate_corrupt_present_batch": (IN_PLACE, ("masks", "res", "sus"), 3),
    "hec_gpu_reconstruct_checked_batch": (IN_PLACE, ("masks", "res", "sus", "use"), 3),
    "hec_gpu_correct_present_batch": (IN_PLACE, ("masks", "spares", "res", "sus"), 5),
    "hec_gpu_reconstruct_corrected_batch": (IN_PLACE, ("masks", "spares", "res", "sus", "use"), 4),
    "hec_gpu_reconstruct_some_batch": (IN_PLACE, ("masks", "wants"), 2),
    "hec_host_reconstruct_some_batch": (IN_PLACE, ("masks", "wants"), 1),
}
# ragged entry point -> (word arrays, takes min_spares, trailing nulls)
RAGGED = {
    "hec_gpu_verify_ragged": (("res",), False, 3),
    "hec_gpu_locate_corrupt_ragged": (("res", "sus"), False, 3),
    "hec_gpu_correct_ragged": (("res", "sus"), True, 5),
    "hec_gpu_reconstruct_corrected_ragged": (("res", "sus", "use"), True, 4),
}


def call(name, rs, **overrides):
    """A strided entry point on fake pointers; overrides by argument name."""
    import helyim_amd as H
    head, rest, tail = STRIDED[name]
    args = dict(head, **{a: 2 if a == "spares" else P for a in rest})
    assert set(overrides) <= set(args), (name, sorted(set(overrides) - set(args)))
    args.update(overrides)
    return getattr(H.lib, name)(rs, *args.values(), *([None] * tail))


def descs_of(rows):
    import helyim_amd.batch as B
    return np.array([tuple(r) for r in rows], dtype=B.desc_dtype())


def two(**change):
    """Two valid stripes back to back; change = fields of stripe 1."""
    rows = [dict(offset=0, shard_stride=4096, shard_len=4096, present_mask=FULL),
            dict(offset=14 * 4096, shard_stride=1008, shard_len=1000, present_mask=FULL & ~(1 << 3))]
    rows[1].update(change)
    return descs_of([(r["offset"], r["shard_stride"], r["shard_len"], r["present_mask"]) for r in rows])


def call_ragged(name, rs, base=P, descs="two", n=None, min_spares=2, **words):
    """A ragged entry point on a fake base; descs: an array, None, or "two"."""
    import helyim_amd as H
    names, spares, tail = RAGGED[name]
    assert set(words) <= set(names), (name, words)
    d = two() if isinstance(descs, str) else descs
    return getattr(H.lib, name)(rs, base, None if d is None else d.ctypes.data,
                                (0 if d is None else len(d)) if n is None else n, *([min_spares] if spares else []),
                                *[words.get(w, P) for w in names], *([None] * tail))


# ---- shard files of zero bytes -----------------------------------------------------
def volume(base, size=700, odd=None, present=range(14), sizes=None):
    """base.ecNN of `size` zero bytes for the present ids; odd = (id, size) or
    sizes = {id: size} give single files another length."""
    sizes = dict(sizes or {})
    if odd:
        sizes[odd[0]] = odd[1]
    for i in present:
        open(str(base) + ".ec%02d" % i, "wb").write(b"\0" * sizes.get(i, size))
