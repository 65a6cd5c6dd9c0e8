"""Which check fires first when two arguments of a device scrub entry point are
wrong at once, without a GPU (fake non-null pointers are never touched). The
other test_*_abi.py files take one wrong argument at a time; the entry points
share their prologues, so the order of the checks inside a prologue is pinned
here, for every strided, pairs, present-mask and ragged scrub call."""
import pytest

from abi_util import two

INVALID_ARGUMENT, EMPTY_SHARD = 66, 11
P, L = 0x1000, 4096


def _split(name, tail):
    """data / parity calls: (rs, data, 2 strides, parity, 2 strides, len, n, mismatch, [suspects], counters.., stream)."""
    def call(lib, rs, length=L, n=2, sh=L, res=P, sus=P):
        words = (res, sus) if "locate" in name or "correct" in name else (res,)
        return getattr(lib, name)(rs, P, 14 * L, sh, P + 10 * L, 14 * L, sh, length, n, *words, *([None] * tail))
    call.__name__ = name
    return call


def _repair(name):
    def call(lib, rs, length=L, n=2, sh=L, res=P, sus=P, use=P):
        return getattr(lib, name)(rs, P, 14 * L, sh, length, n, res, sus, use, None, None)
    call.__name__ = name
    return call


def _present(name, words, tail, spares):
    """masked calls: (rs, shards, 2 strides, len, n, masks, [min_spares], check, [suspects, [use]], counters.., stream)."""
    def call(lib, rs, length=L, n=2, sh=L, res=P, sus=P, use=P, min_spares=2):
        lead = (P, min_spares) if spares else (P,)
        return getattr(lib, name)(rs, P, 14 * L, sh, length, n, *lead, *(res, sus, use)[:words], *([None] * tail))
    call.__name__ = name
    return call


def _ragged(name, words, tail, spares):
    """ragged calls: (rs, base, descs, n, [min_spares], check, [suspects, [use]], counters.., stream)."""
    def call(lib, rs, length=1000, n=2, descs="two", base=P, res=P, sus=P, use=P, min_spares=2):
        d = two(shard_len=length) if isinstance(descs, str) else descs
        lead = (min_spares,) if spares else ()
        return getattr(lib, name)(rs, base, None if d is None else d.ctypes.data, n, *lead, *(res, sus, use)[:words],
                                  *([None] * tail))
    call.__name__ = name
    return call


VERIFY = _split("hec_gpu_verify_batch", 2)
SPLIT = [_split("hec_gpu_locate_corrupt_batch", 2), _split("hec_gpu_locate_corrupt_pairs_batch", 2),
         _split("hec_gpu_correct_batch", 4), _split("hec_gpu_correct_pairs_batch", 4)]
REPAIR = [_repair("hec_gpu_repair_batch"), _repair("hec_gpu_repair_pairs_batch")]
PRESENT = [_present("hec_gpu_verify_present_batch", 1, 3, False),
           _present("hec_gpu_locate_corrupt_present_batch", 2, 3, False),
           _present("hec_gpu_reconstruct_checked_batch", 3, 3, False),
           _present("hec_gpu_correct_present_batch", 2, 5, True),
           _present("hec_gpu_reconstruct_corrected_batch", 3, 4, True)]
RAGGED = [_ragged("hec_gpu_verify_ragged", 1, 3, False), _ragged("hec_gpu_locate_corrupt_ragged", 2, 3, False),
          _ragged("hec_gpu_correct_ragged", 2, 5, True), _ragged("hec_gpu_reconstruct_corrected_ragged", 3, 4, True)]
HAS_SUSPECTS = SPLIT + REPAIR + PRESENT[1:] + RAGGED[1:]
HAS_USE = [REPAIR[0], REPAIR[1], PRESENT[2], PRESENT[4], RAGGED[3]]
HAS_SPARES = [PRESENT[3], PRESENT[4], RAGGED[2], RAGGED[3]]
ALL = [VERIFY] + SPLIT + REPAIR + PRESENT + RAGGED


def outcome(H, status):
    """(status, which check spoke)."""
    detail = H._lib.last_detail()
    for word in ("null", "RS(10,4) only", "min_spares", "32 parity", "aligned", "stride"):
        if word in detail:
            return status, word
    return status, detail


def ids(calls):
    return dict(argvalues=calls, ids=[c.__name__ for c in calls])


@pytest.mark.parametrize("call", **ids(ALL))
def test_a_null_result_pointer_speaks_before_the_codec(call):
    import helyim_amd as H
    other = H.ReedSolomon(5, 5)
    assert outcome(H, call(H.lib, other.handle, res=None)) == (INVALID_ARGUMENT, "null")
    if call in HAS_SUSPECTS:
        assert outcome(H, call(H.lib, other.handle, sus=None)) == (INVALID_ARGUMENT, "null")
    if call in HAS_USE:
        assert outcome(H, call(H.lib, other.handle, use=None)) == (INVALID_ARGUMENT, "null")
    # and the codec before the layout
    if call not in RAGGED and call is not VERIFY:
        assert outcome(H, call(H.lib, other.handle, sh=L - 16)) == (INVALID_ARGUMENT, "RS(10,4) only")


def test_verify_null_words_speak_before_its_33_parity_shards():
    import helyim_amd as H
    wide = H.ReedSolomon(10, 33)
    assert outcome(H, VERIFY(H.lib, wide.handle, res=None)) == (INVALID_ARGUMENT, "null")
    assert outcome(H, VERIFY(H.lib, wide.handle, sh=L - 16)) == (INVALID_ARGUMENT, "32 parity")
    assert outcome(H, VERIFY(H.lib, wide.handle, n=0)) == (INVALID_ARGUMENT, "32 parity")


@pytest.mark.parametrize("call", **ids(ALL))
def test_null_words_against_a_zero_shard_length(call):
    """The data / parity calls test the length with their first three pointers,
    before the result pointers; every other call tests all its pointers first."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    length_first = call is VERIFY or call in SPLIT
    want = (EMPTY_SHARD, "") if length_first else (INVALID_ARGUMENT, "null")
    assert outcome(H, call(H.lib, rs.handle, res=None, length=0)) == want
    if call in HAS_SUSPECTS:
        assert outcome(H, call(H.lib, rs.handle, sus=None, length=0)) == want
    if call in HAS_USE:
        assert outcome(H, call(H.lib, rs.handle, use=None, length=0)) == want
    # the length before the codec, except in the ragged calls (a descriptor's field: after the codec)
    other = H.ReedSolomon(10, 2)
    if call in RAGGED:
        assert outcome(H, call(H.lib, other.handle, length=0)) == (INVALID_ARGUMENT, "RS(10,4) only")
    else:
        assert outcome(H, call(H.lib, other.handle, length=0))[0] == EMPTY_SHARD


@pytest.mark.parametrize("call", **ids(HAS_SPARES))
def test_min_spares_speaks_after_the_other_arguments_and_before_an_empty_batch(call):
    import helyim_amd as H
    rs, other = H.ReedSolomon(10, 4), H.ReedSolomon(10, 6)
    assert outcome(H, call(H.lib, rs.handle, min_spares=5, n=0)) == (INVALID_ARGUMENT, "min_spares")
    assert outcome(H, call(H.lib, rs.handle, min_spares=1, res=None)) == (INVALID_ARGUMENT, "null")
    assert outcome(H, call(H.lib, rs.handle, min_spares=1, sus=None)) == (INVALID_ARGUMENT, "null")
    assert outcome(H, call(H.lib, other.handle, min_spares=1)) == (INVALID_ARGUMENT, "RS(10,4) only")
    assert outcome(H, call(H.lib, rs.handle, min_spares=1, length=0))[0] == EMPTY_SHARD
    if call in RAGGED:
        assert outcome(H, call(H.lib, rs.handle, min_spares=1, base=P + 8)) == (INVALID_ARGUMENT, "aligned")
        assert outcome(H, call(H.lib, rs.handle, min_spares=1, descs=None)) == (INVALID_ARGUMENT, "null")
    else:
        assert outcome(H, call(H.lib, rs.handle, min_spares=1, sh=L - 16)) == (INVALID_ARGUMENT, "stride")


@pytest.mark.parametrize("call", **ids([c for c in ALL if c not in RAGGED]))
def test_the_layout_is_checked_for_an_empty_batch_too(call):
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    assert outcome(H, call(H.lib, rs.handle, n=0, sh=L - 16)) == (INVALID_ARGUMENT, "stride")
    assert call(H.lib, rs.handle, n=0) == 0


@pytest.mark.parametrize("call", **ids(RAGGED))
def test_ragged_null_pointers_speak_before_the_descriptors_are_read(call):
    """A null descriptor list with a count must fail as a null argument whatever
    else is wrong, and must never be walked: not by the kernel pick, not by the
    checks. With null result words too, the answer is the same."""
    import helyim_amd as H
    rs, other = H.ReedSolomon(10, 4), H.ReedSolomon(5, 5)
    assert outcome(H, call(H.lib, rs.handle, descs=None)) == (INVALID_ARGUMENT, "null")
    assert outcome(H, call(H.lib, rs.handle, descs=None, res=None)) == (INVALID_ARGUMENT, "null")
    assert outcome(H, call(H.lib, other.handle, descs=None)) == (INVALID_ARGUMENT, "null")
    assert outcome(H, call(H.lib, rs.handle, descs=None, base=P + 8)) == (INVALID_ARGUMENT, "null")
    assert outcome(H, call(H.lib, rs.handle, res=None, base=P + 8)) == (INVALID_ARGUMENT, "null")
    # the codec before a descriptor's alignment
    assert outcome(H, call(H.lib, other.handle, base=P + 8)) == (INVALID_ARGUMENT, "RS(10,4) only")
    assert call(H.lib, rs.handle, descs=None, n=0) == 0
