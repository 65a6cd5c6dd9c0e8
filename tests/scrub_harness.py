"""What the scrub GPU suites share -- TEST INFRASTRUCTURE ONLY (not collected;
imports torch and the package inside functions, so it loads without a GPU).

One copy of: the constants and masks, the stale result words with their
sentinel, clean stripes with the C oracle's parity, the three arena shapes
(data and parity over tests/footprint.py layouts, the masked single-arena
Batch, Ragged), one device wrapper per argument-list family with the entry
point as a parameter, and the big-batch and shard-file helpers.

Every device wrapper asserts, where the call has such an argument: the 256-byte
alignment of the device arenas; rc == 0 with last_detail(); every arena byte
for byte against the expected image (the input, for a call that writes
nothing) through footprint.Plan, which names the first wrong byte as slack,
gap, absent or present shard; the sentinel at index S of every word array and
no stale word below it; the masks array read back unchanged; no counter below
its preset. The compare functions (check_words, advance, assert_masks,
assert_arenas) take numpy arrays: tests/test_scrub_harness.py plants a fault
for each."""
import functools

import numpy as np
import pytest

import check_model as C
import footprint as F
import locate_model as LM
import locate_pairs_model as PM
from oracle import corc

SENTINEL = 0x5A5AA5A5   # word S of every result array
STALE = 0xFFFFFFFF      # what every result word holds before a call; no call's result
FILL = 0xEE             # absent shards, gaps and slack of Batch and Ragged
UNEXPLAINED, ALL = C.UNEXPLAINED, C.ALL
ABSENT = "absent shard"


def lost(*ids):
    return ALL & ~sum(1 << i for i in ids)


def bits(*shards):
    return sum(1 << c for c in shards)


def hexes(ws):
    return [hex(w) for w in ws]


R4, R3, R2, R1 = ALL, lost(3), lost(0, 12), lost(2, 7, 11)  # one mask for each number of spare shards
TEN, NINE = lost(1, 4, 9, 13), lost(0, 5, 6, 10, 12)


# ---- the compare functions: numpy in, AssertionError out ---------------------------
def check_words(out, S, what="result words"):
    """out: [S + 1] uint32 as read back -> the S words. The sentinel at S is
    intact and no word still holds the stale value."""
    out = np.asarray(out)
    assert out.dtype == np.uint32 and out.shape == (S + 1,), (what, out.dtype, out.shape)
    assert int(out[S]) == SENTINEL, f"{what}: word S is {int(out[S]):#x}, the sentinel was overwritten"
    stale = np.flatnonzero(out[:S] == STALE)
    assert stale.size == 0, f"{what}: stale words left at {stale[:8].tolist()}"
    return [int(w) for w in out[:S]]


def advance(got, preset, want=None, what="counter"):
    """The advance of an accumulated counter over its preset; never negative,
    and `want` when given."""
    assert got >= preset, f"{what}: {got} is below its preset {preset}"
    assert want is None or got - preset == want, f"{what}: advanced by {got - preset} from {preset}, expected {want}"
    return got - preset


def assert_masks(got, given, what="present masks"):
    """The masks array (and the word after it) read back as given."""
    got = [int(w) for w in np.asarray(got).view(np.uint32)]
    want = [int(m) & 0xFFFFFFFF for m in given]
    assert got == want, f"{what} were written: " + \
        str([(s, hex(g), hex(w)) for s, (g, w) in enumerate(zip(got, want)) if g != w][:8])


def assert_arenas(expected, got, stripes, note=None, masks=None, slack=F.SLACK):
    """Every byte of every arena; masks: the present mask per stripe, so that a
    wrong byte in a shard the call was told is absent is named as such."""
    plan = F.Plan(expected, stripes, slack)
    if masks is not None:
        for s, m in enumerate(masks):
            plan.roles[s] = [F.PRESENT if int(m) >> i & 1 else ABSENT for i in range(len(plan.roles[s]))]
    F.assert_footprint(plan, got, note)


# ---- result words and counters on the device ----------------------------------------
def result_words(n, S):
    import torch
    ts = [torch.full((S + 1,), -1, dtype=torch.int32, device="cuda") for _ in range(n)]  # stale 0xFFFFFFFF
    for t in ts:
        t[S] = SENTINEL
    return ts


def read_words(t, S, what="result words"):
    return check_words(t.cpu().numpy().view(np.uint32), S, what)


def i32(values):
    import torch
    return torch.tensor(np.array(values, dtype=np.uint32).view(np.int32), device="cuda")


def preset_counters(presets, wide_last=False):
    """One-element device counters holding `presets`; wide_last: the last one
    is the 64-bit corrected_bytes."""
    import torch
    ts = [torch.full((1,), p, dtype=torch.int32, device="cuda") for p in presets]
    if wide_last:
        ts[-1] = torch.full((1,), presets[-1], dtype=torch.int64, device="cuda")
    return ts


def read_counters(ts, presets):
    """-> the counters' values as they are, each checked against its preset."""
    values = [int(t.item()) for t in ts]
    for n, (v, p) in enumerate(zip(values, presets)):
        advance(v, p, what=f"counter {n}")
    return values


def masks_tensor(given):
    """The masks on the device with a full word after them that must survive."""
    return i32([int(m) & 0xFFFFFFFF for m in given] + [ALL])


# ---- clean data ------------------------------------------------------------------
def strided_seed(S, L, seed):
    return 1000003 * seed + 31 * L + S


def ragged_seed(S, L, seed):
    return 7919 * seed + L


@functools.lru_cache(maxsize=None)
def clean_stripes(S, L, seed=0, rule=strided_seed):
    """[S, 14, L] with the C oracle's parity (never modified: tests corrupt
    copies). rule(S, L, seed) is the generator's seed: each suite keeps its own."""
    rng = np.random.default_rng(rule(S, L, seed))
    st = rng.integers(0, 256, (S, 14, L), dtype=np.uint8)
    st[:, 10:] = corc.encode_stripes(np.ascontiguousarray(st[:, :10]))
    st.setflags(write=False)
    return st


# ---- arenas 1: data and parity over footprint layouts --------------------------------
def layouts(k, m, L, S):
    """(name, data layout, parity layout): stripe-major with a 48-byte shard
    gap, shard-major, data and parity in separate arenas, an odd base."""
    n = k + m
    a = F.stripe_major(n, L, S, F.r16(L) + 48, 16)
    b = F.shard_major(n, L, S, F.r16(L) + 16, 48)
    d = F.stripe_major(n, L, S, F.r16(L) + 16, 16, base=F.SLACK + 3)
    yield "stripe-major gap 48", a.sub(0, k), a.sub(k, m)
    yield "shard-major", b.sub(0, k), b.sub(k, m)
    yield "separate arenas", F.stripe_major(k, L, S, F.r16(L) + 48, 16), \
        F.shard_major(m, L, S, F.r16(L) + 16, 48, arena=1)
    yield "odd base", d.sub(0, k), d.sub(k, m)


@functools.lru_cache(maxsize=None)
def clean_case(k, m, L, S, which):
    """A layout and its arenas with correct parity everywhere (never modified:
    tests corrupt copies). -> (name, data, par, stripes, arenas)."""
    name, data, par = list(layouts(k, m, L, S))[which]
    stripes = F.stripes_of(data, par)
    rng = np.random.default_rng(1000 * L + 10 * S + which + 7 * k + m)
    raw = [F.random_arena(sz, rng) for sz in F.arena_sizes(stripes)]
    arenas = F.plan_encode(raw, stripes, k, m).expected  # the raw bytes with the oracle's parity in place
    for a in arenas:
        a.setflags(write=False)
    return name, data, par, stripes, arenas


def copies(arenas):
    return [np.array(a, copy=True) for a in arenas]


def shard_of(arenas, stripes, s, i):
    a, o = stripes[s].locs[i]
    return arenas[a][o:o + stripes[s].L]


def gather(arenas, stripes):
    """The stripes' shards as they are in the arenas -> [S, 14, L]."""
    return np.stack([np.stack([shard_of(arenas, stripes, s, i) for i in range(14)]) for s in range(len(stripes))])


def oracle_words(arenas, stripes, k, m):
    rs = corc.CReedSolomon(k, m)
    words = []
    for s, st in enumerate(stripes):
        bufs = [shard_of(arenas, stripes, s, i).copy() for i in range(k)] + \
               [np.zeros(st.L, np.uint8) for _ in range(m)]
        rs.encode(bufs)
        words.append(sum(1 << j for j in range(m) if (bufs[k + j] != shard_of(arenas, stripes, s, k + j)).any()))
    return words


def flip_positions(L):
    return sorted({p for p in (0, L - 1, 4095, 4096, 16 * 255, 8191, 8192) if 0 <= p < L})


def in_place_layout(data, par):
    """The 14-shard layout of a clean_case whose parity follows its data."""
    assert par.base == data.base + 10 * data.shard_stride and par.arena == data.arena
    assert (par.stripe_stride, par.shard_stride) == (data.stripe_stride, data.shard_stride)
    return data._replace(shards=14)


# ---- arenas 2: the masked single-arena batch -----------------------------------------
def layout_of(kind, L, S):
    if kind == "aligned":   # 16-byte aligned base and strides: the fast kernel where L allows
        return F.stripe_major(14, L, S, F.r16(L) + 48, 16)
    if kind == "odd":       # odd base, odd strides: the unaligned generic kernel
        return F.stripe_major(14, L, S, F.r16(L) + 17, 3, base=F.SLACK + 1)
    assert kind == "shard-major"
    return F.shard_major(14, L, S, F.r16(L) + 16, 48)


class Batch:
    """Stripes laid out in one arena; absent shards and every gap hold FILL."""

    def __init__(self, stripes, masks, kind="aligned", fill=FILL):
        S, n, L = stripes.shape
        self.S, self.L, self.masks = S, L, [int(m) for m in masks]
        self.layout = layout_of(kind, L, S)
        self.stripes = F.stripes_of(self.layout)
        size, = F.arena_sizes(self.stripes)
        if fill is None:
            self.arena = np.random.default_rng(5).integers(0, 256, size, dtype=np.uint8)
        else:
            self.arena = np.full(size, fill, dtype=np.uint8)
        for s in range(S):
            for i in range(14):
                if self.masks[s] >> i & 1:
                    self.shard(s, i)[:] = stripes[s, i]
                elif fill is None:
                    self.shard(s, i)[:] = FILL

    def shard(self, s, i):
        o = self.layout.off(s, i)
        return self.arena[o:o + self.L]

    def gather(self, arena=None):
        a = self.arena if arena is None else arena
        return np.stack([np.stack([a[self.layout.off(s, i):self.layout.off(s, i) + self.L] for i in range(14)])
                         for s in range(self.S)])


# ---- arenas 3: ragged ------------------------------------------------------------
class Ragged:
    """Stripes (L, mask) back to back in one arena; absent shards, the slack of
    every shard and every gap hold FILL."""
    SLACK = 64  # before the first and after the last stripe

    def __init__(self, shapes, present=None):
        self.shapes = [(int(L), int(m)) for L, m in shapes]
        self.S = len(self.shapes)
        self.offs, self.strides = [], []
        off = self.SLACK
        for L, _ in self.shapes:
            stride = F.r16(L) + 48
            self.offs.append(off)
            self.strides.append(stride)
            off += 14 * stride + 64
        self.arena = np.full(off, FILL, dtype=np.uint8)
        for s, (L, m) in enumerate(self.shapes):
            held = m if present is None else present[s]  # which shards hold data in memory
            for i in range(14):
                if held >> i & 1:
                    self.shard(s, i)[:] = ragged_stripe(L, s)[i]

    def shard(self, s, i):
        o = self.offs[s] + i * self.strides[s]
        return self.arena[o:o + self.shapes[s][0]]

    def flip(self, s, i, pos, xor=0x41):
        """pos may be shard_len and past it: the slack up to the stride."""
        self.arena[self.offs[s] + i * self.strides[s] + pos] ^= xor

    def gather(self, s, arena=None):
        a = self.arena if arena is None else arena
        L = self.shapes[s][0]
        return np.stack([a[self.offs[s] + i * self.strides[s]:][:L] for i in range(14)])

    def masks(self):
        return [m for _, m in self.shapes]

    def descs(self, masks=None):
        masks = self.masks() if masks is None else masks
        return [(self.offs[s], self.strides[s], self.shapes[s][0], masks[s]) for s in range(self.S)]

    def stripes(self):
        """The stripes as footprint.Stripe, for assert_arenas."""
        return [F.Stripe(L, tuple((0, self.offs[s] + i * self.strides[s]) for i in range(14)))
                for s, (L, _) in enumerate(self.shapes)]

    def entries(self, chunk=4096):
        """Map entries of the table form: none for a stripe that is not read."""
        return sum(-(-L // chunk) for L, m in self.shapes if bin(m & ALL).count("1") > 10)

    def model(self):
        chk, sus = [], []
        for s, (_, m) in enumerate(self.shapes):
            st = self.gather(s)[None]
            chk += C.check_words(st, [m])
            sus += C.suspect_words(st, [m])
        return chk, sus


RAGGED_LENGTHS = (16, 1000, 2048, 4096 + 16, 8192, 24576)
RAGGED_MASKS = (R4, R3, R2, R1, TEN, NINE)


def ragged_stripe(L, seed=0):
    """[14, L] with the C oracle's parity: stripe `seed` of a Ragged batch."""
    return clean_stripes(1, L, seed, ragged_seed)[0]


def ragged_flip_cases(lengths, masks):
    """(L, mask, shard, pos): the first and the last byte, in a shard of B and in one of E."""
    out = []
    for L in lengths:
        for m in masks:
            B, E = C.split(m)
            for n, pos in enumerate((0, L - 1)):
                out.append((L, m, B[(3 + n + L) % 10], pos))
                out.append((L, m, E[(n + L) % len(E)], pos))
    return out


def ragged_kernel_name(b):
    import helyim_amd as H
    return H.ragged_scrub_kernel_name(b.descs())


def rs104():
    import helyim_amd as H
    return H.ReedSolomon(10, 4)


# ---- device wrappers: one per argument-list family -------------------------------------
def _upload(arenas):
    import torch
    devs = [torch.from_numpy(a).cuda() for a in arenas]
    assert all(d.data_ptr() % 256 == 0 for d in devs)  # the layout's own offsets decide the alignment
    return devs


def _finish(rc, name):
    import torch
    import helyim_amd as H
    assert rc == 0, (name, rc, H._lib.last_detail())
    torch.cuda.synchronize()


def device_words(call, rs, arenas, stripes, data, par, n_words, presets, wide_last=False, expected=None, note=None):
    """The data + parity words family: hec_gpu_verify_batch (one word array, one
    counter), the two locate calls (two, one), the two correct calls (two,
    three with corrected_bytes last). expected: the arenas afterwards, the
    input when None. -> ([words [S]] * n_words, [counter values as they are])."""
    import torch
    import helyim_amd as H
    S = data.S
    devs = _upload(arenas)
    words = result_words(n_words, S)
    counters = preset_counters(presets, wide_last)
    torch.cuda.synchronize()
    rc = getattr(H.lib, call)(rs.handle, devs[data.arena].data_ptr() + data.base, data.stripe_stride,
                              data.shard_stride, devs[par.arena].data_ptr() + par.base, par.stripe_stride,
                              par.shard_stride, data.L, S, *[w.data_ptr() for w in words],
                              *[c.data_ptr() for c in counters], torch.cuda.current_stream().cuda_stream)
    _finish(rc, call)
    assert_arenas(arenas if expected is None else expected, [d.cpu().numpy() for d in devs], stripes, note)
    return [read_words(w, S, call) for w in words], read_counters(counters, presets)


def device_repair(call, rs, arenas, stripes, layout, expected, preset_left=7):
    """hec_gpu_repair_batch or hec_gpu_repair_pairs_batch on the in-place layout
    -> (mismatch, suspects, masks, unrepaired, verify words afterwards).
    Asserts that the arenas equal `expected` in every byte."""
    import torch
    import helyim_amd as H
    S = layout.S
    devs = _upload(arenas)
    mis, sus, masks = result_words(3, S)
    left, = preset_counters([preset_left])
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    base = devs[layout.arena].data_ptr() + layout.base
    rc = getattr(H.lib, call)(rs.handle, base, layout.stripe_stride, layout.shard_stride, layout.L, S,
                              mis.data_ptr(), sus.data_ptr(), masks.data_ptr(), left.data_ptr(), stream)
    _finish(rc, call)
    assert_arenas(expected, [d.cpu().numpy() for d in devs], stripes, call)
    after, = result_words(1, S)
    rc = H.lib.hec_gpu_verify_batch(rs.handle, base, layout.stripe_stride, layout.shard_stride,
                                    base + 10 * layout.shard_stride, layout.stripe_stride, layout.shard_stride,
                                    layout.L, S, after.data_ptr(), None, stream)
    _finish(rc, "hec_gpu_verify_batch")
    return (read_words(mis, S, call), read_words(sus, S, call), read_words(masks, S, call),
            read_counters([left], [preset_left])[0], read_words(after, S))


def device_masked(call, rs, b, n_words, presets, wide_last=False, min_spares=None, given=None, expected=None,
                  note=None):
    """The masked in-place family on a Batch: hec_gpu_verify_present_batch (one
    word array), hec_gpu_locate_corrupt_present_batch (two),
    hec_gpu_correct_present_batch (two, min_spares), and the checked and the
    corrected reconstruct (three; min_spares for the corrected one). given:
    the masks the call is handed, b.masks when None. expected: the arena
    afterwards, the input when None. -> ([words [S]] * n_words, [counter
    values as they are])."""
    import torch
    import helyim_amd as H
    S, la = b.S, b.layout
    given = b.masks if given is None else list(given)
    dev, = _upload([b.arena])
    words = result_words(n_words, S)
    masks = masks_tensor(given)
    counters = preset_counters(presets, wide_last)
    torch.cuda.synchronize()
    rc = getattr(H.lib, call)(rs.handle, dev.data_ptr() + la.base, la.stripe_stride, la.shard_stride, la.L, S,
                              masks.data_ptr(), *([] if min_spares is None else [min_spares]),
                              *[w.data_ptr() for w in words], *[c.data_ptr() for c in counters],
                              torch.cuda.current_stream().cuda_stream)
    _finish(rc, call)
    assert_arenas([b.arena if expected is None else expected], [dev.cpu().numpy()], b.stripes, note, b.masks)
    assert_masks(masks.cpu().numpy(), given + [ALL])
    return [read_words(w, S, call) for w in words], read_counters(counters, presets)


def device_ragged(fn, rs, b, word_names, counter_names, presets, wide_last=False, min_spares=None, masks=None,
                  expected=None, note=None):
    """The ragged family through the package's mirrors (fn: verify_ragged,
    locate_corrupt_ragged, correct_ragged, reconstruct_corrected_ragged, which
    raise on a status); word and counter arrays go in by keyword. -> ([words
    [S]] per name, [counter values as they are], the device arena)."""
    import torch
    S = b.S
    dev, = _upload([b.arena])
    words = result_words(len(word_names), S)
    counters = preset_counters(presets, wide_last)
    torch.cuda.synchronize()
    fn(rs, dev, b.descs(masks), *([] if min_spares is None else [min_spares]),
       **dict(zip(word_names, words)), **dict(zip(counter_names, counters)))
    torch.cuda.synchronize()
    assert_arenas([b.arena if expected is None else expected], [dev.cpu().numpy()], b.stripes(), note, b.masks(),
                  slack=Ragged.SLACK)
    return [read_words(w, S, n) for n, w in zip(word_names, words)], read_counters(counters, presets), dev


# ---- big batches: built, corrupted and compared on the device ----------------------------
MASK_ROUND = 2048 * 256  # stripes one round of the mask kernels takes: 2048 workgroups of 256 lanes
LAUNCH_LIMIT = 1 << 23   # workgroups of one launch, and of one pass of a grid-stride loop


def expect_words(S, idx, values, rest=0):
    """[S + 1] words on the device: `rest` (a value or an [S] tensor), `values`
    at the stripes idx, the sentinel at S -- what result_words(n, S) must become."""
    import torch
    t = torch.empty(S + 1, dtype=torch.int32, device="cuda")
    t[:S] = rest
    t[idx] = i32(values)
    t[S] = SENTINEL
    return t


def assert_words(got, want, what):
    import torch
    if not torch.equal(got, want):
        at = torch.nonzero(got != want).flatten()[:8].cpu().tolist()
        pytest.fail(f"{what}: wrong at {at}: got {hexes(got[at].cpu().numpy().view(np.uint32))}, "
                    f"expected {hexes(want[at].cpu().numpy().view(np.uint32))}")


def checksum(t):
    """One device reduction over every byte of a contiguous tensor."""
    import torch
    return int(t.view(torch.int64).sum().item())


# ---- shard files -----------------------------------------------------------------
BLOCK = 4096


def ec_names(base):
    return [base + ".ec%02d" % i for i in range(14)]


def flip(base, shard, offset, value=0x5A):
    with open(base + ".ec%02d" % shard, "r+b") as f:
        f.seek(offset)
        b = f.read(1)
        f.seek(offset)
        f.write(bytes([b[0] ^ value]))


def block_words(files, lo, hi, *word_fns):
    """word_fn(block [1, 14, hi - lo])[0] for each of the models' functions, of
    the column block [lo, hi) of fourteen byte strings."""
    block = np.stack([np.frombuffer(bytes(f[lo:hi]), np.uint8) for f in files])[None]
    return tuple(fn(block)[0] for fn in word_fns)


def oracle_volume(base, seed, large, small, tail):
    """A seeded .dat of 3 large and 57 small rows and `tail` bytes, and its shard
    files written by the C oracle -> the fourteen files' bytes."""
    open(base + ".dat", "wb").write(corc.splitmix64_bytes(seed, 10 * large * 3 + 10 * small * 57 + tail).tobytes())
    assert corc.write_ec_files(base, small, large, small) == 0
    return [open(name, "rb").read() for name in ec_names(base)]


def library_volume(base, seed, nbytes, large=16 * 1001, small=1001):
    """A seeded .dat of nbytes and its shard files written by generate_ec_files
    with small blocks: shards that end in a short block -> the files' bytes."""
    import helyim_amd as H
    open(base + ".dat", "wb").write(corc.splitmix64_bytes(seed, nbytes).tobytes())
    H.generate_ec_files(base, small, large, small)
    return [open(name, "rb").read() for name in ec_names(base)]


def with_stray_bits(masks, seed):
    """Random bits 14..30 and bit 31 ORed into every mask: hec.h defines the
    present mask of a stripe as d_present_masks[s] & 0x3FFF."""
    rng = np.random.default_rng(seed)
    out = [m | int(rng.integers(1, 1 << 17)) << 14 | 1 << 31 for m in masks]
    assert all(o & ALL == m and o >> 14 for o, m in zip(out, masks))
    return out


def masked_block_words(files, mask, lo, hi):
    """(check, suspects) of the column block [lo, hi) under a present mask, by check_model."""
    return block_words(files, lo, hi, lambda b: C.check_words(b, [mask]), lambda b: C.suspect_words(b, [mask]))


def degraded_volume(base):
    """A small volume written by generate_ec_files with small blocks: shards
    that end in a short block -> (the fourteen files' bytes, their size)."""
    large, small = 16 * 1001, 1001
    files = library_volume(base, 99, 10 * large * 2 + 10 * small * 23 + 321)
    size = len(files[0])
    assert all(len(f) == size for f in files) and size > 12 * BLOCK and size % BLOCK > 1
    return files, size


def write_volume(tmp_path, files, absent=()):
    base = str(tmp_path / "v")
    for i, f in enumerate(files):
        if i not in absent:
            open(base + ".ec%02d" % i, "wb").write(f)
    return base


# ---- shard files longer than the scrub's two slots ------------------------------------
BIG_SIZE = (8 << 20) + 300_007
# 64 KiB: three chunks of 64 blocks, slot 0 used twice; 0: the 1 MiB default,
# four blocks per chunk; 5 MiB: larger than a chunk's 4 MiB, so one block per
# chunk, and the last chunk is a short block alone (3 MiB + 300007)
BIG_BLOCKS = (65536, 0, 5 << 20)
EDGE = 4 << 20  # the first chunk edge at 64 KiB and 1 MiB blocks
RUN = (EDGE - 2048, EDGE + 2048)
SINGLES = [(11, 5), (2, EDGE - 1), (13, EDGE), (0, (8 << 20) - 1), (10, 8 << 20), (4, BIG_SIZE - 1)]
NEIGHBOURS = [(6, (6 << 20) + 99), (9, (6 << 20) + 100)]
TRIPLE_AT = (8 << 20) + 200_009  # the last chunk at every block size; alone in its 64 KiB block


def big_volume(seed):
    """-> (good, bad, cols, triple): fourteen streams of BIG_SIZE bytes, ten of
    seeded random bytes and the oracle's parity of them (one encode call:
    parity is bytewise, no block geometry), and a damaged copy. Single flips
    in six different files, data and parity, at the first and the last byte
    and on both sides of 4 MiB and 8 MiB; two different files wrong in
    neighbouring columns; files 2 and 13 wrong in the same columns over a run
    of 4096 that straddles 4 MiB -- except that of the two columns at the edge
    itself each is wrong in one of the two files only (file 2 at 4 MiB - 1,
    file 13 at 4 MiB: the single flips there; a third wrong file in a column
    of the run would leave it unexplained for good); and one column with
    three wrong files the pair model calls unexplained. cols: every damaged
    column, ascending."""
    rng = np.random.default_rng(seed)
    good = [rng.integers(0, 256, BIG_SIZE, dtype=np.uint8) for _ in range(10)] + \
           [np.zeros(BIG_SIZE, np.uint8) for _ in range(4)]
    corc.CReedSolomon(10, 4).encode(good)
    bad = [g.copy() for g in good]
    for shard, o in SINGLES + NEIGHBOURS:
        bad[shard][o] ^= 0x33
    lo, hi = RUN
    for shard in (2, 13):
        x = rng.integers(1, 256, hi - lo, dtype=np.uint8)
        x[EDGE - 1 - lo] = x[EDGE - lo] = 0
        bad[shard][lo:hi] ^= x
    triple = PM.unexplained_triple(rng)
    for c, v in triple.items():
        bad[c][TRIPLE_AT] ^= v
    cols = np.array(sorted({o for _, o in SINGLES + NEIGHBOURS} | set(range(lo, hi)) | {TRIPLE_AT}))
    assert all((bad[i] != good[i]).sum() == sum(1 for o in cols if bad[i][o] != good[i][o]) for i in range(14))
    return good, bad, cols, triple


def big_entries(model, files, cols, width):
    """The entries of a scrub of `files` at blocks of `width` bytes, from the
    model on the damaged columns of each block: a column the oracle encoded
    and nobody touched has a zero syndrome."""
    want = []
    for lo in sorted({int(o) // width * width for o in cols}):
        hi = min(lo + width, BIG_SIZE)
        sel = cols[(cols >= lo) & (cols < hi)]
        block = np.stack([f[sel] for f in files])[None]
        mis, sus = LM.mismatch_words(block)[0], model.suspect_words(block)[0]
        if mis:
            want.append((lo, hi - lo, mis, sus))
    return want
