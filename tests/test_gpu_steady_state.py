"""The hash and ChaCha20 kernels past their first pass.

Five launches size their grid as min(need, full) and loop when the work exceeds it: a quad of
blake2b_kernel (content hash, fused Ref.Id, chunk.Get) pulls its next record from the queue,
and the waves of the two ChaCha20 passes (the split Ref.Id form's, the read path's gather)
stride over their keystream blocks.  On a 256-CU device `full` is 16,384 quads or 128 MiB, so
ordinary test inputs end inside the first pass.  Here the loops run:

  * under the PFSCDC_HASH_GRID / PFSCDC_CHACHA_GRID knobs (1-3 workgroups: 64 quads, or 256
    keystream blocks a pass, each), on a few hundred chunks;
  * at the shipped sizing, on inputs sized from the device's CU count to 1.25-1.5 x `full`,
    drawn with repetition from a few distinct contents so that the oracle stays cheap.

Every test computes from its sizes how often the loop under test repeats and asserts it.
Everything is bit-exact and total against oracle/chunker.py (create_ref_id, chacha20_xor,
read_data_ref), coracle.segment_files and hashlib: every record, every output byte."""
import hashlib
import math

import numpy as np
import pytest

from oracle import chunker as Ch
from oracle import coracle
from pfs_amd import _lib
from pfs_amd.cdc import ChunkParams, Chunker, synthetic_bytes
from stored_chunks import Stored, created

pytestmark = pytest.mark.gpu

SMALL = Ch.Params(average_bits=12, seed=1, min=2000, max=30000)
QUADS = 64       # records in flight per hash workgroup (kHashBlock / 4)
KS_BLOCKS = 256  # 64-byte keystream blocks per ChaCha20 workgroup and pass (kChachaBlock)
LONG = [(1 << 20) + 5, (1 << 20) + 128]  # > 8192 blocks: the auto issue priority engages


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu(gpu_available):
    return gpu_available


def refills_per_quad(entries: int, grid: int) -> float:
    """Queue entries a quad takes after its first, on average, at `grid` workgroups."""
    return entries / (grid * QUADS) - 1


def passes(blocks: int, grid: int) -> int:
    """Grid-stride passes of a ChaCha20 launch over `blocks` keystream blocks."""
    return math.ceil(blocks / (grid * KS_BLOCKS))


def ks_blocks(offset: int, size: int) -> int:
    return (offset + size - 1) // 64 - offset // 64 + 1 if size else 0


def compute_units() -> int:
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def assert_rows_equal(got, want, what, sizes=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: {got.shape} records, want {want.shape}"
    bad = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
    assert len(bad) == 0, f"{what} differs at {len(bad)} records, first {bad[:8]}" + \
        (f" (sizes {[int(sizes[i]) for i in bad[:8]]})" if sizes is not None else "")


def check_created(refs, hashes, st):
    assert_rows_equal(hashes, st.hashes, "content hash", st.sizes)
    assert_rows_equal(refs["dek"], st.refs["dek"], "dek", st.sizes)
    assert_rows_equal(refs["id"], st.refs["id"], "id", st.sizes)


# ------------------------------------------------------------------ capped grids: chunk.Create

@pytest.fixture(scope="module")
def mix():
    """About 600 chunks: every block-edge size, exact multiples of 128, random sizes up to
    20,000 and two chunks past 1 MiB; "alt": short and long alternating, "asc": the same
    chunks sorted by size (so refills land at either buffer parity)."""
    rng = np.random.default_rng(601)
    short = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257] * 8
    short += [int(x) for x in rng.integers(1, 300, 300 - len(short))]
    long_ = LONG + [128 * k for k in (3, 4, 5, 8, 16, 31, 32, 64, 100)] * 4
    long_ += [int(x) for x in rng.integers(300, 20_001, 300 - len(long_))]
    sizes = [z for pair in zip(short, long_) for z in pair]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    data = synthetic_bytes(offs, 61)
    chunks = [data[int(a):int(b)].tobytes() for a, b in zip(offs[:-1], offs[1:])]
    asc = [chunks[i] for i in np.argsort(sizes, kind="stable")]
    return {"alt": Stored(None, 0, chunks=chunks), "asc": Stored(None, 0, chunks=asc)}


@pytest.mark.parametrize("order", ["alt", "asc"])
@pytest.mark.parametrize("waves", [1, 2])
@pytest.mark.parametrize("grid", [1, 3])
def test_fused_ref_id_with_refills(mix, knob, grid, waves, order):
    """blake2b_kernel<kModeRefId> (ChaCha20 on the BLAKE2b chain) with every quad refilled:
    600 chunks on 64 or 192 quads, the two long chunks at raised priority while the quads
    around them end chains and begin new ones."""
    st = mix[order]
    n = len(st.sizes)
    assert refills_per_quad(n, grid) >= 2  # 8.4 at one workgroup, 2.1 at three
    assert sum(z > 8192 * 128 for z in st.sizes) == 2 and n > grid * QUADS  # priority is on
    knob("PFSCDC_REFID_SPLIT", 0)
    knob("PFSCDC_HASH_GRID", grid)
    knob("PFSCDC_HASH_WAVES", waves)
    c = Chunker(ChunkParams(), 0)
    refs, hashes = c.create_refs(st.plain, st.offs)
    assert c.last_create_split() is False
    check_created(refs, hashes, st)
    # every other content hash supplied by the caller: same refs, supplied hashes kept
    known = (np.arange(n) % 2).astype(np.uint8)
    given = np.where(known[:, None] == 1, st.hashes, 0).astype(np.uint8)
    refs2, hashes2 = c.create_refs(st.plain, st.offs, given, known)
    assert c.last_create_split() is False
    check_created(refs2, hashes2, st)
    c.close()


@pytest.mark.parametrize("order", ["alt", "asc"])
@pytest.mark.parametrize("grid", [1, 2])
def test_split_ref_id_under_both_caps(mix, knob, grid, order):
    """chacha_xor_coalesced_kernel over many grid-stride passes (a wave's later windows start
    inside chunks, after chunks of no block at all, and reuse its LDS keystream window), then
    the BLAKE2b of the ciphertext on 64 quads.  With every hash known the pass runs as its two
    streams (the two long chunks, then the rest)."""
    st = mix[order]
    n = len(st.sizes)
    blocks = sum(ks_blocks(0, z) for z in st.sizes)
    assert passes(blocks, grid) >= 20  # 304 at one workgroup, 152 at two
    assert passes(sum(ks_blocks(0, z) for z in LONG), grid) >= 20  # the long stream alone
    assert refills_per_quad(n, 1) >= 2
    knob("PFSCDC_REFID_SPLIT", 1)
    knob("PFSCDC_CHACHA_GRID", grid)
    knob("PFSCDC_HASH_GRID", 1)
    c = Chunker(ChunkParams(), 0)
    refs, hashes = c.create_refs(st.plain, st.offs)
    assert c.last_create_split() is True
    check_created(refs, hashes, st)
    refs2, hashes2 = c.create_refs(st.plain, st.offs, st.hashes, np.ones(n, dtype=np.uint8))
    assert c.last_create_split() is True
    check_created(refs2, hashes2, st)
    c.close()


@pytest.mark.parametrize("two_sets", [0, 1])
@pytest.mark.parametrize("grid", [1, 2])
def test_split_ref_id_in_place_under_both_caps(mix, knob, grid, two_sets):
    """The same chunks through pfscdc_commit_refs with PFSCDC_OPT_CTEXT_IN_PLACE (always the
    split form): afterwards the device buffer is the oracle's ciphertext, chunk by chunk, so
    no partial last block spilled into the chunk behind it.  Every file is one stream and
    shorter than min, so the chunks formed are the files; two_sets = 1 puts the short chunks'
    ChaCha20 pass on the helper context (the one-wave-per-SIMD sizing under the cap)."""
    import torch

    st = mix["alt"]
    rest = sum(ks_blocks(0, z) for z in st.sizes if z not in LONG)
    assert min(passes(rest, grid), passes(sum(ks_blocks(0, z) for z in LONG), grid)) >= 20
    knob("PFSCDC_CHACHA_GRID", grid)
    knob("PFSCDC_HASH_GRID", 1)
    knob("PFSCDC_COMMIT_TWO_SETS", two_sets)
    c = Chunker(ChunkParams(23, 1, 2 << 20, 4 << 20), 0)
    c.set_cuts_only(True)
    c.set_ctext_in_place(True)
    t = torch.from_numpy(st.plain).to("cuda:0")
    c.scan(t, st.offs)
    coffs, _, known = c.form_chunks(list(range(len(st.sizes) + 1)))
    formed = [int(z) for z in np.diff(coffs.astype(np.int64))]
    assert [z for z in formed if z] == [z for z in st.sizes if z]
    refs, chash, _ = c.commit_refs(t, coffs, known)
    assert c.last_create_split() is True
    ct = t.cpu().numpy()
    for i in range(len(formed)):
        a, b = int(coffs[i]), int(coffs[i + 1])
        rid, dek, want, h = created(st.plain[a:b].tobytes())
        assert (bytes(refs[i]["id"]), bytes(refs[i]["dek"]), bytes(chash[i])) == (rid, dek, h), i
        assert ct[a:b].tobytes() == want, f"ciphertext of chunk {i} ({b - a} B)"
    assert np.array_equal(ct, st.ctext)
    c.close()


# ------------------------------------------------------------------- capped grids: the scan

@pytest.fixture(scope="module")
def scanned():
    """220 files of 0-70,000 B under the small chunker (about 1,300 segments) with the
    oracle's records and every segment's Ref."""
    rng = np.random.default_rng(603)
    lens = np.concatenate([rng.integers(0, 70_001, 214), [0, 0, 1, 30_000, 70_000, 0]])
    rng.shuffle(lens)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    data = synthetic_bytes(offs, 63)
    segs, begin = coracle.segment_files(data, offs, SMALL, nthreads=8)
    refs = np.zeros(len(segs), dtype=_lib.ref_dtype())
    for i, s in enumerate(segs):
        a = int(offs[s["file"]]) + int(s["offset"])
        rid, dek = Ch.create_ref_id(data[a:a + int(s["size"])].tobytes())
        refs[i]["id"] = np.frombuffer(rid, dtype=np.uint8)
        refs[i]["dek"] = np.frombuffer(dek, dtype=np.uint8)
    return lens, offs, data, segs, begin, refs


@pytest.mark.parametrize("waves", ["1", "2", "2s"])
@pytest.mark.parametrize("bin_bytes", [0, 60000, 10**12])
def test_scan_with_ref_ids_bins_and_refills(scanned, knob, bin_bytes, waves):
    """The scan's hash and fused Ref.Id launches on 64 quads with hash bins: a quad walks its
    bin (next / bin_next) and then pulls its next entry from the queue.  Bins for no file,
    for the files of at most 60,000 B, for every file; waves as in test_hash_bins_equal_oracle
    ("2s": the fair share updated every 16 blocks)."""
    lens, offs, data, segs, begin, want_refs = scanned
    counts = np.diff(begin.astype(np.int64))
    entries = sum(1 if bin_bytes and lens[f] <= bin_bytes else int(counts[f])
                  for f in range(len(lens)) if counts[f])
    assert refills_per_quad(entries, 1) >= 2  # 21 without bins, 7.3 and 2.4 with them
    if bin_bytes:
        assert any(counts[f] > 1 and lens[f] <= bin_bytes for f in range(len(lens)))
    knob("PFSCDC_HASH_GRID", 1)
    knob("PFSCDC_HASH_BIN_BYTES", bin_bytes)
    knob("PFSCDC_HASH_WAVES", waves[0])
    if waves == "2s":
        knob("PFSCDC_HASH_FAIR_EVERY", 16)
    c = Chunker(ChunkParams(SMALL.average_bits, SMALL.seed, SMALL.min, SMALL.max), 0,
                ref_ids=True)
    res = c.scan(data, offs)
    c.close()
    assert np.array_equal(res.file_begin, begin)
    for f in ("offset", "size", "file", "flags"):
        assert np.array_equal(res.segments[f], segs[f]), f
    assert_rows_equal(res.segments["hash"], segs["hash"], "DataRef hash", segs["size"])
    assert_rows_equal(res.refs["dek"], want_refs["dek"], "dek", segs["size"])
    assert_rows_equal(res.refs["id"], want_refs["id"], "id", segs["size"])


# ------------------------------------------------------------------ capped grids: chunk.Get

def _damage(st, rng):
    """A tenth of the chunks damaged: a flipped bit in the first byte, the last byte or inside
    a partial final block, or a Ref.Id that names other bytes."""
    stored, refs, bad = st.ctext.copy(), st.refs.copy(), set()
    n = len(st.sizes)
    kinds = {st.sizes.index(LONG[0]): 2}  # the 1 MiB + 5 chunk: in its 5-byte final block
    for k, i in enumerate(sorted(int(x) for x in rng.choice(n, n // 10, replace=False))):
        kinds.setdefault(i, k % 4)
    for i, kind in kinds.items():
        z = st.sizes[i]
        if z == 0:
            continue
        if kind == 2 and z % 128 == 0:
            kind = 1
        j = (i + 1) % n
        if kind == 3 and bytes(st.refs[j]["id"]) == bytes(st.refs[i]["id"]):
            kind = 0
        if kind == 3:
            refs[i]["id"] = st.refs[j]["id"]
        else:
            pos = (0, z - 1, z // 128 * 128 + int(rng.integers(0, max(z % 128, 1))))[kind]
            stored[int(st.offs[i]) + pos] ^= 1 << int(rng.integers(0, 8))
        bad.add(i)
    return stored, refs, bad


@pytest.mark.parametrize("grid", [1, 3])
def test_get_chunks_with_refills(mix, knob, grid):
    """blake2b_kernel<kModeGet> (verify, decrypt, store the plaintext) with every quad
    refilled: exactly the damaged chunks fail, every other chunk's plaintext is exact, and
    with a device destination inside a larger tensor not a byte outside it changes."""
    import torch

    st = mix["alt"]
    n, total = len(st.sizes), len(st.plain)
    assert refills_per_quad(n, grid) >= 2
    stored, refs, bad = _damage(st, np.random.default_rng(604))
    assert len(bad) >= n // 12 and st.sizes.index(LONG[0]) in bad
    good = np.ones(total, dtype=bool)
    for i in bad:
        good[int(st.offs[i]):int(st.offs[i + 1])] = False
    knob("PFSCDC_HASH_GRID", grid)
    c = Chunker(ChunkParams(), 0)
    pt, ok = c.get_chunks(stored, st.offs, refs)
    assert set(np.flatnonzero(~ok).tolist()) == bad
    assert np.array_equal(pt[good], st.plain[good])
    t = torch.full((32 + total + 48,), 0xA5, dtype=torch.uint8, device="cuda:0")
    dev = torch.from_numpy(stored).to("cuda:0")
    _, ok = c.get_chunks(dev, st.offs, refs, out=t[32:32 + total])
    c.close()
    host = t.cpu().numpy()
    assert set(np.flatnonzero(~ok).tolist()) == bad
    assert np.array_equal(host[32:32 + total][good], st.plain[good])
    assert (host[:32] == 0xA5).all() and (host[32 + total:] == 0xA5).all()


# ------------------------------------------------------------ capped grids: chunk.Reader.Get

TAMPERED = 3


@pytest.fixture(scope="module")
def sliced():
    """Stored chunks and a slice list of more than 15,360 keystream blocks (20 passes of
    three workgroups, 60 of one) holding what a later pass of the gather meets."""
    rng = np.random.default_rng(605)
    sizes = [45_001, 4133, 700, 30_000, 9001, 300_000] + \
        [int(x) for x in rng.integers(1, 201, 200)]
    st = Stored(sizes, 65)
    slices = []

    def first_block():
        return sum(ks_blocks(o, z) for _, o, z in slices)

    def fill_to(res):  # one slice that brings the next slice's first block to res (mod 512)
        k = (res - first_block()) % 512
        if k:
            slices.append((5, 64 * int(rng.integers(0, 2000)) + 5, 64 * (k - 1) + 10))
            assert ks_blocks(*slices[-1][1:]) == k

    # passes of nothing but single-block slices (a lane walks up to 63 records from its
    # wave's first), zero-size slices between them
    for i in range(600):
        slices.append((1, (7 * i) % 4133, 1))
        if i % 5 == 0:
            slices.append((i % 6, min(i, 700), 0))
    # one slice across more than two passes: several waves' first block falls inside it
    slices.append((0, 37, 40_000))
    # multi-block slices that begin on the last block of a wave's window and of a pass, and
    # on the first of the next
    starts = {}
    for res in (63, 64, 255, 256, 0):
        fill_to(res)
        starts[res] = len(slices)
        slices.append((4, 64 * int(rng.integers(0, 100)) + 51, 150))
    # the tampered chunk, in slices longer than a pass, across the pass ends of every grid
    fill_to(200)
    tampered_from = first_block()
    for k in range(4):
        slices.append((TAMPERED, 11 + k, 25_000))
    tampered_to = first_block()
    # every chunk named, the short ones whole (200 more records for the verify pass)
    for ch in range(6, len(sizes)):
        slices.append((ch, 0, sizes[ch]))
    while first_block() < 15_400:
        ch = int(rng.integers(0, 6))
        o = int(rng.integers(0, sizes[ch] + 1))
        slices.append((ch, o, int(rng.integers(0, min(sizes[ch] - o, 3000) + 1))))
    return st, slices, starts, (tampered_from, tampered_to)


@pytest.mark.parametrize("grid", [1, 2, 3, None])
def test_read_slices_over_many_passes(sliced, knob, grid):
    """chacha_slice_gather_kernel over 20 and more grid-stride passes (None: the shipped
    grid, one pass, as a control), and the verify pass with its quads refilled."""
    import torch

    st, slices, starts, (t0, t1) = sliced
    prefix = np.concatenate([[0], np.cumsum([ks_blocks(o, z) for _, o, z in slices])])
    total_blocks = int(prefix[-1])
    assert total_blocks >= 5120
    if grid:
        assert passes(total_blocks, grid) >= 20
    assert refills_per_quad(len(st.sizes), 1) >= 2  # the verify pass: 206 chunks, 64 quads
    ones = [i for i, (_, _, z) in enumerate(slices[:720]) if z == 1]
    assert len(ones) >= 300 and sum(z == 0 for _, _, z in slices) >= 100
    assert any(z == 40_000 and o == 37 and st.sizes[c] == 45_001 for c, o, z in slices)
    # first blocks of multi-block slices at every residue where a wave or a pass changes
    multi = {int(prefix[i]) % 512 for i, (_, o, z) in enumerate(slices) if ks_blocks(o, z) > 1}
    assert {0, 63, 64, 255, 256} <= multi
    assert all(int(prefix[i]) % 512 == res for res, i in starts.items())
    assert {int(p) % 256 for p in prefix[:-1]} >= {0, 63, 64, 255}
    # the tampered chunk's slices straddle a pass end at each capped grid
    for g in (1, 2, 3):
        assert t0 // (KS_BLOCKS * g) < (t1 - 1) // (KS_BLOCKS * g)
    bad = st.ctext.copy()
    bad[int(st.offs[TAMPERED]) + 12_345] ^= 0x20
    want = b"".join(bytes(z) if c == TAMPERED else st.chunks[c][o:o + z] for c, o, z in slices)
    sub = slices[::37]
    assert st.oracle(sub) == st.sliced(sub)
    knob("PFSCDC_CHACHA_GRID", grid)
    knob("PFSCDC_HASH_GRID", 1)
    c = Chunker(ChunkParams(), 0)
    got, cok, sok = c.read_slices(bad, st.offs, st.refs, slices)
    assert [bool(x) for x in cok] == [i != TAMPERED for i in range(len(st.sizes))]
    assert [bool(x) for x in sok] == [ch != TAMPERED for ch, _, _ in slices]
    assert got.tobytes() == want
    t = torch.full((5 + len(want) + 27,), 0xA5, dtype=torch.uint8, device="cuda:0")
    dev = torch.from_numpy(bad).to("cuda:0")
    _, cok, _ = c.read_slices(dev, st.offs, st.refs, slices, out=t[5:5 + len(want)])
    c.close()
    host = t.cpu().numpy()
    assert [bool(x) for x in cok] == [i != TAMPERED for i in range(len(st.sizes))]
    assert host[5:5 + len(want)].tobytes() == want
    assert (host[:5] == 0xA5).all() and (host[5 + len(want):] == 0xA5).all()


# ---------------------------------------------------------------- capped grids: hash_ranges

def test_hash_ranges_with_refills(knob):
    """The size list of test_hash_chain_ends_around_the_quiet_thresholds (chains ending 0-40
    blocks apart, then one long lone chain) on 64 quads: the quiet-run loop and its
    thresholds with refilled quads beside the running ones."""
    rng = np.random.default_rng(77)
    sizes = []
    for base in (1, 4, 5, 6, 9, 64, 300):
        for k in range(48):
            sizes.append(128 * (base + k % 41) + int(rng.integers(0, 128)))
    sizes += [128 * 2000 + 5]
    assert refills_per_quad(len(sizes), 1) >= 2  # 337 ranges: 4.3
    sizes = np.array(sizes, dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    data = synthetic_bytes(offs, 0x51)
    knob("PFSCDC_HASH_GRID", 1)
    ch = Chunker(ChunkParams(), 0)
    got = ch.hash_ranges(data, offs[:-1], sizes)
    ch.close()
    want = np.array([np.frombuffer(hashlib.blake2b(data[int(a):int(b)].tobytes(),
                                                   digest_size=32).digest(), dtype=np.uint8)
                     for a, b in zip(offs[:-1], offs[1:])])
    assert_rows_equal(got, want, "digest", sizes)


# ------------------------------------------------------------------------ the shipped grids

def test_fused_ref_id_in_its_auto_regime(knob):
    """The fused Ref.Id pass where the library itself selects it: more chunks than
    refid_split()'s bound, the quads of two waves per SIMD (CUs x 128).  1.5 x that bound
    (49,152 chunks on 256 CUs; 1.5 x the 16,384 quads of one wave per SIMD would be below
    the bound and take the split form) drawn from 64 distinct contents of 0-3,000 B, at one
    wave per SIMD: three queue entries per quad.  The same chunks, stored, then go through
    chunk.Get and through the verify pass of the read path, one small slice per chunk."""
    cus = compute_units()
    bound = cus * 4 * 2 * 16
    n = 3 * bound // 2
    quads = cus * 4 * 1 * 16  # PFSCDC_HASH_WAVES=1
    assert n > bound and refills_per_quad(n, quads // QUADS) >= 2
    rng = np.random.default_rng(607)
    sizes = np.array([0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 3000] +
                     [int(x) for x in rng.integers(0, 3001, 52)], dtype=np.int64)
    coffs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    pool = synthetic_bytes(coffs, 67)
    contents = [pool[int(a):int(b)] for a, b in zip(coffs[:-1], coffs[1:])]
    made = [created(x.tobytes()) for x in contents]
    table = [np.array([np.frombuffer(m[k], dtype=np.uint8) for m in made]) for k in (0, 1, 3)]
    pick = rng.integers(0, len(sizes), n)
    offs = np.concatenate([[0], np.cumsum(sizes[pick])]).astype(np.uint64)
    data = np.concatenate([contents[i] for i in pick])
    knob("PFSCDC_HASH_WAVES", 1)
    c = Chunker(ChunkParams(), 0)
    refs, hashes = c.create_refs(data, offs)
    assert c.last_create_split() is False
    assert_rows_equal(hashes, table[2][pick], "content hash", sizes[pick])
    assert_rows_equal(refs["dek"], table[1][pick], "dek", sizes[pick])
    assert_rows_equal(refs["id"], table[0][pick], "id", sizes[pick])
    ctexts = [np.frombuffer(m[2], dtype=np.uint8) if m[2] else np.zeros(0, dtype=np.uint8)
              for m in made]
    stored = np.concatenate([ctexts[i] for i in pick])
    want_refs = np.zeros(n, dtype=_lib.ref_dtype())
    want_refs["id"], want_refs["dek"] = table[0][pick], table[1][pick]
    pt, ok = c.get_chunks(stored, offs, want_refs)
    assert ok.all()
    assert np.array_equal(pt, data)
    sl = np.zeros(n, dtype=_lib.slice_dtype())
    sl["chunk"] = np.arange(n)
    sl["size"] = np.minimum(sizes[pick], 1 + np.arange(n) % 7)
    sl["offset"] = (sizes[pick] - sl["size"].astype(np.int64)) // 2
    got, cok, sok = c.read_slices(stored, offs, want_refs, sl)
    c.close()
    assert cok.all() and sok.all()
    at = offs[:-1].astype(np.int64) + sl["offset"].astype(np.int64)
    idx = np.repeat(at, sl["size"].astype(np.int64)) + \
        (np.arange(int(sl["size"].sum())) -
         np.repeat(np.cumsum(sl["size"].astype(np.int64)) - sl["size"].astype(np.int64),
                   sl["size"].astype(np.int64)))
    assert np.array_equal(got, data[idx])


def _past_the_chacha_cap(cus: int) -> int:
    """1.25 x the bytes one pass of a full ChaCha20 grid covers (CUs x 32 workgroups)."""
    return 5 * cus * 32 * KS_BLOCKS * 64 // 4


def test_gather_past_its_default_cap():
    """chacha_slice_gather_kernel at the shipped grid over 1.25 x what one pass covers (160
    MiB on 256 CUs): whole-chunk slices of three stored chunks of odd sizes, repeated, so the
    destination alignment differs from repeat to repeat.  Output compared on the device."""
    import torch

    cus = compute_units()
    st = Stored([(1 << 20) + 77, (3 << 19) + 1, (2 << 20) - 333], 68)
    slices, total = [], 0
    while total < _past_the_chacha_cap(cus):
        ch = len(slices) % 3
        slices.append((ch, 0, st.sizes[ch]))
        total += st.sizes[ch]
    blocks = sum(ks_blocks(o, z) for _, o, z in slices)
    assert passes(blocks, cus * 32) >= 2
    assert len({sum(z for _, _, z in slices[:i]) % 16 for i in range(len(slices))}) >= 8
    dev = torch.from_numpy(st.ctext).to("cuda:0")
    plain = [torch.from_numpy(np.frombuffer(x, dtype=np.uint8).copy()).to("cuda:0")
             for x in st.chunks]
    want = torch.cat([plain[ch] for ch, _, _ in slices])
    t = torch.full((3 + total + 29,), 0xA5, dtype=torch.uint8, device="cuda:0")
    c = Chunker(ChunkParams(), 0)
    _, cok, sok = c.read_slices(dev, st.offs, st.refs, slices, out=t[3:3 + total])
    c.close()
    assert cok.all() and sok.all()
    assert torch.equal(t[3:3 + total], want)
    assert bool((t[:3] == 0xA5).all()) and bool((t[3 + total:] == 0xA5).all())


def test_coalesced_chacha_past_its_default_cap():
    """chacha_xor_coalesced_kernel at the shipped grid over 1.25 x what one pass covers:
    about 80 chunks drawn from four distinct contents of about 2 MiB, fewer chunks than
    refid_split()'s bound, so the split form is the library's own choice."""
    import torch

    cus = compute_units()
    sizes = [(2 << 20) + 1, (2 << 20) - 65, (2 << 20) + 4099, (2 << 20) + 63]
    st = Stored(sizes, 69)
    pick, total = [], 0
    while total < _past_the_chacha_cap(cus):
        pick.append((5 * len(pick) + len(pick) // 4) % 4)
        total += sizes[pick[-1]]
    assert len(set(pick)) == 4 and len(pick) <= cus * 4 * 2 * 16
    blocks = sum(ks_blocks(0, sizes[i]) for i in pick)
    assert passes(blocks, cus * 32) >= 2
    parts = [torch.from_numpy(np.frombuffer(x, dtype=np.uint8).copy()).to("cuda:0")
             for x in st.chunks]
    t = torch.cat([parts[i] for i in pick])
    offs = np.concatenate([[0], np.cumsum([sizes[i] for i in pick])]).astype(np.uint64)
    c = Chunker(ChunkParams(), 0)
    refs, hashes = c.create_refs(t, offs)
    split = c.last_create_split()
    c.close()
    assert split is True
    assert_rows_equal(hashes, st.hashes[pick], "content hash")
    assert_rows_equal(refs["dek"], st.refs["dek"][pick], "dek")
    assert_rows_equal(refs["id"], st.refs["id"][pick], "id")
