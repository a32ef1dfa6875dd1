"""The data plane past 4 GiB and the scan's serial tails past their first pass.

One device-resident batch of 2^32 + ~100 MiB bytes, filled by the device generator and copied
to the host once, goes through the scan at three parameter sets, the candidate list, the static
skip, the Ref.Ids, the generator and the commit round trip.  Every byte offset the kernels
handle above 2^32 (file, chunk and output offsets, the slow-path tail copy), compact_tiles
past 768 tiles, the selection's 64-way search past 4,096 entries, segcompact_block past 2,048
files, more than 65,536 segments, and ranks past the shared bucket (63) and the clamp (255)
are all inside it.  Whole results are compared with oracle/cdc_oracle.c; the sizes that make
the loops wrap are asserted from the layout and the oracle's output, never the kernel's.

Peak device memory is three such tensors (the commit round trip) plus the contexts, ~14 GiB;
the module skips only when the device reports less than 24 GiB free.
"""
import types

import numpy as np
import pytest

import scan_models
from oracle import chunker as Ch
from oracle import coracle
from pfs_amd import _lib
from pfs_amd.cdc import ChunkParams, Chunker, synthetic_piece_bytes

pytestmark = pytest.mark.gpu

P32 = 1 << 32
MIB = 1 << 20
N = P32 + 100 * MIB + 777_777          # 49 mod 64; the last tile holds 2.74 MiB
TILE768 = 768 * scan_models.TILE       # compact_tiles<768> takes its second pass from here
RUN_FILES, RUN_LEN = 700, 700          # a run of 490,000 B crowds a unit (256 KiB)
STRADDLER = 70 * MIB + 37
SEED = 0x4D1B

REFERENCE = Ch.Params()                # 23 / 1,000,000 / 20,000,000
MID = Ch.Params(average_bits=18, seed=1, min=270_001, max=700_000)
DENSE = Ch.Params(average_bits=14, seed=1, min=20_000, max=200_000)
BOTH_SKIPS = _lib.SCAN_SKIPPED_FIRST_MIN | _lib.SCAN_SKIPPED_CUTS


def cp(p):
    return ChunkParams(p.average_bits, p.seed, p.min, p.max)


def build_layout():
    """File lengths of the batch and the indices of its special files (deterministic)."""
    rng = np.random.default_rng(4242)
    lens, at = [], {"empty": [], "runs": []}
    off = 0

    def filler(ok=lambda end: True):
        # 1-6 MiB; neither the length nor the end offset a multiple of 64, the end never 49
        # mod 64 (the last file, which brings the batch to N = 49 mod 64, is then none either)
        nonlocal off
        z = int(rng.integers(1 * MIB, 6 * MIB))
        while z % 64 == 0 or (off + z) % 64 in (0, 49) or not ok(off + z):
            z += 1
        lens.append(z)
        off += z

    def run():
        # 700 files of 700 B from an offset that is 1 mod 4: offset + 700 k is then never a
        # multiple of 64 (700 k is a multiple of 4)
        nonlocal off
        filler(lambda end: end % 4 == 1)
        at["runs"].append((len(lens), off))
        lens.extend([RUN_LEN] * RUN_FILES)
        off += RUN_LEN * RUN_FILES

    def empty():
        at["empty"].append(len(lens))
        lens.append(0)

    while off < 300 * MIB:
        filler()
    empty()
    while off < TILE768 - 16 * MIB:
        filler()
    run()                                             # below the boundary of tile 768
    while off < P32 - 41 * MIB:
        filler()
    filler(lambda end: (end + STRADDLER) % 64 not in (0, 49))
    at["straddler"] = len(lens)
    lens.append(STRADDLER)                            # starts below 2^32, ends above it
    off += STRADDLER
    while off < P32 + 80 * MIB:
        filler()
    run()                                             # above 2^32
    while N - off > 8 * MIB:
        filler()
    lens.append(N - off)
    empty()
    return np.array(lens, dtype=np.int64), at


@pytest.fixture(scope="module")
def batch():
    import torch

    free, _ = torch.cuda.mem_get_info()
    if free < 24 << 30:
        pytest.skip("less than 24 GiB of device memory free")
    lens, at = build_layout()
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(offs[-1])
    nfiles = len(lens)
    U = scan_models.UNIT
    # the properties the tests rely on, from the layout alone
    assert n == N and n % 64 != 0 and -(-n // scan_models.TILE) > 768
    assert nfiles > 2048 and nfiles * 16384 <= n
    assert np.all(lens[lens > 0] % 64 != 0) and np.all(offs[1:] % np.uint64(64) != 0)
    assert len(at["empty"]) == 2 and np.count_nonzero(lens == 0) == 2
    special = np.zeros(nfiles, dtype=bool)
    special[at["empty"] + [at["straddler"], nfiles - 2]] = True
    for first, start in at["runs"]:
        special[first:first + RUN_FILES] = True
        assert int(offs[first]) == start and np.all(lens[first:first + RUN_FILES] == RUN_LEN)
        units = np.bincount((offs[first:first + RUN_FILES] // np.uint64(U)).astype(np.int64))
        assert units.max() > 64, "the run crowds no unit"
    (r1, s1), (r2, s2) = at["runs"]
    assert s1 + RUN_FILES * RUN_LEN < TILE768 and s2 > P32
    plain = lens[~special]
    assert len(plain) > 900 and plain.min() >= MIB and plain.max() < 6 * MIB + 256
    sf = at["straddler"]
    ss, se = int(offs[sf]), int(offs[sf + 1])
    assert ss < P32 < se and se - ss == STRADDLER
    for p in (REFERENCE, MID):  # its ranks pass the shared bucket (63) and the clamp (255)
        assert (se - 1) // U - (ss + p.min - 1) // U >= 256

    c = Chunker(cp(REFERENCE), device=0)
    dev = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    c.fill_synthetic(dev, offs, SEED)
    c.close()
    host = dev.cpu().numpy()
    b = types.SimpleNamespace(dev=dev, host=host, offs=offs, lens=lens, n=n, nfiles=nfiles,
                              straddler=sf, runs=at["runs"], cache={})
    yield b
    b.cache.clear()
    b.dev = b.host = None
    del dev, host
    torch.cuda.empty_cache()


def oracle(b, p):
    """(segments, file_begin) of the batch at p: one oracle run per parameter set."""
    key = ("segs", p)
    if key not in b.cache:
        b.cache[key] = coracle.segment_files(b.host, b.offs, p, nthreads=16)
    return b.cache[key]


def oracle_tiles(b, p):
    """The oracle's candidates per 3 MiB tile (only the mask width and the seed matter)."""
    key = ("tiles", p.average_bits, p.seed)
    if key not in b.cache:
        b.cache[key] = scan_models.tile_candidates(b.host, p, nthreads=16)
    return b.cache[key]


def same_as_oracle(res, want):
    """assert_same of test_gpu_parity.py against a precomputed oracle result."""
    segs, begin = want
    g = res.segments
    assert np.array_equal(res.file_begin, begin), "per-file segment counts differ"
    assert len(g) == len(segs)
    for field in ("offset", "size", "file", "flags"):
        bad = np.nonzero(g[field] != segs[field])[0]
        assert len(bad) == 0, \
            f"{field} differs at segments {bad[:5]}: gpu={g[bad[:5]]} cpu={segs[bad[:5]]}"
    bad = np.nonzero((g["hash"] != segs["hash"]).any(axis=1))[0]
    assert len(bad) == 0, f"digests differ at segments {bad[:5]}"


def seg_start(b, segs):
    return b.offs[segs["file"]] + segs["offset"]


def test_reference_params_whole_batch(batch):
    """23 / 1,000,000 / 20,000,000 with both skips: every segment and digest, the hash queue
    (bins auto) and the dispatch slots, ranks past 63 and 255 included."""
    b = batch
    want = oracle(b, REFERENCE)
    sf = b.straddler
    first, last = int(want[1][sf]), int(want[1][sf + 1]) - 1
    st = seg_start(b, want[0])
    assert st[first] < P32 < st[last] and last - first >= 3, "the oracle's straddling segments"
    c = Chunker(cp(REFERENCE), device=0)
    res = c.scan(b.dev, b.offs)
    assert c.last_scan_mode() == BOTH_SKIPS
    same_as_oracle(res, want)
    order, nxt, bin_bytes = c.debug_hash_queue()
    assert bin_bytes > RUN_LEN, "bins auto: a quad's share of 4 GiB"
    scan_models.check_hash_queue(order, nxt, bin_bytes, res.segments, b.offs)
    units = scan_models.check_scan_plan(c.debug_scan_plan(), b.offs, REFERENCE.min)
    assert max(r for (_, _, r, _) in units) > 255
    assert c.last_scan_bytes() <= scan_models.live_bytes(units, b.n)
    c.close()


def mid_entry_list(b):
    """The entry list the mid parameters produce, from the oracle alone, with the sizes the
    selection's search and the compaction need asserted on it."""
    key = "mid entries"
    if key not in b.cache:
        tiles = oracle_tiles(b, MID)
        counts = np.array([len(t) for t in tiles])
        entries = scan_models.entry_list(tiles, b.n)
        assert len(tiles) > 768
        assert len(entries) > 4096, "the 64-way search takes no second level"
        dense = counts > scan_models.TILE_K
        assert dense.any() and (~dense).any() and (counts[~dense] > 0).any()
        assert dense[768:].any() and (~dense)[768:].any(), "both kinds past the first pass"
        b.cache[key] = entries
    return b.cache[key]


@pytest.mark.parametrize("grid", [1, None])
def test_mid_params_whole_batch(batch, knob, grid):
    """bits 18, min 270,001, max 700,000, plan on: ~12,000 entries over dense and sparse
    tiles (two levels of the selection's 64-way search, rescans of dense tiles above 2^32);
    on one scan workgroup the earlier ranks have reported when the later ones start, so the
    281-rank file skips past settled cuts; and at the shipped grid."""
    b = batch
    mid_entry_list(b)
    want = oracle(b, MID)
    if grid:
        knob("PFSCDC_SCAN_GRID", grid)
    c = Chunker(cp(MID), device=0)
    res = c.scan(b.dev, b.offs)
    assert c.last_scan_mode() == BOTH_SKIPS
    same_as_oracle(res, want)
    units = scan_models.check_scan_plan(c.debug_scan_plan(), b.offs, MID.min)
    static = scan_models.live_bytes(units, b.n)
    rolled = c.last_scan_bytes()
    assert 0 < rolled <= static
    if grid == 1:
        assert rolled < static, "no unit skipped past a settled cut"
    c.close()


def test_dense_params_whole_batch(batch):
    """bits 14, min 20,000, max 200,000: every tile is dense (every cut comes out of
    rescan_first, at offsets on both sides of 2^32) and the batch has more than 65,536
    segments; the hash queue over them."""
    b = batch
    counts = np.array([len(t) for t in oracle_tiles(b, DENSE)])
    assert len(counts) > 768 and counts.min() > scan_models.TILE_K, "a tile is not dense"
    want = oracle(b, DENSE)
    assert len(want[0]) > 65_536
    c = Chunker(cp(DENSE), device=0)
    res = c.scan(b.dev, b.offs)
    same_as_oracle(res, want)
    order, nxt, bin_bytes = c.debug_hash_queue()
    scan_models.check_hash_queue(order, nxt, bin_bytes, res.segments, b.offs)
    c.close()


def test_candidate_list_past_one_compaction_pass(batch, knob):
    """Every byte rolled (PFSCDC_SCAN_SKIP=0) at the mid parameters: the scan's entry list
    equals the one built from the oracle's candidates, tile by tile: the candidates of a tile
    of at most 15, else one marker 1 << 63 | (tile_end - 1).  More than 768 tiles: the second
    pass of compact_tiles, where its carry runs."""
    b = batch
    want = mid_entry_list(b)
    knob("PFSCDC_SCAN_SKIP", 0)
    c = Chunker(cp(MID), device=0)
    c.set_cuts_only(True)
    c.scan(b.dev, b.offs)
    assert c.last_scan_mode() == 0 and c.last_scan_bytes() == b.n
    got = c.debug_candidates(cap=1 << 16)
    c.close()
    assert len(got) == len(want), f"{len(got)} entries, the oracle's list has {len(want)}"
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, \
        f"entries differ first at {bad[:3]} of {len(want)}: gpu={got[bad[:3]]} cpu={want[bad[:3]]}"


@pytest.mark.parametrize("p", [REFERENCE, MID], ids=["reference", "mid"])
def test_static_skip_rolls_the_models_bytes(batch, knob, p):
    """PFSCDC_SCAN_CUTSKIP=0: the bytes rolled are exactly the live bytes of the plan model
    (crowded units scanned whole, units and files above 2^32), not a recorded number."""
    b = batch
    knob("PFSCDC_SCAN_CUTSKIP", 0)
    c = Chunker(cp(p), device=0)
    res = c.scan(b.dev, b.offs)
    assert c.last_scan_mode() == _lib.SCAN_SKIPPED_FIRST_MIN
    same_as_oracle(res, oracle(b, p))
    units = scan_models.plan_units(b.offs, p.min, plan=False)
    assert any(tf is None for (_, tf, _, _) in units), "no crowded unit scanned whole"
    assert c.last_scan_bytes() == scan_models.live_bytes(units, b.n)
    assert len(c.debug_scan_plan()) == 0
    c.close()


def test_ref_ids_on_both_sides_of_4gib(batch):
    """Scan with Ref.Ids at the reference parameters: (id, dek) against Ch.create_ref_id for
    every segment of the file across 2^32, the batch's first and last segment, 8 segments
    wholly above 2^32 and 4 below."""
    b = batch
    segs, begin = oracle(b, REFERENCE)
    st, en = seg_start(b, segs), seg_start(b, segs) + segs["size"]
    sf = b.straddler
    pick = list(range(int(begin[sf]), int(begin[sf + 1]))) + [0, len(segs) - 1]
    above, below = np.flatnonzero(st >= P32), np.flatnonzero(en <= P32)
    tiny_above = above[segs["size"][above] == RUN_LEN]
    tiny_below = below[segs["size"][below] == RUN_LEN]
    big_above = above[segs["size"][above] > MIB]
    big_below = below[segs["size"][below] > MIB]
    pick += [int(x) for x in tiny_above[[0, 350, -1]]] + [int(x) for x in tiny_below[[0, -1]]]
    pick += [int(x) for x in big_above[np.linspace(0, len(big_above) - 1, 5).astype(int)]]
    pick += [int(x) for x in big_below[[3, len(big_below) // 2]]]
    assert sum(st[i] >= P32 for i in pick) >= 8 and sum(en[i] <= P32 for i in pick) >= 4
    c = Chunker(cp(REFERENCE), device=0, ref_ids=True)
    res = c.scan(b.dev, b.offs)
    same_as_oracle(res, (segs, begin))
    for i in sorted(set(pick)):
        rid, dek = Ch.create_ref_id(b.host[int(st[i]):int(en[i])].tobytes())
        assert bytes(res.refs[i]["dek"]) == dek and bytes(res.refs[i]["id"]) == rid, \
            (i, int(st[i]), int(segs["size"][i]))
    c.close()


def test_generator_matches_its_host_mirror_past_4gib(batch):
    """synth_kernel against synthetic_piece_bytes: the straddling file's bytes around 2^32
    (file offsets of tens of MiB at batch offsets across 2^32) and the last file."""
    b = batch
    sf = b.straddler
    ss = int(b.offs[sf])
    for a, z in ((P32 - ss - 70_001, 140_003), (0, 4099), (STRADDLER - 4099, 4099)):
        want = synthetic_piece_bytes(sf, a, z, SEED)
        assert np.array_equal(b.host[ss + a:ss + a + z], want), (a, z)
    last = b.nfiles - 2  # (the very last file is empty)
    ls, le = int(b.offs[last]), int(b.offs[last + 1])
    assert le == b.n and ls > P32
    assert np.array_equal(b.host[ls:le], synthetic_piece_bytes(last, 0, le - ls, SEED))


@pytest.mark.parametrize("split", [0, 1])
def test_commit_round_trip_on_the_device(batch, knob, split):
    """The commit data plane and Get over every byte, on the device: a cuts-only scan at the
    reference parameters, form_chunks, commit_refs(create=True) with the ciphertext in place,
    then get_chunks of that buffer into a second tensor: every chunk verifies and the
    plaintext equals a freshly generated copy of the batch (ChaCha20 both ways and the
    BLAKE2b modes at every offset above 2^32, at no host cost); the Refs of 6 chunks (2 below
    2^32, the one across it, 3 above) equal the oracle's.

    In place the Ref.Id pass always takes the split form (ChaCha20, then BLAKE2b of the
    ciphertext): the fused kernel's pointers must not alias, PFSCDC_REFID_SPLIT=0 cannot
    force it there.  So with the knob at 0 the fused form runs where it can, create_refs over
    the untouched batch, and ITS Refs then open the ciphertext the split form wrote."""
    import torch

    b = batch
    knob("PFSCDC_REFID_SPLIT", split)
    c = Chunker(cp(REFERENCE), device=0)
    c.set_cuts_only(True)
    c.set_ctext_in_place(True)
    work = torch.empty(b.n, dtype=torch.uint8, device="cuda:0")
    c.fill_synthetic(work, b.offs, SEED)
    res = c.scan(work, b.offs)
    want = oracle(b, REFERENCE)
    for f in ("offset", "size", "file", "flags"):
        assert np.array_equal(res.segments[f], want[0][f]), f
    coffs, _, known = c.form_chunks()
    nch = len(coffs) - 1
    assert int(coffs[-1]) == b.n and nch > 200
    fused = None
    if split == 0:
        f = Chunker(cp(REFERENCE), device=0)
        fused, _ = f.create_refs(b.dev, coffs)
        assert f.last_create_split() is False
        f.close()
    refs, chash, seg_hashes = c.commit_refs(work, coffs, known, create=True)
    assert c.last_create_split() is True
    assert np.array_equal(seg_hashes, want[0]["hash"]), "DataRef hashes differ from the oracle's"
    if fused is not None:
        assert np.array_equal(fused["id"], refs["id"]) and np.array_equal(fused["dek"], refs["dek"])
        refs = fused
    across = int(np.searchsorted(coffs, P32, side="right")) - 1
    assert coffs[across] < P32 < coffs[across + 1]
    sample = [1, across // 2, across, across + 1, (across + nch) // 2, nch - 1]
    for i in sample:
        a, e = int(coffs[i]), int(coffs[i + 1])
        key = ("ref", a, e)
        if key not in b.cache:
            b.cache[key] = Ch.create_ref_id(b.host[a:e].tobytes())
        rid, dek = b.cache[key]
        assert bytes(refs[i]["id"]) == rid and bytes(refs[i]["dek"]) == dek, (i, a, e)
    out = torch.empty(b.n, dtype=torch.uint8, device="cuda:0")
    got, ok = c.get_chunks(work, coffs, refs, out=out)
    assert got is out and ok.all(), f"chunks not verified: {np.flatnonzero(~ok)[:5]}"
    del work
    fresh = torch.empty(b.n, dtype=torch.uint8, device="cuda:0")
    c.fill_synthetic(fresh, b.offs, SEED)
    torch.cuda.synchronize()
    assert torch.equal(out, fresh), "the plaintext read back differs from the batch"
    assert torch.equal(fresh, b.dev), "the batch itself changed"
    c.close()
