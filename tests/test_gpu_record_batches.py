"""The data plane's BLAKE2b record batches at degenerate sizes and on reuse of one context:
pfscdc_hash_data_refs, hash_ranges, create_refs, get_chunks, read_slices and commit_refs with
zero, one and a few records, empty records among others, every record known or none, and one
Chunker taken through all of them in turn.  A refused call must leave the context usable.

Every expected value comes from hashlib's BLAKE2b-256 and the oracle (Ch.create_ref_id,
Ch.chacha20_xor, coracle.segment_files), never from the library."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from oracle import chunker as Ch
from oracle import coracle
from pfs_amd import _lib
from pfs_amd.cdc import ChunkParams, Chunker, synthetic_bytes
from stored_chunks import Stored

pytestmark = pytest.mark.gpu

SMALL = Ch.Params(average_bits=12, seed=1, min=2000, max=30000)  # as tests/test_gpu_refid.py
CP = ChunkParams(SMALL.average_bits, SMALL.seed, SMALL.min, SMALL.max)


def b2(data) -> bytes:
    return hashlib.blake2b(bytes(data), digest_size=32).digest()


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


@pytest.fixture(scope="module")
def chunker():
    c = Chunker(CP, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    return synthetic_bytes(np.array([0, 64 << 10], dtype=np.uint64), 1717)


def want_ranges(data, begins, sizes):
    return np.array([np.frombuffer(b2(data[b:b + z]), dtype=np.uint8)
                     for b, z in zip(begins, sizes)]).reshape(len(begins), 32)


def check_created(data, offs, refs, hashes):
    for i in range(len(offs) - 1):
        chunk = data[int(offs[i]):int(offs[i + 1])].tobytes()
        assert bytes(hashes[i]) == b2(chunk), i
        assert (bytes(refs[i]["id"]), bytes(refs[i]["dek"])) == Ch.create_ref_id(chunk), i


# ------------------------------------------------------------------ pfscdc_hash_data_refs

@pytest.mark.parametrize("n", [0, 1, 4, 5])
def test_hash_data_refs_around_one_block(chunker, data, n):
    buf = data[:32 * n].tobytes()  # n = 4: exactly one 128-byte BLAKE2b block
    out = (C.c_uint8 * 32)()
    rc = chunker.lib.pfscdc_hash_data_refs(chunker.ctx, buf if n else None, n, out)
    assert rc == 0
    assert bytes(out) == b2(buf)


# ------------------------------------------------------------------ hash_ranges

@pytest.mark.parametrize("on_device", [False, True])
def test_hash_ranges_degenerate_sizes_in_one_call(chunker, data, on_device):
    buf = data[:1000]
    begins = [10, 0, 3, 100, 200, 300, 400, 1000 - 77, 1000]
    sizes = [0, 1, 127, 128, 129, 200, 200, 77, 0]  # [300, 500) and [400, 600) overlap
    src = buf
    if on_device:
        import torch
        src = torch.from_numpy(buf.copy()).to("cuda:0")
    got = chunker.hash_ranges(src, begins, sizes)
    assert np.array_equal(got, want_ranges(buf, begins, sizes))


# ------------------------------------------------------------------ create_refs

@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("sizes", [[3000], [500, 0, 700], [129, 1, 2048, 64]])
def test_create_refs_few_chunks_known_or_not(chunker, data, knob, split, sizes):
    knob("PFSCDC_REFID_SPLIT", split)
    offs = offsets(sizes)
    buf = data[:int(offs[-1])]
    n = len(sizes)
    want = np.array([np.frombuffer(b2(buf[int(a):int(b)]), dtype=np.uint8)
                     for a, b in zip(offs[:-1], offs[1:])])
    # no content hash known
    refs, hashes = chunker.create_refs(buf, offs)
    assert chunker.last_create_split() == bool(split)
    check_created(buf, offs, refs, hashes)
    # every content hash known (k = 0)
    refs, hashes = chunker.create_refs(buf, offs, want, np.ones(n, np.uint8))
    check_created(buf, offs, refs, hashes)
    # the first one known only
    known = np.zeros(n, np.uint8)
    known[0] = 1
    given = np.where(known[:, None] == 1, want, 0).astype(np.uint8)
    refs, hashes = chunker.create_refs(buf, offs, given, known)
    check_created(buf, offs, refs, hashes)


# ------------------------------------------------------------------ get_chunks

@pytest.mark.parametrize("on_device", [False, True])
def test_get_chunks_empty_chunk_among_others(chunker, on_device):
    st = Stored([700, 0, 129, 1, 0], 1801)
    if on_device:
        import torch
        ct = torch.from_numpy(st.ctext).to("cuda:0")
        out = torch.zeros(len(st.ctext), dtype=torch.uint8, device="cuda:0")
        res, ok = chunker.get_chunks(ct, st.offs, st.refs, out=out)
        assert res is out
        got = out.cpu().numpy()
    else:
        got, ok = chunker.get_chunks(st.ctext, st.offs, st.refs)
    assert len(ok) == 5 and ok.all()
    assert np.array_equal(got, st.plain)


# ------------------------------------------------------------------ read_slices

def test_read_slices_zero_hash_records_zero_slices_some_named(chunker):
    st = Stored([600, 0, 300, 128], 1802)
    # every named chunk marked verified: the verify pass has no record
    slices = [(0, 10, 100), (2, 0, 300), (0, 599, 1)]
    ver = np.array([1, 0, 1, 0], dtype=np.uint8)
    got, cok, sok = chunker.read_slices(st.ctext, st.offs, st.refs, slices, verified=ver)
    assert got.tobytes() == st.sliced(slices) == st.oracle(slices)
    assert sok.all() and [bool(x) for x in cok] == [True, False, True, False]
    # no slice at all over four chunks: nothing is hashed, every chunk reports its mark
    got, cok, sok = chunker.read_slices(st.ctext, st.offs, st.refs, [], verified=ver)
    assert len(got) == 0 and len(sok) == 0
    assert [bool(x) for x in cok] == [True, False, True, False]
    got, cok, sok = chunker.read_slices(st.ctext, st.offs, st.refs, [])
    assert len(got) == 0 and not cok.any()
    # only chunks 3 and 0 named; a damaged chunk nobody names does not matter
    bad = st.ctext.copy()
    bad[int(st.offs[2]) + 5] ^= 0x08
    slices = [(3, 1, 127), (0, 0, 600), (3, 0, 128)]
    got, cok, sok = chunker.read_slices(bad, st.offs, st.refs, slices)
    assert got.tobytes() == st.sliced(slices)
    assert sok.all() and [bool(x) for x in cok] == [True, False, False, True]
    # and named, it is found
    got, cok, sok = chunker.read_slices(bad, st.offs, st.refs, slices + [(2, 0, 4)])
    assert [bool(x) for x in cok] == [True, False, False, True]
    assert [bool(x) for x in sok] == [True, True, True, False]
    assert got.tobytes() == st.sliced(slices) + bytes(4)


# ------------------------------------------------------------------ commit_refs

def scan_for_commit(c, data, offs, streams):
    c.set_cuts_only(True)
    res = c.scan(data, offs)
    coffs, _, known = c.form_chunks(streams)
    segs = [data[int(offs[s["file"]]) + int(s["offset"]):][:int(s["size"])] for s in res.segments]
    return coffs, known, np.array([np.frombuffer(b2(x), dtype=np.uint8) for x in segs])


def test_commit_refs_hashes_only_all_known_one_chunk(data):
    c = Chunker(CP, 0)
    # small files in one stream: multi-DataRef chunks (content hash unknown) among known ones
    lens = [700, 900, 1500, 20_000, 300, 0, 9_000, 800]
    offs = offsets(lens)
    buf = data[:int(offs[-1])]
    coffs, known, want_seg = scan_for_commit(c, buf, offs, None)
    assert (known == 0).any()
    refs, chash, seg = c.commit_refs(buf, coffs, known, create=False)
    assert refs is None
    assert np.array_equal(seg, want_seg)
    for i in range(len(coffs) - 1):
        assert bytes(chash[i]) == b2(buf[int(coffs[i]):int(coffs[i + 1])]), i
    # and with chunk.Create
    coffs, known, want_seg = scan_for_commit(c, buf, offs, None)
    refs, chash, seg = c.commit_refs(buf, coffs, known)
    assert np.array_equal(seg, want_seg)
    check_created(buf, coffs, refs, chash)
    # every file its own stream: every chunk is one segment, every content hash known
    lens = [9_000, 2_500, 14_000]
    offs = offsets(lens)
    buf = data[:int(offs[-1])]
    coffs, known, want_seg = scan_for_commit(c, buf, offs, [0, 1, 2, 3])
    assert known.all() and len(coffs) - 1 == len(want_seg)
    refs, chash, seg = c.commit_refs(buf, coffs, known)
    assert np.array_equal(seg, want_seg) and np.array_equal(chash, want_seg)
    check_created(buf, coffs, refs, chash)
    # one file that is one chunk
    offs = offsets([1500])
    buf = data[:1500]
    coffs, known, want_seg = scan_for_commit(c, buf, offs, None)
    assert coffs.tolist() == [0, 1500] and known.all() and len(want_seg) == 1
    refs, chash, seg = c.commit_refs(buf, coffs, known)
    assert np.array_equal(seg, want_seg)
    check_created(buf, coffs, refs, chash)
    c.close()


# ------------------------------------------------------------------ reuse of one Chunker

def test_one_chunker_through_every_batch_in_turn(data):
    c = Chunker(CP, 0)
    rng = np.random.default_rng(1803)
    begins = rng.integers(0, len(data) - 600, 300)
    sizes = rng.integers(0, 600, 300)
    want300 = want_ranges(data, begins, sizes)
    assert np.array_equal(c.hash_ranges(data, begins, sizes), want300)
    assert np.array_equal(c.hash_ranges(data, [77], [4000]), want_ranges(data, [77], [4000]))
    offs3 = offsets([1000, 2000, 500])
    buf3 = data[:3500]
    refs, hashes = c.create_refs(buf3, offs3)
    check_created(buf3, offs3, refs, hashes)
    st = Stored(None, 0, chunks=[buf3[int(a):int(b)].tobytes()
                                 for a, b in zip(offs3[:-1], offs3[1:])])
    slices = [(2, 0, 500), (0, 999, 1), (1, 64, 1900)]
    got, cok, sok = c.read_slices(st.ctext, st.offs, refs, slices)
    assert cok.all() and sok.all() and got.tobytes() == st.sliced(slices)
    foffs = offsets([20_000, 0, 1, 30_000, 15_535])
    res = c.scan(data, foffs)
    segs, _ = coracle.segment_files(data, foffs, SMALL, nthreads=4)
    assert len(res.segments) == len(segs)
    for f in ("offset", "size", "file", "hash"):
        assert np.array_equal(res.segments[f], segs[f]), f
    assert c.lib.pfscdc_num_segments(c.ctx) == len(segs)
    assert np.array_equal(c.hash_ranges(data, begins, sizes), want300)
    assert c.lib.pfscdc_num_segments(c.ctx) == 0  # the batch took the scan's records
    # a cuts-only scan whose records a batch then overwrote is no scan to commit
    c.set_cuts_only(True)
    c.scan(data, foffs)
    coffs, _, known = c.form_chunks()
    assert np.array_equal(c.hash_ranges(data, [0], [1]), want_ranges(data, [0], [1]))
    with pytest.raises(_lib.PfsCdcError, match="needs the last scan") as e:
        c.commit_refs(data, coffs, known)
    assert e.value.code == _lib.PFSCDC_ESTATE
    c.close()


# ------------------------------------------------------------------ a refused call

def test_refused_calls_leave_the_chunker_usable(data):
    import torch
    c = Chunker(CP, 0)
    st = Stored([700, 300], 1804)
    buf = data[:1000]
    good = offsets([700, 300])
    for offs, text in [([0, 700, 999], "chunk_offsets must start at 0 and end at nbytes"),
                       ([1, 700, 1000], "chunk_offsets must start at 0 and end at nbytes"),
                       ([0, 1200, 1000], "chunk_offsets must be nondecreasing")]:
        for call in (lambda o: c.create_refs(buf, o),
                     lambda o: c.get_chunks(st.ctext, o, st.refs),
                     lambda o: c.read_slices(st.ctext, o, st.refs, [(0, 0, 10)])):
            with pytest.raises(_lib.PfsCdcError, match=text) as e:
                call(np.array(offs, dtype=np.uint64))
            assert e.value.code == _lib.PFSCDC_EINVAL
    refs, hashes = c.create_refs(buf, good)
    check_created(buf, good, refs, hashes)
    got, ok = c.get_chunks(st.ctext, good, st.refs)
    assert ok.all() and np.array_equal(got, st.plain)
    # a device pointer off the 16-byte grid
    t = torch.zeros(1001 + 16, dtype=torch.uint8, device="cuda:0")
    t[1:1001] = torch.from_numpy(buf.copy()).to("cuda:0")
    with pytest.raises(_lib.PfsCdcError, match="device bytes must be 16-byte aligned") as e:
        c.hash_ranges(t[1:1001], [0], [1000])
    assert e.value.code == _lib.PFSCDC_EINVAL
    with pytest.raises(_lib.PfsCdcError, match="device bytes must be 16-byte aligned"):
        c.create_refs(t[1:1001], good)
    t[1:1001] = torch.from_numpy(st.ctext).to("cuda:0")
    with pytest.raises(_lib.PfsCdcError, match="device ctext must be 16-byte aligned"):
        c.get_chunks(t[1:1001], good, st.refs, out=torch.zeros(1000, dtype=torch.uint8,
                                                              device="cuda:0"))
    with pytest.raises(_lib.PfsCdcError, match="device ctext must be 16-byte aligned"):
        c.read_slices(t[1:1001], good, st.refs, [(0, 0, 10)])
    assert np.array_equal(c.hash_ranges(buf, [0, 999], [1000, 1]),
                          want_ranges(buf, [0, 999], [1000, 1]))
    t[16:1016] = torch.from_numpy(st.ctext).to("cuda:0")
    got, cok, _ = c.read_slices(t[16:1016], good, st.refs, [(1, 5, 200)])
    assert cok[1] and not cok[0]  # chunk 0: not named, not marked
    assert got.tobytes() == st.sliced([(1, 5, 200)])
    c.close()
