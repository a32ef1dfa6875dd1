"""Reading filesets back on the GPU: the UnorderedWriter uploads into a store
(pfscdc_uw_set_store), pfscdc_index_read opens the roots it leaves, and the lists are held
against the writer's own PFSCDC_EV_INDEX events (decoded here with the protobuf runtime, an
encoder/decoder pair the library shares no code with) and against pfscdc_index_decode_host;
then filters, both decode arms, streams that do not parse, error codes, the merged view as a
tar stream, a device group, and a plain C process."""
import ctypes as C
import io
import os
import random
import subprocess
import tarfile

import numpy as np
import pytest

import tar_oracle as T
from stored_chunks import created
from test_index_read_cpu import filter_forms, flat_filter

from oracle import chunker as Ch
from oracle import fileset as OF
from pfs_amd import _lib
from pfs_amd import chunk as pc
from pfs_amd import fileset as PF
from pfs_amd.cdc import ChunkParams, Chunker, synthetic_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = Ch.Params(average_bits=12, seed=1, min=2000, max=30000)
# index chunking (test hook): an entry of ~950 bytes must still meet at most one cut on the
# levels above 0, or the index never converges (an entry a chunk lies inside is written again,
# whole, one level up: index/writer.go:102-121)
INDEX = Ch.Params(average_bits=9, seed=2, min=300, max=1000)


# for the Put/Delete sequences: every entry (appended files of a few DataRefs) stays below avg
LOOP_INDEX = Ch.Params(average_bits=12, seed=0, min=3000, max=30000)


def cp(p):
    return ChunkParams(p.average_bits, p.seed, p.min, p.max)


def write(ops, mem_threshold=10 ** 9, index=INDEX, devices=None):
    store = pc.ChunkStore()
    st = PF.Storage(0, cp(SMALL), mem_threshold, cp(index), devices=devices, store=store)
    w = st.new_unordered_writer()
    for op in ops:
        if op[0] == "put":
            w.put(*op[1:])
        else:
            w.delete(*op[1:])
    infos = w.close()
    events = w.events
    w.release()
    return st, infos, events


def frames_of(events, which):
    return [e[2] for e in events if e[0] == "index" and e[1] == which]


def want_entries(events, which):
    """The level-0 entries of one index as the writer's events give them."""
    M = OF._msgs()["Index"]
    out = []
    for fr in frames_of(events, which):
        assert int.from_bytes(fr[:8], "little") == len(fr) - 8
        m = M.FromString(fr[8:])
        out.append((m.path.encode(), m.file.tag.encode(),
                    [(d.ref.id, d.ref.dek, d.ref.size_bytes, d.ref.edge, d.hash, d.offset_bytes,
                      d.size_bytes) for d in m.file.data_refs]))
    return out


def got_entries(lst):
    return [(g["path"], g["tag"],
             [(d.ref.id, d.ref.dek, d.ref.size_bytes, d.ref.edge, d.hash, d.offset_bytes,
               d.size_bytes) for d in g["data_refs"]]) for g in lst.raw()]


def shape(events, which):
    """Index levels, level-0 chunk borders inside a frame, level-0 chunks inside one frame."""
    frames = frames_of(events, which)
    chunks = [e[3] for e in events if e[0] == "chunk" and e[1] == which and e[2] == 0]
    levels = 1 + max([e[2] for e in events if e[0] == "chunk" and e[1] == which], default=-1)
    fb = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    cb = np.concatenate([[0], np.cumsum(chunks)]).astype(np.int64)
    assert fb[-1] == cb[-1]
    starts = set(fb.tolist())
    cross = sum(1 for b in cb[1:-1] if int(b) not in starts)
    inside = 0
    for i in range(len(chunks)):
        k = int(np.searchsorted(fb, cb[i], side="right")) - 1
        inside += bool(fb[k] < cb[i] and cb[i + 1] < fb[k + 1])
    return levels, cross, inside, max((len(f) for f in frames), default=0)


def big_ops():
    """60 files, two of them of 45,000 bytes (about 8 DataRefs: an entry of ~950 bytes)."""
    data = synthetic_bytes([0, 600_000], 3).tobytes()
    ops, pos = [], 0
    for i in range(60):
        n = 45_000 if i in (17, 41) else 300 + 37 * i
        ops.append(("put", "/d%d/f%03d" % (i % 3, i), "", False, data[pos:pos + n]))
        pos += n
    return ops + [("delete", "/gone", ""), ("delete", "/gone2", "")]


@pytest.fixture(scope="module")
def big():
    return write(big_ops())


@pytest.fixture
def chunker():
    c = Chunker(ChunkParams(), 0)
    yield c
    c.close()


def roots(info):
    return [(0, info.additive), (1, info.deletive)]


def test_read_back_equals_the_writers_events(big, chunker):
    st, infos, events = big
    assert len(infos) == 1
    levels, cross, inside, longest = shape(events[0], 0)
    print("additive index: levels", levels, "borders inside a frame", cross,
          "chunks inside a frame", inside, "longest frame", longest)
    assert levels >= 3
    assert cross >= 1
    # a level-0 chunk that lies wholly inside one entry: its Range.Offset (0) is no frame start
    assert inside >= 1 and longest > INDEX.min
    rewalked = 0
    for which, root in roots(infos[0]):
        assert root is not None
        lst = PF.index_read(chunker, st.store, root)
        stats = PF.last_index_stats(chunker)
        print("index", which, stats)
        want = want_entries(events[0], which)
        assert len(want) >= 2
        assert got_entries(lst) == want
        host = PF.index_decode_host(b"".join(frames_of(events[0], which)))
        assert got_entries(host) == want
        assert lst.raw() == host.raw()
        assert stats["frames"] >= len(want) and stats["levels"] >= 1
        if which == 0:
            assert stats["levels"] == levels
            rewalked = stats["rewalked_chunks"]
    assert rewalked > 0


@pytest.mark.parametrize("decode, grid", [(0, 0), (1, 1), (1, 3), (0, 3)])
def test_both_decode_arms_and_many_passes(big, chunker, knob, decode, grid):
    st, infos, events = big
    base = [PF.index_read(chunker, st.store, root).raw() for _, root in roots(infos[0])]
    knob("PFSCDC_INDEX_DECODE", decode)
    knob("PFSCDC_CHACHA_GRID", grid)
    for (which, root), want in zip(roots(infos[0]), base):
        got = PF.index_read(chunker, st.store, root)
        assert got.raw() == want
        assert got_entries(got) == want_entries(events[0], which)


def test_empty_root_and_single_entry_root(chunker):
    store = pc.ChunkStore()
    assert len(PF.index_read(chunker, store, None)) == 0
    assert len(PF.index_read(chunker, store, b"")) == 0
    one = OF.encode_index(OF.Index("/only", "default", []))
    assert [g["path"] for g in PF.index_read(chunker, store, one).raw()] == [b"/only"]
    assert len(PF.index_read(chunker, store, one, prefix="/x")) == 0


def hand_built_index(rng, cut=200):
    """A two-level index built by hand, so that an entry may be larger than twice the chunk
    size (the writer's own levels never converge over such an entry): 24 level-0 entries, one
    of ~1,400 bytes, one pair that shares a path (two tags) with the second starting exactly on
    a chunk border; the stream cut every `cut` bytes; the Range entries index/writer.go:102-121
    would write for those chunks (the chunk's first annotation, or its second when the first
    continues the previous chunk's last path; Offset = where that annotation begins in the
    chunk), in one level-1 chunk; and the root over it."""
    def dr():
        ref = Ch.Ref(size_bytes=rng.randrange(1, 1 << 30), edge=bool(rng.getrandbits(1)),
                     id=rng.randbytes(32), dek=rng.randbytes(32))
        return Ch.DataRef(ref, rng.randbytes(32), rng.randrange(1 << 20), rng.randrange(1 << 20))
    entries = [OF.Index("/e%02d" % i, "default", [dr() for _ in range(12 if i == 9 else i % 3)])
               for i in range(24)]
    frames = [OF.frame(OF.encode_index(e)) for e in entries]
    # pad entry 14's path so that entry 16 (same path as 15, another tag) starts on a border
    entries[15] = OF.Index("/e15", "t1", [dr()])
    entries[16] = OF.Index("/e15", "t2", [dr()])
    for pad in range(cut):
        entries[14] = OF.Index("/e14" + "x" * pad, "default", [])
        frames = [OF.frame(OF.encode_index(e)) for e in entries]
        if sum(map(len, frames[:16])) % cut == 0:
            break
    else:
        raise AssertionError("no padding puts entry 16 on a chunk border")
    stream = b"".join(frames)
    fb = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
    store = pc.ChunkStore()
    ranges, last = [], None
    for a in range(0, len(stream), cut):
        b = min(a + cut, len(stream))
        anns = [k for k in range(len(entries)) if fb[k] < b and fb[k + 1] > a]
        k = anns[0]
        if len(anns) > 1 and last is not None and entries[last].path == entries[k].path:
            k = anns[1]
        last = anns[-1]
        rid, dek, ct, _ = created(stream[a:b])
        store.put(rid, ct)
        ref = Ch.Ref(size_bytes=b - a, edge=False, id=rid, dek=dek)
        ranges.append(OF.Index(entries[k].path, entries[k].tag, entries[k].data_refs,
                               (max(0, int(fb[k]) - a), entries[last].path, ref)))
    top = b"".join(OF.frame(OF.encode_index(r)) for r in ranges)
    rid, dek, ct, _ = created(top)
    store.put(rid, ct)
    root = OF.encode_index(OF.Index(ranges[0].path, None, [], (
        0, ranges[-1].range[1], Ch.Ref(size_bytes=len(top), edge=False, id=rid, dek=dek))))
    inside = sum(1 for a in range(0, len(stream) - cut, cut)
                 if fb[9] < a and a + cut < fb[10])
    return store, root, entries, inside, int(fb[16]), max(map(len, frames))


@pytest.mark.parametrize("decode", [1, 0])
def test_an_entry_larger_than_twice_the_chunk_size(chunker, knob, decode):
    """Chunks wholly inside one entry (their Range.Offset 0 is mid-entry) and a chunk whose
    claim skips its first frame: the walk is settled along the chain and walked again."""
    cut = 200
    store, root, entries, inside, border, longest = hand_built_index(random.Random(31), cut)
    assert longest > 2 * cut and inside >= 2 and border % cut == 0
    knob("PFSCDC_INDEX_DECODE", decode)
    lst = PF.index_read(chunker, store, root)
    stats = PF.last_index_stats(chunker)
    print(stats)
    want = [(e.path.encode(), e.tag.encode(),
             [(d.ref.id, d.ref.dek, d.ref.size_bytes, d.ref.edge, d.hash, d.offset_bytes,
               d.size_bytes) for d in e.data_refs]) for e in entries]
    assert got_entries(lst) == want
    assert stats["levels"] == 2
    if decode:  # the chunks inside the entry, and the chunk that claims its second frame
        assert stats["rewalked_chunks"] >= inside + 1
    # every single path as a range filter: frames that cross the border into the first chunk
    # past the selection are still read whole, and only the chunks needed are read
    for e in entries:
        one = PF.index_read(chunker, store, root, lower=e.path, upper=e.path)
        assert [(g["path"], g["tag"]) for g in one.raw()] == \
            [(p, t) for p, t, _ in want if p == e.path.encode()], e.path
        assert PF.last_index_stats(chunker)["chunks_read"] < stats["chunks_read"]


# ------------------------------------------------------------------ filters

@pytest.fixture(scope="module")
def wide():
    data = synthetic_bytes([0, 300 * 64], 9).tobytes()
    ops = [("put", "/d%d/f%03d" % (i % 5, i), ["", "t1"][i % 7 == 0], False,
            data[64 * i:64 * i + 1 + i % 50]) for i in range(300)]
    return write(ops, index=Ch.Params(average_bits=9, seed=0, min=300, max=1000))


def test_filters_equal_the_flat_restatement(wide, chunker):
    st, infos, events = wide
    pairs = [(p, t) for p, t, _ in want_entries(events[0], 0)]
    assert len(pairs) == 300 and pairs == sorted(pairs)
    full = PF.index_read(chunker, st.store, infos[0].additive)
    all_chunks = PF.last_index_stats(chunker)["chunks_read"]
    assert [(g["path"], g["tag"]) for g in full.raw()] == pairs
    rng = random.Random(4)
    proper = 0
    for form in filter_forms(sorted({p for p, _ in pairs}), rng):
        got = PF.index_read(chunker, st.store, infos[0].additive, **form)
        want = flat_filter(pairs, **form)
        assert [(g["path"], g["tag"]) for g in got.raw()] == want, form
        proper += 0 < len(want) < 300
    assert proper > 20
    mid = pairs[150][0]
    got = PF.index_read(chunker, st.store, infos[0].additive, lower=mid, upper=mid)
    one_chunks = PF.last_index_stats(chunker)["chunks_read"]
    assert [g["path"] for g in got.raw()] == [mid]
    print("chunks read: all", all_chunks, "one file", one_chunks)
    assert one_chunks < all_chunks


# ------------------------------------------------------------------ errors

def _root_over(chunk: bytes, store):
    rid, dek, ct, _ = created(chunk)
    store.put(rid, ct)
    ref = Ch.Ref(size_bytes=len(chunk), edge=False, id=rid, dek=dek)
    return OF.encode_index(OF.Index("/a", None, [], (0, "/z", ref)))


@pytest.mark.parametrize("decode", [1, 0])
def test_a_stream_that_does_not_parse(chunker, knob, decode):
    """Valid launches over verified chunks whose bytes are no index: the bounds logic."""
    knob("PFSCDC_INDEX_DECODE", decode)
    rng = random.Random(21)
    good = OF.frame(OF.encode_index(OF.Index("/ok", "default", [])))
    cases = [(rng.randbytes(700), 0),                                   # a length that runs away
             (good + OF.frame(b"\x0a\x7f" + rng.randbytes(20)) + good, len(good)),  # a bad proto
             (good + (5).to_bytes(8, "little") + b"\x0a", len(good)),    # a frame cut by the end
             (good + b"\x00\x00\x00", len(good))]                        # no room for a length
    for chunk, where in cases:
        store = pc.ChunkStore()
        root = _root_over(chunk, store)
        out = C.c_void_p(0xDEAD)
        rc = chunker.lib.pfscdc_index_read(chunker.ctx, store._s, root, len(root), None,
                                           C.byref(out))
        msg = chunker.lib.pfscdc_last_error(chunker.ctx).decode()
        assert rc == _lib.PFSCDC_ECORRUPT, msg
        assert out.value is None  # no list: nothing was allocated, nothing written
        assert "index level 0" in msg and ("offset %d " % where) in msg, msg
    # the same chunks read fine as what they are
    store = pc.ChunkStore()
    lst = PF.index_read(chunker, store, _root_over(good + good, store))
    assert [g["path"] for g in lst.raw()] == [b"/ok", b"/ok"]


def test_tampered_and_missing_index_chunks(big, chunker):
    st, infos, events = big
    ids = list(dict.fromkeys(e[5] for e in events[0] if e[0] == "chunk"))
    index_ids = [e[5] for e in events[0] if e[0] == "chunk" and e[1] == 0 and e[2] == 0]
    victim = index_ids[len(index_ids) // 2]
    bad, short = pc.ChunkStore(), pc.ChunkStore()
    for rid in ids:
        ct = bytearray(st.store.get(rid))
        if rid != victim:
            short.put(rid, bytes(ct))
        else:
            ct[len(ct) // 2] ^= 0x10
        bad.put(rid, bytes(ct))
    with pytest.raises(_lib.PfsCdcError) as e:
        PF.index_read(chunker, bad, infos[0].additive)
    assert e.value.code == _lib.PFSCDC_ECORRUPT
    with pytest.raises(KeyError):
        PF.index_read(chunker, short, infos[0].additive)
    assert got_entries(PF.index_read(chunker, st.store, infos[0].additive)) == \
        want_entries(events[0], 0)


# ------------------------------------------------------------------ the loop, closed

def model_ops(seed, n=70):
    rng = random.Random(seed)
    data = synthetic_bytes([0, 400_000], seed).tobytes()
    ops, model, pos = [], {}, 0
    names = ["/a/f%02d" % k for k in range(14)] + ["/b/g%02d" % k for k in range(10)] + ["/top"]
    for i in range(n):
        p = rng.choice(names)
        if rng.random() < 0.2 and model:
            p = rng.choice(sorted(model))
            ops.append(("delete", p, ""))
            del model[p]
            continue
        size = rng.choice([0, 1, 511, 512, 513, 3000, 9000])
        body = data[pos:pos + size]
        pos += size
        append = rng.random() < 0.3
        ops.append(("put", p, "", append, body))
        model[p] = (model.get(p, b"") if append else b"") + body
    return ops, model


@pytest.mark.parametrize("seed", [1, 2])
def test_write_open_tar_equals_the_model(seed):
    ops, model = model_ops(seed)
    st, infos, events = write(ops, mem_threshold=30_000, index=LOOP_INDEX)
    assert len(infos) >= 4 and any(i.deletive for i in infos)
    fs = st.open(infos)
    files = fs.files()
    assert [(f.path, f.tag, f.size_bytes) for f in files] == \
        [(p, "default", len(model[p])) for p in sorted(model)]
    want = T.stream([(p, model[p]) for p in sorted(model)])
    tar = fs.tar()
    assert tar.size() == len(want)
    assert tar.read() == want
    assert b"".join(tar.windows(4096)) == want
    with tarfile.open(fileobj=io.BytesIO(tar.read()), mode="r:") as tf:
        got = {"/" + m.name.lstrip("/"): tf.extractfile(m).read() for m in tf}
    assert got == model
    p = sorted(model)[len(model) // 2]
    assert fs.read(p) == model[p]
    sub = st.open(infos, prefix="/b/")
    assert sub.tar().read() == T.stream([(p, model[p]) for p in sorted(model) if p.startswith("/b/")])
    assert [f.path for f in sub.files()] == [p for p in sorted(model) if p.startswith("/b/")]


def test_pax_entries_pass_through_with_the_file_named():
    st, infos, _ = write([("put", "/ascii", "", False, b"x"), ("put", "/é", "", False, b"y")])
    fs = st.open(infos)
    assert [f.path for f in fs.files()] == ["/ascii", "/é"]
    with pytest.raises(_lib.PfsCdcError) as e:
        fs.tar()
    assert e.value.code == _lib.PFSCDC_EUNSUPPORTED and "é" in str(e.value)


def test_store_does_not_change_events_or_roots():
    ops, _ = model_ops(3, 40)
    st, infos, events = write(ops, mem_threshold=30_000, index=LOOP_INDEX)
    plain = PF.Storage(0, cp(SMALL), 30_000, cp(LOOP_INDEX))
    w = plain.new_unordered_writer()
    for op in ops:
        (w.put if op[0] == "put" else w.delete)(*op[1:])
    infos2 = w.close()
    assert infos2 == infos and w.events == events
    w.release()
    ids = {e[5] for fs in events for e in fs if e[0] == "chunk"}
    assert len(st.store) == len(ids)  # data chunks and every index level's chunks


@pytest.mark.parametrize("how", ["workers", "group"])
def test_several_group_writers_upload_too(how, knob):
    ops, model = model_ops(4, 50)
    one, infos1, _ = write(ops, mem_threshold=30_000, index=LOOP_INDEX)
    knob("PFSCDC_UW_INFLIGHT", 60_000)
    if how == "workers":
        knob("PFSCDC_UW_WORKERS", 2)
        st, infos, _ = write(ops, mem_threshold=30_000, index=LOOP_INDEX)
    else:
        st, infos, _ = write(ops, mem_threshold=30_000, index=LOOP_INDEX, devices=[0, 0])
    assert infos == infos1
    got, want = st.open(infos), one.open(infos1)
    assert got._list.raw() == want._list.raw()
    assert got.tar().read() == T.stream([(p, model[p]) for p in sorted(model)])


# ------------------------------------------------------------------ a plain C process

def test_plain_c_process_writes_reads_merges_and_renders(tmp_path):
    exe = str(tmp_path / "index_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "index_consumer.c"),
                    "-L", libdir, "-lpfscdc", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    out = str(tmp_path / "out.tar")
    res = subprocess.run([exe, out], capture_output=True, text=True, timeout=100)
    assert res.returncode == 0, res.stdout + res.stderr
    # the program's workload: file k of 24 is (k * 997 + 13) bytes of (k + j) & 0xff, written
    # over several filesets; /f03 deleted, /f05 put again as "again"
    model = {"/f%02d" % k: bytes((k + j) & 0xFF for j in range(k * 997 + 13)) for k in range(24)}
    del model["/f03"]
    model["/f05"] = b"again"
    assert open(out, "rb").read() == T.stream([(p, model[p]) for p in sorted(model)])
    assert res.stdout.split()[:2] == ["ok", str(len(model))]
