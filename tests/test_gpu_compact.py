"""Compaction on the GPU: Storage.compact / concat / shard and the fileset writer under them
(pfscdc_fsw_*) against the restated oracle (tests/compact_oracle.py: roots, SizeBytes, level-0
index frames and data-chunk events, cheap copies included), against a dict model through the
read path (tar of the compacted fileset = tar of its inputs), the reference's shardedCompact
(shard, compact each range, concat), the error paths, and a plain C99 process."""
import ctypes as C
import os
import random
import subprocess

import pytest

import compact_oracle as CO
import tar_oracle as T
from test_gpu_index_read import LOOP_INDEX, SMALL, cp

from oracle import chunker as Ch
from pfs_amd import _lib
from pfs_amd import chunk as pc
from pfs_amd import fileset as PF
from pfs_amd.cdc import ChunkParams, Chunker, synthetic_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["/a/f%02d" % k for k in range(10)] + ["/b/g%02d" % k for k in range(6)] + ["/top"]


def fileset_ops(seed, nfs):
    """Put/Delete sequences of nfs filesets (one unordered writer each) and the dict model of
    their merge.  Two files per fileset span several chunks, so whole chunks can be copied by
    reference; /never is deleted in fileset 1 and never put."""
    rng = random.Random(seed)
    data = synthetic_bytes([0, 700_000], seed).tobytes()
    seqs, model, pos = [], {}, 0
    for k in range(nfs):
        ops, touched, big = [], set(), 0
        for i in range(11):
            p = rng.choice(NAMES)
            if rng.random() < 0.2 and model:
                p = rng.choice(sorted(model))
                ops.append(("delete", p, ""))
                del model[p]
                touched.add(p)
                continue
            size = rng.choice([0, 1, 700, 3000, 9000])
            if big < 2 and i % 4 == 1:
                size, big = 40_000, big + 1
            body = data[pos:pos + size]
            pos += size
            append = rng.random() < 0.3
            ops.append(("put", p, "", append, body))
            model[p] = (model.get(p, b"") if append else b"") + body
        if k == 1:
            ops.append(("delete", "/never", ""))
        seqs.append(ops)
    assert pos <= len(data)
    return seqs, model


def write_filesets(seqs, st=None):
    st = st or PF.Storage(0, cp(SMALL), 10 ** 9, cp(LOOP_INDEX), store=pc.ChunkStore())
    infos, known = [], set()
    for ops in seqs:
        w = st.new_unordered_writer()
        for op in ops:
            (w.put if op[0] == "put" else w.delete)(*op[1:])
        got = w.close()
        assert len(got) == 1
        infos += got
        known |= {e[5] for fs in w.events for e in fs if e[0] == "chunk"}
        w.release()
    return st, infos, known


@pytest.fixture(scope="module")
def five():
    seqs, model = fileset_ops(7, 5)
    st, infos, known = write_filesets(seqs)
    return st, infos, known, seqs, model


def oracle_ref(d):
    return Ch.DataRef(ref=Ch.Ref(size_bytes=d.ref.size_bytes, edge=d.ref.edge, id=d.ref.id,
                                 dek=d.ref.dek), hash=d.hash, offset_bytes=d.offset_bytes,
                      size_bytes=d.size_bytes)


def oracle_inputs(st, infos):
    """[(deletive, additive)] as compact_oracle takes them, and the dict store of their chunks."""
    c = Chunker(ChunkParams(), 0)
    out, ostore = [], {}
    try:
        for info in infos:
            pair = []
            for root in (info.deletive, info.additive):
                xs = PF.index_read(c, st.store, root).files()
                pair.append([(f.path.encode(), f.tag.encode(), [oracle_ref(d) for d in f.data_refs])
                             for f in xs])
                for f in xs:
                    for d in f.data_refs:
                        ostore[d.ref.id] = st.store.get(d.ref.id)
            out.append(tuple(pair))
    finally:
        c.close()
    return out, ostore


def model_tar(model, keep=lambda p: True):
    return T.stream([(p, model[p]) for p in sorted(model) if keep(p)])


def model_of(seqs):
    model = {}
    for ops in seqs:
        for op in ops:
            if op[0] == "delete":
                model.pop(op[1], None)
            else:
                model[op[1]] = (model.get(op[1], b"") if op[3] else b"") + op[4]
    return model


# ------------------------------------------------------------------ against the oracle

@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_compact_equals_the_oracle(five, n):
    st, infos, known, seqs, _ = five
    infos = infos[:n]
    inputs, ostore = oracle_inputs(st, infos)
    want, log = CO.compact(inputs, SMALL, LOOP_INDEX, ostore)
    before = len(st.store)
    w = st.new_writer()
    w.copy_filesets(infos)
    got = w.close()
    events = w.events
    w.release()
    assert (got.additive, got.deletive) == (want.additive, want.deletive)
    assert got.size_bytes == want.size_bytes
    assert (got.num_files, got.num_deletes) == (len(want.files), len(want.deletes))
    for which in (0, 1):
        assert [e[2] for e in events if e[0] == "index" and e[1] == which] == \
            [e[2] for e in log if e[0] == "index" and e[1] == which]
    data = [e[3:7] for e in events if e[0] == "chunk" and e[1] == -1]
    assert data == [e[3:7] for e in log if e[0] == "chunk" and e[1] == -1]
    # both Copy paths: whole chunks passed by reference (no new object), the rest re-rolled
    copied = {e[2] for e in data if e[3]}
    formed = {e[5] for e in events if e[0] == "chunk" and not e[6]}
    assert copied and copied <= known
    assert any(not e[3] for e in data)
    assert len(st.store) <= before + len(formed - known)
    if n == 1:  # the same files in the same order roll into the chunks they came from
        assert not formed - known
        assert (got.additive, got.deletive, got.size_bytes) == \
            (infos[0].additive, infos[0].deletive, infos[0].size_bytes)
    else:
        assert formed - known, "nothing was re-rolled into a new chunk"
    model = model_of(seqs[:n])
    assert st.open([got]).tar().read() == model_tar(model)


# ------------------------------------------------------------------ against the model

def test_compacted_fileset_reads_back_as_its_inputs(five):
    st, infos, _, _, model = five
    one = st.compact(infos)
    want = st.open(infos).tar().read()
    assert want == model_tar(model)
    assert st.open([one]).tar().read() == want
    assert one.size_bytes == sum(len(v) for v in model.values())
    assert one.num_files == len(model)


def test_a_delete_no_input_holds_survives(five):
    st, infos, _, _, model = five
    one = st.compact(infos)
    c = Chunker(ChunkParams(), 0)
    try:
        dele = [(f.path, f.tag) for f in PF.index_read(c, st.store, one.deletive).files()]
    finally:
        c.close()
    assert ("/never", "default") in dele and dele == sorted(dele)
    _, old, _ = write_filesets([[("put", "/never", "", False, b"old"),
                                 ("put", "/zz-other", "", False, b"stays")]], st)
    merged = dict(model)
    merged["/zz-other"] = b"stays"
    assert st.open(old + [one]).tar().read() == model_tar(merged)
    assert st.open(old).tar().read() == model_tar({"/never": b"old", "/zz-other": b"stays"})


def test_a_path_range_compacts_only_its_range(five):
    st, infos, _, _, model = five
    lo, hi = "/a/f03", "/b/g02"
    part = st.compact(infos, lower=lo, upper=hi)
    assert st.open([part]).tar().read() == model_tar(model, lambda p: lo <= p <= hi)
    part = st.compact(infos, prefix="/b/")
    assert st.open([part]).tar().read() == model_tar(model, lambda p: p.startswith("/b/"))


def test_sharded_compact(five):
    """shardedCompact (compaction.go:124-143): shard, compact each range, concat."""
    st, infos, _, _, model = five
    ranges = st.shard(infos, threshold=40_000)
    assert len(ranges) >= 3 and ranges[0][0] == "" and ranges[-1][1] == ""
    parts = [st.compact(infos, lower=lo or None, upper=up or None) for lo, up in ranges]
    assert all(p.num_files for p in parts)
    whole = st.concat(parts)
    assert st.open([whole]).tar().read() == st.open([st.compact(infos)]).tar().read()
    assert whole.size_bytes == sum(len(v) for v in model.values())
    with pytest.raises(_lib.PfsCdcError) as e:  # out of order: checkPath refuses the second
        st.concat(parts[::-1])
    assert e.value.code == _lib.PFSCDC_EINVAL


def test_both_merge_arms_give_the_same_roots(five, knob):
    st, infos, _, _, _ = five
    out = []
    for arm in (0, 1):
        knob("PFSCDC_INDEX_MERGE", arm)
        out.append(st.compact(infos))
    assert out[0] == out[1]


# ------------------------------------------------------------------ errors

def first_file(st, info):
    c = Chunker(ChunkParams(), 0)
    try:
        return PF.index_read(c, st.store, info.additive).files()[0]
    finally:
        c.close()


def test_check_path_errors_are_sticky(five):
    st = five[0]
    for second in ("/a", "/b"):  # below the path before; the same (path, tag) twice
        w = st.new_writer()
        w.copy("/b", "t", [])
        with pytest.raises(_lib.PfsCdcError) as e:
            w.copy(second, "t", [])
        assert e.value.code == _lib.PFSCDC_EINVAL and second in str(e.value)
        for again in (lambda: w.delete("/z", ""), lambda: w.copy("/z", "t", []), w.close):
            with pytest.raises(_lib.PfsCdcError) as e2:
                again()
            assert e2.value.code == _lib.PFSCDC_EINVAL and second in str(e2.value)
        w.release()
    w = st.new_writer()
    w.copy("/b", "t", [])
    w.copy("/b", "u", [])  # another tag of the same path
    w.delete("/a", "")  # Deletes are checked against Deletes only
    with pytest.raises(_lib.PfsCdcError):
        w.delete("/a", "")
    w.release()


def test_missing_and_tampered_chunks(five):
    st, infos = five[0], five[1]
    f = first_file(st, infos[0])
    d = f.data_refs[0]
    assert d.ref.edge  # the fileset's first chunk: Copy reads it back and rolls it again
    empty = PF.Storage(0, cp(SMALL), 10 ** 9, cp(LOOP_INDEX), store=pc.ChunkStore())
    w = empty.new_writer()
    with pytest.raises(_lib.PfsCdcError) as e:
        w.copy(f.path, f.tag, f.data_refs)
        w.close()
    assert e.value.code == _lib.PFSCDC_ENOTFOUND
    w.release()
    ct = bytearray(st.store.get(d.ref.id))
    ct[len(ct) // 2] ^= 1
    empty.store.put(d.ref.id, bytes(ct))
    w = empty.new_writer()
    with pytest.raises(_lib.PfsCdcError) as e:
        w.copy(f.path, f.tag, f.data_refs[:1])
        w.close()
    assert e.value.code == _lib.PFSCDC_ECORRUPT
    with pytest.raises(_lib.PfsCdcError) as e:
        w.delete("/zz", "")
    assert e.value.code == _lib.PFSCDC_ECORRUPT  # sticky
    w.release()


def test_create_needs_a_store_and_ref_ids():
    lib = _lib.load()
    w = C.c_void_p()
    c = Chunker(cp(SMALL), 0, ref_ids=True)
    plain = Chunker(cp(SMALL), 0)
    store = pc.ChunkStore()
    try:
        assert lib.pfscdc_fsw_create(c.ctx, None, None, _lib.UW_CB(), None, C.byref(w)) == \
            _lib.PFSCDC_EINVAL
        assert lib.pfscdc_fsw_create(plain.ctx, None, store._s, _lib.UW_CB(), None, C.byref(w)) == \
            _lib.PFSCDC_EINVAL
        assert lib.pfscdc_fsw_create(c.ctx, None, store._s, _lib.UW_CB(), None, C.byref(w)) == 0
        info = _lib.FilesetInfo()
        assert lib.pfscdc_fsw_fileset(w, C.byref(info)) == _lib.PFSCDC_EINVAL  # not closed
        assert lib.pfscdc_fsw_close(w) == 0 and lib.pfscdc_fsw_fileset(w, C.byref(info)) == 0
        assert (info.additive_root, info.deletive_root, info.size_bytes) == (None, None, 0)
        assert lib.pfscdc_fsw_destroy(w) == 0
    finally:
        c.close()
        plain.close()
    with pytest.raises(ValueError):
        PF.Storage(0, cp(SMALL)).new_writer()


# ------------------------------------------------------------------ a plain C process

def test_plain_c_process_compacts(tmp_path):
    exe = str(tmp_path / "compact_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "compact_consumer.c"),
                    "-L", libdir, "-lpfscdc", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    out = str(tmp_path / "out.tar")
    res = subprocess.run([exe, out], capture_output=True, text=True, timeout=100)
    assert res.returncode == 0, res.stdout + res.stderr
    model = {"/f%02d" % k: bytes((k + j) & 0xFF for j in range(k * 997 + 13)) for k in range(24)}
    del model["/f03"]
    model["/f05"] = b"again"
    assert open(out, "rb").read() == T.stream([(p, model[p]) for p in sorted(model)])
    assert res.stdout.split()[:2] == ["ok", str(len(model))]
