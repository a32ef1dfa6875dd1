"""CopyFile on the GPU.  The selection and path transform: pfscdc_dev_list_copy_map against its
specification pfscdc_copy_map_host, array for array (entries, blob, DataRefs), both arms, with the
stats saying which arm ran.  UnorderedWriter.copy / copy_file end to end against the restated
oracle (tests/copy_oracle.py: roots, SizeBytes, level-0 index frames and chunk events, chunks
passed by reference included) and against a dict model through the read path, the error paths,
and a plain C99 process.  Every comparison is exact.

The cmap kernels use the tiles of the index kernels (256 lanes per workgroup, 1,024 per scan
pass) and no other, so the entry counts are those sizes and their neighbours."""
import ctypes as C
import os
import random
import subprocess

import pytest

import copy_cases as CC
import copy_oracle as CPO
import source_cases as SC
import tar_oracle as T
from test_gpu_compact import oracle_ref
from test_gpu_index_read import LOOP_INDEX, SMALL, cp

from oracle import fileset as OF
from pfs_amd import _lib
from pfs_amd import chunk as pc
from pfs_amd import fileset as pf
from pfs_amd.cdc import ChunkParams, Chunker, synthetic_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def chunker():
    c = Chunker(ChunkParams(), 0)
    yield c
    c.close()


def both(chunker, knob, lst, src, dst, tag="", arm=1):
    """copy_map over the uploaded ``lst`` with the knob at 1 and at 0: each arm's downloaded
    arrays equal pfscdc_copy_map_host's, the stats name the arm.  ``arm``: what the knob at 1
    runs.  Returns the host result's rows."""
    want = pf.copy_map_host(lst, src, dst, tag)
    wa = CC.arrays(want)
    dev_in = pf.DevIndexList.upload(chunker, lst)
    try:
        for value in (1, 0):
            knob("PFSCDC_COPY_MAP", value)
            for resident in (True, False):
                got = pf.copy_map(chunker, dev_in if resident else lst, src, dst, tag)
                st = pf.last_copy_map_stats(chunker)
                assert st["device"] == (arm if value else 0), st
                assert st["entries_in"] == (len(lst) if lst is not None else 0)
                assert (st["entries_out"], st["datarefs_out"], st["blob_bytes_out"]) == \
                    (len(want), len(wa[2]) // C.sizeof(_lib.FullDataRef), len(wa[1]))
                assert (len(got), got.num_datarefs, got.blob_len) == \
                    (st["entries_out"], st["datarefs_out"], st["blob_bytes_out"])
                ga = CC.arrays(got.download(chunker))
                got.free()
                assert ga[0] == wa[0], "entries"
                assert ga[1] == wa[1], "blob"
                assert ga[2] == wa[2], "DataRefs"
    finally:
        dev_in.free()
    return CC.rows(want)


# ------------------------------------------------------------------ the selection and transform

@pytest.mark.parametrize("name", sorted(CC.table()))
def test_case_table(chunker, knob, name):
    """The table of tests/test_copy_cpu.py; a list out of order or a selected path that is not
    clean reports the host arm and still matches."""
    spec, src, dst, tag, clean = CC.table()[name]
    lst, _ = CC.build(spec, sum(map(ord, name)))
    rows = both(chunker, knob, lst, src, dst, tag, arm=1 if clean else 0)
    assert rows == CC.want_rows(lst, src, dst, tag)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_entry_counts(chunker, knob, n):
    lst, _ = CC.build(CC.every_second(n), n)
    rows = both(chunker, knob, lst if n else None, "/s", "/moved/here")
    assert len(rows) == (n + 1) // 2
    assert [r[0] for r in rows] == ["/moved/here/f%05d" % i for i in range(0, n, 2)]


@pytest.mark.parametrize("n", [600, 2049])
def test_one_workgroup_makes_every_pass(chunker, knob, n):
    """PFSCDC_CHACHA_GRID=1 caps the count, fill and DataRef copy at one workgroup, which then
    strides over the whole list."""
    knob("PFSCDC_CHACHA_GRID", 1)
    lst, _ = CC.build(CC.every_second(n), n)
    rows = both(chunker, knob, lst, "/s", "/")
    assert [r[0] for r in rows] == ["/f%05d" % i for i in range(0, n, 2)]


def test_nothing_and_everything_selected(chunker, knob):
    spec = SC.by_key([("/s/d%d/f%04d" % (i % 3, i), "t", i % 4) for i in range(700)])
    lst, _ = CC.build(spec, 5)
    assert both(chunker, knob, lst, "/t", "/z") == []
    assert both(chunker, knob, lst, "/s/d1/f0001/x", "/z") == []
    assert both(chunker, knob, lst, "/", "/z") == []  # the root selects nothing: test_copy_cpu.py
    rows = both(chunker, knob, lst, "/s", "/s2/deeper")
    assert [r[0] for r in rows] == ["/s2/deeper" + p[2:] for p, _, _ in spec]
    assert sum(len(r[4]) for r in rows) == sum(i % 4 for i in range(700))


def test_long_paths_that_differ_in_the_last_byte(chunker, knob):
    """300-byte paths equal to srcPath + "/" but for the last byte, on both sides of '/' in byte
    order: none is selected; srcPath itself and a path below it are."""
    s = "/p/" + "q" * 296  # 299 bytes
    spec = SC.by_key([(s + c, "t", 1) for c in "!.0Z"] + [(s, "t", 2), (s + "/k", "t", 1),
                                                            (s[:-1] + "r", "t", 1)])
    assert sum(len(p) == 300 for p, _, _ in spec) == 4
    lst, _ = CC.build(spec, 7)
    rows = both(chunker, knob, lst, s, "/z")
    assert [r[0] for r in rows] == ["/z", "/z/k"]
    rows = both(chunker, knob, lst, s + "/", "/" + "y" * 299)  # cleaned to s
    assert [len(r[0]) for r in rows] == [300, 302]


def test_an_unordered_list_takes_the_host_arm(chunker, knob):
    spec = CC.every_second(300)
    spec[100], spec[200] = spec[200], spec[100]
    lst, _ = CC.build(spec, 9)
    both(chunker, knob, lst, "/s", "/z", arm=0)
    # the tags of one path out of order
    lst, _ = CC.build([("/s/a", "u", 1), ("/s/a", "t", 1), ("/s/b", "t", 1)], 9)
    rows = both(chunker, knob, lst, "/s", "/z", arm=0)
    assert [(r[0], r[1]) for r in rows] == [("/z/a", "u"), ("/z/a", "t"), ("/z/b", "t")]


@pytest.mark.parametrize("which", ["path_off", "first_count"])
def test_a_malformed_entry_is_refused_by_both_arms(chunker, knob, which):
    """path_off past the blob, first + count past the DataRefs: PFSCDC_EINVAL from both arms.  The
    count kernel checks an entry's bounds before it reads a byte of the blob."""
    lst, _ = CC.build(CC.every_second(600), 3)
    n, ents, blob, _, ndr = lst._views()
    if which == "path_off":
        ents[301].path_off = len(blob) + (1 << 40)
    else:
        ents[301].first = ndr - 1
        ents[301].count = 2
    out = C.c_void_p(0xDEAD)
    for value in (1, 0):
        knob("PFSCDC_COPY_MAP", value)
        for src in (b"/s", b"/nothing"):
            out = C.c_void_p(0xDEAD)
            rc = chunker.lib.pfscdc_copy_map_list(chunker.ctx, lst._p, src, None, b"/z", C.byref(out))
            assert rc == _lib.PFSCDC_EINVAL and not out.value
            assert b"outside the list" in chunker.lib.pfscdc_last_error(chunker.ctx)


def test_a_range_entry_is_refused_by_both_arms(chunker, knob):
    rng = random.Random(9)
    ref = SC.dr(rng).ref
    lst = pf.index_decode_host(OF.frame(OF.encode_index(OF.Index("/a", None, [], (0, "/b", ref)))))
    for value in (1, 0):
        knob("PFSCDC_COPY_MAP", value)
        with pytest.raises(_lib.PfsCdcError) as ei:
            pf.copy_map(chunker, lst, "/a", "/z")
        assert ei.value.code == _lib.PFSCDC_EINVAL and "Range" in str(ei.value)


def test_the_mapped_list_goes_through_the_tar_layout(chunker, knob):
    knob("PFSCDC_COPY_MAP", 1)
    lst, _ = CC.build(CC.every_second(600), 4)
    got = pf.copy_map(chunker, lst, "/s", "/z")
    assert pf.last_copy_map_stats(chunker)["device"] == 1
    n = len(got)
    assert n == 300
    total, offs = C.c_uint64(), (C.c_uint64 * (n + 1))()
    rc = chunker.lib.pfscdc_dev_list_tar_layout(chunker.ctx, got._p, C.byref(total), offs)
    assert rc == _lib.PFSCDC_OK, chunker.lib.pfscdc_last_error(chunker.ctx)
    assert offs[0] == 0 and all(offs[k] + 512 <= offs[k + 1] for k in range(n))
    assert total.value >= offs[n]
    got.free()


def test_null_arguments(chunker, knob):
    lib = chunker.lib
    out = C.c_void_p(0xDEAD)
    lst, _ = CC.build(CC.every_second(4), 4)
    dev = pf.DevIndexList.upload(chunker, lst)
    assert lib.pfscdc_dev_list_copy_map(None, dev._p, b"/s", None, b"/z", C.byref(out)) == _lib.PFSCDC_EINVAL
    assert lib.pfscdc_dev_list_copy_map(chunker.ctx, None, b"/s", None, b"/z", C.byref(out)) == _lib.PFSCDC_EINVAL
    assert lib.pfscdc_dev_list_copy_map(chunker.ctx, dev._p, b"/s", None, b"/z", None) == _lib.PFSCDC_EINVAL
    assert lib.pfscdc_last_copy_map_stats(chunker.ctx, None) == _lib.PFSCDC_EINVAL
    for value in (1, 0):  # NULL paths are the root
        knob("PFSCDC_COPY_MAP", value)
        assert lib.pfscdc_dev_list_copy_map(chunker.ctx, dev._p, None, None, None, C.byref(out)) == 0
        assert lib.pfscdc_dev_list_count(out) == 0
        lib.pfscdc_dev_list_free(out)
    dev.free()


# ------------------------------------------------------------------ end to end

A_NAMES = ["/a/f%02d" % k for k in range(10)] + ["/a.txt"] + ["/b/g%02d" % k for k in range(4)] + ["/top"]


def commit_a(threshold):
    """Commit A in a ChunkStore of its own: /a/f00..f09 (two of 40,000 bytes, which span whole
    chunks), /a.txt, /b/g* and /top."""
    data = synthetic_bytes([0, 210_000], 21).tobytes()
    rng = random.Random(22)
    model, pos = {}, 0
    for k, p in enumerate(A_NAMES):
        size = 40_000 if p in ("/a/f02", "/a/f07") else rng.choice([1, 700, 3000, 9000])
        model[p] = data[pos:pos + size]
        pos += size
    assert pos <= len(data)
    st = pf.Storage(0, cp(SMALL), threshold, cp(LOOP_INDEX), store=pc.ChunkStore())
    w = st.new_unordered_writer()
    for p in A_NAMES:
        w.put(p, "", False, model[p])
    infos = w.close()
    w.release()
    return st, infos, model


def oracle_files(st, infos, src, dst, tag=""):
    """What copyFile hands to UnorderedWriter.Copy, for the oracle: [(new path, [DataRef])] from
    the opened commit, and the dict store of the chunks they lie in."""
    fs = st.open(infos)
    files = fs.files()
    ostore = {}
    for f in files:
        for d in f.data_refs:
            ostore[d.ref.id] = st.store.get(d.ref.id)
    picks = CPO.copy_map([(f.path, f.tag) for f in files], src, dst, tag)
    return [(np, [oracle_ref(d) for d in files[i].data_refs]) for i, np in picks], ostore


def run_w(st, infos, threshold, with_delete, through_fileset):
    """The writer W of the issue on the GPU and on the oracle; returns both."""
    extra = synthetic_bytes([0, 30_000], 23).tobytes()
    w = st.new_unordered_writer()
    store = {}
    ow = CPO.CopyUnorderedWriter(SMALL, threshold, LOOP_INDEX, store)
    src = st.open(infos, resident=True) if through_fileset else infos

    def put(p, append, body):
        w.put(p, "", append, body)
        ow.put(p, "", append, body)

    def copy_file(s, d, append=False):
        w.copy_file(src, s, d, append=append)
        files, chunks = oracle_files(st, infos, s, d)
        store.update(chunks)
        ow.copy(files, "", append)

    put("/early", False, extra[:5000])
    copy_file("/a", "/z")
    put("/z/f03", True, extra[5000:9000])
    copy_file("/top", "/b/g00", append=True)
    if with_delete:
        w.delete("/z/")
        ow.delete("/z/")
    return w, w.close(), ow, ow.close()


@pytest.mark.parametrize("through_fileset", [False, True])
@pytest.mark.parametrize("with_delete", [False, True])
@pytest.mark.parametrize("threshold", [10 ** 9, 12_000])
def test_copy_file_into_a_commit(knob, threshold, with_delete, through_fileset):
    knob("PFSCDC_COPY_MAP", 1)
    st, infos, model = commit_a(threshold)
    assert (len(infos) > 1) == (threshold != 10 ** 9)
    w, got, ow, want = run_w(st, infos, threshold, with_delete, through_fileset)
    # the oracle's log holds chunks passed by reference, or the test would show nothing of them
    olog = [(k,) + e for k, log in enumerate(ow.log) for e in log]
    assert any(e[1] == "chunk" and e[2] == -1 and e[7] for e in olog if len(e) == 8)
    assert len(got) == len(want) >= 3
    for g, o in zip(got, want):
        assert (g.additive, g.deletive, g.size_bytes) == (o.additive, o.deletive, o.size_bytes)
        assert (g.num_files, g.num_deletes) == (len(o.files), len(o.deletes))
    glog = [e + (c,) for e, c in zip(w.log, w.log_copied)]
    for which in (0, 1):
        assert [(e[0], e[3]) for e in glog if e[1] == "index" and e[2] == which] == \
            [(e[0], e[3]) for e in olog if e[1] == "index" and e[2] == which]
    # data-chunk events: (fileset, size, edge, Ref.Id, copied)
    assert [(e[0],) + e[4:8] for e in glog if e[1] == "chunk" and e[2] == -1] == \
        [(e[0],) + e[4:7] + (e[7] if len(e) == 8 else False,)
         for e in olog if e[1] == "chunk" and e[2] == -1]
    assert any(e[7] for e in glog if e[1] == "chunk")
    w.release()
    # through the read path, against the dict model
    new = dict(model)
    extra = synthetic_bytes([0, 30_000], 23).tobytes()
    new["/early"] = extra[:5000]
    for p in A_NAMES:
        if p.startswith("/a/"):
            new["/z" + p[2:]] = model[p]
    new["/z/f03"] += extra[5000:9000]
    new["/b/g00"] = model["/b/g00"] + model["/top"]
    if with_delete:
        new = {p: v for p, v in new.items() if not p.startswith("/z/")}
    fs = st.open(infos + got, resident=True)
    assert fs.get_file("/b/g00").read() == T.stream([("/b/g00", new["/b/g00"])])
    if with_delete:
        with pytest.raises(KeyError):
            fs.get_file("/z")
        assert not [f for f in fs.files() if f.path.startswith("/z")]
    else:
        want_z = [("/z/", b"")] + [(p, new[p]) for p in sorted(new) if p.startswith("/z/")]
        assert fs.get_file("/z").read() == T.stream(want_z)
    assert st.open(infos + got).tar().read() == T.stream([(p, new[p]) for p in sorted(new)])


def test_both_arms_copy_the_same(knob):
    st, infos, _ = commit_a(10 ** 9)
    out = []
    for arm in (1, 0):
        knob("PFSCDC_COPY_MAP", arm)
        w = st.new_unordered_writer()
        w.copy_file(infos, "/a", "/z")
        out.append((w.close(), [e for e in w.log], list(w.log_copied)))
        w.release()
    assert out[0] == out[1] and out[0][0][0].num_files == 10


def test_an_empty_copy_still_makes_a_fileset(knob):
    st, infos, _ = commit_a(10 ** 9)
    w = st.new_unordered_writer()
    w.put("/x", "", False, b"abc")
    w.copy_file(infos, "/nothing", "/z")
    w.copy_file([], "/a", "/z")  # no filesets: an empty list
    w.copy(None)
    got = w.close()
    w.release()
    assert [(g.additive is None, g.deletive is None, g.num_files) for g in got] == \
        [(False, False, 1), (True, True, 0), (True, True, 0), (True, True, 0)]


@pytest.mark.parametrize("workers", [1, 2])
def test_copy_events_follow_earlier_filesets(knob, workers):
    """Filesets are numbered in order and their events arrive in that order, with any number of
    group writers: the copy waits for every group before it."""
    knob("PFSCDC_UW_WORKERS", workers)
    knob("PFSCDC_UW_INFLIGHT", 0)  # every serialized buffer is a group of its own
    st, infos, _ = commit_a(10 ** 9)
    st2 = pf.Storage(0, cp(SMALL), 6_000, cp(LOOP_INDEX), store=st.store)
    body = synthetic_bytes([0, 40_000], 31).tobytes()
    w = st2.new_unordered_writer()
    for k in range(5):
        w.put("/p%d" % k, "", False, body[k * 5000:k * 5000 + 5000])
    w.copy_file(infos, "/b", "/c")
    for k in range(3):
        w.put("/q%d" % k, "", False, body[k * 5000:k * 5000 + 5000])
    got = w.close()
    order = [e[0] for e in w.log]
    w.release()
    assert order == sorted(order) and len(set(order)) == len(got) >= 6
    copies = [k for k, g in enumerate(got) if g.num_files == 4 and g.num_deletes == 4]
    assert len(copies) == 1
    model_c = st.open(infos).files()
    fs = st2.open(got)
    assert [f.path for f in fs.files() if f.path.startswith("/c/")] == \
        ["/c" + f.path[2:] for f in model_c if f.path.startswith("/b/")]


# ------------------------------------------------------------------ errors

def test_copy_needs_a_store():
    st = pf.Storage(0, cp(SMALL), 10 ** 9, cp(LOOP_INDEX))
    w = st.new_unordered_writer()
    lst, _ = CC.build([("/a", "t", 0)])
    with pytest.raises(_lib.PfsCdcError) as e:
        w.copy(lst)
    assert e.value.code == _lib.PFSCDC_ESTATE
    with pytest.raises(_lib.PfsCdcError) as e:  # sticky
        w.put("/x", "", False, b"abc")
    assert e.value.code == _lib.PFSCDC_ESTATE
    w.release()
    w = st.new_unordered_writer()
    with pytest.raises(_lib.PfsCdcError) as e:
        w.copy_file([], "/a", "/z")
    assert e.value.code == _lib.PFSCDC_ESTATE
    w.release()


def test_copy_after_close():
    st, infos, _ = commit_a(10 ** 9)
    w = st.new_unordered_writer()
    w.close()
    for call in (lambda: w.copy(None), lambda: w.copy_file(infos, "/a", "/z")):
        with pytest.raises(_lib.PfsCdcError) as e:
            call()
        assert e.value.code == _lib.PFSCDC_ESTATE
    w.release()


def test_two_source_tags_of_one_path_collapse():
    """checkPath: both tags of /d/f come to (/z/f, "default"): the second Delete names it."""
    st = pf.Storage(0, cp(SMALL), 10 ** 9, cp(LOOP_INDEX), store=pc.ChunkStore())
    a = st.new_unordered_writer()
    a.put("/d/e", "x", False, b"e" * 100)
    a.put("/d/f", "x", False, b"x" * 100)
    a.put("/d/f", "y", False, b"y" * 100)
    infos = a.close()
    a.release()
    w = st.new_unordered_writer()
    w.copy_file(infos, "/d", "/z", tag="one", src_tag="x")  # one tag of each: fine
    with pytest.raises(_lib.PfsCdcError) as e:
        w.copy_file(infos, "/d", "/z", tag="one")
    assert e.value.code == _lib.PFSCDC_EINVAL and "/z/f" in str(e.value)
    with pytest.raises(_lib.PfsCdcError) as e:  # sticky
        w.close()
    assert e.value.code == _lib.PFSCDC_EINVAL and "/z/f" in str(e.value)
    w.release()
    # appended, they do not collide in the Deletes but still in the Copies
    w = st.new_unordered_writer()
    with pytest.raises(_lib.PfsCdcError) as e:
        w.copy_file(infos, "/d", "/z", append=True)
    assert e.value.code == _lib.PFSCDC_EINVAL and "/z/f" in str(e.value)
    w.release()


def test_a_mapped_list_out_of_order_is_refused():
    st = pf.Storage(0, cp(SMALL), 10 ** 9, cp(LOOP_INDEX), store=pc.ChunkStore())
    lst, _ = CC.build([("/b", "t", 0), ("/a", "t", 0)])
    w = st.new_unordered_writer()
    with pytest.raises(_lib.PfsCdcError) as e:
        w.copy(lst)
    assert e.value.code == _lib.PFSCDC_EINVAL and "/a" in str(e.value)
    w.release()


def test_a_chunk_missing_from_the_store():
    """The copied file's first chunk is an edge chunk, which Copy reads back and rolls again."""
    st, infos, _ = commit_a(10 ** 9)
    files = st.open(infos).files()
    assert files[0].data_refs[0].ref.edge
    # the index chunks only: the data chunks of /a are not in this store
    other = pc.ChunkStore()
    c = Chunker(ChunkParams(), 0)
    try:
        lst = pf.index_read(c, st.store, infos[0].additive)
    finally:
        c.close()
    st2 = pf.Storage(0, cp(SMALL), 10 ** 9, cp(LOOP_INDEX), store=other)
    w = st2.new_unordered_writer()
    with pytest.raises(_lib.PfsCdcError) as e:
        w.copy(pf.copy_map_host(lst, "/a", "/z"))
    assert e.value.code == _lib.PFSCDC_ENOTFOUND
    with pytest.raises(_lib.PfsCdcError) as e:  # sticky
        w.close()
    assert e.value.code == _lib.PFSCDC_ENOTFOUND
    w.release()


# ------------------------------------------------------------------ a plain C process

def test_plain_c_process_copies_a_directory(tmp_path):
    exe = str(tmp_path / "copy_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "copy_consumer.c"),
                    "-L", libdir, "-lpfscdc", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    out = str(tmp_path / "out.tar")
    res = subprocess.run([exe, out], capture_output=True, text=True, timeout=100)
    assert res.returncode == 0, res.stdout + res.stderr
    model = {"/d/f%02d" % k: bytes((k + j) & 0xFF for j in range(k * 997 + 13)) for k in range(24)}
    model["/other"] = b"other"
    for k in range(24):
        model["/moved/to/f%02d" % k] = model["/d/f%02d" % k]
    model["/moved/to/f05"] += b"appended"
    assert open(out, "rb").read() == T.stream([(p, model[p]) for p in sorted(model)])
    assert res.stdout.split()[:3] == ["ok", str(len(model)), "24"]
