"""Index lists that stay on the GPU: pfscdc_dev_list (upload / download), pfscdc_index_read_dev,
pfscdc_index_merge_dev and GetFileTAR over a resident list (pfscdc_dev_list_tar_layout,
pfscdc_dev_list_read_tar).  Every comparison is exact: the resident calls against the host calls
they stand in for (pfscdc_index_read, pfscdc_index_merge[_deletive], pfscdc_store_read_tar over
the downloaded list), array for array and byte for byte, and the tar bytes also against
tests/tar_oracle.py."""
import ctypes as C
import os
import random
import subprocess

import pytest

import tar_oracle as T
from oracle import chunker as Ch
from oracle import fileset as OF
from pfs_amd import _lib
from pfs_amd import chunk as pc
from pfs_amd import fileset as pf
from pfs_amd.cdc import ChunkParams, Chunker
from stored_chunks import Stored
from test_gpu_index_read import LOOP_INDEX, model_ops, wide, write  # noqa: F401 (wide: a fixture)
from test_gpu_merge import arrays, build, key_pool, lst_of
from test_index_read_cpu import _dr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def chunker():
    c = Chunker(ChunkParams(), 0)
    yield c
    c.close()


def up(chunker, lst):
    return pf.DevIndexList.upload(chunker, lst)


def same(a, b):
    x, y = arrays(a), arrays(b)
    assert [len(v) for v in x] == [len(v) for v in y]
    assert x[0] == y[0], "entries"
    assert x[1] == y[1], "blob"
    assert x[2] == y[2], "DataRefs"


# ------------------------------------------------------------------ the handle

def test_upload_download_round_trip(chunker):
    rng = random.Random(1)
    shapes = [[], [OF.Index("/one", "default", [_dr(rng)])],
              [OF.Index("/a", "t", []), OF.Index("/b", "t", [_dr(rng) for _ in range(300)]),
               OF.Index("/c", "", []), OF.Index("/d", "t", [_dr(rng)]),
               OF.Index("/e", "t", [], (5, "/e-last", _dr(rng).ref))]]
    for entries in shapes:
        lst = lst_of(entries)
        dev = up(chunker, lst)
        n, _, blob, _, ndr = lst._views()
        assert (len(dev), dev.num_datarefs, dev.blob_len) == (n, ndr, len(blob))
        same(dev.download(chunker), lst)
        same(dev.download(), lst)  # (a context of its own: the handle is bound to the device)
        dev.free()
    dev = up(chunker, None)  # NULL: an empty list
    assert len(dev) == 0 and len(dev.download(chunker)) == 0
    lib, out = chunker.lib, C.c_void_p()
    assert lib.pfscdc_dev_list_upload(None, None, C.byref(out)) == _lib.PFSCDC_EINVAL
    assert lib.pfscdc_dev_list_download(chunker.ctx, None, C.byref(out)) == _lib.PFSCDC_EINVAL
    assert lib.pfscdc_dev_list_free(None) == _lib.PFSCDC_OK


# ------------------------------------------------------------------ read

@pytest.mark.parametrize("decode", [1, 0])
def test_read_dev_equals_read(wide, chunker, knob, decode):
    """The 300-file, multi-level index: unfiltered the level-0 list stays where the decode wrote
    it (no upload, no list copy); a filter that names a part, or the host decode, is the host
    path and an upload."""
    st, infos, _ = wide
    root = infos[0].additive
    want = pf.index_read(chunker, st.store, root)
    levels = pf.last_index_stats(chunker)["levels"]
    assert len(want) == 300 and levels >= 3
    knob("PFSCDC_INDEX_DECODE", decode)
    dev = pf.index_read_dev(chunker, st.store, root)
    rs, ist = pf.last_resident_stats(chunker), pf.last_index_stats(chunker)
    same(dev.download(chunker), want)
    assert (len(dev), ist["levels"]) == (300, levels)
    if decode:
        assert rs["read_resident"] == 1 and rs["read_uploaded_bytes"] == 0
    else:
        n, _, blob, _, ndr = want._views()
        assert rs["read_resident"] == 0
        assert rs["read_uploaded_bytes"] == 64 * n + 128 * ndr + len(blob)
    paths = sorted({g["path"].decode() for g in want.raw()})
    for form in (dict(lower=paths[40], upper=paths[200]), dict(prefix="/d3/"), dict(tag="t1"),
                 dict(prefix="/nothing")):
        host = pf.index_read(chunker, st.store, root, **form)
        got = pf.index_read_dev(chunker, st.store, root, **form)
        rs = pf.last_resident_stats(chunker)
        assert rs["read_resident"] == 0 and (rs["read_uploaded_bytes"] > 0) == (len(host) > 0)
        assert 0 <= len(host) < 300
        same(got.download(chunker), host)


@pytest.mark.parametrize("decode", [1, 0])
def test_read_dev_empty_root_and_level0_root(chunker, knob, decode):
    knob("PFSCDC_INDEX_DECODE", decode)
    store = pc.ChunkStore()
    for root in (None, b""):
        dev = pf.index_read_dev(chunker, store, root)
        assert len(dev) == 0 and pf.last_resident_stats(chunker)["read_resident"] == 0
        assert len(dev.download(chunker)) == 0
    one = OF.encode_index(OF.Index("/only", "default", []))
    dev = pf.index_read_dev(chunker, store, one)
    rs = pf.last_resident_stats(chunker)
    assert rs["read_resident"] == 0 and rs["read_uploaded_bytes"] > 0  # uploaded
    same(dev.download(chunker), pf.index_read(chunker, store, one))
    assert len(pf.index_read_dev(chunker, store, one, prefix="/x")) == 0


# ------------------------------------------------------------------ merge

def merge_both(chunker, pairs, device=1):
    """Both modes over resident copies of the pairs against the host specifications."""
    dev_pairs = [tuple(up(chunker, l) if l is not None else None for l in p) for p in pairs]
    out = None
    for deletive in (False, True):
        host = pf.index_merge(pairs, deletive=deletive)
        got = pf.index_merge_dev(dev_pairs, chunker, deletive=deletive)
        st = pf.last_merge_stats(chunker)
        n_in = sum(len(l) for p in pairs for l in (p[:1] if deletive else p) if l is not None)
        assert st["entries_in"] == n_in and st["entries_out"] == len(host) == len(got)
        if device is not None:
            assert st["device"] == device, st
        same(got.download(chunker), host)
        if not deletive:
            out = got
    return out


@pytest.mark.parametrize("grid", [1, 0])
def test_merge_dev_stream_lengths(chunker, knob, grid):
    """Ten streams of 0, 1, 63, 64, 65, 255, 256, 257, 1,025 and 100 entries.  The
    PFSCDC_INDEX_MERGE knob at 0 does not govern the resident call."""
    knob("PFSCDC_INDEX_MERGE", 0)
    knob("PFSCDC_CHACHA_GRID", grid)
    rng = random.Random(70 + grid)
    pool = key_pool(1200)
    assert len(pool) > 1500
    _, pairs, _ = build(rng, pool[:1500], [0, 1, 63, 64, 65, 255, 256, 257, 1025, 100])
    merge_both(chunker, pairs)


@pytest.mark.parametrize("nfilesets", [1, 2, 3, 10])
def test_merge_dev_fan_in(chunker, nfilesets):
    rng = random.Random(80 + nfilesets)
    _, pairs, _ = build(rng, key_pool(150), [rng.randrange(20, 90) for _ in range(2 * nfilesets)])
    merge_both(chunker, pairs)


def test_merge_dev_places_of_a_deletive_entry(chunker):
    rng = random.Random(5)
    A = lambda p, t="": OF.Index(p, t, [_dr(rng), _dr(rng)])  # noqa: E731
    D = lambda p, t="": OF.Index(p, t, [])  # noqa: E731
    sets = [
        ([D("/every"), D("/first"), D("/lone-del")],
         [A("/every"), A("/last"), A("/lone-add"), A("/mid"), A("/tags", ""), A("/tags", "t1")]),
        ([D("/every"), D("/mid"), D("/tags", "t1")],
         [A("/every"), A("/first"), A("/last"), A("/mid"), A("/tags", "t1"), A("/tags", "t2")]),
        ([D("/every"), D("/last")], [A("/every"), A("/first"), A("/tags", "")]),
    ]
    merged = merge_both(chunker, [(lst_of(d), lst_of(a)) for d, a in sets])
    paths = [g["path"] for g in merged.download(chunker).raw()]
    assert b"/last" not in paths and b"/lone-del" not in paths and b"/first" in paths


def test_merge_dev_out_of_order_and_nothing(chunker):
    rng = random.Random(9)
    good = lst_of([OF.Index("/f%02d" % i, "t", [_dr(rng)]) for i in range(70)])
    xs = [OF.Index("/f%02d" % i, "t", [_dr(rng)]) for i in range(0, 140, 2)]
    pairs = [(None, good), (None, lst_of(xs[:40] + [xs[39]] + xs[40:]))]
    dev_pairs = [(None, up(chunker, a)) for _, a in pairs]
    got = pf.index_merge_dev(dev_pairs, chunker)
    st = pf.last_merge_stats(chunker)
    assert st["device"] == 0 and st["entries_in"] == 70 + 71  # the host arm, and it says so
    same(got.download(chunker), pf.index_merge(pairs))
    # one fileset whose deletive list is empty; no fileset; NULL lists
    empty = up(chunker, lst_of([]))
    for pairs_, deletive in (([(empty, None)], True), ([(empty, empty)], False), ([], False),
                             ([(None, None)], True)):
        out = pf.index_merge_dev(pairs_, chunker, deletive=deletive)
        assert len(out) == 0 and pf.last_merge_stats(chunker)["device"] == 1
        assert len(out.download(chunker)) == 0
    out = C.c_void_p()
    lib = chunker.lib
    assert lib.pfscdc_index_merge_dev(chunker.ctx, 2, None, 0, C.byref(out)) == _lib.PFSCDC_EINVAL
    assert lib.pfscdc_index_merge_dev(chunker.ctx, 0, None, 1, C.byref(out)) == _lib.PFSCDC_EINVAL


# ------------------------------------------------------------------ tar

@pytest.fixture(scope="module")
def stored():
    st = Stored([3000, 70000, 12345, 41000], 201)
    store = pc.ChunkStore()
    for rid, ct in st.store.items():
        store.put(rid, ct)
    return st, store


def entries_of(st, named):
    """Index entries for (name, [(chunk, offset, size)]) and the files' contents."""
    out, contents = [], []
    for name, sl in named:
        out.append(OF.Index(name, "default",
                            [Ch.DataRef(st.orefs[c], bytes(32), o, z) for c, o, z in sl]))
        contents.append(b"".join(st.chunks[c][o:o + z] for c, o, z in sl))
    return out, contents


def host_tar(chunker, store, lst, begin, n, fill=None):
    """pfscdc_store_read_tar over a host list: (rc, bytes written or the whole buffer, error)."""
    cnt, _, _, drs, ndr = lst._views()
    tf = chunker.lib.pfscdc_index_list_tar_files(lst._p)
    buf = (C.c_uint8 * max(1, n))(*([0xA5] * max(1, n) if fill else []))
    nw = C.c_uint64()
    rc = chunker.lib.pfscdc_store_read_tar(chunker.ctx, store._s, tf, cnt, drs, ndr, begin, n, buf,
                                           n, 0, C.byref(nw))
    msg = chunker.lib.pfscdc_last_error(chunker.ctx).decode("utf-8", "replace") if rc else ""
    return rc, bytes(buf)[:n if fill else nw.value], msg


def dev_tar(chunker, store, dev, begin, n, fill=None):
    buf = (C.c_uint8 * max(1, n))(*([0xA5] * max(1, n) if fill else []))
    nw = C.c_uint64()
    rc = chunker.lib.pfscdc_dev_list_read_tar(chunker.ctx, store._s, dev._p, begin, n, buf, n, 0,
                                              C.byref(nw))
    msg = chunker.lib.pfscdc_last_error(chunker.ctx).decode("utf-8", "replace") if rc else ""
    return rc, bytes(buf)[:n if fill else nw.value], msg


def dev_layout(chunker, dev):
    offs, total = (C.c_uint64 * (len(dev) + 1))(), C.c_uint64()
    rc = chunker.lib.pfscdc_dev_list_tar_layout(chunker.ctx, dev._p, C.byref(total), offs)
    return rc, list(offs), total.value


def whole_stream(chunker, store, entries, contents):
    """The list rendered whole through both paths and by the oracle; layout against the host's."""
    lst = lst_of(entries)
    dev = up(chunker, lst)
    want = T.stream([(e.path, b) for e, b in zip(entries, contents)])
    rc, offs, total = dev_layout(chunker, dev)
    assert rc == 0
    cnt, ents, _, _, _ = lst._views()
    tf = chunker.lib.pfscdc_index_list_tar_files(lst._p)
    sizes = (C.c_uint64 * max(1, cnt))(*[ents[i].size_bytes for i in range(cnt)])
    hoffs, htotal = (C.c_uint64 * (cnt + 1))(), C.c_uint64()
    assert chunker.lib.pfscdc_tar_layout(tf, cnt, sizes, hoffs, C.byref(htotal)) == 0
    assert (offs, total) == (list(hoffs), htotal.value) and total == len(want)
    rc, host, msg = host_tar(chunker, store, dev.download(chunker), 0, total)
    assert rc == 0 and host == want, msg
    rc, got, msg = dev_tar(chunker, store, dev, 0, total)
    assert rc == 0, msg
    assert got == want
    # into a device tensor prefilled with 0xA5: every byte outside the stream stays
    import torch
    t = torch.full((total + 67,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    nw = C.c_uint64()
    rc = chunker.lib.pfscdc_dev_list_read_tar(chunker.ctx, store._s, dev._p, 0, total,
                                              t[3:].data_ptr(), total + 64, 1, C.byref(nw))
    host = t.cpu().numpy()
    assert rc == 0 and nw.value == total and host[3:3 + total].tobytes() == want
    assert (host[:3] == 0xA5).all() and (host[3 + total:] == 0xA5).all()
    return lst, dev, want


def tiny_files(st, n):
    """n files of 0-3 bytes from chunk 0 (and every tenth from chunk 2)."""
    return entries_of(st, [("/t/%05d" % i, [(2 if i % 10 == 9 else 0, i % 2900, i % 4)] if i % 4 else [])
                           for i in range(n)])


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 2049])
def test_tar_entry_counts_at_the_scans_tile_edges(chunker, stored, n):
    st, store = stored
    entries, contents = tiny_files(st, n)
    _, dev, want = whole_stream(chunker, store, entries, contents)
    total = len(want)
    for begin, length in ((total - 1024, 1024), (total, 512), ((total // 1024) * 512, 3 * 512),
                          (max(0, total - 4096), 10 ** 6)):
        rc, got, msg = dev_tar(chunker, store, dev, begin, min(length, total - begin + 512))
        assert rc == 0, msg
        assert got == want[begin:begin + length]
    assert pf.last_resident_stats(chunker)["plan_reused"] == 1


def mixed_named():
    """Sizes 0, 1, 511, 512, 513; a 300-DataRef file between one-DataRef files; zero-size
    DataRefs; a directory; names of 100, 101 (split) and 155 + 1 + 100 bytes."""
    n100 = "/n" + "a" * 98
    n101 = "/" + "d" * 50 + "/" + "f" * 49
    n256 = "/" + "p" * 154 + "/" + "s" * 100
    assert (len(n100), len(n101), len(n256)) == (100, 101, 256)
    return [("/0", []), ("/1", [(0, 2999, 1)]), ("/511", [(1, 69489, 511)]),
            ("/512", [(1, 3, 500), (3, 40988, 12)]), ("/513", [(3, 7, 513)]),
            ("/before", [(2, 5, 9)]),
            ("/big300", [(i % 4, 7 * i, 1 + i % 5) for i in range(300)]),
            ("/behind", [(2, 50, 3)]),
            ("/dir/", []),
            ("/zeros", [(0, 0, 0), (1, 10, 20), (2, 12345, 0), (1, 30, 0), (3, 0, 2), (0, 3000, 0)]),
            ("/only-zeros", [(1, 5, 0), (2, 5, 0)]),
            (n100, [(2, 101, 64)]), (n101, [(2, 101, 63)]), (n256, [(0, 1, 7)])]


def test_tar_list_shapes_every_window(chunker, stored):
    import torch
    st, store = stored
    entries, contents = entries_of(st, mixed_named())
    lst, dev, want = whole_stream(chunker, store, entries, contents)
    total = len(want)
    assert total < 40 * 512
    for begin in range(0, total + 1, 512):
        for length in (512, 1024, 4096, total):
            rc, got, msg = dev_tar(chunker, store, dev, begin, length)
            assert rc == 0, msg
            assert got == want[begin:begin + length], (begin, length)
    # into a device tensor prefilled with 0xA5: nothing outside the window changes
    t = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    ts = pf.FileSet(pc.Storage(device=0, store=store), None, dev).tar()
    for at, begin, length in ((3, 1536, 4096), (0, 0, total), (17, 512, 512)):
        t.fill_(0xA5)
        n = ts.read_into(t[at:], begin, length)
        host = t.cpu().numpy()
        assert n == min(length, total - begin)
        assert host[at:at + n].tobytes() == want[begin:begin + n]
        assert (host[:at] == 0xA5).all() and (host[at + n:] == 0xA5).all()
    assert ts.size() == total and ts.entry_offsets[-1] == total - 1024
    assert ts.read(1024) == want[1024:]
    # window errors as the host's
    for begin, length in ((100, 512), (total + 512, 512), (0, 700)):
        assert dev_tar(chunker, store, dev, begin, length)[::2] == \
            host_tar(chunker, store, lst, begin, length)[::2]


def test_tar_datarefs_at_every_keystream_phase(chunker, stored):
    st, store = stored
    entries, contents = entries_of(
        st, [("/phase/%02d" % k, [(1, 1000 + k, 70 + k), (3, 64 * k + k, 1 + k)]) for k in range(64)])
    whole_stream(chunker, store, entries, contents)


def test_tar_window_shapes(chunker, stored):
    """Windows that begin inside a file's content, end inside a DataRef, cover only a file's last
    byte and its padding, only the trailer, and nothing (begin == total)."""
    st, store = stored
    entries, contents = entries_of(st, [("/a", [(0, 1, 7)]),
                                        ("/big", [(1, 30001, 39999), (3, 0, 2)]),
                                        ("/513", [(3, 7, 513)]), ("/z", [(2, 0, 100)])])
    _, dev, want = whole_stream(chunker, store, entries, contents)
    total = len(want)
    big = 1024  # the header of /big
    pad = big + 512 + 40448 + 512 + 512  # the block of /513 with its last byte and the padding
    for begin, length in ((big + 512 + 2048, 4096), (big, 512 + 1024), (big + 512 + 39936, 512),
                          (pad, 512), (total - 1024, 1024), (total - 512, 512), (total, 0),
                          (total, 512), (0, 512)):
        rc, got, msg = dev_tar(chunker, store, dev, begin, length, fill=True)
        assert rc == 0, msg
        n = min(length, total - begin)
        assert got[:n] == want[begin:begin + n], (begin, length)
        assert set(got[n:]) <= {0xA5}
    assert want[pad + 1:pad + 512] == bytes(511)


def test_tar_runs_of_equal_chunks(chunker, stored):
    st, store = stored
    cases = [
        # files that alternate between two chunks: a run per DataRef, two chunks
        ([("/alt/%02d" % i, [(i % 2, 10 * i, 5)]) for i in range(10)], 10, 2),
        # one file across three chunks
        ([("/three", [(0, 0, 10), (0, 10, 10), (1, 0, 10), (2, 0, 5), (2, 5, 5)])], 3, 3),
        # the same chunk named by the first and the last file only
        ([("/f0", [(0, 0, 4)]), ("/f1", [(1, 0, 4)]), ("/f2", [(1, 4, 4)]), ("/f3", [(0, 4, 4)])],
         3, 2),
        # files packed into one chunk: one run
        ([("/p/%02d" % i, [(1, 100 * i, 100)]) for i in range(40)], 1, 1),
    ]
    for named, runs, chunks in cases:
        entries, contents = entries_of(st, named)
        whole_stream(chunker, store, entries, contents)
        rs = pf.last_resident_stats(chunker)
        assert (rs["runs"], rs["chunks"]) == (runs, chunks), (named[0][0], rs)
        assert rs["pieces"] == sum(len(sl) for _, sl in named)
        # per window, device to host: the window, three totals, the runs, the guards, the
        # bounds flag, the ok flags
        assert rs["d2h_bytes"] == 32 + 24 + 80 * runs + 64 * 7 + 4 + chunks


def test_tar_errors_equal_the_hosts(chunker, stored):
    st, store = stored
    ok = ("/ok", [(0, 0, 5)])
    bad_ref = OF.Index("/past", "default", [Ch.DataRef(st.orefs[0], bytes(32), 2990, 11)])
    cases = [
        ([("/é", [(0, 0, 1)]), ok], _lib.PFSCDC_EUNSUPPORTED, "é"),
        ([ok, ("/x\xff", []), ok, ("/" + "a" * 100, [])], _lib.PFSCDC_EUNSUPPORTED, "/x"),
        ([ok, ("/" + "a" * 100, [(0, 0, 1)])], _lib.PFSCDC_EUNSUPPORTED, "/" + "a" * 100),
        ([ok, ("b" * 101, [(0, 0, 1)])], _lib.PFSCDC_EUNSUPPORTED, "b" * 101),
        ([ok, ("/dir/", [(0, 0, 0)])], _lib.PFSCDC_EINVAL, "/dir/"),
        ([ok, ("/dir/", [(0, 0, 3)]), ("/é", [])], _lib.PFSCDC_EINVAL, "/dir/"),
        ([ok, ("", [])], _lib.PFSCDC_EINVAL, "empty name"),
    ]
    for named, code, names in cases:
        entries, _ = entries_of(st, named)
        lst = lst_of(entries)
        dev = up(chunker, lst)
        want = host_tar(chunker, store, lst, 0, 4096, fill=True)
        for _ in range(2):  # the second call answers from the cached plan
            got = dev_tar(chunker, store, dev, 0, 4096, fill=True)
            assert got == want
        assert want[0] == code and names in want[2], want[2]
        assert set(want[1]) == {0xA5}
        assert dev_layout(chunker, dev)[0] == code
    # a DataRef past its ref_size, behind a name that would be refused too
    entries, _ = entries_of(st, [("/é", [])])
    lst = lst_of(entries + [bad_ref])
    want = host_tar(chunker, store, lst, 0, 4096, fill=True)
    assert want[0] == _lib.PFSCDC_EINVAL
    assert dev_tar(chunker, store, up(chunker, lst), 0, 4096, fill=True) == want


def test_tar_one_id_with_two_ref_sizes_is_corrupt(chunker, stored):
    """Adjacent DataRefs of one Ref.Id that claim different Ref.SizeBytes: each is valid against
    its own ref_size, so only the compare with the stored length can refuse the false one.  It
    must head a run of its own and reach that compare: PFSCDC_ECORRUPT as the host's, out
    untouched, and no slice beyond the stored chunk reaches the gather."""
    st, store = stored
    true_ref = st.orefs[0]
    far = Ch.Ref(size_bytes=10 ** 9, edge=False, id=true_ref.id, dek=true_ref.dek)
    for drs in ([Ch.DataRef(true_ref, bytes(32), 0, 10), Ch.DataRef(far, bytes(32), 5 * 10 ** 8, 10)],
                [Ch.DataRef(true_ref, bytes(32), 0, 10), Ch.DataRef(far, bytes(32), 5, 10),
                 Ch.DataRef(true_ref, bytes(32), 20, 10)]):
        lst = lst_of([OF.Index("/ok", "default", [Ch.DataRef(st.orefs[1], bytes(32), 0, 5)]),
                      OF.Index("/two-sizes", "default", drs)])
        dev = up(chunker, lst)
        want = host_tar(chunker, store, lst, 0, 4096, fill=True)
        got = dev_tar(chunker, store, dev, 0, 4096, fill=True)
        assert want[0] == _lib.PFSCDC_ECORRUPT and set(want[1]) == {0xA5}
        assert got == want
        # a window that holds only the first file renders
        assert dev_tar(chunker, store, dev, 0, 1024) == host_tar(chunker, store, lst, 0, 1024)


def test_tar_path_with_a_nul_inside_ends_there_in_both_arms(chunker, stored):
    st, store = stored
    entries, _ = entries_of(st, [("/a", [(0, 0, 5)]), ("/nul\0tail", [(1, 3, 600)]),
                                 ("/b", [(2, 0, 7)])])
    lst = lst_of(entries)
    dev = up(chunker, lst)
    want = host_tar(chunker, store, lst, 0, 8192)
    assert want[0] == 0 and want[1][1024:1024 + 5] == b"/nul\0"
    assert dev_tar(chunker, store, dev, 0, 8192) == want
    entries, _ = entries_of(st, [("\0hidden", [(0, 0, 5)])])  # an empty name to both
    lst = lst_of(entries)
    want = host_tar(chunker, store, lst, 0, 4096, fill=True)
    assert want[0] == _lib.PFSCDC_EINVAL
    assert dev_tar(chunker, store, up(chunker, lst), 0, 4096, fill=True) == want


def test_tar_store_errors_leave_out_untouched(chunker, stored):
    st, store = stored
    entries, _ = entries_of(st, [("/a", [(0, 0, 100)]), ("/b", [(1, 0, 100), (2, 0, 0)]),
                                 ("/c", [(3, 5, 100)])])
    lst = lst_of(entries)
    dev = up(chunker, lst)
    ids = [r.id for r in st.orefs]

    def variant(change):
        s = pc.ChunkStore()
        for i, rid in enumerate(ids):
            ct = change(i, st.store[rid])
            if ct is not None:
                s.put(rid, ct)
        return s

    missing = variant(lambda i, ct: None if i == 1 else ct)
    tampered = variant(lambda i, ct: ct[:50] + bytes([ct[50] ^ 1]) + ct[51:] if i == 3 else ct)
    shorter = variant(lambda i, ct: ct[:-1] if i == 0 else ct)
    unused = variant(lambda i, ct: None if i == 2 else ct)  # named by a zero-size DataRef only
    for s, code in ((missing, _lib.PFSCDC_ENOTFOUND), (tampered, _lib.PFSCDC_ECORRUPT),
                    (shorter, _lib.PFSCDC_ECORRUPT), (unused, _lib.PFSCDC_OK)):
        want = host_tar(chunker, s, lst, 0, 8192, fill=True)
        got = dev_tar(chunker, s, dev, 0, 8192, fill=True)
        assert want[0] == code and got == want
        if code:
            assert set(got[1]) == {0xA5}
    # the first window names neither the missing nor the tampered chunk
    for s in (missing, tampered):
        assert dev_tar(chunker, s, dev, 0, 1024) == host_tar(chunker, s, lst, 0, 1024)


@pytest.mark.parametrize("grid", [1, 2, 3, 0])
def test_tar_launch_widths(chunker, stored, knob, grid):
    knob("PFSCDC_CHACHA_GRID", grid)
    st, store = stored
    entries, contents = tiny_files(st, 1025)
    entries2, contents2 = entries_of(st, [("/zz-big300", [(i % 4, 7 * i, 1 + i % 5) for i in range(300)])])
    _, dev, want = whole_stream(chunker, store, entries + entries2, contents + contents2)
    rc, got, msg = dev_tar(chunker, store, dev, 512 * 1024, 512 * 1200)
    assert rc == 0 and got == want[512 * 1024:512 * 2224], msg


# ------------------------------------------------------------------ end to end

@pytest.mark.parametrize("seed", [1, 2])
def test_open_resident_equals_open(seed):
    ops, model = model_ops(seed)
    st, infos, _ = write(ops, mem_threshold=30_000, index=LOOP_INDEX)
    assert len(infos) >= 3 and any(i.deletive for i in infos)
    host, res = st.open(infos), st.open(infos, resident=True)
    assert res.resident is not None and host.resident is None
    want = T.stream([(p, model[p]) for p in sorted(model)])
    ht, rt = host.tar(), res.tar()
    assert rt.size() == ht.size() == len(want)
    assert rt.entry_offsets == ht.entry_offsets
    assert list(rt.windows(4096)) == list(ht.windows(4096))
    assert rt.read() == want
    assert rt.last_stats["plan_reused"] == 1
    rt2 = res.tar()  # a second stream over the same handle: the plan is the handle's
    assert rt2.read(512, 1024) == want[512:1536] and rt2.last_stats["plan_reused"] == 1
    assert res._host is None  # nothing above downloaded the list
    assert res._list.raw() == host._list.raw()
    assert [(f.path, f.tag, f.size_bytes) for f in res.files()] == \
        [(p, "default", len(model[p])) for p in sorted(model)]
    p = sorted(model)[len(model) // 2]
    assert res.read(p) == model[p]
    sub = st.open(infos, prefix="/b/", resident=True)
    assert sub.tar().read() == T.stream([(p, model[p]) for p in sorted(model) if p.startswith("/b/")])


def test_plain_c_process_reads_resident(tmp_path):
    exe = str(tmp_path / "resident_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "resident_consumer.c"),
                    "-L", libdir, "-lpfscdc", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    out = str(tmp_path / "out.tar")
    res = subprocess.run([exe, out], capture_output=True, text=True, timeout=100)
    assert res.returncode == 0, res.stdout + res.stderr
    model = {"/f%02d" % k: bytes((k + j) & 0xFF for j in range(k * 997 + 13)) for k in range(24)}
    del model["/f03"]
    model["/f05"] = b"again"
    assert open(out, "rb").read() == T.stream([(p, model[p]) for p in sorted(model)])
    fields = res.stdout.split()
    assert fields[:2] == ["ok", str(len(model))]
    assert int(fields[4]) >= 1  # additive roots over a level of their own were read resident
