"""MergeReader on the GPU: the device arm of pfscdc_index_merge_ctx (rank, group, prefix sums,
fill and DataRef copy kernels) against the host specifications pfscdc_index_merge and
pfscdc_index_merge_deletive, array for array (entries, blob, DataRefs).  The lists come from
pfscdc_index_decode_host over frames the tests encode, so no writer is involved."""
import ctypes as C
import random

import pytest

from oracle import fileset as OF
from pfs_amd import _lib
from pfs_amd import fileset as pf
from pfs_amd.cdc import ChunkParams, Chunker
from test_index_read_cpu import _dr, _drt, _ref, merge_restated, random_entry, stream_of

pytestmark = pytest.mark.gpu

TAGS = ["", "default", "t1", "täg"]
# prefixes of one another, and bytes >= 0x80 (UTF-8) against ASCII: a signed compare misorders
SPECIAL = ["/a", "/a/", "/a0", "/ab", "/a/b", "/é", "/z", "/~", "/日本", "/\x7f", "/zé", "/z\x01"]


def keyb(k):
    return (k[0].encode(), k[1].encode())


def key_pool(n):
    paths = SPECIAL + ["/d%d/f%04d" % (i % 7, i) for i in range(n)]
    return sorted({(p, t) for i, p in enumerate(paths) for t in TAGS[:1 + i % 4]}, key=keyb)


def entry(rng, key, deletive):
    path, tag = key
    r = rng.random()
    if deletive and r < 0.8:
        return OF.Index(path, tag, [])
    if r < 0.005:
        drs = [_dr(rng) for _ in range(300)]
    else:
        drs = [_dr(rng) for _ in range(rng.choice([0, 1, 1, 1, 2, 5]))]
    rngf = (rng.randrange(1 << 33), path + "-last", _ref(rng)) if rng.random() < 0.1 else None
    return OF.Index(path, tag, drs, rngf)


def stream(rng, pool, n, deletive):
    keys = sorted(rng.sample(pool, n), key=keyb)
    return [entry(rng, k, deletive) for k in keys]


def lst_of(entries):
    return pf.index_decode_host(stream_of(entries))


def arrays(lst):
    """The three arrays of a list as bytes."""
    n, ents, blob, drs, ndr = lst._views()
    return (C.string_at(ents, 64 * n) if n else b"", blob, C.string_at(drs, 128 * ndr) if ndr else b"")


def check_lengths(lst):
    """The arrays are exactly as long as the entries say."""
    n, ents, blob, _, ndr = lst._views()
    want_blob = sum(ents[i].path_len + ents[i].tag_len + ents[i].last_path_len + 3 for i in range(n))
    want_recs = sum(ents[i].count + bool(ents[i].flags & _lib.IDX_HAS_CHUNK_REF) for i in range(n))
    assert (len(blob), ndr) == (want_blob, want_recs)
    at = 0
    for i in range(n):
        assert ents[i].first == at
        at += ents[i].count + bool(ents[i].flags & _lib.IDX_HAS_CHUNK_REF)


@pytest.fixture
def chunker():
    c = Chunker(ChunkParams(), 0)
    yield c
    c.close()


def both_arms(chunker, pairs, total_in):
    """Both modes on the device arm against the host specification; the merged file list."""
    out = None
    for deletive in (False, True):
        host = pf.index_merge(pairs, deletive=deletive)
        dev = pf.index_merge(pairs, chunker=chunker, deletive=deletive)
        st = pf.last_merge_stats(chunker)
        assert st["device"] == 1, st
        n_in = total_in[1] if deletive else total_in[0]
        assert (st["entries_in"], st["entries_out"]) == (n_in, len(host))
        assert st["groups"] >= st["entries_out"] and st["groups"] <= max(n_in, 0)
        h, d = arrays(host), arrays(dev)
        assert len(d[0]) == len(h[0]) and len(d[1]) == len(h[1]) and len(d[2]) == len(h[2])
        assert d[0] == h[0], "entries"
        assert d[1] == h[1], "blob"
        assert d[2] == h[2], "DataRefs"
        check_lengths(dev)
        if not deletive:
            out = host
    return out


def build(rng, pool, lengths):
    """Filesets whose streams (deletive, additive, deletive, ...) have the given lengths."""
    sets, pairs, n_all, n_del = [], [], 0, 0
    for i in range(0, len(lengths), 2):
        dele = stream(rng, pool, lengths[i], True)
        add = stream(rng, pool, lengths[i + 1], False)
        sets.append((dele, add))
        pairs.append((lst_of(dele) if dele or rng.random() < 0.5 else None,
                      lst_of(add) if add or rng.random() < 0.5 else None))
        n_all += len(dele) + len(add)
        n_del += len(dele)
    return sets, pairs, (n_all, n_del)


def restated(sets):
    return [(p, t, [_drt(d) for d in drs]) for p, t, drs in merge_restated(
        [([(e.path.encode(), (e.tag or "").encode(), e.data_refs) for e in dele],
          [(e.path.encode(), (e.tag or "").encode(), e.data_refs) for e in add])
         for dele, add in sets])]


def files_of(lst):
    return [(g["path"], g["tag"], [_drt(d) for d in g["data_refs"]]) for g in lst.raw()]


@pytest.mark.parametrize("grid", [1, 3, 0])
def test_stream_lengths_at_fan_in_5(chunker, knob, grid):
    """Ten streams of 0, 1, 2, 63, 64, 65, 255, 256, 257 and 100 entries over 700 keys, with
    1-3 workgroups (every kernel strides many passes) and at the shipped width."""
    knob("PFSCDC_INDEX_MERGE", 1)
    knob("PFSCDC_CHACHA_GRID", grid)
    rng = random.Random(40 + grid)
    sets, pairs, total = build(rng, key_pool(400)[:700], [0, 1, 2, 63, 64, 65, 255, 256, 257, 100])
    merged = both_arms(chunker, pairs, total)
    assert files_of(merged) == restated(sets)


@pytest.mark.parametrize("nfilesets", [1, 2, 3, 10])
def test_fan_in(chunker, knob, nfilesets):
    """Fan-in 1, 2, 3 and the compaction's 10 (20 streams), one key in every stream."""
    knob("PFSCDC_INDEX_MERGE", 1)
    rng = random.Random(60 + nfilesets)
    pool = key_pool(150)
    sets, pairs, total = build(rng, pool[1:], [rng.randrange(20, 90) for _ in range(2 * nfilesets)])
    every = pool[0]
    for dele, add in sets:  # pool[0] sorts first and is in no sample
        dele.insert(0, entry(rng, every, True))
        add.insert(0, entry(rng, every, False))
    pairs = [(lst_of(d), lst_of(a)) for d, a in sets]
    total = (total[0] + 2 * nfilesets, total[1] + nfilesets)
    merged = both_arms(chunker, pairs, total)
    got = files_of(merged)
    assert got == restated(sets)
    # the key in every stream: the last fileset's delete clears all but its own DataRefs
    assert got[0][:2] == keyb(every) and got[0][2] == [_drt(d) for d in sets[-1][1][0].data_refs]


@pytest.mark.parametrize("groups, grid", [(1300, 0), (2500, 0), (2500, 2)])
def test_prefix_sums_cross_their_tile(chunker, knob, groups, grid):
    """More than 1,024 and more than 2,048 groups."""
    knob("PFSCDC_INDEX_MERGE", 1)
    knob("PFSCDC_CHACHA_GRID", grid)
    rng = random.Random(groups)
    pool = key_pool(2000)
    assert len(pool) > 3000
    half = groups // 2
    a, b = pool[:half + 200], pool[half:groups]  # 200 keys in both additive lists
    sets = [([], [entry(rng, k, False) for k in a]),
            (stream(rng, pool[:groups], 150, True), [entry(rng, k, False) for k in b])]
    pairs = [(None, lst_of(sets[0][1])), (lst_of(sets[1][0]), lst_of(sets[1][1]))]
    merged = both_arms(chunker, pairs, (len(a) + len(b) + 150, 150))
    assert pf.last_merge_stats(chunker)["groups"] == 150  # (the deletive mode ran last)
    assert len(merged) > (1024 if groups < 2000 else 2048)
    assert files_of(merged) == restated(sets)


def test_places_of_a_deletive_entry(chunker, knob):
    """A deletive entry in first, middle and last place of a group; the deletive and the
    additive entry of one fileset in one group; lone entries; the empty tag."""
    knob("PFSCDC_INDEX_MERGE", 1)
    rng = random.Random(5)
    A = lambda p, t="": OF.Index(p, t, [_dr(rng), _dr(rng)])
    D = lambda p, t="": OF.Index(p, t, [])
    sets = [
        ([D("/every"), D("/first"), D("/lone-del")],
         [A("/every"), A("/last"), A("/lone-add"), A("/mid"), A("/tags", ""), A("/tags", "t1")]),
        ([D("/every"), D("/mid"), D("/tags", "t1")],
         [A("/every"), A("/first"), A("/last"), A("/mid"), A("/tags", "t1"), A("/tags", "t2")]),
        ([D("/every"), D("/last")],
         [A("/every"), A("/first"), A("/tags", "")]),
    ]
    pairs = [(lst_of(d), lst_of(a)) for d, a in sets]
    merged = both_arms(chunker, pairs, (sum(len(d) + len(a) for d, a in sets), 8))
    got = {(p, t): drs for p, t, drs in files_of(merged)}
    assert files_of(merged) == restated(sets)
    drs = lambda fs, i: [_drt(d) for d in sets[fs][1][i].data_refs]
    assert b"/last" not in [p for p, _ in got] and b"/lone-del" not in [p for p, _ in got]
    assert got[(b"/first", b"")] == drs(1, 1) + drs(2, 1)
    assert got[(b"/mid", b"")] == drs(1, 3)
    assert got[(b"/every", b"")] == drs(2, 0)
    assert got[(b"/lone-add", b"")] == drs(0, 2)
    assert got[(b"/tags", b"")] == drs(0, 4) + drs(2, 2)
    assert got[(b"/tags", b"t1")] == drs(1, 4) and got[(b"/tags", b"t2")] == drs(1, 5)


def test_prefix_keys_and_high_bytes(chunker, knob):
    """/a, /a/, /a0, /ab and keys with bytes >= 0x80: the order is strings.Compare's."""
    knob("PFSCDC_INDEX_MERGE", 1)
    rng = random.Random(6)
    pool = sorted({(p, t) for p in SPECIAL for t in TAGS}, key=keyb)
    sets, pairs, total = build(rng, pool, [10, 30, 12, 30, 8, 30])
    merged = both_arms(chunker, pairs, total)
    got = files_of(merged)
    assert got == restated(sets)
    keys = [g[:2] for g in got]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    paths = [k[0] for k in keys]
    assert paths.index("/z".encode()) < paths.index("/é".encode())  # 0x7a before 0xc3
    assert paths.index(b"/a") < paths.index(b"/a/") < paths.index(b"/a0") < paths.index(b"/ab")


def test_ranges_chunk_refs_and_many_datarefs(chunker, knob):
    """Entries of every shape index_decode_host gives (Range only, Range with a File, 0 and 300
    DataRefs) pass through alone and merge in groups."""
    knob("PFSCDC_INDEX_MERGE", 1)
    rng = random.Random(8)
    a = [random_entry(rng, i) for i in range(0, 120, 2)]
    b = [random_entry(rng, i) for i in range(0, 120, 3)]
    big = OF.Index("/zz-big", "t", [_dr(rng) for _ in range(300)], (9, "/zz-last", _ref(rng)))
    none = OF.Index("/zz-none", "t", [])
    wrap = OF.Index("/zz-wrap", "", [_dr(rng, size=(1 << 63) - 1)])  # twice: the sum wraps
    a += [big, none, wrap]
    b += [OF.Index("/zz-big", "t", [_dr(rng) for _ in range(300)]), none, wrap]
    la, lb = lst_of(a), lst_of(b)
    for x in (la, lb):  # (random_entry's paths ascend with i, its tags vary)
        keys = [(g["path"], g["tag"]) for g in x.raw()]
        assert keys == sorted(keys)
    merged = both_arms(chunker, [(None, la), (lb, lb), (la, None)], (2 * len(a) + 2 * len(b), len(a) + len(b)))
    merged = both_arms(chunker, [(None, la), (None, lb)], (len(a) + len(b), 0))
    raw = merged.raw()
    assert [len(g["data_refs"]) for g in raw if g["path"] == b"/zz-big"] == [600]
    assert [g["range"] for g in raw if g["path"] == b"/zz-big"] == [None]  # merged: a File only
    assert [g["size_bytes"] for g in raw if g["path"] == b"/zz-wrap"] == [-2]
    lone = [g for g in raw if g["range"] is not None]
    assert lone and all(g["range"][2] is not None for g in lone)  # chunk_refs pass through


def test_a_stream_out_of_order_goes_to_the_host_arm(chunker, knob):
    knob("PFSCDC_INDEX_MERGE", 1)
    rng = random.Random(9)
    good = lst_of([OF.Index("/f%02d" % i, "t", [_dr(rng)]) for i in range(70)])
    xs = [OF.Index("/f%02d" % i, "t", [_dr(rng)]) for i in range(0, 140, 2)]
    for bad in ([xs[5]] + xs, xs[:40] + [xs[39]] + xs[40:], xs[:69] + [xs[3]]):
        pairs = [(None, good), (None, lst_of(bad))]
        for deletive in (False, True):
            host = pf.index_merge(pairs, deletive=deletive)
            got = pf.index_merge(pairs, chunker=chunker, deletive=deletive)
            st = pf.last_merge_stats(chunker)
            if deletive:  # (the deletive lists are None: nothing to rank)
                assert st["device"] == 1 and len(got) == 0
                continue
            assert st["device"] == 0 and st["entries_in"] == 70 + len(bad)
            assert arrays(got) == arrays(host)
    # equal keys next to each other are not strictly ascending either
    pairs = [(lst_of([xs[0], xs[1], xs[1]]), None)]
    got = pf.index_merge(pairs, chunker=chunker, deletive=True)
    assert pf.last_merge_stats(chunker)["device"] == 0
    assert arrays(got) == arrays(pf.index_merge(pairs, deletive=True))


def test_the_knob_at_0_is_the_host_arm(chunker, knob):
    knob("PFSCDC_INDEX_MERGE", 0)
    rng = random.Random(10)
    sets, pairs, total = build(rng, key_pool(100), [20, 60, 20, 60])
    for deletive in (False, True):
        got = pf.index_merge(pairs, chunker=chunker, deletive=deletive)
        st = pf.last_merge_stats(chunker)
        assert st["device"] == 0 and st["entries_in"] == total[deletive] and st["entries_out"] == len(got)
        assert arrays(got) == arrays(pf.index_merge(pairs, deletive=deletive))
    knob("PFSCDC_INDEX_MERGE", 1)
    dev = pf.index_merge(pairs, chunker=chunker)
    assert pf.last_merge_stats(chunker)["device"] == 1
    assert arrays(dev) == arrays(pf.index_merge(pairs))


def test_nothing_to_merge(chunker, knob):
    knob("PFSCDC_INDEX_MERGE", 1)
    for pairs in ([], [(None, None)], [(lst_of([]), lst_of([])), (None, lst_of([]))]):
        for deletive in (False, True):
            assert len(pf.index_merge(pairs, chunker=chunker, deletive=deletive)) == 0
            assert pf.last_merge_stats(chunker)["device"] == 1
    out = C.c_void_p()
    lib = chunker.lib
    assert lib.pfscdc_index_merge_ctx(chunker.ctx, 2, None, 0, C.byref(out)) == _lib.PFSCDC_EINVAL
    assert lib.pfscdc_index_merge_ctx(None, 0, None, 0, C.byref(out)) == _lib.PFSCDC_EINVAL
    assert lib.pfscdc_index_merge_ctx(chunker.ctx, 0, None, 1, C.byref(out)) == _lib.PFSCDC_EINVAL
