"""The inputs of tests/test_gpu_index_decode.py, proven without a GPU: for every case of
tests/index_levels.py, pfscdc_index_decode_host of each level's stream gives the entries that
built it (or refuses the stream at the bad frame), the store holds every chunk the Range entries
name, and the shape facts the GPU tests rely on (frames past a scan tile, chunks past a walker's
window, borders inside a length field ...) hold."""
import random

import pytest

import index_levels as IL
from oracle import chunker as Ch
from oracle import fileset as OF
from pfs_amd import _lib
from pfs_amd import fileset as pf
from test_index_read_cpu import _decode_rc, got_of, want_of


def proven(store, info, want0=None):
    """Every level's stream decodes on the host to the items that built it (want0: what level
    0's raw frames stand for), and every chunk lies in the store under the Range's ref."""
    for l, lv in enumerate(info):
        want = want0 if l == 0 and want0 is not None else lv.items
        assert got_of(pf.index_decode_host(lv.stream)) == [want_of(e) for e in want], l
        if l + 1 < len(info):
            up = info[l + 1].items
            assert len(up) == lv.chunks
            for j, r in enumerate(up):
                off, _, ref = r.range
                a, b = lv.borders[j], lv.borders[j + 1]
                assert ref.size_bytes == b - a
                assert Ch.chacha20_xor(ref.dek, store.get(ref.id)) == lv.stream[a:b]
                # the claim is a frame start inside the chunk, or 0 for a chunk inside one frame
                assert a + off in lv.starts or (off == 0 and lv.starts_in_chunk(j) == 0)
    assert info[-1].chunks == 1


def test_build_levels_restates_the_hand_built_index():
    """The same entries and cut as test_gpu_index_read.hand_built_index: the same root."""
    from test_gpu_index_read import hand_built_index
    store, root, entries, inside, border, longest = hand_built_index(random.Random(31), 200)
    store2, root2, info = IL.build_levels(entries, [200])
    assert root2 == root and len(info) == 2
    # (hand_built_index counts the chunks inside its longest entry alone)
    assert info[0].inside >= inside and info[0].longest_frame == longest
    assert border in info[0].borders and border in info[0].starts
    assert info[0].claims[border // 200] == 17  # the second annotation: entry 16 continues 15's path
    proven(store2, info)


def test_pad_to_places_a_frame_and_refuses_what_it_cannot():
    entries = [IL.small(i) for i in range(10)]
    for target in (8 * IL.SMALL_FRAME, 400, 8 * IL.SMALL_FRAME + 117, 8 * IL.SMALL_FRAME + 119, 5000):
        got = IL.pad_to(entries, 8, target)
        assert IL.Level(got, [sum(len(IL.frame_of(e)) for e in got)]).starts[8] == target
        assert [e.path for e in got] == sorted(e.path for e in got)
    with pytest.raises(AssertionError):
        IL.pad_to(entries, 8, 8 * IL.SMALL_FRAME - 1)
    with pytest.raises(AssertionError):  # the path's length varint grows: 128 bytes are skipped
        IL.pad_to(entries, 1, IL.SMALL_FRAME + 118, which=0)


def test_dense():
    store, root, info, entries = IL.dense()
    IL.dense_facts(info)
    proven(store, info)
    assert info[0].items == entries
    plens = {len(e.path.encode()) for e in entries}
    assert {126, 127, 128, 129} <= plens and any(ord(c) > 127 for e in entries for c in e.path)
    assert [len(entries[i].data_refs) for i in (1023, 1024, 1500, 2048)] == [70, 0, 300, 5]
    assert [e.path for e in entries] == sorted(e.path for e in entries)
    for grid, want in ((1, 9), (3, 3)):
        assert IL.passes(info[0].frames, grid) == want >= 2
    # the range filter the GPU test reads: its tail chunk ends inside the 37 KB frame
    j = IL.tail_chunk(info[0], entries[1499].path)
    assert info[0].starts[1500] < info[0].borders[j + 1] < info[0].starts[1501]
    print("dense: level-0 chunks", info[0].chunks, "bytes", info[0].end, "inside", info[0].inside,
          "level-1 bytes", info[1].end)


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2048, 2049])
def test_tile(n):
    store, root, info, entries = IL.tile(n)
    IL.tile_facts(info, n)
    proven(store, info)
    lst = pf.index_decode_host(info[0].stream)
    _, ents, _, _, ndr = lst._views()
    if n > IL.TILE:  # both running sums are non-zero where the second tile begins
        assert ents[IL.TILE].first > 0 and ents[IL.TILE].path_off > 0 and ndr > ents[IL.TILE].first


def test_fine():
    store, root, info, entries = IL.fine()
    IL.fine_facts(info)
    proven(store, info)
    up = IL.mid_frame_upper(info[0], entries, 700)
    assert entries[700].path <= up <= entries[702].path


@pytest.mark.parametrize("s", IL.EDGE_STARTS)
def test_edge(s):
    store, root, info, _ = IL.edge(s)
    IL.edge_facts(info, s)
    proven(store, info)


@pytest.mark.parametrize("r", IL.HOP_ALIGN)
def test_hop(r):
    store, root, info, _ = IL.hop(r)
    IL.hop_facts(info, r)
    proven(store, info)


@pytest.mark.parametrize("n", IL.end_totals())
def test_end(n):
    store, root, info, entries = IL.end(n)
    IL.end_facts(info, n, 0)
    proven(store, info)
    for stray in IL.STRAY:
        _, _, bad, _ = IL.end(n, stray)
        IL.end_facts(bad, n, stray)
        assert bad[0].stream[:n] == info[0].stream
        rc, err, lst = _decode_rc(bad[0].stream)
        assert (rc, err, lst) == (_lib.PFSCDC_ECORRUPT, n, None)


@pytest.mark.parametrize("cut", IL.ZERO_CUTS)
def test_zeros(cut):
    store, root, info = IL.zeros(cut)
    IL.zeros_facts(info, cut)
    # a zero-length frame is an entry of empty strings, no File, no Range
    proven(store, info, want0=[OF.Index("")] * IL.ZERO_N)
    lst = pf.index_decode_host(info[0].stream)
    n, ents, blob, _, ndr = lst._views()
    assert (n, blob, ndr) == (IL.ZERO_N, bytes(3 * IL.ZERO_N), 0)
    assert all(ents[i].flags == 0 for i in range(n))


def test_wire():
    store, root, info, want = IL.wire()
    IL.wire_facts(info)
    proven(store, info, want0=want)
    got = got_of(pf.index_decode_host(info[0].stream))
    by_path = {g["path"]: g for g in got}
    assert [len(g["path"]) for g in got[:4]] == [1, 127, 128, 300]
    assert {b"/nonm", b"/second", b"/path-after-file", b"/unknown-fields"} <= set(by_path)
    assert b"/first" not in by_path
    neg = by_path[b"/negative"]
    assert neg["size_bytes"] == -(1 << 62) and neg["data_refs"][0][5:] == (-5, -(1 << 62))


@pytest.mark.parametrize("place", IL.PLACES)
@pytest.mark.parametrize("name", IL.BAD_NAMES)
def test_corrupt(name, place):
    store, root, info, at = IL.corrupt(name, place)
    IL.corrupt_facts(info, place, at)
    rc, err, lst = _decode_rc(info[0].stream)
    assert (rc, err, lst) == (_lib.PFSCDC_ECORRUPT, at, None)
    assert len(pf.index_decode_host(info[0].stream[:at])) == info[0].starts.index(at)
    if len(info) == 2:
        proven(store, info[1:])


@pytest.mark.parametrize("second", ["proto", "length"])
def test_corrupt_pair(second):
    store, root, info, offs = IL.corrupt_pair(second)
    IL.corrupt_pair_facts(info, offs)
    rc, err, lst = _decode_rc(info[0].stream)
    assert (rc, err, lst) == (_lib.PFSCDC_ECORRUPT, offs[0], None)
    # with the first bad frame mended, the second is the one named
    mended = info[0].stream[:offs[0]] + IL.frame_of(IL.good(0)) + \
        info[0].stream[info[0].starts[IL.PAIR_AT[0] + 1]:]
    later = offs[1] + IL.GOOD_FRAME - (info[0].starts[IL.PAIR_AT[0] + 1] - offs[0])
    assert _decode_rc(mended)[:2] == (_lib.PFSCDC_ECORRUPT, later)


def test_good_root():
    store, root, info, entries = IL.good_root()
    assert len(info) == 2 and info[0].chunks > 2
    proven(store, info)
