"""The index decode kernels (index_walk_kernel, index_count_kernel, index_scan_kernel,
index_fill_kernel, index_flags_kernel) past one scan tile, one walker window and one pass of
their grid-stride loops, over the hand-built indexes of tests/index_levels.py (proven on the host
by tests/test_index_levels_cpu.py).  Every comparison is total and bit-exact, against the entries
that were encoded and against pfscdc_index_decode_host; every test asserts from its own sizes
that the edge it is named for is reached."""
import ctypes as C
import random

import pytest

import index_levels as IL
from oracle import fileset as OF
from pfs_amd import _lib
from pfs_amd import fileset as pf
from pfs_amd.cdc import ChunkParams, Chunker
from test_gpu_merge import arrays, check_lengths
from test_index_read_cpu import _decode_rc, filter_forms, flat_filter, got_of, want_of

pytestmark = pytest.mark.gpu

WIN = 8192 + 16  # index_walk_kernel: kIdxWin + 16 bytes staged per pass
TILE = 1024      # index_scan_kernel: kIdxScanBlock frames per tile
LANES = 256      # index_count_kernel, index_fill_kernel, index_flags_kernel: kIdxBlock
assert (WIN, TILE, LANES) == (IL.WIN, IL.TILE, IL.LANES)

ARMS = [1, 0]  # PFSCDC_INDEX_DECODE: the kernels, and the host arm (which proves the fixture)
# (decode arm, PFSCDC_CHACHA_GRID): the shipped width, one workgroup, three
WIDTHS = [(1, 0), (1, 1), (1, 3), (0, 0)]


@pytest.fixture
def chunker():
    c = Chunker(ChunkParams(), 0)
    yield c
    c.close()


def same(got, want):
    x, y = arrays(got), arrays(want)
    assert [len(v) for v in x] == [len(v) for v in y]
    assert x[0] == y[0], "entries"
    assert x[1] == y[1], "blob"
    assert x[2] == y[2], "DataRefs"


def read_whole(chunker, store, root, info, want, decode):
    """One unfiltered read, host list and resident list, held against the entries that were
    encoded (`want`: oracle entries) and against the host decode of level 0's stream.  The arrays
    are compared as bytes first: nothing is read through an entry's offsets (raw()) before the
    entries are known to be the host decode's."""
    host = pf.index_decode_host(info[0].stream)
    assert got_of(host) == [want_of(e) for e in want]
    lst = pf.index_read(chunker, store, root)
    stats = pf.last_index_stats(chunker)
    same(lst, host)
    check_lengths(lst)
    assert got_of(lst) == [want_of(e) for e in want]
    assert (stats["frames"], stats["levels"]) == (sum(lv.frames for lv in info), len(info)), stats
    dev = pf.index_read_dev(chunker, store, root)
    rs = pf.last_resident_stats(chunker)
    assert rs["read_resident"] == (1 if decode else 0), rs
    assert len(dev) == len(want)
    same(dev.download(chunker), host)
    dev.free()
    return stats


def read_rc(chunker, store, root):
    """pfscdc_index_read as C sees it: (rc, the list pointer's value, the context's message)."""
    out = C.c_void_p(0xDEAD)
    rc = chunker.lib.pfscdc_index_read(chunker.ctx, store._s, root, len(root), None, C.byref(out))
    return rc, out.value, chunker.lib.pfscdc_last_error(chunker.ctx).decode()


def refused(chunker, store, root, info, at):
    """The read is refused as corrupt, naming level 0's stream (the last level read) and the
    offset the host specification names; then the same context reads a good index."""
    rc, err, lst = _decode_rc(info[0].stream)
    assert (rc, err, lst) == (_lib.PFSCDC_ECORRUPT, at, None)
    rc, out, msg = read_rc(chunker, store, root)
    assert rc == _lib.PFSCDC_ECORRUPT, msg
    assert out is None  # no list
    assert ("index level %d:" % (len(info) - 1)) in msg and ("offset %d " % at) in msg, msg
    dev = C.c_void_p(0xDEAD)
    rc = chunker.lib.pfscdc_index_read_dev(chunker.ctx, store._s, root, len(root), None, C.byref(dev))
    assert rc == _lib.PFSCDC_ECORRUPT and dev.value is None
    gstore, groot, ginfo, gentries = IL.good_root()
    assert got_of(pf.index_read(chunker, gstore, groot)) == [want_of(e) for e in gentries]


# ------------------------------------------------------------------ a. tiles and passes

@pytest.mark.parametrize("decode, grid", WIDTHS)
def test_dense_index_past_two_tiles_nine_passes_and_four_windows(chunker, knob, decode, grid):
    """2,049 entries: three scan tiles with a 70-DataRef frame in tile 0's last lane, nine passes
    of the count and fill loops at one workgroup, walkers over chunks from 64 bytes to 20,000
    with a 37 KB frame that whole chunks lie inside, and one walker over the level above."""
    store, root, info, entries = IL.dense()
    IL.dense_facts(info)
    assert info[0].frames == 2049 and -(-2049 // LANES) == 9
    if grid:
        assert IL.passes(info[0].frames, grid) == {1: 9, 3: 3}[grid]
        assert info[0].chunks > 8 * grid  # the walkers: one chunk per workgroup and pass
    knob("PFSCDC_INDEX_DECODE", decode)
    knob("PFSCDC_CHACHA_GRID", grid)
    stats = read_whole(chunker, store, root, info, entries, decode)
    print(stats)
    assert stats["chunks_read"] == info[0].chunks + 1
    if decode:  # every chunk inside the long frames claims offset 0, which is no frame start
        assert stats["rewalked_chunks"] >= info[0].inside


@pytest.mark.parametrize("decode", ARMS)
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2048, 2049])
def test_scan_tile_edges(chunker, knob, decode, n):
    """n entries in one chunk: one walker, and the prefix sums alone decide where the records
    of the entries around 1,024 and 2,048 go."""
    store, root, info, entries = IL.tile(n)
    IL.tile_facts(info, n)
    assert min(abs(n - TILE), abs(n - 2 * TILE)) <= 1
    knob("PFSCDC_INDEX_DECODE", decode)
    read_whole(chunker, store, root, info, entries, decode)


# ------------------------------------------------------------------ b. three levels

@pytest.mark.parametrize("decode, grid", WIDTHS)
def test_three_levels_and_six_hundred_walkers(chunker, knob, decode, grid):
    store, root, info, entries = IL.fine()
    IL.fine_facts(info)
    assert info[0].chunks > 600 and info[1].frames > 2 * LANES
    knob("PFSCDC_INDEX_DECODE", decode)
    knob("PFSCDC_CHACHA_GRID", grid)
    stats = read_whole(chunker, store, root, info, entries, decode)
    assert stats["levels"] == 3
    assert stats["chunks_read"] == sum(lv.chunks for lv in info)


def test_filters_over_three_levels_equal_the_flat_restatement(chunker):
    """Every filter form over the 64-byte chunks: nearly every tail chunk ends mid-frame, so the
    walker's last frame runs past the selection's end and is dropped, not refused."""
    store, root, info, entries = IL.fine()
    IL.fine_facts(info)
    pairs = [(e.path.encode(), e.tag.encode()) for e in entries]
    rng = random.Random(4)
    host = pf.index_decode_host(info[0].stream)
    proper = 0
    for form in filter_forms(sorted({p for p, _ in pairs}), rng):
        got = pf.index_read(chunker, store, root, **form)
        same(got, pf.index_filter(host, **form))
        want = flat_filter(pairs, **form)
        assert [(g["path"], g["tag"]) for g in got.raw()] == want, form
        proper += 0 < len(want) < len(pairs)
    assert proper >= 20
    up = IL.mid_frame_upper(info[0], entries, 700)
    got = pf.index_read(chunker, store, root, upper=up)
    same(got, pf.index_filter(host, upper=up))
    assert got_of(got) == [want_of(e) for e in entries if e.path <= up]
    assert pf.last_index_stats(chunker)["chunks_read"] < sum(lv.chunks for lv in info)


@pytest.mark.parametrize("decode", ARMS)
def test_a_range_filter_that_ends_inside_the_long_frame(chunker, knob, decode):
    """The tail chunk ends inside the 37 KB frame: that frame is past the filter's end."""
    store, root, info, entries = IL.dense()
    lv = info[0]
    j = IL.tail_chunk(lv, entries[1499].path)
    assert lv.starts[1500] < lv.borders[j + 1] < lv.starts[1501]
    knob("PFSCDC_INDEX_DECODE", decode)
    lo = entries[1000].path
    got = pf.index_read(chunker, store, root, lower=lo, upper=entries[1499].path)
    same(got, pf.index_filter(pf.index_decode_host(lv.stream), lower=lo, upper=entries[1499].path))
    check_lengths(got)
    assert got_of(got) == [want_of(e) for e in entries[1000:1500]]
    assert pf.last_index_stats(chunker)["chunks_read"] < lv.chunks


# ------------------------------------------------------------------ c. window edges

@pytest.mark.parametrize("decode", ARMS)
@pytest.mark.parametrize("s", IL.EDGE_STARTS)
def test_a_length_field_at_the_windows_end(chunker, knob, decode, s):
    """A frame whose length field ends exactly at the first window's end, crosses it by 1 to 7
    bytes, or starts at the end or just past it."""
    store, root, info, entries = IL.edge(s)
    IL.edge_facts(info, s)
    assert -9 <= info[0].starts[IL.EDGE_K] - WIN <= 1
    knob("PFSCDC_INDEX_DECODE", decode)
    read_whole(chunker, store, root, info, entries, decode)


@pytest.mark.parametrize("decode", ARMS)
@pytest.mark.parametrize("r", IL.HOP_ALIGN)
def test_the_hop_over_a_frame_longer_than_the_window(chunker, knob, decode, r):
    store, root, info, entries = IL.hop(r)
    IL.hop_facts(info, r)
    assert info[0].longest_frame > WIN and info[0].starts[IL.HOP_K] % 16 == r
    knob("PFSCDC_INDEX_DECODE", decode)
    read_whole(chunker, store, root, info, entries, decode)


@pytest.mark.parametrize("decode", ARMS)
@pytest.mark.parametrize("n", IL.end_totals())
def test_stream_ends_and_stray_bytes_after_them(chunker, knob, decode, n):
    """Streams that end around the first window's end, and past two windows at four lengths
    mod 16 (the last window's clamp); then 1, 3 and 7 bytes after the last frame."""
    store, root, info, entries = IL.end(n)
    IL.end_facts(info, n, 0)
    assert abs(n - WIN) <= 1 or n > 2 * WIN
    knob("PFSCDC_INDEX_DECODE", decode)
    read_whole(chunker, store, root, info, entries, decode)
    for stray in IL.STRAY:
        bstore, broot, binfo, _ = IL.end(n, stray)
        IL.end_facts(binfo, n, stray)
        refused(chunker, bstore, broot, binfo, n)


# ------------------------------------------------------------------ d. densest frames

@pytest.mark.parametrize("decode", ARMS)
@pytest.mark.parametrize("cut", IL.ZERO_CUTS)
def test_zero_length_frames_fill_every_walkers_slots(chunker, knob, decode, cut):
    store, root, info = IL.zeros(cut)
    IL.zeros_facts(info, cut)
    host = pf.index_decode_host(info[0].stream)
    n, ents, blob, _, ndr = host._views()
    assert (n, blob, ndr) == (1025, bytes(3 * 1025), 0) and all(ents[i].flags == 0 for i in range(n))
    knob("PFSCDC_INDEX_DECODE", decode)
    read_whole(chunker, store, root, info, [OF.Index("")] * 1025, decode)
    lst = pf.index_read(chunker, store, root)
    assert arrays(lst)[1:] == (bytes(3 * 1025), b"")


# ------------------------------------------------------------------ e. wire shapes

@pytest.mark.parametrize("decode", ARMS)
def test_every_wire_shape_on_the_device(chunker, knob, decode):
    store, root, info, want = IL.wire()
    IL.wire_facts(info)
    knob("PFSCDC_INDEX_DECODE", decode)
    read_whole(chunker, store, root, info, want, decode)


# ------------------------------------------------------------------ f. corruption

@pytest.mark.parametrize("decode", ARMS)
@pytest.mark.parametrize("place", IL.PLACES)
@pytest.mark.parametrize("name", IL.BAD_NAMES)
def test_a_bad_frame_is_named_wherever_it_lies(chunker, knob, decode, name, place):
    store, root, info, at = IL.corrupt(name, place)
    IL.corrupt_facts(info, place, at)
    knob("PFSCDC_INDEX_DECODE", decode)
    refused(chunker, store, root, info, at)


@pytest.mark.parametrize("decode, grid", [(1, 1), (1, 0), (0, 0)])
def test_the_lower_of_two_bad_protos_is_named(chunker, knob, decode, grid):
    """Frames 300 and 1,500: other passes of one workgroup, other workgroups at full width."""
    store, root, info, offs = IL.corrupt_pair("proto")
    IL.corrupt_pair_facts(info, offs)
    knob("PFSCDC_INDEX_DECODE", decode)
    knob("PFSCDC_CHACHA_GRID", grid)
    refused(chunker, store, root, info, offs[0])


@pytest.mark.parametrize("decode, grid", [(1, 1), (1, 0), (0, 0)])
def test_a_bad_proto_in_front_of_a_bad_length_is_named(chunker, knob, decode, grid):
    """The walk stops at frame 1,500's length; the first frame that fails is frame 300."""
    store, root, info, offs = IL.corrupt_pair("length")
    IL.corrupt_pair_facts(info, offs)
    knob("PFSCDC_INDEX_DECODE", decode)
    knob("PFSCDC_CHACHA_GRID", grid)
    refused(chunker, store, root, info, offs[0])
