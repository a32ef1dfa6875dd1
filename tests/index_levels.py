"""Multi-level indexes built by hand, for the index decode tests (a helper: no tests here).

build_levels() generalises test_gpu_index_read.hand_built_index: any level-0 stream (oracle
entries, or raw frame bytes for malformed and hand-encoded frames), cut at any sizes on every
level, with the Range entries index/writer.go:102-121 would write for those chunks, up to the
root.  `info` says where the frames and the chunk borders of every level lie, so that a test can
assert the edge it is named for from its own sizes.

The cases below are the inputs of tests/test_index_levels_cpu.py (which proves them against
pfscdc_index_decode_host, without a GPU) and tests/test_gpu_index_decode.py (which decodes them
on the device); each case comes with the shape facts both files assert.  Cases are built once per
process (the oracle encrypts every distinct chunk once: stored_chunks.created)."""
import functools
import itertools
import random
from bisect import bisect_right

from stored_chunks import created
from test_index_read_cpu import _dr, _ld, _varint

from oracle import chunker as Ch
from oracle import fileset as OF
from pfs_amd import chunk as pc

# index_walk_kernel stages kIdxWin + 16 bytes per pass, index_scan_kernel scans tiles of
# kIdxScanBlock frames, index_count_kernel / index_fill_kernel / index_flags_kernel have kIdxBlock
# lanes per workgroup (list_kernels.hip section 8)
WIN = 8192 + 16
TILE = 1024
LANES = 256

ONE_CHUNK = 1 << 40  # a cut size no stream reaches: the level is one chunk
MAX_LEVELS = 8


def frame_of(item) -> bytes:
    """An item of a level: an oracle Index (framed here), or a frame's raw bytes, length field
    included (which need be no frame at all)."""
    return item if isinstance(item, bytes) else OF.frame(OF.encode_index(item))


def _path_of(item) -> str:
    if not isinstance(item, bytes):
        return item.path
    try:  # a hand-encoded frame: the protobuf runtime's reading of it
        return OF._msgs()["Index"].FromString(item[8:]).path
    except Exception:
        return ""


def _last_path_of(item) -> str:
    if not isinstance(item, bytes) and item.range is not None:
        return item.range[1]
    return _path_of(item)


def cut_sizes(n: int, cuts) -> list:
    """The chunk sizes of a stream of n bytes cut at `cuts` (one int, or a list that is cycled);
    the last chunk is what remains."""
    cycle = itertools.cycle([cuts] if isinstance(cuts, int) else list(cuts))
    sizes, at = [], 0
    while at < n:
        z = min(next(cycle), n - at)
        assert z > 0
        sizes.append(z)
        at += z
    return sizes


def move_border(sizes: list, j: int, to: int) -> list:
    """`sizes` with the border between chunks j and j + 1 moved to stream offset `to`."""
    lo = sum(sizes[:j])
    hi = lo + sizes[j] + sizes[j + 1]
    assert lo < to < hi, (lo, to, hi)
    return sizes[:j] + [to - lo, hi - to] + sizes[j + 2:]


class Level:
    """One level: its items, its stream, and where frames and chunks lie in it."""

    def __init__(self, items, sizes):
        self.items = list(items)
        frames = [frame_of(x) for x in self.items]
        self.stream = b"".join(frames)
        self.starts = [0]
        for f in frames:
            self.starts.append(self.starts[-1] + len(f))
        self.end = self.starts.pop()  # starts[k]: where frame k begins
        self.borders = [0]
        for z in sizes:
            self.borders.append(self.borders[-1] + z)
        assert self.borders[-1] == self.end
        self.frames, self.chunks = len(frames), len(sizes)
        self.longest_frame = max(map(len, frames), default=0)
        self.longest_chunk = max(sizes, default=0)
        ends = self.starts[1:] + [self.end]
        at = set(self.starts)
        inner = self.borders[1:-1]
        self.crossing = sum(1 for b in inner if b not in at)
        self.on_start = sum(1 for b in inner if b in at)
        self.borders_in_length = 0
        for b in inner:
            k = bisect_right(self.starts, b) - 1
            self.borders_in_length += 1 <= b - self.starts[k] <= 7
        self.inside = 0  # chunks wholly inside one frame
        for a, b in zip(self.borders[:-1], self.borders[1:]):
            k = bisect_right(self.starts, a) - 1
            self.inside += bool(self.starts[k] < a and b < ends[k])
        self.claims = []  # per chunk: the item its Range entry names

    def starts_in_chunk(self, j: int) -> int:
        """Frame starts in chunk j."""
        return sum(1 for s in self.starts if self.borders[j] <= s < self.borders[j + 1])

    def frame_at(self, offset: int) -> int:
        """The frame that holds stream offset `offset`."""
        return bisect_right(self.starts, offset) - 1


def build_levels(entries_or_frames, cuts_per_level):
    """(store, root, info).  Level 0 is `entries_or_frames`; level l is cut at cuts_per_level[l]
    (ONE_CHUNK past the list's end), every chunk goes into the store as chunk.Create stores it,
    and the Range entries of a level's chunks are the level above: the chunk's first annotation,
    or its second when the first continues the previous chunk's last path; Offset = where that
    annotation begins in the chunk (0 for a chunk that holds no frame start).  The level of one
    chunk is the top, and the root points at it.  info[l] is the Level."""
    if isinstance(cuts_per_level, int):
        cuts_per_level = [cuts_per_level]
    store, info, items = pc.ChunkStore(), [], list(entries_or_frames)
    assert items
    for l in range(MAX_LEVELS):
        cuts = cuts_per_level[l] if l < len(cuts_per_level) else ONE_CHUNK
        n = sum(len(frame_of(x)) for x in items)
        lv = Level(items, cut_sizes(n, cuts))
        info.append(lv)
        ends = lv.starts[1:] + [lv.end]
        ranges, last = [], None
        for a, b in zip(lv.borders[:-1], lv.borders[1:]):
            anns, k = [], max(0, bisect_right(lv.starts, a) - 1)
            while k < lv.frames and lv.starts[k] < b:  # the annotations: frames that meet [a, b)
                if ends[k] > a:
                    anns.append(k)
                k += 1
            k = anns[0]
            if len(anns) > 1 and last is not None and _path_of(items[last]) == _path_of(items[k]):
                k = anns[1]
            last = anns[-1]
            lv.claims.append(k)
            rid, dek, ct, _ = created(lv.stream[a:b])
            store.put(rid, ct)
            ref = Ch.Ref(size_bytes=b - a, edge=False, id=rid, dek=dek)
            rng = (max(0, lv.starts[k] - a), _last_path_of(items[last]), ref)
            it = items[k]
            if isinstance(it, bytes):
                ranges.append(OF.Index(_path_of(it), None, [], rng))
            else:
                ranges.append(OF.Index(it.path, it.tag, it.data_refs, rng))
        if lv.chunks == 1:
            r = ranges[0]
            return store, OF.encode_index(OF.Index(r.path, None, [], (0, r.range[1], r.range[2]))), info
        items = ranges
    raise AssertionError("the levels do not converge: the cuts are too small for the entries")


def pad_to(entries, k: int, target: int, which=None) -> list:
    """`entries` with the path of one entry before k (entry `which`, or the nearest that fits)
    lengthened until frame k starts at stream offset `target` (k = len(entries): the stream's
    length).  The pad is searched: the path's length varint grows at 128."""
    sizes = [len(frame_of(e)) for e in entries[:k]]
    for j in ([which] if which is not None else range(k - 1, -1, -1)):
        e = entries[j]
        need = target - (sum(sizes) - sizes[j])
        for pad in range(max(0, need - sizes[j] - 2), max(0, need - sizes[j]) + 1):
            cand = OF.Index(e.path + "x" * pad, e.tag, e.data_refs, e.range)
            if len(frame_of(cand)) == need:
                return list(entries[:j]) + [cand] + list(entries[j + 1:])
    raise AssertionError("no padding puts frame %d at offset %d" % (k, target))


def sized(rng, path: str, ndr: int, size: int) -> OF.Index:
    """A File entry of ndr DataRefs whose frame is exactly `size` bytes: DataRefs are drawn
    again with a one-byte offset while the frame is too long, then the path is lengthened."""
    e = OF.Index(path, "default", [_dr(rng) for _ in range(ndr)])
    for i in range(ndr):
        if len(frame_of(e)) <= size:
            break
        e.data_refs[i] = _dr(rng, offset=rng.randrange(1, 128))
    return pad_to([e], 1, size, which=0)[0]


# ------------------------------------------------------------------ entries

def drawn_path(rng, i: int) -> str:
    """A path as test_index_read_cpu.random_entry draws it (non-ASCII bytes)."""
    return "/f%05d/" % i + "".join(rng.choice("abcé日") for _ in range(rng.randrange(0, 20)))


def small(i: int, ndr_rng=None, ndr=0) -> OF.Index:
    """The shortest kind: a 10-byte path, the default tag, no DataRefs: a 31-byte frame."""
    drs = [_dr(ndr_rng) for _ in range(ndr)] if ndr else []
    return OF.Index("/s%05d/ab" % i, "default", drs)


SMALL_FRAME = 31


def good(i: int) -> OF.Index:
    """A 40-byte frame (the corruption cases' filler)."""
    return OF.Index("/g%05d/abcdefghijk" % i, "default", [])


GOOD_FRAME = 40


# ------------------------------------------------------------------ a. tiles and passes

DENSE_N = 2049
DENSE_CUTS = [300, 9000, 64, 20000, 1000, 8208, 8209, 150]
DENSE_BIG, DENSE_HUGE = 8699, 37248  # the frames of entries 1023 and 1500


@functools.lru_cache(maxsize=None)
def dense():
    """(store, root, info, entries): 2,049 File entries over chunks below and above the
    walker's window, with a frame longer than one window in the last lane of scan tile 0 and
    one longer than four windows."""
    rng = random.Random(2049)
    entries = []
    for i in range(DENSE_N):
        path = drawn_path(rng, i)
        if i % 97 == 5:  # path lengths across 127 and 128: the length varint's second byte
            want = 126 + (i // 97) % 4
            path += "é" * ((want - len(path.encode())) // 2)
            path += "x" * (want - len(path.encode()))
        entries.append(OF.Index(path, rng.choice(["", "default", "täg"]),
                                [_dr(rng) for _ in range(rng.choice([0, 1, 1, 2, 5]))]))
    entries[1023] = sized(rng, "/f01023/", 70, DENSE_BIG)
    entries[1024] = OF.Index(entries[1024].path, "default", [])
    entries[1500] = sized(rng, "/f01500/", 300, DENSE_HUGE)
    entries[2048] = OF.Index(entries[2048].path, "täg", [_dr(rng) for _ in range(5)])
    probe = Level(entries, cut_sizes(sum(len(frame_of(e)) for e in entries), DENSE_CUTS))
    sizes = [b - a for a, b in zip(probe.borders[:-1], probe.borders[1:])]
    # two borders shifted: one into a length field (3 bytes past a frame start), one onto a
    # frame start; both chunks lie before the frames set by hand
    for j, past in ((3, 3), (11, 0)):
        b = probe.borders[j + 1]
        sizes = move_border(sizes, j, probe.starts[probe.frame_at(b)] + past)
    store, root, info = build_levels(entries, [sizes, ONE_CHUNK])
    return store, root, info, entries


def dense_facts(info):
    l0, l1 = info[0], info[1]
    assert len(info) == 2 and l0.frames == DENSE_N > 2 * TILE
    lens = [b - a for a, b in zip(l0.starts, l0.starts[1:] + [l0.end])]
    assert lens[1023] == DENSE_BIG > WIN and lens[1500] == DENSE_HUGE > 4 * WIN
    assert l0.inside >= 2  # chunks inside the 37 KB frame
    assert l0.borders_in_length >= 1 and l0.on_start >= 1 and l0.crossing >= 10
    assert l0.longest_chunk > 2 * WIN
    sizes = {b - a for a, b in zip(l0.borders[:-1], l0.borders[1:])}
    assert min(sizes) < 100 and {WIN, WIN + 1} <= sizes
    # the level above: one walker over many windows of Range frames
    assert l1.chunks == 1 and l1.end > 4 * WIN and l1.frames == l0.chunks
    assert l1.longest_frame > DENSE_HUGE  # the 37 KB entry, written again in its chunks' Ranges


def passes(frames: int, grid: int) -> int:
    """Passes of a one-frame-per-lane kernel over `frames` at `grid` workgroups."""
    return -(-frames // (grid * LANES))


@functools.lru_cache(maxsize=None)
def tile(n: int):
    """(store, root, info, entries): n entries of the shortest kind in one chunk under the root;
    a few carry one DataRef, so that both of the scan's running sums differ across a tile."""
    rng = random.Random(n)
    with_dr = {0, 1022, 1023, 1024, 1500, 2047, 2048}
    entries = [small(i, rng, 1 if i in with_dr else 0) for i in range(n)]
    return build_levels(entries, ONE_CHUNK) + (entries,)


def tile_facts(info, n):
    assert len(info) == 1 and info[0].chunks == 1 and info[0].frames == n
    assert info[0].end > 3 * WIN  # one walker, several windows


# ------------------------------------------------------------------ b. three levels

FINE_N = 1300


@functools.lru_cache(maxsize=None)
def fine():
    """(store, root, info, entries): 1,300 31-byte frames cut every 64 bytes, the level above
    every 3,000."""
    entries = sorted((OF.Index("/d%d/f%05d" % (i % 5, i), "default", []) for i in range(FINE_N)),
                     key=lambda e: e.path)
    return build_levels(entries, [64, 3000]) + (entries,)


def fine_facts(info):
    assert len(info) == 3
    assert info[0].frames == FINE_N and info[0].longest_frame == SMALL_FRAME
    assert info[0].end == FINE_N * SMALL_FRAME
    assert info[0].chunks > 600 and info[0].crossing > 580
    assert info[1].frames == info[0].chunks > 2 * LANES and info[1].chunks > 10
    assert info[2].chunks == 1 and info[2].frames == info[1].chunks


def tail_chunk(lv, upper: str):
    """The level-0 chunk a read with this upper bound ends in (the first whose Range names a
    path beyond it), or None."""
    for j, k in enumerate(lv.claims):
        if _path_of(lv.items[k]).encode() > upper.encode():
            return j
    return None


def mid_frame_upper(lv, entries, k0: int) -> str:
    """The path of the first entry from k0 on that, as an upper bound, makes the read end in a
    tail chunk that is not the level's last and ends inside a frame."""
    for e in entries[k0:]:
        j = tail_chunk(lv, e.path)
        if j is not None and j + 1 < lv.chunks and lv.borders[j + 1] not in lv.starts:
            return e.path
    raise AssertionError("no upper bound ends in a chunk that ends mid-frame")


# ------------------------------------------------------------------ c. window edges

EDGE_STARTS = [WIN - 9, WIN - 8, WIN - 7, WIN - 1, WIN, WIN + 1]
EDGE_K = 40
HOP_ALIGN = [0, 1, 8, 15]
HOP_K = 12
END_TOTALS = [WIN - 1, WIN, WIN + 1]
END_MOD16 = [0, 1, 9, 15]
STRAY = [1, 3, 7]


def _smalls(rng, n, choices):
    return [OF.Index(drawn_path(rng, i), rng.choice(["", "default", "täg"]),
                     [_dr(rng) for _ in range(rng.choice(choices))]) for i in range(n)]


@functools.lru_cache(maxsize=None)
def edge(s: int):
    """60 small entries in one chunk, frame EDGE_K starting at stream offset s."""
    entries = pad_to(_smalls(random.Random(s), 60, [0, 0, 1]), EDGE_K, s)
    return build_levels(entries, ONE_CHUNK) + (entries,)


def edge_facts(info, s):
    lv = info[0]
    assert len(info) == 1 and lv.chunks == 1 and lv.frames == 60
    assert lv.starts[EDGE_K] == s and lv.starts[EDGE_K - 1] < WIN - 16 and lv.end > s + 100


@functools.lru_cache(maxsize=None)
def hop(r: int):
    """Frame HOP_K - 1 is the 8,699-byte one, begun in the first window; frame HOP_K starts
    past that window at an offset that is r mod 16."""
    rng = random.Random(100 + r)
    entries = _smalls(rng, 60, [0, 0, 1])
    entries[HOP_K - 1] = sized(rng, "/f%05d/" % (HOP_K - 1), 70, DENSE_BIG)
    entries = pad_to(entries, HOP_K, 11 * 1024 + r, which=HOP_K - 2)
    return build_levels(entries, ONE_CHUNK) + (entries,)


def hop_facts(info, r):
    lv = info[0]
    assert len(info) == 1 and lv.chunks == 1 and lv.frames == 60
    assert lv.starts[HOP_K - 1] + 8 <= WIN  # the long frame's length is read in the first window
    assert lv.starts[HOP_K] > WIN and lv.starts[HOP_K] % 16 == r
    assert lv.starts[HOP_K] - lv.starts[HOP_K - 1] == DENSE_BIG


def end_totals():
    """Stream lengths around one window, and past two windows at four values mod 16."""
    return END_TOTALS + [2 * WIN + 1600 + r for r in END_MOD16]


@functools.lru_cache(maxsize=None)
def end(n: int, stray: int = 0):
    """Small entries in one chunk of exactly n bytes, then `stray` bytes that are no frame."""
    rng = random.Random(n)
    entries = _smalls(rng, 30 if n < 2 * WIN else 90, [0, 1, 1])
    entries = pad_to(entries, len(entries), n)
    items = entries + ([bytes(stray)] if stray else [])
    return build_levels(items, ONE_CHUNK) + (entries,)


def end_facts(info, n, stray):
    lv = info[0]
    assert len(info) == 1 and lv.chunks == 1 and lv.end == n + stray
    assert lv.frames == (30 if n < 2 * WIN else 90) + bool(stray)
    assert n in END_TOTALS or (n > 2 * WIN and n % 16 in END_MOD16)
    if stray:
        assert lv.starts[-1] == n


# ------------------------------------------------------------------ d. densest frames

ZERO_N = 1025
ZERO_CUTS = [20, 8, 12]


@functools.lru_cache(maxsize=None)
def zeros(cut: int):
    """1,025 zero-length frames (8 zero bytes each), cut every `cut` bytes."""
    return build_levels([OF.frame(b"")] * ZERO_N, [cut, ONE_CHUNK])


def zeros_facts(info, cut):
    lv = info[0]
    assert len(info) == 2 and lv.frames == ZERO_N > TILE and lv.end == 8 * ZERO_N
    assert lv.longest_frame == 8 and lv.chunks == -(-8 * ZERO_N // cut)
    # walker i has room for len / 8 + 1 starts (index.cpp): some chunk fills it
    per = [lv.starts_in_chunk(j) for j in range(lv.chunks)]
    room = [(b - a) // 8 + 1 for a, b in zip(lv.borders[:-1], lv.borders[1:])]
    assert all(p <= r for p, r in zip(per, room))
    if cut % 8:
        assert any(p == r for p, r in zip(per, room))
        assert any(c > lv.frame_at(lv.borders[j]) for j, c in enumerate(lv.claims))  # second ann.
    if cut == 20:
        assert set(per[:-1]) == {2, 3} and set(room[:-1]) == {3}


# ------------------------------------------------------------------ e. wire shapes

def wire_items():
    """(items, want): File-only entries of every field shape, as oracle entries or as frames
    encoded by hand, and what each decodes to (an oracle Index)."""
    rng = random.Random(7)
    entries = []
    for plen in (1, 127, 128, 300):  # the path's length varint is 1 or 2 bytes
        entries.append(OF.Index("/" + "p" * (plen - 1), "default", [_dr(rng)]))
    entries.append(OF.Index("/café/日本語", "default", [_dr(rng)]))  # non-ASCII
    entries.append(OF.Index("/empty-tag", "", [_dr(rng)]))  # proto3 omits the empty tag
    for ndr in (0, 1, 40):
        entries.append(OF.Index("/drs%d" % ndr, "default", [_dr(rng) for _ in range(ndr)]))
    for off in (0, 127, 128, (1 << 32) + 5):  # offset_bytes 0 is omitted on the wire
        entries.append(OF.Index("/off%d" % off, "default", [_dr(rng, offset=off, size=off)]))
    for edge_ in (True, False):  # edge false is omitted
        entries.append(OF.Index("/edge%d" % edge_, "default", [_dr(rng, edge=edge_)]))
    entries.append(OF.Index("/file-no-refs", "default", []))
    items, want = list(entries), list(entries)
    # unknown fields of a known wire type (varint, bytes, fixed64, fixed32) are skipped
    idx = OF.Index("/unknown-fields", "default", [_dr(random.Random(5))])
    extra = b"\x78\x05" + _ld(17, b"zz") + b"\x81\x01" + bytes(8) + b"\x8d\x01" + bytes(4)
    items.append(OF.frame(OF.encode_index(idx) + extra))
    want.append(idx)
    file_ = _ld(3, _ld(1, b"default"))
    # a non-minimal varint for the path's length: 5 as 0x85 0x80 0x00
    items.append(OF.frame(b"\x0a\x85\x80\x00/nonm" + file_))
    want.append(OF.Index("/nonm", "default", []))
    # path twice: the last wins
    items.append(OF.frame(_ld(1, b"/first") + _ld(1, b"/second") + file_))
    want.append(OF.Index("/second", "default", []))
    # file before path
    items.append(OF.frame(file_ + _ld(1, b"/path-after-file")))
    want.append(OF.Index("/path-after-file", "default", []))
    # size_bytes and offset_bytes as ten-byte varints: negative int64
    d = _dr(rng, offset=-5, size=-(1 << 62))
    neg = lambda v: _varint(v & ((1 << 64) - 1))
    assert len(neg(-5)) == 10
    ref = (_ld(1, d.ref.id) + b"\x10" + _varint(d.ref.size_bytes) + (b"\x18\x01" if d.ref.edge else b"")
           + _ld(4, d.ref.dek) + b"\x28\x01")
    dr = _ld(1, ref) + _ld(2, d.hash) + b"\x18" + neg(-5) + b"\x20" + neg(-(1 << 62))
    items.append(OF.frame(_ld(1, b"/negative") + _ld(3, _ld(1, b"default") + _ld(2, dr))))
    want.append(OF.Index("/negative", "default", [d]))
    return items, want


@functools.lru_cache(maxsize=None)
def wire():
    items, want = wire_items()
    return build_levels(items, [700, ONE_CHUNK]) + (want,)


def wire_facts(info):
    assert len(info) == 2 and info[0].chunks > 5 and info[0].frames == len(wire_items()[0])
    assert info[0].crossing >= 5


# ------------------------------------------------------------------ f. corruption

BAD_PROTOS = [
    ("varint of 11 bytes", b"\x0a" + b"\xff" * 10 + b"\x01"),
    ("path length past the frame", b"\x0a\x05ab"),
    ("DataRef length past the File", _ld(3, b"\x12\x7f\x0a\x00")),
    ("path as a varint", b"\x08\x05"),
    ("Range.offset as bytes", _ld(2, b"\x0a\x01x")),
    ("group wire type", b"\x0b"),
    ("id of 31 bytes", _ld(3, _ld(2, _ld(1, _ld(1, bytes(31)))))),
    ("dek of 33 bytes", _ld(3, _ld(2, _ld(1, _ld(4, bytes(33)))))),
    ("hash of 16 bytes", _ld(3, _ld(2, _ld(2, bytes(16))))),
    ("fixed64 cut short", b"\x21\x00\x00"),
]
# a frame length that cannot be: the stream ends with it (and four more bytes)
BAD_LENGTHS = [
    ("negative length", (-1).to_bytes(8, "little", signed=True)),
    ("length of 2^62", (1 << 62).to_bytes(8, "little")),
    ("length past the end", GOOD_FRAME.to_bytes(8, "little")),
    ("three bytes for a length", b"\x01\x00\x00"),
]
BAD = [(name, OF.frame(p), True) for name, p in BAD_PROTOS] + \
      [(name, b + frame_of(good(0))[:4], False) for name, b in BAD_LENGTHS]
BAD_NAMES = [name for name, _, _ in BAD]
PLACES = ["frame 1", "frame 1030", "first of a later chunk"]
FAR = 1030


@functools.lru_cache(maxsize=None)
def corrupt(name: str, place: str):
    """(store, root, info, at): the bad frame among 40-byte frames, and the stream offset it
    starts at.  A bad proto has frames after it; a bad length ends the stream."""
    bad, more = next((b, m) for n_, b, m in BAD if n_ == name)
    k = {"frame 1": 1, "frame 1030": FAR, "first of a later chunk": 20}[place]
    items = [good(i) for i in range(k)] + [bad] + ([good(k + 1 + i) for i in range(20)] if more else [])
    at = k * GOOD_FRAME
    cuts = [[at, ONE_CHUNK], ONE_CHUNK] if place == PLACES[2] else ONE_CHUNK
    return build_levels(items, cuts) + (at,)


def corrupt_facts(info, place, at):
    lv = info[0]
    k = lv.starts.index(at)
    assert k == {"frame 1": 1, "frame 1030": FAR, "first of a later chunk": 20}[place]
    if place == PLACES[1]:  # the second scan tile, past the walker's fourth window
        assert k > TILE and at > 4 * WIN and lv.chunks == 1
    if place == PLACES[2]:  # chunk 1 claims the bad frame
        assert len(info) == 2 and lv.chunks == 2 and lv.borders[1] == at and lv.claims[1] == k
    else:
        assert len(info) == 1


PAIR_AT = (300, 1500)


@functools.lru_cache(maxsize=None)
def corrupt_pair(second: str):
    """1,600 40-byte frames in one chunk with a bad proto as frame 300 and, as frame 1,500,
    another bad proto or a negative frame length.  (store, root, info, offsets of both)."""
    items = [good(i) for i in range(1600)]
    items[PAIR_AT[0]] = OF.frame(BAD_PROTOS[1][1])
    items[PAIR_AT[1]] = OF.frame(BAD_PROTOS[5][1]) if second == "proto" else BAD_LENGTHS[0][1]
    store, root, info = build_levels(items, ONE_CHUNK)
    return store, root, info, tuple(info[0].starts[k] for k in PAIR_AT)


def corrupt_pair_facts(info, offs):
    assert len(info) == 1 and info[0].chunks == 1
    # other workgroups at the shipped width, other passes at one workgroup; another scan tile
    assert PAIR_AT[0] // LANES != PAIR_AT[1] // LANES and PAIR_AT[1] > TILE
    assert offs[0] < offs[1] and offs[1] > 4 * WIN


@functools.lru_cache(maxsize=None)
def good_root():
    """A small good index, read after every corrupt one on the same context."""
    entries = _smalls(random.Random(77), 12, [0, 1, 2])
    return build_levels(entries, [500, ONE_CHUNK]) + (entries,)
