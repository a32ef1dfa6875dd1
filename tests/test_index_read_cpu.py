"""Reading a fileset back, the host side (no GPU): pfscdc_index_decode_host (the specification
the decode kernels are tested against) against oracle.fileset's protobuf-runtime encoder, the
filter against a flat restatement of atStart / atEnd / tag (reader.go:95-122), and
pfscdc_index_merge against a sort-and-group restatement of MergeReader.iterate
(merge.go:37-77).  Truncated streams also run in a stand-alone program built with
-fsanitize=address,undefined around index_decode.cpp itself."""
import os
import random
import subprocess

import pytest

from oracle import chunker as Ch
from oracle import fileset as OF
from pfs_amd import _lib
from pfs_amd import fileset as pf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ref(rng, size=None):
    return Ch.Ref(size_bytes=rng.randrange(1, 1 << 40) if size is None else size,
                  edge=bool(rng.getrandbits(1)), id=rng.randbytes(32), dek=rng.randbytes(32))


def _dr(rng, offset=None, size=None, edge=None):
    ref = _ref(rng)
    if edge is not None:
        ref.edge = edge
    return Ch.DataRef(ref, rng.randbytes(32), rng.randrange(1 << 20) if offset is None else offset,
                      rng.randrange(1 << 20) if size is None else size)


def _drt(d):
    """A DataRef (oracle's or the binding's) as a comparable tuple."""
    return (bytes(d.ref.id), bytes(d.ref.dek), d.ref.size_bytes, bool(d.ref.edge), bytes(d.hash),
            d.offset_bytes, d.size_bytes)


def want_of(idx: OF.Index) -> dict:
    """What IndexList.raw() gives for an oracle Index."""
    rng = None
    if idx.range is not None:
        off, last, ref = idx.range
        # chunk.Reference(dataRef): {Ref, SizeBytes = Ref.SizeBytes}, no hash, offset 0
        rng = (off, last.encode(), (ref.id, ref.dek, ref.size_bytes, ref.edge, bytes(32), 0,
                                    ref.size_bytes))
    return {"path": idx.path.encode(), "tag": (idx.tag or "").encode(),
            "has_file": idx.tag is not None,
            "size_bytes": sum(d.size_bytes for d in idx.data_refs),
            "data_refs": [_drt(d) for d in idx.data_refs], "range": rng}


def got_of(lst: pf.IndexList) -> list:
    out = []
    for d in lst.raw():
        d = dict(d)
        d["data_refs"] = [_drt(x) for x in d["data_refs"]]
        if d["range"] is not None:
            off, last, ref = d["range"]
            d["range"] = (off, last, _drt(ref) if ref is not None else None)
        out.append(d)
    return out


def stream_of(entries) -> bytes:
    return b"".join(OF.frame(OF.encode_index(e)) for e in entries)


def random_entry(rng, i) -> OF.Index:
    path = "/f%05d/" % i + "".join(rng.choice("abcé日") for _ in range(rng.randrange(0, 20)))
    kind = rng.randrange(4)
    if kind == 0:  # a Range entry without a File
        return OF.Index(path, None, [], (rng.randrange(1 << 33), path + "z", _ref(rng)))
    drs = [_dr(rng) for _ in range(rng.choice([0, 1, 1, 2, 5]))]
    rngf = (rng.randrange(300), path + "y", _ref(rng)) if kind == 1 else None
    return OF.Index(path, rng.choice(["", "default", "täg"]), drs, rngf)


# ------------------------------------------------------------------ decode equals the encoder

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_decode_equals_encoder_by_count(n):
    rng = random.Random(1000 + n)
    entries = [random_entry(rng, i) for i in range(n)]
    lst = pf.index_decode_host(stream_of(entries))
    assert len(lst) == n
    assert got_of(lst) == [want_of(e) for e in entries]


def test_decode_covers_every_field_shape():
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
    for edge in (True, False):  # edge false is omitted
        entries.append(OF.Index("/edge%d" % edge, "default", [_dr(rng, edge=edge)]))
    entries.append(OF.Index("/range-only", None, [], (0, "/range-only-last", _ref(rng))))
    entries.append(OF.Index("/range-file", "default", [_dr(rng), _dr(rng)],
                            ((1 << 32) + 5, "/range-file-last", _ref(rng))))
    entries.append(OF.Index("/file-no-refs", "default", []))
    got = got_of(pf.index_decode_host(stream_of(entries)))
    assert got == [want_of(e) for e in entries]
    assert [len(g["path"]) for g in got[:4]] == [1, 127, 128, 300]
    assert got[5]["tag"] == b"" and got[5]["has_file"]
    assert not got[-3]["has_file"] and got[-3]["range"][0] == 0
    assert got[-2]["range"][0] == (1 << 32) + 5 and len(got[-2]["data_refs"]) == 2


def test_list_plugs_into_the_tar_arrays():
    """The accessors give what pfscdc_store_read_tar takes: NUL-terminated paths in the blob
    and (first, count) into the one DataRef array."""
    rng = random.Random(3)
    entries = [OF.Index("/a", "default", [_dr(rng)]), OF.Index("/b/c", "x", [_dr(rng), _dr(rng)])]
    lst = pf.index_decode_host(stream_of(entries))
    tf = lst.lib.pfscdc_index_list_tar_files(lst._p)
    assert [(tf[i].path, tf[i].first, tf[i].count) for i in range(2)] == \
        [(b"/a", 0, 1), (b"/b/c", 1, 2)]


# ------------------------------------------------------------------ malformed streams

def _decode_rc(stream: bytes):
    out, err = _lib.C.c_void_p(), _lib.C.c_uint64()
    rc = _lib.load().pfscdc_index_decode_host(stream, len(stream), _lib.C.byref(out),
                                              _lib.C.byref(err))
    lst = pf.IndexList(out) if out.value else None
    return rc, err.value, lst


def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _ld(field, payload):
    return _varint(field << 3 | 2) + _varint(len(payload)) + payload


def test_every_truncation_is_corrupt_or_a_clean_prefix():
    rng = random.Random(11)
    entries = [random_entry(rng, i) for i in range(12)]
    stream = stream_of(entries)
    want = [want_of(e) for e in entries]
    bounds, at = {0}, 0
    for e in entries:
        at += len(OF.frame(OF.encode_index(e)))
        bounds.add(at)
    for k in range(len(stream) + 1):
        rc, err, lst = _decode_rc(stream[:k])
        if k in bounds:
            assert rc == 0 and got_of(lst) == want[:len(lst)]
        else:
            assert rc == _lib.PFSCDC_ECORRUPT and lst is None
            assert err == max(b for b in bounds if b <= k)  # the frame that was cut


@pytest.mark.parametrize("name, proto", [
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
])
def test_malformed_protos_are_corrupt(name, proto):
    good = OF.frame(OF.encode_index(OF.Index("/ok", "default", [])))
    rc, err, lst = _decode_rc(good + OF.frame(proto) + good)
    assert rc == _lib.PFSCDC_ECORRUPT and lst is None, name
    assert err == len(good)


def test_malformed_frame_lengths_are_corrupt():
    good = OF.frame(OF.encode_index(OF.Index("/ok", "default", [])))
    for bad in ((-1).to_bytes(8, "little", signed=True), (1 << 62).to_bytes(8, "little"),
                (len(good)).to_bytes(8, "little"), b"\x01\x00\x00"):
        rc, err, lst = _decode_rc(good + bad + good[:4])
        assert rc == _lib.PFSCDC_ECORRUPT and err == len(good) and lst is None


def test_unknown_fields_of_a_known_wire_type_are_skipped():
    idx = OF.Index("/p", "default", [_dr(random.Random(5))])
    extra = b"\x78\x05" + _ld(17, b"zz") + b"\x81\x01" + bytes(8) + b"\x8d\x01" + bytes(4)
    got = got_of(pf.index_decode_host(OF.frame(OF.encode_index(idx) + extra)))
    assert got == [want_of(idx)]


def test_truncations_under_host_sanitizers(tmp_path):
    """index_decode.cpp compiled into a stand-alone program with AddressSanitizer and UBSan:
    every truncation in an exactly-sized heap block, then every single-byte flip."""
    rng = random.Random(13)
    entries = [random_entry(rng, i) for i in range(10)]
    entries.append(OF.Index("/many", "default", [_dr(rng) for _ in range(12)],
                            (5, "/many-last", _ref(rng))))
    stream = stream_of(entries)
    (tmp_path / "stream.bin").write_bytes(stream)
    exe = str(tmp_path / "index_truncate")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "index_truncate.cpp"),
                    os.path.join(ROOT, "pfs_amd", "csrc", "index_decode.cpp"), "-o", exe],
                   check=True)
    res = subprocess.run([exe, str(tmp_path / "stream.bin")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.split() == ["ok", str(len(entries)), str(len(entries) + 1)]


# ------------------------------------------------------------------ filters

def flat_filter(entries, lower=None, upper=None, prefix=None, tag=None):
    """Reader.Iterate over level-0 entries [(path, tag)] (bytes), restated flat."""
    lower, upper, prefix, tag = (x or b"" for x in (lower, upper, prefix, tag))

    def at_start(name):
        return name >= lower if lower else name >= prefix

    def at_end(name):
        if upper:
            return name > upper
        k = min(len(name), len(prefix))
        return name[:k] > prefix[:k]

    out = []
    for path, t in entries:
        if at_end(path):
            break
        if not at_start(path):
            continue
        if not tag or tag == t:
            out.append((path, t))
    return out


def filter_forms(paths, rng):
    """Every filter form over a sorted path list: none, each bound alone, both, a prefix, a
    tag, and their mixes, with bounds on, between and beyond the paths."""
    picks = [rng.choice(paths) for _ in range(3)] + [paths[0], paths[-1], b"/", b"/zzzz", b"0"]
    picks += [p[:max(1, len(p) // 2)] for p in picks[:3]] + [picks[0] + b"\x01"]  # (a C string: no NUL)
    forms = [{}]
    for a in picks:
        forms += [{"lower": a}, {"upper": a}, {"prefix": a}, {"prefix": a, "tag": b"t1"}]
        for b in picks[:4]:
            forms += [{"lower": a, "upper": b}, {"lower": a, "prefix": b},
                      {"upper": a, "prefix": b}]
    forms += [{"tag": b"t1"}, {"tag": b"nope"}, {"lower": picks[0], "upper": picks[1], "tag": b"t2"}]
    return forms


def level0(pairs):
    return pf.index_decode_host(stream_of(
        [OF.Index(p.decode(), t.decode(), []) for p, t in pairs]))


def test_reference_comment_prefix_case():
    """reader.go:117-119: "a", "ab", "abc", "b" with prefix "a" ends at "b"."""
    pairs = [(b"a", b"default"), (b"ab", b"default"), (b"abc", b"default"), (b"b", b"default")]
    got = pf.index_filter(level0(pairs), prefix=b"a").raw()
    assert [g["path"] for g in got] == [b"a", b"ab", b"abc"]
    assert flat_filter(pairs, prefix=b"a") == pairs[:3]
    got = pf.index_filter(level0(pairs), prefix=b"ab").raw()
    assert [g["path"] for g in got] == [b"ab", b"abc"]


@pytest.mark.parametrize("seed", range(4))
def test_filters_equal_the_flat_restatement(seed):
    rng = random.Random(seed)
    names = set()
    while len(names) < 60:
        names.add(("/" + "".join(rng.choice("ab/c") for _ in range(rng.randrange(1, 7)))).encode())
    pairs = []
    for p in sorted(names):
        for t in sorted(rng.sample([b"t1", b"t2", b"default"], rng.randrange(1, 3))):
            pairs.append((p, t))
    lst = level0(pairs)
    nonempty = 0
    for form in filter_forms(sorted(names), rng):
        got = [(g["path"], g["tag"]) for g in pf.index_filter(lst, **form).raw()]
        want = flat_filter(pairs, **form)
        assert got == want, form
        nonempty += bool(want) and len(want) < len(pairs)
    assert nonempty > 20  # the forms do select proper subsets


# ------------------------------------------------------------------ merge

def merge_restated(filesets):
    """MergeReader.iterate by sort and group.  filesets: [(deletive, additive)], each a list of
    (path, tag, data_refs)."""
    items = []
    for i, (dele, add) in enumerate(filesets):
        items += [(p, t, 2 * i, drs) for p, t, drs in dele]
        items += [(p, t, 2 * i + 1, drs) for p, t, drs in add]
    items.sort(key=lambda x: (x[0], x[1], x[2]))
    out, i = [], 0
    while i < len(items):
        j = i
        while j < len(items) and items[j][:2] == items[i][:2]:
            j += 1
        group = items[i:j]
        i = j
        if len(group) == 1:
            if group[0][2] % 2 == 1:
                out.append((group[0][0], group[0][1], group[0][3]))
            continue
        if group[-1][2] % 2 == 0:
            continue  # a delete in last place
        acc = []
        for _, _, s, drs in group:
            acc = [] if s % 2 == 0 else acc + drs
        out.append((group[0][0], group[0][1], acc))
    return out


def random_filesets(rng, n):
    """n filesets of a random Put/Delete sequence: per fileset the sorted deletive and additive
    (path, tag, data_refs) lists a Buffer would serialize."""
    paths = [("/d%d/f%d" % (rng.randrange(3), k)).encode() for k in range(8)]
    tags = [b"default", b"t1", b"t2"]
    out = []
    for _ in range(n):
        add, dele = {}, set()
        for _ in range(rng.randrange(2, 14)):
            key = (rng.choice(paths), rng.choice(tags))
            if rng.random() < 0.35:
                add.pop(key, None)
                dele.add(key)
            else:
                if rng.random() < 0.6:  # Put without append: a delete first
                    dele.add(key)
                    add.pop(key, None)
                add.setdefault(key, []).extend(_dr(rng) for _ in range(rng.randrange(0, 3)))
        out.append((sorted((p, t, []) for p, t in dele), sorted((p, t, d) for (p, t), d in add.items())))
    return out


@pytest.mark.parametrize("seed", range(12))
def test_merge_equals_sort_and_group(seed):
    rng = random.Random(100 + seed)
    n = 1 + seed % 4
    filesets = random_filesets(rng, n)
    if seed % 3 == 0:  # a delete in last place of a group that earlier filesets put
        key = filesets[0][1][0][:2] if filesets[0][1] else (b"/d0/f0", b"default")
        dele = sorted(set((p, t) for p, t, _ in filesets[-1][0]) | {key})
        add = [x for x in filesets[-1][1] if x[:2] != key]
        filesets[-1] = ([(p, t, []) for p, t in dele], add)
        filesets.insert(0, ([], [(key[0], key[1], [_dr(rng)])]))
    pairs = []
    for dele, add in filesets:
        mk = lambda xs: pf.index_decode_host(stream_of(
            [OF.Index(p.decode(), t.decode(), drs) for p, t, drs in xs])) if xs else None
        pairs.append((mk(dele), mk(add)))
    got = [(g["path"], g["tag"], [_drt(d) for d in g["data_refs"]], g["size_bytes"])
           for g in pf.index_merge(pairs).raw()]
    want = [(p, t, [_drt(d) for d in drs], sum(d.size_bytes for d in drs))
            for p, t, drs in merge_restated(filesets)]
    assert got == want
    if seed % 3 == 0:
        assert key not in [(p, t) for p, t, _, _ in got]


def test_merge_of_nothing_and_of_one_list():
    assert len(pf.index_merge([])) == 0
    assert len(pf.index_merge([(None, None)])) == 0
    rng = random.Random(2)
    xs = [OF.Index("/a", "default", [_dr(rng)]), OF.Index("/a", "t", []), OF.Index("/b", "default", [])]
    one = pf.index_decode_host(stream_of(xs))
    assert got_of(pf.index_merge([(None, one)])) == [want_of(x) for x in xs]
    assert len(pf.index_merge([(one, None)])) == 0
    # put, then delete and put again in a later fileset: only the later DataRefs stay
    later = pf.index_decode_host(stream_of([OF.Index("/a", "default", [_dr(rng), _dr(rng)])]))
    dele = pf.index_decode_host(stream_of([OF.Index("/a", "default", [])]))
    got = got_of(pf.index_merge([(None, one), (dele, later)]))
    assert [g["path"] for g in got] == [b"/a", b"/a", b"/b"]
    assert got[0]["data_refs"] == got_of(later)[0]["data_refs"]
    # appended in a later fileset (no delete): the DataRefs concatenate
    got = got_of(pf.index_merge([(None, one), (None, later)]))
    assert got[0]["data_refs"] == got_of(one)[0]["data_refs"] + got_of(later)[0]["data_refs"]
