"""Compaction, the host side (no GPU): pfscdc_index_merge_deletive against a sort-and-group
restatement of MergeReader.iterateDeletive (merge.go:79-94), pfscdc_shard against a literal
restatement of shard (shard.go:27-49), and both in a stand-alone program built with
-fsanitize=address,undefined around index_merge.cpp and index_decode.cpp themselves."""
import os
import random
import subprocess

import pytest

from oracle import fileset as OF
from pfs_amd import fileset as pf
from test_index_read_cpu import _dr, _ref, got_of, random_filesets, stream_of, want_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mk(xs):
    """An index list of (path, tag, data_refs) triples (bytes paths), None for none."""
    return pf.index_decode_host(stream_of(
        [OF.Index(p.decode(), t.decode(), drs) for p, t, drs in xs])) if xs else None


def deletive_restated(lists):
    """iterateDeletive by sort and group: per (path, tag) the lowest fileset's entry."""
    items = sorted(((p, t, i, drs) for i, xs in enumerate(lists) for p, t, drs in xs),
                   key=lambda x: x[:3])
    out = []
    for x in items:
        if not out or out[-1][:2] != x[:2]:
            out.append((x[0], x[1], x[3]))
    return out


@pytest.mark.parametrize("seed", range(10))
def test_deletive_merge_equals_sort_and_group(seed):
    rng = random.Random(500 + seed)
    n = seed % 5  # none, one and several filesets
    lists = [dele for dele, _ in random_filesets(rng, n)]
    if n >= 2:  # a key every fileset shares, and NULL lists among them
        lists = [sorted(set(map(lambda x: x[:2], xs)) | {(b"/d1/shared", b"t1")}) for xs in lists]
        lists = [[(p, t, []) for p, t in xs] for xs in lists]
        if seed % 2:
            lists[1] = []
    pairs = [(mk(xs), None) for xs in lists]
    got = [(g["path"], g["tag"]) for g in pf.index_merge(pairs, deletive=True).raw()]
    want = [(p, t) for p, t, _ in deletive_restated(lists)]
    assert got == want
    if n >= 2:
        assert got.count((b"/d1/shared", b"t1")) == 1


def test_deletive_merge_yields_the_first_entry_as_it_is():
    """The group's first entry keeps its DataRefs, its Range and its chunk_ref; the additive
    lists of the pairs play no part."""
    rng = random.Random(9)
    a = [OF.Index("/a", "t", [_dr(rng), _dr(rng)], (7, "/a-last", _ref(rng))),
         OF.Index("/b", "", []), OF.Index("/c", "t", [_dr(rng)])]
    b = [OF.Index("/a", "t", [_dr(rng)]), OF.Index("/b", "", [_dr(rng)]),
         OF.Index("/b", "u", []), OF.Index("/d", None, [], (1, "/d-last", _ref(rng)))]
    la, lb = pf.index_decode_host(stream_of(a)), pf.index_decode_host(stream_of(b))
    got = got_of(pf.index_merge([(la, lb), (None, la), (lb, None)], deletive=True))
    assert got == [want_of(x) for x in (a[0], a[1], b[2], a[2], b[3])]
    assert len(pf.index_merge([], deletive=True)) == 0
    assert len(pf.index_merge([(None, la)], deletive=True)) == 0


# ------------------------------------------------------------------ shard

def shard_restated(files, threshold):
    """shard.go:27-49, line by line.  files: [(path, size)]."""
    out = []
    size, lower, upper = 0, "", ""
    for path, sz in files:
        if size >= threshold:
            out.append((lower, upper))
            lower, upper = path, ""
            size = 0
        upper = path
        size += sz
    out.append((lower, ""))
    return out


def sized(rng, path, tag, size):
    return OF.Index(path, tag, [_dr(rng, size=size)] if size else [])


@pytest.mark.parametrize("seed", range(6))
def test_shard_equals_the_restatement(seed):
    rng = random.Random(700 + seed)
    entries = [sized(rng, "/f%03d" % i, "default", rng.choice([0, 1, 100, 5000]))
               for i in range(rng.randrange(1, 40))]
    files = [(e.path, sum(d.size_bytes for d in e.data_refs)) for e in entries]
    lst = pf.index_decode_host(stream_of(entries))
    total = sum(s for _, s in files)
    for threshold in (0, 1, files[0][1], 100, 5000, 5001, total, total + 1):
        assert pf.shard(lst, threshold) == shard_restated(files, threshold), threshold
    assert pf.shard(lst, total + 1) == [("", "")]
    if len(files) > 1:  # threshold 0: one range in front of every file
        assert len(pf.shard(lst, 0)) == len(files) + 1


def test_shard_of_the_empty_list_and_of_tags_across_a_border():
    assert pf.shard(pf.index_decode_host(b""), 10) == [("", "")]
    assert pf.shard(None, 0) == [("", "")]
    rng = random.Random(3)
    # /b has two tags and the border falls between them: /b closes one range and opens the next
    entries = [sized(rng, "/a", "t", 10), sized(rng, "/b", "t1", 10), sized(rng, "/b", "t2", 10),
               sized(rng, "/c", "t", 10)]
    lst = pf.index_decode_host(stream_of(entries))
    assert pf.shard(lst, 20) == [("", "/b"), ("/b", "")]
    assert pf.shard(lst, 20) == shard_restated([(e.path, 10) for e in entries], 20)


# ------------------------------------------------------------------ under the host sanitizers

def test_merge_and_shard_under_host_sanitizers(tmp_path):
    """index_merge.cpp and index_decode.cpp compiled into a stand-alone program with
    AddressSanitizer and UBSan; its merged list and shards equal the restatements."""
    rng = random.Random(21)
    lists = []
    for k in range(3):
        xs = [sized(rng, "/f%02d" % i, t, rng.choice([0, 3, 50]))
              for i in range(12) for t in ("a", "b") if rng.random() < 0.5]
        xs.append(OF.Index("/zz%d" % k, "t", [_dr(rng, size=7) for _ in range(5)],
                           (5, "/zz-last", _ref(rng))))
        lists.append(xs)
    args = []
    for k, xs in enumerate(lists):
        (tmp_path / ("s%d.bin" % k)).write_bytes(stream_of(xs))
        args.append(str(tmp_path / ("s%d.bin" % k)))
    args.insert(1, "-")  # a NULL list among them
    exe = str(tmp_path / "merge_host")
    csrc = os.path.join(ROOT, "pfs_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "merge_host.cpp"),
                    os.path.join(csrc, "index_merge.cpp"), os.path.join(csrc, "index_decode.cpp"),
                    "-o", exe], check=True)
    res = subprocess.run([exe, "60"] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    assert lines[-1] == "ok"
    keyed = [[(e.path, e.tag, e) for e in xs] for xs in lists]
    keyed.insert(1, [])
    want = deletive_restated(keyed)
    recs = lambda e: len(e.data_refs) + (1 if e.range is not None else 0)
    assert [l[2:].split("\t") for l in lines if l.startswith("e ")] == \
        [[p, t, str(recs(e))] for p, t, e in want]
    shards = [tuple(l[2:].split("\t")) for l in lines if l.startswith("s ")]
    files = [(p, sum(d.size_bytes for d in e.data_refs)) for p, _, e in want]
    assert shards == shard_restated(files, 60) + [("", "")]
    assert len(shards) > 3
