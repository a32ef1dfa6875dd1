"""The Source on the host (no GPU): pfscdc_source_host, which takes dirInserter.Iterate's emit,
indexFilter.Iterate's dir state and source.Iterate's recursion literally, against the
independent restatement in tests/source_oracle.py: list and infos, every comparison exact.  The
data-parallel forms the kernels use (ancestors by the common prefix; children by depth inside a
contiguous subtree) are held against the literal ones here as well.  The same cases run once
more in a stand-alone program built with -fsanitize=address,undefined around source.cpp."""
import os
import random
import subprocess

import pytest

from oracle import fileset as OF
from pfs_amd import _lib
from pfs_amd import fileset as pf

import source_cases as SC
import source_oracle as SO
import tree_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(SC.hand_trees()))
def test_hand_trees_every_predicate(name):
    rng = random.Random(sum(map(ord, name)))
    entries, lst, _ = SC.build(rng, SC.hand_trees()[name])
    seen = set()
    for kind in SC.KINDS:
        for arg in SC.ARGS + ("/d0/d1", "/e", "/e/"):
            seen.add(SC.check_against_oracle(entries, lst, kind, arg)[0])
    assert "ok" in seen


def test_straddle_tree_order_and_children():
    """Siblings on both sides of '/' in byte order: /a!x sorts before /a/ and /a0 after it, and
    /a/b!/d before /a/b/; the directories land in front of their first entry."""
    rng = random.Random(1)
    entries, lst, _ = SC.build(rng, SC.hand_trees()["straddle"])
    res, infos = pf.source_host(lst, _lib.SRC_ALL)
    paths = [d["path"].decode() for d in res.raw()]
    assert paths == ["/", "/a", "/a!x", "/a-c/", "/a-c/d", "/a.x", "/a/", "/a/b", "/a/b!/",
                     "/a/b!/d", "/a/b/", "/a/b/c", "/a/c/", "/a/c/d", "/a/c/e", "/a0", "/ab"]
    assert paths == sorted(paths, key=str.encode)
    # LIST(/a): the file /a and the children of /a/, not /a/ itself and not /ab
    res, infos = pf.source_host(lst, _lib.SRC_LIST, "/a")
    kids = [d["path"].decode() for d, i in zip(res.raw(), infos) if i[3] & _lib.INFO_CHILD]
    assert kids == ["/a", "/a/b", "/a/b!/", "/a/b/", "/a/c/"]
    # GET(/a): the file /a and the directory /a/ with its subtree
    res, _ = pf.source_host(lst, _lib.SRC_GET, "/a")
    assert [d["path"].decode() for d in res.raw()] == \
        ["/a"] + [p for p in paths if p.startswith("/a/")]


@pytest.mark.parametrize("block", range(10))
def test_random_trees(block):
    """200 random trees, every predicate kind with arguments that hit files, directories, both
    and nothing; the prefix rule and the depth rule against the literal forms."""
    rng = random.Random(500 + block)
    for _ in range(20):
        spec = SC.random_tree(rng)
        entries, lst, _ = SC.build(rng, spec)
        paths = [e[0] for e in entries]
        assert SO.insert_by_prefix(paths) == SO.dir_inserter(paths)
        stream = SO.dir_inserter(paths)
        assert SO.infos_by_depth(stream, entries) == SO.iterate(stream, entries)
        args = ["", "/a", "/a/b", "/ab", "/zz"] + rng.sample(paths, min(3, len(paths)))
        for kind in SC.KINDS:
            for arg in args:
                w = SC.check_against_oracle(entries, lst, kind, arg)
                if w[0] == "ok" and kind != SO.ALL:  # the filtered stream too
                    sel = [(p, s) for p, _, s, *_ in w[1]]
                    assert SO.infos_by_depth(sel, entries) == [(r[4], r[5]) for r in w[1]]


@pytest.mark.parametrize("name", sorted(SC.host_only_trees()))
def test_lists_only_the_literal_form_takes(name):
    """Unsorted lists, unclean paths and a directory entry twice: the literal emit and the
    literal recursion, as the oracle's."""
    rng = random.Random(77)
    entries, lst, _ = SC.build(rng, SC.host_only_trees()[name])
    for kind in SC.KINDS:
        for arg in ("", "/a", "/x", "rel"):
            SC.check_against_oracle(entries, lst, kind, arg)


def test_caller_supplied_leaf_hashes():
    rng = random.Random(5)
    for spec in (SC.hand_trees()["straddle"], SC.hand_trees()["explicit_dir"], SC.random_tree(rng, 25)):
        entries, lst, _ = SC.build(rng, spec)
        leaf = SC.leaf_of(len(entries))
        for kind, arg in ((SO.ALL, ""), (SO.SUBTREE, "/a"), (SO.LIST, "/a"), (SO.GET, "/a")):
            w = SC.check_against_oracle(entries, lst, kind, arg, leaf)
            assert w[0] == "ok"
            files = [r for r in w[1] if r[3] == SO.FILE]
            assert files and all(r[5] == leaf[r[2]] for r in files)


def test_glob_bytes_are_unsupported_and_named():
    rng = random.Random(6)
    _, lst, _ = SC.build(rng, SC.hand_trees()["two_tags"])
    for ch in SO.GLOB_BYTES:
        glob = "/a/f" + ch
        with pytest.raises(_lib.PfsCdcError) as ei:
            pf.source_host(lst, _lib.SRC_GET, glob)
        assert ei.value.code == _lib.PFSCDC_EUNSUPPORTED and glob in str(ei.value)
        pf.source_host(lst, _lib.SRC_SUBTREE, "/a")  # only getFile takes a glob
    with pytest.raises(_lib.PfsCdcError) as ei:
        pf.source_host(lst, 9, "/a")
    assert ei.value.code == _lib.PFSCDC_EINVAL


def test_not_found_where_the_reference_errs():
    rng = random.Random(8)
    _, lst, _ = SC.build(rng, SC.hand_trees()["two_tags"])
    for kind, arg, err in ((SO.GET, "/nothing", True), (SO.SUBTREE, "/nothing", True),
                           (SO.GET, "/a/ff", True), (SO.LIST, "/nothing", False),
                           (SO.SUBTREE, "", False), (SO.ALL, "", False)):
        if err:
            with pytest.raises(KeyError):
                pf.source_host(lst, kind, arg)
        else:
            pf.source_host(lst, kind, arg)
    for kind, err in ((SO.ALL, False), (SO.LIST, False), (SO.SUBTREE, False), (SO.GET, True)):
        if err:  # getFile of "/" on an empty commit
            with pytest.raises(KeyError):
                pf.source_host(None, kind, "/")
        else:
            res, infos = pf.source_host(None, kind, "/")
            assert len(res) == 0 and infos == []


def test_a_range_entry_is_refused():
    rng = random.Random(9)
    ref = SC.dr(rng).ref
    lst = pf.index_decode_host(OF.frame(OF.encode_index(OF.Index("/a", None, [], (0, "/b", ref)))))
    with pytest.raises(_lib.PfsCdcError) as ei:
        pf.source_host(lst, _lib.SRC_ALL)
    assert ei.value.code == _lib.PFSCDC_EINVAL


def test_standalone_under_asan_and_ubsan(tmp_path):
    """tests/c/source_host.cpp with source.cpp and index_decode.cpp, no GPU library, under
    AddressSanitizer and UBSan: the hand trees, the host-only lists and random trees, every
    kind, with and without leaf hashes, against the oracle; and the irregular tree of
    tests/tree_cases.py, whose recursion is 71 directories deep."""
    rng = random.Random(31)
    trees = list(SC.hand_trees().values()) + list(SC.host_only_trees().values()) + \
        [SC.random_tree(rng) for _ in range(40)]
    jobs, wants = [], []
    for k, spec in enumerate(trees):
        entries, _, idx = SC.build(rng, spec)
        f = tmp_path / ("s%d.bin" % k)
        f.write_bytes(b"".join(OF.frame(OF.encode_index(e)) for e in idx))
        for kind in SC.KINDS:
            for arg in ("", "/a", "/a/b", "/ab", "/nothing", "/a*"):
                for with_leaf in (0, 1):
                    jobs.append("%s\t%d\t%d\t%s" % (f, kind, with_leaf, arg))
                    wants.append((entries, SC.want(entries, kind, arg,
                                                   SC.leaf_of(len(entries)) if with_leaf else None)))
    jobs.append("-\t%d\t0\t/" % SO.ALL)
    wants.append(([], ("ok", [])))
    _, entries, _, idx = TC.built(70)
    f = tmp_path / "irregular.bin"
    f.write_bytes(b"".join(OF.frame(OF.encode_index(e)) for e in idx))
    for kind, arg, with_leaf in ((SO.ALL, "", 0), (SO.SUBTREE, TC.BUSHES, 1), (SO.GET, "/a", 1)):
        jobs.append("%s\t%d\t%d\t%s" % (f, kind, with_leaf, arg))
        wants.append((entries, SC.want(entries, kind, arg,
                                       SC.leaf_of(len(entries)) if with_leaf else None)))
    (tmp_path / "jobs.txt").write_text("\n".join(jobs) + "\n")
    exe = str(tmp_path / "source_host")
    csrc = os.path.join(ROOT, "pfs_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "source_host.cpp"),
                    os.path.join(csrc, "source.cpp"), os.path.join(csrc, "index_decode.cpp"),
                    "-o", exe], check=True)
    res = subprocess.run([exe, str(tmp_path / "jobs.txt")], capture_output=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.decode("utf-8", "surrogateescape").splitlines()
    assert lines[-1] == "ok"
    got, cur = [], None
    for l in lines[:-1]:
        if l.startswith("j "):
            cur = [int(l[2:].split("\t")[0]), []]
            got.append(cur)
        else:
            cur[1].append(l[2:].split("\t"))
    assert len(got) == len(wants)
    codes = {"ok": 0, "notfound": _lib.PFSCDC_ENOTFOUND, "unsupported": _lib.PFSCDC_EUNSUPPORTED,
             "error": _lib.PFSCDC_EINVAL}
    for (rc, rows), (entries, w) in zip(got, wants):
        assert rc == codes[w[0]]
        if w[0] == "ok":
            assert [r[:6] + [r[7]] for r in rows] == \
                [[p, t, str(typ), str(size), h.hex(), str(flags),
                  str(len(entries[src][3]) if src is not None else 0)]
                 for p, t, src, typ, size, h, flags in w[1]]
