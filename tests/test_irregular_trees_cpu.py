"""The irregular tree of tests/tree_cases.py on the host (no GPU): the shape facts the GPU tests
of tests/test_gpu_irregular_trees.py rely on, the two tile-edge shifts, and the four Python
oracles against the four host specifications over it (pfscdc_source_host for every kind,
PFSCDC_SRC_GLOB and PFSCDC_SRC_DIFF included, pfscdc_diff_host, pfscdc_copy_map_host), so that
what the device arms are held against there is itself held here.  Every comparison is exact.
The stand-alone sanitizer programs of test_source_cpu.py, test_glob_cpu.py, test_diff_cpu.py and
test_copy_cpu.py each run one job from this tree."""
from collections import Counter

import pytest

import copy_cases as CC
import diff_oracle as DO
import glob_oracle as GO
import source_cases as SC
import source_oracle as SO
import tree_cases as TC
from pfs_amd import _lib
from pfs_amd import fileset as pf
from test_glob_cpu import check as glob_check

SPINE = 70


@pytest.fixture(scope="module")
def tree():
    return TC.built(SPINE)


@pytest.fixture(scope="module")
def rows():
    return TC.oracle_all(SPINE)


# ------------------------------------------------------------------ the shape

def test_shape_facts(tree, rows):
    spec, entries, lst, _ = tree
    assert len(entries) == len(lst) > 3 * 1024 and len(rows) > 5 * 1024
    depth = [TC.depth_of(r[0]) for r in rows]
    assert max(depth) == SPINE + 1
    assert max(depth) == max(SO._b(e[0]).count(b"/") for e in entries)  # the deepest is a file
    dirs = Counter(d for d, r in zip(depth, rows) if r[3] == SO.DIR)
    level = Counter(depth)
    assert dirs[3] > 1024 and level[4] > 1024  # both columns of level 3's scan pass a tile edge
    paths = [r[0] for r in rows]
    at = paths.index(TC.BUSHES + "/")
    assert sum(1 for p in paths[at:] if p.startswith(TC.BUSHES + "/")) > 1024
    at = paths.index(TC.WIDE + "/")
    kids = [p for p in paths[at + 1:] if p.startswith(TC.WIDE + "/") and
            "/" not in p[len(TC.WIDE) + 1:].rstrip("/")]
    assert len(set(kids)) >= 1030
    longest = max(len(SO._b(r[0])) for r in rows if r[3] == SO.DIR)
    assert longest > 256
    assert {64 < n <= 128 for n in map(len, map(SO._b, paths))} == {False, True}
    assert max(len(e[3]) for e in entries) == 300
    assert max(Counter(e[0] for e in entries).values()) == 4  # four tags of one path
    assert sum(1 for p, _, _ in spec if p.endswith("/")) >= 5  # explicit directory entries
    assert any(p.startswith(TC.BUSH + "/sub/") for p in paths)
    assert not any(p.startswith(TC.NOT_THERE) for p in paths)


def test_bytes_above_0x80_sort_after_their_ascii_siblings(tree, rows):
    """In the list, in the output, and among the children of one directory: /a/a!/a-/w/é0001
    comes after every g-NNNN and /é/ after /ab/ and /z~/ (0xC3 > 0x7A)."""
    _, entries, _, _ = tree
    for paths in ([e[0] for e in entries], [r[0] for r in rows]):
        raw = [SO._b(p) for p in paths if p != "/"]
        assert raw == sorted(raw)
        high = [k for k, p in enumerate(raw) if p[1] >= 0x80]
        assert high and min(high) > max(k for k, p in enumerate(raw) if p[1] < 0x80)
        wide = [p[len(SO._b(TC.WIDE)) + 1:] for p in raw
                if p.startswith(SO._b(TC.WIDE) + b"/") and len(p) > len(SO._b(TC.WIDE)) + 1]
        first_high = next(k for k, p in enumerate(wide) if p[0] >= 0x80)
        assert 0 < first_high < len(wide) and all(p[0] >= 0x80 for p in wide[first_high:])
        assert any(p[0] == 0x67 for p in wide[:first_high])  # g-NNNN
    # a signed compare would order them the other way round
    assert sorted(raw, key=lambda p: [c - 256 if c >= 0x80 else c for c in p]) != raw


def test_tile_edge_shifts_are_found(rows):
    p_dir, p_tag, p_out = TC.shifts(SPINE)
    assert None not in (p_dir, p_tag, p_out) and max(p_dir, p_tag, p_out) < 64
    assert 0 < p_out  # ("/" does not move: the run lies behind the pads)
    side = TC.diff_sides(SPINE, p_out)[0].source
    assert side[1023][0] == side[1024][0] and side[1023][1] != side[1024][1]
    shifted = TC.oracle_all(SPINE, p_dir)
    assert len(shifted) == len(rows) + p_dir
    assert shifted[1023][2] is None and shifted[1023][3] == SO.DIR  # an inserted directory
    assert shifted[1024][0].startswith(shifted[1023][0])
    assert TC.depth_of(shifted[1024][0]) == TC.depth_of(shifted[1023][0]) + 1
    entries = TC.built(SPINE, p_tag)[1]
    assert entries[1023][0] == entries[1024][0] and entries[1023][1] != entries[1024][1]


# ------------------------------------------------------------------ oracle against host

def test_source_all_equals_the_host(tree, rows):
    _, entries, lst, _ = tree
    res, infos = pf.source_host(lst, SO.ALL, "")
    assert SC.rows_of(res, infos) == SC.rows_want(rows, entries)
    leaf = SC.leaf_of(len(entries))
    w = SC.check_against_oracle(entries, lst, SO.ALL, "", leaf)
    assert w[0] == "ok" and all(r[5] == leaf[r[2]] for r in w[1] if r[3] == SO.FILE)


@pytest.mark.parametrize("with_leaf", [False, True])
@pytest.mark.parametrize("kind", [SO.SUBTREE, SO.LIST, SO.GET])
def test_source_kinds_equal_the_host(tree, kind, with_leaf):
    _, entries, lst, _ = tree
    leaf = SC.leaf_of(len(entries)) if with_leaf else None
    seen = []
    for arg in TC.source_args(SPINE):
        w = SC.check_against_oracle(entries, lst, kind, arg, leaf)
        seen.append(w[0] if w[0] != "ok" else len(w[1]))
    # the wide directory, the bushes, one bush, the deepest directory, the root, nothing
    # (getFile takes the '!' of /a/a!/a-/w for a pattern and refuses it)
    assert seen[0] == "unsupported" if kind == SO.GET else seen[0] > 1030
    assert seen[1] > 1024 and 2 < seen[2] <= 10
    assert seen[3] == (1 if kind == SO.LIST else 2)
    assert seen[5] == (0 if kind == SO.LIST else "notfound")
    # LIST of "/" leaves out the root itself; GET of "/" selects it and with it everything
    assert seen[4] == len(TC.oracle_all(SPINE)) - (kind == SO.LIST)


@pytest.mark.parametrize("glob", TC.GLOBS)
def test_globs_equal_the_host(tree, glob):
    _, entries, lst, _ = tree
    w = glob_check(entries, lst, glob)
    assert w[0] == "ok" and any(r[6] & GO.MATCH for r in w[1])


def test_diff_equals_the_host():
    a, b = TC.diff_sides(SPINE)
    oa, ob = [(r[0], r[5]) for r in a.source], [(r[0], r[5]) for r in b.source]
    want = DO.diff(oa, ob)
    sides = []
    for s in (a, b):
        res, infos = pf.source_host(s.lst, _lib.SRC_DIFF, "", s.leaf)
        assert SC.rows_of(res, infos) == SC.rows_want(s.source, s.entries)
        sides += [res, infos]
    assert pf.diff_host(*sides) == want
    check_diff_facts(a, b, want)


def check_diff_facts(a, b, want):
    """More than 1,024 pairs of all three kinds; the spine's deepest file and its 71 ancestors
    changed; a pair whose members are not the first of their runs of equal paths."""
    both = [(i, j) for i, j in want if i is not None and j is not None]
    assert len(want) > 1024 and both
    assert any(j is None for _, j in want) and any(i is None for i, _ in want)
    changed = {a.source[i][0] for i, _ in both}
    spine = TC.spine_dirs(SPINE)
    assert {"/", spine[-1] + "/f"} | {d + "/" for d in spine} <= changed
    assert len({"/"} | {d + "/" for d in spine}) + 1 == SPINE + 2
    assert any(i and a.source[i - 1][0] == a.source[i][0] and b.source[j - 1][0] == b.source[j][0]
               for i, j in both)


@pytest.mark.parametrize("src,dst,tag", TC.copy_pairs(SPINE))
def test_copy_map_equals_the_host(tree, src, dst, tag):
    _, _, lst, _ = tree
    got = CC.rows(pf.copy_map_host(lst, src, dst, tag))
    assert got == CC.want_rows(lst, src, dst, tag)
    assert bool(got) == (src != TC.NOT_THERE)
    assert not any(r[0].endswith("/") for r in got)  # what the device arm takes: clean file paths
    if tag:
        assert {r[1] for r in got} == {tag}


def test_the_data_parallel_forms_equal_the_literal_ones(tree):
    _, entries, _, _ = tree
    paths = [e[0] for e in entries]
    stream = SO.dir_inserter(paths)
    assert SO.insert_by_prefix(paths) == stream
    assert SO.infos_by_depth(stream, entries) == SO.iterate(stream, entries)
    leaf = SC.leaf_of(len(entries))
    w = SO.source(entries, SO.SUBTREE, TC.BUSHES, leaf)
    sel = [(p, s) for p, _, s, *_ in w]
    assert SO.infos_by_depth(sel, entries, leaf) == [(r[4], r[5]) for r in w]
