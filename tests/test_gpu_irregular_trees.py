"""The tree passes on the GPU over the irregular tree of tests/tree_cases.py: the Source
(src_* kernels and the level loop of source_dev.cpp at 72 levels), GlobFile (src_glob_kernel and
the passes that read its masks), DiffFile (diff_*) and CopyFile's map (cmap_*).  A few thousand
entries of which no two neighbours share common-prefix length, depth, name length and tag count,
with bytes >= 0x80, directory paths past 256 bytes, a level whose two scan columns pass 1,024 at
different entries and shifted copies that put a directory and its first child, or two tags of
one path, on both sides of a tile edge.  tests/test_irregular_trees_cpu.py asserts those shape
facts and holds the Python oracles against the host specifications over the same trees.

Each device arm is compared with its host specification array for array through the helpers of
the passes' own test files, the stats say which arm ran, and the results are held against the
Python oracle's rows as well.  Every comparison is exact."""
import functools

import pytest

import copy_cases as CC
import diff_oracle as DO
import glob_oracle as GO
import source_cases as SC
import source_oracle as SO
import tree_cases as TC
from pfs_amd import _lib
from pfs_amd import fileset as pf
from pfs_amd.cdc import ChunkParams, Chunker
from test_gpu_copy import both as copy_both
from test_gpu_diff import both as diff_both
from test_gpu_glob import MASK_GLOBS, both_and_oracle, want_mask
from test_gpu_source import both
from test_irregular_trees_cpu import check_diff_facts

pytestmark = pytest.mark.gpu

SPINE = 70
GLOB_SPINE = 62  # 63 '/' in the deepest path: the most src_glob_kernel takes


@pytest.fixture
def chunker():
    c = Chunker(ChunkParams(), 0)
    yield c
    c.close()


@pytest.fixture
def device_arm(knob):
    knob("PFSCDC_SOURCE", 1)


def grids(knob, grid):
    """PFSCDC_CHACHA_GRID and PFSCDC_HASH_GRID at one workgroup, or (0) at the shipped widths."""
    knob("PFSCDC_CHACHA_GRID", grid)
    knob("PFSCDC_HASH_GRID", grid)


# ------------------------------------------------------------------ the Source

@functools.lru_cache(maxsize=None)
def wanted(spine, shift, kind, arg, with_leaf):
    entries = TC.built(spine, shift)[1]
    return SC.want(entries, kind, arg, SC.leaf_of(len(entries)) if with_leaf else None)


def source_case(chunker, spine, shift, kind, arg, with_leaf, dev=None):
    """One call through ``both`` (device arm against host arm), then against the oracle's rows
    and the stats the oracle's rows imply."""
    _, entries, lst, _ = TC.built(spine, shift)
    leaf = b"".join(SC.leaf_of(len(entries))) if with_leaf else None
    res, st = both(chunker, lst, kind, arg, leaf=leaf, dev=dev)
    w = wanted(spine, shift, kind, arg, with_leaf)
    assert (res is None) == (w[0] != "ok"), (kind, arg, w[0])
    if res is None:
        return None
    # a list the count pass flags as unordered (a signed byte compare would) takes the host arm
    assert st["device"] == 1, (kind, arg, st)
    assert SC.rows_of(*res) == SC.rows_want(w[1], entries), (kind, arg)
    levels = max((TC.depth_of(r[0]) for r in w[1]), default=-1) + 1
    assert st["levels"] == levels, (kind, arg, st)
    assert st["hash_launches"] == (0 if not w[1] else levels if with_leaf else levels + 1)
    assert st["dirs_inserted"] == sum(1 for r in w[1] if r[2] is None), (kind, arg, st)
    return w[1]


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("with_leaf", [False, True])
@pytest.mark.parametrize("grid", [1, 0])
def test_source_every_kind(chunker, device_arm, knob, grid, with_leaf, resident):
    grids(knob, grid)
    lst = TC.built(SPINE)[2]
    dev = pf.DevIndexList.upload(chunker, lst) if resident else None
    rows = source_case(chunker, SPINE, 0, SO.ALL, "", with_leaf, dev)
    assert len(rows) > 5 * 1024
    st = pf.last_source_stats(chunker)
    assert st["levels"] == SPINE + 2
    assert st["hash_launches"] == SPINE + 2 + (not with_leaf)
    oks = 0
    for kind in (SO.SUBTREE, SO.LIST, SO.GET):
        for arg in TC.source_args(SPINE):
            oks += source_case(chunker, SPINE, 0, kind, arg, with_leaf, dev) is not None
    # GET refuses the '!' of the wide directory's path; SUBTREE and GET miss the absent path
    assert oks == 18 - 3
    if dev is not None:
        dev.free()


@pytest.mark.parametrize("which", ["directory", "tags"])
def test_source_with_a_tile_edge_inside(chunker, device_arm, which):
    """Output entry 1,023 an inserted directory and 1,024 its first child; input entries 1,023
    and 1,024 two tags of one path."""
    shift = TC.shifts(SPINE)[which == "tags"]
    rows = source_case(chunker, SPINE, shift, SO.ALL, "", False)
    if which == "directory":
        assert rows[1023][2] is None and rows[1024][0].startswith(rows[1023][0])
    else:
        entries = TC.built(SPINE, shift)[1]
        assert entries[1023][0] == entries[1024][0]


# ------------------------------------------------------------------ GlobFile

@functools.lru_cache(maxsize=None)
def wanted_masks(glob):
    memo = {}
    return [want_mask(glob, SO._b(e[0]), memo)[0] for e in TC.built(GLOB_SPINE)[1]]


@pytest.mark.parametrize("globs", ["mask_globs", "tree_globs"])
@pytest.mark.parametrize("grid", [1, 0])
def test_glob_masks_equal_the_specification_on_every_prefix(chunker, knob, grid, globs):
    knob("PFSCDC_CHACHA_GRID", grid)
    _, entries, lst, _ = TC.built(GLOB_SPINE)
    assert max(SO._b(e[0]).count(b"/") for e in entries) == 63
    dev = pf.DevIndexList.upload(chunker, lst)
    for glob in (MASK_GLOBS if globs == "mask_globs" else TC.GLOBS):
        masks, bad = pf.glob_masks(chunker, dev, glob)
        assert bad == 0, glob
        want = wanted_masks(glob)
        got = [int(m) for m in masks]
        assert got == want, (glob, next((entries[i][0], hex(g), hex(w))
                                        for i, (g, w) in enumerate(zip(got, want)) if g != w))
        if globs == "tree_globs":
            assert any(want), glob
    if globs == "tree_globs":  # the deepest directory's own bit
        assert any(m >> 62 & 1 for m in wanted_masks("/**"))
    dev.free()


@pytest.mark.parametrize("glob", TC.GLOBS)
def test_glob_source_equals_the_host_and_the_oracle(chunker, device_arm, glob):
    _, entries, lst, _ = TC.built(GLOB_SPINE)
    want, st = both_and_oracle(chunker, entries, lst, glob, arm=1)
    assert st["device"] == 1 and any(r[6] & GO.MATCH for r in want)


def test_glob_over_64_slashes_takes_the_host_arm(chunker, device_arm):
    _, entries, lst, _ = TC.built(SPINE)
    want, st = both_and_oracle(chunker, entries, lst, "/**/f", arm=0)
    assert st["device"] == 0
    assert sum(1 for r in want if r[6] & GO.MATCH) >= SPINE


# ------------------------------------------------------------------ DiffFile

def open_side(chunker, side):
    return pf.source_open(chunker, side.lst, _lib.SRC_DIFF, "", side.leaf)


def diff_case(chunker, knob, shift):
    a, b = TC.diff_sides(SPINE, shift)
    sa, sb = open_side(chunker, a), open_side(chunker, b)
    assert pf.last_source_stats(chunker)["device"] == 1
    want = diff_both(chunker, knob, sa, sb)
    assert want == DO.diff([(r[0], r[5]) for r in a.source], [(r[0], r[5]) for r in b.source])
    check_diff_facts(a, b, want)
    sa.free()
    sb.free()
    return a, b, want


@pytest.mark.parametrize("grid", [1, 0])
def test_diff_of_the_tree_and_its_changed_copy(chunker, device_arm, knob, grid):
    grids(knob, grid)
    diff_case(chunker, knob, 0)


@pytest.mark.parametrize("where", ["list", "source"])
def test_diff_with_a_tile_edge_inside_a_two_tag_run(chunker, device_arm, knob, where):
    """Entries 1,023 and 1,024 two tags of one path: of the list the side's Source is opened
    over, and of the Source itself, which is what the diff kernels read."""
    shift = TC.shifts(SPINE)[1 if where == "list" else 2]
    a, _, _ = diff_case(chunker, knob, shift)
    rows = a.rows if where == "list" else a.source
    assert rows[1023][0] == rows[1024][0]


# ------------------------------------------------------------------ CopyFile's map

@pytest.mark.parametrize("src,dst,tag", TC.copy_pairs(SPINE))
@pytest.mark.parametrize("grid", [1, 0])
def test_copy_map(chunker, knob, grid, src, dst, tag):
    grids(knob, grid)
    lst = TC.built(SPINE)[2]
    rows = copy_both(chunker, knob, lst, src, dst, tag)
    assert rows == CC.want_rows(lst, src, dst, tag)
    assert bool(rows) == (src != TC.NOT_THERE)
