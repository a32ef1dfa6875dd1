"""DiffFile on the GPU: pfscdc_source_diff against its specification pfscdc_diff_host over the
downloaded sides (the pairs), its two arms against each other array for array (both selections:
entries, blob, DataRefs, infos) with the stats saying which arm ran, and ``FileSet.diff_file`` end
to end against the two-pointer walk of tests/diff_oracle.py over ``walk_file``.  Every comparison
is exact.

The sides are hand-built lists (source_cases.build) opened with caller-supplied leaf hashes, so a
test chooses which files differ and needs no chunk store.  The diff kernels use the tiles of the
index kernels (256 lanes per workgroup, 1,024 per scan pass) and no other, so the entry counts are
those sizes and their neighbours."""
import ctypes as C
import os
import random
import subprocess

import pytest

import diff_oracle as DO
import source_cases as SC
from pfs_amd import _lib
from pfs_amd import fileset as pf
from pfs_amd.cdc import ChunkParams, Chunker
from test_gpu_index_read import LOOP_INDEX, model_ops, write
from test_gpu_merge import arrays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def chunker():
    c = Chunker(ChunkParams(), 0)
    yield c
    c.close()


def open_rows(chunker, rows, arg=""):
    """A Source over ``rows`` ([(path, tag, hash)] in list order), the hashes as leaf hashes."""
    rng = random.Random(len(rows))
    _, lst, _ = SC.build(rng, [(p, t, 0 if p.endswith("/") else 1) for p, t, _ in rows])
    leaf = b"".join(h for _, _, h in rows)
    return pf.source_open(chunker, lst if rows else None, _lib.SRC_DIFF, arg, leaf if rows else None)


def flat(ks, salt=0, changed=()):
    """Files /d/fKKKKK for k in ks; the hash of k depends on salt only for k in changed."""
    return [("/d/f%05d" % k, "t", DO.hash_of(1000003 * (salt if k in changed else 0) + k)) for k in ks]


def open_n(chunker, n, first=0, salt=0, changed=()):
    """A Source of exactly n entries: /d/ and n - 1 files of it; one file alone; nothing."""
    if n == 0:
        return open_rows(chunker, [])
    if n == 1:
        return open_rows(chunker, flat([first], salt, changed), "/d/f%05d" % first)
    src = open_rows(chunker, flat(range(first, first + n - 1), salt, changed), "/d")
    assert len(src) == n
    return src


def host_side(chunker, src):
    if src is None:
        return None, []
    return src.list.download(chunker), src.infos(chunker)


def selection_rows(lst, infos, picks):
    raw = lst.raw() if lst is not None else []
    return [(raw[i]["path"], raw[i]["tag"], [bytes(d.hash) for d in raw[i]["data_refs"]], infos[i])
            for i in picks]


def both(chunker, knob, a, b, arm=1):
    """pfscdc_source_diff over (a, b) with the knob at 1 and at 0: the pairs equal
    pfscdc_diff_host's over the downloaded sides, the selections hold the paired entries, the
    two arms' arrays are identical, the stats name the arm.  ``arm``: what the knob at 1 runs."""
    la, ia = host_side(chunker, a)
    lb, ib = host_side(chunker, b)
    want = pf.diff_host(la, ia, lb, ib)
    got = []
    for value in (1, 0):
        knob("PFSCDC_DIFF", value)
        d = pf.source_diff(chunker, a, b)
        st = pf.last_diff_stats(chunker)
        assert st["device"] == (arm if value else 0), st
        assert (st["entries_a"], st["entries_b"]) == (len(ia), len(ib))
        assert st["pairs"] == len(want) == len(d)
        assert st["both"] == sum(1 for i, j in want if i is not None and j is not None)
        assert d.pairs(chunker) == want
        sides = []
        for which, (lst, infos) in enumerate(((la, ia), (lb, ib))):
            s = d.side(which)
            picks = [p[which] for p in want if p[which] is not None]
            assert len(s) == len(picks)
            sl, si = s.list.download(chunker), s.infos(chunker)
            assert selection_rows(sl, si, range(len(picks))) == selection_rows(lst, infos, picks)
            sides.append((arrays(sl), si))
        got.append(sides)
        d.free()
    for which in (0, 1):
        dev, host = got[0][which], got[1][which]
        assert dev[0][0] == host[0][0], "entries"
        assert dev[0][1] == host[0][1], "blob"
        assert dev[0][2] == host[0][2], "DataRefs"
        assert dev[1] == host[1], "infos"
    return want


# ------------------------------------------------------------------ shapes

@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_entry_counts(chunker, knob, n):
    """Both sides of n entries: side b is side a shifted by one file with every fifth hash
    changed, so the first file is a's alone, the last b's alone and /d/ differs."""
    a = open_n(chunker, n)
    b = open_n(chunker, n, first=1 if n > 1 else 0, salt=1, changed=set(range(0, n + 1, 5)))
    assert len(a) == len(b) == n
    want = both(chunker, knob, a, b)
    if n > 2:
        assert want[0] == (0, 0) and want[1] == (1, None) and want[-1] == (None, n - 1)
    assert bool(want) == (n > 0)


@pytest.mark.parametrize("na,nb", [(1, 2049), (2049, 1), (1025, 300), (0, 257), (257, 0)])
def test_unequal_sides(chunker, knob, na, nb):
    a = open_n(chunker, na, first=40)
    b = open_n(chunker, nb, first=0 if nb > 1 else 40, salt=2, changed={40, 41, 250})
    assert (len(a), len(b)) == (na, nb)
    both(chunker, knob, a, b)


@pytest.mark.parametrize("n", [600, 2049])
def test_one_workgroup_makes_every_pass(chunker, knob, n):
    """PFSCDC_CHACHA_GRID=1: every grid-stride loop of the diff kernels makes three or more
    passes over each side (600 entries: 1,200 lanes of the rank and fill kernels)."""
    knob("PFSCDC_CHACHA_GRID", 1)
    a = open_n(chunker, n)
    b = open_n(chunker, n, first=3, salt=3, changed=set(range(0, n, 3)))
    both(chunker, knob, a, b)


@pytest.mark.parametrize("nb", [0, 2, 5, 7])
def test_a_run_of_five_equal_paths(chunker, knob, nb):
    """Five tags of /r against nb: the k-th meets the k-th, the surplus follows alone."""
    h = [DO.hash_of(k) for k in range(32)]
    a = [("/q", "t", h[0])] + [("/r", "t%d" % k, h[1 + k]) for k in range(5)] + [("/s", "t", h[7])]
    # b's run: tag u*, the hash of k = 1 equal to a's, the others not
    b = [("/q", "t", h[0])] + [("/r", "u%d" % k, h[2] if k == 1 else h[10 + k]) for k in range(nb)] + \
        [("/s", "t", h[7])]
    want = both(chunker, knob, open_rows(chunker, a), open_rows(chunker, b))
    # entries: "/", "/q", the run from 2 on, "/s"
    run = [(2 + k, 2 + k) for k in range(min(5, nb)) if k != 1] + \
        [(2 + k, None) for k in range(nb, 5)] + [(None, 2 + k) for k in range(5, nb)]
    assert want == [(0, 0)] + run  # "/" differs whenever the runs do


def test_300_byte_paths_that_differ_in_the_last_byte(chunker, knob):
    stem = "/" + "x" * 298
    h = [DO.hash_of(100 + k) for k in range(8)]
    a = [(stem + c, "t", h[k]) for k, c in enumerate("ace")]
    b = [(stem + c, "t", h[k]) for k, c in zip((3, 1, 4, 5), "bcde")]
    want = both(chunker, knob, open_rows(chunker, a), open_rows(chunker, b))
    # "/" differs; a, then b, c equal, d, e differs
    assert want == [(0, 0), (1, None), (None, 1), (None, 3), (3, 4)]


def test_one_leaf_at_depth_12_changes_every_ancestor(chunker, knob):
    (path, tag, _), = SC.hand_trees()["chain12"]
    a = open_rows(chunker, [(path, tag, DO.hash_of(1)), ("/z", "t", DO.hash_of(3))])
    b = open_rows(chunker, [(path, tag, DO.hash_of(2)), ("/z", "t", DO.hash_of(3))])
    want = both(chunker, knob, a, b)
    # "/", /d0/ ... /d0/.../d11/ and the leaf: 14 pairs with both members; /z is equal
    assert want == [(k, k) for k in range(14)] and len(a) == 15


def test_everything_changed_and_nothing_changed(chunker, knob):
    rng = random.Random(21)
    rows = [(p, t, rng.randbytes(32)) for p, t, _ in SC.random_tree(rng, 29) if not p.endswith("/")]
    a = open_rows(chunker, rows)
    assert both(chunker, knob, a, open_rows(chunker, rows)) == []
    b = open_rows(chunker, [(p, t, rng.randbytes(32)) for p, t, _ in rows])
    # every file's hash changed, and with it every directory's
    assert both(chunker, knob, a, b) == [(k, k) for k in range(len(a))]


@pytest.mark.parametrize("block", range(3))
def test_random_trees_changed(chunker, knob, block):
    rng = random.Random(800 + block)
    for _ in range(8):
        ra = [(p, t, rng.randbytes(32)) for p, t, _ in SC.random_tree(rng)]
        rb = DO.changed(rng, ra)
        a, b = open_rows(chunker, ra), open_rows(chunker, rb)
        both(chunker, knob, a, b)
        both(chunker, knob, b, a)
        sub = rng.choice(["/a", "/ab", "/a/b", "/nothing"])  # a path one side may lack
        both(chunker, knob, open_rows(chunker, ra, sub), open_rows(chunker, rb, sub))


# ------------------------------------------------------------------ arms and errors

def test_a_side_whose_paths_decrease_takes_the_host_arm(chunker, knob):
    """The Source of an unsorted list (the host arm's literal emit) is itself out of order: the
    rank kernel flags it and the walk is taken literally on the host."""
    rng = random.Random(77)
    _, lst, _ = SC.build(rng, SC.host_only_trees()["unsorted"])
    leaf = b"".join(SC.leaf_of(3))
    # listFile of the root is a predicate under which source.Iterate gets through this list
    bad = pf.source_open(chunker, lst, _lib.SRC_LIST, "", leaf)
    paths = [d["path"] for d in bad.list.download(chunker).raw()]
    assert paths != sorted(paths)
    good = open_rows(chunker, [("/a/x", "t", DO.hash_of(1)), ("/c", "t", DO.hash_of(2))])
    assert both(chunker, knob, bad, good, arm=0)
    assert both(chunker, knob, good, bad, arm=0)


def test_a_null_side_a_is_the_nil_commit(chunker, knob):
    b = open_n(chunker, 257)
    assert both(chunker, knob, None, b) == [(None, k) for k in range(257)]


def test_errors(chunker, knob):
    knob("PFSCDC_DIFF", 1)
    a = open_n(chunker, 3)
    lib = chunker.lib
    out = C.c_void_p(0xDEAD)
    assert lib.pfscdc_source_diff(chunker.ctx, a._p, None, C.byref(out)) == _lib.PFSCDC_EINVAL
    assert not out.value
    assert lib.pfscdc_source_diff(None, a._p, a._p, C.byref(out)) == _lib.PFSCDC_EINVAL
    assert lib.pfscdc_source_diff(chunker.ctx, a._p, a._p, None) == _lib.PFSCDC_EINVAL
    # a Source of another device: the handle's first member is its device number (one GPU here,
    # so the number is set by hand and put back)
    b = open_n(chunker, 3)
    dev = C.c_int.from_address(b._p.value)
    assert dev.value == 0
    for x, y in ((a, b), (b, a)):
        dev.value = 1
        out = C.c_void_p(0xDEAD)
        rc = lib.pfscdc_source_diff(chunker.ctx, x._p, y._p, C.byref(out))
        dev.value = 0
        assert rc == _lib.PFSCDC_EINVAL and not out.value
        assert b"another device" in lib.pfscdc_last_error(chunker.ctx)
    d = pf.source_diff(chunker, a, b)
    assert lib.pfscdc_diff_side(d._p, 2) is None and len(d) == 0
    d.free()


def test_a_selection_goes_through_the_tar_layout(chunker, knob):
    knob("PFSCDC_DIFF", 1)
    a = open_n(chunker, 300)
    b = open_n(chunker, 300, first=2, salt=5, changed=set(range(0, 300, 4)))
    d = pf.source_diff(chunker, a, b)
    assert pf.last_diff_stats(chunker)["device"] == 1
    for which in (0, 1):
        s = d.side(which)
        n = len(s)
        assert n > 70
        total, offs = C.c_uint64(), (C.c_uint64 * (n + 1))()
        rc = chunker.lib.pfscdc_dev_list_tar_layout(chunker.ctx, s.list._p, C.byref(total), offs)
        assert rc == _lib.PFSCDC_OK, chunker.lib.pfscdc_last_error(chunker.ctx)
        assert offs[0] == 0 and all(offs[k] + 512 <= offs[k + 1] for k in range(n))
        assert total.value >= offs[n]
    d.free()


# ------------------------------------------------------------------ end to end

def two_commits(threshold):
    """Two commits in one ChunkStore: 24-odd files of a few KB; in the second some are
    rewritten, some deleted, some added and one moved under a new directory."""
    ops, model = model_ops(5, 50)
    st, infos1, _ = write(ops, mem_threshold=threshold, index=LOOP_INDEX)
    rng = random.Random(6)
    new = dict(model)
    names = sorted(model)
    for p in names[0:len(names):4]:
        new[p] = bytes(rng.randbytes(len(model[p]) or 700))  # rewritten
    for p in names[1:len(names):5]:
        del new[p]  # deleted
    for k in range(3):
        new["/b/new%d" % k] = rng.randbytes(1500 + 900 * k)  # added
    moved = names[2]
    new["/moved/here" + moved] = new.pop(moved)
    w = st.new_unordered_writer()
    for p in sorted(new):
        w.put(p, "", False, new[p])
    infos2 = w.close()
    w.release()
    return st, infos1, infos2, model, new


def walk(fs, p):
    try:
        return fs.walk_file(p)
    except KeyError:
        return []  # diffFile wraps neither side in NewErrOnEmpty


def want_diff(old_rows, new_rows):
    return [(old_rows[i] if i is not None else None, new_rows[j] if j is not None else None)
            for i, j in DO.diff([(f.path, f.hash) for f in old_rows],
                                [(f.path, f.hash) for f in new_rows])]


@pytest.mark.parametrize("threshold", [10 ** 9, 12_000])
def test_diff_file_of_two_commits(knob, threshold):
    """``threshold`` 12,000 closes several filesets per commit, so the files' hashes are
    ``MergeFileReader.Hash`` (of the content): an untouched file is then in no pair."""
    knob("PFSCDC_DIFF", 1)
    st, infos1, infos2, model, new_model = two_commits(threshold)
    assert (len(infos1) > 1) == (len(infos2) > 1) == (threshold != 10 ** 9)
    old, new = st.open(infos1, resident=True), st.open(infos2, resident=True)
    moved = sorted(model)[2]
    some = sorted(set(model) & set(new_model))[3]
    for p in ("", "/", "/a", "/b/", some, moved, "/moved", "/nothing"):
        got = new.diff_file(old, p)
        assert got == want_diff(walk(old, p), walk(new, p)), p
    whole = new.diff_file(old)
    reported = {(o or n).path for o, n in whole}
    assert "/" in reported and moved in reported and "/moved/here" + moved in reported
    assert all(n is None for o, n in whole if o is not None and o.path not in new_model
               and not o.path.endswith("/"))
    if threshold != 10 ** 9:
        same = {p for p in model if new_model.get(p) == model[p]}
        assert same and not same & reported
    # the nil parent commit: every entry of the new one, alone
    assert new.diff_file(None) == [(None, fi) for fi in new.walk_file("")]
    # old_path: one directory of the old commit against another of the new one
    got = new.diff_file(old, "/b", old_path="/a")
    assert got == want_diff(walk(old, "/a"), walk(new, "/b")) and got


def test_plain_c_process_diffs_two_commits(tmp_path):
    exe = str(tmp_path / "diff_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "diff_consumer.c"),
                    "-L", libdir, "-lpfscdc", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=100)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    pairs = [l[2:].split("\t") for l in lines if l.startswith("p ")]
    by_path = {(a if a != "-" else b): (a, b) for a, b in pairs}
    assert by_path["/"] == ("/", "/")
    assert by_path["/d0/f03"] == ("/d0/f03", "/d0/f03")  # rewritten
    assert by_path["/d2/f05"] == ("/d2/f05", "-")  # deleted
    assert by_path["/d0/f12"] == ("-", "/d0/f12")  # added
    assert by_path["/d1/f07"] == ("/d1/f07", "-") and by_path["/new/f07"] == ("-", "/new/f07")
    assert by_path["/new/"] == ("-", "/new/")
    assert lines[-1].split() == ["ok", str(len(pairs)), "1"]
