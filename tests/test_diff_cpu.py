"""DiffFile on the host (no GPU): pfscdc_diff_host, Differ.Iterate's two-pointer walk taken
literally, against the restatement in tests/diff_oracle.py, pair for pair; the predicate kind
PFSCDC_SRC_DIFF through pfscdc_source_host; and the same walk once more in a stand-alone program
built with -fsanitize=address,undefined around diff.cpp.  Every comparison is exact."""
import os
import random
import subprocess

import pytest

from oracle import fileset as OF
from pfs_amd import _lib
from pfs_amd import fileset as pf

import diff_oracle as DO
import source_cases as SC
import tree_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H = [DO.hash_of(k) for k in range(64)]


def rows(paths, tag="t", first=0):
    return [(p, tag, H[(first + k) % 64]) for k, p in enumerate(paths)]


def check(rng, ra, rb):
    la, ia, oa = DO.side(rng, ra)
    lb, ib, ob = DO.side(rng, rb)
    want = DO.diff(oa, ob)
    assert pf.diff_host(la, ia, lb, ib) == want
    return want


STRADDLE = sorted(["/a!x", "/a-c/d", "/a.x", "/a/b", "/a/c/d", "/a0", "/a/b!/d", "/a/b/c", "/a", "/ab",
                   "/a/c/e"], key=str.encode)


def test_both_sides_empty_or_null():
    assert pf.diff_host(None, [], None, []) == []
    empty = pf.index_decode_host(b"")
    assert pf.diff_host(empty, [], None, []) == []
    assert pf.diff_host(None, [], empty, []) == []
    rng = random.Random(1)
    r = rows(["/a", "/b"])
    assert check(rng, [], r) == [(None, 0), (None, 1)]  # the old commit is nil
    assert check(rng, r, []) == [(0, None), (1, None)]


def test_identical_sides_give_no_pairs():
    rng = random.Random(2)
    r = rows(STRADDLE)
    assert check(rng, r, r) == []


def test_disjoint_and_interleaved_sides():
    rng = random.Random(3)
    assert check(rng, rows(["/a", "/b"]), rows(["/c", "/d"])) == \
        [(0, None), (1, None), (None, 0), (None, 1)]
    assert check(rng, rows(["/c", "/d"]), rows(["/a", "/b"])) == \
        [(None, 0), (None, 1), (0, None), (1, None)]
    assert check(rng, rows(["/a", "/c", "/e"]), rows(["/b", "/d", "/f"])) == \
        [(0, None), (None, 0), (1, None), (None, 1), (2, None), (None, 2)]


def test_straddle_paths():
    """Siblings on both sides of '/' in byte order: every other path on each side, then the same
    paths with every third hash changed."""
    rng = random.Random(4)
    want = check(rng, rows(STRADDLE[0::2]), rows(STRADDLE[1::2]))
    assert len(want) == len(STRADDLE)
    b = [(p, t, DO.hash_of(1000 + k) if k % 3 == 0 else h) for k, (p, t, h) in enumerate(rows(STRADDLE))]
    want = check(rng, rows(STRADDLE), b)
    assert want == [(k, k) for k in range(0, len(STRADDLE), 3)]


def test_a_proper_prefix_comes_first():
    rng = random.Random(5)
    assert check(rng, rows(["/a", "/a/b"]), rows(["/a/b"], first=1)) == [(0, None)]
    assert check(rng, rows(["/ab"]), rows(["/a", "/ab", "/abc"], first=3)) == \
        [(None, 0), (0, 1), (None, 2)]


@pytest.mark.parametrize("nb", [1, 3])
def test_two_tags_of_one_path_pair_positionally(nb):
    """The tag is no part of the key: the k-th entry of a path meets the k-th of the other side,
    and the longer run's surplus follows alone."""
    rng = random.Random(6)
    a = [("/f", "x", H[0]), ("/f", "y", H[1]), ("/g", "", H[2])]
    b = [("/f", t, H[10 + k]) for k, t in enumerate(["w", "x", "y"][:nb])] + [("/g", "", H[2])]
    want = check(rng, a, b)
    assert want == ([(0, 0), (1, None)] if nb == 1 else [(0, 0), (1, 1), (None, 2)])
    same_first = [("/f", "w", H[0])] + b[1:]  # the pair of k = 0 is equal and not reported
    assert check(rng, a, same_first) == want[1:]


@pytest.mark.parametrize("byte", [0, 31])
def test_hashes_that_differ_in_one_byte(byte):
    rng = random.Random(7)
    h = bytearray(H[5])
    h[byte] ^= 0x80
    assert check(rng, [("/a", "t", H[5])], [("/a", "t", bytes(h))]) == [(0, 0)]
    assert check(rng, [("/a", "t", H[5])], [("/a", "t", H[5])]) == []


def test_unsorted_sides_are_walked_literally():
    rng = random.Random(8)
    a = rows(["/b", "/a", "/c"])
    b = rows(["/a", "/c", "/b"], first=7)
    want = check(rng, a, b)
    assert want == [(None, 0), (0, None), (1, None), (2, 1), (None, 2)]
    check(rng, b, a)


@pytest.mark.parametrize("block", range(6))
def test_random_trees_changed(block):
    """300 random trees; side b is side a with entries dropped, added and re-hashed."""
    rng = random.Random(700 + block)
    reported = 0
    for _ in range(50):
        ra = [(p, t, rng.randbytes(32)) for p, t, _ in SC.random_tree(rng)]
        rb = DO.changed(rng, ra)
        reported += len(check(rng, ra, rb))
        check(rng, rb, ra)
    assert reported


def test_infos_are_required_and_paths_checked():
    lib = _lib.load()
    rng = random.Random(9)
    la, ia, _ = DO.side(rng, rows(["/a"]))
    out, n = pf.C.POINTER(_lib.DiffPairC)(), pf.C.c_uint64()
    assert lib.pfscdc_diff_host(la._p, None, None, None, pf.C.byref(out), pf.C.byref(n)) == \
        _lib.PFSCDC_EINVAL
    assert not out and n.value == 0
    assert lib.pfscdc_diff_host(None, None, None, None, None, None) == _lib.PFSCDC_EINVAL


# ---- PFSCDC_SRC_DIFF: SUBTREE's predicate without NewErrOnEmpty

def test_src_diff_selects_as_subtree_and_never_errs_on_empty():
    rng = random.Random(10)
    for name in ("straddle", "two_tags", "explicit_dir", "chain12", "empty"):
        _, lst, _ = SC.build(rng, SC.hand_trees()[name])
        for arg in SC.ARGS + ("/d0/d1",):
            try:
                want = pf.source_host(lst, _lib.SRC_SUBTREE, arg)
            except KeyError:
                want = None
            res, infos = pf.source_host(lst, _lib.SRC_DIFF, arg)
            if want is None:  # a path that is not there: an empty side
                assert len(res) == 0 and infos == []
            else:
                assert SC.rows_of(res, infos) == SC.rows_of(*want)
    res, infos = pf.source_host(None, _lib.SRC_DIFF, "/nothing")
    assert len(res) == 0 and infos == []
    with pytest.raises(_lib.PfsCdcError) as ei:  # kind 9 stays unknown
        pf.source_host(None, 9, "/a")
    assert ei.value.code == _lib.PFSCDC_EINVAL


# ---- the walk in a stand-alone program under ASan and UBSan

def test_standalone_under_asan_and_ubsan(tmp_path):
    """tests/c/diff_host.cpp with diff.cpp and index_decode.cpp, no GPU library, under
    AddressSanitizer and UBSan: empty and NULL sides, the straddle paths, runs of one path,
    unsorted sides and random trees against the oracle; and the irregular tree of
    tests/tree_cases.py against its changed copy."""
    rng = random.Random(41)
    cases = [([], []), (rows(STRADDLE[0::2]), rows(STRADDLE[1::2])),
             (rows(STRADDLE), rows(STRADDLE, first=1)), (rows(STRADDLE), rows(STRADDLE)),
             ([("/f", t, H[k]) for k, t in enumerate("vwxyz")], [("/f", "a", H[9]), ("/f", "b", H[1])]),
             (rows(["/b", "/a", "/c"]), rows(["/a", "/c", "/b"], first=7)),
             ([], rows(["/a"])), (rows(["/a"]), [])]
    for _ in range(40):
        ra = [(p, t, rng.randbytes(32)) for p, t, _ in SC.random_tree(rng)]
        cases.append((ra, DO.changed(rng, ra)))
    jobs, wants = [], []
    for k, (ra, rb) in enumerate(cases):
        names = []
        for s, r in (("a", ra), ("b", rb)):
            if not r and k % 2 == 0:
                names += ["-", "-"]  # a NULL side
                continue
            _, _, idx = SC.build(rng, [(p, t, 0 if p.endswith("/") else 1) for p, t, _ in r])
            f, g = tmp_path / ("%s%d.bin" % (s, k)), tmp_path / ("%s%d.hash" % (s, k))
            f.write_bytes(b"".join(OF.frame(OF.encode_index(e)) for e in idx))
            g.write_bytes(b"".join(h for _, _, h in r))
            names += [str(f), str(g)]
        jobs.append("\t".join(names))
        wants.append(DO.diff([(p, h) for p, _, h in ra], [(p, h) for p, _, h in rb]))
    names = []
    for s, side in zip("ab", TC.diff_sides(70)):
        f, g = tmp_path / ("irregular_%s.bin" % s), tmp_path / ("irregular_%s.hash" % s)
        f.write_bytes(b"".join(OF.frame(OF.encode_index(e)) for e in side.idx))
        g.write_bytes(side.leaf)
        names += [str(f), str(g)]
    jobs.append("\t".join(names))
    wants.append(DO.diff(*([(p, h) for p, _, h in side.rows] for side in TC.diff_sides(70))))
    assert len(wants[-1]) > 1024
    (tmp_path / "jobs.txt").write_text("\n".join(jobs) + "\n")
    exe = str(tmp_path / "diff_host")
    csrc = os.path.join(ROOT, "pfs_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "diff_host.cpp"),
                    os.path.join(csrc, "diff.cpp"), os.path.join(csrc, "index_decode.cpp"),
                    "-o", exe], check=True)
    res = subprocess.run([exe, str(tmp_path / "jobs.txt")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    assert lines[-1] == "ok"
    got = []
    for l in lines[:-1]:
        if l.startswith("j "):
            assert l.split()[1] == "0"
            got.append([])
        else:
            _, a, b = l.split()
            got[-1].append((None if a == "-" else int(a), None if b == "-" else int(b)))
    assert got == wants
