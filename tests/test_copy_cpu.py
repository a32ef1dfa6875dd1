"""CopyFile's selection and path transform on the host (no GPU): pfscdc_copy_map_host, which
takes the open's options, NewIndexFilter's predicate and NewIndexMapper's transform literally,
against the independent restatement in tests/copy_oracle.py; every comparison exact.  The same
cases run once more in a stand-alone program built with -fsanitize=address,undefined around
copy_map.cpp."""
import ctypes as C
import os
import random
import subprocess

import pytest

from oracle import fileset as OF
from pfs_amd import _lib
from pfs_amd import fileset as pf

import copy_cases as CC
import copy_oracle as CPO
import source_cases as SC
import tree_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_path_functions():
    """cleanPath's own examples (paths.go:48-53) and the points where posixpath and Go differ."""
    for p, want in (("", "/"), ("abc", "/abc"), ("/abc", "/abc"), ("abc/", "/abc"), ("/", "/"),
                    ("//a//b/", "/a/b"), ("/a/../..", "/"), ("a/./b/../c", "/a/c"), (".", "/")):
        assert CPO.clean_path(p) == want
    assert CPO.go_clean("//a") == "/a" and CPO.go_clean("///a") == "/a"
    assert CPO.go_rel("/a", "/a") == "." and CPO.go_rel("/a", "/a/x/") == "x"
    assert CPO.go_rel("/a", "/a/../b") == "../b" and CPO.go_rel("/", "//x") == "x"
    assert CPO.go_join("/", "x") == "/x" and CPO.go_join("/z", ".") == "/z"
    assert CPO.go_join("/z", "../b") == "/b" and CPO.go_join("/", "../b") == "/b"


@pytest.mark.parametrize("name", sorted(CC.table()))
def test_case_table(name):
    spec, src, dst, tag, _ = CC.table()[name]
    lst, _ = CC.build(spec, sum(map(ord, name)))
    got = pf.copy_map_host(lst, src, dst, tag)
    assert CC.rows(got) == CC.want_rows(lst, src, dst, tag)


def test_the_table_selects_what_it_says():
    """The cases by name: two runs around /a.txt, one file, a tag, an unclean path as Go maps it."""
    t = CC.table()

    def paths(name):
        spec, src, dst, tag, _ = t[name]
        lst, _ = CC.build(spec, 1)
        return [(r[0], r[1]) for r in CC.rows(pf.copy_map_host(lst, src, dst, tag))]

    assert paths("neighbours") == [("/z", "t"), ("/z/x", "t"), ("/z/y/z", "t")]
    assert paths("cleaning") == paths("neighbours") == paths("cleaning_dots")
    assert paths("single_file") == [("/q/r", "t")]
    assert paths("single_file_to_root") == [("/", "t")]
    assert paths("dst_root") == [("/", "t"), ("/x", "t"), ("/y/z", "t")]
    assert paths("src_is_dst") == [("/a", "t"), ("/a/x", "t"), ("/a/y/z", "t")]
    assert paths("src_absent") == paths("src_below_all") == paths("empty") == []
    assert paths("src_tag_x") == [("/z/f", "x"), ("/z/g", "x")]
    assert paths("src_tag_y") == [("/f2", "y")]
    assert paths("src_tag_none") == []
    assert paths("two_tags_all") == [("/z/f", "x"), ("/z/f", "y"), ("/z/g", "x"), ("/z/g", "y")]
    assert paths("unclean_trailing") == [("/z/w", "t"), ("/z/x", "t"), ("/z/y", "t")]
    assert paths("unclean_dotdot") == [("/z/b", "t"), ("/z/y/c", "t")]  # Join(dst, "../b")
    assert paths("unclean_dotdot_root") == [("/b", "t"), ("/c", "t")]
    assert paths("unsorted") == []  # the open ends at /b: atEnd comes first
    assert [len(p) for p, _ in paths("long_path")] == [291 + 2, 291 + 298, 291 + 298]


def test_the_root_selects_nothing_from_a_clean_list():
    """driver_file.go:162-164: idx.Path == srcPath || HasPrefix(idx.Path, srcPath + "/").  With
    srcPath "/" that is path == "/" or HasPrefix(path, "//"): "/a" != "/" and no clean path
    starts with "//", so copying the root of a commit copies nothing.  The call is PFSCDC_OK with
    an empty list, as the reference's is; it is not widened to mean "everything"."""
    for spec in (SC.hand_trees()["straddle"], CC.random_list(random.Random(3), 50)):
        lst, _ = CC.build(spec)
        for src in ("/", "", ".", "//"):
            got = pf.copy_map_host(lst, src, "/z")
            assert len(got) == 0 and CC.arrays(got) == (b"", b"", b"")


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_random_lists(seed):
    rng = random.Random(seed)
    spec = CC.random_list(rng, 300)
    lst, _ = CC.build(spec, seed)
    paths = sorted({p for p, _, _ in spec})
    dirs = sorted({p.rsplit("/", 1)[0] for p in paths if p.count("/") > 1})
    hit = 0
    for src in ["/a0", "/ab1", "/nothing"] + rng.sample(paths, 5) + rng.sample(dirs, 8):
        for dst in ("/", "/z", "/a0/deep/er"):
            for tag in ("", "t", "u"):
                got = CC.rows(pf.copy_map_host(lst, src, dst, tag))
                assert got == CC.want_rows(lst, src, dst, tag)
                hit += bool(got)
    assert hit > 30


def test_null_list_and_null_strings():
    lib = _lib.load()
    out = C.c_void_p()
    assert lib.pfscdc_copy_map_host(None, b"/a", None, b"/z", C.byref(out)) == 0
    assert lib.pfscdc_index_list_count(out) == 0
    lib.pfscdc_index_list_free(out)
    lst, _ = CC.build(CC.table()["neighbours"][0])
    assert lib.pfscdc_copy_map_host(lst._p, None, None, None, C.byref(out)) == 0  # "/" to "/"
    assert lib.pfscdc_index_list_count(out) == 0
    lib.pfscdc_index_list_free(out)
    assert lib.pfscdc_copy_map_host(lst._p, b"/a", b"", b"/z", None) == _lib.PFSCDC_EINVAL
    assert len(pf.copy_map_host(None, "/a", "/z")) == 0


def test_the_result_is_a_list_of_its_own():
    """A fresh blob and packed DataRefs: the tar layout and an upload take it as it is."""
    lst, _ = CC.build(CC.table()["refs_0_1_300"][0])
    got = pf.copy_map_host(lst, "/a/r300", "/z")
    n, ents, blob, _, ndr = got._views()
    assert (n, ndr) == (1, 300) and ents[0].first == 0 and ents[0].count == 300
    assert blob == b"/z\0t\0\0"
    assert (ents[0].path_off, ents[0].tag_off, ents[0].last_path_off) == (0, 3, 5)
    files = got.lib.pfscdc_index_list_tar_files(got._p)
    assert (files[0].path, files[0].first, files[0].count) == (b"/z", 0, 300)


def malformed(which):
    """The neighbours list with one entry pointing outside the arrays."""
    lst, _ = CC.build(CC.table()["neighbours"][0])
    n, ents, blob, _, ndr = lst._views()
    e = ents[3]
    if which == "path_off":
        e.path_off = len(blob) + 1
    elif which == "path_len":
        e.path_len = len(blob)
    elif which == "tag_off":
        e.tag_off = len(blob) + 7
    elif which == "first":
        e.first = ndr + 1
    else:
        e.count = ndr + 1
    return lst


@pytest.mark.parametrize("which", ["path_off", "path_len", "tag_off", "first", "count"])
def test_entries_outside_the_arrays_are_refused(which):
    lst = malformed(which)
    lib = _lib.load()
    out = C.c_void_p(1)
    # whether or not the bad entry is selected
    for src in (b"/a", b"/nothing"):
        assert lib.pfscdc_copy_map_host(lst._p, src, None, b"/z", C.byref(out)) == _lib.PFSCDC_EINVAL
        assert not out.value


def test_a_range_entry_is_refused():
    rng = random.Random(9)
    ref = SC.dr(rng).ref
    lst = pf.index_decode_host(OF.frame(OF.encode_index(OF.Index("/a", None, [], (0, "/b", ref)))))
    with pytest.raises(_lib.PfsCdcError) as ei:
        pf.copy_map_host(lst, "/a", "/z")
    assert ei.value.code == _lib.PFSCDC_EINVAL


def test_standalone_under_asan_and_ubsan(tmp_path):
    """tests/c/copy_host.cpp with copy_map.cpp and index_decode.cpp, no GPU library, under
    AddressSanitizer and UBSan: the case table and a random list against the oracle; and /a of
    the irregular tree of tests/tree_cases.py copied into itself."""
    rng = random.Random(41)
    cases = [(n,) + CC.table()[n][:4] for n in sorted(CC.table())]
    rnd = CC.random_list(rng, 200)
    cases += [("random", rnd, src, dst, tag) for src in ("/a0", "/ab1/c2", "/", "/b3")
              for dst in ("/", "/z/y") for tag in ("", "u")]
    jobs, wants = [], []
    for k, (name, spec, src, dst, tag) in enumerate(cases):
        lst, idx = CC.build(spec, k)
        f = tmp_path / ("s%d.bin" % k)
        f.write_bytes(b"".join(OF.frame(OF.encode_index(e)) for e in idx))
        jobs.append("%s\t%s\t%s\t%s" % (f, src, tag, dst))
        wants.append(CC.want_rows(lst, src, dst, tag))
    jobs.append("-\t/a\t\t/z")
    wants.append([])
    _, _, lst, idx = TC.built(70)
    f = tmp_path / "irregular.bin"
    f.write_bytes(b"".join(OF.frame(OF.encode_index(e)) for e in idx))
    jobs.append("%s\t/a\t\t/a/a!" % f)
    wants.append(CC.want_rows(lst, "/a", "/a/a!"))
    assert len(wants[-1]) > 1024
    (tmp_path / "jobs.txt").write_text("\n".join(jobs) + "\n")
    exe = str(tmp_path / "copy_host")
    csrc = os.path.join(ROOT, "pfs_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "copy_host.cpp"),
                    os.path.join(csrc, "copy_map.cpp"), os.path.join(csrc, "index_decode.cpp"),
                    "-o", exe], check=True)
    res = subprocess.run([exe, str(tmp_path / "jobs.txt")], capture_output=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.decode("utf-8", "surrogateescape").splitlines()
    assert lines[-1] == "ok"
    got, cur = [], None
    for l in lines[:-1]:
        if l.startswith("j "):
            cur = [int(l[2:]), []]
            got.append(cur)
        else:
            cur[1].append(l[2:].split("\t"))
    assert len(got) == len(wants)
    for (rc, rws), w in zip(got, wants):
        assert rc == 0
        assert rws == [[p, t, str(size), str(len(drs)), drs[0][4].hex() if drs else "-"]
                       for p, t, size, _, drs in w]
