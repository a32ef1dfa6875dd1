"""GlobFile on the host (no GPU): the dialect's specification pfscdc_glob_match against the two
restatements of tests/glob_oracle.py and against the compiled position automaton simulated in
numpy; the reference's own pinned expectations (server_test.go, GlobFile / GlobFile2 / GlobFile3);
pfscdc_source_host with PFSCDC_SRC_GLOB against the oracle's literal pipeline; the two
equivalences the device arm rests on; the errors; and all of it once more in a stand-alone
program under -fsanitize=address,undefined.  Every comparison is exact."""
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import fileset as OF
from pfs_amd import _lib
from pfs_amd import fileset as pf

import glob_oracle as GO
import source_cases as SC
import source_oracle as SO
import tree_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ helpers

def simulate(prog, s: bytes) -> bool:
    """The automaton of pfscdc_debug_glob_program over ``s``, as the device runs it."""
    follow, accept = prog["follow"], prog["accept_byte"]
    T, acc = prog["first"], prog["nullable"]
    for c in s:
        S = T & int(accept[c])
        acc = (S & prog["last"]) != 0
        bits = np.array([S >> b & 1 for b in range(64)], dtype=bool)
        T = int(np.bitwise_or.reduce(follow[bits])) if bits.any() else 0
    return acc


def instance(rng, ast, alphabet=b"ab./") -> bytes:
    """A string the AST matches (classes permitting)."""
    out = b""
    for t in ast:
        if t[0] == "lit":
            out += bytes([t[1]])
        elif t[0] == "one":
            out += bytes([rng.choice(alphabet.replace(b"/", b""))])
        elif t[0] == "star":
            out += bytes(rng.choice(alphabet.replace(b"/", b"")) for _ in range(rng.randrange(3)))
        elif t[0] == "super":
            out += bytes(rng.choice(alphabet) for _ in range(rng.randrange(4)))
        elif t[0] == "class":
            out += bytes([rng.choice([b for b in alphabet if b in t[1]] or [0x61])])
        else:
            out += instance(rng, rng.choice(t[1]), alphabet)
    return out


def oracle_mf(glob: str):
    """(mf by the matcher, mf by the regex) of a cleaned glob that compiles."""
    ast = GO.parse(glob)

    def by_match(path):
        return (path == "/" and glob == "/") or GO.match(ast, path.rstrip("/"))

    def by_regex(path):
        return (path == "/" and glob == "/") or GO.match_regex(glob, path.rstrip("/"))
    return by_match, by_regex, ast


def table_tree():
    """GlobFile's tree: file{i}, dir1/file{i}, dir2/dir3/file{i}, i < 100."""
    spec = [(p % i, "default", [1]) for i in range(100)
            for p in ("/file%d", "/dir1/file%d", "/dir2/dir3/file%d")]
    return SC.by_key(spec)


def check(entries, lst, arg, leaf=None):
    """pfscdc_source_host(SRC_GLOB) against the oracle: the outcome, and every row."""
    try:
        want = ("ok", GO.source(entries, arg, leaf))
    except KeyError:
        want = ("notfound",)
    except GO.GlobError:
        want = ("error",)
    except GO.GlobUnsupported:
        want = ("unsupported",)
    except SO.StreamError:
        want = ("error",)
    got, _ = SC.got_host(lst, _lib.SRC_GLOB, arg, leaf)
    assert got[0] == want[0], (arg, got[0], want[0])
    if want[0] == "ok":
        assert got[1] == SC.rows_want(want[1], entries), arg
    return want


# ------------------------------------------------------------------ 1. the dialect

@pytest.mark.parametrize("block", range(4))
def test_matcher_regex_library_and_automaton_agree(block):
    rng = random.Random(4100 + block)
    hits = cases = 0
    for _ in range(150):
        arg = GO.random_glob(rng)  # (cleanPath is not idempotent: ".." -> "/.." -> "/")
        glob = SO.clean_path(arg)
        try:
            by_match, by_regex, ast = oracle_mf(glob)
        except GO.GlobError:  # cleanPath took a '..' through a brace
            with pytest.raises(_lib.PfsCdcError) as ei:
                pf.glob_match(arg, "/a")
            assert ei.value.code == _lib.PFSCDC_EINVAL
            continue
        prog = pf.glob_program(arg)
        assert prog["positions"] == GO.positions(ast)
        strings = [instance(rng, ast) for _ in range(3)] + \
            [bytes(rng.choice(b"ab./") for _ in range(rng.randrange(9))) for _ in range(3)] + [b"/"]
        for s in strings:
            if not s or b"\0" in s:
                continue
            path = s.decode()
            a = by_match(path)
            assert by_regex(path) == a, (glob, path)
            assert pf.glob_match(arg, path) == a, (glob, path)
            if glob != "/":
                assert simulate(prog, s.rstrip(b"/")) == a, (glob, path)
            hits += a
            cases += 1
    assert cases > 600 and hits * 5 > cases  # the strings hit often enough to mean something


def test_classes_ranges_escapes_and_bytes_above_0x80():
    for glob, path, want in [
            ("/[a-c]x", "/bx", True), ("/[a-c]x", "/dx", False), ("/[!a-c]x", "/dx", True),
            ("/[!x]b", "//b", True),  # a class can match '/'
            ("/a[/]b", "/a/b", True), ("/a?b", "/a/b", False), ("/a*b", "/a/b", False),
            ("/a**b", "/a/b", True), ("/a**b", "/ab", True), ("/***", "/a/b", True),
            ("/[a-]", "/-", True), ("/[-a]", "/-", True), ("/[a\\]]", "/]", True),
            ("/[\\!a]", "/!", True), ("/\\*", "/*", True), ("/\\*", "/a", False),
            ("/a,b", "/a,b", True), ("/{a,b}", "/a,b", False), ("/{a,}c", "/c", True),
            ("/{a,{b,}{,c}}d", "/d", True), ("/{a,{b,}{,c}}d", "/bcd", True),
            ("/{a,{b,}{,c}}d", "/abd", False), ("/{[,]}", "/,", True),
            ("/[\udc80-\udcff]", "/\udce9", True), ("/[\udc80-\udcff]", "/a", False),
            ("/[!\udc80-\udcff]", "/a", True), ("/*", "/", False), ("/", "/", True),
            ("", "/", True), ("/**", "/", False), ("a", "/a/", True), ("/a/", "/a", True)]:
        by_match, by_regex, _ = oracle_mf(SO.clean_path(glob))
        assert by_match(path) == want and by_regex(path) == want, (glob, path)
        assert pf.glob_match(glob, path) == want, (glob, path)
        prog = pf.glob_program(glob)
        if SO.clean_path(glob) != "/":
            assert simulate(prog, GO._b(path).rstrip(b"/")) == want, (glob, path)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_the_automaton_at_its_width(n):
    """n positions: '/', then '?' and '*' and literals up to n.  64 fill the mask; 65 leave no
    program, which is no error."""
    glob = "/" if n == 1 else "/" + "?" * 20 + "*" + "a" * (n - 22)
    prog = pf.glob_program(glob)
    assert prog["positions"] == n
    if n > 64:
        assert not prog["follow"].any() and not prog["accept_byte"].any()
        assert pf.glob_match(glob, "/" + "b" * 20 + "a" * (n - 22))
        return
    if n == 1:
        assert prog["last"] == 1 and simulate(prog, b"/") and not simulate(prog, b"/a")
        return
    assert prog["last"] == 1 << (n - 1)
    for path in ("/" + "b" * 20 + "a" * (n - 22), "/" + "b" * 20 + "xyz" + "a" * (n - 22),
                 "/" + "b" * 20 + "a" * (n - 21), "/" + "b" * 20 + "a" * (n - 23),
                 "/" + "b" * 19 + "/" + "a" * (n - 22), "/" + "b" * 20 + "x/" + "a" * (n - 22)):
        assert simulate(prog, path.encode()) == pf.glob_match(glob, path), path
    assert simulate(prog, ("/" + "b" * 20 + "a" * (n - 22)).encode())


def test_literal_prefix():
    for glob in ("/a/b*", "/a/b", "*", "/a[b]", "/a\\*b", "/x{a,b}", "a/b/c?", "/a]b", "/q!", ""):
        assert pf.glob_literal_prefix(glob) == GO.literal_prefix(SO.clean_path(glob)), glob
    assert pf.glob_literal_prefix("/a/b*") == "/a/b" and pf.glob_literal_prefix("/a\\*b") == "/a\\"


# ------------------------------------------------------------------ 2. the pinned expectations

@pytest.fixture(scope="module")
def table():
    rng = random.Random(3094)
    entries, lst, _ = SC.build(rng, table_tree())
    return entries, lst


def files_of(rows):
    return [r for r in rows if r[2] == SO.FILE]


@pytest.mark.parametrize("pattern,count", [("*", 102), ("file*", 100), ("dir1/*", 100),
                                           ("dir2/dir3/*", 100), ("*/*", 101)])
def test_reference_glob_file_counts(table, pattern, count):
    entries, lst = table
    w = check(entries, lst, pattern)
    res, infos = pf.source_host(lst, _lib.SRC_GLOB, pattern)
    assert sum(1 for i in infos if i[3] & _lib.INFO_MATCH) == count
    assert len(GO.glob_file(entries, pattern)) == count
    assert w[0] == "ok"


@pytest.mark.parametrize("pattern,files", [("*", 300), ("dir2/dir3/file1?", 10), ("**file1?", 30),
                                           ("**file1", 3), ("dir?", 200), ("", 300)])
def test_reference_get_file_counts(table, pattern, files):
    entries, lst = table
    assert check(entries, lst, pattern)[0] == "ok"
    rows = SC.rows_of(*pf.source_host(lst, _lib.SRC_GLOB, pattern))
    assert len(files_of(rows)) == files
    if pattern == "**file1":  # one of each content
        assert sorted(r[0] for r in files_of(rows)) == ["/dir1/file1", "/dir2/dir3/file1", "/file1"]


def test_reference_get_file_garbage_is_not_found(table):
    entries, lst = table
    assert check(entries, lst, "garbage") == ("notfound",)
    with pytest.raises(KeyError) as ei:
        pf.source_host(lst, _lib.SRC_GLOB, "garbage")
    assert "/garbage" in str(ei.value)
    assert GO.glob_file(entries, "garbage") == []


def matched_paths(lst, pattern):
    res, infos = pf.source_host(lst, _lib.SRC_GLOB, pattern)
    return [d["path"].decode() for d, i in zip(res.raw(), infos) if i[3] & _lib.INFO_MATCH]


def test_reference_glob_file_2_and_3():
    rng = random.Random(3201)
    names = ["/%d" % i for i in range(100)]
    entries, lst, _ = SC.build(rng, SC.by_key([(p, "default", [len(p)]) for p in names]))
    check(entries, lst, "/1*")
    assert sorted(matched_paths(lst, "/1*")) == sorted(p for p in names if p.startswith("/1"))
    entries, lst, _ = SC.build(rng, [(p, "default", 0) for p in
                                     ("/dir1/file1.1", "/dir1/file1.2", "/dir2/file2.1",
                                      "/dir2/file2.2")])
    for pattern, want in (("**.2", ["/dir1/file1.2", "/dir2/file2.2"]),
                          ("/dir1/*", ["/dir1/file1.1", "/dir1/file1.2"]),
                          ("/*", ["/dir1/", "/dir2/"]), ("/", ["/"])):
        check(entries, lst, pattern)
        assert matched_paths(lst, pattern) == want, pattern
    # GlobFile's last check: "**" over an empty commit reports nothing (and getFile errs)
    assert GO.glob_file([], "**") == []
    with pytest.raises(KeyError):
        pf.source_host(None, _lib.SRC_GLOB, "**")


# ------------------------------------------------------------------ 3. against the literal pipeline

HAND_GLOBS = ("/{a,b/f*}", "/a*", "/a/*", "/a/**", "/**", "/*/*", "/a/b", "/a", "/", "", "/a?",
              "/[!x]*", "/**/d", "/a/c{,/*}", "/d0/**/leaf", "/*/f", "/e", "**c**", "/nothing*")


@pytest.mark.parametrize("name", sorted(SC.hand_trees()))
def test_hand_trees(name):
    rng = random.Random(sum(map(ord, name)))
    entries, lst, _ = SC.build(rng, SC.hand_trees()[name])
    seen = {check(entries, lst, g)[0] for g in HAND_GLOBS}
    assert "ok" in seen or name == "empty"
    leaf = SC.leaf_of(len(entries))
    for g in ("/a*", "/**", "/"):
        check(entries, lst, g, leaf)


def test_orphans_nested_matches_and_a_file_inside_a_matched_directory():
    rng = random.Random(37)
    spec = SC.by_key([(p, "t", 1) for p in ("/a/1", "/a/2", "/b/f1", "/b/f2", "/b/g", "/c/f1/x",
                                            "/c/f1/y", "/c/h")])
    entries, lst, _ = SC.build(rng, spec)
    # the stream holds /a/, /a/1, /a/2 and the orphans /b/f1, /b/f2: no "/" and no /b/
    w = check(entries, lst, "/{a,b/f*}")
    assert [r[0] for r in w[1]] == ["/a/", "/a/1", "/a/2", "/b/f1", "/b/f2"]
    assert [r[0] for r in w[1] if r[6] & GO.MATCH] == ["/a/", "/b/f1", "/b/f2"]
    # orphans beside another directory's children of the same depth
    w = check(entries, lst, "/{a,b/f*,c/f1}")
    assert [r[0] for r in w[1]][-3:] == ["/c/f1/", "/c/f1/x", "/c/f1/y"]
    # a matched directory and a matched file inside it; nested matched directories
    w = check(entries, lst, "/{a,a/1}")
    assert [(r[0], r[6]) for r in w[1]] == [("/a/", 2), ("/a/1", 2), ("/a/2", 0)]
    w = check(entries, lst, "/{c,c/f1,c/f1/x}")
    assert [r[0] for r in w[1] if r[6] & GO.MATCH] == ["/c/", "/c/f1/", "/c/f1/x"]
    assert len(w[1]) == 5
    w = check(entries, lst, "/**")  # everything but "/", each matched itself
    assert len(w[1]) == len(entries) + 4 and all(r[6] & GO.MATCH for r in w[1])
    w = check(entries, lst, "")
    assert [r[0] for r in w[1] if r[6] & GO.MATCH] == ["/"] and len(w[1]) == len(entries) + 5


@pytest.mark.parametrize("name", sorted(SC.host_only_trees()))
def test_unordered_and_unclean_lists_take_the_literal_filter(name):
    """Where the filter's dir state shows: /b matched as a directory... or not, by list order."""
    rng = random.Random(77)
    entries, lst, _ = SC.build(rng, SC.host_only_trees()[name])
    for g in ("/a*", "/*", "/**", "/a/*", "/{a,b}", "/", "/x", "rel", "/?"):
        check(entries, lst, g)


@pytest.mark.parametrize("block", range(6))
def test_random_trees_and_globs(block):
    rng = random.Random(7300 + block)
    selected = cases = 0
    for _ in range(25):
        entries, lst, _ = SC.build(rng, SC.random_tree(rng))
        leaf = SC.leaf_of(len(entries)) if rng.random() < 0.3 else None
        for _ in range(4):
            w = check(entries, lst, GO.random_glob(rng), leaf)
            cases += 1
            selected += w[0] == "ok"
    assert cases == 100 and selected * 3 >= cases, (selected, cases)


# ------------------------------------------------------------------ 4. the equivalences

@pytest.mark.parametrize("block", range(4))
def test_stateless_form_and_with_prefix_change_nothing(block):
    rng = random.Random(9100 + block)
    ok = 0
    for _ in range(40):
        spec = [e for e in SC.random_tree(rng) if not e[0].endswith("/") or rng.random() < 0.5]
        entries, _, _ = SC.build(rng, spec)
        for _ in range(4):
            g = GO.random_glob(rng)
            try:
                want = GO.source(entries, g)
            except (KeyError, GO.GlobError):
                want = None
            for kw in ({"stateless": True}, {"with_prefix": True}):
                if "with_prefix" in kw and "\\" in GO.literal_prefix(SO.clean_path(g)):
                    continue  # (the test below)
                try:
                    got = GO.source(entries, g, **kw)
                except (KeyError, GO.GlobError):
                    got = None
                assert got == want, (g, kw)
            ok += want is not None
    assert ok >= 40


def test_with_prefix_defeats_an_escape_ahead_of_the_first_glob_byte():
    """globRegex does not know the backslash, so globLiteralPrefix("/\\b*") is "/\\b", which no
    path the glob matches starts with: the reference's open would select nothing.  The library
    applies no WithPrefix and serves what the glob matches."""
    rng = random.Random(12)
    entries, lst, _ = SC.build(rng, [("/b1", "t", 1), ("/c", "t", 1)])
    assert GO.literal_prefix("/\\b*") == "/\\b" == pf.glob_literal_prefix("/\\b*")
    with pytest.raises(KeyError):
        GO.source(entries, "/\\b*", with_prefix=True)
    w = check(entries, lst, "/\\b*")
    assert [r[0] for r in w[1]] == ["/b1"]


# ------------------------------------------------------------------ 5. errors

INVALID = [("/a]", 2), ("/a}b", 2), ("/a[bc", 2), ("/a{b,c", 2), ("/a{b,{c}", 2), ("/a\\", 2),
           ("/[]", 1), ("/[!]", 1), ("/[b-a]", 2), ("/a[b\\", 4), ("/{a,b]}", 5), ("/ab[a-", 3)]


def test_compile_errors_name_the_glob_and_the_offset():
    rng = random.Random(6)
    _, lst, _ = SC.build(rng, SC.hand_trees()["two_tags"])
    for glob, offset in INVALID:
        with pytest.raises(GO.GlobError) as oe:
            GO.parse(glob)
        assert oe.value.offset == offset, glob
        for call in (lambda: pf.source_host(lst, _lib.SRC_GLOB, glob),
                     lambda: pf.glob_match(glob, "/a"), lambda: pf.glob_program(glob)):
            with pytest.raises(_lib.PfsCdcError) as ei:
                call()
            assert ei.value.code == _lib.PFSCDC_EINVAL, glob
            assert glob in str(ei.value) and "at byte %d" % offset in str(ei.value), str(ei.value)


def test_extglob_is_unsupported_and_named():
    rng = random.Random(6)
    _, lst, _ = SC.build(rng, SC.hand_trees()["two_tags"])
    for ch in "!()@+^":
        glob = "/a/f" + ch + "x"
        with pytest.raises(GO.GlobUnsupported):
            GO.parse(glob)
        for call in (lambda: pf.source_host(lst, _lib.SRC_GLOB, glob),
                     lambda: pf.glob_match(glob, "/a")):
            with pytest.raises(_lib.PfsCdcError) as ei:
                call()
            assert ei.value.code == _lib.PFSCDC_EUNSUPPORTED and glob in str(ei.value)
        assert pf.glob_match("/a/f\\" + ch + "x", glob)  # escaped: itself
        assert pf.glob_match("/a/f[x" + ch + "]x", glob)  # in a class: a member
    assert pf.glob_match("/[!a]", "/b") and not pf.glob_match("/[!a]", "/a")
    # the first from the left decides
    with pytest.raises(_lib.PfsCdcError) as ei:
        pf.glob_match("/a(b]", "/a")
    assert ei.value.code == _lib.PFSCDC_EUNSUPPORTED
    with pytest.raises(_lib.PfsCdcError) as ei:
        pf.glob_match("/a]b(", "/a")
    assert ei.value.code == _lib.PFSCDC_EINVAL


def test_get_with_a_pattern_and_kind_9_are_as_before():
    rng = random.Random(6)
    _, lst, _ = SC.build(rng, SC.hand_trees()["two_tags"])
    for ch in SO.GLOB_BYTES:
        with pytest.raises(_lib.PfsCdcError) as ei:
            pf.source_host(lst, _lib.SRC_GET, "/a/f" + ch)
        assert ei.value.code == _lib.PFSCDC_EUNSUPPORTED
    with pytest.raises(_lib.PfsCdcError) as ei:
        pf.source_host(lst, 9, "/a")
    assert ei.value.code == _lib.PFSCDC_EINVAL
    assert (_lib.SRC_GLOB, _lib.INFO_MATCH) == (5, 2)
    import pfs_amd
    assert pfs_amd.glob_match("/a*", "/ab") and pfs_amd.SRC_GLOB == 5 and pfs_amd.INFO_MATCH == 2


# ------------------------------------------------------------------ 6. under the sanitizers

def test_standalone_under_asan_and_ubsan(tmp_path, table):
    """tests/c/glob_host.cpp with glob.cpp, source.cpp and index_decode.cpp, no GPU library,
    under AddressSanitizer and UBSan: the table, hand and random trees, the error cases, match
    jobs and the automaton at 1, 63, 64 and 65 positions; and two globs over the irregular tree
    of tests/tree_cases.py, whose deepest path has 71 '/'."""
    rng = random.Random(41)
    trees = [table_tree()] + list(SC.hand_trees().values()) + list(SC.host_only_trees().values()) + \
        [SC.random_tree(rng) for _ in range(20)]
    table_globs = ("*", "file*", "dir1/*", "dir2/dir3/*", "*/*", "dir2/dir3/file1?", "**file1?",
                   "**file1", "dir?", "", "garbage")
    jobs, wants = [], []
    for k, spec in enumerate(trees):
        entries, _, idx = SC.build(rng, spec)
        f = tmp_path / ("s%d.bin" % k)
        f.write_bytes(b"".join(OF.frame(OF.encode_index(e)) for e in idx))
        globs = table_globs if k == 0 else HAND_GLOBS[:8] + tuple(GO.random_glob(rng) for _ in range(4))
        for g in globs + tuple(x for x, _ in INVALID[:4]) + ("/a(b",):
            if "\t" in g or "\n" in g:
                continue
            jobs.append("s\t%s\t%d\t%s" % (f, _lib.SRC_GLOB, g))
            try:
                wants.append(("j", entries, ("ok", GO.source(entries, g))))
            except KeyError:
                wants.append(("j", entries, ("notfound",)))
            except (GO.GlobError, SO.StreamError):
                wants.append(("j", entries, ("error",)))
            except GO.GlobUnsupported:
                wants.append(("j", entries, ("unsupported",)))
    jobs.append("s\t-\t%d\t/**" % _lib.SRC_GLOB)
    wants.append(("j", [], ("notfound",)))
    _, entries, _, idx = TC.built(70)
    f = tmp_path / "irregular.bin"
    f.write_bytes(b"".join(OF.frame(OF.encode_index(e)) for e in idx))
    for g in ("/**/f", "/{a,b}/**0"):
        jobs.append("s\t%s\t%d\t%s" % (f, _lib.SRC_GLOB, g))
        wants.append(("j", entries, ("ok", GO.source(entries, g))))
    for _ in range(200):
        arg = GO.random_glob(rng)
        glob = SO.clean_path(arg)
        try:
            by_match, _, ast = oracle_mf(glob)
        except GO.GlobError:
            continue
        path = (instance(rng, ast) if rng.random() < 0.5 else
                bytes(rng.choice(b"ab./") for _ in range(rng.randrange(1, 9)))).decode()
        if not path:
            continue
        jobs.append("m\t%s\t%s" % (arg, path))
        wants.append(("m", by_match(path)))
    for n in (1, 63, 64, 65):
        glob = "/" if n == 1 else "/" + "?" * 20 + "*" + "a" * (n - 22)
        jobs.append("p\t" + glob)
        wants.append(("p", n, GO.literal_prefix(glob), GO.match(GO.parse(glob), GO.literal_prefix(glob))))
    (tmp_path / "jobs.txt").write_text("\n".join(jobs) + "\n")
    exe = str(tmp_path / "glob_host")
    csrc = os.path.join(ROOT, "pfs_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "glob_host.cpp"),
                    os.path.join(csrc, "glob.cpp"), os.path.join(csrc, "source.cpp"),
                    os.path.join(csrc, "index_decode.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe, str(tmp_path / "jobs.txt")], capture_output=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.decode("utf-8", "surrogateescape").splitlines()
    assert lines[-1] == "ok"
    got = []
    for l in lines[:-1]:
        if l[0] == "e":
            got[-1][2].append(l[2:].split("\t"))
        else:
            got.append([l[0], l[2:].split("\t"), []])
    assert len(got) == len(wants)
    codes = {"ok": 0, "notfound": _lib.PFSCDC_ENOTFOUND, "unsupported": _lib.PFSCDC_EUNSUPPORTED,
             "error": _lib.PFSCDC_EINVAL}
    for (tag, head, rows), w in zip(got, wants):
        assert tag == w[0]
        if tag == "m":
            assert head[:2] == ["0", str(int(w[1]))]
        elif tag == "p":
            assert head == ["0", str(w[1]), "-1" if w[1] > 64 else str(int(w[3])), w[2]]
        else:
            entries, want = w[1], w[2]
            assert int(head[0]) == codes[want[0]]
            if want[0] == "ok":
                assert rows == [[p, t, str(typ), str(size), h.hex(), str(flags),
                                 str(len(entries[src][3]) if src is not None else 0)]
                                for p, t, src, typ, size, h, flags in want[1]]
