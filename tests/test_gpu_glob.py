"""GlobFile on the GPU: src_glob_kernel alone (pfscdc_debug_glob_masks) against the specification
pfscdc_glob_match on every prefix of every path; pfscdc_source_open with PFSCDC_SRC_GLOB against
pfscdc_source_host, array for array and info for info, with the stats saying which arm ran; the
hand-overs to the host arm; the errors; ``FileSet.get_file`` / ``glob_file`` end to end against
tests/glob_oracle.py and tests/tar_oracle.py; and a plain C process.  Every comparison is exact."""
import ctypes as C
import os
import random
import subprocess

import pytest

import glob_oracle as GO
import source_cases as SC
import source_oracle as SO
import tar_oracle as T
from pfs_amd import _lib
from pfs_amd import fileset as pf
from pfs_amd.cdc import ChunkParams, Chunker, synthetic_bytes
from test_gpu_index_read import LOOP_INDEX, write
from test_gpu_source import as_rows, both, model_rows, outcome

pytestmark = pytest.mark.gpu

TOO_DEEP = 32  # kSrcTooDeep


@pytest.fixture
def chunker():
    c = Chunker(ChunkParams(), 0)
    yield c
    c.close()


@pytest.fixture
def device_arm(knob):
    knob("PFSCDC_SOURCE", 1)


def wide(n):
    """A glob of n positions: '/', 20 '?', one '*' and literals."""
    return "/" + "?" * 20 + "*" + "a" * (n - 22)


def table_tree():
    spec = [(p % i, "default", [1]) for i in range(100)
            for p in ("/file%d", "/dir1/file%d", "/dir2/dir3/file%d")]
    return SC.by_key(spec)


# ------------------------------------------------------------------ 1. the kernel alone

def mask_paths():
    """3 x 256 + 17 paths: 0, 1, 62 and 63 '/', directories, the case builders' paths (the
    longest is chain12's), bytes above 0x80, paths that are a glob's literal prefix or its
    whole match at 63 and 64 positions."""
    rng = random.Random(785)
    paths = ["rel", "/", "/x", "/x/", "/" + "a/" * 61 + "f", "/" + "a/" * 62 + "f", "/" + "a/" * 62,
             "/éx", "/é/éx", "/a/b", "/ab", "/a!b", "/s03/f", "/s03/", "/s03", "/d",
             "/c", "/bcd", "/ccd", "/b/cd", "/xaxaxaxa", "/aaaa", "/a/a/a/a/x", "/xa/ya/za/wa",
             "/aaa/a", "/" + "b" * 20 + "a" * 41, "/" + "b" * 20 + "a" * 42,
             "/" + "b" * 20 + "xyz" + "a" * 42, "/" + "b" * 19 + "/" + "a" * 42,
             "/" + "b" * 20 + "a" * 42 + "/", "/" + "b" * 20 + "a" * 42 + "/t"]
    for spec in list(SC.hand_trees().values()) + [SC.sequence(300)]:
        paths += [e[0] for e in spec]
    while len(paths) < 3 * 256 + 17:
        paths += [e[0] for e in SC.random_tree(rng)]
    return paths[:3 * 256 + 17]


MASK_GLOBS = ("/", wide(63), wide(64), "/**a**a**a**a*", "/[é][é]x", "/[\udc80-\udcff]*/**",
              "/a[!x]b", "/{b,{c,}{,c}}*d", "/s03/f*", "/s0?/**", "/*/*", "/**", "/a*", "/**/leaf")


def want_mask(glob, path: bytes, memo):
    def hit(s):
        if s not in memo:
            memo[s] = pf.glob_match(glob, s.decode("utf-8", "surrogateescape"))
        return memo[s]
    mask = j = 0
    for k, c in enumerate(path):
        if c == 0x2F:
            if j < 63 and hit(path[:k]):
                mask |= 1 << j
            j += 1
    if path and path[-1] != 0x2F and hit(path):
        mask |= 1 << 63
    return mask, j


def test_masks_equal_the_specification_on_every_prefix(chunker, knob):
    """One workgroup (the grid knob at 1) over 785 entries: three full passes of the stride
    loop and a last partial block, the program staged once."""
    knob("PFSCDC_CHACHA_GRID", 1)
    rng = random.Random(1)
    paths = mask_paths()
    assert len(paths) == 3 * 256 + 17
    _, lst, _ = SC.build(rng, [(p, "t", 0) for p in paths])
    dev = pf.DevIndexList.upload(chunker, lst)
    raw = [p.encode("utf-8", "surrogateescape") for p in paths]
    assert sorted({p.count(b"/") for p in raw})[:2] == [0, 1] and max(p.count(b"/") for p in raw) == 63
    for glob in MASK_GLOBS:
        masks, bad = pf.glob_masks(chunker, dev, glob)
        assert bad == 0, glob
        memo, live = {}, 0
        for i, p in enumerate(raw):
            want, _ = want_mask(glob, p, memo)
            assert int(masks[i]) == want, (glob, p, hex(int(masks[i])), hex(want))
            live += want != 0
        assert live or glob == "/", glob  # every other glob selects something here
    # 64 '/' and more: the flag, and the masks of the other entries as before
    _, deep, _ = SC.build(rng, [("/" + "a/" * 63 + "f", "t", 0), ("/x", "t", 0),
                                ("/" + "a/" * 70, "t", 0)])
    masks, bad = pf.glob_masks(chunker, pf.DevIndexList.upload(chunker, deep), "/*")
    assert bad == TOO_DEEP and int(masks[1]) == 1 << 63
    with pytest.raises(_lib.PfsCdcError) as ei:
        pf.glob_masks(chunker, dev, wide(65))
    assert ei.value.code == _lib.PFSCDC_EUNSUPPORTED
    masks, bad = pf.glob_masks(chunker, pf.DevIndexList.upload(chunker, None), "/*")
    assert len(masks) == 0 and bad == 0


# ------------------------------------------------------------------ 2. the Source, both arms

def both_and_oracle(chunker, entries, lst, glob, arm=1, dev=None):
    res, st = both(chunker, lst, _lib.SRC_GLOB, glob, arm=arm, dev=dev)
    try:
        want = GO.source(entries, glob)
    except (KeyError, SO.StreamError):  # not found; source.Iterate's own error on an unclean list
        want = None
    assert (res is None) == (want is None), glob
    if want is not None:
        assert SC.rows_of(*res) == SC.rows_want(want, entries), glob
    return want, st


@pytest.fixture(scope="module")
def table():
    rng = random.Random(3094)
    entries, lst, _ = SC.build(rng, table_tree())
    return entries, lst


@pytest.mark.parametrize("grid", [0, 1])
def test_reference_table_both_arms(chunker, device_arm, knob, table, grid):
    knob("PFSCDC_CHACHA_GRID", grid)
    entries, lst = table
    dev = pf.DevIndexList.upload(chunker, lst)
    counts = {}
    for glob in ("*", "file*", "dir1/*", "dir2/dir3/*", "*/*", "dir2/dir3/file1?", "**file1?",
                 "**file1", "dir?", "", "garbage"):
        want, _ = both_and_oracle(chunker, entries, lst, glob, dev=dev)
        counts[glob] = None if want is None else \
            (sum(1 for r in want if r[6] & GO.MATCH), sum(1 for r in want if r[3] == SO.FILE))
    assert [counts[g][0] for g in ("*", "file*", "dir1/*", "dir2/dir3/*", "*/*")] == \
        [102, 100, 100, 100, 101]
    assert [counts[g][1] for g in ("*", "dir2/dir3/file1?", "**file1?", "**file1", "")] == \
        [300, 10, 30, 3, 300]
    assert counts["garbage"] is None and counts["dir?"] is not None


def test_orphans_nested_matches_and_three_levels(chunker, device_arm):
    rng = random.Random(37)
    spec = SC.by_key([(p, "t", 1) for p in ("/a/1", "/a/2", "/b/f1", "/b/f2", "/b/g", "/c/f1/x",
                                            "/c/f1/y", "/c/h", "/c/f1/z/w")])
    entries, lst, _ = SC.build(rng, spec)
    want, st = both_and_oracle(chunker, entries, lst, "/{a,b/f*}")
    assert [r[0] for r in want] == ["/a/", "/a/1", "/a/2", "/b/f1", "/b/f2"]
    assert st["dirs_inserted"] == 1
    # orphans at the depth of another directory's children
    both_and_oracle(chunker, entries, lst, "/{a,b/f*,c/f1}")
    both_and_oracle(chunker, entries, lst, "/{b/g,c/f1/z,a/2}")
    # a matched directory with a matched file inside; nested matched directories
    want, _ = both_and_oracle(chunker, entries, lst, "/{a,a/1}")
    assert [(r[0], r[6]) for r in want] == [("/a/", 2), ("/a/1", 2), ("/a/2", 0)]
    both_and_oracle(chunker, entries, lst, "/{c,c/f1,c/f1/x}")
    want, st = both_and_oracle(chunker, entries, lst, "/**")  # three levels deep
    assert len(want) == len(entries) + 5 and all(r[6] & GO.MATCH for r in want)
    want, _ = both_and_oracle(chunker, entries, lst, "/")
    assert [r[0] for r in want if r[6] & GO.MATCH] == ["/"] and len(want) == len(entries) + 6
    for glob in ("/*/f1", "/?/f*", "/[!a]/**", "/c/**/w", "/c/*", "/nothing*", "**1"):
        both_and_oracle(chunker, entries, lst, glob)


@pytest.mark.parametrize("name", sorted(SC.hand_trees()))
def test_hand_trees_equal_the_host(chunker, device_arm, name):
    rng = random.Random(sum(map(ord, name)))
    entries, lst, _ = SC.build(rng, SC.hand_trees()[name])
    dev = pf.DevIndexList.upload(chunker, lst)
    for glob in ("/{a,b/f*}", "/a*", "/a/*", "/a/**", "/**", "/*/*", "/a", "/", "/a?",
                 "/[!x]*", "/**/d", "/a/c{,/*}", "/d0/**/leaf", "**c**"):
        both_and_oracle(chunker, entries, lst, glob, dev=dev)


@pytest.mark.parametrize("block", range(2))
def test_random_trees_and_globs_equal_the_host(chunker, device_arm, block):
    rng = random.Random(8800 + block)
    oks = 0
    for _ in range(15):
        entries, lst, _ = SC.build(rng, SC.random_tree(rng))
        for _ in range(4):
            glob = GO.random_glob(rng)
            try:
                GO.parse(SO.clean_path(glob))
            except GO.GlobError:
                continue
            oks += both_and_oracle(chunker, entries, lst, glob)[0] is not None
    assert oks >= 15


# ------------------------------------------------------------------ 3. the hand-overs

def test_65_positions_and_64_slashes_take_the_host_arm(chunker, device_arm):
    rng = random.Random(65)
    hit = "/" + "b" * 20 + "a" * 43
    entries, lst, _ = SC.build(rng, SC.by_key([(hit, "t", 1), (hit + "/x", "t", 1), ("/x", "t", 2),
                                               (hit[:-1], "t", 1)]))
    want, st = both_and_oracle(chunker, entries, lst, wide(65), arm=0)
    assert [r[0] for r in want] == [hit, hit + "/", hit + "/x"] and st["device"] == 0
    want, st = both_and_oracle(chunker, entries, lst, wide(64) + "?", arm=0)
    assert [r[0] for r in want] == [hit, hit + "/", hit + "/x"] and st["device"] == 0
    want, st = both_and_oracle(chunker, entries, lst, wide(64), arm=1)  # 64 still run on the device
    # ('*' takes the 43rd 'a')
    assert [r[0] for r in want] == [hit[:-1], hit, hit + "/", hit + "/x"] and st["device"] == 1
    deep = "/" + "a/" * 63 + "f"
    entries, lst, _ = SC.build(rng, SC.by_key([(deep, "t", 1), ("/x", "t", 1)]))
    assert deep.count("/") == 64
    want, st = both_and_oracle(chunker, entries, lst, "/**/f", arm=0)
    assert [r[0] for r in want] == [deep] and st["device"] == 0
    both_and_oracle(chunker, entries, lst, "/?", arm=0)  # the depth decides, whatever matches
    both_and_oracle(chunker, entries, lst, "/", arm=1)  # "/" runs no automaton
    entries, lst, _ = SC.build(rng, SC.by_key([(deep[:-3] + "f", "t", 1), ("/x", "t", 1)]))
    both_and_oracle(chunker, entries, lst, "/**/f", arm=1)  # 63 '/' stay on the device


@pytest.mark.parametrize("name", sorted(SC.host_only_trees()))
def test_lists_the_device_refuses(chunker, device_arm, name):
    rng = random.Random(77)
    entries, lst, _ = SC.build(rng, SC.host_only_trees()[name])
    for glob in ("/a*", "/*", "/**", "/{a,b}", "/"):
        both_and_oracle(chunker, entries, lst, glob, arm=0)


# ------------------------------------------------------------------ 4. errors

def test_errors_equal_the_hosts_and_write_nothing(chunker, device_arm):
    rng = random.Random(6)
    _, lst, _ = SC.build(rng, SC.hand_trees()["two_tags"])
    dev = pf.DevIndexList.upload(chunker, lst)
    lib = chunker.lib
    cases = [("/a[bc", _lib.PFSCDC_EINVAL), ("/a}", _lib.PFSCDC_EINVAL), ("/a\\", _lib.PFSCDC_EINVAL),
             ("/a/f@(x)", _lib.PFSCDC_EUNSUPPORTED), ("/a/!f", _lib.PFSCDC_EUNSUPPORTED),
             ("/nothing*", _lib.PFSCDC_ENOTFOUND), ("/a/f/*", _lib.PFSCDC_ENOTFOUND)]
    for glob, code in cases:
        out = C.c_void_p(0xDEAD)
        rc = lib.pfscdc_source_open(chunker.ctx, dev._p, _lib.SRC_GLOB, glob.encode(), None, 0,
                                    C.byref(out))
        assert rc == code and not out.value, (glob, rc)
        text = lib.pfscdc_last_error(chunker.ctx).decode()
        host = outcome(lambda: pf.source_host(lst, _lib.SRC_GLOB, glob))
        assert host[1] == code and text and text in host[2]
        assert SO.clean_path(glob) in text
    out = C.c_void_p(0xDEAD)
    empty = pf.DevIndexList.upload(chunker, None)
    assert lib.pfscdc_source_open(chunker.ctx, empty._p, _lib.SRC_GLOB, b"/", None, 0,
                                  C.byref(out)) == _lib.PFSCDC_ENOTFOUND and not out.value
    # SRC_GET with a pattern is what it was
    assert lib.pfscdc_source_open(chunker.ctx, dev._p, _lib.SRC_GET, b"/a/*", None, 0,
                                  C.byref(out)) == _lib.PFSCDC_EUNSUPPORTED and not out.value


# ------------------------------------------------------------------ 5. end to end

def commit_ops():
    data = synthetic_bytes([0, 200_000], 9).tobytes()
    names = ["/d%d/f%02d" % (k % 3, k) for k in range(24)] + ["/d1/sub/f15", "/e/f10", "/top"]
    ops, model, pos = [], {}, 0
    for k, p in enumerate(names):
        size = (0, 1, 511, 512, 513, 3000, 9000)[k % 7]
        model[p] = data[pos:pos + size]
        ops.append(("put", p, "", False, model[p]))
        pos += size
    return ops, model


@pytest.mark.parametrize("resident", [False, True])
def test_get_file_and_glob_file_against_the_oracle(device_arm, resident):
    ops, model = commit_ops()
    st, infos, _ = write(ops, mem_threshold=10 ** 9, index=LOOP_INDEX)
    fs = st.open(infos, resident=resident)
    entries, leaf = model_rows(fs, len(infos))
    for glob in ("/d*/f1?", "/d1", "/d?/sub/**", "/top"):
        g = GO.source(entries, glob, leaf) if glob != "/d1" and glob != "/top" else \
            SO.source(entries, SO.GET, glob, leaf)
        tar = fs.get_file(glob)
        assert tar.read() == T.stream([(r[0], model[r[0]] if r[3] == SO.FILE else b"") for r in g])
    hit = [r[0] for r in GO.source(entries, "/d*/f1?", leaf)]
    assert "/d1/f10" in hit and "/e/f10" not in hit and "/d1/sub/f15" not in hit
    for glob in ("*", "/d*/f1?", "/d1/**", "**/f1[05]", "/", "", "/d{0,1/sub}", "/nothing*"):
        want = GO.glob_file(entries, glob, leaf)
        assert as_rows(fs.glob_file(glob)) == [(p, t, typ, size, h) for p, t, _, typ, size, h, _ in want]
    assert [i.path for i in fs.glob_file("*")] == ["/d0/", "/d1/", "/d2/", "/e/", "/top"]
    d1 = [i for i in fs.glob_file("*") if i.path == "/d1/"][0]
    assert d1.size == sum(len(v) for p, v in model.items() if p.startswith("/d1/"))
    assert fs.glob_file("/nothing*") == []
    with pytest.raises(KeyError):
        fs.get_file("garbage*")
    with pytest.raises(_lib.PfsCdcError) as ei:
        fs.glob_file("/d[")
    assert ei.value.code == _lib.PFSCDC_EINVAL
    empty = st.open(infos, prefix="/no/such/", resident=resident)
    assert empty.glob_file("*") == [] and empty.glob_file("**") == [] and empty.glob_file("/") == []
    with pytest.raises(KeyError):
        empty.get_file("*")


# ------------------------------------------------------------------ 6. a plain C process

def test_plain_c_process_globs(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "glob_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror",
                    "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "c", "glob_consumer.c"),
                    "-L", libdir, "-lpfscdc", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    out = str(tmp_path / "out.tar")
    glob = "/top/d[12]/{f1?,deep}"
    res = subprocess.run([exe, glob, out], capture_output=True, text=True, timeout=100)
    assert res.returncode == 0, res.stdout + res.stderr

    def path_of(k):
        return "/top/d1/deep/f07" if k == 7 else "/f11" if k == 11 else "/top/d%d/f%02d" % (k % 3, k)
    model = {path_of(k): bytes((k + j) & 0xFF for j in range(k * 997 + 13)) for k in range(24)}
    lines = res.stdout.splitlines()
    got = [l[2:].split("\t") for l in lines if l.startswith("i ")]
    # the files' hashes are the process's own; everything else follows from them
    leaf_by_path = {p: bytes.fromhex(h) for p, t, _, h, _ in got if int(t) == SO.FILE}
    paths = sorted(model, key=str.encode)
    entries = [(p, "default", len(model[p]), []) for p in paths]
    want = GO.source(entries, glob, [leaf_by_path.get(p, bytes(32)) for p in paths])
    assert got == [[p, str(typ), str(size), h.hex(), str(fl)] for p, _, _, typ, size, h, fl in want]
    assert [r[0] for r in want if r[6] & GO.MATCH] == \
        ["/top/d1/deep/", "/top/d1/f10", "/top/d1/f13", "/top/d1/f16", "/top/d1/f19",
         "/top/d2/f14", "/top/d2/f17"]
    assert open(out, "rb").read() == \
        T.stream([(r[0], model[r[0]] if r[3] == SO.FILE else b"") for r in want])
    fields = lines[-1].split()
    dirs = sum(1 for r in want if r[2] is None)
    assert fields[:5] == ["ok", str(len(want)), str(dirs), "1", "7"]
