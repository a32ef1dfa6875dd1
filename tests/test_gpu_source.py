"""The Source on the GPU: pfscdc_source_open against its specification pfscdc_source_host, array
for array (entries, blob, DataRefs) and info for info, with the stats saying which arm ran; and
the file RPCs of ``FileSet`` end to end against a dict model, tests/source_oracle.py and
tests/tar_oracle.py.  Every comparison is exact."""
import ctypes as C
import io
import random
import tarfile

import pytest
import torch

import source_cases as SC
import source_oracle as SO
import tar_oracle as T
from oracle import fileset as OF
from pfs_amd import _lib
from pfs_amd import chunk as pc
from pfs_amd import fileset as pf
from pfs_amd.cdc import ChunkParams, Chunker
from test_gpu_index_read import LOOP_INDEX, model_ops, write
from test_gpu_merge import arrays

pytestmark = pytest.mark.gpu

GPU_ARGS = ("", "/a", "/a/", "/a/b", "/a/c", "/ab", "/nothing")


@pytest.fixture
def chunker():
    c = Chunker(ChunkParams(), 0)
    yield c
    c.close()


@pytest.fixture
def device_arm(knob):
    knob("PFSCDC_SOURCE", 1)


def same(a, b):
    x, y = arrays(a), arrays(b)
    assert [len(v) for v in x] == [len(v) for v in y]
    assert x[0] == y[0], "entries"
    assert x[1] == y[1], "blob"
    assert x[2] == y[2], "DataRefs"


def outcome(fn):
    """("ok", value) or the error as (kind, code, text)."""
    try:
        return ("ok", fn())
    except KeyError as e:
        return ("notfound", _lib.PFSCDC_ENOTFOUND, e.args[0])
    except _lib.PfsCdcError as e:
        return ("error", e.code, str(e))


def both(chunker, lst, kind, arg, leaf=None, arm=1, dev=None):
    """pfscdc_source_open over ``lst`` (resident copy ``dev`` if given) against
    pfscdc_source_host: the same list and infos, or the same error code and text."""
    host = outcome(lambda: pf.source_host(lst, kind, arg, leaf))
    got = outcome(lambda: pf.source_open(chunker, dev if dev is not None else lst, kind, arg, leaf))
    st = pf.last_source_stats(chunker)
    assert got[0] == host[0], (kind, arg, got, host[:1])
    if host[0] != "ok":
        assert got[1:] == host[1:]
        return None, st
    src = got[1]
    hres, hinfos = host[1]
    assert st["device"] == arm, (kind, arg, st)
    assert (st["entries_in"], st["entries_out"]) == (len(lst) if lst is not None else 0, len(hres))
    assert len(src) == len(hres)
    same(src.list.download(chunker), hres)
    assert src.infos(chunker) == hinfos
    n_in = {(d["path"], d["tag"]) for d in (lst.raw() if lst is not None else [])}
    assert st["dirs_inserted"] == sum(1 for d in hres.raw() if (d["path"], d["tag"]) not in n_in)
    src.free()
    return (hres, hinfos), st


# ------------------------------------------------------------------ the CPU cases

@pytest.mark.parametrize("name", sorted(SC.hand_trees()))
def test_hand_trees_equal_the_host(chunker, device_arm, name):
    rng = random.Random(sum(map(ord, name)))
    entries, lst, _ = SC.build(rng, SC.hand_trees()[name])
    dev = pf.DevIndexList.upload(chunker, lst)
    oks = 0
    for kind in SC.KINDS:
        for arg in GPU_ARGS + ("/d0/d1", "/e"):
            res, st = both(chunker, lst, kind, arg, dev=dev)
            if res is not None:
                oks += 1
                w = SC.want(entries, kind, arg)  # and the oracle itself
                assert SC.rows_of(*res) == SC.rows_want(w[1], entries)
    assert oks


def test_chain_levels_and_hash_launches(chunker, device_arm):
    rng = random.Random(2)
    _, lst, _ = SC.build(rng, SC.hand_trees()["chain12"])
    _, st = both(chunker, lst, SO.ALL, "")
    # "/" has depth 0, the leaf depth 13: one launch per depth and one for the leaves
    assert (st["levels"], st["hash_launches"], st["dirs_inserted"]) == (14, 15, 13)
    _, st = both(chunker, lst, SO.ALL, "", leaf=b"".join(SC.leaf_of(1)))
    assert st["hash_launches"] == 14


@pytest.mark.parametrize("block", range(4))
def test_random_trees_equal_the_host(chunker, device_arm, block):
    rng = random.Random(900 + block)
    for _ in range(12):
        entries, lst, _ = SC.build(rng, SC.random_tree(rng))
        paths = [e[0] for e in entries]
        for kind in SC.KINDS:
            for arg in ["", "/a", "/ab"] + rng.sample(paths, min(2, len(paths))):
                both(chunker, lst, kind, arg)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_input_lengths(chunker, device_arm, n):
    rng = random.Random(n)
    _, lst, _ = SC.build(rng, SC.sequence(n))
    res, st = both(chunker, lst, SO.ALL, "")
    assert len(res[0]) == (n + min(n, 7) + 1 if n else 0)
    both(chunker, lst, SO.SUBTREE, "/s03")
    both(chunker, lst, SO.LIST, "/")
    both(chunker, lst, SO.GET, "/s00/f00000")


def wide_flat():
    return [("/big/f%04d" % i, "t", 1) for i in range(1025)]


def wide_dirs():
    return [("/sub/d%04d/f" % i, "t", 1) for i in range(1025)]


@pytest.mark.parametrize("shape", ["flat", "dirs"])
@pytest.mark.parametrize("grid", [1, 2, 3, 0])
def test_1025_children_and_grid_knobs(chunker, device_arm, knob, shape, grid):
    """A directory of 1,025 immediate children is one BLAKE2b chain of 32,800 bytes (257 blocks:
    past the kernel's first pass and tile edges); 1,025 sub-directories are 1,025 chains of one
    level and one long chain of the next.  PFSCDC_CHACHA_GRID and PFSCDC_HASH_GRID at 1-3
    workgroups and at the shipped widths."""
    knob("PFSCDC_CHACHA_GRID", grid)
    knob("PFSCDC_HASH_GRID", grid)
    rng = random.Random(11)
    entries, lst, _ = SC.build(rng, wide_flat() if shape == "flat" else wide_dirs())
    res, st = both(chunker, lst, SO.ALL, "")
    w = SC.want(entries, SO.ALL, "")
    assert SC.rows_of(*res) == SC.rows_want(w[1], entries)
    assert st["dirs_inserted"] == (2 if shape == "flat" else 1027)
    both(chunker, lst, SO.LIST, "/big" if shape == "flat" else "/sub")
    both(chunker, lst, SO.GET, "/sub/d0512")


@pytest.mark.parametrize("arm", [1, 0])
def test_both_knob_values(chunker, knob, arm):
    knob("PFSCDC_SOURCE", arm)
    rng = random.Random(13)
    for spec in (SC.hand_trees()["straddle"], SC.random_tree(rng, 29), SC.sequence(300), []):
        _, lst, _ = SC.build(rng, spec)
        for kind in SC.KINDS:
            for arg in ("", "/a", "/s01", "/nothing"):
                both(chunker, lst, kind, arg, arm=arm)


@pytest.mark.parametrize("name", sorted(SC.host_only_trees()))
def test_host_arm_only_for_lists_the_device_refuses(chunker, device_arm, name):
    """An unsorted list, unclean paths (//x, rel, /a/./b) and one directory path twice set the
    device flag and take the host arm; the results still equal the specification."""
    rng = random.Random(77)
    _, lst, _ = SC.build(rng, SC.host_only_trees()[name])
    for kind in SC.KINDS:
        for arg in ("", "/a", "/x", "rel"):
            both(chunker, lst, kind, arg, arm=0)


def test_leaf_hashes_from_host_and_device(chunker, device_arm):
    rng = random.Random(5)
    for spec in (SC.hand_trees()["straddle"], SC.hand_trees()["explicit_dir"], SC.sequence(257)):
        entries, lst, _ = SC.build(rng, spec)
        leaf = b"".join(SC.leaf_of(len(entries)))
        on_dev = torch.frombuffer(bytearray(leaf), dtype=torch.uint8).to("cuda:0")
        for kind, arg in ((SO.ALL, ""), (SO.SUBTREE, "/a"), (SO.LIST, "/s02"), (SO.GET, "/a")):
            a, _ = both(chunker, lst, kind, arg, leaf=leaf)
            host = outcome(lambda: pf.source_host(lst, kind, arg, leaf))
            got = outcome(lambda: pf.source_open(chunker, lst, kind, arg, on_dev))
            assert got[0] == host[0]
            if got[0] == "ok":
                assert got[1].infos(chunker) == host[1][1]
                w = SC.want(entries, kind, arg, SC.leaf_of(len(entries)))
                assert [i[0] for i in host[1][1]] == [r[5] for r in w[1]]


def test_errors_equal_the_hosts_and_write_nothing(chunker, device_arm):
    rng = random.Random(6)
    _, lst, _ = SC.build(rng, SC.hand_trees()["two_tags"])
    dev = pf.DevIndexList.upload(chunker, lst)
    lib = chunker.lib
    ranged = pf.index_decode_host(OF.frame(OF.encode_index(
        OF.Index("/a", None, [], (0, "/b", SC.dr(rng).ref)))))
    cases = [(dev, SO.GET, "/a/f" + ch, _lib.PFSCDC_EUNSUPPORTED) for ch in SO.GLOB_BYTES] + \
        [(dev, SO.GET, "/nothing", _lib.PFSCDC_ENOTFOUND),
         (dev, SO.SUBTREE, "/a/ff", _lib.PFSCDC_ENOTFOUND), (dev, 9, "/a", _lib.PFSCDC_EINVAL),
         (pf.DevIndexList.upload(chunker, ranged), SO.ALL, "", _lib.PFSCDC_EINVAL),
         (pf.DevIndexList.upload(chunker, None), SO.GET, "/", _lib.PFSCDC_ENOTFOUND)]
    for d, kind, arg, code in cases:
        out = C.c_void_p(0xDEAD)
        rc = lib.pfscdc_source_open(chunker.ctx, d._p, kind, arg.encode(), None, 0, C.byref(out))
        assert rc == code and not out.value, (kind, arg, rc)
        text = lib.pfscdc_last_error(chunker.ctx).decode()
        hl = ranged if code == _lib.PFSCDC_EINVAL and kind == SO.ALL else \
            (None if arg == "/" else lst)
        host = outcome(lambda: pf.source_host(hl, kind, arg))
        assert host[1] == code and text and text in host[2]
    both(chunker, lst, SO.LIST, "/nothing")  # an empty source, no error
    both(chunker, None, SO.SUBTREE, "/")


# ------------------------------------------------------------------ end to end

def model_rows(fs, nfilesets, device=0):
    """The oracle's entries of an opened fileset, and the leaf hashes the reference would use."""
    files = fs.files()
    entries = [(f.path, f.tag, f.size_bytes, [bytes(d.hash) for d in f.data_refs]) for f in files]
    leaf = None
    if nfilesets > 1:
        leaf = [pc.merge_file_hash(fs._storage.store, f.data_refs, device) for f in files]
    return entries, leaf


def as_rows(infos):
    return [(i.path, i.tag, i.type, i.size, i.hash) for i in infos]


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("seed,threshold", [(1, 10 ** 9), (2, 30_000), (3, 12_000)])
def test_put_delete_sequences_against_the_model(device_arm, seed, threshold, resident):
    ops, model = model_ops(seed, 50)
    st, infos, _ = write(ops, mem_threshold=threshold, index=LOOP_INDEX)
    assert (len(infos) == 1) == (threshold == 10 ** 9)
    fs = st.open(infos, resident=resident)
    entries, leaf = model_rows(fs, len(infos))
    assert [(e[0], e[2]) for e in entries] == [(p, len(model[p])) for p in sorted(model)]
    want = SO.source(entries, SO.SUBTREE, "", leaf)
    assert as_rows(fs.walk_file("")) == [(p, t, typ, size, h) for p, t, _, typ, size, h, _ in want]
    root = fs.inspect_file("/")
    assert (root.path, root.type, root.size) == ("/", pf.DIR, sum(len(v) for v in model.values()))
    for d in ("/a", "/b", "/"):
        w = SO.source(entries, SO.LIST, d, leaf)
        assert as_rows(fs.list_file(d)) == \
            [(p, t, typ, size, h) for p, t, _, typ, size, h, fl in w if fl & SO.CHILD]
    some = sorted(model)[len(model) // 2]
    for p in ("/a", "/b/", some):
        w = SO.source(entries, SO.SUBTREE, p, leaf)
        q = SO.clean_path(p)
        hit = [r for r in w if r[0] in (q, q + "/")][-1]
        assert as_rows([fs.inspect_file(p)]) == [hit[:2] + hit[3:6]]
        assert as_rows(fs.walk_file(p)) == [r[:2] + r[3:6] for r in w]
        # GetFileTAR as the reference serves it: the directories are entries too
        g = SO.source(entries, SO.GET, p, leaf)
        tar = fs.get_file(p)
        assert tar.read() == T.stream([(r[0], model[r[0]] if r[3] == SO.FILE else b"") for r in g])
    for p in ("/zzz", "/a/f"):
        with pytest.raises(KeyError):
            fs.walk_file(p)
        with pytest.raises(KeyError):
            fs.get_file(p)
    assert fs.list_file("/zzz") == []


def test_get_file_of_a_directory_into_a_prefilled_tensor(device_arm):
    ops, model = model_ops(4, 60)
    st, infos, _ = write(ops, mem_threshold=10 ** 9, index=LOOP_INDEX)
    fs = st.open(infos, resident=True)
    entries, _ = model_rows(fs, 1)
    g = SO.source(entries, SO.GET, "/a")
    want = T.stream([(r[0], model[r[0]] if r[3] == SO.FILE else b"") for r in g])
    tar = fs.get_file("/a")
    assert tar.size() == len(want)
    buf = torch.full((len(want) + 4096,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert tar.read_into(buf) == len(want)
    host = bytes(buf.cpu().numpy())
    assert host[:len(want)] == want and set(host[len(want):]) == {0xA5}
    with tarfile.open(fileobj=io.BytesIO(want), mode="r:") as tf:
        members = list(tf)
    assert [m.name.strip("/") for m in members] == [r[0].strip("/") for r in g]
    assert [m.isdir() for m in members] == [r[3] == SO.DIR for r in g] and members[0].isdir()


# ------------------------------------------------------------------ a plain C process

def test_plain_c_process_walks_and_gets(tmp_path):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "source_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror",
                    "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "c", "source_consumer.c"),
                    "-L", libdir, "-lpfscdc", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    out = str(tmp_path / "out.tar")
    res = subprocess.run([exe, out], capture_output=True, text=True, timeout=100)
    assert res.returncode == 0, res.stdout + res.stderr

    def path_of(k):
        return "/top/d1/deep/f07" if k == 7 else "/f11" if k == 11 else "/top/d%d/f%02d" % (k % 3, k)
    model = {path_of(k): bytes((k + j) & 0xFF for j in range(k * 997 + 13)) for k in range(24)}
    lines = res.stdout.splitlines()
    got = [l[2:].split("\t") for l in lines if l.startswith("i ")]
    # the files' hashes are the process's own; sizes, types, order and every directory's hash
    # and size follow from them
    leaf_by_path = {p: bytes.fromhex(h) for p, t, _, h in got if int(t) == SO.FILE}
    paths = sorted(model, key=str.encode)
    entries = [(p, "default", len(model[p]), []) for p in paths]
    want = SO.source(entries, SO.SUBTREE, "/", [leaf_by_path[p] for p in paths])
    assert got == [[p, str(typ), str(size), h.hex()] for p, _, _, typ, size, h, _ in want]
    g = SO.source(entries, SO.GET, "/top/d1", [leaf_by_path[p] for p in paths])
    assert open(out, "rb").read() == \
        T.stream([(r[0], model[r[0]] if r[3] == SO.FILE else b"") for r in g])
    fields = lines[-1].split()
    dirs = sum(1 for r in want if r[3] == SO.DIR)
    assert fields[:5] == ["ok", str(len(want)), str(dirs), "1", str(len(g))]
