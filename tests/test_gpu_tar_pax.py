"""GetFileTAR with PAX entries on the GPU: tar_frame_kernel's extended header, record and main
header blocks and the resident plan's longer heads, through pfscdc_read_tar,
pfscdc_store_read_tar and pfscdc_dev_list_read_tar.  Every comparison is exact and over the whole
output: the byte oracle is tests/tar_pax_oracle.py (independent of the C code), the reader is
Python's tarfile, the cases are tests/tar_pax_cases.py's."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import tar_pax_cases as K
import tar_pax_oracle as P
from oracle import chunker as Ch
from oracle import fileset as OF
from pfs_amd import _lib
from pfs_amd import chunk as pc
from pfs_amd import fileset as pf
from pfs_amd.cdc import ChunkParams, Chunker, synthetic_bytes
from stored_chunks import Stored
from test_gpu_resident import dev_layout, dev_tar, host_tar, up
from test_gpu_tar import Files

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAX = _lib.TAR_USTAR | _lib.TAR_PAX
MIB = 1 << 20


@pytest.fixture(scope="module")
def chunker():
    c = Chunker(ChunkParams(), 0)
    yield c
    c.close()


@pytest.fixture
def pax_ctx():
    """A context whose tar format allows PAX (the raw C calls of the resident helpers)."""
    c = Chunker(ChunkParams(), 0)
    assert c.lib.pfscdc_set_tar_format(c.ctx, PAX) == 0
    yield c
    c.close()


def index_list(st, named):
    """An index list of (name bytes, [(chunk, offset, size)]).  A name that is no UTF-8 cannot go
    through the proto library: it is encoded under a stand-in of its length and patched into the
    message, whose first field is the path."""
    frames = []
    for name, sl in named:
        try:
            path, patch = name.decode(), False
        except UnicodeDecodeError:
            path, patch = "\x7f" * len(name), True
        msg = bytearray(OF.encode_index(OF.Index(
            path, "default", [Ch.DataRef(st.orefs[c], bytes(32), o, z) for c, o, z in sl])))
        if patch:
            assert len(name) < 128 and msg[:2 + len(name)] == b"\x0a" + bytes([len(name)]) + path.encode()
            msg[2:2 + len(name)] = name
        frames.append(OF.frame(bytes(msg)))
    return pf.index_decode_host(b"".join(frames))


@pytest.fixture(scope="module")
def mixed():
    """40 files: every PAX case of tests/tar_pax_cases.py between USTAR entries, contents of 0
    bytes to a few KiB at odd offsets of three chunks."""
    st = Stored([9000, 9000, 9000], 301)
    ustar = [(b"/u/%02d.txt" % i, z) for i, z in enumerate([7, 513, 3000, 0, 512, 64, 1, 2100])] + \
        [(K.LONG_SPLITS, 63), (b"/udir/", 0), (b"/n" + b"a" * 98, 511), (b"/u/last", 33),
         (b"/u/z", 700)]
    named, at, u = [], [3, 1, 5], iter(ustar)
    for i, (_, name, size) in enumerate(K.PAX):
        for n, z in ([next(u)] if i % 2 == 0 and i < 26 else []) + [(name, size)]:
            c = len(named) % 3
            named.append((n, [(c, at[c], z)] if z else []))
            at[c] += z
    assert len(named) == 40 and max(at) <= 9000
    f = Files(st, named)
    assert sum(1 for n, z in zip(f.names, f.sizes) if z == 0 and not n.endswith(b"/")) >= 2
    assert max(f.sizes) == 3000
    return f


def want_stream(f):
    return P.stream(list(zip(f.names, f.contents())))


def test_whole_stream_into_a_prefilled_tensor_all_arms(chunker, pax_ctx, mixed):
    import torch
    f = mixed
    want = want_stream(f)
    offs, total = P.layout(list(zip(f.names, f.sizes)))
    assert len(want) == total
    assert P.read_back(want) == [(n.rstrip(b"/") or n, len(b), n.endswith(b"/"), b)
                                 for n, b in zip(f.names, f.contents())]
    # pfscdc_read_tar: every byte of the tensor's window is overwritten, none outside it
    dev = torch.from_numpy(f.st.ctext).to("cuda:0")
    t = torch.full((3 + total + 29,), 0xA5, dtype=torch.uint8, device="cuda:0")
    _, cok, nw = chunker.read_tar(dev, f.st.offs, f.st.refs, f.triples, f.slices,
                                  out=t[3:3 + total], pax=True)
    host = t.cpu().numpy()
    assert nw == total and cok.all()
    assert host[3:3 + total].tobytes() == want
    assert (host[:3] == 0xA5).all() and (host[3 + total:] == 0xA5).all()
    # every head equals the host specification
    for name, size, at in zip(f.names, f.sizes, offs):
        h = pf.tar_head(name, size, pax=True)
        assert want[at:at + len(h)] == h, name[:40]
    # pfscdc_store_read_tar
    files, store = f.store_files()
    ts = pf.TarStream(pc.Storage(device=0, store=store), files, pax=True)
    assert ts.size() == total and ts.entry_offsets == offs
    assert ts.read() == want
    t.fill_(0xA5)
    assert ts.read_into(t[3:]) == total
    host = t.cpu().numpy()
    assert host[3:3 + total].tobytes() == want and (host[3 + total:] == 0xA5).all()
    # pfscdc_dev_list_read_tar, and its layout
    lst = index_list(f.st, list(zip(f.names, f.per_file)))
    dvl = up(pax_ctx, lst)
    assert dev_layout(pax_ctx, dvl) == (0, offs, total)
    assert host_tar(pax_ctx, store, lst, 0, total) == (0, want, "")
    assert dev_tar(pax_ctx, store, dvl, 0, total) == (0, want, "")
    t.fill_(0xA5)
    torch.cuda.synchronize()
    nwc = C.c_uint64()
    rc = pax_ctx.lib.pfscdc_dev_list_read_tar(pax_ctx.ctx, store._s, dvl._p, 0, total,
                                              t[3:].data_ptr(), total + 26, 1, C.byref(nwc))
    host = t.cpu().numpy()
    assert rc == 0 and nwc.value == total and host[3:3 + total].tobytes() == want
    assert (host[:3] == 0xA5).all() and (host[3 + total:] == 0xA5).all()
    # the same handle under the default format is refused as ever, then plans again for PAX
    assert chunker.lib.pfscdc_set_tar_format(chunker.ctx, _lib.TAR_USTAR) == 0
    rc, got, msg = dev_tar(chunker, store, dvl, 0, 4096, fill=True)
    assert rc == _lib.PFSCDC_EUNSUPPORTED and set(got) == {0xA5} and "needs a PAX header" in msg
    assert dev_tar(pax_ctx, store, dvl, 0, total) == (0, want, "")


@pytest.mark.parametrize("window", [512, 1024, 1536])
def test_windows_at_every_block_all_arms(chunker, pax_ctx, mixed, window):
    """Every window of 512, 1,024 and 1,536 bytes at every multiple of 512: each block of each
    head is a window of its own, and window borders fall inside heads."""
    import torch
    f = mixed
    want = want_stream(f)
    total = len(want)
    files, store = f.store_files()
    ts = pf.TarStream(pc.Storage(device=0, store=store), files, pax=True)
    lst = index_list(f.st, list(zip(f.names, f.per_file)))
    dvl = up(pax_ctx, lst)
    dev = torch.from_numpy(f.st.ctext).to("cuda:0")
    store_ctx = Chunker(ChunkParams(), 0)
    try:
        buf = (C.c_uint8 * window)()
        for b in range(0, total, 512):
            n = min(window, total - b)
            out = np.full(window + 8, 0xA5, dtype=np.uint8)
            _, _, nw = chunker.read_tar(dev, f.st.offs, f.st.refs, f.triples, f.slices, begin=b,
                                        length=window, out=out, pax=True)
            assert nw == n and (out[n:] == 0xA5).all()
            assert out[:n].tobytes() == want[b:b + n], b
            assert ts._read(buf, window, 0, b, n, store_ctx) == n
            assert bytes(buf)[:n] == want[b:b + n], b
            assert dev_tar(pax_ctx, store, dvl, b, window) == (0, want[b:b + n], ""), b
    finally:
        store_ctx.close()


@pytest.mark.parametrize("grid", [1, 0])
def test_launch_widths_wrap_the_block_loop(chunker, pax_ctx, mixed, knob, grid):
    """One workgroup (4 waves for 40 entries, 2 trailer blocks and the PAX blocks, of which the
    5,000-byte name alone has 11), and the shipped width."""
    f = mixed
    assert K.flat(5000) in f.names
    assert len(pf.tar_head(K.flat(5000), 4, pax=True)) == 512 * 12  # records span 10 blocks
    want = want_stream(f)
    knob("PFSCDC_CHACHA_GRID", grid)
    got, cok, nw = chunker.read_tar(f.st.ctext, f.st.offs, f.st.refs, f.triples, f.slices, pax=True)
    assert cok.all() and nw == len(want)
    assert got.tobytes() == want
    files, store = f.store_files()
    lst = index_list(f.st, list(zip(f.names, f.per_file)))
    assert dev_tar(pax_ctx, store, up(pax_ctx, lst), 0, len(want)) == (0, want, "")
    offs, _ = P.layout(list(zip(f.names, f.sizes)))
    at = offs[f.names.index(K.flat(5000))] + 512 * 3  # a window inside the long name's records
    got, _, nw = chunker.read_tar(f.st.ctext, f.st.offs, f.st.refs, f.triples, f.slices,
                                  begin=at, length=3072, pax=True)
    assert got.tobytes() == want[at:at + 3072]


def test_shipped_width_takes_more_than_one_pass_over_pax_blocks(chunker):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    full_waves = 4 * 8 * cus
    n = full_waves // 2 + 3  # items: n entries + 2 + 2n PAX blocks > 2 passes of the full width
    names = [("/é/%06d" % i).encode() for i in range(n)]
    assert -(-(3 * n + 2) // full_waves) >= 2
    want = P.stream([(p, b"") for p in names])
    out = torch.full((len(want) + 5,), 0xA5, dtype=torch.uint8, device="cuda:0")
    _, _, nw = chunker.read_tar(b"", [0], np.zeros(0, dtype=_lib.ref_dtype()),
                                [(p, 0, 0) for p in names], [], out=out[5:], pax=True)
    host = out.cpu().numpy()
    assert nw == len(want) and (host[:5] == 0xA5).all()
    assert host[5:].tobytes() == want


def test_not_clean_is_refused_alike_and_out_untouched(chunker, pax_ctx, mixed):
    f = mixed
    files, store = f.store_files()
    for bad in K.NOT_CLEAN[:3]:
        named = [(b"/ok", [(0, 0, 5)]), (bad, [(1, 0, 7)]), (b"/" + K.E, [])]
        lst = index_list(f.st, named)
        want = host_tar(pax_ctx, store, lst, 0, 4096, fill=True)
        assert want[0] == _lib.PFSCDC_EUNSUPPORTED and set(want[1]) == {0xA5}
        assert "not clean" in want[2] and bad.decode() in want[2]
        dvl = up(pax_ctx, lst)
        for _ in range(2):  # the second call answers from the cached plan
            assert dev_tar(pax_ctx, store, dvl, 0, 4096, fill=True) == want
        assert dev_layout(pax_ctx, dvl)[0] == _lib.PFSCDC_EUNSUPPORTED
        with pytest.raises(_lib.PfsCdcError) as e:
            chunker.read_tar(f.st.ctext, f.st.offs, f.st.refs,
                             [(n, i, len(sl)) for i, (n, sl) in enumerate(named)],
                             [(0, 0, 5), (1, 0, 7)], pax=True)
        assert e.value.code == _lib.PFSCDC_EUNSUPPORTED and "not clean" in str(e.value)
    # with PAX off the same list names the earlier reason, in both arms
    lst = index_list(f.st, [(b"/ok", [(0, 0, 5)]), (K.NOT_CLEAN[0], [])])
    assert chunker.lib.pfscdc_set_tar_format(chunker.ctx, _lib.TAR_USTAR) == 0
    want = host_tar(chunker, store, lst, 0, 4096, fill=True)
    assert want[0] == _lib.PFSCDC_EUNSUPPORTED and "not ASCII" in want[2]
    assert dev_tar(chunker, store, up(chunker, lst), 0, 4096, fill=True) == want


def test_a_file_above_8_gib(pax_ctx):
    """One file whose 8,193 DataRefs name the same 1 MiB stored chunk (the last one 100 bytes
    short, so the stream has padding): a size record, a size field of zeros, and only the first
    and the last window rendered."""
    st = Stored([MIB], 302)
    store = pc.ChunkStore()
    for rid, ct in st.store.items():
        store.put(rid, ct)
    sl = [(0, 0, MIB)] * 8192 + [(0, 0, MIB - 100)]
    size = 8193 * MIB - 100
    assert size > P.MAX_SIZE
    names = [(b"/big.bin", sl), (b"/after-" + K.E, [(0, 5, 9)])]
    head = P.head(b"/big.bin", size)
    assert len(head) == 1536 and b"19 size=%d\n" % size in head
    offs, total = P.layout([(b"/big.bin", size), (names[1][0], 9)])
    assert total == 1536 + size + 100 + 2048 + 1024
    lst = index_list(st, names)
    dvl = up(pax_ctx, lst)
    assert dev_layout(pax_ctx, dvl) == (0, offs, total)
    cnt, ents, _, _, _ = lst._views()
    tf = pax_ctx.lib.pfscdc_index_list_tar_files(lst._p)
    sizes = (C.c_uint64 * cnt)(*[ents[i].size_bytes for i in range(cnt)])
    hoffs, htotal = (C.c_uint64 * (cnt + 1))(), C.c_uint64()
    assert pax_ctx.lib.pfscdc_tar_layout_format(tf, cnt, sizes, PAX, hoffs, C.byref(htotal)) == 0
    assert (list(hoffs), htotal.value) == (offs, total)
    chunk = st.chunks[0]
    first = head + chunk[:512]
    tail_at = 1536 + size - 412  # the last content block: 412 bytes of content, 100 of padding
    assert tail_at % 512 == 0
    last = chunk[MIB - 100 - 412:MIB - 100] + bytes(100) + P.head(names[1][0], 9) + \
        chunk[5:14] + bytes(503) + bytes(1024)
    for arm in (host_tar, dev_tar):
        src = lst if arm is host_tar else dvl
        assert arm(pax_ctx, store, src, 0, 2048) == (0, first, "")
        assert arm(pax_ctx, store, src, tail_at, 1 << 20) == (0, last, "")
    assert P.first_member(first) == (b"/big.bin", size)


SMALL = Ch.Params(average_bits=12, seed=1, min=2000, max=30000)
LOOP_INDEX = Ch.Params(average_bits=12, seed=0, min=3000, max=30000)


@pytest.mark.parametrize("resident", [False, True])
def test_write_open_get_file_with_utf8_names(resident):
    data = synthetic_bytes([0, 20_000], 303).tobytes()
    long_name = "/" + "L" * 149  # 150 bytes, one component: no split
    model = {"/données/été.csv": data[:700], "/données/vide": b"", "/日本/ファイル.bin": data[700:5200],
             long_name: data[5200:5713], "/plain/a.txt": data[6000:6007]}
    store = pc.ChunkStore()
    cp = lambda p: ChunkParams(p.average_bits, p.seed, p.min, p.max)  # noqa: E731
    st = pf.Storage(0, cp(SMALL), 10 ** 9, cp(LOOP_INDEX), store=store)
    w = st.new_unordered_writer()
    for p, body in model.items():
        w.put(p, "", False, body)
    infos = w.close()
    w.release()
    fs = st.open(infos, resident=resident)
    with pytest.raises(_lib.PfsCdcError) as e:
        fs.get_file("/")
    assert e.value.code == _lib.PFSCDC_EUNSUPPORTED
    with pytest.raises(_lib.PfsCdcError) as e:
        fs.tar()
    assert e.value.code == _lib.PFSCDC_EUNSUPPORTED
    tar = fs.get_file("/", pax=True)
    got = tar.read()
    assert len(got) == tar.size()
    members = P.read_back(got)
    assert {n.decode(): b for n, _, d, b in members if not d} == model
    dirs = {n.decode() for n, _, d, _ in members if d}
    assert {"/données", "/日本", "/plain"} <= dirs
    # the stream is the oracle's over the same entries, directories included
    entries = [((n + b"/") if d else n, b) for n, _, d, b in members]
    assert got == P.stream(entries)
    # the files alone, and a storage whose default is PAX
    flat = fs.tar(pax=True).read()
    assert {n.decode(): b for n, _, _, b in P.read_back(flat)} == model
    st.pax = True
    assert st.open(infos, resident=resident).get_file("/données").read() == \
        fs.get_file("/données", pax=True).read()


def test_plain_c_process_reads_a_pax_stream(tmp_path, mixed):
    f = mixed
    exe = str(tmp_path / "tar_pax_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "tar_pax_consumer.c"),
                    "-L", libdir, "-lpfscdc", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    order = [i for i, n in enumerate(f.names) if b"\0" not in n]
    order.sort(key=lambda i: f.names[i] != K.flat(600))  # the first file: a PAX entry
    path, outp = str(tmp_path / "chunks.bin"), str(tmp_path / "out.tar")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<III", len(f.st.sizes), len(f.slices), len(order)))
        for i, n in enumerate(f.st.sizes):
            fh.write(bytes(f.st.refs[i]["id"]) + bytes(f.st.refs[i]["dek"]) + struct.pack("<Q", n))
        for c, o, z in f.slices:
            fh.write(struct.pack("<IIQQ", c, 0, o, z))
        for i in order:
            name, first, count = f.triples[i]
            fh.write(struct.pack("<III", first, count, len(name)) + name)
        fh.write(f.st.ctext.tobytes())
    res = subprocess.run([exe, path, outp], capture_output=True, text=True, timeout=100)
    assert res.returncode == 0, res.stderr
    contents = f.contents()
    want = P.stream([(f.names[i], contents[i]) for i in order])
    header = open(os.path.join(ROOT, "include", "pfscdc.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"#define (PFSCDC_E\w+) (-\d+)", header)}
    assert res.stdout.splitlines() == [
        "ustar %d %d" % (codes["PFSCDC_EUNSUPPORTED"], codes["PFSCDC_EUNSUPPORTED"]),
        "pax %d %d" % (len(want), len(want)),
        "head %d" % len(P.head(K.flat(600), 4)),
        "einval %d %d" % (codes["PFSCDC_EINVAL"], codes["PFSCDC_EINVAL"]),
    ]
    assert open(outp, "rb").read() == want
