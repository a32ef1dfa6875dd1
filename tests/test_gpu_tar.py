"""GetFileTAR on the GPU (pfscdc_read_tar, pfscdc_store_read_tar, fileset.TarStream): the tar
stream of files of stored chunks, content decrypted straight into place by the slice gather and
headers, padding and trailer formed by tar_frame_kernel.  Every comparison is exact and over
the whole output: the byte oracle is tests/tar_oracle.py (independent of the C code), the
reader is Python's tarfile, the chunks are tests/stored_chunks.py's."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import tar_oracle as T
from oracle import chunker as Ch
from pfs_amd import _lib
from pfs_amd import chunk as pc
from pfs_amd import fileset as pf
from pfs_amd.cdc import ChunkParams, Chunker, synthetic_bytes
from stored_chunks import Stored

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = Ch.Params(average_bits=12, seed=1, min=2000, max=30000)
LONG = "/" + "d" * 60 + "/" + "f" * 80  # splits at the second '/'
N100 = "/n" + "a" * 98                   # 100 bytes: the longest name without a split


@pytest.fixture(scope="module")
def chunker():
    c = Chunker(ChunkParams(), 0)
    yield c
    c.close()


class Files:
    """Named files over a Stored batch: per file its slices (chunk, offset, size)."""

    def __init__(self, st, named):
        self.st = st
        self.names = [n for n, _ in named]
        self.per_file = [list(sl) for _, sl in named]
        self.slices = [s for sl in self.per_file for s in sl]
        self.triples, at = [], 0
        for n, sl in named:
            self.triples.append((n, at, len(sl)))
            at += len(sl)
        self.sizes = [sum(z for _, _, z in sl) for sl in self.per_file]

    def contents(self, zeroed=()):
        return [b"".join(bytes(z) if c in zeroed else self.st.chunks[c][o:o + z]
                         for c, o, z in sl) for sl in self.per_file]

    def stream(self, zeroed=()):
        return T.stream(list(zip(self.names, self.contents(zeroed))))

    def store_files(self, store=None):
        """[(path, [DataRef])] for TarStream and a ChunkStore holding the chunks."""
        st = self.st
        if store is None:
            store = pc.ChunkStore()
            for i in range(len(st.sizes)):
                store.put(bytes(st.refs[i]["id"]), st.store[bytes(st.refs[i]["id"])])
        refs = [pc.Ref(size_bytes=st.sizes[i], edge=False, chunk_index=i,
                       id=bytes(st.refs[i]["id"]), dek=bytes(st.refs[i]["dek"]))
                for i in range(len(st.sizes))]
        files = [(n, [pc.DataRef(ref=refs[c], hash=bytes(32), offset_bytes=o, size_bytes=z)
                      for c, o, z in sl]) for n, sl in zip(self.names, self.per_file)]
        return files, store


@pytest.fixture(scope="module")
def twelve():
    """12 files of sizes 0 .. 40,001 over 4 chunks: DataRefs at odd chunk offsets, files that
    span two chunks, share a chunk, and repeat a DataRef."""
    st = Stored([3000, 70000, 12345, 41000], 201)
    f = Files(st, [
        ("/empty", []),
        ("/one", [(0, 2999, 1)]),                        # the chunk's last byte
        ("/a/seven.txt", [(0, 1, 7)]),
        ("/a/eight", [(0, 1, 4), (0, 1, 4)]),            # one DataRef twice
        ("/a/nine", [(0, 2995, 5), (2, 0, 4)]),          # spans two chunks
        (LONG, [(2, 101, 63)]),
        (N100, [(2, 101, 64)]),                          # shares (overlaps) the file before
        ("/b/65", [(2, 12280, 65)]),
        ("/b/511", [(1, 69489, 511)]),
        ("/b/512", [(1, 3, 500), (3, 40988, 12)]),
        ("/b/513 with spaces", [(3, 7, 513)]),
        ("/big/40001.bin", [(1, 30001, 39999), (3, 0, 2)]),
    ])
    assert f.sizes == [0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 40001]
    return f


def _read_back_matches(data, f, contents):
    got = T.read_back(data)
    assert got == [(T.tarfile_name(n), len(b), n.endswith("/"), b)
                   for n, b in zip(f.names, contents)]


def test_whole_stream_into_host_memory(chunker, twelve):
    f = twelve
    want = f.stream()
    offs, total = T.layout(f.sizes)
    assert len(want) == total
    got, cok, nw = chunker.read_tar(f.st.ctext, f.st.offs, f.st.refs, f.triples, f.slices)
    assert nw == total and cok.all()
    assert got.tobytes() == want
    _read_back_matches(got.tobytes(), f, f.contents())
    t = chunker.last_read_timings()
    assert t["verify"] > 0 and t["gather"] > 0 and chunker.last_frame_ms() > 0
    # the strict form over a store gives the same stream
    files, store = f.store_files()
    ts = pf.TarStream(pc.Storage(device=0, store=store), files)
    assert ts.size() == total and ts.entry_offsets == offs
    assert ts.read() == want


@pytest.mark.parametrize("at", [0, 3])
def test_whole_stream_into_a_device_tensor_writes_each_byte_once(chunker, twelve, at):
    import torch
    f = twelve
    want = f.stream()
    total = len(want)
    dev = torch.from_numpy(f.st.ctext).to("cuda:0")
    t = torch.full((at + total + 29,), 0xA5, dtype=torch.uint8, device="cuda:0")
    res, cok, nw = chunker.read_tar(dev, f.st.offs, f.st.refs, f.triples, f.slices,
                                    out=t[at:at + total])
    assert nw == total and cok.all()
    host = t.cpu().numpy()
    assert host[at:at + nw].tobytes() == want
    assert (host[:at] == 0xA5).all() and (host[at + nw:] == 0xA5).all()
    # a window in the middle of a larger tensor: nothing outside it changes (no memset)
    t.fill_(0xA5)
    begin, n = 1536, 4096
    _, _, nw = chunker.read_tar(dev, f.st.offs, f.st.refs, f.triples, f.slices, begin=begin,
                                length=n, out=t[at:])
    host = t.cpu().numpy()
    assert nw == n and host[at:at + n].tobytes() == want[begin:begin + n]
    assert (host[:at] == 0xA5).all() and (host[at + n:] == 0xA5).all()
    # through the public API
    files, store = f.store_files()
    t.fill_(0xA5)
    assert pf.TarStream(pc.Storage(device=0, store=store), files).read_into(t[at:]) == total
    host = t.cpu().numpy()
    assert host[at:at + total].tobytes() == want
    assert (host[:at] == 0xA5).all() and (host[at + total:] == 0xA5).all()


@pytest.mark.parametrize("window", [512, 1536, 4096])
def test_windows_concatenate_to_the_whole_stream(chunker, twelve, window):
    import torch
    f = twelve
    want = f.stream()
    total = len(want)
    offs, _ = T.layout(f.sizes)
    begins = list(range(0, total, window))
    if window == 512:
        # windows that begin inside content; that end just after a header; that hold one content
        # byte and 511 of padding (padding is shorter than a block, so none holds padding
        # alone); that lie wholly inside the trailer
        assert offs[11] + 1024 in begins and offs[2] in begins and offs[1] + 512 in begins
        assert f.sizes[1] == 1 and begins[-2] == total - 1024
    dev = torch.from_numpy(f.st.ctext).to("cuda:0")
    parts = []
    for b in begins:
        buf = np.full(window + 8, 0xA5, dtype=np.uint8)
        _, cok, nw = chunker.read_tar(dev, f.st.offs, f.st.refs, f.triples, f.slices, begin=b,
                                      length=window, out=buf)
        assert nw == min(window, total - b)
        assert (buf[nw:] == 0xA5).all()
        parts.append(buf[:nw].tobytes())
    assert b"".join(parts) == want


def test_window_that_reaches_the_end_with_an_odd_length(chunker, twelve):
    f = twelve
    want = f.stream()
    total = len(want)
    first, _, nw = chunker.read_tar(f.st.ctext, f.st.offs, f.st.refs, f.triples, f.slices,
                                    begin=0, length=1024)
    assert nw == 1024
    rest = total - 1024
    assert (rest + 77) % 512
    out = np.full(rest + 77, 0xA5, dtype=np.uint8)
    _, _, nw = chunker.read_tar(f.st.ctext, f.st.offs, f.st.refs, f.triples, f.slices,
                                begin=1024, length=rest + 77, out=out)
    assert nw == rest and (out[rest:] == 0xA5).all()
    assert first.tobytes() + out[:rest].tobytes() == want
    # the store form in windows, the last one short
    files, store = f.store_files()
    ts = pf.TarStream(pc.Storage(device=0, store=store), files)
    parts = list(ts.windows(16384))
    assert [len(p) for p in parts[:-1]] == [16384] * (len(parts) - 1)
    assert b"".join(parts) == want


def test_bad_windows_and_names_are_rejected_with_a_ctx(chunker, twelve):
    f = twelve
    args = (f.st.ctext, f.st.offs, f.st.refs)
    total = len(f.stream())
    for begin, length in [(7, 512), (0, 100), (512, 1000), (total + 512, 512)]:
        with pytest.raises(_lib.PfsCdcError) as e:
            chunker.read_tar(*args, f.triples, f.slices, begin=begin, length=length,
                             out=np.zeros(total, dtype=np.uint8))
        assert e.value.code == _lib.PFSCDC_EINVAL
    for name in ["/" + "g" * 100, "/é", "/" + "p" * 156 + "/q"]:
        with pytest.raises(_lib.PfsCdcError) as e:
            chunker.read_tar(*args, [("/ok", 0, 1), (name, 1, 1)], f.slices[:2])
        assert e.value.code == _lib.PFSCDC_EUNSUPPORTED
        assert name in str(e.value)  # the file is named
    with pytest.raises(_lib.PfsCdcError) as e:
        chunker.read_tar(*args, [("/dir/", 0, 1)], f.slices[:1])
    assert e.value.code == _lib.PFSCDC_EINVAL


# ------------------------------------------------------------------- many entries, grid-stride

def _names(n, rng):
    names = []
    for i in range(n):
        k = i % 10
        if k == 3:
            names.append(("/n%05d" % i).ljust(100, "x"))  # 100 bytes, no split
        elif k == 6:  # splits: a prefix of up to 155 bytes, a suffix of up to 100
            plen, slen = int(rng.integers(1, 149)), int(rng.integers(1, 94))
            names.append("/" + "p" * plen + "%05d" % i + "/" + "%05d" % i + "s" * slen)
            if len(names[-1]) <= 100:
                names[-1] = "/" + "q" * 100 + names[-1]
        elif k == 8:
            names.append("/dir%05d/" % i)
        else:
            names.append("/f/%05d.dat" % i)
    return names


@pytest.fixture(scope="module")
def three_hundred():
    """300 files of 0-700 bytes packed back to back into two chunks."""
    rng = np.random.default_rng(202)
    names = _names(300, rng)
    sizes = [0 if n.endswith("/") else int(rng.integers(0, 701)) for n in names]
    half = sum(sizes[:150])
    st = Stored([half + 5, sum(sizes[150:]) + 9], 202)
    named, at = [], [3, 1]
    for i, (n, z) in enumerate(zip(names, sizes)):
        c = 0 if i < 150 else 1
        named.append((n, [] if n.endswith("/") else [(c, at[c], z)]))
        at[c] += z
    f = Files(st, named)
    assert any(len(n) == 100 for n in names) and any(len(n) > 156 for n in names)
    return f


def _header_blocks(data, sizes):
    offs, _ = T.layout(sizes)
    return [data[o:o + 512] for o in offs[:-1]]


def test_every_header_equals_the_host_specification(chunker, three_hundred):
    f = three_hundred
    got, cok, nw = chunker.read_tar(f.st.ctext, f.st.offs, f.st.refs, f.triples, f.slices)
    data = got.tobytes()
    assert cok.all() and nw == len(data)
    blocks = _header_blocks(data, f.sizes)
    assert len(blocks) == 300
    for name, size, blk in zip(f.names, f.sizes, blocks):
        assert blk == pf.tar_header(name, size), name
        assert blk == T.header(name, size), name
    assert data == f.stream()


@pytest.mark.parametrize("grid", [1, 3])
def test_capped_launch_takes_many_passes(chunker, three_hundred, knob, grid):
    f = three_hundred
    waves = 4 * grid  # launch_tar_frame: 4 waves a workgroup, one item per wave and pass
    passes = -(-(len(f.names) + 2) // waves)
    assert passes >= 2
    knob("PFSCDC_CHACHA_GRID", grid)
    got, cok, _ = chunker.read_tar(f.st.ctext, f.st.offs, f.st.refs, f.triples, f.slices)
    assert cok.all()
    assert got.tobytes() == f.stream()


def test_shipped_width_takes_more_than_one_pass(chunker):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # launch_tar_frame: workgroups = min(ceil((n + 2) / 4), 8 * CUs), 4 waves each
    full_waves = 4 * 8 * cus
    n = 2 * full_waves + 1
    waves = 4 * min(-(-(n + 2) // 4), 8 * cus)
    assert waves == full_waves and -(-(n + 2) // waves) >= 2
    names = ["/e/%06d" % i for i in range(n)]
    out = torch.full((512 * n + 1024 + 5,), 0xA5, dtype=torch.uint8, device="cuda:0")
    _, _, nw = chunker.read_tar(b"", [0], np.zeros(0, dtype=_lib.ref_dtype()),
                                [(p, 0, 0) for p in names], [], out=out[5:])
    assert nw == 512 * n + 1024
    host = out.cpu().numpy()
    assert (host[:5] == 0xA5).all()
    assert host[5:].tobytes() == T.stream([(p, b"") for p in names])


# ------------------------------------------------------------------------- tampering, marks

def test_tampered_chunk_batch_form_zeroes_its_content_only(chunker, twelve):
    f = twelve
    k = 2
    bad = f.st.ctext.copy()
    bad[int(f.st.offs[k]) + 150] ^= 0x20
    got, cok, _ = chunker.read_tar(bad, f.st.offs, f.st.refs, f.triples, f.slices)
    assert [bool(x) for x in cok] == [c != k for c in range(4)]
    want = f.stream(zeroed={k})
    assert want != f.stream()
    assert got.tobytes() == want  # every header and every other file intact
    _read_back_matches(got.tobytes(), f, f.contents(zeroed={k}))


def test_tampered_and_missing_chunks_store_form(twelve):
    import torch
    f = twelve
    files, good = f.store_files()
    total = len(f.stream())
    bad = pc.ChunkStore()
    for i in range(4):
        ct = bytearray(good.get(bytes(f.st.refs[i]["id"])))
        if i == 3:
            ct[100] ^= 0x01
        bad.put(bytes(f.st.refs[i]["id"]), bytes(ct))
    ts = pf.TarStream(pc.Storage(device=0, store=bad), files)
    with pytest.raises(_lib.PfsCdcError) as e:
        ts.read()
    assert e.value.code == _lib.PFSCDC_ECORRUPT
    t = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(_lib.PfsCdcError) as e:
        ts.read_into(t)
    assert e.value.code == _lib.PFSCDC_ECORRUPT
    assert (t.cpu().numpy() == 0xA5).all()  # nothing was written, headers included
    # a window that names only good chunks reads: chunk 3 first appears in "/b/512"
    offs, _ = T.layout(f.sizes)
    assert ts.read(0, offs[9]) == f.stream()[:offs[9]]
    short = pc.ChunkStore()
    for i in range(3):
        short.put(bytes(f.st.refs[i]["id"]), good.get(bytes(f.st.refs[i]["id"])))
    ts = pf.TarStream(pc.Storage(device=0, store=short), files)
    with pytest.raises(KeyError):
        ts.read()
    with pytest.raises(KeyError):
        ts.read_into(t)
    assert (t.cpu().numpy() == 0xA5).all()


def test_verified_marks_carry_over_to_the_next_window(chunker, twelve):
    import torch
    f = twelve
    want = f.stream()
    offs, total = T.layout(f.sizes)
    dev = torch.from_numpy(f.st.ctext).to("cuda:0")
    cut = offs[9]  # windows 1 names chunks 0, 1, 2; chunk 3 first appears in "/b/512"
    a, cok1, _ = chunker.read_tar(dev, f.st.offs, f.st.refs, f.triples, f.slices, begin=0,
                                  length=cut)
    assert [bool(x) for x in cok1] == [True, True, True, False]  # chunk 3: not named, not hashed
    b, cok2, _ = chunker.read_tar(dev, f.st.offs, f.st.refs, f.triples, f.slices, begin=cut,
                                  verified=cok1)
    assert cok2.all()
    assert a.tobytes() + b.tobytes() == want
    # a mark is honoured: chunk 1, tampered after it was verified, is not hashed again
    bad = f.st.ctext.copy()
    bad[int(f.st.offs[1]) + 40000] ^= 0x80
    _, cok3, _ = chunker.read_tar(bad, f.st.offs, f.st.refs, f.triples, f.slices, begin=cut,
                                  verified=cok1)
    assert cok3.all()
    _, cok4, _ = chunker.read_tar(bad, f.st.offs, f.st.refs, f.triples, f.slices, begin=cut)
    assert [bool(x) for x in cok4] == [False, False, False, True]  # chunk 1 fails; 0, 2: unnamed


# ------------------------------------------------------------------ write -> read, public API

def test_write_then_read_as_tar():
    lens = [30_000, 0, 4_133]
    names = ["/data/big.bin", "/data/empty", "/small"]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    data = synthetic_bytes(offs, 204)
    files = [data[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(lens))]
    st = pc.Storage(device=0, store=pc.ChunkStore())
    drs = [[] for _ in files]

    def cb(anns):
        for a in anns:
            if a.next_data_ref is not None:
                drs[a.data].append(a.next_data_ref)

    w = st.new_writer("w", cb, pc.with_rolling_hash_config(SMALL.average_bits, SMALL.seed),
                      pc.with_min_max(SMALL.min, SMALL.max))
    for i, body in enumerate(files):
        w.annotate(pc.Annotation(data=i))
        w.write(body)
    w.close()
    assert len(drs[0]) > 1  # a file of several chunks
    ts = pf.TarStream(st, list(zip(names, drs)))
    got = ts.read()
    assert got == T.stream(list(zip(names, files)))
    assert T.read_back(got) == [(n, len(b), False, b) for n, b in zip(names, files)]
    assert b"".join(ts.windows(2048)) == got


# ------------------------------------------------------------------------------- plain C

def test_plain_c_process_writes_a_tar_in_two_windows(tmp_path, twelve):
    f = twelve
    exe = str(tmp_path / "tar_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "tar_consumer.c"),
                    "-L", libdir, "-lpfscdc", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    path, outp = str(tmp_path / "chunks.bin"), str(tmp_path / "out.tar")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<III", len(f.st.sizes), len(f.slices), len(f.names)))
        for i, n in enumerate(f.st.sizes):
            fh.write(bytes(f.st.refs[i]["id"]) + bytes(f.st.refs[i]["dek"]) + struct.pack("<Q", n))
        for c, o, z in f.slices:
            fh.write(struct.pack("<IIQQ", c, 0, o, z))
        for name, first, count in f.triples:
            fh.write(struct.pack("<III", first, count, len(name.encode())) + name.encode())
        fh.write(f.st.ctext.tobytes())
    res = subprocess.run([exe, path, outp], capture_output=True, text=True, timeout=100)
    assert res.returncode == 0, res.stderr
    want = f.stream()
    first = len(want) // 2 // 512 * 512
    header = open(os.path.join(ROOT, "include", "pfscdc.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"#define (PFSCDC_E\w+) (-\d+)", header)}
    assert res.stdout.splitlines() == [
        "tar %d %d %d" % (len(want), first, len(want) - first),
        "einval %d %d" % (codes["PFSCDC_EINVAL"], codes["PFSCDC_EINVAL"]),
    ]
    data = open(outp, "rb").read()
    assert data == want
    _read_back_matches(data, f, f.contents())
