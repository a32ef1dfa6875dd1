"""GetFileTAR's host side (no GPU): pfscdc_tar_header and pfscdc_tar_layout, the specification
the framing kernel is checked against, held against the issue's known answers, against
tests/tar_oracle.py (an independent restatement of Go's archive/tar header) and against
Python's tarfile as the reader; the entries that would need PAX are refused; TarStream rejects
a bad window before any GPU context exists."""
import ctypes as C
import hashlib
import os
import random
import re
import subprocess
import tarfile

import pytest

import tar_oracle as T
from pfs_amd import _lib
from pfs_amd import cdc
from pfs_amd import chunk as pc
from pfs_amd import fileset as pf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pfscdc.h")
TAR_API = {"pfscdc_tar_header": 3, "pfscdc_tar_layout": 5, "pfscdc_read_tar": 18,
           "pfscdc_last_frame_ms": 2, "pfscdc_store_read_tar": 12}

LONG = "/" + "d" * 60 + "/" + "f" * 80
N100 = "/n" + "a" * 98
KNOWN = [  # name, size, chksum field, SHA-256 of the header (first 16 hex)
    ("/a/b.txt", 5, b"010443\0 ", "18ce4e0c240495a0"),
    ("/dir/", 0, b"010021\0 ", "0d944cb68475a3d1"),
    (LONG, 513, b"042760\0 ", "f8967952d10ca22f"),
    ("/e", 0, b"007403\0 ", "35c527de689825bc"),
    (N100, 512, b"032057\0 ", "3a35f64bd5125209"),
]
CONTENTS = [b"hello", b"", b"x" * 513, b"", b"y" * 512]
STREAM_SHA = "0b169e2cba0bce09820afd77cd5dee10673bfe17830894c3a3f8d4134ef2922f"
UNSUPPORTED = [("/" + "g" * 100, 0), ("/é", 0), ("/" + "p" * 156 + "/q", 0), ("/big", 1 << 33)]


def _dr(size, ref_size=None, offset=0):
    ref = pc.Ref(size_bytes=size + offset if ref_size is None else ref_size, edge=False,
                 chunk_index=0, id=bytes(32), dek=bytes(32))
    return pc.DataRef(ref=ref, hash=bytes(32), offset_bytes=offset, size_bytes=size)


@pytest.fixture
def no_ctx(monkeypatch):
    """Any attempt to create a GPU context fails the test."""
    def boom(*a, **k):
        raise AssertionError("a GPU context was created")
    monkeypatch.setattr(cdc.Chunker, "__init__", boom)


@pytest.mark.parametrize("name,size,chk,digest", KNOWN)
def test_known_headers(name, size, chk, digest):
    h = pf.tar_header(name, size)
    assert len(h) == 512
    assert h[148:156] == chk
    assert hashlib.sha256(h).hexdigest()[:16] == digest
    assert h == T.header(name, size)
    if name == LONG:  # split at the second '/'
        assert h[345:345 + 61] == LONG[:61].encode() and h[:81] == b"f" * 80 + b"\0"


def test_known_stream_from_header_and_layout():
    files = [(n, [_dr(z)] if z else []) for n, z, _, _ in KNOWN]
    offs, total = pf.tar_layout(files)
    assert total == 5632
    out = bytearray(total)
    for (name, size, _, _), body, at in zip(KNOWN, CONTENTS, offs):
        out[at:at + 512] = pf.tar_header(name, size)
        out[at + 512:at + 512 + size] = body
    assert hashlib.sha256(out).hexdigest() == STREAM_SHA
    assert bytes(out) == T.stream([(n, b) for (n, _, _, _), b in zip(KNOWN, CONTENTS)])
    got = T.read_back(bytes(out))
    assert got == [(T.tarfile_name(n), z, n.endswith("/"), b)
                   for (n, z, _, _), b in zip(KNOWN, CONTENTS)]


@pytest.mark.parametrize("size", [0, 7, 8, 511, 512, (1 << 33) - 1])
def test_size_field(size):
    h = pf.tar_header("/s", size)
    assert h[124:136] == b"%011o\0" % size
    assert int(h[124:135], 8) == size
    assert h == T.header("/s", size)


@pytest.mark.parametrize("name,size", UNSUPPORTED)
def test_entries_that_need_pax_are_unsupported(name, size):
    lib = _lib.load()
    out = (C.c_uint8 * 512)()
    assert lib.pfscdc_tar_header(name.encode(), size, out) == _lib.PFSCDC_EUNSUPPORTED
    with pytest.raises(T.NeedsPax):
        T.header(name, size)
    with pytest.raises(_lib.PfsCdcError) as e:
        pf.tar_header(name, size)
    assert e.value.code == _lib.PFSCDC_EUNSUPPORTED
    # the layout of a file list that holds it, by every entry point without a ctx
    drs = [_dr(size)] if size else []
    with pytest.raises(_lib.PfsCdcError) as e:
        pf.tar_layout([("/ok", [_dr(3)]), (name, drs)])
    assert e.value.code == _lib.PFSCDC_EUNSUPPORTED
    assert repr(name) in str(e.value)  # the file is named
    with pytest.raises(_lib.PfsCdcError):
        pf.TarStream(pc.Storage(device=0, store=pc.ChunkStore()), [(name, drs)])


def test_directory_with_data_is_invalid():
    lib = _lib.load()
    out = (C.c_uint8 * 512)()
    assert lib.pfscdc_tar_header(b"/dir/", 5, out) == _lib.PFSCDC_EINVAL
    assert lib.pfscdc_tar_header(b"", 0, out) == _lib.PFSCDC_EINVAL
    tf = _lib.tar_files([("/dir/", 0, 1)])
    total = C.c_uint64()
    for size in (0, 5):  # a DataRef is data, even an empty one
        sizes = (C.c_uint64 * 1)(size)
        assert lib.pfscdc_tar_layout(tf, 1, sizes, None, C.byref(total)) == _lib.PFSCDC_EINVAL
    with pytest.raises(ValueError):
        pf.tar_layout([("/dir/", [_dr(5)])])
    with pytest.raises(ValueError):
        pf.tar_header("/dir/", 5)


def test_layout_offsets_and_total():
    sizes = [0, 1, 511, 512, 513]
    files = [("/f%d" % i, [_dr(z)] if z else []) for i, z in enumerate(sizes)]
    offs, total = pf.tar_layout(files)
    assert offs == [0, 512, 1536, 2560, 3584, 5120]
    assert total == 5120 + 1024
    assert (offs, total) == T.layout(sizes)
    # a file's size is the sum of its DataRefs'
    assert pf.tar_layout([("/a", [_dr(500), _dr(13)]), ("/b", [])]) == ([0, 1536, 2048], 3072)
    assert pf.tar_layout([]) == ([0], 1024)
    lib = _lib.load()
    total = C.c_uint64()
    assert lib.pfscdc_tar_layout(None, 0, None, None, C.byref(total)) == 0 and total.value == 1024


def test_window_validation_happens_before_any_gpu_call(no_ctx):
    st = pc.Storage(device=0, store=pc.ChunkStore())
    ts = pf.TarStream(st, [("/a", [_dr(1000)]), ("/b", [_dr(5)])])
    assert ts.size() == 512 + 1024 + 512 + 512 + 1024
    for begin, length in [(1, 512), (511, None), (0, 100), (512, 513), (1024, 3583 - 1024),
                          (ts.size() + 512, None), (-512, 512)]:
        with pytest.raises(ValueError):
            ts.read(begin, length)
    with pytest.raises(ValueError):
        list(ts.windows(1000))
    with pytest.raises(ValueError):  # a DataRef past its chunk, as chunk.Reader rejects it
        pf.TarStream(st, [("/a", [_dr(10, ref_size=5)])]).read()
    with pytest.raises(ValueError):
        pf.TarStream(pc.Storage(device=0), [("/a", [_dr(10)])]).read()


def _random_names(n, seed):
    rng = random.Random(seed)
    alphabet = "abcdefghijklmnopqrstuvwxyzABCXYZ0123456789._- "
    names = []
    while len(names) < n:
        if len(names) % 2 == 0:  # 1-100 bytes, no split
            ln = rng.choice([1, 2, 99, 100]) if rng.random() < 0.2 else rng.randint(1, 100)
            body = "".join(rng.choice(alphabet + "/") for _ in range(ln - 1))
            name = "/" + body
        else:  # 101-255 bytes with a '/' where splitUSTARPath can cut
            suffix = "".join(rng.choice(alphabet) for _ in range(rng.randint(1, 100)))
            plen = rng.randint(max(1, 100 - len(suffix)), 154)
            prefix = "/" + "".join(rng.choice(alphabet + "/") for _ in range(plen - 1))
            name = prefix + "/" + suffix
            if len(name) <= 100:
                continue
        if rng.random() < 0.15 and len(name) < 255:
            name += "/"  # a directory
        if "//" in name or name.rstrip("/") == "":
            continue
        try:
            T.header(name, 0)
        except T.NeedsPax:
            continue
        names.append(name)
    return names


def test_tarfile_reads_back_random_names():
    rng = random.Random(7)
    names = _random_names(200, 20240611)
    assert any(len(n) == 100 for n in names) and any(len(n) > 156 for n in names)
    assert any(n.endswith("/") for n in names)
    blocks = bytearray()
    want = []
    for name in names:
        size = 0 if name.endswith("/") else rng.choice([0, 1, 511, 512, rng.randint(0, (1 << 33) - 1)])
        h = pf.tar_header(name, size)
        assert h == T.header(name, size), name
        ti = tarfile.TarInfo.frombuf(h, "utf-8", "surrogateescape")  # verifies the checksum
        want.append((T.tarfile_name(name), size, name.endswith("/")))
        assert (ti.name, ti.size, ti.isdir()) == want[-1], name
        assert ti.isreg() != ti.isdir() and (ti.mode, ti.uid, ti.gid, ti.mtime) == (0, 0, 0, 0)
        if size == 0:
            blocks += h
    got = [(n, z, d) for n, z, d, _ in T.read_back(bytes(blocks) + bytes(1024))]
    assert got == [w for w in want if w[1] == 0]


def test_tar_consumer_builds_as_strict_c99(tmp_path):
    """tests/c/tar_consumer.c (run on the GPU by tests/test_gpu_tar.py) compiles and links as
    strict C99 against the header and library, like the other C drivers."""
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "tar_consumer.c"),
                    "-L", libdir, "-lpfscdc", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(tmp_path / "tar_consumer")],
                   check=True)


def test_tar_api_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()
    for name, nargs in TAR_API.items():
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED
        assert len(getattr(lib, name).argtypes) == nargs, name
    m = re.search(r"typedef struct pfscdc_tar_file \{(.*?)\} pfscdc_tar_file;", text, flags=re.S)
    fields = re.findall(r"(const char\*|uint32_t)\s+(\w+);", m.group(1))
    assert [n for _, n in fields] == [n for n, _ in _lib.TarFile._fields_]
    assert C.sizeof(_lib.TarFile) == 16
    nw = C.c_uint64()
    assert lib.pfscdc_store_read_tar(None, None, None, 0, None, 0, 0, 0, None, 0, 0,
                                     C.byref(nw)) == _lib.PFSCDC_EINVAL
