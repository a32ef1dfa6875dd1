"""GetFileTAR's PAX entries on the host (no GPU): pfscdc_tar_head and pfscdc_tar_layout_format,
the specification the framing kernel is checked against, held byte for byte against
tests/tar_pax_oracle.py (rules restated from Go's archive/tar, with path.Split / Join / Clean
literal), against hand-written blocks for "/é", "/é/f" and "/é/", and against Python's tarfile
as the reader.  With the format left at USTAR everything is as before; a PAX name that
path.Join would rewrite is refused.  The same heads once more from a stand-alone program built
with -fsanitize=address,undefined around tar.cpp."""
import ctypes as C
import os
import subprocess

import pytest

import tar_oracle as T
import tar_pax_cases as K
import tar_pax_oracle as P
from pfs_amd import _lib
from pfs_amd import chunk as pc
from pfs_amd import fileset as pf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USTAR, PAX = _lib.TAR_USTAR, _lib.TAR_USTAR | _lib.TAR_PAX
ALL = K.PAX + K.HUGE + K.USTAR


def head(name: bytes, size: int, fmt: int = PAX):
    """(rc, bytes) of pfscdc_tar_head."""
    lib, n = _lib.load(), C.c_uint64()
    rc = lib.pfscdc_tar_head(name, size, fmt, None, 0, C.byref(n))
    if rc:
        return rc, b""
    out = (C.c_uint8 * n.value)()
    assert lib.pfscdc_tar_head(name, size, fmt, out, n.value - 1, C.byref(n)) == _lib.PFSCDC_EINVAL
    assert lib.pfscdc_tar_head(name, size, fmt, out, n.value, C.byref(n)) == 0
    return 0, bytes(out)


def layout(entries, fmt: int):
    """(rc, offsets, total) of pfscdc_tar_layout_format over (name, size) pairs (files have one
    piece each, directories and empty files none)."""
    lib = _lib.load()
    tf = _lib.tar_files([(n, i, 1 if z else 0) for i, (n, z) in enumerate(entries)])
    sizes = (C.c_uint64 * max(1, len(entries)))(*[z for _, z in entries])
    offs, total = (C.c_uint64 * (len(entries) + 1))(), C.c_uint64()
    rc = lib.pfscdc_tar_layout_format(tf, len(entries), sizes, fmt, offs, C.byref(total))
    return rc, list(offs), total.value


def _dr(size):
    ref = pc.Ref(size_bytes=size, edge=False, chunk_index=0, id=bytes(32), dek=bytes(32))
    return pc.DataRef(ref=ref, hash=bytes(32), offset_bytes=0, size_bytes=size)


@pytest.mark.parametrize("label,name,size", ALL, ids=[c[0] for c in ALL])
def test_head_equals_oracle_and_tarfile_reads_it(label, name, size):
    rc, got = head(name, size)
    assert rc == 0
    want = P.head(name, size)
    assert len(got) == len(want)
    assert got == want
    assert pf.tar_head(name, size, pax=True) == want
    recs = P.records(name, size)
    assert len(got) == (512 if not recs else 1024 + (len(recs) + 511) // 512 * 512)  # rule 5
    # tarfile reads the full name and the size back from the head alone
    assert P.first_member(got + bytes(1024)) == (name.rstrip(b"/") or name, size)


@pytest.mark.parametrize("label,name,size", K.USTAR, ids=[c[0] for c in K.USTAR])
def test_an_entry_ustar_can_hold_stays_ustar(label, name, size):
    out = (C.c_uint8 * 512)()
    assert _lib.load().pfscdc_tar_header(name, size, out) == 0
    for fmt in (USTAR, PAX):
        assert head(name, size, fmt) == (0, bytes(out))
    assert bytes(out) == T.header(name, size)


@pytest.mark.parametrize("label,name,size", K.PAX + K.HUGE, ids=[c[0] for c in K.PAX + K.HUGE])
def test_which_records_an_entry_gets(label, name, size):
    """Rule 1 and rule 2 from the head's bytes: the records sit behind the first block, sorted,
    each as long as its own prefix says."""
    _, got = head(name, size)
    assert got[156:157] == b"x"
    n = int(got[124:135], 8)
    recs, keys = got[512:512 + n], []
    assert not any(got[512 + n:len(got) - 512])
    while recs:
        ln = int(recs.split(b" ", 1)[0])
        assert ln not in (10, 100, 1000, 10000)
        rec, recs = recs[:ln], recs[ln:]
        assert rec.endswith(b"\n")
        key, value = rec[len(str(ln)) + 1:-1].split(b"=", 1)
        keys.append(key)
        assert value == (name if key == b"path" else b"%d" % size)
    want = ([b"path"] if len(name) > 100 or any(c >= 0x80 for c in name) else []) + \
        ([b"size"] if size > T.MAX_SIZE else [])
    assert keys == want
    if label.startswith("record ") or label.startswith("records "):
        assert n == int(label.split()[1])


def _block(name: bytes, size_field: bytes, typeflag: bytes, devs: bool) -> bytes:
    """One header block from literal field bytes."""
    dev = b"0000000\0" if devs else bytes(8)
    blk = name.ljust(100, b"\0") + b"0000000\0" * 3 + size_field + b"00000000000\0" + b" " * 8 + \
        typeflag + bytes(100) + b"ustar\x0000" + bytes(64) + dev * 2 + bytes(155) + bytes(12)
    assert len(blk) == 512
    return blk[:148] + b"%06o\0 " % sum(blk) + blk[156:]


def test_the_three_spelled_out_heads():
    e = "é".encode()
    # "/é": 12 bytes of records; path.Join leaves "/PaxHeaders.0/é", toASCII and the trim
    # "/PaxHeaders.0"; the main name is "/"
    rec = b"12 path=/" + e + b"\n"
    assert len(rec) == 12
    want = _block(b"/PaxHeaders.0", b"00000000014\0", b"x", False) + rec.ljust(512, b"\0") + \
        _block(b"/", b"00000000000\0", b"0", True)
    assert head(b"/" + e, 0) == (0, want)
    # "/é/f": toASCII runs after Join, so the directory's two slashes stay
    rec = b"14 path=/" + e + b"/f\n"
    assert len(rec) == 14
    want = _block(b"//PaxHeaders.0/f", b"00000000016\0", b"x", False) + rec.ljust(512, b"\0") + \
        _block(b"//f", b"00000000003\0", b"0", True)
    assert head(b"/" + e + b"/f", 3) == (0, want)
    # "/é/": a directory, typeflag 5 in the main block
    rec = b"13 path=/" + e + b"/\n"
    assert len(rec) == 13
    want = _block(b"//PaxHeaders.0", b"00000000015\0", b"x", False) + rec.ljust(512, b"\0") + \
        _block(b"//", b"00000000000\0", b"5", True)
    assert head(b"/" + e + b"/", 0) == (0, want)
    # a directory "/a/b/" (were it PAX) would be named "/a/b/PaxHeaders.0"; and the size record
    assert P.ext_name(b"/a/b/") == b"/a/b/PaxHeaders.0"
    assert P.records(b"/big", 8589934592) == b"19 size=8589934592\n"
    _, got = head(b"/big", 8589934592)
    assert got[512:531] == b"19 size=8589934592\n" and got[1024 + 124:1024 + 136] == b"0" * 11 + b"\0"


def test_field_details_of_the_two_header_blocks():
    # the main name is cut behind its last non-slash byte when byte 99 is '/'
    name = dict((c[0], c[1]) for c in K.PAX)["main name cut at a slash"]
    _, got = head(name, 9)
    main = got[-512:]
    assert main[:99] == b"/" + b"a" * 98 and main[99] == 0 and not any(main[345:500])
    # the extended header's name, cut at 100, loses the slash it then ends in
    name = dict((c[0], c[1]) for c in K.PAX)["ext name cut at a slash"]
    _, got = head(name, 9)
    assert got[:100] == b"/" + b"z" * 85 + b"/PaxHeaders.0" + b"\0"
    assert not any(got[265:512])  # uname .. prefix, devmajor and devminor included, stay zero
    assert got[-512:][329:345] == b"0000000\0" * 2
    # entirely non-ASCII: both names lose every byte of it
    _, got = head("ééé".encode(), 9)
    assert got[:13] == b"PaxHeaders.0\0" and got[-512] == 0


def test_streams_read_back_through_tarfile():
    files = [(n, bytes([i]) * z) for i, (_, n, z) in enumerate(K.PAX + K.USTAR) if z < 10000]
    data = P.stream(files)
    assert P.read_back(data) == [(n.rstrip(b"/") or n, len(b), n.endswith(b"/"), b)
                                 for n, b in files]
    rc, offs, total = layout([(n, len(b)) for n, b in files], PAX)
    assert (rc, offs, total) == (0,) + P.layout([(n, len(b)) for n, b in files])
    assert total == len(data)
    got = bytearray(total)
    for (n, b), at in zip(files, offs):
        h = head(n, len(b))[1]
        got[at:at + len(h)] = h
        got[at + len(h):at + len(h) + len(b)] = b
    assert bytes(got) == data
    # the Python layer: tar_layout over DataRefs
    assert pf.tar_layout([(n, [_dr(len(b))] if b else []) for n, b in files], pax=True) == \
        (offs, total)


@pytest.mark.parametrize("label,name,size", K.PAX + K.HUGE, ids=[c[0] for c in K.PAX + K.HUGE])
def test_with_pax_off_everything_is_as_before(label, name, size):
    lib = _lib.load()
    assert head(name, size, USTAR) == (_lib.PFSCDC_EUNSUPPORTED, b"")
    out = (C.c_uint8 * 512)()
    assert lib.pfscdc_tar_header(name, size, out) == _lib.PFSCDC_EUNSUPPORTED
    entries = [(b"/ok", 3), (name, size)]
    assert layout(entries, USTAR)[0] == _lib.PFSCDC_EUNSUPPORTED
    drs = [_dr(size)] if size else []
    for call in (lambda: pf.tar_layout([("/ok", [_dr(3)]), (name, drs)]),
                 lambda: pf.tar_head(name, size, pax=False),
                 lambda: pf.TarStream(pc.Storage(device=0, store=pc.ChunkStore()), [(name, drs)])):
        with pytest.raises(_lib.PfsCdcError) as e:
            call()
        assert e.value.code == _lib.PFSCDC_EUNSUPPORTED
        assert repr(name) in str(e.value) and "needs a PAX header" in str(e.value)


def test_pax_on_over_an_all_ustar_list_changes_nothing():
    entries = [(n, z) for _, n, z in K.USTAR]
    assert layout(entries, PAX) == layout(entries, USTAR)
    lib = _lib.load()
    tf = _lib.tar_files([(n, i, 1 if z else 0) for i, (n, z) in enumerate(entries)])
    sizes = (C.c_uint64 * len(entries))(*[z for _, z in entries])
    offs, total = (C.c_uint64 * (len(entries) + 1))(), C.c_uint64()
    assert lib.pfscdc_tar_layout(tf, len(entries), sizes, offs, C.byref(total)) == 0
    assert (0, list(offs), total.value) == layout(entries, PAX)
    assert (list(offs), total.value) == T.layout([z for _, z in entries])
    files = [(n, [_dr(z)] if z else []) for n, z in entries]
    assert pf.tar_layout(files, pax=True) == pf.tar_layout(files)


@pytest.mark.parametrize("name", K.NOT_CLEAN)
def test_a_pax_name_that_is_not_clean_is_refused(name):
    assert not P.name_is_built(name)
    with pytest.raises(P.Refused):
        P.head(name, 0)
    assert head(name, 0, PAX) == (_lib.PFSCDC_EUNSUPPORTED, b"")
    assert head(name, 0, USTAR) == (_lib.PFSCDC_EUNSUPPORTED, b"")
    assert layout([(b"/ok", 3), (name, 0)], PAX)[0] == _lib.PFSCDC_EUNSUPPORTED
    with pytest.raises(_lib.PfsCdcError) as e:
        pf.tar_head(name, 0, pax=True)
    assert e.value.code == _lib.PFSCDC_EUNSUPPORTED and "not clean" in str(e.value)
    # the same components in a name USTAR can hold are no one's business
    ascii_name = name.replace("é".encode(), b"e")
    if len(ascii_name) <= 100:
        assert head(ascii_name, 0, PAX)[0] == 0


def test_the_shortcut_equals_path_join_for_every_name_that_is_built():
    """Rule 6: for a name with no empty, "." or ".." component, dir + "PaxHeaders.0"
    [+ "/" + file] is path.Join(dir, "PaxHeaders.0", file)."""
    for _, name, _ in K.PAX + K.HUGE:
        assert P.name_is_built(name)
        d, f = P.go_split(name.decode("latin-1"))
        short = d + "PaxHeaders.0" + ("/" + f if f else "")
        assert P.go_join(d, "PaxHeaders.0", f) == short
    differ = 0  # (the rule is sufficient, not necessary: "../x" joins to itself)
    for name in K.NOT_CLEAN:
        d, f = P.go_split(name.decode("latin-1"))
        differ += P.go_join(d, "PaxHeaders.0", f) != d + "PaxHeaders.0" + ("/" + f if f else "")
    assert differ == len(K.NOT_CLEAN) - 1


def test_bad_arguments_and_bounds():
    lib, n = _lib.load(), C.c_uint64()
    assert lib.pfscdc_tar_head(b"/a", 0, 2, None, 0, C.byref(n)) == _lib.PFSCDC_EINVAL  # PAX alone
    assert lib.pfscdc_tar_head(b"/a", 0, 0, None, 0, C.byref(n)) == _lib.PFSCDC_EINVAL
    assert lib.pfscdc_tar_head(None, 0, PAX, None, 0, C.byref(n)) == _lib.PFSCDC_EINVAL
    assert lib.pfscdc_tar_head(b"", 0, PAX, None, 0, C.byref(n)) == _lib.PFSCDC_EINVAL
    assert lib.pfscdc_tar_head(b"/d/", 5, PAX, None, 0, C.byref(n)) == _lib.PFSCDC_EINVAL
    assert lib.pfscdc_set_tar_format(None, PAX) == _lib.PFSCDC_EINVAL
    assert layout([(b"/a", 1)], 2)[0] == _lib.PFSCDC_EINVAL
    # the longest name a PAX entry may have, and one byte more
    assert head(K.flat(65535), 0)[0] == 0
    assert len(head(K.flat(65535), 0)[1]) == len(P.head(K.flat(65535), 0))
    assert head(K.flat(65536), 0) == (_lib.PFSCDC_EUNSUPPORTED, b"")
    with pytest.raises(P.Refused):
        P.head(K.flat(65536), 0)


def test_new_symbols_are_declared_bound_and_exported():
    import re
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfscdc.h")).read(),
                  flags=re.S)
    lib = _lib.load()
    for name, nargs in {"pfscdc_tar_head": 6, "pfscdc_tar_layout_format": 6,
                        "pfscdc_set_tar_format": 2}.items():
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED
        assert len(getattr(lib, name).argtypes) == nargs, name
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    macros = dict(re.findall(r"#define (PFSCDC_TAR_\w+) (\d+)", text))
    assert macros == {"PFSCDC_TAR_USTAR": str(_lib.TAR_USTAR), "PFSCDC_TAR_PAX": str(_lib.TAR_PAX)}


def test_standalone_under_asan_and_ubsan(tmp_path):
    """tests/c/tar_pax_host.cpp with tar.cpp, no GPU library, under AddressSanitizer and UBSan:
    the head of every case under both formats into a buffer of exactly its length, and the
    layout of the whole list."""
    cases = [(n, z) for _, n, z in ALL] + [(n, 0) for n in K.NOT_CLEAN] + \
        [(K.flat(65535), 0), (K.flat(65536), 0), (b"/d/", 5)]
    (tmp_path / "jobs.txt").write_text("".join("%s %d\n" % (n.hex(), z) for n, z in cases))
    exe = str(tmp_path / "tar_pax_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "tar_pax_host.cpp"),
                    os.path.join(ROOT, "pfs_amd", "csrc", "tar.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe, str(tmp_path / "jobs.txt")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    assert lines[-1] == "ok"
    assert len(lines) == 2 * len(cases) + 3
    for i, (n, z) in enumerate(cases):
        for k, fmt in enumerate((USTAR, PAX)):
            rc, hx = lines[2 * i + k].split(" ")
            want_rc, want = head(n, z, fmt)
            assert (int(rc), bytes.fromhex(hx)) == (want_rc, want), (n[:40], z, fmt)
    good = [(n, z) for _, n, z in ALL] + [(K.flat(65535), 0)]
    for line, fmt in zip(lines[-3:-1], (USTAR, PAX)):
        rc, offs, total = layout(good, fmt)
        assert line.split() == [str(rc)] + ([str(total)] + [str(o) for o in offs] if rc == 0 else [])
