"""Byte oracle of the GetFileTAR stream with PAX entries, independent of the C code: rules 1-6 of
the PAX feature restated in Python from Go 1.16's archive/tar (common.go, writer.go, format.go,
strconv.go) for Header{Name, Size} as WriteHeader handles it, with Go's path.Split, path.Join and
path.Clean taken literally.  Never held against a Go run; Python's tarfile is the reader the
tests check it with.  USTAR entries are tar_oracle's."""
import io
import tarfile

import tar_oracle as TO

MAX_SIZE = TO.MAX_SIZE
MAX_NAME = 65535  # the library's bound on a PAX entry's name


class Refused(Exception):
    """A PAX entry the library does not build (rule 6): PFSCDC_EUNSUPPORTED."""


# ---- Go's path package

def go_clean(p: str) -> str:
    """path.Clean."""
    if p == "":
        return "."
    rooted = p[0] == "/"
    n = len(p)
    out = []
    r, dotdot = 0, 0
    if rooted:
        out.append("/")
        r, dotdot = 1, 1
    while r < n:
        if p[r] == "/":
            r += 1
        elif p[r] == "." and (r + 1 == n or p[r + 1] == "/"):
            r += 1
        elif p[r] == "." and p[r + 1:r + 2] == "." and (r + 2 == n or p[r + 2] == "/"):
            r += 2
            if len(out) > dotdot:
                w = len(out) - 1
                while w > dotdot and out[w] != "/":
                    w -= 1
                del out[w:]
            elif not rooted:
                if out:
                    out.append("/")
                out += [".", "."]
                dotdot = len(out)
        else:
            if (rooted and len(out) != 1) or (not rooted and out):
                out.append("/")
            while r < n and p[r] != "/":
                out.append(p[r])
                r += 1
    return "".join(out) if out else "."


def go_split(p: str):
    """path.Split: (dir, file), dir ending behind the last slash."""
    i = p.rfind("/")
    return p[:i + 1], p[i + 1:]


def go_join(*elem: str) -> str:
    """path.Join: empty elements dropped, the rest joined with slashes and cleaned."""
    parts = [e for e in elem if e != ""]
    return go_clean("/".join(parts)) if parts else ""


# bytes <-> str one to one, so the path functions above see Go's bytes
def _s(b: bytes) -> str:
    return b.decode("latin-1")


def _b(s: str) -> bytes:
    return s.encode("latin-1")


def to_ascii(b: bytes) -> bytes:
    """toASCII: every byte >= 0x80, and NUL, dropped."""
    return bytes(c for c in b if 0 < c < 0x80)


# ---- rules 1-5

def is_ascii(name: bytes) -> bool:
    return all(0 < c < 0x80 for c in name)


def pax_keys(name: bytes, size: int):
    """Rule 1: the PAX records of the entry, {} where it stays USTAR."""
    ustar_ok = is_ascii(name) and size <= MAX_SIZE and \
        (len(name) <= 100 or TO.split_ustar_path(name) is not None)
    if ustar_ok:
        return {}
    recs = {}
    if not is_ascii(name) or len(name) > 100:
        recs["path"] = name
    if size > MAX_SIZE:
        recs["size"] = b"%d" % size
    return recs


def format_pax_record(key: bytes, value: bytes) -> bytes:
    """Rule 2: formatPAXRecord."""
    base = len(key) + len(value) + 3
    n = base + len(str(base))
    rec = b"%d %s=%s\n" % (n, key, value)
    if len(rec) != n:
        n = len(rec)
        rec = b"%d %s=%s\n" % (n, key, value)
    assert len(rec) == n
    return rec


def records(name: bytes, size: int) -> bytes:
    recs = pax_keys(name, size)
    return b"".join(format_pax_record(k.encode(), recs[k]) for k in sorted(recs))


def name_is_built(name: bytes) -> bool:
    """Rule 6: no empty, "." or ".." component, a leading '/' and a directory's trailing '/'
    aside."""
    rest = name[1:] if name.startswith(b"/") else name
    if rest == b"":
        return name == b"/"
    if rest.endswith(b"/"):
        rest = rest[:-1]
    return all(c not in (b"", b".", b"..") for c in rest.split(b"/"))


def _finish(blk: bytearray, size_field: int, typeflag: bytes, devs: bool) -> bytes:
    for at in (100, 108, 116):            # mode, uid, gid
        blk[at:at + 8] = b"0000000\0"
    blk[124:136] = b"%011o\0" % size_field
    blk[136:148] = b"00000000000\0"
    blk[156:157] = typeflag
    blk[257:265] = b"ustar\x0000"
    if devs:
        for at in (329, 337):
            blk[at:at + 8] = b"0000000\0"
    blk[148:156] = b" " * 8
    blk[148:156] = b"%06o\0 " % sum(blk)
    return bytes(blk)


def ext_name(name: bytes) -> bytes:
    """Rule 3: the extended header block's name, with path.Split and path.Join."""
    d, f = go_split(_s(name))
    joined = _b(go_join(d, "PaxHeaders.0", f))
    cut = to_ascii(joined)[:100]
    return cut.rstrip(b"/")


def ext_block(name: bytes, recs: bytes) -> bytes:
    blk = bytearray(512)
    xn = ext_name(name)
    blk[0:len(xn)] = xn
    return _finish(blk, len(recs), b"x", False)  # uname .. prefix stay zero bytes


def main_block(name: bytes, size: int) -> bytes:
    """Rule 4."""
    blk = bytearray(512)
    a = to_ascii(name)
    blk[0:min(100, len(a))] = a[:100]
    if len(a) > 100 and a[99:100] == b"/":
        n = len(a[:100].rstrip(b"/"))
        blk[n] = 0
    typeflag = b"5" if name.endswith(b"/") else b"0"
    return _finish(blk, size if size <= MAX_SIZE else 0, typeflag, True)


def head(path, size: int) -> bytes:
    """Every byte in front of the entry's content, PAX allowed."""
    name = path.encode() if isinstance(path, str) else bytes(path)
    if not name or b"\0" in name:
        raise ValueError("empty name or NUL")
    if not pax_keys(name, size):
        return TO.header(name, size)
    if len(name) > MAX_NAME or not name_is_built(name):
        raise Refused(name)
    recs = records(name, size)
    return ext_block(name, recs) + recs + bytes(-len(recs) % 512) + main_block(name, size)


def layout(entries):
    """entries: (path, size).  (entry offsets with the trailer's as the last, total): rule 5."""
    offs, at = [], 0
    for path, size in entries:
        offs.append(at)
        at += len(head(path, size)) + (size + 511) // 512 * 512
    offs.append(at)
    return offs, at + 1024


def stream(files) -> bytes:
    """files: (path, content) pairs."""
    out = bytearray()
    for path, content in files:
        out += head(path, len(content)) + content + bytes(-len(content) % 512)
    return bytes(out + bytes(1024))


def read_back(data: bytes):
    """[(name, size, is_dir, content)] as tarfile reads the stream; names as UTF-8 with
    surrogateescape, so any bytes come back as they went in."""
    got = []
    with tarfile.open(fileobj=io.BytesIO(data), mode="r:", encoding="utf-8",
                      errors="surrogateescape") as tf:
        for m in tf:
            body = tf.extractfile(m).read() if m.isreg() else b""
            got.append((m.name.encode("utf-8", "surrogateescape"), m.size, m.isdir(), body))
    return got


def first_member(data: bytes):
    """(name, size) of the first member, from its head alone."""
    with tarfile.open(fileobj=io.BytesIO(data), mode="r:", encoding="utf-8",
                      errors="surrogateescape") as tf:
        m = tf.next()
        return m.name.encode("utf-8", "surrogateescape"), m.size
