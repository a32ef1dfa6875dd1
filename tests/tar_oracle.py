"""Byte oracle of the GetFileTAR stream for the tar tests, independent of the C code: the
USTAR header Go's archive/tar writes for Header{Name, Size} with every other field zero
(restated from its field table and splitUSTARPath; never held against a Go run), and the
stream getFileTar forms from it.  Python's tarfile is the reader the tests check it with; its
writer is no byte oracle (it leaves devmajor/devminor NUL)."""
import io
import tarfile

MAX_SIZE = 0o77777777777  # 8 GiB - 1: above it Go writes PAX records


class NeedsPax(Exception):
    pass


def split_ustar_path(name: bytes):
    """(prefix, suffix) as archive/tar's splitUSTARPath, None where the name does not split."""
    length = len(name)
    if length <= 100:
        return None
    if length > 156:
        length = 156
    elif name.endswith(b"/"):
        length -= 1
    i = name[:length].rfind(b"/")
    nlen, plen = len(name) - i - 1, i
    if i <= 0 or nlen > 100 or nlen == 0 or plen > 155:
        return None
    return name[:i], name[i + 1:]


def header(path, size: int) -> bytes:
    name = path.encode() if isinstance(path, str) else bytes(path)
    if not name or any(b == 0 or b >= 0x80 for b in name):
        raise NeedsPax("name is not ASCII 0x01-0x7F")
    if size > MAX_SIZE:
        raise NeedsPax("size above 8 GiB - 1")
    prefix = b""
    if len(name) > 100:
        sp = split_ustar_path(name)
        if sp is None:
            raise NeedsPax("name longer than 100 bytes does not split")
        prefix, short = sp
    else:
        short = name
    blk = bytearray(512)
    blk[0:len(short)] = short
    for at in (100, 108, 116):            # mode, uid, gid
        blk[at:at + 8] = b"0000000\0"
    blk[124:136] = b"%011o\0" % size
    blk[136:148] = b"00000000000\0"       # a zero ModTime is written as Unix 0
    blk[148:156] = b" " * 8
    blk[156] = ord("5") if name.endswith(b"/") else ord("0")
    blk[257:265] = b"ustar\x0000"
    for at in (329, 337):                 # devmajor, devminor
        blk[at:at + 8] = b"0000000\0"
    blk[345:345 + len(prefix)] = prefix
    blk[148:156] = b"%06o\0 " % sum(blk)
    return bytes(blk)


def layout(sizes):
    """(entry offsets with the trailer's as the last, total)."""
    offs, at = [], 0
    for z in sizes:
        offs.append(at)
        at += 512 + (z + 511) // 512 * 512
    offs.append(at)
    return offs, at + 1024


def stream(files) -> bytes:
    """files: (path, content) pairs."""
    out = bytearray()
    for path, content in files:
        out += header(path, len(content)) + content + bytes(-len(content) % 512)
    return bytes(out + bytes(1024))


def read_back(data: bytes):
    """[(name, size, is_dir, content)] as tarfile reads the stream."""
    got = []
    with tarfile.open(fileobj=io.BytesIO(data), mode="r:") as tf:
        for m in tf:
            body = tf.extractfile(m).read() if m.isreg() else b""
            got.append((m.name, m.size, m.isdir(), body))
    return got


def tarfile_name(path: str) -> str:
    """How tarfile reports a member's name: trailing slashes stripped."""
    return path.rstrip("/") if path.rstrip("/") else path
