"""The names and sizes the PAX tests share (CPU, sanitizer program, GPU): every case of the
feature's test list, as (label, name bytes, size).  Sizes here are what a header may claim; the
GPU tests give the small ones real content."""

E = "é".encode()  # 2 bytes
EURO = "€".encode()  # 3 bytes


def flat(n: int, ch: bytes = b"n") -> bytes:
    """An ASCII name of n bytes with no '/' but the first: over 100 bytes it does not split."""
    return b"/" + ch * (n - 1)


def path_record_len(name_len: int) -> int:
    """The length of "<n> path=<name>\\n", worked out by hand: 7 bytes around the name and
    n's own digits."""
    base = name_len + 7
    for digits in range(1, 7):
        if len(str(base + digits)) == digits:
            return base + digits
    raise AssertionError


LONG_SPLITS = b"/" + b"d" * 60 + b"/" + b"f" * 80  # ASCII, 142 bytes, splits: stays USTAR

PAX = [
    # 1-3 bytes that are not ASCII (record lengths 9, 11, 12: both sides of 9 / 11)
    ("1 byte", b"\xc3", 5),
    ("2 bytes", E, 0),
    ("3 bytes", EURO, 700),
    ("slash e-acute", b"/" + E, 0),
    ("e-acute dir and file", b"/" + E + b"/f", 3),
    ("e-acute dir", b"/" + E + b"/", 0),
    # record lengths on both sides of 99 / 101, 999 / 1001, 9999 / 10001
    ("record 99", b"/" + E + b"r" * 87, 1),
    ("record 101", b"/" + E + b"r" * 88, 1),
    ("record 999", flat(989), 1),
    ("record 1001", flat(990), 1),
    ("record 9999", flat(9988), 1),
    ("record 10001", flat(9989), 1),
    # records of 511, 512 and 513 bytes: the record blocks end before, at and after a block
    ("records 511", flat(501), 2),
    ("records 512", flat(502), 2),
    ("records 513", flat(503), 2),
    # names that do not split
    ("name 101", flat(101), 4),
    ("name 156", flat(156), 4),
    ("name 256", flat(256), 4),
    ("name 600", flat(600), 4),
    ("name 5000", flat(5000), 4),
    # not ASCII, over 100 bytes, would split: PAX all the same
    ("non-ASCII that would split", b"/" + b"d" * 60 + b"/" + E + b"f" * 80, 9),
    # the first 100 bytes after toASCII end in '/'
    ("main name cut at a slash", b"/" + b"a" * 98 + b"/" + E + b"tail", 9),
    ("entirely non-ASCII", E * 3, 9),
    # directories
    ("non-ASCII directory", b"/dir-" + E + b"/", 0),
    ("long directory", b"/" + b"q" * 120 + b"/", 0),
    # the extended header's name is cut at 100 bytes and then ends in '/'
    ("ext name cut at a slash", b"/" + b"z" * 85 + b"/" + E + b"x" * 30, 9),
    # an unrooted name, and one with no directory
    ("unrooted", b"rel/" + E + b".csv", 9),
]
assert [path_record_len(len(n)) for _, n, _ in PAX[6:15]] == \
    [99, 101, 999, 1001, 9999, 10001, 511, 512, 513]

HUGE = [  # sizes only a header can claim here
    ("size only", b"/big", 1 << 33),
    ("size 2^40 only", b"/big40", 1 << 40),
    ("path and size", b"/big-" + E, 1 << 40),
    ("splits, but too big: path and size", LONG_SPLITS, 1 << 33),
]

USTAR = [
    ("splits", LONG_SPLITS, 513),
    ("largest USTAR size", b"/big", (1 << 33) - 1),
    ("short", b"/a/b.txt", 5),
    ("100 bytes", b"/n" + b"a" * 98, 512),
    ("directory", b"/dir/", 0),
]

# PAX entries whose name path.Join would rewrite: refused with PAX on
NOT_CLEAN = [b"/a//" + E, b"/./" + E, b"/a/../" + E, E + b"//", b"//" + E, b"../" + E,
             b"/" + E + b"/.", b"/x/./" + flat(120)[1:]]
