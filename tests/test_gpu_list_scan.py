"""The prefix-sum kernels of the index list passes alone (pfscdc_debug_list_scan):
index_scan_kernel ({records, blob bytes} per frame), merge_scan_kernel ({entries, DataRefs, blob
bytes} per item) and rtar_scan_kernel (the tar plan's saturating sums) against sums made with
Python integers.  Sizes on both sides of
a tile of 1,024 and with two and three carries; every comparison is exact."""
import random

import numpy as np
import pytest

from pfs_amd import fileset as pf
from pfs_amd.cdc import ChunkParams, Chunker

pytestmark = pytest.mark.gpu

TILE = 1024  # kIdxScanBlock
CAP = (1 << 62) + 1  # kRtarCap
SIZES = [0, 1, 1023, 1024, 1025, 2048, 2049, 3073]
COLS = {0: 2, 1: 3, 2: 1}


@pytest.fixture(scope="module")
def chunker():
    c = Chunker(ChunkParams(), 0)
    yield c
    c.close()


def expected(kind, rows):
    """rows: n tuples of Python integers; the n + 1 rows of exclusive sums, the totals last."""
    s = [0] * COLS[kind]
    out = [tuple(s)]
    for r in rows:
        s = [min(a + v, CAP) if kind == 2 else a + v for a, v in zip(s, r)]
        out.append(tuple(s))
    return out


def check(chunker, kind, rows):
    dtype = pf._LIST_SCAN_KINDS[kind][0]
    rec = np.array([r[0] for r in rows] if kind == 2 else rows, dtype=dtype)
    assert len(rec) == len(rows)
    got = pf.list_scan(chunker, kind, rec)
    assert got.shape == (len(rows) + 1, COLS[kind])
    want = expected(kind, rows)
    assert [tuple(int(x) for x in g) for g in got] == want
    return want


def random_rows(kind, n, rng):
    def u32():  # 0xffffffff often enough that a column's sum passes 2^32 inside a tile
        return 0xffffffff if rng.random() < 0.25 else rng.randrange(1 << 32)
    if kind == 0:
        return [(u32(), u32()) for _ in range(n)]
    return [(u32(), u32(), rng.randrange(1 << 40)) for _ in range(n)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", [0, 1])
def test_counts(chunker, kind, n):
    rng = random.Random(1000 * kind + n)
    want = check(chunker, kind, random_rows(kind, n, rng))
    if n >= TILE:
        assert want[TILE][0] > 1 << 32
    check(chunker, kind, [(0,) * COLS[kind]] * n)
    # nothing but the last item of tile 0 and the first of tile 1
    rows = [(0,) * COLS[kind]] * n
    for i, v in ((TILE - 1, 0xffffffff), (TILE, 7)):
        if i < n:
            rows[i] = (v,) * COLS[kind]
    check(chunker, kind, rows)


@pytest.mark.parametrize("n", SIZES)
def test_saturating_small(chunker, n):
    rng = random.Random(2000 + n)
    check(chunker, 2, [(rng.randrange(1 << 20),) for _ in range(n)])


def test_saturating_meets_the_cap_at_a_tile_edge(chunker):
    """Every value 2^52: the sum is 2^62 before item 1,024, the first of tile 1, and the cap
    from there on."""
    n = 2 * TILE + 1
    want = check(chunker, 2, [(1 << 52,)] * n)
    assert want[TILE] == (1 << 62,)
    assert all(w == (CAP,) for w in want[TILE + 1:])


@pytest.mark.parametrize("at", [0, 1500])
def test_saturating_cap_as_an_item(chunker, at):
    rng = random.Random(3000 + at)
    rows = [(rng.randrange(1 << 20),) for _ in range(2 * TILE + 1)]
    rows[at] = (CAP,)
    want = check(chunker, 2, rows)
    assert all(w == (CAP,) for w in want[at + 1:])
