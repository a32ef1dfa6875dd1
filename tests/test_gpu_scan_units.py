"""The scan keeps a unit's state (unit, skip, file | rank) in scalar registers.  A value that is
scalar for the compiler but not the same in every lane, or one carried over from the previous
unit, would show where a wave takes many units in a row that differ in all three: one scan
workgroup (PFSCDC_SCAN_GRID=1) over about 40 files of 0.3-2.5 MiB whose lengths and offsets
miss every 64 B, 4 KiB, 256 KiB and 3 MiB boundary, each file with several cuts.

Parameters: average_bits 16 with min 70,000 / max 700,000, and with min 270,001 / max 700,000.
Cut skipping (the ScanPlan, whose slots the unit state is read from) is in force only from
min - 1 >= one 256 KiB unit, so the first set runs the plain unit order under either setting
of the PFSCDC_SCAN_CUTSKIP knob and the second set is the one where settled cuts skip steps.
Both run under both settings, the wide form (33-bit mask) too, and a single stream of
5 MiB + 37 B ends in a partial unit, which takes the slow DMA path.

Records and digests equal the oracle's.  The bytes the scan rolled (Chunker.last_scan_bytes)
are pinned to what the kernel rolled before its unit state became scalar, wherever that is one
number: without the plan, and for the single stream, it is a function of the layout alone (four
runs of the earlier kernel and four of this one gave the same count each).  With the plan over
the 40 files a unit skips what its file's earlier units had settled when it started, and the
twelve waves of the one workgroup run ranks of the same file side by side near the end of the
rank order: the earlier kernel itself rolled 35,258,368 / 35,315,712 / 35,356,672 / 35,758,080
bytes in four runs (33-bit mask: 45,932,544 to 46,292,992), this one 34,684,928 to 35,373,056
(46,292,992 to 46,776,320).  There is no one value to pin there, so those two runs are held
between bounds that do not come from the kernel: above, the count with cut skipping off (pinned;
the plan only ever takes steps away); below, the live positions of the oracle's segments -- a
segment's first min - 1 positions are the only ones a settled cut makes dead, so every other
position of every segment has to be rolled -- and skipping must have happened at all."""
import numpy as np
import pytest

from oracle import chunker as Ch
from oracle import coracle
from pfs_amd.cdc import ChunkParams, Chunker, synthetic_bytes

pytestmark = pytest.mark.gpu

PLAIN = dict(min=70_000, max=700_000)   # below one unit: no plan
PLAN = dict(min=270_001, max=700_000)   # the cut-skipping plan is in force


def _layout():
    """40 file lengths in [0.3, 2.5] MiB; no length and no offset on a 64-byte boundary (so on
    no 4 KiB, 256 KiB or 3 MiB boundary either)."""
    rng = np.random.default_rng(20250)
    lens, off = [], 0
    for n in rng.integers(300 * 1024, 2560 * 1024, 40):
        n = int(n)
        while n % 64 == 0 or (off + n) % 64 == 0:
            n += 1
        lens.append(n)
        off += n
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    for b in (64, 4096, 262_144, 3 << 20):
        assert all(n % b for n in lens) and all(int(o) % b for o in offs[1:])
    return offs


_CASES = {}


def case(name):
    """(data, offs) of a layout, made once."""
    if name not in _CASES:
        offs = _layout() if name == "files" else np.array([0, (5 << 20) + 37], dtype=np.uint64)
        _CASES[name] = (synthetic_bytes(offs, 77 if name == "files" else 78), offs)
    return _CASES[name]


_ORACLE = {}


def oracle(name, p):
    if (name, p) not in _ORACLE:
        data, offs = case(name)
        _ORACLE[(name, p)] = coracle.segment_files(data, offs, p, nthreads=8)
    return _ORACLE[(name, p)]


def assert_same(res, name, p):
    segs, begin = oracle(name, p)
    g = res.segments
    assert np.array_equal(res.file_begin, begin), "per-file segment counts differ"
    assert len(g) == len(segs)
    for field in ("offset", "size", "file", "flags"):
        bad = np.nonzero(g[field] != segs[field])[0]
        assert len(bad) == 0, f"{field} differs at segments {bad[:5]}: gpu={g[bad[:5]]} cpu={segs[bad[:5]]}"
    bad = np.nonzero((g["hash"] != segs["hash"]).any(axis=1))[0]
    assert len(bad) == 0, f"digests differ at segments {bad[:5]}"


# Chunker.last_scan_bytes() of the kernel before this change for these inputs, one workgroup:
# (layout, average_bits, min, PFSCDC_SCAN_CUTSKIP) -> bytes rolled; a pair: the bounds of a
# run whose count depends on timing (the count with cut skipping off, and above the live
# positions of the oracle's segments)
FILES_BYTES, STREAM_BYTES = 57_468_489, 5_242_917
ROLLED = {
    ("files", 16, 70_000, 0): 57_075_273,
    ("files", 16, 70_000, 1): 57_075_273,
    ("files", 16, 270_001, 0): 51_897_929,
    ("files", 16, 270_001, 1): ("live", 51_897_929),
    ("files", 33, 70_000, 1): 57_075_273,
    ("files", 33, 270_001, 1): ("live", 51_897_929),
    ("stream", 16, 70_000, 0): 5_177_381,
    ("stream", 16, 70_000, 1): 5_177_381,
    ("stream", 16, 270_001, 0): 4_980_773,
    ("stream", 16, 270_001, 1): 4_980_773,
}


def live_bytes(name, p):
    """The positions no settled cut can make dead: all but the first min - 1 of each segment."""
    segs, _ = oracle(name, p)
    return int(np.maximum(segs["size"].astype(np.int64) - (p.min - 1), 0).sum())


def run(knob, name, bits, lim, cutskip):
    knob("PFSCDC_SCAN_GRID", 1)
    knob("PFSCDC_SCAN_CUTSKIP", cutskip)
    p = Ch.Params(average_bits=bits, seed=1, **lim)
    data, offs = case(name)
    assert int(offs[-1]) == (FILES_BYTES if name == "files" else STREAM_BYTES)
    c = Chunker(ChunkParams(p.average_bits, p.seed, p.min, p.max), device=0)
    try:
        res = c.scan(data, offs)
        rolled = c.last_scan_bytes()
    finally:
        c.close()
    want = ROLLED[(name, bits, lim["min"], cutskip)]
    live = live_bytes(name, p)
    print(f"rolled[{name!r}, {bits}, {lim['min']}, {cutskip}] = {rolled} of {int(offs[-1])}, "
          f"live {live}, pinned {want}")
    assert_same(res, name, p)
    if isinstance(want, tuple):
        assert live <= rolled < want[1], (live, rolled, want[1])
    else:
        assert live <= rolled == want, (live, rolled, want)
    return rolled, res


@pytest.mark.parametrize("cutskip", [0, 1])
@pytest.mark.parametrize("lim", [PLAIN, PLAN], ids=["min70000", "min270001"])
def test_many_units_per_wave_across_files(knob, lim, cutskip):
    _, res = run(knob, "files", 16, lim, cutskip)
    per_file = np.diff(res.file_begin)
    assert np.median(per_file) >= 3, per_file  # the files carry several cuts each


@pytest.mark.parametrize("lim", [PLAIN, PLAN], ids=["min70000", "min270001"])
def test_wide_form_many_units_per_wave(knob, lim):
    run(knob, "files", 33, lim, 1)


@pytest.mark.parametrize("cutskip", [0, 1])
@pytest.mark.parametrize("lim", [PLAIN, PLAN], ids=["min70000", "min270001"])
def test_single_stream_ends_on_the_slow_dma_path(knob, lim, cutskip):
    run(knob, "stream", 16, lim, cutskip)
