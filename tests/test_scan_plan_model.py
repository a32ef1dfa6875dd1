"""The plan model the GPU tests hold against scan_skip_kernel (scan_models.plan_units), proved
here against the oracle and not against the kernel: on random layouts every cut the reference
rule makes over ALL candidates lies in a step the model's plan leaves scanned, in a unit that
tracks the cut's own file at the rank the kernel's rank slots assume.  A model that skipped
too much would agree with a kernel that skips too much; this test is what keeps the pair
honest.  The geometry is scaled down as in test_cut_replay_model.py (unit 1024, step 32,
min - 1 >= one unit), the bytes and the cuts are real: oracle/cdc_oracle.c over the synthetic
generator, cross-checked with that file's select_cuts over the oracle's candidates."""
import numpy as np
import pytest

import scan_models
from oracle import chunker as Ch
from oracle import coracle
from pfs_amd.cdc import synthetic_bytes
from test_cut_replay_model import STEP, U, select_cuts


def _layout(rng, mn):
    """A few MiB: runs of tiny files crowding units (more than 64 starts in one), empty,
    sub-min, around-min, unit-sized files, and long ones of 64+ ranks."""
    kinds = [lambda: 0, lambda: int(rng.integers(1, 15)), lambda: int(rng.integers(1, mn)),
             lambda: int(mn + rng.integers(-2, 3)), lambda: int(U + rng.integers(-2, 3)),
             lambda: int(rng.integers(mn, 12 * mn)), lambda: int(rng.integers(60 * U, 300 * U))]
    lens, total = [], 0
    while total < 3 << 20:
        k = int(rng.integers(0, len(kinds)))
        for _ in range(int(rng.integers(1, 300 if k <= 1 else 5))):
            lens.append(kinds[k]())
            total += lens[-1]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


@pytest.mark.parametrize("bits,mn,mx", [(8, 1100, 4000), (11, 1025, 3000), (6, 2200, 9000),
                                        (30, 1100, 2500)])
def test_the_plan_model_leaves_every_cut_scanned(bits, mn, mx):
    p = Ch.Params(average_bits=bits, seed=1, min=mn, max=mx)
    rng = np.random.default_rng(bits * 1000 + mn)
    ncuts = crowded = high_rank = 0
    for trial in range(3):
        offs = _layout(rng, mn)
        n = int(offs[-1])
        data = synthetic_bytes(offs, 40 + trial)
        if trial == 1:  # constant runs: candidates everywhere or nowhere
            a = int(rng.integers(0, n - 70_000))
            data[a:a + 70_000] = 0x5A
        cands = coracle.candidates(data, p, cap=1 << 22).astype(np.int64)
        segs, begin = coracle.segment_files(data, offs, p, do_hash=False)
        cut = (segs["flags"] & 2) != 0
        cuts = (offs[segs["file"]] + segs["offset"] + segs["size"] - np.uint64(1))[cut].astype(np.int64)
        cut_file = segs["file"][cut].astype(np.int64)
        mine = [c for f in range(len(offs) - 1)
                for c in select_cuts(cands, int(offs[f]), int(offs[f + 1]), mn, mx)]
        assert mine == cuts.tolist(), "select_cuts over the oracle's candidates != the oracle"
        ncuts += len(cuts)
        starts = np.bincount((offs[:-1] // np.uint64(U)).astype(np.int64))
        crowded += int(np.count_nonzero(starts > 64))
        for plan in (True, False):
            units = scan_models.plan_units(offs, mn, unit=U, step=STEP, plan=plan)
            ids = [u for (u, _, _, _) in units]
            assert len(set(ids)) == len(ids), "a unit is planned twice"
            by_unit = {u: (tf, rank, s) for (u, tf, rank, s) in units}
            for c, f in zip(cuts.tolist(), cut_file.tolist()):
                u = c // U
                assert u in by_unit, (plan, "the cut's unit is not scanned", c, f)
                tf, rank, s = by_unit[u]
                assert c >= u * U + s * STEP, (plan, "the cut lies in a skipped step", c, f, s)
                if plan:  # the replay reads file tf's rank slots for this unit
                    assert tf == f, (c, f, tf)
                    assert rank == u - (int(offs[f]) + mn - 1) // U, (c, f, rank)
                    high_rank += rank >= 63
            want = sum(min((u + 1) * U, n) - (u * U + s * STEP) for (u, _, _, s) in units)
            assert scan_models.live_bytes(units, n, unit=U, step=STEP) == want
            if plan:
                assert all(tf is not None for (_, tf, _, _) in units)
                buckets = [min(r, 63) for (_, _, r, _) in units]
                assert buckets == sorted(buckets)
    assert ncuts > 100 and crowded > 0 and high_rank > 0, (ncuts, crowded, high_rank)
