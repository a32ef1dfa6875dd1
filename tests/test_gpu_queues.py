"""What the scan's one-workgroup tails produce besides the segments: the hash queue of
lpt_order_block (order, next, qlen) and the rank-ordered dispatch slots of scan_skip_kernel +
scan_slots_kernel, read back through the two test hooks pfscdc_debug_hash_queue and
pfscdc_debug_scan_plan and held against plain numpy restatements (scan_models.py).

A queue that is not longest-first, or holds an entry twice, and a plan that visits a unit
twice or orders ranks wrongly, change no digest: they only cost time, so no parity test sees
them.  The segments the queue is checked over are first compared with the oracle; the plan
model is proved against the oracle on the CPU (test_scan_plan_model.py).  The same checks at
the sizes where the tails' loops wrap run over the 4 GiB batch of test_gpu_past_4gib.py.
"""
import numpy as np
import pytest

import scan_models
from oracle import chunker as Ch
from oracle import coracle
from pfs_amd import _lib
from pfs_amd.cdc import Chunker
from test_gpu_parity import DEFAULT, SMALL, _cut_skip_layout, assert_same, cp

pytestmark = pytest.mark.gpu


def device_batch(c, offs, seed):
    """(device tensor, host copy) of the synthetic stream of offs."""
    import torch

    t = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda:0")
    c.fill_synthetic(t, offs, seed)
    return t, t.cpu().numpy()


def offsets(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.uint64)


# ---- the hash queue ------------------------------------------------------------------------


@pytest.mark.parametrize("bins", [None, 0])
def test_queue_key_boundaries_one_segment_per_file(knob, bins):
    """Files of one segment each (a 40-bit mask and a huge max: the oracle reports no cut)
    whose sizes sit on both sides of the 8 KiB steps of lpt_key -- 8192k - 128 is the last
    size of key step k - 1, 8192k - 127 the first of step k -- at k = 1, 2 and 1023 (the
    clamp), two sizes past 8 MiB that share key 0, and sizes 0 and 1; bins auto and off."""
    p = Ch.Params(average_bits=40, seed=1, min=64, max=1 << 40)
    lens = [8192 * k + d for k in (1, 2, 1023) for d in (-128, -127, 0, 1)]
    lens += [(8 << 20) + 5, (9 << 20) + 77, 0, 1, 100, 8063, 8064, 8065, 0]
    rng = np.random.default_rng(3)
    lens = [int(x) for x in rng.permutation(lens)]
    offs = offsets(lens)
    if bins is not None:
        knob("PFSCDC_HASH_BIN_BYTES", bins)
    c = Chunker(cp(p), device=0)
    dev, host = device_batch(c, offs, 31)
    res = c.scan(dev, offs)
    segs, begin = coracle.segment_files(host, offs, p, nthreads=8)
    assert np.diff(begin.astype(np.int64)).max() == 1 and len(segs) == np.count_nonzero(lens)
    assert_same(res, host, offs, p)
    order, nxt, bin_bytes = c.debug_hash_queue()
    assert (bin_bytes == 0) == (bins == 0)
    scan_models.check_hash_queue(order, nxt, bin_bytes, res.segments, offs)
    # every key step the sizes were chosen for is there
    assert {0, 1, 1021, 1022, 1023} <= set(scan_models.lpt_key(res.segments["size"]).tolist())
    c.close()


@pytest.mark.parametrize("bins", [60_000, 0])
def test_queue_bins_around_the_bin_size(knob, bins):
    """SMALL parameters with the bin size fixed at B = 60,000: files of B - 1, B (binned),
    B + 1 (not), empty files, binned and unbinned files of many segments, more than 1,024
    segments in all (the 1,024-bin histogram's threads each see several); and bins off."""
    B = 60_000
    rng = np.random.default_rng(17)
    lens = np.concatenate([rng.integers(0, 70_000, 300), [B - 1, B, B + 1, 0, 0, 250_000, 1,
                                                          59_000, 400_000]])
    rng.shuffle(lens)
    offs = offsets(lens)
    knob("PFSCDC_HASH_BIN_BYTES", bins)
    c = Chunker(cp(SMALL), device=0)
    dev, host = device_batch(c, offs, 23)
    res = c.scan(dev, offs)
    segs, begin = coracle.segment_files(host, offs, SMALL, nthreads=8)
    per_file = np.diff(begin.astype(np.int64))
    assert len(segs) > 1024
    assert per_file[lens <= B].max() > 4 and per_file[lens > B].max() > 4
    assert_same(res, host, offs, SMALL)
    order, nxt, bin_bytes = c.debug_hash_queue()
    assert bin_bytes == bins
    scan_models.check_hash_queue(order, nxt, bin_bytes, res.segments, offs)
    if bins:
        assert len(order) < len(segs)
    else:
        assert len(order) == len(segs)
    c.close()


def test_queue_of_an_empty_batch():
    c = Chunker(cp(SMALL), device=0)
    for offs in ([0], [0, 0, 0]):
        res = c.scan(b"", offs)
        order, nxt, bin_bytes = c.debug_hash_queue()
        assert len(order) == 0
        scan_models.check_hash_queue(order, nxt, bin_bytes, res.segments, np.array(offs))
        assert len(c.debug_scan_plan()) == 0
    c.close()


# ---- the cut-skipping plan -----------------------------------------------------------------


def plan_case(knob, p, offs, seed, grid=None):
    """Scan offs' synthetic stream with the plan on, compare with the oracle, hold the slots
    against the model; then the static skip alone: no slots, and exactly the model's bytes."""
    if grid:
        knob("PFSCDC_SCAN_GRID", grid)
    c = Chunker(cp(p), device=0)
    dev, host = device_batch(c, offs, seed)
    res = c.scan(dev, offs)
    assert_same(res, host, offs, p)
    both = _lib.SCAN_SKIPPED_FIRST_MIN | _lib.SCAN_SKIPPED_CUTS
    assert c.last_scan_mode() == both
    n = int(offs[-1])
    units = scan_models.check_scan_plan(c.debug_scan_plan(), offs, p.min)
    assert 0 < c.last_scan_bytes() <= scan_models.live_bytes(units, n)
    knob("PFSCDC_SCAN_CUTSKIP", 0)
    assert_same(c.scan(dev, offs), host, offs, p)
    assert c.last_scan_mode() == _lib.SCAN_SKIPPED_FIRST_MIN
    assert len(c.debug_scan_plan()) == 0
    static = scan_models.plan_units(offs, p.min, plan=False)
    assert c.last_scan_bytes() == scan_models.live_bytes(static, n)
    knob("PFSCDC_SCAN_CUTSKIP", None)
    c.close()
    return units


@pytest.mark.parametrize("bits,min_,max_,grid", [(18, 262_145, 700_000, None),
                                                 (16, 300_000, 1_200_000, 1)])
def test_plan_slots_of_the_cut_skip_layout(knob, bits, min_, max_, grid):
    """_cut_skip_layout: file lengths around min, the unit and the step, empty files, and
    whole units crowded with more than 64 sub-min files (they take no slot with the plan and
    are scanned whole without it); min - 1 exactly one unit, and above."""
    lens, offs = _cut_skip_layout(min_)
    units = plan_case(knob, Ch.Params(average_bits=bits, seed=1, min=min_, max=max_), offs,
                      300 + bits, grid)
    planned = {u for (u, _, _, _) in units}
    starts = np.bincount((offs[:-1] // np.uint64(scan_models.UNIT)).astype(np.int64))
    crowded = set(np.flatnonzero(starts > 64).tolist())
    assert crowded and len(crowded - planned) > 0, "no crowded unit without a slot"


@pytest.mark.parametrize("mib,lo,hi", [(17.5, 63, 255), (66, 255, 1 << 30)])
def test_plan_ranks_across_the_shared_bucket_and_the_clamp(knob, mib, lo, hi):
    """One file at the reference parameters: 17.5 MiB has ranks on both sides of 63 (the
    bucket every later rank shares), 66 MiB on both sides of 255 (the slot word's clamp)."""
    n = int(mib * (1 << 20)) + 37
    units = plan_case(knob, DEFAULT, np.array([0, n], dtype=np.uint64), 0xA1)
    top = max(r for (_, _, r, _) in units)
    assert lo < top < hi, top


def test_no_plan_for_a_batch_of_mostly_tiny_files():
    """nfiles * 16384 > nbytes: the rank slots would outweigh the bytes, the scan keeps the
    first-min skip alone and reports no slots."""
    lens = [10_000] * 200
    offs = offsets(lens)
    assert (len(offs) - 1) * 16384 > int(offs[-1])
    c = Chunker(cp(DEFAULT), device=0)
    dev, host = device_batch(c, offs, 9)
    assert_same(c.scan(dev, offs), host, offs, DEFAULT)
    assert c.last_scan_mode() == _lib.SCAN_SKIPPED_FIRST_MIN
    assert len(c.debug_scan_plan()) == 0
    c.close()
