"""Plain numpy / Python restatements of what the scan's one-workgroup tails produce, for the
tests that pin them (test_gpu_queues.py, test_gpu_past_4gib.py, test_cut_replay_model.py):

  plan_units        scan_skip_kernel: per work unit its static skip, tracked file and rank
  check_scan_plan   the dispatch slots of scan_skip_kernel + scan_slots_kernel against it
  check_hash_queue  lpt_order_block's order / next / qlen against the segments they order
  entry_list        compact_tiles: per 3 MiB tile its candidates, or one marker when dense
  tile_candidates   the oracle's candidates of a large batch, one tile per task

Test infrastructure only: nothing here runs on the product path.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

# the kernels' geometry (pfscdc_internal.h)
UNIT = 262_144        # kScanUnit: one wave's 64 strips
STEP = 8_192          # kUnitStep: the skip granularity
UNIT_FILES = 64       # files scan_skip_kernel looks at per unit
BUCKETS = 64          # kPlanBuckets: ranks >= 63 share the last dispatch bucket
RANK_CLAMP = 255      # the rank a slot word can hold
TILE = 3 << 20        # kTile
TILE_K = 15           # kTileK: candidates a tile record holds
DENSE_BIT = 1 << 63
NO_NEXT = 0xFFFFFFFF


def plan_units(offs, mn, unit=UNIT, step=STEP, unit_files=UNIT_FILES, buckets=BUCKETS,
               plan=True):
    """scan_skip_kernel: (unit, tracked file, rank, skipped steps) of every unit the scan
    still visits, in dispatch order up to the order inside a bucket (rank unclamped).
    plan=False: the first-min skip alone (no dispatch slots): a unit crowded with more than
    unit_files sub-min files is then scanned whole and has no tracked file (None)."""
    offs = np.asarray(offs).astype(np.int64)
    n = int(offs[-1])
    nfiles = len(offs) - 1
    kall = unit // step
    units = []
    for u in range((n + unit - 1) // unit):
        ub, ue = u * unit, min((u + 1) * unit, n)
        f = int(np.searchsorted(offs, ub, side="right") - 1)
        s, tf, rank = 0, None, 0  # the kernel starts from "scan whole" (a crowded unit)
        for g in range(f, f + unit_files):
            if g >= nfiles or offs[g] >= ue:
                s = kall
                break
            ls, fe = int(offs[g]) + mn - 1, int(offs[g + 1])
            if ls < fe:
                first = max(ls, ub)
                s = (first - ub) // step if first < ue else kall
                tf, rank = g, ub // unit - ls // unit
                break
        if tf is None and plan:
            s = kall  # plan mode: a crowded unit holds no eligible position, takes no slot
        if s < kall and ub + s * step < ue:
            units.append((u, tf, rank, s))
    units.sort(key=lambda t: (min(t[2], buckets - 1), t[0]))
    return units


def live_bytes(units, n, unit=UNIT, step=STEP):
    """Bytes the scan still rolls under the static skip of plan_units' units."""
    return sum(min((u + 1) * unit, n) - (u * unit + s * step) for (u, _, _, s) in units)


def check_scan_plan(slots, offs, mn):
    """The kernel's dispatch slots (Chunker.debug_scan_plan) against plan_units at the real
    geometry: the same set of (unit, file, skip, min(rank, 255)), every unit once, buckets
    min(rank, 63) non-decreasing along the slots (the order inside a bucket is free: the
    kernel places slots there with atomics).  Returns the model's units."""
    units = plan_units(offs, mn)
    want = sorted((u, f, s, min(r, RANK_CLAMP)) for (u, f, r, s) in units)
    slots = np.asarray(slots, dtype=np.uint32).reshape(-1, 3)
    assert len(slots) == len(want), f"{len(slots)} slots, the model has {len(want)}"
    got = sorted(zip(slots[:, 0].tolist(), slots[:, 1].tolist(),
                     (slots[:, 2] & 0xFF).tolist(), (slots[:, 2] >> 8).tolist()))
    if got != want:
        bad = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
        raise AssertionError(f"slot set differs first at {bad}: kernel {got[bad]}, model {want[bad]}")
    bucket = np.minimum(slots[:, 2] >> 8, BUCKETS - 1).astype(np.int64)
    down = np.flatnonzero(np.diff(bucket) < 0)
    assert len(down) == 0, f"rank buckets fall at slots {down[:5]}: {bucket[down[:5] + 1]}"
    return units


def lpt_key(length):
    """lpt_key of cdc_kernels.hip: ascending key = descending length, 8 KiB granularity."""
    length = np.asarray(length, dtype=np.uint64)
    nblk = (length + np.uint64(127)) // np.uint64(128)
    return 1023 - np.minimum(nblk >> np.uint64(6), 1023).astype(np.int64)


def check_hash_queue(order, nxt, bin_bytes, segs, offs):
    """The hash queue of a scan (Chunker.debug_hash_queue) against the segments it orders
    (themselves checked against the oracle by the caller) and the file offsets:
    a segment is binned iff bin_bytes != 0 and its file is at most bin_bytes long; the queue's
    entries are every unbinned segment and the first segment of every binned file, each once;
    longest first by lpt_key (a bin counts with its file's length); next links a binned
    segment to its file's following one."""
    offs = np.asarray(offs, dtype=np.uint64)
    nseg = len(segs)
    order = np.asarray(order, dtype=np.int64)
    file = segs["file"].astype(np.int64)
    flen = (offs[1:] - offs[:-1])[file] if nseg else np.zeros(0, np.uint64)
    binned = (flen <= np.uint64(bin_bytes)) if bin_bytes else np.zeros(nseg, dtype=bool)
    first = np.ones(nseg, dtype=bool)
    first[1:] = file[1:] != file[:-1]
    entries = np.flatnonzero(~binned | first)
    assert len(order) == len(entries), f"qlen {len(order)}, {len(entries)} entries expected"
    assert order.min(initial=0) >= 0 and order.max(initial=-1) < max(nseg, 1)
    srt = np.sort(order)
    assert np.array_equal(srt, entries), \
        f"the queue is no permutation of its entries (first bad: {np.flatnonzero(srt != entries)[:5]})"
    key = lpt_key(np.where(binned, flen, segs["size"].astype(np.uint64)))
    along = key[order]
    down = np.flatnonzero(np.diff(along) < 0)
    assert len(down) == 0, f"not longest first at queue positions {down[:5]}"
    if not bin_bytes:
        assert nxt is None
        return
    assert nxt is not None and len(nxt) == nseg
    linked = np.zeros(nseg, dtype=bool)
    linked[:-1] = binned[:-1] & (file[1:] == file[:-1])
    want = np.where(linked, np.arange(1, nseg + 1), NO_NEXT).astype(np.uint32)
    bad = np.flatnonzero(np.asarray(nxt, dtype=np.uint32) != want)
    assert len(bad) == 0, f"next differs at segments {bad[:5]}: {nxt[bad[:5]]} != {want[bad[:5]]}"


def tile_candidates(host, params, nthreads=16, cap=1 << 14):
    """The oracle's candidate positions (absolute, >= 63) of every 3 MiB tile of host, a list
    of uint64 arrays; one oracle run per tile over the tile's bytes with 64 bytes of halo in
    front (the hash at a position is a function of the 64 bytes ending there)."""
    from oracle import coracle

    n = len(host)

    def one(t):
        ts, te = t * TILE, min((t + 1) * TILE, n)
        a = max(ts - 64, 0)
        c = coracle.candidates(host[a:te], params, cap=cap)
        assert len(c) < cap
        c = c[c >= np.uint64(ts - a)] if ts else c
        return c + np.uint64(a)

    with ThreadPoolExecutor(nthreads) as pool:
        return list(pool.map(one, range((n + TILE - 1) // TILE)))


def entry_list(per_tile, n):
    """compact_tiles: the sorted entry list of a batch of n bytes from each tile's candidates:
    a tile's candidates if there are at most 15, otherwise one marker 1 << 63 | (tile_end - 1)."""
    out = []
    for t, c in enumerate(per_tile):
        if len(c) <= TILE_K:
            out.append(np.asarray(c, dtype=np.uint64))
        else:
            te = min((t + 1) * TILE, n)
            out.append(np.array([DENSE_BIT | (te - 1)], dtype=np.uint64))
    return np.concatenate(out) if out else np.zeros(0, np.uint64)
