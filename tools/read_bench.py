"""Read path on one GPU, device-resident: pfscdc_read_slices (chunk.Reader.Get: verify each
referenced chunk once, decrypt only the referenced bytes) over seeded synthetic chunks that are
encrypted on the GPU with their own Ref.Dek, as benchkit/get.py does.  Three layouts:

  whole   one DataRef per chunk (the whole chunk), alternated in the same process with
          pfscdc_get_chunks on the same bytes
  packed  64 odd-sized slices per chunk, at odd offsets
  sparse  one 4 KiB slice per chunk, every chunk marked verified (the memCache hit)

Per layout: median device ms of the verification and of the gather kernel after a warm-up, and
the gather's (bytes read + bytes written) / ms against benchkit.common.HBM_PEAK_GBS, the
gather kernel's share of HBM peak.  Every output is compared with the plaintext before
anything is printed.  Writes one JSON (default profiles/r7/read_path/read_bench.json).

--tar: the same three layouts as GetFileTAR streams (pfscdc_read_tar, one file per slice),
alternated in the same process with pfscdc_read_slices over the same slices (the yardstick: its
code does not change with the tar path).  Per layout two lines, one with ASCII names (USTAR
entries) and one with names that are not ASCII and PAX allowed (every entry a PAX entry): stream
bytes, median device ms of the verification, the gather and tar_frame_kernel, the wall ms of the
read_tar call, and read_slices' two figures, with their spreads.  The first tar stream of each
line is checked: every file's content against the plaintext, sampled heads against
pfscdc_tar_head, padding and trailer zero.  Writes profiles/r8/read_tar/read_tar.json.

--index: reading a fileset back (pfscdc_index_read).  Two commits are written through the
unordered writer into a store at the reference's index parameters, 65,536 files of 4 KiB and
1,048,576 files of 256 B, and the additive root of each is read back with the device decode
(PFSCDC_INDEX_DECODE=1) and the host decode (0), the arms alternating call by call.  Per arm:
median, min and max of the call's wall time and of its stages (read-path verification and
gather of the index chunks, frame walk with the re-walk count, decode, copy to the host).
Every list is compared, array for array, with pfscdc_index_decode_host over the writer's own
level-0 index events, and its first and last 500 entries with the events decoded by the protobuf
runtime.  Writes profiles/r9/index_read/index_read.json.

--merge: MergeReader over index lists (pfscdc_index_merge_ctx), the device arm
(PFSCDC_INDEX_MERGE=1) and the host arm (0) alternating call by call, in both modes (iterate,
iterateDeletive).  Two shapes, each file Put without append (a deletive and an additive entry
with one DataRef per file): two filesets of 524,288 files, and ten filesets of 104,858 files
of which 10,486 are in every fileset.  The lists are assembled from fixed-layout frames and
decoded by pfscdc_index_decode_host.  Per arm: median, min and max of the call's wall time and
of the device arm's stages; every output is compared array for array between the arms.  Writes
profiles/r10/compact/merge.json.

--compact: one compaction of a commit of two filesets (--files files of 256 B: the even files,
then the odd files again with every 16th file deleted), split into index reads, merges, copies
(cheap-copied against re-rolled bytes) and close.  Writes profiles/r10/compact/compact.json.

--resident: the two commits of --index opened and rendered as tar, the host hand-over
(pfscdc_index_read of both roots, pfscdc_index_merge_ctx with PFSCDC_INDEX_MERGE=1,
pfscdc_store_read_tar of the first 64 MiB window into a device tensor) against the same through
the resident calls (pfscdc_index_read_dev, pfscdc_index_merge_dev, pfscdc_dev_list_read_tar),
alternating call by call.  Per arm: median, min and max of each stage's and the whole call's wall
time; the bytes each arm copies across the host link besides chunk ciphertext (the resident
arm's tar figures are the library's tallies of its copies; the host arm's are computed from the
lists' array sizes and from what pfscdc_store_read_tar uploads per piece, entry and chunk); the
window's runs.
Every resident window is compared with the host hand-over's bytes.  Writes
profiles/r11/resident/resident.json.

--source: the Source (pfscdc_source_open: directory entries, path predicate, FileInfo) over the
index lists of --index's two commits (65,536 files of 4 KiB, --files files of 256 B), laid out
over a directory tree of fan-out 64 and flat, as a resident input: SUBTREE("") and GET of one
second-level directory (flat: of the one directory), the device arm (PFSCDC_SOURCE=1) and the
host arm (0) alternating call by call.  Per arm: median, min and max of each stage's (insert and
select, sizes, leaf hashes, the directory levels) and the whole call's wall time, and the stats'
counts and bytes each way.  Every device result is compared with the host arm's, array for array
and info for info.  Writes profiles/r12/source/source.json.

--diff: DiffFile (pfscdc_source_diff) over two resident commits of 65,536 files of 4 KiB and of
--files files of 256 B at fan-out 64, the new commit the old one with 1 % of the files' content
changed, 8 files added and 8 removed: the device arm (PFSCDC_DIFF=1) and the host arm (0:
download of both sides, pfscdc_diff_host, upload of the pairs and the selections) alternating call
by call, with the two pfscdc_source_open calls timed beside them.  Per arm: median, min and max of
each stage's and the whole call's wall time and of what the call leaves behind (after_ms: the
diff's release and an upload of 16,384 entries, timed after every call so that no arm's figure
holds the other's leftovers), the counts and the bytes each way.  The arms' pairs
and selections are compared array for array.  Writes profiles/r7/read_path/diff.json.

--copy: CopyFile's selection and path transform (pfscdc_dev_list_copy_map) over resident lists of
65,536 files of 4 KiB and of --files files of 256 B, at fan-out 64 and flat, the second half of
each under /c instead of /b, so that src = /b selects half: the device arm (PFSCDC_COPY_MAP=1) and
the host arm (0: download, pfscdc_copy_map_host, upload) alternating call by call.  Per arm:
median, min and max of the call's stages and wall time (map_ms), and of the map together with
what pfscdc_uw_copy needs next, the selection on the host (flow_ms: the device arm downloads its
result; the host arm downloads the whole list and calls pfscdc_copy_map_host on it, with no
upload).  The arms' arrays are compared.  One copy_file of a directory of 1,024 files of 256 KiB
whose chunks pass by reference is recorded beside them.  Writes
profiles/r7/read_path/copy.json.

--glob: GlobFile (pfscdc_source_open with PFSCDC_SRC_GLOB) over resident lists of 65,536 files of
4 KiB and of --files files of 256 B at fan-out 64, five globs ("/**", "/*/*/f1*" and "/**.2",
which select nothing in this tree, "/b/*/0?/**" and "/**1"), the device arm (PFSCDC_SOURCE=1) and
the host arm (0) alternating call by call, and SUBTREE("") on the device arm beside them.  Per
arm: median, min and max of each stage's and the whole call's wall time.  The arms' first results
are compared array for array and info for info.  Writes profiles/r25/glob/glob.json.

usage: python tools/read_bench.py [--tar | --index | --merge | --compact | --resident | --source
                                   | --diff | --copy | --glob]
                                  [--chunks N]
                                  [--chunk-bytes B] [--files N] [--reps R] [--warmup W]
                                  [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchkit.common import HBM_PEAK_GBS  # noqa: E402
from pfs_amd import _lib  # noqa: E402
from pfs_amd.cdc import ChunkParams, Chunker  # noqa: E402


def layouts(nchunks, cb, rng):
    """name -> (slices, verified, per-chunk (source offset, bytes) of the consecutive run)."""
    sdt = _lib.slice_dtype()
    whole = np.zeros(nchunks, dtype=sdt)
    whole["chunk"] = np.arange(nchunks)
    whole["size"] = cb
    per = 64
    sizes = 2 * rng.integers(0, cb // (2 * per) - 1, (nchunks, per)) + 1  # odd, sum < cb - 1
    offs = 1 + np.concatenate([np.zeros((nchunks, 1), dtype=np.int64),
                               np.cumsum(sizes, axis=1)[:, :-1]], axis=1)
    packed = np.zeros(nchunks * per, dtype=sdt)
    packed["chunk"] = np.repeat(np.arange(nchunks), per)
    packed["offset"] = offs.ravel()
    packed["size"] = sizes.ravel()
    sparse = np.zeros(nchunks, dtype=sdt)
    sparse["chunk"] = np.arange(nchunks)
    sparse["offset"] = rng.integers(0, cb - 4096 + 1, nchunks)
    sparse["size"] = 4096
    return {
        "whole": (whole, None, [(0, cb)] * nchunks),
        "packed": (packed, None, [(1, int(s)) for s in sizes.sum(axis=1)]),
        "sparse": (sparse, np.ones(nchunks, dtype=np.uint8),
                   [(int(o), 4096) for o in sparse["offset"]]),
    }


def check(out, data, cb, runs):
    """out is the concatenation of data[c * cb + o : ... + n] over the per-chunk runs."""
    at = 0
    for c, (o, n) in enumerate(runs):
        if not torch.equal(out[at:at + n], data[c * cb + o:c * cb + o + n]):
            raise SystemExit(f"read_bench: output differs from the plaintext in chunk {c}")
        at += n
    assert at == out.numel()


def check_tar(out, data, cb, sl, names, offs, total, pax=False):
    """The tar stream in out: every file's content is the plaintext of its slice, sampled
    heads are pfscdc_tar_head's, the sampled files' padding and the trailer are zero."""
    from pfs_amd.fileset import tar_head
    chunk, off, size = (sl[k].astype(np.int64) for k in ("chunk", "offset", "size"))
    hl = len(tar_head(names[0], int(size[0]), pax))  # (the names are equally long)
    for i in range(len(sl)):
        a, b = int(chunk[i]) * cb + int(off[i]), int(offs[i]) + hl
        if not torch.equal(out[b:b + int(size[i])], data[a:a + int(size[i])]):
            raise SystemExit(f"read_bench: tar content differs from the plaintext in file {i}")
    for i in sorted({0, 1, len(sl) // 2, len(sl) - 1} | set(range(0, len(sl), max(1, len(sl) // 61)))):
        at, z = int(offs[i]), int(size[i])
        if out[at:at + hl].cpu().numpy().tobytes() != tar_head(names[i], z, pax):
            raise SystemExit(f"read_bench: tar head {i} differs from pfscdc_tar_head")
        if int(out[at + hl + z:int(offs[i + 1])].max().item() if -z % 512 else 0) != 0:
            raise SystemExit(f"read_bench: tar padding of file {i} is not zero")
    if int(out[total - 1024:total].max().item()) != 0:
        raise SystemExit("read_bench: tar trailer is not zero")


def tar_rows(args, c, data, ctext, cofs, refs, n, cb):
    """Per layout two lines: the USTAR stream, and the same files under names that are not
    ASCII, every entry a PAX entry (names "pax": a three-block head per file)."""
    rows = []
    med = statistics.median
    for name, (sl, ver, runs) in layouts(n, cb, np.random.default_rng(7)).items():
        payload = int(sl["size"].sum())
        out = torch.empty(payload, dtype=torch.uint8, device="cuda:0")
        for pax in (False, True):
            names = [("/bench/%s/é%07d" if pax else "/bench/%s/%07d") % (name, i)
                     for i in range(len(sl))]
            files = [(p, i, 1) for i, p in enumerate(names)]
            head = 1536 if pax else 512  # (a 23-byte name: one block of records)
            padded = (sl["size"].astype(np.int64) + 511) // 512 * 512 + head
            offs = np.concatenate([[0], np.cumsum(padded)])
            total = int(offs[-1]) + 1024
            tout = torch.empty(total, dtype=torch.uint8, device="cuda:0")
            t_v, t_g, t_f, t_c, s_v, s_g = [], [], [], [], [], []
            for i in range(args.warmup + args.reps):
                out.fill_(0xA5)
                _, cok, _ = c.read_slices(ctext, cofs, refs, sl, out=out, verified=ver)
                s = c.last_read_timings()
                if not cok.all():
                    raise SystemExit(f"read_bench: {name}: a chunk failed verification")
                check(out, data, cb, runs)
                tout.fill_(0xA5)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, cok, nw = c.read_tar(ctext, cofs, refs, files, sl, out=tout, verified=ver,
                                        pax=pax)
                call_ms = (time.perf_counter() - t0) * 1e3
                t = c.last_read_timings()
                fms = c.last_frame_ms()
                if not cok.all() or nw != total:
                    raise SystemExit(f"read_bench: {name}: tar read failed")
                if i == 0:
                    check_tar(tout, data, cb, sl, names, offs, total, pax)
                if i >= args.warmup:
                    s_v.append(s["verify"])
                    s_g.append(s["gather"])
                    t_v.append(t["verify"])
                    t_g.append(t["gather"])
                    t_f.append(fms)
                    t_c.append(call_ms)
            row = {"layout": name, "names": "pax" if pax else "ustar", "chunks": n,
                   "chunk_bytes": cb, "files": int(len(sl)),
                   "payload_bytes": payload, "stream_bytes": total,
                   "header_padding_trailer_bytes": total - payload,
                   "tar_verify_ms_median": round(med(t_v), 4),
                   "tar_gather_ms_median": round(med(t_g), 4),
                   "tar_gather_ms_min_max": [round(min(t_g), 4), round(max(t_g), 4)],
                   "tar_frame_ms_median": round(med(t_f), 4),
                   "tar_frame_ms_min_max": [round(min(t_f), 4), round(max(t_f), 4)],
                   "tar_call_ms_median": round(med(t_c), 3),
                   "tar_call_ms_min_max": [round(min(t_c), 3), round(max(t_c), 3)],
                   "read_slices_verify_ms_median": round(med(s_v), 4),
                   "read_slices_gather_ms_median": round(med(s_g), 4),
                   "read_slices_gather_ms_min_max": [round(min(s_g), 4), round(max(s_g), 4)],
                   "reps": args.reps, "warmup": args.warmup, "first_stream_checked": True}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del tout
        del out
    return rows


def list_arrays(lst):
    """The three arrays of an IndexList as bytes."""
    import ctypes as C
    n, ents, _, drs, ndr = lst._views()
    blen = C.c_uint64()
    bp = lst.lib.pfscdc_index_list_blob(lst._p, C.byref(blen))
    return (C.string_at(ents, 64 * n) if n else b"", C.string_at(bp, blen.value) if blen.value else b"",
            C.string_at(drs, 128 * ndr) if ndr else b"")


def index_rows(args):
    import time

    from oracle import fileset as OF
    from pfs_amd import chunk as pc
    from pfs_amd import fileset as PF
    rows = []
    for nfiles, fbytes in ((65536, 4096), (1 << 20, 256)):
        store = pc.ChunkStore()
        st = PF.Storage(0, ChunkParams(), store=store)
        w = st.new_unordered_writer()
        data = np.random.default_rng(nfiles).integers(0, 256, nfiles * fbytes + 64, dtype=np.uint8)
        t0 = time.perf_counter()
        for i in range(nfiles):
            w.put("/bench/d%03d/f%07d" % (i >> 12, i), "", False, data[i * fbytes:(i + 1) * fbytes])
        infos = w.close()
        write_s = time.perf_counter() - t0
        frames = [e[2] for e in w.events[0] if e[0] == "index" and e[1] == 0]
        index_chunks = sum(1 for e in w.events[0] if e[0] == "chunk" and e[1] == 0)
        w.release()
        assert len(infos) == 1 and len(frames) == nfiles
        want = list_arrays(PF.index_decode_host(b"".join(frames)))
        M = OF._msgs()["Index"]
        c = Chunker(ChunkParams(), 0)
        keys = ["verify_ms", "gather_ms", "walk_ms", "decode_ms", "d2h_ms"]
        runs = {1: [], 0: []}
        for i in range(args.warmup + args.reps):
            for arm in (1, 0):
                _lib.set_knob("PFSCDC_INDEX_DECODE", arm)
                t0 = time.perf_counter()
                lst = PF.index_read(c, store, infos[0].additive)
                wall = (time.perf_counter() - t0) * 1e3
                stats = PF.last_index_stats(c)
                if list_arrays(lst) != want:
                    raise SystemExit("read_bench: the list differs from the writer's events")
                if i == 0:
                    raw = lst.raw()
                    for k in list(range(500)) + list(range(nfiles - 500, nfiles)):
                        m = M.FromString(frames[k][8:])
                        got = raw[k]
                        if (got["path"], got["tag"]) != (m.path.encode(), m.file.tag.encode()) or \
                                [(d.ref.id, d.hash, d.offset_bytes, d.size_bytes) for d in got["data_refs"]] != \
                                [(d.ref.id, d.hash, d.offset_bytes, d.size_bytes) for d in m.file.data_refs]:
                            raise SystemExit(f"read_bench: entry {k} differs from its event")
                lst.free()
                if i >= args.warmup:
                    stats["wall_ms"] = wall
                    runs[arm].append(stats)
        _lib.set_knob("PFSCDC_INDEX_DECODE", 1)
        c.close()
        row = {"files": nfiles, "file_bytes": fbytes, "index_stream_bytes": sum(map(len, frames)),
               "index_chunks_all_levels": index_chunks, "write_s": round(write_s, 2),
               "reps": args.reps, "warmup": args.warmup, "lists_equal_events": True}
        for arm, name in ((1, "device"), (0, "host")):
            r = runs[arm]
            row[name] = {k: {"median": round(statistics.median(x[k] for x in r), 3),
                             "min": round(min(x[k] for x in r), 3),
                             "max": round(max(x[k] for x in r), 3)} for k in keys + ["wall_ms"]}
            row[name].update({k: r[0][k] for k in ("chunks_read", "rewalked_chunks", "levels", "frames")})
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def resident_rows(args):
    """--resident: the two commits of --index opened and rendered, host hand-over against the
    resident calls, alternating call by call."""
    import ctypes as C
    import time

    from pfs_amd import chunk as pc
    from pfs_amd import fileset as PF
    window = 64 << 20
    rows = []
    for nfiles, fbytes in ((65536, 4096), (1 << 20, 256)):
        store = pc.ChunkStore()
        st = PF.Storage(0, ChunkParams(), store=store)
        w = st.new_unordered_writer()
        data = np.random.default_rng(nfiles).integers(0, 256, nfiles * fbytes + 64, dtype=np.uint8)
        for i in range(nfiles):
            w.put("/bench/d%03d/f%07d" % (i >> 12, i), "", False, data[i * fbytes:(i + 1) * fbytes])
        infos = w.close()
        w.release()
        assert len(infos) == 1
        roots = (infos[0].deletive, infos[0].additive)
        c = Chunker(ChunkParams(), 0)
        lib = c.lib
        out_a = torch.empty(window, dtype=torch.uint8, device="cuda:0")
        out_b = torch.empty(window, dtype=torch.uint8, device="cuda:0")
        _lib.set_knob("PFSCDC_INDEX_MERGE", 1)
        runs = {"a": [], "b": []}
        traffic = {}

        def list_bytes(n, ndr, blob):
            return 64 * n + 128 * ndr + blob

        for i in range(args.warmup + args.reps):
            # (a) the host hand-over
            out_a.fill_(0xA5)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lists = [PF.index_read(c, store, r) for r in roots]
            t1 = time.perf_counter()
            merged = PF.index_merge([tuple(lists)], chunker=c)
            t2 = time.perf_counter()
            n, ents, blob, drs, ndr = merged._views()
            tf = lib.pfscdc_index_list_tar_files(merged._p)
            nw = C.c_uint64()
            rc = lib.pfscdc_store_read_tar(c.ctx, store._s, tf, n, drs, ndr, 0, window,
                                           out_a.data_ptr(), window, 1, C.byref(nw))
            t3 = time.perf_counter()
            if rc:
                raise SystemExit(f"read_bench: pfscdc_store_read_tar: {rc}")
            got_a = nw.value
            runs["a"].append({"read_ms": (t1 - t0) * 1e3, "merge_ms": (t2 - t1) * 1e3,
                              "tar_ms": (t3 - t2) * 1e3, "wall_ms": (t3 - t0) * 1e3})
            if i == 0:
                sizes = [(len(x), x._views()[4], len(x._views()[2])) for x in lists]
                ins = sum(list_bytes(*s) for s in sizes)
                traffic["a_read_d2h"] = ins
                traffic["a_merge_h2d"] = ins
                traffic["a_merge_d2h"] = list_bytes(n, ndr, len(blob))
            for x in lists:
                x.free()
            # (b) the resident calls
            out_b.fill_(0xA5)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dl = [PF.index_read_dev(c, store, r) for r in roots]
            up_bytes = PF.last_resident_stats(c)["read_uploaded_bytes"]
            t1 = time.perf_counter()
            dm = PF.index_merge_dev([tuple(dl)], c)
            t2 = time.perf_counter()
            rc = lib.pfscdc_dev_list_read_tar(c.ctx, store._s, dm._p, 0, window, out_b.data_ptr(),
                                              window, 1, C.byref(nw))
            t3 = time.perf_counter()
            if rc:
                raise SystemExit(f"read_bench: pfscdc_dev_list_read_tar: {rc}")
            rs = PF.last_resident_stats(c)
            if nw.value != got_a or not torch.equal(out_a, out_b):
                raise SystemExit("read_bench: the resident window differs from the host hand-over's")
            runs["b"].append({"read_ms": (t1 - t0) * 1e3, "merge_ms": (t2 - t1) * 1e3,
                              "tar_ms": (t3 - t2) * 1e3, "wall_ms": (t3 - t0) * 1e3})
            if i == 0:
                # computed, not measured: what (a)'s pfscdc_store_read_tar uploads for the same
                # window besides ciphertext:
                # 24 B per piece, two 8 B prefixes per piece (+1), 24 B and the name per entry,
                # and per chunk its offset, Ref, ok flag and hash record
                e = np.frombuffer(C.string_at(ents, 64 * n), dtype=np.uint8).reshape(n, 64)
                plen = e[:, 24:28].copy().view(np.uint32).ravel()
                offs, total = (C.c_uint64 * (n + 1))(), C.c_uint64()
                lib.pfscdc_dev_list_tar_layout(c.ctx, dm._p, C.byref(total), offs)
                nent = int(np.searchsorted(np.frombuffer(offs, dtype=np.uint64), window))
                per_chunk = 8 + 64 + 1 + 56
                traffic["a_tar_h2d"] = 24 * rs["pieces"] + 16 * (rs["pieces"] + 1) + 24 * nent + \
                    int(plen[:nent].sum()) + per_chunk * rs["chunks"] + 16
                traffic["a_tar_d2h"] = rs["chunks"]
                traffic["b_read_h2d"] = up_bytes
                traffic["b_tar_d2h"] = rs["d2h_bytes"]
                traffic["b_tar_h2d"] = rs["h2d_bytes"]
                traffic["window_entries"] = nent
                traffic["window_pieces"] = rs["pieces"]
                traffic["window_runs"] = rs["runs"]
                traffic["window_chunks"] = rs["chunks"]
                traffic["window_bytes"] = got_a
            merged.free()
            for x in dl + [dm]:
                x.free()
        _lib.set_knob("PFSCDC_INDEX_MERGE", 0)
        c.close()
        row = {"files": nfiles, "file_bytes": fbytes, "reps": args.reps, "warmup": args.warmup,
               "windows_equal": True, "traffic_bytes_excluding_ciphertext": traffic}
        for arm, name in (("a", "host_handover"), ("b", "resident")):
            r = runs[arm][args.warmup:]
            row[name] = {k: {"median": round(statistics.median(x[k] for x in r), 3),
                             "min": round(min(x[k] for x in r), 3),
                             "max": round(max(x[k] for x in r), 3)}
                         for k in ("read_ms", "merge_ms", "tar_ms", "wall_ms")}
        a, b = row["host_handover"]["wall_ms"], row["resident"]["wall_ms"]
        row["margin_ms"] = round(a["median"] - b["median"], 3)
        row["spread_ms"] = {"host_handover": round(a["max"] - a["min"], 3),
                            "resident": round(b["max"] - b["min"], 3)}
        row["resident_wins_by_more_than_both_spreads"] = bool(
            row["margin_ms"] > max(row["spread_ms"].values()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def synthetic_lists(ids, seed):
    """The deletive and additive index lists of one fileset whose files are /bench/dDDD/fNNNNNNN
    for N in ids (ascending), each Put without append (so every file has a deletive entry too)
    and one DataRef of 256 bytes: fixed-layout frames assembled with numpy, decoded by
    pfscdc_index_decode_host.  Returns (deletive, additive, one additive frame)."""
    from pfs_amd import fileset as PF
    ids = np.asarray(ids, dtype=np.int64)
    n = len(ids)
    rng = np.random.default_rng(seed)

    def path_cols(m, at):
        m[:, at:at + 8] = np.frombuffer(b"/bench/d", dtype=np.uint8)
        d = ids >> 12
        for k in range(3):
            m[:, at + 8 + k] = 48 + (d // 10 ** (2 - k)) % 10
        m[:, at + 11:at + 13] = np.frombuffer(b"/f", dtype=np.uint8)
        for k in range(7):
            m[:, at + 13 + k] = 48 + (ids // 10 ** (6 - k)) % 10

    a = np.zeros((n, 159), dtype=np.uint8)
    a[:, 0] = 151  # int64 LE frame length
    a[:, 8:10] = (0x0A, 20)  # path
    path_cols(a, 10)
    a[:, 30:34] = (0x1A, 127, 0x0A, 7)  # file { tag
    a[:, 34:41] = np.frombuffer(b"default", dtype=np.uint8)
    a[:, 41:47] = (0x12, 116, 0x0A, 73, 0x0A, 32)  # data_refs { ref { id
    a[:, 47:79] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    a[:, 79:84] = (0x10, 0x80, 0xA4, 0xE8, 0x03)  # Ref.size_bytes 8,000,000
    a[:, 84:86] = (0x22, 32)  # dek
    a[:, 86:118] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    a[:, 118:120] = (0x12, 32)  # hash
    a[:, 120:152] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    off = 16384 + 256 * (ids % 8000)  # offset_bytes: a three-byte varint
    a[:, 152] = 0x18
    a[:, 153] = (off & 0x7F) | 0x80
    a[:, 154] = ((off >> 7) & 0x7F) | 0x80
    a[:, 155] = off >> 14
    a[:, 156:159] = (0x20, 0x80, 0x02)  # size_bytes 256
    d = np.zeros((n, 41), dtype=np.uint8)
    d[:, 0] = 33
    d[:, 8:10] = (0x0A, 20)
    path_cols(d, 10)
    d[:, 30:41] = np.frombuffer(bytes([0x1A, 9, 0x0A, 7]) + b"default", dtype=np.uint8)
    return (PF.index_decode_host(d.tobytes()), PF.index_decode_host(a.tobytes()),
            a[0].tobytes())


def merge_rows(args):
    import time

    from oracle import fileset as OF
    from pfs_amd import fileset as PF
    rows = []
    shapes = []
    n2 = 524_288
    perm = np.random.default_rng(1).permutation(2 * n2)  # which fileset holds file i
    shapes.append(("two filesets of 524,288 files", [np.sort(perm[:n2]), np.sort(perm[n2:])]))
    n10, shared = 104_858, 10_486
    own = n10 - shared
    perm = np.random.default_rng(2).permutation(10 * own + shared)
    shapes.append(("ten filesets of 104,858 files, 10,486 of them in every fileset",
                   [np.sort(np.concatenate([perm[:shared],
                                            perm[shared + k * own:shared + (k + 1) * own]]))
                    for k in range(10)]))
    c = Chunker(ChunkParams(), 0)
    keys = ["upload_ms", "rank_group_ms", "emit_ms", "d2h_ms"]
    for name, id_sets in shapes:
        pairs = []
        for k, ids in enumerate(id_sets):
            assert len(np.unique(ids)) == len(ids)
            dele, add, frame = synthetic_lists(ids, 100 + k)
            assert len(dele) == len(add) == len(ids)
            pairs.append((dele, add))
        m = OF._msgs()["Index"].FromString(frame[8:])  # the hand-built frame is what protobuf reads
        assert m.path.startswith("/bench/d") and m.file.tag == "default" and \
            m.file.data_refs[0].size_bytes == 256 and m.file.data_refs[0].ref.size_bytes == 8_000_000
        row = {"shape": name, "filesets": len(pairs), "streams": 2 * len(pairs),
               "reps": args.reps, "warmup": args.warmup}
        for deletive in (False, True):
            runs = {1: [], 0: []}
            want = None
            for i in range(args.warmup + args.reps):
                for arm in (1, 0):
                    _lib.set_knob("PFSCDC_INDEX_MERGE", arm)
                    t0 = time.perf_counter()
                    lst = PF.index_merge(pairs, chunker=c, deletive=deletive)
                    wall = (time.perf_counter() - t0) * 1e3
                    stats = PF.last_merge_stats(c)
                    if stats["device"] != arm:
                        raise SystemExit("read_bench: the other arm ran")
                    arrs = list_arrays(lst)
                    if want is None:
                        want = arrs
                    elif arrs != want:
                        raise SystemExit("read_bench: the arms' lists differ")
                    lst.free()
                    if i >= args.warmup:
                        stats["wall_ms"] = wall
                        runs[arm].append(stats)
            mode = {}
            for arm, an in ((1, "device"), (0, "host")):
                r = runs[arm]
                mode[an] = {k: {"median": round(statistics.median(x[k] for x in r), 3),
                                "min": round(min(x[k] for x in r), 3),
                                "max": round(max(x[k] for x in r), 3)} for k in keys + ["wall_ms"]}
                mode[an].update({k: r[0][k] for k in ("entries_in", "groups", "entries_out")})
            mode["lists_equal"] = True
            row["deletive" if deletive else "files"] = mode
        _lib.set_knob("PFSCDC_INDEX_MERGE", _lib.knob_info()["PFSCDC_INDEX_MERGE"][2])
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pairs
    c.close()
    return rows


def compact_rows(args):
    """One compaction of a commit of two filesets, stage by stage."""
    import time

    from pfs_amd import chunk as pc
    from pfs_amd import fileset as PF
    nfiles, fbytes = args.files, 256
    store = pc.ChunkStore()
    st = PF.Storage(0, ChunkParams(), store=store)
    data = np.random.default_rng(nfiles).integers(0, 256, nfiles * fbytes + 64, dtype=np.uint8)
    infos = []
    t0 = time.perf_counter()
    for half in (0, 1):  # the second fileset: the odd files again, and every 16th file deleted
        w = st.new_unordered_writer()
        for i in range(half, nfiles, 1 + half):
            w.put("/bench/d%03d/f%07d" % (i >> 12, i), "", False, data[i * fbytes:(i + 1) * fbytes])
        if half:
            for i in range(0, nfiles, 16):
                w.delete("/bench/d%03d/f%07d" % (i >> 12, i), "")
        infos += w.close()
        w.release()
    write_s = time.perf_counter() - t0
    assert len(infos) == 2
    row = {"files": nfiles, "file_bytes": fbytes, "filesets": 2, "write_s": round(write_s, 2),
           "index_merge_knob": _lib.get_knob("PFSCDC_INDEX_MERGE"),
           "note": "copies_ms includes the Python event callback (one call per index entry "
                   "and chunk)"}
    c = Chunker(ChunkParams(), 0)
    t0 = time.perf_counter()
    pairs = [(PF.index_read(c, store, i.deletive), PF.index_read(c, store, i.additive)) for i in infos]
    t1 = time.perf_counter()
    deletes = PF.index_merge(pairs, chunker=c, deletive=True)
    files = PF.index_merge(pairs, chunker=c)
    merge_stats = PF.last_merge_stats(c)
    t2 = time.perf_counter()
    before = len(store)
    w = st.new_writer()
    w.copy_lists(files, deletes)
    t3 = time.perf_counter()
    prim = w.close()
    t4 = time.perf_counter()
    data_ev = [e for e in w.events if e[0] == "chunk" and e[1] == -1]
    cheap = sum(e[3] for e in data_ev if e[6])
    row.update({
        "index_reads_ms": round((t1 - t0) * 1e3, 1), "merge_ms": round((t2 - t1) * 1e3, 1),
        "merge_files_stats": merge_stats, "copies_ms": round((t3 - t2) * 1e3, 1),
        "close_ms": round((t4 - t3) * 1e3, 1),
        "files_out": prim.num_files, "deletes_out": prim.num_deletes, "size_bytes": prim.size_bytes,
        "cheap_copied_bytes": int(cheap), "rerolled_bytes": int(prim.size_bytes - cheap),
        "data_chunks_cheap": sum(1 for e in data_ev if e[6]),
        "data_chunks_formed": sum(1 for e in data_ev if not e[6]),
        "index_chunks_formed": sum(1 for e in w.events if e[0] == "chunk" and e[1] >= 0),
        "new_store_objects": len(store) - before})
    w.release()
    got = st.open([prim])
    want = st.open(infos)
    row["reads_back_as_its_inputs"] = got._list.raw() is not None and \
        [(f.path, f.size_bytes) for f in got.files()[:2000]] == \
        [(f.path, f.size_bytes) for f in want.files()[:2000]] and len(got._list) == len(want._list)
    c.close()
    print(json.dumps(row), flush=True)
    return [row]


def source_frames(n, fbytes, flat, seed):
    """The pbutil frames of n files of one DataRef of fbytes bytes each, in path order, one row
    per file: over a directory tree of fan-out 64 (/b/AA/BB/CC/fNNNNNNN, the directories the
    base-64 digits of N) or flat (/b/fNNNNNNN).  Fixed-layout frames assembled with numpy, as
    synthetic_lists does.  Also the column at which a row's 32 DataRef hash bytes begin."""
    ids = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(seed)
    L = 11 if flat else 20
    a = np.zeros((n, 8 + L + 131), dtype=np.uint8)
    a[:, 0] = L + 131  # int64 LE frame length
    a[:, 8:10] = (0x0A, L)  # path
    at = 10
    a[:, at:at + 3] = np.frombuffer(b"/b/", dtype=np.uint8)
    at += 3
    if not flat:
        for shift in (18, 12, 6):
            d = (ids >> shift) & 63
            a[:, at] = 48 + d // 10
            a[:, at + 1] = 48 + d % 10
            a[:, at + 2] = 0x2F
            at += 3
    a[:, at] = ord("f")
    for k in range(7):
        a[:, at + 1 + k] = 48 + (ids // 10 ** (6 - k)) % 10
    at += 8
    a[:, at:at + 4] = (0x1A, 127, 0x0A, 7)  # file { tag
    a[:, at + 4:at + 11] = np.frombuffer(b"default", dtype=np.uint8)
    a[:, at + 11:at + 17] = (0x12, 116, 0x0A, 73, 0x0A, 32)  # data_refs { ref { id
    a[:, at + 17:at + 49] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    a[:, at + 49:at + 54] = (0x10, 0x80, 0xA4, 0xE8, 0x03)  # Ref.size_bytes 8,000,000
    a[:, at + 54:at + 56] = (0x22, 32)  # dek
    a[:, at + 56:at + 88] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    a[:, at + 88:at + 90] = (0x12, 32)  # hash
    a[:, at + 90:at + 122] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    off = 16384 + 256 * (ids % 8000)  # offset_bytes: a three-byte varint
    a[:, at + 122] = 0x18
    a[:, at + 123] = (off & 0x7F) | 0x80
    a[:, at + 124] = ((off >> 7) & 0x7F) | 0x80
    a[:, at + 125] = off >> 14
    assert fbytes in (256, 4096)  # size_bytes: a two-byte varint
    a[:, at + 126:at + 129] = (0x20, 0x80, fbytes >> 7)
    return a, at + 90


def source_list(n, fbytes, flat, seed):
    """The level-0 list of source_frames' files."""
    from pfs_amd import fileset as PF
    return PF.index_decode_host(source_frames(n, fbytes, flat, seed)[0].tobytes())


def diff_rows(args):
    """--diff: DiffFile over two resident commits laid out over a tree of fan-out 64: the new
    commit is the old one with 1 % of the files' content changed, 8 files added and 8 removed.
    pfscdc_source_diff's device arm (PFSCDC_DIFF=1) and host arm (0: download of both sides,
    pfscdc_diff_host, upload of the pairs and the selections) alternating call by call, and the
    two pfscdc_source_open calls beside them; the arms' pairs and selections are compared array
    for array."""
    import time

    from pfs_amd import fileset as PF
    rows = []
    keys = ["rank_ms", "fill_ms", "select_ms", "guards_ms", "wall_ms", "after_ms"]
    shapes = [(65536, 4096), (args.files, 256)] if args.files != 65536 else [(65536, 4096)]
    for nfiles, fbytes in shapes:
        extra = 8
        frames, hcol = source_frames(nfiles + extra, fbytes, False, nfiles)
        rng = np.random.default_rng(nfiles + 1)
        old = PF.index_decode_host(frames[:nfiles].tobytes())
        new_frames = frames.copy()
        changed = rng.choice(nfiles, nfiles // 100, replace=False)
        new_frames[changed, hcol] ^= 0xFF  # another DataRef hash: another content
        keep = np.ones(nfiles + extra, dtype=bool)
        keep[rng.choice(nfiles, extra, replace=False)] = False
        new = PF.index_decode_host(new_frames[keep].tobytes())
        settle = PF.index_decode_host(frames[:16384].tobytes())
        c = Chunker(ChunkParams(), 0)
        dev_old, dev_new = PF.DevIndexList.upload(c, old), PF.DevIndexList.upload(c, new)
        opens = []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            a = PF.source_open(c, dev_old, _lib.SRC_DIFF, "")
            t1 = time.perf_counter()
            b = PF.source_open(c, dev_new, _lib.SRC_DIFF, "")
            t2 = time.perf_counter()
            if i >= args.warmup:
                opens.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
            if i + 1 < args.warmup + args.reps:
                a.free()
                b.free()
        runs = {1: [], 0: []}
        last = {}
        for i in range(args.warmup + args.reps):
            for arm in (1, 0):
                _lib.set_knob("PFSCDC_DIFF", arm)
                t0 = time.perf_counter()
                d = PF.source_diff(c, a, b)
                wall = (time.perf_counter() - t0) * 1e3
                stats = PF.last_diff_stats(c)
                if stats["device"] != arm:
                    raise SystemExit("read_bench: the wrong arm ran")
                if i == 0:
                    res = [d.pairs(c)]
                    for which in (0, 1):
                        got = d.side(which).list.download(c)
                        res.append((list_arrays(got), d.side(which).infos(c)))
                        got.free()
                    last[arm] = res
                    if arm == 0 and last[0] != last[1]:
                        raise SystemExit("read_bench: the device arm's diff differs from the host arm's")
                # what a call leaves for the next one to pay: the diff's release and one call that
                # allocates and copies (an upload of 16,384 entries), charged to the arm that ran,
                # so that neither arm's figure holds the other's leftovers.  (The host arm's
                # download of both sides keeps the runtime busy for some 20 ms after it returns;
                # a call that allocates device memory right after it waits that long.)
                t0 = time.perf_counter()
                d.free()
                PF.DevIndexList.upload(c, settle).free()
                stats["after_ms"] = (time.perf_counter() - t0) * 1e3
                if i >= args.warmup:
                    stats["wall_ms"] = wall
                    runs[arm].append(stats)
        row = {"files": nfiles, "file_bytes": fbytes, "layout": "fanout64", "changed": len(changed),
               "added": extra, "removed": extra, "reps": args.reps, "warmup": args.warmup,
               "device_equals_host": True,
               "stages": {"device": "rank and prefix sums, pairs, selections, guards",
                          "host": "download, pfscdc_diff_host, selections on the host, upload"}}
        for k, name in enumerate(("source_open_old_ms", "source_open_new_ms")):
            x = [o[k] for o in opens]
            row[name] = {"median": round(statistics.median(x), 3), "min": round(min(x), 3),
                         "max": round(max(x), 3)}
        for arm, name in ((1, "device"), (0, "host")):
            r = runs[arm]
            row[name] = {k: {"median": round(statistics.median(x[k] for x in r), 3),
                             "min": round(min(x[k] for x in r), 3),
                             "max": round(max(x[k] for x in r), 3)} for k in keys}
            row[name].update({k: r[0][k] for k in ("entries_a", "entries_b", "pairs", "both",
                                                   "h2d_bytes", "d2h_bytes")})
        rows.append(row)
        print(json.dumps(row), flush=True)
        _lib.set_knob("PFSCDC_DIFF", _lib.knob_info()["PFSCDC_DIFF"][2])
        a.free()
        b.free()
        dev_old.free()
        dev_new.free()
        c.close()
    return rows


def source_rows(args):
    """--source: the Source (directory entries, predicate, FileInfo) over the index lists of
    --index's two commits, laid out over a tree of fan-out 64 and flat: SUBTREE("") and GET of
    one second-level directory (flat: of /b), the device arm (PFSCDC_SOURCE=1) and the host arm
    (0) alternating call by call over a resident input; every device result is compared with
    the host arm's, array for array and info for info."""
    import time

    from pfs_amd import fileset as PF
    rows = []
    keys = ["select_ms", "tree_ms", "leaf_ms", "levels_ms", "wall_ms"]
    shapes = [(65536, 4096), (args.files, 256)] if args.files != 65536 else [(65536, 4096)]
    for nfiles, fbytes in shapes:
        for flat in (False, True):
            lst = source_list(nfiles, fbytes, flat, nfiles)
            c = Chunker(ChunkParams(), 0)
            dev = PF.DevIndexList.upload(c, lst)
            for kind, arg in ((_lib.SRC_SUBTREE, ""), (_lib.SRC_GET, "/b" if flat else "/b/00/01")):
                runs = {1: [], 0: []}
                last = {}
                for i in range(args.warmup + args.reps):
                    for arm in (1, 0):
                        _lib.set_knob("PFSCDC_SOURCE", arm)
                        t0 = time.perf_counter()
                        src = PF.source_open(c, dev, kind, arg)
                        wall = (time.perf_counter() - t0) * 1e3
                        stats = PF.last_source_stats(c)
                        if stats["device"] != arm:
                            raise SystemExit("read_bench: the wrong arm ran")
                        got = src.list.download(c)
                        last[arm] = (list_arrays(got), src.infos(c))
                        got.free()
                        src.free()
                        if arm == 0 and last[0] != last[1]:
                            raise SystemExit("read_bench: the device arm's result differs from the host arm's")
                        if i >= args.warmup:
                            stats["wall_ms"] = wall
                            runs[arm].append(stats)
                row = {"files": nfiles, "file_bytes": fbytes, "layout": "flat" if flat else "fanout64",
                       "predicate": ["ALL", "SUBTREE", "LIST", "GET"][kind], "arg": arg,
                       "reps": args.reps, "warmup": args.warmup, "device_equals_host": True}
                for arm, name in ((1, "device"), (0, "host")):
                    r = runs[arm]
                    row[name] = {k: {"median": round(statistics.median(x[k] for x in r), 3),
                                     "min": round(min(x[k] for x in r), 3),
                                     "max": round(max(x[k] for x in r), 3)} for k in keys}
                    row[name].update({k: r[0][k] for k in ("entries_in", "entries_out", "dirs_inserted",
                                                           "levels", "hash_launches", "h2d_bytes",
                                                           "d2h_bytes")})
                rows.append(row)
                print(json.dumps(row), flush=True)
            _lib.set_knob("PFSCDC_SOURCE", _lib.knob_info()["PFSCDC_SOURCE"][2])
            dev.free()
            c.close()
    return rows


GLOB_PATTERNS = ("/**", "/*/*/f1*", "/**.2", "/b/*/0?/**", "/**1")


def glob_rows(args):
    """--glob: PFSCDC_SRC_GLOB over a resident list of 65,536 and of --files files laid out
    over a tree of fan-out 64 (/b/AA/BB/CC/fNNNNNNN), the device arm (PFSCDC_SOURCE=1: the glob
    kernel ahead of the count pass) and the host arm (0) alternating call by call.  "/**"
    selects everything below the root; "/*/*/f1*" and "/**.2" select nothing in this tree (the
    whole cost is the predicate; both arms answer not-found); "/b/*/0?/**" selects ten of the 64
    second-level directories of each top one whole and "/**1" a tenth of the files, as orphans,
    and of the directories.  SUBTREE("") on the device arm is timed beside them, for comparison
    with the commit before.  In the first round of every pattern the device result is compared
    with the host arm's, array for array and info for info."""
    import time

    from pfs_amd import fileset as PF
    rows = []
    keys = ["select_ms", "tree_ms", "leaf_ms", "levels_ms", "wall_ms"]
    for nfiles, fbytes in [(65536, 4096)] + ([(args.files, 256)] if args.files != 65536 else []):
        lst = source_list(nfiles, fbytes, False, nfiles)
        c = Chunker(ChunkParams(), 0)
        dev = PF.DevIndexList.upload(c, lst)
        for kind, arg in [(_lib.SRC_GLOB, g) for g in GLOB_PATTERNS] + [(_lib.SRC_SUBTREE, "")]:
            arms = (1, 0) if kind == _lib.SRC_GLOB else (1,)
            runs = {arm: [] for arm in arms}
            last = {}
            for i in range(args.warmup + args.reps):
                for arm in arms:
                    _lib.set_knob("PFSCDC_SOURCE", arm)
                    t0 = time.perf_counter()
                    try:
                        src = PF.source_open(c, dev, kind, arg)
                    except KeyError:
                        src = None
                    wall = (time.perf_counter() - t0) * 1e3
                    stats = PF.last_source_stats(c)
                    if src is not None and stats["device"] != arm:
                        raise SystemExit("read_bench: the wrong arm ran")
                    if src is None:
                        last[arm] = None
                    else:
                        if i == 0:
                            got = src.list.download(c)
                            last[arm] = (list_arrays(got), src.infos(c))
                            got.free()
                        src.free()
                    if i == 0 and arm == 0 and last[0] != last[1]:
                        raise SystemExit("read_bench: the device arm's result differs from the host arm's")
                    if i >= args.warmup:
                        stats["wall_ms"] = wall
                        runs[arm].append(stats)
            row = {"files": nfiles, "file_bytes": fbytes, "layout": "fanout64",
                   "predicate": "GLOB" if kind == _lib.SRC_GLOB else "SUBTREE", "arg": arg,
                   "reps": args.reps, "warmup": args.warmup, "found": last[1] is not None,
                   "device_equals_host": len(arms) == 2}
            for arm in arms:
                r = runs[arm]
                name = "device" if arm else "host"
                row[name] = {k: {"median": round(statistics.median(x[k] for x in r), 3),
                                 "min": round(min(x[k] for x in r), 3),
                                 "max": round(max(x[k] for x in r), 3)} for k in keys}
                row[name].update({k: r[0][k] for k in ("entries_in", "entries_out", "dirs_inserted",
                                                       "levels", "hash_launches")})
            rows.append(row)
            print(json.dumps(row), flush=True)
        _lib.set_knob("PFSCDC_SOURCE", _lib.knob_info()["PFSCDC_SOURCE"][2])
        dev.free()
        c.close()
    return rows


def copy_rows(args):
    """--copy: pfscdc_dev_list_copy_map over a resident list whose first half lies under /b and
    whose second half under /c, src = /b: the device arm (PFSCDC_COPY_MAP=1) and the host arm (0)
    alternating call by call; per arm the map alone and the map with the selection brought to the
    host, as pfscdc_uw_copy needs it.  The arms' arrays are compared."""
    import time

    from pfs_amd import fileset as PF
    rows = []
    keys = ["count_ms", "fill_ms", "copy_ms", "guards_ms", "map_ms", "flow_ms"]
    shapes = [(65536, 4096), (args.files, 256)] if args.files != 65536 else [(65536, 4096)]
    for nfiles, fbytes in shapes:
        for flat in (False, True):
            frames, _ = source_frames(nfiles, fbytes, flat, nfiles)
            frames[nfiles // 2:, 11] = ord("c")  # /b/... becomes /c/...: still in path order
            lst = PF.index_decode_host(frames.tobytes())
            del frames
            c = Chunker(ChunkParams(), 0)
            dev = PF.DevIndexList.upload(c, lst)
            runs = {1: [], 0: []}
            last = {}
            for i in range(args.warmup + args.reps):
                for arm in (1, 0):
                    _lib.set_knob("PFSCDC_COPY_MAP", arm)
                    t0 = time.perf_counter()
                    got = PF.copy_map(c, dev, "/b", "/copied/here")
                    t1 = time.perf_counter()
                    stats = PF.last_copy_map_stats(c)
                    if stats["device"] != arm:
                        raise SystemExit("read_bench: the wrong arm ran")
                    if arm:  # the selection to the host
                        host = got.download(c)
                        flow = (time.perf_counter() - t0) * 1e3
                    else:  # the whole list to the host, the selection made there
                        t2 = time.perf_counter()
                        whole = dev.download(c)
                        host = PF.copy_map_host(whole, "/b", "/copied/here")
                        flow = (time.perf_counter() - t2) * 1e3
                        whole.free()
                    if i == 0:
                        check = got.download(c)
                        last[arm] = (list_arrays(check), list_arrays(host))
                        check.free()
                        if last[arm][0] != last[arm][1] or (arm == 0 and last[0] != last[1]):
                            raise SystemExit("read_bench: the device arm's list differs from the host arm's")
                    host.free()
                    got.free()
                    if i >= args.warmup:
                        stats["map_ms"] = (t1 - t0) * 1e3
                        stats["flow_ms"] = flow
                        runs[arm].append(stats)
            row = {"files": nfiles, "file_bytes": fbytes, "layout": "flat" if flat else "fanout64",
                   "src": "/b", "dst": "/copied/here", "reps": args.reps, "warmup": args.warmup,
                   "device_equals_host": True,
                   "stages": {"device": "count and prefix sums, fill, DataRef copy, guards",
                              "host": "download, pfscdc_copy_map_host, upload, -"}}
            for arm, name in ((1, "device"), (0, "host")):
                r = runs[arm]
                row[name] = {k: {"median": round(statistics.median(x[k] for x in r), 3),
                                 "min": round(min(x[k] for x in r), 3),
                                 "max": round(max(x[k] for x in r), 3)} for k in keys}
                row[name].update({k: r[0][k] for k in ("entries_in", "entries_out", "datarefs_out",
                                                       "blob_bytes_out", "h2d_bytes", "d2h_bytes")})
            rows.append(row)
            print(json.dumps(row), flush=True)
            _lib.set_knob("PFSCDC_COPY_MAP", _lib.knob_info()["PFSCDC_COPY_MAP"][2])
            dev.free()
            lst.free()
            c.close()
    return rows


def copy_file_row():
    """One copy_file of a directory whose chunks pass by reference: 1,024 files of 256 KiB under
    /d at the default chunking, copied to /moved."""
    import time

    from pfs_amd import chunk as pc
    from pfs_amd import fileset as PF
    from pfs_amd.cdc import synthetic_bytes
    nfiles, fbytes = 1024, 256 << 10
    st = PF.Storage(0, store=pc.ChunkStore())
    body = synthetic_bytes([0, nfiles * fbytes], 77)
    a = st.new_unordered_writer()
    for k in range(nfiles):
        a.put("/d/f%05d" % k, "", False, body[k * fbytes:(k + 1) * fbytes])
    a.put("/other", "", False, b"other")
    infos = a.close()
    a.release()
    w = st.new_unordered_writer()
    t0 = time.perf_counter()
    w.copy_file(infos, "/d", "/moved")
    t1 = time.perf_counter()
    got = w.close()
    t2 = time.perf_counter()
    data = [(e, c) for e, c in zip(w.log, w.log_copied) if e[1] == "chunk" and e[2] == -1]
    w.release()
    row = {"copy_file": "/d to /moved", "files": nfiles, "file_bytes": fbytes,
           "copy_map_knob": _lib.get_knob("PFSCDC_COPY_MAP"),
           "copy_file_ms": round((t1 - t0) * 1e3, 1), "close_ms": round((t2 - t1) * 1e3, 1),
           "files_out": got[0].num_files, "size_bytes": got[0].size_bytes,
           "data_chunks_by_reference": sum(1 for _, c in data if c),
           "bytes_by_reference": int(sum(e[4] for e, c in data if c)),
           "data_chunks_formed": sum(1 for _, c in data if not c)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", action="store_true")
    ap.add_argument("--merge", action="store_true")
    ap.add_argument("--compact", action="store_true")
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--source", action="store_true")
    ap.add_argument("--diff", action="store_true")
    ap.add_argument("--copy", action="store_true")
    ap.add_argument("--glob", action="store_true")
    ap.add_argument("--files", type=int, default=1 << 20)
    ap.add_argument("--tar", action="store_true")
    ap.add_argument("--chunks", type=int, default=1024)
    ap.add_argument("--chunk-bytes", type=int, default=4 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "r8", "read_tar", "read_tar.json") if args.tar \
            else os.path.join(ROOT, "profiles", "r7", "read_path", "read_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("read_bench: needs a GPU")
    if args.merge or args.compact:
        what = "merge" if args.merge else "compact"
        if args.out == os.path.join(ROOT, "profiles", "r7", "read_path", "read_bench.json"):
            args.out = os.path.join(ROOT, "profiles", "r10", "compact", what + ".json")
        rows = merge_rows(args) if args.merge else compact_rows(args)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/read_bench.py --" + what,
                       "device": torch.cuda.get_device_name(0), "shapes": rows}, f, indent=1)
            f.write("\n")
        return
    if args.source:
        if args.out == os.path.join(ROOT, "profiles", "r7", "read_path", "read_bench.json"):
            args.out = os.path.join(ROOT, "profiles", "r12", "source", "source.json")
        rows = source_rows(args)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/read_bench.py --source",
                       "device": torch.cuda.get_device_name(0), "shapes": rows}, f, indent=1)
            f.write("\n")
        return
    if args.glob:
        if args.out == os.path.join(ROOT, "profiles", "r7", "read_path", "read_bench.json"):
            args.out = os.path.join(ROOT, "profiles", "r25", "glob", "glob.json")
        rows = glob_rows(args)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/read_bench.py --glob",
                       "device": torch.cuda.get_device_name(0), "shapes": rows}, f, indent=1)
            f.write("\n")
        return
    if args.copy:
        if args.out == os.path.join(ROOT, "profiles", "r7", "read_path", "read_bench.json"):
            args.out = os.path.join(ROOT, "profiles", "r7", "read_path", "copy.json")
        rows = copy_rows(args)
        record = copy_file_row()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/read_bench.py --copy",
                       "device": torch.cuda.get_device_name(0),
                       "copy": {"shapes": rows, "copy_file": record}}, f, indent=1)
            f.write("\n")
        return
    if args.diff:
        if args.out == os.path.join(ROOT, "profiles", "r7", "read_path", "read_bench.json"):
            args.out = os.path.join(ROOT, "profiles", "r7", "read_path", "diff.json")
        rows = diff_rows(args)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/read_bench.py --diff",
                       "device": torch.cuda.get_device_name(0), "shapes": rows}, f, indent=1)
            f.write("\n")
        return
    if args.resident:
        if args.out == os.path.join(ROOT, "profiles", "r7", "read_path", "read_bench.json"):
            args.out = os.path.join(ROOT, "profiles", "r11", "resident", "resident.json")
        rows = resident_rows(args)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/read_bench.py --resident",
                       "device": torch.cuda.get_device_name(0), "shapes": rows}, f, indent=1)
            f.write("\n")
        return
    if args.index:
        if args.out == os.path.join(ROOT, "profiles", "r7", "read_path", "read_bench.json"):
            args.out = os.path.join(ROOT, "profiles", "r9", "index_read", "index_read.json")
        rows = index_rows(args)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/read_bench.py --index", "device": torch.cuda.get_device_name(0),
                       "shapes": rows}, f, indent=1)
            f.write("\n")
        return
    n, cb = args.chunks, args.chunk_bytes
    c = Chunker(ChunkParams(), 0)
    cofs = np.arange(n + 1, dtype=np.uint64) * np.uint64(cb)
    data = torch.empty(n * cb, dtype=torch.uint8, device="cuda:0")
    c.fill_synthetic(data, cofs, 0x7EAD)
    refs, _ = c.create_refs(data, cofs)  # Ref.Dek and Ref.Id of every chunk
    ctext = torch.empty_like(data)
    c.get_chunks(data, cofs, refs, out=ctext)  # XOR is its own inverse: the stored form
    rows = tar_rows(args, c, data, ctext, cofs, refs, n, cb) if args.tar else []
    plain = None if args.tar else torch.empty_like(data)
    for name, (sl, ver, runs) in ({} if args.tar else
                                  layouts(n, cb, np.random.default_rng(7))).items():
        total = int(sl["size"].sum())
        out = torch.empty(total, dtype=torch.uint8, device="cuda:0")
        vms, gms, getms = [], [], []
        for i in range(args.warmup + args.reps):
            out.zero_()
            _, cok, sok = c.read_slices(ctext, cofs, refs, sl, out=out, verified=ver)
            t = c.last_read_timings()
            if not (cok.all() and sok.all()):
                raise SystemExit(f"read_bench: {name}: a chunk failed verification")
            check(out, data, cb, runs)
            if name == "whole":  # the same bytes through chunk.Get, alternating
                _, ok = c.get_chunks(ctext, cofs, refs, out=plain)
                if not (ok.all() and torch.equal(plain, data)):
                    raise SystemExit("read_bench: get_chunks output differs from the plaintext")
                g = c.last_get_ms()
            if i >= args.warmup:
                vms.append(t["verify"])
                gms.append(t["gather"])
                if name == "whole":
                    getms.append(g)
        gm = statistics.median(gms)
        gbs = 2 * total / (gm * 1e-3) / 1e9
        row = {"layout": name, "chunks": n, "chunk_bytes": cb, "slices": int(len(sl)),
               "slice_bytes": total, "verify_ms_median": round(statistics.median(vms), 4),
               "gather_ms_median": round(gm, 4),
               "gather_read_plus_written_gbs": round(gbs, 1),
               "gather_share_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
               "hbm_peak_gbs": HBM_PEAK_GBS, "reps": args.reps, "warmup": args.warmup,
               "outputs_equal_plaintext": True}
        if name == "whole":
            row["get_chunks_ms_median_same_run"] = round(statistics.median(getms), 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
    c.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/read_bench.py" + (" --tar" if args.tar else ""), "device": torch.cuda.get_device_name(0),
                   "layouts": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
