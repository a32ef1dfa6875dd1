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
code does not change with the tar path).  Per layout: stream bytes, median device ms of the
verification, the gather and tar_frame_kernel, and read_slices' two figures with their spread.
The first tar stream of each layout is checked: every file's content against the plaintext,
sampled headers against pfscdc_tar_header, padding and trailer zero.  Writes
profiles/r8/read_tar/read_tar.json.

--index: reading a fileset back (pfscdc_index_read).  Two commits are written through the
unordered writer into a store at the reference's index parameters, 65,536 files of 4 KiB and
1,048,576 files of 256 B, and the additive root of each is read back with the device decode
(PFSCDC_INDEX_DECODE=1) and the host decode (0), the arms alternating call by call.  Per arm:
median, min and max of the call's wall time and of its stages (read-path verification and
gather of the index chunks, frame walk with the re-walk count, decode, copy to the host).
Every list is compared, array for array, with pfscdc_index_decode_host over the writer's own
level-0 index events, and its first and last 500 entries with the events decoded by the protobuf
runtime.  Writes profiles/r9/index_read/index_read.json.

usage: python tools/read_bench.py [--tar | --index] [--chunks N] [--chunk-bytes B] [--reps R]
                                  [--warmup W] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

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


def check_tar(out, data, cb, sl, names, offs, total):
    """The tar stream in out: every file's content is the plaintext of its slice, sampled
    headers are pfscdc_tar_header's, the sampled files' padding and the trailer are zero."""
    from pfs_amd.fileset import tar_header
    chunk, off, size = (sl[k].astype(np.int64) for k in ("chunk", "offset", "size"))
    for i in range(len(sl)):
        a, b = int(chunk[i]) * cb + int(off[i]), int(offs[i]) + 512
        if not torch.equal(out[b:b + int(size[i])], data[a:a + int(size[i])]):
            raise SystemExit(f"read_bench: tar content differs from the plaintext in file {i}")
    for i in sorted({0, 1, len(sl) // 2, len(sl) - 1} | set(range(0, len(sl), max(1, len(sl) // 61)))):
        at, z = int(offs[i]), int(size[i])
        if out[at:at + 512].cpu().numpy().tobytes() != tar_header(names[i], z):
            raise SystemExit(f"read_bench: tar header {i} differs from pfscdc_tar_header")
        if int(out[at + 512 + z:int(offs[i + 1])].max().item() if -z % 512 else 0) != 0:
            raise SystemExit(f"read_bench: tar padding of file {i} is not zero")
    if int(out[total - 1024:total].max().item()) != 0:
        raise SystemExit("read_bench: tar trailer is not zero")


def tar_rows(args, c, data, ctext, cofs, refs, n, cb):
    rows = []
    med = statistics.median
    for name, (sl, ver, runs) in layouts(n, cb, np.random.default_rng(7)).items():
        payload = int(sl["size"].sum())
        names = ["/bench/%s/%07d" % (name, i) for i in range(len(sl))]
        files = [(p, i, 1) for i, p in enumerate(names)]
        padded = (sl["size"].astype(np.int64) + 511) // 512 * 512 + 512
        offs = np.concatenate([[0], np.cumsum(padded)])
        total = int(offs[-1]) + 1024
        out = torch.empty(payload, dtype=torch.uint8, device="cuda:0")
        tout = torch.empty(total, dtype=torch.uint8, device="cuda:0")
        t_v, t_g, t_f, s_v, s_g = [], [], [], [], []
        for i in range(args.warmup + args.reps):
            out.fill_(0xA5)
            _, cok, _ = c.read_slices(ctext, cofs, refs, sl, out=out, verified=ver)
            s = c.last_read_timings()
            if not cok.all():
                raise SystemExit(f"read_bench: {name}: a chunk failed verification")
            check(out, data, cb, runs)
            tout.fill_(0xA5)
            _, cok, nw = c.read_tar(ctext, cofs, refs, files, sl, out=tout, verified=ver)
            t = c.last_read_timings()
            fms = c.last_frame_ms()
            if not cok.all() or nw != total:
                raise SystemExit(f"read_bench: {name}: tar read failed")
            if i == 0:
                check_tar(tout, data, cb, sl, names, offs, total)
            if i >= args.warmup:
                s_v.append(s["verify"])
                s_g.append(s["gather"])
                t_v.append(t["verify"])
                t_g.append(t["gather"])
                t_f.append(fms)
        row = {"layout": name, "chunks": n, "chunk_bytes": cb, "files": int(len(sl)),
               "payload_bytes": payload, "stream_bytes": total,
               "header_padding_trailer_bytes": total - payload,
               "tar_verify_ms_median": round(med(t_v), 4),
               "tar_gather_ms_median": round(med(t_g), 4),
               "tar_gather_ms_min_max": [round(min(t_g), 4), round(max(t_g), 4)],
               "tar_frame_ms_median": round(med(t_f), 4),
               "tar_frame_ms_min_max": [round(min(t_f), 4), round(max(t_f), 4)],
               "read_slices_verify_ms_median": round(med(s_v), 4),
               "read_slices_gather_ms_median": round(med(s_g), 4),
               "read_slices_gather_ms_min_max": [round(min(s_g), 4), round(max(s_g), 4)],
               "reps": args.reps, "warmup": args.warmup, "first_stream_checked": True}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del out, tout
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", action="store_true")
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
