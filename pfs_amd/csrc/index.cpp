// index.cpp — reading a fileset back: index.Reader.Iterate over a chunk store and
// MergeReader.iterate (host logic; the frame walk and entry decode kernels are in
// list_kernels.hip, the proto parser both sides share in index_parse.h).  Both also with a
// device-resident result (pfscdc_index_read_dev, pfscdc_index_merge_dev: the decode's and the
// merge's output arrays become a pfscdc_dev_list, dev_list.h, instead of being copied out).
//
// Reference (paths under /root/reference/src/internal):
//   storage/fileset/index/reader.go:41-83    Iterate: levels, atEnd / atStart / tag
//   storage/fileset/index/reader.go:95-122   atStart, atEnd (range and prefix filters)
//   storage/fileset/index/reader.go:124-181  levelReader: chunk[Offset:], then whole chunks
//   storage/fileset/merge.go:37-77,157-164   MergeReader.iterate, compare (path, then tag)
//   stream/priority_queue.go:103-127         groups of equal streams, sorted by priority
//   pbutil/pbutil.go:39,65                   int64 LE length + proto
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "dev_pass.h"

namespace {

using namespace pfscdc;
using List = pfscdc_index_list;

// Reader.Iterate's walk over one level's entries: the level-0 entries the filter selects go to
// sel, the Range entries whose chunks hold the level below to parents.  *tail: the Range entry
// the walk ended at (the first with atEnd(Path)), or -1.  Its chunk is read too, as
// levelReader.next fetches it whatever its path when a frame runs on into it: the last wanted
// frame may end there, and a wanted entry may even begin there (an entry that begins on the
// chunk's border with the path of the entry before it, another tag, is not the one the chunk's
// Range names).  Nothing wanted begins after it.  false: an entry that cannot be followed (why
// set).
bool select(const List& l, const IdxFilter& f, std::vector<uint32_t>* sel,
            std::vector<uint32_t>* parents, int64_t* tail, const char** why) {
  bool leaf = false, range = false;
  *tail = -1;
  for (uint32_t i = 0; i < l.entries.size(); i++) {
    const pfscdc_index_entry& e = l.entries[i];
    if (f.at_end(idx_path(l, e))) {
      if ((e.flags & PFSCDC_IDX_HAS_RANGE) && (e.flags & PFSCDC_IDX_HAS_CHUNK_REF)) *tail = i;
      break;
    }
    if (!(e.flags & PFSCDC_IDX_HAS_RANGE)) {
      leaf = true;
      if (f.at_start(idx_path(l, e)) && f.tag_ok(idx_tag(l, e))) sel->push_back(i);
    } else {
      range = true;
      if (!(e.flags & PFSCDC_IDX_HAS_CHUNK_REF)) {
        *why = "a Range without a chunk_ref";
        return false;
      }
      if (f.at_start(idx_last_path(l, e))) parents->push_back(i);
    }
  }
  if (leaf && range) {
    *why = "Range entries and level-0 entries in one level";
    return false;
  }
  return true;
}

int corrupt(pfscdc_ctx* ctx, uint32_t level, uint64_t offset) {
  return pfscdc::ctx_fail(ctx, PFSCDC_ECORRUPT,
                          "index level " + std::to_string(level) + ": the frame at stream offset " +
                              std::to_string(offset) + " does not parse");
}

// One level's stream, already on the device (d_buf[0, n), allocated 64 bytes longer; chunk i < nc
// is [cb[i], cb[i + 1]) and claims the frame start cb[i] + off[i]), walked and decoded into out.
// open_end: the selection ends before the level does (its last chunk is the tail chunk).
int decode_level_device(pfscdc_ctx* ctx, uint32_t level, const uint8_t* d_buf, uint64_t n,
                        const std::vector<uint64_t>& cb, const std::vector<int64_t>& off,
                        uint32_t nc, bool open_end, List* out, pfscdc_dev_list* keep = nullptr,
                        bool* kept = nullptr) {
  IndexStats& st = ctx_index_stats(ctx);
  hipStream_t s = ctx_stream(ctx);
  const int cus = ctx_num_cus(ctx);
  const uint64_t start0 = cb[0] + (uint64_t)off[0];
  Clock clk;
  // ---- the frame walk: one speculative walker per chunk, settled along the chain
  std::vector<IdxWalk> walks(nc);
  for (uint32_t i = 0; i < nc; i++) {
    const uint64_t len = cb[i + 1] - cb[i];
    const bool claim = off[i] >= 0 && (uint64_t)off[i] <= len;
    walks[i] = IdxWalk{claim ? cb[i] + (uint64_t)off[i] : kIdxNone, cb[i + 1], cb[i] / 8 + i,
                       len / 8 + 1};
  }
  DevMem d_walks, d_outs, d_starts;
  PFS_HIP(ctx, d_walks.alloc(sizeof(IdxWalk) * nc));
  PFS_HIP(ctx, d_outs.alloc(sizeof(IdxWalkOut) * nc));
  PFS_HIP(ctx, d_starts.alloc(sizeof(uint64_t) * (n / 8 + nc + 1)));
  PFS_HIP(ctx, hipMemcpyAsync(d_walks.p, walks.data(), sizeof(IdxWalk) * nc, hipMemcpyHostToDevice, s));
  PFS_HIP(ctx, launch_index_walk(d_buf, n, d_walks.as<IdxWalk>(), nc, d_starts.as<uint64_t>(),
                                 d_outs.as<IdxWalkOut>(), cus, s));
  std::vector<IdxWalkOut> outs(nc);
  PFS_HIP(ctx, hipMemcpyAsync(outs.data(), d_outs.p, sizeof(IdxWalkOut) * nc, hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  // The truth is the chain from chunk 0's claim: chunk i's walk stands only if the chunk
  // before is settled and its exit is chunk i's claim.  A chunk wholly inside one entry (its
  // one annotation gets Offset 0, index/writer.go:102-121) holds no frame start at all; any
  // other chunk with a wrong claim is walked again from the exit.  Each repeat settles a chunk.
  // A length the walk cannot follow ends it (walk_err, in chunk settled - 1); the frames it did
  // settle still go through the count pass, since the first frame that fails is the one to name
  // and a frame in front of the bad length may fail to parse.
  uint64_t nf = 0, walk_err = kIdxNone;
  uint32_t settled = nc;
  for (uint32_t i = 0; i < nc; i++) {
    if (i > 0 && walks[i].start != outs[i - 1].exit) {
      st.n[1]++;
      const uint64_t from = outs[i - 1].exit;
      if (from >= cb[i + 1]) {
        outs[i] = IdxWalkOut{from, 0, kIdxNone, 0};
      } else {
        walks[i].start = from;
        PFS_HIP(ctx, hipMemcpyAsync(d_walks.as<IdxWalk>() + i, &walks[i], sizeof(IdxWalk),
                                    hipMemcpyHostToDevice, s));
        PFS_HIP(ctx, launch_index_walk(d_buf, n, d_walks.as<IdxWalk>() + i, 1,
                                       d_starts.as<uint64_t>(), d_outs.as<IdxWalkOut>() + i, cus, s));
        PFS_HIP(ctx, hipMemcpyAsync(&outs[i], d_outs.as<IdxWalkOut>() + i, sizeof(IdxWalkOut),
                                    hipMemcpyDeviceToHost, s));
        PFS_HIP(ctx, hipStreamSynchronize(s));
      }
    }
    nf += outs[i].count;
    if (outs[i].err != kIdxNone) {
      // A frame that runs past a selection that ends before the level does is past the filter's
      // end (a wanted frame ends inside the tail chunk): the stream ends in front of it.
      if (!(open_end && outs[i].past)) {
        walk_err = outs[i].err;
        settled = i + 1;
      } else {
        for (uint32_t k = i + 1; k < nc; k++) outs[k] = IdxWalkOut{n, 0, kIdxNone, 0};
      }
      break;
    }
  }
  st.ms[2] += clk.lap();
  st.n[3] += nf;
  if (nf == 0) return walk_err != kIdxNone ? corrupt(ctx, level, walk_err - start0) : PFSCDC_OK;
  if (nf > 0xffffffffull) return ctx_fail(ctx, PFSCDC_EUNSUPPORTED, "more than 2^32 index entries");
  // ---- the decode: frame starts packed, count pass, prefix sums, fill pass
  clk.lap();
  DevMem d_fstart, d_cnt, d_base, d_err;
  PFS_HIP(ctx, d_fstart.alloc(sizeof(uint64_t) * nf));
  PFS_HIP(ctx, d_cnt.alloc(sizeof(IdxCount) * nf));
  PFS_HIP(ctx, d_base.alloc(sizeof(uint64_t) * 2 * (nf + 1)));
  PFS_HIP(ctx, d_err.alloc(sizeof(uint64_t)));
  uint64_t at = 0;
  for (uint32_t i = 0; i < settled; at += outs[i].count, i++)
    if (outs[i].count)
      PFS_HIP(ctx, hipMemcpyAsync(d_fstart.as<uint64_t>() + at, d_starts.as<uint64_t>() + walks[i].slot,
                                  sizeof(uint64_t) * outs[i].count, hipMemcpyDeviceToDevice, s));
  uint64_t h_err = kIdxNone, totals[2] = {0, 0};
  PFS_HIP(ctx, hipMemcpyAsync(d_err.p, &h_err, sizeof h_err, hipMemcpyHostToDevice, s));
  PFS_HIP(ctx, launch_index_count(d_buf, n, d_fstart.as<uint64_t>(), nf, d_cnt.as<IdxCount>(),
                                  d_err.as<unsigned long long>(), cus, s));
  PFS_HIP(ctx, launch_index_scan(d_cnt.as<IdxCount>(), nf, d_base.as<uint64_t>(), s));
  PFS_HIP(ctx, hipMemcpyAsync(&h_err, d_err.p, sizeof h_err, hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipMemcpyAsync(totals, d_base.as<uint64_t>() + 2 * nf, sizeof totals,
                              hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  h_err = std::min(h_err, walk_err);  // (every settled frame starts in front of walk_err)
  if (h_err != kIdxNone) return corrupt(ctx, level, h_err - start0);
  if (totals[0] > 0xffffffffull) return ctx_fail(ctx, PFSCDC_EUNSUPPORTED, "more than 2^32 DataRefs");
  DevMem d_entries, d_drs, d_blob;
  PFS_HIP(ctx, d_entries.alloc(sizeof(pfscdc_index_entry) * nf));
  PFS_HIP(ctx, d_drs.alloc(sizeof(pfscdc_full_dataref) * totals[0]));
  PFS_HIP(ctx, d_blob.alloc(totals[1]));
  PFS_HIP(ctx, launch_index_fill(d_buf, n, d_fstart.as<uint64_t>(), nf, d_base.as<uint64_t>(),
                                 d_entries.as<pfscdc_index_entry>(),
                                 d_drs.as<pfscdc_full_dataref>(), d_blob.as<char>(), cus, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.ms[3] += clk.lap();
  if (keep) {  // a level of File entries only is level 0: its arrays are the resident list
    DevMem d_flags;
    uint32_t flags[2] = {0, ~0u};  // OR and AND of the entries' flags
    PFS_HIP(ctx, d_flags.alloc(sizeof flags));
    PFS_HIP(ctx, hipMemcpyAsync(d_flags.p, flags, sizeof flags, hipMemcpyHostToDevice, s));
    PFS_HIP(ctx, launch_index_flags(d_entries.as<pfscdc_index_entry>(), nf, d_flags.as<uint32_t>(),
                                    cus, s));
    PFS_HIP(ctx, hipMemcpyAsync(flags, d_flags.p, sizeof flags, hipMemcpyDeviceToHost, s));
    PFS_HIP(ctx, hipStreamSynchronize(s));
    if (!(flags[0] & PFSCDC_IDX_HAS_RANGE)) {
      std::swap(keep->entries, d_entries.p);
      std::swap(keep->drs, d_drs.p);
      std::swap(keep->blob, d_blob.p);
      keep->n = nf;
      keep->nr = totals[0];
      keep->nb = totals[1];
      *kept = true;
    }
    st.ms[3] += clk.lap();  // the flags pass counts as decode time, kept or not
    if (*kept) return PFSCDC_OK;
  }
  // ---- the list to the host
  clk.lap();
  out->entries.resize(nf);
  out->drs.resize(totals[0]);
  out->blob.resize(totals[1]);
  PFS_HIP(ctx, hipMemcpyAsync(out->entries.data(), d_entries.p, sizeof(pfscdc_index_entry) * nf,
                              hipMemcpyDeviceToHost, s));
  if (totals[0])
    PFS_HIP(ctx, hipMemcpyAsync(out->drs.data(), d_drs.p, sizeof(pfscdc_full_dataref) * totals[0],
                                hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipMemcpyAsync(out->blob.data(), d_blob.p, totals[1], hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.ms[4] += clk.lap();
  return PFSCDC_OK;
}

// The level below the entries parents of cur: their chunks through the read path into one
// device buffer, then the decode (device, or host with the PFSCDC_INDEX_DECODE knob at 0).
int read_level(pfscdc_ctx* ctx, const pfscdc_store* store, uint32_t level, const List& cur,
               std::vector<uint32_t> parents, int64_t tail, List* out,
               pfscdc_dev_list* keep = nullptr, bool* kept = nullptr) {
  IndexStats& st = ctx_index_stats(ctx);
  if (tail >= 0) parents.push_back((uint32_t)tail);
  const uint32_t nc = (uint32_t)parents.size();
  std::vector<pfscdc_full_dataref> refs(nc);
  std::vector<uint64_t> cb(nc + 1, 0);
  std::vector<int64_t> off(nc);
  for (uint32_t i = 0; i < nc; i++) {
    const pfscdc_index_entry& e = cur.entries[parents[i]];
    if ((uint64_t)e.first + e.count >= cur.drs.size())  // (select() saw PFSCDC_IDX_HAS_CHUNK_REF)
      return ctx_fail(ctx, PFSCDC_ECORRUPT, "index level " + std::to_string(level) +
                                                ": a Range's chunk_ref lies outside the list");
    refs[i] = cur.drs[e.first + e.count];
    off[i] = e.range_offset;
    if (refs[i].data.size_bytes < 0 || cb[i] + (uint64_t)refs[i].data.size_bytes < cb[i])
      return ctx_fail(ctx, PFSCDC_ECORRUPT, "index level " + std::to_string(level) +
                                                ": a Range's chunk_ref has a bad size");
    cb[i + 1] = cb[i] + (uint64_t)refs[i].data.size_bytes;
  }
  const uint64_t n = cb[nc];
  // levelReader.setup: the first chunk from Range.Offset on (Go panics on an offset beyond it)
  if (off[0] < 0 || (uint64_t)off[0] > cb[1])
    return ctx_fail(ctx, PFSCDC_ECORRUPT, "index level " + std::to_string(level) +
                                              ": Range.Offset beyond its chunk");
  PFS_HIP(ctx, hipSetDevice(ctx_device(ctx)));
  DevMem d_buf;
  PFS_HIP(ctx, d_buf.alloc(n + 64));
  uint64_t nw = 0;
  int rc = pfscdc_store_read(ctx, store, refs.data(), nc, d_buf.p, n, 1, &nw);
  if (rc == PFSCDC_ENOTFOUND)
    return ctx_fail(ctx, rc,
                    "index level " + std::to_string(level) + ": a chunk id is not in the store");
  if (rc == PFSCDC_EINVAL)
    return ctx_fail(ctx, PFSCDC_ECORRUPT, "index level " + std::to_string(level) +
                                              ": a Range's chunk_ref reaches past its chunk");
  if (rc) return rc;
  float rt[2] = {0.f, 0.f};
  (void)pfscdc_last_read_timings(ctx, rt);
  st.ms[0] += rt[0];
  st.ms[1] += rt[1];
  st.n[0] += nc;
  st.n[2]++;
  if (knob(Knob::IndexDecode) != 0)
    return decode_level_device(ctx, level, d_buf.as<uint8_t>(), n, cb, off, nc, tail >= 0, out,
                               keep, kept);
  // the host arm: the level's bytes to the host, then the specification's decode
  const uint64_t start0 = (uint64_t)off[0];
  Clock clk;
  std::vector<uint8_t> h(n - start0);
  if (!h.empty())
    PFS_HIP(ctx, hipMemcpy(h.data(), d_buf.as<uint8_t>() + start0, h.size(), hipMemcpyDeviceToHost));
  st.ms[4] += clk.lap();
  uint64_t err = kIdxNone;
  rc = idx_decode_stream(h.data(), h.size(), h.size(), tail >= 0, out, &err);
  st.ms[3] += clk.lap();
  st.n[3] += out->entries.size();
  if (rc == PFSCDC_ECORRUPT) return corrupt(ctx, level, err);
  return rc ? ctx_fail(ctx, rc, "more than 2^32 index records") : PFSCDC_OK;
}

// MergeReader on the device (list_kernels.hip §9) over ns streams.  *ran = false: the call
// belongs to the host arm (a stream out of order, or more than 2^32 - 1 entries or records).
// The output arrays are an OutList's: a kernel that wrote past what the prefix sums counted fails
// the call.

// One input stream: its three arrays where they lie (host vectors, or a resident list's arrays).
struct MrgSrc {
  const void *entries = nullptr, *blob = nullptr, *drs = nullptr;
  uint64_t n = 0, nb = 0, nr = 0;
};

// kind: where the streams lie (host to device, or device to device for resident lists).  keep
// (nullable): the output arrays become this resident list and nothing but the guards is copied
// to the host; else the list is copied into out.
int merge_device(pfscdc_ctx* ctx, int mode, const MrgSrc* src, uint32_t ns, hipMemcpyKind kind,
                 List* out, pfscdc_dev_list* keep, bool* ran) {
  MergeStats& st = ctx_merge_stats(ctx);
  *ran = false;
  std::vector<uint64_t> tab(3 * (uint64_t)ns + 1, 0);  // stream_begin[ns + 1], blob_base, dr_base
  uint64_t *sb = tab.data(), *bb = sb + ns + 1, *db = bb + ns;
  uint64_t n = 0, nb = 0, nr = 0;
  for (uint32_t s = 0; s < ns; s++) {
    sb[s] = n;
    bb[s] = nb;
    db[s] = nr;
    n += src[s].n;
    nb += src[s].nb;
    nr += src[s].nr;
  }
  sb[ns] = n;
  st.n[1] = n;
  if (n > 0xffffffffull || nr > 0xffffffffull) return PFSCDC_OK;
  *ran = true;
  if (n == 0) return PFSCDC_OK;
  hipStream_t s = ctx_stream(ctx);
  const int cus = ctx_num_cus(ctx);
  PFS_HIP(ctx, hipSetDevice(ctx_device(ctx)));
  // ---- upload: the streams' three arrays, concatenated stream-major
  Clock clk;
  DevMem d_tab, d_entries, d_blob, d_drs, d_order, d_bad, d_cnt, d_base, d_heads;
  PFS_HIP(ctx, d_tab.alloc(sizeof(uint64_t) * tab.size()));
  PFS_HIP(ctx, d_entries.alloc(sizeof(pfscdc_index_entry) * n));
  PFS_HIP(ctx, d_blob.alloc(nb));
  PFS_HIP(ctx, d_drs.alloc(sizeof(pfscdc_full_dataref) * nr));
  PFS_HIP(ctx, d_order.alloc(sizeof(uint32_t) * n));
  PFS_HIP(ctx, d_bad.alloc(sizeof(uint32_t)));
  PFS_HIP(ctx, d_heads.alloc(sizeof(uint64_t)));
  PFS_HIP(ctx, d_cnt.alloc(sizeof(MrgCount) * n));
  PFS_HIP(ctx, d_base.alloc(sizeof(uint64_t) * 3 * (n + 1)));
  PFS_HIP(ctx, hipMemcpyAsync(d_tab.p, tab.data(), sizeof(uint64_t) * tab.size(), hipMemcpyHostToDevice, s));
  for (uint32_t k = 0; k < ns; k++) {
    const MrgSrc& l = src[k];
    if (l.n)
      PFS_HIP(ctx, hipMemcpyAsync(d_entries.as<pfscdc_index_entry>() + sb[k], l.entries,
                                  sizeof(pfscdc_index_entry) * l.n, kind, s));
    if (l.nb) PFS_HIP(ctx, hipMemcpyAsync(d_blob.as<char>() + bb[k], l.blob, l.nb, kind, s));
    if (l.nr)
      PFS_HIP(ctx, hipMemcpyAsync(d_drs.as<pfscdc_full_dataref>() + db[k], l.drs,
                                  sizeof(pfscdc_full_dataref) * l.nr, kind, s));
  }
  PFS_HIP(ctx, hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.ms[0] = clk.lap();
  // ---- rank, then group and count, then the prefix sums
  const MrgIn in{d_entries.as<pfscdc_index_entry>(), d_blob.as<char>(), d_drs.as<pfscdc_full_dataref>(),
                 d_tab.as<uint64_t>(), d_tab.as<uint64_t>() + ns + 1, d_tab.as<uint64_t>() + 2 * (uint64_t)ns + 1,
                 n, ns, mode};
  uint32_t bad = 0;
  PFS_HIP(ctx, launch_merge_rank(in, d_order.as<uint32_t>(), d_bad.as<uint32_t>(), cus, s));
  PFS_HIP(ctx, hipMemcpyAsync(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  if (bad) {  // a stream is not strictly ascending: the ranks are no permutation
    st.ms[1] = clk.lap();
    *ran = false;
    return PFSCDC_OK;
  }
  uint64_t totals[3] = {0, 0, 0}, heads = 0;
  PFS_HIP(ctx, hipMemsetAsync(d_heads.p, 0, sizeof(uint64_t), s));
  PFS_HIP(ctx, launch_merge_group(in, d_order.as<uint32_t>(), d_cnt.as<MrgCount>(),
                                  d_heads.as<unsigned long long>(), cus, s));
  PFS_HIP(ctx, launch_merge_scan(d_cnt.as<MrgCount>(), n, d_base.as<uint64_t>(), s));
  PFS_HIP(ctx, hipMemcpyAsync(totals, d_base.as<uint64_t>() + 3 * n, sizeof totals, hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipMemcpyAsync(&heads, d_heads.p, sizeof heads, hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.ms[1] = clk.lap();
  if (totals[0] > n || totals[1] > nr || totals[2] > nb)  // (the output is a part of the input)
    return ctx_fail(ctx, PFSCDC_EHIP, "index merge: the counts exceed the input");
  // ---- emit: entries, strings and the copy plan, then the DataRefs
  OutList o;
  Guards g;
  DevMem d_copy;
  PFS_HIP(ctx, o.alloc(totals, s, &g));
  PFS_HIP(ctx, d_copy.alloc(sizeof(MrgCopy) * n));
  PFS_HIP(ctx, hipMemsetAsync(d_copy.p, 0, sizeof(MrgCopy) * n, s));
  PFS_HIP(ctx, launch_merge_fill(in, d_order.as<uint32_t>(), d_cnt.as<MrgCount>(), d_base.as<uint64_t>(),
                                 o.entries.as<pfscdc_index_entry>(), o.blob.as<char>(),
                                 d_copy.as<MrgCopy>(), cus, s));
  PFS_HIP(ctx, launch_list_copy(in.drs, d_copy.as<MrgCopy>(), n, o.drs.as<pfscdc_full_dataref>(),
                                cus, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.ms[2] = clk.lap();
  // ---- the list to the host
  if (!keep) {
    out->entries.resize(o.m);
    out->drs.resize(o.nr);
    out->blob.resize(o.nb);
    if (o.m)
      PFS_HIP(ctx, hipMemcpyAsync(out->entries.data(), o.entries.p, o.entries.bytes,
                                  hipMemcpyDeviceToHost, s));
    if (o.nr)
      PFS_HIP(ctx, hipMemcpyAsync(out->drs.data(), o.drs.p, o.drs.bytes, hipMemcpyDeviceToHost, s));
    if (o.nb)
      PFS_HIP(ctx, hipMemcpyAsync(out->blob.data(), o.blob.p, o.blob.bytes, hipMemcpyDeviceToHost, s));
  }
  PFS_HIP(ctx, g.fetch(s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.ms[3] = clk.lap();
  if (!g.ok()) return ctx_fail(ctx, PFSCDC_EHIP, "index merge: a kernel wrote past its array");
  if (keep) o.release(ctx, keep);
  st.n[2] = heads;
  st.n[3] = totals[0];
  return PFSCDC_OK;
}

// index.NewReader(chunks, topIdx, opts...).Iterate: the walk both read entry points share.  The
// selected level-0 entries go to *result.  keep (nullable; only with a filter that selects
// everything): a level of File entries stays on the device as keep's arrays, *kept is set and
// *result stays empty.
int read_index(pfscdc_ctx* ctx, const pfscdc_store* store, const void* root, uint64_t root_len,
               const IdxFilter& f, std::unique_ptr<List>* result, pfscdc_dev_list* keep,
               bool* kept) {
  pfscdc::ctx_index_stats(ctx) = pfscdc::IndexStats();
  if (!root || !root_len) return PFSCDC_OK;  // r.topIdx == nil
  // topLevel(): the root as a stream of one entry
  std::unique_ptr<List> cur(new List());
  {
    const uint8_t *b = (const uint8_t*)root, *e = b + root_len;
    IdxFrame fr;
    if (!pfscdc::idx_parse(b, e, &fr, nullptr, 0) || !idx_append_frame(cur.get(), fr, b, e))
      return pfscdc::ctx_fail(ctx, PFSCDC_ECORRUPT, "the root index does not parse");
  }
  for (uint32_t level = 0;; level++) {
    std::vector<uint32_t> sel, parents;
    int64_t tail = -1;
    const char* why = nullptr;
    if (!select(*cur, f, &sel, &parents, &tail, &why))
      return pfscdc::ctx_fail(ctx, PFSCDC_ECORRUPT,
                              "index level " + std::to_string(level) + " (its parent): " + why);
    if (!sel.empty()) {
      if (sel.size() == cur->entries.size() && (*result)->entries.empty())
        result->swap(cur);  // everything selected: the decoded list is the result
      else
        for (uint32_t i : sel) idx_append_entry(result->get(), *cur, cur->entries[i]);
    }
    if (parents.empty()) break;
    if (level >= 64) return pfscdc::ctx_fail(ctx, PFSCDC_ECORRUPT, "more than 64 index levels");
    std::unique_ptr<List> next(new List());
    if (int rc = read_level(ctx, store, level, *cur, parents, tail, next.get(), keep, kept)) return rc;
    if (kept && *kept) break;
    cur.swap(next);
  }
  return PFSCDC_OK;
}

}  // namespace

extern "C" {

int pfscdc_index_merge_ctx(pfscdc_ctx* ctx, int mode, const pfscdc_index_list* const* lists,
                           uint32_t nfilesets, pfscdc_index_list** out) {
  if (!ctx || !out || (nfilesets && !lists) || nfilesets > (1u << 30) ||
      (mode != PFSCDC_MERGE_FILES && mode != PFSCDC_MERGE_DELETIVE))
    return PFSCDC_EINVAL;
  *out = nullptr;
  MergeStats& st = pfscdc::ctx_merge_stats(ctx);
  st = MergeStats();
  const uint32_t ns = mode == PFSCDC_MERGE_FILES ? 2 * nfilesets : nfilesets;
  if (pfscdc::knob(pfscdc::Knob::IndexMerge) != 0) {
    std::unique_ptr<List> l(new List());
    bool ran = false;
    std::vector<MrgSrc> src(ns);
    for (uint32_t k = 0; k < ns; k++)
      if (lists[k])
        src[k] = MrgSrc{lists[k]->entries.data(), lists[k]->blob.data(), lists[k]->drs.data(),
                        lists[k]->entries.size(), lists[k]->blob.size(), lists[k]->drs.size()};
    if (int rc = merge_device(ctx, mode, src.data(), ns, hipMemcpyHostToDevice, l.get(), nullptr, &ran))
      return rc;
    if (ran) {
      st.n[0] = 1;
      *out = l.release();
      return PFSCDC_OK;
    }
  }
  uint64_t n_in = 0;
  for (uint32_t k = 0; k < ns; k++) n_in += lists[k] ? lists[k]->entries.size() : 0;
  pfscdc::Clock clk;
  const int rc = mode == PFSCDC_MERGE_FILES ? pfscdc_index_merge(lists, nfilesets, out)
                                            : pfscdc_index_merge_deletive(lists, nfilesets, out);
  st.ms[1] += clk.lap();
  st.n[0] = 0;
  st.n[1] = n_in;
  st.n[3] = *out ? (*out)->entries.size() : 0;
  if (rc) return pfscdc::ctx_fail(ctx, rc, "index merge: more than 2^32 - 1 records in the merged list");
  return PFSCDC_OK;
}

int pfscdc_last_merge_stats(pfscdc_ctx* ctx, uint64_t out[4]) {
  if (!ctx || !out) return PFSCDC_EINVAL;
  std::memcpy(out, pfscdc::ctx_merge_stats(ctx).n, sizeof(uint64_t) * 4);
  return PFSCDC_OK;
}

int pfscdc_last_merge_timings(pfscdc_ctx* ctx, float out[4]) {
  if (!ctx || !out) return PFSCDC_EINVAL;
  std::memcpy(out, pfscdc::ctx_merge_stats(ctx).ms, sizeof(float) * 4);
  return PFSCDC_OK;
}

int pfscdc_index_read(pfscdc_ctx* ctx, const pfscdc_store* store, const void* root,
                      uint64_t root_len, const pfscdc_index_filter* filter,
                      pfscdc_index_list** out) {
  if (!ctx || !store || !out) return PFSCDC_EINVAL;
  *out = nullptr;
  std::unique_ptr<List> result(new List());
  if (int rc = read_index(ctx, store, root, root_len, IdxFilter(filter), &result, nullptr, nullptr))
    return rc;
  *out = result.release();
  return PFSCDC_OK;
}

int pfscdc_index_read_dev(pfscdc_ctx* ctx, const pfscdc_store* store, const void* root,
                          uint64_t root_len, const pfscdc_index_filter* filter,
                          pfscdc_dev_list** out) {
  if (!ctx || !store || !out) return PFSCDC_EINVAL;
  *out = nullptr;
  ResidentStats& rs = pfscdc::ctx_resident_stats(ctx);
  rs.n[0] = rs.n[1] = 0;
  const IdxFilter f(filter);
  // no filter: every entry of a level is wanted, and the level of File entries is the result as
  // the decode left it on the device
  const bool whole = f.lower.empty() && f.upper.empty() && f.prefix.empty() && f.tag.empty();
  std::unique_ptr<pfscdc_dev_list> keep;
  if (whole && pfscdc::knob(pfscdc::Knob::IndexDecode) != 0) keep.reset(pfscdc::dev_list_new(ctx));
  std::unique_ptr<List> result(new List());
  bool kept = false;
  if (int rc = read_index(ctx, store, root, root_len, f, &result, keep.get(), &kept)) return rc;
  if (kept) {
    rs.n[0] = 1;
    *out = keep.release();
    return PFSCDC_OK;
  }
  // the host path's list, uploaded
  if (int rc = pfscdc::dev_list_upload(ctx, *result, out)) return rc;
  rs.n[1] = pfscdc::list_bytes(*result);
  return PFSCDC_OK;
}

int pfscdc_index_merge_dev(pfscdc_ctx* ctx, int mode, const pfscdc_dev_list* const* lists,
                           uint32_t nfilesets, pfscdc_dev_list** out) {
  if (!ctx || !out || (nfilesets && !lists) || nfilesets > (1u << 30) ||
      (mode != PFSCDC_MERGE_FILES && mode != PFSCDC_MERGE_DELETIVE))
    return PFSCDC_EINVAL;
  *out = nullptr;
  MergeStats& st = pfscdc::ctx_merge_stats(ctx);
  st = MergeStats();
  const uint32_t ns = mode == PFSCDC_MERGE_FILES ? 2 * nfilesets : nfilesets;
  std::vector<MrgSrc> src(ns);
  for (uint32_t k = 0; k < ns; k++) {
    if (!lists[k]) continue;
    if (lists[k]->device != pfscdc::ctx_device(ctx))
      return pfscdc::ctx_fail(ctx, PFSCDC_EINVAL, "a resident list of another device");
    src[k] = MrgSrc{lists[k]->entries, lists[k]->blob, lists[k]->drs,
                    lists[k]->n, lists[k]->nb, lists[k]->nr};
  }
  std::unique_ptr<pfscdc_dev_list> keep(pfscdc::dev_list_new(ctx));
  bool ran = false;
  if (int rc = merge_device(ctx, mode, src.data(), ns, hipMemcpyDeviceToDevice, nullptr, keep.get(), &ran))
    return rc;
  if (ran) {
    st.n[0] = 1;
    *out = keep.release();
    return PFSCDC_OK;
  }
  // the host arm: a stream out of order, or more than 2^32 - 1 records in
  const float ms_rank = st.ms[1];
  std::vector<std::unique_ptr<List>> own(ns);
  std::vector<const List*> hl(ns, nullptr);
  pfscdc::Clock clk;
  for (uint32_t k = 0; k < ns; k++) {
    if (!lists[k]) continue;
    own[k].reset(new List());
    if (int rc = pfscdc::dev_list_download(ctx, *lists[k], own[k].get())) return rc;
    hl[k] = own[k].get();
  }
  const float ms_down = clk.lap();
  pfscdc_index_list* merged = nullptr;
  int rc = mode == PFSCDC_MERGE_FILES ? pfscdc_index_merge(hl.data(), nfilesets, &merged)
                                      : pfscdc_index_merge_deletive(hl.data(), nfilesets, &merged);
  std::unique_ptr<List> m(merged);
  if (rc) return pfscdc::ctx_fail(ctx, rc, "index merge: more than 2^32 - 1 records in the merged list");
  const float ms_host = clk.lap();
  rc = pfscdc::dev_list_upload(ctx, *m, out);
  const uint64_t n_in = st.n[1];
  st = MergeStats();
  st.n[1] = n_in;
  st.n[3] = m->entries.size();
  st.ms[0] = clk.lap();
  st.ms[1] = ms_rank + ms_host;
  st.ms[3] = ms_down;
  return rc;
}

int pfscdc_last_resident_stats(pfscdc_ctx* ctx, uint64_t out[8]) {
  if (!ctx || !out) return PFSCDC_EINVAL;
  std::memcpy(out, pfscdc::ctx_resident_stats(ctx).n, sizeof(uint64_t) * 8);
  return PFSCDC_OK;
}

int pfscdc_last_index_stats(pfscdc_ctx* ctx, uint64_t out[4]) {
  if (!ctx || !out) return PFSCDC_EINVAL;
  std::memcpy(out, pfscdc::ctx_index_stats(ctx).n, sizeof(uint64_t) * 4);
  return PFSCDC_OK;
}

int pfscdc_last_index_timings(pfscdc_ctx* ctx, float out[5]) {
  if (!ctx || !out) return PFSCDC_EINVAL;
  std::memcpy(out, pfscdc::ctx_index_stats(ctx).ms, sizeof(float) * 5);
  return PFSCDC_OK;
}

}  // extern "C"
