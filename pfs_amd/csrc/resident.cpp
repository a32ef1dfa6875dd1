// resident.cpp — index lists that stay on the device: the pfscdc_dev_list handle, its copies to
// and from the host, and GetFileTAR over it (the plan and window stages of tar_plan as kernels,
// list_kernels.hip §10; the read path's sibling read_slices_dev_impl is in pfscdc.cpp, the
// batch of the runs' chunks beside StoreBatch in writer.cpp).
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "dev_pass.h"

pfscdc_dev_list::~pfscdc_dev_list() {
  for (void* p : {entries, blob, drs, dpre, ent, off, xblk})
    if (p) (void)hipFree(p);
}

namespace {

using namespace pfscdc;
using List = pfscdc_index_list;

int check_handle(pfscdc_ctx* ctx, const pfscdc_dev_list* d) {
  if (d->device != ctx_device(ctx))
    return ctx_fail(ctx, PFSCDC_EINVAL, "a resident list of another device");
  return PFSCDC_OK;
}

// entry i's path, fetched from the device for an error text
int fetch_path(pfscdc_ctx* ctx, const pfscdc_dev_list& d, uint64_t i, std::string* path) {
  hipStream_t s = ctx_stream(ctx);
  pfscdc_index_entry e;
  PFS_HIP(ctx, hipMemcpyAsync(&e, (const pfscdc_index_entry*)d.entries + i, sizeof e,
                              hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  path->clear();
  if (e.path_off <= d.nb && e.path_len <= d.nb - e.path_off && e.path_len) {
    path->resize(e.path_len);
    PFS_HIP(ctx, hipMemcpyAsync(&(*path)[0], (const char*)d.blob + e.path_off, e.path_len,
                                hipMemcpyDeviceToHost, s));
    PFS_HIP(ctx, hipStreamSynchronize(s));
    path->resize(std::strlen(path->c_str()));  // as the host reads it: up to the first NUL
  }
  return PFSCDC_OK;
}

// The plan stage, once per handle: d.dpre, d.ent, d.off, d.total, or the error tar_plan gives.
int plan(pfscdc_ctx* ctx, pfscdc_dev_list* d) {
  ResidentStats& rs = ctx_resident_stats(ctx);
  const int format = ctx_tar_format(ctx);
  if (d->planned && d->plan_format != format) {  // laid out under the other format: plan again
    PFS_HIP(ctx, hipSetDevice(ctx_device(ctx)));
    for (void** p : {&d->dpre, &d->ent, &d->off, &d->xblk}) {
      if (*p) PFS_HIP(ctx, hipFree(*p));
      *p = nullptr;
    }
    d->planned = false;
  }
  rs.n[7] = d->planned ? 1 : 0;
  if (d->planned) return d->plan_rc ? ctx_fail(ctx, d->plan_rc, d->plan_err) : PFSCDC_OK;
  auto done = [&](int rc, const std::string& msg) {
    d->planned = true;
    d->plan_format = format;
    d->plan_rc = rc;
    d->plan_err = msg;
    return rc ? ctx_fail(ctx, rc, msg) : PFSCDC_OK;
  };
  if (d->nb >= (1ull << 32))
    return done(PFSCDC_EUNSUPPORTED, "a resident list's strings of 4 GiB or more as a tar name table");
  PFS_HIP(ctx, hipSetDevice(ctx_device(ctx)));
  hipStream_t s = ctx_stream(ctx);
  const int cus = ctx_num_cus(ctx);
  const RtarList l = view(*d);
  GuardMem dsz, dpre, ent, span, off, flags;
  Guards g;
  PFS_HIP(ctx, dsz.alloc(sizeof(uint64_t) * l.nr, s));
  PFS_HIP(ctx, dpre.alloc(sizeof(uint64_t) * (l.nr + 1), s));
  PFS_HIP(ctx, ent.alloc(sizeof(TarEntry) * l.n, s));
  PFS_HIP(ctx, span.alloc(sizeof(uint64_t) * l.n, s));
  PFS_HIP(ctx, off.alloc(sizeof(uint64_t) * (l.n + 1), s));
  PFS_HIP(ctx, flags.alloc(16, s));
  for (const GuardMem* m : {&dsz, &dpre, &ent, &span, &off, &flags}) g.add(*m);
  const bool pax = format & PFSCDC_TAR_PAX;
  GuardMem xb, xblk;  // PAX: head blocks other than the main header per entry, and their sums
  if (pax) {
    PFS_HIP(ctx, xb.alloc(sizeof(uint64_t) * l.n, s));
    PFS_HIP(ctx, xblk.alloc(sizeof(uint64_t) * (l.n + 1), s));
    g.add(xb);
    g.add(xblk);
  }
  struct {
    unsigned long long err;
    uint32_t bad, pad;
  } h{kRtarNoErr, 0, 0};
  PFS_HIP(ctx, hipMemcpyAsync(flags.p, &h, sizeof h, hipMemcpyHostToDevice, s));
  PFS_HIP(ctx, launch_rtar_sizes(l.drs, l.nr, dsz.as<uint64_t>(), flags.as<uint32_t>() + 2, cus, s));
  PFS_HIP(ctx, launch_rtar_scan(dsz.as<uint64_t>(), l.nr, dpre.as<uint64_t>(), nullptr, s));
  PFS_HIP(ctx, launch_rtar_entries(l, dpre.as<uint64_t>(), format, ent.as<TarEntry>(),
                                   span.as<uint64_t>(), pax ? xb.as<uint64_t>() : nullptr,
                                   flags.as<unsigned long long>(), cus, s));
  PFS_HIP(ctx, launch_rtar_scan(span.as<uint64_t>(), l.n, off.as<uint64_t>(), ent.as<TarEntry>(), s));
  uint64_t at = 0, nx = 0;
  if (pax) {
    PFS_HIP(ctx, launch_rtar_scan(xb.as<uint64_t>(), l.n, xblk.as<uint64_t>(), nullptr, s));
    PFS_HIP(ctx, hipMemcpyAsync(&nx, xblk.as<uint64_t>() + l.n, sizeof nx, hipMemcpyDeviceToHost, s));
  }
  PFS_HIP(ctx, hipMemcpyAsync(&h, flags.p, sizeof h, hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipMemcpyAsync(&at, off.as<uint64_t>() + l.n, sizeof at, hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, g.fetch(s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  if (!g.ok()) return ctx_fail(ctx, PFSCDC_EHIP, "tar plan: a kernel wrote past its array");
  if (h.bad) return done(PFSCDC_EINVAL, "a DataRef reaches past its chunk");
  uint64_t over = ~0ull;  // the entry at which the offsets pass 2^62
  if (at > (1ull << 62)) {
    // the first i with off[i] > 2^62: entry i - 1 is where tar_plan's running offset passes it
    GuardMem w;
    PFS_HIP(ctx, w.alloc(sizeof(RtarWindow), s));
    RtarWindow hw;
    PFS_HIP(ctx, launch_rtar_window(l, off.as<uint64_t>(), nullptr, 1ull << 62, ~0ull,
                                    w.as<RtarWindow>(), nullptr, s));
    PFS_HIP(ctx, hipMemcpyAsync(&hw, w.p, sizeof hw, hipMemcpyDeviceToHost, s));
    PFS_HIP(ctx, hipStreamSynchronize(s));
    over = hw.i0;  // the last entry whose offset is still <= 2^62
  }
  if (h.err != kRtarNoErr && (h.err >> 8) <= over) {
    const uint64_t i = h.err >> 8;
    std::string path;
    if (int rc = fetch_path(ctx, *d, i, &path)) return rc;
    switch ((uint32_t)(h.err & 0xff)) {
      case kRtarBeyond: return done(PFSCDC_EINVAL, path + ": pieces beyond the array");
      case kRtarNotPacked:
        return done(PFSCDC_EUNSUPPORTED, "tar entry " + path + ": a resident list whose DataRefs are "
                                         "not packed in entry order");
      case kRtarString: return done(PFSCDC_EINVAL, "an entry's path lies outside the blob");
      case kRtarOverflow: return done(PFSCDC_EINVAL, "sizes overflow");
      case kRtarEmpty: return done(PFSCDC_EINVAL, "tar entry " + path + ": empty name");
      case kRtarDirContent:
        return done(PFSCDC_EINVAL, "tar entry " + path + ": a directory entry with content");
      case kRtarNotAscii:
        return done(PFSCDC_EUNSUPPORTED, "tar entry " + path + ": a name that is not ASCII needs a PAX header");
      case kRtarTooBig:
        return done(PFSCDC_EUNSUPPORTED, "tar entry " + path + ": a size above 8 GiB - 1 needs a PAX header");
      case kRtarNoSplit:
        return done(PFSCDC_EUNSUPPORTED, "tar entry " + path + ": a name longer than 100 bytes that does "
                                         "not split needs a PAX header");
      case kRtarPaxLong:
        return done(PFSCDC_EUNSUPPORTED, "tar entry " + path + ": a PAX entry's name longer than "
                                         "65,535 bytes");
      case kRtarPaxJoin:
        return done(PFSCDC_EUNSUPPORTED, "tar entry " + path + ": a PAX entry's name that is not "
                                         "clean (an empty, \".\" or \"..\" component)");
      default: return done(PFSCDC_EINVAL, "tar entry " + path + ": a directory entry with pieces");
    }
  }
  if (at > (1ull << 62)) return done(PFSCDC_EINVAL, "sizes overflow");
  d->dpre = dpre.release();
  d->ent = ent.release();
  d->off = off.release();
  d->xblk = nx ? xblk.release() : nullptr;
  d->total = at + 1024;
  return done(PFSCDC_OK, "");
}

}  // namespace

namespace pfscdc {

pfscdc_dev_list* dev_list_new(pfscdc_ctx* ctx) {
  pfscdc_dev_list* d = new pfscdc_dev_list();
  d->device = ctx_device(ctx);
  return d;
}

int dev_list_upload(pfscdc_ctx* ctx, const pfscdc_index_list& l, pfscdc_dev_list** out) {
  *out = nullptr;
  if (l.entries.size() > 0xffffffffull || l.drs.size() > 0xffffffffull)
    return ctx_fail(ctx, PFSCDC_EUNSUPPORTED, "more than 2^32 - 1 records in a resident list");
  std::unique_ptr<pfscdc_dev_list> d(dev_list_new(ctx));
  PFS_HIP(ctx, hipSetDevice(ctx_device(ctx)));
  hipStream_t s = ctx_stream(ctx);
  d->n = l.entries.size();
  d->nr = l.drs.size();
  d->nb = l.blob.size();
  const uint64_t eb = sizeof(pfscdc_index_entry) * d->n, rb = sizeof(pfscdc_full_dataref) * d->nr;
  PFS_HIP(ctx, hipMalloc(&d->entries, eb + kGuard));
  PFS_HIP(ctx, hipMalloc(&d->drs, rb + kGuard));
  PFS_HIP(ctx, hipMalloc(&d->blob, d->nb + kGuard));
  if (eb) PFS_HIP(ctx, hipMemcpyAsync(d->entries, l.entries.data(), eb, hipMemcpyHostToDevice, s));
  if (rb) PFS_HIP(ctx, hipMemcpyAsync(d->drs, l.drs.data(), rb, hipMemcpyHostToDevice, s));
  if (d->nb) PFS_HIP(ctx, hipMemcpyAsync(d->blob, l.blob.data(), d->nb, hipMemcpyHostToDevice, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  *out = d.release();
  return PFSCDC_OK;
}

int dev_list_download(pfscdc_ctx* ctx, const pfscdc_dev_list& d, pfscdc_index_list* out) {
  if (int rc = check_handle(ctx, &d)) return rc;
  PFS_HIP(ctx, hipSetDevice(ctx_device(ctx)));
  hipStream_t s = ctx_stream(ctx);
  out->entries.resize(d.n);
  out->drs.resize(d.nr);
  out->blob.resize(d.nb);
  out->tar.clear();
  if (d.n)
    PFS_HIP(ctx, hipMemcpyAsync(out->entries.data(), d.entries, sizeof(pfscdc_index_entry) * d.n,
                                hipMemcpyDeviceToHost, s));
  if (d.nr)
    PFS_HIP(ctx, hipMemcpyAsync(out->drs.data(), d.drs, sizeof(pfscdc_full_dataref) * d.nr,
                                hipMemcpyDeviceToHost, s));
  if (d.nb) PFS_HIP(ctx, hipMemcpyAsync(out->blob.data(), d.blob, d.nb, hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  return PFSCDC_OK;
}

hipError_t OutList::alloc(const uint64_t totals[3], hipStream_t s, Guards* g) {
  m = totals[0];
  nr = totals[1];
  nb = totals[2];
  const struct {
    GuardMem* mem;
    uint64_t bytes;
  } want[] = {{&entries, sizeof(pfscdc_index_entry) * m},
              {&blob, nb},
              {&drs, sizeof(pfscdc_full_dataref) * nr}};
  for (const auto& w : want) {
    if (hipError_t e = w.mem->alloc(w.bytes, s)) return e;
    g->add(*w.mem);
  }
  return hipSuccess;
}

pfscdc_dev_list* OutList::release(pfscdc_ctx* ctx, pfscdc_dev_list* keep) {
  pfscdc_dev_list* d = keep ? keep : dev_list_new(ctx);
  std::swap(d->entries, entries.p);  // (what keep held before goes with this OutList)
  std::swap(d->blob, blob.p);
  std::swap(d->drs, drs.p);
  d->n = m;
  d->nr = nr;
  d->nb = nb;
  return d;
}

pfscdc_source* source_new(pfscdc_ctx* ctx, OutList* o, GuardMem* infos) {
  pfscdc_source* src = new pfscdc_source();
  src->device = ctx_device(ctx);
  src->list = o->release(ctx);
  src->infos = infos->release();
  return src;
}

int source_upload(pfscdc_ctx* ctx, const pfscdc_index_list& l,
                  const std::vector<pfscdc_file_info>& infos, pfscdc_source** out, uint64_t* bytes) {
  std::unique_ptr<pfscdc_source> src(new pfscdc_source());
  src->device = ctx_device(ctx);
  if (int rc = dev_list_upload(ctx, l, &src->list)) return rc;
  *bytes += list_bytes(l);
  const uint64_t ib = sizeof(pfscdc_file_info) * infos.size();
  PFS_HIP(ctx, hipMalloc(&src->infos, ib + kGuard));
  if (ib) {
    hipStream_t s = ctx_stream(ctx);
    PFS_HIP(ctx, hipMemcpyAsync(src->infos, infos.data(), ib, hipMemcpyHostToDevice, s));
    PFS_HIP(ctx, hipStreamSynchronize(s));
    *bytes += ib;
  }
  *out = src.release();
  return PFSCDC_OK;
}

}  // namespace pfscdc

extern "C" {

int pfscdc_dev_list_upload(pfscdc_ctx* ctx, const pfscdc_index_list* l, pfscdc_dev_list** out) {
  if (!ctx || !out) return PFSCDC_EINVAL;
  static const List empty;
  return pfscdc::dev_list_upload(ctx, l ? *l : empty, out);
}

int pfscdc_dev_list_download(pfscdc_ctx* ctx, const pfscdc_dev_list* d, pfscdc_index_list** out) {
  if (!ctx || !d || !out) return PFSCDC_EINVAL;
  *out = nullptr;
  std::unique_ptr<List> l(new List());
  if (int rc = pfscdc::dev_list_download(ctx, *d, l.get())) return rc;
  *out = l.release();
  return PFSCDC_OK;
}

uint32_t pfscdc_dev_list_count(const pfscdc_dev_list* d) { return d ? (uint32_t)d->n : 0; }
uint32_t pfscdc_dev_list_num_datarefs(const pfscdc_dev_list* d) { return d ? (uint32_t)d->nr : 0; }
uint64_t pfscdc_dev_list_blob_len(const pfscdc_dev_list* d) { return d ? d->nb : 0; }

int pfscdc_dev_list_free(pfscdc_dev_list* d) {
  if (!d) return PFSCDC_OK;
  (void)hipSetDevice(d->device);
  delete d;
  return PFSCDC_OK;
}

int pfscdc_dev_list_tar_layout(pfscdc_ctx* ctx, pfscdc_dev_list* d, uint64_t* total,
                               uint64_t* entry_offsets) {
  if (!ctx || !d || !total) return PFSCDC_EINVAL;
  if (int rc = check_handle(ctx, d)) return rc;
  if (int rc = plan(ctx, d)) return rc;
  *total = d->total;
  if (entry_offsets) {
    hipStream_t s = ctx_stream(ctx);
    PFS_HIP(ctx, hipMemcpyAsync(entry_offsets, d->off, sizeof(uint64_t) * (d->n + 1),
                                hipMemcpyDeviceToHost, s));
    PFS_HIP(ctx, hipStreamSynchronize(s));
  }
  return PFSCDC_OK;
}

int pfscdc_dev_list_read_tar(pfscdc_ctx* ctx, const pfscdc_store* store, pfscdc_dev_list* d,
                             uint64_t begin, uint64_t len, void* out, uint64_t out_cap,
                             int out_on_device, uint64_t* nwritten) {
  if (!ctx || !store || !d) return PFSCDC_EINVAL;
  if (nwritten) *nwritten = 0;
  if (int rc = check_handle(ctx, d)) return rc;
  ResidentStats& rs = ctx_resident_stats(ctx);
  for (int i = 2; i < 8; i++) rs.n[i] = 0;
  if (int rc = plan(ctx, d)) return rc;
  // the window rules of tar_plan
  const uint64_t total = d->total;
  if (begin % 512) return ctx_fail(ctx, PFSCDC_EINVAL, "begin must be a multiple of 512");
  if (begin > total) return ctx_fail(ctx, PFSCDC_EINVAL, "begin beyond the stream");
  const uint64_t end = len < total - begin ? begin + len : total;
  if (end < total && len % 512)
    return ctx_fail(ctx, PFSCDC_EINVAL, "len must be a multiple of 512 unless the window reaches the end");
  const uint64_t window = end - begin;
  if (window > out_cap || (window && !out))
    return ctx_fail(ctx, PFSCDC_EINVAL, "out_cap below the window's bytes");
  if (window == 0) return PFSCDC_OK;
  PFS_HIP(ctx, hipSetDevice(ctx_device(ctx)));
  hipStream_t s = ctx_stream(ctx);
  const int cus = ctx_num_cus(ctx);
  const RtarList l = view(*d);
  // ---- the entries that meet the window, and their DataRefs
  GuardMem d_w, d_cnt, d_base, d_slices, d_out_off, d_blk, d_runs;
  Guards g;
  struct {
    RtarWindow w;
    uint64_t nx;  // with PAX entries in the list: the window's head blocks besides main headers
  } hw{};
  const size_t wbytes = d->xblk ? sizeof hw : sizeof(RtarWindow);
  PFS_HIP(ctx, d_w.alloc(sizeof hw, s));
  g.add(d_w);
  PFS_HIP(ctx, launch_rtar_window(l, (const uint64_t*)d->off, (const uint64_t*)d->xblk, begin, end,
                                  d_w.as<RtarWindow>(), d_w.as<uint64_t>() + 4, s));
  PFS_HIP(ctx, hipMemcpyAsync(&hw, d_w.p, wbytes, hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  rs.n[5] += wbytes;
  const RtarWindow w = hw.w;
  // (a name of kTarMaxName bytes has 130 blocks in front of its main header)
  if (w.i0 > w.i1 || w.i1 > l.n || w.k0 > w.k1 || w.k1 > l.nr || hw.nx > (w.i1 - w.i0) * 130)
    return ctx_fail(ctx, PFSCDC_EHIP, "tar window: the search left the list");
  // ---- pieces: count, scan, fill
  const uint64_t nk = w.k1 - w.k0;
  const RtarPieces pc{l, (const uint64_t*)d->dpre, (const TarEntry*)d->ent, w, begin, end};
  uint64_t totals[3] = {0, 0, 0};  // pieces, runs, keystream blocks
  PFS_HIP(ctx, d_cnt.alloc(sizeof(MrgCount) * nk, s));
  PFS_HIP(ctx, d_base.alloc(sizeof(uint64_t) * 3 * (nk + 1), s));
  g.add(d_cnt);
  g.add(d_base);
  if (nk) {
    PFS_HIP(ctx, launch_rtar_pieces(pc, d_cnt.as<MrgCount>(), nullptr, nullptr, nullptr, nullptr,
                                    nullptr, cus, s));
    PFS_HIP(ctx, launch_merge_scan(d_cnt.as<MrgCount>(), nk, d_base.as<uint64_t>(), s));
    PFS_HIP(ctx, hipMemcpyAsync(totals, d_base.as<uint64_t>() + 3 * nk, sizeof totals,
                                hipMemcpyDeviceToHost, s));
    PFS_HIP(ctx, hipStreamSynchronize(s));
    rs.n[5] += sizeof totals;
  }
  const uint64_t m = totals[0], nruns = totals[1], nblocks = totals[2];
  if (m > nk || nruns > m || m > 0xffffffffull)
    return ctx_fail(ctx, PFSCDC_EHIP, "tar window: the counts exceed the input");
  PFS_HIP(ctx, d_slices.alloc(sizeof(pfscdc_slice) * m, s));
  PFS_HIP(ctx, d_out_off.alloc(sizeof(uint64_t) * (m + 1), s));
  PFS_HIP(ctx, d_blk.alloc(sizeof(uint64_t) * (m + 1), s));
  PFS_HIP(ctx, d_runs.alloc(sizeof(RtarRun) * nruns, s));
  for (const GuardMem* x : {&d_slices, &d_out_off, &d_blk, &d_runs}) g.add(*x);
  std::vector<RtarRun> runs(nruns);
  if (m) {
    PFS_HIP(ctx, launch_rtar_pieces(pc, d_cnt.as<MrgCount>(), d_base.as<uint64_t>(),
                                    d_slices.as<pfscdc_slice>(), d_out_off.as<uint64_t>(),
                                    d_blk.as<uint64_t>(), d_runs.as<RtarRun>(), cus, s));
    PFS_HIP(ctx, hipMemcpyAsync(runs.data(), d_runs.p, sizeof(RtarRun) * nruns,
                                hipMemcpyDeviceToHost, s));
    rs.n[5] += sizeof(RtarRun) * nruns;
  } else {
    const uint64_t zero[1] = {0};  // the arrays' one entry each: no pieces, no blocks
    PFS_HIP(ctx, hipMemcpyAsync(d_out_off.p, zero, sizeof zero, hipMemcpyHostToDevice, s));
    PFS_HIP(ctx, hipMemcpyAsync(d_blk.p, zero, sizeof zero, hipMemcpyHostToDevice, s));
    rs.n[6] += 2 * sizeof zero;
  }
  PFS_HIP(ctx, g.fetch(s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  rs.n[5] += g.host.size();
  if (!g.ok()) return ctx_fail(ctx, PFSCDC_EHIP, "tar window: a kernel wrote past its array");
  // ---- the runs' chunks: looked up and deduplicated on the host, one number per run back
  RunBatch b;
  const int brc = store_batch_runs(store, runs.data(), (uint32_t)nruns, &b);
  if (brc == PFSCDC_ENOTFOUND) return ctx_fail(ctx, brc, "a chunk id is not in the store");
  if (brc == PFSCDC_ECORRUPT)
    return ctx_fail(ctx, brc, "a stored chunk's length differs from its Ref's");
  if (brc) return brc;
  const uint32_t nchunks = (uint32_t)b.refs.size();
  if (b.offs.empty()) b.offs.assign(1, 0);
  // the run -> chunk table and the chunks' stored offsets; the kernel that sets slice.chunk also
  // holds every slice against its chunk's stored length, since the gather checks nothing
  GuardMem d_table, d_coffs, d_bad;
  PFS_HIP(ctx, d_table.alloc(sizeof(uint32_t) * nruns, s));
  PFS_HIP(ctx, d_coffs.alloc(sizeof(uint64_t) * (nchunks + 1), s));
  PFS_HIP(ctx, d_bad.alloc(sizeof(uint32_t), s));
  if (nruns) {
    uint32_t bad = 0;
    PFS_HIP(ctx, hipMemcpyAsync(d_table.p, b.table.data(), sizeof(uint32_t) * nruns,
                                hipMemcpyHostToDevice, s));
    PFS_HIP(ctx, hipMemcpyAsync(d_coffs.p, b.offs.data(), sizeof(uint64_t) * (nchunks + 1),
                                hipMemcpyHostToDevice, s));
    PFS_HIP(ctx, hipMemsetAsync(d_bad.p, 0, sizeof bad, s));
    rs.n[6] += sizeof(uint32_t) * nruns + sizeof(uint64_t) * (nchunks + 1);
    PFS_HIP(ctx, launch_rtar_chunks(d_slices.as<pfscdc_slice>(), m, d_table.as<uint32_t>(),
                                    d_coffs.as<uint64_t>(), nchunks, d_bad.as<uint32_t>(), cus, s));
    PFS_HIP(ctx, hipMemcpyAsync(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost, s));
    PFS_HIP(ctx, hipStreamSynchronize(s));
    rs.n[5] += sizeof bad;
    if (bad) return ctx_fail(ctx, PFSCDC_ECORRUPT, "a DataRef reaches past its stored chunk");
  }
  rs.n[2] = nruns;
  rs.n[3] = nchunks;
  rs.n[4] = m;
  std::vector<uint8_t> ok(nchunks + 1);
  const DevSlices sl{d_slices.as<pfscdc_slice>(), d_out_off.as<uint64_t>(), d_blk.as<uint64_t>(),
                     (uint32_t)m, nblocks};
  const DevTar tar{(const TarEntry*)d->ent + w.i0, (const uint8_t*)d->blob, (uint32_t)(w.i1 - w.i0),
                   begin, end, total, hw.nx ? (const uint64_t*)d->xblk + w.i0 : nullptr, hw.nx};
  if (int rc = read_slices_dev_impl(ctx, b.ct.data(), b.ct.size(), b.offs.data(), nchunks,
                                    b.refs.data(), sl, out, out_on_device, ok.data(), tar,
                                    &rs.n[6], &rs.n[5]))
    return rc;
  if (nwritten) *nwritten = window;
  return PFSCDC_OK;
}

}  // extern "C"
