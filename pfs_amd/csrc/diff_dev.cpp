// diff_dev.cpp — DiffFile over two Sources of one device (pfscdc_source_diff): the driver of the
// diff_* kernels (cdc_kernels.hip §12) and the hand-over to the host arm (diff.cpp).
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "dev_list.h"
#include "diff.h"
#include "index_list.h"
#include "pfscdc_internal.h"

struct pfscdc_diff {
  int device = 0;
  uint64_t n = 0;
  void* pairs = nullptr;  // n pfscdc_diff_pair, on the device
  pfscdc_source* side[2] = {nullptr, nullptr};
  ~pfscdc_diff() {
    if (pairs) (void)hipFree(pairs);
    delete side[0];
    delete side[1];
  }
};

namespace {

using namespace pfscdc;
using List = pfscdc_index_list;

#define DIFF_HIP(ctx, expr)                                                            \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return pfscdc::ctx_fail(ctx, e_ == hipErrorOutOfMemory ? PFSCDC_ENOMEM : PFSCDC_EHIP, \
                              std::string(#expr) + ": " + hipGetErrorString(e_));      \
  } while (0)

struct Clock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  float lap() {  // ms since the last lap
    const auto t1 = std::chrono::steady_clock::now();
    const float ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
    t0 = t1;
    return ms;
  }
};

DiffSide view(const pfscdc_source* s) {
  if (!s || !s->list) return DiffSide{RtarList{nullptr, nullptr, nullptr, 0, 0, 0}, nullptr};
  const pfscdc_dev_list& d = *s->list;
  return DiffSide{RtarList{(const pfscdc_index_entry*)d.entries, (const char*)d.blob,
                           (const pfscdc_full_dataref*)d.drs, d.n, d.nr, d.nb},
                  (const pfscdc_file_info*)s->infos};
}

// one side to the host: its list and infos
int download(pfscdc_ctx* ctx, const pfscdc_source* s, List* l, std::vector<pfscdc_file_info>* infos,
             uint64_t* bytes) {
  infos->clear();
  if (!s || !s->list) return PFSCDC_OK;
  if (int rc = dev_list_download(ctx, *s->list, l)) return rc;
  const pfscdc_dev_list& d = *s->list;
  *bytes += sizeof(pfscdc_index_entry) * d.n + sizeof(pfscdc_full_dataref) * d.nr + d.nb;
  infos->resize(d.n);
  if (d.n) {
    hipStream_t st = ctx_stream(ctx);
    DIFF_HIP(ctx, hipMemcpyAsync(infos->data(), s->infos, sizeof(pfscdc_file_info) * d.n,
                                 hipMemcpyDeviceToHost, st));
    DIFF_HIP(ctx, hipStreamSynchronize(st));
    *bytes += sizeof(pfscdc_file_info) * d.n;
  }
  return PFSCDC_OK;
}

// a selection made on the host as a source on the device
int upload(pfscdc_ctx* ctx, const List& l, const std::vector<pfscdc_file_info>& infos,
           pfscdc_source** out, uint64_t* bytes) {
  std::unique_ptr<pfscdc_source> src(new pfscdc_source());
  src->device = ctx_device(ctx);
  if (int rc = dev_list_upload(ctx, l, &src->list)) return rc;
  *bytes += sizeof(pfscdc_index_entry) * l.entries.size() +
            sizeof(pfscdc_full_dataref) * l.drs.size() + l.blob.size();
  const uint64_t ib = sizeof(pfscdc_file_info) * infos.size();
  DIFF_HIP(ctx, hipMalloc(&src->infos, ib + kGuard));
  if (ib) {
    hipStream_t st = ctx_stream(ctx);
    DIFF_HIP(ctx, hipMemcpyAsync(src->infos, infos.data(), ib, hipMemcpyHostToDevice, st));
    DIFF_HIP(ctx, hipStreamSynchronize(st));
    *bytes += ib;
  }
  *out = src.release();
  return PFSCDC_OK;
}

// The host arm: both sides come to the host, pfscdc_diff_host's body runs, the pairs and the two
// selections go back.
int host_arm(pfscdc_ctx* ctx, const pfscdc_source* a, const pfscdc_source* b, pfscdc_diff** out) {
  DiffStats& st = ctx_diff_stats(ctx);
  Clock clk;
  hipStream_t s = ctx_stream(ctx);
  List la, lb;
  std::vector<pfscdc_file_info> ia, ib;
  if (int rc = download(ctx, a, &la, &ia, &st.n[6])) return rc;
  if (int rc = download(ctx, b, &lb, &ib, &st.n[6])) return rc;
  st.ms[0] = clk.lap();
  std::vector<pfscdc_diff_pair> pairs;
  if (int rc = diff_host(la, ia.data(), lb, ib.data(), &pairs))
    return ctx_fail(ctx, rc, "diff: a side's entries lie outside its arrays");
  st.ms[1] = clk.lap();
  List sa, sb;
  std::vector<pfscdc_file_info> sia, sib;
  diff_select(la, ia.data(), pairs, 0, &sa, &sia);
  diff_select(lb, ib.data(), pairs, 1, &sb, &sib);
  st.ms[2] = clk.lap();
  std::unique_ptr<pfscdc_diff> d(new pfscdc_diff());
  d->device = ctx_device(ctx);
  d->n = pairs.size();
  if (int rc = upload(ctx, sa, sia, &d->side[0], &st.n[5])) return rc;
  if (int rc = upload(ctx, sb, sib, &d->side[1], &st.n[5])) return rc;
  const uint64_t pb = sizeof(pfscdc_diff_pair) * pairs.size();
  DIFF_HIP(ctx, hipMalloc(&d->pairs, pb + kGuard));
  if (pb) {
    DIFF_HIP(ctx, hipMemcpyAsync(d->pairs, pairs.data(), pb, hipMemcpyHostToDevice, s));
    DIFF_HIP(ctx, hipStreamSynchronize(s));
    st.n[5] += pb;
  }
  st.ms[3] = clk.lap();
  st.n[3] = pairs.size();
  st.n[4] = sa.entries.size() + sb.entries.size() - pairs.size();
  *out = d.release();
  return PFSCDC_OK;
}

// One side's selection: the fill at the prefix-summed ranges, the DataRef copy.
struct Selection {
  GuardMem entries, blob, drs, copy, infos;
  uint64_t m = 0, nr = 0, nb = 0;
};

int select_side(pfscdc_ctx* ctx, const DiffSide& in, const MrgCount* sel, const uint64_t* base,
                const uint64_t totals[3], Selection* o, Guards* g) {
  hipStream_t s = ctx_stream(ctx);
  o->m = totals[0];
  o->nr = totals[1];
  o->nb = totals[2];
  if (o->m > in.l.n || o->nr > in.l.nr)
    return ctx_fail(ctx, PFSCDC_EHIP, "diff: the counts exceed the input");
  DIFF_HIP(ctx, o->entries.alloc(sizeof(pfscdc_index_entry) * o->m, s));
  DIFF_HIP(ctx, o->blob.alloc(o->nb, s));
  DIFF_HIP(ctx, o->drs.alloc(sizeof(pfscdc_full_dataref) * o->nr, s));
  DIFF_HIP(ctx, o->copy.alloc(sizeof(MrgCopy) * in.l.n, s));
  DIFF_HIP(ctx, o->infos.alloc(sizeof(pfscdc_file_info) * o->m, s));
  for (const GuardMem* x : {&o->entries, &o->blob, &o->drs, &o->copy, &o->infos}) g->add(*x);
  if (in.l.n) DIFF_HIP(ctx, hipMemsetAsync(o->copy.p, 0, sizeof(MrgCopy) * in.l.n, s));
  DIFF_HIP(ctx, launch_diff_select(in, sel, base, o->entries.as<pfscdc_index_entry>(),
                                   o->blob.as<char>(), o->copy.as<MrgCopy>(),
                                   o->infos.as<pfscdc_file_info>(),
                                   o->drs.as<pfscdc_full_dataref>(), ctx_num_cus(ctx), s));
  return PFSCDC_OK;
}

pfscdc_source* as_source(pfscdc_ctx* ctx, Selection* o) {
  pfscdc_source* src = new pfscdc_source();
  src->device = ctx_device(ctx);
  src->list = dev_list_new(ctx);
  src->list->n = o->m;
  src->list->nr = o->nr;
  src->list->nb = o->nb;
  src->list->entries = o->entries.release();
  src->list->blob = o->blob.release();
  src->list->drs = o->drs.release();
  src->infos = o->infos.release();
  return src;
}

int source_diff(pfscdc_ctx* ctx, const pfscdc_source* a, const pfscdc_source* b, pfscdc_diff** out) {
  *out = nullptr;
  DiffStats& st = ctx_diff_stats(ctx);
  st = DiffStats();
  if (!b || !b->list) return ctx_fail(ctx, PFSCDC_EINVAL, "diff: no side b");
  if ((a && a->device != ctx_device(ctx)) || b->device != ctx_device(ctx))
    return ctx_fail(ctx, PFSCDC_EINVAL, "a source of another device");
  const DiffSide da = view(a), db = view(b);
  const uint64_t na = da.l.n, nb = db.l.n;
  st.n[1] = na;
  st.n[2] = nb;
  DIFF_HIP(ctx, hipSetDevice(ctx_device(ctx)));
  if (knob(Knob::Diff) == 0) return host_arm(ctx, a, b, out);
  hipStream_t s = ctx_stream(ctx);
  const int cus = ctx_num_cus(ctx);
  Clock clk;
  // ---- rank, and the prefix sums of side a's selection, side b's selection, side b's records
  GuardMem d_rank, d_sel, d_emit, d_base_a, d_base_b, d_base_e, d_bad;
  Guards g;
  DIFF_HIP(ctx, d_rank.alloc(sizeof(DiffRank) * (na + nb), s));
  DIFF_HIP(ctx, d_sel.alloc(sizeof(MrgCount) * (na + nb), s));
  DIFF_HIP(ctx, d_emit.alloc(sizeof(MrgCount) * nb, s));
  DIFF_HIP(ctx, d_base_a.alloc(sizeof(uint64_t) * 3 * (na + 1), s));
  DIFF_HIP(ctx, d_base_b.alloc(sizeof(uint64_t) * 3 * (nb + 1), s));
  DIFF_HIP(ctx, d_base_e.alloc(sizeof(uint64_t) * 3 * (nb + 1), s));
  DIFF_HIP(ctx, d_bad.alloc(sizeof(uint32_t), s));
  for (const GuardMem* x : {&d_rank, &d_sel, &d_emit, &d_base_a, &d_base_b, &d_base_e, &d_bad})
    g.add(*x);
  DIFF_HIP(ctx, hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), s));
  DIFF_HIP(ctx, launch_diff_rank(da, db, d_rank.as<DiffRank>(), d_sel.as<MrgCount>(),
                                 d_emit.as<MrgCount>(), d_bad.as<uint32_t>(), cus, s));
  DIFF_HIP(ctx, launch_merge_scan(d_sel.as<MrgCount>(), na, d_base_a.as<uint64_t>(), s));
  DIFF_HIP(ctx, launch_merge_scan(d_sel.as<MrgCount>() + na, nb, d_base_b.as<uint64_t>(), s));
  DIFF_HIP(ctx, launch_merge_scan(d_emit.as<MrgCount>(), nb, d_base_e.as<uint64_t>(), s));
  uint64_t ta[3] = {0, 0, 0}, tb[3] = {0, 0, 0}, te[3] = {0, 0, 0};
  uint32_t bad = 0;
  DIFF_HIP(ctx, hipMemcpyAsync(ta, d_base_a.as<uint64_t>() + 3 * na, sizeof ta, hipMemcpyDeviceToHost, s));
  DIFF_HIP(ctx, hipMemcpyAsync(tb, d_base_b.as<uint64_t>() + 3 * nb, sizeof tb, hipMemcpyDeviceToHost, s));
  DIFF_HIP(ctx, hipMemcpyAsync(te, d_base_e.as<uint64_t>() + 3 * nb, sizeof te, hipMemcpyDeviceToHost, s));
  DIFF_HIP(ctx, hipMemcpyAsync(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost, s));
  DIFF_HIP(ctx, hipStreamSynchronize(s));
  st.n[6] += sizeof ta + sizeof tb + sizeof te + sizeof bad;
  if (bad) return host_arm(ctx, a, b, out);  // a side's paths decrease: the walk taken literally
  st.ms[0] = clk.lap();
  // ---- the pairs: every a-record, and the b-entries reported alone
  const uint64_t npairs = ta[0] + te[0];
  if (ta[0] > na || te[0] > nb || tb[0] > nb || te[0] > tb[0])
    return ctx_fail(ctx, PFSCDC_EHIP, "diff: the counts exceed the input");
  GuardMem d_pairs;
  DIFF_HIP(ctx, d_pairs.alloc(sizeof(pfscdc_diff_pair) * npairs, s));
  g.add(d_pairs);
  DIFF_HIP(ctx, launch_diff_fill(na, nb, d_rank.as<DiffRank>(), d_sel.as<MrgCount>(),
                                 d_base_a.as<uint64_t>(), d_emit.as<MrgCount>(),
                                 d_base_e.as<uint64_t>(), d_pairs.as<pfscdc_diff_pair>(), npairs,
                                 cus, s));
  DIFF_HIP(ctx, hipStreamSynchronize(s));
  st.ms[1] = clk.lap();
  // ---- the two selections
  Selection sa, sb;
  if (int rc = select_side(ctx, da, d_sel.as<MrgCount>(), d_base_a.as<uint64_t>(), ta, &sa, &g))
    return rc;
  if (int rc = select_side(ctx, db, d_sel.as<MrgCount>() + na, d_base_b.as<uint64_t>(), tb, &sb, &g))
    return rc;
  DIFF_HIP(ctx, hipStreamSynchronize(s));
  st.ms[2] = clk.lap();
  DIFF_HIP(ctx, g.fetch(s));
  DIFF_HIP(ctx, hipStreamSynchronize(s));
  st.n[6] += g.host.size();
  if (!g.ok()) return ctx_fail(ctx, PFSCDC_EHIP, "diff: a kernel wrote past its array");
  st.ms[3] = clk.lap();
  std::unique_ptr<pfscdc_diff> d(new pfscdc_diff());
  d->device = ctx_device(ctx);
  d->n = npairs;
  d->pairs = d_pairs.release();
  d->side[0] = as_source(ctx, &sa);
  d->side[1] = as_source(ctx, &sb);
  st.n[0] = 1;
  st.n[3] = npairs;
  st.n[4] = tb[0] - te[0];
  *out = d.release();
  return PFSCDC_OK;
}

}  // namespace

extern "C" {

int pfscdc_source_diff(pfscdc_ctx* ctx, const pfscdc_source* a, const pfscdc_source* b,
                       pfscdc_diff** out) {
  if (!ctx || !out) return PFSCDC_EINVAL;
  return source_diff(ctx, a, b, out);
}

uint64_t pfscdc_diff_count(const pfscdc_diff* d) { return d ? d->n : 0; }

int pfscdc_diff_pairs(pfscdc_ctx* ctx, const pfscdc_diff* d, pfscdc_diff_pair* out) {
  if (!ctx || !d) return PFSCDC_EINVAL;
  if (d->device != pfscdc::ctx_device(ctx))
    return pfscdc::ctx_fail(ctx, PFSCDC_EINVAL, "a diff of another device");
  if (!d->n) return PFSCDC_OK;
  if (!out) return PFSCDC_EINVAL;
  hipStream_t st = pfscdc::ctx_stream(ctx);
  DIFF_HIP(ctx, hipSetDevice(d->device));
  DIFF_HIP(ctx, hipMemcpyAsync(out, d->pairs, sizeof(pfscdc_diff_pair) * d->n, hipMemcpyDeviceToHost, st));
  DIFF_HIP(ctx, hipStreamSynchronize(st));
  return PFSCDC_OK;
}

pfscdc_source* pfscdc_diff_side(pfscdc_diff* d, int side) {
  return d && (side == 0 || side == 1) ? d->side[side] : nullptr;
}

int pfscdc_diff_free(pfscdc_diff* d) {
  if (!d) return PFSCDC_OK;
  (void)hipSetDevice(d->device);
  delete d;
  return PFSCDC_OK;
}

int pfscdc_last_diff_stats(pfscdc_ctx* ctx, uint64_t out[8]) {
  if (!ctx || !out) return PFSCDC_EINVAL;
  std::memcpy(out, pfscdc::ctx_diff_stats(ctx).n, sizeof(uint64_t) * 8);
  return PFSCDC_OK;
}

int pfscdc_last_diff_timings(pfscdc_ctx* ctx, float out[4]) {
  if (!ctx || !out) return PFSCDC_EINVAL;
  std::memcpy(out, pfscdc::ctx_diff_stats(ctx).ms, sizeof(float) * 4);
  return PFSCDC_OK;
}

}  // extern "C"
