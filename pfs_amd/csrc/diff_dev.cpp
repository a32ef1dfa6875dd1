// diff_dev.cpp — DiffFile over two Sources of one device (pfscdc_source_diff): the driver of the
// diff_* kernels (list_kernels.hip §12) and the hand-over to the host arm (diff.cpp).
#include <memory>
#include <string>
#include <vector>

#include "dev_pass.h"
#include "diff.h"

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

DiffSide side(const pfscdc_source* s) {
  if (!s || !s->list) return DiffSide{RtarList{nullptr, nullptr, nullptr, 0, 0, 0}, nullptr};
  return DiffSide{view(*s->list), (const pfscdc_file_info*)s->infos};
}

// one side to the host: its list and infos
int download(pfscdc_ctx* ctx, const pfscdc_source* s, List* l, std::vector<pfscdc_file_info>* infos,
             uint64_t* bytes) {
  infos->clear();
  if (!s || !s->list) return PFSCDC_OK;
  if (int rc = dev_list_download(ctx, *s->list, l)) return rc;
  const pfscdc_dev_list& d = *s->list;
  *bytes += list_bytes(d);
  infos->resize(d.n);
  if (d.n) {
    hipStream_t st = ctx_stream(ctx);
    PFS_HIP(ctx, hipMemcpyAsync(infos->data(), s->infos, sizeof(pfscdc_file_info) * d.n,
                                hipMemcpyDeviceToHost, st));
    PFS_HIP(ctx, hipStreamSynchronize(st));
    *bytes += sizeof(pfscdc_file_info) * d.n;
  }
  return PFSCDC_OK;
}

// The host arm: both sides come to the host, pfscdc_diff_host's body runs, the pairs and the two
// selections go back.
int host_arm(pfscdc_ctx* ctx, const pfscdc_source* a, const pfscdc_source* b, pfscdc_diff** out) {
  PassStats& st = ctx_diff_stats(ctx);
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
  if (int rc = source_upload(ctx, sa, sia, &d->side[0], &st.n[5])) return rc;
  if (int rc = source_upload(ctx, sb, sib, &d->side[1], &st.n[5])) return rc;
  const uint64_t pb = sizeof(pfscdc_diff_pair) * pairs.size();
  PFS_HIP(ctx, hipMalloc(&d->pairs, pb + kGuard));
  if (pb) {
    PFS_HIP(ctx, hipMemcpyAsync(d->pairs, pairs.data(), pb, hipMemcpyHostToDevice, s));
    PFS_HIP(ctx, hipStreamSynchronize(s));
    st.n[5] += pb;
  }
  st.ms[3] = clk.lap();
  st.n[3] = pairs.size();
  st.n[4] = sa.entries.size() + sb.entries.size() - pairs.size();
  *out = d.release();
  return PFSCDC_OK;
}

// One side's selection: the fill at the prefix-summed ranges, the DataRef copy.
struct SideOut {
  OutList list;
  GuardMem copy, infos;
};

int select_side(pfscdc_ctx* ctx, const DiffSide& in, const MrgCount* sel, const uint64_t* base,
                const uint64_t totals[3], SideOut* o, Guards* g) {
  hipStream_t s = ctx_stream(ctx);
  if (totals[0] > in.l.n || totals[1] > in.l.nr)
    return ctx_fail(ctx, PFSCDC_EHIP, "diff: the counts exceed the input");
  PFS_HIP(ctx, o->list.alloc(totals, s, g));
  PFS_HIP(ctx, copy_plan_alloc(&o->copy, in.l.n, s, g));
  PFS_HIP(ctx, o->infos.alloc(sizeof(pfscdc_file_info) * o->list.m, s));
  g->add(o->infos);
  PFS_HIP(ctx, launch_diff_select(in, sel, base, o->list.entries.as<pfscdc_index_entry>(),
                                  o->list.blob.as<char>(), o->copy.as<MrgCopy>(),
                                  o->infos.as<pfscdc_file_info>(),
                                  o->list.drs.as<pfscdc_full_dataref>(), ctx_num_cus(ctx), s));
  return PFSCDC_OK;
}

int source_diff(pfscdc_ctx* ctx, const pfscdc_source* a, const pfscdc_source* b, pfscdc_diff** out) {
  *out = nullptr;
  PassStats& st = ctx_diff_stats(ctx);
  st = PassStats();
  if (!b || !b->list) return ctx_fail(ctx, PFSCDC_EINVAL, "diff: no side b");
  if ((a && a->device != ctx_device(ctx)) || b->device != ctx_device(ctx))
    return ctx_fail(ctx, PFSCDC_EINVAL, "a source of another device");
  const DiffSide da = side(a), db = side(b);
  const uint64_t na = da.l.n, nb = db.l.n;
  st.n[1] = na;
  st.n[2] = nb;
  PFS_HIP(ctx, hipSetDevice(ctx_device(ctx)));
  if (knob(Knob::Diff) == 0) return host_arm(ctx, a, b, out);
  hipStream_t s = ctx_stream(ctx);
  const int cus = ctx_num_cus(ctx);
  Clock clk;
  // ---- rank, and the prefix sums of side a's selection, side b's selection, side b's records
  GuardMem d_rank, d_sel, d_emit, d_base_a, d_base_b, d_base_e, d_bad;
  Guards g;
  PFS_HIP(ctx, d_rank.alloc(sizeof(DiffRank) * (na + nb), s));
  PFS_HIP(ctx, d_sel.alloc(sizeof(MrgCount) * (na + nb), s));
  PFS_HIP(ctx, d_emit.alloc(sizeof(MrgCount) * nb, s));
  PFS_HIP(ctx, d_base_a.alloc(sizeof(uint64_t) * 3 * (na + 1), s));
  PFS_HIP(ctx, d_base_b.alloc(sizeof(uint64_t) * 3 * (nb + 1), s));
  PFS_HIP(ctx, d_base_e.alloc(sizeof(uint64_t) * 3 * (nb + 1), s));
  PFS_HIP(ctx, d_bad.alloc(sizeof(uint32_t), s));
  for (const GuardMem* x : {&d_rank, &d_sel, &d_emit, &d_base_a, &d_base_b, &d_base_e, &d_bad})
    g.add(*x);
  PFS_HIP(ctx, hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), s));
  PFS_HIP(ctx, launch_diff_rank(da, db, d_rank.as<DiffRank>(), d_sel.as<MrgCount>(),
                                d_emit.as<MrgCount>(), d_bad.as<uint32_t>(), cus, s));
  PFS_HIP(ctx, launch_merge_scan(d_sel.as<MrgCount>(), na, d_base_a.as<uint64_t>(), s));
  PFS_HIP(ctx, launch_merge_scan(d_sel.as<MrgCount>() + na, nb, d_base_b.as<uint64_t>(), s));
  PFS_HIP(ctx, launch_merge_scan(d_emit.as<MrgCount>(), nb, d_base_e.as<uint64_t>(), s));
  uint64_t ta[3] = {0, 0, 0}, tb[3] = {0, 0, 0}, te[3] = {0, 0, 0};
  uint32_t bad = 0;
  PFS_HIP(ctx, hipMemcpyAsync(ta, d_base_a.as<uint64_t>() + 3 * na, sizeof ta, hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipMemcpyAsync(tb, d_base_b.as<uint64_t>() + 3 * nb, sizeof tb, hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipMemcpyAsync(te, d_base_e.as<uint64_t>() + 3 * nb, sizeof te, hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipMemcpyAsync(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.n[6] += sizeof ta + sizeof tb + sizeof te + sizeof bad;
  if (bad) return host_arm(ctx, a, b, out);  // a side's paths decrease: the walk taken literally
  st.ms[0] = clk.lap();
  // ---- the pairs: every a-record, and the b-entries reported alone
  const uint64_t npairs = ta[0] + te[0];
  if (ta[0] > na || te[0] > nb || tb[0] > nb || te[0] > tb[0])
    return ctx_fail(ctx, PFSCDC_EHIP, "diff: the counts exceed the input");
  GuardMem d_pairs;
  PFS_HIP(ctx, d_pairs.alloc(sizeof(pfscdc_diff_pair) * npairs, s));
  g.add(d_pairs);
  PFS_HIP(ctx, launch_diff_fill(na, nb, d_rank.as<DiffRank>(), d_sel.as<MrgCount>(),
                                d_base_a.as<uint64_t>(), d_emit.as<MrgCount>(),
                                d_base_e.as<uint64_t>(), d_pairs.as<pfscdc_diff_pair>(), npairs,
                                cus, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.ms[1] = clk.lap();
  // ---- the two selections
  SideOut sa, sb;
  if (int rc = select_side(ctx, da, d_sel.as<MrgCount>(), d_base_a.as<uint64_t>(), ta, &sa, &g))
    return rc;
  if (int rc = select_side(ctx, db, d_sel.as<MrgCount>() + na, d_base_b.as<uint64_t>(), tb, &sb, &g))
    return rc;
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.ms[2] = clk.lap();
  PFS_HIP(ctx, g.fetch(s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.n[6] += g.host.size();
  if (!g.ok()) return ctx_fail(ctx, PFSCDC_EHIP, "diff: a kernel wrote past its array");
  st.ms[3] = clk.lap();
  std::unique_ptr<pfscdc_diff> d(new pfscdc_diff());
  d->device = ctx_device(ctx);
  d->n = npairs;
  d->pairs = d_pairs.release();
  d->side[0] = source_new(ctx, &sa.list, &sa.infos);
  d->side[1] = source_new(ctx, &sb.list, &sb.infos);
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
  PFS_HIP(ctx, hipSetDevice(d->device));
  PFS_HIP(ctx, hipMemcpyAsync(out, d->pairs, sizeof(pfscdc_diff_pair) * d->n, hipMemcpyDeviceToHost, st));
  PFS_HIP(ctx, hipStreamSynchronize(st));
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
  return pfscdc::last_pass_stats(ctx, pfscdc::ctx_diff_stats, out, nullptr);
}

int pfscdc_last_diff_timings(pfscdc_ctx* ctx, float out[4]) {
  return pfscdc::last_pass_stats(ctx, pfscdc::ctx_diff_stats, nullptr, out);
}

}  // extern "C"
