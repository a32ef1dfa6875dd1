// copy_map_dev.cpp — CopyFile's selection and path transform over a device-resident list
// (pfscdc_dev_list_copy_map): the driver of the cmap_* kernels (list_kernels.hip §13) and the
// hand-over to the host arm (copy_map.cpp).
#include <memory>
#include <string>

#include "copy_map.h"
#include "dev_pass.h"

namespace {

using namespace pfscdc;
using List = pfscdc_index_list;

// The host arm: the list comes to the host, pfscdc_copy_map_host's body runs, its result goes back.
int host_arm(pfscdc_ctx* ctx, const pfscdc_dev_list& in, const CopyArg& a, pfscdc_dev_list** out) {
  PassStats& st = ctx_copy_map_stats(ctx);
  Clock clk;
  List l, res;
  if (int rc = dev_list_download(ctx, in, &l)) return rc;
  st.n[6] += list_bytes(l);
  st.ms[0] = clk.lap();
  std::string err;
  if (int rc = copy_map_host(l, a, &res, &err)) return ctx_fail(ctx, rc, err);
  st.ms[1] = clk.lap();
  if (int rc = dev_list_upload(ctx, res, out)) return rc;
  st.n[5] += list_bytes(res);
  st.ms[2] = clk.lap();
  st.n[2] = res.entries.size();
  st.n[3] = res.drs.size();
  st.n[4] = res.blob.size();
  return PFSCDC_OK;
}

int copy_map(pfscdc_ctx* ctx, const pfscdc_dev_list& in, const CopyArg& a, pfscdc_dev_list** out) {
  *out = nullptr;
  PassStats& st = ctx_copy_map_stats(ctx);
  st = PassStats();
  st.n[1] = in.n;
  if (in.device != ctx_device(ctx))
    return ctx_fail(ctx, PFSCDC_EINVAL, "a resident list of another device");
  PFS_HIP(ctx, hipSetDevice(ctx_device(ctx)));
  if (knob(Knob::CopyMap) == 0) return host_arm(ctx, in, a, out);
  hipStream_t s = ctx_stream(ctx);
  const int cus = ctx_num_cus(ctx);
  const RtarList l = view(in);
  Clock clk;
  // ---- select: count, prefix sums
  GuardMem d_arg, d_cnt, d_base, d_bad;
  Guards g;
  const std::string args = a.src + a.dst + a.tag;
  PFS_HIP(ctx, d_arg.alloc(args.size(), s));
  PFS_HIP(ctx, d_cnt.alloc(sizeof(MrgCount) * l.n, s));
  PFS_HIP(ctx, d_base.alloc(sizeof(uint64_t) * 3 * (l.n + 1), s));
  PFS_HIP(ctx, d_bad.alloc(sizeof(uint32_t), s));
  for (const GuardMem* x : {&d_cnt, &d_base, &d_bad}) g.add(*x);
  PFS_HIP(ctx, hipMemcpyAsync(d_arg.p, args.data(), args.size(), hipMemcpyHostToDevice, s));
  st.n[5] += args.size();
  PFS_HIP(ctx, hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), s));
  const CmapPred pr{d_arg.as<char>(), d_arg.as<char>() + a.src.size(),
                    d_arg.as<char>() + a.src.size() + a.dst.size(), (uint32_t)a.src.size(),
                    (uint32_t)a.dst.size(), (uint32_t)a.tag.size(), 0};
  PFS_HIP(ctx, launch_cmap_count(l, pr, d_cnt.as<MrgCount>(), d_bad.as<uint32_t>(), cus, s));
  PFS_HIP(ctx, launch_merge_scan(d_cnt.as<MrgCount>(), l.n, d_base.as<uint64_t>(), s));
  uint64_t totals[3] = {0, 0, 0};
  uint32_t bad = 0;
  PFS_HIP(ctx, hipMemcpyAsync(totals, d_base.as<uint64_t>() + 3 * l.n, sizeof totals,
                              hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipMemcpyAsync(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.n[6] += sizeof totals + sizeof bad;
  if (bad & kSrcMalformed)
    return ctx_fail(ctx, PFSCDC_EINVAL, "an entry's strings or DataRefs lie outside the list's arrays");
  // a Range, a list out of order, a selected path that is not clean: the reference taken literally
  if (bad) return host_arm(ctx, in, a, out);
  st.ms[0] = clk.lap();
  const uint64_t m = totals[0], nr = totals[1], nb = totals[2];
  if (m > l.n || nr > l.nr) return ctx_fail(ctx, PFSCDC_EHIP, "copy map: the counts exceed the input");
  // ---- fill: entries and strings, then the DataRefs
  OutList o;
  GuardMem d_copy;
  PFS_HIP(ctx, o.alloc(totals, s, &g));
  PFS_HIP(ctx, copy_plan_alloc(&d_copy, l.n, s, &g));
  PFS_HIP(ctx, launch_cmap_fill(l, pr, d_cnt.as<MrgCount>(), d_base.as<uint64_t>(),
                                o.entries.as<pfscdc_index_entry>(), o.blob.as<char>(),
                                d_copy.as<MrgCopy>(), cus, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.ms[1] = clk.lap();
  PFS_HIP(ctx, launch_list_copy(l.drs, d_copy.as<MrgCopy>(), l.n, o.drs.as<pfscdc_full_dataref>(),
                                cus, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.ms[2] = clk.lap();
  PFS_HIP(ctx, g.fetch(s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.n[6] += g.host.size();
  if (!g.ok()) return ctx_fail(ctx, PFSCDC_EHIP, "copy map: a kernel wrote past its array");
  st.ms[3] = clk.lap();
  st.n[0] = 1;
  st.n[2] = m;
  st.n[3] = nr;
  st.n[4] = nb;
  *out = o.release(ctx);
  return PFSCDC_OK;
}

}  // namespace

extern "C" {

int pfscdc_dev_list_copy_map(pfscdc_ctx* ctx, const pfscdc_dev_list* in, const char* src,
                             const char* src_tag, const char* dst, pfscdc_dev_list** out) {
  if (!ctx || !in || !out) return PFSCDC_EINVAL;
  return copy_map(ctx, *in, pfscdc::copy_arg(src, src_tag, dst), out);
}

int pfscdc_copy_map_list(pfscdc_ctx* ctx, const pfscdc_index_list* in, const char* src,
                         const char* src_tag, const char* dst, pfscdc_dev_list** out) {
  if (!ctx || !out) return PFSCDC_EINVAL;
  *out = nullptr;
  static const List empty;
  const List& l = in ? *in : empty;
  pfscdc_dev_list* d = nullptr;
  if (int rc = pfscdc::dev_list_upload(ctx, l, &d)) return rc;
  const int rc = copy_map(ctx, *d, pfscdc::copy_arg(src, src_tag, dst), out);
  pfscdc::ctx_copy_map_stats(ctx).n[5] += list_bytes(l);
  (void)hipSetDevice(d->device);
  delete d;
  return rc;
}

int pfscdc_last_copy_map_stats(pfscdc_ctx* ctx, uint64_t out[8]) {
  return pfscdc::last_pass_stats(ctx, pfscdc::ctx_copy_map_stats, out, nullptr);
}

int pfscdc_last_copy_map_timings(pfscdc_ctx* ctx, float out[4]) {
  return pfscdc::last_pass_stats(ctx, pfscdc::ctx_copy_map_stats, nullptr, out);
}

}  // extern "C"
