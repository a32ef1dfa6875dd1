// source_dev.cpp — the Source over a device-resident list (pfscdc_source_open): the driver of
// the src_* kernels (list_kernels.hip §11) and the hand-over to the host arm (source.cpp).
#include <memory>
#include <string>
#include <vector>

#include "dev_pass.h"
#include "source.h"

namespace {

using namespace pfscdc;
using List = pfscdc_index_list;

// The host arm: the list comes to the host, pfscdc_source_host's body runs, its result goes back.
int host_arm(pfscdc_ctx* ctx, const pfscdc_dev_list& in, const SrcArg& a, const uint8_t* leaf,
             int leaf_on_device, pfscdc_source** out) {
  PassStats& st = ctx_source_stats(ctx);
  Clock clk;
  hipStream_t s = ctx_stream(ctx);
  List l, res;
  if (int rc = dev_list_download(ctx, in, &l)) return rc;
  st.n[7] += list_bytes(in);
  std::vector<uint8_t> hleaf;
  if (leaf && leaf_on_device && in.n) {
    hleaf.resize(32 * in.n);
    PFS_HIP(ctx, hipMemcpyAsync(hleaf.data(), leaf, hleaf.size(), hipMemcpyDeviceToHost, s));
    PFS_HIP(ctx, hipStreamSynchronize(s));
    st.n[7] += hleaf.size();
    leaf = hleaf.data();
  }
  std::vector<pfscdc_file_info> infos;
  std::string err;
  if (int rc = source_host(l, a, leaf, &res, &infos, &err, &st.n[3])) return ctx_fail(ctx, rc, err);
  if (int rc = source_upload(ctx, res, infos, out, &st.n[6])) return rc;
  st.n[2] = infos.size();
  st.ms[0] = clk.lap();
  return PFSCDC_OK;
}

int source_open(pfscdc_ctx* ctx, const pfscdc_dev_list& in, int kind, const char* arg,
                const uint8_t* leaf, int leaf_on_device, pfscdc_source** out) {
  *out = nullptr;
  PassStats& st = ctx_source_stats(ctx);
  st = PassStats();
  st.n[1] = in.n;
  if (in.device != ctx_device(ctx))
    return ctx_fail(ctx, PFSCDC_EINVAL, "a resident list of another device");
  SrcArg a;
  std::string err;
  if (int rc = source_arg(kind, arg, &a, &err)) return ctx_fail(ctx, rc, err);
  PFS_HIP(ctx, hipSetDevice(ctx_device(ctx)));
  if (knob(Knob::Source) == 0) return host_arm(ctx, in, a, leaf, leaf_on_device, out);
  // a glob but "/" (all, with PFSCDC_INFO_MATCH on "/" alone) runs as a position automaton
  const bool automaton = kind == PFSCDC_SRC_GLOB && !a.all;
  std::unique_ptr<GlobProgram> prog;
  if (automaton) {
    prog.reset(new GlobProgram());
    glob_compile(a.glob, prog.get());
    // more positions than one uint64_t holds: no device program
    if (prog->positions > 64) return host_arm(ctx, in, a, leaf, leaf_on_device, out);
  }
  hipStream_t s = ctx_stream(ctx);
  const int cus = ctx_num_cus(ctx);
  const RtarList l = view(in);
  Clock clk;
  // ---- insert and select: (the glob masks,) count, prefix sums
  GuardMem d_arg, d_cnt, d_base, d_flags, d_prog, d_masks;
  Guards g;
  PFS_HIP(ctx, d_arg.alloc(a.name.size() + a.dir.size(), s));
  PFS_HIP(ctx, d_cnt.alloc(sizeof(MrgCount) * l.n, s));
  PFS_HIP(ctx, d_base.alloc(sizeof(uint64_t) * 3 * (l.n + 1), s));
  // SrcBad, the deepest depth, the directories inserted
  PFS_HIP(ctx, d_flags.alloc(4 * sizeof(uint32_t), s));
  g.add(d_cnt);
  g.add(d_base);
  g.add(d_flags);
  const std::string both = a.name + a.dir;
  if (!both.empty()) {
    PFS_HIP(ctx, hipMemcpyAsync(d_arg.p, both.data(), both.size(), hipMemcpyHostToDevice, s));
    st.n[6] += both.size();
  }
  PFS_HIP(ctx, hipMemsetAsync(d_flags.p, 0, 4 * sizeof(uint32_t), s));
  if (automaton) {
    PFS_HIP(ctx, d_prog.alloc(sizeof prog->table, s));
    PFS_HIP(ctx, d_masks.alloc(sizeof(uint64_t) * l.n, s));
    g.add(d_masks);
    PFS_HIP(ctx, hipMemcpyAsync(d_prog.p, prog->table, sizeof prog->table, hipMemcpyHostToDevice, s));
    st.n[6] += sizeof prog->table;
    PFS_HIP(ctx, launch_src_glob(l, d_prog.as<uint64_t>(), prog->first, prog->last, prog->nullable,
                                 d_masks.as<uint64_t>(), d_flags.as<uint32_t>(), cus, s));
  }
  const uint32_t glob = automaton ? kSrcGlobMasks : kind == PFSCDC_SRC_GLOB ? kSrcGlobRoot : kSrcGlobNone;
  const SrcPred pr{d_arg.as<char>(), d_arg.as<char>() + a.name.size(), (uint32_t)a.name.size(),
                   (uint32_t)a.dir.size(), a.all, a.exclude_dir, a.child_flag, glob,
                   d_masks.as<uint64_t>()};
  PFS_HIP(ctx, launch_src_count(l, pr, d_cnt.as<MrgCount>(), d_flags.as<uint32_t>(), cus, s));
  PFS_HIP(ctx, launch_merge_scan(d_cnt.as<MrgCount>(), l.n, d_base.as<uint64_t>(), s));
  uint64_t totals[3] = {0, 0, 0};
  uint32_t flags[4] = {0, 0, 0, 0};
  PFS_HIP(ctx, hipMemcpyAsync(totals, d_base.as<uint64_t>() + 3 * l.n, sizeof totals,
                              hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipMemcpyAsync(flags, d_flags.p, sizeof flags, hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.n[7] += sizeof totals + sizeof flags;
  if (flags[0] & kSrcMalformed)
    return ctx_fail(ctx, PFSCDC_EINVAL, "an entry's strings or DataRefs lie outside the list's arrays");
  if (flags[0] & kSrcNotLevel0)
    return ctx_fail(ctx, PFSCDC_EINVAL, "an entry with a Range: not a level-0 list");
  if (flags[0]) {  // out of order, an unclean path, a directory twice: emit() taken literally
    return host_arm(ctx, in, a, leaf, leaf_on_device, out);
  }
  const uint64_t m = totals[0], nr = totals[1];
  if (m > 0xffffffffull) return ctx_fail(ctx, PFSCDC_EUNSUPPORTED, "more than 2^32 - 1 entries");
  if (nr > l.nr) return ctx_fail(ctx, PFSCDC_EHIP, "source: the counts exceed the input");
  if (m == 0 && source_errs_on_empty(a)) return ctx_fail(ctx, PFSCDC_ENOTFOUND, source_not_found(a));
  // ---- fill: entries, strings, DataRefs; per output entry its source, depth, type and size
  OutList o;
  GuardMem d_copy, d_meta, d_infos, d_sizes, d_sbase;
  PFS_HIP(ctx, o.alloc(totals, s, &g));
  PFS_HIP(ctx, copy_plan_alloc(&d_copy, l.n, s, &g));
  PFS_HIP(ctx, d_meta.alloc(sizeof(SrcMeta) * m, s));
  PFS_HIP(ctx, d_infos.alloc(sizeof(pfscdc_file_info) * m, s));
  PFS_HIP(ctx, d_sizes.alloc(sizeof(MrgCount) * m, s));
  PFS_HIP(ctx, d_sbase.alloc(sizeof(uint64_t) * 3 * (m + 1), s));
  for (const GuardMem* x : {&d_meta, &d_infos, &d_sizes, &d_sbase}) g.add(*x);
  PFS_HIP(ctx, launch_src_fill(l, pr, d_cnt.as<MrgCount>(), d_base.as<uint64_t>(),
                               o.entries.as<pfscdc_index_entry>(), o.blob.as<char>(),
                               d_copy.as<MrgCopy>(), d_meta.as<SrcMeta>(),
                               d_infos.as<pfscdc_file_info>(), d_sizes.as<MrgCount>(),
                               d_flags.as<uint32_t>() + 1, o.drs.as<pfscdc_full_dataref>(), cus, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.ms[0] = clk.lap();
  // ---- subtree ends and directory sizes
  const RtarList ol = o.view();
  PFS_HIP(ctx, launch_merge_scan(d_sizes.as<MrgCount>(), m, d_sbase.as<uint64_t>(), s));
  PFS_HIP(ctx, launch_src_tree(ol, d_meta.as<SrcMeta>(), d_sbase.as<uint64_t>(),
                               d_infos.as<pfscdc_file_info>(), cus, s));
  // only the deepest depth comes back, to size the level loop
  PFS_HIP(ctx, hipMemcpyAsync(flags, d_flags.p, sizeof flags, hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, g.fetch(s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.n[7] += sizeof flags + g.host.size();
  if (!g.ok()) return ctx_fail(ctx, PFSCDC_EHIP, "source: a kernel wrote past its array");
  st.ms[1] = clk.lap();
  const uint32_t maxdepth = flags[1];
  st.n[3] = flags[2];
  if (maxdepth > 0xffffu) return ctx_fail(ctx, PFSCDC_EHIP, "source: a depth beyond any path");
  // ---- hashes: the existing hash path over segments of one packed buffer
  GuardMem d_buf, d_segs, d_order, d_qctr, d_offs, d_lcnt, d_lbase;
  Guards gh;
  const uint64_t buf_bytes = 32 * (m > nr ? m : nr);
  PFS_HIP(ctx, d_buf.alloc(buf_bytes, s));
  PFS_HIP(ctx, d_segs.alloc(sizeof(pfscdc_segment) * m, s));
  PFS_HIP(ctx, d_order.alloc(sizeof(uint32_t) * m, s));
  PFS_HIP(ctx, d_qctr.alloc(2 * sizeof(uint32_t), s));
  PFS_HIP(ctx, d_offs.alloc(2 * sizeof(uint64_t), s));  // one "file": the buffer, from 0
  PFS_HIP(ctx, d_lcnt.alloc(sizeof(MrgCount) * m, s));
  PFS_HIP(ctx, d_lbase.alloc(sizeof(uint64_t) * 3 * (m + 1), s));
  for (const GuardMem* x : {&d_buf, &d_segs, &d_order, &d_qctr, &d_offs, &d_lcnt, &d_lbase, &d_infos})
    gh.add(*x);
  const int64_t forced = knob(Knob::HashWaves);
  const int waves = forced >= 1 && forced <= 8 ? (int)forced : 0;
  if (m) {
    const uint64_t offs[2] = {0, buf_bytes};
    PFS_HIP(ctx, hipMemcpyAsync(d_offs.p, offs, sizeof offs, hipMemcpyHostToDevice, s));
    PFS_HIP(ctx, hipMemsetAsync(d_qctr.p, 0, 2 * sizeof(uint32_t), s));
    st.n[6] += sizeof offs;
    GuardMem d_leaf;
    if (leaf) {  // the caller's: MergeFileReader.Hash per file
      if (!leaf_on_device) {
        PFS_HIP(ctx, d_leaf.alloc(32 * l.n, s));
        PFS_HIP(ctx, hipMemcpyAsync(d_leaf.p, leaf, 32 * l.n, hipMemcpyHostToDevice, s));
        st.n[6] += 32 * l.n;
        leaf = d_leaf.as<uint8_t>();
      }
      PFS_HIP(ctx, launch_src_leaf_copy(d_meta.as<SrcMeta>(), leaf, m, d_infos.as<pfscdc_file_info>(),
                                        cus, s));
    } else {  // hashDataRefs: one record per entry (a directory's is empty and overwritten below)
      PFS_HIP(ctx, launch_src_leaf(ol, d_buf.as<uint8_t>(), d_segs.as<pfscdc_segment>(), cus, s));
      // the records' count: the entries emitted, base[3 n] of the first prefix sums
      PFS_HIP(ctx, launch_blake2b(d_buf.as<uint8_t>(), d_offs.as<uint64_t>(), d_segs.as<pfscdc_segment>(),
                                  d_base.as<uint64_t>() + 3 * l.n, m, d_order.as<uint32_t>(),
                                  d_qctr.as<uint32_t>(), cus, buf_bytes, s, false, nullptr, waves));
      st.n[5]++;
      PFS_HIP(ctx, launch_src_scatter(d_meta.as<SrcMeta>(), nullptr, d_segs.as<pfscdc_segment>(), m,
                                      -1, d_infos.as<pfscdc_file_info>(), cus, s));
    }
    PFS_HIP(ctx, hipStreamSynchronize(s));
    st.ms[2] = clk.lap();
    // the directories, deepest first (those of the deepest depth are empty)
    for (uint32_t level = maxdepth + 1; level-- > 0;) {
      PFS_HIP(ctx, launch_src_level_count(d_meta.as<SrcMeta>(), d_infos.as<pfscdc_file_info>(), m,
                                          level, d_lcnt.as<MrgCount>(), cus, s));
      PFS_HIP(ctx, launch_merge_scan(d_lcnt.as<MrgCount>(), m, d_lbase.as<uint64_t>(), s));
      PFS_HIP(ctx, launch_src_level_gather(d_meta.as<SrcMeta>(), d_infos.as<pfscdc_file_info>(),
                                           d_lbase.as<uint64_t>(), m, level, d_buf.as<uint8_t>(),
                                           d_segs.as<pfscdc_segment>(), cus, s));
      PFS_HIP(ctx, launch_blake2b(d_buf.as<uint8_t>(), d_offs.as<uint64_t>(), d_segs.as<pfscdc_segment>(),
                                  d_lbase.as<uint64_t>() + 3 * m + 1, m, d_order.as<uint32_t>(),
                                  d_qctr.as<uint32_t>(), cus, buf_bytes, s, false, nullptr, waves));
      st.n[5]++;
      PFS_HIP(ctx, launch_src_scatter(d_meta.as<SrcMeta>(), d_lbase.as<uint64_t>(),
                                      d_segs.as<pfscdc_segment>(), m, (int)level,
                                      d_infos.as<pfscdc_file_info>(), cus, s));
    }
    st.n[4] = (uint64_t)maxdepth + 1;
  }
  PFS_HIP(ctx, gh.fetch(s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  st.n[7] += gh.host.size();
  if (!gh.ok()) return ctx_fail(ctx, PFSCDC_EHIP, "source: a kernel wrote past its array");
  st.ms[3] = clk.lap();
  st.n[0] = 1;
  st.n[2] = m;
  *out = source_new(ctx, &o, &d_infos);
  return PFSCDC_OK;
}

}  // namespace

extern "C" {

int pfscdc_source_open(pfscdc_ctx* ctx, const pfscdc_dev_list* in, int kind, const char* arg,
                       const uint8_t* leaf_hashes, int leaf_on_device, pfscdc_source** out) {
  if (!ctx || !in || !out) return PFSCDC_EINVAL;
  return source_open(ctx, *in, kind, arg, leaf_hashes, leaf_on_device, out);
}

int pfscdc_source_open_list(pfscdc_ctx* ctx, const pfscdc_index_list* in, int kind,
                            const char* arg, const uint8_t* leaf_hashes, int leaf_on_device,
                            pfscdc_source** out) {
  if (!ctx || !out) return PFSCDC_EINVAL;
  *out = nullptr;
  static const List empty;
  const List& l = in ? *in : empty;
  pfscdc_dev_list* d = nullptr;
  if (int rc = pfscdc::dev_list_upload(ctx, l, &d)) return rc;
  const int rc = source_open(ctx, *d, kind, arg, leaf_hashes, leaf_on_device, out);
  pfscdc::ctx_source_stats(ctx).n[6] += pfscdc::list_bytes(l);
  delete d;
  return rc;
}

pfscdc_dev_list* pfscdc_source_list(pfscdc_source* s) { return s ? s->list : nullptr; }

uint32_t pfscdc_source_count(const pfscdc_source* s) { return s && s->list ? (uint32_t)s->list->n : 0; }

int pfscdc_source_infos(pfscdc_ctx* ctx, const pfscdc_source* s, pfscdc_file_info* out) {
  if (!ctx || !s || !s->list) return PFSCDC_EINVAL;
  if (s->device != pfscdc::ctx_device(ctx))
    return pfscdc::ctx_fail(ctx, PFSCDC_EINVAL, "a source of another device");
  if (!s->list->n) return PFSCDC_OK;
  if (!out) return PFSCDC_EINVAL;
  hipStream_t st = pfscdc::ctx_stream(ctx);
  PFS_HIP(ctx, hipSetDevice(s->device));
  PFS_HIP(ctx, hipMemcpyAsync(out, s->infos, sizeof(pfscdc_file_info) * s->list->n,
                              hipMemcpyDeviceToHost, st));
  PFS_HIP(ctx, hipStreamSynchronize(st));
  return PFSCDC_OK;
}

int pfscdc_source_free(pfscdc_source* s) {
  if (!s) return PFSCDC_OK;
  (void)hipSetDevice(s->device);
  delete s;
  return PFSCDC_OK;
}

int pfscdc_debug_glob_masks(pfscdc_ctx* ctx, const pfscdc_dev_list* list, const char* glob,
                            uint64_t* masks, uint32_t* bad) {
  if (!ctx || !list || !glob || !bad || (list->n && !masks)) return PFSCDC_EINVAL;
  if (list->device != pfscdc::ctx_device(ctx))
    return pfscdc::ctx_fail(ctx, PFSCDC_EINVAL, "a resident list of another device");
  pfscdc::Glob g;
  std::string err;
  if (int rc = pfscdc::glob_parse(pfscdc::clean_path(glob), &g, &err))
    return pfscdc::ctx_fail(ctx, rc, err);
  std::unique_ptr<pfscdc::GlobProgram> prog(new pfscdc::GlobProgram());
  pfscdc::glob_compile(g, prog.get());
  if (prog->positions > 64)
    return pfscdc::ctx_fail(ctx, PFSCDC_EUNSUPPORTED, "a glob of more than 64 positions");
  hipStream_t s = pfscdc::ctx_stream(ctx);
  PFS_HIP(ctx, hipSetDevice(list->device));
  pfscdc::GuardMem d_prog, d_masks, d_bad;
  pfscdc::Guards gd;
  PFS_HIP(ctx, d_prog.alloc(sizeof prog->table, s));
  PFS_HIP(ctx, d_masks.alloc(sizeof(uint64_t) * list->n, s));
  PFS_HIP(ctx, d_bad.alloc(sizeof(uint32_t), s));
  gd.add(d_masks);
  gd.add(d_bad);
  PFS_HIP(ctx, hipMemcpyAsync(d_prog.p, prog->table, sizeof prog->table, hipMemcpyHostToDevice, s));
  PFS_HIP(ctx, hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), s));
  PFS_HIP(ctx, pfscdc::launch_src_glob(pfscdc::view(*list), d_prog.as<uint64_t>(), prog->first,
                                       prog->last, prog->nullable, d_masks.as<uint64_t>(),
                                       d_bad.as<uint32_t>(), pfscdc::ctx_num_cus(ctx), s));
  if (list->n)
    PFS_HIP(ctx, hipMemcpyAsync(masks, d_masks.p, sizeof(uint64_t) * list->n, hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipMemcpyAsync(bad, d_bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, gd.fetch(s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  if (!gd.ok()) return pfscdc::ctx_fail(ctx, PFSCDC_EHIP, "glob: the kernel wrote past its array");
  return PFSCDC_OK;
}

int pfscdc_debug_list_scan(pfscdc_ctx* ctx, int kind, const void* in, uint64_t n, uint64_t* out) {
  static const uint64_t rec[3] = {sizeof(pfscdc::IdxCount), sizeof(pfscdc::MrgCount), 8};
  static const uint64_t cols[3] = {2, 3, 1};
  if (!ctx || kind < 0 || kind > 2 || !out || (n && !in) || n > 0xffffffffull)
    return PFSCDC_EINVAL;
  hipStream_t s = pfscdc::ctx_stream(ctx);
  PFS_HIP(ctx, hipSetDevice(pfscdc::ctx_device(ctx)));
  pfscdc::DevMem d_in, d_out;
  PFS_HIP(ctx, d_in.alloc(rec[kind] * n));
  PFS_HIP(ctx, d_out.alloc(8 * cols[kind] * (n + 1)));
  if (n) PFS_HIP(ctx, hipMemcpyAsync(d_in.p, in, rec[kind] * n, hipMemcpyHostToDevice, s));
  uint64_t* base = d_out.as<uint64_t>();
  PFS_HIP(ctx, kind == 0   ? pfscdc::launch_index_scan(d_in.as<pfscdc::IdxCount>(), n, base, s)
               : kind == 1 ? pfscdc::launch_merge_scan(d_in.as<pfscdc::MrgCount>(), n, base, s)
                           : pfscdc::launch_rtar_scan(d_in.as<uint64_t>(), n, base, nullptr, s));
  PFS_HIP(ctx, hipMemcpyAsync(out, d_out.p, 8 * cols[kind] * (n + 1), hipMemcpyDeviceToHost, s));
  PFS_HIP(ctx, hipStreamSynchronize(s));
  return PFSCDC_OK;
}

int pfscdc_last_source_stats(pfscdc_ctx* ctx, uint64_t out[8]) {
  return pfscdc::last_pass_stats(ctx, pfscdc::ctx_source_stats, out, nullptr);
}

int pfscdc_last_source_timings(pfscdc_ctx* ctx, float out[4]) {
  return pfscdc::last_pass_stats(ctx, pfscdc::ctx_source_stats, nullptr, out);
}

}  // extern "C"
