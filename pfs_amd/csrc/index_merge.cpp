// index_merge.cpp — the host-only pieces of compaction: MergeReader.iterateDeletive
// (pfscdc_index_merge_deletive, the specification the merge kernels' deletive mode is tested
// against) and shard (pfscdc_shard).  No GPU call and no HIP header in this file: a stand-alone
// sanitizer build compiles it with index_decode.cpp and a plain C++ compiler.
//
// Reference (paths under the reference's src/internal):
//   storage/fileset/merge.go:79-94,157-164   MergeReader.iterateDeletive, compare
//   stream/priority_queue.go:103-127         groups of equal streams, sorted by priority
//   storage/fileset/shard.go:27-49           shard
#include <memory>
#include <string>
#include <vector>

#include "index_list.h"

using List = pfscdc_index_list;
using namespace pfscdc;

extern "C" {

int pfscdc_index_merge_deletive(const pfscdc_index_list* const* lists, uint32_t nfilesets,
                                pfscdc_index_list** out) {
  if (!out || (nfilesets && !lists) || nfilesets > (1u << 30)) return PFSCDC_EINVAL;
  *out = nullptr;
  std::vector<size_t> pos(nfilesets, 0);
  std::unique_ptr<List> l(new List());
  auto head = [&](uint32_t k) -> const pfscdc_index_entry* {
    return lists[k] && pos[k] < lists[k]->entries.size() ? &lists[k]->entries[pos[k]] : nullptr;
  };
  auto compare = [&](uint32_t a, uint32_t b) {  // merge.go:157-164
    const int c = idx_cmp(idx_path(*lists[a], *head(a)), idx_path(*lists[b], *head(b)));
    return c ? c : idx_cmp(idx_tag(*lists[a], *head(a)), idx_tag(*lists[b], *head(b)));
  };
  std::vector<uint32_t> group;
  for (;;) {
    // the streams whose heads are the least (path, tag), in priority (stream) order
    group.clear();
    for (uint32_t k = 0; k < nfilesets; k++) {
      if (!head(k)) continue;
      const int c = group.empty() ? -1 : compare(k, group[0]);
      if (c < 0) group.assign(1, k);
      else if (c == 0) group.push_back(k);
    }
    if (group.empty()) break;
    const uint32_t k0 = group[0];
    const pfscdc_index_entry& e = *head(k0);  // fss[0].file.Index(), as it is
    const uint64_t recs = (uint64_t)e.count + ((e.flags & PFSCDC_IDX_HAS_CHUNK_REF) ? 1u : 0u);
    if (l->drs.size() + recs > 0xffffffffull || l->entries.size() >= 0xffffffffull)
      return PFSCDC_EUNSUPPORTED;
    idx_append_entry(l.get(), *lists[k0], e);
    for (uint32_t k : group) pos[k]++;
  }
  *out = l.release();
  return PFSCDC_OK;
}

int pfscdc_shard(const pfscdc_index_list* files, int64_t threshold, pfscdc_shard_cb cb,
                 void* user) {
  if (!cb) return PFSCDC_EINVAL;
  int64_t size = 0;
  std::string lower, upper;  // pathRange := &index.PathRange{}
  if (files)
    for (const pfscdc_index_entry& e : files->entries) {
      const IdxStr p = idx_path(*files, e);
      if (size >= threshold) {
        if (cb(user, lower.c_str(), upper.c_str()) != 0) return PFSCDC_ECALLBACK;
        lower.assign(p.p, p.n);
        size = 0;
      }
      upper.assign(p.p, p.n);
      size = (int64_t)((uint64_t)size + (uint64_t)e.size_bytes);
    }
  return cb(user, lower.c_str(), "") != 0 ? PFSCDC_ECALLBACK : PFSCDC_OK;
}

}  // extern "C"
