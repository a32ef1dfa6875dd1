// diff.cpp — DiffFile on the host (pfscdc_diff_host): Differ.Iterate's two-pointer walk taken
// literally.  It is the specification the diff_* kernels (list_kernels.hip §12, driven by
// diff_dev.cpp) are tested against, and the arm for the sides the device refuses.  No GPU call
// and no HIP header in this file: a stand-alone sanitizer build compiles it with
// index_decode.cpp and a plain C++ compiler.
//
// Reference (paths under the reference's src):
//   server/pfs/server/diff.go:26-96            Differ.Iterate, equalFileInfos
//   server/pfs/server/driver_file.go:320-385   diffFile: old = emptySource for a nil commit
#include "diff.h"

#include <cstdlib>
#include <cstring>

using List = pfscdc_index_list;

namespace pfscdc {

namespace {

bool paths_inside(const List& l) {
  const uint64_t nb = l.blob.size();
  for (const pfscdc_index_entry& e : l.entries)
    if (e.path_off > nb || e.path_len > nb - e.path_off) return false;
  return true;
}

}  // namespace

int diff_host(const List& a, const pfscdc_file_info* ai, const List& b, const pfscdc_file_info* bi,
              std::vector<pfscdc_diff_pair>* out) {
  out->clear();
  const size_t na = a.entries.size(), nb = b.entries.size();
  if ((na && !ai) || (nb && !bi) || na >= PFSCDC_DIFF_NONE || nb >= PFSCDC_DIFF_NONE)
    return PFSCDC_EINVAL;
  if (!paths_inside(a) || !paths_inside(b)) return PFSCDC_EINVAL;
  size_t i = 0, j = 0;
  while (i < na && j < nb) {  // for aOpen && bOpen
    const int c = idx_cmp(idx_path(a, a.entries[i]), idx_path(b, b.entries[j]));
    if (c < 0) {
      out->push_back({(uint32_t)i++, PFSCDC_DIFF_NONE});
    } else if (c > 0) {
      out->push_back({PFSCDC_DIFF_NONE, (uint32_t)j++});
    } else {
      if (std::memcmp(ai[i].hash, bi[j].hash, 32) != 0)  // !equalFileInfos
        out->push_back({(uint32_t)i, (uint32_t)j});
      i++;
      j++;
    }
  }
  for (; i < na; i++) out->push_back({(uint32_t)i, PFSCDC_DIFF_NONE});
  for (; j < nb; j++) out->push_back({PFSCDC_DIFF_NONE, (uint32_t)j});
  return PFSCDC_OK;
}

void diff_select(const List& l, const pfscdc_file_info* infos,
                 const std::vector<pfscdc_diff_pair>& pairs, int member, List* out,
                 std::vector<pfscdc_file_info>* out_infos) {
  out->entries.clear();
  out->drs.clear();
  out->blob.clear();
  out->tar.clear();
  out_infos->clear();
  for (const pfscdc_diff_pair& p : pairs) {
    const uint32_t x = member ? p.b : p.a;
    if (x == PFSCDC_DIFF_NONE) continue;
    idx_append_entry(out, l, l.entries[x]);
    out_infos->push_back(infos[x]);
  }
}

}  // namespace pfscdc

extern "C" {

int pfscdc_diff_host(const pfscdc_index_list* a, const pfscdc_file_info* a_infos,
                     const pfscdc_index_list* b, const pfscdc_file_info* b_infos,
                     pfscdc_diff_pair** out, uint64_t* n) {
  if (!out || !n) return PFSCDC_EINVAL;
  *out = nullptr;
  *n = 0;
  static const List empty;
  std::vector<pfscdc_diff_pair> v;
  if (int rc = pfscdc::diff_host(a ? *a : empty, a_infos, b ? *b : empty, b_infos, &v)) return rc;
  pfscdc_diff_pair* p = (pfscdc_diff_pair*)std::malloc(sizeof(pfscdc_diff_pair) * (v.size() + 1));
  if (!p) return PFSCDC_ENOMEM;
  if (!v.empty()) std::memcpy(p, v.data(), sizeof(pfscdc_diff_pair) * v.size());
  *out = p;
  *n = v.size();
  return PFSCDC_OK;
}

void pfscdc_diff_pairs_free(pfscdc_diff_pair* pairs) { std::free(pairs); }

}  // extern "C"
