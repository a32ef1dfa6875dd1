// dev_list.h — the device-resident index list: the three arrays of a pfscdc_index_list as the
// decode and merge kernels write them, kept on the ctx's device, with the tar plan
// (resident.cpp) cached beside them.
#pragma once
#include <string>
#include <vector>

#include "pfscdc_internal.h"

struct pfscdc_dev_list {
  int device = 0;
  void *entries = nullptr, *blob = nullptr, *drs = nullptr;  // hipMalloc'ed, owned
  uint64_t n = 0, nr = 0, nb = 0;                            // entries, DataRefs, blob bytes
  // the plan stage of pfscdc_dev_list_read_tar, made once per tar format (plan_format: the one
  // it holds)
  bool planned = false;
  int plan_format = 0;
  int plan_rc = 0;
  std::string plan_err;
  uint64_t total = 0;
  void *dpre = nullptr, *ent = nullptr, *off = nullptr;  // nr + 1 sums, n TarEntry, n + 1 offsets
  void* xblk = nullptr;  // n + 1 running counts of PAX head blocks; nullptr where there is none
  ~pfscdc_dev_list();
};

// A Source on the device (source_dev.cpp; a diff's selections, diff_dev.cpp): the list and one
// pfscdc_file_info per entry of it.
struct pfscdc_source {
  int device = 0;
  pfscdc_dev_list* list = nullptr;
  void* infos = nullptr;  // pfscdc_file_info per entry of list, on the device
  ~pfscdc_source() {
    if (infos) (void)hipFree(infos);
    delete list;
  }
};

namespace pfscdc {

// what pfscdc_last_resident_stats reports
struct ResidentStats {
  uint64_t n[8] = {};
};
ResidentStats& ctx_resident_stats(pfscdc_ctx* ctx);

// A handle on ctx's device with no arrays yet (an empty list; arrays of a count of 0 may stay
// NULL).
pfscdc_dev_list* dev_list_new(pfscdc_ctx* ctx);
// pfscdc_dev_list_upload / _download over the internal list type (synchronous on the ctx stream)
int dev_list_upload(pfscdc_ctx* ctx, const pfscdc_index_list& l, pfscdc_dev_list** out);
int dev_list_download(pfscdc_ctx* ctx, const pfscdc_dev_list& d, pfscdc_index_list* out);

}  // namespace pfscdc
