// dev_pass.h — what the drivers of the index list passes share (index.cpp, resident.cpp,
// source_dev.cpp, diff_dev.cpp, copy_map_dev.cpp): the lap clock, the views
// and byte sizes of a list, the scratch and the guarded device arrays, the output list of a pass,
// the upload of a host-made Source and the body of the pfscdc_last_*_stats calls.  It needs HIP:
// the host arms (source.cpp, diff.cpp, copy_map.cpp, index_decode.cpp, index_merge.cpp) stay
// free of it.
#pragma once
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "dev_list.h"
#include "index_list.h"
#include "list_kernels.h"

namespace pfscdc {

struct Clock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  float lap() {  // ms since the last lap
    const auto t1 = std::chrono::steady_clock::now();
    const float ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
    t0 = t1;
    return ms;
  }
};

inline RtarList view(const pfscdc_dev_list& d) {
  return RtarList{(const pfscdc_index_entry*)d.entries, (const char*)d.blob,
                  (const pfscdc_full_dataref*)d.drs, d.n, d.nr, d.nb};
}

// the bytes of a list's three arrays
inline uint64_t list_bytes(uint64_t n, uint64_t nr, uint64_t nb) {
  return sizeof(pfscdc_index_entry) * n + sizeof(pfscdc_full_dataref) * nr + nb;
}
inline uint64_t list_bytes(const pfscdc_dev_list& d) { return list_bytes(d.n, d.nr, d.nb); }
inline uint64_t list_bytes(const pfscdc_index_list& l) {
  return list_bytes(l.entries.size(), l.drs.size(), l.blob.size());
}

struct DevMem {  // hipMalloc'ed for the call, unguarded: a pass's scratch
  void* p = nullptr;
  ~DevMem() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(uint64_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
  template <class T>
  T* as() const { return (T*)p; }
};

constexpr uint64_t kGuard = 64;

// A device array a planning kernel fills, 64 bytes longer than the kernel may write; the guard
// is preset to 0xA5 and read back by Guards::fetch.
struct GuardMem {
  void* p = nullptr;
  uint64_t bytes = 0;
  ~GuardMem() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(uint64_t n, hipStream_t s) {
    bytes = n;
    hipError_t e = hipMalloc(&p, n + kGuard);
    if (e != hipSuccess) return e;
    return hipMemsetAsync((char*)p + n, 0xA5, kGuard, s);
  }
  void* release() {
    void* r = p;
    p = nullptr;
    return r;
  }
  template <class T>
  T* as() const { return (T*)p; }
};

struct Guards {
  std::vector<const GuardMem*> mems;
  std::vector<uint8_t> host;
  void add(const GuardMem& m) { mems.push_back(&m); }
  // enqueue the guards' copies; after the stream is synchronised ok() tells whether all stand
  hipError_t fetch(hipStream_t s) {
    host.assign(mems.size() * kGuard, 0);
    for (size_t i = 0; i < mems.size(); i++) {
      hipError_t e = hipMemcpyAsync(host.data() + i * kGuard, (const char*)mems[i]->p + mems[i]->bytes,
                                    kGuard, hipMemcpyDeviceToHost, s);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  bool ok() const {
    for (uint8_t b : host)
      if (b != 0xA5) return false;
    return true;
  }
};

// The list a pass writes: the arrays its fill kernel and launch_list_copy fill at the ranges the
// prefix sums gave (list_kernels.h, "the list passes").
struct OutList {
  GuardMem entries, blob, drs;
  uint64_t m = 0, nr = 0, nb = 0;  // entries, DataRefs, blob bytes: the prefix sums' totals
  // the three arrays under g's guards
  hipError_t alloc(const uint64_t totals[3], hipStream_t s, Guards* g);
  RtarList view() const {
    return RtarList{entries.as<pfscdc_index_entry>(), blob.as<char>(),
                    drs.as<pfscdc_full_dataref>(), m, nr, nb};
  }
  // the three arrays become keep's, or those of a new handle on ctx's device
  pfscdc_dev_list* release(pfscdc_ctx* ctx, pfscdc_dev_list* keep = nullptr);
};

// The copy plan between a fill kernel and launch_list_copy, one MrgCopy per input entry, zeroed,
// under g's guards.  (merge_device keeps its own as scratch: guarded, the 64 bytes past a whole
// number of MiB made its call measurably slower.)
inline hipError_t copy_plan_alloc(GuardMem* copy, uint64_t n_in, hipStream_t s, Guards* g) {
  if (hipError_t e = copy->alloc(sizeof(MrgCopy) * n_in, s)) return e;
  g->add(*copy);
  return n_in ? hipMemsetAsync(copy->p, 0, sizeof(MrgCopy) * n_in, s) : hipSuccess;
}

// o's list and the infos a pass wrote beside it (one per entry) as a Source on ctx's device
pfscdc_source* source_new(pfscdc_ctx* ctx, OutList* o, GuardMem* infos);
// A list made on the host and one info per entry of it as a Source on ctx's device; *bytes += what
// went up.
int source_upload(pfscdc_ctx* ctx, const pfscdc_index_list& l,
                  const std::vector<pfscdc_file_info>& infos, pfscdc_source** out, uint64_t* bytes);

// the body of a pfscdc_last_*_stats (ms == nullptr) or pfscdc_last_*_timings (n == nullptr)
inline int last_pass_stats(pfscdc_ctx* ctx, PassStats& (*of)(pfscdc_ctx*), uint64_t* n, float* ms) {
  if (!ctx || (!n && !ms)) return PFSCDC_EINVAL;
  if (n) std::memcpy(n, of(ctx).n, sizeof(uint64_t) * 8);
  if (ms) std::memcpy(ms, of(ctx).ms, sizeof(float) * 4);
  return PFSCDC_OK;
}

}  // namespace pfscdc
