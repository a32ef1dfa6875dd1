// tar.h — what the host side of GetFileTAR (tar.cpp) shares with its kernels (tar_frame_kernel in
// cdc_kernels.hip, the resident plan in list_kernels.hip §10): the entry record, the plan of one
// window, and the lengths of a PAX entry's head.  No HIP in this file, so tar.cpp builds with a
// plain C++ compiler for a sanitizer run; the functions the kernels call are constexpr.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pfscdc.h"

namespace pfscdc {

// One tar entry as tar_frame_kernel takes it: where its head begins in the stream, the size
// field, and its name in the packed name table.  split: index of the '/' that splitUSTARPath
// cuts at, -1 for none; kTarPaxPath / kTarPaxSize for a PAX entry with / without a path record
// (a size record goes with either where size > kTarMaxSize).
struct TarEntry {
  uint64_t off;   // stream offset of the head's first block
  uint64_t size;  // content bytes (the padding follows them up to the next multiple of 512)
  uint32_t name_off;
  uint16_t name_len;
  int16_t split;
};
static_assert(sizeof(TarEntry) == 24, "tar entry record layout");
constexpr uint64_t kTarMaxSize = 077777777777ull;  // 11 octal digits: above it Go writes PAX
constexpr int kTarPaxPath = -2, kTarPaxSize = -3;   // TarEntry::split of a PAX entry
constexpr uint32_t kTarMaxName = 65535;             // TarEntry::name_len is 16 bits

constexpr uint32_t tar_digits(uint64_t v) {  // decimal digits of v
  uint32_t d = 1;
  for (; v >= 10; v /= 10) d++;
  return d;
}
// formatPAXRecord's length of "<n> <key>=<value>\n": n counts its own digits
constexpr uint32_t tar_pax_record_len(uint32_t key_len, uint32_t value_len) {
  const uint32_t base = key_len + value_len + 3;
  const uint32_t n = base + tar_digits(base);
  return base + tar_digits(n);
}
// bytes of a PAX entry's records: "path" (split == kTarPaxPath), then "size" (size > kTarMaxSize)
constexpr uint32_t tar_pax_records_len(uint32_t name_len, uint64_t size, int split) {
  return (split == kTarPaxPath ? tar_pax_record_len(4, name_len) : 0u) +
         (size > kTarMaxSize ? tar_pax_record_len(4, tar_digits(size)) : 0u);
}
// every byte in front of an entry's content: 512 for USTAR; for PAX the extended header block,
// the records up to a multiple of 512, the main header block
constexpr uint64_t tar_head_len(uint32_t name_len, uint64_t size, int split) {
  return split >= -1 ? 512u
                     : 1024u + ((tar_pax_records_len(name_len, size, split) + 511u) & ~511u);
}

// IsClean's component rule for s[from, n): no empty component, none of "." or ".."; with
// allow_trailing_slash the last component may be empty.  The one test the list passes
// (path_is_clean, list_kernels.hip) and the PAX name rule share.
constexpr bool path_components_clean(const uint8_t* s, uint32_t n, uint32_t from,
                                     bool allow_trailing_slash) {
  bool clean = true;
  for (uint32_t k = from, start = from; clean && k <= n; k++) {
    if (k < n && s[k] != '/') continue;
    const uint32_t cl = k - start;
    if (cl == 0) clean = allow_trailing_slash && k == n;
    else if (cl == 1) clean = s[start] != '.';
    else if (cl == 2) clean = s[start] != '.' || s[start + 1] != '.';
    start = k + 1;
  }
  return clean;
}
// A PAX entry's extended header is named path.Join(dir, "PaxHeaders.0", file), which cleans its
// result; the library writes dir + "PaxHeaders.0" [+ "/" + file], the same bytes exactly for a
// name (n > 0) with no empty, "." or ".." component, a leading '/' and a directory's trailing '/'
// aside.  Any other PAX name is refused.
constexpr bool tar_name_joins(const uint8_t* s, uint32_t n) {
  return path_components_clean(s, n, s[0] == '/' ? 1u : 0u, true);
}

// Why a name or size has no header (nullptr: it has one); *split as TarEntry::split.  *rc:
// PFSCDC_EUNSUPPORTED where Go would write PAX records and format has no PFSCDC_TAR_PAX, for a
// PAX name that path.Join would rewrite (an empty, "." or ".." component) and for a PAX name above
// kTarMaxName bytes; PFSCDC_EINVAL for an empty name or a directory (name ending in '/') with
// content.
const char* tar_name_check(const char* name, size_t len, uint64_t size, int format, int* split,
                           int* rc);
// One window [begin, end) of the stream of getFileTar over files whose pieces are
// [first, first + count) of an array of npieces pieces (slices or DataRefs) of piece_sizes
// bytes: the entries that meet the window, their names, and the pieces' bytes inside it.
struct TarPiece {
  uint32_t src;      // index of the piece in the caller's array
  uint64_t skip;     // bytes of the piece in front of the window
  uint64_t size;     // bytes of it inside the window (> 0)
  uint64_t out_off;  // where they go, relative to begin
};
struct TarPlan {
  uint64_t total = 0, begin = 0, end = 0;
  std::vector<TarEntry> entries;
  std::string names;
  // xblk[i] = head blocks other than the main header in entries[0, i) (entries.size() + 1
  // values; empty where no entry of the window is PAX)
  std::vector<uint64_t> xblk;
  std::vector<TarPiece> pieces;
  std::string err;
};
// PFSCDC_EINVAL / PFSCDC_EUNSUPPORTED with plan->err set; no GPU call
int tar_plan(const pfscdc_tar_file* files, uint32_t nfiles, const uint64_t* piece_sizes,
             uint32_t npieces, uint64_t begin, uint64_t len, int format, TarPlan* plan);

}  // namespace pfscdc
