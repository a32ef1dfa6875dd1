// index_list.h — the owned index list and the host-only pieces of the index reader (no HIP
// header: a stand-alone sanitizer build compiles index_decode.cpp with a plain C++ compiler).
#pragma once
#include <stdint.h>

#include <cstddef>
#include <string>
#include <vector>

#define PFSCDC_HD  // host only here
#include "index_parse.h"

struct pfscdc_index_list {
  std::vector<pfscdc_index_entry> entries;
  std::vector<pfscdc_full_dataref> drs;
  std::vector<char> blob;
  std::vector<pfscdc_tar_file> tar;  // built by pfscdc_index_list_tar_files
};

namespace pfscdc {

constexpr uint64_t kIdxNone = ~0ull;

// the frame's records appended to l (fr parsed from [p, end) before); false: 2^32 records
bool idx_append_frame(pfscdc_index_list* l, const IdxFrame& fr, const uint8_t* p,
                      const uint8_t* end);
// the frames of p[0, n) that begin below limit: PFSCDC_OK, or PFSCDC_ECORRUPT with *err = the
// start of the first frame that does not parse.  open_end: p[0, n) ends before its level does
// (a filtered selection), and a frame that runs past n ends the stream in front of it.
int idx_decode_stream(const uint8_t* p, uint64_t n, uint64_t limit, bool open_end,
                      pfscdc_index_list* l, uint64_t* err);

struct IdxStr {
  const char* p;
  size_t n;
};
IdxStr idx_path(const pfscdc_index_list& l, const pfscdc_index_entry& e);
IdxStr idx_tag(const pfscdc_index_list& l, const pfscdc_index_entry& e);
IdxStr idx_last_path(const pfscdc_index_list& l, const pfscdc_index_entry& e);
int idx_cmp(IdxStr a, IdxStr b);  // strings.Compare: bytewise

struct IdxFilter {  // reader.go:23-26 pathFilter + Reader.tag
  std::string lower, upper, prefix, tag;
  explicit IdxFilter(const pfscdc_index_filter* f);
  bool at_start(IdxStr name) const;  // reader.go:95-103
  bool at_end(IdxStr name) const;    // reader.go:108-122
  bool tag_ok(IdxStr t) const;
};

// entry e of src appended to dst: strings, File DataRefs and the Range's chunk_ref
void idx_append_entry(pfscdc_index_list* dst, const pfscdc_index_list& src,
                      const pfscdc_index_entry& e);

}  // namespace pfscdc
