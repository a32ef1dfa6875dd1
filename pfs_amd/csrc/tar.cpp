// tar.cpp — host side of GetFileTAR: the USTAR header as Go's archive/tar writes it for
// Header{Name, Size} (tarutil.NewHeader, tarutil/tar.go:35-40), the stream layout of getFileTar
// (api_server.go:578-593, fileset.WriteTarEntry util.go:42-53), and the clipping of a file
// list's pieces to one window of that stream.  No GPU call in this file: pfscdc_tar_header is
// the specification tar_frame_kernel is tested against.
#include <algorithm>
#include <cstring>

#include "pfscdc_internal.h"

namespace pfscdc {

const char* tar_name_check(const char* name, size_t len, uint64_t size, int* split, int* rc) {
  *split = -1;
  *rc = PFSCDC_EINVAL;
  if (len == 0) return "empty name";
  if (name[len - 1] == '/' && size) return "a directory entry with content";
  *rc = PFSCDC_EUNSUPPORTED;
  for (size_t i = 0; i < len; i++)
    if ((uint8_t)name[i] >= 0x80) return "a name that is not ASCII needs a PAX header";
  if (size > kTarMaxSize) return "a size above 8 GiB - 1 needs a PAX header";
  if (len > 100) {  // splitUSTARPath
    size_t l = std::min<size_t>(len, 156);
    if (len <= 156 && name[len - 1] == '/') l = len - 1;
    size_t i = l;
    while (i > 0 && name[i - 1] != '/') i--;
    // the last '/' of name[:l] is name[i - 1]; none, or only name[0]: no split
    if (i < 2 || len - i > 100 || len - i == 0 || i - 1 > 155)
      return "a name longer than 100 bytes that does not split needs a PAX header";
    *split = (int)(i - 1);
  }
  *rc = PFSCDC_OK;
  return nullptr;
}

static void octal(uint8_t* at, int digits, uint64_t v) {  // digits octal digits, then NUL
  for (int k = digits - 1; k >= 0; k--, v >>= 3) at[k] = (uint8_t)('0' + (v & 7));
  at[digits] = 0;
}

int tar_plan(const pfscdc_tar_file* files, uint32_t nfiles, const uint64_t* piece_sizes,
             uint32_t npieces, uint64_t begin, uint64_t len, TarPlan* plan) {
  auto bad = [&](int rc, const std::string& msg) {
    plan->err = msg;
    return rc;
  };
  if ((nfiles && !files) || (npieces && !piece_sizes)) return bad(PFSCDC_EINVAL, "NULL argument");
  std::vector<uint64_t> off(nfiles + 1), size(nfiles);
  std::vector<int> split(nfiles);
  uint64_t at = 0;
  for (uint32_t i = 0; i < nfiles; i++) {
    const pfscdc_tar_file& f = files[i];
    if (!f.path) return bad(PFSCDC_EINVAL, "NULL path");
    if (f.first > npieces || f.count > npieces - f.first)
      return bad(PFSCDC_EINVAL, std::string(f.path) + ": pieces beyond the array");
    uint64_t z = 0;
    for (uint32_t k = f.first; k < f.first + f.count; k++) {
      if (z + piece_sizes[k] < z) return bad(PFSCDC_EINVAL, "sizes overflow");
      z += piece_sizes[k];
    }
    const size_t nl = std::strlen(f.path);
    int rc;
    const char* why = tar_name_check(f.path, nl, z, &split[i], &rc);
    if (!why && nl && f.path[nl - 1] == '/' && f.count) {
      why = "a directory entry with pieces";
      rc = PFSCDC_EINVAL;
    }
    if (why) return bad(rc, "tar entry " + std::string(f.path) + ": " + why);
    off[i] = at;
    size[i] = z;
    at += 512 + ((z + 511) & ~511ull);
    if (at > (1ull << 62)) return bad(PFSCDC_EINVAL, "sizes overflow");
  }
  off[nfiles] = at;
  plan->total = at + 1024;
  if (begin % 512) return bad(PFSCDC_EINVAL, "begin must be a multiple of 512");
  if (begin > plan->total) return bad(PFSCDC_EINVAL, "begin beyond the stream");
  const uint64_t end = len < plan->total - begin ? begin + len : plan->total;
  if (end < plan->total && len % 512)
    return bad(PFSCDC_EINVAL, "len must be a multiple of 512 unless the window reaches the end");
  plan->begin = begin;
  plan->end = end;
  if (end == begin) return PFSCDC_OK;
  // the first entry that ends after begin; entries from there on until one starts at or after end
  uint32_t i = (uint32_t)(std::upper_bound(off.begin(), off.end(), begin) - off.begin());
  i = i ? i - 1 : 0;
  for (; i < nfiles && off[i] < end; i++) {
    const pfscdc_tar_file& f = files[i];
    const size_t nl = std::strlen(f.path);
    plan->entries.push_back(TarEntry{off[i], size[i], (uint32_t)plan->names.size(), (uint16_t)nl,
                                     (int16_t)split[i]});
    plan->names.append(f.path, nl);
    uint64_t p = off[i] + 512;  // stream offset of the piece's first byte
    for (uint32_t k = f.first; k < f.first + f.count; p += piece_sizes[k], k++) {
      const uint64_t lo = std::max(p, begin), hi = std::min(p + piece_sizes[k], end);
      if (lo < hi) plan->pieces.push_back(TarPiece{k, lo - p, hi - lo, lo - begin});
    }
  }
  return PFSCDC_OK;
}

}  // namespace pfscdc

extern "C" {

int pfscdc_tar_header(const char* path, uint64_t size, uint8_t out[512]) {
  if (!path || !out) return PFSCDC_EINVAL;
  const size_t len = std::strlen(path);
  int split, rc;
  if (pfscdc::tar_name_check(path, len, size, &split, &rc)) return rc;
  std::memset(out, 0, 512);
  if (split >= 0) {
    std::memcpy(out + 345, path, (size_t)split);
    std::memcpy(out, path + split + 1, len - (size_t)split - 1);
  } else {
    std::memcpy(out, path, len);
  }
  pfscdc::octal(out + 100, 7, 0);  // mode, uid, gid
  pfscdc::octal(out + 108, 7, 0);
  pfscdc::octal(out + 116, 7, 0);
  pfscdc::octal(out + 124, 11, size);
  pfscdc::octal(out + 136, 11, 0);  // a zero ModTime is written as Unix 0
  out[156] = path[len - 1] == '/' ? '5' : '0';
  std::memcpy(out + 257, "ustar\0" "00", 8);
  pfscdc::octal(out + 329, 7, 0);  // devmajor, devminor
  pfscdc::octal(out + 337, 7, 0);
  std::memset(out + 148, ' ', 8);
  uint32_t sum = 0;
  for (int i = 0; i < 512; i++) sum += out[i];
  pfscdc::octal(out + 148, 6, sum);
  return PFSCDC_OK;
}

int pfscdc_tar_layout(const pfscdc_tar_file* files, uint32_t nfiles, const uint64_t* sizes,
                      uint64_t* entry_offsets, uint64_t* total) {
  if (!total || (nfiles && (!files || !sizes))) return PFSCDC_EINVAL;
  uint64_t at = 0;
  for (uint32_t i = 0; i < nfiles; i++) {
    if (!files[i].path) return PFSCDC_EINVAL;
    const size_t nl = std::strlen(files[i].path);
    int split, rc;
    if (pfscdc::tar_name_check(files[i].path, nl, sizes[i], &split, &rc)) return rc;
    if (files[i].path[nl - 1] == '/' && files[i].count) return PFSCDC_EINVAL;
    if (entry_offsets) entry_offsets[i] = at;
    at += 512 + ((sizes[i] + 511) & ~511ull);
    if (at > (1ull << 62)) return PFSCDC_EINVAL;
  }
  if (entry_offsets) entry_offsets[nfiles] = at;
  *total = at + 1024;
  return PFSCDC_OK;
}

}  // extern "C"
