// tar.cpp — host side of GetFileTAR: the USTAR header as Go's archive/tar writes it for
// Header{Name, Size} (tarutil.NewHeader, tarutil/tar.go:35-40), the PAX head it switches to for
// one entry whose name or size USTAR cannot hold (archive/tar's writer.go writePAXHeader,
// strconv.go formatPAXRecord; restated in DESIGN §4), the stream layout of getFileTar
// (api_server.go:578-593, fileset.WriteTarEntry util.go:42-53), and the clipping of a file
// list's pieces to one window of that stream.  No GPU call in this file, and no HIP header, so it
// builds alone under a sanitizer: pfscdc_tar_header and pfscdc_tar_head are the specification
// tar_frame_kernel is tested against.
#include <algorithm>
#include <cstring>

#include "tar.h"

namespace pfscdc {

const char* tar_name_check(const char* name, size_t len, uint64_t size, int format, int* split,
                           int* rc) {
  *split = -1;
  *rc = PFSCDC_EINVAL;
  if (len == 0) return "empty name";
  if (name[len - 1] == '/' && size) return "a directory entry with content";
  *rc = PFSCDC_EUNSUPPORTED;
  const char* why = nullptr;
  bool ascii = true;
  for (size_t i = 0; i < len && ascii; i++) ascii = (uint8_t)name[i] < 0x80;
  if (!ascii) {
    why = "a name that is not ASCII needs a PAX header";
  } else if (size > kTarMaxSize) {
    why = "a size above 8 GiB - 1 needs a PAX header";
  } else if (len > 100) {  // splitUSTARPath
    size_t l = std::min<size_t>(len, 156);
    if (len <= 156 && name[len - 1] == '/') l = len - 1;
    size_t i = l;
    while (i > 0 && name[i - 1] != '/') i--;
    // the last '/' of name[:l] is name[i - 1]; none, or only name[0]: no split
    if (i < 2 || len - i > 100 || len - i == 0 || i - 1 > 155)
      why = "a name longer than 100 bytes that does not split needs a PAX header";
    else
      *split = (int)(i - 1);
  }
  if (why && (format & PFSCDC_TAR_PAX)) {
    if (len > kTarMaxName) return "a PAX entry's name longer than 65,535 bytes";
    if (!tar_name_joins((const uint8_t*)name, (uint32_t)len))
      return "a PAX entry's name that is not clean (an empty, \".\" or \"..\" component)";
    *split = !ascii || len > 100 ? kTarPaxPath : kTarPaxSize;
    why = nullptr;
  }
  if (!why) *rc = PFSCDC_OK;
  return why;
}

static void octal(uint8_t* at, int digits, uint64_t v) {  // digits octal digits, then NUL
  for (int k = digits - 1; k >= 0; k--, v >>= 3) at[k] = (uint8_t)('0' + (v & 7));
  at[digits] = 0;
}

// the fields every header block has, and the checksum last
static void finish_block(uint8_t* out, uint64_t size, char type, bool devs) {
  octal(out + 100, 7, 0);  // mode, uid, gid
  octal(out + 108, 7, 0);
  octal(out + 116, 7, 0);
  octal(out + 124, 11, size);
  octal(out + 136, 11, 0);  // a zero ModTime is written as Unix 0
  out[156] = (uint8_t)type;
  std::memcpy(out + 257, "ustar\0" "00", 8);
  if (devs) {  // devmajor, devminor: the extended header block leaves them zero bytes
    octal(out + 329, 7, 0);
    octal(out + 337, 7, 0);
  }
  std::memset(out + 148, ' ', 8);
  uint32_t sum = 0;
  for (int i = 0; i < 512; i++) sum += out[i];
  octal(out + 148, 6, sum);
}

static void ustar_header(const char* path, size_t len, uint64_t size, int split, uint8_t* out) {
  std::memset(out, 0, 512);
  if (split >= 0) {
    std::memcpy(out + 345, path, (size_t)split);
    std::memcpy(out, path + split + 1, len - (size_t)split - 1);
  } else {
    std::memcpy(out, path, len);
  }
  finish_block(out, size, path[len - 1] == '/' ? '5' : '0', true);
}

static std::string to_ascii(const std::string& s) {  // toASCII: no byte >= 0x80, no NUL
  std::string out;
  for (char ch : s)
    if ((uint8_t)ch < 0x80 && ch) out.push_back(ch);
  return out;
}

static std::string pax_record(const std::string& key, const std::string& value) {
  const std::string rest = " " + key + "=" + value + "\n";
  return std::to_string(tar_pax_record_len((uint32_t)key.size(), (uint32_t)value.size())) + rest;
}

// The head of a PAX entry (split: kTarPaxPath or kTarPaxSize): tar_head_len bytes at out.
static void pax_head(const char* path, size_t len, uint64_t size, int split, uint8_t* out) {
  const std::string name(path, len);
  std::string recs;
  if (split == kTarPaxPath) recs += pax_record("path", name);
  if (size > kTarMaxSize) recs += pax_record("size", std::to_string(size));
  const size_t padded = (recs.size() + 511) & ~(size_t)511;
  std::memset(out, 0, 1024 + padded);
  // the extended header block: dir + "PaxHeaders.0" [+ "/" + file] for path.Join (tar_name_joins)
  size_t d = len;
  while (d > 0 && path[d - 1] != '/') d--;
  std::string xname = name.substr(0, d) + "PaxHeaders.0";
  if (d < len) xname += "/" + name.substr(d);
  xname = to_ascii(xname).substr(0, 100);
  while (!xname.empty() && xname.back() == '/') xname.pop_back();
  std::memcpy(out, xname.data(), xname.size());
  finish_block(out, recs.size(), 'x', false);
  std::memcpy(out + 512, recs.data(), recs.size());
  // the main header block: no prefix, the name without its non-ASCII bytes, cut at 100
  uint8_t* m = out + 512 + padded;
  const std::string a = to_ascii(name);
  std::memcpy(m, a.data(), std::min<size_t>(a.size(), 100));
  if (a.size() > 100 && a[99] == '/') {  // formatString: a cut that ends in '/' loses one
    size_t n = 100;
    while (n > 0 && a[n - 1] == '/') n--;
    m[n] = 0;
  }
  finish_block(m, size > kTarMaxSize ? 0 : size, path[len - 1] == '/' ? '5' : '0', true);
}

static bool format_ok(int format) {
  return format == PFSCDC_TAR_USTAR || format == (PFSCDC_TAR_USTAR | PFSCDC_TAR_PAX);
}

int tar_plan(const pfscdc_tar_file* files, uint32_t nfiles, const uint64_t* piece_sizes,
             uint32_t npieces, uint64_t begin, uint64_t len, int format, TarPlan* plan) {
  auto bad = [&](int rc, const std::string& msg) {
    plan->err = msg;
    return rc;
  };
  if ((nfiles && !files) || (npieces && !piece_sizes)) return bad(PFSCDC_EINVAL, "NULL argument");
  if (!format_ok(format)) return bad(PFSCDC_EINVAL, "unknown tar format");
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
    const char* why = tar_name_check(f.path, nl, z, format, &split[i], &rc);
    if (!why && nl && f.path[nl - 1] == '/' && f.count) {
      why = "a directory entry with pieces";
      rc = PFSCDC_EINVAL;
    }
    if (why) return bad(rc, "tar entry " + std::string(f.path) + ": " + why);
    off[i] = at;
    size[i] = z;
    at += tar_head_len((uint32_t)nl, z, split[i]) + ((z + 511) & ~511ull);
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
  uint64_t nx = 0;
  for (; i < nfiles && off[i] < end; i++) {
    const pfscdc_tar_file& f = files[i];
    const size_t nl = std::strlen(f.path);
    plan->entries.push_back(TarEntry{off[i], size[i], (uint32_t)plan->names.size(), (uint16_t)nl,
                                     (int16_t)split[i]});
    plan->names.append(f.path, nl);
    const uint64_t head = tar_head_len((uint32_t)nl, size[i], split[i]);
    // xblk begins with the window's first PAX entry: a zero for it and each entry before it
    if (head > 512 && plan->xblk.empty()) plan->xblk.assign(plan->entries.size(), 0);
    nx += head / 512 - 1;
    if (!plan->xblk.empty()) plan->xblk.push_back(nx);
    uint64_t p = off[i] + head;  // stream offset of the piece's first byte
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
  if (pfscdc::tar_name_check(path, len, size, PFSCDC_TAR_USTAR, &split, &rc)) return rc;
  pfscdc::ustar_header(path, len, size, split, out);
  return PFSCDC_OK;
}

int pfscdc_tar_head(const char* path, uint64_t size, int format, uint8_t* out, uint64_t cap,
                    uint64_t* len) {
  if (!path || !len || !pfscdc::format_ok(format)) return PFSCDC_EINVAL;
  *len = 0;
  const size_t nl = std::strlen(path);
  int split, rc;
  if (pfscdc::tar_name_check(path, nl, size, format, &split, &rc)) return rc;
  *len = pfscdc::tar_head_len((uint32_t)nl, size, split);
  if (!out) return PFSCDC_OK;
  if (cap < *len) return PFSCDC_EINVAL;
  if (split >= -1) pfscdc::ustar_header(path, nl, size, split, out);
  else pfscdc::pax_head(path, nl, size, split, out);
  return PFSCDC_OK;
}

int pfscdc_tar_layout_format(const pfscdc_tar_file* files, uint32_t nfiles, const uint64_t* sizes,
                             int format, uint64_t* entry_offsets, uint64_t* total) {
  if (!total || (nfiles && (!files || !sizes)) || !pfscdc::format_ok(format)) return PFSCDC_EINVAL;
  uint64_t at = 0;
  for (uint32_t i = 0; i < nfiles; i++) {
    if (!files[i].path) return PFSCDC_EINVAL;
    const size_t nl = std::strlen(files[i].path);
    int split, rc;
    if (pfscdc::tar_name_check(files[i].path, nl, sizes[i], format, &split, &rc)) return rc;
    if (files[i].path[nl - 1] == '/' && files[i].count) return PFSCDC_EINVAL;
    if (entry_offsets) entry_offsets[i] = at;
    at += pfscdc::tar_head_len((uint32_t)nl, sizes[i], split) + ((sizes[i] + 511) & ~511ull);
    if (at > (1ull << 62)) return PFSCDC_EINVAL;
  }
  if (entry_offsets) entry_offsets[nfiles] = at;
  *total = at + 1024;
  return PFSCDC_OK;
}

int pfscdc_tar_layout(const pfscdc_tar_file* files, uint32_t nfiles, const uint64_t* sizes,
                      uint64_t* entry_offsets, uint64_t* total) {
  return pfscdc_tar_layout_format(files, nfiles, sizes, PFSCDC_TAR_USTAR, entry_offsets, total);
}

}  // extern "C"
