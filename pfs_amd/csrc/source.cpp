// source.cpp — the Source on the host (pfscdc_source_host): the directory inserter, the index
// filter and source.Iterate's FileInfo recursion, each taken literally.  It is the specification
// the src_* kernels (list_kernels.hip §11, driven by source_dev.cpp) are tested against, and the
// arm for the lists the device refuses.  No GPU call and no HIP header in this file: a
// stand-alone sanitizer build compiles it with index_decode.cpp and a plain C++ compiler.
//
// Reference (paths under the reference's src):
//   internal/storage/fileset/dir_inserter.go:22-58   dirInserter.Iterate (emit), parentOf
//   internal/storage/fileset/transforms.go:31-49     indexFilter.Iterate (the `full` dir state)
//   internal/storage/fileset/util.go:67-88,149-158   Clean, IsClean, IsDir, hashDataRefs
//   server/pfs/server/source.go:28-157               source.Iterate, checkFileInfoCache,
//                                                    computeFileInfo, NewErrOnEmpty
//   server/pfs/server/driver_file.go:173-385         the predicates of getFile, inspectFile,
//                                                    listFile, walkFile, diffFile
//   server/pfs/server/paths.go:22-60                 globMatchFunction, pathIsChild, cleanPath
//   server/pfs/server/driver_file.go:284-308         globFile's second match, over the same stream
#include "source.h"

#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>

using List = pfscdc_index_list;

namespace pfscdc {

// ---- BLAKE2b-256, unkeyed (RFC 7693), for the host arm ----
namespace {

constexpr uint64_t kIV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                             0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                             0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
constexpr uint8_t kSigma[12][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15},
    {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4},
    {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13},
    {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11},
    {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5},
    {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15},
    {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};

inline uint64_t rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

}  // namespace

Blake2b256::Blake2b256() {
  for (int i = 0; i < 8; i++) h[i] = kIV[i];
  h[0] ^= 0x01010020ull;  // digest 32 bytes, no key, fanout 1, depth 1
}

void Blake2b256::compress(bool last) {
  uint64_t m[16], v[16];
  for (int i = 0; i < 16; i++) {
    uint64_t w = 0;
    for (int b = 7; b >= 0; b--) w = (w << 8) | buf[8 * i + b];
    m[i] = w;
  }
  for (int i = 0; i < 8; i++) {
    v[i] = h[i];
    v[8 + i] = kIV[i];
  }
  v[12] ^= t;  // the counter's high word stays 0 below 2^64 bytes
  if (last) v[14] = ~v[14];
  auto g = [&](int a, int b, int c, int d, uint64_t x, uint64_t y) {
    v[a] = v[a] + v[b] + x;
    v[d] = rotr(v[d] ^ v[a], 32);
    v[c] = v[c] + v[d];
    v[b] = rotr(v[b] ^ v[c], 24);
    v[a] = v[a] + v[b] + y;
    v[d] = rotr(v[d] ^ v[a], 16);
    v[c] = v[c] + v[d];
    v[b] = rotr(v[b] ^ v[c], 63);
  };
  for (int r = 0; r < 12; r++) {
    const uint8_t* s = kSigma[r];
    g(0, 4, 8, 12, m[s[0]], m[s[1]]);
    g(1, 5, 9, 13, m[s[2]], m[s[3]]);
    g(2, 6, 10, 14, m[s[4]], m[s[5]]);
    g(3, 7, 11, 15, m[s[6]], m[s[7]]);
    g(0, 5, 10, 15, m[s[8]], m[s[9]]);
    g(1, 6, 11, 12, m[s[10]], m[s[11]]);
    g(2, 7, 8, 13, m[s[12]], m[s[13]]);
    g(3, 4, 9, 14, m[s[14]], m[s[15]]);
  }
  for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[8 + i];
}

void Blake2b256::write(const uint8_t* p, size_t n) {
  while (n) {
    if (fill == 128) {  // a full buffer is compressed only once more input follows
      t += 128;
      compress(false);
      fill = 0;
    }
    const size_t k = n < 128 - fill ? n : 128 - fill;
    std::memcpy(buf + fill, p, k);
    fill += k;
    p += k;
    n -= k;
  }
}

void Blake2b256::sum(uint8_t out[32]) {
  t += fill;
  std::memset(buf + fill, 0, 128 - fill);
  compress(true);
  for (int i = 0; i < 4; i++)
    for (int b = 0; b < 8; b++) out[8 * i + b] = (uint8_t)(h[i] >> (8 * b));
}

// ---- Go's path.Dir; fileset.Clean (path.Clean, strings.Trim* and cleanPath: paths.h) ----
namespace {

bool is_dir(const std::string& p) { return !p.empty() && p.back() == '/'; }  // fileset.IsDir

std::string fs_clean(const std::string& p0, bool dir) {  // fileset.Clean (util.go:67-77)
  const std::string p = go_clean(p0);
  if (p == ".") return "/";
  std::string y = "/" + trim_slashes(p, true, true);
  if (dir && !is_dir(y)) y += "/";
  return y;
}

std::string go_dir(const std::string& p) {  // path.Dir: Clean of everything up to the last slash
  const size_t k = p.rfind('/');
  return go_clean(k == std::string::npos ? std::string() : p.substr(0, k + 1));
}

std::string parent_of(const std::string& x0) {  // dir_inserter.go:48-58
  const std::string x = trim_slashes(x0, false, true);
  std::string y = go_dir(x);
  if (y == x) return "/";
  if (!is_dir(y)) y += "/";
  return y;
}

bool has_prefix(const std::string& s, const std::string& p) {
  return s.size() >= p.size() && std::memcmp(s.data(), p.data(), p.size()) == 0;
}

bool path_is_child(const std::string& parent, const std::string& child) {  // paths.go:39-46
  if (!has_prefix(child, parent)) return false;
  const std::string rel = trim_slashes(child.substr(parent.size()), true, true);
  return rel.find('/') == std::string::npos;
}

thread_local std::string t_host_error;

}  // namespace

int source_arg(int kind, const char* arg, SrcArg* out, std::string* err) {
  out->kind = kind;
  out->all = out->exclude_dir = out->child_flag = false;
  out->name.clear();
  out->dir.clear();
  const std::string a = clean_path(arg ? arg : "");
  switch (kind) {
    case PFSCDC_SRC_ALL:
      out->all = true;
      return PFSCDC_OK;
    case PFSCDC_SRC_SUBTREE:  // p == "/" -> p = ""
    case PFSCDC_SRC_DIFF:     // the same filter; diffFile leaves NewErrOnEmpty out
      out->name = a == "/" ? std::string() : a;
      out->dir = out->name + "/";
      return PFSCDC_OK;
    case PFSCDC_SRC_LIST:
      out->name = a;
      out->dir = fs_clean(a, true);
      out->exclude_dir = out->child_flag = true;
      return PFSCDC_OK;
    case PFSCDC_SRC_GET:
      if (a.find_first_of("*?[]{}!()@+^\\") != std::string::npos) {
        *err = "getFile: the glob " + a + " is a pattern, and only literal globs are built";
        return PFSCDC_EUNSUPPORTED;
      }
      out->name = a;
      out->dir = a + "/";
      out->all = a == "/";  // mf("/") holds, "/" comes first and every path has its prefix
      return PFSCDC_OK;
    case PFSCDC_SRC_GLOB:  // getFile / globFile: globMatchFunction(cleanPath(arg))
      out->name = a;
      out->all = a == "/";
      return glob_parse(a, &out->glob, err);
    default:
      *err = "an unknown Source predicate";
      return PFSCDC_EINVAL;
  }
}

std::string source_not_found(const SrcArg& a) {
  return "file " + (a.name.empty() ? std::string("/") : a.name) + " not found";
}

// NewErrOnEmpty: getFile (literal or glob), and inspect / walk below the root (walkFile forgives
// it for the root); never a side of diffFile, whose missing path is an empty side
bool source_errs_on_empty(const SrcArg& a) {
  return a.kind == PFSCDC_SRC_GET || a.kind == PFSCDC_SRC_GLOB ||
         (a.kind == PFSCDC_SRC_SUBTREE && !a.name.empty());
}

void source_host_set_error(const std::string& text) { t_host_error = text; }

namespace {

// One File of the stream: an entry of the input, or a dirFile (src < 0).
struct Item {
  std::string path;
  int64_t src;
};

// The predicate each RPC hands to NewIndexFilter.
bool predicate(const SrcArg& a, const std::string& path) {
  switch (a.kind) {
    case PFSCDC_SRC_ALL: return true;
    case PFSCDC_SRC_SUBTREE:
    case PFSCDC_SRC_DIFF: return path == a.name || has_prefix(path, a.name + "/");
    case PFSCDC_SRC_LIST:
      if (path == a.dir) return false;  // the directory itself is not listed
      if (path == a.name) return true;
      return has_prefix(path, a.dir);
    case PFSCDC_SRC_GLOB: return glob_mf(a.glob, path);
    default: {  // globMatchFunction of a literal glob
      if (path == "/" && a.name == "/") return true;
      return trim_slashes(path, false, true) == a.name;
    }
  }
}

struct Info {
  int64_t size;
  uint8_t hash[32];
};

struct Iterate {  // source.Iterate's state: the stream, the second iterator, the cache
  const List& in;
  const uint8_t* leaf;
  const std::vector<Item>& fs;
  Iterate(const List& in_, const uint8_t* leaf_, const std::vector<Item>& fs_)
      : in(in_), leaf(leaf_), fs(fs_) {}
  size_t iter = 0;
  std::map<std::string, Info> cache;
  std::string err;

  Info regular(const Item& f) {  // computeRegularFileInfo
    Info fi{0, {}};
    if (f.src < 0) {  // dirFile.Hash panics in the reference; no caller gets here
      err = "Hash of a dirFile";
      return fi;
    }
    const pfscdc_index_entry& e = in.entries[f.src];
    fi.size = e.size_bytes;  // index.SizeBytes: the wrapping sum of the File's DataRefs
    if (leaf) {
      std::memcpy(fi.hash, leaf + 32 * (size_t)f.src, 32);
    } else {  // hashDataRefs
      Blake2b256 h;
      for (uint32_t k = 0; k < e.count; k++) h.write(in.drs[e.first + k].data.hash, 32);
      h.sum(fi.hash);
    }
    return fi;
  }

  bool compute(const std::string& target, Info* out) {  // computeFileInfo
    if (iter >= fs.size()) {
      err = "stream is done, can't compute hash for " + target;
      return false;
    }
    const Item& f = fs[iter++];
    if (f.path != target) {
      err = "stream is wrong place to compute hash for " + target;
      return false;
    }
    if (!is_dir(f.path)) {
      *out = regular(f);
      return err.empty();
    }
    uint64_t size = 0;
    Blake2b256 h;
    while (iter < fs.size() && has_prefix(fs[iter].path, target)) {
      Info child;
      const std::string next = fs[iter].path;
      if (!compute(next, &child)) return false;
      size += (uint64_t)child.size;
      h.write(child.hash, 32);
    }
    out->size = (int64_t)size;
    h.sum(out->hash);
    cache[target] = *out;
    return true;
  }

  bool info(const Item& f, Info* out) {
    auto it = cache.find(f.path);  // checkFileInfoCache: a cached directory
    if (it != cache.end()) {
      *out = it->second;
      return true;
    }
    // a regular file already iterated through when its directory was computed (path.Split)
    const size_t k = f.path.rfind('/');
    if (cache.count(k == std::string::npos ? std::string() : f.path.substr(0, k + 1))) {
      *out = regular(f);
      return err.empty();
    }
    return compute(f.path, out);
  }
};

}  // namespace

int source_host(const List& in, const SrcArg& a, const uint8_t* leaf, List* out,
                std::vector<pfscdc_file_info>* infos, std::string* err, uint64_t* ndirs_out) {
  out->entries.clear();
  out->drs.clear();
  out->blob.clear();
  out->tar.clear();
  infos->clear();
  for (const pfscdc_index_entry& e : in.entries) {
    const uint64_t nb = in.blob.size(), nr = in.drs.size();
    if (e.path_off > nb || e.path_len > nb - e.path_off || e.tag_off > nb ||
        e.tag_len > nb - e.tag_off || e.last_path_off > nb || e.last_path_len > nb - e.last_path_off ||
        e.first > nr || e.count > nr - e.first) {
      *err = "an entry's strings or DataRefs lie outside the list's arrays";
      return PFSCDC_EINVAL;
    }
  }
  for (const pfscdc_index_entry& e : in.entries)
    if (e.flags & (PFSCDC_IDX_HAS_RANGE | PFSCDC_IDX_HAS_CHUNK_REF)) {
      *err = "an entry with a Range: not a level-0 list";
      return PFSCDC_EINVAL;
    }
  // ---- dirInserter.Iterate (dir_inserter.go:22-46)
  std::vector<Item> inserted;
  {
    std::string last_path;
    struct Emit {
      std::vector<Item>& dst;
      std::string& last_path;
      void operator()(const std::string& p, int64_t src) {
        const std::string parent = fs_clean(parent_of(p), true);
        if (p == "/" || last_path >= parent) {
          dst.push_back(Item{p, src});
          last_path = p;
          return;
        }
        (*this)(parent, -1);  // need to create entry for parent
        (*this)(p, src);
      }
    } emit{inserted, last_path};
    for (size_t i = 0; i < in.entries.size(); i++) {
      const IdxStr p = idx_path(in, in.entries[i]);
      emit(std::string(p.p, p.n), (int64_t)i);
    }
  }
  // ---- indexFilter.Iterate (transforms.go:31-49); getFile and globFile alone pass full
  std::vector<Item> selected;
  {
    const bool full = a.kind == PFSCDC_SRC_GET || a.kind == PFSCDC_SRC_GLOB;
    std::string dir;
    for (const Item& f : inserted) {
      if (full) {
        if (!dir.empty() && has_prefix(f.path, dir)) {
          selected.push_back(f);
          continue;
        }
        if (predicate(a, f.path) && is_dir(f.path)) dir = f.path;
      }
      if (predicate(a, f.path)) selected.push_back(f);
    }
  }
  // ---- source.Iterate (source.go:45-85)
  Iterate it(in, leaf, selected);
  uint64_t ndirs = 0;
  for (const Item& f : selected) {
    Info fi;
    if (!it.info(f, &fi)) {
      *err = it.err;
      return PFSCDC_EINVAL;
    }
    pfscdc_file_info r;
    std::memcpy(r.hash, fi.hash, 32);
    r.size = fi.size;
    r.type = is_dir(f.path) ? PFSCDC_FILE_TYPE_DIR : PFSCDC_FILE_TYPE_FILE;
    r.flags = a.child_flag && path_is_child(a.name, clean_path(f.path)) ? PFSCDC_INFO_CHILD : 0u;
    // globFile's second mf(fi.File.Path) (driver_file.go:284-308)
    if (a.kind == PFSCDC_SRC_GLOB && predicate(a, f.path)) r.flags |= PFSCDC_INFO_MATCH;
    infos->push_back(r);
    if (out->entries.size() >= 0xffffffffull) {
      *err = "more than 2^32 - 1 entries";
      return PFSCDC_EUNSUPPORTED;
    }
    if (f.src >= 0) {
      idx_append_entry(out, in, in.entries[f.src]);
      continue;
    }
    ndirs++;
    pfscdc_index_entry e;  // dirFile.Index(): Index{Path: path, File: &index.File{}}
    std::memset(&e, 0, sizeof e);
    e.path_off = out->blob.size();
    e.path_len = (uint32_t)f.path.size();
    out->blob.insert(out->blob.end(), f.path.begin(), f.path.end());
    out->blob.push_back(0);
    e.tag_off = out->blob.size();
    out->blob.push_back(0);
    e.last_path_off = out->blob.size();
    out->blob.push_back(0);
    e.flags = PFSCDC_IDX_HAS_FILE;
    e.first = (uint32_t)out->drs.size();
    out->entries.push_back(e);
  }
  if (ndirs_out) *ndirs_out = ndirs;
  // ---- NewErrOnEmpty
  if (selected.empty() && source_errs_on_empty(a)) {
    *err = source_not_found(a);
    return PFSCDC_ENOTFOUND;
  }
  return PFSCDC_OK;
}

}  // namespace pfscdc

extern "C" {

int pfscdc_source_host(const pfscdc_index_list* in, int kind, const char* arg,
                       const uint8_t* leaf_hashes, pfscdc_index_list** out,
                       pfscdc_file_info** infos) {
  if (!out || !infos) return PFSCDC_EINVAL;
  *out = nullptr;
  *infos = nullptr;
  std::string& err = pfscdc::t_host_error;
  err.clear();
  pfscdc::SrcArg a;
  if (int rc = pfscdc::source_arg(kind, arg, &a, &err)) return rc;
  static const List empty;
  std::unique_ptr<List> l(new List());
  std::vector<pfscdc_file_info> v;
  if (int rc = pfscdc::source_host(in ? *in : empty, a, leaf_hashes, l.get(), &v, &err, nullptr))
    return rc;
  pfscdc_file_info* p = (pfscdc_file_info*)std::malloc(sizeof(pfscdc_file_info) * (v.size() + 1));
  if (!p) return PFSCDC_ENOMEM;
  if (!v.empty()) std::memcpy(p, v.data(), sizeof(pfscdc_file_info) * v.size());
  *infos = p;
  *out = l.release();
  return PFSCDC_OK;
}

const char* pfscdc_source_host_error(void) { return pfscdc::t_host_error.c_str(); }

void pfscdc_file_infos_free(pfscdc_file_info* infos) { std::free(infos); }

}  // extern "C"
