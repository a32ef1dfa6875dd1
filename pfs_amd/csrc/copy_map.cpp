// copy_map.cpp — CopyFile's selection and path transform on the host (pfscdc_copy_map_host): the
// open's options, NewIndexFilter's predicate and NewIndexMapper's transform, each taken literally.
// It is the specification the cmap_* kernels (list_kernels.hip §13, driven by copy_map_dev.cpp)
// are tested against, and the arm for the lists the device refuses.  No GPU call and no HIP header
// in this file: a stand-alone sanitizer build compiles it with index_decode.cpp and a plain C++
// compiler.
//
// Reference (paths under the reference's src):
//   server/pfs/server/driver_file.go:143-171          copyFile: cleanPath, pathTransform, the
//                                                     open's options, the filter and the mapper
//   server/pfs/server/paths.go:54-60                  cleanPath
//   internal/storage/fileset/transforms.go:20-90      NewIndexFilter, NewIndexMapper
//   internal/storage/fileset/index/reader.go:95-122   atStart, atEnd (WithPrefix), the tag
//   Go's path.Clean, path.Join and (Unix) filepath.Rel
#include "copy_map.h"

#include <cstring>
#include <memory>

using List = pfscdc_index_list;

namespace pfscdc {

namespace {

// filepath.Rel on Unix (no volume names; the separator is '/'); false for its error
bool go_rel(const std::string& basepath, const std::string& targpath, std::string* out) {
  std::string base = go_clean(basepath);
  const std::string targ = go_clean(targpath);
  if (targ == base) {
    *out = ".";
    return true;
  }
  if (base == ".") base.clear();
  const bool base_slashed = !base.empty() && base[0] == '/';
  const bool targ_slashed = !targ.empty() && targ[0] == '/';
  if (base_slashed != targ_slashed) return false;
  // position base[b0:bi] and targ[t0:ti] at the first differing elements
  const size_t bl = base.size(), tl = targ.size();
  size_t b0 = 0, bi = 0, t0 = 0, ti = 0;
  while (bi < bl && ti < tl) {
    while (bi < bl && base[bi] != '/') bi++;
    while (ti < tl && targ[ti] != '/') ti++;
    if (targ.compare(t0, ti - t0, base, b0, bi - b0) != 0) break;
    if (bi < bl) bi++;
    if (ti < tl) ti++;
    b0 = bi;
    t0 = ti;
  }
  if (base.compare(b0, bi - b0, "..") == 0) return false;
  if (b0 != bl) {  // base elements left: go up before going down
    size_t seps = 0;
    for (size_t k = b0; k < bl; k++) seps += base[k] == '/';
    std::string r = "..";
    for (size_t k = 0; k < seps; k++) r += "/..";
    if (t0 != tl) {
      r.push_back('/');
      r.append(targ, t0, std::string::npos);
    }
    *out = r;
    return true;
  }
  *out = targ.substr(t0);
  return true;
}

// path.Join of two elements: the empty ones dropped, the rest joined by '/' and cleaned
std::string go_join(const std::string& a, const std::string& b) {
  if (a.empty() && b.empty()) return std::string();
  if (a.empty()) return go_clean(b);
  if (b.empty()) return go_clean(a);
  return go_clean(a + "/" + b);
}

bool has_prefix(IdxStr s, const std::string& p) {
  return s.n >= p.size() && std::memcmp(s.p, p.data(), p.size()) == 0;
}

// pathTransform (driver_file.go:151-157): path.Join(dst, filepath.Rel(src, path)); false where
// Rel returns an error (the reference panics; no path the filter keeps gets there)
bool copy_map_path(const CopyArg& a, const std::string& path, std::string* out) {
  std::string rel;
  if (!go_rel(a.src, path, &rel)) return false;
  *out = go_join(a.dst, rel);
  return true;
}

}  // namespace

CopyArg copy_arg(const char* src, const char* src_tag, const char* dst) {
  CopyArg a;
  a.src = clean_path(src ? src : "");
  a.dst = clean_path(dst ? dst : "");
  a.tag = src_tag ? src_tag : "";
  return a;
}

int copy_map_host(const List& in, const CopyArg& a, List* out, std::string* err) {
  out->entries.clear();
  out->drs.clear();
  out->blob.clear();
  out->tar.clear();
  const uint64_t nb = in.blob.size(), nr = in.drs.size();
  for (const pfscdc_index_entry& e : in.entries)
    if (e.path_off > nb || e.path_len > nb - e.path_off || e.tag_off > nb ||
        e.tag_len > nb - e.tag_off || e.last_path_off > nb || e.last_path_len > nb - e.last_path_off ||
        e.first > nr || e.count > nr - e.first) {
      *err = "an entry's strings or DataRefs lie outside the list's arrays";
      return PFSCDC_EINVAL;
    }
  for (const pfscdc_index_entry& e : in.entries)
    if (e.flags & (PFSCDC_IDX_HAS_RANGE | PFSCDC_IDX_HAS_CHUNK_REF)) {
      *err = "an entry with a Range: not a level-0 list";
      return PFSCDC_EINVAL;
    }
  // index.WithPrefix(srcPath), index.WithTag(src.Tag): Reader.Iterate as pfscdc_index_filter_list
  // restates it
  const pfscdc_index_filter fo{nullptr, nullptr, a.src.c_str(), a.tag.c_str()};
  const IdxFilter f(&fo);
  const std::string dir = a.src + "/";
  for (const pfscdc_index_entry& e : in.entries) {
    const IdxStr p = idx_path(in, e);
    if (f.at_end(p)) break;
    if (!f.at_start(p) || !f.tag_ok(idx_tag(in, e))) continue;
    // NewIndexFilter: idx.Path == srcPath || strings.HasPrefix(idx.Path, srcPath+"/")
    if (!(idx_cmp(p, IdxStr{a.src.data(), a.src.size()}) == 0 || has_prefix(p, dir))) continue;
    // NewIndexMapper: idx2.Path = pathTransform(idx2.Path)
    std::string np;
    if (!copy_map_path(a, std::string(p.p, p.n), &np)) {
      *err = "cannot apply path transform";
      return PFSCDC_EINVAL;
    }
    if (np.size() > 0xffffffffull) {
      *err = "a new path longer than 2^32 - 1 bytes";
      return PFSCDC_EINVAL;
    }
    if (out->entries.size() >= 0xffffffffull) {
      *err = "more than 2^32 - 1 entries";
      return PFSCDC_EUNSUPPORTED;
    }
    pfscdc_index_entry o = e;
    o.first = (uint32_t)out->drs.size();
    out->drs.insert(out->drs.end(), in.drs.begin() + e.first, in.drs.begin() + e.first + e.count);
    o.path_off = out->blob.size();
    o.path_len = (uint32_t)np.size();
    out->blob.insert(out->blob.end(), np.begin(), np.end());
    out->blob.push_back(0);
    const IdxStr t = idx_tag(in, e);
    o.tag_off = out->blob.size();
    out->blob.insert(out->blob.end(), t.p, t.p + t.n);
    out->blob.push_back(0);
    o.last_path_off = out->blob.size();  // a File's entry has no LastPath
    o.last_path_len = 0;
    out->blob.push_back(0);
    out->entries.push_back(o);
  }
  return PFSCDC_OK;
}

}  // namespace pfscdc

extern "C" {

int pfscdc_copy_map_host(const pfscdc_index_list* in, const char* src, const char* src_tag,
                         const char* dst, pfscdc_index_list** out) {
  if (!out) return PFSCDC_EINVAL;
  *out = nullptr;
  std::string err;
  static const List empty;
  std::unique_ptr<List> l(new List());
  if (int rc = pfscdc::copy_map_host(in ? *in : empty, pfscdc::copy_arg(src, src_tag, dst), l.get(),
                                     &err))
    return rc;
  *out = l.release();
  return PFSCDC_OK;
}

}  // extern "C"
