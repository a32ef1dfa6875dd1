// index_decode.cpp — the host-only half of reading a fileset back: the owned index list, the
// decode of one level's stream of pbutil frames (pfscdc_index_decode_host, the specification
// the decode kernels are tested against), Reader.Iterate's filter and MergeReader.iterate.
// No GPU call and no HIP header in this file.
//
// Reference (paths under /root/reference/src/internal):
//   storage/fileset/index/reader.go:95-122   atStart, atEnd (range and prefix filters)
//   storage/fileset/merge.go:37-77,157-164   MergeReader.iterate, compare (path, then tag)
//   stream/priority_queue.go:103-127         groups of equal streams, sorted by priority
//   pbutil/pbutil.go:39,65                   int64 LE length + proto
#include <algorithm>
#include <cstring>
#include <memory>

#include "index_list.h"

using List = pfscdc_index_list;

namespace pfscdc {

static_assert(sizeof(pfscdc_index_entry) == 64, "index entry record layout");
static_assert(sizeof(pfscdc_full_dataref) == 128, "full DataRef record layout");

// the frame's records appended to l (fr parsed from [p, end) before, so this parse succeeds)
bool idx_append_frame(List* l, const IdxFrame& fr, const uint8_t* p, const uint8_t* end) {
  const uint64_t first = l->drs.size(), recs = idx_records(fr);
  if (first + recs > 0xffffffffull || l->entries.size() >= 0xffffffffull) return false;
  l->drs.resize(first + recs);
  IdxFrame again;
  if (!idx_parse(p, end, &again, l->drs.data() + first, recs)) return false;
  const uint64_t at = l->blob.size();
  l->blob.resize(at + idx_blob_bytes(again));
  l->entries.emplace_back();
  idx_emit(again, first, at, l->blob.data(), &l->entries.back());
  return true;
}

// PFSCDC_OK, or PFSCDC_ECORRUPT with *err = the start of the first frame that does not parse
int idx_decode_stream(const uint8_t* p, uint64_t n, uint64_t limit, bool open_end, List* l,
                      uint64_t* err) {
  for (uint64_t pos = 0; pos < n && pos < limit;) {
    *err = pos;
    if (n - pos < 8) {
      if (open_end) break;
      return PFSCDC_ECORRUPT;
    }
    const int64_t len = idx_le64(p + pos);
    if (len >= 0 && (uint64_t)len > n - pos - 8 && open_end) break;
    if (len < 0 || (uint64_t)len > n - pos - 8) return PFSCDC_ECORRUPT;
    const uint8_t *b = p + pos + 8, *e = b + len;
    IdxFrame fr;
    if (!idx_parse(b, e, &fr, nullptr, 0)) return PFSCDC_ECORRUPT;
    if (!idx_append_frame(l, fr, b, e)) return PFSCDC_EUNSUPPORTED;  // 2^32 records
    pos += 8 + (uint64_t)len;
  }
  *err = kIdxNone;
  return PFSCDC_OK;
}

IdxStr idx_path(const List& l, const pfscdc_index_entry& e) { return {l.blob.data() + e.path_off, e.path_len}; }
IdxStr idx_tag(const List& l, const pfscdc_index_entry& e) { return {l.blob.data() + e.tag_off, e.tag_len}; }
IdxStr idx_last_path(const List& l, const pfscdc_index_entry& e) {
  return {l.blob.data() + e.last_path_off, e.last_path_len};
}
int idx_cmp(IdxStr a, IdxStr b) {  // strings.Compare: bytewise
  const size_t k = std::min(a.n, b.n);
  const int c = k ? std::memcmp(a.p, b.p, k) : 0;
  return c ? c : (a.n < b.n ? -1 : a.n > b.n ? 1 : 0);
}

IdxFilter::IdxFilter(const pfscdc_index_filter* f) {
  if (!f) return;
  if (f->lower) lower = f->lower;
  if (f->upper) upper = f->upper;
  if (f->prefix) prefix = f->prefix;
  if (f->tag) tag = f->tag;
}
bool IdxFilter::at_start(IdxStr name) const {
  const std::string& b = !lower.empty() ? lower : prefix;
  return idx_cmp(name, IdxStr{b.data(), b.size()}) >= 0;
}
bool IdxFilter::at_end(IdxStr name) const {
  if (!upper.empty()) return idx_cmp(name, IdxStr{upper.data(), upper.size()}) > 0;
  // the first min(len(name), len(prefix)) bytes of each
  const size_t k = std::min(name.n, prefix.size());
  return k && std::memcmp(name.p, prefix.data(), k) > 0;
}
bool IdxFilter::tag_ok(IdxStr t) const {
  return tag.empty() || idx_cmp(t, IdxStr{tag.data(), tag.size()}) == 0;
}

// entry e of src appended to dst: strings, File DataRefs and the Range's chunk_ref
void idx_append_entry(List* dst, const List& src, const pfscdc_index_entry& e) {
  pfscdc_index_entry o = e;
  const uint32_t recs = e.count + ((e.flags & PFSCDC_IDX_HAS_CHUNK_REF) ? 1u : 0u);
  o.first = (uint32_t)dst->drs.size();
  dst->drs.insert(dst->drs.end(), src.drs.begin() + e.first, src.drs.begin() + e.first + recs);
  auto put = [&](IdxStr s, uint64_t* off) {
    *off = dst->blob.size();
    dst->blob.insert(dst->blob.end(), s.p, s.p + s.n);
    dst->blob.push_back(0);
  };
  put(idx_path(src, e), &o.path_off);
  put(idx_tag(src, e), &o.tag_off);
  put(idx_last_path(src, e), &o.last_path_off);
  dst->entries.push_back(o);
}

}  // namespace pfscdc

using namespace pfscdc;

extern "C" {


uint32_t pfscdc_index_list_count(const pfscdc_index_list* l) {
  return l ? (uint32_t)l->entries.size() : 0;
}
const pfscdc_index_entry* pfscdc_index_list_entries(const pfscdc_index_list* l) {
  return l ? l->entries.data() : nullptr;
}
const char* pfscdc_index_list_blob(const pfscdc_index_list* l, uint64_t* len) {
  if (len) *len = l ? l->blob.size() : 0;
  return l ? l->blob.data() : nullptr;
}
const pfscdc_full_dataref* pfscdc_index_list_datarefs(const pfscdc_index_list* l, uint32_t* n) {
  if (n) *n = l ? (uint32_t)l->drs.size() : 0;
  return l ? l->drs.data() : nullptr;
}
const pfscdc_tar_file* pfscdc_index_list_tar_files(pfscdc_index_list* l) {
  if (!l) return nullptr;
  if (l->tar.size() != l->entries.size()) {
    l->tar.resize(l->entries.size());
    for (size_t i = 0; i < l->entries.size(); i++) {
      const pfscdc_index_entry& e = l->entries[i];
      l->tar[i] = pfscdc_tar_file{l->blob.data() + e.path_off, e.first, e.count};
    }
  }
  return l->tar.data();
}
int pfscdc_index_list_free(pfscdc_index_list* l) {
  delete l;
  return PFSCDC_OK;
}

int pfscdc_index_decode_host(const void* stream, uint64_t n, pfscdc_index_list** out,
                             uint64_t* err_offset) {
  if (!out || (n && !stream)) return PFSCDC_EINVAL;
  *out = nullptr;
  std::unique_ptr<List> l(new List());
  uint64_t err = kIdxNone;
  const int rc = idx_decode_stream((const uint8_t*)stream, n, n, false, l.get(), &err);
  if (err_offset) *err_offset = rc == PFSCDC_ECORRUPT ? err : 0;
  if (rc) return rc;
  *out = l.release();
  return PFSCDC_OK;
}

int pfscdc_index_filter_list(const pfscdc_index_list* in, const pfscdc_index_filter* filter,
                             pfscdc_index_list** out) {
  if (!in || !out) return PFSCDC_EINVAL;
  *out = nullptr;
  const IdxFilter f(filter);
  std::unique_ptr<List> l(new List());
  for (const pfscdc_index_entry& e : in->entries) {
    if (f.at_end(idx_path(*in, e))) break;
    if (f.at_start(idx_path(*in, e)) && f.tag_ok(idx_tag(*in, e))) idx_append_entry(l.get(), *in, e);
  }
  *out = l.release();
  return PFSCDC_OK;
}

int pfscdc_index_merge(const pfscdc_index_list* const* lists, uint32_t nfilesets,
                       pfscdc_index_list** out) {
  if (!out || (nfilesets && !lists) || nfilesets > (1u << 30)) return PFSCDC_EINVAL;
  *out = nullptr;
  const uint32_t ns = 2 * nfilesets;  // stream k: fileset k / 2, deletive iff k is even
  std::vector<size_t> pos(ns, 0);
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
    for (uint32_t k = 0; k < ns; k++) {
      if (!head(k)) continue;
      const int c = group.empty() ? -1 : compare(k, group[0]);
      if (c < 0) group.assign(1, k);
      else if (c == 0) group.push_back(k);
    }
    if (group.empty()) break;
    const uint32_t k0 = group[0];
    if (group.size() == 1) {
      if (k0 % 2 == 1) idx_append_entry(l.get(), *lists[k0], *head(k0));
    } else {
      std::vector<pfscdc_full_dataref> acc;
      bool drop = false;
      for (size_t g = 0; g < group.size(); g++) {
        const uint32_t k = group[g];
        if (k % 2 == 0) {
          if (g + 1 == group.size()) drop = true;
          acc.clear();
          continue;
        }
        const pfscdc_index_entry& e = *head(k);
        acc.insert(acc.end(), lists[k]->drs.begin() + e.first, lists[k]->drs.begin() + e.first + e.count);
      }
      if (!drop) {
        if (l->drs.size() + acc.size() > 0xffffffffull) return PFSCDC_EUNSUPPORTED;
        pfscdc_index_entry e = *head(k0);  // the group's first entry, with the merged DataRefs
        e.flags &= ~(PFSCDC_IDX_HAS_CHUNK_REF | PFSCDC_IDX_HAS_RANGE);
        e.flags |= PFSCDC_IDX_HAS_FILE;
        e.count = 0;
        e.first = 0;
        idx_append_entry(l.get(), *lists[k0], e);
        pfscdc_index_entry& o = l->entries.back();
        o.first = (uint32_t)l->drs.size();
        o.count = (uint32_t)acc.size();
        o.size_bytes = 0;
        for (const pfscdc_full_dataref& d : acc)
          o.size_bytes = (int64_t)((uint64_t)o.size_bytes + (uint64_t)d.data.size_bytes);
        l->drs.insert(l->drs.end(), acc.begin(), acc.end());
      }
    }
    for (uint32_t k : group) pos[k]++;
  }
  *out = l.release();
  return PFSCDC_OK;
}

}  // extern "C"
