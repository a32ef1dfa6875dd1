// index_parse.h — bounded parser of one index.Index proto (fileset/index/index.proto with
// chunk/chunk.proto's DataRef and Ref), shared by the host specification
// (pfscdc_index_decode_host, index_decode.cpp) and the device decode (index_count_kernel /
// index_fill_kernel, list_kernels.hip).  Plain C++ with no library call, so a sanitizer build
// of the host side checks the very bounds logic the kernels run.
//
// Every read is bounded by the range the caller gives: a varint longer than 10 bytes, a nested
// length past its parent, a wire type that does not fit a known field, and an id, dek or hash
// that is not 32 bytes all return false.  Unknown fields of a known wire type are skipped.
// proto3 semantics: an absent field is zero, the last occurrence of a scalar wins, repeated
// data_refs append.
#pragma once
#include <stdint.h>

#include "../../include/pfscdc.h"

// PFSCDC_HD comes from the including file: `__host__ __device__` in list_kernels.hip, empty in
// index_list.h (host code, which a plain C++ compiler must be able to build).

namespace pfscdc {

struct IdxFrame {
  const uint8_t *path, *tag, *last, *cref;  // into the frame (the last occurrence of each)
  uint32_t path_len, tag_len, last_len, cref_len;
  uint32_t flags;  // PFSCDC_IDX_*
  uint32_t count;  // File.data_refs
  int64_t size_sum, range_offset;
};

PFSCDC_HD inline bool idx_varint(const uint8_t*& p, const uint8_t* end, uint64_t* v) {
  uint64_t x = 0;
  for (int i = 0; i < 10; i++) {
    if (p >= end) return false;
    const uint8_t b = *p++;
    x |= (uint64_t)(b & 0x7f) << (7 * i);
    if (!(b & 0x80)) {
      *v = x;
      return true;
    }
  }
  return false;  // longer than 10 bytes
}

// a length-delimited field's payload: [*s, *s + *n) inside [p, end)
PFSCDC_HD inline bool idx_len(const uint8_t*& p, const uint8_t* end, const uint8_t** s,
                              uint32_t* n) {
  uint64_t l;
  if (!idx_varint(p, end, &l)) return false;
  if (l > (uint64_t)(end - p) || l > 0xffffffffull) return false;
  *s = p;
  *n = (uint32_t)l;
  p += l;
  return true;
}

PFSCDC_HD inline bool idx_skip(const uint8_t*& p, const uint8_t* end, uint32_t wire) {
  uint64_t v;
  const uint8_t* s;
  uint32_t n;
  switch (wire) {
    case 0: return idx_varint(p, end, &v);
    case 1:
      if ((uint64_t)(end - p) < 8) return false;
      p += 8;
      return true;
    case 2: return idx_len(p, end, &s, &n);
    case 5:
      if ((uint64_t)(end - p) < 4) return false;
      p += 4;
      return true;
    default: return false;  // groups and the two unassigned wire types
  }
}

PFSCDC_HD inline bool idx_bytes32(const uint8_t*& p, const uint8_t* end, uint8_t out[32]) {
  const uint8_t* s;
  uint32_t n;
  if (!idx_len(p, end, &s, &n) || n != 32) return false;
  for (int i = 0; i < 32; i++) out[i] = s[i];
  return true;
}

// chunk.Ref: id 1, size_bytes 2, edge 3, dek 4, encryption_algo 5, compression_algo 6
PFSCDC_HD inline bool idx_ref(const uint8_t* p, const uint8_t* end, pfscdc_full_dataref* d) {
  while (p < end) {
    uint64_t key, v;
    if (!idx_varint(p, end, &key)) return false;
    const uint32_t wire = (uint32_t)(key & 7);
    const uint64_t field = key >> 3;
    if (field == 1 || field == 4) {
      if (wire != 2 || !idx_bytes32(p, end, field == 1 ? d->ref.id : d->ref.dek)) return false;
    } else if (field == 2 || field == 3 || field == 5 || field == 6) {
      if (wire != 0 || !idx_varint(p, end, &v)) return false;
      if (field == 2) d->ref_size = (int64_t)v;
      if (field == 3) d->edge = v != 0;
    } else if (!idx_skip(p, end, wire)) {
      return false;
    }
  }
  return true;
}

// chunk.DataRef: ref 1, hash 2, offset_bytes 3, size_bytes 4
PFSCDC_HD inline bool idx_dataref(const uint8_t* p, const uint8_t* end, pfscdc_full_dataref* d) {
  for (int i = 0; i < 32; i++) d->ref.id[i] = d->ref.dek[i] = d->data.hash[i] = 0;
  d->ref_size = 0;
  d->edge = 0;
  d->reserved = 0;
  d->data.offset_bytes = d->data.size_bytes = 0;
  while (p < end) {
    uint64_t key, v;
    if (!idx_varint(p, end, &key)) return false;
    const uint32_t wire = (uint32_t)(key & 7);
    const uint64_t field = key >> 3;
    if (field == 1) {
      const uint8_t* s;
      uint32_t n;
      if (wire != 2 || !idx_len(p, end, &s, &n) || !idx_ref(s, s + n, d)) return false;
    } else if (field == 2) {
      if (wire != 2 || !idx_bytes32(p, end, d->data.hash)) return false;
    } else if (field == 3 || field == 4) {
      if (wire != 0 || !idx_varint(p, end, &v)) return false;
      if (field == 3) d->data.offset_bytes = (int64_t)v;
      else d->data.size_bytes = (int64_t)v;
    } else if (!idx_skip(p, end, wire)) {
      return false;
    }
  }
  return true;
}

// index.Index [p, end): path 1, range 2 {offset 1, last_path 2, chunk_ref 3}, file 3 {tag 1,
// data_refs 2}.  out (nullable): receives the File's DataRefs in order and then, with
// PFSCDC_IDX_HAS_CHUNK_REF, the Range's chunk_ref, at most cap records.  The count of records
// (fr->count, + 1 with a chunk_ref) is the same with and without out: a count pass sizes what
// a fill pass writes.
PFSCDC_HD inline bool idx_parse(const uint8_t* p, const uint8_t* end, IdxFrame* fr,
                                pfscdc_full_dataref* out, uint64_t cap) {
  fr->path = fr->tag = fr->last = fr->cref = nullptr;
  fr->path_len = fr->tag_len = fr->last_len = fr->cref_len = 0;
  fr->flags = fr->count = 0;
  fr->size_sum = fr->range_offset = 0;
  pfscdc_full_dataref tmp;
  while (p < end) {
    uint64_t key;
    if (!idx_varint(p, end, &key)) return false;
    const uint32_t wire = (uint32_t)(key & 7);
    const uint64_t field = key >> 3;
    const uint8_t* s;
    uint32_t n;
    if (field == 1) {
      if (wire != 2 || !idx_len(p, end, &fr->path, &fr->path_len)) return false;
    } else if (field == 2) {  // Range
      if (wire != 2 || !idx_len(p, end, &s, &n)) return false;
      fr->flags |= PFSCDC_IDX_HAS_RANGE;
      for (const uint8_t* e = s + n; s < e;) {
        uint64_t k, v;
        if (!idx_varint(s, e, &k)) return false;
        const uint32_t w = (uint32_t)(k & 7);
        const uint64_t f = k >> 3;
        if (f == 1) {
          if (w != 0 || !idx_varint(s, e, &v)) return false;
          fr->range_offset = (int64_t)v;
        } else if (f == 2) {
          if (w != 2 || !idx_len(s, e, &fr->last, &fr->last_len)) return false;
        } else if (f == 3) {
          if (w != 2 || !idx_len(s, e, &fr->cref, &fr->cref_len)) return false;
          fr->flags |= PFSCDC_IDX_HAS_CHUNK_REF;
        } else if (!idx_skip(s, e, w)) {
          return false;
        }
      }
    } else if (field == 3) {  // File
      if (wire != 2 || !idx_len(p, end, &s, &n)) return false;
      fr->flags |= PFSCDC_IDX_HAS_FILE;
      for (const uint8_t* e = s + n; s < e;) {
        uint64_t k;
        if (!idx_varint(s, e, &k)) return false;
        const uint32_t w = (uint32_t)(k & 7);
        const uint64_t f = k >> 3;
        if (f == 1) {
          if (w != 2 || !idx_len(s, e, &fr->tag, &fr->tag_len)) return false;
        } else if (f == 2) {
          const uint8_t* d;
          uint32_t dn;
          if (w != 2 || !idx_len(s, e, &d, &dn) || !idx_dataref(d, d + dn, &tmp)) return false;
          if (fr->count == 0xffffffffu) return false;
          if (out && fr->count < cap) out[fr->count] = tmp;
          fr->count++;
          fr->size_sum = (int64_t)((uint64_t)fr->size_sum + (uint64_t)tmp.data.size_bytes);
        } else if (!idx_skip(s, e, w)) {
          return false;
        }
      }
    } else if (!idx_skip(p, end, wire)) {
      return false;
    }
  }
  if (fr->flags & PFSCDC_IDX_HAS_CHUNK_REF) {
    if (!idx_dataref(fr->cref, fr->cref + fr->cref_len, &tmp)) return false;
    if (out && fr->count < cap) out[fr->count] = tmp;
  }
  return true;
}

// records a frame takes in the DataRef array, bytes in the blob (each string NUL-terminated)
PFSCDC_HD inline uint32_t idx_records(const IdxFrame& fr) {
  return fr.count + ((fr.flags & PFSCDC_IDX_HAS_CHUNK_REF) ? 1u : 0u);
}
PFSCDC_HD inline uint64_t idx_blob_bytes(const IdxFrame& fr) {
  return (uint64_t)fr.path_len + fr.tag_len + fr.last_len + 3;
}

// the frame's entry record and strings, once its DataRefs lie at drs[first, ...) and its
// strings go to blob + at
PFSCDC_HD inline void idx_emit(const IdxFrame& fr, uint64_t first, uint64_t at, char* blob,
                               pfscdc_index_entry* e) {
  e->path_off = at;
  e->path_len = fr.path_len;
  for (uint32_t i = 0; i < fr.path_len; i++) blob[at + i] = (char)fr.path[i];
  at += fr.path_len;
  blob[at++] = 0;
  e->tag_off = at;
  e->tag_len = fr.tag_len;
  for (uint32_t i = 0; i < fr.tag_len; i++) blob[at + i] = (char)fr.tag[i];
  at += fr.tag_len;
  blob[at++] = 0;
  e->last_path_off = at;
  e->last_path_len = fr.last_len;
  for (uint32_t i = 0; i < fr.last_len; i++) blob[at + i] = (char)fr.last[i];
  at += fr.last_len;
  blob[at] = 0;
  e->flags = fr.flags;
  e->first = (uint32_t)first;
  e->count = fr.count;
  e->size_bytes = fr.size_sum;
  e->range_offset = fr.range_offset;
}

// the int64 little-endian length at p (8 readable bytes, any alignment)
PFSCDC_HD inline int64_t idx_le64(const uint8_t* p) {
  uint64_t v = 0;
  for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i);
  return (int64_t)v;
}

}  // namespace pfscdc
