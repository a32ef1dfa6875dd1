// list_kernels.hip — gfx950 kernels of the index list passes, which read filesets back: §8
// index.Reader, §9 MergeReader, §10 the tar plan of a resident list, §11 the Source, §12 DiffFile,
// §13 CopyFile's map (each section names the reference's lines; §1-§7, the data plane, are
// cdc_kernels.hip).  Every pass is a count kernel (one lane per item: what it emits), the prefix
// sums of the counts (index_scan_kernel, merge_scan_kernel or rtar_scan_kernel: one workgroup)
// and a fill kernel that writes each item's output at its own ranges.  Records and launchers:
// list_kernels.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PFSCDC_HD __host__ __device__  // index_parse.h: the parser runs in the kernels
#include "index_parse.h"
#include "list_kernels.h"

#define PFS_DEV __device__ __forceinline__

namespace pfscdc {

// ---- 8. index.Reader: one level's stream of pbutil frames into flat records -------------------
// (fileset/index/reader.go:124-181 levelReader, pbutil/pbutil.go:39,65; parser: index_parse.h)
//
// 8a. Frame walk.  The frames are a chain (int64 LE length, proto, next length ...), so one
// walker is serial; the level's chunks give the parallelism: every parent entry's Range.Offset
// claims a frame start inside its chunk, and one wave walks from each claim to the first frame
// start at or beyond the next chunk's begin (its exit), recording the starts on the way.  The
// walks are speculative: index.cpp accepts chunk i + 1's walk only if chunk i's exit equals its
// claim and launches the walk again from the exit otherwise.
// One wave per walker: the wave stages kIdxWin bytes from the 16-byte line holding the current
// position into LDS with one 16-byte load per lane and pass (1 KiB per wave instruction), then
// lane 0 hops through the window in LDS (a hop is one dependent 8-byte read: ~64 cycles of LDS
// latency against ~1-2 us for a dependent global load) until a length field crosses the
// window's end.  A frame longer than the window is hopped over: the next window starts at the
// next frame.  Every read lies in [0, n + 32) of a buffer allocated 64 bytes longer than n; a
// length that is negative or reaches past n ends the walk with err = the frame's start.
constexpr int kIdxWin = 8192;  // bytes staged per pass (+ 16: the window starts on a 16-B line)

__global__ __launch_bounds__(64) void index_walk_kernel(
    const uint8_t* __restrict__ buf, uint64_t n, const IdxWalk* __restrict__ walks, uint32_t nw,
    uint64_t* __restrict__ starts, IdxWalkOut* __restrict__ out) {
  __shared__ uint4 win[(kIdxWin + 16) / 16];
  __shared__ uint64_t s_pos;
  __shared__ uint32_t s_done;
  const uint8_t* wb = (const uint8_t*)win;
  const uint32_t lane = threadIdx.x;
  for (uint32_t i = blockIdx.x; i < nw; i += gridDim.x) {
    const IdxWalk w = walks[i];
    uint64_t pos = w.start, cnt = 0, err = kNone, past = 0;
    if (pos == kNone) {
      if (lane == 0) out[i] = IdxWalkOut{kNone, 0, kNone, 0};
      continue;
    }
    for (;;) {  // pos, and the loop's exits, are uniform over the wave
      if (pos >= w.limit) break;
      if (pos + 8 > n) {  // bytes left, but not a length field
        err = pos;
        past = 1;
        break;
      }
      const uint64_t base = pos & ~15ull;
      // bytes [base, wend) are staged; wend <= n + 16 rounded: inside the padded allocation
      const uint64_t wend = base + kIdxWin + 16 < n ? base + kIdxWin + 16 : ((n + 15) & ~15ull);
      for (uint64_t t = base + 16ull * lane; t < wend; t += 16 * 64)
        win[(t - base) >> 4] = *(const uint4*)(buf + t);
      __syncthreads();
      if (lane == 0) {
        const uint64_t valid = wend < n ? wend : n;  // stream bytes in the window end here
        uint64_t cur = pos;
        uint32_t done = 0;
        while (cur < w.limit) {
          if (cur + 8 > valid) {
            if (cur + 8 > n) {
              err = cur;
              past = 1;
              done = 1;
            }
            break;  // stage again from cur
          }
          const int64_t len = idx_le64(wb + (cur - base));
          if (len < 0 || (uint64_t)len > n - cur - 8 || cnt >= w.cap) {
            err = cur;
            past = len >= 0;
            done = 1;
            break;
          }
          starts[w.slot + cnt++] = cur;
          cur += 8 + (uint64_t)len;
        }
        if (cur >= w.limit) done = 1;
        s_pos = cur;
        s_done = done;
      }
      __syncthreads();
      pos = s_pos;
      const uint32_t done = s_done;
      __syncthreads();  // s_pos / win are rewritten by the next pass
      if (done) break;
    }
    if (lane == 0) out[i] = IdxWalkOut{pos, cnt, err, past};
  }
}

// 8b. Entry decode: a count pass (records and blob bytes per frame, every frame validated), the
// prefix sums, and a fill pass that parses again and writes the entry record, the
// pfscdc_full_datarefs and the strings at the frame's own ranges.  One frame per lane: frames
// are ~250 bytes and independent, a level-0 stream of a large commit has 10^5..10^6 of them.
// A frame that does not parse leaves {0, 0} and its start in *err_min (atomic min: the lowest
// offending offset); index.cpp then never launches the fill.  The fill writes at most the
// count pass's records (idx_parse's cap), so it stays inside its range whatever the bytes.
constexpr int kIdxBlock = 256;

__global__ __launch_bounds__(kIdxBlock) void index_count_kernel(
    const uint8_t* __restrict__ buf, uint64_t n, const uint64_t* __restrict__ fstart, uint64_t nf,
    IdxCount* __restrict__ cnt, unsigned long long* __restrict__ err_min) {
  for (uint64_t f = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; f < nf;
       f += (uint64_t)gridDim.x * kIdxBlock) {
    const uint64_t s = fstart[f];
    IdxCount c{0, 0};
    bool ok = s + 8 <= n;
    if (ok) {
      const int64_t len = idx_le64(buf + s);
      ok = len >= 0 && (uint64_t)len <= n - s - 8;
      IdxFrame fr;
      if (ok) ok = idx_parse(buf + s + 8, buf + s + 8 + len, &fr, nullptr, 0);
      if (ok) ok = idx_blob_bytes(fr) <= 0xffffffffull;
      if (ok) c = IdxCount{idx_records(fr), (uint32_t)idx_blob_bytes(fr)};
    }
    if (!ok) atomicMin(err_min, (unsigned long long)s);
    cnt[f] = c;
  }
}

// Exclusive prefix sums of both counts by one workgroup: tiles of 1,024 frames, a Hillis-Steele
// scan in LDS per tile and the running totals carried in registers.  base[2 f] = records
// before frame f, base[2 f + 1] = blob bytes before it; base[2 nf], base[2 nf + 1] the totals.
constexpr int kIdxScanBlock = 1024;

__global__ __launch_bounds__(kIdxScanBlock) void index_scan_kernel(
    const IdxCount* __restrict__ cnt, uint64_t nf, uint64_t* __restrict__ base) {
  __shared__ uint64_t a[kIdxScanBlock], b[kIdxScanBlock];
  const uint32_t t = threadIdx.x;
  uint64_t ca = 0, cb = 0;
  for (uint64_t f0 = 0; f0 < nf; f0 += kIdxScanBlock) {
    const uint64_t f = f0 + t;
    const IdxCount c = f < nf ? cnt[f] : IdxCount{0, 0};
    a[t] = c.ndr;
    b[t] = c.blob;
    __syncthreads();
    for (uint32_t d = 1; d < kIdxScanBlock; d <<= 1) {
      const uint64_t xa = t >= d ? a[t - d] : 0, xb = t >= d ? b[t - d] : 0;
      __syncthreads();
      a[t] += xa;
      b[t] += xb;
      __syncthreads();
    }
    if (f < nf) {
      base[2 * f] = ca + a[t] - c.ndr;
      base[2 * f + 1] = cb + b[t] - c.blob;
    }
    ca += a[kIdxScanBlock - 1];
    cb += b[kIdxScanBlock - 1];
    __syncthreads();
  }
  if (t == 0) {
    base[2 * nf] = ca;
    base[2 * nf + 1] = cb;
  }
}

__global__ __launch_bounds__(kIdxBlock) void index_fill_kernel(
    const uint8_t* __restrict__ buf, uint64_t n, const uint64_t* __restrict__ fstart, uint64_t nf,
    const uint64_t* __restrict__ base, pfscdc_index_entry* __restrict__ entries,
    pfscdc_full_dataref* __restrict__ drs, char* __restrict__ blob) {
  for (uint64_t f = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; f < nf;
       f += (uint64_t)gridDim.x * kIdxBlock) {
    const uint64_t s = fstart[f];
    const uint64_t first = base[2 * f], cap = base[2 * f + 2] - first;
    const uint64_t at = base[2 * f + 1], room = base[2 * f + 3] - at;
    if (s + 8 > n) continue;  // (the count pass refused such a frame: the fill is not launched)
    const int64_t len = idx_le64(buf + s);
    if (len < 0 || (uint64_t)len > n - s - 8) continue;
    IdxFrame fr;
    if (!idx_parse(buf + s + 8, buf + s + 8 + len, &fr, drs + first, cap)) continue;
    if (idx_records(fr) != cap || idx_blob_bytes(fr) != room) continue;
    idx_emit(fr, first, at, blob, &entries[f]);
  }
}

// Launch widths: one wave per walker, one lane per frame, both up to 8 workgroups' worth of
// waves per CU and capped by the PFSCDC_CHACHA_GRID knob like the gather's (the kernels stride).
hipError_t launch_index_walk(const uint8_t* buf, uint64_t n, const IdxWalk* w, uint32_t nw,
                             uint64_t* starts, IdxWalkOut* out, int num_cus, hipStream_t st) {
  if (nw == 0) return hipSuccess;
  const uint64_t full = (uint64_t)num_cus * 32;
  index_walk_kernel<<<capped_grid(nw < full ? nw : full, Knob::ChachaGrid), 64, 0, st>>>(
      buf, n, w, nw, starts, out);
  return hipGetLastError();
}

hipError_t launch_index_count(const uint8_t* buf, uint64_t n, const uint64_t* fstart, uint64_t nf,
                              IdxCount* cnt, unsigned long long* err_min, int num_cus,
                              hipStream_t st) {
  if (nf == 0) return hipSuccess;
  const uint64_t need = (nf + kIdxBlock - 1) / kIdxBlock, full = (uint64_t)num_cus * 8;
  index_count_kernel<<<capped_grid(need < full ? need : full, Knob::ChachaGrid), kIdxBlock, 0,
                       st>>>(buf, n, fstart, nf, cnt, err_min);
  return hipGetLastError();
}

hipError_t launch_index_scan(const IdxCount* cnt, uint64_t nf, uint64_t* base, hipStream_t st) {
  index_scan_kernel<<<1, kIdxScanBlock, 0, st>>>(cnt, nf, base);
  return hipGetLastError();
}

hipError_t launch_index_fill(const uint8_t* buf, uint64_t n, const uint64_t* fstart, uint64_t nf,
                             const uint64_t* base, pfscdc_index_entry* entries,
                             pfscdc_full_dataref* drs, char* blob, int num_cus, hipStream_t st) {
  if (nf == 0) return hipSuccess;
  const uint64_t need = (nf + kIdxBlock - 1) / kIdxBlock, full = (uint64_t)num_cus * 8;
  index_fill_kernel<<<capped_grid(need < full ? need : full, Knob::ChachaGrid), kIdxBlock, 0,
                      st>>>(buf, n, fstart, nf, base, entries, drs, blob);
  return hipGetLastError();
}

// ---- 9. MergeReader: the index lists of several filesets merged into one ----------------------
// (fileset/merge.go:37-94 iterate / iterateDeletive, :157-164 compare;
// stream/priority_queue.go:103-127: groups of equal keys, ordered by stream)
//
// The streams lie concatenated stream-major (MrgIn).  Every stream is strictly ascending in
// (path, tag), so an entry's place in the merged order is a sum of binary searches:
//   rank(e of stream s at index i) = i + sum_{t > s} lower_bound_t(key e) + sum_{t < s} upper_bound_t(key e)
// which orders equal keys by stream number, the PriorityQueue's order.  Keys compare as
// strings.Compare: unsigned bytes, a proper prefix first, the path and then the tag.
// 9a rank: one lane per entry, one compare against its predecessor (a stream out of order sets
//    *bad: the ranks are then no permutation and index.cpp hands the call to the host arm).
// 9b group: one lane per merged position; a position whose key differs from its predecessor's
//    is a head, walks its group (at most one entry per stream) and leaves what it emits.
// 9c scan: index_scan_kernel's shape with three running sums (entries, records, blob bytes).
// 9d fill: one lane per emitting head writes the entry, its strings, and one MrgCopy per
//    contributing source entry; it walks the group as 9b did and writes nothing unless its
//    counts equal the ranges the prefix sums gave it.
// 9e copy: the DataRefs (128 B each, the bulk of the bytes) in 16-byte pieces, 8 neighbouring
//    lanes per source entry.
struct MrgKey {
  const uint8_t *p, *t;
  uint32_t pn, tn;
};

__device__ inline uint32_t mrg_stream(const MrgIn& in, uint64_t g) {
  // the last s with stream_begin[s] <= g (stream_begin[0] = 0, stream_begin[ns] = n > g)
  uint32_t lo = 0, hi = in.ns;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (in.stream_begin[mid] <= g) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ inline MrgKey mrg_key(const MrgIn& in, uint64_t g, uint32_t s) {
  const pfscdc_index_entry& e = in.entries[g];
  const uint8_t* b = (const uint8_t*)in.blob + in.blob_base[s];
  return MrgKey{b + e.path_off, b + e.tag_off, e.path_len, e.tag_len};
}

__device__ inline int mrg_cmp_str(const uint8_t* a, uint32_t an, const uint8_t* b, uint32_t bn) {
  const uint32_t k = an < bn ? an : bn;
  for (uint32_t i = 0; i < k; i++)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return an < bn ? -1 : an > bn ? 1 : 0;
}

__device__ inline int mrg_cmp(const MrgKey& a, const MrgKey& b) {
  const int c = mrg_cmp_str(a.p, a.pn, b.p, b.pn);
  return c ? c : mrg_cmp_str(a.t, a.tn, b.t, b.tn);
}

// What the fill kernels of the list passes share (the contract is in list_kernels.h).
// s[0, n) and a NUL at blob + at; the place after them
PFS_DEV uint64_t put_str(char* blob, uint64_t at, const char* s, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) blob[at + i] = s[i];
  blob[at + n] = 0;
  return at + n + 1;
}

// o's path, tag and LastPath from src, where its offsets point, to blob + at, where they then point
PFS_DEV void put_entry_strings(pfscdc_index_entry& o, const char* src, char* blob, uint64_t at) {
  const uint64_t tag = put_str(blob, at, src + o.path_off, o.path_len);
  const uint64_t last = put_str(blob, tag, src + o.tag_off, o.tag_len);
  put_str(blob, last, src + o.last_path_off, o.last_path_len);
  o.path_off = at;
  o.tag_off = tag;
  o.last_path_off = last;
}

// item i's ranges in the prefix sums are what it counts: else it writes nothing
PFS_DEV bool ranges_are(const uint64_t* base, uint64_t i, MrgCount c) {
  return base[3 * i + 3] - base[3 * i] == c.emit && base[3 * i + 4] - base[3 * i + 1] == c.recs &&
         base[3 * i + 5] - base[3 * i + 2] == c.blob;
}

__global__ __launch_bounds__(kIdxBlock) void merge_rank_kernel(MrgIn in,
                                                               uint32_t* __restrict__ order,
                                                               uint32_t* __restrict__ bad) {
  for (uint64_t g = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; g < in.n;
       g += (uint64_t)gridDim.x * kIdxBlock) {
    const uint32_t s = mrg_stream(in, g);
    const MrgKey key = mrg_key(in, g, s);
    uint64_t rank = g - in.stream_begin[s];
    if (rank > 0 && mrg_cmp(mrg_key(in, g - 1, s), key) >= 0) atomicOr(bad, 1u);
    for (uint32_t t = 0; t < in.ns; t++) {
      if (t == s) continue;
      const uint64_t b = in.stream_begin[t];
      uint64_t lo = b, hi = in.stream_begin[t + 1];
      while (lo < hi) {  // t > s: the entries below key; t < s: those not above it
        const uint64_t mid = lo + (hi - lo) / 2;
        const int c = mrg_cmp(mrg_key(in, mid, t), key);
        if (t > s ? c < 0 : c <= 0) lo = mid + 1;
        else hi = mid;
      }
      rank += lo - b;
    }
    order[rank] = (uint32_t)g;  // rank < n whatever the streams hold: every term is a count
  }
}

struct MrgGroup {
  uint32_t emit, merged;
  uint64_t recs, blob;
  int64_t size;
};

// The group that begins at merged position p.  copy (nullable): the MrgCopy of every source
// entry whose DataRefs the group keeps, laid out from record first on, written only if the
// group's records are cap in all (what the count pass found).
__device__ inline MrgGroup mrg_walk(const MrgIn& in, const uint32_t* __restrict__ order, uint64_t p,
                                    MrgCopy* __restrict__ copy, uint64_t first, uint64_t cap) {
  const uint64_t g0 = order[p];
  const uint32_t s0 = mrg_stream(in, g0);
  const pfscdc_index_entry& e0 = in.entries[g0];
  const MrgKey k0 = mrg_key(in, g0, s0);
  const bool files = in.mode == PFSCDC_MERGE_FILES;  // stream 2k: fileset k's deletive list
  uint64_t q = p + 1, from = (files && s0 % 2 == 0) ? p + 1 : p;  // members [from, q) are kept
  for (; q < in.n; q++) {
    const uint64_t g = order[q];
    const uint32_t s = mrg_stream(in, g);
    if (mrg_cmp(mrg_key(in, g, s), k0) != 0) break;
    if (files && s % 2 == 0) from = q + 1;
  }
  MrgGroup r{0, 0, 0, 0, 0};
  r.blob = (uint64_t)e0.path_len + e0.tag_len + e0.last_path_len + 3;
  if (!files || q - p == 1) {  // the first entry as it is (iterate: a lone deletive entry: nothing)
    if (files && s0 % 2 == 0) return r;
    r.emit = 1;
    r.recs = (uint64_t)e0.count + ((e0.flags & PFSCDC_IDX_HAS_CHUNK_REF) ? 1u : 0u);
    r.size = e0.size_bytes;
    if (copy && r.recs && r.recs == cap)
      copy[g0] = MrgCopy{(uint32_t)first, (uint32_t)r.recs, (uint32_t)(in.dr_base[s0] + e0.first), 0};
    return r;
  }
  if (from == q) return r;  // a deletive entry in last place drops the file
  r.emit = r.merged = 1;
  uint64_t size = 0;
  for (uint64_t m = from; m < q; m++) {
    const pfscdc_index_entry& e = in.entries[order[m]];
    r.recs += e.count;
    size += (uint64_t)e.size_bytes;  // an entry's size_bytes is its File DataRefs' wrapping sum
  }
  r.size = (int64_t)size;
  if (copy && r.recs == cap) {
    uint64_t at = first;
    for (uint64_t m = from; m < q; m++) {
      const uint64_t g = order[m];
      const pfscdc_index_entry& e = in.entries[g];
      if (e.count)
        copy[g] = MrgCopy{(uint32_t)at, e.count, (uint32_t)(in.dr_base[mrg_stream(in, g)] + e.first), 0};
      at += e.count;
    }
  }
  return r;
}

__global__ __launch_bounds__(kIdxBlock) void merge_group_kernel(MrgIn in,
                                                                const uint32_t* __restrict__ order,
                                                                MrgCount* __restrict__ cnt,
                                                                unsigned long long* __restrict__ heads) {
  unsigned long long mine = 0;
  for (uint64_t p = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; p < in.n;
       p += (uint64_t)gridDim.x * kIdxBlock) {
    const uint64_t g = order[p];
    bool head = p == 0;
    if (!head) {
      const uint64_t h = order[p - 1];
      head = mrg_cmp(mrg_key(in, h, mrg_stream(in, h)), mrg_key(in, g, mrg_stream(in, g))) != 0;
    }
    MrgCount c{0, 0, 0};
    if (head) {
      mine++;
      const MrgGroup r = mrg_walk(in, order, p, nullptr, 0, 0);
      if (r.emit) c = MrgCount{1, (uint32_t)r.recs, r.blob};  // recs <= the input's, < 2^32
    }
    cnt[p] = c;
  }
  if (mine) atomicAdd(heads, mine);
}

// Exclusive prefix sums of the three counts by one workgroup, as index_scan_kernel does two:
// base[3 p], base[3 p + 1], base[3 p + 2] = entries, records, blob bytes before position p;
// base[3 n ...] the totals.
__global__ __launch_bounds__(kIdxScanBlock) void merge_scan_kernel(
    const MrgCount* __restrict__ cnt, uint64_t n, uint64_t* __restrict__ base) {
  __shared__ uint64_t a[kIdxScanBlock], b[kIdxScanBlock], c[kIdxScanBlock];
  const uint32_t t = threadIdx.x;
  uint64_t ca = 0, cb = 0, cc = 0;
  for (uint64_t f0 = 0; f0 < n; f0 += kIdxScanBlock) {
    const uint64_t f = f0 + t;
    const MrgCount x = f < n ? cnt[f] : MrgCount{0, 0, 0};
    a[t] = x.emit;
    b[t] = x.recs;
    c[t] = x.blob;
    __syncthreads();
    for (uint32_t d = 1; d < kIdxScanBlock; d <<= 1) {
      const uint64_t xa = t >= d ? a[t - d] : 0, xb = t >= d ? b[t - d] : 0,
                     xc = t >= d ? c[t - d] : 0;
      __syncthreads();
      a[t] += xa;
      b[t] += xb;
      c[t] += xc;
      __syncthreads();
    }
    if (f < n) {
      base[3 * f] = ca + a[t] - x.emit;
      base[3 * f + 1] = cb + b[t] - x.recs;
      base[3 * f + 2] = cc + c[t] - x.blob;
    }
    ca += a[kIdxScanBlock - 1];
    cb += b[kIdxScanBlock - 1];
    cc += c[kIdxScanBlock - 1];
    __syncthreads();
  }
  if (t == 0) {
    base[3 * n] = ca;
    base[3 * n + 1] = cb;
    base[3 * n + 2] = cc;
  }
}

__global__ __launch_bounds__(kIdxBlock) void merge_fill_kernel(
    MrgIn in, const uint32_t* __restrict__ order, const MrgCount* __restrict__ cnt,
    const uint64_t* __restrict__ base, pfscdc_index_entry* __restrict__ entries,
    char* __restrict__ blob, MrgCopy* __restrict__ copy) {
  for (uint64_t p = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; p < in.n;
       p += (uint64_t)gridDim.x * kIdxBlock) {
    if (!cnt[p].emit) continue;
    const uint64_t oi = base[3 * p], first = base[3 * p + 1], cap = base[3 * p + 4] - first;
    if (base[3 * p + 3] - oi != 1) continue;
    const MrgGroup r = mrg_walk(in, order, p, copy, first, cap);
    // (never: the count pass's walk; recs compared in full, as cnt[] holds its low 32 bits)
    if (!r.emit || r.recs != cap || !ranges_are(base, p, MrgCount{1, (uint32_t)cap, r.blob}))
      continue;
    const uint64_t g0 = order[p];
    const pfscdc_index_entry e0 = in.entries[g0];
    pfscdc_index_entry o = e0;
    put_entry_strings(o, in.blob + in.blob_base[mrg_stream(in, g0)], blob, base[3 * p + 2]);
    o.first = (uint32_t)first;
    if (r.merged) {  // mergeIdx: the group's first entry with the merged File.DataRefs
      o.flags = (e0.flags & ~(PFSCDC_IDX_HAS_CHUNK_REF | PFSCDC_IDX_HAS_RANGE)) | PFSCDC_IDX_HAS_FILE;
      o.count = (uint32_t)r.recs;
      o.size_bytes = r.size;
    }
    entries[oi] = o;
  }
}

__global__ __launch_bounds__(kIdxBlock) void merge_copy_kernel(
    const uint4* __restrict__ src, const MrgCopy* __restrict__ copy, uint64_t n,
    uint4* __restrict__ dst) {
  for (uint64_t w = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; w < n * 8;
       w += (uint64_t)gridDim.x * kIdxBlock) {
    const MrgCopy c = copy[w >> 3];
    const uint32_t l = (uint32_t)(w & 7);  // 8 lanes x 16 B = one pfscdc_full_dataref
    for (uint64_t r = 0; r < c.recs; r++) dst[((uint64_t)c.dst + r) * 8 + l] = src[((uint64_t)c.src + r) * 8 + l];
  }
}

static unsigned merge_grid(uint64_t items, int num_cus) {
  const uint64_t need = (items + kIdxBlock - 1) / kIdxBlock, full = (uint64_t)num_cus * 8;
  return capped_grid(need < full ? need : full, Knob::ChachaGrid);
}

hipError_t launch_merge_rank(const MrgIn& in, uint32_t* order, uint32_t* bad, int num_cus,
                             hipStream_t st) {
  if (in.n == 0) return hipSuccess;
  merge_rank_kernel<<<merge_grid(in.n, num_cus), kIdxBlock, 0, st>>>(in, order, bad);
  return hipGetLastError();
}

hipError_t launch_merge_group(const MrgIn& in, const uint32_t* order, MrgCount* cnt,
                              unsigned long long* heads, int num_cus, hipStream_t st) {
  if (in.n == 0) return hipSuccess;
  merge_group_kernel<<<merge_grid(in.n, num_cus), kIdxBlock, 0, st>>>(in, order, cnt, heads);
  return hipGetLastError();
}

hipError_t launch_merge_scan(const MrgCount* cnt, uint64_t n, uint64_t* base, hipStream_t st) {
  merge_scan_kernel<<<1, kIdxScanBlock, 0, st>>>(cnt, n, base);
  return hipGetLastError();
}

hipError_t launch_merge_fill(const MrgIn& in, const uint32_t* order, const MrgCount* cnt,
                             const uint64_t* base, pfscdc_index_entry* entries, char* blob,
                             MrgCopy* copy, int num_cus, hipStream_t st) {
  if (in.n == 0) return hipSuccess;
  merge_fill_kernel<<<merge_grid(in.n, num_cus), kIdxBlock, 0, st>>>(in, order, cnt, base, entries,
                                                                    blob, copy);
  return hipGetLastError();
}

hipError_t launch_list_copy(const pfscdc_full_dataref* src, const MrgCopy* copy, uint64_t n,
                            pfscdc_full_dataref* dst, int num_cus, hipStream_t st) {
  if (n == 0) return hipSuccess;
  merge_copy_kernel<<<merge_grid(n * 8, num_cus), kIdxBlock, 0, st>>>((const uint4*)src, copy, n,
                                                                     (uint4*)dst);
  return hipGetLastError();
}

// ---- 10. GetFileTAR over a device-resident list ------------------------------------------------
// tar_plan (tar.cpp) restated for a list whose entries, strings and DataRefs lie on the device, so
// that a window renders with nothing per file or per DataRef crossing to the host.
//
// Plan, once per list:
//  10a sizes    one lane per DataRef: StoreBatch::valid's rule, dsz[k] = SizeBytes.
//  10b scan     dpre = prefix sums of dsz (one workgroup, index_scan_kernel's shape, the add
//               saturating at kRtarCap so no sum wraps): a file's size is a difference of two
//               prefixes, whatever its DataRef count, and a piece's place in its file another.
//  10c entries  one lane per entry: the packed layout (first = the first + count of the entry
//               before, the last ends at nr) so that a DataRef's file is found by a search;
//               tar_name_check over the path in the blob; the TarEntry record (name_off =
//               path_off: the blob is the name table) and the span.  The lowest refused entry
//               and its reason leave through one atomic minimum.
//  10b again    offsets = prefix sums of the spans, written into the TarEntry records as well;
//               with PAX allowed (pfscdc_set_tar_format) once more over the entries' head blocks
//               other than the main header: xblk, what tar_frame_kernel finds such a block by.
// Window, per call:
//  10d window   one lane: the entries [i0, i1) that meet [begin, end) by two searches in the
//               offsets, and their DataRefs [k0, k1).
//  10e pieces   one lane per DataRef of [k0, k1) (a 300-DataRef file is 300 lanes, not a loop):
//               its file by a search in the entries' first (the last entry with first <= k, which
//               skips entries of count 0), its place p = off + head + dpre[k] - dpre[first]
//               (head: tar_head_len, 512 for a USTAR entry), the
//               clip to the window as TarPiece.  A non-empty piece is a run head when the DataRef
//               before it gave no piece or names another chunk or another size of it.  Count pass, merge_scan_kernel
//               over {piece, head, keystream blocks}, fill pass: the dense arrays
//               chacha_slice_gather_kernel takes, slice.chunk = the run's number, and one record
//               per run for the host, which alone knows the store.
//  10f chunks   slice.chunk = table[run] once the host has looked the runs' chunks up, and each
//               slice held against its chunk's stored length: the gather checks no bounds.
// Every kernel strides; widths as §9's (merge_grid: capped by the PFSCDC_CHACHA_GRID knob).

// What kind of level a decoded list is, without the list leaving the device: flags[0] |= and
// flags[1] &= every entry's flags (a wave reduces first; one atomic pair per wave).
__global__ __launch_bounds__(kIdxBlock) void index_flags_kernel(
    const pfscdc_index_entry* __restrict__ entries, uint64_t n, uint32_t* __restrict__ flags) {
  uint32_t any = 0, all = ~0u;
  for (uint64_t i = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kIdxBlock) {
    any |= entries[i].flags;
    all &= entries[i].flags;
  }
  for (int o = 32; o > 0; o >>= 1) {
    any |= (uint32_t)__shfl_xor((int)any, o, 64);
    all &= (uint32_t)__shfl_xor((int)all, o, 64);
  }
  if ((threadIdx.x & 63u) == 0) {
    atomicOr(&flags[0], any);
    atomicAnd(&flags[1], all);
  }
}

hipError_t launch_index_flags(const pfscdc_index_entry* entries, uint64_t n, uint32_t* flags,
                              int num_cus, hipStream_t st) {
  if (n == 0) return hipSuccess;
  index_flags_kernel<<<merge_grid(n, num_cus), kIdxBlock, 0, st>>>(entries, n, flags);
  return hipGetLastError();
}

PFS_DEV uint64_t rtar_sat_add(uint64_t a, uint64_t b) {  // a, b <= kRtarCap
  const uint64_t s = a + b;
  return s < kRtarCap ? s : kRtarCap;
}

__global__ __launch_bounds__(kIdxBlock) void rtar_sizes_kernel(
    const pfscdc_full_dataref* __restrict__ drs, uint64_t nr, uint64_t* __restrict__ dsz,
    uint32_t* __restrict__ bad) {
  for (uint64_t k = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; k < nr;
       k += (uint64_t)gridDim.x * kIdxBlock) {
    const int64_t rs = drs[k].ref_size, ob = drs[k].data.offset_bytes, sb = drs[k].data.size_bytes;
    const bool ok = rs >= 0 && ob >= 0 && sb >= 0 && ob <= rs && sb <= rs - ob;
    if (!ok) atomicOr(bad, 1u);
    dsz[k] = !ok ? 0 : (uint64_t)sb < kRtarCap ? (uint64_t)sb : kRtarCap;
  }
}

__global__ __launch_bounds__(kIdxScanBlock) void rtar_scan_kernel(
    const uint64_t* __restrict__ in, uint64_t n, uint64_t* __restrict__ out,
    TarEntry* __restrict__ ent) {
  __shared__ uint64_t a[kIdxScanBlock];
  const uint32_t t = threadIdx.x;
  uint64_t carry = 0;
  for (uint64_t f0 = 0; f0 < n; f0 += kIdxScanBlock) {
    const uint64_t f = f0 + t;
    a[t] = f < n ? in[f] : 0;
    __syncthreads();
    for (uint32_t d = 1; d < kIdxScanBlock; d <<= 1) {
      const uint64_t x = t >= d ? a[t - d] : 0;
      __syncthreads();
      a[t] = rtar_sat_add(a[t], x);
      __syncthreads();
    }
    if (f < n) {  // exclusive: the inclusive sum of the lane before
      const uint64_t v = rtar_sat_add(carry, t ? a[t - 1] : 0);
      out[f] = v;
      if (ent) ent[f].off = v;
    }
    const uint64_t next = rtar_sat_add(carry, a[kIdxScanBlock - 1]);
    __syncthreads();
    carry = next;
  }
  if (t == 0) out[n] = carry;
}

__global__ __launch_bounds__(kIdxBlock) void rtar_entries_kernel(
    RtarList l, const uint64_t* __restrict__ dpre, int format, TarEntry* __restrict__ ent,
    uint64_t* __restrict__ span, uint64_t* __restrict__ xb, unsigned long long* __restrict__ err) {
  for (uint64_t i = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; i < l.n;
       i += (uint64_t)gridDim.x * kIdxBlock) {
    const pfscdc_index_entry e = l.entries[i];
    const uint64_t first = e.first, count = e.count;
    uint64_t len = e.path_len;
    uint32_t why = 0;
    uint64_t z = 0;
    int32_t split = -1;
    if (first > l.nr || count > l.nr - first) {
      why = kRtarBeyond;
    } else {
      const uint64_t want = i ? (uint64_t)l.entries[i - 1].first + l.entries[i - 1].count : 0;
      if (first != want || (i + 1 == l.n && first + count != l.nr)) why = kRtarNotPacked;
    }
    if (!why && (e.path_off > l.nb || len >= l.nb - e.path_off)) why = kRtarString;
    if (!why) {
      const uint64_t hi = dpre[first + count];
      z = hi - dpre[first];
      if (hi >= kRtarCap) why = kRtarOverflow;
    }
    if (!why) {  // tar_name_check, then tar_plan's directory rule
      const uint8_t* name = (const uint8_t*)l.blob + e.path_off;
      // the host reads the path as a C string: a path with a NUL inside ends there in both arms
      for (uint64_t k = 0; k < len; k++)
        if (name[k] == 0) len = k;
      if (len == 0) {
        why = kRtarEmpty;
      } else if (name[len - 1] == '/' && z) {
        why = kRtarDirContent;
      } else {
        for (uint64_t k = 0; k < len && !why; k++)
          if (name[k] >= 0x80) why = kRtarNotAscii;
        if (!why && z > kTarMaxSize) why = kRtarTooBig;
        if (!why && len > 100) {  // splitUSTARPath
          uint64_t lim = len < 156 ? len : 156;
          if (len <= 156 && name[len - 1] == '/') lim = len - 1;
          uint64_t k = lim;
          while (k > 0 && name[k - 1] != '/') k--;
          if (k < 2 || len - k > 100 || len - k == 0 || k - 1 > 155) why = kRtarNoSplit;
          else split = (int32_t)(k - 1);
        }
        if (why && (format & PFSCDC_TAR_PAX)) {  // tar_name_check's PAX arm
          if (len > kTarMaxName) {
            why = kRtarPaxLong;
          } else if (!tar_name_joins(name, (uint32_t)len)) {
            why = kRtarPaxJoin;
          } else {
            split = why == kRtarNotAscii || len > 100 ? kTarPaxPath : kTarPaxSize;
            why = 0;
          }
        }
        if (!why && name[len - 1] == '/' && count) why = kRtarDirPieces;
      }
    }
    if (why) atomicMin(err, (unsigned long long)(i << 8 | why));
    ent[i] = TarEntry{0, z, (uint32_t)e.path_off, (uint16_t)len, (int16_t)split};
    const uint64_t head = tar_head_len((uint32_t)(len & 0xffff), z, split);
    span[i] = why ? 0 : head + ((z + 511) & ~511ull);
    if (xb) xb[i] = why ? 0 : head / 512 - 1;
  }
}

__global__ void rtar_window_kernel(RtarList l, const uint64_t* __restrict__ off,
                                   const uint64_t* __restrict__ xblk, uint64_t begin,
                                   uint64_t end, RtarWindow* __restrict__ w,
                                   uint64_t* __restrict__ nx) {
  if (blockIdx.x || threadIdx.x) return;
  uint64_t lo = 0, hi = l.n + 1;  // the first i of off[0, n] with off[i] > begin
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (off[mid] > begin) hi = mid;
    else lo = mid + 1;
  }
  const uint64_t i0 = lo ? lo - 1 : 0;  // the entry (or the trailer, i0 = n) that holds begin
  lo = i0 < l.n ? i0 : l.n;
  hi = l.n;  // the first i >= i0 of off[0, n) with off[i] >= end
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (off[mid] >= end) hi = mid;
    else lo = mid + 1;
  }
  RtarWindow r{i0 < l.n ? i0 : l.n, lo, 0, 0};
  if (xblk) *nx = r.i0 < r.i1 ? xblk[r.i1] - xblk[r.i0] : 0;
  if (r.i0 < r.i1) {
    r.k0 = l.entries[r.i0].first;
    r.k1 = (uint64_t)l.entries[r.i1 - 1].first + l.entries[r.i1 - 1].count;
  }
  *w = r;
}

struct RtarClip {
  uint64_t offset, size, out_off;  // size 0: no piece
};
// DataRef k of the window's entries, clipped as TarPiece (tar_plan)
PFS_DEV RtarClip rtar_clip(const RtarPieces& p, uint64_t k) {
  uint64_t lo = p.w.i0, hi = p.w.i1;  // the last entry with first <= k
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (p.l.entries[mid].first <= k) lo = mid;
    else hi = mid;
  }
  const TarEntry en = p.ent[lo];
  const uint64_t at = en.off + tar_head_len(en.name_len, en.size, en.split) +
                      (p.dpre[k] - p.dpre[p.l.entries[lo].first]);
  const uint64_t sz = p.dpre[k + 1] - p.dpre[k];
  const uint64_t a = at > p.begin ? at : p.begin, b = at + sz < p.end ? at + sz : p.end;
  if (a >= b) return RtarClip{0, 0, 0};
  return RtarClip{(uint64_t)p.l.drs[k].data.offset_bytes + (a - at), b - a, a - p.begin};
}

// Same Ref.Id and same Ref.SizeBytes: the host compares a run's ref_size with the stored
// chunk's length once, for its head, so a DataRef that claims another size for the same id must
// head a run of its own (StoreBatch::add then refuses it as pfscdc_store_read_tar does).
PFS_DEV bool rtar_same_chunk(const pfscdc_full_dataref* a, const pfscdc_full_dataref* b) {
  const uint64_t *x = (const uint64_t*)a->ref.id, *y = (const uint64_t*)b->ref.id;
  return x[0] == y[0] && x[1] == y[1] && x[2] == y[2] && x[3] == y[3] &&
         a->ref_size == b->ref_size;
}

__global__ __launch_bounds__(kIdxBlock) void rtar_pieces_kernel(
    RtarPieces p, MrgCount* __restrict__ cnt, const uint64_t* __restrict__ base,
    pfscdc_slice* __restrict__ slices, uint64_t* __restrict__ out_off,
    uint64_t* __restrict__ blk_base, RtarRun* __restrict__ runs) {
  const uint64_t nk = p.w.k1 - p.w.k0;
  for (uint64_t q = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; q < nk;
       q += (uint64_t)gridDim.x * kIdxBlock) {
    const uint64_t k = p.w.k0 + q;
    const RtarClip c = rtar_clip(p, k);
    MrgCount x{0, 0, 0};
    if (c.size) {
      x.emit = 1;
      x.blob = (c.offset + c.size - 1) / 64 - c.offset / 64 + 1;
      x.recs = q == 0 || !rtar_same_chunk(&p.l.drs[k], &p.l.drs[k - 1]) ||
               rtar_clip(p, k - 1).size == 0;
    }
    if (!slices) {
      cnt[q] = x;
      continue;
    }
    if (q == 0) {  // the arrays' last entries: the totals
      const uint64_t m = base[3 * nk];
      out_off[m] = p.end - p.begin;
      blk_base[m] = base[3 * nk + 2];
    }
    if (!c.size) continue;
    const uint64_t j = base[3 * q], r = base[3 * q + 1] + x.recs - 1;
    if (base[3 * q + 3] - j != 1) continue;  // (never: the count pass's clip)
    slices[j] = pfscdc_slice{(uint32_t)r, 0, c.offset, c.size};
    out_off[j] = c.out_off;
    blk_base[j] = base[3 * q + 2];
    if (x.recs) {
      const pfscdc_full_dataref* dr = &p.l.drs[k];
      RtarRun run;
      run.ref = dr->ref;
      run.ref_size = dr->ref_size;
      run.first_piece = (uint32_t)j;
      run.reserved = 0;
      runs[r] = run;
    }
  }
}

// The gather checks no bounds, so the last word before it is said here: a slice that does not
// lie inside its chunk's stored bytes (chunk_offs: the batch's nchunks + 1 offsets) sets *bad.
__global__ __launch_bounds__(kIdxBlock) void rtar_chunks_kernel(
    pfscdc_slice* __restrict__ slices, uint64_t m, const uint32_t* __restrict__ table,
    const uint64_t* __restrict__ chunk_offs, uint32_t nchunks, uint32_t* __restrict__ bad) {
  for (uint64_t j = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; j < m;
       j += (uint64_t)gridDim.x * kIdxBlock) {
    const pfscdc_slice sl = slices[j];
    const uint32_t c = table[sl.chunk];
    bool ok = c < nchunks;
    if (ok) {
      const uint64_t len = chunk_offs[c + 1] - chunk_offs[c];
      ok = sl.offset <= len && sl.size <= len - sl.offset;
    }
    if (!ok) atomicOr(bad, 1u);
    slices[j].chunk = ok ? c : 0u;
  }
}

hipError_t launch_rtar_sizes(const pfscdc_full_dataref* drs, uint64_t nr, uint64_t* dsz,
                             uint32_t* bad, int num_cus, hipStream_t st) {
  if (nr == 0) return hipSuccess;
  rtar_sizes_kernel<<<merge_grid(nr, num_cus), kIdxBlock, 0, st>>>(drs, nr, dsz, bad);
  return hipGetLastError();
}

hipError_t launch_rtar_scan(const uint64_t* in, uint64_t n, uint64_t* out, TarEntry* ent,
                            hipStream_t st) {
  rtar_scan_kernel<<<1, kIdxScanBlock, 0, st>>>(in, n, out, ent);
  return hipGetLastError();
}

hipError_t launch_rtar_entries(const RtarList& l, const uint64_t* dpre, int format, TarEntry* ent,
                               uint64_t* span, uint64_t* xb, unsigned long long* err, int num_cus,
                               hipStream_t st) {
  if (l.n == 0) return hipSuccess;
  rtar_entries_kernel<<<merge_grid(l.n, num_cus), kIdxBlock, 0, st>>>(l, dpre, format, ent, span,
                                                                       xb, err);
  return hipGetLastError();
}

hipError_t launch_rtar_window(const RtarList& l, const uint64_t* off, const uint64_t* xblk,
                              uint64_t begin, uint64_t end, RtarWindow* w, uint64_t* nx,
                              hipStream_t st) {
  rtar_window_kernel<<<1, 64, 0, st>>>(l, off, xblk, begin, end, w, nx);
  return hipGetLastError();
}

hipError_t launch_rtar_pieces(const RtarPieces& p, MrgCount* cnt, const uint64_t* base,
                              pfscdc_slice* slices, uint64_t* out_off, uint64_t* blk_base,
                              RtarRun* runs, int num_cus, hipStream_t st) {
  if (p.w.k1 <= p.w.k0) return hipSuccess;
  rtar_pieces_kernel<<<merge_grid(p.w.k1 - p.w.k0, num_cus), kIdxBlock, 0, st>>>(
      p, cnt, base, slices, out_off, blk_base, runs);
  return hipGetLastError();
}

hipError_t launch_rtar_chunks(pfscdc_slice* slices, uint64_t m, const uint32_t* table,
                              const uint64_t* chunk_offs, uint32_t nchunks, uint32_t* bad, int num_cus,
                              hipStream_t st) {
  if (m == 0) return hipSuccess;
  rtar_chunks_kernel<<<merge_grid(m, num_cus), kIdxBlock, 0, st>>>(slices, m, table, chunk_offs,
                                                                    nchunks, bad);
  return hipGetLastError();
}

// ---- 11. The Source: directory entries, path filters and FileInfo ------------------------------
// (fileset/dir_inserter.go:22-58 emit / parentOf, fileset/transforms.go:31-49 indexFilter,
// server/pfs/server/source.go:45-145 Iterate / computeFileInfo; source.cpp takes them literally)
//
// Directory insertion without the running lastPath.  emit(p) inserts parent = Clean(parentOf(p),
// true) exactly when lastPath < parent, recursively, so the directories put in front of p are its
// ancestors a (every prefix p[0..k] with p[k] == '/', k < len - 1: the entry itself is not its own
// ancestor) with lastPath < a, lastPath being the entry emitted before.  Claim: for a list of
// clean paths in ascending order, with q the input entry before p, lastPath < a <=> a is not a
// prefix of q <=> k >= lcp(q, p).  Proof: (1) if a is a prefix of q, then q >= a, and every entry
// emitted since q (q's own and then p's shorter ancestors, each a prefix of p, emitted in
// ascending length) is >= a too or is a itself already emitted; in either case lastPath >= a.
// (2) if a is not a prefix of q: q <= p and a is a prefix of p.  Were q >= a, then a <= q <= p
// with a a prefix of p but not of q; at the first byte where q and a differ (q is no proper
// prefix of a, else q < a) q holds the larger byte, so q > every string with prefix a, p
// included: contradiction.  So q < a; the ancestors of p emitted after q and before a are proper
// prefixes of a, hence < a.  So lastPath < a.  (3) a is a prefix of q iff its k + 1
// bytes lie inside the common prefix, k < lcp.  For the first entry lastPath = "" < every
// ancestor: lcp = 0.  The same argument shows that the output is ascending, so a directory's
// subtree (the paths with its prefix) lies contiguously after it, and since each of the four
// predicates selects a selected directory's subtree whole, computeFileInfo's recursion over the
// second iterator with its cache reduces to: a directory's children are the entries of the next
// depth inside its subtree, in order (tests/source_oracle.py holds both against the literal
// forms).
// 11a count  one lane per input entry: order and cleanliness against its predecessor (flags for
//     the host arm), lcp, the new ancestors and the entry itself under the predicate:
//     {entries, DataRefs, blob bytes} it emits.
// 11b scan   merge_scan_kernel as it is.
// 11c fill   one lane per input entry writes its directories and itself at its own ranges
//     (nothing unless its counts equal them), one MrgCopy per selected file for
//     merge_copy_kernel, and per output entry {source, depth}, type, flags and its file size.
// 11d tree   one lane per output entry: a directory's subtree end by a search for the first path
//     without its prefix; its size a difference of the prefix sums of the file sizes (wrapping).
// 11e leaf   the files' DataRef hashes packed 32 bytes apart, one segment per entry, for one
//     blake2b_kernel launch (or the caller's leaf hashes copied in).
// 11f level  per depth L, deepest first: {entry of depth L + 1, directory of depth L} counted and
//     prefix-summed (merge_scan_kernel); the children's hashes gathered at 32 x their number
//     among the entries of depth L + 1 (every such entry between a directory and its subtree's
//     end is its child), one segment per directory; one blake2b_kernel launch; the digests
//     scattered into the infos, where level L - 1 reads them.
PFS_DEV bool src_selected(const SrcPred& p, const uint8_t* s, uint32_t n) {
  if (p.all) return true;
  bool eq = n == p.name_len, pre = n >= p.dir_len;
  for (uint32_t k = 0; eq && k < n; k++) eq = s[k] == (uint8_t)p.name[k];
  for (uint32_t k = 0; pre && k < p.dir_len; k++) pre = s[k] == (uint8_t)p.dir[k];
  if (!eq && !pre) return false;
  return !(p.exclude_dir && pre && n == p.dir_len);
}

// pathIsChild(name, cleanPath(path)) for a clean path (paths.go:39-46)
PFS_DEV uint32_t src_child(const SrcPred& p, const uint8_t* s, uint32_t n) {
  if (!p.child_flag) return 0;
  const uint32_t cn = (n > 1 && s[n - 1] == '/') ? n - 1 : n;
  if (cn < p.name_len) return 0;
  for (uint32_t k = 0; k < p.name_len; k++)
    if (s[k] != (uint8_t)p.name[k]) return 0;
  uint32_t a = p.name_len, b = cn;
  while (a < b && s[a] == '/') a++;
  while (b > a && s[b - 1] == '/') b--;
  for (uint32_t k = a; k < b; k++)
    if (s[k] == '/') return 0;
  return PFSCDC_INFO_CHILD;
}

PFS_DEV bool src_entry_ok(const RtarList& in, const pfscdc_index_entry& e) {
  return e.path_off <= in.nb && e.path_len <= in.nb - e.path_off && e.tag_off <= in.nb &&
         e.tag_len <= in.nb - e.tag_off && e.last_path_off <= in.nb &&
         e.last_path_len <= in.nb - e.last_path_off && e.first <= in.nr &&
         e.count <= in.nr - e.first;
}

// IsClean(p, false) for s[0, n): rooted, no empty component, none of "." or ".."; with
// allow_trailing_slash IsClean(p, IsDir(p)): the last component may be empty
PFS_DEV bool path_is_clean(const uint8_t* s, uint32_t n, bool allow_trailing_slash) {
  return n > 0 && s[0] == '/' && path_components_clean(s, n, 1, allow_trailing_slash);
}

// Entry i > 0 (e, inside the arrays) against the entry before it.  false and kSrcMalformed in
// *bad: that one lies outside the arrays.  Else *bad |= kSrcUnordered if it is above e by path,
// then tag; *lcp the two paths' common prefix, *same whether they are one path.
PFS_DEV bool src_follows(const RtarList& in, uint64_t i, const pfscdc_index_entry& e, uint32_t* bad,
                         uint32_t* lcp, bool* same) {
  const pfscdc_index_entry q = in.entries[i - 1];
  if (!src_entry_ok(in, q)) {
    *bad |= kSrcMalformed;
    return false;
  }
  const uint8_t* s = (const uint8_t*)in.blob + e.path_off;
  const uint8_t* t = (const uint8_t*)in.blob + q.path_off;
  const uint32_t n = e.path_len, m = n < q.path_len ? n : q.path_len;
  uint32_t l = 0;
  while (l < m && s[l] == t[l]) l++;
  int cmp = l < m ? (t[l] < s[l] ? -1 : 1) : q.path_len < n ? -1 : q.path_len > n ? 1 : 0;
  *lcp = l;
  *same = cmp == 0;
  if (cmp == 0)
    cmp = mrg_cmp_str((const uint8_t*)in.blob + q.tag_off, q.tag_len,
                      (const uint8_t*)in.blob + e.tag_off, e.tag_len);
  if (cmp > 0) *bad |= kSrcUnordered;
  return true;
}

// 11g glob   (PFSCDC_SRC_GLOB, ahead of 11a) one lane per input entry walks its path once through
//     the glob's position automaton (glob.cpp: at most 64 positions, the set of live ones one
//     uint64_t): per byte c, S = T & accept_byte[c], T = OR of follow[b] over the bits b of S.
//     At the j-th '/' it records in bit j of the entry's mask whether the bytes before it are
//     accepted, which is mf of the directory p[0..k] (TrimRight drops that one '/' of a clean
//     path), and in bit 63 whether a path that is no directory is accepted whole.  For clean
//     paths in ascending order the `full` filter selects an entry iff mf holds for it or for one
//     of its directory prefixes (tests/test_glob_cpu.py holds that against the literal filter),
//     so the count and fill passes read: the directory ending at '/' j is selected iff a bit
//     <= j is set, the entry iff any bit is, and PFSCDC_INFO_MATCH is the own bit.
//     The program is staged into LDS once per workgroup.  follow[] is indexed by the bits of S
//     and accept_byte[] by the path byte, both per lane, so neither can sit in SGPRs.  A 64-bit
//     LDS read has 64 banks of 4 bytes per 32-lane half, so entries 32 apart share a bank pair:
//     'A'..'Z' against 'a'..'z', and each against the digits and punctuation 32 below.  Entry c
//     is therefore staged at c ^ (c >> 5), which moves the eight blocks of 32 apart by one entry
//     each; lanes on the same byte (a common prefix) read one address and broadcast.
constexpr int kGlobFollow = 64, kGlobWords = 64 + 256;

PFS_DEV uint32_t glob_accept_slot(uint32_t c) { return kGlobFollow + (c ^ (c >> 5)); }

__global__ __launch_bounds__(kIdxBlock) void src_glob_kernel(RtarList in,
                                                             const uint64_t* __restrict__ prog,
                                                             uint64_t first, uint64_t last,
                                                             uint32_t nullable,
                                                             uint64_t* __restrict__ masks,
                                                             uint32_t* __restrict__ bad) {
  __shared__ uint64_t lds[kGlobWords];
  for (uint32_t w = threadIdx.x; w < kGlobWords; w += kIdxBlock)
    lds[w < kGlobFollow ? w : glob_accept_slot(w - kGlobFollow)] = prog[w];
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; i < in.n;
       i += (uint64_t)gridDim.x * kIdxBlock) {
    const pfscdc_index_entry e = in.entries[i];
    uint64_t mask = 0;
    if (src_entry_ok(in, e)) {  // (else the count pass answers kSrcMalformed)
      const uint8_t* s = (const uint8_t*)in.blob + e.path_off;
      const uint32_t n = e.path_len;
      uint64_t T = first;
      bool acc = nullable != 0;
      uint32_t j = 0;
      for (uint32_t k = 0; k < n; k++) {
        const uint32_t c = s[k];
        if (c == '/') {
          if (j < 63) mask |= (uint64_t)acc << j;
          j++;
        }
        if (!T) {  // dead for good: only the '/' are still counted
          acc = false;
          continue;
        }
        uint64_t S = T & lds[glob_accept_slot(c)];
        acc = (S & last) != 0;
        T = 0;
        while (S) {
          T |= lds[__builtin_ctzll(S)];
          S &= S - 1;
        }
      }
      if (n && s[n - 1] != '/') mask |= (uint64_t)acc << 63;
      if (j > 63) atomicOr(bad, (uint32_t)kSrcTooDeep);
    }
    masks[i] = mask;
  }
}

// The predicate on the directory s[0, k + 1) that ends at the j-th '/' of input entry i's path
// (mk: the entry's glob mask, under kSrcGlobMasks).
PFS_DEV bool src_dir_selected(const SrcPred& pr, const uint8_t* s, uint32_t k, uint32_t j,
                              uint64_t mk) {
  if (pr.glob != kSrcGlobMasks) return src_selected(pr, s, k + 1);
  return (mk & (j < 63 ? (2ull << j) - 1 : ~0ull)) != 0;
}

// PFSCDC_INFO_MATCH of the output entry s[0, len): own = its own bit of the glob mask
PFS_DEV uint32_t src_match(const SrcPred& pr, uint32_t len, bool own) {
  if (pr.glob == kSrcGlobMasks) return own ? PFSCDC_INFO_MATCH : 0;
  return pr.glob == kSrcGlobRoot && len == 1 ? PFSCDC_INFO_MATCH : 0;
}

// What input entry i emits, *lcp its common prefix with the entry before, *bad |= SrcBad.
PFS_DEV MrgCount src_item(const RtarList& in, const SrcPred& pr, uint64_t i, uint32_t* bad,
                          uint32_t* lcp) {
  MrgCount c{0, 0, 0};
  *lcp = 0;
  const pfscdc_index_entry e = in.entries[i];
  if (!src_entry_ok(in, e)) {
    *bad |= kSrcMalformed;
    return c;
  }
  if (e.flags & (PFSCDC_IDX_HAS_RANGE | PFSCDC_IDX_HAS_CHUNK_REF)) *bad |= kSrcNotLevel0;
  const uint8_t* s = (const uint8_t*)in.blob + e.path_off;
  const uint32_t n = e.path_len;
  if (!path_is_clean(s, n, true)) *bad |= kSrcUnclean;
  if (i > 0) {
    bool same;
    if (!src_follows(in, i, e, bad, lcp, &same)) return c;
    if (same && n && s[n - 1] == '/') *bad |= kSrcDirTwice;
  }
  if (pr.glob == kSrcGlobMasks) {  // the masks in place of the predicate
    const uint64_t mk = pr.masks[i];
    uint32_t j = 0;
    for (uint32_t k = 0; k < *lcp; k++) j += s[k] == '/';
    for (uint32_t k = *lcp; k + 1 < n; k++) {
      if (s[k] != '/') continue;
      if (src_dir_selected(pr, s, k, j, mk)) {
        c.emit++;
        c.blob += (uint64_t)k + 4;
      }
      j++;
    }
    if (mk) {
      c.emit++;
      c.recs = e.count;
      c.blob += (uint64_t)n + e.tag_len + e.last_path_len + 3;
    }
    return c;
  }
  for (uint32_t k = *lcp; k + 1 < n; k++)
    if (s[k] == '/' && src_selected(pr, s, k + 1)) {
      c.emit++;
      c.blob += (uint64_t)k + 4;  // the path and three NULs (path, empty tag, empty LastPath)
    }
  if (src_selected(pr, s, n)) {
    c.emit++;
    c.recs = e.count;
    c.blob += (uint64_t)n + e.tag_len + e.last_path_len + 3;
  }
  return c;
}

__global__ __launch_bounds__(kIdxBlock) void src_count_kernel(RtarList in, SrcPred pr,
                                                              MrgCount* __restrict__ cnt,
                                                              uint32_t* __restrict__ bad) {
  for (uint64_t i = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; i < in.n;
       i += (uint64_t)gridDim.x * kIdxBlock) {
    uint32_t b = 0, lcp;
    cnt[i] = src_item(in, pr, i, &b, &lcp);
    if (b) atomicOr(bad, b);
  }
}

__global__ __launch_bounds__(kIdxBlock) void src_fill_kernel(
    RtarList in, SrcPred pr, const MrgCount* __restrict__ cnt, const uint64_t* __restrict__ base,
    pfscdc_index_entry* __restrict__ entries, char* __restrict__ blob, MrgCopy* __restrict__ copy,
    SrcMeta* __restrict__ meta, pfscdc_file_info* __restrict__ infos, MrgCount* __restrict__ sizes,
    uint32_t* __restrict__ maxdepth) {
  for (uint64_t i = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; i < in.n;
       i += (uint64_t)gridDim.x * kIdxBlock) {
    if (!cnt[i].emit) continue;
    uint64_t oi = base[3 * i], at = base[3 * i + 2];
    const uint64_t first = base[3 * i + 1];
    uint32_t b = 0, lcp;
    const MrgCount c = src_item(in, pr, i, &b, &lcp);
    if (b || !ranges_are(base, i, c)) continue;  // (never: the count pass's walk)
    const pfscdc_index_entry e = in.entries[i];
    const uint8_t* s = (const uint8_t*)in.blob + e.path_off;
    const uint32_t n = e.path_len;
    uint32_t depth = 0;  // the '/' in s[0, k): a path's depth is that of its bytes but the last
    for (uint32_t k = 0; k < lcp; k++) depth += s[k] == '/';
    // under a glob the '/' at k is the path's depth-th, and bit depth of the mask is its own
    const uint64_t mk = pr.glob == kSrcGlobMasks ? pr.masks[i] : 0;
    for (uint32_t k = lcp; k + 1 < n; k++) {
      if (s[k] != '/') continue;
      if (src_dir_selected(pr, s, k, depth, mk)) {  // dirFile.Index(): Index{Path: dir, File: {}}
        pfscdc_index_entry o;
        o.path_off = at;
        at = put_str(blob, at, (const char*)s, k + 1);
        o.tag_off = at;  // an empty tag, an empty LastPath
        at = put_str(blob, at, nullptr, 0);
        o.last_path_off = at;
        at = put_str(blob, at, nullptr, 0);
        o.path_len = k + 1;
        o.tag_len = o.last_path_len = 0;
        o.flags = PFSCDC_IDX_HAS_FILE;
        o.first = (uint32_t)first;
        o.count = 0;
        o.size_bytes = o.range_offset = 0;
        entries[oi] = o;
        meta[oi] = SrcMeta{kSrcDir, depth, 0};
        infos[oi].size = 0;
        infos[oi].type = PFSCDC_FILE_TYPE_DIR;
        infos[oi].flags =
            src_child(pr, s, k + 1) | src_match(pr, k + 1, depth < 63 && (mk >> depth & 1));
        sizes[oi] = MrgCount{0, 0, 0};
        atomicMax(maxdepth, depth);
        atomicAdd(maxdepth + 1, 1u);  // directories inserted
        oi++;
      }
      depth++;
    }
    if (pr.glob == kSrcGlobMasks ? mk == 0 : !src_selected(pr, s, n)) continue;
    pfscdc_index_entry o = e;
    put_entry_strings(o, in.blob, blob, at);
    o.first = (uint32_t)first;
    entries[oi] = o;
    if (e.count) copy[i] = MrgCopy{(uint32_t)first, e.count, e.first, 0};
    const bool dir = n && s[n - 1] == '/';
    meta[oi] = SrcMeta{(uint32_t)i, depth, 0};
    infos[oi].size = dir ? 0 : e.size_bytes;
    infos[oi].type = dir ? PFSCDC_FILE_TYPE_DIR : PFSCDC_FILE_TYPE_FILE;
    infos[oi].flags =
        src_child(pr, s, n) | src_match(pr, n, mk >> (dir ? (depth < 63 ? depth : 0) : 63) & 1);
    sizes[oi] = MrgCount{0, 0, dir ? 0 : (uint64_t)e.size_bytes};
    atomicMax(maxdepth, depth);
  }
}

__global__ __launch_bounds__(kIdxBlock) void src_tree_kernel(
    RtarList out, SrcMeta* __restrict__ meta, const uint64_t* __restrict__ sbase,
    pfscdc_file_info* __restrict__ infos) {
  for (uint64_t o = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; o < out.n;
       o += (uint64_t)gridDim.x * kIdxBlock) {
    uint64_t end = o + 1;
    if (infos[o].type == PFSCDC_FILE_TYPE_DIR) {
      const pfscdc_index_entry e = out.entries[o];
      const uint8_t* s = (const uint8_t*)out.blob + e.path_off;
      uint64_t lo = o + 1, hi = out.n;  // the first entry after o without o's path as a prefix
      while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const pfscdc_index_entry q = out.entries[mid];
        const uint8_t* t = (const uint8_t*)out.blob + q.path_off;
        bool pre = q.path_len >= e.path_len;
        for (uint32_t k = 0; pre && k < e.path_len; k++) pre = s[k] == t[k];
        if (pre) lo = mid + 1;
        else hi = mid;
      }
      end = lo;
      infos[o].size = (int64_t)(sbase[3 * end + 2] - sbase[3 * o + 2]);
    }
    meta[o].end = end;
  }
}

PFS_DEV pfscdc_segment src_segment(uint64_t offset, uint64_t size) {
  pfscdc_segment sg;
  sg.offset = offset;
  sg.size = size;
  sg.file = 0;
  sg.flags = PFSCDC_SEG_VALID;
  for (int k = 0; k < 32; k++) sg.hash[k] = 0;
  return sg;
}

__global__ __launch_bounds__(kIdxBlock) void src_leaf_kernel(RtarList out,
                                                             uint8_t* __restrict__ buf,
                                                             pfscdc_segment* __restrict__ segs) {
  const uint64_t items = out.n > out.nr ? out.n : out.nr;
  for (uint64_t x = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; x < items;
       x += (uint64_t)gridDim.x * kIdxBlock) {
    if (x < out.nr) {  // hashDataRefs: the DataRefs' hashes back to back
      const uint4* h = reinterpret_cast<const uint4*>(out.drs[x].data.hash);
      uint4* d = reinterpret_cast<uint4*>(buf + 32 * x);
      d[0] = h[0];
      d[1] = h[1];
    }
    if (x < out.n) segs[x] = src_segment(32ull * out.entries[x].first, 32ull * out.entries[x].count);
  }
}

// The caller's leaf hashes (32 bytes per input entry) as the files' hashes.
__global__ __launch_bounds__(kIdxBlock) void src_leaf_copy_kernel(
    const SrcMeta* __restrict__ meta, const uint8_t* __restrict__ leaf, uint64_t n,
    pfscdc_file_info* __restrict__ infos) {
  for (uint64_t o = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; o < n;
       o += (uint64_t)gridDim.x * kIdxBlock) {
    if (infos[o].type == PFSCDC_FILE_TYPE_DIR) continue;
    for (int k = 0; k < 32; k++) infos[o].hash[k] = leaf[32ull * meta[o].src + k];
  }
}

__global__ __launch_bounds__(kIdxBlock) void src_level_count_kernel(
    const SrcMeta* __restrict__ meta, const pfscdc_file_info* __restrict__ infos, uint64_t n,
    uint32_t level, MrgCount* __restrict__ cnt) {
  for (uint64_t o = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; o < n;
       o += (uint64_t)gridDim.x * kIdxBlock)
    cnt[o] = MrgCount{meta[o].depth == level + 1 ? 1u : 0u,
                      meta[o].depth == level && infos[o].type == PFSCDC_FILE_TYPE_DIR ? 1u : 0u, 0};
}

__global__ __launch_bounds__(kIdxBlock) void src_level_gather_kernel(
    const SrcMeta* __restrict__ meta, const pfscdc_file_info* __restrict__ infos,
    const uint64_t* __restrict__ base, uint64_t n, uint32_t level, uint8_t* __restrict__ buf,
    pfscdc_segment* __restrict__ segs) {
  for (uint64_t o = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; o < n;
       o += (uint64_t)gridDim.x * kIdxBlock) {
    const SrcMeta m = meta[o];
    if (m.depth == level + 1) {
      const uint4* h = reinterpret_cast<const uint4*>(infos[o].hash);
      uint4* d = reinterpret_cast<uint4*>(buf + 32 * base[3 * o]);
      d[0] = h[0];
      d[1] = h[1];
    }
    if (m.depth == level && infos[o].type == PFSCDC_FILE_TYPE_DIR) {
      // its children: the entries of depth level + 1 in (o, end)
      const uint64_t a = base[3 * (o + 1)], b = base[3 * m.end];
      segs[base[3 * o + 1]] = src_segment(32 * a, 32 * (b - a));
    }
  }
}

// level < 0: the leaf pass's digests (segs[o]) into the files' infos; else the digests of the
// directories of depth level (segs[their number among them]) into theirs.
__global__ __launch_bounds__(kIdxBlock) void src_scatter_kernel(
    const SrcMeta* __restrict__ meta, const uint64_t* __restrict__ base,
    const pfscdc_segment* __restrict__ segs, uint64_t n, int level,
    pfscdc_file_info* __restrict__ infos) {
  for (uint64_t o = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; o < n;
       o += (uint64_t)gridDim.x * kIdxBlock) {
    const bool dir = infos[o].type == PFSCDC_FILE_TYPE_DIR;
    if (level < 0 ? dir : (!dir || meta[o].depth != (uint32_t)level)) continue;
    const pfscdc_segment* sg = &segs[level < 0 ? o : base[3 * o + 1]];
    for (int k = 0; k < 32; k++) infos[o].hash[k] = sg->hash[k];
  }
}

hipError_t launch_src_glob(const RtarList& in, const uint64_t* prog, uint64_t first, uint64_t last,
                           bool nullable, uint64_t* masks, uint32_t* bad, int num_cus,
                           hipStream_t st) {
  if (in.n == 0) return hipSuccess;
  src_glob_kernel<<<merge_grid(in.n, num_cus), kIdxBlock, 0, st>>>(in, prog, first, last,
                                                                   nullable ? 1u : 0u, masks, bad);
  return hipGetLastError();
}

hipError_t launch_src_count(const RtarList& in, const SrcPred& pr, MrgCount* cnt, uint32_t* bad,
                            int num_cus, hipStream_t st) {
  if (in.n == 0) return hipSuccess;
  src_count_kernel<<<merge_grid(in.n, num_cus), kIdxBlock, 0, st>>>(in, pr, cnt, bad);
  return hipGetLastError();
}

hipError_t launch_src_fill(const RtarList& in, const SrcPred& pr, const MrgCount* cnt,
                           const uint64_t* base, pfscdc_index_entry* entries, char* blob,
                           MrgCopy* copy, SrcMeta* meta, pfscdc_file_info* infos, MrgCount* sizes,
                           uint32_t* maxdepth, pfscdc_full_dataref* drs, int num_cus,
                           hipStream_t st) {
  if (in.n == 0) return hipSuccess;
  src_fill_kernel<<<merge_grid(in.n, num_cus), kIdxBlock, 0, st>>>(
      in, pr, cnt, base, entries, blob, copy, meta, infos, sizes, maxdepth);
  return launch_list_copy(in.drs, copy, in.n, drs, num_cus, st);
}

hipError_t launch_src_tree(const RtarList& out, SrcMeta* meta, const uint64_t* sbase,
                           pfscdc_file_info* infos, int num_cus, hipStream_t st) {
  if (out.n == 0) return hipSuccess;
  src_tree_kernel<<<merge_grid(out.n, num_cus), kIdxBlock, 0, st>>>(out, meta, sbase, infos);
  return hipGetLastError();
}

hipError_t launch_src_leaf(const RtarList& out, uint8_t* buf, pfscdc_segment* segs, int num_cus,
                           hipStream_t st) {
  if (out.n == 0) return hipSuccess;
  src_leaf_kernel<<<merge_grid(out.n > out.nr ? out.n : out.nr, num_cus), kIdxBlock, 0, st>>>(
      out, buf, segs);
  return hipGetLastError();
}

hipError_t launch_src_leaf_copy(const SrcMeta* meta, const uint8_t* leaf, uint64_t n,
                                pfscdc_file_info* infos, int num_cus, hipStream_t st) {
  if (n == 0) return hipSuccess;
  src_leaf_copy_kernel<<<merge_grid(n, num_cus), kIdxBlock, 0, st>>>(meta, leaf, n, infos);
  return hipGetLastError();
}

hipError_t launch_src_level_count(const SrcMeta* meta, const pfscdc_file_info* infos, uint64_t n,
                                  uint32_t level, MrgCount* cnt, int num_cus, hipStream_t st) {
  if (n == 0) return hipSuccess;
  src_level_count_kernel<<<merge_grid(n, num_cus), kIdxBlock, 0, st>>>(meta, infos, n, level, cnt);
  return hipGetLastError();
}

hipError_t launch_src_level_gather(const SrcMeta* meta, const pfscdc_file_info* infos,
                                   const uint64_t* base, uint64_t n, uint32_t level, uint8_t* buf,
                                   pfscdc_segment* segs, int num_cus, hipStream_t st) {
  if (n == 0) return hipSuccess;
  src_level_gather_kernel<<<merge_grid(n, num_cus), kIdxBlock, 0, st>>>(meta, infos, base, n, level,
                                                                        buf, segs);
  return hipGetLastError();
}

hipError_t launch_src_scatter(const SrcMeta* meta, const uint64_t* base, const pfscdc_segment* segs,
                              uint64_t n, int level, pfscdc_file_info* infos, int num_cus,
                              hipStream_t st) {
  if (n == 0) return hipSuccess;
  src_scatter_kernel<<<merge_grid(n, num_cus), kIdxBlock, 0, st>>>(meta, base, segs, n, level,
                                                                   infos);
  return hipGetLastError();
}

// ---- 12. DiffFile: two Sources joined by path --------------------------------------------------
// (server/pfs/server/diff.go:26-96 Differ.Iterate / equalFileInfos; diff.cpp takes it literally)
//
// Within a side the paths do not decrease (a path occurs once per tag), so the two-pointer walk is
// a join.  For a path p with na_p entries on side a and nb_p on side b it reports the first
// min(na_p, nb_p) entries of both sides as pairs, k-th with k-th, each only if the hashes differ,
// and then the longer run's surplus alone; everything of a lesser path comes before.  So with
// k = an entry's number in its run, [lb, ub) = the run of its path in the other side:
//   an entry is paired iff k < ub - lb, with entry lb + k of the other side;
//   an a-entry is reported if it is unpaired or its hash differs, a b-entry alone if unpaired;
//   an a-record lies after the a-records of the a-entries before it and the b-records of the
//   b-entries of a lesser path: exA[i] + exB[lb_b(p)] (the b-entries [lb, lb + k) are paired and
//   report nothing of their own, and unpaired ones of p have k' >= na_p > k and follow);
//   a b-record lies after the b-records before it and the a-records of paths <= p:
//   exB[j] + exA[ub_a(p)].
// 12a rank   one lane per entry of either side: one compare with its predecessor (a side whose
//     paths decrease sets *bad, and diff_dev.cpp hands the call to the host arm), k by a search
//     in its own side only if the predecessor's path is equal, lb and ub by searches in the other
//     side, the 32 hash bytes; what the entry brings into its side's selection.
// 12b scan   merge_scan_kernel as it is: side a's and side b's selections, side b's records.
// 12c fill   one lane per entry writes its own pfscdc_diff_pair.
// 12d select per side, one lane per selected entry: the entry, its strings and its info at its own
//     ranges (nothing unless its counts equal them), one MrgCopy for merge_copy_kernel.
PFS_DEV int diff_cmp_path(const RtarList& x, uint64_t i, const uint8_t* s, uint32_t n) {
  const pfscdc_index_entry& e = x.entries[i];
  return mrg_cmp_str((const uint8_t*)x.blob + e.path_off, e.path_len, s, n);
}

// the first entry of x[lo, hi) whose path is not below s (upper: that is above s)
PFS_DEV uint64_t diff_bound(const RtarList& x, uint64_t lo, uint64_t hi, const uint8_t* s,
                            uint32_t n, bool upper) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    const int c = diff_cmp_path(x, mid, s, n);
    if (upper ? c <= 0 : c < 0) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kIdxBlock) void diff_rank_kernel(DiffSide a, DiffSide b,
                                                              DiffRank* __restrict__ rank,
                                                              MrgCount* __restrict__ sel,
                                                              MrgCount* __restrict__ emit_b,
                                                              uint32_t* __restrict__ bad) {
  const uint64_t na = a.l.n, items = a.l.n + b.l.n;
  for (uint64_t x = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; x < items;
       x += (uint64_t)gridDim.x * kIdxBlock) {
    const bool is_b = x >= na;
    const DiffSide& own = is_b ? b : a;
    const DiffSide& oth = is_b ? a : b;
    const uint64_t i = is_b ? x - na : x;
    const pfscdc_index_entry e = own.l.entries[i];
    const uint8_t* s = (const uint8_t*)own.l.blob + e.path_off;
    const uint32_t n = e.path_len;
    uint64_t k = 0;  // its number among the entries of its path
    if (i > 0) {
      const int c = diff_cmp_path(own.l, i - 1, s, n);
      if (c > 0) atomicOr(bad, 1u);
      if (c == 0) k = i - diff_bound(own.l, 0, i, s, n, false);
    }
    const uint64_t lb = diff_bound(oth.l, 0, oth.l.n, s, n, false);
    uint64_t ub = lb;
    if (lb < oth.l.n && diff_cmp_path(oth.l, lb, s, n) == 0)
      ub = diff_bound(oth.l, lb + 1, oth.l.n, s, n, true);
    const bool paired = k < ub - lb;  // then lb + k < ub <= the other side's count
    bool differ = false;
    if (paired) {
      const uint4* p = reinterpret_cast<const uint4*>(own.infos[i].hash);
      const uint4* q = reinterpret_cast<const uint4*>(oth.infos[lb + k].hash);
      const uint4 p0 = p[0], p1 = p[1], q0 = q[0], q1 = q[1];
      differ = p0.x != q0.x || p0.y != q0.y || p0.z != q0.z || p0.w != q0.w || p1.x != q1.x ||
               p1.y != q1.y || p1.z != q1.z || p1.w != q1.w;
    }
    rank[x] = DiffRank{paired ? (uint32_t)(lb + k) : PFSCDC_DIFF_NONE, (uint32_t)(is_b ? ub : lb)};
    sel[x] = (!paired || differ)
                 ? MrgCount{1, e.count, (uint64_t)e.path_len + e.tag_len + e.last_path_len + 3}
                 : MrgCount{0, 0, 0};
    if (is_b) emit_b[i] = MrgCount{paired ? 0u : 1u, 0, 0};
  }
}

__global__ __launch_bounds__(kIdxBlock) void diff_fill_kernel(
    uint64_t na, uint64_t nb, const DiffRank* __restrict__ rank, const MrgCount* __restrict__ sel,
    const uint64_t* __restrict__ base_a, const MrgCount* __restrict__ emit_b,
    const uint64_t* __restrict__ base_e, pfscdc_diff_pair* __restrict__ pairs, uint64_t npairs) {
  for (uint64_t x = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; x < na + nb;
       x += (uint64_t)gridDim.x * kIdxBlock) {
    const DiffRank r = rank[x];
    if (x < na) {
      if (!sel[x].emit || r.other > nb) continue;
      const uint64_t at = base_a[3 * x] + base_e[3 * (uint64_t)r.other];
      if (at < npairs) pairs[at] = pfscdc_diff_pair{(uint32_t)x, r.partner};
    } else {
      const uint64_t j = x - na;
      if (!emit_b[j].emit || r.other > na) continue;
      const uint64_t at = base_e[3 * j] + base_a[3 * (uint64_t)r.other];
      if (at < npairs) pairs[at] = pfscdc_diff_pair{PFSCDC_DIFF_NONE, (uint32_t)j};
    }
  }
}

__global__ __launch_bounds__(kIdxBlock) void diff_select_kernel(
    DiffSide in, const MrgCount* __restrict__ sel, const uint64_t* __restrict__ base,
    pfscdc_index_entry* __restrict__ entries, char* __restrict__ blob, MrgCopy* __restrict__ copy,
    pfscdc_file_info* __restrict__ infos) {
  for (uint64_t i = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; i < in.l.n;
       i += (uint64_t)gridDim.x * kIdxBlock) {
    if (!sel[i].emit) continue;
    const uint64_t oi = base[3 * i], first = base[3 * i + 1];
    const pfscdc_index_entry e = in.l.entries[i];
    const uint64_t room = (uint64_t)e.path_len + e.tag_len + e.last_path_len + 3;
    if (!ranges_are(base, i, MrgCount{1, e.count, room})) continue;  // (never: the rank pass's counts)
    pfscdc_index_entry o = e;
    put_entry_strings(o, in.l.blob, blob, base[3 * i + 2]);
    o.first = (uint32_t)first;
    entries[oi] = o;
    if (e.count) copy[i] = MrgCopy{(uint32_t)first, e.count, e.first, 0};
    infos[oi] = in.infos[i];
  }
}

hipError_t launch_diff_rank(const DiffSide& a, const DiffSide& b, DiffRank* rank, MrgCount* sel,
                            MrgCount* emit_b, uint32_t* bad, int num_cus, hipStream_t st) {
  if (a.l.n + b.l.n == 0) return hipSuccess;
  diff_rank_kernel<<<merge_grid(a.l.n + b.l.n, num_cus), kIdxBlock, 0, st>>>(a, b, rank, sel,
                                                                            emit_b, bad);
  return hipGetLastError();
}

hipError_t launch_diff_fill(uint64_t na, uint64_t nb, const DiffRank* rank, const MrgCount* sel,
                            const uint64_t* base_a, const MrgCount* emit_b, const uint64_t* base_e,
                            pfscdc_diff_pair* pairs, uint64_t npairs, int num_cus, hipStream_t st) {
  if (na + nb == 0 || npairs == 0) return hipSuccess;
  diff_fill_kernel<<<merge_grid(na + nb, num_cus), kIdxBlock, 0, st>>>(na, nb, rank, sel, base_a,
                                                                      emit_b, base_e, pairs, npairs);
  return hipGetLastError();
}

hipError_t launch_diff_select(const DiffSide& in, const MrgCount* sel, const uint64_t* base,
                              pfscdc_index_entry* entries, char* blob, MrgCopy* copy,
                              pfscdc_file_info* infos, pfscdc_full_dataref* drs, int num_cus,
                              hipStream_t st) {
  if (in.l.n == 0) return hipSuccess;
  diff_select_kernel<<<merge_grid(in.l.n, num_cus), kIdxBlock, 0, st>>>(in, sel, base, entries,
                                                                       blob, copy, infos);
  return launch_list_copy(in.l.drs, copy, in.l.n, drs, num_cus, st);
}

// ---- 13. CopyFile: a subtree selected and moved under a new root -------------------------------
// (server/pfs/server/driver_file.go:143-171 copyFile, fileset/transforms.go:20-90 NewIndexFilter /
// NewIndexMapper, index/reader.go:95-122 atStart / atEnd; copy_map.cpp takes them literally)
//
// The open's options keep the entries from the first atStart (path >= srcPath) to the first atEnd
// (the path's first min(len) bytes above srcPath's) whose tag passes; the filter then keeps
// path == srcPath || HasPrefix(path, srcPath + "/"); the mapper rewrites the path to
// Join(dstPath, Rel(srcPath, path)).  Two facts let one lane decide its entry alone:
//  (1) For a list in (path, tag) order both atStart and atEnd are monotone along the list (a path
//      at or above srcPath stays so, and once a path's leading bytes exceed srcPath's every later
//      path's do), so the entries between them are those with path >= srcPath and !atEnd(path),
//      which is HasPrefix(path, srcPath) for a non-empty srcPath: a shorter path is below srcPath
//      or past it.  The filter's predicate implies that test, so the selection is the predicate
//      and the tag test, entry by entry.
//  (2) For a selected path that is clean as a file path (IsClean(p, false): rooted, no empty, "."
//      or ".." component, no trailing '/'), Clean(path) = path, so Rel(srcPath, path) is "." for
//      path == srcPath and else the bytes after srcPath + "/", and Join gives dstPath, or
//      dstPath + "/" + tail ("/" + tail under the root).  The selected paths share the prefix
//      srcPath, which is replaced whole, so the output keeps the input's (path, tag) order.
// A list out of order, or a selected path that is not clean, sets a bit in *bad and
// copy_map_dev.cpp hands the call to the host arm, which does what the reference does.
// 13a count  one lane per input entry: its bounds before any byte of the blob is read, the order
//     against its predecessor, the tag test and the predicate, cleanliness if selected:
//     {1, DataRefs, new path + tag + empty LastPath + three NULs}.
// 13b scan   merge_scan_kernel as it is.
// 13c fill   one lane per selected entry writes the entry, dstPath and the path's tail, the tag
//     (nothing unless its counts equal its ranges), one MrgCopy for merge_copy_kernel.
struct CmapItem {
  MrgCount c;
  uint32_t keep;  // the path's bytes [n - keep, n) follow the new root
  uint32_t root;  // the new root's bytes: dst_len, or 0 for a tail under "/"
};

PFS_DEV CmapItem cmap_item(const RtarList& in, const CmapPred& pr, uint64_t i, uint32_t* bad) {
  CmapItem it{MrgCount{0, 0, 0}, 0, 0};
  const pfscdc_index_entry e = in.entries[i];
  if (!src_entry_ok(in, e)) {
    *bad |= kSrcMalformed;
    return it;
  }
  if (e.flags & (PFSCDC_IDX_HAS_RANGE | PFSCDC_IDX_HAS_CHUNK_REF)) *bad |= kSrcNotLevel0;
  const uint8_t* s = (const uint8_t*)in.blob + e.path_off;
  const uint8_t* t = (const uint8_t*)in.blob + e.tag_off;
  const uint32_t n = e.path_len;
  uint32_t lcp;
  bool same;
  if (i > 0 && !src_follows(in, i, e, bad, &lcp, &same)) return it;
  if (pr.tag_len) {  // index.WithTag
    bool eq = e.tag_len == pr.tag_len;
    for (uint32_t k = 0; eq && k < pr.tag_len; k++) eq = t[k] == (uint8_t)pr.tag[k];
    if (!eq) return it;
  }
  // path == srcPath || HasPrefix(path, srcPath + "/")
  if (n < pr.src_len) return it;
  for (uint32_t k = 0; k < pr.src_len; k++)
    if (s[k] != (uint8_t)pr.src[k]) return it;
  if (n > pr.src_len && s[pr.src_len] != '/') return it;
  const bool clean = path_is_clean(s, n, false);
  it.keep = n - pr.src_len;
  it.root = (it.keep && pr.dst_len == 1) ? 0 : pr.dst_len;  // dstPath "/" + "/tail" is "/tail"
  const uint64_t len = (uint64_t)it.root + it.keep;
  if (!clean || len > 0xffffffffull) *bad |= kSrcUnclean;
  it.c = MrgCount{1, e.count, len + e.tag_len + 3};
  return it;
}

__global__ __launch_bounds__(kIdxBlock) void cmap_count_kernel(RtarList in, CmapPred pr,
                                                               MrgCount* __restrict__ cnt,
                                                               uint32_t* __restrict__ bad) {
  for (uint64_t i = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; i < in.n;
       i += (uint64_t)gridDim.x * kIdxBlock) {
    uint32_t b = 0;
    cnt[i] = cmap_item(in, pr, i, &b).c;
    if (b) atomicOr(bad, b);
  }
}

__global__ __launch_bounds__(kIdxBlock) void cmap_fill_kernel(
    RtarList in, CmapPred pr, const MrgCount* __restrict__ cnt, const uint64_t* __restrict__ base,
    pfscdc_index_entry* __restrict__ entries, char* __restrict__ blob, MrgCopy* __restrict__ copy) {
  for (uint64_t i = (uint64_t)blockIdx.x * kIdxBlock + threadIdx.x; i < in.n;
       i += (uint64_t)gridDim.x * kIdxBlock) {
    if (!cnt[i].emit) continue;
    const uint64_t oi = base[3 * i], first = base[3 * i + 1];
    uint64_t at = base[3 * i + 2];
    uint32_t b = 0;
    const CmapItem it = cmap_item(in, pr, i, &b);
    if (b || !ranges_are(base, i, it.c)) continue;  // (never: the count pass's walk)
    const pfscdc_index_entry e = in.entries[i];
    pfscdc_index_entry o = e;
    o.path_off = at;
    o.path_len = it.root + it.keep;
    at = put_str(blob, at, pr.dst, it.root) - 1;  // the new root; the tail goes over its NUL
    at = put_str(blob, at, in.blob + e.path_off + (e.path_len - it.keep), it.keep);
    o.tag_off = at;
    at = put_str(blob, at, in.blob + e.tag_off, e.tag_len);
    o.last_path_off = at;
    o.last_path_len = 0;
    put_str(blob, at, nullptr, 0);
    o.first = (uint32_t)first;
    entries[oi] = o;
    if (e.count) copy[i] = MrgCopy{(uint32_t)first, e.count, e.first, 0};
  }
}

hipError_t launch_cmap_count(const RtarList& in, const CmapPred& pr, MrgCount* cnt, uint32_t* bad,
                             int num_cus, hipStream_t st) {
  if (in.n == 0) return hipSuccess;
  cmap_count_kernel<<<merge_grid(in.n, num_cus), kIdxBlock, 0, st>>>(in, pr, cnt, bad);
  return hipGetLastError();
}

hipError_t launch_cmap_fill(const RtarList& in, const CmapPred& pr, const MrgCount* cnt,
                            const uint64_t* base, pfscdc_index_entry* entries, char* blob,
                            MrgCopy* copy, int num_cus, hipStream_t st) {
  if (in.n == 0) return hipSuccess;
  cmap_fill_kernel<<<merge_grid(in.n, num_cus), kIdxBlock, 0, st>>>(in, pr, cnt, base, entries,
                                                                   blob, copy);
  return hipGetLastError();
}

}  // namespace pfscdc
