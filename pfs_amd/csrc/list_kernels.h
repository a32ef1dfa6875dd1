// list_kernels.h — the records and launchers of the index list passes (kernels: list_kernels.hip):
// index decode, MergeReader, the resident tar plan, the Source, DiffFile and CopyFile's map.
// Their drivers see it through dev_pass.h; the data plane (pfscdc_internal.h) does not.
#pragma once
#include "pfscdc_internal.h"

namespace pfscdc {

// ---- index.Reader on the device (index.cpp; kernels in list_kernels.hip §8) ----
// One frame walker: hop from start (kNone: no walk) length by length until the first frame
// start at or beyond limit; the starts go to starts[slot, slot + cap).
struct IdxWalk {
  uint64_t start, limit, slot, cap;
};
struct IdxWalkOut {
  uint64_t exit;   // first frame start >= limit (where the walk stopped, with err)
  uint64_t count;  // frame starts recorded
  uint64_t err;    // kNone, or the start of the frame whose length does not fit the stream
  uint64_t past;   // with err: 1 the frame (or its length field) runs past the stream's end,
                   // 0 a negative length
};
struct IdxCount {  // per frame: records in the DataRef array, bytes in the blob
  uint32_t ndr, blob;
};
// walkers w[0, nw) over the stream buf[0, n) (buf 16-B aligned, readable to n + 32)
hipError_t launch_index_walk(const uint8_t* buf, uint64_t n, const IdxWalk* w, uint32_t nw,
                             uint64_t* starts, IdxWalkOut* out, int num_cus, hipStream_t st);
// count pass over the nf frames at fstart[]: cnt[f]; *err_min = the lowest start of a frame
// that does not parse (preset to kNone)
hipError_t launch_index_count(const uint8_t* buf, uint64_t n, const uint64_t* fstart, uint64_t nf,
                              IdxCount* cnt, unsigned long long* err_min, int num_cus,
                              hipStream_t st);
// exclusive prefix sums of cnt[0, nf) into base[0, nf] ({records, blob bytes} per frame)
hipError_t launch_index_scan(const IdxCount* cnt, uint64_t nf, uint64_t* base, hipStream_t st);
// fill pass: entries[f], drs[base[2f], base[2f + 2)), blob[base[2f + 1], base[2f + 3))
hipError_t launch_index_fill(const uint8_t* buf, uint64_t n, const uint64_t* fstart, uint64_t nf,
                             const uint64_t* base, pfscdc_index_entry* entries,
                             pfscdc_full_dataref* drs, char* blob, int num_cus, hipStream_t st);
// ---- MergeReader on the device (index.cpp; kernels in list_kernels.hip §9) ----
// The streams of one merge, concatenated stream-major on the device: stream s holds entries
// [stream_begin[s], stream_begin[s + 1]), whose string offsets count from blob + blob_base[s]
// and whose DataRef indexes from drs + dr_base[s].
struct MrgIn {
  const pfscdc_index_entry* entries;
  const char* blob;
  const pfscdc_full_dataref* drs;
  const uint64_t *stream_begin, *blob_base, *dr_base;  // ns + 1, ns, ns
  uint64_t n;   // entries in all (< 2^32)
  uint32_t ns;  // streams
  int mode;     // PFSCDC_MERGE_*
};
struct MrgCount {  // per merged position: what the group that begins there emits
  uint32_t emit, recs;
  uint64_t blob;
};
struct MrgCopy {  // per source entry: its recs DataRefs drs[src, ...) go to out[dst, ...)
  uint32_t dst, recs, src, reserved;
};
// order[rank of entry e in the merged order] = e; *bad |= 1 if a stream is not strictly
// ascending in (path, tag) (order is then not a permutation and must not be used)
hipError_t launch_merge_rank(const MrgIn& in, uint32_t* order, uint32_t* bad, int num_cus,
                             hipStream_t st);
// cnt[p] for every merged position p ({0, 0, 0} where no emitting group begins); *heads (zeroed
// before) += the groups
hipError_t launch_merge_group(const MrgIn& in, const uint32_t* order, MrgCount* cnt,
                              unsigned long long* heads, int num_cus, hipStream_t st);
// The list passes (merge, Source, diff, copy map) share one contract.  A count kernel gives
// cnt[i] = {entries, DataRefs, blob bytes} item i emits; launch_merge_scan turns cnt[0, n) into
// exclusive prefix sums base[0, n], three per item, the totals last.  A fill kernel then writes
// item i's entries from entries[base[3i]] and their strings from blob + base[3i + 2], and only if
// what it counts again equals its ranges base[3i + 3 ...] - base[3i ...]; into copy[] (zeroed
// before) it puts the source entries whose DataRefs go to drs[base[3i + 1], ...), and
// launch_list_copy moves those.
hipError_t launch_merge_scan(const MrgCount* cnt, uint64_t n, uint64_t* base, hipStream_t st);
// the merged entries and their strings, copy[] (the contract above, p a merged position)
hipError_t launch_merge_fill(const MrgIn& in, const uint32_t* order, const MrgCount* cnt,
                             const uint64_t* base, pfscdc_index_entry* entries, char* blob,
                             MrgCopy* copy, int num_cus, hipStream_t st);
// dst[copy[i].dst ...] = src[copy[i].src ...] for each of the n source entries, 16 bytes per lane
hipError_t launch_list_copy(const pfscdc_full_dataref* src, const MrgCopy* copy, uint64_t n,
                            pfscdc_full_dataref* dst, int num_cus, hipStream_t st);

// ---- GetFileTAR over a device-resident list (resident.cpp; kernels in list_kernels.hip §10) ----
struct RtarList {  // the three arrays of a pfscdc_dev_list
  const pfscdc_index_entry* entries;
  const char* blob;
  const pfscdc_full_dataref* drs;
  uint64_t n, nr, nb;  // entries, DataRefs, blob bytes (n, nr < 2^32)
};
// Sums of sizes saturate here: a sum that reaches it is past the 2^62 tar_plan refuses.
constexpr uint64_t kRtarCap = (1ull << 62) + 1;
// Why an entry has no place in the stream, in the order tar_plan finds them.
enum RtarWhy : uint32_t {
  kRtarBeyond = 1,  // pieces beyond the DataRef array
  kRtarNotPacked,   // DataRefs not at [first, first + count) packed in entry order
  kRtarString,      // path outside the blob
  kRtarOverflow,    // the sizes' sum overflows
  kRtarEmpty,       // tar_name_check's reasons
  kRtarDirContent,
  kRtarNotAscii,
  kRtarTooBig,
  kRtarNoSplit,
  kRtarPaxLong,   // with PFSCDC_TAR_PAX: a PAX name above kTarMaxName bytes
  kRtarPaxJoin,   // ... or one path.Join would rewrite (tar_name_joins)
  kRtarDirPieces,
};
constexpr unsigned long long kRtarNoErr = ~0ull;  // else entry index << 8 | RtarWhy
struct RtarWindow {  // entries [i0, i1) meet the window; their DataRefs are [k0, k1)
  uint64_t i0, i1, k0, k1;
};
// flags[0] |= and flags[1] &= the flags of entries[0, n) (preset to 0 and ~0)
hipError_t launch_index_flags(const pfscdc_index_entry* entries, uint64_t n, uint32_t* flags,
                              int num_cus, hipStream_t st);
// dsz[k] = DataRef k's size (saturated); *bad |= 1 for one StoreBatch::valid refuses (size 0)
hipError_t launch_rtar_sizes(const pfscdc_full_dataref* drs, uint64_t nr, uint64_t* dsz,
                             uint32_t* bad, int num_cus, hipStream_t st);
// out[0, n] = saturating exclusive prefix sums of in[0, n); ent (nullable): ent[i].off = out[i]
hipError_t launch_rtar_scan(const uint64_t* in, uint64_t n, uint64_t* out, TarEntry* ent,
                            hipStream_t st);
// per entry: the checks of tar_plan under format, ent[i] (off unset), span[i] = head +
// roundup512(size) (0 for a refused entry) and, where xb is not nullptr, xb[i] = head / 512 - 1;
// *err = min(entry << 8 | RtarWhy) (preset to kRtarNoErr)
hipError_t launch_rtar_entries(const RtarList& l, const uint64_t* dpre, int format, TarEntry* ent,
                               uint64_t* span, uint64_t* xb, unsigned long long* err, int num_cus,
                               hipStream_t st);
// the entries that meet stream bytes [begin, end), by searches in off[0, n]; xblk (nullable): the
// prefix sums of launch_rtar_entries' xb, and then *nx = xblk[w->i1] - xblk[w->i0], the head
// blocks of those entries other than main headers
hipError_t launch_rtar_window(const RtarList& l, const uint64_t* off, const uint64_t* xblk,
                              uint64_t begin, uint64_t end, RtarWindow* w, uint64_t* nx,
                              hipStream_t st);
// Pieces of DataRefs [w.k0, w.k1) clipped to the window.  Count pass (slices == nullptr):
// cnt[k - k0] = {non-empty, run head, keystream blocks}.  Fill pass, after launch_merge_scan of
// cnt into base: the dense slices (chunk = the run's number), out_off, blk_base (m + 1) and runs.
struct RtarPieces {
  RtarList l;
  const uint64_t* dpre;
  const TarEntry* ent;
  RtarWindow w;
  uint64_t begin, end;
};
hipError_t launch_rtar_pieces(const RtarPieces& p, MrgCount* cnt, const uint64_t* base,
                              pfscdc_slice* slices, uint64_t* out_off, uint64_t* blk_base,
                              RtarRun* runs, int num_cus, hipStream_t st);
// slices[j].chunk = table[slices[j].chunk] for j < m; *bad |= 1 (and chunk 0) for a slice that
// does not lie inside its chunk of the batch (chunk_offs: nchunks + 1 offsets)
hipError_t launch_rtar_chunks(pfscdc_slice* slices, uint64_t m, const uint32_t* table,
                              const uint64_t* chunk_offs, uint32_t nchunks, uint32_t* bad, int num_cus,
                              hipStream_t st);

// ---- the Source on the device (source_dev.cpp; kernels in list_kernels.hip §11) ----
struct SrcPred {  // SrcArg (source.h) with its strings on the device
  const char *name, *dir;
  uint32_t name_len, dir_len;
  uint32_t all, exclude_dir, child_flag;
  uint32_t glob;          // SrcGlob: 0 for the four kinds of the shared form
  const uint64_t* masks;  // kSrcGlobMasks: launch_src_glob's mask per input entry
};
enum SrcGlob : uint32_t {
  kSrcGlobNone = 0,
  kSrcGlobMasks = 1,  // selection and PFSCDC_INFO_MATCH from masks[]
  kSrcGlobRoot = 2,   // glob == "/": all is set, PFSCDC_INFO_MATCH on "/" alone
};
enum SrcBad : uint32_t {  // what the count pass found in the input
  kSrcUnordered = 1,  // not in (path, tag) order                    } the host arm
  kSrcUnclean = 2,    // a path that is not IsClean(p, IsDir(p))     } takes the
  kSrcDirTwice = 4,   // one directory path twice                    } call
  kSrcMalformed = 8,  // strings or DataRefs outside the arrays: PFSCDC_EINVAL
  kSrcNotLevel0 = 16, // an entry with a Range: PFSCDC_EINVAL
  kSrcTooDeep = 32,   // (launch_src_glob) a path of more than 63 '/': the host arm takes the call
};
// The glob pass, ahead of the count pass.  prog: GlobProgram's follow[64] and accept_byte[256]
// (glob.h) on the device.  masks[i] for input entry i: bit j = the bytes before the j-th '/' of
// its path are accepted (j = 0: the root, the empty string; a directory's own final '/' is one of
// them), bit 63 = a path that does not end in '/' is accepted as a whole; 0 for an entry outside
// the arrays.  *bad |= kSrcTooDeep.  Each path is walked once.
hipError_t launch_src_glob(const RtarList& in, const uint64_t* prog, uint64_t first, uint64_t last,
                           bool nullable, uint64_t* masks, uint32_t* bad, int num_cus,
                           hipStream_t st);
constexpr uint32_t kSrcDir = 0xffffffffu;  // SrcMeta::src of an inserted directory
struct SrcMeta {  // per output entry
  uint32_t src;    // the input entry it is, or kSrcDir
  uint32_t depth;  // the '/' in its path but for the last byte: "/" 0, "/a" and "/a/" 1
  uint64_t end;    // a directory's subtree is entries (own index, end); a file's end = index + 1
};
// cnt[i] = {entries, DataRefs, blob bytes} input entry i emits; *bad |= SrcBad (zeroed before)
hipError_t launch_src_count(const RtarList& in, const SrcPred& pr, MrgCount* cnt, uint32_t* bad,
                            int num_cus, hipStream_t st);
// the output entries, their strings and through copy[] the selected files' DataRefs into drs (the
// list passes' contract); meta (end unset), the infos' type, flags and file size, sizes[o] =
// {0, 0, file size}, maxdepth[0] and the directories inserted in maxdepth[1] (both zeroed before)
hipError_t launch_src_fill(const RtarList& in, const SrcPred& pr, const MrgCount* cnt,
                           const uint64_t* base, pfscdc_index_entry* entries, char* blob,
                           MrgCopy* copy, SrcMeta* meta, pfscdc_file_info* infos, MrgCount* sizes,
                           uint32_t* maxdepth, pfscdc_full_dataref* drs, int num_cus,
                           hipStream_t st);
// after launch_merge_scan of sizes into sbase: meta[].end and the directories' sizes
hipError_t launch_src_tree(const RtarList& out, SrcMeta* meta, const uint64_t* sbase,
                           pfscdc_file_info* infos, int num_cus, hipStream_t st);
// buf[32 k ...] = DataRef k's hash; segs[o] = entry o's DataRef hashes as one hash record
hipError_t launch_src_leaf(const RtarList& out, uint8_t* buf, pfscdc_segment* segs, int num_cus,
                           hipStream_t st);
hipError_t launch_src_leaf_copy(const SrcMeta* meta, const uint8_t* leaf, uint64_t n,
                                pfscdc_file_info* infos, int num_cus, hipStream_t st);
// cnt[o] = {depth == level + 1, directory of depth level, 0}
hipError_t launch_src_level_count(const SrcMeta* meta, const pfscdc_file_info* infos, uint64_t n,
                                  uint32_t level, MrgCount* cnt, int num_cus, hipStream_t st);
// after launch_merge_scan of cnt into base: the children's hashes into buf, one record per
// directory of depth level into segs
hipError_t launch_src_level_gather(const SrcMeta* meta, const pfscdc_file_info* infos,
                                   const uint64_t* base, uint64_t n, uint32_t level, uint8_t* buf,
                                   pfscdc_segment* segs, int num_cus, hipStream_t st);
// the digests into the infos: level < 0 the leaf pass's, else those of depth level's directories
hipError_t launch_src_scatter(const SrcMeta* meta, const uint64_t* base, const pfscdc_segment* segs,
                              uint64_t n, int level, pfscdc_file_info* infos, int num_cus,
                              hipStream_t st);

// ---- DiffFile on the device (diff_dev.cpp; kernels in list_kernels.hip §12) ----
struct DiffSide {  // a Source: its list and one info per entry
  RtarList l;
  const pfscdc_file_info* infos;
};
struct DiffRank {    // per entry of a side
  uint32_t partner;  // the entry of the other side the walk meets it with, or PFSCDC_DIFF_NONE
  uint32_t other;    // a: lower_bound of its path in b; b: upper_bound of its path in a
};
// One lane per entry of a (x < a.l.n) and of b: rank[x]; sel[x] = {1, DataRefs, blob bytes} if the
// entry occurs in a pair, else zeros; emit_b[j] = {1, 0, 0} if b's entry j is reported alone;
// *bad |= 1 (zeroed before) if a side's paths decrease: nothing else is then to be used.
hipError_t launch_diff_rank(const DiffSide& a, const DiffSide& b, DiffRank* rank, MrgCount* sel,
                            MrgCount* emit_b, uint32_t* bad, int num_cus, hipStream_t st);
// after launch_merge_scan of sel[0, na) into base_a and of emit_b into base_e: pairs[0, npairs)
hipError_t launch_diff_fill(uint64_t na, uint64_t nb, const DiffRank* rank, const MrgCount* sel,
                            const uint64_t* base_a, const MrgCount* emit_b, const uint64_t* base_e,
                            pfscdc_diff_pair* pairs, uint64_t npairs, int num_cus, hipStream_t st);
// a side's selected entries, their strings and infos, and through copy[] their DataRefs into drs
// (the list passes' contract, sel the counts)
hipError_t launch_diff_select(const DiffSide& in, const MrgCount* sel, const uint64_t* base,
                              pfscdc_index_entry* entries, char* blob, MrgCopy* copy,
                              pfscdc_file_info* infos, pfscdc_full_dataref* drs, int num_cus,
                              hipStream_t st);

// ---- CopyFile's selection and path transform (copy_map_dev.cpp; kernels in list_kernels.hip §13) ----
struct CmapPred {  // CopyArg (copy_map.h) with its strings on the device
  const char *src, *dst, *tag;  // cleanPath(src), cleanPath(dst), the source tag ("": every tag)
  uint32_t src_len, dst_len, tag_len, reserved;
};
// cnt[i] = {1, DataRefs, blob bytes} if input entry i is selected, else zeros; *bad |= SrcBad
// (zeroed before): kSrcMalformed, kSrcNotLevel0, kSrcUnordered, and kSrcUnclean for a selected
// path that is not IsClean(p, false) or whose new path exceeds 2^32 - 1 bytes
hipError_t launch_cmap_count(const RtarList& in, const CmapPred& pr, MrgCount* cnt, uint32_t* bad,
                             int num_cus, hipStream_t st);
// the selected entries with their new paths and tags, copy[] (the list passes' contract)
hipError_t launch_cmap_fill(const RtarList& in, const CmapPred& pr, const MrgCount* cnt,
                            const uint64_t* base, pfscdc_index_entry* entries, char* blob,
                            MrgCopy* copy, int num_cus, hipStream_t st);

}  // namespace pfscdc
