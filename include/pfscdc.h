/*
 * pfscdc.h — C ABI of the MI355X PFS chunk-ingest path (libpfscdc.so).
 *
 * Drop-in boundary for the reference's chunk layer.  The reference has no FFI on this path
 * (pure Go, no cgo); its seam is the Go type chunk.Writer.  Each entry point below names
 * the reference interface it replaces (paths under /root/reference).  Plain pointers and
 * sizes only; no torch or HIP types cross this boundary except the opaque stream handle.
 *
 * Status codes: 0 = ok, negative = error (PFSCDC_E*).  Errors are sticky on a writer, like
 * chunk.Writer.err (src/internal/storage/chunk/writer.go:145-161).
 * Threading: a ctx (and its writers) is owned by one thread at a time; one ctx per GPU;
 * distinct ctxs may run concurrently (independent chunk.Writers, chunk/storage.go:60-66).
 */
#ifndef PFSCDC_H
#define PFSCDC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFSCDC_OK 0
#define PFSCDC_EINVAL -1      /* bad argument */
#define PFSCDC_EHIP -2        /* HIP runtime error (see pfscdc_last_error) */
#define PFSCDC_ENOMEM -3      /* device or host allocation failed */
#define PFSCDC_EUNSUPPORTED -4 /* configuration the GPU path does not implement */
#define PFSCDC_ESTATE -5      /* call order violated (e.g. Write before Annotate) */
#define PFSCDC_ECALLBACK -6   /* the writer callback returned non-zero */
#define PFSCDC_ECORRUPT -7    /* a stored chunk failed verification (chunk.Get verifyData) */
#define PFSCDC_ENOTFOUND -8   /* a chunk id is not in the store */

/* chunk.WithRollingHashConfig(averageBits, seed) + chunk.WithMinMax(min, max)
 * (chunk/option.go:50-64); defaults writer.go:39-44: 23, 1, 1 MB, 20 MB (decimal). */
typedef struct pfscdc_params {
  uint32_t average_bits; /* split mask = 2^bits - 1, avg = 2^bits (1..32) */
  uint32_t reserved;
  int64_t seed;          /* buzhash64.GenerateHashes seed */
  int64_t min_chunk;     /* must be >= 64 (the window) on the GPU path */
  int64_t max_chunk;
} pfscdc_params;

/* One segment = the bytes of one file (annotation) inside one chunk = one DataRef
 * (writer.go:288-312: DataRef.Hash = BLAKE2b-256 of exactly these bytes). */
typedef struct pfscdc_segment {
  uint64_t offset;  /* offset of the segment inside its file */
  uint64_t size;    /* bytes */
  uint32_t file;    /* index of the file in the batch */
  uint32_t flags;   /* PFSCDC_SEG_* */
  uint8_t hash[32]; /* BLAKE2b-256 (pachhash.Sum, pachhash/hash.go:27-30) */
} pfscdc_segment;   /* 56 bytes */

/* Ref of the chunk a segment forms when each file is its own writer (the batch form): what
 * chunk.Create(ctx, CreateOptions{}, chunk, ...) stores (transform.go:26-46, client.go:57).
 * CreateOptions{} means no compression and an empty secret, so
 *   dek = BLAKE2b-256(BLAKE2b-256(chunk))      (deriveKey, transform.go:173-178)
 *   id  = BLAKE2b-256(ChaCha20_dek,nonce0(chunk)) (cryptoXOR :181-188, then Hash) */
typedef struct pfscdc_ref {
  uint8_t id[32];  /* Ref.Id */
  uint8_t dek[32]; /* Ref.Dek */
} pfscdc_ref;

#define PFSCDC_SEG_VALID 1u
#define PFSCDC_SEG_CUT 2u /* the segment ends on a CDC cut (else: at end of file) */

typedef struct pfscdc_ctx pfscdc_ctx;

/* Fills params with the reference defaults (writer.go:39-44). */
void pfscdc_default_params(pfscdc_params* p);

/* buzhash64.GenerateHashes(seed) (called at chunk/option.go:54). */
int pfscdc_table(int64_t seed, uint64_t out[256]);

/* First n values of Go's rand.NewSource(seed).Int63() (known-answer hook for tests). */
int pfscdc_go_int63(int64_t seed, int64_t* out, int n);

/* Replaces chunk.Storage.NewWriter's per-writer config (chunk/storage.go:60-66,
 * writer.go:74-98): binds params and a GPU.  device = HIP ordinal. */
int pfscdc_ctx_create(const pfscdc_params* params, int device, pfscdc_ctx** out);
int pfscdc_ctx_destroy(pfscdc_ctx* ctx);
const char* pfscdc_last_error(const pfscdc_ctx* ctx);

/* Run every following GPU call of ctx on this hipStream_t (NULL = the ctx's own stream). */
int pfscdc_set_stream(pfscdc_ctx* ctx, void* hip_stream);

/* Ordering rule for device-resident inputs: the ctx's stream is a non-blocking stream of its
 * own, so a device buffer written by work on another stream (a kernel, a non-blocking copy)
 * must be ordered before a call that reads it.  pfscdc_stream_wait makes every following GPU
 * call of ctx wait for the work already enqueued on hip_stream (NULL = the legacy default
 * stream); it does not block the host.  The Python binding calls it with torch's current
 * stream before each call on a torch tensor. */
int pfscdc_stream_wait(pfscdc_ctx* ctx, void* hip_stream);
/* The hipStream_t the ctx enqueues on (its own, or the one given to pfscdc_set_stream), e.g.
 * for pfscdc_stream_wait(other_ctx, pfscdc_stream_handle(ctx)): every later call of other_ctx
 * runs after the work ctx has enqueued so far. */
void* pfscdc_stream_handle(const pfscdc_ctx* ctx);

/* Steps in flight on two ctxs of one GPU: every later scan of ctx starts its BLAKE2b kernel
 * only after the BLAKE2b kernel last enqueued by other (NULL: no ordering).  The next step's
 * candidate scan still fills the CUs the current hash frees as its queue drains, but two
 * hashes never share the SIMDs, so each hash launch runs for its own duration.  other must
 * outlive the ordering (set NULL before destroying it). */
int pfscdc_order_hash_after(pfscdc_ctx* ctx, pfscdc_ctx* other);

/* CDC + content hash of a batch of files (one annotation each, concatenated).
 * Replaces, for every file of the batch, Writer.Annotate + Writer.Write + the hash part of
 * processChunk (writer.go:118-143,163-196,233-253,288-312): per-file cut positions and
 * per-segment BLAKE2b-256.  bytes: nbytes bytes, device pointer (16-B aligned) if
 * bytes_on_device else host memory (copied with hipMemcpyAsync).  file_offsets: host array
 * of nfiles+1 nondecreasing offsets, file_offsets[0] == 0, file_offsets[nfiles] == nbytes.
 * Blocks until the segment records are on the host; read them with pfscdc_segments. */
int pfscdc_scan(pfscdc_ctx* ctx, const void* bytes, uint64_t nbytes, int bytes_on_device,
                const uint64_t* file_offsets, uint32_t nfiles);

/* Asynchronous form: enqueue on the ctx stream; pfscdc_wait() completes it. */
int pfscdc_scan_async(pfscdc_ctx* ctx, const void* bytes, uint64_t nbytes,
                      int bytes_on_device, const uint64_t* file_offsets, uint32_t nfiles);
int pfscdc_wait(pfscdc_ctx* ctx);

/* Results of the last completed scan, ordered by (file, offset).  Valid until the next
 * scan on ctx.  seg_begin[f]..seg_begin[f+1] index file f's segments (nfiles+1 entries). */
uint64_t pfscdc_num_segments(const pfscdc_ctx* ctx);
const pfscdc_segment* pfscdc_segments(const pfscdc_ctx* ctx);
const uint64_t* pfscdc_file_segment_begin(const pfscdc_ctx* ctx);

/* Options of every following scan on ctx (bit set).  PFSCDC_OPT_REF_IDS: also compute each
 * segment's pfscdc_ref (a second BLAKE2b pass over the ChaCha20 ciphertext, fused). */
#define PFSCDC_OPT_REF_IDS 1u
/* PFSCDC_OPT_CUTS_ONLY: the scan finds the segments (cut positions) but leaves their DataRef
 * hashes to a following pfscdc_commit_refs, which computes them in one launch together with
 * the formed chunks' content hashes. */
#define PFSCDC_OPT_CUTS_ONLY 2u
/* PFSCDC_OPT_CTEXT_IN_PLACE: pfscdc_commit_refs writes every chunk's ciphertext (the object
 * chunk.Create uploads, ChaCha20_dek(chunk)) over the chunk's plaintext in the caller's device
 * buffer, which then holds the upload stream.  The commit needs no second buffer of its size
 * (a 200 GiB commit on one 288 GB GPU), and the Ref.Id pass can always take the split form.
 * Needs the scan over caller-owned device bytes. */
#define PFSCDC_OPT_CTEXT_IN_PLACE 4u
int pfscdc_set_options(pfscdc_ctx* ctx, uint32_t options);
/* Refs of the last completed scan, aligned with pfscdc_segments (NULL unless the scan ran
 * with PFSCDC_OPT_REF_IDS). */
const pfscdc_ref* pfscdc_refs(const pfscdc_ctx* ctx);
/* Device time (ms) of the last scan's Ref.Id kernels (0 without PFSCDC_OPT_REF_IDS). */
int pfscdc_last_ref_ms(pfscdc_ctx* ctx, float* ms);

/* chunk.Get (transform.go:50-78) for a batch of stored chunks, the GetFile read path: for
 * chunk i (bytes [chunk_offsets[i], chunk_offsets[i+1]) of ctext) compute BLAKE2b-256 of the
 * stored bytes, set ok[i] = 1 iff it equals refs[i].id (verifyData), and write the ChaCha20
 * decryption with refs[i].dek to the same range of ptext (CreateOptions{} never compresses).
 * ctext/ptext: device pointers if *_on_device (16-B aligned ctext), else host memory.
 * Returns PFSCDC_OK even when some chunk fails verification (see ok[]). */
int pfscdc_get_chunks(pfscdc_ctx* ctx, const void* ctext, uint64_t nbytes, int ctext_on_device,
                      const uint64_t* chunk_offsets, uint32_t nchunks, const pfscdc_ref* refs,
                      void* ptext, int ptext_on_device, uint8_t* ok);
/* Device time (ms) of the last pfscdc_get_chunks kernels (after the input copy). */
int pfscdc_last_get_ms(pfscdc_ctx* ctx, float* ms);

/* One DataRef's bytes inside a batch of stored chunks: bytes [offset, offset + size) of the
 * plaintext of chunk `chunk` (DataRef.OffsetBytes / SizeBytes, chunk.proto). */
typedef struct pfscdc_slice {
  uint32_t chunk;    /* index into chunk_offsets / refs */
  uint32_t reserved;
  uint64_t offset;   /* DataRef.OffsetBytes */
  uint64_t size;     /* DataRef.SizeBytes (0 is legal and writes nothing) */
} pfscdc_slice;      /* 24 bytes */

/* chunk.Reader.Get (reader.go:43-48; per DataRef DataReader.Get, reader.go:72-79) over a
 * batch of stored chunks (ctext, chunk_offsets, refs as for pfscdc_get_chunks): out receives,
 * back to back in slice order, the plaintext bytes [offset, offset + size) of each slice's
 * chunk.  Slices may name chunks in any order, repeat and overlap.  Every chunk that a slice
 * names is verified once
 * (BLAKE2b-256 of the stored bytes against refs[c].id, verifyData, transform.go:207-215) unless
 * verified[c] != 0 (verified NULL = verify all): a chunk the caller has verified before counts
 * as ok and is not hashed again, the memCache hit of chunk.Get (transform.go:50-53).  ChaCha20
 * is seekable (RFC 8439 §2.4, zero nonce, block counter = offset / 64, transform.go:159-170), so
 * only the 64-byte keystream blocks that a slice touches are computed and only the slices'
 * bytes are read and written: a 4 KiB file packed into an 8 MB chunk costs 4 KiB of decryption.
 * chunk_ok[c] (nchunks entries): 1 iff chunk c was verified now or marked verified; a chunk no
 * slice names is not hashed and reports its verified mark.  slice_ok (nullable, nslices
 * entries) = chunk_ok of the slice's chunk.  The bytes of a slice whose chunk is not ok are
 * zeros: nothing decrypted from unverified ciphertext reaches out.
 * ctext: device pointer (16-B aligned) if ctext_on_device, else host memory.  out: device
 * pointer if out_on_device, else host memory, of sum(size) bytes at any alignment; when both are
 * device pointers they must not overlap.  PFSCDC_EINVAL for a slice with chunk >= nchunks or
 * offset + size beyond its chunk.  Returns PFSCDC_OK even when some chunk fails verification
 * (see chunk_ok).  Synchronous on the ctx stream (ordering: pfscdc_stream_wait). */
int pfscdc_read_slices(pfscdc_ctx* ctx, const void* ctext, uint64_t nbytes, int ctext_on_device,
                       const uint64_t* chunk_offsets, uint32_t nchunks, const pfscdc_ref* refs,
                       const uint8_t* verified, const pfscdc_slice* slices, uint32_t nslices,
                       void* out, int out_on_device, uint8_t* chunk_ok, uint8_t* slice_ok);
/* Device time (ms) of the last pfscdc_read_slices / pfscdc_store_read: out[0] verification (the
 * hash pass and the id compare), out[1] the sliced decrypt-and-gather kernel. */
int pfscdc_last_read_timings(pfscdc_ctx* ctx, float out[2]);

/* ---- GetFileTAR (api_server.go:508-531,578-593; fileset/util.go:42-53; tarutil/tar.go:35-40) --
 * The stream getFileTar writes for files f_0 .. f_{n-1}: per file a 512-byte USTAR header as
 * Go's archive/tar forms it for Header{Name, Size} (every other field zero), the file's bytes,
 * zeros to the next multiple of 512; after the last file 1,024 zero bytes.  total =
 * sum(512 + roundup512(size_i)) + 1024.  The header layout is restated from archive/tar's
 * source; like everything else here it has not been held against a Go run (README "Scope and
 * correctness"), and Python's tarfile reads the stream back.
 * The entries Go writes PAX records for: a name that is not pure ASCII 0x01-0x7F, a name longer
 * than 100 bytes that splitUSTARPath cannot split (prefix <= 155 and suffix 1-100 bytes around a
 * '/'), a size above 077777777777 (8 GiB - 1).  With the format PFSCDC_TAR_USTAR, the default,
 * every entry point below returns PFSCDC_EUNSUPPORTED for them and those with a ctx name the
 * file in pfscdc_last_error.  With PFSCDC_TAR_USTAR | PFSCDC_TAR_PAX such an entry, and no
 * other, gets the head archive/tar's FormatPAX writes in front of its content: an extended
 * header block (typeflag 'x', named dir/PaxHeaders.0/file without its non-ASCII bytes, cut at
 * 100), the records "<n> path=<name>\n" (a name that is not ASCII or longer than 100 bytes) and
 * "<n> size=<decimal>\n" (a size above 8 GiB - 1) padded to a multiple of 512, and the main
 * header block with no prefix, the name without its non-ASCII bytes cut at 100, and a size field
 * of zeros where the size does not fit: 512 + roundup512(records) + 512 bytes where a USTAR
 * entry has 512.  An entry USTAR can hold is written as before, so a stream with no such entry
 * is the same bytes under either format.  Restated from archive/tar's source (Go 1.16) and read
 * back by Python's tarfile, not held against a Go run; DESIGN.md §5 lists what to confirm.
 * Not implemented under either format (PFSCDC_EUNSUPPORTED): a PAX entry whose name has an
 * empty, "." or ".." component (a leading '/' and a directory's trailing '/' aside), which
 * path.Join would rewrite in the extended header's name (PFS cleans every index path, so no
 * written commit has one), and a PAX entry's name above 65,535 bytes (the entry record's name
 * length is 16 bits; the USTAR rules bound every other name at 256).
 * PFSCDC_EINVAL: an empty name, or a directory (name ending in '/') that has pieces or a
 * size. */
#define PFSCDC_TAR_USTAR 1 /* USTAR entries only: what USTAR cannot hold is refused */
#define PFSCDC_TAR_PAX 2   /* with PFSCDC_TAR_USTAR: such an entry is written in PAX format */
typedef struct pfscdc_tar_file {
  const char* path;  /* index.Index.Path, NUL-terminated */
  uint32_t first;    /* its pieces are [first, first + count) of the slice / DataRef array */
  uint32_t count;
} pfscdc_tar_file;

/* The header block of one entry.  Host only: the specification tar_frame_kernel is tested
 * against. */
int pfscdc_tar_header(const char* path, uint64_t size, uint8_t out[512]);
/* Where the entries lie: sizes[i] = file i's size (the sum of its pieces' sizes);
 * entry_offsets (nfiles + 1 entries, nullable): entry i = stream bytes [entry_offsets[i],
 * entry_offsets[i + 1]), the trailer begins at entry_offsets[nfiles]; *total the stream's
 * length.  Host only: what a caller sizes its buffers and windows with. */
int pfscdc_tar_layout(const pfscdc_tar_file* files, uint32_t nfiles, const uint64_t* sizes,
                      uint64_t* entry_offsets, uint64_t* total);
/* The head of one entry under format (PFSCDC_TAR_USTAR, or PFSCDC_TAR_USTAR | PFSCDC_TAR_PAX;
 * anything else PFSCDC_EINVAL): every byte in front of its content, *len of them (512 for an
 * entry USTAR can hold, then the bytes of pfscdc_tar_header), into out[0, cap) (out NULL: only
 * *len; cap < *len: PFSCDC_EINVAL).  Host only: the specification tar_frame_kernel is tested
 * against. */
int pfscdc_tar_head(const char* path, uint64_t size, int format, uint8_t* out, uint64_t cap,
                    uint64_t* len);
/* pfscdc_tar_layout under format: an entry spans its head, its content and the padding. */
int pfscdc_tar_layout_format(const pfscdc_tar_file* files, uint32_t nfiles, const uint64_t* sizes,
                             int format, uint64_t* entry_offsets, uint64_t* total);
/* The format of every later pfscdc_read_tar, pfscdc_store_read_tar, pfscdc_dev_list_tar_layout
 * and pfscdc_dev_list_read_tar on ctx.  Not a knob: it changes the stream (for the entries named
 * above, and for no other).  A resident list keeps the plan of the format it was last laid out
 * under and plans again when the format has changed. */
int pfscdc_set_tar_format(pfscdc_ctx* ctx, int format);
/* Stream bytes [begin, min(begin + len, total)) of the files' tar stream into out (*nwritten of
 * them, nullable), over a batch of stored chunks as pfscdc_read_slices takes it: file i's
 * content is the concatenation of slices [first, first + count).  begin must be a multiple of
 * 512, and so must len unless the window reaches the end of the stream, so a header is never
 * cut; content is cut anywhere.  The slices are clipped to the window on the host: only the
 * chunks the clipped slices name are uploaded (host ctext) and verified (unless verified[c]),
 * and only the window's content bytes are decrypted, straight to their place in the stream
 * (pfscdc_read_slices' gather kernel).  Headers, padding and trailer are formed on the device
 * by tar_frame_kernel from each file's name and size; every byte of the window is written
 * exactly once and out is never cleared first.  chunk_ok as for pfscdc_read_slices; the content
 * bytes of a chunk that is not ok are zeros, the headers are written all the same.
 * out: device pointer if out_on_device, else host memory, at any alignment.  Window and name
 * errors are returned before any GPU call.  Synchronous on the ctx stream, as
 * pfscdc_read_slices. */
int pfscdc_read_tar(pfscdc_ctx* ctx, const void* ctext, uint64_t nbytes, int ctext_on_device,
                    const uint64_t* chunk_offsets, uint32_t nchunks, const pfscdc_ref* refs,
                    const uint8_t* verified, const pfscdc_tar_file* files, uint32_t nfiles,
                    const pfscdc_slice* slices, uint32_t nslices, uint64_t begin, uint64_t len,
                    void* out, int out_on_device, uint8_t* chunk_ok, uint64_t* nwritten);
/* Device time (ms) tar_frame_kernel took in the last pfscdc_read_tar / pfscdc_store_read_tar
 * (0 after a read without framing); verification and gather are pfscdc_last_read_timings'. */
int pfscdc_last_frame_ms(pfscdc_ctx* ctx, float* ms);

/* chunk.Create(ctx, CreateOptions{}, chunk, createFunc) (transform.go:26-46) for a batch of
 * formed chunks, the upload half of processChunk (writer.go:233-271): chunk i is bytes
 * [chunk_offsets[i], chunk_offsets[i+1]) (offsets as for pfscdc_get_chunks).  refs[i] gets
 * Ref.Dek = Hash(Hash(chunk)) and Ref.Id = Hash(ChaCha20_dek(chunk)).  content_hashes
 * (NULL or 32 B per chunk) is Hash(chunk) (chunkDataRef.Hash, writer.go:240): taken as
 * given where hash_known[i] != 0 (e.g. a single-DataRef chunk, whose hash the scan already
 * has), computed and written back otherwise.  Blocks until refs are on the host.
 * The Ref.Id pass runs fused (keystream on the BLAKE2b chain) or split (a parallel ChaCha20
 * pass into a ctx-owned ciphertext copy, then BLAKE2b of it) when nchunks cannot fill the
 * GPU and 8 GiB of device memory stay free; the environment variable PFSCDC_REFID_SPLIT=0/1
 * forces either.  Same results either way. */
int pfscdc_create_refs(pfscdc_ctx* ctx, const void* bytes, uint64_t nbytes, int bytes_on_device,
                       const uint64_t* chunk_offsets, uint32_t nchunks, uint8_t* content_hashes,
                       const uint8_t* hash_known, pfscdc_ref* refs);
/* The commit data plane's hashing in one pass, after a scan made with PFSCDC_OPT_CUTS_ONLY
 * over the same bytes and pfscdc_form_chunks: every segment's DataRef hash (writer.go:301-312,
 * into segment_hashes, 32 B each in pfscdc_segments order) and every chunk's content hash
 * (content_hashes out; a chunk with hash_known[i] != 0 is one segment, and its hash is that
 * segment's) run as one BLAKE2b launch in longest-first order, so the two independent sets of
 * serial chains share the GPU instead of running one pass after the other; then
 * chunk.Create's dek and Ref.Id as pfscdc_create_refs.  refs as pfscdc_create_refs, or NULL:
 * then only the hashes (every BLAKE2b Writer.processChunk computes, writer.go:240,301-312)
 * and no chunk.Create.  With refs and more chunks than the quads of one wave per SIMD, the
 * long chunks (and their Ref.Ids) run on the ctx stream beside the rest on a second one, so
 * their Ref.Id chains start as soon as their own content hashes are done (same results;
 * PFSCDC_COMMIT_TWO_SETS=0/1 forces either form).
 * Synchronous; the scan's segment list is consumed (pfscdc_segments is empty afterwards). */
int pfscdc_commit_refs(pfscdc_ctx* ctx, const void* bytes, uint64_t nbytes, int bytes_on_device,
                       const uint64_t* chunk_offsets, uint32_t nchunks, uint8_t* content_hashes,
                       const uint8_t* hash_known, pfscdc_ref* refs, uint8_t* segment_hashes);
/* hashDataRefs (fileset/util.go:149-158): FileInfo.Hash = BLAKE2b-256 over the n concatenated
 * 32-byte DataRef hashes (host array), computed by the hash kernel. */
int pfscdc_hash_data_refs(pfscdc_ctx* ctx, const uint8_t* hashes, uint32_t n, uint8_t out[32]);
/* Device time (ms) of the last chunk.Create batch (pfscdc_create_refs or a writer flush). */
int pfscdc_last_create_ms(pfscdc_ctx* ctx, float* ms);
/* Its split: out[0] content-hash pass, out[1] Ref.Id pass (dek, ChaCha20, BLAKE2b). */
int pfscdc_last_create_timings(pfscdc_ctx* ctx, float out[2]);
/* The form its Ref.Id pass took on this ctx: *split = 0 fused ChaCha20 + BLAKE2b, 1 a ChaCha20
 * pass then BLAKE2b of the ciphertext, -1 no batch yet (the library chooses by chunk count,
 * see the PFSCDC_REFID_SPLIT knob). */
int pfscdc_last_create_form(pfscdc_ctx* ctx, int* split);

/* ---- one stream split across GPUs (writer.go:163-189 block-parallel) --------
 * A stream of N bytes is cut into equal byte ranges, one per GPU.  The rolling hash at a
 * position is a pure function of the 64 bytes ending there, so each GPU finds the candidate
 * positions of its range from its bytes plus the 64 bytes in front (the halo); the serial
 * min/max selection then runs once over the gathered, sorted candidates (cheap: ~1 per 8 MiB),
 * and each segment is hashed by the GPU whose range holds its first byte, after the bytes of a
 * segment that straddles the border are copied over from the next range. */

/* Candidates of one range: every position p of bytes (halo <= p < nbytes, p >= 63) where the
 * buzhash64 of bytes [p-63, p] has (h & mask) == 0, sorted ascending, as offsets into bytes.
 * halo (<= 64) = the bytes in front of the range copied from the previous one (0 at the
 * stream start, where positions < 63 are never candidates: min >= 64 puts them before the
 * first eligible cut).  out: cap entries; *n = the count (PFSCDC_ENOMEM if > cap, out holds
 * the first cap).  Tiles with more than 15 candidates are re-rolled exactly on the host.
 * Timings: pfscdc_last_timings out[0] (scan, compaction included). */
int pfscdc_candidates(pfscdc_ctx* ctx, const void* bytes, uint64_t nbytes, int bytes_on_device,
                      uint64_t halo, uint64_t* out, uint64_t cap, uint64_t* n);

/* BLAKE2b-256 of n byte ranges [begins[i], begins[i] + sizes[i]) of bytes (device pointer,
 * 16-B aligned, if bytes_on_device), into out (32 B each): the DataRef hashes of segments
 * whose cuts were selected elsewhere (writer.go:240,301-312).  Synchronous. */
int pfscdc_hash_ranges(pfscdc_ctx* ctx, const void* bytes, uint64_t nbytes, int bytes_on_device,
                       const uint64_t* begins, const uint64_t* sizes, uint32_t n, uint8_t* out);

/* Candidate positions (h & mask == 0, absolute offset >= 63) found by the last scan, sorted;
 * positions inside dense tiles are reported through the tile marker instead.  Positions the
 * scan skipped (see pfscdc_last_scan_bytes) are never listed.  Debug/test hook for the
 * candidate-scan kernel. */
uint64_t pfscdc_debug_candidates(pfscdc_ctx* ctx, uint64_t* out, uint64_t cap);

/* Two more test hooks, valid after a completed scan (pfscdc_wait) and before the next call
 * that stages records on the ctx; neither is part of the product path.
 *
 * The hash queue the last scan built: order[0, qlen) are segment indices in dispatch order;
 * next[0, nseg) are the hash bins' links (0xffffffff: none).  *bin_bytes = the bin size
 * that scan used (0: no bins, next is then left alone).  At most order_cap / next_cap words
 * are written.  Returns qlen. */
uint64_t pfscdc_debug_hash_queue(pfscdc_ctx* ctx, uint32_t* order, uint64_t order_cap,
                                 uint32_t* next, uint64_t next_cap, uint64_t* bin_bytes);
/* The cut-skipping plan's dispatch slots, 3 words each: unit, file, skip | rank << 8 (skip in
 * 8 KiB steps of the 256 KiB unit, rank clamped at 255), in dispatch order; at most cap slots
 * are written.  Returns their number (0: the scan ran without a plan). */
uint64_t pfscdc_debug_scan_plan(pfscdc_ctx* ctx, uint32_t* slots, uint64_t cap);

/* Bytes the last pfscdc_scan's candidate kernel actually rolled.  Writer.roll never cuts in
 * the first min - 1 bytes after an Annotate (writer.go:125-128,167-170), so the scan skips
 * that part of every file (in 8 KiB steps of its work units) and the count is below nbytes
 * when files are longer than min; results are unchanged.  With min - 1 >= 256 KiB it also
 * skips the min - 1 positions after every cut of a file that the scan has already settled
 * (its work units go out in rank order and report per file), so the count then also depends
 * on timing.  The knob PFSCDC_SCAN_CUTSKIP=0 keeps only the first skip; PFSCDC_SCAN_SKIP=0
 * rolls every byte (pfscdc_last_scan_mode tells which skipping the last scan did). */
int pfscdc_last_scan_bytes(pfscdc_ctx* ctx, uint64_t* out);

/* Device timing of the last scan's kernels (ms, HIP events on the ctx stream):
 * out[0] candidate scan (its last workgroup also compacts the candidates), out[1] 0 (the
 * compaction used to be a launch of its own), out[2] selection (its last workgroup also
 * compacts the segment list and builds the hash queue's LPT order), out[3] BLAKE2b,
 * out[4] total.  An interval between two events includes any time the kernel waited for
 * free CUs behind work of another stream. */
int pfscdc_last_timings(pfscdc_ctx* ctx, float out[5]);
/* Execution spans of the last scan's two main kernels (ms): out[0] the candidate scan, out[1]
 * the BLAKE2b kernel, each from its first wavefront's start to its last wavefront's end
 * (s_memrealtime in the kernels), so a kernel queued behind another stream's work is not
 * charged for the wait — the per-launch duration a kernel-trace profiler reports. */
int pfscdc_last_kernel_spans(pfscdc_ctx* ctx, float out[2]);
/* Shader clock (MHz) the last scan's two main kernels ran at: out[0] the candidate scan,
 * out[1] the BLAKE2b kernel; each the sum over its waves of their lifetimes in shader cycles
 * (s_memtime) divided by the same in wall-clock ticks (s_memrealtime).  The chip lowers its
 * clock under load, so an instruction-issue ceiling is priced at this clock. */
int pfscdc_last_kernel_clocks(pfscdc_ctx* ctx, float out[2]);

/* Pinned host memory for staging (PCIe-inclusive end-to-end path). */
void* pfscdc_host_alloc(uint64_t nbytes);
void pfscdc_host_free(void* p);

/* Synthetic data generator used by bench/tests (device-side): word k of file f is
 * splitmix64-finalize((f << 40 | k) + (seed + 1) * 0x9E3779B97F4A7C15), little endian.
 * Writes every file of file_offsets into dev_bytes on the ctx stream. */
int pfscdc_fill_synthetic(pfscdc_ctx* ctx, void* dev_bytes, const uint64_t* file_offsets,
                          uint32_t nfiles, uint64_t seed);

/* Dedup-heavy variants (BASELINE configs[4]).  With m(x) the murmur3 64-bit finalizer:
 *  PFSCDC_SYNTH_DEDUP_BLOCKS: the 1 MiB block k of file f is, when
 *    h = m((seed << 48) ^ (f << 24) ^ k ^ 0xC5C5C5C5) is odd, a copy of pooled block
 *    (h >> 1) & 63, whose word w is splitmix64-finalize(((2^23 + id) << 40 | w) + gamma);
 *  PFSCDC_SYNTH_DEDUP_FILES: the same decision per whole file with
 *    h = m((seed << 48) ^ (f << 24) ^ 0x5EEDF11E), the pooled file's words indexed from 0. */
#define PFSCDC_SYNTH_RANDOM 0u
#define PFSCDC_SYNTH_DEDUP_BLOCKS 1u
#define PFSCDC_SYNTH_DEDUP_FILES 2u
int pfscdc_fill_synthetic_ex(pfscdc_ctx* ctx, void* dev_bytes, const uint64_t* file_offsets,
                             uint32_t nfiles, uint64_t seed, uint32_t mode);
/* The same bytes for pieces of files: piece i (bytes [piece_offsets[i], piece_offsets[i+1])
 * of dev_bytes) holds bytes [file_starts[i], ...) of file file_ids[i] (NULL ids: file i;
 * NULL starts: from byte 0).  A rank generates just its pieces of a commit whose files are
 * cut across serialized filesets or ranks. */
int pfscdc_fill_synthetic_pieces(pfscdc_ctx* ctx, void* dev_bytes, const uint64_t* piece_offsets,
                                 uint32_t npieces, const uint32_t* file_ids,
                                 const uint64_t* file_starts, uint64_t seed, uint32_t mode);

/* ---- chunk.Writer mirror (writer.go:52-438) ------------------------------------------
 * A writer buffers annotated bytes in host memory, runs them through pfscdc_scan in
 * batches of whole files, assembles chunks exactly as createChunk/Annotate do (including
 * multi-file chunks, the buf.Len() >= avg cut before a file, edge flags and the empty last
 * chunk of Close) and invokes the callback serially in chunk order, like TaskChain
 * (chunk/chain.go:55-68). */

typedef struct pfscdc_dataref {
  uint8_t hash[32];      /* DataRef.Hash */
  int64_t offset_bytes;  /* DataRef.OffsetBytes (offset inside the chunk) */
  int64_t size_bytes;    /* DataRef.SizeBytes */
} pfscdc_dataref;

typedef struct pfscdc_chunk_ref {
  uint64_t chunk_index;  /* 0-based order of createChunk calls */
  int64_t size_bytes;    /* Ref.SizeBytes (== plaintext size: CreateOptions{} => no gzip) */
  int32_t edge;          /* Ref.Edge = first || last (writer.go:200) */
  int32_t has_ref;       /* ref below is set (the writer was created with PFSCDC_OPT_REF_IDS) */
  pfscdc_ref ref;        /* Ref.Id / Ref.Dek of the whole chunk (maybeUpload, writer.go:255-271) */
  int32_t copied;        /* 1: a cheap copy (maybeCheapCopy, writer.go:403-420): no new chunk;
                            the annotations' DataRefs point into the existing chunk whose
                            Ref this is (has_ref = 1, chunk_index = -1) */
  int32_t reserved2;
} pfscdc_chunk_ref;

typedef struct pfscdc_annotation_out {
  uint64_t user;         /* Annotation.Data: the id passed to pfscdc_writer_annotate */
  int32_t has_data_ref;  /* 0 => NextDataRef == nil (size-0 piece) */
  int32_t reserved;
  pfscdc_dataref data_ref;
} pfscdc_annotation_out;

/* WriterCallback (writer.go:31): annotations of one chunk, in order.  Non-zero aborts. */
typedef int (*pfscdc_writer_cb)(void* user, const pfscdc_chunk_ref* chunk,
                                const pfscdc_annotation_out* annotations, uint32_t n);

typedef struct pfscdc_writer pfscdc_writer;

/* A DataRef with its chunk's Ref (what fileset indexes store, chunk.proto DataRef). */
typedef struct pfscdc_full_dataref {
  pfscdc_ref ref;       /* Ref.Id, Ref.Dek */
  int64_t ref_size;     /* Ref.SizeBytes */
  int32_t edge;         /* Ref.Edge */
  int32_t reserved;
  pfscdc_dataref data;  /* Hash, OffsetBytes, SizeBytes */
} pfscdc_full_dataref;

/* In-memory chunk store (the chunk client's object store, keyed by Ref.Id: client.go
 * Create/Get).  Writers with a store upload the ciphertext of every new chunk (deduplicated
 * by id) and read chunks back for Copy. */
typedef struct pfscdc_store pfscdc_store;
int pfscdc_store_create(pfscdc_store** out);
int pfscdc_store_destroy(pfscdc_store* s);
int pfscdc_store_put(pfscdc_store* s, const uint8_t id[32], const void* ctext, uint64_t n);
int pfscdc_store_get(const pfscdc_store* s, const uint8_t id[32], const void** ctext,
                     uint64_t* n);
uint64_t pfscdc_store_count(const pfscdc_store* s);
/* chunk.Storage.NewReader(ctx, dataRefs).Get(w) (storage.go:50-55, reader.go:43-48) against a
 * store, the call under every GetFile: out receives the concatenation of the n DataRefs' bytes
 * (*nwritten of them, nullable).  The distinct chunks of drs (by Ref.Id) are uploaded once and
 * verified once each, however many DataRefs share them, then gathered by pfscdc_read_slices'
 * kernel.  out: device pointer if out_on_device, else host memory, out_cap bytes.
 * PFSCDC_ENOTFOUND: a Ref.Id is not in the store.  PFSCDC_ECORRUPT: a chunk fails verification
 * or its stored length differs from ref_size; nothing is then written to out.  PFSCDC_EINVAL: a
 * DataRef reaching past its ref_size, or out_cap below the DataRefs' total size. */
int pfscdc_store_read(pfscdc_ctx* ctx, const pfscdc_store* s, const pfscdc_full_dataref* drs,
                      uint32_t n, void* out, uint64_t out_cap, int out_on_device,
                      uint64_t* nwritten);
/* getFileTar against a store: pfscdc_read_tar's window over files whose pieces are the DataRefs
 * drs[first, first + count).  The batch is the distinct chunks of the DataRefs that meet the
 * window, uploaded and verified once each.  out_cap: bytes out can take, at least the window's.
 * Errors as pfscdc_store_read's (PFSCDC_ENOTFOUND / PFSCDC_ECORRUPT: nothing is written to out)
 * and pfscdc_read_tar's. */
int pfscdc_store_read_tar(pfscdc_ctx* ctx, const pfscdc_store* s, const pfscdc_tar_file* files,
                          uint32_t nfiles, const pfscdc_full_dataref* drs, uint32_t ndrs,
                          uint64_t begin, uint64_t len, void* out, uint64_t out_cap,
                          int out_on_device, uint64_t* nwritten);

/* batch_bytes: flush threshold for buffered file bytes (0 = 1 GiB).  If ctx has
 * PFSCDC_OPT_REF_IDS set when the writer is created, every chunk also gets its Ref
 * (pfscdc_create_refs over the assembled chunk bytes, multi-file chunks and chunks that span
 * flushes included); the writer's own scans never compute per-segment refs. */
int pfscdc_writer_create(pfscdc_ctx* ctx, pfscdc_writer_cb cb, void* user,
                         uint64_t batch_bytes, pfscdc_writer** out);
int pfscdc_writer_annotate(pfscdc_writer* w, uint64_t user);            /* writer.go:118 */
int pfscdc_writer_write(pfscdc_writer* w, const void* data, uint64_t n); /* writer.go:132 */
int pfscdc_writer_close(pfscdc_writer* w);                               /* writer.go:423 */
int64_t pfscdc_writer_chunk_count(const pfscdc_writer* w);               /* writer.go:113 */
int64_t pfscdc_writer_annotation_count(const pfscdc_writer* w);          /* writer.go:107 */
int pfscdc_writer_destroy(pfscdc_writer* w);

/* The writer's chunk client: Copy reads chunks from store (chunk.Get: verify + decrypt on
 * the GPU); with upload != 0 every new chunk's ciphertext is stored (needs Ref ids, i.e.
 * PFSCDC_OPT_REF_IDS on the ctx; WithNoUpload = upload 0). */
int pfscdc_writer_set_store(pfscdc_writer* w, pfscdc_store* store, int upload);
/* Writer.Copy(dataRef) (writer.go:315-420): consecutive whole-chunk DataRefs at a chunk
 * boundary are buffered and passed through by reference (cheap copy, a callback with
 * chunk.copied = 1); anything else is read back and re-rolled like written bytes. */
int pfscdc_writer_copy(pfscdc_writer* w, const pfscdc_full_dataref* dr);
/* Optional hint before a run of Copies: verifies and decrypts, in one batch, every chunk
 * those DataRefs will certainly be re-rolled from (edge chunks, DataRefs not starting at
 * offset 0), so their BLAKE2b chains run in parallel instead of one per Copy. */
int pfscdc_writer_prefetch(pfscdc_writer* w, const pfscdc_full_dataref* drs, uint32_t n);
/* MergeFileReader.Hash (fileset/merge.go:125-143): a fresh writer on ctx (no upload), one
 * annotation, Copy of every DataRef, Close; out = BLAKE2b-256 over the resolved DataRefs'
 * hashes (hashDataRefs, fileset/util.go:149-158). */
int pfscdc_merge_file_hash(pfscdc_ctx* ctx, pfscdc_store* store, const pfscdc_full_dataref* drs,
                           uint32_t n, uint8_t out[32]);

/* Chunk formation over a device-resident batch: the chunks chunk.Writer would create
 * (Annotate cut, CDC cuts, Close's last chunk: writer.go:118-130,198-231,423-438) for the
 * files of the last pfscdc_scan, each stream k = files [stream_file_begin[k],
 * stream_file_begin[k+1]) being one writer (one serialized fileset: a fresh chunk.Writer per
 * fileset.Writer, fileset/writer.go:36-50) that annotates its files in order and closes.
 * stream_file_begin: nstreams+1 entries from 0 to nfiles (NULL = one stream of all files).
 * Out: chunk_offsets (cap+1 entries; chunk i = scanned bytes [off[i], off[i+1]), so the
 * chunks tile the batch), per chunk hash_known/content_hashes as pfscdc_create_refs takes
 * them (known iff the chunk is one DataRef).  *nchunks = number of chunks; PFSCDC_ENOMEM if
 * it exceeds cap (outputs truncated).  Must follow the scan directly (PFSCDC_ESTATE after
 * a pfscdc_create_refs / pfscdc_get_chunks). */
int pfscdc_form_chunks(pfscdc_ctx* ctx, const uint32_t* stream_file_begin, uint32_t nstreams,
                       uint64_t* chunk_offsets, uint8_t* content_hashes, uint8_t* hash_known,
                       uint64_t cap, uint64_t* nchunks);

/* ---- pachd-level stream formation (fileset/unordered_writer.go, fileset/writer.go,
 * fileset/index/writer.go) --------------------------------------------------------------
 * An unordered writer buffers Put bytes (host memory) until memThreshold bytes are buffered,
 * then serializes the buffer as one fileset: files sorted by (path, tag) go through a fresh
 * chunk writer (pfscdc_writer on data_ctx, Ref ids on), per-file DataRefs are collected by
 * the fileset.Writer callback, and the additive and deletive index entries go through the
 * multilevel index writer (level k: its own pfscdc_writer with WithRollingHashConfig(20, k)).
 * Chunk bytes are not returned (the upload is out of scope); every chunk and every level-0
 * index entry is reported through the event callback, and each fileset's root indexes are
 * kept as encoded index.Index protos. */

#define PFSCDC_EV_CHUNK 1 /* a chunk was formed (data or index stream) */
#define PFSCDC_EV_INDEX 2 /* a level-0 index entry was written (additive or deletive) */

typedef struct pfscdc_uw_event {
  int32_t kind;           /* PFSCDC_EV_* */
  int32_t index;          /* -1: the data stream; 0: additive index; 1: deletive index */
  int32_t level;          /* CHUNK of an index stream: index level */
  uint32_t fileset;       /* serialized fileset number (UnorderedWriter.subFileSet) */
  pfscdc_chunk_ref chunk; /* CHUNK: chunk index, size, edge, Ref */
  const uint8_t* bytes;   /* INDEX: the pbutil frame (int64 LE length + index.Index proto) */
  uint64_t len;
} pfscdc_uw_event;

typedef int (*pfscdc_uw_cb)(void* user, const pfscdc_uw_event* ev); /* non-zero aborts */

typedef struct pfscdc_fileset_info {
  int64_t size_bytes;            /* Primitive.SizeBytes */
  const uint8_t* additive_root;  /* encoded index.Index (NULL: no additive entries) */
  uint64_t additive_root_len;
  const uint8_t* deletive_root;  /* encoded index.Index (NULL: no deletive entries) */
  uint64_t deletive_root_len;
  uint32_t num_files;            /* additive entries */
  uint32_t num_deletes;          /* deletive entries */
} pfscdc_fileset_info;

typedef struct pfscdc_uwriter pfscdc_uwriter;

/* fileset.Storage.NewUnorderedWriter (fileset/storage.go:84-92).  data_ctx must have
 * PFSCDC_OPT_REF_IDS set.  mem_threshold: 0 = DefaultMemoryThreshold (1e9 bytes).
 * index_params: NULL = the reference's index chunking (avgBits 20, seed 0 + level,
 * 1 MB / 20 MB); other values are a test hook. */
int pfscdc_uw_create(pfscdc_ctx* data_ctx, int64_t mem_threshold,
                     const pfscdc_params* index_params, pfscdc_uw_cb cb, void* user,
                     pfscdc_uwriter** out);
/* UnorderedWriter.Put(p, tag, appendFile, r) with r = the n bytes at data (tag NULL/"" =
 * "default"). */
int pfscdc_uw_put(pfscdc_uwriter* w, const char* path, const char* tag, int append_file,
                  const void* data, uint64_t n);
/* UnorderedWriter.Delete(p, tag); a path ending in "/" deletes a directory (buffered files
 * and the live files of the filesets this writer serialized; no parent fileset). */
int pfscdc_uw_delete(pfscdc_uwriter* w, const char* path, const char* tag);
int pfscdc_uw_close(pfscdc_uwriter* w); /* serializes the rest (Close, :171-179) */
/* Serialized filesets are written in groups of up to PFSCDC_UW_INFLIGHT bytes (knob, default
 * 32 GiB) on a background thread while Puts continue; the event callback may run on that
 * thread, never on two threads at once.  Order: groups in order (with several group writers,
 * PFSCDC_UW_WORKERS > 1 or a device group, each group's events are held until the groups
 * before it have emitted theirs); within a group, within one (fileset, index, level) stream
 * and within each fileset's data stream, events come in stream order; a group's data-stream
 * events come fileset by fileset, but its index streams are closed level by level across the
 * group's filesets, so index events of different filesets (and additive and deletive ones)
 * interleave.  Filesets are readable after Close. */
uint32_t pfscdc_uw_num_filesets(const pfscdc_uwriter* w);
/* Fileset i's Primitive (pointers valid until pfscdc_uw_destroy). */
int pfscdc_uw_fileset(const pfscdc_uwriter* w, uint32_t i, pfscdc_fileset_info* out);
int pfscdc_uw_destroy(pfscdc_uwriter* w);
/* Message of the writer's sticky error (Put/Delete/Close or the background fileset write,
 * with the data ctx's last error appended); "" while there is none. */
const char* pfscdc_uw_last_error(const pfscdc_uwriter* w);
/* Where the writer's time went (ms, summed over its Puts and its group writes; a group
 * write runs on a background thread while Puts continue (PFSCDC_UW_WORKERS > 1: several
 * groups in flight, each on a ctx of its own), so the stages overlap the Puts: out[0] the
 * Puts' host copies into the fileset arenas; per grouped close of the data streams out[1] the
 * upload (until the Puts' uploads into the arena mirrors have landed, then the gathers
 * queued; without mirrors the H2D copies queued), out[2] the cuts-only scan (without mirrors
 * it waits for the H2D copies), out[3] the chunk replay, out[4] the one BLAKE2b
 * launch over every piece and multi-piece chunk, out[5] chunk.Create (dek, ChaCha20, Ref.Id),
 * out[6] the data chunks' callbacks; out[7] the index writers; out[8] the group writes'
 * wall time. */
int pfscdc_uw_timings(const pfscdc_uwriter* w, double out[9]);

/* Memory the writers keep for the next writer (no reference counterpart: a GPU-side cache).
 * Each fileset's page-locked host arena (memThreshold bytes) and its device mirror (as many
 * bytes of HBM) go to a process-wide pool when the writer is destroyed, up to
 * PFSCDC_UW_ARENA_POOL_BYTES (env, default 40e9 host bytes + as many device bytes); the
 * contexts a writer made for itself (index levels, extra group writers), with their grow-only
 * device staging, go to a cache of up to PFSCDC_CTX_CACHE (default 32) contexts.  Both count
 * against the device memory other calls see (pfscdc_commit_refs takes its ciphertext copy only
 * with 8 GiB to spare).  pfscdc_uw_trim_cache frees the pooled arenas and destroys the cached
 * contexts of one device (-1: all devices); call it when no writer is being created or
 * destroyed.  pfscdc_uw_cached_arena_bytes: host bytes of the pooled arenas now. */
int pfscdc_uw_trim_cache(int device, uint64_t* arena_bytes_freed, uint32_t* ctxs_destroyed);
uint64_t pfscdc_uw_cached_arena_bytes(void);

/* ---- device groups: one process, several GPUs ------------------------------
 * pachd is one process owning one chunk storage (src/server/pfs/server/driver.go:110-122),
 * so the GPUs of a node are reached through one caller.  A group holds one ctx per member
 * device (a device may appear more than once: several ctxs on one GPU) and deals one call's
 * work across them; results never depend on the dealing or on the number of members.
 *   Files of a batch: each file is its own chunk stream (writer.go:125-128 resets hash and
 *     seglen at Annotate), dealt as contiguous file ranges balanced by bytes (pfscdc_deal).
 *   Unordered writer: serialized filesets (independent chunk streams, fileset/
 *     unordered_writer.go:83-122, fileset/writer.go:36-50) dealt in groups, round robin.
 * The chunk-ref index is gathered over xGMI: each member's segment records and Refs stay on
 * its device and are copied peer to peer (hipMemcpyPeerAsync, direct peer access enabled at
 * create) into one index on the first member's device (the index device), where their file ids
 * are rebased, then copied to the host once.  A group is owned by one thread at a time; its
 * member ctxs belong to it (do not destroy them; do not scan on the group while an unordered
 * writer made from it is open). */

typedef struct pfscdc_group pfscdc_group;

/* Byte-balanced contiguous split of nitems items (item i = [offsets[i], offsets[i+1]),
 * nondecreasing) into nparts parts: part r = items [part_begin[r], part_begin[r+1]), starting
 * at the first item whose prefix reaches ceil(r * total / nparts) bytes (greedy prefix split,
 * items whole and in order; parts may be empty).  part_begin: nparts + 1 entries.  Host only. */
int pfscdc_deal(const uint64_t* offsets, uint32_t nitems, uint32_t nparts, uint32_t* part_begin);

/* One ctx per devices[k] (k < n) with params and options (0 or PFSCDC_OPT_REF_IDS).  The
 * index device is devices[0]. */
int pfscdc_group_create(const pfscdc_params* params, const int* devices, uint32_t n,
                        uint32_t options, pfscdc_group** out);
int pfscdc_group_destroy(pfscdc_group* g);
uint32_t pfscdc_group_size(const pfscdc_group* g);
/* Member i's ctx (owned by the group), e.g. for pfscdc_fill_synthetic on its device. */
pfscdc_ctx* pfscdc_group_ctx(pfscdc_group* g, uint32_t i);
const char* pfscdc_group_last_error(const pfscdc_group* g);

/* pfscdc_scan of a batch of files in host memory over the group: member k scans the files
 * [part_begin[k], part_begin[k+1]) of pfscdc_deal(file_offsets, nfiles, n), copying its own
 * byte range to its device, all members at once.  Blocks until the gathered index is on the
 * host.  Results as pfscdc_scan's, file ids global. */
int pfscdc_group_scan(pfscdc_group* g, const void* bytes, uint64_t nbytes,
                      const uint64_t* file_offsets, uint32_t nfiles);
/* The same over device-resident bytes: member_bytes[k] (device pointer on member k's device,
 * 16-B aligned) holds files [part_begin[k], part_begin[k+1]) contiguously, i.e. bytes
 * [file_offsets[part_begin[k]], file_offsets[part_begin[k+1]]) of the batch.  part_begin:
 * n + 1 entries (NULL = pfscdc_deal's split). */
int pfscdc_group_scan_resident(pfscdc_group* g, const void* const* member_bytes,
                               const uint64_t* file_offsets, uint32_t nfiles,
                               const uint32_t* part_begin);
/* One stream (a single file of nbytes in host memory, e.g. configs[2]'s 10 GiB) split across
 * the members, block-parallel with window-overlap stitching: member k holds an equal byte range
 * (borders on 64-byte boundaries) plus the 64 bytes in front (the window) and up to
 * max_chunk - 1 bytes after (for the segment that straddles its end), finds its range's
 * candidate positions (pfscdc_candidates); the serial min/max selection (writer.go:163-189)
 * then runs once over the gathered candidates on the host, and each segment is hashed by the
 * member holding its first byte.  Results as for one file through the accessors below (file 0;
 * no Refs, no dealing, no device index); equal to pfscdc_scan of the stream on one ctx. */
int pfscdc_group_scan_stream(pfscdc_group* g, const void* bytes, uint64_t nbytes);
/* Results of the last group scan (valid until the next one): the gathered index ordered by
 * (file, offset) with global file ids, per-file ranges (nfiles + 1), Refs (NULL unless the
 * group has PFSCDC_OPT_REF_IDS), and the dealing used (n + 1). */
uint64_t pfscdc_group_num_segments(const pfscdc_group* g);
const pfscdc_segment* pfscdc_group_segments(const pfscdc_group* g);
const uint64_t* pfscdc_group_file_segment_begin(const pfscdc_group* g);
const pfscdc_ref* pfscdc_group_refs(const pfscdc_group* g);
const uint32_t* pfscdc_group_part_begin(const pfscdc_group* g);
/* The gathered index as it lies on the index device (device pointers; nullable outputs). */
int pfscdc_group_index_device(const pfscdc_group* g, const pfscdc_segment** segs,
                              const pfscdc_ref** refs, int* device);
/* Device time of the last group scan: member_ms[k] (n entries) member k's scan-to-hash
 * (pfscdc_last_timings out[4]); gather_ms the peer copies and rebase on the index device;
 * gather_bytes the bytes they moved. */
int pfscdc_group_last_timings(const pfscdc_group* g, float* member_ms, float* gather_ms,
                              uint64_t* gather_bytes);

/* fileset.Storage.NewUnorderedWriter over a device group (the group needs PFSCDC_OPT_REF_IDS):
 * as pfscdc_uw_create, with one group writer per member, each writing on its member's ctx and
 * device (index levels too).  Serialized filesets go out in groups of max(mem_threshold,
 * PFSCDC_UW_INFLIGHT / n) bytes, round robin over the members, and each Put's bytes are
 * uploaded to the device of the member that will write them.  Events reach cb in group order,
 * each group's events as one writer would emit them, so the event stream equals that of
 * pfscdc_uw_create on one ctx with PFSCDC_UW_INFLIGHT set to the same group bytes; roots
 * are identical whatever the grouping. */
int pfscdc_uw_create_group(pfscdc_group* g, int64_t mem_threshold,
                           const pfscdc_params* index_params, pfscdc_uw_cb cb, void* user,
                           pfscdc_uwriter** out);

/* The unordered writer's chunk client: every chunk writer it makes from now on (the data
 * writers and every index level of both indexes, with one or several group writers and over a
 * device group) uploads its chunks' ciphertext into store (pfscdc_writer_set_store(w, store,
 * 1)), so the filesets can be read back (pfscdc_index_read) after Close.  Call it before the
 * first Put (PFSCDC_ESTATE afterwards); events, roots and Ref.Ids do not depend on it.  The
 * store must outlive the writer; NULL turns the upload off again. */
int pfscdc_uw_set_store(pfscdc_uwriter* w, pfscdc_store* store);

/* ---- reading a fileset back (fileset/index/reader.go:41-181, fileset/merge.go:37-77) ------
 * A fileset root (pfscdc_fileset_info.additive_root / deletive_root) is opened against the
 * store the writer uploaded into: the index levels are read breadth-first, each level's chunks
 * verified, decrypted and gathered by the read path into one device buffer, its pbutil frames
 * (int64 LE length + index.Index proto, pbutil.go:39,65) walked and decoded on the device into
 * the flat records below, which pfscdc_store_read_tar takes as they are. */

/* index.WithRange / index.WithPrefix / the tag filter (index/option.go).  Each member may be
 * NULL or "" (unset); a NULL filter selects everything.  atStart(name): name >= lower if lower
 * is set, else name >= prefix.  atEnd(name): name > upper if upper is set, else the first
 * min(len(name), len(prefix)) bytes of name > those of prefix (reader.go:95-122).  tag selects
 * level-0 entries whose File.Tag equals it. */
typedef struct pfscdc_index_filter {
  const char* lower;
  const char* upper;
  const char* prefix;
  const char* tag;
} pfscdc_index_filter;

#define PFSCDC_IDX_HAS_RANGE 1u     /* Index.Range is set (an entry of a level above 0) */
#define PFSCDC_IDX_HAS_FILE 2u      /* Index.File is set */
#define PFSCDC_IDX_HAS_CHUNK_REF 4u /* Range.ChunkRef is set: DataRef first + count of the list */

/* One index.Index.  Strings lie in the list's blob, each followed by a NUL; absent proto3
 * fields are zero / empty. */
typedef struct pfscdc_index_entry {
  uint64_t path_off;      /* Index.Path */
  uint64_t tag_off;       /* File.Tag */
  uint64_t last_path_off; /* Range.LastPath */
  uint32_t path_len;
  uint32_t tag_len;
  uint32_t last_path_len;
  uint32_t flags;         /* PFSCDC_IDX_* */
  uint32_t first;         /* File.DataRefs = DataRefs [first, first + count) of the list */
  uint32_t count;
  int64_t size_bytes;     /* sum of the File's DataRef.SizeBytes */
  int64_t range_offset;   /* Range.Offset */
} pfscdc_index_entry;     /* 64 bytes */

/* An owned list of entries in stream order: the entries, one packed blob of their strings and
 * one pfscdc_full_dataref array.  pfscdc_index_list_tar_files gives one pfscdc_tar_file per
 * entry (path into the blob, first, count), so that
 *   pfscdc_store_read_tar(ctx, store, tar_files, count, datarefs, ndatarefs, ...)
 * renders the list as a tar stream with no conversion.  Pointers stay valid until
 * pfscdc_index_list_free. */
typedef struct pfscdc_index_list pfscdc_index_list;
uint32_t pfscdc_index_list_count(const pfscdc_index_list* l);
const pfscdc_index_entry* pfscdc_index_list_entries(const pfscdc_index_list* l);
const char* pfscdc_index_list_blob(const pfscdc_index_list* l, uint64_t* len);
const pfscdc_full_dataref* pfscdc_index_list_datarefs(const pfscdc_index_list* l, uint32_t* n);
const pfscdc_tar_file* pfscdc_index_list_tar_files(pfscdc_index_list* l);
int pfscdc_index_list_free(pfscdc_index_list* l);

/* The decode of one level's stream (n bytes of pbutil frames) on the host, with no GPU call:
 * the specification the decode kernels are tested against, and the decode pfscdc_index_read
 * uses when the PFSCDC_INDEX_DECODE knob is 0.  Every entry of the stream, unfiltered.
 * PFSCDC_ECORRUPT for a stream that does not parse (a frame length that is negative or runs
 * past the stream, a varint longer than 10 bytes, a nested length past its parent, a wire type
 * that does not fit the field, an id, dek or hash that is not 32 bytes), with *err_offset
 * (nullable) the offset of the first frame that does not; *out is then NULL.  Unknown fields of
 * a known wire type are skipped.  Never reads outside [stream, stream + n). */
int pfscdc_index_decode_host(const void* stream, uint64_t n, pfscdc_index_list** out,
                             uint64_t* err_offset);
/* Reader.Iterate's selection over a list of level-0 entries in path order: entries are taken
 * from the first with atStart(path) up to the first with atEnd(path), those with another tag
 * than filter->tag left out.  Host only. */
int pfscdc_index_filter_list(const pfscdc_index_list* in, const pfscdc_index_filter* filter,
                             pfscdc_index_list** out);
/* index.NewReader(chunks, topIdx, opts...).Iterate (reader.go:41-83): the level-0 entries under
 * root (an encoded index.Index) that the filter selects, in order.  A NULL or empty root gives
 * an empty list; a root without a Range is itself a level-0 entry.  Levels are read breadth-
 * first: of one level's entries, those with atStart(Range.LastPath) that precede the first with
 * atEnd(Path) name the chunks of the level below, which are read whole (chunk.Reference: offset
 * 0, Ref.SizeBytes) in one read-path call; the level's stream is the first chunk from its
 * Range.Offset on followed by the later chunks whole (levelReader.setup / next).  The chunk of
 * the entry the selection ends at (the first with atEnd(Path)) is read as well, as
 * levelReader.next fetches it for the frame that runs on into it; no other chunk is read.
 * Errors: PFSCDC_ENOTFOUND (a chunk id is not in the store), PFSCDC_ECORRUPT (a chunk fails
 * verification, or a stream does not parse: pfscdc_last_error then names the level, counted
 * from 0 for the stream the root names, and the offset in that level's stream of the first
 * frame that does not parse); *out is then NULL and nothing was written past any array.
 * The PFSCDC_INDEX_DECODE knob: 1 decodes on the device, 0 copies each level's bytes to the
 * host and decodes them with pfscdc_index_decode_host; the lists are identical. */
int pfscdc_index_read(pfscdc_ctx* ctx, const pfscdc_store* store, const void* root,
                      uint64_t root_len, const pfscdc_index_filter* filter,
                      pfscdc_index_list** out);
/* Counts of the last pfscdc_index_read on ctx: out[0] index chunks read, out[1] chunks whose
 * speculative frame walk was discarded and walked again from the chunk before's exit, out[2]
 * levels read, out[3] frames decoded (all levels). */
int pfscdc_last_index_stats(pfscdc_ctx* ctx, uint64_t out[4]);
/* Its time (ms): out[0] the read path's verification and out[1] its decrypt-and-gather of the
 * index chunks (device time, summed over the levels), out[2] the frame walk with its
 * re-walks, out[3] the decode (device: count, prefix sums, fill; host arm: the host decode),
 * out[4] the copy of the list (host arm: of the level's bytes) to the host; [2..4] wall time
 * around synchronised stages. */
int pfscdc_last_index_timings(pfscdc_ctx* ctx, float out[5]);

/* MergeReader.iterate (merge.go:37-77) over stream.PriorityQueue (priority_queue.go:103-127):
 * lists holds, for each of nfilesets filesets in order, its deletive list and then its additive
 * list (2 * nfilesets pointers; NULL = an empty list), each in (path, tag) order.  Entries
 * with equal (path, tag) form a group, groups come in path-then-tag order, and within a group
 * the order is fileset 0 deletive, fileset 0 additive, fileset 1 deletive, ...  A group of one
 * entry: deletive gives nothing, additive passes through.  A longer group: a deletive entry in
 * last place drops the file, an earlier one clears the DataRefs collected so far, an additive
 * one appends its DataRefs; the merged entry keeps the group's first entry's path and tag.
 * Different tags of one path stay separate entries.  Host only. */
int pfscdc_index_merge(const pfscdc_index_list* const* lists, uint32_t nfilesets,
                       pfscdc_index_list** out);
/* MergeReader.iterateDeletive (merge.go:79-94): lists holds the deletive list of each of
 * nfilesets filesets (nfilesets pointers; NULL = an empty list).  Entries with equal (path, tag)
 * form a group, and each group yields its first entry (the lowest fileset's) as it is.  Host
 * only: the specification of PFSCDC_MERGE_DELETIVE. */
int pfscdc_index_merge_deletive(const pfscdc_index_list* const* lists, uint32_t nfilesets,
                                pfscdc_index_list** out);
#define PFSCDC_MERGE_FILES 0    /* MergeReader.iterate: lists as pfscdc_index_merge takes them */
#define PFSCDC_MERGE_DELETIVE 1 /* MergeReader.iterateDeletive: nfilesets deletive lists */
/* Either merge on ctx.  The PFSCDC_INDEX_MERGE knob: 1 merges on the device (the streams are
 * uploaded, every entry is ranked by binary searches in the other streams, the groups are formed
 * and counted, and the merged entries, strings and DataRefs are written at prefix-summed
 * ranges), 0 calls the host function of the mode; the lists are identical, array for array.
 * The device arm hands a call to the host arm in two cases only: a list that is not strictly
 * ascending in (path, tag), and more than 2^32 - 1 entries or DataRef records in the input. */
int pfscdc_index_merge_ctx(pfscdc_ctx* ctx, int mode, const pfscdc_index_list* const* lists,
                           uint32_t nfilesets, pfscdc_index_list** out);
/* The last pfscdc_index_merge_ctx on ctx: out[0] 1 the device arm ran, 0 the host arm; out[1]
 * entries in; out[2] groups (device arm; 0 from the host arm); out[3] entries out. */
int pfscdc_last_merge_stats(pfscdc_ctx* ctx, uint64_t out[4]);
/* Its time (ms, wall time around synchronised stages): out[0] the upload of the lists, out[1]
 * rank, grouping and prefix sums (host arm: the whole host merge), out[2] the emit (entries,
 * strings, DataRef copy), out[3] the copy of the list to the host. */
int pfscdc_last_merge_timings(pfscdc_ctx* ctx, float out[4]);

/* ---- index lists that stay on the device (no reference counterpart: a GPU-side hand-over) ----
 * pfscdc_index_read copies each decoded list to the host, pfscdc_index_merge_ctx uploads the lists
 * again and copies the result back, and pfscdc_store_read_tar reads every DataRef on the host to
 * plan its window.  A pfscdc_dev_list owns the same three arrays (pfscdc_index_entry, the string
 * blob, pfscdc_full_dataref) in the formats the decode and merge kernels write, on the ctx's
 * device; only the counts are on the host.  Read, merge and tar over such lists move nothing per
 * file or per DataRef across the host link.  A handle is bound to the device of the ctx that made
 * it (PFSCDC_EINVAL with a ctx of another device) and is owned by one thread at a time. */
typedef struct pfscdc_dev_list pfscdc_dev_list;
/* A resident copy of a host list, and back: the downloaded list equals the uploaded one array for
 * array. */
int pfscdc_dev_list_upload(pfscdc_ctx* ctx, const pfscdc_index_list* l, pfscdc_dev_list** out);
int pfscdc_dev_list_download(pfscdc_ctx* ctx, const pfscdc_dev_list* d, pfscdc_index_list** out);
uint32_t pfscdc_dev_list_count(const pfscdc_dev_list* d);
uint32_t pfscdc_dev_list_num_datarefs(const pfscdc_dev_list* d);
uint64_t pfscdc_dev_list_blob_len(const pfscdc_dev_list* d);
int pfscdc_dev_list_free(pfscdc_dev_list* d);
/* pfscdc_index_read with a resident result.  With no filter (NULL, or every member unset) and the
 * PFSCDC_INDEX_DECODE knob at 1, the levels above 0 are read as pfscdc_index_read reads them
 * (small lists the host selection needs) and the level of File entries stays where the decode
 * kernels wrote it: nothing of it is copied out, and pfscdc_last_index_timings' out[4] covers the
 * upper levels only.  With a filter that names a part, with the knob at 0, for an empty root and
 * for a root that is itself a level-0 entry the call is pfscdc_index_read followed by
 * pfscdc_dev_list_upload (a level-0 selection on the device is not built);
 * pfscdc_last_resident_stats tells which.  Errors as pfscdc_index_read's. */
int pfscdc_index_read_dev(pfscdc_ctx* ctx, const pfscdc_store* store, const void* root,
                          uint64_t root_len, const pfscdc_index_filter* filter,
                          pfscdc_dev_list** out);
/* Both modes of pfscdc_index_merge_ctx over resident lists (lists as that call takes them; NULL =
 * an empty list) with a resident result: the streams are gathered by device-to-device copies, the
 * merge kernels run as they do for pfscdc_index_merge_ctx, and their output arrays become the new
 * list.  The PFSCDC_INDEX_MERGE knob does not govern this call: resident inputs mean the device
 * arm.  A stream that is not strictly ascending, or more than 2^32 - 1 entries or DataRef records
 * in, is downloaded, merged by the host function of the mode and uploaded;
 * pfscdc_last_merge_stats' out[0] is then 0.  pfscdc_last_merge_timings: out[0] the gather (host
 * arm: the upload of the result), out[3] the guards' copy alone (host arm: the download of the
 * inputs). */
int pfscdc_index_merge_dev(pfscdc_ctx* ctx, int mode, const pfscdc_dev_list* const* lists,
                           uint32_t nfilesets, pfscdc_dev_list** out);
/* pfscdc_tar_layout for a resident list: *total the stream's length, entry_offsets (nullable,
 * count + 1 entries) as pfscdc_tar_layout's.  Runs the plan stage of pfscdc_dev_list_read_tar if
 * the handle has none yet (kernels: every DataRef's size and validity, prefix sums, per entry the
 * name rules above and the span, prefix sums of the spans) and caches it in the handle, for the
 * ctx's tar format (pfscdc_set_tar_format: a handle planned under the other format is planned
 * again); errors as pfscdc_dev_list_read_tar's name and size errors. */
int pfscdc_dev_list_tar_layout(pfscdc_ctx* ctx, pfscdc_dev_list* d, uint64_t* total,
                               uint64_t* entry_offsets);
/* pfscdc_store_read_tar over a resident list: the same window rules, the same bytes, the same
 * error codes (PFSCDC_ENOTFOUND and PFSCDC_ECORRUPT before anything is written to out;
 * PFSCDC_EUNSUPPORTED / PFSCDC_EINVAL with the lowest refused file named in pfscdc_last_error,
 * PFSCDC_EINVAL for a DataRef that reaches past its chunk).  Per call, on the device: the entries
 * that meet the window are found by searches in the cached offsets; every DataRef of theirs is
 * clipped to the window, one lane each, and the non-empty pieces are counted, prefix-summed and
 * written as the dense slice arrays the gather kernel takes; a piece whose DataRef before it gave
 * none, or names another chunk or another Ref.SizeBytes of the same chunk, heads a run, and only the
 * runs' {id, dek, size} records (80 bytes each) come to the host, which looks their chunks up in
 * the store, holds each stored length against the run's size, deduplicates them by id and sends
 * back one chunk number per run; the kernel that applies it checks every slice against its
 * chunk's stored length once more, since the gather checks nothing (PFSCDC_ECORRUPT).  A path is
 * read up to its first NUL, as the host call reads it.  The tar entries are the plan's own records with the
 * list's blob as the name table.  Refused with PFSCDC_EUNSUPPORTED: a list whose entries do not
 * hold their DataRefs at [first, first + count) packed in entry order (every list this library
 * makes does), and a blob of 4 GiB or more.  Every array the planning kernels fill ends in a
 * 64-byte guard that the call checks (PFSCDC_EHIP). */
int pfscdc_dev_list_read_tar(pfscdc_ctx* ctx, const pfscdc_store* store, pfscdc_dev_list* d,
                             uint64_t begin, uint64_t len, void* out, uint64_t out_cap,
                             int out_on_device, uint64_t* nwritten);
/* Counts of the last resident calls on ctx: out[0] 1 the last pfscdc_index_read_dev kept the
 * decode's device arrays, 0 it uploaded the host path's list, out[1] the bytes it uploaded;
 * of the last pfscdc_dev_list_read_tar: out[2] runs, out[3] distinct chunks, out[4] non-empty
 * pieces, out[5] bytes copied device to host (the window into a host out not counted), out[6]
 * bytes copied host to device except chunk ciphertext, out[7] 1 the cached plan was reused. */
int pfscdc_last_resident_stats(pfscdc_ctx* ctx, uint64_t out[8]);

/* ---- the Source: directory entries, path filters and FileInfo (src/server/pfs/server/
 * source.go:28-157, driver_file.go:173-385; fileset/dir_inserter.go:22-58, transforms.go:31-49) ----
 * Every PFS file RPC wraps the opened commit in a Source.  The input is a level-0 list in
 * (path, tag) order (what pfscdc_index_read[_dev] or pfscdc_index_merge[_dev] returns; the open
 * has applied index.WithPrefix and WithTag).  The result:
 *   1. dirInserter: a directory entry Index{Path: dir, File: {}} (empty tag, no DataRefs, size 0)
 *      in front of the first entry under every directory, "/" included;
 *   2. indexFilter: the entries a path predicate selects (below), directories included;
 *   3. source.Iterate: per selected entry a pfscdc_file_info.  A file: its size_bytes and
 *      hashDataRefs (fileset/util.go:149-158: BLAKE2b-256 over its DataRefs' hashes; the hash of
 *      the empty string for none), or the caller's leaf hash.  A directory: the wrapping sum of
 *      its descendants' file sizes and BLAKE2b-256 over its immediate children's hashes in stream
 *      order (sub-directories and each tag of one path count as a child).
 * The result's list holds the selected entries with a fresh blob and the compacted DataRefs of the
 * selected entries, first packed in entry order, so the tar calls take it as it is and write one
 * entry per entry of the stream, directories (typeflag 5) included: GetFileTAR as served.
 * Predicates (arg goes through cleanPath here; "" and "/" name the root):
 *   PFSCDC_SRC_ALL      everything (arg ignored);
 *   PFSCDC_SRC_SUBTREE  inspectFile / walkFile: path == p || HasPrefix(path, p + "/"),
 *                       p = cleanPath(arg), "" for the root;
 *   PFSCDC_SRC_LIST     listFile: not Clean(name, true) itself, else path == name or
 *                       HasPrefix(path, Clean(name, true)); PFSCDC_INFO_CHILD is set in the flags
 *                       of the entries with pathIsChild(name, cleanPath(path));
 *   PFSCDC_SRC_GET      getFile's `full` filter for a literal glob: path == glob, path == glob + "/"
 *                       or HasPrefix(path, glob + "/"); "/" selects everything.  A glob holding one
 *                       of *?[]{}!()@+^ or a backslash: PFSCDC_EUNSUPPORTED with the glob named;
 *   PFSCDC_SRC_DIFF     diffFile: SUBTREE's predicate and cleaning, but neither side of a diff is
 *                       wrapped in NewErrOnEmpty (driver_file.go:356-383): nothing selected is
 *                       PFSCDC_OK with no entries;
 *   PFSCDC_SRC_GLOB     getFile / globFile of a glob pattern (the dialect: pfscdc_glob_match below):
 *                       mf(path) = (path == "/" && glob == "/") || Match(glob, TrimRight(path, "/"))
 *                       under the `full` filter, so an entry is selected if mf holds for it or it
 *                       lies under the last directory that matched.  PFSCDC_INFO_MATCH is set in the
 *                       flags of the entries for which mf holds itself: the whole result is what
 *                       getFile serves, the entries with the flag are what globFile reports (a
 *                       matched directory's size and hash cover its whole subtree).  A glob that
 *                       does not compile: PFSCDC_EINVAL with the glob and the byte offset named;
 *                       extglob: PFSCDC_EUNSUPPORTED with the glob named.
 * PFSCDC_ENOTFOUND (NewErrOnEmpty): nothing selected by GET or GLOB, or by SUBTREE with p != ""
 * (globFile does not wrap its stream: its caller takes this answer of GLOB as an empty result).
 * PFSCDC_EINVAL: an entry with a Range (not a level-0 list), or strings / DataRefs outside the
 * list's arrays. */
#define PFSCDC_SRC_ALL 0
#define PFSCDC_SRC_SUBTREE 1
#define PFSCDC_SRC_LIST 2
#define PFSCDC_SRC_GET 3
#define PFSCDC_SRC_DIFF 4
#define PFSCDC_SRC_GLOB 5
#define PFSCDC_FILE_TYPE_FILE 1u /* pfs.FileType_FILE */
#define PFSCDC_FILE_TYPE_DIR 2u  /* pfs.FileType_DIR: the path ends in '/' */
#define PFSCDC_INFO_CHILD 1u
#define PFSCDC_INFO_MATCH 2u
typedef struct pfscdc_file_info {
  uint8_t hash[32];
  int64_t size;
  uint32_t type;  /* PFSCDC_FILE_TYPE_* */
  uint32_t flags; /* PFSCDC_INFO_* */
} pfscdc_file_info; /* 48 bytes */

/* The Source on the host, with no GPU call: emit() of dirInserter.Iterate, indexFilter.Iterate
 * with its dir state and source.Iterate's recursion over a second iterator with its cache, taken
 * literally.  The specification of pfscdc_source_open, and its arm for the lists the device
 * refuses.  leaf_hashes (nullable): 32 bytes per entry of in, used as the files' hashes (the
 * reference's MergeFileReader.Hash when more than one fileset was opened, storage.go:124-127).
 * *out: pfscdc_index_list_free; *infos (one per entry of *out): pfscdc_file_infos_free.  On an
 * error both are NULL and pfscdc_source_host_error names it (per thread, until the next call). */
int pfscdc_source_host(const pfscdc_index_list* in, int kind, const char* arg,
                       const uint8_t* leaf_hashes, pfscdc_index_list** out,
                       pfscdc_file_info** infos);
const char* pfscdc_source_host_error(void);
void pfscdc_file_infos_free(pfscdc_file_info* infos);

/* The glob dialect of PFSCDC_SRC_GLOB (gobwas/glob syntax with separator '/'; the glob library of
 * the reference is not in its tree, so DESIGN.md writes the dialect down): * any run of non-'/'
 * bytes, ** any run of bytes, ? one non-'/' byte, [...] and [!...] a class of bytes and lo-hi
 * ranges (it may hold '/'), {a,b} alternatives that nest, \c the byte c; bytewise, the whole
 * string.  *matched = mf(path) for glob = cleanPath(glob): the backtracking matcher that is the
 * specification of what the device computes, with no GPU call.  PFSCDC_EINVAL (a stray ] or }, an
 * unterminated [ or {, an empty class, a range with hi < lo, a trailing backslash) and
 * PFSCDC_EUNSUPPORTED (extglob: an unescaped ! ( ) @ + ^ outside a class) with
 * pfscdc_source_host_error naming the glob and the byte offset. */
int pfscdc_glob_match(const char* glob, const char* path, int* matched);
/* globLiteralPrefix(cleanPath(glob)): the glob up to its first of * ? [ ] { } ! ( ) @ + ^, as a
 * C string in out[0, cap) (PFSCDC_EINVAL if it does not fit). */
int pfscdc_glob_literal_prefix(const char* glob, char* out, size_t cap);
/* Test hook: the position automaton compiled from cleanPath(glob), what the device stages.
 * out[0, 64) follow, out[64, 320) accept_byte (masks of positions), out[320] first, out[321] last,
 * out[322] nullable, out[323] the positions (more than 64: no program, the masks are zero).  A
 * string is accepted iff, with T = first and acc = nullable before its first byte and per byte c
 * S = T & accept_byte[c], acc = (S & last) != 0, T = OR of follow[b] over the bits b of S, acc
 * holds after its last byte. */
int pfscdc_debug_glob_program(const char* glob, uint64_t out[324]);

/* The Source over a resident list on ctx.  The PFSCDC_SOURCE knob: 1 runs the device arm
 * (per input entry the new ancestors by the common prefix with its predecessor and the predicate on
 * each, prefix sums, a fill at the item's own ranges and the DataRef copy; per output entry its depth
 * and its subtree's end by a search, directory sizes as differences of one prefix sum; the leaf
 * hashes in one BLAKE2b launch and then one launch per depth, deepest first, over the children's
 * hashes gathered 32 bytes apart), 0 downloads the list, calls pfscdc_source_host and uploads its
 * result; list and infos are identical.  The device arm hands a call to the host arm for a list
 * that is not in (path, tag) order, that holds a path not IsClean(p, IsDir(p)), or that holds one
 * directory path twice; pfscdc_last_source_stats says which ran.  PFSCDC_SRC_GLOB on the device:
 * one kernel ahead of the count pass walks each path once through the glob's position automaton
 * (pfscdc_debug_glob_program) and leaves one 64-bit mask per entry, which the count and fill
 * passes read in place of a predicate; a glob of more than 64 positions or a path of more than
 * 63 '/' hands the call to the host arm.  leaf_hashes as
 * pfscdc_source_host's, on the device when leaf_on_device.  Errors and their texts
 * (pfscdc_last_error) as pfscdc_source_host's, with *out NULL.  Every array the kernels fill ends
 * in a 64-byte guard that the call checks (PFSCDC_EHIP). */
typedef struct pfscdc_source pfscdc_source;
int pfscdc_source_open(pfscdc_ctx* ctx, const pfscdc_dev_list* in, int kind, const char* arg,
                       const uint8_t* leaf_hashes, int leaf_on_device, pfscdc_source** out);
/* The same over a host list, which is uploaded first (NULL: an empty list). */
int pfscdc_source_open_list(pfscdc_ctx* ctx, const pfscdc_index_list* in, int kind,
                            const char* arg, const uint8_t* leaf_hashes, int leaf_on_device,
                            pfscdc_source** out);
/* The result's list, owned by the source: pfscdc_dev_list_read_tar, _tar_layout and _download
 * take it as it is. */
pfscdc_dev_list* pfscdc_source_list(pfscdc_source* s);
uint32_t pfscdc_source_count(const pfscdc_source* s);
/* The infos copied to out (pfscdc_source_count records). */
int pfscdc_source_infos(pfscdc_ctx* ctx, const pfscdc_source* s, pfscdc_file_info* out);
int pfscdc_source_free(pfscdc_source* s);
/* The last pfscdc_source_open on ctx: out[0] 1 the device arm ran, 0 the host arm; out[1] entries
 * in; out[2] entries out; out[3] directories inserted and selected; out[4] levels (the deepest
 * entry's depth); out[5] BLAKE2b launches; out[6] bytes copied host to device; out[7] bytes copied
 * device to host (pfscdc_source_infos not counted). */
int pfscdc_last_source_stats(pfscdc_ctx* ctx, uint64_t out[8]);
/* Its time (ms, wall time around synchronised stages): out[0] insert and select (count, prefix
 * sums, fill, DataRef copy; host arm: the download, the host call and the upload), out[1] depths,
 * subtree ends and sizes, out[2] the leaf hashes, out[3] the directory levels. */
int pfscdc_last_source_timings(pfscdc_ctx* ctx, float out[4]);
/* Test hook: the glob kernel alone over a resident list, so that it is held against
 * pfscdc_glob_match directly.  masks[i] of entry i's path: bit j = the bytes before its j-th '/'
 * (j from 0: the root, the empty string) are matched by cleanPath(glob), a directory's own final
 * '/' included; bit 63 = a path that does not end in '/' is matched as a whole.  *bad: 32 if a
 * path holds more than 63 '/' (its mask is then not used), else 0.  PFSCDC_EUNSUPPORTED for a
 * glob of more than 64 positions; compile errors as pfscdc_glob_match's (pfscdc_last_error). */
int pfscdc_debug_glob_masks(pfscdc_ctx* ctx, const pfscdc_dev_list* list, const char* glob,
                            uint64_t* masks, uint32_t* bad);
/* Test hook: a prefix-sum kernel of the list passes alone.  in: n < 2^32 host records of kind 0
 * {uint32 records, uint32 blob bytes} (2 columns), 1 {uint32 entries, uint32 DataRefs, uint64
 * blob bytes} (3 columns) or 2 one uint64 <= 2^62 + 1 (1 column, the add saturating at
 * 2^62 + 1).  out: N (n + 1) words, out[N i + c] = column c summed over the records before i,
 * out[N n + c] the totals. */
int pfscdc_debug_list_scan(pfscdc_ctx* ctx, int kind, const void* in, uint64_t n, uint64_t* out);

/* ---- DiffFile: two Sources joined by path (src/server/pfs/server/diff.go:22-96) -----------------
 * Differ.Iterate walks sides a (the old commit; emptySource when there is none) and b (the new
 * one) with two pointers: the side with the lesser path (Go's string order: unsigned bytes, a
 * proper prefix first; the tag is no part of the key) is reported alone and advances; equal paths
 * advance both sides and are reported as a pair only if the 32 hash bytes differ (equalFileInfos);
 * then both tails are drained.  One pfscdc_diff_pair per callback, in callback order: a and b are
 * indexes into their sides, PFSCDC_DIFF_NONE for the side the callback got nil for. */
#define PFSCDC_DIFF_NONE 0xffffffffu
typedef struct pfscdc_diff_pair {
  uint32_t a, b;
} pfscdc_diff_pair;

/* The walk on the host, with no GPU call, taken literally: it does not assume sorted sides and
 * does whatever the two pointers do.  Each side is a list with one pfscdc_file_info per entry
 * (what pfscdc_source_host returns); a NULL or empty list is an empty side.  *out (*n pairs):
 * pfscdc_diff_pairs_free.  PFSCDC_EINVAL: entries without infos, or a path outside the list's
 * blob; *out is then NULL.  The specification of pfscdc_source_diff. */
int pfscdc_diff_host(const pfscdc_index_list* a, const pfscdc_file_info* a_infos,
                     const pfscdc_index_list* b, const pfscdc_file_info* b_infos,
                     pfscdc_diff_pair** out, uint64_t* n);
void pfscdc_diff_pairs_free(pfscdc_diff_pair* pairs);

/* The walk over two Sources of ctx's device (a NULL a: emptySource).  The PFSCDC_DIFF knob: 1 runs
 * the device arm.  Within a side the paths do not decrease, so the walk pairs the k-th entry of a
 * path on side a with the k-th on side b and the longer run's surplus follows unpaired: one lane
 * per entry finds its number in its run and the run of its path in the other side by searches,
 * compares the hashes, and the places of the pairs follow from prefix sums of both sides' flags.
 * 0, or a side whose paths decrease, downloads both lists and infos, calls pfscdc_diff_host and
 * uploads the result; the two arms' arrays are identical.  Beside the pairs the diff holds, per
 * side, the entries of that side that occur in a pair as a pfscdc_source of its own (entries in
 * order, a fresh blob, the DataRefs packed in entry order, the infos gathered): the i-th pair
 * with an a member is entry i of side 0's selection, and likewise b and side 1, so the paths of
 * what changed come from the diff alone and the tar calls render only the changed files.
 * PFSCDC_EINVAL: a NULL b, a Source of another device.  Every array the kernels fill ends in a
 * 64-byte guard that the call checks (PFSCDC_EHIP). */
typedef struct pfscdc_diff pfscdc_diff;
int pfscdc_source_diff(pfscdc_ctx* ctx, const pfscdc_source* a, const pfscdc_source* b,
                       pfscdc_diff** out);
uint64_t pfscdc_diff_count(const pfscdc_diff* d);
/* The pairs copied to out (pfscdc_diff_count records). */
int pfscdc_diff_pairs(pfscdc_ctx* ctx, const pfscdc_diff* d, pfscdc_diff_pair* out);
/* Side 0 (a) or 1 (b)'s selection, owned by the diff: pfscdc_source_list, _count and _infos take
 * it; NULL for another side. */
pfscdc_source* pfscdc_diff_side(pfscdc_diff* d, int side);
int pfscdc_diff_free(pfscdc_diff* d);
/* The last pfscdc_source_diff on ctx: out[0] 1 the device arm ran, 0 the host arm; out[1], out[2]
 * entries of a and of b; out[3] pairs; out[4] pairs with both members; out[5] bytes copied host
 * to device; out[6] bytes copied device to host (the accessors not counted); out[7] 0. */
int pfscdc_last_diff_stats(pfscdc_ctx* ctx, uint64_t out[8]);
/* Its time (ms, wall time around synchronised stages): out[0] rank and prefix sums (host arm: the
 * download of both sides), out[1] the pairs' fill (host arm: pfscdc_diff_host), out[2] the two
 * selections (host arm: built on the host), out[3] the guards' copy (host arm: the upload). */
int pfscdc_last_diff_timings(pfscdc_ctx* ctx, float out[4]);

/* ---- CopyFile: a file or subtree selected and moved under a new root (src/server/pfs/server/
 * driver_file.go:143-171 copyFile; fileset/transforms.go:20-90 NewIndexFilter, NewIndexMapper) ----
 * in is a level-0 list (what pfscdc_index_read[_dev] or pfscdc_index_merge[_dev] returns).  With
 * srcPath = cleanPath(src) and dstPath = cleanPath(dst) (paths.go:54-60):
 *   1. the open's options index.WithPrefix(srcPath) and index.WithTag(src_tag), as
 *      pfscdc_index_filter_list applies a prefix and a tag (a NULL or "" src_tag: every tag);
 *   2. NewIndexFilter: path == srcPath || HasPrefix(path, srcPath + "/").  srcPath "/" therefore
 *      selects nothing from a list of clean paths: PFSCDC_OK and an empty list, as in the reference;
 *   3. NewIndexMapper: the new path is path.Join(dstPath, filepath.Rel(srcPath, path)), with Go's
 *      Clean, Rel and Join in full: srcPath itself becomes dstPath, srcPath + "/r" becomes
 *      dstPath + "/r" ("/r" under the root), and a path that is not clean becomes what Go makes of it.
 * The tag, the flags, size_bytes and the DataRefs stay.  The result owns a fresh blob (the new
 * path, the tag and an empty LastPath per entry) and the selected entries' DataRefs packed at
 * [first, first + count) in entry order: the tar calls and pfscdc_dev_list_upload take it as it
 * is.  PFSCDC_EINVAL, with *out NULL: an entry with a Range, strings or DataRefs outside the
 * list's arrays, a new path longer than 2^32 - 1 bytes.  The specification of
 * pfscdc_dev_list_copy_map, with no GPU call. */
int pfscdc_copy_map_host(const pfscdc_index_list* in, const char* src, const char* src_tag,
                         const char* dst, pfscdc_index_list** out);
/* The same over a resident list on ctx; *out: pfscdc_dev_list_free.  The PFSCDC_COPY_MAP knob: 1
 * runs the device arm (one lane per entry checks its bounds and its order against its
 * predecessor, evaluates the tag test and the predicate and counts what it emits; prefix sums; a
 * fill that writes dstPath and the path's tail at the entry's own ranges; the DataRef copy), 0
 * downloads the list, calls pfscdc_copy_map_host and uploads its result; the arrays are identical.
 * The device arm hands a call to the host arm for a list that is not in (path, tag) order, holds
 * an entry with a Range, or selects a path that is not clean as a file path (IsClean(p, false));
 * pfscdc_last_copy_map_stats says which ran.  Errors as pfscdc_copy_map_host's (texts:
 * pfscdc_last_error).  Every array the kernels fill ends in a 64-byte guard that the call checks
 * (PFSCDC_EHIP). */
int pfscdc_dev_list_copy_map(pfscdc_ctx* ctx, const pfscdc_dev_list* in, const char* src,
                             const char* src_tag, const char* dst, pfscdc_dev_list** out);
/* The same over a host list, which is uploaded first (NULL: an empty list). */
int pfscdc_copy_map_list(pfscdc_ctx* ctx, const pfscdc_index_list* in, const char* src,
                         const char* src_tag, const char* dst, pfscdc_dev_list** out);
/* The last of the two calls above on ctx: out[0] 1 the device arm ran, 0 the host arm; out[1]
 * entries in; out[2] entries out; out[3] DataRefs out; out[4] blob bytes out; out[5] bytes copied
 * host to device; out[6] bytes copied device to host; out[7] 0. */
int pfscdc_last_copy_map_stats(pfscdc_ctx* ctx, uint64_t out[8]);
/* Its time (ms, wall time around synchronised stages): out[0] count and prefix sums, out[1] the
 * fill, out[2] the DataRef copy, out[3] the guards' copy (host arm: the download, the host call,
 * the upload, 0). */
int pfscdc_last_copy_map_timings(pfscdc_ctx* ctx, float out[4]);

/* UnorderedWriter.Copy (fileset/unordered_writer.go:151-168): the buffer is serialized, then one
 * more fileset is written (withWriter): for every entry of files in order Delete(path, tag)
 * unless append_file, then Copy(entry, tag) as pfscdc_fsw_copy, in prefetch runs as
 * pfscdc_fsw_copy_lists forms them.  tag (NULL or "": "default") replaces the entries' tags.
 * The fileset takes the next number after everything serialized so far, and its events follow
 * all earlier filesets' events: what is pending is written and every group writer is joined
 * first, with any PFSCDC_UW_WORKERS.  An empty (or NULL) list still yields a fileset, with no
 * roots.  A later directory Delete sees the copied files.  Sticky errors, named by
 * pfscdc_uw_last_error: PFSCDC_ESTATE without a store (pfscdc_uw_set_store) or after Close;
 * PFSCDC_EINVAL (checkPath, the path named) for two entries that come to one (path, tag), as two
 * source tags of one path do, and for a list that is not in path order; PFSCDC_ENOTFOUND /
 * PFSCDC_ECORRUPT from the reads of the chunks that are re-rolled. */
int pfscdc_uw_copy(pfscdc_uwriter* w, const pfscdc_index_list* files, const char* tag,
                   int append_file);
/* driver.copyFile (driver_file.go:143-171) in one call: Storage.Open(filesets,
 * WithPrefix(cleanPath(src)), WithTag(src_tag)) as pfscdc_fsw_copy_filesets opens them (both roots
 * of every fileset read with the filter, then merged as PFSCDC_MERGE_FILES; one fileset is read
 * with no merge) on a cached context that is not the data ctx, the selection and path transform
 * (PFSCDC_COPY_MAP at 1: pfscdc_copy_map_list and a download; at 0: pfscdc_copy_map_host on the
 * opened list), and pfscdc_uw_copy.  n == 0 copies an empty list. */
int pfscdc_uw_copy_file(pfscdc_uwriter* w, const pfscdc_fileset_info* filesets, uint32_t n,
                        const char* src, const char* src_tag, const char* dst, const char* tag,
                        int append_file);

/* shard (fileset/shard.go:27-49) over a merged list: cb receives each shard's path range
 * (lower, upper; "" = an open end).  A range is closed in front of the first file that finds
 * threshold or more content bytes collected (the test comes before the file is added); its upper
 * is the last file's path and the next lower is that next file's path; the last upper is "".  An
 * empty (or NULL) list gives one open range.  A path whose tags lie on both sides of a border is
 * in both ranges, as in the reference.  A non-zero return of cb ends the walk with
 * PFSCDC_ECALLBACK.  Host only. */
typedef int (*pfscdc_shard_cb)(void* user, const char* lower, const char* upper);
int pfscdc_shard(const pfscdc_index_list* files, int64_t threshold, pfscdc_shard_cb cb, void* user);

/* ---- fileset.Writer with Delete and Copy (fileset/writer.go:77-125,151-182), for Compact and
 * Concat (fileset/compaction.go:43-57, storage.go:226-238) --------------------------------------
 * Storage.newWriter: one fileset written in path order.  data_ctx must have PFSCDC_OPT_REF_IDS;
 * store (not NULL) is the chunk client: Copy reads chunks from it, new data and index chunks are
 * uploaded into it.  index_params as for pfscdc_uw_create.  Events are the unordered writer's,
 * with fileset 0; a chunk passed through by reference arrives as a PFSCDC_EV_CHUNK with
 * chunk.copied = 1.  Errors are sticky and named by pfscdc_fsw_last_error.
 *   Storage.Compact: create, one pfscdc_fsw_copy_filesets over all inputs (the task's path
 *     range as the filter), close.
 *   Storage.Concat: create, one pfscdc_fsw_copy_filesets per input in order (each input's paths
 *     after the one before's, or checkPath refuses them), close. */
typedef struct pfscdc_fswriter pfscdc_fswriter;
int pfscdc_fsw_create(pfscdc_ctx* data_ctx, const pfscdc_params* index_params, pfscdc_store* store,
                      pfscdc_uw_cb cb, void* user, pfscdc_fswriter** out);
/* Writer.Delete (writer.go:77-90).  PFSCDC_EINVAL (checkPath): the same (path, tag) as the
 * Delete before, or a path below its path. */
int pfscdc_fsw_delete(pfscdc_fswriter* w, const char* path, const char* tag);
/* Writer.Copy (writer.go:105-125): a fresh Index{Path, File{Tag}} through checkPath (against the
 * Copy before: PFSCDC_EINVAL as above) and Annotate, then per DataRef sizeBytes += SizeBytes and
 * pfscdc_writer_copy.  PFSCDC_ENOTFOUND: a chunk that has to be read is not in the store;
 * PFSCDC_ECORRUPT: it fails verification. */
int pfscdc_fsw_copy(pfscdc_fswriter* w, const char* path, const char* tag,
                    const pfscdc_full_dataref* drs, uint32_t n);
/* CopyFiles(ctx, w, fs, true) (util.go:27-40) over the two lists of an opened fileset: every
 * deletive entry as a Delete, then every additive entry as a Copy.  The Copies go in runs, each
 * prefetched together (pfscdc_writer_prefetch over the run's DataRefs); a run ends once the
 * chunks it will re-roll hold 256 MiB, and their plaintext is dropped after the run.  Either
 * list may be NULL (empty). */
int pfscdc_fsw_copy_lists(pfscdc_fswriter* w, const pfscdc_index_list* additive,
                          const pfscdc_index_list* deletive);
/* Storage.Open(ids, opts...) (storage.go:111-128) and CopyFiles: both roots of every fileset are
 * read with the filter (pfscdc_index_read), merged in both modes (pfscdc_index_merge_ctx) and
 * copied (pfscdc_fsw_copy_lists).  One fileset is read with no merge; none copies nothing. */
int pfscdc_fsw_copy_filesets(pfscdc_fswriter* w, const pfscdc_fileset_info* filesets, uint32_t n,
                             const pfscdc_index_filter* filter);
int pfscdc_fsw_close(pfscdc_fswriter* w); /* Writer.Close (writer.go:151-182) */
/* The Primitive of the closed writer; the roots stay valid until pfscdc_fsw_destroy. */
int pfscdc_fsw_fileset(const pfscdc_fswriter* w, pfscdc_fileset_info* out);
const char* pfscdc_fsw_last_error(const pfscdc_fswriter* w);
int pfscdc_fsw_destroy(pfscdc_fswriter* w);

/* fileset.Clean(p, isDir) (fileset/util.go:67-77) into out (cap bytes incl. NUL). */
int pfscdc_path_clean(const char* path, int is_directory, char* out, uint64_t cap);

/* ---- tuning knobs (no reference counterpart; INTEGRATION.md lists each with its range) ----
 * Every knob is one process-wide integer named after its environment variable (PFSCDC_*).
 * The library reads the environment once, the first time any knob is used; an unset, empty,
 * non-numeric or out-of-range variable leaves the default (a bad value is reported on stderr).
 * No knob changes any result: they select between exact forms of the same computation or size
 * the host-fed writer's pools.  pfscdc_set_knob changes a knob for the whole process (atomic:
 * a launch already enqueued keeps the value it read).  When a knob takes effect:
 *   PFSCDC_UW_* (and PFSCDC_CTX_CACHE for the contexts it makes): when an unordered writer
 *     is created, for that writer's lifetime;
 *   PFSCDC_COPY_THREADS: once, when the first large Put builds the process-wide copy pool;
 *     from then on setting it to another value returns PFSCDC_ESTATE;
 *   every other knob: at the next call that launches the kernels it selects.
 * PFSCDC_EINVAL for an unknown name or a value outside the knob's range.  A PFSCDC_* variable
 * in the environment that is not a knob is reported on stderr and ignored. */
int pfscdc_set_knob(const char* name, int64_t value);
int pfscdc_get_knob(const char* name, int64_t* value);
/* The i-th knob's name (0-based), NULL past the last; lo/hi (nullable) its range and def
 * (nullable) its built-in default. */
const char* pfscdc_knob_info(int i, int64_t* lo, int64_t* hi, int64_t* def);

/* How the last pfscdc_scan on ctx skipped bytes (bit set): PFSCDC_SCAN_SKIPPED_FIRST_MIN =
 * the first min - 1 bytes of each file were not rolled; PFSCDC_SCAN_SKIPPED_CUTS = the scan
 * also skipped past the cuts it had settled (rank-ordered units; needs min - 1 >= 256 KiB and
 * at most one file per 16 KiB of the batch).  0: every byte was rolled. */
#define PFSCDC_SCAN_SKIPPED_FIRST_MIN 1u
#define PFSCDC_SCAN_SKIPPED_CUTS 2u
int pfscdc_last_scan_mode(pfscdc_ctx* ctx, uint32_t* mode);

#ifdef __cplusplus
}
#endif
#endif /* PFSCDC_H */
