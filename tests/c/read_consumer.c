/* A plain C99 process driving the read path through include/pfscdc.h alone, as a cgo binary in
 * pachd would: chunk.Reader.Get over a batch of stored chunks (pfscdc_read_slices) and over a
 * chunk store (pfscdc_store_read).  tests/test_gpu_read.py writes the input file, runs this on
 * the GPU and checks every line.
 *
 * usage: read_consumer CHUNKS_FILE
 *   CHUNKS_FILE (little endian): u32 nchunks, u32 nslices; per chunk id[32] dek[32] u64 size;
 *   per slice one pfscdc_slice; then the chunks' stored bytes back to back.
 * prints
 *   slices TOTAL FNV1A64 ok FLAGS    pfscdc_read_slices, host memory in and out
 *   store TOTAL FNV1A64              pfscdc_store_read of the same slices as DataRefs
 *   einval RC RC RC                  chunk index out of range, slice past its chunk's end,
 *                                    out overlapping ctext
 *   missing RC                       pfscdc_store_read with an id the store lacks */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pfscdc.h"

static uint64_t fnv1a64(const uint8_t* b, uint64_t n) {
  uint64_t h = 0xcbf29ce484222325ull, i;
  for (i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
  return h;
}

#define DIE(msg, ctx)                                                      \
  do {                                                                     \
    fprintf(stderr, "%s: %s\n", msg, (ctx) ? pfscdc_last_error(ctx) : ""); \
    return 1;                                                              \
  } while (0)

int main(int argc, char** argv) {
  pfscdc_params p;
  pfscdc_ctx* ctx = NULL;
  pfscdc_store* store = NULL;
  pfscdc_ref* refs;
  pfscdc_slice *slices, bad;
  pfscdc_full_dataref* drs;
  uint64_t *offs, total = 0, nbytes, nw = 0;
  uint32_t hdr[2], nchunks, nslices, i;
  uint8_t *ctext, *out, *ok, *pinned;
  int rc[3], r;
  FILE* f;

  if (argc != 2) {
    fprintf(stderr, "usage: %s CHUNKS_FILE\n", argv[0]);
    return 2;
  }
  f = fopen(argv[1], "rb");
  if (!f || fread(hdr, sizeof hdr[0], 2, f) != 2) return 1;
  nchunks = hdr[0];
  nslices = hdr[1];
  refs = (pfscdc_ref*)calloc(nchunks + 1, sizeof *refs);
  offs = (uint64_t*)calloc(nchunks + 1, sizeof *offs);
  slices = (pfscdc_slice*)calloc(nslices + 1, sizeof *slices);
  drs = (pfscdc_full_dataref*)calloc(nslices + 1, sizeof *drs);
  ok = (uint8_t*)calloc(nchunks + 1, 1);
  if (!refs || !offs || !slices || !drs || !ok) return 1;
  for (i = 0; i < nchunks; i++) {
    uint64_t size;
    if (fread(&refs[i], sizeof refs[i], 1, f) != 1 || fread(&size, sizeof size, 1, f) != 1)
      return 1;
    offs[i + 1] = offs[i] + size;
  }
  if (nslices && fread(slices, sizeof *slices, nslices, f) != nslices) return 1;
  nbytes = offs[nchunks];
  ctext = (uint8_t*)malloc(nbytes ? nbytes : 1);
  if (!ctext || fread(ctext, 1, nbytes, f) != nbytes || fclose(f) != 0) return 1;
  for (i = 0; i < nslices; i++) total += slices[i].size;
  out = (uint8_t*)malloc(total ? total : 1);
  if (!out) return 1;

  pfscdc_default_params(&p);
  if (pfscdc_ctx_create(&p, 0, &ctx) != PFSCDC_OK) DIE("ctx_create", ctx);

  /* 1. the batch form */
  if (pfscdc_read_slices(ctx, ctext, nbytes, 0, offs, nchunks, refs, NULL, slices, nslices, out,
                         0, ok, NULL) != PFSCDC_OK)
    DIE("read_slices", ctx);
  printf("slices %" PRIu64 " %016" PRIx64 " ok ", total, fnv1a64(out, total));
  for (i = 0; i < nchunks; i++) putchar(ok[i] ? '1' : '0');
  printf("\n");

  /* 2. the same slices as DataRefs against a store */
  if (pfscdc_store_create(&store) != PFSCDC_OK) return 1;
  for (i = 0; i < nchunks; i++)
    if (pfscdc_store_put(store, refs[i].id, ctext + offs[i], offs[i + 1] - offs[i]) != PFSCDC_OK)
      return 1;
  for (i = 0; i < nslices; i++) {
    uint32_t c = slices[i].chunk;
    drs[i].ref = refs[c];
    drs[i].ref_size = (int64_t)(offs[c + 1] - offs[c]);
    drs[i].data.offset_bytes = (int64_t)slices[i].offset;
    drs[i].data.size_bytes = (int64_t)slices[i].size;
  }
  memset(out, 0, total);
  if (pfscdc_store_read(ctx, store, drs, nslices, out, total, 0, &nw) != PFSCDC_OK)
    DIE("store_read", ctx);
  printf("store %" PRIu64 " %016" PRIx64 "\n", nw, fnv1a64(out, nw));

  /* 3. rejected arguments */
  memset(&bad, 0, sizeof bad);
  bad.chunk = nchunks;
  rc[0] = pfscdc_read_slices(ctx, ctext, nbytes, 0, offs, nchunks, refs, NULL, &bad, 1, out, 0,
                             ok, NULL);
  bad.chunk = nchunks - 1;
  bad.offset = 1;
  bad.size = offs[nchunks] - offs[nchunks - 1];
  rc[1] = pfscdc_read_slices(ctx, ctext, nbytes, 0, offs, nchunks, refs, NULL, &bad, 1, out, 0,
                             ok, NULL);
  /* both sides device-visible (page-locked) memory, out inside ctext */
  pinned = (uint8_t*)pfscdc_host_alloc(nbytes + 64);
  if (!pinned) return 1;
  memcpy(pinned, ctext, nbytes);
  bad.offset = 0;
  bad.size = 1;
  rc[2] = pfscdc_read_slices(ctx, pinned, nbytes, 1, offs, nchunks, refs, NULL, &bad, 1,
                             pinned + nbytes - 1, 1, ok, NULL);
  pfscdc_host_free(pinned);
  printf("einval %d %d %d\n", rc[0], rc[1], rc[2]);

  /* 4. a DataRef whose chunk the store lacks */
  drs[0].ref.id[0] ^= 0xff;
  r = pfscdc_store_read(ctx, store, drs, nslices, out, total, 0, &nw);
  printf("missing %d\n", r);

  if (pfscdc_store_destroy(store) != PFSCDC_OK || pfscdc_ctx_destroy(ctx) != PFSCDC_OK) return 1;
  free(out);
  free(ctext);
  free(ok);
  free(drs);
  free(slices);
  free(offs);
  free(refs);
  return 0;
}
