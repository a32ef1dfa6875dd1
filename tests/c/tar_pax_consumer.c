/* A plain C99 process serving GetFileTAR with PAX entries through include/pfscdc.h alone: the
 * default format refuses the list, pfscdc_set_tar_format allows PAX, and the stream is read in
 * one window from a chunk store (pfscdc_store_read_tar) and written to a file.
 * tests/test_gpu_tar_pax.py writes the input file, runs this on the GPU and opens the output
 * with Python's tarfile.
 *
 * usage: tar_pax_consumer CHUNKS_FILE OUT_FILE
 *   CHUNKS_FILE: as tar_consumer.c's (little endian): u32 nchunks, u32 nslices, u32 nfiles; per
 *   chunk id[32] dek[32] u64 size; per slice one pfscdc_slice; per file u32 first, u32 count,
 *   u32 name length, the name; then the chunks' stored bytes back to back.
 * prints
 *   ustar RC RC          the layout and the read under the default format
 *   pax TOTAL WRITTEN    the stream's length under PFSCDC_TAR_USTAR | PFSCDC_TAR_PAX, and the
 *                        bytes the one window wrote
 *   head LEN             the length of the first file's head (pfscdc_tar_head)
 *   einval RC RC         pfscdc_set_tar_format(ctx, PFSCDC_TAR_PAX) and (ctx, 0) */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pfscdc.h"

#define DIE(msg, ctx)                                                      \
  do {                                                                     \
    fprintf(stderr, "%s: %s\n", msg, (ctx) ? pfscdc_last_error(ctx) : ""); \
    return 1;                                                              \
  } while (0)

int main(int argc, char** argv) {
  const int pax = PFSCDC_TAR_USTAR | PFSCDC_TAR_PAX;
  pfscdc_params p;
  pfscdc_ctx* ctx = NULL;
  pfscdc_store* store = NULL;
  pfscdc_ref* refs;
  pfscdc_slice* slices;
  pfscdc_full_dataref* drs;
  pfscdc_tar_file* files;
  uint64_t *offs, *sizes, total = 0, nbytes, nw = 0, k, head = 0;
  uint32_t hdr[3], nchunks, nslices, nfiles, i;
  uint8_t *ctext, *out;
  int rc[2];
  FILE* f;

  if (argc != 3) {
    fprintf(stderr, "usage: %s CHUNKS_FILE OUT_FILE\n", argv[0]);
    return 2;
  }
  f = fopen(argv[1], "rb");
  if (!f || fread(hdr, sizeof hdr[0], 3, f) != 3) return 1;
  nchunks = hdr[0];
  nslices = hdr[1];
  nfiles = hdr[2];
  refs = (pfscdc_ref*)calloc(nchunks + 1, sizeof *refs);
  offs = (uint64_t*)calloc(nchunks + 1, sizeof *offs);
  slices = (pfscdc_slice*)calloc(nslices + 1, sizeof *slices);
  drs = (pfscdc_full_dataref*)calloc(nslices + 1, sizeof *drs);
  files = (pfscdc_tar_file*)calloc(nfiles + 1, sizeof *files);
  sizes = (uint64_t*)calloc(nfiles + 1, sizeof *sizes);
  if (!refs || !offs || !slices || !drs || !files || !sizes || !nfiles) return 1;
  for (i = 0; i < nchunks; i++) {
    uint64_t size;
    if (fread(&refs[i], sizeof refs[i], 1, f) != 1 || fread(&size, sizeof size, 1, f) != 1)
      return 1;
    offs[i + 1] = offs[i] + size;
  }
  if (nslices && fread(slices, sizeof *slices, nslices, f) != nslices) return 1;
  for (i = 0; i < nfiles; i++) {
    uint32_t rec[3];
    char* name;
    if (fread(rec, sizeof rec[0], 3, f) != 3) return 1;
    name = (char*)calloc((size_t)rec[2] + 1, 1);
    if (!name || (rec[2] && fread(name, 1, rec[2], f) != rec[2])) return 1;
    files[i].path = name;
    files[i].first = rec[0];
    files[i].count = rec[1];
    if (rec[0] > nslices || rec[1] > nslices - rec[0]) return 1;
    for (k = rec[0]; k < (uint64_t)rec[0] + rec[1]; k++) sizes[i] += slices[k].size;
  }
  nbytes = offs[nchunks];
  ctext = (uint8_t*)malloc(nbytes ? nbytes : 1);
  if (!ctext || fread(ctext, 1, nbytes, f) != nbytes || fclose(f) != 0) return 1;

  pfscdc_default_params(&p);
  if (pfscdc_ctx_create(&p, 0, &ctx) != PFSCDC_OK) DIE("ctx_create", ctx);
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

  /* the default format: the list is refused, by the layout and by the read */
  rc[0] = pfscdc_tar_layout(files, nfiles, sizes, NULL, &total);
  rc[1] = pfscdc_store_read_tar(ctx, store, files, nfiles, drs, nslices, 0, 512, &hdr, 0, 0, NULL);
  printf("ustar %d %d\n", rc[0], rc[1]);

  /* with PAX allowed: the length before any GPU call, then the whole stream in one window */
  if (pfscdc_tar_layout_format(files, nfiles, sizes, pax, NULL, &total) != PFSCDC_OK) return 1;
  out = (uint8_t*)malloc(total);
  if (!out) return 1;
  memset(out, 0xa5, total);
  if (pfscdc_set_tar_format(ctx, pax) != PFSCDC_OK) DIE("set_tar_format", ctx);
  if (pfscdc_store_read_tar(ctx, store, files, nfiles, drs, nslices, 0, total, out, total, 0,
                            &nw) != PFSCDC_OK)
    DIE("store_read_tar", ctx);
  printf("pax %" PRIu64 " %" PRIu64 "\n", total, nw);
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out, 1, total, f) != total || fclose(f) != 0) return 1;
  if (pfscdc_tar_head(files[0].path, sizes[0], pax, NULL, 0, &head) != PFSCDC_OK) return 1;
  printf("head %" PRIu64 "\n", head);

  rc[0] = pfscdc_set_tar_format(ctx, PFSCDC_TAR_PAX);
  rc[1] = pfscdc_set_tar_format(ctx, 0);
  printf("einval %d %d\n", rc[0], rc[1]);

  if (pfscdc_store_destroy(store) != PFSCDC_OK || pfscdc_ctx_destroy(ctx) != PFSCDC_OK) return 1;
  for (i = 0; i < nfiles; i++) free((void*)files[i].path);
  free(out);
  free(ctext);
  free(sizes);
  free(files);
  free(drs);
  free(slices);
  free(offs);
  free(refs);
  return 0;
}
