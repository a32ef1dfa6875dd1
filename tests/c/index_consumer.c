/* A plain C99 process that closes the loop through include/pfscdc.h alone, as a cgo binary in
 * pachd would: an unordered writer with a store writes several filesets, both indexes of each
 * are read back from their roots (pfscdc_index_read), merged (pfscdc_index_merge) and the
 * merged list is rendered as a tar stream in two windows (pfscdc_store_read_tar over the
 * list's own arrays).  tests/test_gpu_index_read.py compares the output with its model.
 *
 * usage: index_consumer OUT_FILE
 * workload: file /fKK (KK = 00..23) is KK * 997 + 13 bytes, byte j = (KK + j) & 0xff, put with
 * a memory threshold of 40,000 bytes; then /f03 is deleted and /f05 put again as "again".
 * prints: ok FILES FILESETS TOTAL */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pfscdc.h"

#define NFILES 24
#define MAXFS 64

#define DIE(msg, ctx)                                                      \
  do {                                                                     \
    fprintf(stderr, "%s: %s\n", msg, (ctx) ? pfscdc_last_error(ctx) : ""); \
    return 1;                                                              \
  } while (0)

int main(int argc, char** argv) {
  pfscdc_params p, ip;
  pfscdc_ctx *ctx = NULL, *rctx = NULL;
  pfscdc_store* store = NULL;
  pfscdc_uwriter* w = NULL;
  pfscdc_index_list* lists[2 * MAXFS];
  pfscdc_index_list* merged = NULL;
  const pfscdc_index_entry* ents;
  const pfscdc_full_dataref* drs;
  const pfscdc_tar_file* files;
  uint64_t sizes[NFILES + 1], total = 0, first, nw[2] = {0, 0};
  uint32_t nfs, n, ndrs = 0, i;
  uint8_t *body, *out;
  char name[16];
  FILE* f;

  if (argc != 2) {
    fprintf(stderr, "usage: %s OUT_FILE\n", argv[0]);
    return 2;
  }
  pfscdc_default_params(&p);
  p.average_bits = 12;
  p.min_chunk = 2000;
  p.max_chunk = 30000;
  ip = p;
  ip.average_bits = 9;
  ip.seed = 0;
  ip.min_chunk = 300;
  ip.max_chunk = 1000;
  if (pfscdc_ctx_create(&p, 0, &ctx) != PFSCDC_OK) DIE("ctx_create", ctx);
  if (pfscdc_set_options(ctx, PFSCDC_OPT_REF_IDS) != PFSCDC_OK) DIE("set_options", ctx);
  if (pfscdc_store_create(&store) != PFSCDC_OK) return 1;
  if (pfscdc_uw_create(ctx, 40000, &ip, NULL, NULL, &w) != PFSCDC_OK) DIE("uw_create", ctx);
  if (pfscdc_uw_set_store(w, store) != PFSCDC_OK) DIE("uw_set_store", ctx);
  body = (uint8_t*)malloc(NFILES * 997 + 13);
  if (!body) return 1;
  for (i = 0; i < NFILES; i++) {
    uint32_t j, len = i * 997 + 13;
    for (j = 0; j < len; j++) body[j] = (uint8_t)((i + j) & 0xff);
    snprintf(name, sizeof name, "/f%02u", (unsigned)i);
    if (pfscdc_uw_put(w, name, "", 0, body, len) != PFSCDC_OK) {
      fprintf(stderr, "put: %s\n", pfscdc_uw_last_error(w));
      return 1;
    }
  }
  if (pfscdc_uw_set_store(w, NULL) != PFSCDC_ESTATE) return 1; /* only before the first Put */
  if (pfscdc_uw_delete(w, "/f03", "") != PFSCDC_OK) return 1;
  if (pfscdc_uw_put(w, "/f05", "", 0, "again", 5) != PFSCDC_OK) return 1;
  if (pfscdc_uw_close(w) != PFSCDC_OK) {
    fprintf(stderr, "close: %s\n", pfscdc_uw_last_error(w));
    return 1;
  }
  nfs = pfscdc_uw_num_filesets(w);
  if (nfs < 2 || nfs > MAXFS) return 1;

  /* read both indexes of every fileset back on a context of its own, and merge them */
  if (pfscdc_ctx_create(&p, 0, &rctx) != PFSCDC_OK) DIE("ctx_create", rctx);
  for (i = 0; i < nfs; i++) {
    pfscdc_fileset_info info;
    if (pfscdc_uw_fileset(w, i, &info) != PFSCDC_OK) return 1;
    if (pfscdc_index_read(rctx, store, info.deletive_root, info.deletive_root_len, NULL,
                          &lists[2 * i]) != PFSCDC_OK)
      DIE("index_read (deletive)", rctx);
    if (pfscdc_index_read(rctx, store, info.additive_root, info.additive_root_len, NULL,
                          &lists[2 * i + 1]) != PFSCDC_OK)
      DIE("index_read (additive)", rctx);
    if (pfscdc_index_list_count(lists[2 * i + 1]) != info.num_files ||
        pfscdc_index_list_count(lists[2 * i]) != info.num_deletes)
      return 1;
  }
  if (pfscdc_index_merge((const pfscdc_index_list* const*)lists, nfs, &merged) != PFSCDC_OK)
    return 1;
  n = pfscdc_index_list_count(merged);
  if (n > NFILES) return 1;
  ents = pfscdc_index_list_entries(merged);
  drs = pfscdc_index_list_datarefs(merged, &ndrs);
  files = pfscdc_index_list_tar_files(merged);
  for (i = 0; i < n; i++) sizes[i] = (uint64_t)ents[i].size_bytes;

  /* the merged list as a tar stream, in two windows */
  if (pfscdc_tar_layout(files, n, sizes, NULL, &total) != PFSCDC_OK) return 1;
  out = (uint8_t*)malloc(total);
  if (!out) return 1;
  memset(out, 0xa5, total);
  first = total / 2 / 512 * 512;
  if (pfscdc_store_read_tar(rctx, store, files, n, drs, ndrs, 0, first, out, first, 0, &nw[0]) !=
      PFSCDC_OK)
    DIE("store_read_tar (first window)", rctx);
  if (pfscdc_store_read_tar(rctx, store, files, n, drs, ndrs, first, total, out + first,
                            total - first, 0, &nw[1]) != PFSCDC_OK)
    DIE("store_read_tar (second window)", rctx);
  if (nw[0] + nw[1] != total) return 1;
  f = fopen(argv[1], "wb");
  if (!f || fwrite(out, 1, total, f) != total || fclose(f) != 0) return 1;
  printf("ok %u %u %" PRIu64 "\n", (unsigned)n, (unsigned)nfs, total);

  for (i = 0; i < 2 * nfs; i++) pfscdc_index_list_free(lists[i]);
  pfscdc_index_list_free(merged);
  free(out);
  free(body);
  if (pfscdc_uw_destroy(w) != PFSCDC_OK || pfscdc_store_destroy(store) != PFSCDC_OK ||
      pfscdc_ctx_destroy(rctx) != PFSCDC_OK || pfscdc_ctx_destroy(ctx) != PFSCDC_OK)
    return 1;
  return 0;
}
