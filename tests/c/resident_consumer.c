/* A plain C99 process that reads filesets back with the index lists staying on the device,
 * through include/pfscdc.h alone: an unordered writer with a store writes several filesets, both
 * indexes of each are read with pfscdc_index_read_dev, merged with pfscdc_index_merge_dev, and
 * the merged resident list is rendered as a tar stream in two windows
 * (pfscdc_dev_list_tar_layout, pfscdc_dev_list_read_tar).  tests/test_gpu_resident.py compares
 * the output with its model.
 *
 * usage: resident_consumer OUT_FILE
 * workload: file /fKK (KK = 00..23) is KK * 997 + 13 bytes, byte j = (KK + j) & 0xff, put with
 * a memory threshold of 40,000 bytes; then /f03 is deleted and /f05 put again as "again".
 * prints: ok FILES FILESETS TOTAL RESIDENT_READS */
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
  pfscdc_dev_list* lists[2 * MAXFS];
  pfscdc_dev_list* merged = NULL;
  pfscdc_index_list* host = NULL;
  uint64_t offs[NFILES + 1], total = 0, first, nw[2] = {0, 0}, stats[8], merge_stats[4];
  uint32_t nfs, n, i, resident = 0;
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
  if (pfscdc_uw_delete(w, "/f03", "") != PFSCDC_OK) return 1;
  if (pfscdc_uw_put(w, "/f05", "", 0, "again", 5) != PFSCDC_OK) return 1;
  if (pfscdc_uw_close(w) != PFSCDC_OK) {
    fprintf(stderr, "close: %s\n", pfscdc_uw_last_error(w));
    return 1;
  }
  nfs = pfscdc_uw_num_filesets(w);
  if (nfs < 2 || nfs > MAXFS) return 1;

  /* both indexes of every fileset as resident lists, on a context of its own, then the merge */
  if (pfscdc_ctx_create(&p, 0, &rctx) != PFSCDC_OK) DIE("ctx_create", rctx);
  for (i = 0; i < nfs; i++) {
    pfscdc_fileset_info info;
    if (pfscdc_uw_fileset(w, i, &info) != PFSCDC_OK) return 1;
    if (pfscdc_index_read_dev(rctx, store, info.deletive_root, info.deletive_root_len, NULL,
                              &lists[2 * i]) != PFSCDC_OK)
      DIE("index_read_dev (deletive)", rctx);
    if (pfscdc_index_read_dev(rctx, store, info.additive_root, info.additive_root_len, NULL,
                              &lists[2 * i + 1]) != PFSCDC_OK)
      DIE("index_read_dev (additive)", rctx);
    if (pfscdc_last_resident_stats(rctx, stats) != PFSCDC_OK) return 1;
    resident += (uint32_t)stats[0];
    if (pfscdc_dev_list_count(lists[2 * i + 1]) != info.num_files ||
        pfscdc_dev_list_count(lists[2 * i]) != info.num_deletes)
      return 1;
  }
  if (pfscdc_index_merge_dev(rctx, PFSCDC_MERGE_FILES, (const pfscdc_dev_list* const*)lists, nfs,
                             &merged) != PFSCDC_OK)
    DIE("index_merge_dev", rctx);
  if (pfscdc_last_merge_stats(rctx, merge_stats) != PFSCDC_OK || merge_stats[0] != 1) return 1;
  n = pfscdc_dev_list_count(merged);
  if (n > NFILES) return 1;

  /* the merged list as a tar stream, in two windows */
  if (pfscdc_dev_list_tar_layout(rctx, merged, &total, offs) != PFSCDC_OK)
    DIE("dev_list_tar_layout", rctx);
  if (offs[0] != 0 || offs[n] + 1024 != total) return 1;
  out = (uint8_t*)malloc(total);
  if (!out) return 1;
  memset(out, 0xa5, total);
  first = total / 2 / 512 * 512;
  if (pfscdc_dev_list_read_tar(rctx, store, merged, 0, first, out, first, 0, &nw[0]) != PFSCDC_OK)
    DIE("dev_list_read_tar (first window)", rctx);
  if (pfscdc_dev_list_read_tar(rctx, store, merged, first, total, out + first, total - first, 0,
                               &nw[1]) != PFSCDC_OK)
    DIE("dev_list_read_tar (second window)", rctx);
  if (nw[0] + nw[1] != total) return 1;
  if (pfscdc_last_resident_stats(rctx, stats) != PFSCDC_OK || stats[7] != 1) return 1;
  /* the list comes to the host only when asked for */
  if (pfscdc_dev_list_download(rctx, merged, &host) != PFSCDC_OK) DIE("dev_list_download", rctx);
  if (pfscdc_index_list_count(host) != n) return 1;
  f = fopen(argv[1], "wb");
  if (!f || fwrite(out, 1, total, f) != total || fclose(f) != 0) return 1;
  printf("ok %u %u %" PRIu64 " %u\n", (unsigned)n, (unsigned)nfs, total, (unsigned)resident);

  for (i = 0; i < 2 * nfs; i++) pfscdc_dev_list_free(lists[i]);
  pfscdc_dev_list_free(merged);
  pfscdc_index_list_free(host);
  free(out);
  free(body);
  if (pfscdc_uw_destroy(w) != PFSCDC_OK || pfscdc_store_destroy(store) != PFSCDC_OK ||
      pfscdc_ctx_destroy(rctx) != PFSCDC_OK || pfscdc_ctx_destroy(ctx) != PFSCDC_OK)
    return 1;
  return 0;
}
