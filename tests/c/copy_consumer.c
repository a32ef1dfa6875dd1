/* A plain C99 process that copies a directory of one commit into another through
 * include/pfscdc.h alone, as a cgo binary in pachd would serve a ModifyFile stream with a
 * CopyFile message: an unordered writer with a store writes commit A; a second unordered writer
 * on the same store copies A's /d under /moved/to (pfscdc_uw_copy_file), appends to one of the
 * copies and closes; both commits are opened together, merged and rendered as tar.
 * tests/test_gpu_copy.py compares the output with its model.
 *
 * usage: copy_consumer OUT_FILE
 * workload: file /d/fKK (KK = 00..23) is KK * 997 + 13 bytes, byte j = (KK + j) & 0xff, and
 * /other is "other", put with a memory threshold of 150,000 bytes; the copy's source is spelled
 * "d/" and its destination "moved//to/"; then "appended" is appended to /moved/to/f05.
 * prints: ok FILES COPIED_FILES CHUNKS_BY_REFERENCE */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pfscdc.h"

#define NFILES 24
#define MAXFS 16
#define MAXOUT 64

#define DIE(msg, ctx)                                                      \
  do {                                                                     \
    fprintf(stderr, "%s: %s\n", msg, (ctx) ? pfscdc_last_error(ctx) : ""); \
    return 1;                                                              \
  } while (0)

static int on_event(void* user, const pfscdc_uw_event* ev) {
  if (ev->kind == PFSCDC_EV_CHUNK && ev->index == -1 && ev->chunk.copied) ++*(uint32_t*)user;
  return 0;
}

int main(int argc, char** argv) {
  pfscdc_params p, ip;
  pfscdc_ctx *ctx = NULL, *ctx2 = NULL, *rctx = NULL;
  pfscdc_store* store = NULL;
  pfscdc_uwriter *a = NULL, *w = NULL;
  pfscdc_fileset_info infos[2 * MAXFS];
  pfscdc_index_list* lists[4 * MAXFS];
  pfscdc_index_list* merged = NULL;
  const pfscdc_index_entry* ents;
  const pfscdc_full_dataref* drs;
  const pfscdc_tar_file* files;
  uint64_t sizes[MAXOUT], total = 0, nw = 0;
  uint32_t na, nw_fs, nfs, i, n, ndrs = 0, cheap = 0, copied_files = 0;
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
  ip.seed = 0;
  ip.min_chunk = 3000;
  if (pfscdc_ctx_create(&p, 0, &ctx) != PFSCDC_OK) DIE("ctx_create", ctx);
  if (pfscdc_set_options(ctx, PFSCDC_OPT_REF_IDS) != PFSCDC_OK) DIE("set_options", ctx);
  if (pfscdc_ctx_create(&p, 0, &ctx2) != PFSCDC_OK) DIE("ctx_create", ctx2);
  if (pfscdc_set_options(ctx2, PFSCDC_OPT_REF_IDS) != PFSCDC_OK) DIE("set_options", ctx2);
  if (pfscdc_store_create(&store) != PFSCDC_OK) return 1;

  /* commit A */
  if (pfscdc_uw_create(ctx, 150000, &ip, NULL, NULL, &a) != PFSCDC_OK) DIE("uw_create", ctx);
  if (pfscdc_uw_set_store(a, store) != PFSCDC_OK) DIE("uw_set_store", ctx);
  body = (uint8_t*)malloc(NFILES * 997 + 13);
  if (!body) return 1;
  for (i = 0; i < NFILES; i++) {
    uint32_t j, len = i * 997 + 13;
    for (j = 0; j < len; j++) body[j] = (uint8_t)((i + j) & 0xff);
    snprintf(name, sizeof name, "/d/f%02u", (unsigned)i);
    if (pfscdc_uw_put(a, name, "", 0, body, len) != PFSCDC_OK) {
      fprintf(stderr, "put: %s\n", pfscdc_uw_last_error(a));
      return 1;
    }
  }
  if (pfscdc_uw_put(a, "/other", "", 0, "other", 5) != PFSCDC_OK) return 1;
  if (pfscdc_uw_close(a) != PFSCDC_OK) {
    fprintf(stderr, "close: %s\n", pfscdc_uw_last_error(a));
    return 1;
  }
  na = pfscdc_uw_num_filesets(a);
  if (na < 2 || na > MAXFS) return 1;
  for (i = 0; i < na; i++)
    if (pfscdc_uw_fileset(a, i, &infos[i]) != PFSCDC_OK) return 1;

  /* the writer of the next commit: CopyFile, then a Put that appends to one of the copies */
  if (pfscdc_uw_create(ctx2, 150000, &ip, on_event, &cheap, &w) != PFSCDC_OK) DIE("uw_create", ctx2);
  if (pfscdc_uw_copy_file(w, infos, na, "/d", NULL, "/z", NULL, 0) != PFSCDC_ESTATE) return 1;
  if (pfscdc_uw_destroy(w) != PFSCDC_OK) return 1; /* no store: refused, and the error is sticky */
  if (pfscdc_uw_create(ctx2, 150000, &ip, on_event, &cheap, &w) != PFSCDC_OK) DIE("uw_create", ctx2);
  if (pfscdc_uw_set_store(w, store) != PFSCDC_OK) DIE("uw_set_store", ctx2);
  if (pfscdc_uw_copy_file(w, infos, na, "d/", NULL, "moved//to/", NULL, 0) != PFSCDC_OK) {
    fprintf(stderr, "copy_file: %s\n", pfscdc_uw_last_error(w));
    return 1;
  }
  if (pfscdc_uw_put(w, "/moved/to/f05", "", 1, "appended", 8) != PFSCDC_OK) return 1;
  if (pfscdc_uw_close(w) != PFSCDC_OK) {
    fprintf(stderr, "close: %s\n", pfscdc_uw_last_error(w));
    return 1;
  }
  if (pfscdc_uw_copy(w, NULL, NULL, 0) != PFSCDC_ESTATE) return 1; /* after Close */
  nw_fs = pfscdc_uw_num_filesets(w);
  if (nw_fs != 2) return 1; /* the copy's fileset, then the Put's */
  for (i = 0; i < nw_fs; i++)
    if (pfscdc_uw_fileset(w, i, &infos[na + i]) != PFSCDC_OK) return 1;
  copied_files = infos[na].num_files;
  if (infos[na].num_deletes != copied_files) return 1; /* a Delete in front of every Copy */
  nfs = na + nw_fs;

  /* both commits opened together, as tar */
  if (pfscdc_ctx_create(&p, 0, &rctx) != PFSCDC_OK) DIE("ctx_create", rctx);
  for (i = 0; i < nfs; i++) {
    if (pfscdc_index_read(rctx, store, infos[i].deletive_root, infos[i].deletive_root_len, NULL,
                          &lists[2 * i]) != PFSCDC_OK ||
        pfscdc_index_read(rctx, store, infos[i].additive_root, infos[i].additive_root_len, NULL,
                          &lists[2 * i + 1]) != PFSCDC_OK)
      DIE("index_read", rctx);
  }
  if (pfscdc_index_merge_ctx(rctx, PFSCDC_MERGE_FILES, (const pfscdc_index_list* const*)lists, nfs,
                             &merged) != PFSCDC_OK)
    DIE("index_merge_ctx", rctx);
  n = pfscdc_index_list_count(merged);
  if (n > MAXOUT) return 1;
  ents = pfscdc_index_list_entries(merged);
  drs = pfscdc_index_list_datarefs(merged, &ndrs);
  files = pfscdc_index_list_tar_files(merged);
  for (i = 0; i < n; i++) sizes[i] = (uint64_t)ents[i].size_bytes;
  if (pfscdc_tar_layout(files, n, sizes, NULL, &total) != PFSCDC_OK) return 1;
  out = (uint8_t*)malloc(total);
  if (!out) return 1;
  if (pfscdc_store_read_tar(rctx, store, files, n, drs, ndrs, 0, total, out, total, 0, &nw) !=
          PFSCDC_OK ||
      nw != total)
    DIE("store_read_tar", rctx);
  f = fopen(argv[1], "wb");
  if (!f || fwrite(out, 1, total, f) != total || fclose(f) != 0) return 1;
  printf("ok %u %u %u\n", (unsigned)n, (unsigned)copied_files, (unsigned)cheap);

  for (i = 0; i < 2 * nfs; i++) pfscdc_index_list_free(lists[i]);
  pfscdc_index_list_free(merged);
  free(out);
  free(body);
  if (pfscdc_uw_destroy(w) != PFSCDC_OK || pfscdc_uw_destroy(a) != PFSCDC_OK ||
      pfscdc_store_destroy(store) != PFSCDC_OK || pfscdc_ctx_destroy(rctx) != PFSCDC_OK ||
      pfscdc_ctx_destroy(ctx2) != PFSCDC_OK || pfscdc_ctx_destroy(ctx) != PFSCDC_OK)
    return 1;
  return 0;
}
