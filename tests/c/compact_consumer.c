/* A plain C99 process that compacts through include/pfscdc.h alone, as a cgo binary in pachd
 * would: an unordered writer with a store writes two (or more) filesets, a fileset writer
 * compacts them (pfscdc_fsw_create, pfscdc_fsw_copy_filesets, pfscdc_fsw_close), the result is
 * read back and rendered as tar, and the tar is compared with the tar of the inputs opened
 * together (read, merged through pfscdc_index_merge_ctx, rendered).
 * tests/test_gpu_compact.py compares the output with its model.
 *
 * usage: compact_consumer OUT_FILE
 * workload: file /fKK (KK = 00..23) is KK * 997 + 13 bytes, byte j = (KK + j) & 0xff, put with
 * a memory threshold of 150,000 bytes; then /f03 is deleted and /f05 put again as "again".
 * prints: ok FILES FILESETS TOTAL CHEAP_COPIES */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pfscdc.h"

#define NFILES 24
#define MAXFS 16

#define DIE(msg, ctx)                                                      \
  do {                                                                     \
    fprintf(stderr, "%s: %s\n", msg, (ctx) ? pfscdc_last_error(ctx) : ""); \
    return 1;                                                              \
  } while (0)

static int on_event(void* user, const pfscdc_uw_event* ev) {
  if (ev->kind == PFSCDC_EV_CHUNK && ev->index == -1 && ev->chunk.copied) ++*(uint32_t*)user;
  return ev->fileset == 0 ? 0 : 1;
}

/* the tar stream of a list into a fresh buffer */
static uint8_t* render(pfscdc_ctx* ctx, const pfscdc_store* store, pfscdc_index_list* l,
                       uint64_t* total) {
  uint64_t sizes[NFILES + 1], nw = 0;
  uint32_t i, ndrs = 0, n = pfscdc_index_list_count(l);
  const pfscdc_index_entry* ents = pfscdc_index_list_entries(l);
  const pfscdc_full_dataref* drs = pfscdc_index_list_datarefs(l, &ndrs);
  const pfscdc_tar_file* files = pfscdc_index_list_tar_files(l);
  uint8_t* out;
  if (n > NFILES) return NULL;
  for (i = 0; i < n; i++) sizes[i] = (uint64_t)ents[i].size_bytes;
  if (pfscdc_tar_layout(files, n, sizes, NULL, total) != PFSCDC_OK) return NULL;
  out = (uint8_t*)malloc(*total);
  if (!out) return NULL;
  if (pfscdc_store_read_tar(ctx, store, files, n, drs, ndrs, 0, *total, out, *total, 0, &nw) !=
          PFSCDC_OK ||
      nw != *total) {
    fprintf(stderr, "store_read_tar: %s\n", pfscdc_last_error(ctx));
    free(out);
    return NULL;
  }
  return out;
}

int main(int argc, char** argv) {
  pfscdc_params p, ip;
  pfscdc_ctx *ctx = NULL, *rctx = NULL;
  pfscdc_store* store = NULL;
  pfscdc_uwriter* w = NULL;
  pfscdc_fswriter* fw = NULL;
  pfscdc_fileset_info infos[MAXFS], compacted;
  pfscdc_index_list* lists[2 * MAXFS];
  pfscdc_index_list *merged = NULL, *back = NULL, *back_del = NULL;
  uint64_t total = 0, total2 = 0;
  uint32_t nfs, i, cheap = 0;
  uint8_t *body, *want, *got;
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
  if (pfscdc_store_create(&store) != PFSCDC_OK) return 1;
  if (pfscdc_uw_create(ctx, 150000, &ip, NULL, NULL, &w) != PFSCDC_OK) DIE("uw_create", ctx);
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
  for (i = 0; i < nfs; i++)
    if (pfscdc_uw_fileset(w, i, &infos[i]) != PFSCDC_OK) return 1;

  /* Storage.Compact: a fresh writer, the inputs opened, merged and copied, Close */
  if (pfscdc_fsw_create(ctx, &ip, NULL, on_event, &cheap, &fw) != PFSCDC_EINVAL) return 1;
  if (pfscdc_fsw_create(ctx, &ip, store, on_event, &cheap, &fw) != PFSCDC_OK) DIE("fsw_create", ctx);
  if (pfscdc_fsw_fileset(fw, &compacted) != PFSCDC_EINVAL) return 1; /* not closed yet */
  if (pfscdc_fsw_copy_filesets(fw, infos, nfs, NULL) != PFSCDC_OK ||
      pfscdc_fsw_close(fw) != PFSCDC_OK || pfscdc_fsw_fileset(fw, &compacted) != PFSCDC_OK) {
    fprintf(stderr, "compact: %s\n", pfscdc_fsw_last_error(fw));
    return 1;
  }
  if (pfscdc_fsw_delete(fw, "/zz", "") != PFSCDC_ESTATE) return 1; /* after Close; sticky */
  if (pfscdc_fsw_close(fw) != PFSCDC_ESTATE) return 1;

  /* the inputs opened together, and the result opened alone, both as tar */
  if (pfscdc_ctx_create(&p, 0, &rctx) != PFSCDC_OK) DIE("ctx_create", rctx);
  for (i = 0; i < nfs; i++) {
    if (pfscdc_index_read(rctx, store, infos[i].deletive_root, infos[i].deletive_root_len, NULL,
                          &lists[2 * i]) != PFSCDC_OK ||
        pfscdc_index_read(rctx, store, infos[i].additive_root, infos[i].additive_root_len, NULL,
                          &lists[2 * i + 1]) != PFSCDC_OK)
      DIE("index_read (inputs)", rctx);
  }
  if (pfscdc_index_merge_ctx(rctx, PFSCDC_MERGE_FILES, (const pfscdc_index_list* const*)lists, nfs,
                             &merged) != PFSCDC_OK)
    DIE("index_merge_ctx", rctx);
  if (pfscdc_index_read(rctx, store, compacted.additive_root, compacted.additive_root_len, NULL,
                        &back) != PFSCDC_OK ||
      pfscdc_index_read(rctx, store, compacted.deletive_root, compacted.deletive_root_len, NULL,
                        &back_del) != PFSCDC_OK)
    DIE("index_read (compacted)", rctx);
  if (pfscdc_index_list_count(back) != compacted.num_files ||
      pfscdc_index_list_count(back_del) != compacted.num_deletes ||
      pfscdc_index_list_count(back) != pfscdc_index_list_count(merged))
    return 1;
  want = render(rctx, store, merged, &total);
  got = render(rctx, store, back, &total2);
  if (!want || !got || total != total2 || memcmp(want, got, total) != 0) {
    fprintf(stderr, "the compacted fileset reads back as another tar\n");
    return 1;
  }
  f = fopen(argv[1], "wb");
  if (!f || fwrite(got, 1, total, f) != total || fclose(f) != 0) return 1;
  printf("ok %u %u %" PRIu64 " %u\n", (unsigned)pfscdc_index_list_count(back), (unsigned)nfs, total,
         (unsigned)cheap);

  for (i = 0; i < 2 * nfs; i++) pfscdc_index_list_free(lists[i]);
  pfscdc_index_list_free(merged);
  pfscdc_index_list_free(back);
  pfscdc_index_list_free(back_del);
  free(want);
  free(got);
  free(body);
  if (pfscdc_fsw_destroy(fw) != PFSCDC_OK || pfscdc_uw_destroy(w) != PFSCDC_OK ||
      pfscdc_store_destroy(store) != PFSCDC_OK || pfscdc_ctx_destroy(rctx) != PFSCDC_OK ||
      pfscdc_ctx_destroy(ctx) != PFSCDC_OK)
    return 1;
  return 0;
}
