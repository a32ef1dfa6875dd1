/* A plain C99 process that serves getFile and globFile of a glob pattern, through
 * include/pfscdc.h alone: an unordered writer with a store writes one fileset, its additive index
 * is read with pfscdc_index_read_dev and wrapped in a Source with PFSCDC_SRC_GLOB, whose FileInfos
 * are printed with their flags (PFSCDC_INFO_MATCH: what globFile reports) and whose list is
 * rendered as a tar stream (what getFile serves).  tests/test_gpu_glob.py compares both with its
 * model.
 *
 * usage: glob_consumer GLOB OUT_FILE
 * workload: file KK (00..23) is KK * 997 + 13 bytes, byte j = (KK + j) & 0xff, at /top/dD/fKK
 * (D = KK % 3), KK = 7 at /top/d1/deep/f07 and KK = 11 at /f11.
 * prints: "i <path>\t<type>\t<size>\t<hash hex>\t<flags>" per entry of the source, then
 *         "ok ENTRIES DIRS_INSERTED DEVICE_ARM MATCHED TOTAL" */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pfscdc.h"

#define NFILES 24

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
  pfscdc_dev_list* files = NULL;
  pfscdc_source *src = NULL, *none = NULL;
  pfscdc_index_list* host = NULL;
  pfscdc_file_info* infos;
  pfscdc_fileset_info info;
  const pfscdc_index_entry* e;
  const char* blob;
  uint64_t blen = 0, total = 0, nw = 0, stats[8];
  uint32_t n, i, matched = 0;
  uint8_t *body, *out;
  char name[32];
  int hit = 0;
  FILE* f;

  if (argc != 3) {
    fprintf(stderr, "usage: %s GLOB OUT_FILE\n", argv[0]);
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
  if (pfscdc_set_knob("PFSCDC_SOURCE", 1) != PFSCDC_OK) return 1;
  if (pfscdc_ctx_create(&p, 0, &ctx) != PFSCDC_OK) DIE("ctx_create", ctx);
  if (pfscdc_set_options(ctx, PFSCDC_OPT_REF_IDS) != PFSCDC_OK) DIE("set_options", ctx);
  if (pfscdc_store_create(&store) != PFSCDC_OK) return 1;
  if (pfscdc_uw_create(ctx, 1000000000, &ip, NULL, NULL, &w) != PFSCDC_OK) DIE("uw_create", ctx);
  if (pfscdc_uw_set_store(w, store) != PFSCDC_OK) DIE("uw_set_store", ctx);
  body = (uint8_t*)malloc(NFILES * 997 + 13);
  if (!body) return 1;
  for (i = 0; i < NFILES; i++) {
    uint32_t j, len = i * 997 + 13;
    for (j = 0; j < len; j++) body[j] = (uint8_t)((i + j) & 0xff);
    if (i == 7) snprintf(name, sizeof name, "/top/d1/deep/f07");
    else if (i == 11) snprintf(name, sizeof name, "/f11");
    else snprintf(name, sizeof name, "/top/d%u/f%02u", (unsigned)(i % 3), (unsigned)i);
    if (pfscdc_uw_put(w, name, "", 0, body, len) != PFSCDC_OK) {
      fprintf(stderr, "put: %s\n", pfscdc_uw_last_error(w));
      return 1;
    }
  }
  if (pfscdc_uw_close(w) != PFSCDC_OK) {
    fprintf(stderr, "close: %s\n", pfscdc_uw_last_error(w));
    return 1;
  }
  if (pfscdc_uw_num_filesets(w) != 1 || pfscdc_uw_fileset(w, 0, &info) != PFSCDC_OK) return 1;

  /* the commit's files as a resident list, on a context of its own */
  if (pfscdc_ctx_create(&p, 0, &rctx) != PFSCDC_OK) DIE("ctx_create", rctx);
  if (pfscdc_index_read_dev(rctx, store, info.additive_root, info.additive_root_len, NULL,
                            &files) != PFSCDC_OK)
    DIE("index_read_dev", rctx);
  if (pfscdc_dev_list_count(files) != NFILES) return 1;

  /* the glob's stream: what getFile serves, with globFile's entries flagged */
  if (pfscdc_source_open(rctx, files, PFSCDC_SRC_GLOB, argv[1], NULL, 0, &src) != PFSCDC_OK)
    DIE("source_open (glob)", rctx);
  if (pfscdc_last_source_stats(rctx, stats) != PFSCDC_OK) return 1;
  n = pfscdc_source_count(src);
  if (n != stats[2]) return 1;
  infos = (pfscdc_file_info*)malloc(sizeof(pfscdc_file_info) * (n + 1));
  if (!infos) return 1;
  if (pfscdc_source_infos(rctx, src, infos) != PFSCDC_OK) DIE("source_infos", rctx);
  if (pfscdc_dev_list_download(rctx, pfscdc_source_list(src), &host) != PFSCDC_OK)
    DIE("dev_list_download", rctx);
  if (pfscdc_index_list_count(host) != n) return 1;
  e = pfscdc_index_list_entries(host);
  blob = pfscdc_index_list_blob(host, &blen);
  for (i = 0; i < n; i++) {
    int k;
    /* the flag is the specification's answer for the entry's own path */
    if (pfscdc_glob_match(argv[1], blob + e[i].path_off, &hit) != PFSCDC_OK) return 1;
    if ((hit != 0) != ((infos[i].flags & PFSCDC_INFO_MATCH) != 0)) return 1;
    matched += (uint32_t)hit;
    printf("i %s\t%u\t%" PRId64 "\t", blob + e[i].path_off, (unsigned)infos[i].type, infos[i].size);
    for (k = 0; k < 32; k++) printf("%02x", infos[i].hash[k]);
    printf("\t%u\n", (unsigned)infos[i].flags);
  }

  /* getFile: the stream as a tar */
  if (pfscdc_dev_list_tar_layout(rctx, pfscdc_source_list(src), &total, NULL) != PFSCDC_OK)
    DIE("dev_list_tar_layout", rctx);
  out = (uint8_t*)malloc(total ? total : 1);
  if (!out) return 1;
  memset(out, 0xa5, total);
  if (pfscdc_dev_list_read_tar(rctx, store, pfscdc_source_list(src), 0, total, out, total, 0,
                               &nw) != PFSCDC_OK)
    DIE("dev_list_read_tar", rctx);
  if (nw != total) return 1;
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out, 1, total, f) != total || fclose(f) != 0) return 1;

  /* nothing matched (getFile's ErrFileNotFound), a glob that does not compile, and extglob */
  if (pfscdc_source_open(rctx, files, PFSCDC_SRC_GLOB, "/top/d9*", NULL, 0, &none) != PFSCDC_ENOTFOUND ||
      none != NULL)
    return 1;
  if (pfscdc_source_open(rctx, files, PFSCDC_SRC_GLOB, "/top/[", NULL, 0, &none) != PFSCDC_EINVAL ||
      none != NULL || !strstr(pfscdc_last_error(rctx), "/top/["))
    return 1;
  if (pfscdc_source_open(rctx, files, PFSCDC_SRC_GLOB, "/top/@(a)", NULL, 0, &none) != PFSCDC_EUNSUPPORTED ||
      none != NULL || !strstr(pfscdc_last_error(rctx), "/top/@(a)"))
    return 1;
  printf("ok %u %u %u %u %" PRIu64 "\n", (unsigned)n, (unsigned)stats[3], (unsigned)stats[0],
         (unsigned)matched, total);

  pfscdc_source_free(src);
  pfscdc_dev_list_free(files);
  pfscdc_index_list_free(host);
  free(infos);
  free(out);
  free(body);
  if (pfscdc_uw_destroy(w) != PFSCDC_OK || pfscdc_store_destroy(store) != PFSCDC_OK ||
      pfscdc_ctx_destroy(rctx) != PFSCDC_OK || pfscdc_ctx_destroy(ctx) != PFSCDC_OK)
    return 1;
  return 0;
}
