/* A plain C99 process that serves diffFile, through include/pfscdc.h alone: two unordered writers
 * with one store write two commits, both additive indexes are read with pfscdc_index_read_dev and
 * wrapped in a Source with PFSCDC_SRC_DIFF, pfscdc_source_diff joins them, and the pairs are held
 * against the two-pointer walk done here over the downloaded sides, the selections against the
 * pairs.  tests/test_gpu_diff.py looks at the printed pairs.
 *
 * workload: the old commit holds file KK (00..11), KK * 397 + 13 bytes, byte j = (KK + j) & 0xff,
 * at /dD/fKK (D = KK % 3).  The new commit rewrites 03 (byte j = (KK + j + 1) & 0xff), deletes 05,
 * adds 12 and moves 07 to /new/f07.
 * prints: "p <old path or ->\t<new path or ->" per pair, then "ok PAIRS DEVICE_ARM" */
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

/* One commit written into store; its additive index comes back as a resident list on rctx. */
static int commit(pfscdc_ctx* ctx, pfscdc_ctx* rctx, pfscdc_store* store, const pfscdc_params* ip,
                  int second, pfscdc_dev_list** files) {
  pfscdc_uwriter* w = NULL;
  pfscdc_fileset_info info;
  uint8_t body[12 * 397 + 13];
  char name[32];
  uint32_t k;
  if (pfscdc_uw_create(ctx, 1000000000, ip, NULL, NULL, &w) != PFSCDC_OK) DIE("uw_create", ctx);
  if (pfscdc_uw_set_store(w, store) != PFSCDC_OK) DIE("uw_set_store", ctx);
  for (k = 0; k < 13; k++) {
    uint32_t j, len = k * 397 + 13;
    if (second ? k == 5 : k == 12) continue;
    for (j = 0; j < len; j++) body[j] = (uint8_t)((k + j + (second && k == 3)) & 0xff);
    if (second && k == 7) snprintf(name, sizeof name, "/new/f07");
    else snprintf(name, sizeof name, "/d%u/f%02u", (unsigned)(k % 3), (unsigned)k);
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
  if (pfscdc_index_read_dev(rctx, store, info.additive_root, info.additive_root_len, NULL,
                            files) != PFSCDC_OK)
    DIE("index_read_dev", rctx);
  if (pfscdc_uw_destroy(w) != PFSCDC_OK) return 1;
  return 0;
}

struct side {
  pfscdc_index_list* list;
  pfscdc_file_info* infos;
  const pfscdc_index_entry* e;
  const char* blob;
  uint32_t n;
};

static int fetch(pfscdc_ctx* ctx, pfscdc_source* src, struct side* s) {
  uint64_t blen = 0;
  s->n = pfscdc_source_count(src);
  s->infos = (pfscdc_file_info*)malloc(sizeof(pfscdc_file_info) * (s->n + 1));
  if (!s->infos) return 1;
  if (pfscdc_source_infos(ctx, src, s->infos) != PFSCDC_OK) DIE("source_infos", ctx);
  if (pfscdc_dev_list_download(ctx, pfscdc_source_list(src), &s->list) != PFSCDC_OK)
    DIE("dev_list_download", ctx);
  if (pfscdc_index_list_count(s->list) != s->n) return 1;
  s->e = pfscdc_index_list_entries(s->list);
  s->blob = pfscdc_index_list_blob(s->list, &blen);
  return 0;
}

static void drop(struct side* s) {
  pfscdc_index_list_free(s->list);
  free(s->infos);
}

static const char* path_of(const struct side* s, uint32_t i) { return s->blob + s->e[i].path_off; }

int main(void) {
  pfscdc_params p, ip;
  pfscdc_ctx *ctx = NULL, *rctx = NULL;
  pfscdc_store* store = NULL;
  pfscdc_dev_list *old_files = NULL, *new_files = NULL;
  pfscdc_source *old_src = NULL, *new_src = NULL, *none = NULL;
  pfscdc_diff *diff = NULL, *from_nil = NULL;
  pfscdc_diff_pair* pairs;
  struct side a, b, sa, sb;
  uint64_t n, k, stats[8];
  uint32_t i = 0, j = 0, ia = 0, ib = 0;

  pfscdc_default_params(&p);
  p.average_bits = 12;
  p.min_chunk = 2000;
  p.max_chunk = 30000;
  ip = p;
  ip.average_bits = 9;
  ip.seed = 0;
  ip.min_chunk = 300;
  ip.max_chunk = 1000;
  if (pfscdc_set_knob("PFSCDC_DIFF", 1) != PFSCDC_OK) return 1;
  if (pfscdc_ctx_create(&p, 0, &ctx) != PFSCDC_OK) DIE("ctx_create", ctx);
  if (pfscdc_set_options(ctx, PFSCDC_OPT_REF_IDS) != PFSCDC_OK) DIE("set_options", ctx);
  if (pfscdc_ctx_create(&p, 0, &rctx) != PFSCDC_OK) DIE("ctx_create", rctx);
  if (pfscdc_store_create(&store) != PFSCDC_OK) return 1;
  if (commit(ctx, rctx, store, &ip, 0, &old_files) || commit(ctx, rctx, store, &ip, 1, &new_files))
    return 1;
  if (pfscdc_dev_list_count(old_files) != 12 || pfscdc_dev_list_count(new_files) != 12) return 1;

  /* diffFile(old "/", new "/") */
  if (pfscdc_source_open(rctx, old_files, PFSCDC_SRC_DIFF, "/", NULL, 0, &old_src) != PFSCDC_OK)
    DIE("source_open (old)", rctx);
  if (pfscdc_source_open(rctx, new_files, PFSCDC_SRC_DIFF, "/", NULL, 0, &new_src) != PFSCDC_OK)
    DIE("source_open (new)", rctx);
  if (pfscdc_source_diff(rctx, old_src, new_src, &diff) != PFSCDC_OK) DIE("source_diff", rctx);
  if (pfscdc_last_diff_stats(rctx, stats) != PFSCDC_OK) return 1;
  n = pfscdc_diff_count(diff);
  if (n != stats[3] || n == 0) return 1;
  pairs = (pfscdc_diff_pair*)malloc(sizeof(pfscdc_diff_pair) * n);
  if (!pairs) return 1;
  if (pfscdc_diff_pairs(rctx, diff, pairs) != PFSCDC_OK) DIE("diff_pairs", rctx);
  if (fetch(rctx, old_src, &a) || fetch(rctx, new_src, &b) ||
      fetch(rctx, pfscdc_diff_side(diff, 0), &sa) || fetch(rctx, pfscdc_diff_side(diff, 1), &sb))
    return 1;
  if (pfscdc_diff_side(diff, 2) != NULL) return 1;

  /* Differ.Iterate over the downloaded sides: pair k is what the walk reports k-th, and its
   * members are the next entries of the two selections */
  for (k = 0; k < n; k++) {
    uint32_t wa = PFSCDC_DIFF_NONE, wb = PFSCDC_DIFF_NONE;
    for (;;) {
      int c;
      if (i >= a.n && j >= b.n) return 3;
      c = i >= a.n ? 1 : j >= b.n ? -1 : strcmp(path_of(&a, i), path_of(&b, j));
      if (c < 0) {
        wa = i++;
        break;
      }
      if (c > 0) {
        wb = j++;
        break;
      }
      if (memcmp(a.infos[i].hash, b.infos[j].hash, 32) != 0) {
        wa = i++;
        wb = j++;
        break;
      }
      i++;
      j++;
    }
    if (pairs[k].a != wa || pairs[k].b != wb) return 3;
    if (wa != PFSCDC_DIFF_NONE) {
      if (ia >= sa.n || strcmp(path_of(&sa, ia), path_of(&a, wa)) != 0 ||
          memcmp(&sa.infos[ia], &a.infos[wa], sizeof(pfscdc_file_info)) != 0 ||
          sa.e[ia].count != a.e[wa].count)
        return 4;
      ia++;
    }
    if (wb != PFSCDC_DIFF_NONE) {
      if (ib >= sb.n || strcmp(path_of(&sb, ib), path_of(&b, wb)) != 0 ||
          memcmp(&sb.infos[ib], &b.infos[wb], sizeof(pfscdc_file_info)) != 0 ||
          sb.e[ib].count != b.e[wb].count)
        return 4;
      ib++;
    }
    printf("p %s\t%s\n", wa != PFSCDC_DIFF_NONE ? path_of(&a, wa) : "-",
           wb != PFSCDC_DIFF_NONE ? path_of(&b, wb) : "-");
  }
  /* nothing is left to report, and the selections hold nothing else */
  for (; i < a.n && j < b.n; i++, j++)
    if (strcmp(path_of(&a, i), path_of(&b, j)) != 0 ||
        memcmp(a.infos[i].hash, b.infos[j].hash, 32) != 0)
      return 5;
  if (i != a.n || j != b.n || ia != sa.n || ib != sb.n) return 5;

  /* the nil parent commit: every entry of the new one, alone */
  if (pfscdc_source_diff(rctx, NULL, new_src, &from_nil) != PFSCDC_OK) DIE("source_diff (nil)", rctx);
  if (pfscdc_diff_count(from_nil) != b.n || pfscdc_source_count(pfscdc_diff_side(from_nil, 0)) != 0 ||
      pfscdc_source_count(pfscdc_diff_side(from_nil, 1)) != b.n)
    return 6;
  pfscdc_diff_free(from_nil);
  /* a path the commit lacks is an empty side, not ErrFileNotFound; no side b is an error */
  if (pfscdc_source_open(rctx, old_files, PFSCDC_SRC_DIFF, "/new", NULL, 0, &none) != PFSCDC_OK ||
      pfscdc_source_count(none) != 0)
    return 6;
  if (pfscdc_source_diff(rctx, old_src, NULL, &from_nil) != PFSCDC_EINVAL || from_nil != NULL) return 6;
  printf("ok %" PRIu64 " %u\n", n, (unsigned)stats[0]);

  drop(&a);
  drop(&b);
  drop(&sa);
  drop(&sb);
  free(pairs);
  pfscdc_diff_free(diff);
  pfscdc_source_free(none);
  pfscdc_source_free(old_src);
  pfscdc_source_free(new_src);
  pfscdc_dev_list_free(old_files);
  pfscdc_dev_list_free(new_files);
  if (pfscdc_store_destroy(store) != PFSCDC_OK || pfscdc_ctx_destroy(rctx) != PFSCDC_OK ||
      pfscdc_ctx_destroy(ctx) != PFSCDC_OK)
    return 1;
  return 0;
}
