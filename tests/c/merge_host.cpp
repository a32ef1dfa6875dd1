/* Stand-alone driver of pfscdc_index_merge_deletive and pfscdc_shard for a host sanitizer build:
 * compiled together with pfs_amd/csrc/index_merge.cpp and index_decode.cpp (no GPU library, no
 * HIP header) under -fsanitize=address,undefined.  argv[1]: the shard threshold; argv[2...]:
 * files holding one level's stream of pbutil frames each ("-": a NULL list).  Prints the
 * deletive merge of the lists ("e <path>\t<tag>\t<records>" per entry), then the shards of
 * that merged list and of the empty list ("s <lower>\t<upper>"), then "ok". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pfscdc.h"

static int on_shard(void* user, const char* lower, const char* upper) {
  ++*(int*)user;
  printf("s %s\t%s\n", lower, upper);
  return 0;
}

static int stop(void*, const char*, const char*) { return 1; }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const long long threshold = atoll(argv[1]);
  std::vector<pfscdc_index_list*> lists;
  for (int i = 2; i < argc; i++) {
    if (strcmp(argv[i], "-") == 0) {
      lists.push_back(NULL);
      continue;
    }
    FILE* f = fopen(argv[i], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* all = (uint8_t*)malloc(n ? (size_t)n : 1);  // exactly n bytes: a read past them reports
    if (fread(all, 1, (size_t)n, f) != (size_t)n) return 2;
    fclose(f);
    pfscdc_index_list* l = NULL;
    if (pfscdc_index_decode_host(all, (uint64_t)n, &l, NULL) != PFSCDC_OK) return 3;
    free(all);
    lists.push_back(l);
  }
  pfscdc_index_list* m = NULL;
  if (pfscdc_index_merge_deletive(lists.data(), (uint32_t)lists.size(), &m) != PFSCDC_OK || !m) return 4;
  const pfscdc_index_entry* e = pfscdc_index_list_entries(m);
  uint64_t blen = 0;
  const char* blob = pfscdc_index_list_blob(m, &blen);
  uint32_t ndr = 0, at = 0;
  (void)pfscdc_index_list_datarefs(m, &ndr);
  for (uint32_t i = 0; i < pfscdc_index_list_count(m); i++) {
    const uint32_t recs = e[i].count + ((e[i].flags & PFSCDC_IDX_HAS_CHUNK_REF) ? 1u : 0u);
    if (e[i].first != at || e[i].path_off + e[i].path_len >= blen) return 5;
    at += recs;
    printf("e %s\t%s\t%u\n", blob + e[i].path_off, blob + e[i].tag_off, recs);
  }
  if (at != ndr) return 5;
  int calls = 0;
  if (pfscdc_shard(m, threshold, on_shard, &calls) != PFSCDC_OK || calls < 1) return 6;
  calls = 0;
  if (pfscdc_shard(NULL, threshold, on_shard, &calls) != PFSCDC_OK || calls != 1) return 6;
  if (pfscdc_shard(m, threshold, stop, NULL) != PFSCDC_ECALLBACK) return 7;
  if (pfscdc_shard(m, threshold, NULL, NULL) != PFSCDC_EINVAL) return 7;
  pfscdc_index_list_free(m);
  if (pfscdc_index_merge_deletive(NULL, 0, &m) != PFSCDC_OK || pfscdc_index_list_count(m) != 0) return 8;
  pfscdc_index_list_free(m);
  for (pfscdc_index_list* l : lists) pfscdc_index_list_free(l);
  printf("ok\n");
  return 0;
}
