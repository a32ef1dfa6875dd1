/* Stand-alone driver of pfscdc_copy_map_host for a host sanitizer build: compiled together with
 * pfs_amd/csrc/copy_map.cpp and index_decode.cpp (no GPU library, no HIP header) under
 * -fsanitize=address,undefined.  argv[1]: a job file, one job per line:
 *   <stream file>\t<src>\t<src tag>\t<dst>
 * the stream file holding one level's pbutil frames ("-": a NULL list).  Per job it prints
 * "j <rc>", then per entry
 *   "e <path>\t<tag>\t<size>\t<count>\t<first DataRef's hash in hex, or ->", and "ok" at the end. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pfscdc.h"

static pfscdc_index_list* load(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) exit(2);
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t* all = (uint8_t*)malloc(n ? (size_t)n : 1);  // exactly n bytes: a read past them reports
  if (fread(all, 1, (size_t)n, f) != (size_t)n) exit(2);
  fclose(f);
  pfscdc_index_list* l = NULL;
  if (pfscdc_index_decode_host(all, (uint64_t)n, &l, NULL) != PFSCDC_OK) exit(3);
  free(all);
  return l;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* jobs = fopen(argv[1], "rb");
  if (!jobs) return 2;
  char line[4096];
  while (fgets(line, sizeof line, jobs)) {
    size_t len = strlen(line);
    if (len && line[len - 1] == '\n') line[--len] = 0;
    char* t1 = strchr(line, '\t');
    char* t2 = t1 ? strchr(t1 + 1, '\t') : NULL;
    char* t3 = t2 ? strchr(t2 + 1, '\t') : NULL;
    if (!t3) return 2;
    *t1 = *t2 = *t3 = 0;
    pfscdc_index_list* in = strcmp(line, "-") ? load(line) : NULL;
    pfscdc_index_list* out = NULL;
    const int rc = pfscdc_copy_map_host(in, t1 + 1, t2 + 1, t3 + 1, &out);
    printf("j %d\n", rc);
    if (rc == PFSCDC_OK) {
      if (!out) return 4;
      const pfscdc_index_entry* e = pfscdc_index_list_entries(out);
      uint64_t blen = 0;
      const char* blob = pfscdc_index_list_blob(out, &blen);
      uint32_t ndr = 0, at = 0;
      const pfscdc_full_dataref* drs = pfscdc_index_list_datarefs(out, &ndr);
      for (uint32_t i = 0; i < pfscdc_index_list_count(out); i++) {
        if (e[i].first != at || e[i].last_path_off >= blen || e[i].last_path_len != 0) return 5;
        at += e[i].count;
        if (at > ndr) return 5;
        char hex[65] = "-";
        for (int k = 0; e[i].count && k < 32; k++)
          snprintf(hex + 2 * k, 3, "%02x", drs[e[i].first].data.hash[k]);
        printf("e %s\t%s\t%lld\t%u\t%s\n", blob + e[i].path_off, blob + e[i].tag_off,
               (long long)e[i].size_bytes, e[i].count, hex);
      }
      if (at != ndr) return 5;
    } else if (out) {
      return 6;
    }
    pfscdc_index_list_free(out);
    pfscdc_index_list_free(in);
  }
  fclose(jobs);
  if (pfscdc_copy_map_host(NULL, "/a", NULL, "/z", NULL) != PFSCDC_EINVAL) return 7;
  printf("ok\n");
  return 0;
}
