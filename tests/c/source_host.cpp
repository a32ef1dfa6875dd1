/* Stand-alone driver of pfscdc_source_host for a host sanitizer build: compiled together with
 * pfs_amd/csrc/source.cpp and index_decode.cpp (no GPU library, no HIP header) under
 * -fsanitize=address,undefined.  argv[1]: a job file, one job per line:
 *   <stream file>\t<kind>\t<leaf: 0 or 1>\t<arg>
 * the stream file holding one level's pbutil frames ("-": a NULL list).  With leaf 1 the call
 * gets leaf hashes, byte k of entry i being (7 i + 3 k + 1) & 0xff.  Per job it prints
 * "j <rc>\t<error text>", then per entry
 *   "e <path>\t<tag>\t<type>\t<size>\t<hash hex>\t<flags>\t<first>\t<count>", and "ok" at the end. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

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
    const int kind = atoi(t1 + 1);
    const uint32_t n = pfscdc_index_list_count(in);
    std::vector<uint8_t> leaf;
    if (atoi(t2 + 1)) {
      leaf.resize(32 * (size_t)n + 1);
      for (uint32_t i = 0; i < n; i++)
        for (uint32_t k = 0; k < 32; k++) leaf[32 * (size_t)i + k] = (uint8_t)(7 * i + 3 * k + 1);
    }
    pfscdc_index_list* out = NULL;
    pfscdc_file_info* infos = NULL;
    const int rc = pfscdc_source_host(in, kind, t3 + 1, leaf.empty() ? NULL : leaf.data(), &out, &infos);
    printf("j %d\t%s\n", rc, pfscdc_source_host_error());
    if (rc == PFSCDC_OK) {
      if (!out || !infos) return 4;
      const pfscdc_index_entry* e = pfscdc_index_list_entries(out);
      uint64_t blen = 0;
      const char* blob = pfscdc_index_list_blob(out, &blen);
      uint32_t ndr = 0, at = 0;
      (void)pfscdc_index_list_datarefs(out, &ndr);
      for (uint32_t i = 0; i < pfscdc_index_list_count(out); i++) {
        if (e[i].first != at || e[i].path_off + e[i].path_len >= blen) return 5;
        at += e[i].count;
        char hex[65];
        for (int k = 0; k < 32; k++) snprintf(hex + 2 * k, 3, "%02x", infos[i].hash[k]);
        printf("e %s\t%s\t%u\t%lld\t%s\t%u\t%u\t%u\n", blob + e[i].path_off, blob + e[i].tag_off,
               infos[i].type, (long long)infos[i].size, hex, infos[i].flags, e[i].first, e[i].count);
      }
      if (at != ndr) return 5;
    } else if (out || infos) {
      return 6;
    }
    pfscdc_file_infos_free(infos);
    pfscdc_index_list_free(out);
    pfscdc_index_list_free(in);
  }
  fclose(jobs);
  if (pfscdc_source_host(NULL, PFSCDC_SRC_ALL, NULL, NULL, NULL, NULL) != PFSCDC_EINVAL) return 7;
  printf("ok\n");
  return 0;
}
