/* Stand-alone driver of pfscdc_diff_host for a host sanitizer build: compiled together with
 * pfs_amd/csrc/diff.cpp and index_decode.cpp (no GPU library, no HIP header) under
 * -fsanitize=address,undefined.  argv[1]: a job file, one job per line:
 *   <stream a>\t<hashes a>\t<stream b>\t<hashes b>
 * a stream file holding one level's pbutil frames and a hash file 32 bytes per entry of it ("-"
 * for both: a NULL side).  Per job it prints "j <rc> <pairs>", then per pair "p <a> <b>" with
 * "-" for PFSCDC_DIFF_NONE, and "ok" at the end. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pfscdc.h"

static std::vector<uint8_t> slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) exit(2);
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<uint8_t> all((size_t)n);  // exactly n bytes: a read past them reports
  if (n && fread(all.data(), 1, (size_t)n, f) != (size_t)n) exit(2);
  fclose(f);
  return all;
}

struct Side {
  pfscdc_index_list* l = NULL;
  std::vector<pfscdc_file_info> infos;  // exactly one per entry
};

static void load(const char* stream, const char* hashes, Side* s) {
  if (!strcmp(stream, "-")) return;
  const std::vector<uint8_t> bytes = slurp(stream), h = slurp(hashes);
  if (pfscdc_index_decode_host(bytes.data(), bytes.size(), &s->l, NULL) != PFSCDC_OK) exit(3);
  const uint32_t n = pfscdc_index_list_count(s->l);
  if (h.size() != 32 * (size_t)n) exit(3);
  s->infos.resize(n);
  for (uint32_t i = 0; i < n; i++) {
    memset(&s->infos[i], 0, sizeof(pfscdc_file_info));
    memcpy(s->infos[i].hash, h.data() + 32 * (size_t)i, 32);
    s->infos[i].type = PFSCDC_FILE_TYPE_FILE;
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* jobs = fopen(argv[1], "rb");
  if (!jobs) return 2;
  char line[8192];
  while (fgets(line, sizeof line, jobs)) {
    size_t len = strlen(line);
    if (len && line[len - 1] == '\n') line[--len] = 0;
    char* t1 = strchr(line, '\t');
    char* t2 = t1 ? strchr(t1 + 1, '\t') : NULL;
    char* t3 = t2 ? strchr(t2 + 1, '\t') : NULL;
    if (!t3) return 2;
    *t1 = *t2 = *t3 = 0;
    Side a, b;
    load(line, t1 + 1, &a);
    load(t2 + 1, t3 + 1, &b);
    pfscdc_diff_pair* pairs = NULL;
    uint64_t n = 0;
    const int rc = pfscdc_diff_host(a.l, a.infos.empty() ? NULL : a.infos.data(), b.l,
                                    b.infos.empty() ? NULL : b.infos.data(), &pairs, &n);
    printf("j %d %llu\n", rc, (unsigned long long)n);
    if (rc == PFSCDC_OK) {
      if (!pairs) return 4;
      for (uint64_t k = 0; k < n; k++) {
        char x[16], y[16];
        snprintf(x, sizeof x, "%u", pairs[k].a);
        snprintf(y, sizeof y, "%u", pairs[k].b);
        printf("p %s %s\n", pairs[k].a == PFSCDC_DIFF_NONE ? "-" : x,
               pairs[k].b == PFSCDC_DIFF_NONE ? "-" : y);
      }
    } else if (pairs) {
      return 6;
    }
    pfscdc_diff_pairs_free(pairs);
    pfscdc_index_list_free(a.l);
    pfscdc_index_list_free(b.l);
  }
  fclose(jobs);
  if (pfscdc_diff_host(NULL, NULL, NULL, NULL, NULL, NULL) != PFSCDC_EINVAL) return 7;
  printf("ok\n");
  return 0;
}
