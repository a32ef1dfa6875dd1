/* Stand-alone driver of the glob dialect and of pfscdc_source_host with PFSCDC_SRC_GLOB for a host
 * sanitizer build: compiled together with pfs_amd/csrc/glob.cpp, source.cpp and index_decode.cpp
 * (no GPU library, no HIP header) under -fsanitize=address,undefined.  argv[1]: a job file, one
 * job per line:
 *   s\t<stream file>\t<kind>\t<arg>   pfscdc_source_host over one level's pbutil frames ("-": a
 *                                     NULL list): "j <rc>\t<error text>", then per entry
 *                                     "e <path>\t<tag>\t<type>\t<size>\t<hash hex>\t<flags>\t<count>"
 *   m\t<glob>\t<path>                 pfscdc_glob_match: "m <rc>\t<matched>\t<error text>"
 *   p\t<glob>                         pfscdc_debug_glob_program and pfscdc_glob_literal_prefix:
 *                                     "p <rc>\t<positions>\t<accepted by the automaton: the glob's
 *                                     own literal prefix>\t<literal prefix>"
 * and "ok" at the end. */
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

/* the automaton of pfscdc_debug_glob_program over s */
static int accepts(const uint64_t* w, const std::string& s) {
  uint64_t T = w[320];
  int acc = w[322] != 0;
  for (unsigned char c : s) {
    uint64_t S = T & w[64 + c];
    acc = (S & w[321]) != 0;
    T = 0;
    for (int b = 0; b < 64; b++)
      if (S >> b & 1) T |= w[b];
  }
  return acc;
}

static int source_job(char* stream, int kind, const char* arg) {
  pfscdc_index_list* in = strcmp(stream, "-") ? load(stream) : NULL;
  pfscdc_index_list* out = NULL;
  pfscdc_file_info* infos = NULL;
  const int rc = pfscdc_source_host(in, kind, arg, NULL, &out, &infos);
  printf("j %d\t%s\n", rc, pfscdc_source_host_error());
  if (rc == PFSCDC_OK) {
    if (!out || !infos) return 4;
    const pfscdc_index_entry* e = pfscdc_index_list_entries(out);
    uint64_t blen = 0;
    const char* blob = pfscdc_index_list_blob(out, &blen);
    for (uint32_t i = 0; i < pfscdc_index_list_count(out); i++) {
      if (e[i].path_off + e[i].path_len >= blen) return 5;
      char hex[65];
      for (int k = 0; k < 32; k++) snprintf(hex + 2 * k, 3, "%02x", infos[i].hash[k]);
      printf("e %s\t%s\t%u\t%lld\t%s\t%u\t%u\n", blob + e[i].path_off, blob + e[i].tag_off,
             infos[i].type, (long long)infos[i].size, hex, infos[i].flags, e[i].count);
    }
  } else if (out || infos) {
    return 6;
  }
  pfscdc_file_infos_free(infos);
  pfscdc_index_list_free(out);
  pfscdc_index_list_free(in);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* jobs = fopen(argv[1], "rb");
  if (!jobs) return 2;
  char line[4096];
  while (fgets(line, sizeof line, jobs)) {
    size_t len = strlen(line);
    if (len && line[len - 1] == '\n') line[--len] = 0;
    std::vector<char*> f;
    f.push_back(line);
    for (char* p = line; (p = strchr(p, '\t')) != NULL && f.size() < 4;) {
      *p++ = 0;
      f.push_back(p);
    }
    if (line[0] == 's' && f.size() == 4) {
      if (int rc = source_job(f[1], atoi(f[2]), f[3])) return rc;
    } else if (line[0] == 'm' && f.size() == 3) {
      int hit = -1;
      const int rc = pfscdc_glob_match(f[1], f[2], &hit);
      printf("m %d\t%d\t%s\n", rc, hit, rc ? pfscdc_source_host_error() : "");
    } else if (line[0] == 'p' && f.size() == 2) {
      std::vector<uint64_t> w(324);  // exactly 324 words: a write past them reports
      const int rc = pfscdc_debug_glob_program(f[1], w.data());
      std::vector<char> pre(strlen(f[1]) + 2);  // "/" in front at the most
      if (pfscdc_glob_literal_prefix(f[1], pre.data(), pre.size()) != PFSCDC_OK) return 8;
      if (pfscdc_glob_literal_prefix(f[1], pre.data(), strlen(pre.data())) != PFSCDC_EINVAL) return 8;
      printf("p %d\t%llu\t%d\t%s\n", rc, rc ? 0ull : (unsigned long long)w[323],
             rc || w[323] > 64 ? -1 : accepts(w.data(), pre.data()), pre.data());
    } else {
      return 2;
    }
  }
  fclose(jobs);
  int hit = 0;
  if (pfscdc_glob_match(NULL, "/", &hit) != PFSCDC_EINVAL) return 7;
  printf("ok\n");
  return 0;
}
