/* Stand-alone driver of pfscdc_index_decode_host for a host sanitizer build: compiled together
 * with pfs_amd/csrc/index_decode.cpp (no GPU library, no HIP header) under
 * -fsanitize=address,undefined.  argv[1]: a file holding one level's stream of pbutil frames.
 * For every k the stream truncated at k, in a heap block of exactly k bytes (so a read at or
 * past k is a heap-buffer-overflow report), must decode to PFSCDC_ECORRUPT or to a clean list
 * no longer than the whole stream's; then the same with every single byte of the whole stream
 * flipped, where any status but a crash is fine.  Prints "ok <full count> <clean prefixes>". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pfscdc.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t* all = (uint8_t*)malloc(n ? (size_t)n : 1);
  if (fread(all, 1, (size_t)n, f) != (size_t)n) return 2;
  fclose(f);
  pfscdc_index_list* l = NULL;
  uint64_t err = 0;
  if (pfscdc_index_decode_host(all, (uint64_t)n, &l, &err) != PFSCDC_OK) return 3;
  const uint32_t full = pfscdc_index_list_count(l);
  pfscdc_index_list_free(l);
  long clean = 0;
  for (long k = 0; k <= n; k++) {
    uint8_t* cut = (uint8_t*)malloc((size_t)k ? (size_t)k : 1);
    memcpy(cut, all, (size_t)k);
    l = NULL;
    const int rc = pfscdc_index_decode_host(k ? cut : NULL, (uint64_t)k, &l, &err);
    if (rc == PFSCDC_OK) {
      if (!l || pfscdc_index_list_count(l) > full) return 4;
      clean++;
      pfscdc_index_list_free(l);
    } else if (rc != PFSCDC_ECORRUPT || l || err > (uint64_t)k) {
      return 5;
    }
    free(cut);
  }
  for (long k = 0; k < n; k++) {
    uint8_t* bad = (uint8_t*)malloc((size_t)n);
    memcpy(bad, all, (size_t)n);
    bad[k] ^= (uint8_t)(0x80u >> (k % 8));
    l = NULL;
    if (pfscdc_index_decode_host(bad, (uint64_t)n, &l, &err) == PFSCDC_OK) pfscdc_index_list_free(l);
    free(bad);
  }
  free(all);
  printf("ok %u %ld\n", full, clean);
  return 0;
}
