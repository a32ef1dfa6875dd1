// tar_pax_host.cpp — the host side of GetFileTAR's PAX entries (tar.cpp alone, no GPU library)
// for a sanitizer build: per job line "<name in hex> <size>" the head under PFSCDC_TAR_USTAR and
// under PFSCDC_TAR_USTAR | PFSCDC_TAR_PAX, each into a heap buffer of exactly its length, as
// "<rc> <head in hex>"; then the layout of the jobs whose PAX head exists, under both formats, as
// "<rc> <total> <offsets...>"; then "ok".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "pfscdc.h"

static std::string unhex(const std::string& h) {
  std::string out;
  for (size_t i = 0; i + 1 < h.size(); i += 2)
    out.push_back((char)std::strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return out;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::vector<std::string> names;
  std::vector<uint64_t> sizes;
  std::string hex;
  unsigned long long size;
  while (in >> hex >> size) {
    const std::string name = unhex(hex);
    bool keep = false;
    for (int format : {PFSCDC_TAR_USTAR, PFSCDC_TAR_USTAR | PFSCDC_TAR_PAX}) {
      uint64_t len = 0;
      int rc = pfscdc_tar_head(name.c_str(), size, format, nullptr, 0, &len);
      std::string out;
      if (rc == PFSCDC_OK) {
        std::vector<uint8_t> buf(len);  // exactly as long: a byte past it is the sanitizer's
        rc = pfscdc_tar_head(name.c_str(), size, format, buf.data(), len, &len);
        static const char* digits = "0123456789abcdef";
        for (uint8_t b : buf) {
          out.push_back(digits[b >> 4]);
          out.push_back(digits[b & 15]);
        }
        keep = format != PFSCDC_TAR_USTAR;
      }
      std::printf("%d %s\n", rc, out.c_str());
    }
    if (keep) {
      names.push_back(name);
      sizes.push_back(size);
    }
  }
  std::vector<pfscdc_tar_file> files(names.size());
  for (size_t i = 0; i < names.size(); i++)
    files[i] = pfscdc_tar_file{names[i].c_str(), (uint32_t)i, sizes[i] ? 1u : 0u};
  for (int format : {PFSCDC_TAR_USTAR, PFSCDC_TAR_USTAR | PFSCDC_TAR_PAX}) {
    std::vector<uint64_t> offs(names.size() + 1);
    uint64_t total = 0;
    const int rc = pfscdc_tar_layout_format(files.data(), (uint32_t)files.size(), sizes.data(),
                                            format, offs.data(), &total);
    std::printf("%d", rc);
    if (rc == PFSCDC_OK) {
      std::printf(" %llu", (unsigned long long)total);
      for (uint64_t o : offs) std::printf(" %llu", (unsigned long long)o);
    }
    std::printf("\n");
  }
  std::printf("ok\n");
  return 0;
}
