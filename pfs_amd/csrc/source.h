// source.h — the host side of the Source (source.cpp), shared with its device arm
// (source_dev.cpp).  No HIP header: a stand-alone sanitizer build compiles source.cpp with a
// plain C++ compiler.
#pragma once
#include <stdint.h>

#include <cstddef>
#include <string>
#include <vector>

#include "glob.h"
#include "index_list.h"
#include "paths.h"

namespace pfscdc {

// A predicate with its argument cleaned (driver_file.go:173-385), in the one form all four kinds
// share once the list is known to hold clean paths:
//   selected(path) = all || ((path == name || HasPrefix(path, dir)) && !(exclude_dir && path == dir))
// SUBTREE(p) and DIFF(p): name = p, dir = p + "/" (DIFF: never NewErrOnEmpty).  LIST(n): name = n, dir = Clean(n, true), exclude_dir.
// GET(g): name = g, dir = g + "/" (TrimRight(path, "/") == g is path == g or path == g + "/" for a
// clean path, and the `full` filter's dir state, set at g + "/", passes HasPrefix(path, g + "/"):
// stateless, because the inserter puts g + "/" in front of everything below it); g == "/": all.
// GLOB(g) is outside that form: name = g, glob = g parsed, and the predicate is glob_mf (glob.h)
// under the `full` filter; g == "/": all, as GET's.
struct SrcArg {
  int kind = 0;
  std::string name, dir;
  bool all = false, exclude_dir = false, child_flag = false;
  Glob glob;
};
// PFSCDC_EUNSUPPORTED (GET: a glob pattern; GLOB: extglob) / PFSCDC_EINVAL (an unknown kind; GLOB:
// a glob that does not compile) with *err set
int source_arg(int kind, const char* arg, SrcArg* out, std::string* err);
std::string source_not_found(const SrcArg& a);  // NewErrOnEmpty's text
bool source_errs_on_empty(const SrcArg& a);     // whether the RPC wraps its stream in NewErrOnEmpty
void source_host_set_error(const std::string& text);  // what pfscdc_source_host_error returns

// pfscdc_source_host over the internal types; *err names an error, *ndirs (nullable) = the
// directory entries the inserter made that the filter selected
int source_host(const pfscdc_index_list& in, const SrcArg& a, const uint8_t* leaf,
                pfscdc_index_list* out, std::vector<pfscdc_file_info>* infos, std::string* err,
                uint64_t* ndirs);

// BLAKE2b-256, unkeyed (pachhash.New), on the host
struct Blake2b256 {
  uint64_t h[8];
  uint64_t t = 0;
  uint8_t buf[128];
  size_t fill = 0;
  Blake2b256();
  void write(const uint8_t* p, size_t n);
  void sum(uint8_t out[32]);

 private:
  void compress(bool last);
};

}  // namespace pfscdc
