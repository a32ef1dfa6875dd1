// glob.cpp — the position automaton of a glob (what src_glob_kernel, list_kernels.hip §11, runs),
// globLiteralPrefix, and the C entry points of the dialect.  The parser and the backtracking
// matcher, which is the specification, are in glob.h; nothing here calls the matcher and the
// matcher calls nothing here, so the two are held against each other as independent statements.
// No GPU call and no HIP header.
#include "glob.h"

#include <cstring>

#include "paths.h"
#include "source.h"

namespace pfscdc {

std::string glob_literal_prefix(const std::string& glob) {  // paths.go:12-20
  const size_t k = glob.find_first_of("*?[]{}!()@+^");
  return k == std::string::npos ? glob : glob.substr(0, k);
}

namespace {

// What can come first from term t on, through everything after it: the positions that may take
// the next byte, and whether the end can be reached without one.
struct Entry {
  uint64_t mask = 0;
  bool end = false;
};

struct Compiler {
  const Glob& g;
  std::vector<int> pos;      // term -> its position, -1 for an Alt
  std::vector<Entry> entry;  // term -> Entry, once known
  std::vector<uint8_t> known;

  Entry of(int t) {
    if (t < 0) return Entry{0, true};
    if (known[t]) return entry[t];
    const GlobTerm& x = g.terms[t];
    Entry e;
    switch (x.kind) {
      case GlobTerm::Alt:
        for (int h : x.heads) {
          const Entry a = of(h);
          e.mask |= a.mask;
          e.end = e.end || a.end;
        }
        break;
      case GlobTerm::Star:
      case GlobTerm::Super:  // zero bytes: whatever follows may come first as well
        e = of(x.next);
        e.mask |= 1ull << pos[t];
        break;
      default: e.mask = 1ull << pos[t];
    }
    known[t] = 1;
    return entry[t] = e;
  }
};

}  // namespace

void glob_compile(const Glob& g, GlobProgram* out) {
  out->positions = 0;
  out->nullable = false;
  out->first = out->last = 0;
  std::memset(out->table, 0, sizeof out->table);
  const size_t n = g.terms.size();
  Compiler c{g, std::vector<int>(n, -1), std::vector<Entry>(n), std::vector<uint8_t>(n, 0)};
  for (size_t t = 0; t < n; t++)
    if (g.terms[t].kind != GlobTerm::Alt) c.pos[t] = (int)out->positions++;
  if (out->positions > 64) return;
  for (size_t t = 0; t < n; t++) {
    const GlobTerm& x = g.terms[t];
    if (x.kind == GlobTerm::Alt) continue;
    const int p = c.pos[t];
    const Entry after = c.of(x.next);
    const bool loops = x.kind == GlobTerm::Star || x.kind == GlobTerm::Super;
    out->follow()[p] = after.mask | (loops ? 1ull << p : 0);
    if (after.end) out->last |= 1ull << p;
    for (unsigned b = 0; b < 256; b++) {
      bool takes;
      switch (x.kind) {
        case GlobTerm::Lit: takes = b == x.byte; break;
        case GlobTerm::One:
        case GlobTerm::Star: takes = b != '/'; break;
        case GlobTerm::Super: takes = true; break;
        default: takes = x.cls[b >> 6] >> (b & 63) & 1;
      }
      if (takes) out->accept_byte()[b] |= 1ull << p;
    }
  }
  const Entry e = c.of(g.start);
  out->first = e.mask;
  out->nullable = e.end;
}

}  // namespace pfscdc

extern "C" {

int pfscdc_glob_match(const char* glob, const char* path, int* matched) {
  if (!glob || !path || !matched) return PFSCDC_EINVAL;
  *matched = 0;
  pfscdc::Glob g;
  std::string err;
  if (int rc = pfscdc::glob_parse(pfscdc::clean_path(glob), &g, &err)) {
    pfscdc::source_host_set_error(err);
    return rc;
  }
  *matched = pfscdc::glob_mf(g, path) ? 1 : 0;
  return PFSCDC_OK;
}

int pfscdc_glob_literal_prefix(const char* glob, char* out, size_t cap) {
  if (!glob || !out) return PFSCDC_EINVAL;
  const std::string p = pfscdc::glob_literal_prefix(pfscdc::clean_path(glob));
  if (p.size() + 1 > cap) return PFSCDC_EINVAL;
  std::memcpy(out, p.c_str(), p.size() + 1);
  return PFSCDC_OK;
}

int pfscdc_debug_glob_program(const char* glob, uint64_t out[324]) {
  if (!glob || !out) return PFSCDC_EINVAL;
  pfscdc::Glob g;
  std::string err;
  if (int rc = pfscdc::glob_parse(pfscdc::clean_path(glob), &g, &err)) {
    pfscdc::source_host_set_error(err);
    return rc;
  }
  pfscdc::GlobProgram p;
  pfscdc::glob_compile(g, &p);
  std::memcpy(out, p.table, sizeof p.table);
  out[320] = p.first;
  out[321] = p.last;
  out[322] = p.nullable;
  out[323] = p.positions;
  return PFSCDC_OK;
}

}  // extern "C"
