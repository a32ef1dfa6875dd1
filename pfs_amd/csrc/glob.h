// glob.h — the glob dialect of getFile / globFile: the parser and the backtracking matcher, which
// is the specification (header only and host only, like paths.h: source.cpp takes them and still
// links into a stand-alone sanitizer build alone), and the declarations of the position automaton
// the device runs (glob.cpp).
//
// Reference: src/server/pfs/server/paths.go:12-35 globLiteralPrefix / globMatchFunction; the glob
// library itself (ohmyglob, gobwas/glob syntax with separator '/') is not in the reference tree,
// so the dialect is the one DESIGN.md §4 "GlobFile" writes down:
//   *        any run of non-'/' bytes, empty included      **   any run of bytes, empty included
//   ?        one non-'/' byte                              \c   the byte c
//   [...]    one byte of the class, [!...] one byte outside it: single bytes, lo-hi ranges, \c; a
//            '-' that does not stand between two members is itself a member; a class may hold '/'
//   {a,b}    alternatives, nesting, an empty one allowed; ',' outside braces is itself
// A stray ']' or '}', an unterminated '[' or '{', an empty class, a range with hi < lo and a
// trailing '\' are compile errors (PFSCDC_EINVAL, the glob and the byte offset named); an
// unescaped ! ( ) @ + ^ outside a class is extglob (PFSCDC_EUNSUPPORTED, the glob named).  The
// first of these from the left decides.  Matching is bytewise and of the whole string.
#pragma once
#include <stdint.h>

#include <cstddef>
#include <string>
#include <vector>

#include "../../include/pfscdc.h"

namespace pfscdc {

struct GlobTerm {
  enum Kind : uint8_t { Lit, One, Star, Super, Class, Alt };
  Kind kind = Lit;
  uint8_t byte = 0;                    // Lit
  uint64_t cls[4] = {0, 0, 0, 0};      // Class: the bytes it matches (negation applied)
  std::vector<std::vector<int>> alts;  // Alt: each alternative's terms, in order
  int next = -1;                       // the term after this one, through the closing braces; -1: the end
  std::vector<int> heads;              // Alt: each alternative's first term (its own next if empty)
};

struct Glob {
  std::string text;             // the glob as given (cleaned by the caller)
  std::vector<GlobTerm> terms;  // every term; the top sequence is `top`
  std::vector<int> top;
  int start = -1;  // the first term, -1 for the empty glob
};

namespace glob_detail {

struct Parser {
  const std::string& g;
  Glob* out;
  std::string* err;
  size_t at = 0;
  int rc = PFSCDC_OK;

  int fail(int code, const std::string& what, size_t off) {
    if (rc == PFSCDC_OK) {
      rc = code;
      *err = "glob " + g + ": " + what + " at byte " + std::to_string(off);
    }
    return -1;
  }
  int add(GlobTerm t) {
    out->terms.push_back(std::move(t));
    return (int)out->terms.size() - 1;
  }

  int parse_class() {  // g[at] == '['
    const size_t open = at++;
    GlobTerm t;
    t.kind = GlobTerm::Class;
    bool negate = false;
    if (at < g.size() && g[at] == '!') {
      negate = true;
      at++;
    }
    size_t members = 0;
    for (;;) {
      if (at >= g.size()) return fail(PFSCDC_EINVAL, "an unterminated '['", open);
      if (g[at] == ']') {
        at++;
        break;
      }
      auto member = [&](uint8_t* b) {
        if (g[at] == '\\') {
          if (at + 1 >= g.size()) {
            fail(PFSCDC_EINVAL, "a trailing '\\'", at);
            return false;
          }
          at++;
        }
        *b = (uint8_t)g[at++];
        return true;
      };
      uint8_t lo, hi;
      const size_t lo_at = at;
      if (!member(&lo)) return -1;
      hi = lo;
      if (at + 1 < g.size() && g[at] == '-' && g[at + 1] != ']') {
        at++;
        if (!member(&hi)) return -1;
        if (hi < lo) return fail(PFSCDC_EINVAL, "a range whose end is below its start", lo_at);
      }
      for (unsigned b = lo; b <= hi; b++) t.cls[b >> 6] |= 1ull << (b & 63);
      members++;
    }
    if (!members) return fail(PFSCDC_EINVAL, "an empty class", open);
    if (negate)
      for (uint64_t& w : t.cls) w = ~w;
    return add(std::move(t));
  }

  // a sequence up to the end (depth 0) or up to an unescaped ',' or '}' (depth > 0)
  bool parse_seq(int depth, std::vector<int>* seq) {
    while (at < g.size()) {
      const char c = g[at];
      if (depth && (c == ',' || c == '}')) return true;
      GlobTerm t;
      switch (c) {
        case '*':
          if (at + 1 < g.size() && g[at + 1] == '*') {
            t.kind = GlobTerm::Super;
            at += 2;
          } else {
            t.kind = GlobTerm::Star;
            at++;
          }
          seq->push_back(add(std::move(t)));
          break;
        case '?':
          t.kind = GlobTerm::One;
          at++;
          seq->push_back(add(std::move(t)));
          break;
        case '[': {
          const int k = parse_class();
          if (k < 0) return false;
          seq->push_back(k);
          break;
        }
        case '{': {
          const size_t open = at++;
          t.kind = GlobTerm::Alt;
          for (;;) {
            std::vector<int> alt;
            if (!parse_seq(depth + 1, &alt)) return false;
            t.alts.push_back(std::move(alt));
            if (at >= g.size()) {
              fail(PFSCDC_EINVAL, "an unterminated '{'", open);
              return false;
            }
            if (g[at++] == '}') break;
          }
          seq->push_back(add(std::move(t)));
          break;
        }
        case ']':
        case '}':
          fail(PFSCDC_EINVAL, std::string("a stray '") + c + "'", at);
          return false;
        case '!':
        case '(':
        case ')':
        case '@':
        case '+':
        case '^':
          fail(PFSCDC_EUNSUPPORTED, std::string("extglob ('") + c + "') is not built", at);
          return false;
        case '\\':
          if (at + 1 >= g.size()) {
            fail(PFSCDC_EINVAL, "a trailing '\\'", at);
            return false;
          }
          at++;
          [[fallthrough]];
        default:
          t.kind = GlobTerm::Lit;
          t.byte = (uint8_t)g[at++];
          seq->push_back(add(std::move(t)));
      }
    }
    return true;
  }

  // next and heads: the first term of seq followed by cont (cont itself if seq is empty)
  int link(const std::vector<int>& seq, int cont) {
    for (size_t i = seq.size(); i-- > 0;) {
      GlobTerm& t = out->terms[seq[i]];
      t.next = cont;
      if (t.kind == GlobTerm::Alt) {
        t.heads.clear();
        const std::vector<std::vector<int>> alts = t.alts;  // (link may not hold t across calls)
        std::vector<int> heads;
        for (const std::vector<int>& a : alts) heads.push_back(link(a, cont));
        out->terms[seq[i]].heads = std::move(heads);
      }
      cont = seq[i];
    }
    return cont;
  }
};

struct Matcher {
  const Glob& g;
  const uint8_t* s;
  size_t n;
  std::vector<uint8_t> memo;  // (term, position): 0 not tried, 1 matches, 2 does not

  bool from(int t, size_t pos) {  // s[pos, n) matches term t and everything after it
    if (t < 0) return pos == n;
    const size_t key = (size_t)t * (n + 1) + pos;
    if (memo[key]) return memo[key] == 1;
    const GlobTerm& x = g.terms[t];
    bool ok = false;
    switch (x.kind) {
      case GlobTerm::Lit: ok = pos < n && s[pos] == x.byte && from(x.next, pos + 1); break;
      case GlobTerm::One: ok = pos < n && s[pos] != '/' && from(x.next, pos + 1); break;
      case GlobTerm::Class:
        ok = pos < n && (x.cls[s[pos] >> 6] >> (s[pos] & 63) & 1) && from(x.next, pos + 1);
        break;
      case GlobTerm::Star:
        for (size_t k = pos; !ok; k++) {
          ok = from(x.next, k);
          if (k >= n || s[k] == '/') break;
        }
        break;
      case GlobTerm::Super:
        for (size_t k = pos; !ok && k <= n; k++) ok = from(x.next, k);
        break;
      case GlobTerm::Alt:
        for (size_t a = 0; !ok && a < x.heads.size(); a++) ok = from(x.heads[a], pos);
        break;
    }
    memo[key] = ok ? 1 : 2;
    return ok;
  }
};

}  // namespace glob_detail

// The glob (cleaned already) as an AST.  PFSCDC_EINVAL / PFSCDC_EUNSUPPORTED with *err set.
inline int glob_parse(const std::string& glob, Glob* out, std::string* err) {
  *out = Glob();
  out->text = glob;
  glob_detail::Parser p{glob, out, err};
  if (!p.parse_seq(0, &out->top)) return p.rc;
  out->start = p.link(out->top, -1);
  return PFSCDC_OK;
}

// Match(glob, s[0, n)): the backtracking matcher, memoised on (term, position)
inline bool glob_match(const Glob& g, const char* s, size_t n) {
  glob_detail::Matcher m{g, (const uint8_t*)s, n, {}};
  m.memo.assign(g.terms.size() * (n + 1), 0);
  return m.from(g.start, 0);
}

// globMatchFunction's closure: (path == "/" && glob == "/") || Match(glob, TrimRight(path, "/"))
inline bool glob_mf(const Glob& g, const std::string& path) {
  if (path == "/" && g.text == "/") return true;
  size_t n = path.size();
  while (n && path[n - 1] == '/') n--;
  return glob_match(g, path.data(), n);
}

// globLiteralPrefix: the glob up to globRegex's first hit, one of * ? [ ] { } ! ( ) @ + ^
std::string glob_literal_prefix(const std::string& glob);

// The position (Glushkov) automaton of a glob: one position per byte-consuming term, '*' and '**'
// one position with a self loop each.  A string is accepted iff, with T = first and acc =
// nullable before its first byte and, per byte c, S = T & accept_byte[c], acc = (S & last) != 0,
// T = OR of follow[b] over the bits b of S, acc holds after its last byte.
struct GlobProgram {
  uint32_t positions = 0;  // more than 64: no program (the arrays are left zero)
  bool nullable = false;
  uint64_t first = 0, last = 0;
  uint64_t table[64 + 256];  // follow[64], then accept_byte[256]: what the device stages, 2.5 KiB
  uint64_t* follow() { return table; }
  uint64_t* accept_byte() { return table + 64; }
};
void glob_compile(const Glob& g, GlobProgram* out);

}  // namespace pfscdc
