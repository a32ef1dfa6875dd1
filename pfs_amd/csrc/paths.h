// paths.h — Go's path.Clean and the reference's cleanPath, shared by the Source (source.cpp) and
// CopyFile (copy_map.cpp).  Header only and host only: either file links into a stand-alone
// sanitizer build without the other.
//
// Reference: Go's path.Clean; src/server/pfs/server/paths.go:54-60 cleanPath.
#pragma once
#include <cstddef>
#include <string>

namespace pfscdc {

inline std::string go_clean(const std::string& p) {  // path.Clean
  if (p.empty()) return ".";
  const bool rooted = p[0] == '/';
  const size_t n = p.size();
  std::string out;
  size_t r = 0, dotdot = 0;
  if (rooted) {
    out.push_back('/');
    r = dotdot = 1;
  }
  while (r < n) {
    if (p[r] == '/') {
      r++;
    } else if (p[r] == '.' && (r + 1 == n || p[r + 1] == '/')) {
      r++;
    } else if (p[r] == '.' && r + 1 < n && p[r + 1] == '.' && (r + 2 == n || p[r + 2] == '/')) {
      r += 2;
      if (out.size() > dotdot) {
        size_t w = out.size() - 1;
        while (w > dotdot && out[w] != '/') w--;
        out.resize(w);
      } else if (!rooted) {
        if (!out.empty()) out.push_back('/');
        out += "..";
        dotdot = out.size();
      }
    } else {
      if ((rooted && out.size() != 1) || (!rooted && !out.empty())) out.push_back('/');
      for (; r < n && p[r] != '/'; r++) out.push_back(p[r]);
    }
  }
  return out.empty() ? "." : out;
}

inline std::string trim_slashes(const std::string& p, bool left, bool right) {
  size_t a = 0, b = p.size();
  while (left && a < b && p[a] == '/') a++;
  while (right && b > a && p[b - 1] == '/') b--;
  return p.substr(a, b - a);
}

inline std::string clean_path(const std::string& p0) {  // paths.go:54-60
  const std::string p = go_clean(p0);
  if (p == ".") return "/";
  return "/" + trim_slashes(p, true, true);
}

}  // namespace pfscdc
