// copy_map.h — the host side of CopyFile's selection and path transform (copy_map.cpp), shared
// with its device arm (copy_map_dev.cpp).  No HIP header: a stand-alone sanitizer build compiles
// copy_map.cpp with a plain C++ compiler.
#pragma once
#include <stdint.h>

#include <string>

#include "index_list.h"
#include "paths.h"

namespace pfscdc {

// copyFile's arguments as the driver forms them (driver_file.go:149-150, 158)
struct CopyArg {
  std::string src, dst, tag;  // cleanPath(src), cleanPath(dst), src.Tag ("" selects every tag)
};
CopyArg copy_arg(const char* src, const char* src_tag, const char* dst);

// pfscdc_copy_map_host over the internal types; *err names an error
int copy_map_host(const pfscdc_index_list& in, const CopyArg& a, pfscdc_index_list* out,
                  std::string* err);

}  // namespace pfscdc
