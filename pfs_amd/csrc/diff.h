// diff.h — the host side of DiffFile (diff.cpp), shared with its device arm (diff_dev.cpp).  No
// HIP header: a stand-alone sanitizer build compiles diff.cpp with a plain C++ compiler.
#pragma once
#include <stdint.h>

#include <vector>

#include "index_list.h"

namespace pfscdc {

// Differ.Iterate (diff.go:26-92) over two sides, each a list with one info per entry (infos may be
// NULL for an empty list): one pair per callback, in callback order.  PFSCDC_EINVAL: entries
// without infos, a path outside its blob.
int diff_host(const pfscdc_index_list& a, const pfscdc_file_info* a_infos,
              const pfscdc_index_list& b, const pfscdc_file_info* b_infos,
              std::vector<pfscdc_diff_pair>* out);

// The entries of side l that occur in pairs (member 0: a, 1: b), in pair order, as a list of
// their own with their infos.
void diff_select(const pfscdc_index_list& l, const pfscdc_file_info* infos,
                 const std::vector<pfscdc_diff_pair>& pairs, int member, pfscdc_index_list* out,
                 std::vector<pfscdc_file_info>* out_infos);

}  // namespace pfscdc
