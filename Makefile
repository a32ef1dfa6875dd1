# Builds the product library (gfx950) and the oracle/CPU-baseline library.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CXXFLAGS := -O3 -std=c++17 -fPIC -Wall -Wno-unused-result -pthread
SRC := pfs_amd/csrc/cdc_kernels.hip pfs_amd/csrc/pfscdc.cpp pfs_amd/csrc/writer.cpp pfs_amd/csrc/tar.cpp pfs_amd/csrc/index.cpp pfs_amd/csrc/resident.cpp pfs_amd/csrc/index_decode.cpp pfs_amd/csrc/index_merge.cpp pfs_amd/csrc/fileset.cpp pfs_amd/csrc/group.cpp pfs_amd/csrc/gorand.cpp pfs_amd/csrc/knobs.cpp pfs_amd/csrc/glob.cpp pfs_amd/csrc/source.cpp pfs_amd/csrc/source_dev.cpp pfs_amd/csrc/diff.cpp pfs_amd/csrc/diff_dev.cpp pfs_amd/csrc/copy_map.cpp pfs_amd/csrc/copy_map_dev.cpp
HDR := include/pfscdc.h pfs_amd/csrc/pfscdc_internal.h pfs_amd/csrc/index_parse.h pfs_amd/csrc/index_list.h pfs_amd/csrc/dev_list.h pfs_amd/csrc/dev_pass.h pfs_amd/csrc/source.h pfs_amd/csrc/glob.h pfs_amd/csrc/diff.h pfs_amd/csrc/paths.h pfs_amd/csrc/copy_map.h

all: pfs_amd/libpfscdc.so oracle/_build/liboracle.so

pfs_amd/libpfscdc.so: $(SRC) $(HDR)
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -shared -x hip $(filter %.hip %.cpp,$(SRC)) -o $@

oracle/_build/liboracle.so: oracle/cdc_oracle.c oracle/Makefile
	$(MAKE) -C oracle

clean:
	rm -f pfs_amd/libpfscdc.so oracle/_build/liboracle.so

.PHONY: all clean
