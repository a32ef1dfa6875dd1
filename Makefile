# Builds the product library (gfx950) and the oracle/CPU-baseline library.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CXXFLAGS := -O3 -std=c++17 -fPIC -Wall -Wno-unused-result -pthread
# one object per source, JOBS of them at a time (a make that ignores the line builds serially);
# the line also overrides a -j on the command line: JOBS=n is the knob
JOBS ?= 8
MAKEFLAGS += -j$(JOBS)
SRC := $(addprefix pfs_amd/csrc/,cdc_kernels.hip list_kernels.hip pfscdc.cpp writer.cpp tar.cpp \
  index.cpp resident.cpp index_decode.cpp index_merge.cpp fileset.cpp group.cpp gorand.cpp \
  knobs.cpp glob.cpp source.cpp source_dev.cpp diff.cpp diff_dev.cpp copy_map.cpp copy_map_dev.cpp)
HDR := include/pfscdc.h $(addprefix pfs_amd/csrc/,pfscdc_internal.h list_kernels.h index_parse.h \
  index_list.h dev_list.h dev_pass.h source.h glob.h diff.h paths.h copy_map.h tar.h)
OBJ := $(patsubst pfs_amd/csrc/%,build/obj/%.o,$(SRC))

all: pfs_amd/libpfscdc.so oracle/_build/liboracle.so

build/obj/%.o: pfs_amd/csrc/% $(HDR)
	@mkdir -p $(@D)
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -x hip -c $< -o $@

pfs_amd/libpfscdc.so: $(OBJ)
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -shared $(OBJ) -o $@

oracle/_build/liboracle.so: oracle/cdc_oracle.c oracle/Makefile
	$(MAKE) -C oracle

clean:
	rm -rf build/obj
	rm -f pfs_amd/libpfscdc.so oracle/_build/liboracle.so

.PHONY: all clean
