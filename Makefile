# Builds the product library helyim_amd/libhec.so (gfx950) and the test
# oracle oracle/build/liboracle.so. `make -j8`.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-result
SRC := $(wildcard helyim_amd/csrc/*.cpp) $(wildcard helyim_amd/csrc/*.hip)
HDR := $(wildcard helyim_amd/csrc/*.hpp) $(wildcard helyim_amd/csrc/*.inc) include/hec.h
OBJ := $(patsubst helyim_amd/csrc/%,build/obj/%.o,$(SRC))

all: helyim_amd/libhec.so oracle build/cabi_bench build/membench_calib build/variants/libhec_smallgrid.so \
    build/variants/libhec_smallchunk.so

helyim_amd/libhec.so: $(OBJ)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $(OBJ) -lpthread

build/obj/%.hip.o: helyim_amd/csrc/%.hip $(HDR)
	@mkdir -p build/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

build/obj/%.cpp.o: helyim_amd/csrc/%.cpp $(HDR)
	@mkdir -p build/obj
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

oracle:
	$(MAKE) -C oracle

# The BASELINE workload through the C ABI alone (no Python / PyTorch).
build/cabi_bench: tools/cabi_bench.cpp include/hec.h helyim_amd/libhec.so
	@mkdir -p build
	$(HIPCC) -O2 -std=c++17 -Wall -o $@ $< -Lhelyim_amd -lhec -Wl,-rpath,'$$ORIGIN/../helyim_amd'

# FETCH_SIZE / WRITE_SIZE calibration streams + the shipped kernels in one
# process (tools/membench.hip calib; profiles/pmc_traffic.json "calibration").
build/membench_calib: tools/membench.hip include/hec.h helyim_amd/libhec.so
	@mkdir -p build
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) -DMEMBENCH_WITH_HEC -o $@ $< -Lhelyim_amd -lhec \
	    -Wl,-rpath,'$$ORIGIN/../helyim_amd'

# Variants: the sources VSRC_<v> names rebuilt with VFLAGS_<v> and linked with
# the product's other objects into a library of its own (HEC_LIB_PATH loads
# one).
#  * null: a byte-identical rebuild, to measure the spread of
#    alternating-process A/Bs between two library builds (tools/tune.py).
#  * smallgrid: tiny launch limits, so the GPU suites' small batches go in
#    several stripe ranges, grid-stride iterations and mask rounds
#    (tests/test_gpu_small_grid.py). 100 is no multiple of 8, 3 or 5; 4
#    workgroups make the mask kernels go round after 1024 stripes. Part of
#    `all`: the tests need it.
#  * smallchunk: tiny chunks in the host layer's staging loops, so the host
#    and file suites' small batches and volumes go in many chunks through
#    every reusable slot and stream (tests/test_gpu_small_chunk.py); the
#    kernels are the product's own object. 48 KiB a host chunk: 3 stripes of
#    14 x 1000 bytes (64 stripes: 21 chunks and one of 1), 5 of RS(6,3)'s, one
#    stripe of anything from 2048 bytes up, while 9 stripes of 17 bytes stay in
#    one chunk of 13. 12 KiB of columns a scrub chunk: 3 of the tests' 4096-byte
#    blocks, no power of two. 5000 bytes a pread: no multiple of 256, so a
#    chunk's row is read in three pieces, the last ragged. The module's CPU
#    tests pin these conditions. Part of `all`: the tests need it.
VARIANTS := null smallgrid smallchunk
VFLAGS_null := -DHEC_NULL_VARIANT=1
VSRC_null := rs_kernels.hip
VFLAGS_smallgrid := -DHEC_MAX_LAUNCH_BLOCKS=100 -DHEC_LOCATE_MAX_BLOCKS=4
VSRC_smallgrid := rs_kernels.hip rs_update_ragged.hip
VFLAGS_smallchunk := -DHEC_HOST_CHUNK_BYTES=49152 -DHEC_SCRUB_CHUNK_COLS=12288 -DHEC_SCRUB_READ_PIECE=5000
VSRC_smallchunk := host_pipeline.cpp verify_files.cpp
variants: $(foreach v,$(VARIANTS),build/variants/libhec_$(v).so)
define VARIANT_RULES
build/variants/$(1)/%.o: helyim_amd/csrc/%.hip $$(HDR)
	@mkdir -p build/variants/$(1)
	$$(HIPCC) $$(HIPFLAGS) $$(VFLAGS_$(1)) -c $$< -o $$@
build/variants/$(1)/%.o: helyim_amd/csrc/%.cpp $$(HDR)
	@mkdir -p build/variants/$(1)
	$$(HIPCC) $$(HIPFLAGS) $$(VFLAGS_$(1)) -x hip -c $$< -o $$@
build/variants/libhec_$(1).so: $$(patsubst %,build/variants/$(1)/%.o,$$(basename $$(VSRC_$(1)))) \
    $$(filter-out $$(patsubst %,build/obj/%.o,$$(VSRC_$(1))),$$(OBJ))
	$$(HIPCC) -shared -fPIC --offload-arch=$$(ARCH) -o $$@ $$^ -lpthread
endef
$(foreach v,$(VARIANTS),$(eval $(call VARIANT_RULES,$(v))))

clean:
	rm -rf build helyim_amd/libhec.so
	$(MAKE) -C oracle clean

.PHONY: all oracle clean variants
