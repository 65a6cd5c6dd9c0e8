# Builds the product library helyim_amd/libhec.so (gfx950) and the test
# oracle oracle/build/liboracle.so. `make -j8`.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-result
SRC := $(wildcard helyim_amd/csrc/*.cpp) $(wildcard helyim_amd/csrc/*.hip)
HDR := $(wildcard helyim_amd/csrc/*.hpp) $(wildcard helyim_amd/csrc/*.inc) include/hec.h
OBJ := $(patsubst helyim_amd/csrc/%,build/obj/%.o,$(SRC))

all: helyim_amd/libhec.so oracle build/cabi_bench build/membench_calib build/variants/libhec_smallgrid.so

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

# Kernel variants: rs_kernels.hip rebuilt with other flags and linked with the
# product's other objects into a library of its own (HEC_LIB_PATH loads one).
#  * null: a byte-identical rebuild, to measure the spread of
#    alternating-process A/Bs between two library builds (tools/tune.py).
#  * smallgrid: tiny launch limits, so the GPU suites' small batches go in
#    several stripe ranges, grid-stride iterations and mask rounds
#    (tests/test_gpu_small_grid.py). 100 is no multiple of 8, 3 or 5; 4
#    workgroups make the mask kernels go round after 1024 stripes. Part of
#    `all`: the tests need it.
VARIANTS := null smallgrid
VFLAGS_null := -DHEC_NULL_VARIANT=1
VFLAGS_smallgrid := -DHEC_MAX_LAUNCH_BLOCKS=100 -DHEC_LOCATE_MAX_BLOCKS=4
VOBJ := $(filter-out build/obj/rs_kernels.hip.o,$(OBJ))
variants: $(foreach v,$(VARIANTS),build/variants/libhec_$(v).so)
build/variants/libhec_%.so: $(SRC) $(HDR) $(VOBJ)
	@mkdir -p build/variants/$*
	$(HIPCC) $(HIPFLAGS) $(VFLAGS_$*) -c helyim_amd/csrc/rs_kernels.hip -o build/variants/$*/rs_kernels.o
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ build/variants/$*/rs_kernels.o $(VOBJ) -lpthread

clean:
	rm -rf build helyim_amd/libhec.so
	$(MAKE) -C oracle clean

.PHONY: all oracle clean variants
