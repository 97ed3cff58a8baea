# TEST-ONLY: the two builds of tests/device_math_harness.hip (see its header) with the product's flags (icicle_amd/csrc/Makefile):
# as shipped, and with -DBIGFIELD_NO_ASM. Run from the repository root or anywhere: make -f tests/device_math.mk -j2
HERE  := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC  := $(HERE)../icicle_amd/csrc
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
OUT   := $(HERE)_build
FLAGS := -std=c++17 -O3 -fPIC --offload-arch=$(ARCH) -Wno-unused-result -Wno-pass-failed -fvisibility=hidden -shared
DEPS  := $(HERE)device_math_harness.hip $(HERE)math_cases.hpp $(addprefix $(CSRC)/,bigfield.hpp mont_asm.hpp fq2.hpp ec.hpp ec_dbl_quad.hpp goldfield.hpp smallfield.hpp field_consts.h)

all: $(OUT)/libdevice_math_asm.so $(OUT)/libdevice_math_noasm.so

$(OUT)/libdevice_math_asm.so: $(DEPS)
	@mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) $< -o $@.tmp && mv $@.tmp $@

$(OUT)/libdevice_math_noasm.so: $(DEPS)
	@mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) -DBIGFIELD_NO_ASM $< -o $@.tmp && mv $@.tmp $@

.PHONY: all
