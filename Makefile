# Builds dgppo_fov_amd/lib/libdgppo_hip.so for gfx950 (MI355X).  `make -j16`: one object per csrc/*.hip (env_step.hip,
# about 2.5 minutes, is the longest).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CSRC := dgppo_fov_amd/csrc
OUT := dgppo_fov_amd/lib
OBJ := dgppo_fov_amd/_build
SRCS := $(wildcard $(CSRC)/*.hip)
OBJS := $(patsubst $(CSRC)/%.hip,$(OBJ)/%.o,$(SRCS))
HDRS := $(wildcard $(CSRC)/*.h) include/dgppo_hip.h
# env kernels must not contract a*b+c into FMA (bit parity with the NumPy oracle): env_step.hip, math32.h and
# noise.h carry `#pragma clang fp contract(off)`; the network kernels keep the default (FMA).
HIPFLAGS := --offload-arch=$(ARCH) -O3 -fPIC -std=c++17 -Wall -Iinclude

all: $(OUT)/libdgppo_hip.so

$(OBJ)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OUT)/libdgppo_hip.so: $(OBJS)
	@mkdir -p $(OUT)
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $(OBJS)

clean:
	rm -rf $(OBJ) $(OUT)/libdgppo_hip.so

# Diagnostic libraries (DGPPO_HIP_LIB points at one): $(call diag_lib,NAME,FLAGS,UNITS) makes target NAME, which
# recompiles UNITS with FLAGS into _build/UNIT_NAME.o and links them with every other in-tree object into
# lib/libdgppo_hip_NAME.so.
define diag_lib
$(1)_OBJS := $$(filter-out $$(patsubst %,$(OBJ)/%.o,$(3)),$$(OBJS)) $$(patsubst %,$(OBJ)/%_$(1).o,$(3))
$(OBJ)/%_$(1).o: $(CSRC)/%.hip $$(HDRS)
	@mkdir -p $(OBJ)
	$$(HIPCC) $$(HIPFLAGS) $(2) -c $$< -o $$@
$(1): $$($(1)_OBJS)
	@mkdir -p $(OUT)
	$$(HIPCC) --offload-arch=$$(ARCH) -shared -o $(OUT)/libdgppo_hip_$(1).so $$($(1)_OBJS)
.PHONY: $(1)
endef

# the env kernels' phase timers: block step (scripts/block_stamps.py) and persistent wave rollout (scripts/env_stamps.py)
$(eval $(call diag_lib,stamps,-DDGPPO_ENV_STAMPS,env_step))
# every env-graph store dropped from the wave kernels (timing experiments only)
$(eval $(call diag_lib,nostore,-DDGPPO_DIAG_NOSTORE,env_step))
# the fused policy step's phase timestamps (scripts/policy_probe.py)
$(eval $(call diag_lib,probe,-DPOLICY_PROBE,policy))
# register-form policy step at 4 waves per SIMD instead of the default 3 (A/B against the in-tree library)
$(eval $(call diag_lib,w4,-DPOLICY_REG_WAVES=4,policy))

.PHONY: all clean
