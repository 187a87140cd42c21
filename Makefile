# Builds the product library (HIP for gfx950 + host C) and the test-only oracle.
#   make            -> uvhttp_amd/lib/libuvhttp_ws_amd.so  +  oracle/_build/libws_oracle.so
ROCM ?= /opt/rocm
HIPCC ?= $(ROCM)/bin/hipcc
CC ?= gcc
ARCH ?= gfx950
BUILD := uvhttp_amd/build
LIB := uvhttp_amd/lib/libuvhttp_ws_amd.so
# the same library built with -DUVWS_TEST_HOOKS -DUVWS_EXPERIMENTS (tests and A/B tools only):
# the batcher's fault-injection hook and the environment switches (UVHTTP_WS_*): most force a
# path the product takes on its own for some input (walk kind, fused / speculative ranges,
# poll bound, ...), so tests and measurements reach it at a small shape; REC_SCAN, PLAN_WIDE,
# WALK_FUSE and DESC_EMIT=1 (in place) select measured variants the GPU suite still runs against the
# oracle.  The product library reads no environment.
TESTLIB := uvhttp_amd/lib/libuvhttp_ws_amd_testhooks.so
# reads the switches above (experiment_knobs in ws_gpu.hip and their like in the other sources)
EXP := -DUVWS_EXPERIMENTS

HIPFLAGS := --offload-arch=$(ARCH) -O3 -fPIC -std=c++17 -Iinclude -Wall -Werror \
            -mcode-object-version=5
CFLAGS := -O2 -DNDEBUG -fPIC -std=gnu11 -Iinclude -Wall -Wextra -Werror

all: $(LIB) $(TESTLIB) oracle ctests probes

DEVICE_GUARD := uvhttp_amd/csrc/device_guard.h
ENGINE_INT := uvhttp_amd/csrc/ws_engine_int.h $(DEVICE_GUARD)
UTF8_RULES := uvhttp_amd/csrc/utf8_rules.h

$(BUILD)/ws_gpu.o: uvhttp_amd/csrc/ws_gpu.hip include/uvhttp_ws_amd.h $(ENGINE_INT)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

# the stages after a decode (UTF-8 of messages and of frames, control replies, echo / relay /
# answers, the server's CLOSE frames, fail points): no environment switches, so one object each
# serves both libraries
STAGES := utf8_gpu utf8_frames_gpu ws_replies_gpu ws_echo_gpu ws_close_gpu ws_fail_gpu
STAGE_OBJS := $(STAGES:%=$(BUILD)/%.o)
WS_SCAN := uvhttp_amd/csrc/ws_scan.h

$(STAGE_OBJS): $(BUILD)/%.o: uvhttp_amd/csrc/%.hip include/uvhttp_ws_amd.h $(ENGINE_INT) $(WS_SCAN)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(BUILD)/utf8_gpu.o $(BUILD)/utf8_frames_gpu.o: $(UTF8_RULES)

$(BUILD)/tls_gpu.o: uvhttp_amd/csrc/tls_gpu.hip include/uvhttp_tls_amd.h $(DEVICE_GUARD)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(BUILD)/ws_batcher.o: uvhttp_amd/csrc/ws_batcher.hip include/uvhttp_ws_amd.h
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(BUILD)/ws_batcher_testhooks.o: uvhttp_amd/csrc/ws_batcher.hip include/uvhttp_ws_amd.h
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DUVWS_TEST_HOOKS $(EXP) -c -o $@ $<

$(BUILD)/ws_gpu_exp.o: uvhttp_amd/csrc/ws_gpu.hip include/uvhttp_ws_amd.h $(ENGINE_INT)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(EXP) -c -o $@ $<

$(BUILD)/tls_gpu_exp.o: uvhttp_amd/csrc/tls_gpu.hip include/uvhttp_tls_amd.h $(DEVICE_GUARD)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(EXP) -c -o $@ $<

$(BUILD)/ws_host_exp.o: uvhttp_amd/csrc/ws_host.c include/uvhttp_ws_amd.h $(UTF8_RULES)
	@mkdir -p $(BUILD)
	$(CC) $(CFLAGS) $(EXP) -c -o $@ $<

$(BUILD)/ws_host.o: uvhttp_amd/csrc/ws_host.c include/uvhttp_ws_amd.h $(UTF8_RULES)
	@mkdir -p $(BUILD)
	$(CC) $(CFLAGS) -c -o $@ $<

# host-only C++ (the multi-GPU batcher group): no device code, no HIP headers
$(BUILD)/ws_batcher_group.o: uvhttp_amd/csrc/ws_batcher_group.cpp include/uvhttp_ws_amd.h
	@mkdir -p $(BUILD)
	$(CXX) -O2 -fPIC -std=c++17 -Iinclude -Wall -Wextra -Werror -c -o $@ $<

$(LIB): $(BUILD)/ws_gpu.o $(STAGE_OBJS) $(BUILD)/tls_gpu.o $(BUILD)/ws_batcher.o $(BUILD)/ws_host.o \
        $(BUILD)/ws_batcher_group.o
	@mkdir -p $(dir $@)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

$(TESTLIB): $(BUILD)/ws_gpu_exp.o $(STAGE_OBJS) $(BUILD)/tls_gpu_exp.o $(BUILD)/ws_batcher_testhooks.o $(BUILD)/ws_host_exp.o \
            $(BUILD)/ws_batcher_group.o
	@mkdir -p $(dir $@)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

oracle:
	$(MAKE) -C oracle

# test programs: the C1 libuv echo harness (against the product library) and the
# ASan/UBSan builds of the host decoder + oracle (tests/c/Makefile)
ctests: $(LIB) oracle tests/c/_build/close_check tests/c/_build/fail_check tests/c/_build/answer_check
	$(MAKE) -C tests/c

# ws_host.c's close frames, fail points and answers under ASan/UBSan, each in a program of its
# own (tests/c/NAME_check.c, run by tests/test_close_frames_host.py, test_fail_points_host.py and
# test_answer_host.py)
tests/c/_build/%_check: tests/c/%_check.c uvhttp_amd/csrc/ws_host.c include/uvhttp_ws_amd.h
	@mkdir -p tests/c/_build
	$(CC) -std=gnu11 -Wall -Wextra -Werror -Iinclude -O1 -g -fno-omit-frame-pointer \
	  -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ $< uvhttp_amd/csrc/ws_host.c

# measurement tools run on the GPU box (PCIe ceilings beside the live-shape e2e)
probes: tools/bin/pcie_probe tools/bin/copy_probe

tools/bin/pcie_probe: tools/pcie_probe.hip
	@mkdir -p tools/bin
	$(HIPCC) --offload-arch=$(ARCH) -O2 -o $@ $<

# host-only (HIP runtime API, no kernels): g++, so the AVX variants can use target attributes
tools/bin/copy_probe: tools/copy_probe.cpp $(BUILD)/ws_host.o
	@mkdir -p tools/bin
	g++ -O2 -std=c++17 -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -Iinclude -o $@ $^ -L$(ROCM)/lib -lamdhip64 -Wl,-rpath,$(ROCM)/lib

asm:
	@mkdir -p $(BUILD)
	set -e; for f in ws_gpu tls_gpu $(STAGES); do \
	  $(HIPCC) $(HIPFLAGS) -Wno-unused-command-line-argument --cuda-device-only -S -o $(BUILD)/$$f.s uvhttp_amd/csrc/$$f.hip; \
	done

clean:
	rm -rf $(BUILD) uvhttp_amd/lib
	$(MAKE) -C oracle clean
	$(MAKE) -C tests/c clean

.PHONY: all oracle ctests probes clean asm
