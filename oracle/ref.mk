# TEST INFRASTRUCTURE: builds the reference's own WebSocket unit into _ref/libws_ref.so, so that
# tests can run it beside the restatement in ws_oracle.c (tests/test_reference_diff.py, and the
# maker of tests/golden/reference_transcripts.json).
#
# The compiler reads the reference where it lies, $(REFERENCE_DIR): its src/uvhttp_websocket.c by
# path and its include/ by -I.  Nothing of it is copied here.  What it needs beyond its own tree
# and the system's uv.h are the third-party names in ref_stub/ (empty headers plus
# ref_third_party.h, forced into each compile) and the symbols ref_driver.c defines.
#
# Without a reference tree (a GPU machine, a clean checkout elsewhere) the target does nothing and
# succeeds: the committed fixture and tests/test_reference_transcripts_host.py guard that case.
REFERENCE_DIR ?= /root/reference
REF_SRC := $(REFERENCE_DIR)/src/uvhttp_websocket.c
REF_INC := -include ref_stub/ref_third_party.h -Iref_stub -I$(REFERENCE_DIR)/include
# the feature and platform definitions of the reference's default 64-bit build
REF_DEFS := -D_GNU_SOURCE -DUVHTTP_64BIT -DUVHTTP_FEATURE_WEBSOCKET=1 -DUVHTTP_FEATURE_TLS=1 \
            -DUVHTTP_ALLOCATOR_TYPE=0
# the reference's release flags (its CMakeLists.txt: C99 with GNU extensions, -O2 -DNDEBUG).  Its
# warnings stay as they come: the stand-ins declare no mbedtls prototypes, so the five mbedtls
# calls are implicit declarations, which must not become errors with a newer compiler.
REF_CFLAGS := -std=gnu99 -O2 -DNDEBUG -fPIC -Wno-error=implicit-function-declaration
DRV_CFLAGS := -std=gnu11 -O2 -fPIC -Wall -Wextra -Werror

ifneq ($(wildcard $(REF_SRC)),)
ref: _ref/libws_ref.so

_ref/uvhttp_websocket.o: $(REF_SRC) ref_stub/ref_third_party.h
	@mkdir -p _ref
	$(CC) $(REF_CFLAGS) $(REF_DEFS) $(REF_INC) -c -o $@ $(REF_SRC)

_ref/ref_driver.o: ref_driver.c ref_stub/ref_third_party.h $(REF_SRC)
	@mkdir -p _ref
	$(CC) $(DRV_CFLAGS) $(REF_DEFS) $(REF_INC) -c -o $@ ref_driver.c

_ref/libws_ref.so: _ref/uvhttp_websocket.o _ref/ref_driver.o
	$(CC) -shared -Wl,-z,defs -o $@ $^
else
ref:
	@echo "no reference tree at $(REFERENCE_DIR): oracle/_ref is not built"
endif

.PHONY: ref
