# The build recipe of a library layered on libmldsa_hip.so, included by the Makefiles of ../ph, ../keys, ../mu, ../seed, ../keycheck and ../mus
# (paths are relative to those directories).  The including Makefile sets LIB (the library's file name), OBJS and HDRS.
# The headers of this directory go into HDRS as each library includes them: layer_host.h and layer_dev.h, and for ../ph and ../mus
# host_feed.h with host_chunks.h.
# The core library is built by ../csrc/Makefile and only linked here: nothing in this file rebuilds, relinks or re-flags it.
# Every kernel's register / scratch / LDS use is written next to its object as <file>.res (-Rpass-analysis=kernel-resource-usage).
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
CXXFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-function
CORE    = ../csrc/libmldsa_hip.so

all: $(LIB)

$(LIB): $(OBJS) | $(CORE)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $(OBJS) -L../csrc -lmldsa_hip -Wl,-rpath,'$$ORIGIN/../csrc' -Wl,-rpath,/opt/rocm/lib

%.o: %.hip $(HDRS)
	$(HIPCC) $(CXXFLAGS) -Rpass-analysis=kernel-resource-usage -c $< -o $@ 2> $*.res || { cat $*.res >&2; rm -f $*.res; exit 1; }
	@grep -E "warning|error" $*.res >&2 || true

$(CORE):
	@echo "$(CORE) is missing: build the core first (make -C ../csrc)" >&2; exit 1

clean:
	rm -f *.o *.res $(LIB)

.PHONY: all clean
