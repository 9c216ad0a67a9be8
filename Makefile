# Builds the MI355X codec library in-tree (it travels to the GPU box with the
# snapshot) and the parity checker under oracle/.
#
#   make            -> coldforce_amd/libcfws.so + oracle/liboracle.so
#   make ref        -> also oracle/_ref/ (reference codec, needs /root/reference)

HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 -fPIC -Wall -Wno-unused-result
DEVSRC   := cfws_device cfws_plan cfws_slots cfws_h2 cfws_split cfws_relay cfws_keys cfws_handshake cfws_ops cfws_h2index cfws_messages cfws_h2streams cfws_utf8 cfws_uniform
HOSTSRC  := cfws_frame cfws_pipeline cfws_index cfws_graph
HDR      := include/cfws.h include/cfws_co_ws_frame.h coldforce_amd/csrc/cfws_internal.h coldforce_amd/csrc/cfws_rules.h coldforce_amd/csrc/cfws_chunks.h coldforce_amd/csrc/cfws_keyrules.h coldforce_amd/csrc/cfws_keydev.h coldforce_amd/csrc/cfws_devpolicy.h
LIB      := coldforce_amd/libcfws.so
OBJDIR   := build

all: $(LIB) oracle examples guard

# test infrastructure: device buffers between unmapped guard ranges
# (tests/test_gpu_guard.py); host code only, no kernels
guard: tests/native/libguardmem.so

tests/native/libguardmem.so: tests/native/guardmem.cpp
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

# C users of the ABI (no Python): built against include/, linked to libcfws.so
examples: build/examples/batch_roundtrip

build/examples/batch_roundtrip: examples/batch_roundtrip.c $(LIB) $(HDR)
	@mkdir -p build/examples
	$(CC) -O2 -std=gnu11 -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -o $@ $< \
	    -Lcoldforce_amd -lcfws -L/opt/rocm/lib -lamdhip64 \
	    -Wl,-rpath,'$$ORIGIN/../../coldforce_amd' -Wl,-rpath,/opt/rocm/lib

$(OBJDIR)/%.o: coldforce_amd/csrc/%.hip $(HDR) coldforce_amd/csrc/cfws_kernels.h coldforce_amd/csrc/cfws_tables.h
	@mkdir -p $(OBJDIR)
	$(HIPCC) --offload-arch=$(ARCH) $(HIPFLAGS) -Iinclude -Icoldforce_amd/csrc -c $< -o $@

$(OBJDIR)/%.o: coldforce_amd/csrc/%.cpp $(HDR)
	@mkdir -p $(OBJDIR)
	$(HIPCC) --offload-arch=$(ARCH) $(HIPFLAGS) -Iinclude -Icoldforce_amd/csrc -c $< -o $@

$(LIB): $(addprefix $(OBJDIR)/,$(addsuffix .o,$(DEVSRC) $(HOSTSRC)))
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $^

# tools/h2_index_bench.py's host leg (threads of cfws_h2_index_frames calls)
build/libh2hostwalk.so: tools/h2_index_host_walk.cpp $(LIB) $(HDR)
	@mkdir -p build
	$(CXX) -O2 -std=c++17 -fPIC -shared -Wall -Iinclude -o $@ $< -Lcoldforce_amd -lcfws \
	    -Wl,-rpath,'$$ORIGIN/../coldforce_amd' -lpthread

# tools/messages_bench.py's host leg (threads of cfws_messages_from_frames calls)
build/libmsghostwalk.so: tools/messages_host_walk.cpp $(LIB) $(HDR)
	@mkdir -p build
	$(CXX) -O2 -std=c++17 -fPIC -shared -Wall -Iinclude -o $@ $< -Lcoldforce_amd -lcfws \
	    -Wl,-rpath,'$$ORIGIN/../coldforce_amd' -lpthread

# tools/h2_streams_bench.py's host leg (threads of cfws_h2_streams_from_frames calls)
build/libh2streamshostwalk.so: tools/h2_streams_host_walk.cpp $(LIB) $(HDR)
	@mkdir -p build
	$(CXX) -O2 -std=c++17 -fPIC -shared -Wall -Iinclude -o $@ $< -Lcoldforce_amd -lcfws \
	    -Wl,-rpath,'$$ORIGIN/../coldforce_amd' -lpthread

oracle:
	$(MAKE) -s -C oracle

# the host HTTP/2 walk (cfws_index.cpp alone) in a stand-alone host program
# under AddressSanitizer + UBSan; tests/test_h2_index.py builds and runs it
build/h2_index_asan: tests/native/h2_index_asan.cpp coldforce_amd/csrc/cfws_index.cpp $(HDR)
	@mkdir -p build
	$(HIPCC) -x c++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Icoldforce_amd/csrc -o $@ \
	    tests/native/h2_index_asan.cpp coldforce_amd/csrc/cfws_index.cpp

# the host message walk (cfws_messages_from_frames, cfws_index.cpp alone) in a
# stand-alone host program under AddressSanitizer + UBSan;
# tests/test_messages_host.py builds and runs it
build/messages_asan: tests/native/messages_asan.cpp coldforce_amd/csrc/cfws_index.cpp $(HDR)
	@mkdir -p build
	$(HIPCC) -x c++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Icoldforce_amd/csrc -o $@ \
	    tests/native/messages_asan.cpp coldforce_amd/csrc/cfws_index.cpp

# the host UTF-8 check (cfws_utf8_check_messages, cfws_index.cpp alone) in a
# stand-alone host program under AddressSanitizer + UBSan;
# tests/test_utf8_host.py builds and runs it
build/utf8_asan: tests/native/utf8_asan.cpp coldforce_amd/csrc/cfws_index.cpp $(HDR)
	@mkdir -p build
	$(HIPCC) -x c++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Icoldforce_amd/csrc -o $@ \
	    tests/native/utf8_asan.cpp coldforce_amd/csrc/cfws_index.cpp

# tools/utf8_bench.py's host leg (threads of cfws_utf8_check_messages calls)
build/libutf8hostwalk.so: tools/utf8_host_walk.cpp $(LIB) $(HDR)
	@mkdir -p build
	$(CXX) -O2 -std=c++17 -fPIC -shared -Wall -Iinclude -o $@ $< -Lcoldforce_amd -lcfws \
	    -Wl,-rpath,'$$ORIGIN/../coldforce_amd' -lpthread

# the host stream grouping (cfws_h2_streams_from_frames, cfws_index.cpp alone)
# in a stand-alone host program under AddressSanitizer + UBSan;
# tests/test_h2_streams.py builds and runs it
build/h2_streams_asan: tests/native/h2_streams_asan.cpp coldforce_amd/csrc/cfws_index.cpp $(HDR)
	@mkdir -p build
	$(HIPCC) -x c++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Icoldforce_amd/csrc -o $@ \
	    tests/native/h2_streams_asan.cpp coldforce_amd/csrc/cfws_index.cpp

# the pipeline's chunk cuts (cfws_chunks.h, header only) in a stand-alone host
# program under AddressSanitizer + UBSan; tests/test_pipeline_chunks.py builds
# and runs it
build/chunks_test: tests/native/chunks_test.cpp $(HDR)
	@mkdir -p build
	$(HIPCC) -x c++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Icoldforce_amd/csrc -o $@ \
	    tests/native/chunks_test.cpp

ref: all
	$(MAKE) -s -C oracle ref

asm: $(HDR) coldforce_amd/csrc/cfws_kernels.h coldforce_amd/csrc/cfws_tables.h
	@mkdir -p $(OBJDIR)/asm
	rm -f $(OBJDIR)/asm/resource-usage.txt
	for d in $(DEVSRC); do $(HIPCC) --offload-arch=$(ARCH) $(HIPFLAGS) -Iinclude -Icoldforce_amd/csrc -c coldforce_amd/csrc/$$d.hip -o $(OBJDIR)/asm/$$d.o \
	    -save-temps=obj -Rpass-analysis=kernel-resource-usage 2>> $(OBJDIR)/asm/resource-usage.txt || exit 1; done

clean:
	rm -rf $(OBJDIR) $(LIB) tests/native/libguardmem.so
	$(MAKE) -s -C oracle clean

.PHONY: all oracle ref asm clean examples guard

# A/B build variants of the numeric tunables (kept out of git under build/): make variant V=ser4 F="-DCFWS_SER_LDS=40000"
variant: $(HDR)
	@mkdir -p $(OBJDIR)/variants/$(V)
	for d in $(DEVSRC); do $(HIPCC) --offload-arch=$(ARCH) $(HIPFLAGS) $(F) -Iinclude -Icoldforce_amd/csrc -c coldforce_amd/csrc/$$d.hip -o $(OBJDIR)/variants/$(V)/$$d.o || exit 1; done
	for h in $(HOSTSRC); do $(HIPCC) --offload-arch=$(ARCH) $(HIPFLAGS) $(F) -Iinclude -Icoldforce_amd/csrc -c coldforce_amd/csrc/$$h.cpp -o $(OBJDIR)/variants/$(V)/$$h.o || exit 1; done
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $(OBJDIR)/variants/libcfws_$(V).so $(OBJDIR)/variants/$(V)/*.o

.PHONY: variant
