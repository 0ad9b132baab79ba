# Builds the product without Python: the gfx950 HIP library (C ABI) and the native `mapquik` driver.
# (python __graft_entry__.py does the same and also builds the test-only oracle and input generator.)
HIPCC ?= /opt/rocm/bin/hipcc
CXX   ?= g++
LIBDIR := mapquik_amd/lib
CSRC   := mapquik_amd/csrc

all: $(LIBDIR)/libmapquik_hip.so $(LIBDIR)/mapquik

# every part of the library's one translation unit (mq_capi.hip includes them all) and both headers: a stale .so would make parity
# and perf numbers describe old kernels (mapquik_amd/build.py globs the same files)
$(LIBDIR)/libmapquik_hip.so: $(CSRC)/mq_capi.hip $(wildcard $(CSRC)/*.hpp) $(wildcard include/*.h)
	mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -Wno-unused-value -Wno-align-mismatch -mllvm -amdgpu-atomic-optimizer-strategy=None -mllvm -pragma-unroll-threshold=65536 -o $@ $(CSRC)/mq_capi.hip

$(LIBDIR)/mapquik: $(CSRC)/host/mapquik_main.cc $(wildcard $(CSRC)/host/*.hpp) $(wildcard include/*.h) $(LIBDIR)/libmapquik_hip.so
	$(CXX) -O2 -std=c++17 -Wall -o $@ $(CSRC)/host/mapquik_main.cc -L$(LIBDIR) -lmapquik_hip -lz -lpthread -ldl -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,/opt/rocm/lib

# Sanitizer builds of the threaded host code (CPU only: no sanitizer runs on the GPU build).  The driver links a host-only stub of
# the C ABI with canned results (tests/cpp/stub_mapquik_hip.cc, stub_mapquik_hip_lines.cc on top of it for line-wrapped references, and
# stub_mapquik_hip_reads_lines.cc on top of that for line-wrapped reads, stub_mapquik_hip_extend.cc on top of that for the reopen / resize
# entry points, stub_mapquik_hip_anchors.cc on top of that for the anchor output, stub_mapquik_hip_chains.cc on top of that for the chains output, stub_mapquik_hip_merge.cc on top of that for mq_index_merge*, stub_mapquik_hip_coverage.cc on top of that for mq_index_coverage, stub_mapquik_hip_depth.cc on top of that for mq_depth_*, stub_mapquik_hip_sort.cc on top of that for mq_sort_*); tests/test_sort_host.py, tests/test_depth_host.py, tests/test_index_coverage_host.py, tests/test_index_merge_host.py, tests/test_chains_host.py, tests/test_anchors_host.py, tests/test_sanitizers.py, tests/test_wrapped_reference_host.py, tests/test_wrapped_reads_host.py and
# tests/test_index_extend_host.py build and run these.
HOSTSRC := $(CSRC)/host/mapquik_main.cc $(wildcard $(CSRC)/host/*.hpp) $(wildcard include/*.h)
SAN_A := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1
SAN_T := -fsanitize=thread -fno-omit-frame-pointer -g -O1

asan: $(LIBDIR)/feeder_dump_asan $(LIBDIR)/mapquik_asan $(LIBDIR)/chains_format_asan
tsan: $(LIBDIR)/feeder_dump_tsan $(LIBDIR)/mapquik_tsan $(LIBDIR)/chains_format_tsan

$(LIBDIR)/feeder_dump_asan: $(CSRC)/host/feeder_dump.cc $(HOSTSRC)
	mkdir -p $(LIBDIR)
	$(CXX) $(SAN_A) -std=c++17 -Wall -o $@ $(CSRC)/host/feeder_dump.cc -lz -lpthread -ldl
$(LIBDIR)/feeder_dump_tsan: $(CSRC)/host/feeder_dump.cc $(HOSTSRC)
	mkdir -p $(LIBDIR)
	$(CXX) $(SAN_T) -std=c++17 -Wall -o $@ $(CSRC)/host/feeder_dump.cc -lz -lpthread -ldl
STUB := tests/cpp/stub_mapquik_hip_sort.cc tests/cpp/stub_mapquik_hip_depth.cc tests/cpp/stub_mapquik_hip_coverage.cc tests/cpp/stub_mapquik_hip_merge.cc tests/cpp/stub_mapquik_hip_chains.cc tests/cpp/stub_mapquik_hip_anchors.cc tests/cpp/stub_mapquik_hip_extend.cc tests/cpp/stub_mapquik_hip_reads_lines.cc tests/cpp/stub_mapquik_hip_lines.cc tests/cpp/stub_mapquik_hip.cc  # (each includes the next)
$(LIBDIR)/mapquik_asan: $(HOSTSRC) $(STUB)
	mkdir -p $(LIBDIR)
	$(CXX) $(SAN_A) -std=c++17 -Wall -o $@ $(CSRC)/host/mapquik_main.cc tests/cpp/stub_mapquik_hip_sort.cc -lz -lpthread -ldl
$(LIBDIR)/mapquik_tsan: $(HOSTSRC) $(STUB)
	mkdir -p $(LIBDIR)
	$(CXX) $(SAN_T) -std=c++17 -Wall -o $@ $(CSRC)/host/mapquik_main.cc tests/cpp/stub_mapquik_hip_sort.cc -lz -lpthread -ldl
# mq_format_paf_chain through the C ABI, stand-alone over the stub (tests/test_chains_host.py)
$(LIBDIR)/chains_format_asan: tests/cpp/chains_format_test.cc $(STUB) $(wildcard include/*.h)
	mkdir -p $(LIBDIR)
	$(CXX) $(SAN_A) -std=c++17 -Wall -o $@ tests/cpp/chains_format_test.cc tests/cpp/stub_mapquik_hip_chains.cc -lz -lpthread -ldl
$(LIBDIR)/chains_format_tsan: tests/cpp/chains_format_test.cc $(STUB) $(wildcard include/*.h)
	mkdir -p $(LIBDIR)
	$(CXX) $(SAN_T) -std=c++17 -Wall -o $@ tests/cpp/chains_format_test.cc tests/cpp/stub_mapquik_hip_chains.cc -lz -lpthread -ldl

clean:
	rm -rf $(LIBDIR)

.PHONY: all clean asan tsan
