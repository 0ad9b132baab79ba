// mq_capi.hip -- kernels + the extern "C" boundary declared in include/mapquik_hip.h.
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC (see mapquik_amd/build.py).  gfx950 only; no CPU fallback.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

// The device parts (each includes what it needs):
#include "mq_blocks.hpp"         // the word blocks kernels and host share: MapCounters, RefBuildInfo, the scanners' results
#include "mq_wave.hpp"           // wave helpers, stage clocks, L2-served loads
#include "mq_device.hpp"         // parameters, Spec, table and Match record types
#include "mq_hash.hpp"           // ntHash seeds, tuple hashes (SipHash-1-3, KhFast)
#include "mq_seed.hpp"           // the fast seeder
#include "mq_seed_general.hpp"   // the general streaming seeder and its list sink
#include "mq_probe.hpp"          // index probe, MapSink
#include "mq_chain.hpp"          // chain stage
#include "mq_fastx.hpp"          // record scanner: one sequence line per record
#include "mq_join.hpp"           // one line-wrapped reference record joined
#include "mq_fastx_lines.hpp"    // record scanner: line-wrapped records, found and joined
#include "mq_redo.hpp"           // overflow redo of a device-resident batch: collect, copy, scatter

using namespace mq;

// The library is ONE translation unit (the kernels inline the device headers; the entry points share static state), kept in parts:
#include "mq_map_kernels.hpp"    // map_kernel and its split-pipeline twins
#include "mq_build_kernels.hpp"  // index build, on-disk form, lookup
#include "mq_cover_kernels.hpp"  // index coverage: bitmap of covered bases, intervals
#include "mq_depth_kernels.hpp"  // mapping depth: per-window accumulators fed from finished hits
#include "mq_sort_kernels.hpp"   // coordinate order of finished hits: a stable LSD radix sort
#include "mq_host_buf.hpp"       // error text, owning buffers and handles, the guard of the extern "C" boundary
#include "mq_host_state.hpp"     // mq_index, mq_ctx, the map kernels' table, geometry, scratch
#include "mq_capi_index.hpp"     // mq_index_new .. mq_index_finalize
#include "mq_ix_chunks.hpp"      // chunk arithmetic of an index file's slot section (plain C++)
#include "mq_capi_index_io.hpp"  // save / load / clone / merge
#include "mq_capi_cover.hpp"     // mq_index_coverage
#include "mq_capi_depth.hpp"     // mq_depth_*
#include "mq_capi_sort.hpp"      // mq_sort_*
#include "mq_capi_map.hpp"       // contexts, map entry points, FASTA chunks, PAF, host memory
#include "mq_capi_diag.hpp"      // include/mapquik_hip_diag.h
