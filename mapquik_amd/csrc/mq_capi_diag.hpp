// mq_capi_diag.hpp -- measurement and diagnostic entry points (include/mapquik_hip_diag.h): probe statistics, stage clocks, launch timers, the
// random-probe rate of the memory system (part of the one translation unit mq_capi.hip).  Nothing here is on the product path.  The entry
// points run inside guarded() and own what they allocate, like the rest of the C ABI.
#pragma once

// Diagnostic (tools/probe_rate.py): how many random index probes per second the memory system sustains, detached from
// everything else the map path does.  Every thread looks up `per_thread` pseudo-random keys (absent with probability ~1,
// like ~85 % of a read's k-min-mers), `ilp` home-slot loads in flight per thread.
__global__ void probe_rate_kernel(const Bucket *__restrict__ table, uint64_t mask, uint32_t per_thread, uint64_t seed,
                                  unsigned long long *__restrict__ acc, const uint32_t *__restrict__ bitmap, uint64_t bit_mask,
                                  uint32_t table_too) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nb = (mask + 1) >> 1;
    unsigned long long found = 0, steps = 0;
    auto mix = [](uint64_t z) {
        z += 0x9e3779b97f4a7c15ULL;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        return z ^ (z >> 31);
    };
    for (uint32_t j = 0; j < per_thread; j += 4) {
        uint64_t key[4];
        uint4 kk[4];
        uint32_t bw[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            key[u] = mix(seed + tid * per_thread + j + u) | 1ull;
            if (bitmap) bw[u] = bitmap[(key[u] & bit_mask) >> 5];
            else kk[u] = ld_u4(&table[(key[u] & mask) >> 1].key[0]);
        }
        if (bitmap) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool maybe = (bw[u] >> (key[u] & 31u)) & 1u;
                found += maybe;
                kk[u] = (maybe && table_too) ? ld_u4(&table[(key[u] & mask) >> 1].key[0]) : make_uint4(0, 0, 0, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            // the probe sequence of mq_device.hpp ("Index table"): home way, other way, then the following buckets
            const uint32_t w0 = (uint32_t)(key[u] & mask) & 1u;
            uint64_t ka = u64_of(kk[u].x, kk[u].y), kb = u64_of(kk[u].z, kk[u].w);
            uint64_t kh = w0 ? kb : ka, kp = w0 ? ka : kb;
            uint64_t b = (key[u] & mask) >> 1;
            bool hit = kh == key[u], go = !hit && kh != 0;
            if (go) {
                steps++;
                hit = kp == key[u];
                go = !hit && kp != 0;
            }
            while (go) {
                b = b + 1 == nb ? 0 : b + 1;
                const uint4 v = ld_u4(&table[b].key[0]);
                ka = u64_of(v.x, v.y);
                kb = u64_of(v.z, v.w);
                steps++;
                hit = ka == key[u];
                go = !hit && ka != 0;
                if (go) {
                    steps++;
                    hit = kb == key[u];
                    go = !hit && kb != 0;
                }
            }
            if (hit) found += table[b].pay[0].start & 1u;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        found += __shfl_xor(found, d, 64);
        steps += __shfl_xor(steps, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&acc[0], found);
        atomicAdd(&acc[1], steps);
    }
}

// one field (or a run of neighbouring fields) of the context's counter block, copied to the host
static hipError_t counter_field(const mq_ctx *c, void *dst, size_t offset, size_t bytes) {
    return hipMemcpy(dst, reinterpret_cast<const uint8_t *>(c->d_counter.p) + offset, bytes, hipMemcpyDeviceToHost);
}

extern "C" {

int mq_last_map_path_counts(mq_index *idx, uint32_t *n_fast, uint32_t *n_general) {
    return guarded([&]() -> int {
        if (!idx || !n_fast || !n_general) return set_err(MQ_EINVAL, "bad arguments");
        std::lock_guard<std::mutex> lk(idx->mu);
        mq_ctx *c = idx->def_ctx.get();
        if (!c->ev_valid) return set_err(MQ_ESTATE, "no map launch recorded");
        int rc = use_device(idx);
        if (rc) return rc;
        HIPCHK(hipEventSynchronize(c->ev1));
        uint32_t v[2] = {0, 0};  // n_fast and n_general are neighbours: one copy
        static_assert(offsetof(MapCounters, n_general) == offsetof(MapCounters, n_fast) + sizeof(MapCounters::n_fast), "n_fast, n_general");
        HIPCHK(counter_field(c, v, offsetof(MapCounters, n_fast), sizeof(MapCounters::n_fast) + sizeof(MapCounters::n_general)));
        *n_fast = v[0];
        *n_general = v[1];
        return MQ_OK;
    });
}

// Which MAP_SPECS pair the last fused launch sequence ran: of the index's default context / of a context (0: SpecNone)
int mqdiag_last_map_spec(mq_index *idx, uint32_t *spec_id) {
    return guarded([&]() -> int {
        if (!idx || !spec_id) return set_err(MQ_EINVAL, "bad arguments");
        std::lock_guard<std::mutex> lk(idx->mu);
        mq_ctx *c = idx->def_ctx.get();
        if (!c->ev_valid) return set_err(MQ_ESTATE, "no map launch recorded");
        *spec_id = c->last_spec;
        return MQ_OK;
    });
}
int mqdiag_ctx_last_map_spec(mq_ctx *ctx, uint32_t *spec_id) {
    return guarded([&]() -> int {
        if (!ctx || !spec_id) return set_err(MQ_EINVAL, "bad arguments");
        if (!ctx->ev_valid) return set_err(MQ_ESTATE, "no map launch recorded");
        *spec_id = ctx->last_spec;
        return MQ_OK;
    });
}

int mq_last_map_order(mq_index *idx, uint32_t *n_flagged, uint32_t *n_first) {
    return guarded([&]() -> int {
        if (!idx || !n_flagged || !n_first) return set_err(MQ_EINVAL, "bad arguments");
        std::lock_guard<std::mutex> lk(idx->mu);
        mq_ctx *c = idx->def_ctx.get();
        if (!c->ev_valid) return set_err(MQ_ESTATE, "no map launch recorded");
        int rc = use_device(idx);
        if (rc) return rc;
        HIPCHK(hipEventSynchronize(c->ev1));
        uint32_t v = 0;
        HIPCHK(counter_field(c, &v, offsetof(MapCounters, n_flagged), sizeof(MapCounters::n_flagged)));
        *n_flagged = v;
        *n_first = v < WORK_FRONT_CAP ? v : WORK_FRONT_CAP;
        return MQ_OK;
    });
}

int mq_index_table_alloc_ms(mq_index *idx, float *ms) {
    return guarded([&]() -> int {
        if (!idx || !ms) return set_err(MQ_EINVAL, "bad arguments");
        std::lock_guard<std::mutex> lk(idx->mu);
        if (!idx->finalized) return set_err(MQ_ESTATE, "index not finalized");
        *ms = (float)idx->table_alloc_ms;
        return MQ_OK;
    });
}

int mq_map_launch_waves(mq_index *idx, uint32_t n_reads, uint32_t *n_waves) {
    return guarded([&]() -> int {
        if (!idx || !n_waves) return set_err(MQ_EINVAL, "bad arguments");
        int rc = use_device(idx);
        if (rc) return rc;
        if ((rc = ensure_geometry(idx))) return rc;
        *n_waves = fused_grid(idx, n_reads) * (uint32_t)MAP_WAVES;
        return MQ_OK;
    });
}

int mq_map_probe_stats(mq_index *idx, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n, uint64_t total_bases, mq_hit *d_out,
                       uint64_t *lookups, uint64_t *extra_steps) {
    return guarded([&]() -> int {
        if (!idx || !lookups || !extra_steps) return set_err(MQ_EINVAL, "bad arguments");
        std::lock_guard<std::mutex> lk(idx->mu);
        mq_ctx *c = idx->def_ctx.get();
        int rc = ctx_map_device(c, d_bases, d_offsets, n, total_bases, d_out, nullptr, true);  // the choice travels with this launch: contexts never see it
        if (rc) return rc;
        HIPCHK(hipEventSynchronize(c->ev1));
        ProbeStats v;
        HIPCHK(counter_field(c, &v, offsetof(MapCounters, probe), sizeof(MapCounters::probe)));
        *extra_steps = v.steps;
        *lookups = v.lookups;
        return MQ_OK;
    });
}

// Diagnostic: what every read of the last mq_map_probe_stats launch cost its wave (shader-clock cycles from the read's first instruction to
// its result's store) and when the wave took it up (the 100-MHz constant clock): where a launch's tail comes from.
int mq_last_read_cycles(mq_index *idx, uint32_t n, uint32_t *cycles, uint64_t *start_ticks) {
    return guarded([&]() -> int {
        if (!idx || !cycles || !start_ticks) return set_err(MQ_EINVAL, "bad arguments");
        std::lock_guard<std::mutex> lk(idx->mu);
        mq_ctx *c = idx->def_ctx.get();
        if (!c->ev_valid || n > c->reads_cap) return set_err(MQ_ESTATE, "no instrumented launch of that size recorded");
        int rc = use_device(idx);
        if (rc) return rc;
        HIPCHK(hipEventSynchronize(c->ev1));
        HIPCHK(hipMemcpy(cycles, ctx_read_cycles(c), (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(start_ticks, ctx_read_start(c), (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
        return MQ_OK;
    });
}

// Diagnostic (-DMQ_STAGE_CLOCKS builds; zeros otherwise): shader-clock cycles the waves of the last map_kernel launch of the default
// context spent per stage, summed over waves (stage list: mq_wave.hpp, mq_clk).
int mq_last_stage_clocks(mq_index *idx, uint64_t *out16) {
    return guarded([&]() -> int {
        if (!idx || !out16) return set_err(MQ_EINVAL, "bad arguments");
        std::lock_guard<std::mutex> lk(idx->mu);
        mq_ctx *c = idx->def_ctx.get();
        if (!c->ev_valid) return set_err(MQ_ESTATE, "no map launch recorded");
        int rc = use_device(idx);
        if (rc) return rc;
        HIPCHK(hipEventSynchronize(c->ev1));
        static_assert(MQ_N_CLK == 16, "mq_last_stage_clocks fills 16 words (include/mapquik_hip_diag.h)");
        HIPCHK(counter_field(c, out16, offsetof(MapCounters, clk), sizeof(MapCounters::clk)));
        return MQ_OK;
    });
}

int mq_last_map_ms(mq_index *idx, float *ms) {
    return guarded([&]() -> int {
        if (!idx || !ms) return set_err(MQ_EINVAL, "bad arguments");
        std::lock_guard<std::mutex> lk(idx->mu);
        mq_ctx *c = idx->def_ctx.get();
        if (!c->ev_valid) return set_err(MQ_ESTATE, "no map launch recorded");
        HIPCHK(hipEventSynchronize(c->ev1));
        HIPCHK(hipEventElapsedTime(ms, c->ev0, c->ev1));
        return MQ_OK;
    });
}

int mq_probe_rate(mq_index *idx, uint32_t blocks, uint32_t per_thread, uint32_t bitmap_log2, uint32_t table_too, float *ms,
                  uint64_t *lookups, uint64_t *extra_steps) {
    return guarded([&]() -> int {
        if (!idx || !ms || !lookups || !extra_steps) return set_err(MQ_EINVAL, "bad arguments");
        if (!idx->finalized) return set_err(MQ_ESTATE, "index not finalized");
        std::lock_guard<std::mutex> lk(idx->mu);
        int rc = use_device(idx);
        if (rc) return rc;
        Buf<unsigned long long> d_acc;
        Buf<uint8_t> bm_bytes;
        ScopedEvent e0, e1;
        uint64_t bit_mask = 0;
        if ((rc = d_acc.alloc(2))) return rc;
        HIPCHK(hipMemset(d_acc, 0, 16));
        if (bitmap_log2) {  // a stand-in bitmap with one bit in eight set
            bit_mask = (1ull << bitmap_log2) - 1;
            if ((rc = bm_bytes.alloc((uint64_t)1 << (bitmap_log2 - 3)))) return rc;
            HIPCHK(hipMemset(bm_bytes, 0x10, (size_t)1 << (bitmap_log2 - 3)));
        }
        const uint32_t *const bm = reinterpret_cast<const uint32_t *>(bm_bytes.p);
        HIPCHK(hipEventCreate(&e0.h));
        HIPCHK(hipEventCreate(&e1.h));
        per_thread = (per_thread + 3u) & ~3u;
        hipLaunchKernelGGL(probe_rate_kernel, dim3(blocks), dim3(256), 0, 0, idx->table, idx->nslots - 1, per_thread, 1ull, d_acc, bm, bit_mask, table_too);  // warm-up
        HIPCHK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(probe_rate_kernel, dim3(blocks), dim3(256), 0, 0, idx->table, idx->nslots - 1, per_thread, 0x1234567ull, d_acc, bm, bit_mask, table_too);
        HIPCHK(hipEventRecord(e1, 0));
        HIPCHK(hipEventSynchronize(e1));
        HIPCHK(hipEventElapsedTime(ms, e0, e1));
        unsigned long long acc[2];
        HIPCHK(hipMemcpy(acc, d_acc, 16, hipMemcpyDeviceToHost));
        *lookups = (uint64_t)blocks * 256ull * per_thread;
        *extra_steps = acc[1] / 2;  // two launches accumulated
        return MQ_OK;
    });
}

int mq_ctx_last_map_ms(mq_ctx *ctx, float *ms) {
    return guarded([&]() -> int {
        if (!ctx || !ms) return set_err(MQ_EINVAL, "bad arguments");
        if (!ctx->ev_valid) return set_err(MQ_ESTATE, "no map launch recorded");
        HIPCHK(hipEventSynchronize(ctx->ev1));
        HIPCHK(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
        return MQ_OK;
    });
}

uint64_t mqdiag_coverage_tile_bits(void) { return 64ull * MQ_COV_TILE_WORDS; }
uint64_t mqdiag_coverage_held(const mq_index *idx) { return idx ? idx->cov.held() : 0; }
// MQ_COVER_TIMING=1: the last mq_index_coverage of this thread, in ms -- [0] bitmap clear [1] cover_mark_kernel [2] cover_count_kernel
// [3] cover_scan_kernel [4] cover_emit_kernel [5] count_kernel's pass over the same table
int mqdiag_coverage_ms(float *out6) {
    if (!out6) return set_err(MQ_EINVAL, "bad arguments");
    memcpy(out6, g_cover_ms, sizeof(g_cover_ms));
    return MQ_OK;
}

uint64_t mqdiag_depth_tile_windows(void) { return MQ_DEPTH_TILE_WINDOWS; }
// the kernels of the accumulator's last mq_depth_result, between two events on its stream
int mqdiag_depth_result_ms(mq_depth *d, float *ms) {
    if (!d || !ms) return set_err(MQ_EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(d->mu);
    *ms = d->result_ms;
    return MQ_OK;
}

uint64_t mqdiag_sort_tile_records(void) { return MQ_SORT_TILE; }
// the digits the sorter's last mq_sort_result sorted (of 11), and that result's device time between two events on its stream
int mqdiag_sort_passes(mq_sorter *s, uint32_t *passes) {
    if (!s || !passes) return set_err(MQ_EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(s->mu);
    *passes = s->passes;
    return MQ_OK;
}
int mqdiag_sort_result_ms(mq_sorter *s, float *ms) {
    if (!s || !ms) return set_err(MQ_EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(s->mu);
    *ms = s->result_ms;
    return MQ_OK;
}

}  // extern "C"
