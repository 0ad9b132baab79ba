// mq_capi_map.hpp -- C ABI, mapping side: launch sequences (the kernel pair of each comes from MAP_KERNELS), stream-slot contexts
// (mq_ctx_*), host-buffer and device-resident entry points (mq_map_reserve for the default context's), the overflow redo (through the host, and in stream), the reservation and
// read-back of the pooled outputs (PooledOutput, mq_host_state.hpp: anchors and chains share every line but the chain windows),
// device-parsed FASTA chunks, PAF formatting, page-locked host memory (part of the one translation unit mq_capi.hip).  Temporary device
// memory is a Buf: it goes when its function returns, by whichever way.
#pragma once

struct LaunchOpt {
    mq_kminmer *d_dump = nullptr;
    const uint64_t *d_dump_off = nullptr;
    uint32_t *d_dump_counts = nullptr;
    MatchRec *scratch_override = nullptr;  // overflow redo: worst-case Match scratch on a small grid
    uint32_t cap_override = 0;
    uint32_t grid_override = 0;
    uint32_t f16 = 0;                      // 0 => list_f16(idx)
    const uint32_t *d_lens = nullptr;      // spans form: per-read lengths
    bool instrumented = false;             // mq_map_probe_stats: the launch that counts lookups and probe steps (slower, never timed)
    // the pooled outputs (PooledOutput: anchors, chains) the launch delivers to
    mq_ctx *outputs_of = nullptr;          // the context whose reservations they are (nullptr: c itself; the arena's launch: its owner)
    bool redo = false;                     // a redo launch of a batch: the batch's cursors go on, every span goes where the id map says
    const uint32_t *d_ids = nullptr;       // ... the id map of both outputs (MapArgs::anchor_ids, ChainLaunch::ids); nullptr: each reservation's own `ids`
    ChainRec *chain_windows_override = nullptr;  // goes with scratch_override: as many windows, of chain_win_cap(cap_override) records
};

// (nothing of the context changes here: the batch becomes "the last batch" in launch_map)
static int outputs_admit(const mq_ctx *c, uint32_t n) {
    int rc = c->anchors.admit(n);
    return rc ? rc : c->chains.admit(n);
}

// One launch sequence on stream `st` using the context's scratch.  ctx_ensure(c, n, total_bases, f16) must have succeeded.
static int launch_map(mq_ctx *c, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n, mq_hit *d_out, hipStream_t st,
                      const LaunchOpt &o = LaunchOpt()) {
    mq_index *idx = c->idx;
    if (n == 0) return MQ_OK;
    // a context with an anchors reservation takes the anchors pair, one with a chains reservation the chains pair, one with both the pair
    // that writes both (never for the instrumented launch, nor for mq_kminmers_batch's, nor in the split pipeline)
    mq_ctx *oc = o.outputs_of ? o.outputs_of : c;
    const bool delivers = !o.instrumented && !o.d_dump && !idx->split;
    const bool anch = oc->anchors.reads != 0 && delivers, chn = oc->chains.reads != 0 && delivers;
    int rc;
    if (anch && !o.redo && ((rc = oc->anchors.admit(n)) || (rc = oc->anchors.begin_batch(n, st)))) return rc;
    if (chn) {
        if (o.scratch_override && !o.chain_windows_override) return set_err(MQ_ESTATE, "a redo launch of a chains context without chain windows");
        if (!o.redo && ((rc = oc->chains.admit(n)) || (rc = oc->chains.begin_batch(n, st)))) return rc;
    }
    const auto id_map = [&o](const Buf<uint32_t> &own) -> const uint32_t * { return !o.redo ? nullptr : o.d_ids ? o.d_ids : own.p; };
    HIPCHK(hipMemsetAsync(c->d_counter, 0, sizeof(MapCounters), st));
    HIPCHK(hipEventRecord(c->ev0, st));
    MapArgs A;
    A.bases = d_bases;
    A.offsets = d_offsets;
    A.lens = o.d_lens;
    A.n = n;
    A.P = idx->dp;
    A.mz_hash = c->mz_hash;
    A.mz_pos = c->mz_pos;
    A.mz_last = c->mz_last;
    A.mz_count = c->mz_count;
    A.mz_base = c->mz_base;
    A.pool_base = c->pool_base;
    A.pool_cap = c->pool_cap;
    A.f16 = o.f16 ? o.f16 : list_f16(idx);
    A.slack = LIST_SLACK;
    A.queue = c->queue;
    A.counters = c->d_counter;
    A.force_general = idx->force_general ? 1u : 0u;
    A.table = idx->table;
    A.mask = idx->nslots - 1;
    A.ref_lens = idx->d_ref_lens;
    A.scratch_all = o.scratch_override ? o.scratch_override : c->scratch;
    A.cap_matches = o.scratch_override ? o.cap_override : idx->cap_matches;
    A.out = d_out;
    A.dump = o.d_dump;
    A.dump_off = o.d_dump_off;
    A.dump_counts = o.d_dump_counts;
    A.stats64 = &c->d_counter.p->probe;
    A.work = c->work;
    A.heavy_first = idx->heavy_first ? 1u : 0u;
    A.anchors.pool = anch ? oc->anchors.pool.p : nullptr;
    A.anchors.cap = anch ? (uint32_t)oc->anchors.cap : 0u;
    A.anchors.counters = anch ? oc->anchors.counters.p : nullptr;
    A.anchor_spans = anch ? oc->anchors.spans.p : nullptr;
    A.anchor_ids = anch ? id_map(oc->anchors.ids) : nullptr;
    if (chn) {
        // the chains output's launch arguments: into the counter block, behind its clearing (from pageable memory: the bytes are taken now)
        ChainLaunch cl;
        cl.pool = oc->chains.pool.p;
        cl.cap = (uint32_t)oc->chains.cap;
        cl.win_cap = chain_win_cap(A.cap_matches);
        cl.counters = oc->chains.counters.p;
        cl.windows = o.scratch_override ? o.chain_windows_override : oc->chn_windows.p;
        cl.spans = oc->chains.spans.p;
        cl.ids = id_map(oc->chains.ids);
        HIPCHK(hipMemcpyAsync(&c->d_counter.p->chains, &cl, sizeof(ChainLaunch), hipMemcpyHostToDevice, st));
    }
    if (!idx->split) {
        if (n > WORK_ID_MASK) return set_err(MQ_EINVAL, "more than 2^30 - 1 reads in one batch");
        hipLaunchKernelGGL(order_reads_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, A);  // the launch order (and map_kernel's work descriptors)
        uint32_t grid = fused_grid(idx, n);
        if (o.grid_override) grid = std::min(grid, o.grid_override);
        if (anch || chn) grid = std::min(grid, idx->grid_fused_outputs);
        const dim3 blk(64 * MAP_WAVES);
        // (a seeding variant other than the frozen reading takes the instantiation built with the variants; the frozen reading with the
        // parameters of a MAP_SPECS entry takes the pair compiled for them)
        const MapPair &kp = map_pair_of(idx, o.instrumented, &c->last_spec, anch, chn);
        hipLaunchKernelGGL(kp.map, dim3(grid), blk, 0, st, A);
        HIPCHK(hipGetLastError());
        // the reads the fast seeder declined (queue length on the device: map_kernel's grid, its waves leave at once when there are none)
        hipLaunchKernelGGL(kp.declined, dim3(grid), blk, 0, st, A);
        HIPCHK(hipGetLastError());
    } else {
        const uint32_t gs = std::min<uint32_t>(idx->grid_seed, (n + SEED_WAVES - 1) / SEED_WAVES);
        const char *ss = getenv("MQ_SEED_STOP");  // diagnostic: stage attribution by truncation (results are NOT valid)
        const int stop = ss ? atoi(ss) : 0;
        if (stop == 1) hipLaunchKernelGGL(seed_reads_kernel<1>, dim3(gs), dim3(64 * SEED_WAVES), 0, st, A);
        else if (stop == 2) hipLaunchKernelGGL(seed_reads_kernel<2>, dim3(gs), dim3(64 * SEED_WAVES), 0, st, A);
        else hipLaunchKernelGGL(seed_reads_kernel<0>, dim3(gs), dim3(64 * SEED_WAVES), 0, st, A);
        HIPCHK(hipGetLastError());
        // the reads the fast seeder declined: the queue length lives on the device, so the grid is fixed and waves that find
        // the queue empty leave at once
        const uint32_t gg = std::min<uint32_t>((uint32_t)idx->n_cu * 8u, n);
        hipLaunchKernelGGL(seed_general_kernel, dim3(gg), dim3(64), 0, st, A);
        HIPCHK(hipGetLastError());
        uint32_t gm = std::min<uint32_t>(idx->grid_map, (n + ML_WAVES - 1) / ML_WAVES);
        if (o.grid_override) gm = std::min(gm, o.grid_override);
        const dim3 blk(64 * ML_WAVES);
        if (o.instrumented) hipLaunchKernelGGL((map_lists_kernel<64, true>), dim3(gm), blk, 0, st, A);
        else if (idx->chain_chunk == 4) hipLaunchKernelGGL((map_lists_kernel<4, false>), dim3(gm), blk, 0, st, A);
        else hipLaunchKernelGGL((map_lists_kernel<64, false>), dim3(gm), blk, 0, st, A);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(c->ev1, st));
    c->ev_valid = true;
    if (anch && (rc = oc->anchors.mark_done(st))) return rc;
    return chn ? oc->chains.mark_done(st) : MQ_OK;
}

// Reads that came back MQ_HIT_OVERFLOW (more Match runs than the per-wave scratch holds, or a minimizer list denser than its
// region) are mapped again on the GPU with worst-case scratch and list regions on a small grid.  Never a CPU path.
static std::vector<uint32_t> overflow_reads(const mq_hit *out, uint32_t n) {
    std::vector<uint32_t> redo;
    for (uint32_t i = 0; i < n; ++i)
        if (out[i].status == MQ_HIT_OVERFLOW) redo.push_back(i);
    return redo;
}

// The small grid of a redo launch: as many workgroups as have worst-case Match windows (cap records per wave) in 1 GB, at least one
constexpr uint32_t REDO_WAVES = (uint32_t)std::max(MAP_WAVES, ML_WAVES);  // windows per workgroup, whichever pipeline runs
static uint32_t redo_grid(const mq_index *idx, uint32_t cap) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min(idx->grid_fused, idx->grid_map), (1ull << 30) / ((uint64_t)cap * sizeof(MatchRec) * REDO_WAVES)));
}

// The relaunch: read j of the redo list is sb[so[j], so[j + 1]); its hit goes to out[redo[j]]
static int redo_relaunch(mq_ctx *c, const std::vector<uint32_t> &redo, const std::vector<uint8_t> &sb, const std::vector<uint64_t> &so, mq_hit *out) {
    mq_index *idx = c->idx;
    uint64_t sub_max = 0;
    for (size_t j = 0; j < redo.size(); ++j) sub_max = std::max(sub_max, so[j + 1] - so[j]);
    const uint64_t sub_total = so.back();
    const uint32_t cap = (uint32_t)std::max<uint64_t>(sub_max, 1);  // a read cannot have more runs than bases
    const uint32_t waves = REDO_WAVES;
    const uint32_t rgrid = redo_grid(idx, cap);
    int rc = ctx_ensure(c, (uint32_t)redo.size(), sub_total, 65536u);
    if (rc) return rc;
    Buf<MatchRec> big;
    Buf<ChainRec> big_chains;  // (a context with a chains reservation) the redo's chain windows, beside its Match windows
    Buf<uint8_t> d_sb;
    Buf<uint64_t> d_so;
    Buf<mq_hit> d_sh;
    hipError_t e = big.try_alloc((uint64_t)rgrid * waves * cap);
    if (e == hipSuccess && c->chains.reads) e = big_chains.try_alloc((uint64_t)rgrid * waves * chain_win_cap(cap));
    if (e == hipSuccess) e = d_sb.try_alloc(sub_total + 1);
    if (e == hipSuccess) e = d_so.try_alloc(so.size());
    if (e == hipSuccess) e = d_sh.try_alloc(redo.size());
    if (e == hipSuccess && sub_total) e = hipMemcpyAsync(d_sb, sb.data(), sub_total, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_so, so.data(), so.size() * 8, hipMemcpyHostToDevice, c->stream);
    int rrc = MQ_OK;
    std::vector<mq_hit> sh(redo.size());
    if (e == hipSuccess) {
        LaunchOpt o;
        o.scratch_override = big;
        o.cap_override = cap;
        o.grid_override = rgrid;
        o.f16 = 65536u;
        // a read that is redone delivers its anchors and chains from the redo: same pools, same cursors, its spans to the batch's read number
        // (each reservation's own `ids`)
        o.redo = true;
        if (c->anchors.reads) e = hipMemcpyAsync(c->anchors.ids, redo.data(), redo.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
        if (c->chains.reads && e == hipSuccess) {
            e = hipMemcpyAsync(c->chains.ids, redo.data(), redo.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
            o.chain_windows_override = big_chains;
        }
        if (e == hipSuccess) rrc = launch_map(c, d_sb, d_so, (uint32_t)redo.size(), d_sh, c->stream, o);
    }
    if (e == hipSuccess && rrc == MQ_OK) e = hipMemcpyAsync(sh.data(), d_sh, redo.size() * sizeof(mq_hit), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    else hipStreamSynchronize(c->stream);  // (the stream is idle before the buffers go, whichever way this returns)
    if (e != hipSuccess) return set_err(e == hipErrorOutOfMemory ? MQ_ENOMEM : MQ_EHIP, std::string("overflow retry: ") + hipGetErrorString(e));
    if (rrc) return rrc;
    for (size_t j = 0; j < redo.size(); ++j) out[redo[j]] = sh[j];
    return MQ_OK;
}

// ... of a batch in host arrays (lens == nullptr: read i ends at offsets[i + 1])
static int redo_overflow(mq_ctx *c, const uint8_t *bases, const uint64_t *offsets, const uint32_t *lens, uint32_t n, mq_hit *out) {
    const std::vector<uint32_t> redo = overflow_reads(out, n);
    if (redo.empty()) return MQ_OK;
    std::vector<uint64_t> so(redo.size() + 1, 0);
    for (size_t j = 0; j < redo.size(); ++j) so[j + 1] = so[j] + (lens ? (uint64_t)lens[redo[j]] : offsets[redo[j] + 1] - offsets[redo[j]]);
    std::vector<uint8_t> sb(so.back() ? so.back() : 1);
    for (size_t j = 0; j < redo.size(); ++j) memcpy(sb.data() + so[j], bases + offsets[redo[j]], (size_t)(so[j + 1] - so[j]));
    return redo_relaunch(c, redo, sb, so, out);
}

// ... of a piece whose records the device found: THOSE reads' offsets, lengths (d_lens == nullptr: up to d_offsets[r + 1]) and bytes come back from the arrays the launch read
static int redo_overflow_device(mq_ctx *c, const uint8_t *d_bytes, const uint64_t *d_offsets, const uint32_t *d_lens, uint32_t n, mq_hit *out) {
    const std::vector<uint32_t> redo = overflow_reads(out, n);
    if (redo.empty()) return MQ_OK;
    std::vector<uint64_t> at(2 * redo.size()), so(redo.size() + 1, 0);  // at[2 j], at[2 j + 1]: where read j begins and (device form) ends
    std::vector<uint32_t> len(redo.size());
    for (size_t j = 0; j < redo.size(); ++j) {
        HIPCHK(hipMemcpyAsync(&at[2 * j], d_offsets + redo[j], (d_lens ? 1 : 2) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        if (d_lens) HIPCHK(hipMemcpyAsync(&len[j], d_lens + redo[j], sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t j = 0; j < redo.size(); ++j) so[j + 1] = so[j] + (d_lens ? (uint64_t)len[j] : at[2 * j + 1] - at[2 * j]);
    std::vector<uint8_t> sb(so.back() ? so.back() : 1);
    for (size_t j = 0; j < redo.size(); ++j)
        if (so[j + 1] > so[j]) HIPCHK(hipMemcpyAsync(sb.data() + so[j], d_bytes + at[2 * j], (size_t)(so[j + 1] - so[j]), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return redo_relaunch(c, redo, sb, so, out);
}

// What a batch of n reads in `total` bytes needs of a context on its way through the host-buffer entry points: the page-locked side,
// scratch, device staging.
static int ctx_ensure_staging(mq_ctx *c, uint32_t n, uint64_t total, bool with_lens) {
    int rc;
    if ((rc = c->h_off.ensure((uint64_t)n + 1))) return rc;
    if ((rc = c->h_out.ensure((uint64_t)n))) return rc;
    if ((rc = ctx_ensure(c, n, total, list_f16(c->idx)))) return rc;
    if ((rc = c->st_bases.ensure(total + 64))) return rc;
    if ((rc = c->st_off.ensure((uint64_t)n + 1))) return rc;
    if ((rc = c->st_out.ensure((uint64_t)n))) return rc;
    return with_lens ? c->st_lens.ensure((uint64_t)n) : MQ_OK;
}

// One context runs one thing at a time: a batch or a piece that has been submitted is waited for before the next
static int ctx_require_idle(const mq_ctx *c) {
    if (c->pending || c->fx_kind != FxKind::None) return set_err(MQ_ESTATE, "context has a submitted batch: call mq_ctx_wait / mq_ctx_wait_fasta first");
    return MQ_OK;
}

// host buffers -> device staging -> launch sequence -> page-locked hits, all asynchronous on the context's stream.
// lens == nullptr: offsets has n + 1 entries and read i is bases[offsets[i], offsets[i+1]).  lens != nullptr (spans form): the
// whole buffer bases[0, buf_bytes) goes to the device and read i is bases[offsets[i], offsets[i] + lens[i]) (n offsets).
static int ctx_submit(mq_ctx *c, const uint8_t *bases, uint64_t buf_bytes, const uint64_t *offsets, const uint32_t *lens, uint32_t n,
                      mq_hit *out) {
    mq_index *idx = c->idx;
    int rc = ctx_require_idle(c);
    if (rc) return rc;
    if (!idx->finalized) return set_err(MQ_ESTATE, "index not finalized");
    if ((rc = outputs_admit(c, n))) return rc;
    if (n == 0) return MQ_OK;
    if ((rc = use_device(idx))) return rc;
    if ((rc = c->h_off.ensure((uint64_t)n + 1))) return rc;  // (ahead of the rest: the offsets are checked into it)
    uint64_t total, first;
    if (!lens) {
        first = offsets[0];
        total = offsets[n] - offsets[0];
        for (uint32_t i = 0; i < n; ++i) {
            if (offsets[i + 1] < offsets[i]) return set_err(MQ_EINVAL, "offsets must be non-decreasing");
            if (offsets[i + 1] - offsets[i] >= (1ull << 32)) return set_err(MQ_EINVAL, "sequence length must be < 2^32");
            c->h_off[i] = offsets[i] - first;
        }
    } else {
        first = 0;
        total = buf_bytes;
        uint64_t prev_end = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if (offsets[i] < prev_end || offsets[i] + lens[i] > buf_bytes) return set_err(MQ_EINVAL, "spans must be in order, disjoint and inside the buffer");
            prev_end = offsets[i] + lens[i];
            c->h_off[i] = offsets[i];
        }
    }
    c->h_off[n] = total;
    if ((rc = ctx_ensure_staging(c, n, total, lens != nullptr))) return rc;
    if (total) HIPCHK(hipMemcpyAsync(c->st_bases, bases + first, total, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->st_off, c->h_off, ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    LaunchOpt o;
    if (lens) {
        HIPCHK(hipMemcpyAsync(c->st_lens, lens, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        o.d_lens = c->st_lens;
    }
    rc = launch_map(c, c->st_bases, c->st_off, n, c->st_out, c->stream, o);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->h_out, c->st_out, (size_t)n * sizeof(mq_hit), hipMemcpyDeviceToHost, c->stream));
    c->pending = true;
    c->p_bases = bases;
    c->p_offsets = offsets;
    c->p_lens = lens;
    c->p_n = n;
    c->p_out = out;
    return MQ_OK;
}

static int ctx_wait(mq_ctx *c) {
    if (!c->pending) return MQ_OK;
    c->pending = false;
    int rc = use_device(c->idx);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(c->p_out, c->h_out, (size_t)c->p_n * sizeof(mq_hit));
    return redo_overflow(c, c->p_bases, c->p_offsets, c->p_lens, c->p_n, c->p_out);
}

// ---- the overflow redo of the device-resident form, in stream (mq_ctx_reserve_redo): the kernels of mq_redo.hpp around a launch sequence
// over the context's redo arena.  Everything is allocated at the reservation; a call queues and returns.

// max_reads == 0: the arena goes.  A failure leaves the context with the arena it had.
static int ctx_reserve_redo(mq_ctx *c, uint32_t max_reads, uint32_t max_read_len) {
    mq_index *idx = c->idx;
    int rc = ctx_require_idle(c);
    if (rc) return rc;
    if ((rc = use_device(idx))) return rc;
    if (max_reads == 0) {
        c->redo.reset();
        return MQ_OK;
    }
    if (max_read_len == 0) return set_err(MQ_EINVAL, "max_read_len must be positive");
    const uint64_t stride = ((uint64_t)max_read_len + 64u + 63u) & ~(uint64_t)63;
    // (list regions are placed at offset * f16 >> 16 with f16 = 65536: the arena's bytes times 2^16 must fit 64 bits)
    if (max_reads > WORK_ID_MASK || (uint64_t)max_reads * stride >= (1ull << 47)) return set_err(MQ_EINVAL, "max_reads x max_read_len is too large");
    if ((rc = ensure_geometry(idx))) return rc;
    std::unique_ptr<RedoArena> a(new RedoArena());
    a->max_reads = max_reads;
    a->max_read_len = max_read_len;
    a->stride = stride;
    a->cap = max_read_len;  // a read cannot have more runs than bases
    // no launch over max_reads reads has more workgroups than this, in either pipeline
    a->grid = std::min(redo_grid(idx, a->cap), (max_reads + (uint32_t)std::min(MAP_WAVES, ML_WAVES) - 1u) / (uint32_t)std::min(MAP_WAVES, ML_WAVES));
    a->sub.idx = idx;
    if ((rc = ctx_ensure(&a->sub, max_reads, (uint64_t)max_reads * stride, 65536u))) return rc;
    if ((rc = a->bases.alloc((uint64_t)max_reads * stride)) || (rc = a->offsets.alloc((uint64_t)max_reads + 1)) || (rc = a->lens.alloc(max_reads)) ||
        (rc = a->ids.alloc(max_reads)) || (rc = a->src.alloc(max_reads)) || (rc = a->hits.alloc(max_reads)) ||
        (rc = a->windows.alloc((uint64_t)a->grid * REDO_WAVES * a->cap)) || (rc = a->counters.alloc(1)) ||
        (c->chains.reads && (rc = a->chain_windows.alloc((uint64_t)a->grid * REDO_WAVES * chain_win_cap(a->cap)))))
        return rc;
    std::vector<uint64_t> slot_at((size_t)max_reads + 1);
    for (size_t j = 0; j <= max_reads; ++j) slot_at[j] = j * stride;
    HIPCHK(hipMemcpy(a->offsets, slot_at.data(), slot_at.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(a->bases, 0, (size_t)max_reads * stride));  // (the seeders look up to 64 bytes past a read's end, never into its result)
    HIPCHK(hipEventCreateWithFlags(&a->done.h, hipEventDisableTiming));
    c->redo = std::move(a);  // (the arena it had waits for its last launch and goes)
    return MQ_OK;
}

// Queued behind the launch sequence that wrote d_out, on the same stream: no allocation, no synchronisation, no hit read by the host
static int redo_in_stream(mq_ctx *c, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n, mq_hit *d_out, hipStream_t st) {
    RedoArena &a = *c->redo;
    a.last_n = n;
    if (n == 0) return MQ_OK;
    int rc;
    HIPCHK(hipMemsetAsync(a.counters, 0, sizeof(RedoCounters), st));
    HIPCHK(hipMemsetAsync(a.lens, 0, (size_t)a.max_reads * sizeof(uint32_t), st));  // a slot nobody claims is a read of length 0
    const bool outputs = (c->anchors.reads != 0 || c->chains.reads != 0) && !c->idx->split;
    if (outputs) HIPCHK(hipMemsetAsync(a.ids, 0xFF, (size_t)a.max_reads * sizeof(uint32_t), st));  // a slot nobody claims writes no span
    if ((rc = launch(redo_collect_kernel, (n + 255u) / 256u, 256, st, d_out, d_offsets, n, a.max_reads, a.max_read_len, a.counters, a.ids, a.src, a.lens))) return rc;
    if ((rc = launch(redo_copy_kernel, (a.max_reads + REDO_COPY_WAVES - 1u) / REDO_COPY_WAVES, 64 * REDO_COPY_WAVES, st, d_bases, a.src, a.lens, a.max_reads, a.bases, a.stride))) return rc;
    LaunchOpt o;
    o.scratch_override = a.windows;
    o.cap_override = a.cap;
    o.grid_override = a.grid;
    o.f16 = 65536u;
    o.d_lens = a.lens;
    // the arena's launch delivers to c's reservations; the slot-to-read array is its id map, and stream order makes the redo's span the read's final one
    o.outputs_of = c;
    o.redo = true;
    o.d_ids = a.ids;
    if (c->chains.reads) o.chain_windows_override = a.chain_windows;
    if ((rc = launch_map(&a.sub, a.bases, a.offsets, a.max_reads, a.hits, st, o))) return rc;
    if ((rc = launch(redo_scatter_kernel, (a.max_reads + 255u) / 256u, 256, st, a.hits, a.ids, a.counters, a.max_reads, d_out))) return rc;
    HIPCHK(hipEventRecord(a.done, st));
    a.ran = true;
    return MQ_OK;
}

// (redone, left) of the context's last device-form call, once its stream has passed the redo
static int ctx_redo_counts(mq_ctx *c, uint32_t *redone, uint32_t *left) {
    if (!c->redo) return set_err(MQ_ESTATE, "no redo arena reserved on this context: call mq_ctx_reserve_redo first");
    RedoArena &a = *c->redo;
    *redone = *left = 0;
    if (a.last_n == 0) return MQ_OK;  // no call yet, or one without reads
    int rc = use_device(c->idx);
    if (rc) return rc;
    HIPCHK(hipEventSynchronize(a.done));
    RedoCounters v;
    HIPCHK(hipMemcpy(&v, a.counters, sizeof(RedoCounters), hipMemcpyDeviceToHost));
    *redone = std::min(v.claimed, a.max_reads);
    *left = v.left;
    return MQ_OK;
}

// ---- the pooled outputs (PooledOutput, mq_host_state.hpp): the two operations that need the context's own

// A failure leaves the context with the reservation it had: everything is allocated into locals first.
template <class Item, class Span>
template <class Alloc, class Commit>
int PooledOutput<Item, Span>::reserve(mq_ctx *c, uint32_t max_reads, uint64_t max_entries, Alloc alloc_extra, Commit commit_extra) {
    mq_index *idx = c->idx;
    int rc = ctx_require_idle(c);
    if (rc) return rc;
    if ((rc = use_device(idx))) return rc;
    const bool release = max_reads == 0 && max_entries == 0;
    Buf<Item> new_pool;
    Buf<Span> new_spans;
    Buf<PoolCounters> new_counters;
    Buf<uint32_t> new_ids;
    PinnedBuf<Item> new_h_pool;
    PinnedBuf<Span> new_h_spans;
    PinnedBuf<PoolCounters> new_h_counters;
    hipEvent_t new_done = nullptr;
    if (!release) {
        const std::string max_noun = std::string("max_") + noun;
        if (max_reads == 0 || max_entries == 0) return set_err(MQ_EINVAL, "max_reads and " + max_noun + " must both be positive (or both 0: release)");
        if (max_reads > WORK_ID_MASK || max_entries >= 0xFFFFFFFFull) return set_err(MQ_EINVAL, "max_reads must be below 2^30 and " + max_noun + " below 2^32 - 1");
        if (idx->split)
            return set_err(MQ_EINVAL, std::string("the split pipeline (MQ_PIPELINE=split) writes no ") + noun + ": reserve them on an index that runs the fused kernels");
        if ((rc = ensure_outputs_geometry(idx))) return rc;
        if ((rc = new_pool.alloc(max_entries)) || (rc = new_spans.alloc(max_reads)) || (rc = new_counters.alloc(1)) || (rc = new_ids.alloc(max_reads)) ||
            (rc = alloc_extra()) || (rc = new_h_pool.alloc(max_entries)) || (rc = new_h_spans.alloc(max_reads)) || (rc = new_h_counters.alloc(1)))
            return rc;
        if (!done) HIPCHK(hipEventCreateWithFlags(&new_done, hipEventDisableTiming));
    }
    if (ran) (void)hipEventSynchronize(done);  // the stream of the last launch has passed the arrays that go
    pool = std::move(new_pool);
    spans = std::move(new_spans);
    counters = std::move(new_counters);
    ids = std::move(new_ids);
    commit_extra();
    h_pool = std::move(new_h_pool);
    h_spans = std::move(new_h_spans);
    h_counters = std::move(new_h_counters);
    if (new_done) done.h = new_done;
    reads = max_reads;
    cap = max_entries;
    ran = false;
    n = 0;
    return MQ_OK;
}

template <class Item, class Span>
int PooledOutput<Item, Span>::read_back(mq_ctx *c, const Span **out_spans, const Item **out_pool, uint32_t *n_reads, uint64_t *stored, uint64_t *needed,
                                        uint32_t *dropped_reads) {
    if (!reads) return require_reserved();
    if (c->fx_kind != FxKind::None) return set_err(MQ_ESTATE, "context has a submitted piece: call mq_ctx_wait_fasta first");
    int rc;
    if (c->pending && (rc = ctx_wait(c))) return rc;  // (the host-driven redo, which delivers the redone reads' items, runs there)
    *out_spans = h_spans;
    *out_pool = h_pool;
    *n_reads = 0;
    *stored = *needed = 0;
    *dropped_reads = 0;
    if (!ran || n == 0) return MQ_OK;  // no batch yet, or one without reads
    if ((rc = use_device(c->idx))) return rc;
    HIPCHK(hipEventSynchronize(done));
    HIPCHK(hipMemcpy(h_counters, counters, sizeof(PoolCounters), hipMemcpyDeviceToHost));
    const PoolCounters &v = *h_counters.p;
    const uint64_t have = std::min<uint64_t>(v.cursor, cap);
    HIPCHK(hipMemcpy(h_spans, spans, (size_t)n * sizeof(Span), hipMemcpyDeviceToHost));
    if (have) HIPCHK(hipMemcpy(h_pool, pool, (size_t)have * sizeof(Item), hipMemcpyDeviceToHost));
    *n_reads = n;
    *stored = have;
    *needed = v.cursor;
    *dropped_reads = v.dropped_reads;
    return MQ_OK;
}

static int ctx_reserve_anchors(mq_ctx *c, uint32_t max_reads, uint64_t max_anchors) {
    return c->anchors.reserve(c, max_reads, max_anchors, [] { return (int)MQ_OK; }, [] {});
}

// ... the chains bring the chain windows: the context's, and its redo arena's when it has one (an arena reserved later allocates its own:
// ctx_reserve_redo)
static int ctx_reserve_chains(mq_ctx *c, uint32_t max_reads, uint64_t max_chains) {
    mq_index *idx = c->idx;
    Buf<ChainRec> windows, arena_windows;
    return c->chains.reserve(
        c, max_reads, max_chains,
        [&]() -> int {
            int rc = windows.alloc((uint64_t)map_waves_for(idx, max_reads) * chain_win_cap(idx->cap_matches));
            if (!rc && c->redo) rc = arena_windows.alloc((uint64_t)c->redo->grid * REDO_WAVES * chain_win_cap(c->redo->cap));
            return rc;
        },
        [&] {
            c->chn_windows = std::move(windows);
            if (c->redo) c->redo->chain_windows = std::move(arena_windows);
        });
}

static int ctx_map_device(mq_ctx *c, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n, uint64_t total_bases, mq_hit *d_out,
                          hipStream_t st, bool instrumented = false) {
    mq_index *idx = c->idx;
    if (n && (!d_offsets || !d_out)) return set_err(MQ_EINVAL, "bad arguments");
    if (!idx->finalized) return set_err(MQ_ESTATE, "index not finalized");
    int rc = ctx_require_idle(c);
    if (rc) return rc;
    if ((rc = use_device(idx))) return rc;
    if (!instrumented && (rc = outputs_admit(c, n))) return rc;
    if ((rc = ctx_ensure(c, n, total_bases, list_f16(idx)))) return rc;
    LaunchOpt o;
    o.instrumented = instrumented;
    if ((rc = launch_map(c, d_bases, d_offsets, n, d_out, st, o))) return rc;
    // a context with a redo arena finishes its overflow reads behind the launch sequence (never for the instrumented, diagnostic launch)
    return c->redo && !instrumented ? redo_in_stream(c, d_bases, d_offsets, n, d_out, st) : MQ_OK;
}

// ---- device-parsed FASTX pieces: the raw bytes go to the device, a record scanner (mq_fastx.hpp, mq_fastx_lines.hpp) finds the records,
// map_kernel takes them from device memory.  Two steps, so that the host learns the number of records without standing in the stream's
// way: submit = copy + scan + the scan's result words back (all asynchronous); wait = read them, launch the map kernels, hits and side
// arrays back.  The copy of the NEXT piece (another context, another stream) runs meanwhile: the link stays busy.
static uint32_t fx_line_cap(uint64_t bytes) { return (uint32_t)std::min<uint64_t>(bytes / 16 + 4096, 1u << 28); }
// grid of the kernels that take a record per thread (at most fx_line_cap / 2 records)
static dim3 fx_record_grid(const mq_index *idx, uint32_t span_cap) { return dim3(std::max<uint32_t>(1, std::min<uint32_t>(span_cap / 256 + 1, (uint32_t)idx->n_cu * 4u))); }

// MQ_FASTX_FASTA_LINES only: the joined bytes (at most the piece's own) and the header spans of a piece of `bytes` bytes.  A context that
// never sees the format never has them: mq_ctx_reserve sizes them only once a LINES piece has been submitted on the context.
static int ctx_ensure_lines(mq_ctx *c, uint64_t bytes) {
    const uint64_t cap = fx_line_cap(bytes) / 2;
    int rc;
    if ((rc = c->fl_joined.ensure(bytes + 64))) return rc;
    if ((rc = c->fl_hb.ensure(cap + 1))) return rc;
    return c->fl_he.ensure(cap + 1);
}

// buf[0, bytes) to st_bases (which holds it), asynchronously.  The bytes behind the last page boundary (< 4 KB) go through a page-locked
// buffer of the context: a caller that page-locks the whole pages of its pieces (the feeder, on a mapped file: mq_host_register) gets
// an asynchronous copy for all the rest, and the last partial page -- which may belong to a range somebody else locks and releases --
// is never the source of a DMA.
static int fx_stage_piece(mq_ctx *c, const uint8_t *buf, uint64_t bytes) {
    int rc;
    if (!bytes) return MQ_OK;
    const uintptr_t cut = ((uintptr_t)buf + bytes) & ~(uintptr_t)4095;
    const uint64_t main_len = cut > (uintptr_t)buf ? (uint64_t)(cut - (uintptr_t)buf) : 0, tail_len = bytes - main_len;
    if (!c->h_fx_tail && (rc = c->h_fx_tail.alloc(4096))) return rc;
    if (main_len) HIPCHK(hipMemcpyAsync(c->st_bases, buf, main_len, hipMemcpyHostToDevice, c->stream));
    if (tail_len) {
        memcpy(c->h_fx_tail, buf + main_len, tail_len);
        HIPCHK(hipMemcpyAsync(c->st_bases + main_len, c->h_fx_tail, tail_len, hipMemcpyHostToDevice, c->stream));
    }
    return MQ_OK;
}

// Records of one sequence line in st_bases[b, e) (FASTA: 2 lines, FASTQ: 4): line ends to fx_nl, spans to st_off / st_lens, FxRecords to fx_info
static void fx_find_records(mq_ctx *c, FxKind kind, uint32_t b, uint32_t e, uint32_t n_tiles) {
    const uint32_t cap = fx_line_cap(e), grid = fx_grid(c->idx, n_tiles);
    hipLaunchKernelGGL(count_newlines_kernel, dim3(grid), dim3(256), 0, c->stream, c->st_bases, b, e, n_tiles, c->fx_tile_counts);
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(1024), 0, c->stream, c->st_bases, b, e, c->fx_tile_counts, n_tiles, c->fx_tile_off, c->fx_nl, cap, c->fx_info.p->words, kind == FxKind::Fastq ? 4u : 2u);
    hipLaunchKernelGGL(list_newlines_kernel, dim3(grid), dim3(256), 0, c->stream, c->st_bases, b, e, n_tiles, c->fx_tile_off, c->fx_nl, cap);
    const auto spans_kernel = kind == FxKind::Fastq ? fastq_spans_kernel : fasta_spans_kernel;
    hipLaunchKernelGGL(spans_kernel, fx_record_grid(c->idx, cap / 2), dim3(256), 0, c->stream, c->st_bases, b, e, c->fx_nl, c->fx_info.p->words, reinterpret_cast<unsigned long long *>(c->st_off.p), c->st_lens, cap / 2);
}

// MQ_FASTX_FASTA_LINES: joined sequences to fl_joined, header spans to fl_hb / fl_he, their offsets / lengths to st_off / st_lens, FxJoined to fx_info
static void fx_join_records(mq_ctx *c, uint32_t b, uint32_t e, uint32_t n_tiles) {
    const uint32_t cap = fx_line_cap(e), grid = fx_grid(c->idx, n_tiles);
    unsigned long long *offs = reinterpret_cast<unsigned long long *>(c->st_off.p);
    hipLaunchKernelGGL(fl_count_kernel, dim3(grid), dim3(256), 0, c->stream, c->st_bases, b, e, n_tiles, c->fx_tile_counts);
    hipLaunchKernelGGL(fl_scan_kernel, dim3(1), dim3(1024), 0, c->stream, c->st_bases, b, e, c->fx_tile_counts, n_tiles, c->fx_tile_off, offs, c->fl_he, cap / 2, c->fx_info.p->words);
    hipLaunchKernelGGL(fl_write_kernel, dim3(grid), dim3(256), 0, c->stream, c->st_bases, b, e, n_tiles, c->fx_tile_off, c->fx_info.p->words, c->fl_joined, c->fl_hb, c->fl_he, offs, cap / 2);
    hipLaunchKernelGGL(fl_check_kernel, fx_record_grid(c->idx, cap / 2), dim3(256), 0, c->stream, offs, c->st_lens, c->fx_info.p->words);
}

static int ctx_submit_fasta(mq_ctx *c, const uint8_t *buf, uint64_t begin, uint64_t bytes, uint32_t format) {
    mq_index *idx = c->idx;
    int rc = ctx_require_idle(c);
    if (rc) return rc;
    if (!idx->finalized) return set_err(MQ_ESTATE, "index not finalized");
    if (bytes >= (1ull << 32) || begin > bytes) return set_err(MQ_EINVAL, "a chunk must be smaller than 4 GB");
    const FxKind kind = format == MQ_FASTX_FASTA ? FxKind::Fasta : format == MQ_FASTX_FASTQ ? FxKind::Fastq : format == MQ_FASTX_FASTA_LINES ? FxKind::FastaLines : FxKind::None;
    if (kind == FxKind::None) return set_err(MQ_EINVAL, "format must be MQ_FASTX_FASTA, MQ_FASTX_FASTQ or MQ_FASTX_FASTA_LINES");
    if ((rc = use_device(idx))) return rc;
    const bool wrapped = kind == FxKind::FastaLines;  // (four counts and three offsets per tile, no line-end list); every ensure runs before anything is queued
    const uint32_t b = (uint32_t)begin, e = (uint32_t)bytes, n_tiles = (uint32_t)((bytes + FX_TILE - 1) / FX_TILE), cap = fx_line_cap(bytes);
    if ((rc = c->st_bases.ensure(bytes + 64))) return rc;
    if ((rc = c->fx_tile_counts.ensure(((uint64_t)n_tiles + 1) * (wrapped ? 4u : 1u)))) return rc;
    if ((rc = c->fx_tile_off.ensure(((uint64_t)n_tiles + 1) * (wrapped ? 3u : 1u)))) return rc;
    if (wrapped) c->fl_used = true;
    if ((rc = wrapped ? ctx_ensure_lines(c, bytes) : c->fx_nl.ensure(cap))) return rc;
    if ((rc = c->st_off.ensure((uint64_t)cap / 2 + 1))) return rc;
    if ((rc = c->st_lens.ensure((uint64_t)cap / 2 + 1))) return rc;
    if ((!c->fx_info && (rc = c->fx_info.alloc(1))) || (!c->h_fx_info && (rc = c->h_fx_info.alloc(1)))) return rc;
    if ((rc = fx_stage_piece(c, buf, bytes))) return rc;
    if (wrapped) fx_join_records(c, b, e, n_tiles);
    else fx_find_records(c, kind, b, e, n_tiles);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_fx_info, c->fx_info, sizeof(FxResult), hipMemcpyDeviceToHost, c->stream));
    c->fx_kind = kind;  // (the one place a piece becomes pending)
    c->fx_bytes = e;
    return MQ_OK;
}

// The piece in flight is finished: its scanner's result is in h_fx_info when this returns MQ_OK
static int fx_take_info(mq_ctx *c) {
    c->fx_kind = FxKind::None;
    int rc = use_device(c->idx);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return MQ_OK;
}

// The map kernels on the n records a scanner found (read r: d_lens[r] bytes at d_bytes + d_offsets[r]; d_lens == nullptr: up to d_offsets[r + 1]),
// the hits back in h_out, side_copies() -- the caller's own arrays, queued behind the hit copy -- and overflowing reads redone
template <typename F>
static int fx_map_found(mq_ctx *c, const uint8_t *d_bytes, const uint64_t *d_offsets, const uint32_t *d_lens, uint32_t n, uint64_t total_bytes, F side_copies) {
    int rc;
    if ((rc = outputs_admit(c, n))) return rc;
    if ((rc = c->h_out.ensure((uint64_t)n))) return rc;
    if ((rc = c->st_out.ensure((uint64_t)n))) return rc;
    if ((rc = ctx_ensure(c, n, total_bytes, list_f16(c->idx)))) return rc;
    if (getenv("MQ_FX_POISON_HITS")) HIPCHK(hipMemsetAsync(c->st_out, 0xFF, (size_t)n * sizeof(mq_hit), c->stream));  // test hook: a record no wave writes shows
    LaunchOpt o;
    o.d_lens = d_lens;
    if ((rc = launch_map(c, d_bytes, d_offsets, n, c->st_out, c->stream, o))) return rc;
    HIPCHK(hipMemcpyAsync(c->h_out, c->st_out, (size_t)n * sizeof(mq_hit), hipMemcpyDeviceToHost, c->stream));
    if ((rc = side_copies())) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return redo_overflow_device(c, d_bytes, d_offsets, d_lens, n, c->h_out);
}

static int ctx_wait_fasta(mq_ctx *c, uint32_t *n_reads, const uint32_t **line_ends, uint32_t *n_lines, const mq_hit **hits, uint32_t *flags) {
    if (c->fx_kind == FxKind::None) return set_err(MQ_ESTATE, "no FASTA chunk submitted on this context");
    if (c->fx_kind == FxKind::FastaLines) return set_err(MQ_ESTATE, "the submitted piece is MQ_FASTX_FASTA_LINES: call mq_ctx_wait_fasta_lines");
    int rc = fx_take_info(c);
    if (rc) return rc;
    const FxRecords &res = c->h_fx_info.p->one;
    const uint32_t lines = res.lines, n = res.records;
    *flags = res.flags;
    *n_reads = *n_lines = 0;
    *line_ends = nullptr;
    *hits = nullptr;
    if ((*flags & FX_IRREGULAR) || n == 0) return MQ_OK;  // irregular (not "header line, sequence line" all through): the caller parses this chunk on the host
    if ((rc = c->h_fx_nl.ensure((uint64_t)lines))) return rc;
    rc = fx_map_found(c, c->st_bases, c->st_off, c->st_lens, n, c->fx_bytes, [&]() -> int {
        HIPCHK(hipMemcpyAsync(c->h_fx_nl, c->fx_nl, (size_t)lines * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        return MQ_OK;
    });
    if (rc) return rc;
    *n_reads = n;
    *n_lines = lines;
    *line_ends = c->h_fx_nl;
    *hits = c->h_out;
    return MQ_OK;
}

// MQ_FASTX_FASTA_LINES: the map kernels on (joined bytes, offsets) -- the device form, no lengths; hits, header spans, joined lengths back
static int ctx_wait_fasta_lines(mq_ctx *c, uint32_t *n_reads, const uint32_t **hdr_begin, const uint32_t **hdr_end, const uint32_t **seq_lens,
                                const mq_hit **hits, uint32_t *flags) {
    if (c->fx_kind != FxKind::FastaLines) return set_err(MQ_ESTATE, "no MQ_FASTX_FASTA_LINES piece submitted on this context");
    int rc = fx_take_info(c);
    if (rc) return rc;
    const FxJoined &res = c->h_fx_info.p->lines;
    const uint32_t n = res.records, joined = res.joined;
    *flags = res.flags;
    *n_reads = 0;
    *hdr_begin = *hdr_end = *seq_lens = nullptr;
    *hits = nullptr;
    if ((*flags & FX_IRREGULAR) || n == 0) return MQ_OK;  // irregular: the caller parses this piece on the host
    if ((rc = c->h_fl_hb.ensure((uint64_t)n))) return rc;
    if ((rc = c->h_fl_he.ensure((uint64_t)n))) return rc;
    if ((rc = c->h_fl_lens.ensure((uint64_t)n))) return rc;
    rc = fx_map_found(c, c->fl_joined, c->st_off, nullptr, n, joined, [&]() -> int {
        HIPCHK(hipMemcpyAsync(c->h_fl_hb, c->fl_hb, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(c->h_fl_he, c->fl_he, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(c->h_fl_lens, c->st_lens, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        return MQ_OK;
    });
    if (rc) return rc;
    *n_reads = n;
    *hdr_begin = c->h_fl_hb;
    *hdr_end = c->h_fl_he;
    *seq_lens = c->h_fl_lens;
    *hits = c->h_out;
    return MQ_OK;
}

extern "C" {

int mq_ctx_submit_fasta(mq_ctx *ctx, const uint8_t *buf, uint64_t begin, uint64_t bytes) {
    return guarded([&]() -> int {
        if (!ctx || (bytes && !buf)) return set_err(MQ_EINVAL, "bad arguments");
        return ctx_submit_fasta(ctx, buf, begin, bytes, MQ_FASTX_FASTA);
    });
}

int mq_ctx_submit_fastx(mq_ctx *ctx, const uint8_t *buf, uint64_t begin, uint64_t bytes, uint32_t format) {
    return guarded([&]() -> int {
        if (!ctx || (bytes && !buf)) return set_err(MQ_EINVAL, "bad arguments");
        return ctx_submit_fasta(ctx, buf, begin, bytes, format);
    });
}

int mq_ctx_wait_fasta(mq_ctx *ctx, uint32_t *n_reads, const uint32_t **line_ends, uint32_t *n_lines, const mq_hit **hits, uint32_t *flags) {
    return guarded([&]() -> int {
        if (!ctx || !n_reads || !line_ends || !n_lines || !hits || !flags) return set_err(MQ_EINVAL, "bad arguments");
        return ctx_wait_fasta(ctx, n_reads, line_ends, n_lines, hits, flags);
    });
}

int mq_ctx_wait_fasta_lines(mq_ctx *ctx, uint32_t *n_reads, const uint32_t **hdr_begin, const uint32_t **hdr_end, const uint32_t **seq_lens,
                            const mq_hit **hits, uint32_t *flags) {
    return guarded([&]() -> int {
        if (!ctx || !n_reads || !hdr_begin || !hdr_end || !seq_lens || !hits || !flags) return set_err(MQ_EINVAL, "bad arguments");
        return ctx_wait_fasta_lines(ctx, n_reads, hdr_begin, hdr_end, seq_lens, hits, flags);
    });
}

mq_ctx *mq_ctx_new(mq_index *idx) {
    return guarded([&]() -> mq_ctx * {
        if (!idx) {
            set_err(MQ_EINVAL, "idx is NULL");
            return nullptr;
        }
        mq_ctx *c = ctx_create(idx);
        if (c) {
            std::lock_guard<std::mutex> lk(idx->ctx_mu);
            idx->ctxs.push_back(c);
        }
        return c;
    });
}

void mq_ctx_free(mq_ctx *ctx) {
    if (!ctx) return;
    {
        std::lock_guard<std::mutex> lk(ctx->idx->ctx_mu);
        auto &v = ctx->idx->ctxs;
        v.erase(std::remove(v.begin(), v.end(), ctx), v.end());
    }
    hipSetDevice(ctx->idx->device);
    ctx_release(ctx);
}

int mq_ctx_submit(mq_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint32_t n, mq_hit *out) {
    return guarded([&]() -> int {
        if (!ctx || (n && (!offsets || !out))) return set_err(MQ_EINVAL, "bad arguments");
        return ctx_submit(ctx, bases, 0, offsets, nullptr, n, out);
    });
}

int mq_ctx_submit_spans(mq_ctx *ctx, const uint8_t *buf, uint64_t buf_bytes, const uint64_t *starts, const uint32_t *lens, uint32_t n,
                        mq_hit *out) {
    return guarded([&]() -> int {
        if (!ctx || (n && (!buf || !starts || !lens || !out))) return set_err(MQ_EINVAL, "bad arguments");
        return ctx_submit(ctx, buf, buf_bytes, starts, lens, n, out);
    });
}

int mq_ctx_reserve(mq_ctx *ctx, uint32_t n_reads, uint64_t total_bytes) {
    return guarded([&]() -> int {
        if (!ctx) return set_err(MQ_EINVAL, "ctx is NULL");
        int rc = use_device(ctx->idx);
        if (rc) return rc;
        if ((rc = ctx_ensure_staging(ctx, n_reads, total_bytes, true))) return rc;
        return ctx->fl_used ? ctx_ensure_lines(ctx, total_bytes) : MQ_OK;  // (a context that never saw a LINES piece does not pay for its buffers)
    });
}

int mq_ctx_wait(mq_ctx *ctx) {
    return guarded([&]() -> int {
        if (!ctx) return set_err(MQ_EINVAL, "ctx is NULL");
        return ctx_wait(ctx);
    });
}

int mq_ctx_map_batch(mq_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint32_t n, mq_hit *out) {
    return guarded([&]() -> int {
        if (!ctx || (n && (!offsets || !out))) return set_err(MQ_EINVAL, "bad arguments");
        int rc = ctx_submit(ctx, bases, 0, offsets, nullptr, n, out);
        if (rc) return rc;
        return ctx_wait(ctx);
    });
}

int mq_ctx_map_batch_device(mq_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n, uint64_t total_bases,
                            mq_hit *d_out, void *stream) {
    return guarded([&]() -> int {
        if (!ctx) return set_err(MQ_EINVAL, "ctx is NULL");
        return ctx_map_device(ctx, d_bases, d_offsets, n, total_bases, d_out, (hipStream_t)stream);
    });
}

int mq_map_reserve(mq_index *idx, uint32_t n_reads, uint64_t total_bases) {
    return guarded([&]() -> int {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        std::lock_guard<std::mutex> lk(idx->mu);
        int rc = use_device(idx);
        if (rc) return rc;
        return ctx_ensure(idx->def_ctx.get(), n_reads, total_bases, list_f16(idx));
    });
}

int mq_map_batch_device(mq_index *idx, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n, uint64_t total_bases,
                        mq_hit *d_out, void *stream) {
    return guarded([&]() -> int {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        std::lock_guard<std::mutex> lk(idx->mu);
        return ctx_map_device(idx->def_ctx.get(), d_bases, d_offsets, n, total_bases, d_out, (hipStream_t)stream);
    });
}

int mq_ctx_reserve_redo(mq_ctx *ctx, uint32_t max_reads, uint32_t max_read_len) {
    return guarded([&]() -> int {
        if (!ctx) return set_err(MQ_EINVAL, "ctx is NULL");
        return ctx_reserve_redo(ctx, max_reads, max_read_len);
    });
}

int mq_map_reserve_redo(mq_index *idx, uint32_t max_reads, uint32_t max_read_len) {
    return guarded([&]() -> int {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        std::lock_guard<std::mutex> lk(idx->mu);
        return ctx_reserve_redo(idx->def_ctx.get(), max_reads, max_read_len);
    });
}

int mq_ctx_redo_counts(mq_ctx *ctx, uint32_t *redone, uint32_t *left) {
    return guarded([&]() -> int {
        if (!ctx || !redone || !left) return set_err(MQ_EINVAL, "bad arguments");
        return ctx_redo_counts(ctx, redone, left);
    });
}

int mq_map_redo_counts(mq_index *idx, uint32_t *redone, uint32_t *left) {
    return guarded([&]() -> int {
        if (!idx || !redone || !left) return set_err(MQ_EINVAL, "bad arguments");
        std::lock_guard<std::mutex> lk(idx->mu);
        return ctx_redo_counts(idx->def_ctx.get(), redone, left);
    });
}

int mq_ctx_reserve_anchors(mq_ctx *ctx, uint32_t max_reads, uint64_t max_anchors) {
    return guarded([&]() -> int {
        if (!ctx) return set_err(MQ_EINVAL, "ctx is NULL");
        return ctx_reserve_anchors(ctx, max_reads, max_anchors);
    });
}

int mq_map_reserve_anchors(mq_index *idx, uint32_t max_reads, uint64_t max_anchors) {
    return guarded([&]() -> int {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        std::lock_guard<std::mutex> lk(idx->mu);
        return ctx_reserve_anchors(idx->def_ctx.get(), max_reads, max_anchors);
    });
}

int mq_ctx_anchors(mq_ctx *ctx, const mq_anchor_span **spans, const mq_anchor **anchors, uint32_t *n_reads, uint64_t *stored, uint64_t *needed,
                   uint32_t *dropped_reads) {
    return guarded([&]() -> int {
        if (!ctx || !spans || !anchors || !n_reads || !stored || !needed || !dropped_reads) return set_err(MQ_EINVAL, "bad arguments");
        return ctx->anchors.read_back(ctx, spans, anchors, n_reads, stored, needed, dropped_reads);
    });
}

int mq_map_anchors(mq_index *idx, const mq_anchor_span **spans, const mq_anchor **anchors, uint32_t *n_reads, uint64_t *stored, uint64_t *needed,
                   uint32_t *dropped_reads) {
    return guarded([&]() -> int {
        if (!idx || !spans || !anchors || !n_reads || !stored || !needed || !dropped_reads) return set_err(MQ_EINVAL, "bad arguments");
        std::lock_guard<std::mutex> lk(idx->mu);
        return idx->def_ctx->anchors.read_back(idx->def_ctx.get(), spans, anchors, n_reads, stored, needed, dropped_reads);
    });
}

int mq_ctx_anchors_device(mq_ctx *ctx, const mq_anchor_span **d_spans, const mq_anchor **d_anchors) {
    return guarded([&]() -> int {
        if (!ctx || !d_spans || !d_anchors) return set_err(MQ_EINVAL, "bad arguments");
        return ctx->anchors.device_pointers(d_spans, d_anchors);
    });
}

int mq_ctx_reserve_chains(mq_ctx *ctx, uint32_t max_reads, uint64_t max_chains) {
    return guarded([&]() -> int {
        if (!ctx) return set_err(MQ_EINVAL, "ctx is NULL");
        return ctx_reserve_chains(ctx, max_reads, max_chains);
    });
}

int mq_map_reserve_chains(mq_index *idx, uint32_t max_reads, uint64_t max_chains) {
    return guarded([&]() -> int {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        std::lock_guard<std::mutex> lk(idx->mu);
        return ctx_reserve_chains(idx->def_ctx.get(), max_reads, max_chains);
    });
}

int mq_ctx_chains(mq_ctx *ctx, const mq_chain_span **spans, const mq_chain **chains, uint32_t *n_reads, uint64_t *stored, uint64_t *needed,
                  uint32_t *dropped_reads) {
    return guarded([&]() -> int {
        if (!ctx || !spans || !chains || !n_reads || !stored || !needed || !dropped_reads) return set_err(MQ_EINVAL, "bad arguments");
        return ctx->chains.read_back(ctx, spans, chains, n_reads, stored, needed, dropped_reads);
    });
}

int mq_map_chains(mq_index *idx, const mq_chain_span **spans, const mq_chain **chains, uint32_t *n_reads, uint64_t *stored, uint64_t *needed,
                  uint32_t *dropped_reads) {
    return guarded([&]() -> int {
        if (!idx || !spans || !chains || !n_reads || !stored || !needed || !dropped_reads) return set_err(MQ_EINVAL, "bad arguments");
        std::lock_guard<std::mutex> lk(idx->mu);
        return idx->def_ctx->chains.read_back(idx->def_ctx.get(), spans, chains, n_reads, stored, needed, dropped_reads);
    });
}

int mq_ctx_chains_device(mq_ctx *ctx, const mq_chain_span **d_spans, const mq_chain **d_chains) {
    return guarded([&]() -> int {
        if (!ctx || !d_spans || !d_chains) return set_err(MQ_EINVAL, "bad arguments");
        return ctx->chains.device_pointers(d_spans, d_chains);
    });
}

int mq_map_batch(mq_index *idx, const uint8_t *bases, const uint64_t *offsets, uint32_t n, mq_hit *out) {
    return guarded([&]() -> int {
        if (!idx || (n && (!offsets || !out))) return set_err(MQ_EINVAL, "bad arguments");
        std::lock_guard<std::mutex> lk(idx->mu);
        int rc = ctx_submit(idx->def_ctx.get(), bases, 0, offsets, nullptr, n, out);
        if (rc) return rc;
        return ctx_wait(idx->def_ctx.get());
    });
}

int mq_kminmers_batch(mq_index *idx, const uint8_t *bases, const uint64_t *offsets, uint32_t n, const uint64_t *kmm_offsets,
                      mq_kminmer *out, uint32_t *counts) {
    return guarded([&]() -> int {
        if (!idx || (n && (!offsets || !kmm_offsets || !counts))) return set_err(MQ_EINVAL, "bad arguments");
        if (n == 0) return MQ_OK;
        std::lock_guard<std::mutex> lk(idx->mu);
        int rc = use_device(idx);
        if (rc) return rc;
        const uint64_t total = offsets[n] - offsets[0];
        const uint64_t ktotal = kmm_offsets[n] - kmm_offsets[0];
        for (uint32_t i = 0; i < n; ++i)
            if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] >= (1ull << 32)) return set_err(MQ_EINVAL, "bad offsets / sequence length must be < 2^32");
        // parity/debug entry point: list regions sized for the worst case (one minimizer per base), so no sequence overflows
        rc = ctx_ensure(idx->def_ctx.get(), n, total, 65536u);
        if (rc) return rc;
        Buf<uint8_t> d_b;
        Buf<uint64_t> d_o, d_ko;
        Buf<mq_kminmer> d_k;
        Buf<uint32_t> d_c;
        Buf<mq_hit> d_h;
        std::vector<uint64_t> rel((size_t)n + 1), krel((size_t)n + 1);
        for (uint32_t i = 0; i <= n; ++i) {
            rel[i] = offsets[i] - offsets[0];
            krel[i] = kmm_offsets[i] - kmm_offsets[0];
        }
        hipError_t e = hipSuccess;
        auto ok = [&](hipError_t x) { if (e == hipSuccess) e = x; return e == hipSuccess; };
        ok(d_b.try_alloc(total + 1));
        ok(d_o.try_alloc((uint64_t)n + 1));
        ok(d_ko.try_alloc((uint64_t)n + 1));
        ok(d_k.try_alloc(ktotal + 1));
        ok(d_c.try_alloc(n));
        ok(d_h.try_alloc(n));
        if (e == hipSuccess && total) ok(hipMemcpy(d_b, bases + offsets[0], total, hipMemcpyHostToDevice));
        if (e == hipSuccess) ok(hipMemcpy(d_o, rel.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
        if (e == hipSuccess) ok(hipMemcpy(d_ko, krel.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
        if (e != hipSuccess) return set_err(MQ_EHIP, std::string("mq_kminmers_batch setup: ") + hipGetErrorString(e));
        // before finalize there is no ref table: the 1-slot empty table never hits, so ref_lens is never read
        {
            LaunchOpt o;
            o.d_dump = d_k;
            o.d_dump_off = d_ko;
            o.d_dump_counts = d_c;
            o.f16 = 65536u;
            rc = launch_map(idx->def_ctx.get(), d_b, d_o, n, d_h, 0, o);
        }
        if (rc) return rc;
        ok(hipMemcpy(counts, d_c, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (e == hipSuccess && ktotal && out) ok(hipMemcpy(out + kmm_offsets[0], d_k, ktotal * sizeof(mq_kminmer), hipMemcpyDeviceToHost));
        if (e != hipSuccess) return set_err(MQ_EHIP, std::string("mq_kminmers_batch copy-out: ") + hipGetErrorString(e));
        return MQ_OK;
    });
}

int mq_index_lookup(mq_index *idx, const uint64_t *hashes, uint32_t n, uint8_t *found, mq_kminmer *entries, uint32_t *ref_ids) {
    return guarded([&]() -> int {
        if (!idx || (n && (!hashes || !found || !entries || !ref_ids))) return set_err(MQ_EINVAL, "bad arguments");
        if (!idx->finalized) return set_err(MQ_ESTATE, "index not finalized");
        if (n == 0) return MQ_OK;
        std::lock_guard<std::mutex> lk(idx->mu);
        int rc = use_device(idx);
        if (rc) return rc;
        Buf<uint64_t> d_k;
        Buf<uint8_t> d_f;
        Buf<mq_kminmer> d_e;
        Buf<uint32_t> d_r;
        hipError_t e = hipSuccess;
        auto ok = [&](hipError_t x) { if (e == hipSuccess) e = x; return e == hipSuccess; };
        ok(d_k.try_alloc(n));
        ok(d_f.try_alloc(n));
        ok(d_e.try_alloc(n));
        ok(d_r.try_alloc(n));
        if (e == hipSuccess) ok(hipMemcpy(d_k, hashes, (size_t)n * 8, hipMemcpyHostToDevice));
        if (e == hipSuccess) {
            hipLaunchKernelGGL(lookup_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, idx->table, idx->nslots - 1, d_k, n, d_f, d_e, d_r);
            ok(hipGetLastError());
        }
        if (e == hipSuccess) ok(hipMemcpy(found, d_f, (size_t)n, hipMemcpyDeviceToHost));
        if (e == hipSuccess) ok(hipMemcpy(entries, d_e, (size_t)n * sizeof(mq_kminmer), hipMemcpyDeviceToHost));
        if (e == hipSuccess) ok(hipMemcpy(ref_ids, d_r, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (e != hipSuccess) return set_err(MQ_EHIP, std::string("mq_index_lookup: ") + hipGetErrorString(e));
        return MQ_OK;
    });
}

int mq_format_paf(const mq_index *idx, const char *q_id, uint64_t q_len, const mq_hit *hit, char *buf, size_t cap) {
    return guarded([&]() -> int {
        if (!idx || !q_id || !hit || !buf) return set_err(MQ_EINVAL, "bad arguments");
        if (hit->status != MQ_HIT_MAPPED) return set_err(MQ_EINVAL, "hit is not mapped: the reference writes no line");
        auto it = idx->refs.find(hit->ref_id);
        if (it == idx->refs.end()) return set_err(MQ_EINVAL, "unknown ref_id in hit");
        const unsigned long long r_len = it->second.second;
        // src/mers.rs:181: column 11 repeats r_len, column 10 is the score
        const unsigned long long qs = ((unsigned long long)hit->q_start_hi << 32) | hit->q_start, qe = ((unsigned long long)hit->q_end_hi << 32) | hit->q_end;
        int w = snprintf(buf, cap, "%s\t%llu\t%llu\t%llu\t%s\t%s\t%llu\t%u\t%u\t%u\t%llu\t%u", q_id, (unsigned long long)q_len, qs, qe,
                         hit->rc ? "-" : "+", it->second.first.c_str(), r_len, hit->r_start, hit->r_end, hit->score, r_len,
                         hit->mapq);
        return w;
    });
}

int mq_format_paf_chain(const mq_index *idx, const char *q_id, uint64_t q_len, const mq_chain *chain, char *buf, size_t cap) {
    return guarded([&]() -> int {
        if (!idx || !q_id || !chain || !buf) return set_err(MQ_EINVAL, "bad arguments");
        auto it = idx->refs.find(chain->ref_id);
        if (it == idx->refs.end()) return set_err(MQ_EINVAL, "unknown ref_id in chain");
        const unsigned long long r_len = it->second.second;
        // the columns of mq_format_paf, from the words the two records share
        const unsigned long long qs = ((unsigned long long)chain->q_start_hi << 32) | chain->q_start, qe = ((unsigned long long)chain->q_end_hi << 32) | chain->q_end;
        return snprintf(buf, cap, "%s\t%llu\t%llu\t%llu\t%s\t%s\t%llu\t%u\t%u\t%u\t%llu\t%u", q_id, (unsigned long long)q_len, qs, qe,
                        chain->rc ? "-" : "+", it->second.first.c_str(), r_len, chain->r_start, chain->r_end, chain->score, r_len, chain->mapq);
    });
}

// Page-locked host memory.  hipHostMalloc pins at ~4 GB/s on this platform (and hipHostFree costs another 0.14 s per GB), which
// made the feeder's chunk pool the start-up cost of the read phase; an anonymous mapping backed by transparent huge pages,
// touched and then registered, is page-locked at ~15 GB/s and copies to the device at the full PCIe rate
// (tools/pin_rate.hip, profiles/r03_pin_rate.txt).  Falls back to hipHostMalloc when the mapping or the registration fails.
namespace {
std::mutex g_host_mu;
std::map<void *, std::pair<size_t, bool>> g_host_allocs;  // pointer -> (mapped bytes, true: mmap + hipHostRegister)
}  // namespace

void *mq_host_alloc(size_t bytes) {
    if (!bytes) bytes = 1;
    const size_t huge = 2u << 20;
    const size_t mapped = (bytes + huge - 1) / huge * huge;
    void *p = mmap(nullptr, mapped, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (p != MAP_FAILED) {
        madvise(p, mapped, MADV_HUGEPAGE);
        for (size_t o = 0; o < mapped; o += 4096) ((volatile uint8_t *)p)[o] = 0;  // fault the pages in (2 MB at a time under THP)
        if (hipHostRegister(p, mapped, hipHostRegisterPortable) == hipSuccess) {  // portable: a feeder's chunk goes to whichever GPU's worker takes it
            std::lock_guard<std::mutex> lk(g_host_mu);
            g_host_allocs[p] = std::make_pair(mapped, true);
            return p;
        }
        (void)hipGetLastError();
        munmap(p, mapped);
    }
    p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocPortable);
    if (e != hipSuccess) {
        set_err(e == hipErrorOutOfMemory ? MQ_ENOMEM : MQ_EHIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(g_host_mu);
    g_host_allocs[p] = std::make_pair(bytes, false);
    return p;
}

// Page-lock a range the caller owns (a slice of a mapped file: the copy to the device then runs by DMA straight out of the page cache,
// asynchronously, at the link's rate -- tools/file_h2d.hip).  ptr and bytes whole pages.  0 on success.
int mq_host_register(void *ptr, size_t bytes) {
    if (!ptr || !bytes) return set_err(MQ_EINVAL, "bad arguments");
    const hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterPortable);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_err(MQ_EHIP, std::string("hipHostRegister: ") + hipGetErrorString(e));
    }
    return MQ_OK;
}
int mq_host_unregister(void *ptr) {
    if (!ptr) return MQ_OK;
    const hipError_t e = hipHostUnregister(ptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_err(MQ_EHIP, std::string("hipHostUnregister: ") + hipGetErrorString(e));
    }
    return MQ_OK;
}

void mq_host_free(void *p) {
    if (!p) return;
    std::pair<size_t, bool> info(0, false);
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        auto it = g_host_allocs.find(p);
        if (it == g_host_allocs.end()) return;  // not ours
        info = it->second;
        g_host_allocs.erase(it);
    }
    if (info.second) {
        hipHostUnregister(p);
        munmap(p, info.first);
    } else {
        hipHostFree(p);
    }
}

}  // extern "C"
