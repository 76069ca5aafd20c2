// ctx_fill.hip -- the fill dispatcher: one batch of omegas -> which kernels, in which order, with which chunk tables
// (matrixAssembler, include/solver.h:417-515, batched over omega).  The decisions that need no device are taken by
// fill_plan.cpp; this file turns them into launches.
#include "ctx.hpp"
#include "fill_plan.hpp"

namespace emme {

namespace {

// (mirrored: the request runs on the half pair list -- runs_mirrored)
FillShape shape_of(const emme_ctx* c, bool mirrored = false) {
    FillShape s;
    s.tiled = c->tiled, s.folded = c->folded;
    s.nm = c->nm, s.gk_points = c->p.integration_start_points, s.npairs = mirrored ? c->npairs_half : c->npairs;
    s.fill_lanes = c->opt.fill == EMME_FILL_LANES;
    s.dense_min_tasks = c->opt.dense_min_tasks, s.dense_cost_ratio = c->opt.dense_cost_ratio;
    s.union_ipg_few = c->opt.union_ipg_few, s.union_few_chunks = c->opt.union_few_chunks;
    return s;
}

// A derivative request that may go through the node cache (option deriv_cached): k_assemble_dense_deriv
// exists for electrostatic GK15 on the tiled layout, k_assemble_dense_shape_deriv<PTS, NM> for tiled
// electromagnetic and GK31 contexts once the context's derivative cache shapes are EMME_DERIV_CACHE_SHAPES_ALL
// (emme_ctx_set_deriv_cache_shapes), and the contour classes need the omegas' host values.  Every other derivative
// request keeps the uncached kernels.
bool deriv_shape_is_es15(const emme_ctx* c) { return c->nm == 1 && c->p.integration_start_points == 15; }
bool deriv_from_cache(const emme_ctx* c, const FillRequest& r) {
    return r.d_Md && c->opt.deriv_cached != 0 && c->tiled &&
           (deriv_shape_is_es15(c) || c->deriv_cache_shapes == EMME_DERIV_CACHE_SHAPES_ALL) && r.host_omega != nullptr;
}

// A request runs mirrored -- on one pair of every mirror-image couple -- when the context's tiled cache
// is laid out that way and the request goes to it: the plain dense fill and its deferred pass.  Every other kernel
// family (tile fills, omega-lane, lanes-are-nodes, sets, every derivative kernel) keeps the full list.
bool runs_mirrored(const emme_ctx* c, const FillRequest& r, bool use_cache) {
    return c->mirror && c->tiled && use_cache && !r.d_Md && !r.d_set;
}

// what the fill kernels are told: the context's tables and counters, the request's operands and, for the plain
// fills, the context's options (a derivative fill runs its two kernels on the struct defaults)
AssembleLaunch make_launch(const emme_ctx* c, const FillRequest& r, bool mirrored) {
    AssembleLaunch L;
    L.P = c->P;
    L.gk_points = c->p.integration_start_points;
    L.nbatch = r.nbatch;
    L.npairs = mirrored ? c->npairs_half : c->npairs;
    L.tab = c->d_tab;
    L.pairs = mirrored ? c->d_pairs_half : c->d_pairs;
    L.mirror = mirrored ? 1 : 0;
    L.omega = r.d_omega;
    L.active = r.d_active;
    L.M = r.d_M;
    L.Mold = r.d_Mold;
    L.Mp = r.d_Mp;
    L.domega = r.d_domega;
    L.Md = r.d_Md;
    L.intervals = c->d_intervals;
    L.status = c->d_status;
    L.rounds = c->d_rounds;
    if (r.d_Md) return L;
    // inside a root search a matrix that already holds a non-finite integral is lost (k_newton_update retires its
    // chain): the fill kernels leave it alone.  Plain assembly calls always get the whole matrix.
    L.skip_lost = r.newton_loop && c->opt.skip_lost != 0;
    L.union_sel = c->opt.union_sel;
    L.union_walk = c->opt.fill != EMME_FILL_LANES;
    L.coop_wide_min = c->opt.coop_wide_min;
    L.defer_one_group = c->opt.defer_one_group;
    L.dense_min_cols = c->opt.dense_min_cols;
    L.dense_stage = c->opt.dense_stage;
    return L;
}

// The cache costs a few hundred ms of kernels plus the allocation of up to ~170 GB to build
// and pays off after ~10 fills: a call with a handful of omegas (a single root of a
// parameter scan) goes through the on-the-fly kernels unless the cache already exists.
// (The contour classes need the omegas' host values; a derivative request reads the cache only where
// deriv_from_cache says so.)
bool wants_cache(const emme_ctx* c, const FillRequest& r) {
    return (!r.d_Md || deriv_from_cache(c, r)) && !r.force_uncached && r.host_omega != nullptr && c->cache_depth != -2 &&
           (r.nbatch >= c->opt.cache_min_batch || c->cache[0].recs || c->cache[1].recs);
}

// omega order (c->h_actidx) | chunk table | position map: into a pinned slot, then ONE small kernel moves them to
// the device
int stage_lists(emme_ctx* c, const std::vector<int>* chunks) {
    const std::vector<int>& order = c->h_actidx;
    const int n = (int)order.size(), n2 = chunks ? (int)chunks->size() : 0;
    int* slot = nullptr;
    HIP_TRY(c->lists.take(n + n2, &slot));
    std::copy(order.begin(), order.end(), slot);
    if (chunks) std::copy(chunks->begin(), chunks->end(), slot + n);
    HIP_TRY(launch_stage_ints(slot, c->d_actidx, n, chunks ? c->d_chunks.get() : nullptr, n2, c->stream));
    HIP_TRY(c->lists.read_on(c->stream));
    return EMME_OK;
}

// the previous cached fill deferred a sizeable share of its integrals: look at which
// intervals they were missing and cache a subtree around the most frequent one(s)
int grow_cache_from_deferrals(emme_ctx* c, const AssembleLaunch& L) {
    if (!c->d_worklist_count || !c->d_defer_info) return EMME_OK;
    if (!c->fb.pub_valid) {  // (the Newton loop gets the count from k_retire through pinned memory)
        HIP_TRY(hipMemcpyAsync(&c->fb.last_deferred, c->d_worklist_count, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->fb.pub_valid = false;
    if (c->fb.last_deferred < 32) return EMME_OK;
    const size_t cnt = std::min<size_t>(c->fb.last_deferred, 1u << 16);
    std::vector<unsigned long long> info(cnt);
    HIP_TRY(hipMemcpy(info.data(), c->d_defer_info, cnt * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::sort(info.begin(), info.end());
    // most frequent missing interval per contour class (bit 55 of an entry)
    unsigned long long best[2] = {0, 0};
    size_t best_n[2] = {0, 0}, total[2] = {0, 0};
    for (size_t q = 0; q < cnt;) {
        size_t e = q;
        while (e < cnt && info[e] == info[q]) ++e;
        const int k = (int)((info[q] >> 55) & 1ull);
        total[k] += e - q;
        if (e - q > best_n[k]) best_n[k] = e - q, best[k] = info[q];
        q = e;
    }
    if (std::getenv("EMME_DEBUG"))
        for (int k = 0; k < 2; ++k)
            if (total[k])
                fprintf(stderr, "[emme] deferrals of class %d: %zu, most frequent missing interval depth %d path %llx (%zu)\n", k,
                        total[k], (int)(best[k] >> 56), best[k] & 0x7fffffffffffffull, best_n[k]);
    for (int k = 0; k < 2; ++k)
        if (total[k] >= 32 && best_n[k] * 4 >= total[k])
            add_cache_subtree(c, L, (int)(best[k] >> 56), best[k] & 0x7fffffffffffffull, k);
    return EMME_OK;
}

// EMME_DEBUG_STAMPS (with an EMME_DENSE_STAMPS build): the tasks of one dense launch, their total and longest time
struct DenseStamps {
    emme_ctx* c;
    const bool on;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    unsigned long long r0[16] = {};
    explicit DenseStamps(emme_ctx* ctx) : c(ctx), on(enabled()) {}
    ~DenseStamps() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    static bool enabled() {
        static const bool stamps = std::getenv("EMME_DEBUG_STAMPS") != nullptr;
        return stamps;
    }
    int before() {
        if (!on) return EMME_OK;
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(r0, c->d_rounds, sizeof r0, hipMemcpyDeviceToHost));
        const unsigned long long zero = 0;
        HIP_TRY(hipMemcpy(c->d_rounds + 9, &zero, sizeof zero, hipMemcpyHostToDevice));
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e0, c->stream));
        return EMME_OK;
    }
    int after(int n_lane, int nchunks) {
        if (!on) return EMME_OK;
        HIP_TRY(hipEventRecord(e1, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        unsigned long long r1[16] = {};
        HIP_TRY(hipMemcpy(r1, c->d_rounds, sizeof r1, hipMemcpyDeviceToHost));
        const double tasks = (double)(r1[3] - r0[3]), tot = (double)(r1[8] - r0[8]);
        fprintf(stderr, "[emme] dense launch: %d omegas in %d chunks, %.0f tasks, %.3f ms; task ticks: mean %.0f, longest %.0f, "
                "sum / 2048 wave slots %.0f; rounds dense %llu sparse %llu\n", n_lane, nchunks, tasks, ms,
                tasks > 0 ? tot / tasks : 0.0, (double)r1[9], tot / 2048.0, r1[0] - r0[0], r1[1] - r0[1]);
        // how the tiles' times are spread (all chunks of the launch added up per tile)
        const size_t nt = std::min<size_t>(((size_t)cache_npairs(c) + 15) / 16, 8192);
        std::vector<unsigned long long> tt(nt);
        HIP_TRY(hipMemcpy(tt.data(), c->d_rounds + 16, nt * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(c->d_rounds + 16, 0, nt * sizeof(unsigned long long)));
        // first, middle and last tiles in index order, then percentiles
        fprintf(stderr, "[emme]   tile ticks by index: %llu %llu %llu %llu %llu | ", tt[0], tt[nt / 4], tt[nt / 2], tt[3 * nt / 4], tt[nt - 1]);
        std::sort(tt.begin(), tt.end());
        fprintf(stderr, "sorted: min %llu p25 %llu p50 %llu p75 %llu p90 %llu p97 %llu max %llu\n", tt[0], tt[nt / 4], tt[nt / 2],
                tt[3 * nt / 4], tt[nt * 9 / 10], tt[nt * 97 / 100], tt[nt - 1]);
        return EMME_OK;
    }
};

// EMME_DEBUG: how many integrals the cached fill just queued deferred, and the first few of them
void print_deferred(emme_ctx* c, int n_act) {
    unsigned int cnt = 0;
    (void)hipMemcpy(&cnt, c->d_worklist_count, sizeof cnt, hipMemcpyDeviceToHost);
    std::vector<unsigned long long> wl(cnt < 8 ? cnt : 8);
    if (!wl.empty()) (void)hipMemcpy(wl.data(), c->d_worklist, wl.size() * 8, hipMemcpyDeviceToHost);
    fprintf(stderr, "[emme] cached fill: %d items, %u integrals deferred (of %ld)", n_act, cnt,
            (long)cache_npairs(c) * c->nm * n_act);
    std::vector<unsigned long long> dg(wl.size());
    if (!wl.empty() && c->d_defer_info) (void)hipMemcpy(dg.data(), c->d_defer_info, wl.size() * 8, hipMemcpyDeviceToHost);
    for (size_t q = 0; q < wl.size(); ++q)
        fprintf(stderr, " b%llu:i%llu@d%llu:p%llx", wl[q] >> 32, wl[q] & 0xffffffffull, dg[q] >> 56,
                dg[q] & 0x7fffffffffffffull);
    fprintf(stderr, "\n");
}

// dense fill: weighted phase tables for every cached interval and omega chunk, then one wave
// per (16-pair tile, omega chunk) of the cost-sorted list
int launch_dense(emme_ctx* c, const AssembleLaunch& L, const NodeCacheView& cache, const FillRequest& r, int n_lane,
                 int nchunks, int n_wide) {
    const int n_int = node_cache_intervals(c->cache_geom);
    const size_t need = btab_bytes(n_int, nchunks, L.gk_points);
    if (need > c->d_btab.bytes()) HIP_TRY(c->d_btab.grow(need + need / 4));
    {
        ScopedSpan s(c, K_OTHER);
        HIP_TRY(launch_btab(L.gk_points, c->nm, n_int, cache, r.d_omega, c->d_actidx, n_lane, c->d_chunks + 2 * nchunks,
                            nchunks, c->d_btab, c->stream));
    }
    ScopedSpan s(c, K_ASM);
    DenseStamps stamps(c);
    EMME_TRY(stamps.before());
    HIP_TRY(launch_assemble_dense(L, cache, c->d_btab, c->d_worklist, c->d_worklist_count, c->d_defer_info,
                                  c->d_actidx, n_lane, c->d_chunks, nchunks, c->d_rounds, c->stream,
                                  (c->opt.dense_wide && c->nm == 1) ? nchunks : n_wide, r.newton_loop ? c->d_overflow : nullptr));
    return stamps.after(n_lane, nchunks);
}

// independent lanes or union walk over the cached records; on folded records behind the phase table of this
// launch, exp(T omega) for every cached interval, node and omega
int launch_cached_lanes(emme_ctx* c, const AssembleLaunch& L, const NodeCacheView& cache, const FillRequest& r, int n_lane,
                        int nchunks) {
    if (c->folded) {
        const int n_int = node_cache_intervals(c->cache_geom);
        const size_t need = (size_t)n_lane * n_int * (L.gk_points == 15 ? 16 : 32) * 2 * sizeof(double);
        if (need > c->d_etab.bytes()) HIP_TRY(c->d_etab.grow(need + need / 4));
        ScopedSpan s(c, K_OTHER);
        HIP_TRY(launch_phase_table(L.gk_points, n_int, cache, r.d_omega, c->d_actidx, n_lane, c->d_etab, c->stream));
    }
    ScopedSpan s(c, K_ASM);
    const void* etab = c->folded ? c->d_etab : nullptr;
    if (c->em_shared)
        HIP_TRY(launch_assemble_cached_em(L, cache, etab, c->d_worklist, c->d_worklist_count, c->d_defer_info,
                                          c->d_actidx, n_lane, c->d_chunks, nchunks, c->stream));
    else
        HIP_TRY(launch_assemble_cached(L, cache, etab, c->d_worklist, c->d_worklist_count, c->d_defer_info,
                                       c->d_actidx, n_lane, c->d_chunks, nchunks, c->stream));
    return EMME_OK;
}

// M and M' from the tiled cache: twin-column phase tables, then one wave per (16-pair tile, chunk of <= 8 omegas), then
// the integrals that left the cache through the list-driven from-scratch derivative kernel
int launch_dense_deriv(emme_ctx* c, const AssembleLaunch& L, const NodeCacheView& cache, const FillRequest& r, int n_lane,
                       int nchunks) {
    // (electromagnetic and GK31 contexts, DESIGN.md 12.5: twin columns too -- 8 electrostatic omegas, 2 x 3 moments)
    const bool es15 = deriv_shape_is_es15(c);
    const int chunk_max = dense_shape_deriv_chunk(c->nm);  // (8 for every electrostatic shape)
    for (int k = 0; k < nchunks; ++k)
        if (c->h_chunks[2 * k + 1] > chunk_max) {
            set_error(es15 ? "derivative fill: a chunk of more than 8 omegas was planned"
                           : "derivative fill: a chunk wider than the twin-column layout of this shape was planned");
            return EMME_EINVAL;
        }
    const int n_int = node_cache_intervals(c->cache_geom);
    const size_t need = btab_bytes(n_int, nchunks, L.gk_points);
    if (need > c->d_btab.bytes()) HIP_TRY(c->d_btab.grow(need + need / 4));
    {
        ScopedSpan s(c, K_OTHER);
        if (es15)
            HIP_TRY(launch_btab_deriv(n_int, cache, r.d_omega, c->d_actidx, n_lane, c->d_chunks + 2 * nchunks, nchunks,
                                      c->d_btab, c->stream));
        else
            HIP_TRY(launch_btab_shape_deriv(L.gk_points, c->nm, n_int, cache, r.d_omega, c->d_actidx, n_lane,
                                            c->d_chunks + 2 * nchunks, nchunks, c->d_btab, c->stream));
    }
    {
        ScopedSpan s(c, K_ASM);
        HIP_TRY((es15 ? launch_assemble_dense_deriv : launch_assemble_dense_shape_deriv)(
            L, cache, c->d_btab, c->d_worklist, c->d_worklist_count, c->d_defer_info, c->d_actidx, c->d_chunks, nchunks,
            c->d_rounds, c->stream));
    }
    ScopedSpan s(c, K_DEFER);
    HIP_TRY((es15 ? launch_assemble_deriv_list : launch_assemble_deriv_list_shape)(L, c->d_worklist, c->d_worklist_count,
                                                                                   c->stream));
    return EMME_OK;
}

// the integrals the cached kernels could not finish from the cache
int launch_deferred(emme_ctx* c, const AssembleLaunch& L, const NodeCacheView& cache) {
    ScopedSpan s(c, K_DEFER);
    // (tiled electromagnetic / GK31 contexts: the cooperative kernel reads the electrostatic GK15 tile blocks
    // only -- the few integrals that leave the cache are evaluated from scratch)
    const bool coop_cached = !(c->tiled && (c->nm > 1 || L.gk_points != 15));
    NodeCacheView coop = cache;  // (moment factors of the shared EM layout only)
    if (!c->em_shared) coop.wtab[0] = coop.wtab[1] = nullptr;
    HIP_TRY(launch_assemble_list(L, c->d_worklist, c->d_worklist_count, coop_cached ? &coop : nullptr, c->folded,
                                 c->stream, c->tiled && coop_cached));
    return EMME_OK;
}

// the omegas of c->h_actidx from the node cache: chunk plan, lists to the device, the layout's fill kernel, then
// the deferred list
int fill_cached(emme_ctx* c, AssembleLaunch& L, const FillRequest& r, int n_wide) {
    const NodeCacheView cache = c->cache_view();
    const int n_lane = (int)c->h_actidx.size();
    // work list for integrals that outgrow the cache (worst case: every one of them)
    const size_t need = (size_t)c->npairs * c->nm * (size_t)r.nbatch;
    HIP_TRY(c->d_worklist.grow(need * sizeof(unsigned long long)));
    HIP_TRY(c->d_defer_info.grow(need * sizeof(unsigned long long)));
    HIP_TRY(c->d_worklist_count.grow(sizeof(unsigned int)));
    FillShape shape = shape_of(c, L.mirror != 0);
    shape.deriv = r.d_Md != nullptr;
    const ChunkPlan plan = plan_chunks(shape, c->h_actidx, r.cost, n_wide, c->h_chunks);
    L.items_per_group = plan.items_per_group;
    EMME_TRY(stage_lists(c, &c->h_chunks));
    HIP_TRY(hipMemsetAsync(c->d_worklist_count, 0, sizeof(unsigned int), c->stream));
    c->last_fill_listed = 1;
    if (r.d_Md) {
        // (make_launch leaves a derivative request on the struct defaults, which the uncached kernels keep; here the
        // context's options apply as to a plain dense fill.  last_fill_mode keeps naming the last plain fill.)
        L.skip_lost = r.newton_loop && c->opt.skip_lost != 0;
        L.dense_min_cols = c->opt.dense_min_cols;
        EMME_TRY(launch_dense_deriv(c, L, cache, r, n_lane, plan.nchunks));
        if (std::getenv("EMME_DEBUG")) print_deferred(c, n_lane);
        return EMME_OK;
    }
    c->last_fill_mode = c->tiled ? FILL_DENSE : (plan.union_walk ? FILL_CACHED_UNION : FILL_CACHED_LANES);
    EMME_TRY(c->tiled ? launch_dense(c, L, cache, r, n_lane, plan.nchunks, n_wide)
                      : launch_cached_lanes(c, L, cache, r, n_lane, plan.nchunks));
    EMME_TRY(launch_deferred(c, L, cache));
    if (std::getenv("EMME_DEBUG")) print_deferred(c, n_lane);
    return EMME_OK;
}

// A request without a node cache that the table-free tile fill serves (option tile_uncached):
// k_assemble_tile exists for electrostatic GK15 under the dense fill's accuracy precondition (the GEMM cannot apply
// the safe_exp clamp), and its chunks need the omegas' host values (one contour class per chunk).  Electromagnetic and
// GK31 contexts have k_assemble_tile_shape under the same preconditions once the context's tile shapes
// are EMME_TILE_SHAPES_ALL (emme_ctx_set_tile_shapes).
// A derivative request asks for the option deriv_cached as well: it is what hands such a request
// the host omegas, costs and feedback, and so lets it follow the plain fills' policy.  Neither a tiled layout nor a
// cache budget is asked for, and the tile shapes count on contexts that have a node cache too: a derivative request of
// those shapes reads it only under EMME_DERIV_CACHE_SHAPES_ALL (deriv_from_cache), and then the cache takes what its
// policy gives it and the tile fill what that policy leaves without a cache -- the rule of electrostatic GK15.
bool tile_shape_is_es15(const emme_ctx* c) { return c->nm == 1 && c->p.integration_start_points == 15; }
bool tile_fill_applies(const emme_ctx* c, const FillRequest& r, bool omega_lane) {
    if (r.d_Md && c->opt.deriv_cached == 0) return false;
    return c->opt.tile_uncached != 0 && omega_lane && r.host_omega != nullptr &&
           (tile_shape_is_es15(c) || c->tile_shapes == EMME_TILE_SHAPES_ALL) && c->p.integration_accuracy >= 1e-9;
}

// the omegas of c->h_actidx through the tile fill: chunk plan, lists to the device, the kernel picked by (derivative
// request?, shape) -- k_assemble_tile, k_assemble_tile_shape or their _deriv forms -- then the integrals it handed
// over, from scratch, by the list kernel of the same pick (a derivative request: M and M').  last_fill_mode names the
// plain fills' kernel: a derivative fill leaves it alone.
int launch_tile(emme_ctx* c, AssembleLaunch& L, const FillRequest& r) {
    const bool deriv = r.d_Md != nullptr, es15 = tile_shape_is_es15(c);
    // a work list of its own (worst case: every integral of the omegas it fills): see ctx.hpp
    const size_t need = (size_t)c->npairs * c->nm * c->h_actidx.size();
    HIP_TRY(c->d_tile_worklist.grow(need * sizeof(unsigned long long)));
    HIP_TRY(c->d_tile_count.grow(sizeof(unsigned int)));
    const ChunkPlan plan = plan_tile_chunks(shape_of(c), c->h_actidx, r.host_omega, r.cost, c->h_chunks);
    L.items_per_group = plan.items_per_group;
    // (make_launch leaves a derivative request on the struct defaults: as in fill_cached's derivative branch)
    if (deriv) L.skip_lost = r.newton_loop && c->opt.skip_lost != 0;
    EMME_TRY(stage_lists(c, &c->h_chunks));
    HIP_TRY(hipMemsetAsync(c->d_tile_count, 0, sizeof(unsigned int), c->stream));
    if (!deriv) c->last_fill_mode = FILL_TILE;
    c->last_fill_listed = 2;
    {
        ScopedSpan s(c, K_ASM);
        const auto kernel = deriv ? (es15 ? launch_assemble_tile_deriv : launch_assemble_tile_shape_deriv)
                                  : (es15 ? launch_assemble_tile : launch_assemble_tile_shape);
        HIP_TRY(kernel(L, c->d_tile_worklist, c->d_tile_count, c->d_actidx, c->d_chunks, plan.nchunks, c->d_rounds, c->stream));
    }
    ScopedSpan s(c, K_DEFER);
    if (!deriv)
        HIP_TRY(launch_assemble_list(L, c->d_tile_worklist, c->d_tile_count, nullptr, c->folded, c->stream, false));
    else if (es15)
        HIP_TRY(launch_assemble_deriv_list(L, c->d_tile_worklist, c->d_tile_count, c->stream));
    else
        HIP_TRY(launch_assemble_deriv_list_shape(L, c->d_tile_worklist, c->d_tile_count, c->stream));
    return EMME_OK;
}

// without the node cache, plain (L.Md null) or with the exact derivative: batches of wl_min or more items (and
// the minority pass, whatever its size) go through the omega-lane kernel, which shares the omega-independent node
// data between items -- or, where tile_fill_applies, through the table-free tile fill; smaller ones through the
// lanes-are-nodes kernel.  last_fill_mode names the plain fills' kernel: a derivative fill leaves it alone.
int fill_uncached(emme_ctx* c, AssembleLaunch& L, const FillRequest& r) {
    const FillShape s = shape_of(c);
    const int n_act = (int)c->h_actidx.size(), gw = s.lane_group();
    const bool omega_lane = n_act >= c->opt.wl_min || r.force_uncached;
    if (tile_fill_applies(c, r, omega_lane)) return launch_tile(c, L, r);
    c->last_fill_listed = 0;
    L.items_per_group = items_per_group_for(s, omega_lane ? (n_act + gw - 1) / gw : r.nbatch);
    if (omega_lane) {
        EMME_TRY(stage_lists(c, nullptr));
    }
    if (!r.d_Md) c->last_fill_mode = omega_lane ? FILL_OMEGA_LANE : FILL_NODES;
    ScopedSpan span(c, K_ASM);
    if (omega_lane)
        HIP_TRY(launch_assemble_wl(L, c->d_actidx, n_act, c->stream));
    else
        HIP_TRY(launch_assemble(L, c->stream));
    return EMME_OK;
}

// A request over parameter sets that the table-free tile fill may serve: tile_fill_applies' rule,
// with the accuracy precondition asked of EVERY bound set (any of them may be an item's): electrostatic GK15, and once
// the context's tile shapes are EMME_TILE_SHAPES_ALL electromagnetic and GK31 contexts too.
bool tile_sets_applies(const emme_ctx* c, const FillRequest& r) {
    if (r.d_Md && c->opt.deriv_cached == 0) return false;
    if (c->opt.tile_uncached == 0 || !r.host_omega || !r.host_set) return false;
    if (!(tile_shape_is_es15(c) || c->tile_shapes == EMME_TILE_SHAPES_ALL)) return false;
    for (const emme_params_t& p : c->sets)
        if (!(p.integration_accuracy >= 1e-9)) return false;
    return true;
}

// The items of c->h_actidx (every group of them: one parameter set, one contour class, wl_min items or more) through
// the tile fill over sets: chunk plan, lists to the device -- the omega order; behind the chunk table and the position
// map, where the work-list segment of every set begins and, `rest` given, the items left to k_assemble_sets -- then
// the kernel picked by (derivative request?, shape) -- k_assemble_tile_sets, k_assemble_tile_shape_sets<PTS, NM> or their
// _deriv forms -- then the segments from scratch by the list kernel of the same pick.
// *d_rest <- the device image of `rest`.
int launch_tile_sets(emme_ctx* c, AssembleLaunch& L, const FillRequest& r, const std::vector<int>* rest, const int** d_rest) {
    const bool deriv = r.d_Md != nullptr, es15 = tile_shape_is_es15(c);
    const int nsets = (int)c->sets.size(), n = (int)c->h_actidx.size();
    // a segment holds every integral of its set's items of this launch: npairs * nm per item
    std::vector<int> seg(nsets, 0), items(nsets, 0);
    for (int b : c->h_actidx) ++items[r.host_set[b]];
    size_t need = 0;
    for (int s = 0; s < nsets; ++s) {
        // (a segment's begin and every position inside it are ints on the device)
        seg[s] = (int)need, need += (size_t)c->npairs * c->nm * items[s];
        if (need > (size_t)std::numeric_limits<int>::max()) {
            set_error("fill over parameter sets: the work list of the tile fill is too long");
            return EMME_EINVAL;
        }
    }
    HIP_TRY(c->d_tile_worklist.grow(need * sizeof(unsigned long long)));
    HIP_TRY(c->d_tile_count.grow(sizeof(unsigned int) * nsets));
    const ChunkPlan plan = plan_tile_chunks(shape_of(c), c->h_actidx, r.host_omega, r.cost, c->h_chunks, r.host_set);
    L.skip_lost = r.newton_loop && c->opt.skip_lost != 0;
    const size_t n2 = c->h_chunks.size(), n_rest = rest ? rest->size() : 0, total = (size_t)n + n2 + nsets + n_rest;
    HIP_TRY(c->d_set_lists.grow(sizeof(int) * (total - n)));
    HIP_TRY(c->lists.reserve(total));
    int* slot = nullptr;
    HIP_TRY(c->lists.take(total, &slot));
    std::copy(c->h_actidx.begin(), c->h_actidx.end(), slot);
    std::copy(c->h_chunks.begin(), c->h_chunks.end(), slot + n);
    std::copy(seg.begin(), seg.end(), slot + n + n2);
    if (rest) std::copy(rest->begin(), rest->end(), slot + n + n2 + nsets);
    HIP_TRY(launch_stage_ints(slot, c->d_actidx, n, c->d_set_lists, (int)(total - n), c->stream));
    HIP_TRY(c->lists.read_on(c->stream));
    const int* d_seg = c->d_set_lists + n2;
    *d_rest = rest ? d_seg + nsets : nullptr;
    HIP_TRY(hipMemsetAsync(c->d_tile_count, 0, sizeof(unsigned int) * nsets, c->stream));
    c->last_fill_listed = 3, c->last_fill_counters = nsets;
    {
        ScopedSpan s(c, K_ASM);
        const auto kernel = deriv ? (es15 ? launch_assemble_tile_sets_deriv : launch_assemble_tile_shape_sets_deriv)
                                  : (es15 ? launch_assemble_tile_sets : launch_assemble_tile_shape_sets);
        HIP_TRY(kernel(
            L, c->d_sets, c->d_set_tabs, r.d_set, d_seg, c->d_tile_worklist, c->d_tile_count, c->d_actidx, c->d_set_lists,
            plan.nchunks, c->d_rounds, c->stream));
    }
    ScopedSpan s(c, K_DEFER);
    const auto list = deriv ? (es15 ? launch_assemble_sets_deriv_list : launch_assemble_sets_deriv_list_shape)
                            : (es15 ? launch_assemble_sets_list : launch_assemble_sets_list_shape);
    HIP_TRY(list(L, c->d_sets, c->d_set_tabs, nsets, c->d_tile_worklist, d_seg, c->d_tile_count, c->stream));
    return EMME_OK;
}

// A request whose items carry their own parameter set (r.d_set).  Never the node cache or the omega-lane
// kernel; no fused secant.  Where tile_sets_applies, every (set, contour class) group of wl_min items or more -- the
// project's threshold for "sharing node data between omegas pays" -- goes through the tile fill over sets (DESIGN.md
// 13.7); the smaller groups, and every request that fails a precondition, through k_assemble_sets, or with r.d_Md
// k_assemble_sets_deriv: in a second pass of the same call where both kinds of group exist.  The reported mode is
// FILL_TILE_SETS when at least one group took the tile fill.
int launch_sets(emme_ctx* c, AssembleLaunch& L, const FillRequest& r) {
    if (c->sets.empty() || !c->d_sets || !c->d_set_tabs) {
        set_error("fill over parameter sets: no sets are bound to the context");
        return EMME_EINVAL;
    }
    if (r.d_Mold) {
        set_error("fill over parameter sets: no fused secant");
        return EMME_EINVAL;
    }
    c->last_fill_listed = 0;
    c->last_fill_mode = FILL_SETS;
    bool all_tiled = false;
    if (tile_sets_applies(c, r)) {
        std::vector<int> group_items(2 * c->sets.size(), 0);
        auto group_of = [&](int b) { return 2 * r.host_set[b] + contour_class(r.host_omega[2 * b]); };
        for (int b : c->h_actidx) ++group_items[group_of(b)];
        std::vector<int> tiled, rest(r.nbatch, 0);
        for (int b : c->h_actidx) {
            if (group_items[group_of(b)] >= c->opt.wl_min)
                tiled.push_back(b);
            else
                rest[b] = 1;
        }
        if (!tiled.empty()) {
            all_tiled = tiled.size() == c->h_actidx.size();
            c->h_actidx = tiled;
            const int* d_rest = nullptr;
            EMME_TRY(launch_tile_sets(c, L, r, all_tiled ? nullptr : &rest, &d_rest));
            c->last_fill_mode = FILL_TILE_SETS;
            L.active = d_rest;
        }
    }
    if (all_tiled) return EMME_OK;
    L.items_per_group = items_per_group_for(shape_of(c), r.nbatch);
    ScopedSpan span(c, K_ASM);
    HIP_TRY((r.d_Md ? launch_assemble_sets_deriv : launch_assemble_sets)(L, c->d_sets, c->d_set_tabs, r.d_set, c->stream));
    return EMME_OK;
}

// the majority class through the cache, then the `minority` class through the omega-lane kernel; the call's fill
// kernel, as reported, stays the majority's
int fill_by_class(emme_ctx* c, const FillRequest& r, int minority) {
    std::vector<int> major(r.nbatch, 0), minor(r.nbatch, 0);
    for (int b : c->h_actidx) (contour_class(r.host_omega[2 * b]) == minority ? minor : major)[b] = 1;
    FillRequest part = r;
    part.host_active = major.data();
    EMME_TRY(fill(c, part));
    const int mode = c->last_fill_mode;
    part.host_active = minor.data(), part.force_uncached = true;
    const int rc = fill(c, part);
    c->last_fill_mode = mode;
    c->last_fill_mirrored = false;  // (the minority's matrices come from the full pair list)
    return rc;
}

}  // namespace

int fill(emme_ctx* c, const FillRequest& r) {
    // omegas whose level lists overflowed in their previous fill (root search only): first, a chunk each, through the
    // wide-list build of the dense fill
    // (a derivative request has no wide-list build)
    const bool has_wide = r.newton_loop && !r.d_Md && !r.d_set && c->tiled && c->nm == 1 && !c->fb.wide.empty();
    const int n_wide = plan_order(r.nbatch, r.host_active, r.cost, has_wide ? c->fb.wide.data() : nullptr, c->h_actidx);
    const int n_act = (int)c->h_actidx.size();
    c->last_fill_mirrored = false;  // (until every matrix of the request has gone down the mirrored route)
    if (n_act == 0) return EMME_OK;
    if (r.d_set) {
        AssembleLaunch L = make_launch(c, r, false);
        EMME_TRY(launch_sets(c, L, r));
        c->acc.matrices += n_act;
        return EMME_OK;
    }
    // no derivative kernel reads a half pair list: a cached derivative request ends a context's mirroring
    if (c->mirror && deriv_from_cache(c, r)) EMME_TRY(drop_mirror(c));
    bool use_cache = wants_cache(c, r);
    // the pair list is part of the tiled cache's layout: fixed when the first part of the cache is allocated
    if (use_cache && !c->cache[0].recs && !c->cache[1].recs) c->mirror = mirror_wanted(c) && r.may_mirror;
    AssembleLaunch L = make_launch(c, r, runs_mirrored(c, r, use_cache));
    if (use_cache) {
        const bool has_cache[2] = {(bool)c->cache[0].recs, (bool)c->cache[1].recs};
        const ClassCensus classes = plan_classes(c->h_actidx, r.host_omega, has_cache);
        if (classes.minority >= 0) return fill_by_class(c, r, classes.minority);
        for (int k = 0; k < 2 && use_cache; ++k)
            if (classes.count[k] > 0) use_cache = ensure_node_cache(c, L, k);
        if (!use_cache && L.mirror) L = make_launch(c, r, false);  // (the cache did not fit: the uncached kernels' list)
    }
    EMME_TRY(use_cache ? grow_cache_from_deferrals(c, L) : EMME_OK);
    EMME_TRY(use_cache ? fill_cached(c, L, r, n_wide) : fill_uncached(c, L, r));
    c->last_fill_mirrored = use_cache && L.mirror != 0;
    c->acc.matrices += n_act;
    return EMME_OK;
}

}  // namespace emme
