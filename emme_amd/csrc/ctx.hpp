// ctx.hpp -- the context behind the C ABI (include/emme_hip.h) and the host-side helpers its translation
// units share: emme_capi.hip (context lifecycle, options, profile, the assembly entry points), ctx_linstep.hip (the
// Newton linear step, the batched LU and the null-vector driver), ctx_search.hip (the two root searches),
// ctx_cache.hip (buffer pool and the HBM node cache's host side), ctx_fill.hip (the fill dispatcher), probe.hip (the
// probe entry points).  What needs no device is plain C++ under the sanitizer build (make host-sanitize): options.cpp,
// fill_plan.cpp, linstep_plan.hpp, step_feedback.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/emme_hip.h"
#include "buffers.hpp"
#include "launch.hpp"
#include "options.hpp"
#include "pair_list.hpp"
#include "step_feedback.hpp"

namespace emme {

void set_error(const std::string& msg);

#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess) {                                                        \
            emme::set_error(std::string(#expr) + ": " + hipGetErrorString(e_));       \
            return e_ == hipErrorOutOfMemory ? EMME_ENOMEM : EMME_EDEVICE;             \
        }                                                                              \
    } while (0)

// the same for the EMME_* codes of the host layer's own functions
#define EMME_TRY(expr)             \
    do {                           \
        const int rc_ = (expr);    \
        if (rc_) return rc_;       \
    } while (0)

enum Kind { K_ASM = 0, K_LIN = 1, K_OTHER = 2, K_DEFER = 3, K_CACHE = 4, K_NULL = 5 };

// kernel family of a plain fill, as emme_ctx_fill_mode reports it (include/emme_hip.h)
enum FillMode { FILL_NODES = 0, FILL_OMEGA_LANE = 1, FILL_CACHED_LANES = 2, FILL_CACHED_UNION = 3, FILL_DENSE = 4, FILL_TILE = 5, FILL_SETS = 6, FILL_TILE_SETS = 7 };

// HBM node cache of one contour class (omi = +1, -1)
struct NodeCacheClass {
    PooledBuffer recs;                                // main part
    PooledBuffer recs_ext[NODE_CACHE_MAX_SUB - 1];    // run-time subtrees
    DeviceBuffer<> ttab;                              // T table
    DeviceBuffer<> wtab;                              // moment-factor table (shared EM layout, tiled EM)
    DeviceBuffer<unsigned char> tile_poison;          // tiled layout: tiles that hold a poisoned block
};

}  // namespace emme

// (the C ABI's opaque context type lives at global scope; its members are types of namespace emme)
using emme::DevParams;
using emme::DeviceBuffer;
using emme::NodeCacheClass;
using emme::NodeCacheGeom;
using emme::NODE_CACHE_MAX_SUB;
using emme::PinnedBuffer;

struct emme_ctx {
    emme_params_t p;
    int device = 0;
    hipStream_t stream = nullptr;
    DevParams P;
    int N = 0, dim = 0, nm = 1, npairs = 0;
    DeviceBuffer<double> d_tab;
    DeviceBuffer<ushort2> d_pairs;
    // Mirror-image pairs: on a grid symmetric under i -> N-1-i the integral of pair (i, j) is that of
    // (N-1-j, N-1-i), so the tiled cache and the dense fill behind it take one pair of each couple (d_pairs_half, same
    // order as d_pairs) and the result section writes both.  Every other kernel family keeps d_pairs.
    int npairs_half = 0;
    DeviceBuffer<ushort2> d_pairs_half;
    bool mirror_ok = false;    // the grid is symmetric under i -> N-1-i: decided at creation (mirror_wanted)
    int mirror_shapes = EMME_MIRROR_SHAPES_ES15;  // shapes that mirror on such a grid (emme_ctx_set_mirror_shapes;
                               // EMME_MIRROR_SHAPES read at creation); fixed once a cache exists
    int mirror_opt = 1;        // emme_ctx_set_mirror_pairs (EMME_MIRROR read at creation); fixed once a cache exists
    bool mirror = false;       // the tiled cache is laid out over d_pairs_half: fixed when it is first allocated
    // parameter sets bound to the context (emme_ctx_bind_param_sets): each has the shape of `p`
    std::vector<emme_params_t> sets;   // host copy
    DeviceBuffer<DevParams> d_sets;    // the kernels' scalars, one per set
    DeviceBuffer<double> d_set_tabs;   // eta | g | b of every set, 3N doubles each
    DeviceBuffer<int> d_set;           // the set of every batch item of the current call
    DeviceBuffer<int> d_set_lists;     // tile fill over sets: chunk table | position map | work-list
                                       // segment offset of every set | the items left to k_assemble_sets
    // batch scratch
    DeviceBuffer<double> d_omega, d_domega, d_tr;
    DeviceBuffer<int> d_active, d_iters, d_info, d_status;
    DeviceBuffer<unsigned long long> d_intervals;
    DeviceBuffer<unsigned long long> d_rounds;  // diagnostic counter of the omega-lane kernel
    DeviceBuffer<int> d_actidx;   // compacted list of batch items for the omega-lane kernel
    DeviceBuffer<int> d_chunks;   // (first, size) of every omega chunk of the cached kernel
    std::vector<int> h_chunks;
    std::vector<int> h_actidx; // its host image
    int last_fill_mode = -1;   // FillMode of the last plain fill (-1: none yet)
    int last_fill_listed = 0;  // work list the last fill reset and used (emme_ctx_last_deferred): 0 none, 1 the cached
                               // fills' (d_worklist), 2 the tile fill's (d_tile_worklist), 3 the tile fill's over
                               // parameter sets (d_tile_worklist in segments, a counter per bound set in d_tile_count)
    int last_fill_counters = 1;  // ... and how many counters that work list has (3: the sets bound at that fill)
    int tile_shapes = EMME_TILE_SHAPES_ES15;  // shapes the option tile_uncached serves (emme_ctx_set_tile_shapes;
                               // EMME_TILE_SHAPES read at creation)
    int deriv_cache_shapes = EMME_DERIV_CACHE_SHAPES_ES15;  // shapes whose derivative fills the option deriv_cached sends
                               // through the node cache (emme_ctx_set_deriv_cache_shapes; EMME_DERIV_CACHE_SHAPES
                               // read at creation)
    emme_options_t opt{};      // per-context options (emme_options_t; environment overrides applied at creation)
    // HBM cache of omega-independent node records, per contour class (omi = +1, -1)
    int cache_depth = -1;      // -1: not decided yet, -2: disabled / does not fit, else dfull
    NodeCacheGeom cache_geom{};
    int cache_max_intervals = 0;  // capacity of the T / scale tables
    NodeCacheClass cache[2];
    bool em_shared = false;    // nm == 3: one record per (pair, interval, node), three moments per lane
    bool folded = true;        // records carry exp(A0); exp(T omega) comes from a per-launch phase table
    bool tiled = false;        // electrostatic GK15: tiled record layout + dense (matrix-core) fill
    DeviceBuffer<> d_btab;     // weighted phase tables of the current launch (dense fill)
    DeviceBuffer<> d_etab;     // phase table of the current launch
    DeviceBuffer<int> d_lu_items;  // blocked LU: the live matrices of the launch
    DeviceBuffer<> d_lu_scratch;   // blocked LU: diagonal of X, hand-over flags, row-map snapshots
    int n_cu = 256;                // compute units of the device
    int last_lu_nwg = 1;           // workgroups per matrix of the last LU launch
    const char* last_lu_symbol = "";  // ... its kernel (emme_ctx_linstep_kernel_symbol; "": none yet)
    int last_lu_slices = 0;        // ... and, for lu_factor_batch, the launches its matrices were cut into
    bool lu_one_wg = false;        // a hand-over of the multi-workgroup LU timed out once: never again
    // the folded trace-secant step (linstep_fold.hip)
    int lu_fold = 1;               // emme_ctx_set_lu_fold (EMME_LU_FOLD read at creation)
    bool last_fill_mirrored = false;  // the last fill() wrote every matrix it was asked for through the mirrored route
    int last_folded_steps = 0;     // steps of the last root search that ran folded (emme_ctx_last_folded_steps)
    struct FoldScratch {
        DeviceBuffer<double> vecs, tr2, part;    // folds of u and u'; traces of the half problems; k_fold_solve's sums
        DeviceBuffer<int> act2, info2, lu_info, items;
        DeviceBuffer<> lu_scratch;               // row orders of the second factorisation (launch_lu_inplace)
        DeviceBuffer<double> eig_vecs, eig_part; // the folded eigenpair step: what k_eigpair_fold_half leaves behind
    } fold;
    // the folded secant eigenpair step (eigpair_fold.hip)
    int eigpair_fold = 0;          // emme_ctx_set_eigpair_fold (EMME_EIGPAIR_FOLD read at creation)
    int last_folded_eigpair_steps = 0;  // steps of the last eigenpair search that ran folded
    PinnedBuffer<int> p_act;       // pinned host copies of d_active / d_intervals / omega / the deferred
    PinnedBuffer<unsigned long long> p_iv;  // count, WRITTEN BY KERNELS (k_retire, k_newton_update): the
    PinnedBuffer<double> p_w;      // Newton loop reads them after its one synchronisation per step
    PinnedBuffer<unsigned int> p_deferred;
    DeviceBuffer<unsigned int> d_overflow;  // per item: integrals that left the dense fill because a level list was full
    PinnedBuffer<unsigned int> p_overflow;  // ... published by k_retire
    emme::StepFeedback fb;         // a root search's item costs and wide items; the previous fill's deferred count
    emme::StagingRing lists;       // per-launch index lists (omega order | chunks; LU items) on their way to the device
    bool ext_failed = false;
    DeviceBuffer<unsigned long long> d_defer_info;  // missing interval of every deferred integral
    double cache_bytes_used = 0.0;
    DeviceBuffer<double> d_scale;  // half-widths of the cached intervals
    DeviceBuffer<unsigned long long> d_worklist;  // integrals deferred to the cooperative kernel
    DeviceBuffer<unsigned int> d_worklist_count;
    // the tile fill's own work list: as the minority pass of a cached call it must leave the cached fill's list, count
    // and missing intervals alone (the next fill grows the cache from them)
    DeviceBuffer<unsigned long long> d_tile_worklist;
    DeviceBuffer<unsigned int> d_tile_count;
    DeviceBuffer<double> d_M, d_Mold, d_Mp, d_work;  // matrix sets
    DeviceBuffer<double> d_iterates;
    DeviceBuffer<double> d_vecs, d_resid;  // eigenpair search: the chains' vectors [n][dim], residuals [n]
    PinnedBuffer<int> p_live;      // ... and, in the secant loop, d_active as the step's update left it
    int last_n = 0;
    // profiling
    bool prof = false;
    emme_profile_t acc{};
    struct Span {
        int kind;
        hipEvent_t a, b;
    };
    std::vector<Span> spans;
    std::vector<hipEvent_t> free_events;

    // what the fill kernels read of the node cache
    emme::NodeCacheView cache_view() const {
        emme::NodeCacheView v{&cache_geom, {}, {}, {}, {}, {}, d_scale};
        for (int k = 0; k < 2; ++k) {
            v.recs[k] = cache[k].recs;
            for (int e = 0; e < NODE_CACHE_MAX_SUB - 1; ++e) v.recs_ext[k][e] = cache[k].recs_ext[e];
            v.ttab[k] = cache[k].ttab, v.wtab[k] = cache[k].wtab, v.tile_poison[k] = cache[k].tile_poison;
        }
        return v;
    }
    ~emme_ctx() {
        // the records go back to the pool in this order (class 0 main, its subtrees, class 1 ...): the pool evicts
        // its oldest entries first
        for (auto& k : cache) {
            k.recs.reset();
            for (auto& e : k.recs_ext) e.reset();
        }
        for (auto& s : spans) (void)hipEventDestroy(s.a), (void)hipEventDestroy(s.b);
        for (auto e : free_events) (void)hipEventDestroy(e);
    }
};

namespace emme {

// ---- ctx_cache.hip: buffer pool (pool_alloc / pool_free / malloc_retry: buffers.hpp) and node cache ------------
void pool_release_all();
// what a tiled cache allocated now would be laid out over: the half list on a symmetric grid -- electrostatic GK15, or
// any shape under EMME_MIRROR_SHAPES_ALL -- unless switched off or the context serves cached
// derivative fills (their kernels read the full list)
inline bool mirror_shape_ok(const emme_ctx* c) {
    return (c->nm == 1 && c->p.integration_start_points == 15) || c->mirror_shapes == EMME_MIRROR_SHAPES_ALL;
}
inline bool mirror_wanted(const emme_ctx* c) {
    return c->mirror_ok && mirror_shape_ok(c) && c->mirror_opt != 0 && c->tiled && c->opt.deriv_cached == 0;
}
// pairs the tiled cache is laid out over, and with it its builder, the dense fill and the deferred pass
inline int cache_npairs(const emme_ctx* c) { return c->mirror ? c->npairs_half : c->npairs; }
long cache_items(const emme_ctx* c);
size_t cache_part_bytes(const emme_ctx* c, int gk_points, const NodeCacheGeom& g, int part);
// a cached derivative request has reached a mirrored cache: the context gives mirroring up for good
int drop_mirror(emme_ctx* c);
bool ensure_node_cache(emme_ctx* c, const AssembleLaunch& L, int cls);
void add_cache_subtree(emme_ctx* c, const AssembleLaunch& L, int depth, unsigned long long path, int cls);

// ---- ctx_fill.hip: the fill dispatcher ------------------------------------------------------------------
// One fill of M(omega) for a batch.  Pointers starting with d_ are device memory, host_ their host images.
struct FillRequest {
    int nbatch;
    const double* d_omega;
    const double* host_omega = nullptr;  // the omegas' host values: without them the node cache is not used
    const int* d_active = nullptr;       // which items to assemble (null = all), and its host image
    const int* host_active = nullptr;
    double* d_M;
    double* d_Md = nullptr;              // set: the exact dM/domega beside M; through the node cache
                                         // only with the option deriv_cached, where k_assemble_dense_deriv or (derivative
                                         // cache shapes ALL) k_assemble_dense_shape_deriv applies
    const double* d_Mold = nullptr;      // fused secant: Mp = (M - Mold) / domega
    double* d_Mp = nullptr;
    const double* d_domega = nullptr;
    const unsigned long long* cost = nullptr;  // per item (interval count of its previous fill): orders the omegas
    bool newton_loop = false;            // a fill of a root search (skip_lost, wide items, deferred count published)
    bool force_uncached = false;         // omega-lane kernel whatever the batch size and the cache
    const int* d_set = nullptr;          // set: item b belongs to the bound parameter set d_set[b]: the
    const int* host_set = nullptr;       // fills over sets (launch_sets); and its host image
    bool may_mirror = true;              // false: a node cache this request is the first to allocate is laid out over the
                                         // full pair list (the region searches: their nodes' matrices, and with them the
                                         // roots they return, are pinned bit for bit to that list -- DESIGN.md 5.0c)
    FillRequest(int n, const double* omega, double* M) : nbatch(n), d_omega(omega), d_M(M) {}
};
int fill(emme_ctx* c, const FillRequest& r);

// ---- emme_capi.hip ----------------------------------------------------------------------------------------
hipEvent_t get_event(emme_ctx* c);
int require_device();                        // EMME_EDEVICE where there is no HIP device
int check_npoints(const emme_params_t* p);  // EMME_EINVAL outside [2, 65535]
// the kernels' scalars and tables (eta | g | b) of a parameter set
void dev_params_from(const emme_params_t* p, DevParams& P, std::vector<double>& tab);
bool is_device_ptr(const void* p);
// *dev <- a and b are device pointers; EMME_EINVAL ("<names> must both be ...") if only one of them is
int same_side(const void* a, const void* b, const char* names, bool* dev);
// the same for n arrays: EMME_EINVAL ("<names> must all be ...") unless every one is on the side of the first
int same_side_all(const void* const* ptrs, int n, const char* names, bool* dev);
// bytes of nbatch complex n x n matrices
inline size_t batch_bytes(int n, int nbatch) { return (size_t)n * n * 2 * sizeof(double) * nbatch; }
// a call over parameter sets: EMME_EINVAL unless sets are bound and every set[b] names one; the indices into c->d_set
int check_set_indices(const emme_ctx* c, const int* set, int n, const char* who);
int upload_set_indices(emme_ctx* c, const int* set, int n);
int ensure_batch(emme_ctx* c, int nb);            // batch scratch for nb items
int ensure_mats(emme_ctx* c, int nb, int sets);  // matrix sets for nb items: bit0 M, bit1 Mold, bit2 Mp, bit3 work
// around a fill: the batch's omegas into d_omega; interval counts and status flags zeroed; afterwards the counts
// read back (into `intervals` if given, and the profile) -- synchronises; EMME_ENUMERIC if an item's flag is set
// (*bad_item, if given: the first such item)
int upload_omega(emme_ctx* c, const double* omega, int n, hipMemcpyKind kind = hipMemcpyHostToDevice);
int reset_fill_counters(emme_ctx* c, int n);
int collect_fill_status(emme_ctx* c, int n, long long* intervals, int* bad_item = nullptr);
// its two halves, for callers with read-backs of their own: queue the copies of d_intervals (and, st given, d_status)
// into the caller's vectors; after the caller's synchronisation, add the counts to the profile (and to `intervals`)
// and return the first flagged item, -1 if none
int queue_fill_counters(emme_ctx* c, int n, std::vector<unsigned long long>& iv, std::vector<int>* st);
int fold_fill_counters(emme_ctx* c, const std::vector<unsigned long long>& iv, const std::vector<int>* st,
                       long long* intervals = nullptr);

// ---- ctx_linstep.hip --------------------------------------------------------------------------------------
int check_method(const emme_ctx* c, int method);
// One Newton linear step on the batch: leaves tr[b] with domega = -1/tr[b] (h_active: host copy of `active`, null =
// all live; work_ready: work holds M already)
hipError_t linear_step(emme_ctx* c, int method, int n, int nbatch, const double* M, double* work, double* Mp,
                       const int* active, double* tr, int* info, const int* h_active = nullptr, bool work_ready = false);
// The trace-secant step folded into two half-size problems: whether an order qualifies (the option, an
// even order, the blocked one-workgroup kernels for n / 2), and the step itself on symmetric matrices that are
// centrosymmetric apart from their last row and column.  Reads the upper triangles of M and Mold, leaves tr / info of
// the live chains; Mold_w (nullable): M_old = M there, upper triangle only.  work and Mp hold nbatch n x n matrices each
// (the half problems' work copies and right-hand sides); h_active: host copy of `active` (null: all live).
// halves_fit: the order alone -- even, and n / 2 within the blocked one-workgroup kernels (not lu_unblocked).
bool halves_fit(const emme_ctx* c, int n);
bool fold_applies(const emme_ctx* c, int n);
int folded_secant_step(emme_ctx* c, int n, int nbatch, const double* M, const double* Mold, double* Mold_w, double* work,
                       double* Mp, const double* domega, const int* active, double* tr, int* info, const int* h_active);
// The secant eigenpair step folded the same way: whether an order qualifies (even, the blocked
// one-workgroup kernels for n / 2; no option is consulted), and the step on matrices of that structure: fold edges and
// pass, ONE k_lu_inplace per half problem, k_eigpair_fold_half, k_eigpair_fold_combine.  Reads the upper triangles of M
// and Mold and the chains' unit vectors in `vecs`; leaves the new vectors there, tau, resid (before the step) and info
// of the live chains.  work and Mp as above; h_live: host flags, 1 = the chain takes the step (null: every chain).
bool eigpair_fold_applies(const emme_ctx* c, int n);
int folded_eigpair_secant_step(emme_ctx* c, int n, int nbatch, const double* M, const double* Mold, double* work, double* Mp,
                               const double* domega, const int* active, const int* h_live, double* vecs, double* tau,
                               double* resid, int* info);
// scratch of lu_factor_batch that the caller keeps until what it queued behind the factorisation has run
struct LuScratch {
    DeviceBuffer<double> b;  // dummy right-hand sides of the chunked multi-workgroup factorisation
    DeviceBuffer<int> maps;  // row order of the unblocked factorisation
};
int lu_factor_batch(emme_ctx* c, int n, int nbatch, double* work, LuScratch& s, const char* who,
                    const std::function<hipError_t(int b0, int nb, const int* maps, int map_nb, const int* lu_info)>& after,
                    const int* d_items = nullptr, int nitems = 0);

// The live items of a launch as a device list, from host flags: item b with keep(flags[b]) gives `width` entries,
// width b .. width b + width - 1 (1: the item itself; 2: the two half problems of chain b, side by side).
// live_list_fill grows d_list, takes a pinned slot of c->lists and fills it with *count entries; live_list_send queues
// their copy to d_list on c->stream; stage_live_list is both, and sends nothing where the list is empty -- the caller
// returns early on *count == 0.
template <class Keep>
hipError_t live_list_fill(emme_ctx* c, DeviceBuffer<int>& d_list, const int* flags, int n, int width, Keep keep, int** slot,
                          int* count) {
    hipError_t e = d_list.grow(sizeof(int) * (size_t)n * width);
    if (e == hipSuccess) e = c->lists.take((size_t)n * width, slot);
    if (e != hipSuccess) return e;
    *count = 0;
    for (int b = 0; b < n; ++b)
        if (keep(flags[b]))
            for (int k = 0; k < width; ++k) (*slot)[(*count)++] = width * b + k;
    return hipSuccess;
}
inline hipError_t live_list_send(emme_ctx* c, const int* slot, int* d_list, int count) {
    const hipError_t e = emme::launch_stage_ints(slot, d_list, count, nullptr, 0, c->stream);
    return e == hipSuccess ? c->lists.read_on(c->stream) : e;
}
template <class Keep>
hipError_t stage_live_list(emme_ctx* c, DeviceBuffer<int>& d_list, const int* flags, int n, int width, Keep keep, int* count) {
    int* slot = nullptr;
    const hipError_t e = live_list_fill(c, d_list, flags, n, width, keep, &slot, count);
    return e == hipSuccess && *count > 0 ? live_list_send(c, slot, d_list, *count) : e;
}

// host wall time of the cache allocations (hipMalloc of tens of GB: the cold cost of a context)
struct AllocTimer {
    emme_ctx* c;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    bool running = true;
    explicit AllocTimer(emme_ctx* ctx) : c(ctx) {}
    void stop() {
        if (running) {
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            c->acc.cache_alloc_ms += ms;
            if (std::getenv("EMME_DEBUG")) fprintf(stderr, "[emme] node cache: allocation took %.1f ms\n", ms);
        }
        running = false;
    }
    ~AllocTimer() { stop(); }
};

struct ScopedSpan {
    emme_ctx* c;
    int kind;
    hipStream_t st;
    hipEvent_t a = nullptr, b = nullptr;
    ScopedSpan(emme_ctx* ctx, int k, hipStream_t on = nullptr, bool use_on = false)
        : c(ctx), kind(k), st(use_on ? on : ctx->stream) {
        if (c->prof) {
            a = get_event(c);
            b = get_event(c);
            if (a) (void)hipEventRecord(a, st);
        }
    }
    ~ScopedSpan() {
        if (c->prof && a && b) {
            (void)hipEventRecord(b, st);
            c->spans.push_back({kind, a, b});
        }
    }
};

}  // namespace emme
