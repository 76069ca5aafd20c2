// emme_capi.hip -- the context of the C ABI declared in include/emme_hip.h (device tables, batch scratch, options,
// stream, profiling), the helpers around a fill that its translation units share (ctx.hpp), and the assembly entry
// points, which stand where the reference has matrixAssembler (include/solver.h:417-515).  The linear step is in
// ctx_linstep.hip, the root searches in ctx_search.hip, the probes in probe.hip.
#include "ctx.hpp"

namespace emme {

static thread_local std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }

bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // plain host memory: clear the sticky error
        return false;
    }
    return attr.type == hipMemoryTypeDevice;
}

hipEvent_t get_event(emme_ctx* c) {
    if (!c->free_events.empty()) {
        hipEvent_t e = c->free_events.back();
        c->free_events.pop_back();
        return e;
    }
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

int upload_omega(emme_ctx* c, const double* omega, int n, hipMemcpyKind kind) {
    HIP_TRY(hipMemcpyAsync(c->d_omega, omega, sizeof(double) * 2 * n, kind, c->stream));
    return EMME_OK;
}

int reset_fill_counters(emme_ctx* c, int n) {
    HIP_TRY(hipMemsetAsync(c->d_intervals, 0, sizeof(unsigned long long) * n, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_status, 0, sizeof(int) * n, c->stream));
    return EMME_OK;
}

int queue_fill_counters(emme_ctx* c, int n, std::vector<unsigned long long>& iv, std::vector<int>* st) {
    iv.resize(n);
    HIP_TRY(hipMemcpyAsync(iv.data(), c->d_intervals, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, c->stream));
    if (!st) return EMME_OK;
    st->resize(n);
    HIP_TRY(hipMemcpyAsync(st->data(), c->d_status, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    return EMME_OK;
}

int fold_fill_counters(emme_ctx* c, const std::vector<unsigned long long>& iv, const std::vector<int>* st, long long* intervals) {
    int bad = -1;
    for (size_t b = 0; b < iv.size(); ++b) {
        c->acc.gk_intervals += (long long)iv[b];
        if (intervals) intervals[b] = (long long)iv[b];
        if (st && (*st)[b] != 0 && bad < 0) bad = (int)b;
    }
    return bad;
}

int collect_fill_status(emme_ctx* c, int n, long long* intervals, int* bad_item) {
    std::vector<unsigned long long> iv;
    std::vector<int> stv;
    EMME_TRY(queue_fill_counters(c, n, iv, &stv));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int bad = fold_fill_counters(c, iv, &stv, intervals);
    if (bad < 0) return EMME_OK;
    if (bad_item) *bad_item = bad;
    set_error("quadrature depth cap hit or non-finite integral in at least one item");
    return EMME_ENUMERIC;
}

int ensure_batch(emme_ctx* c, int nb) {
    const size_t n = (size_t)nb;
    HIP_TRY(c->d_omega.grow(sizeof(double) * 2 * n));
    HIP_TRY(c->d_domega.grow(sizeof(double) * 2 * n));
    HIP_TRY(c->d_tr.grow(sizeof(double) * 2 * n));
    HIP_TRY(c->d_active.grow(sizeof(int) * n));
    HIP_TRY(c->d_iters.grow(sizeof(int) * n));
    HIP_TRY(c->d_info.grow(sizeof(int) * n));
    HIP_TRY(c->d_status.grow(sizeof(int) * n));
    HIP_TRY(c->d_intervals.grow(sizeof(unsigned long long) * n));
    HIP_TRY(c->d_overflow.grow(sizeof(unsigned int) * n));  // (zeroed by the root search, its only user)
    HIP_TRY(c->d_actidx.grow(sizeof(int) * n));
    HIP_TRY(c->d_chunks.grow(sizeof(int) * 3 * n));  // (first, size) per chunk | position map
    HIP_TRY(c->p_act.grow(sizeof(int) * n));
    HIP_TRY(c->p_iv.grow(sizeof(unsigned long long) * n));
    HIP_TRY(c->p_w.grow(sizeof(double) * 2 * n));
    HIP_TRY(c->p_overflow.grow(sizeof(unsigned int) * n));
    HIP_TRY(c->p_deferred.grow(sizeof(unsigned int)));
    HIP_TRY(c->lists.reserve(4 * n));  // omega order | chunks | position map of a fill; the live matrices of an LU
    if (!c->d_rounds) {
        HIP_TRY(c->d_rounds.grow((16 + 8192) * sizeof(unsigned long long)));  // (+ per-tile ticks of the diagnostic build)
        HIP_TRY(hipMemset(c->d_rounds, 0, (16 + 8192) * sizeof(unsigned long long)));
    }
    return EMME_OK;
}

// which matrix sets a call needs: bit0 M, bit1 Mold, bit2 Mp, bit3 work
int ensure_mats(emme_ctx* c, int nb, int sets) {
    const size_t bytes = batch_bytes(c->dim, nb);
    DeviceBuffer<double>* mats[4] = {&c->d_M, &c->d_Mold, &c->d_Mp, &c->d_work};
    for (int k = 0; k < 4; ++k)
        if (sets & (1 << k)) HIP_TRY(mats[k]->grow(bytes));
    return EMME_OK;
}

// The kernels' scalars and tables (eta | g | b) of a parameter set: what every context launches with, and what the
// probe entry points (emme_integrand_batch, probe.hip) evaluate single nodes with.
void dev_params_from(const emme_params_t* p, DevParams& P, std::vector<double>& tab) {
    const int N = p->npoints;
    const bool es = std::fpclassify(p->beta_e) == FP_ZERO;  // include/solver.h:406-407
    tab.assign(3 * (size_t)N, 0.0);
    double dx = 0;
    emme_tables(p, tab.data(), tab.data() + N, tab.data() + 2 * N, &dx);
    P.N = N, P.dim = es ? N : 2 * N, P.nm = es ? 1 : 3, P.max_sub = p->integration_iteration_limit;
    P.dx = dx;
    P.inv_arc = 1.0 / p->arc_coeff;
    P.qR = p->q * p->R;
    P.vt = p->vt;
    P.cb = (p->q * p->R) / p->vt * (p->omega_d_bar);                                  // :88
    P.cbe = (p->q * p->R) / p->vt * (p->omega_d_bar * p->omega_s_e / p->omega_s_i);  // :93
    P.omega_s_i = p->omega_s_i, P.omega_s_e = p->omega_s_e;
    P.eta_i = p->eta_i, P.eta_e = p->eta_e, P.tau = p->tau;
    P.rel_tol = p->integration_precision;
    P.prec_goal = p->integration_accuracy;
    P.pref = (p->q * p->R) / (p->vt * std::sqrt(2.0 * M_PI));
    P.diag_a = 1.0 + 1.0 / p->tau;
    P.diag_d = es ? 0.0 : (2.0 * p->tau) / p->beta_e;
}

int check_set_indices(const emme_ctx* c, const int* set, int n, const char* who) {
    if (c->sets.empty()) {
        set_error(std::string(who) + ": no parameter sets are bound to the context (emme_ctx_bind_param_sets)");
        return EMME_EINVAL;
    }
    for (int b = 0; b < n; ++b)
        if (set[b] < 0 || set[b] >= (int)c->sets.size()) {
            set_error(std::string(who) + ": set[" + std::to_string(b) + "] = " + std::to_string(set[b]) + " is outside [0, " +
                      std::to_string(c->sets.size()) + ")");
            return EMME_EINVAL;
        }
    return EMME_OK;
}

int upload_set_indices(emme_ctx* c, const int* set, int n) {
    HIP_TRY(c->d_set.grow(sizeof(int) * (size_t)n));
    // (pageable host memory: the copy has left `set` when the call returns)
    HIP_TRY(hipMemcpyAsync(c->d_set, set, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    return EMME_OK;
}

int require_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        set_error("no HIP device available (the MI355X path has no CPU fallback)");
        return EMME_EDEVICE;
    }
    return EMME_OK;
}

int check_npoints(const emme_params_t* p) {
    if (p->npoints < 2 || p->npoints > 65535) {
        set_error("npoints must be in [2, 65535]");
        return EMME_EINVAL;
    }
    return EMME_OK;
}

int same_side(const void* a, const void* b, const char* names, bool* dev) {
    *dev = is_device_ptr(a);
    if (*dev == is_device_ptr(b)) return EMME_OK;
    set_error(std::string(names) + " must both be host or both be device pointers");
    return EMME_EINVAL;
}

int same_side_all(const void* const* ptrs, int n, const char* names, bool* dev) {
    *dev = is_device_ptr(ptrs[0]);
    for (int k = 1; k < n; ++k)
        if (is_device_ptr(ptrs[k]) != *dev) {
            set_error(std::string(names) + " must all be host or all be device pointers");
            return EMME_EINVAL;
        }
    return EMME_OK;
}

}  // namespace emme

using namespace emme;

namespace {

int drain_spans(emme_ctx* c) {
    for (auto& s : c->spans) {
        HIP_TRY(hipEventSynchronize(s.b));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s.a, s.b));
        if (s.kind == K_ASM)
            c->acc.assemble_ms += ms, c->acc.assemble_launches++;
        else if (s.kind == K_LIN)
            c->acc.linstep_ms += ms, c->acc.linstep_launches++;
        else if (s.kind == K_DEFER)
            c->acc.deferred_ms += ms, c->acc.deferred_launches++;
        else if (s.kind == K_CACHE)
            c->acc.cache_build_ms += ms, c->acc.cache_build_launches++;
        else if (s.kind == K_NULL)
            c->acc.nullspace_ms += ms, c->acc.nullspace_launches++;
        else
            c->acc.other_ms += ms, c->acc.other_launches++;
        c->free_events.push_back(s.a);
        c->free_events.push_back(s.b);
    }
    c->spans.clear();
    return EMME_OK;
}

// one fill of a plain assembly call: the omegas into d_omega, counters zeroed, M (and, dMd given, the exact
// derivative) queued.  The node cache needs the omegas' host values: the derivative entry point, which also takes
// device omegas, hands them on only with the option deriv_cached, and only if they are on the host.
int fill_at(emme_ctx* c, const double* omega, int nbatch, double* dM, double* dMd, hipMemcpyKind kind) {
    EMME_TRY(upload_omega(c, omega, nbatch, kind));
    EMME_TRY(reset_fill_counters(c, nbatch));
    FillRequest r(nbatch, c->d_omega, dM);
    r.d_Md = dMd;
    if (!dMd || (c->opt.deriv_cached != 0 && !is_device_ptr(omega))) r.host_omega = omega;
    return fill(c, r);
}

}  // namespace

extern "C" {

const char* emme_last_error(void) { return g_error.c_str(); }
int emme_version(void) { return 4; }

void emme_options_default(emme_options_t* opt) {
    if (opt) options_default(*opt);
}

int emme_ctx_create(const emme_params_t* p, int device, emme_ctx_t** out) {
    return emme_ctx_create_ex(p, device, nullptr, out);
}

int emme_ctx_create_ex(const emme_params_t* p, int device, const emme_options_t* opt, emme_ctx_t** out) {
    if (!p || !out) return EMME_EINVAL;
    *out = nullptr;
    emme_options_t o;
    options_default(o);
    if (opt) {
        EMME_TRY(options_check(opt));
        o = *opt;
    }
    options_env_overrides(o);
    EMME_TRY(options_check(&o));
    if (p->integration_start_points != 15 && p->integration_start_points != 31) {
        // include/functions.h:329
        set_error("integration_start_points should be 15 or 31");
        return EMME_ECONFIG;
    }
    EMME_TRY(check_npoints(p));
    EMME_TRY(require_device());
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
        set_error(std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950");
        return EMME_EDEVICE;
    }

    emme_ctx* c = new emme_ctx;
    c->p = *p;
    c->device = device;
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c->opt = o;
    // (developer override, read once per context like the options': EMME_TILE_SHAPES=1 is emme_ctx_set_tile_shapes(ALL))
    if (const char* v = std::getenv("EMME_TILE_SHAPES"))
        c->tile_shapes = std::atoi(v) == EMME_TILE_SHAPES_ALL ? EMME_TILE_SHAPES_ALL : EMME_TILE_SHAPES_ES15;
    // (the same for the shapes of deriv_cached: EMME_DERIV_CACHE_SHAPES=1 is emme_ctx_set_deriv_cache_shapes(ALL))
    if (const char* v = std::getenv("EMME_DERIV_CACHE_SHAPES"))
        c->deriv_cache_shapes =
            std::atoi(v) == EMME_DERIV_CACHE_SHAPES_ALL ? EMME_DERIV_CACHE_SHAPES_ALL : EMME_DERIV_CACHE_SHAPES_ES15;
    const int N = p->npoints;
    c->N = N;
    const bool es = std::fpclassify(p->beta_e) == FP_ZERO;  // include/solver.h:406-407
    c->dim = es ? N : 2 * N;
    c->nm = es ? 1 : 3;
    // electromagnetic contexts share one node record per (pair, interval, node) between the three
    // moments (EMME_EM_SHARED=0: one record per moment, for A/B comparisons)
    c->em_shared = !es && o.em_shared != 0;
    // phase_table = 0: unfolded records and exp(A0 + T omega) per (pair, node, omega) in the fill
    c->folded = o.phase_table != 0;
    // electrostatic GK15 on folded records: tiled record layout + dense fill on the FP64 matrix cores
    // (assemble_dense.hip) instead of the union walk (EMME_DENSE=0 restores that).  It
    // carries the safe_exp-clamped tails (<= 4e-14 absolute), so inputs whose absolute quadrature goal
    // (integration_accuracy) is tighter than 1e-9 keep the exact union kernel.
    c->tiled = wants_tiled(*p, c->folded, o.fill);

    DevParams& P = c->P;
    std::vector<double> tab;
    dev_params_from(p, P, tab);

    // pair list ordered by diagonal offset (see assemble.hip header), and one pair of every mirror-image couple
    std::vector<PairIJ> pairs, half;
    full_pair_list(N, pairs);
    half_pair_list(N, half);
    c->npairs = (int)pairs.size();
    c->npairs_half = (int)half.size();
    // Mirror-image pairs share their integral where the grid is symmetric (theta = 0): eta, g odd and b even to 1e-13
    // of the table's largest value -- 30 times the rounding of the tables themselves (3e-15), nine orders below a real
    // asymmetry (theta = 0.3: 3e-2).  Which shapes then mirror is mirror_wanted's rule (electrostatic GK15, or every
    // shape under EMME_MIRROR_SHAPES_ALL: and only on the tiled layout, which emme_ctx_set_options may still change
    // while no cache exists).
    c->mirror_ok = grid_is_mirror_symmetric(tab.data(), N, 1e-13);
    // (developer override, read once per context: EMME_MIRROR=0 is emme_ctx_set_mirror_pairs(0))
    if (const char* v = std::getenv("EMME_MIRROR")) c->mirror_opt = std::atoi(v) != 0;
    // (and EMME_MIRROR_SHAPES=1 is emme_ctx_set_mirror_shapes(EMME_MIRROR_SHAPES_ALL))
    if (const char* v = std::getenv("EMME_MIRROR_SHAPES"))
        c->mirror_shapes = std::atoi(v) == EMME_MIRROR_SHAPES_ALL ? EMME_MIRROR_SHAPES_ALL : EMME_MIRROR_SHAPES_ES15;
    // (the same for the folded trace-secant step, DESIGN.md 5.4c: EMME_LU_FOLD=0 is emme_ctx_set_lu_fold(0))
    if (const char* v = std::getenv("EMME_LU_FOLD")) c->lu_fold = std::atoi(v) != 0;
    // (and for the folded secant eigenpair step, DESIGN.md 14.2: EMME_EIGPAIR_FOLD=1 is emme_ctx_set_eigpair_fold(1))
    if (const char* v = std::getenv("EMME_EIGPAIR_FOLD")) c->eigpair_fold = std::atoi(v) != 0;

    auto fail = [&](int code) {
        emme_ctx_destroy(c);
        return code;
    };
    if (c->d_tab.grow(tab.size() * sizeof(double)) != hipSuccess ||
        c->d_pairs.grow(pairs.size() * sizeof(ushort2)) != hipSuccess ||
        c->d_pairs_half.grow(half.size() * sizeof(ushort2)) != hipSuccess) {
        set_error("hipMalloc failed for tables");
        return fail(EMME_ENOMEM);
    }
    if (hipMemcpy(c->d_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->d_pairs, pairs.data(), pairs.size() * sizeof(ushort2), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->d_pairs_half, half.data(), half.size() * sizeof(ushort2), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("hipMemcpy failed for tables");
        return fail(EMME_EDEVICE);
    }
    *out = c;
    return EMME_OK;
}

void emme_ctx_destroy(emme_ctx_t* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    else (void)hipDeviceSynchronize();
    delete c;
}

void emme_release_pooled_memory(void) { pool_release_all(); }

int emme_ctx_set_options(emme_ctx_t* c, const emme_options_t* opt) {
    if (!c || !opt) return EMME_EINVAL;
    EMME_TRY(options_check(opt));
    const bool layout_differs = opt->fill != c->opt.fill || (opt->phase_table != 0) != (c->opt.phase_table != 0) ||
                                (opt->em_shared != 0) != (c->opt.em_shared != 0);
    if (layout_differs) {
        if (c->cache[0].recs || c->cache[1].recs) {
            set_error("emme_ctx_set_options: fill / phase_table / em_shared fix the layout of the node cache, which exists already");
            return EMME_EINVAL;
        }
        const bool es = c->nm == 1;
        c->em_shared = !es && opt->em_shared != 0;
        c->folded = opt->phase_table != 0;
        c->tiled = wants_tiled(c->p, c->folded, opt->fill);
    }
    if (opt->node_cache_gb > 0.0 && c->cache_depth == -2 && !c->cache[0].recs && !c->cache[1].recs)
        c->cache_depth = -1;  // a budget after "no cache": decide again
    if (opt->lu_split != c->opt.lu_split) c->lu_one_wg = false;
    c->opt = *opt;
    return EMME_OK;
}

int emme_ctx_get_options(const emme_ctx_t* c, emme_options_t* opt) {
    if (!c || !opt) return EMME_EINVAL;
    *opt = c->opt;
    return EMME_OK;
}

int emme_ctx_set_tile_shapes(emme_ctx_t* c, int shapes) {
    if (!c) {
        set_error("emme_ctx_set_tile_shapes: NULL context");
        return EMME_EINVAL;
    }
    if (shapes != EMME_TILE_SHAPES_ES15 && shapes != EMME_TILE_SHAPES_ALL) {
        set_error("emme_ctx_set_tile_shapes: value out of range (EMME_TILE_SHAPES_ES15, EMME_TILE_SHAPES_ALL)");
        return EMME_EINVAL;
    }
    c->tile_shapes = shapes;
    return EMME_OK;
}

int emme_ctx_get_tile_shapes(const emme_ctx_t* c) { return c ? c->tile_shapes : EMME_EINVAL; }

int emme_ctx_set_mirror_pairs(emme_ctx_t* c, int on) {
    if (!c) {
        set_error("emme_ctx_set_mirror_pairs: NULL context");
        return EMME_EINVAL;
    }
    if (on != 0 && on != 1) {
        set_error("emme_ctx_set_mirror_pairs: value out of range (0, 1)");
        return EMME_EINVAL;
    }
    if (c->cache[0].recs || c->cache[1].recs) {
        set_error("emme_ctx_set_mirror_pairs: the pair list fixes the layout of the node cache, which exists already");
        return EMME_EINVAL;
    }
    c->mirror_opt = on;
    return EMME_OK;
}

int emme_ctx_get_mirror_pairs(const emme_ctx_t* c) {
    if (!c) return EMME_EINVAL;
    return (c->cache[0].recs || c->cache[1].recs) ? (int)c->mirror : (int)mirror_wanted(c);
}

int emme_ctx_set_mirror_shapes(emme_ctx_t* c, int shapes) {
    if (!c) {
        set_error("emme_ctx_set_mirror_shapes: NULL context");
        return EMME_EINVAL;
    }
    if (shapes != EMME_MIRROR_SHAPES_ES15 && shapes != EMME_MIRROR_SHAPES_ALL) {
        set_error("emme_ctx_set_mirror_shapes: value out of range (EMME_MIRROR_SHAPES_ES15, EMME_MIRROR_SHAPES_ALL)");
        return EMME_EINVAL;
    }
    if (c->cache[0].recs || c->cache[1].recs) {
        set_error("emme_ctx_set_mirror_shapes: the pair list fixes the layout of the node cache, which exists already");
        return EMME_EINVAL;
    }
    c->mirror_shapes = shapes;
    return EMME_OK;
}

int emme_ctx_get_mirror_shapes(const emme_ctx_t* c) { return c ? c->mirror_shapes : EMME_EINVAL; }

int emme_ctx_set_lu_fold(emme_ctx_t* c, int on) {
    if (!c) {
        set_error("emme_ctx_set_lu_fold: NULL context");
        return EMME_EINVAL;
    }
    if (on != 0 && on != 1) {
        set_error("emme_ctx_set_lu_fold: value out of range (0, 1)");
        return EMME_EINVAL;
    }
    c->lu_fold = on;
    return EMME_OK;
}

int emme_ctx_get_lu_fold(const emme_ctx_t* c) { return c ? c->lu_fold : EMME_EINVAL; }

int emme_ctx_last_folded_steps(const emme_ctx_t* c) { return c ? c->last_folded_steps : EMME_EINVAL; }

int emme_ctx_set_eigpair_fold(emme_ctx_t* c, int on) {
    if (!c) {
        set_error("emme_ctx_set_eigpair_fold: NULL context");
        return EMME_EINVAL;
    }
    if (on != 0 && on != 1) {
        set_error("emme_ctx_set_eigpair_fold: value out of range (0, 1)");
        return EMME_EINVAL;
    }
    c->eigpair_fold = on;
    return EMME_OK;
}

int emme_ctx_get_eigpair_fold(const emme_ctx_t* c) { return c ? c->eigpair_fold : EMME_EINVAL; }

int emme_ctx_last_folded_eigpair_steps(const emme_ctx_t* c) { return c ? c->last_folded_eigpair_steps : EMME_EINVAL; }

// Share of every vector in the even subspace of the flip J: plain host arithmetic, no device
int emme_vector_parity(int n, int nvec, const double* vecs, double* even) {
    if (!vecs || !even || n < 1 || nvec < 1) {
        set_error("emme_vector_parity: a required pointer is NULL, n < 1 or nvec < 1");
        return EMME_EINVAL;
    }
    for (int k = 0; k < nvec; ++k) {
        const double* v = vecs + 2 * (size_t)k * n;
        double ev = 0.0, all = 0.0;
        for (int i = 0; i < n / 2; ++i) {
            const double *p = v + 2 * i, *q = v + 2 * (size_t)(n - 1 - i);
            const double sr = p[0] + q[0], si = p[1] + q[1];
            ev += sr * sr + si * si;
            // (grouped so that an exactly even or odd vector gives exactly 1 or 0)
            all += (p[0] * p[0] + p[1] * p[1]) + (q[0] * q[0] + q[1] * q[1]);
        }
        if (n % 2 != 0) {  // the middle entry is its own mirror image: even
            const double* p = v + 2 * (size_t)(n / 2);
            const double s = p[0] * p[0] + p[1] * p[1];
            ev += 2.0 * s, all += s;
        }
        const double share = ev / (2.0 * all);
        even[k] = (all > 0.0 && std::isfinite(all) && std::isfinite(share)) ? share : std::numeric_limits<double>::quiet_NaN();
    }
    return EMME_OK;
}

const char* emme_ctx_linstep_kernel_symbol(const emme_ctx_t* c) { return c ? c->last_lu_symbol : nullptr; }

int emme_ctx_last_lu_workgroups(const emme_ctx_t* c) { return c ? c->last_lu_nwg : EMME_EINVAL; }

int emme_ctx_last_lu_slices(const emme_ctx_t* c) { return c ? c->last_lu_slices : EMME_EINVAL; }

int emme_ctx_compute_units(const emme_ctx_t* c) { return c ? c->n_cu : EMME_EINVAL; }

int emme_ctx_set_deriv_cache_shapes(emme_ctx_t* c, int shapes) {
    if (!c) {
        set_error("emme_ctx_set_deriv_cache_shapes: NULL context");
        return EMME_EINVAL;
    }
    if (shapes != EMME_DERIV_CACHE_SHAPES_ES15 && shapes != EMME_DERIV_CACHE_SHAPES_ALL) {
        set_error("emme_ctx_set_deriv_cache_shapes: value out of range (EMME_DERIV_CACHE_SHAPES_ES15, EMME_DERIV_CACHE_SHAPES_ALL)");
        return EMME_EINVAL;
    }
    c->deriv_cache_shapes = shapes;
    return EMME_OK;
}

int emme_ctx_get_deriv_cache_shapes(const emme_ctx_t* c) { return c ? c->deriv_cache_shapes : EMME_EINVAL; }

int emme_ctx_set_stream(emme_ctx_t* c, void* s) {
    if (!c) return EMME_EINVAL;
    c->stream = (hipStream_t)s;
    return EMME_OK;
}

int emme_ctx_dim(const emme_ctx_t* c) { return c ? c->dim : EMME_EINVAL; }

int emme_ctx_fill_mode(const emme_ctx_t* c) { return c ? c->last_fill_mode : EMME_EINVAL; }

long long emme_ctx_last_deferred(emme_ctx_t* c) {
    if (!c) return EMME_EINVAL;
    const unsigned int* src = c->last_fill_listed >= 2 ? c->d_tile_count.get() : c->d_worklist_count.get();
    if (!c->last_fill_listed || !src) return 0;
    HIP_TRY(hipSetDevice(c->device));
    // (a tile fill over parameter sets has a counter per bound set: their sum)
    std::vector<unsigned int> cnts(c->last_fill_listed == 3 ? (size_t)c->last_fill_counters : 1, 0u);
    HIP_TRY(hipMemcpyAsync(cnts.data(), src, sizeof(unsigned int) * cnts.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    long long cnt = 0;
    for (unsigned int v : cnts) cnt += v;
    return cnt;
}

double emme_ctx_node_cache_gib(const emme_ctx_t* c) {
    return c ? c->cache_bytes_used / (1024.0 * 1024.0 * 1024.0) : 0.0;
}

int emme_ctx_profile_enable(emme_ctx_t* c, int on) {
    if (!c) return EMME_EINVAL;
    c->prof = on != 0;
    return EMME_OK;
}

int emme_ctx_profile_read(emme_ctx_t* c, emme_profile_t* out, int reset) {
    if (!c || !out) return EMME_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    EMME_TRY(drain_spans(c));
    c->acc.integrand_evals = c->acc.gk_intervals * c->p.integration_start_points;
    if (c->d_rounds) {
        unsigned long long r[16] = {};
        HIP_TRY(hipMemcpy(r, c->d_rounds, sizeof r, hipMemcpyDeviceToHost));
        if (std::getenv("EMME_DEBUG_STAMPS") && r[10])
            fprintf(stderr, "[emme] dense fill: %llu integrals handed over because a level list overflowed\n", r[10]);
        if (std::getenv("EMME_DEBUG_STAMPS") && r[8])  // diagnostic build (EMME_DENSE_STAMPS) only
            fprintf(stderr, "[emme] dense stamps: select %.3g  dense %.3g  sparse %.3g  decide %.3g  task total %.3g  "
                    "longest task %.3g cycles; per round: select %.0f dense %.0f sparse %.0f decide %.0f\n",
                    (double)r[4], (double)r[5], (double)r[6], (double)r[7], (double)r[8], (double)r[9],
                    (double)r[4] / (double)(r[0] + r[1] + 1), (double)r[5] / (double)(r[0] + 1),
                    (double)r[6] / (double)(r[1] + 1), (double)r[7] / (double)(r[0] + r[1] + 1));
        if (c->tiled || c->last_fill_mode == FILL_TILE || c->last_fill_mode == FILL_TILE_SETS) {
            c->acc.union_rounds = (long long)(r[0] + r[1]);
            c->acc.dense_rounds = (long long)r[0], c->acc.sparse_rounds = (long long)r[1];
            c->acc.sparse_columns = (long long)r[2], c->acc.tile_tasks = (long long)r[3];
        } else {
            c->acc.union_rounds = (long long)r[0];
        }
        if (reset) HIP_TRY(hipMemset(c->d_rounds, 0, sizeof r));
    }
    *out = c->acc;
    if (reset) c->acc = emme_profile_t{};
    return EMME_OK;
}

int emme_assemble_batch(emme_ctx_t* c, const double* omega, int nbatch, double* M,
                        long long* intervals) {
    if (!c || !omega || !M || nbatch < 1) return EMME_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    // (the fill plan reads the omegas on the host: contour classes, cache policy)
    if (is_device_ptr(omega)) {
        set_error("emme_assemble_batch: omega must be a host pointer");
        return EMME_EINVAL;
    }
    EMME_TRY(ensure_batch(c, nbatch));
    const bool dev_out = is_device_ptr(M);
    double* dM = M;
    if (!dev_out) {
        EMME_TRY(ensure_mats(c, nbatch, 1));
        dM = c->d_M;
    }
    EMME_TRY(fill_at(c, omega, nbatch, dM, nullptr, hipMemcpyHostToDevice));
    if (!dev_out)
        HIP_TRY(hipMemcpyAsync(M, dM, batch_bytes(c->dim, nbatch), hipMemcpyDeviceToHost, c->stream));
    return collect_fill_status(c, nbatch, intervals);
}

int emme_ctx_cache_settle(emme_ctx_t* c, const double* omega, int nbatch, int* fills_done) {
    if (!c || !omega || nbatch < 1) return EMME_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    EMME_TRY(ensure_batch(c, nbatch));
    EMME_TRY(ensure_mats(c, nbatch, 1));
    int fills = 0;
    // a fill that deferred integrals makes the NEXT one cache a subtree around the interval most of
    // them were missing; at most NODE_CACHE_MAX_SUB - 1 run-time subtrees per contour class exist, so
    // the shape is final after at most that many growing fills plus one that finds nothing to add
    for (int round = 0; round < 2 * NODE_CACHE_MAX_SUB + 2; ++round) {
        const double before = c->cache_bytes_used;
        EMME_TRY(fill_at(c, omega, nbatch, c->d_M, nullptr, hipMemcpyHostToDevice));
        HIP_TRY(hipStreamSynchronize(c->stream));
        ++fills;
        if (round > 0 && c->cache_bytes_used == before) break;  // this fill found the shape it started with
    }
    if (fills_done) *fills_done = fills;
    return EMME_OK;
}

int emme_ctx_cache_state(const emme_ctx_t* c, int* full_depth, int* subtrees, double* gib) {
    if (!c) return EMME_EINVAL;
    if (full_depth) *full_depth = c->cache_depth;
    if (subtrees) *subtrees = c->cache_depth >= 0 ? c->cache_geom.nsub : 0;
    if (gib) *gib = c->cache_bytes_used / (1024.0 * 1024.0 * 1024.0);
    return EMME_OK;
}

int emme_assemble_derivative_batch(emme_ctx_t* c, const double* omega, int nbatch, double* M, double* Mp,
                                   long long* intervals) {
    if (!c || !omega || !M || !Mp || nbatch < 1) return EMME_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    bool dev_out = false;
    EMME_TRY(same_side(M, Mp, "M and Mp", &dev_out));
    EMME_TRY(ensure_batch(c, nbatch));
    double *dM = M, *dMp = Mp;
    if (!dev_out) {
        EMME_TRY(ensure_mats(c, nbatch, 1 | 4));
        dM = c->d_M, dMp = c->d_Mp;
    }
    EMME_TRY(fill_at(c, omega, nbatch, dM, dMp, hipMemcpyDefault));
    if (!dev_out) {
        HIP_TRY(hipMemcpyAsync(M, dM, batch_bytes(c->dim, nbatch), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(Mp, dMp, batch_bytes(c->dim, nbatch), hipMemcpyDeviceToHost, c->stream));
    }
    return collect_fill_status(c, nbatch, intervals);
}

// ---- parameter sets ---------------------------------------------------------------------------
int emme_ctx_bind_param_sets(emme_ctx_t* c, const emme_params_t* sets, int nsets) {
    if (!c || nsets < 0 || (nsets > 0 && !sets)) {
        set_error("emme_ctx_bind_param_sets: NULL context or sets, or nsets < 0");
        return EMME_EINVAL;
    }
    for (int s = 0; s < nsets; ++s)
        if (emme_params_same_shape(&c->p, &sets[s]) != EMME_OK) {
            set_error("emme_ctx_bind_param_sets: set " + std::to_string(s) + ": " + emme_last_error());
            return EMME_EINVAL;
        }
    if (nsets == 0) {
        c->sets.clear();
        return EMME_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    const size_t tn = 3 * (size_t)c->N;
    std::vector<DevParams> P(nsets);
    std::vector<double> tabs(tn * nsets), tab;
    for (int s = 0; s < nsets; ++s) {
        dev_params_from(&sets[s], P[s], tab);
        std::copy(tab.begin(), tab.end(), tabs.begin() + tn * s);
    }
    // (an earlier call's kernels may still read the old binding)
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->sets.clear();
    HIP_TRY(c->d_sets.grow(sizeof(DevParams) * nsets));
    HIP_TRY(c->d_set_tabs.grow(sizeof(double) * tabs.size()));
    HIP_TRY(hipMemcpy(c->d_sets, P.data(), sizeof(DevParams) * nsets, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_set_tabs, tabs.data(), sizeof(double) * tabs.size(), hipMemcpyHostToDevice));
    c->sets.assign(sets, sets + nsets);
    return EMME_OK;
}

int emme_ctx_param_sets(const emme_ctx_t* c) { return c ? (int)c->sets.size() : EMME_EINVAL; }

int emme_assemble_sets_batch(emme_ctx_t* c, const int* set, const double* omega, int nbatch, double* M, double* Mp,
                             long long* intervals) {
    if (!c || !set || !omega || !M || nbatch < 1) return EMME_EINVAL;
    EMME_TRY(check_set_indices(c, set, nbatch, "emme_assemble_sets_batch"));
    HIP_TRY(hipSetDevice(c->device));
    bool dev_out = is_device_ptr(M);
    if (Mp) EMME_TRY(same_side(M, Mp, "M and Mp", &dev_out));
    EMME_TRY(ensure_batch(c, nbatch));
    double *dM = M, *dMp = Mp;
    if (!dev_out) {
        EMME_TRY(ensure_mats(c, nbatch, Mp ? (1 | 4) : 1));
        dM = c->d_M, dMp = Mp ? c->d_Mp.get() : nullptr;
    }
    EMME_TRY(upload_set_indices(c, set, nbatch));
    EMME_TRY(upload_omega(c, omega, nbatch, hipMemcpyDefault));
    EMME_TRY(reset_fill_counters(c, nbatch));
    FillRequest r(nbatch, c->d_omega, dM);
    r.d_Md = dMp, r.d_set = c->d_set, r.host_set = set;
    // (the tile fill over sets needs the omegas' host values for its chunks: DESIGN.md 13.7; host_active null = all)
    if (!is_device_ptr(omega)) r.host_omega = omega;
    EMME_TRY(fill(c, r));
    if (!dev_out) {
        HIP_TRY(hipMemcpyAsync(M, dM, batch_bytes(c->dim, nbatch), hipMemcpyDeviceToHost, c->stream));
        if (Mp) HIP_TRY(hipMemcpyAsync(Mp, dMp, batch_bytes(c->dim, nbatch), hipMemcpyDeviceToHost, c->stream));
    }
    return collect_fill_status(c, nbatch, intervals);
}

int emme_ctx_get_matrix(emme_ctx_t* c, int b, double* M_host) {
    if (!c || !M_host || b < 0 || b >= c->last_n || !c->d_M) return EMME_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpy(M_host, c->d_M + (size_t)c->dim * c->dim * 2 * b, batch_bytes(c->dim, 1), hipMemcpyDeviceToHost));
    return EMME_OK;
}

}  // extern "C"
