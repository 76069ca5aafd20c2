// emme_capi.hip -- implementation of the C ABI declared in include/emme_hip.h:
// context (device tables, batch scratch, stream, profiling) and the batched drivers that
// stand where the reference has EigenSolver's constructor / matrixAssembler /
// newtonTraceSecantIteration (include/solver.h:396-415, 417-515, 113-160) and the
// solve_once_eigen loop (src/main.cpp:19-80).
#include "ctx.hpp"

namespace emme {

static thread_local std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }

namespace {

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

}  // namespace
}  // namespace emme

using namespace emme;

namespace emme {

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

int collect_fill_status(emme_ctx* c, int n, long long* intervals, int* bad_item) {
    std::vector<unsigned long long> iv(n);
    std::vector<int> stv(n);
    HIP_TRY(hipMemcpyAsync(iv.data(), c->d_intervals, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(stv.data(), c->d_status, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int bad = -1;
    for (int b = 0; b < n; ++b) {
        c->acc.gk_intervals += (long long)iv[b];
        if (intervals) intervals[b] = (long long)iv[b];
        if (stv[b] != 0 && bad < 0) bad = b;
    }
    if (bad < 0) return EMME_OK;
    if (bad_item) *bad_item = bad;
    set_error("quadrature depth cap hit or non-finite integral in at least one item");
    return EMME_ENUMERIC;
}
}  // namespace emme

namespace {

size_t mat_doubles(const emme_ctx* c) { return (size_t)c->dim * c->dim * 2; }

// Which contexts get the tiled record layout + dense (matrix-core) fill (assemble_dense.hip): both quadrature orders,
// electrostatic and electromagnetic (BASELINE.json's configurations use electrostatic GK15 and electromagnetic GK31),
// on folded records, with the default fill option.  The dense path carries the safe_exp-clamped tails (<= 4e-14 absolute), so inputs whose absolute quadrature
// goal (integration_accuracy) is tighter than 1e-9 keep the exact kernels.
bool wants_tiled(const emme_params_t& p, bool es, bool folded, int fill) {
    const bool shape = p.integration_start_points == 15 || p.integration_start_points == 31;
    (void)es;
    return shape && folded && p.integration_accuracy >= 1e-9 && fill == EMME_FILL_AUTO;
}

void options_default(emme_options_t& o) {
    o = emme_options_t{};
    o.size = (int)sizeof(emme_options_t);
    o.node_cache_gb = 176.0;  // both contour classes together (MI355X: 288 GB of HBM3E)
    o.cache_min_batch = 8;
    o.cache_min_depth = 0;
    o.fill = EMME_FILL_AUTO;
    o.phase_table = 1;
    o.em_shared = 1;
    o.wl_min = 4;
    o.union_sel = 2;
    o.union_ipg_few = 2, o.union_few_chunks = 3;
    o.coop_wide_min = 4096;
    o.defer_one_group = 0;
    o.dense_min_cols = 3;
    o.dense_min_tasks = 2000;
    o.dense_cost_ratio = 4.0;
    o.dense_wide = 0;
    o.skip_lost = 1;
    o.lu_split = 0;
    o.lu_group_min_n = 256;
    o.lu_spin_limit = 16000000;  // about 4 s
    o.lu_unblocked = 0;
    o.deriv_cached = 0;
}

// The EMME_* environment variables: developer overrides, read ONCE per context (at creation), winning over
// the caller's struct.  Library callers use emme_options_t.
void options_env_overrides(emme_options_t& o) {
    auto geti = [](const char* name, int& v) {
        if (const char* e = std::getenv(name)) v = std::atoi(e);
    };
    auto getd = [](const char* name, double& v) {
        if (const char* e = std::getenv(name)) v = std::atof(e);
    };
    getd("EMME_NODE_CACHE_GB", o.node_cache_gb);
    geti("EMME_CACHE_MIN_BATCH", o.cache_min_batch);
    geti("EMME_CACHE_MIN_DEPTH", o.cache_min_depth);
    if (const char* e = std::getenv("EMME_DENSE"))
        if (std::atoi(e) == 0 && o.fill == EMME_FILL_AUTO) o.fill = EMME_FILL_UNION;
    if (const char* e = std::getenv("EMME_UNION"))
        if (std::atoi(e) == 0) o.fill = EMME_FILL_LANES;
    geti("EMME_PHASE_TABLE", o.phase_table);
    geti("EMME_EM_SHARED", o.em_shared);
    geti("EMME_WL_MIN", o.wl_min);
    geti("EMME_UNION_SEL", o.union_sel);
    geti("EMME_UNION_IPG_FEW", o.union_ipg_few);
    geti("EMME_UNION_FEW_CHUNKS", o.union_few_chunks);
    geti("EMME_COOP_WIDE_MIN", o.coop_wide_min);
    if (std::getenv("EMME_DEFER_ONE_GROUP")) o.defer_one_group = 1;
    geti("EMME_DENSE_MIN_COLS", o.dense_min_cols);
    geti("EMME_DENSE_MIN_TASKS", o.dense_min_tasks);
    getd("EMME_DENSE_COST_RATIO", o.dense_cost_ratio);
    geti("EMME_DENSE_WIDE", o.dense_wide);
    geti("EMME_SKIP_LOST", o.skip_lost);
    geti("EMME_LU_SPLIT", o.lu_split);
    if (const char* e = std::getenv("EMME_LU_GROUP")) o.lu_group_min_n = std::atoi(e) <= 0 ? -1 : std::atoi(e);
    geti("EMME_LU_SPIN_LIMIT", o.lu_spin_limit);
    if (std::getenv("EMME_LU_UNBLOCKED")) o.lu_unblocked = 1;
    geti("EMME_DERIV_CACHED", o.deriv_cached);
}

int options_check(const emme_options_t* o) {
    if (o->size != (int)sizeof(emme_options_t)) {
        set_error("emme_options_t: size field does not match this library (use emme_options_default)");
        return EMME_EINVAL;
    }
    if (!(o->node_cache_gb >= 0.0) || o->cache_min_batch < 1 || o->cache_min_depth < 0 || o->fill < EMME_FILL_AUTO ||
        o->fill > EMME_FILL_LANES || o->wl_min < 1 || (o->union_sel != 1 && o->union_sel != 2 && o->union_sel != 4) ||
        o->union_ipg_few < 1 || o->union_few_chunks < 0 || o->coop_wide_min < -1 || o->dense_min_cols < 1 ||
        o->dense_min_cols > 17 || o->dense_min_tasks < 0 || !(o->dense_cost_ratio > 0.0) || o->lu_split < 0 ||
        o->lu_split > 16 || o->lu_spin_limit < 1 || o->deriv_cached < 0 || o->deriv_cached > 1) {
        set_error("emme_options_t: value out of range");
        return EMME_EINVAL;
    }
    return EMME_OK;
}
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
    const size_t bytes = mat_doubles(c) * sizeof(double) * (size_t)nb;
    DeviceBuffer<double>* mats[4] = {&c->d_M, &c->d_Mold, &c->d_Mp, &c->d_work};
    for (int k = 0; k < 4; ++k)
        if (sets & (1 << k)) HIP_TRY(mats[k]->grow(bytes));
    return EMME_OK;
}

// the Newton linear step: blocked kernel while its panel fits in LDS, else the unblocked one
// `h_active`: host copy of `active` (null: all live).  With fewer live matrices than compute
// units each gets up to 8 workgroups (EMME_LU_SPLIT=k pins k; 1 = one workgroup per matrix).
hipError_t trace_solve(emme_ctx* c, int n, int nbatch, double* A, double* B, const int* active,
                       double* tr, int* info, const int* h_active) {
    const bool force_unblocked = c->opt.lu_unblocked != 0;
    const int split_env = c->opt.lu_split;
    // n <= ~560: the whole L21 panel fits in LDS; up to 1024 the chunked build takes over, which
    // needs helper workgroups (>= 2 per matrix, all resident); otherwise the unblocked kernel
    const bool fits = trace_solve_blocked_lds(n) <= 150 * 1024;
    if (!force_unblocked && (fits || n <= 1024)) {
        hipError_t e = c->d_lu_scratch.grow(trace_solve_blocked_scratch(n, nbatch));
        if (e != hipSuccess) return e;
        // dense list of the live matrices (h_active: host copy of `active`, null = all live)
        int n_live = nbatch;
        int* lu_slot = nullptr;
        if (h_active) {
            e = c->d_lu_items.grow(sizeof(int) * nbatch);
            if (e == hipSuccess) e = c->lists.take(nbatch, &lu_slot);
            if (e != hipSuccess) return e;
            n_live = 0;
            for (int b = 0; b < nbatch; ++b)
                if (h_active[b]) lu_slot[n_live++] = b;
            if (n_live == 0) return hipSuccess;
        }
        int nwg = 1;
        if (c->lu_one_wg) {
            nwg = 1;
        } else if (split_env > 0) {
            nwg = std::min(split_env, 16);
        } else if (n >= 128) {
            // every workgroup of a matrix must be resident at once (they wait for each other):
            // never more workgroups than compute units.  Below n = 128 the hand-over costs more
            // than the idle units are worth, and beyond 8 the factoring workgroup is the limit.
            // (n = 256: four are enough, role 0 is the limit then; n = 512: two A-helpers pay)
            nwg = std::max(1, std::min(n >= 768 ? 16 : (n >= 384 ? 8 : 4), c->n_cu / n_live));
        }
        if (!fits && nwg < 2 && !c->lu_one_wg && split_env != 1) nwg = 2;
        c->last_lu_nwg = nwg;
        const int* d_items = nullptr;
        if (nwg > 1 && h_active) {
            e = launch_stage_ints(lu_slot, c->d_lu_items, n_live, nullptr, 0, c->stream);
            if (e == hipSuccess) e = c->lists.read_on(c->stream);
            if (e != hipSuccess) return e;
            d_items = c->d_lu_items;
        }
        e = launch_trace_solve_blocked(n, nbatch, A, B, active, tr, info, nwg, d_items, n_live, c->d_lu_scratch, c->stream,
                                       c->opt.lu_group_min_n, c->opt.lu_spin_limit);
        if (e != hipErrorNotSupported) return e;
        (void)hipGetLastError();  // chunked build not possible here (one workgroup per matrix, or no room)
        c->last_lu_nwg = 1;
    }
    return launch_trace_solve(n, nbatch, A, B, active, tr, info, c->stream);
}

// One Newton linear step on the batch: leaves tr[b] with domega = -1/tr[b].
//   trace-secant (include/solver.h:113-160): work <- M, LU of [work | Mp], tr(M^-1 M')
//   QR-secant    (include/solver.h:210-383): work <- M^T, pivoted QR of work, t_n / R_nn
hipError_t linear_step(emme_ctx* c, int method, int n, int nbatch, const double* M, double* work,
                       double* Mp, const int* active, double* tr, int* info,
                       const int* h_active = nullptr, bool work_ready = false) {
    const size_t mbytes = (size_t)n * n * 2 * sizeof(double) * nbatch;
    if (method == EMME_METHOD_QR_SECANT) {
        hipError_t e = launch_transpose(n, nbatch, M, work, active, c->stream);
        if (e != hipSuccess) return e;
        return launch_qr_secant(n, nbatch, work, Mp, active, tr, info, c->stream);
    }
    if (!work_ready) {  // (the root search copies M -> work together with M -> Mold)
        hipError_t e = hipMemcpyAsync(work, M, mbytes, hipMemcpyDeviceToDevice, c->stream);
        if (e != hipSuccess) return e;
    }
    return trace_solve(c, n, nbatch, work, Mp, active, tr, info, h_active);
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

// The two operands of a linear step where the kernels can read them: A and B themselves if they are device
// pointers, else copies that live as long as this object.  EMME_EINVAL if one is on the host and one on the device;
// otherwise *e is the status of the allocations and copies, which each caller reports in its own words.
struct DeviceOperands {
    double *A = nullptr, *B = nullptr;  // (written only by a caller whose own operands are not const)
    DeviceBuffer<double> st_a, st_b;
    int stage(emme_ctx* c, const double* hA, const double* hB, size_t bytes, hipError_t* e) {
        const bool dev = is_device_ptr(hA);
        if (dev != is_device_ptr(hB)) {
            set_error("A and B must both be host or both be device pointers");
            return EMME_EINVAL;
        }
        A = const_cast<double*>(hA), B = const_cast<double*>(hB), *e = hipSuccess;
        if (dev) return EMME_OK;
        if ((*e = st_a.grow(bytes)) == hipSuccess) *e = st_b.grow(bytes);
        if (*e == hipSuccess) *e = hipMemcpyAsync(st_a, hA, bytes, hipMemcpyHostToDevice, c->stream);
        if (*e == hipSuccess) *e = hipMemcpyAsync(st_b, hB, bytes, hipMemcpyHostToDevice, c->stream);
        A = st_a, B = st_b;
        return EMME_OK;
    }
};

int check_method(const emme_ctx* c, int method) {
    if (method != EMME_METHOD_TRACE_SECANT && method != EMME_METHOD_QR_SECANT) {
        set_error("unknown iteration method");
        return EMME_EINVAL;
    }
    if (method == EMME_METHOD_QR_SECANT && c->dim > 1024) {
        set_error("QR-secant step: matrix dimension above 1024 is not supported");
        return EMME_ECONFIG;
    }
    return EMME_OK;
}


// ---- the two root searches: what they share --------------------------------------------------------------------
// One call's arguments and the host images its loop keeps.
struct RootSearch {
    const double* guesses;
    int n;
    double tol;
    int step_limit;
    bool want_iterates;
    int method = 0;
    std::vector<int> act, zeros;  // host image of d_active (every chain live at the start); n zeros
    int stride() const { return step_limit + 1; }
    // (d_iterates is sized by the last call that asked for iterates: a call that does not ask must not write it)
    double* d_iterates(const emme_ctx* c) const { return want_iterates ? c->d_iterates.get() : nullptr; }
};

// buffers for n chains and the matrix sets of `mat_sets` (ensure_mats); the iterate record, if asked for, all NaN;
// every chain live, no step taken, counters and flags clean
int search_begin(emme_ctx* c, RootSearch& s, int mat_sets) {
    const int n = s.n;
    EMME_TRY(ensure_batch(c, n));
    EMME_TRY(ensure_mats(c, n, mat_sets));
    if (s.want_iterates) {
        const size_t need = (size_t)n * s.stride() * 2;
        HIP_TRY(c->d_iterates.grow(need * sizeof(double)));
        std::vector<double> nanv(need, std::numeric_limits<double>::quiet_NaN());
        HIP_TRY(hipMemcpyAsync(c->d_iterates, nanv.data(), need * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    s.act.assign(n, 1), s.zeros.assign(n, 0);
    HIP_TRY(hipMemcpyAsync(c->d_active, s.act.data(), sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_iters, s.zeros.data(), sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_info, s.zeros.data(), sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    return reset_fill_counters(c, n);
}

// the results to the caller, per-chain failures marked.  *repeat: the search has to be run again (below).
int search_end(emme_ctx* c, const RootSearch& s, double* roots, int* iters, int* info, double* iterates, bool* repeat) {
    const int n = s.n;
    std::vector<unsigned long long> iv(n);
    std::vector<int> stv(n);
    HIP_TRY(hipMemcpyAsync(roots, c->d_omega, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(iters, c->d_iters, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(info, c->d_info, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(iv.data(), c->d_intervals, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(stv.data(), c->d_status, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    if (iterates)
        HIP_TRY(hipMemcpyAsync(iterates, c->d_iterates, sizeof(double) * 2 * (size_t)n * s.stride(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->last_n = n;
    bool timed_out = false;
    for (int b = 0; b < n; ++b) {
        c->acc.gk_intervals += (long long)iv[b];
        // a chain that met a non-finite integral or the quadrature depth cap is reported
        // per item (the reference would carry the NaN to its "eigenvalue": "NaN" record,
        // src/main.cpp:311-316); the other chains of the batch are unaffected
        if (stv[b] != 0 && info[b] == 0) info[b] = EMME_ENUMERIC;
        // whatever the cause, a non-finite omega is never handed back as a root
        if (info[b] == 0 && !(std::isfinite(roots[2 * b]) && std::isfinite(roots[2 * b + 1]))) info[b] = EMME_ENUMERIC;
        timed_out |= info[b] == EMME_EDEVICE;
    }
    // The multi-workgroup LU needs its workgroups resident together; if something else held
    // compute units for seconds (a foreign kernel on a shared device) a hand-over wait timed out
    // and retired those chains with EMME_EDEVICE.  Do the search again with one workgroup per
    // matrix, and keep it that way for this context.
    *repeat = timed_out && !c->lu_one_wg;
    if (*repeat) {
        c->lu_one_wg = true;
        if (std::getenv("EMME_DEBUG")) fprintf(stderr, "[emme] LU hand-over timed out: repeating the search with one workgroup per matrix\n");
    }
    return EMME_OK;
}

// The secant search of emme_solve_roots (EigenSolver's constructor and newtonTraceSecantIteration, include/solver.h:
// 396-415 and 113-160, under the loop of src/main.cpp:19-80), between search_begin and search_end.
int secant_loop(emme_ctx* c, RootSearch& search) {
    const int n = search.n, method = search.method, step_limit = search.step_limit, stride = search.stride();
    const double* guesses = search.guesses;
    const double tol = search.tol;
    double* const d_iterates = search.d_iterates(c);
    std::vector<int>& act = search.act;
    // EigenSolver ctor (include/solver.h:396-415): eigen_value = 0.99 g, d = 0.01 g;
    // M_old = M(eigen_value); eigen_value += d; M = M(eigen_value); M' = (M - M_old)/d
    std::vector<double> w0(2 * (size_t)n), dw(2 * (size_t)n), w1(2 * (size_t)n);
    for (int b = 0; b < 2 * n; ++b) {
        w0[b] = 0.99 * guesses[b];
        dw[b] = 0.01 * guesses[b];
        w1[b] = w0[b] + dw[b];
    }
    HIP_TRY(hipMemcpyAsync(c->d_omega, w0.data(), sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_domega, dw.data(), sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
    c->h_wide.assign(n, 0);
    HIP_TRY(hipMemsetAsync(c->d_overflow, 0, sizeof(unsigned int) * n, c->stream));
    std::vector<double> h_w(2 * (size_t)n);
    std::vector<unsigned long long> iv_prev(n, 0), iv_now(n, 0), cost(n, 0), iv_prev_dbg(n, 0);
    auto refresh_cost = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(iv_now.data(), c->d_intervals, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (int b = 0; b < n; ++b) {
            if (iv_now[b] != iv_prev[b]) cost[b] = iv_now[b] - iv_prev[b];
            iv_prev[b] = iv_now[b];
        }
        return EMME_OK;
    };
    FillRequest first(n, c->d_omega, c->d_Mold);
    first.host_omega = w0.data(), first.newton_loop = true;
    EMME_TRY(fill(c, first));
    EMME_TRY(refresh_cost());  // synchronises; the first fill's interval counts order the second
    HIP_TRY(hipMemcpyAsync(c->d_omega, w1.data(), sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
    // (the fills of a root search write M only: the secant M' = (M - M_old) / d, include/solver.h:157 and :412, is
    // taken by k_secant_copy at the top of the step that uses it, in one coalesced pass)
    FillRequest next(n, c->d_omega, c->d_M);
    next.host_omega = w1.data(), next.cost = cost.data(), next.newton_loop = true;
    EMME_TRY(fill(c, next));
    next.host_omega = h_w.data(), next.d_active = c->d_active, next.host_active = act.data();  // (the steps' fills)

    EMME_TRY(refresh_cost());
    // One stream synchronisation per Newton step: the host needs the new omegas (contour
    // classes, cache growth) before it can launch the fill.  The active flags and interval
    // counts a fill leaves behind travel to pinned memory asynchronously and are read after the
    // NEXT step's synchronisation, so the LU and the update of that step are queued behind the
    // fill without a bubble (their list of live matrices is one step old: a superset).
    bool pending = false;
    int j_pending = 0;
    auto take_pending = [&]() {  // results of the previous step's fill + retire
        for (int b = 0; b < n; ++b) {
            act[b] = c->p_act[b];
            iv_now[b] = c->p_iv[b];
            // (an eighth of its integrals did not fit the 64-entry level lists: 128 entries from now on)
            if (c->p_overflow[b] * 8u >= (unsigned)c->npairs) c->h_wide[b] = 1;
            c->last_deferred = *c->p_deferred, c->pub_valid = true;
            if (iv_now[b] != iv_prev[b]) cost[b] = iv_now[b] - iv_prev[b];
            iv_prev[b] = iv_now[b];
        }
        pending = false;
        if (std::getenv("EMME_DEBUG")) {
            unsigned long long tot = 0, mx = 0;
            int na = 0, nprev = 0;
            for (int b = 0; b < n; ++b) {
                if (iv_now[b] != iv_prev_dbg[b]) {
                    const unsigned long long d = iv_now[b] - iv_prev_dbg[b];
                    tot += d, mx = d > mx ? d : mx, ++nprev;
                }
                iv_prev_dbg[b] = iv_now[b];
                na += act[b] != 0;
            }
            fprintf(stderr, "[emme] LU workgroups per matrix %d\n", c->last_lu_nwg);
            fprintf(stderr, "[emme] iter %2d: assembled %3d, lane-intervals %10llu (max/item %9llu), still active %d\n",
                    j_pending, nprev, tot, mx, na);
        }
    };
    for (int j = 0; j <= step_limit; ++j) {  // src/main.cpp:43
        const bool fused_copy = method == EMME_METHOD_TRACE_SECANT;
        {
            // the secant M' of the step just taken, then this step's matrix becomes the "previous" one (and the
            // LU's work copy): one pass, for the chains still iterating only
            ScopedSpan s(c, K_OTHER);
            HIP_TRY(launch_secant_copy_sym(c->dim, n, c->d_M, c->d_Mold, fused_copy ? c->d_work : nullptr, c->d_Mp,
                                           c->d_domega, c->d_active, c->stream));
        }
        {
            ScopedSpan s(c, K_LIN);
            HIP_TRY(linear_step(c, method, c->dim, n, c->d_M, c->d_work, c->d_Mp, c->d_active, c->d_tr, c->d_info,
                                act.data(), fused_copy));
        }
        {
            ScopedSpan s(c, K_OTHER);
            HIP_TRY(launch_newton_update(n, c->d_tr, c->d_omega, c->d_domega, c->d_active, c->d_iters,
                                         c->d_info, tol, d_iterates, j, stride, c->stream, c->p_w,
                                         c->opt.skip_lost ? c->d_status : nullptr));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        std::copy(c->p_w.get(), c->p_w.get() + 2 * (size_t)n, h_w.begin());
        if (pending) {
            take_pending();
            bool any = false;
            for (int b = 0; b < n; ++b) any |= act[b] != 0;
            if (!any) break;  // (this step's LU and update found nothing active: no-ops)
        }
        EMME_TRY(fill(c, next));
        {
            ScopedSpan s(c, K_OTHER);
            HIP_TRY(launch_retire(n, c->d_active, c->stream, c->p_act, c->d_intervals, c->p_iv,
                                  c->d_worklist_count, c->p_deferred, c->d_overflow, c->p_overflow));
        }
        pending = true, j_pending = j;
    }
    return EMME_OK;
}

// The Newton search of emme_solve_roots_newton, between search_begin and search_end.
int newton_loop(emme_ctx* c, RootSearch& search) {
    const int n = search.n, method = search.method, step_limit = search.step_limit, stride = search.stride();
    const double tol = search.tol;
    double* const d_iterates = search.d_iterates(c);
    std::vector<int>& act = search.act;
    // omega_0 = g: one fill of M and the exact M' there, no secant bootstrap
    HIP_TRY(hipMemcpyAsync(c->d_omega, search.guesses, sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
    FillRequest both(n, c->d_omega, c->d_M);
    both.d_Md = c->d_Mp, both.d_active = c->d_active, both.host_active = act.data();
    // Option deriv_cached: the fills may go through the node cache, which needs what the secant loop gives its fills --
    // the live omegas on the host (contour classes), every omega's interval count of its previous fill (cost order)
    // and the root-search flag (skip_lost).  They travel as there: k_newton_update writes the omegas, k_retire the
    // counters and the deferred count into pinned memory, read after the step's one synchronisation.
    const bool cached = c->opt.deriv_cached != 0;
    std::vector<double> h_w;
    std::vector<unsigned long long> iv_prev, cost;
    bool pending = false;
    if (cached) {
        h_w.assign(search.guesses, search.guesses + 2 * (size_t)n);
        iv_prev.assign(n, 0), cost.assign(n, 0);
        both.host_omega = h_w.data(), both.newton_loop = true;
        c->pub_valid = false;
    }
    auto publish = [&]() -> hipError_t {
        if (!cached) return launch_retire(n, c->d_active, c->stream);
        pending = true;
        return launch_retire(n, c->d_active, c->stream, nullptr, c->d_intervals, c->p_iv, c->d_worklist_count, c->p_deferred);
    };
    EMME_TRY(fill(c, both));
    if (cached) {
        // (the first fill's counts order the second; no chain has been retired yet: every flag is 1)
        ScopedSpan s(c, K_OTHER);
        HIP_TRY(publish());
        both.cost = cost.data();
    }
    for (int j = 0; j <= step_limit; ++j) {
        {
            // the step of the context's iteration_method on (M, M'): trace form on a work copy of M (the LU destroys
            // both operands; M' is filled again before it is needed), QR form on the transpose
            ScopedSpan s(c, K_LIN);
            const bool trace = method == EMME_METHOD_TRACE_SECANT;
            if (trace) HIP_TRY(launch_copy_active(c->dim, n, c->d_M, c->d_work, nullptr, c->d_active, c->stream));
            HIP_TRY(linear_step(c, method, c->dim, n, c->d_M, c->d_work, c->d_Mp, c->d_active, c->d_tr, c->d_info,
                                act.data(), trace));
        }
        {
            ScopedSpan s(c, K_OTHER);
            HIP_TRY(launch_newton_update(n, c->d_tr, c->d_omega, c->d_domega, c->d_active, c->d_iters, c->d_info, tol,
                                         d_iterates, j, stride, c->stream, cached ? c->p_w.get() : nullptr,
                                         c->opt.skip_lost ? c->d_status : nullptr));
        }
        // the live chains (2 = converged at this step: M and M' are filled at the new omega once more)
        HIP_TRY(hipMemcpyAsync(c->p_act, c->d_active, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        bool any = false;
        for (int b = 0; b < n; ++b) {
            act[b] = c->p_act[b];
            any |= act[b] != 0;
        }
        if (!any) break;
        if (cached) {
            std::copy(c->p_w.get(), c->p_w.get() + 2 * (size_t)n, h_w.begin());
            if (pending) {  // what the previous fill left behind
                for (int b = 0; b < n; ++b) {
                    const unsigned long long now = c->p_iv[b];
                    if (now != iv_prev[b]) cost[b] = now - iv_prev[b];
                    iv_prev[b] = now;
                }
                c->last_deferred = *c->p_deferred, c->pub_valid = true;
                pending = false;
            }
        }
        EMME_TRY(fill(c, both));
        {
            ScopedSpan s(c, K_OTHER);
            HIP_TRY(publish());
        }
    }
    return EMME_OK;
}

int run_search(emme_ctx* c, const double* guesses, int n, double tol, int step_limit, double* roots, int* iters, int* info,
               double* iterates, int mat_sets, int (*loop)(emme_ctx*, RootSearch&)) {
    if (!c || !guesses || !roots || !iters || !info || n < 1 || step_limit < 0) return EMME_EINVAL;
    RootSearch s{guesses, n, tol, step_limit, iterates != nullptr};
    s.method = c->p.iteration_method;  // src/main.cpp:45-49
    EMME_TRY(check_method(c, s.method));
    HIP_TRY(hipSetDevice(c->device));
    for (;;) {
        bool repeat = false;
        EMME_TRY(search_begin(c, s, mat_sets));
        EMME_TRY(loop(c, s));
        EMME_TRY(search_end(c, s, roots, iters, info, iterates, &repeat));
        if (!repeat) return EMME_OK;
    }
}

}  // namespace


// The kernels' scalars and tables (eta | g | b) of a parameter set: what every context launches with, and what the
// probe entry points (emme_integrand_batch) evaluate single nodes with.
static void dev_params_from(const emme_params_t* p, DevParams& P, std::vector<double>& tab) {
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
    {
        EMME_TRY(options_check(&o));
    }
    if (p->integration_start_points != 15 && p->integration_start_points != 31) {
        // include/functions.h:329
        set_error("integration_start_points should be 15 or 31");
        return EMME_ECONFIG;
    }
    if (p->npoints < 2 || p->npoints > 65535) {
        set_error("npoints must be in [2, 65535]");
        return EMME_EINVAL;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        set_error("no HIP device available (the MI355X path has no CPU fallback)");
        return EMME_EDEVICE;
    }
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
    c->tiled = wants_tiled(*p, es, c->folded, o.fill);

    DevParams& P = c->P;
    std::vector<double> tab;
    dev_params_from(p, P, tab);

    // pair list ordered by diagonal offset (see assemble.hip header)
    std::vector<ushort2> pairs;
    pairs.reserve((size_t)N * (N - 1) / 2);
    for (int off = 1; off < N; ++off)
        for (int i = 0; i + off < N; ++i) pairs.push_back(make_ushort2((unsigned short)i, (unsigned short)(i + off)));
    c->npairs = (int)pairs.size();

    auto fail = [&](int code) {
        emme_ctx_destroy(c);
        return code;
    };
    if (c->d_tab.grow(tab.size() * sizeof(double)) != hipSuccess ||
        c->d_pairs.grow(pairs.size() * sizeof(ushort2)) != hipSuccess) {
        set_error("hipMalloc failed for tables");
        return fail(EMME_ENOMEM);
    }
    if (hipMemcpy(c->d_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->d_pairs, pairs.data(), pairs.size() * sizeof(ushort2), hipMemcpyHostToDevice) != hipSuccess) {
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
        c->tiled = wants_tiled(c->p, es, c->folded, opt->fill);
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

int emme_ctx_set_stream(emme_ctx_t* c, void* s) {
    if (!c) return EMME_EINVAL;
    c->stream = (hipStream_t)s;
    return EMME_OK;
}

int emme_ctx_dim(const emme_ctx_t* c) { return c ? c->dim : EMME_EINVAL; }

int emme_ctx_fill_mode(const emme_ctx_t* c) { return c ? c->last_fill_mode : EMME_EINVAL; }

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
        if (c->tiled) {
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
    EMME_TRY(ensure_batch(c, nbatch));
    const bool dev_out = is_device_ptr(M);
    double* dM = M;
    if (!dev_out) {
        EMME_TRY(ensure_mats(c, nbatch, 1));
        dM = c->d_M;
    }
    EMME_TRY(fill_at(c, omega, nbatch, dM, nullptr, hipMemcpyHostToDevice));
    if (!dev_out)
        HIP_TRY(hipMemcpyAsync(M, dM, mat_doubles(c) * sizeof(double) * nbatch, hipMemcpyDeviceToHost, c->stream));
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

int emme_trace_solve_batch(emme_ctx_t* c, int n, int nbatch, double* A, double* B, double* tr,
                           int* info) {
    if (!c || !A || !B || !tr || !info || n < 1 || nbatch < 1) return EMME_EINVAL;
    if ((size_t)2 * n * sizeof(double2) > 64 * 1024) {
        set_error("n too large for the LDS-staged pivot row");
        return EMME_EINVAL;
    }
    HIP_TRY(hipSetDevice(c->device));
    EMME_TRY(ensure_batch(c, nbatch));
    const size_t bytes = (size_t)n * n * 2 * sizeof(double) * nbatch;
    DeviceOperands ops;
    hipError_t staged = hipSuccess;
    EMME_TRY(ops.stage(c, A, B, bytes, &staged));
    HIP_TRY(staged);
    double *dA = ops.A, *dB = ops.B;
    {
        ScopedSpan s(c, K_LIN);
        HIP_TRY(trace_solve(c, n, nbatch, dA, dB, nullptr, c->d_tr, c->d_info, nullptr));
    }
    HIP_TRY(hipMemcpyAsync(tr, c->d_tr, sizeof(double) * 2 * nbatch, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(info, c->d_info, sizeof(int) * nbatch, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EMME_OK;
}

int emme_qr_secant_batch(emme_ctx_t* c, int n, int nbatch, const double* A, const double* B,
                         double* q, int* info) {
    if (!c || !A || !B || !q || !info || n < 1 || nbatch < 1) return EMME_EINVAL;
    if (n > 1024) {
        set_error("QR-secant step: matrix dimension above 1024 is not supported");
        return EMME_ECONFIG;
    }
    HIP_TRY(hipSetDevice(c->device));
    EMME_TRY(ensure_batch(c, nbatch));
    const size_t bytes = (size_t)n * n * 2 * sizeof(double) * nbatch;
    DeviceOperands ops;
    DeviceBuffer<double> dW;  // transposed work copy
    hipError_t e = hipSuccess;
    EMME_TRY(ops.stage(c, A, B, bytes, &e));
    if (e == hipErrorOutOfMemory || dW.grow(bytes) != hipSuccess) {
        set_error("hipMalloc failed");
        return EMME_ENOMEM;
    }
    const double *dA = ops.A, *dB = ops.B;
    {
        ScopedSpan s(c, K_LIN);
        if (e == hipSuccess) e = launch_transpose(n, nbatch, dA, dW, nullptr, c->stream);
        if (e == hipSuccess) e = launch_qr_secant(n, nbatch, dW, dB, nullptr, c->d_tr, c->d_info, c->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(q, c->d_tr, sizeof(double) * 2 * nbatch, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(info, c->d_info, sizeof(int) * nbatch, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        set_error(hipGetErrorString(e));
        return EMME_EDEVICE;
    }
    return EMME_OK;
}

int emme_newton_step_batch(emme_ctx_t* c, double* omega, double* domega, int nbatch, double* M,
                           double* Mp, int method, int* info) {
    if (!c || !omega || !domega || !M || !Mp || !info || nbatch < 1) return EMME_EINVAL;
    EMME_TRY(check_method(c, method));
    HIP_TRY(hipSetDevice(c->device));
    EMME_TRY(ensure_batch(c, nbatch));
    const bool dev = is_device_ptr(M);
    if (dev != is_device_ptr(Mp)) {
        set_error("M and Mp must both be host or both be device pointers");
        return EMME_EINVAL;
    }
    const size_t mbytes = mat_doubles(c) * sizeof(double) * nbatch;
    EMME_TRY(ensure_mats(c, nbatch, dev ? (2 | 8) : (1 | 2 | 4 | 8)));
    double *dM = M, *dMp = Mp;
    if (!dev) {
        dM = c->d_M, dMp = c->d_Mp;
        HIP_TRY(hipMemcpyAsync(dM, M, mbytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(dMp, Mp, mbytes, hipMemcpyHostToDevice, c->stream));
    }
    const hipMemcpyKind in_kind = is_device_ptr(omega) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind out_kind = is_device_ptr(omega) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    EMME_TRY(upload_omega(c, omega, nbatch, in_kind));
    EMME_TRY(reset_fill_counters(c, nbatch));
    {
        // eigen_matrix_old = eigen_matrix (include/solver.h:114); the factorisation then
        // consumes a scratch copy so M_old survives for the secant update
        ScopedSpan s(c, K_OTHER);
        HIP_TRY(hipMemcpyAsync(c->d_Mold, dM, mbytes, hipMemcpyDeviceToDevice, c->stream));
    }
    {
        ScopedSpan s(c, K_LIN);
        HIP_TRY(linear_step(c, method, c->dim, nbatch, dM, c->d_work, dMp, nullptr, c->d_tr, c->d_info));
    }
    {
        ScopedSpan s(c, K_OTHER);
        HIP_TRY(launch_newton_update(nbatch, c->d_tr, c->d_omega, c->d_domega, nullptr, nullptr,
                                     c->d_info, 0.0, nullptr, 0, 0, c->stream));
    }
    std::vector<double> h_w(2 * (size_t)nbatch);
    HIP_TRY(hipMemcpyAsync(h_w.data(), c->d_omega, sizeof(double) * 2 * nbatch, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    FillRequest secant_fill(nbatch, c->d_omega, dM);
    secant_fill.host_omega = h_w.data();
    secant_fill.d_Mold = c->d_Mold, secant_fill.d_Mp = dMp, secant_fill.d_domega = c->d_domega;
    EMME_TRY(fill(c, secant_fill));
    if (!dev) {
        HIP_TRY(hipMemcpyAsync(M, dM, mbytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(Mp, dMp, mbytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(omega, c->d_omega, sizeof(double) * 2 * nbatch, out_kind, c->stream));
    HIP_TRY(hipMemcpyAsync(domega, c->d_domega, sizeof(double) * 2 * nbatch, out_kind, c->stream));
    std::vector<unsigned long long> iv(nbatch);
    HIP_TRY(hipMemcpyAsync(iv.data(), c->d_intervals, sizeof(unsigned long long) * nbatch, hipMemcpyDeviceToHost, c->stream));
    if (is_device_ptr(info))
        HIP_TRY(hipMemcpyAsync(info, c->d_info, sizeof(int) * nbatch, hipMemcpyDeviceToDevice, c->stream));
    else
        HIP_TRY(hipMemcpyAsync(info, c->d_info, sizeof(int) * nbatch, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int b = 0; b < nbatch; ++b) c->acc.gk_intervals += (long long)iv[b];
    return EMME_OK;
}

int emme_solve_roots(emme_ctx_t* c, const double* guesses, int n, double tol, int step_limit,
                     double* roots, int* iters, int* info, double* iterates) {
    return run_search(c, guesses, n, tol, step_limit, roots, iters, info, iterates, 1 | 2 | 4 | 8, secant_loop);
}

int emme_assemble_derivative_batch(emme_ctx_t* c, const double* omega, int nbatch, double* M, double* Mp,
                                   long long* intervals) {
    if (!c || !omega || !M || !Mp || nbatch < 1) return EMME_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    const bool dev_out = is_device_ptr(M);
    if (dev_out != is_device_ptr(Mp)) {
        set_error("M and Mp must both be host or both be device pointers");
        return EMME_EINVAL;
    }
    EMME_TRY(ensure_batch(c, nbatch));
    double *dM = M, *dMp = Mp;
    if (!dev_out) {
        EMME_TRY(ensure_mats(c, nbatch, 1 | 4));
        dM = c->d_M, dMp = c->d_Mp;
    }
    EMME_TRY(fill_at(c, omega, nbatch, dM, dMp, hipMemcpyDefault));
    if (!dev_out) {
        HIP_TRY(hipMemcpyAsync(M, dM, mat_doubles(c) * sizeof(double) * nbatch, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(Mp, dMp, mat_doubles(c) * sizeof(double) * nbatch, hipMemcpyDeviceToHost, c->stream));
    }
    return collect_fill_status(c, nbatch, intervals);
}

int emme_solve_roots_newton(emme_ctx_t* c, const double* guesses, int n, double tol, int step_limit, double* roots,
                            int* iters, int* info, double* iterates) {
    return run_search(c, guesses, n, tol, step_limit, roots, iters, info, iterates, 1 | 4 | 8, newton_loop);  // (no M_old)
}

static int probe_device_check() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        set_error("no HIP device available (the MI355X path has no CPU fallback)");
        return EMME_EDEVICE;
    }
    return EMME_OK;
}

int emme_bessel_batch(const double* z, int n, double* out) {
    if (!z || !out || n < 1) return EMME_EINVAL;
    EMME_TRY(probe_device_check());
    DeviceBuffer<double> dz, dout;
    HIP_TRY(dz.grow(sizeof(double) * 2 * n));
    HIP_TRY(dout.grow(sizeof(double) * 8 * n));
    HIP_TRY(hipMemcpy(dz, z, sizeof(double) * 2 * n, hipMemcpyHostToDevice));
    HIP_TRY(launch_bessel_probe(dz, n, dout, nullptr));
    HIP_TRY(hipMemcpy(out, dout, sizeof(double) * 8 * n, hipMemcpyDeviceToHost));
    return EMME_OK;
}

int emme_elementary_batch(int fn, const double* x, int n, double* out) {
    if (!x || !out || n < 1 || fn < 0 || fn > EMME_FN_CRCP) return EMME_EINVAL;
    EMME_TRY(probe_device_check());
    const size_t n_in = fn == EMME_FN_CRCP ? 2 : 1;
    const size_t n_out = fn >= EMME_FN_SINCOS ? 2 : 1;
    DeviceBuffer<double> dx, dout;
    HIP_TRY(dx.grow(sizeof(double) * n_in * n));
    HIP_TRY(dout.grow(sizeof(double) * n_out * n));
    HIP_TRY(hipMemcpy(dx, x, sizeof(double) * n_in * n, hipMemcpyHostToDevice));
    HIP_TRY(launch_elementary_probe(fn, dx, n, dout, nullptr));
    HIP_TRY(hipMemcpy(out, dout, sizeof(double) * n_out * n, hipMemcpyDeviceToHost));
    return EMME_OK;
}

int emme_integrand_batch(const emme_params_t* p, int form, int n, const int* i, const int* j, const int* m,
                         const double* x, const double* omega, double* out) {
    if (!p || !i || !j || !m || !x || !omega || !out || n < 1 || form < 0 || form > EMME_FORM_W) return EMME_EINVAL;
    if (p->npoints < 2 || p->npoints > 65535) {
        set_error("npoints must be in [2, 65535]");
        return EMME_EINVAL;
    }
    // the scalars DevParams divides by: a zero or non-finite one would put inf / NaN into every item
    for (const double v : {p->arc_coeff, p->vt, p->tau, p->q, p->R, p->omega_s_i}) {
        if (!std::isfinite(v) || v == 0.0) {
            set_error("emme_integrand_batch: arc_coeff, vt, tau, q, R and omega_s_i must be finite and non-zero");
            return EMME_EINVAL;
        }
    }
    const int nm = std::fpclassify(p->beta_e) == FP_ZERO ? 1 : 3;
    for (int k = 0; k < n; ++k) {
        const bool pair_ok = i[k] >= 0 && i[k] < j[k] && j[k] < p->npoints;
        const bool x_ok = x[k] > 0.0 && x[k] < M_PI / 2;  // (false for NaN)
        if (!pair_ok || m[k] < 0 || m[k] >= nm || !x_ok) {
            set_error("emme_integrand_batch: item " + std::to_string(k) +
                      " needs 0 <= i < j < npoints, a moment of the context (0, or 0..2 with beta_e != 0) and x in (0, pi/2)");
            return EMME_EINVAL;
        }
    }
    EMME_TRY(probe_device_check());
    IntegrandProbe A;
    std::vector<double> tab;
    dev_params_from(p, A.P, tab);
    A.form = form, A.n = n;
    const size_t per = (size_t)integrand_probe_doubles(form);
    DeviceBuffer<double> dtab, dx, dw, dout;
    DeviceBuffer<int> dijm;
    HIP_TRY(dtab.grow(sizeof(double) * tab.size()));
    HIP_TRY(dx.grow(sizeof(double) * n));
    HIP_TRY(dw.grow(sizeof(double) * 2 * n));
    HIP_TRY(dout.grow(sizeof(double) * per * n));
    HIP_TRY(dijm.grow(sizeof(int) * 3 * (size_t)n));
    HIP_TRY(hipMemcpy(dtab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dw, omega, sizeof(double) * 2 * n, hipMemcpyHostToDevice));
    int* d_ijm = dijm;
    HIP_TRY(hipMemcpy(d_ijm, i, sizeof(int) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_ijm + n, j, sizeof(int) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_ijm + 2 * (size_t)n, m, sizeof(int) * n, hipMemcpyHostToDevice));
    A.tab = dtab, A.i = d_ijm, A.j = d_ijm + n, A.m = d_ijm + 2 * (size_t)n;
    A.x = dx, A.omega = dw, A.out = dout;
    HIP_TRY(launch_integrand_probe(A, nullptr));
    HIP_TRY(hipMemcpy(out, dout, sizeof(double) * per * n, hipMemcpyDeviceToHost));
    return EMME_OK;
}

}  // extern "C"

namespace emme {

// Partial-pivot LU of nbatch n x n matrices in place (P M = L U, rows never moved; n <= 2048), by the branch the
// order allows: k_lu_inplace where the whole L21 panel fits one workgroup's LDS; above that, up to n = 1024, the chunked
// multi-workgroup kernel of the Newton step (two workgroups per matrix, which must be resident together: slices of at
// most half the compute units; its right-hand side is a dummy); beyond, k_lu_unblocked_inplace.  After each slice's
// factorisation `after(b0, nb, maps, map_nb, lu_info)` queues what reads it: matrices b0 .. b0 + nb - 1, their row-order
// snapshots (logical row x of slice item b is physical row maps[(b ceil(n / map_nb) + x / map_nb) n + x]) and their
// info (0 or the column at which the factorisation stopped), both valid until the next slice is factored.  Used by
// emme_null_vectors_batch and the contour solver (contour.hip); the launches are stream-ordered on c->stream.
int lu_factor_batch(emme_ctx* c, int n, int nbatch, double* work, LuScratch& s, const char* who,
                    const std::function<hipError_t(int, int, const int*, int, const int*)>& after) {
    const size_t mbytes = (size_t)n * n * 2 * sizeof(double);
    const bool one_wg = trace_solve_blocked_lds(n) <= 150 * 1024;  // the whole L21 panel in one workgroup's LDS
    if (one_wg || n <= 1024) {
        const int slice_max = one_wg ? nbatch : std::max(1, c->n_cu / 2);
        HIP_TRY(c->d_lu_scratch.grow(trace_solve_blocked_scratch(n, std::min(nbatch, slice_max))));
        if (!one_wg) HIP_TRY(s.b.grow(mbytes * std::min(nbatch, slice_max)));
        for (int b0 = 0; b0 < nbatch; b0 += slice_max) {
            const int nb = std::min(slice_max, nbatch - b0);
            double* a0 = work + (size_t)b0 * n * n * 2;
            ScopedSpan sp(c, K_NULL);
            if (one_wg) {
                HIP_TRY(launch_lu_inplace(n, nb, a0, nullptr, nb, c->d_info, c->d_lu_scratch, c->stream));
            } else {
                HIP_TRY(hipMemsetAsync(s.b, 0, mbytes * nb, c->stream));
                const hipError_t e = launch_trace_solve_blocked(n, nb, a0, s.b, nullptr, c->d_tr, c->d_info, 2, nullptr, nb,
                                                                c->d_lu_scratch, c->stream, -1, c->opt.lu_spin_limit);
                if (e != hipSuccess) {
                    (void)hipGetLastError();
                    set_error(std::string(who) + ": the chunked factorisation could not be launched (its two workgroups per matrix must be resident together)");
                    return EMME_EDEVICE;
                }
            }
            HIP_TRY(after(b0, nb, trace_solve_rowmaps(c->d_lu_scratch, n, nb), trace_solve_nb(), c->d_info));
        }
    } else {
        HIP_TRY(s.maps.grow(sizeof(int) * (size_t)n * nbatch));
        ScopedSpan sp(c, K_NULL);
        HIP_TRY(launch_lu_unblocked_inplace(n, nbatch, work, s.maps, c->d_info, c->stream));
        HIP_TRY(after(0, nbatch, s.maps, n, c->d_info));
    }
    return EMME_OK;
}

int ctx_ensure_batch(emme_ctx* c, int nb) { return ensure_batch(c, nb); }
bool ptr_on_device(const void* p) { return is_device_ptr(p); }

}  // namespace emme

extern "C" {

// nullSpace (reference include/solver.h:58-112), batched on the device: see nullspace.hip
int emme_null_vectors_batch(emme_ctx_t* c, int n, int nbatch, const double* M, double* vecs, int* info) {
    if (!c || !vecs || !info || n < 1 || nbatch < 1) return EMME_EINVAL;
    if (!M && (n != c->dim || nbatch > c->last_n || !c->d_M)) {
        set_error("emme_null_vectors_batch: M = NULL needs a preceding emme_solve_roots call (n = emme_ctx_dim, nbatch <= its n)");
        return EMME_EINVAL;
    }
    if (n > 2048) {
        set_error("emme_null_vectors_batch: order above 2048 is not supported");
        return EMME_ECONFIG;
    }
    HIP_TRY(hipSetDevice(c->device));
    EMME_TRY(ensure_batch(c, nbatch));
    const size_t mbytes = (size_t)n * n * 2 * sizeof(double);
    // device scratch of this call
    DeviceBuffer<double> t_a, t_v;
    DeviceBuffer<int> t_info;
    // work copy the factorisation overwrites: the context's LU work set after a root search, else a buffer of its own
    double* work = nullptr;
    if (!M && c->d_work.bytes() >= mbytes * nbatch) {
        work = c->d_work;
        HIP_TRY(hipMemcpyAsync(work, c->d_M, mbytes * nbatch, hipMemcpyDeviceToDevice, c->stream));
    } else {
        HIP_TRY(t_a.grow(mbytes * nbatch));
        work = t_a;
        const double* src = M ? M : c->d_M;
        HIP_TRY(hipMemcpyAsync(work, src, mbytes * nbatch, is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(t_v.grow(sizeof(double) * 2 * (size_t)n * nbatch));
    HIP_TRY(t_info.grow(sizeof(int) * nbatch));
    // two sweeps at a converged root; the rest is for matrices that are not singular (chains that never converged):
    // a launch lasts as long as its slowest matrix, 0.18 ms per sweep at n = 256.  Measured on the 128 matrices of the
    // headline search (worst 1 - overlap against the SVD where the SVD itself determines the vector): 60 sweeps
    // 11.6 ms / 2.7e-14, 30 sweeps 6.7 ms / 8.9e-14, 20 sweeps 4.9 ms / 2.2e-9
    const int max_sweeps = 30;
    LuScratch scratch;
    const int rc = lu_factor_batch(c, n, nbatch, work, scratch, "emme_null_vectors_batch",
                              [&](int b0, int nb, const int* maps, int map_nb, const int* lu_info) -> hipError_t {
                                  return launch_null_iterate(n, work + (size_t)b0 * n * n * 2, maps, map_nb, nullptr,
                                                             nb, lu_info, t_v + (size_t)b0 * n * 2, t_info + b0,
                                                             max_sweeps, c->stream);
                              });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(vecs, t_v, sizeof(double) * 2 * (size_t)n * nbatch, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(info, t_info, sizeof(int) * nbatch, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EMME_OK;
}

int emme_ctx_get_matrix(emme_ctx_t* c, int b, double* M_host) {
    if (!c || !M_host || b < 0 || b >= c->last_n || !c->d_M) return EMME_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpy(M_host, c->d_M + mat_doubles(c) * (size_t)b, mat_doubles(c) * sizeof(double), hipMemcpyDeviceToHost));
    return EMME_OK;
}

}  // extern "C"
