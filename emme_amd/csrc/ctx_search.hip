// ctx_search.hip -- the two root searches: what stands where the reference has EigenSolver's constructor and
// newtonTraceSecantIteration (include/solver.h:396-415, 113-160) under the solve_once_eigen loop (src/main.cpp:19-80),
// the Newton search on the exact derivative and, in the same loop, Newton on the eigenpair.
// Entry points: emme_solve_roots, emme_solve_roots_newton, emme_solve_roots_sets, emme_solve_eigenpairs,
// emme_solve_eigenpairs_secant, emme_newton_step_batch.
#include "ctx.hpp"

using namespace emme;

namespace {

// ---- the two root searches: what they share --------------------------------------------------------------------
// One call's arguments and the host images its loop keeps.
struct RootSearch {
    const double* guesses;
    int n;
    double tol;
    int step_limit;
    bool want_iterates;
    int method = 0;
    const int* set = nullptr;  // host, n ints: chain b searches on the bound parameter set set[b] (null: the context's own)
    bool eigpair = false;      // the loop's linear step is the eigenpair step (secant_loop: its secant
                               // reading): `method` is not consulted
    const double* v0 = nullptr;  // eigenpair search: host, n * dim complex unit start vectors (null: from M(omega_0)^-1 s)
    LuScratch lu;              // ... and what its factorisations keep between launches
    std::vector<int> act, zeros;  // host image of d_active (every chain live at the start); n zeros
    int stride() const { return step_limit + 1; }
    // the parameter sets of the chains (uploaded by search_begin), for the loops' FillRequests
    void to(const emme_ctx* c, FillRequest& r) const {
        if (set) r.d_set = c->d_set, r.host_set = set;
    }
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
    c->last_folded_steps = 0;
    if (s.set) EMME_TRY(upload_set_indices(c, s.set, n));
    if (s.eigpair) {
        c->last_folded_eigpair_steps = 0;
        const size_t vbytes = sizeof(double) * 2 * (size_t)n * c->dim;
        HIP_TRY(c->d_vecs.grow(vbytes));
        HIP_TRY(c->d_resid.grow(sizeof(double) * n));
        HIP_TRY(c->p_live.grow(sizeof(int) * n));
        if (s.v0) HIP_TRY(hipMemcpyAsync(c->d_vecs, s.v0, vbytes, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(c->d_active, s.act.data(), sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_iters, s.zeros.data(), sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_info, s.zeros.data(), sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    return reset_fill_counters(c, n);
}

// the results to the caller, per-chain failures marked.  *repeat: the search has to be run again (below).
int search_end(emme_ctx* c, const RootSearch& s, double* roots, int* iters, int* info, double* iterates, bool* repeat) {
    const int n = s.n;
    std::vector<unsigned long long> iv;
    std::vector<int> stv;
    HIP_TRY(hipMemcpyAsync(roots, c->d_omega, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(iters, c->d_iters, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(info, c->d_info, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    EMME_TRY(queue_fill_counters(c, n, iv, &stv));
    if (iterates)
        HIP_TRY(hipMemcpyAsync(iterates, c->d_iterates, sizeof(double) * 2 * (size_t)n * s.stride(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->last_n = n;
    (void)fold_fill_counters(c, iv, nullptr);  // (flagged chains are marked one by one, below)
    bool timed_out = false;
    for (int b = 0; b < n; ++b) {
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

// One eigenpair step (eigpair.hip) for the chains still iterating, on the work copies the loop has just made:
// factor the live ones only (lu_factor_batch with their list; its launches count as K_NULL spans), then
// k_eigpair_step on the same list leaves tau in d_tr for launch_newton_update, the new vectors in d_vecs and the
// residual before the step in d_resid.  A factorisation that stops leaves the column in d_info: the chain retires.
// `live`: the chains' flags as the last launch_newton_update left them (1: iterating; 2: converged at that step and
// retired behind its fill).  secant: k_eigpair_secant_step on (d_M, d_Mold, d_domega) instead of (d_M, d_Mp).
int eigpair_step(emme_ctx* c, RootSearch& search, const int* live, bool first, bool secant) {
    const int n = search.n, dim = c->dim;
    int n_live = 0;
    HIP_TRY(stage_live_list(c, c->d_lu_items, live, n, 1, [](int flag) { return flag == 1; }, &n_live));
    if (n_live == 0) return EMME_OK;
    return lu_factor_batch(
        c, dim, n, c->d_work, search.lu, secant ? "emme_solve_eigenpairs_secant" : "emme_solve_eigenpairs",
        [&](int i0, int ni, const int* maps, int map_nb, const int* lu_info) -> hipError_t {
            if (secant)
                return launch_eigpair_secant_step(dim, c->d_M, c->d_Mold, c->d_domega, c->d_work, maps, map_nb,
                                                  c->d_lu_items + i0, ni, c->d_active, lu_info, c->d_vecs, c->d_tr, c->d_resid,
                                                  c->d_info, first, c->stream);
            return launch_eigpair_step(dim, c->d_M, c->d_Mp, c->d_work, maps, map_nb, c->d_lu_items + i0, ni, c->d_active,
                                       lu_info, c->d_vecs, c->d_tr, c->d_resid, c->d_info, first, c->stream);
        },
        c->d_lu_items, n_live);
}

// The secant search of emme_solve_roots (EigenSolver's constructor and newtonTraceSecantIteration, include/solver.h:
// 396-415 and 113-160, under the loop of src/main.cpp:19-80), between search_begin and search_end; with search.eigpair,
// that of emme_solve_eigenpairs_secant: the same bootstrap, fills and feedback around the secant
// eigenpair step, which reads M and M_old themselves -- no M' is formed, and M_old follows M by a copy of the live
// matrices once the step has read both.
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
    StepFeedback& fb = c->fb;
    fb.begin(n);
    HIP_TRY(hipMemsetAsync(c->d_overflow, 0, sizeof(unsigned int) * n, c->stream));
    std::vector<double> h_w(2 * (size_t)n);
    std::vector<unsigned long long> iv_now(n, 0), iv_prev_dbg(n, 0);
    auto refresh_cost = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(iv_now.data(), c->d_intervals, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        fb.take(iv_now.data());
        return EMME_OK;
    };
    FillRequest first(n, c->d_omega, c->d_Mold);
    first.host_omega = w0.data(), first.newton_loop = true;
    search.to(c, first);
    EMME_TRY(fill(c, first));
    // The folded step needs both matrices of the secant written by mirrored fills for every live
    // chain: old_mirrored / new_mirrored say so of what d_Mold and d_M hold (a minority class that went through the
    // omega-lane kernel, or a cache that did not fit, makes a fill unmirrored)
    bool old_mirrored = c->last_fill_mirrored, new_mirrored = false;
    EMME_TRY(refresh_cost());  // synchronises; the first fill's interval counts order the second
    HIP_TRY(hipMemcpyAsync(c->d_omega, w1.data(), sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
    // (the fills of a root search write M only: the secant M' = (M - M_old) / d, include/solver.h:157 and :412, is
    // taken by k_secant_copy at the top of the step that uses it, in one coalesced pass)
    FillRequest next(n, c->d_omega, c->d_M);
    next.host_omega = w1.data(), next.cost = fb.cost.data(), next.newton_loop = true;
    search.to(c, next);
    EMME_TRY(fill(c, next));
    new_mirrored = c->last_fill_mirrored;
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
        std::copy(c->p_act.get(), c->p_act.get() + n, act.begin());
        // (an item an eighth of whose integrals did not fit the 64-entry level lists: 128 entries from now on)
        // (the dense fill is the only one that counts overflows: of the integrals it ran, half of them when mirrored)
        fb.take(c->p_iv, c->p_overflow, cache_npairs(c), c->p_deferred);
        pending = false;
        if (std::getenv("EMME_DEBUG")) {
            unsigned long long tot = 0, mx = 0;
            int na = 0, nprev = 0;
            for (int b = 0; b < n; ++b) {
                if (fb.iv_prev[b] != iv_prev_dbg[b]) {  // (iv_prev: the counters just taken)
                    const unsigned long long d = fb.iv_prev[b] - iv_prev_dbg[b];
                    tot += d, mx = d > mx ? d : mx, ++nprev;
                }
                iv_prev_dbg[b] = fb.iv_prev[b];
                na += act[b] != 0;
            }
            fprintf(stderr, "[emme] LU workgroups per matrix %d\n", c->last_lu_nwg);
            fprintf(stderr, "[emme] iter %2d: assembled %3d, lane-intervals %10llu (max/item %9llu), still active %d\n",
                    j_pending, nprev, tot, mx, na);
        }
    };
    // eigenpair search: the flags as every launch_newton_update leaves them, read at the step's one synchronisation --
    // the list of the next factorisation is exact (it writes d_info of what it is given), where `act` is a step old
    const bool eig = search.eigpair;
    if (eig) std::fill(c->p_live.get(), c->p_live.get() + n, 1);
    for (int j = 0; j <= step_limit; ++j) {  // src/main.cpp:43
        const bool fused_copy = method == EMME_METHOD_TRACE_SECANT;
        // Option eigpair_fold: under the routing rule of the folded trace step -- both fills mirrored
        // for every live chain, an even order whose halves fit -- the eigenpair step factors the even and the odd block
        // instead.  Not the first step of a call without v0, which also makes v_0 = M^-1 s.
        // (d_Mp holds the half problems' S': solve_eigenpairs allocates it exactly where a step can fold, and a step
        // without it is never folded.  The list of the folded step is p_live == 1, which is d_active == 1: k_retire
        // only turns 2 into 0 after the flags were read; the kernels check d_active as well, as the parent's does.)
        // (electrostatic only: the matrix of a mirrored electromagnetic context is a 2 x 2 block matrix of
        // centrosymmetric blocks, not centrosymmetric itself -- its even order dim = 2 N must not route it here)
        const bool pair_mirrored = c->mirror && c->nm == 1 && old_mirrored && new_mirrored;  // both matrices of the secant
        const bool eig_folded = eig && c->eigpair_fold != 0 && pair_mirrored &&
                                eigpair_fold_applies(c, c->dim) && !(j == 0 && !search.v0) && !search.set &&
                                c->d_Mp.bytes() >= batch_bytes(c->dim, n);
        if (eig_folded) {
            EMME_TRY(folded_eigpair_secant_step(c, c->dim, n, c->d_M, c->d_Mold, c->d_work, c->d_Mp, c->d_domega, c->d_active,
                                                c->p_live.get(), c->d_vecs, c->d_tr, c->d_resid, c->d_info));
            ++c->last_folded_eigpair_steps;
            // (the fold pass writes upper triangles only; an unfolded step that follows reads whole rows of M_old)
            ScopedSpan s(c, K_OTHER);
            HIP_TRY(launch_copy_active(c->dim, n, c->d_M, c->d_Mold, nullptr, c->d_active, c->stream));
        } else if (eig) {
            // the work copy of the live M, its factorisation and the secant eigenpair step on (M, M_old, domega); then
            // this step's matrix becomes the "previous" one
            {
                ScopedSpan s(c, K_LIN);
                HIP_TRY(launch_copy_active(c->dim, n, c->d_M, c->d_work, nullptr, c->d_active, c->stream));
            }
            EMME_TRY(eigpair_step(c, search, c->p_live.get(), j == 0 && !search.v0, true));
            ScopedSpan s(c, K_OTHER);
            HIP_TRY(launch_copy_active(c->dim, n, c->d_M, c->d_Mold, nullptr, c->d_active, c->stream));
        } else if (fused_copy && pair_mirrored && fold_applies(c, c->dim)) {
            // both fills mirrored: the even and the odd block instead of the matrix; M_old follows M in the same pass
            EMME_TRY(folded_secant_step(c, c->dim, n, c->d_M, c->d_Mold, c->d_Mold, c->d_work, c->d_Mp, c->d_domega,
                                        c->d_active, c->d_tr, c->d_info, act.data()));
            ++c->last_folded_steps;
        } else {
            {
                // the secant M' of the step just taken, then this step's matrix becomes the "previous" one (and the
                // LU's work copy): one pass, for the chains still iterating only
                ScopedSpan s(c, K_OTHER);
                HIP_TRY(launch_secant_copy_sym(c->dim, n, c->d_M, c->d_Mold, fused_copy ? c->d_work : nullptr, c->d_Mp,
                                               c->d_domega, c->d_active, c->stream));
            }
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
        if (eig) HIP_TRY(hipMemcpyAsync(c->p_live, c->d_active, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        std::copy(c->p_w.get(), c->p_w.get() + 2 * (size_t)n, h_w.begin());
        if (pending) {
            take_pending();
            bool any = false;
            for (int b = 0; b < n; ++b) any |= act[b] != 0;
            if (!any) break;  // (this step's LU and update found nothing active: no-ops)
        }
        old_mirrored = new_mirrored;  // (the step's pass has made M_old of M)
        EMME_TRY(fill(c, next));
        new_mirrored = c->last_fill_mirrored;
        {
            ScopedSpan s(c, K_OTHER);
            HIP_TRY(launch_retire(n, c->d_active, c->stream, c->p_act, c->d_intervals, c->p_iv,
                                  c->d_worklist_count, c->p_deferred, c->d_overflow, c->p_overflow));
        }
        pending = true, j_pending = j;
    }
    if (eig) {
        // the residual of what is returned, omega and v, on the last fill's matrix, as newton_loop takes it
        ScopedSpan s(c, K_LIN);
        HIP_TRY(launch_eigpair_resid(c->dim, c->d_M, nullptr, n, c->d_vecs, c->d_resid, c->stream));
    }
    return EMME_OK;
}

// The Newton search of emme_solve_roots_newton, between search_begin and search_end; with
// search.eigpair, that of emme_solve_eigenpairs: the same loop around another linear step.
int newton_loop(emme_ctx* c, RootSearch& search) {
    const int n = search.n, method = search.method, step_limit = search.step_limit, stride = search.stride();
    const double tol = search.tol;
    double* const d_iterates = search.d_iterates(c);
    std::vector<int>& act = search.act;
    // omega_0 = g: one fill of M and the exact M' there, no secant bootstrap
    HIP_TRY(hipMemcpyAsync(c->d_omega, search.guesses, sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
    FillRequest both(n, c->d_omega, c->d_M);
    both.d_Md = c->d_Mp, both.d_active = c->d_active, both.host_active = act.data();
    search.to(c, both);
    // Option deriv_cached: the fills may go through the node cache, which needs what the secant loop gives its fills --
    // the live omegas on the host (contour classes), every omega's interval count of its previous fill (cost order)
    // and the root-search flag (skip_lost).  They travel as there: k_newton_update writes the omegas, k_retire the
    // counters and the deferred count into pinned memory, read after the step's one synchronisation.
    const bool cached = c->opt.deriv_cached != 0;
    std::vector<double> h_w;
    StepFeedback& fb = c->fb;
    bool pending = false;
    if (cached) {
        h_w.assign(search.guesses, search.guesses + 2 * (size_t)n);
        fb.begin(n);
        both.host_omega = h_w.data(), both.newton_loop = true;
        fb.pub_valid = false;
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
        both.cost = fb.cost.data();
    }
    for (int j = 0; j <= step_limit; ++j) {
        {
            // the step of the context's iteration_method on (M, M'): trace form on a work copy of M (the LU destroys
            // both operands; M' is filled again before it is needed), QR form on the transpose
            ScopedSpan s(c, K_LIN);
            const bool trace = method == EMME_METHOD_TRACE_SECANT;
            if (trace || search.eigpair) HIP_TRY(launch_copy_active(c->dim, n, c->d_M, c->d_work, nullptr, c->d_active, c->stream));
            if (!search.eigpair)
                HIP_TRY(linear_step(c, method, c->dim, n, c->d_M, c->d_work, c->d_Mp, c->d_active, c->d_tr, c->d_info,
                                    act.data(), trace));
        }
        // the eigenpair search: d_tr <- v^H M^-1 M' v instead, and the chain's vector moves with it
        if (search.eigpair) EMME_TRY(eigpair_step(c, search, act.data(), j == 0 && !search.v0, false));
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
                fb.take(c->p_iv, nullptr, 0, c->p_deferred);
                pending = false;
            }
        }
        EMME_TRY(fill(c, both));
        {
            ScopedSpan s(c, K_OTHER);
            HIP_TRY(publish());
        }
    }
    if (search.eigpair) {
        // every chain whose last step was followed by a fill (converged, or out of steps): the residual of what is
        // returned, omega and v, on that matrix.  (Chains that failed hold anything: emme_solve_eigenpairs blanks them.)
        ScopedSpan s(c, K_LIN);
        HIP_TRY(launch_eigpair_resid(c->dim, c->d_M, nullptr, n, c->d_vecs, c->d_resid, c->stream));
    }
    return EMME_OK;
}

// eigpair: the eigenpair search (newton_loop only; v0: its start vectors or null), which consults no iteration method
int run_search(emme_ctx* c, const double* guesses, int n, double tol, int step_limit, double* roots, int* iters, int* info,
               double* iterates, int mat_sets, int (*loop)(emme_ctx*, RootSearch&), const int* set = nullptr,
               bool eigpair = false, const double* v0 = nullptr) {
    if (!c || !guesses || !roots || !iters || !info || n < 1 || step_limit < 0) return EMME_EINVAL;
    RootSearch s{guesses, n, tol, step_limit, iterates != nullptr};
    s.method = c->p.iteration_method;  // src/main.cpp:45-49
    s.set = set;
    s.eigpair = eigpair, s.v0 = v0;
    if (!eigpair) EMME_TRY(check_method(c, s.method));
    HIP_TRY(hipSetDevice(c->device));
    for (;;) {
        bool repeat = false;
        EMME_TRY(search_begin(c, s, mat_sets));
        EMME_TRY(loop(c, s));
        EMME_TRY(search_end(c, s, roots, iters, info, iterates, &repeat));
        if (!repeat) return EMME_OK;
    }
}

// What emme_solve_eigenpairs (newton_loop: exact M') and emme_solve_eigenpairs_secant (secant_loop: two plain fills)
// are: the argument rules, the start vectors normalised, the search, the pairs read back and failed chains blanked
int solve_eigenpairs(emme_ctx* c, const std::string& who, bool secant, const int* set, const double* guesses, int n,
                     const double* v0, double tol, int step_limit, double* roots, double* vecs, double* resid, int* iters,
                     int* info, double* iterates) {
    if (!c || !guesses || !roots || !vecs || !resid || !iters || !info || n < 1 || step_limit < 0 || !(tol > 0.0)) {
        set_error(who + ": a required pointer is NULL, n < 1, step_limit < 0 or tol <= 0");
        return EMME_EINVAL;
    }
    const int dim = c->dim;
    if (dim > 2048) {
        set_error(who + ": matrix dimension above 2048 is not supported");
        return EMME_ECONFIG;
    }
    if (set) EMME_TRY(check_set_indices(c, set, n, who.c_str()));
    std::vector<double> vn;  // the caller's start vectors, each of unit 2-norm
    if (v0) {
        vn.assign(v0, v0 + 2 * (size_t)n * dim);
        for (int b = 0; b < n; ++b) {
            double* row = vn.data() + 2 * (size_t)b * dim;
            double s2 = 0.0;
            for (int i = 0; i < 2 * dim; ++i) s2 += row[i] * row[i];
            const double nrm = std::sqrt(s2);
            if (!(nrm > 0.0) || !std::isfinite(nrm)) {
                set_error(who + ": v0 row " + std::to_string(b) + " is zero or not finite");
                return EMME_EINVAL;
            }
            for (int i = 0; i < 2 * dim; ++i) row[i] /= nrm;
        }
    }
    // (the secant search keeps M, M_old and the work copy: no M' -- with the option eigpair_fold its set holds the half
    // problems' S')
    // -- only where a step can fold at all: no parameter sets, an order whose halves qualify, and a node cache that is,
    // or once allocated would be, laid out over the half pair list
    // (and an electrostatic context: see pair_mirrored in secant_loop)
    const bool may_fold = c->eigpair_fold != 0 && !set && c->nm == 1 && eigpair_fold_applies(c, dim) &&
                          ((c->cache[0].recs || c->cache[1].recs) ? c->mirror : mirror_wanted(c));
    const int secant_sets = 1 | 2 | 8 | (may_fold ? 4 : 0);
    EMME_TRY(run_search(c, guesses, n, tol, step_limit, roots, iters, info, iterates, secant ? secant_sets : 1 | 4 | 8,
                        secant ? secant_loop : newton_loop, set, true, v0 ? vn.data() : nullptr));
    HIP_TRY(hipMemcpyAsync(vecs, c->d_vecs, sizeof(double) * 2 * (size_t)n * dim, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(resid, c->d_resid, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    for (int b = 0; b < n; ++b)
        if (info[b] != 0) {  // a failed chain has no pair
            std::fill(vecs + 2 * (size_t)b * dim, vecs + 2 * (size_t)(b + 1) * dim, qnan);
            resid[b] = qnan;
        }
    return EMME_OK;
}

}  // namespace

extern "C" {

int emme_newton_step_batch(emme_ctx_t* c, double* omega, double* domega, int nbatch, double* M,
                           double* Mp, int method, int* info) {
    if (!c || !omega || !domega || !M || !Mp || !info || nbatch < 1) return EMME_EINVAL;
    EMME_TRY(check_method(c, method));
    HIP_TRY(hipSetDevice(c->device));
    // (every copy kind below follows from this one side)
    bool dev = false;
    const void* const arrays[5] = {omega, domega, M, Mp, info};
    EMME_TRY(same_side_all(arrays, 5, "emme_newton_step_batch: omega, domega, M, Mp and info", &dev));
    EMME_TRY(ensure_batch(c, nbatch));
    const size_t mbytes = batch_bytes(c->dim, nbatch);
    EMME_TRY(ensure_mats(c, nbatch, dev ? (2 | 8) : (1 | 2 | 4 | 8)));
    double *dM = M, *dMp = Mp;
    if (!dev) {
        dM = c->d_M, dMp = c->d_Mp;
        HIP_TRY(hipMemcpyAsync(dM, M, mbytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(dMp, Mp, mbytes, hipMemcpyHostToDevice, c->stream));
    }
    const hipMemcpyKind in_kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind out_kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
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
    std::vector<unsigned long long> iv;
    EMME_TRY(queue_fill_counters(c, nbatch, iv, nullptr));  // (the status flags are not this call's to report)
    HIP_TRY(hipMemcpyAsync(info, c->d_info, sizeof(int) * nbatch, out_kind, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    (void)fold_fill_counters(c, iv, nullptr);
    return EMME_OK;
}

int emme_solve_roots(emme_ctx_t* c, const double* guesses, int n, double tol, int step_limit,
                     double* roots, int* iters, int* info, double* iterates) {
    return run_search(c, guesses, n, tol, step_limit, roots, iters, info, iterates, 1 | 2 | 4 | 8, secant_loop);
}

int emme_solve_roots_newton(emme_ctx_t* c, const double* guesses, int n, double tol, int step_limit, double* roots,
                            int* iters, int* info, double* iterates) {
    return run_search(c, guesses, n, tol, step_limit, roots, iters, info, iterates, 1 | 4 | 8, newton_loop);  // (no M_old)
}

int emme_solve_roots_sets(emme_ctx_t* c, const int* set, const double* guesses, int n, int exact, double tol,
                          int step_limit, double* roots, int* iters, int* info, double* iterates) {
    if (!c || !set || !guesses || !roots || !iters || !info || n < 1 || step_limit < 0) return EMME_EINVAL;
    EMME_TRY(check_set_indices(c, set, n, "emme_solve_roots_sets"));
    return exact ? run_search(c, guesses, n, tol, step_limit, roots, iters, info, iterates, 1 | 4 | 8, newton_loop, set)
                 : run_search(c, guesses, n, tol, step_limit, roots, iters, info, iterates, 1 | 2 | 4 | 8, secant_loop, set);
}

// Newton on the eigenpair: newton_loop around k_eigpair_step
int emme_solve_eigenpairs(emme_ctx_t* c, const int* set, const double* guesses, int n, const double* v0, double tol,
                          int step_limit, double* roots, double* vecs, double* resid, int* iters, int* info,
                          double* iterates) {
    return solve_eigenpairs(c, "emme_solve_eigenpairs", false, set, guesses, n, v0, tol, step_limit, roots, vecs, resid, iters,
                            info, iterates);
}

// The same on two consecutive plain fills: secant_loop around k_eigpair_secant_step
int emme_solve_eigenpairs_secant(emme_ctx_t* c, const int* set, const double* guesses, int n, const double* v0, double tol,
                                 int step_limit, double* roots, double* vecs, double* resid, int* iters, int* info,
                                 double* iterates) {
    return solve_eigenpairs(c, "emme_solve_eigenpairs_secant", true, set, guesses, n, v0, tol, step_limit, roots, vecs, resid,
                            iters, info, iterates);
}

}  // extern "C"
