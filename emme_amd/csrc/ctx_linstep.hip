// ctx_linstep.hip -- the Newton linear step and the batched LU above their kernels (linstep*.hip, nullspace.hip):
// which kernel and how many workgroups a launch gets (linstep_plan.hpp), operands staged where the kernels can read
// them, and the entry points emme_trace_solve_batch, emme_qr_secant_batch, emme_null_vectors_batch,
// emme_eigenpair_step_batch, emme_eigenpair_secant_step_batch.
#include "ctx.hpp"
#include "linstep_plan.hpp"

using namespace emme;

namespace {

// what the getters report of the context's last LU launch (emme_ctx_linstep_kernel_symbol and its two companions):
// written together, and only where a launch was made
void note_lu_launch(emme_ctx* c, const char* symbol, int nwg, int slices) {
    c->last_lu_symbol = symbol, c->last_lu_nwg = nwg, c->last_lu_slices = slices;
}

// the Newton linear step: blocked kernel while its panel fits in LDS, else the unblocked one
// `h_active`: host copy of `active` (null: all live).  With fewer live matrices than compute
// units each gets several workgroups (lu_workgroups, linstep_plan.hpp).
hipError_t trace_solve(emme_ctx* c, int n, int nbatch, double* A, double* B, const int* active,
                       double* tr, int* info, const int* h_active) {
    // n <= 525: the whole L21 panel fits in LDS; up to 1024 the chunked build takes over, which
    // needs helper workgroups (>= 2 per matrix, all resident); otherwise the unblocked kernel
    const bool fits = trace_solve_blocked_lds(n) <= 150 * 1024;
    if (c->opt.lu_unblocked == 0 && (fits || n <= 1024)) {
        hipError_t e = c->d_lu_scratch.grow(trace_solve_blocked_scratch(n, nbatch));
        if (e != hipSuccess) return e;
        // dense list of the live matrices (h_active: host copy of `active`, null = all live)
        int n_live = nbatch;
        int* lu_slot = nullptr;
        if (h_active) {
            e = live_list_fill(c, c->d_lu_items, h_active, nbatch, 1, [](int f) { return f != 0; }, &lu_slot, &n_live);
            if (e != hipSuccess || n_live == 0) return e;
        }
        const int nwg = lu_workgroups(n, n_live, c->n_cu, c->opt.lu_split, c->lu_one_wg, fits);
        const int* d_items = nullptr;
        if (nwg > 1 && h_active) {  // (one workgroup per matrix reads the flags themselves)
            e = live_list_send(c, lu_slot, c->d_lu_items, n_live);
            if (e != hipSuccess) return e;
            d_items = c->d_lu_items;
        }
        LuRoute route;
        e = launch_trace_solve_blocked(n, nbatch, A, B, active, tr, info, nwg, d_items, n_live, c->d_lu_scratch, c->stream,
                                       c->opt.lu_group_min_n, c->opt.lu_spin_limit, &route);
        if (e != hipErrorNotSupported) {
            // (the launcher itself falls back to one workgroup per matrix where a split grid cannot be resident)
            if (route.nwg > 0) note_lu_launch(c, route.symbol, route.nwg, 1);
            return e;
        }
        (void)hipGetLastError();  // chunked build not possible here (one workgroup per matrix, or no room)
    }
    const hipError_t e = launch_trace_solve(n, nbatch, A, B, active, tr, info, c->stream);
    if (e == hipSuccess) note_lu_launch(c, LU_SYM_UNBLOCKED, 1, 1);
    return e;
}

// The two operands of a linear step where the kernels can read them: A and B themselves if they are device
// pointers, else copies that live as long as this object.  EMME_EINVAL if one is on the host and one on the device;
// otherwise *e is the status of the allocations and copies, which each caller reports in its own words.
struct DeviceOperands {
    double *A = nullptr, *B = nullptr;  // (written only by a caller whose own operands are not const)
    DeviceBuffer<double> st_a, st_b;
    int stage(emme_ctx* c, const double* hA, const double* hB, size_t bytes, hipError_t* e) {
        bool dev = false;
        EMME_TRY(same_side(hA, hB, "A and B", &dev));
        A = const_cast<double*>(hA), B = const_cast<double*>(hB), *e = hipSuccess;
        if (dev) return EMME_OK;
        if ((*e = st_a.grow(bytes)) == hipSuccess) *e = st_b.grow(bytes);
        if (*e == hipSuccess) *e = hipMemcpyAsync(st_a, hA, bytes, hipMemcpyHostToDevice, c->stream);
        if (*e == hipSuccess) *e = hipMemcpyAsync(st_b, hB, bytes, hipMemcpyHostToDevice, c->stream);
        A = st_a, B = st_b;
        return EMME_OK;
    }
};

}  // namespace

namespace emme {

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

// One Newton linear step on the batch: leaves tr[b] with domega = -1/tr[b].
//   trace-secant (include/solver.h:113-160): work <- M, LU of [work | Mp], tr(M^-1 M')
//   QR-secant    (include/solver.h:210-383): work <- M^T, pivoted QR of work, t_n / R_nn
hipError_t linear_step(emme_ctx* c, int method, int n, int nbatch, const double* M, double* work,
                       double* Mp, const int* active, double* tr, int* info, const int* h_active, bool work_ready) {
    if (method == EMME_METHOD_QR_SECANT) {
        hipError_t e = launch_transpose(n, nbatch, M, work, active, c->stream);
        if (e != hipSuccess) return e;
        return launch_qr_secant(n, nbatch, work, Mp, active, tr, info, c->stream);
    }
    if (!work_ready) {  // (the root search copies M -> work together with M -> Mold)
        hipError_t e = hipMemcpyAsync(work, M, batch_bytes(n, nbatch), hipMemcpyDeviceToDevice, c->stream);
        if (e != hipSuccess) return e;
    }
    return trace_solve(c, n, nbatch, work, Mp, active, tr, info, h_active);
}

// an even order whose halves fit the one-workgroup kernels (k_lu_inplace, the blocked trace kernel, the solve frame)
bool halves_fit(const emme_ctx* c, int n) {
    return n >= 2 && n % 2 == 0 && c->opt.lu_unblocked == 0 && trace_solve_blocked_lds(n / 2) <= 150 * 1024 &&
           null_iterate_lds(n / 2) <= 150 * 1024;
}
bool fold_applies(const emme_ctx* c, int n) { return c->lu_fold != 0 && halves_fit(c, n); }
bool eigpair_fold_applies(const emme_ctx* c, int n) { return halves_fit(c, n); }

namespace {

// What the two folded steps share.  The four matrix areas: the first halves of `work` and `Mp` (S1, D1) and the second
// halves (S2, D2) receive the same S and S' from the pass -- a factorisation destroys the copy it is given.
struct FoldAreas {
    int m, nhalf;
    double *S1, *S2, *D1, *D2;
    FoldAreas(int n, int nbatch, double* work, double* Mp) : m(n / 2), nhalf(2 * nbatch) {
        const size_t second = (size_t)nbatch * n * n;  // doubles: half of a set of nbatch n x n complex matrices
        S1 = work, S2 = work + second, D1 = Mp, D2 = Mp + second;
    }
};
// the scratch both steps use: the folds of u and u', the half problems' flags, the codes and row orders of k_lu_inplace
int fold_scratch(emme_ctx::FoldScratch& f, const FoldAreas& a) {
    HIP_TRY(f.vecs.grow(sizeof(double) * 2 * 4 * (size_t)a.m * (a.nhalf / 2)));
    HIP_TRY(f.act2.grow(sizeof(int) * a.nhalf));
    HIP_TRY(f.lu_info.grow(sizeof(int) * a.nhalf));
    HIP_TRY(f.lu_scratch.grow(trace_solve_blocked_scratch(a.m, a.nhalf)));
    return EMME_OK;
}
// k_fold_edges and k_fold_pass under one profile span of the caller's kind
int fold_edges_and_pass(emme_ctx* c, int kind, int n, int nbatch, const double* M, const double* Mold, double* Mold_w,
                        const FoldAreas& a, const double* domega, const int* active) {
    ScopedSpan s(c, kind);
    HIP_TRY(launch_fold_edges(n, nbatch, M, Mold, domega, active, c->fold.vecs, c->fold.act2, c->stream));
    HIP_TRY(launch_fold_pass(n, nbatch, M, Mold, Mold_w, a.S1, a.S2, a.D1, a.D2, domega, active, c->stream));
    return EMME_OK;
}
// the live half problems, the two of a chain side by side, on their way to f.items (flags null: all of them, no list)
template <class Keep>
int fold_live_halves(emme_ctx* c, const int* flags, int nbatch, Keep keep, const int** d_items, int* n_live) {
    *d_items = nullptr, *n_live = 2 * nbatch;
    if (!flags) return EMME_OK;
    HIP_TRY(c->lists.reserve(2 * nbatch));
    HIP_TRY(stage_live_list(c, c->fold.items, flags, nbatch, 2, keep, n_live));
    *d_items = c->fold.items;
    return EMME_OK;
}

}  // namespace

// The folded step (linstep_fold.hip): the fold pass, then per half problem the trace kernel on [S | S'] and, for the
// rank-2 part, a second factorisation that keeps its factors (the one-workgroup trace kernel keeps its multipliers in
// LDS) with two full solves behind it, then the sum per chain.  The first halves of `work` and `Mp` hold what the
// factorisations destroy, the second halves the copies that are read afterwards.
int folded_secant_step(emme_ctx* c, int n, int nbatch, const double* M, const double* Mold, double* Mold_w, double* work,
                       double* Mp, const double* domega, const int* active, double* tr, int* info, const int* h_active) {
    const FoldAreas a(n, nbatch, work, Mp);
    const int m = a.m, nhalf = a.nhalf;
    emme_ctx::FoldScratch& f = c->fold;
    EMME_TRY(fold_scratch(f, a));
    HIP_TRY(f.tr2.grow(sizeof(double) * 2 * nhalf));
    HIP_TRY(f.part.grow(fold_part_bytes(nbatch)));
    HIP_TRY(f.info2.grow(sizeof(int) * nhalf));
    EMME_TRY(fold_edges_and_pass(c, K_OTHER, n, nbatch, M, Mold, Mold_w, a, domega, active));
    // the live half problems: host flags for the trace kernel's launch, a device list for the other two
    std::vector<int> h2;
    const int* d_items = nullptr;
    int n_live = nhalf;
    if (h_active) {
        h2.resize(nhalf);
        for (int b = 0; b < nbatch; ++b) h2[2 * b] = h2[2 * b + 1] = h_active[b] != 0;
    }
    EMME_TRY(fold_live_halves(c, h_active, nbatch, [](int flag) { return flag != 0; }, &d_items, &n_live));
    if (n_live == 0) return EMME_OK;
    ScopedSpan s(c, K_LIN);
    HIP_TRY(launch_lu_inplace(m, nhalf, a.S2, d_items, n_live, f.lu_info, f.lu_scratch, c->stream));
    HIP_TRY(trace_solve(c, m, nhalf, a.S1, a.D1, f.act2, f.tr2, f.info2, h_active ? h2.data() : nullptr));
    HIP_TRY(launch_fold_solve(m, a.S2, trace_solve_rowmaps(f.lu_scratch, m, nhalf), trace_solve_nb(), d_items, n_live,
                              f.lu_info, a.D2, f.vecs, f.part, c->stream));
    HIP_TRY(launch_fold_combine(n, nbatch, active, f.tr2, f.info2, f.lu_info, f.part, tr, info, c->stream));
    return EMME_OK;
}

// The folded secant eigenpair step (eigpair_fold.hip): the fold pass, ONE factorisation per half problem that keeps its
// factors, then the half problems' solves and the chains' sums.  The first half of `work` holds what the factorisation
// destroys, the second halves of `work` and `Mp` the copies of S and S' that are read afterwards (the first half of
// `Mp` is the pass's other copy of S', which nothing reads here).  M_old is not written: an unfolded step that follows
// reads whole rows of it, and the search's own copy M -> M_old stays.
int folded_eigpair_secant_step(emme_ctx* c, int n, int nbatch, const double* M, const double* Mold, double* work, double* Mp,
                               const double* domega, const int* active, const int* h_live, double* vecs, double* tau,
                               double* resid, int* info) {
    const FoldAreas a(n, nbatch, work, Mp);
    const int m = a.m, nhalf = a.nhalf;
    emme_ctx::FoldScratch& f = c->fold;
    EMME_TRY(fold_scratch(f, a));
    HIP_TRY(f.eig_vecs.grow(eigpair_fold_vec_bytes(n, nbatch)));
    HIP_TRY(f.eig_part.grow(eigpair_fold_part_bytes(nbatch)));
    // the list goes first: an empty one launches nothing
    const int* d_items = nullptr;
    int n_live = nhalf;
    EMME_TRY(fold_live_halves(c, h_live, nbatch, [](int flag) { return flag == 1; }, &d_items, &n_live));
    if (n_live == 0) return EMME_OK;
    EMME_TRY(fold_edges_and_pass(c, K_LIN, n, nbatch, M, Mold, nullptr, a, domega, active));
    ScopedSpan s(c, K_NULL);
    HIP_TRY(launch_lu_inplace(m, nhalf, a.S1, d_items, n_live, f.lu_info, f.lu_scratch, c->stream));
    note_lu_launch(c, LU_SYM_INPLACE, 1, 1);
    HIP_TRY(launch_eigpair_fold_half(n, a.S1, trace_solve_rowmaps(f.lu_scratch, m, nhalf), trace_solve_nb(), d_items, n_live,
                                     active, f.lu_info, a.S2, a.D2, f.vecs, vecs, f.eig_vecs, f.eig_part, c->stream));
    HIP_TRY(launch_eigpair_fold_combine(n, d_items, n_live / 2, active, M, domega, f.vecs, f.lu_info, f.eig_vecs, f.eig_part, vecs,
                                        tau, resid, info, c->stream));
    return EMME_OK;
}

// Partial-pivot LU of nbatch n x n matrices in place (P M = L U, rows never moved; n <= 2048), by the branch the
// order allows: k_lu_inplace where the whole L21 panel fits one workgroup's LDS; above that, up to n = 1024, the chunked
// multi-workgroup kernel of the Newton step (two workgroups per matrix, which must be resident together: slices of at
// most half the compute units; its right-hand side is a dummy); beyond, k_lu_unblocked_inplace.  After each slice's
// factorisation `after(b0, nb, maps, map_nb, lu_info)` queues what reads it: matrices b0 .. b0 + nb - 1, their row-order
// snapshots (logical row x of slice item b is physical row maps[(b ceil(n / map_nb) + x / map_nb) n + x]) and their
// info (0 or the column at which the factorisation stopped), both valid until the next slice is factored.  Used by
// emme_null_vectors_batch and the contour solver (contour.hip); the launches are stream-ordered on c->stream.
// With an item list (d_items: device list of nitems batch indices, the root search's live chains) only the listed
// matrices are factored, and nothing is relative to a slice: `after(i0, ni, ...)` gets the list positions i0 .. i0 + ni
// - 1 of the slice, maps and lu_info are indexed by the batch index itself, and the info goes to c->d_info[b].  (A
// context whose multi-workgroup LU has timed out once, lu_one_wg, takes the unblocked kernel instead of the chunked.)
int lu_factor_batch(emme_ctx* c, int n, int nbatch, double* work, LuScratch& s, const char* who,
                    const std::function<hipError_t(int, int, const int*, int, const int*)>& after, const int* d_items,
                    int nitems) {
    const size_t mbytes = batch_bytes(n, 1);
    const bool one_wg = trace_solve_blocked_lds(n) <= 150 * 1024;  // the whole L21 panel in one workgroup's LDS
    const int todo = d_items ? nitems : nbatch;  // matrices to factor
    if (todo < 1) return EMME_OK;
    if (one_wg || (n <= 1024 && !(d_items && c->lu_one_wg))) {
        const int slice_max = one_wg ? todo : std::max(1, c->n_cu / 2);
        // (with a list the kernels index scratch, right-hand sides and row orders by the batch index)
        const int held = d_items ? nbatch : std::min(nbatch, slice_max);
        HIP_TRY(c->d_lu_scratch.grow(trace_solve_blocked_scratch(n, held)));
        if (!one_wg) HIP_TRY(s.b.grow(mbytes * held));
        int slices = 0;
        for (int b0 = 0; b0 < todo; b0 += slice_max) {
            const int nb = std::min(slice_max, todo - b0);
            double* a0 = d_items ? work : work + (size_t)b0 * n * n * 2;
            const int* list = d_items ? d_items + b0 : nullptr;
            const int dimb = d_items ? nbatch : nb;  // what the kernels' batch index runs over
            ScopedSpan sp(c, K_NULL);
            if (one_wg) {
                HIP_TRY(launch_lu_inplace(n, dimb, a0, list, nb, c->d_info, c->d_lu_scratch, c->stream));
                note_lu_launch(c, LU_SYM_INPLACE, 1, ++slices);
            } else {
                HIP_TRY(hipMemsetAsync(s.b, 0, mbytes * dimb, c->stream));
                LuRoute route;
                const hipError_t e = launch_trace_solve_blocked(n, dimb, a0, s.b, nullptr, c->d_tr, c->d_info, 2, list, nb,
                                                                c->d_lu_scratch, c->stream, -1, c->opt.lu_spin_limit, &route);
                if (e != hipSuccess) {
                    (void)hipGetLastError();
                    set_error(std::string(who) + ": the chunked factorisation could not be launched (its two workgroups per matrix must be resident together)");
                    return EMME_EDEVICE;
                }
                note_lu_launch(c, route.symbol, route.nwg, ++slices);
            }
            HIP_TRY(after(b0, nb, trace_solve_rowmaps(c->d_lu_scratch, n, dimb), trace_solve_nb(), c->d_info));
        }
    } else {
        HIP_TRY(s.maps.grow(sizeof(int) * (size_t)n * nbatch));
        ScopedSpan sp(c, K_NULL);
        HIP_TRY(launch_lu_unblocked_inplace(n, nbatch, work, s.maps, c->d_info, c->stream, d_items, nitems));
        note_lu_launch(c, LU_SYM_INPLACE_UNBLOCKED, 1, 1);
        HIP_TRY(after(0, todo, s.maps, n, c->d_info));
    }
    return EMME_OK;
}

}  // namespace emme

namespace {

// What emme_eigenpair_step_batch (domega null: Mp is dM/domega) and emme_eigenpair_secant_step_batch (domega: host,
// nbatch complex; Mp is M_old) are: one step of eigpair.hip on caller matrices, which are not modified
int caller_eigenpair_step(emme_ctx* c, const char* who, int n, int nbatch, const double* M, const double* Mp,
                          const double* domega, double* v, int have_v, double* tau, double* resid, int* info) {
    if (!c || !M || !Mp || !v || !tau || !resid || !info || n < 1 || nbatch < 1) {
        set_error(std::string(who) + ": a required pointer is NULL, n < 1 or nbatch < 1");
        return EMME_EINVAL;
    }
    if (n > 2048) {
        set_error(std::string(who) + ": order above 2048 is not supported");
        return EMME_ECONFIG;
    }
    HIP_TRY(hipSetDevice(c->device));
    EMME_TRY(ensure_batch(c, nbatch));
    const size_t bytes = batch_bytes(n, nbatch), vbytes = sizeof(double) * 2 * (size_t)n * nbatch;
    DeviceOperands ops;
    hipError_t staged = hipSuccess;
    EMME_TRY(ops.stage(c, M, Mp, bytes, &staged));
    HIP_TRY(staged);
    // device scratch of this call: the work copy the factorisation overwrites, vectors, tau, residuals, info
    DeviceBuffer<double> t_a, t_v, t_tau, t_res, t_dw;
    DeviceBuffer<int> t_info;
    HIP_TRY(t_a.grow(bytes));
    HIP_TRY(t_v.grow(vbytes));
    HIP_TRY(t_tau.grow(sizeof(double) * 2 * nbatch));
    HIP_TRY(t_res.grow(sizeof(double) * nbatch));
    HIP_TRY(t_info.grow(sizeof(int) * nbatch));
    HIP_TRY(hipMemcpyAsync(t_a, ops.A, bytes, hipMemcpyDeviceToDevice, c->stream));
    if (have_v) HIP_TRY(hipMemcpyAsync(t_v, v, vbytes, hipMemcpyHostToDevice, c->stream));
    if (domega) {
        HIP_TRY(t_dw.grow(sizeof(double) * 2 * nbatch));
        HIP_TRY(hipMemcpyAsync(t_dw, domega, sizeof(double) * 2 * nbatch, hipMemcpyHostToDevice, c->stream));
    }
    LuScratch scratch;
    const int rc = lu_factor_batch(c, n, nbatch, t_a, scratch, who,
                                   [&](int b0, int nb, const int* maps, int map_nb, const int* lu_info) -> hipError_t {
                                       const size_t m0 = (size_t)b0 * n * n * 2;
                                       if (domega)
                                           return launch_eigpair_secant_step(n, ops.A + m0, ops.B + m0, t_dw + 2 * b0, t_a + m0, maps,
                                                                             map_nb, nullptr, nb, nullptr, lu_info,
                                                                             t_v + (size_t)b0 * n * 2, t_tau + 2 * b0, t_res + b0,
                                                                             t_info + b0, !have_v, c->stream);
                                       return launch_eigpair_step(n, ops.A + m0, ops.B + m0, t_a + m0, maps, map_nb, nullptr, nb,
                                                                  nullptr, lu_info, t_v + (size_t)b0 * n * 2, t_tau + 2 * b0,
                                                                  t_res + b0, t_info + b0, !have_v, c->stream);
                                   });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(v, t_v, vbytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(tau, t_tau, sizeof(double) * 2 * nbatch, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(resid, t_res, sizeof(double) * nbatch, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(info, t_info, sizeof(int) * nbatch, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EMME_OK;
}

}  // namespace

extern "C" {

int emme_trace_solve_batch(emme_ctx_t* c, int n, int nbatch, double* A, double* B, double* tr,
                           int* info) {
    if (!c || !A || !B || !tr || !info || n < 1 || nbatch < 1) return EMME_EINVAL;
    if ((size_t)2 * n * sizeof(double2) > 64 * 1024) {
        set_error("n too large for the LDS-staged pivot row");
        return EMME_EINVAL;
    }
    HIP_TRY(hipSetDevice(c->device));
    EMME_TRY(ensure_batch(c, nbatch));
    const size_t bytes = batch_bytes(n, nbatch);
    DeviceOperands ops;
    hipError_t staged = hipSuccess;
    EMME_TRY(ops.stage(c, A, B, bytes, &staged));
    HIP_TRY(staged);
    {
        ScopedSpan s(c, K_LIN);
        HIP_TRY(trace_solve(c, n, nbatch, ops.A, ops.B, nullptr, c->d_tr, c->d_info, nullptr));
    }
    HIP_TRY(hipMemcpyAsync(tr, c->d_tr, sizeof(double) * 2 * nbatch, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(info, c->d_info, sizeof(int) * nbatch, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EMME_OK;
}

// The folded trace-secant step on caller matrices, whatever the context's lu_fold says
int emme_trace_secant_folded_batch(emme_ctx_t* c, int n, int nbatch, const double* M, const double* M_old,
                                   const double* domega, double* tr, int* info) {
    const char* who = "emme_trace_secant_folded_batch";
    if (!c || !M || !M_old || !domega || !tr || !info || n < 1 || nbatch < 1) {
        set_error(std::string(who) + ": a required pointer is NULL, n < 1 or nbatch < 1");
        return EMME_EINVAL;
    }
    if (n % 2 != 0) {
        set_error(std::string(who) + ": the order must be even");
        return EMME_EINVAL;
    }
    if (!halves_fit(c, n)) {
        set_error(std::string(who) + ": the half problems need the blocked one-workgroup kernels (order above 1050, or lu_unblocked)");
        return EMME_ECONFIG;
    }
    const void* sides[5] = {M, M_old, domega, tr, info};
    bool dev = false;
    EMME_TRY(same_side_all(sides, 5, "M, M_old, domega, tr and info", &dev));
    HIP_TRY(hipSetDevice(c->device));
    EMME_TRY(ensure_batch(c, 2 * nbatch));
    const size_t bytes = batch_bytes(n, nbatch), cb = sizeof(double) * 2 * nbatch, ib = sizeof(int) * nbatch;
    DeviceBuffer<double> t_m, t_old, t_dw, t_work, t_mp, t_tr;
    DeviceBuffer<int> t_info;
    HIP_TRY(t_work.grow(bytes));
    HIP_TRY(t_mp.grow(bytes));
    const double *dM = M, *dOld = M_old, *dDw = domega;
    double* dTr = tr;
    int* dInfo = info;
    if (!dev) {
        HIP_TRY(t_m.grow(bytes));
        HIP_TRY(t_old.grow(bytes));
        HIP_TRY(t_dw.grow(cb));
        HIP_TRY(t_tr.grow(cb));
        HIP_TRY(t_info.grow(ib));
        HIP_TRY(hipMemcpyAsync(t_m, M, bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(t_old, M_old, bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(t_dw, domega, cb, hipMemcpyHostToDevice, c->stream));
        dM = t_m, dOld = t_old, dDw = t_dw, dTr = t_tr, dInfo = t_info;
    }
    EMME_TRY(folded_secant_step(c, n, nbatch, dM, dOld, nullptr, t_work, t_mp, dDw, nullptr, dTr, dInfo, nullptr));
    if (!dev) {
        HIP_TRY(hipMemcpyAsync(tr, t_tr, cb, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(info, t_info, ib, hipMemcpyDeviceToHost, c->stream));
    }
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
    const size_t bytes = batch_bytes(n, nbatch);
    DeviceOperands ops;
    DeviceBuffer<double> dW;  // transposed work copy
    hipError_t e = hipSuccess;
    EMME_TRY(ops.stage(c, A, B, bytes, &e));
    if (e == hipErrorOutOfMemory || dW.grow(bytes) != hipSuccess) {
        set_error("hipMalloc failed");
        return EMME_ENOMEM;
    }
    {
        ScopedSpan s(c, K_LIN);
        if (e == hipSuccess) e = launch_transpose(n, nbatch, ops.A, dW, nullptr, c->stream);
        if (e == hipSuccess) e = launch_qr_secant(n, nbatch, dW, ops.B, nullptr, c->d_tr, c->d_info, c->stream);
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
    const size_t mbytes = batch_bytes(n, 1);
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

// One eigenpair step (eigpair.hip) on caller matrices, which are not modified
int emme_eigenpair_step_batch(emme_ctx_t* c, int n, int nbatch, const double* M, const double* Mp, double* v, int have_v,
                              double* tau, double* resid, int* info) {
    return caller_eigenpair_step(c, "emme_eigenpair_step_batch", n, nbatch, M, Mp, nullptr, v, have_v, tau, resid, info);
}

// The secant reading of it: M_old = the previous fill, domega (host) the step between the two
int emme_eigenpair_secant_step_batch(emme_ctx_t* c, int n, int nbatch, const double* M, const double* M_old,
                                     const double* domega, double* v, int have_v, double* tau, double* resid, int* info) {
    if (!domega) {
        set_error("emme_eigenpair_secant_step_batch: a required pointer is NULL, n < 1 or nbatch < 1");
        return EMME_EINVAL;
    }
    return caller_eigenpair_step(c, "emme_eigenpair_secant_step_batch", n, nbatch, M, M_old, domega, v, have_v, tau, resid,
                                 info);
}

// The folded secant eigenpair step on caller matrices, whatever the context's eigpair_fold says
int emme_eigenpair_secant_folded_step_batch(emme_ctx_t* c, int n, int nbatch, const double* M, const double* M_old,
                                            const double* domega, double* v, double* tau, double* resid, int* info) {
    const char* who = "emme_eigenpair_secant_folded_step_batch";
    if (!c || !M || !M_old || !domega || !v || !tau || !resid || !info || n < 2 || nbatch < 1) {
        set_error(std::string(who) + ": a required pointer is NULL, n < 2 or nbatch < 1");
        return EMME_EINVAL;
    }
    if (n % 2 != 0) {
        set_error(std::string(who) + ": the order must be even");
        return EMME_EINVAL;
    }
    if (!eigpair_fold_applies(c, n)) {
        set_error(std::string(who) + ": the half problems need the blocked one-workgroup kernels (order above 1050, or lu_unblocked)");
        return EMME_ECONFIG;
    }
    HIP_TRY(hipSetDevice(c->device));
    EMME_TRY(ensure_batch(c, 2 * nbatch));
    const size_t bytes = batch_bytes(n, nbatch), vbytes = sizeof(double) * 2 * (size_t)n * nbatch, cb = sizeof(double) * 2 * nbatch;
    DeviceOperands ops;
    hipError_t staged = hipSuccess;
    EMME_TRY(ops.stage(c, M, M_old, bytes, &staged));
    HIP_TRY(staged);
    // device scratch of this call: the half problems' work copies, vectors, domega, tau, residuals, info
    DeviceBuffer<double> t_work, t_mp, t_v, t_dw, t_tau, t_res;
    DeviceBuffer<int> t_info;
    HIP_TRY(t_work.grow(bytes));
    HIP_TRY(t_mp.grow(bytes));
    HIP_TRY(t_v.grow(vbytes));
    HIP_TRY(t_dw.grow(cb));
    HIP_TRY(t_tau.grow(cb));
    HIP_TRY(t_res.grow(sizeof(double) * nbatch));
    HIP_TRY(t_info.grow(sizeof(int) * nbatch));
    HIP_TRY(hipMemcpyAsync(t_v, v, vbytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(t_dw, domega, cb, hipMemcpyHostToDevice, c->stream));
    EMME_TRY(folded_eigpair_secant_step(c, n, nbatch, ops.A, ops.B, t_work, t_mp, t_dw, nullptr, nullptr, t_v, t_tau, t_res,
                                        t_info));
    HIP_TRY(hipMemcpyAsync(v, t_v, vbytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(tau, t_tau, cb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(resid, t_res, sizeof(double) * nbatch, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(info, t_info, sizeof(int) * nbatch, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EMME_OK;
}

}  // extern "C"
