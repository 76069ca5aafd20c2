// eigpair.hip -- one step of Newton's method on the eigenpair (omega, v) of M(omega) v = 0: nonlinear
// inverse iteration.  With |v| = 1 the bordered system M(omega) v = 0, v_k^H v = 1 gives
//     u = M(omega_k)^-1 M'(omega_k) v_k,   omega_k+1 = omega_k - 1 / (v_k^H u),   v_k+1 = u / |u|,
// so a step is ONE factorisation without right-hand sides (k_lu_inplace and its kin, linstep_blocked.hip /
// nullspace.hip), one matrix-vector product and one pair of triangular solves -- against the LU plus n right-hand
// sides of the trace form -- and the vector and the residual |M v| / |M|_F come with the root.
//
// k_eigpair_step: one 512-thread workgroup per live matrix.  The products M v and M' v go a wave per row, rows dealt
// to the waves in a fixed order (row r to wave r mod 8), every sum in a fixed order and nothing atomic: two runs are
// bit-identical.  The triangular solves and the workgroup's frame are k_null_iterate's (tri_solve.hpp).
//
// k_eigpair_secant_step: the same step for a search that holds two consecutive plain fills M = M(omega_k), M_old =
// M(omega_k-1) and no derivative: M' v is replaced by (M - M_old) v / (omega_k - omega_k-1).  ONE pass over the rows of
// both matrices takes the difference entry by entry (two separately rounded products would lose n eps / |domega / omega|
// near convergence) and gives M v, (M - M_old) v and |M|_F^2 together: no matrix M' is formed, written or read, and
// there is no separate residual pass.  Both kernels are readings of one text, eigpair_step_body<SECANT>: start vector,
// residual, tau, normalisation and finite check exist once.
#include <hip/hip_runtime.h>

#include <cmath>

#include "emme_device.hpp"
#include "launch.hpp"
#include "tri_solve.hpp"

namespace emme {

namespace {

using namespace trisolve;

struct EigArgs {
    int n, nb, nblk;     // order; rows per panel snapshot and snapshots per matrix of the factorisation
    const double2* M;    // [nbatch][n][n] the un-factored matrices
    const double2* Mp;   // [nbatch][n][n] dM/domega
    const double2* A;    // [nbatch][n][n] P M = L U in place (a work copy)
    const int* maps;     // [nbatch][nblk][n] row-order snapshots
    const int* items;    // batch indices of this launch (null: 0 .. grid-1)
    const int* active;   // nullable: an item whose flag is 0 is left alone
    const int* lu_info;  // per batch item: 0, or the column at which the factorisation stopped
    double2* vecs;       // [nbatch][n] in: v_k (not read with `first`), out: v_k+1
    double2* tau;        // [nbatch] v_k^H u
    double* resid;       // [nbatch] |M v_k| / |M|_F
    int* info;           // [nbatch]
    int first;           // v_0 = M^-1 s / |M^-1 s| before the step (s: launch.hpp)
    int resid_only;      // the residual of vecs alone: no factors read, nothing else written
};

// y = Mat x for one n x n row-major matrix: row r by wave r mod NW, columns strided over the lanes, the lanes' partial
// sums by xor shuffles.  Returns this lane's share of sum |Mat(r, c)|^2 over the wave's rows (FRO), else 0.
template <bool FRO>
__device__ __forceinline__ double matvec(int n, const double2* mat, const double2* x, double2* y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double fro = 0.0;
    for (int r = wave; r < n; r += NW) {
        const double2* row = mat + (size_t)r * n;
        cd acc = mk(0.0, 0.0);
#pragma unroll 4
        for (int c = lane; c < n; c += 64) {
            const cd m = ld2(&row[c]);
            acc = acc + m * mk(x[c].x, x[c].y);
            if (FRO) fro += norm2(m);
        }
        acc.x = wave_sum(acc.x), acc.y = wave_sum(acc.y);
        if (lane == 0) y[r] = make_double2(acc.x, acc.y);
    }
    return fro;
}

// y = Mat x and yd = (Mat - Old) x in one pass, rows, columns and sums as matvec: the difference is taken per entry
// before it meets x.  Returns this lane's share of sum |Mat(r, c)|^2 over the wave's rows.
__device__ __forceinline__ double matvec_diff(int n, const double2* mat, const double2* old, const double2* x, double2* y,
                                              double2* yd) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double fro = 0.0;
    for (int r = wave; r < n; r += NW) {
        const double2* row = mat + (size_t)r * n;
        const double2* row_old = old + (size_t)r * n;
        cd acc = mk(0.0, 0.0), acc_d = mk(0.0, 0.0);
#pragma unroll 4
        for (int c = lane; c < n; c += 64) {
            const cd m = ld2(&row[c]), mo = ld2(&row_old[c]);
            const cd xc = mk(x[c].x, x[c].y);
            acc_d = acc_d + (m - mo) * xc;
            acc = acc + m * xc;
            fro += norm2(m);
        }
        acc.x = wave_sum(acc.x), acc.y = wave_sum(acc.y);
        acc_d.x = wave_sum(acc_d.x), acc_d.y = wave_sum(acc_d.y);
        if (lane == 0) y[r] = make_double2(acc.x, acc.y), yd[r] = make_double2(acc_d.x, acc_d.y);
    }
    return fro;
}

// The step, plain (SECANT = false: P.Mp is dM/domega, P.resid_only is honoured) or secant (P.Mp holds M_old =
// M(omega_k-1), domega[b] = omega_k - omega_k-1 on the device, P.resid_only is not read: launch_eigpair_resid serves).
// One text, two kernels: what differs is the product pass, the division by domega and one term of the finite check.
template <bool SECANT>
__device__ __forceinline__ void eigpair_step_body(const EigArgs& P, const double2* domega) {
    extern __shared__ double2 sm[];
    __shared__ double s_red[3 * NW];
    const int n = P.n;
    const int b = pick_item(P.items);
    if (P.active && P.active[b] == 0) return;  // uniform
    const bool resid_only = !SECANT && P.resid_only;
    const int tid = threadIdx.x;
    double2* out = P.vecs + (size_t)b * n;
    if (!resid_only && P.lu_info && P.lu_info[b] != 0) {  // no factorisation (exactly singular column / time-out)
        const double qnan = __builtin_nan("");
        nan_out(out, n);
        if (tid == 0) P.info[b] = P.lu_info[b], P.tau[b] = make_double2(qnan, qnan), P.resid[b] = qnan;
        return;
    }
    const Frame fr(sm, n, P.A + (size_t)b * n * n);
    const Factors& F = fr.F;
    double2* v = fr.x0;  // the iterate
    double2* w = fr.x1;  // plain: M v, then M' v; secant: (M - M_old) v, then that over domega
    double2* t = fr.x2;  // the solves' work vector: u (secant: M v until the residual is taken)
    double one[1], tot[2];
    if (!resid_only) fr.load_rowmap(P.maps + (size_t)b * P.nblk * n, P.nb);
    if (P.first && !resid_only) {
        // v_0 = M^-1 s / |M^-1 s|: the start vector of k_null_iterate
        for (int i = tid; i < n; i += NT) w[i] = start_vector(i);
        __syncthreads();
        solve_plain(F, w, t);
        double s = 0.0;
        for (int i = tid; i < n; i += NT) s += t[i].x * t[i].x + t[i].y * t[i].y;
        const double ws[1] = {wave_sum(s)};
        block_sum(s_red, ws, one);
        const double r = 1.0 / sqrt(one[0]);
        for (int i = tid; i < n; i += NT) v[i] = make_double2(t[i].x * r, t[i].y * r);
    } else {
        for (int i = tid; i < n; i += NT) v[i] = out[i];
    }
    __syncthreads();
    // ---- the residual of (omega_k, v_k) on the un-factored M; secant: the same pass over M and M_old also gives
    // (M - M_old) v ----
    const double2* Mb = P.M + (size_t)b * n * n;
    const double2* mv = SECANT ? t : w;
    const double fro = SECANT ? matvec_diff(n, Mb, P.Mp + (size_t)b * n * n, v, t, w) : matvec<true>(n, Mb, v, w);
    __syncthreads();
    double y2 = 0.0;
    for (int i = tid; i < n; i += NT) y2 += mv[i].x * mv[i].x + mv[i].y * mv[i].y;
    const double wr[2] = {wave_sum(y2), wave_sum(fro)};
    block_sum(s_red, wr, tot);
    if (tid == 0) P.resid[b] = sqrt(tot[0]) / sqrt(tot[1]);
    if (resid_only) return;  // uniform
    // ---- the step: w = M' v (secant: (M - M_old) v / domega), u = M^-1 w, tau = v^H u, v <- u / |u| ----
    cd inv = mk(0.0, 0.0);
    if (SECANT) {
        // (a zero or non-finite domega has no reciprocal: EMME_ENUMERIC below)
        const double2 dw = domega[b];
        const double dw2 = dw.x * dw.x + dw.y * dw.y;
        inv = mk(dw.x / dw2, -dw.y / dw2);
        for (int i = tid; i < n; i += NT) w[i] = d2(mk(w[i].x, w[i].y) * inv);
    } else {
        (void)matvec<false>(n, P.Mp + (size_t)b * n * n, v, w);
    }
    __syncthreads();
    solve_plain(F, w, t);  // (its barriers stand between the sum above and the one below)
    cd tau = mk(0.0, 0.0);
    double u2 = 0.0;
    for (int i = tid; i < n; i += NT) {
        const cd u = mk(t[i].x, t[i].y);
        tau = tau + conj_(mk(v[i].x, v[i].y)) * u;
        u2 += u.x * u.x + u.y * u.y;
    }
    const double wt[3] = {wave_sum(tau.x), wave_sum(tau.y), wave_sum(u2)};
    double tt[3];
    block_sum(s_red, wt, tt);
    const double tx = tt[0], ty = tt[1], r = 1.0 / sqrt(tt[2]);
    bool finite = isfinite(inv.x) && isfinite(inv.y) && isfinite(tx) && isfinite(ty) && isfinite(r);
    for (int i = tid; i < n; i += NT) {
        const double2 o = make_double2(t[i].x * r, t[i].y * r);
        out[i] = o;
        finite = finite && isfinite(o.x) && isfinite(o.y);
    }
    const int bad = __syncthreads_or(!finite);
    if (tid == 0) P.tau[b] = make_double2(tx, ty), P.info[b] = bad ? -6 /* EMME_ENUMERIC */ : 0;
}

__global__ __launch_bounds__(NT) void k_eigpair_step(EigArgs P) { eigpair_step_body<false>(P, nullptr); }
__global__ __launch_bounds__(NT) void k_eigpair_secant_step(EigArgs P, const double2* domega) { eigpair_step_body<true>(P, domega); }

// what the three launchers hand a kernel (resid_only: launch_eigpair_resid, which has no factors, flags or outputs
// beside resid)
EigArgs eig_args(int n, const double* M, const double* Mp, const double* A_lu, const int* rowmaps, int nb, const int* items,
                 const int* active, const int* lu_info, double* vecs, double* tau, double* resid, int* info, bool first,
                 bool resid_only) {
    EigArgs P{};
    P.n = n, P.nb = nb, P.nblk = (n + nb - 1) / nb;
    P.M = (const double2*)M, P.Mp = (const double2*)Mp, P.A = (const double2*)A_lu;
    P.maps = rowmaps, P.items = items, P.active = active, P.lu_info = lu_info;
    P.vecs = (double2*)vecs, P.tau = (double2*)tau, P.resid = resid, P.info = info;
    P.first = first ? 1 : 0, P.resid_only = resid_only ? 1 : 0;
    return P;
}

}  // namespace

hipError_t launch_eigpair_secant_step(int n, const double* M, const double* Mold, const double* domega, const double* A_lu,
                                      const int* rowmaps, int nb, const int* items, int nitems, const int* active,
                                      const int* lu_info, double* vecs, double* tau, double* resid, int* info, bool first,
                                      hipStream_t stream) {
    if (nitems < 1) return hipSuccess;
    return launch_dyn_lds(k_eigpair_secant_step, nitems, frame_lds(n), stream,
                          eig_args(n, M, Mold, A_lu, rowmaps, nb, items, active, lu_info, vecs, tau, resid, info, first, false),
                          (const double2*)domega);
}

hipError_t launch_eigpair_step(int n, const double* M, const double* Mp, const double* A_lu, const int* rowmaps, int nb,
                               const int* items, int nitems, const int* active, const int* lu_info, double* vecs,
                               double* tau, double* resid, int* info, bool first, hipStream_t stream) {
    if (nitems < 1) return hipSuccess;
    return launch_dyn_lds(k_eigpair_step, nitems, frame_lds(n), stream,
                          eig_args(n, M, Mp, A_lu, rowmaps, nb, items, active, lu_info, vecs, tau, resid, info, first, false));
}

hipError_t launch_eigpair_resid(int n, const double* M, const int* items, int nitems, const double* vecs, double* resid,
                                hipStream_t stream) {
    if (nitems < 1) return hipSuccess;
    return launch_dyn_lds(k_eigpair_step, nitems, frame_lds(n), stream,
                          eig_args(n, M, nullptr, nullptr, nullptr, n, items, nullptr, nullptr, const_cast<double*>(vecs), nullptr,
                                   resid, nullptr, false, true));
}

}  // namespace emme
