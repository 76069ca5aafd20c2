// eigpair.hip -- one step of Newton's method on the eigenpair (omega, v) of M(omega) v = 0: nonlinear
// inverse iteration.  With |v| = 1 the bordered system M(omega) v = 0, v_k^H v = 1 gives
//     u = M(omega_k)^-1 M'(omega_k) v_k,   omega_k+1 = omega_k - 1 / (v_k^H u),   v_k+1 = u / |u|,
// so a step is ONE factorisation without right-hand sides (k_lu_inplace and its kin, linstep_blocked.hip /
// nullspace.hip), one matrix-vector product and one pair of triangular solves -- against the LU plus n right-hand
// sides of the trace form -- and the vector and the residual |M v| / |M|_F come with the root.
//
// k_eigpair_step: one 512-thread workgroup per live matrix.  The products M v and M' v go a wave per row, rows dealt
// to the waves in a fixed order (row r to wave r mod 8), every sum in a fixed order and nothing atomic: two runs are
// bit-identical.  The triangular solves are k_null_iterate's (tri_solve.hpp), on the same LDS layout.
//
// k_eigpair_secant_step: the same step for a search that holds two consecutive plain fills M = M(omega_k), M_old =
// M(omega_k-1) and no derivative: M' v is replaced by (M - M_old) v / (omega_k - omega_k-1).  ONE pass over the rows of
// both matrices takes the difference entry by entry (two separately rounded products would lose n eps / |domega / omega|
// near convergence) and gives M v, (M - M_old) v and |M|_F^2 together: no matrix M' is formed, written or read, and
// there is no separate residual pass.  A sibling kernel and not a template reading of k_eigpair_step, whose code object
// stays what it was.
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

__global__ __launch_bounds__(NT) void k_eigpair_step(EigArgs P) {
    extern __shared__ double2 sm[];
    __shared__ double s_red[2 * NW];
    const int n = P.n;
    double2* v = sm;                  // the iterate
    double2* w = sm + n;              // M v, then M' v
    double2* t = sm + 2 * (size_t)n;  // the solves' work vector: u
    int* rowmap = reinterpret_cast<int*>(sm + 3 * (size_t)n);
    const int b = P.items ? P.items[blockIdx.x] : blockIdx.x;
    if (P.active && P.active[b] == 0) return;  // uniform
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double2* out = P.vecs + (size_t)b * n;
    const double qnan = __builtin_nan("");
    if (!P.resid_only && P.lu_info && P.lu_info[b] != 0) {  // no factorisation (exactly singular column / time-out)
        for (int i = tid; i < n; i += NT) out[i] = make_double2(qnan, qnan);
        if (tid == 0) P.info[b] = P.lu_info[b], P.tau[b] = make_double2(qnan, qnan), P.resid[b] = qnan;
        return;
    }
    // (total of a and of b over the workgroup, in wave order, to every thread)
    auto block_sum2 = [&](double a, double bb, double& ta, double& tb) {
        a = wave_sum(a), bb = wave_sum(bb);
        if (lane == 0) s_red[wave] = a, s_red[NW + wave] = bb;
        __syncthreads();
        ta = 0.0, tb = 0.0;
#pragma unroll
        for (int k = 0; k < NW; ++k) ta += s_red[k], tb += s_red[NW + k];
        __syncthreads();
    };
    Factors F;
    F.n = n, F.a = P.A + (size_t)b * n * n, F.rowmap = rowmap;
    F.bA = sm + 3 * (size_t)n + rowmap_slots(n);
    F.bD = F.bA + 2 * TB * (TB + 1);
    if (!P.resid_only) {
        const int* maps = P.maps + (size_t)b * P.nblk * n;
        for (int x = tid; x < n; x += NT) rowmap[x] = maps[(size_t)(x / P.nb) * n + x];
    }
    if (P.first && !P.resid_only) {
        // v_0 = M^-1 s / |M^-1 s|: the start vector of k_null_iterate
        for (int i = tid; i < n; i += NT) w[i] = make_double2(1.0 + 0.37 * sin(1.0 + i), 0.21 * cos(2.0 * i));
        __syncthreads();
        solve_plain(F, w, t);
        double s = 0.0, s0, s1;
        for (int i = tid; i < n; i += NT) s += t[i].x * t[i].x + t[i].y * t[i].y;
        block_sum2(s, 0.0, s0, s1);
        const double r = 1.0 / sqrt(s0);
        for (int i = tid; i < n; i += NT) v[i] = make_double2(t[i].x * r, t[i].y * r);
    } else {
        for (int i = tid; i < n; i += NT) v[i] = out[i];
    }
    __syncthreads();
    // ---- the residual of (omega_k, v_k) on the un-factored M ----
    const double2* Mb = P.M + (size_t)b * n * n;
    const double fro = matvec<true>(n, Mb, v, w);
    __syncthreads();
    double y2 = 0.0, ty2, tfro;
    for (int i = tid; i < n; i += NT) y2 += w[i].x * w[i].x + w[i].y * w[i].y;
    block_sum2(y2, fro, ty2, tfro);
    if (tid == 0) P.resid[b] = sqrt(ty2) / sqrt(tfro);
    if (P.resid_only) return;  // uniform
    // ---- the step: w = M' v, u = M^-1 w, tau = v^H u, v <- u / |u| ----
    (void)matvec<false>(n, P.Mp + (size_t)b * n * n, v, w);
    __syncthreads();
    solve_plain(F, w, t);
    cd tau = mk(0.0, 0.0);
    double u2 = 0.0;
    for (int i = tid; i < n; i += NT) {
        const cd u = mk(t[i].x, t[i].y);
        tau = tau + conj_(mk(v[i].x, v[i].y)) * u;
        u2 += u.x * u.x + u.y * u.y;
    }
    double tx, ty, tu2, unused;
    block_sum2(tau.x, tau.y, tx, ty);
    block_sum2(u2, 0.0, tu2, unused);
    const double r = 1.0 / sqrt(tu2);
    bool finite = isfinite(tx) && isfinite(ty) && isfinite(r);
    for (int i = tid; i < n; i += NT) {
        const double2 o = make_double2(t[i].x * r, t[i].y * r);
        out[i] = o;
        finite = finite && isfinite(o.x) && isfinite(o.y);
    }
    const int bad = __syncthreads_or(!finite);
    if (tid == 0) P.tau[b] = make_double2(tx, ty), P.info[b] = bad ? -6 /* EMME_ENUMERIC */ : 0;
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

// The secant reading of the step.  P.Mp holds M_old = M(omega_k-1), domega[b] = omega_k - omega_k-1 (device); P.first,
// items, active, lu_info and the outputs as in k_eigpair_step, P.resid_only is not read (launch_eigpair_resid serves).
__global__ __launch_bounds__(NT) void k_eigpair_secant_step(EigArgs P, const double2* domega) {
    extern __shared__ double2 sm[];
    __shared__ double s_red[2 * NW];
    const int n = P.n;
    double2* v = sm;                  // the iterate
    double2* w = sm + n;              // (M - M_old) v, then that over domega
    double2* t = sm + 2 * (size_t)n;  // M v until the residual is taken, then the solves' work vector: u
    int* rowmap = reinterpret_cast<int*>(sm + 3 * (size_t)n);
    const int b = P.items ? P.items[blockIdx.x] : blockIdx.x;
    if (P.active && P.active[b] == 0) return;  // uniform
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double2* out = P.vecs + (size_t)b * n;
    const double qnan = __builtin_nan("");
    if (P.lu_info && P.lu_info[b] != 0) {  // no factorisation (exactly singular column / time-out)
        for (int i = tid; i < n; i += NT) out[i] = make_double2(qnan, qnan);
        if (tid == 0) P.info[b] = P.lu_info[b], P.tau[b] = make_double2(qnan, qnan), P.resid[b] = qnan;
        return;
    }
    // (total of a and of b over the workgroup, in wave order, to every thread)
    auto block_sum2 = [&](double a, double bb, double& ta, double& tb) {
        a = wave_sum(a), bb = wave_sum(bb);
        if (lane == 0) s_red[wave] = a, s_red[NW + wave] = bb;
        __syncthreads();
        ta = 0.0, tb = 0.0;
#pragma unroll
        for (int k = 0; k < NW; ++k) ta += s_red[k], tb += s_red[NW + k];
        __syncthreads();
    };
    Factors F;
    F.n = n, F.a = P.A + (size_t)b * n * n, F.rowmap = rowmap;
    F.bA = sm + 3 * (size_t)n + rowmap_slots(n);
    F.bD = F.bA + 2 * TB * (TB + 1);
    const int* maps = P.maps + (size_t)b * P.nblk * n;
    for (int x = tid; x < n; x += NT) rowmap[x] = maps[(size_t)(x / P.nb) * n + x];
    if (P.first) {
        // v_0 = M^-1 s / |M^-1 s|: the start vector of k_null_iterate
        for (int i = tid; i < n; i += NT) w[i] = make_double2(1.0 + 0.37 * sin(1.0 + i), 0.21 * cos(2.0 * i));
        __syncthreads();
        solve_plain(F, w, t);
        double s = 0.0, s0, s1;
        for (int i = tid; i < n; i += NT) s += t[i].x * t[i].x + t[i].y * t[i].y;
        block_sum2(s, 0.0, s0, s1);
        const double r = 1.0 / sqrt(s0);
        for (int i = tid; i < n; i += NT) v[i] = make_double2(t[i].x * r, t[i].y * r);
    } else {
        for (int i = tid; i < n; i += NT) v[i] = out[i];
    }
    __syncthreads();
    // ---- one pass over M and M_old: M v (the residual of (omega_k, v_k)), (M - M_old) v and |M|_F^2 ----
    const double fro = matvec_diff(n, P.M + (size_t)b * n * n, P.Mp + (size_t)b * n * n, v, t, w);
    __syncthreads();
    double y2 = 0.0, ty2, tfro;
    for (int i = tid; i < n; i += NT) y2 += t[i].x * t[i].x + t[i].y * t[i].y;
    block_sum2(y2, fro, ty2, tfro);
    if (tid == 0) P.resid[b] = sqrt(ty2) / sqrt(tfro);
    // ---- the step: w = (M - M_old) v / domega, u = M^-1 w, tau = v^H u, v <- u / |u| ----
    // (a zero or non-finite domega has no reciprocal: EMME_ENUMERIC below)
    const double2 dw = domega[b];
    const double dw2 = dw.x * dw.x + dw.y * dw.y;
    const cd inv = mk(dw.x / dw2, -dw.y / dw2);
    for (int i = tid; i < n; i += NT) {
        const cd q = mk(w[i].x, w[i].y) * inv;
        w[i] = make_double2(q.x, q.y);
    }
    __syncthreads();
    solve_plain(F, w, t);
    cd tau = mk(0.0, 0.0);
    double u2 = 0.0;
    for (int i = tid; i < n; i += NT) {
        const cd u = mk(t[i].x, t[i].y);
        tau = tau + conj_(mk(v[i].x, v[i].y)) * u;
        u2 += u.x * u.x + u.y * u.y;
    }
    double tx, ty, tu2, unused;
    block_sum2(tau.x, tau.y, tx, ty);
    block_sum2(u2, 0.0, tu2, unused);
    const double r = 1.0 / sqrt(tu2);
    bool finite = isfinite(inv.x) && isfinite(inv.y) && isfinite(tx) && isfinite(ty) && isfinite(r);
    for (int i = tid; i < n; i += NT) {
        const double2 o = make_double2(t[i].x * r, t[i].y * r);
        out[i] = o;
        finite = finite && isfinite(o.x) && isfinite(o.y);
    }
    const int bad = __syncthreads_or(!finite);
    if (tid == 0) P.tau[b] = make_double2(tx, ty), P.info[b] = bad ? -6 /* EMME_ENUMERIC */ : 0;
}

// domega null: k_eigpair_step, else k_eigpair_secant_step
hipError_t launch(const EigArgs& P, int nitems, hipStream_t stream, const double2* domega = nullptr) {
    const size_t lds = null_iterate_lds(P.n);
    if (lds > 150 * 1024) return hipErrorNotSupported;
    if (lds > 48 * 1024) {  // (beyond the default dynamic-LDS limit only)
        const void* kernel = domega ? (const void*)k_eigpair_secant_step : (const void*)k_eigpair_step;
        const hipError_t ea = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ea != hipSuccess) return ea;
    }
    if (domega)
        hipLaunchKernelGGL(k_eigpair_secant_step, dim3(nitems), dim3(NT), lds, stream, P, domega);
    else
        hipLaunchKernelGGL(k_eigpair_step, dim3(nitems), dim3(NT), lds, stream, P);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_eigpair_secant_step(int n, const double* M, const double* Mold, const double* domega, const double* A_lu,
                                      const int* rowmaps, int nb, const int* items, int nitems, const int* active,
                                      const int* lu_info, double* vecs, double* tau, double* resid, int* info, bool first,
                                      hipStream_t stream) {
    if (nitems < 1) return hipSuccess;
    EigArgs P{};
    P.n = n, P.nb = nb, P.nblk = (n + nb - 1) / nb;
    P.M = (const double2*)M, P.Mp = (const double2*)Mold, P.A = (const double2*)A_lu;
    P.maps = rowmaps, P.items = items, P.active = active, P.lu_info = lu_info;
    P.vecs = (double2*)vecs, P.tau = (double2*)tau, P.resid = resid, P.info = info;
    P.first = first ? 1 : 0, P.resid_only = 0;
    return launch(P, nitems, stream, (const double2*)domega);
}

hipError_t launch_eigpair_step(int n, const double* M, const double* Mp, const double* A_lu, const int* rowmaps, int nb,
                               const int* items, int nitems, const int* active, const int* lu_info, double* vecs,
                               double* tau, double* resid, int* info, bool first, hipStream_t stream) {
    if (nitems < 1) return hipSuccess;
    EigArgs P{};
    P.n = n, P.nb = nb, P.nblk = (n + nb - 1) / nb;
    P.M = (const double2*)M, P.Mp = (const double2*)Mp, P.A = (const double2*)A_lu;
    P.maps = rowmaps, P.items = items, P.active = active, P.lu_info = lu_info;
    P.vecs = (double2*)vecs, P.tau = (double2*)tau, P.resid = resid, P.info = info;
    P.first = first ? 1 : 0, P.resid_only = 0;
    return launch(P, nitems, stream);
}

hipError_t launch_eigpair_resid(int n, const double* M, const int* items, int nitems, const double* vecs, double* resid,
                                hipStream_t stream) {
    if (nitems < 1) return hipSuccess;
    EigArgs P{};
    P.n = n, P.nb = n, P.nblk = 1;
    P.M = (const double2*)M, P.items = items;
    P.vecs = (double2*)const_cast<double*>(vecs), P.resid = resid;
    P.resid_only = 1;
    return launch(P, nitems, stream);
}

}  // namespace emme
