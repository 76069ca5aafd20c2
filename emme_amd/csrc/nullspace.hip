// nullspace.hip -- EigenSolver::nullSpace (reference include/solver.h:58-112, called once per solve by
// src/main.cpp:70-75) on the device, batched over the roots of a search.
//
// The reference takes the last row of V^H of a full SVD (LAPACK zgesdd), i.e. the right singular vector of
// the smallest singular value of M(omega_root).  Here: inverse iteration on M^H M, applied as
// v <- M^-1 (M^-H v) through ONE partial-pivot LU of M itself (M^H M is never formed, so the factorisation
// sees cond(M), not its square); the convergence factor per sweep is (s_n / s_n-1)^2 -- <= 1e-8 at a
// converged root -- and the sweeps stop when the direction has stopped moving.  Same vector as the SVD's up
// to the arbitrary complex phase LAPACK would return.  No symmetry of M is assumed: M^-H goes through the
// transposed triangular solves U^H, L^H of the same factors.
//
// The factorisation is the Newton step's (linstep_blocked.hip): k_lu_inplace for orders whose panel fits one
// workgroup's LDS, the chunked multi-workgroup kernel above that; both leave P M = L U in place with the row
// order in panel snapshots.  k_null_iterate then runs the four triangular solves of a sweep with one
// 1024-thread workgroup per matrix: the non-transposed ones in dot form (a wave per row of a 16-row block,
// rows are contiguous), the transposed ones in axpy form (a thread per column, the 16 rows of the block are
// contiguous across threads), the 16 x 16 triangles by one wave with the block's entries in registers.  The solves
// and the workgroup's frame (LDS layout, row map, start vector, sums) live in tri_solve.hpp, which the eigenpair step
// kernels (eigpair.hip) and the folded steps' solve kernels (linstep_fold.hip, eigpair_fold.hip) read too.
#include <hip/hip_runtime.h>

#include <cmath>

#include "emme_device.hpp"
#include "launch.hpp"
#include "tri_solve.hpp"

namespace emme {

namespace {

using namespace trisolve;  // the frame of a solve workgroup and the triangular solves (tri_solve.hpp)

struct NullArgs {
    int n, nb, nblk;       // order; rows per panel snapshot and snapshots per matrix of the factorisation
    const double2* A;      // [nbatch][n][n]  P M = L U in place
    const int* maps;       // [nbatch][nblk][n] row-order snapshots
    const int* items;      // batch indices of this launch (null: 0 .. grid-1)
    const int* lu_info;    // per batch item: 0, or the column at which the factorisation stopped
    double2* vecs;         // [nbatch][n]
    int* info;             // [nbatch]
    int max_sweeps;
};

__global__ __launch_bounds__(NT) void k_null_iterate(NullArgs P) {
    extern __shared__ double2 sm[];
    __shared__ double s_red[2 * NW];
    const int n = P.n;
    const int b = pick_item(P.items);
    const int tid = threadIdx.x;
    double2* out = P.vecs + (size_t)b * n;
    if (P.lu_info && P.lu_info[b] != 0) {  // no factorisation (exactly singular column / time-out): no vector
        nan_out(out, n);
        if (tid == 0) P.info[b] = P.lu_info[b];
        return;
    }
    const Frame fr(sm, n, P.A + (size_t)b * n * n);
    const Factors& F = fr.F;
    double2* v = fr.x0;  // the iterate / right-hand side
    double2* t = fr.x1;  // work vector
    double2* o = fr.x2;  // the direction before the sweep
    const int* rowmap = fr.rowmap;
    fr.load_rowmap(P.maps + (size_t)b * P.nblk * n, P.nb);
    for (int i = tid; i < n; i += NT) v[i] = start_vector(i);
    __syncthreads();

    // v <- v / |v|; ends on a barrier (which is also the one block_sum's next call is owed)
    auto normalise = [&]() {
        double s = 0.0;
        for (int i = tid; i < n; i += NT) s += v[i].x * v[i].x + v[i].y * v[i].y;
        const double w[1] = {wave_sum(s)};
        double tot[1];
        block_sum(s_red, w, tot);
        const double r = 1.0 / sqrt(tot[0]);
        for (int i = tid; i < n; i += NT) v[i] = make_double2(v[i].x * r, v[i].y * r);
        __syncthreads();
    };
    // z = M^-H b:  U^H w = b, L^H z' = w, z = P^T z'
    auto solve_h = [&]() {
        solve_tri<true, false>(F, v);
        solve_tri<true, true>(F, v);
        for (int r = tid; r < n; r += NT) t[rowmap[r]] = v[r];
        __syncthreads();
        for (int r = tid; r < n; r += NT) v[r] = t[r];
        __syncthreads();
    };
    // y = M^-1 b:  c = P b, L c' = c, U y = c'
    auto solve_n = [&]() {
        solve_plain(F, v, t);
        for (int r = tid; r < n; r += NT) v[r] = t[r];
        __syncthreads();
    };

    normalise();
    for (int it = 0; it < P.max_sweeps; ++it) {
        for (int i = tid; i < n; i += NT) o[i] = v[i];  // (each thread reads back only what it wrote)
        solve_h();
        normalise();
        solve_n();
        normalise();
        // |<old, v>| -> 1 when the direction has stopped moving
        cd ov = mk(0.0, 0.0);
        for (int i = tid; i < n; i += NT) ov = ov + conj_(mk(o[i].x, o[i].y)) * mk(v[i].x, v[i].y);
        const double w[2] = {wave_sum(ov.x), wave_sum(ov.y)};
        double tot[2];
        block_sum(s_red, w, tot);  // (the next one stands behind the barriers of solve_h)
        const double overlap = sqrt(tot[0] * tot[0] + tot[1] * tot[1]);
        if (it >= 1 && !(fabs(1.0 - overlap) > 1e-14)) break;  // uniform (a NaN ends the loop too)
    }
    bool finite = true;
    for (int i = tid; i < n; i += NT) {
        out[i] = v[i];
        finite = finite && isfinite(v[i].x) && isfinite(v[i].y);
    }
    const int bad = __syncthreads_or(!finite);
    if (tid == 0) P.info[b] = bad ? -6 /* EMME_ENUMERIC */ : 0;
}

// Orders above the blocked factorisations' reach (n > 1024): plain right-looking partial-pivot LU in place, one
// workgroup per matrix, the pivot row staged in LDS, rows never moved (row map in LDS, written out as ONE
// snapshot: nb = n).  O(n) barriers per column block of one -- slow, and only there so that every order the
// Newton step accepts has a device nullSpace too.
__global__ __launch_bounds__(NT) void k_lu_unblocked_inplace(int n, double2* A, int* maps, int* info_out, const int* items) {
    extern __shared__ double2 sm[];
    __shared__ double s_val[NW];
    __shared__ int s_idx[NW];
    __shared__ int s_piv, s_info;
    double2* prow = sm;
    int* rowmap = reinterpret_cast<int*>(sm + n);
    const int b = items ? items[blockIdx.x] : blockIdx.x;
    double2* a = A + (size_t)b * n * n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int r = tid; r < n; r += NT) rowmap[r] = r;
    if (tid == 0) s_info = 0;
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        double best = -1.0;
        int brow = n;
        for (int r = k + tid; r < n; r += NT) {
            const double v = norm2(ld2(&a[(size_t)rowmap[r] * n + k]));
            if (v > best) best = v, brow = r;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ov = __shfl_xor(best, off);
            const int oi = __shfl_xor(brow, off);
            if (ov > best || (ov == best && oi < brow)) best = ov, brow = oi;
        }
        if (lane == 0) s_val[wave] = best, s_idx[wave] = brow;
        __syncthreads();
        if (tid == 0) {
            double bv = s_val[0];
            int bi = s_idx[0];
            for (int w = 1; w < NW; ++w)
                if (s_val[w] > bv || (s_val[w] == bv && s_idx[w] < bi)) bv = s_val[w], bi = s_idx[w];
            if (!(bv > 0.0) || !isfinite(bv)) {
                if (s_info == 0) s_info = k + 1;
                bi = -1;
            } else {
                const int tmp = rowmap[k];
                rowmap[k] = rowmap[bi], rowmap[bi] = tmp;
            }
            s_piv = bi;
        }
        __syncthreads();
        if (s_piv < 0) break;  // uniform
        const double2* pr = a + (size_t)rowmap[k] * n;
        for (int c = k + tid; c < n; c += NT) prow[c] = pr[c];
        __syncthreads();
        const cd rp = rcp(mk(prow[k].x, prow[k].y));
        for (int r = k + 1 + wave; r < n; r += NW) {
            double2* ar = a + (size_t)rowmap[r] * n;
            const cd f = ld2(&ar[k]) * rp;
            if (lane == 0) ar[k] = make_double2(f.x, f.y);
            for (int c = k + 1 + lane; c < n; c += 64) {
                const cd u = ld2(&ar[c]) - f * mk(prow[c].x, prow[c].y);
                ar[c] = make_double2(u.x, u.y);
            }
        }
        __syncthreads();
    }
    __syncthreads();
    for (int r = tid; r < n; r += NT) maps[(size_t)b * n + r] = rowmap[r];
    if (tid == 0) info_out[b] = s_info;
}

}  // namespace

size_t null_iterate_lds(int n) { return frame_lds(n); }

hipError_t launch_lu_unblocked_inplace(int n, int nbatch, double* A, int* maps, int* info, hipStream_t stream,
                                       const int* items, int nitems) {
    const size_t lds = (size_t)n * sizeof(double2) + (size_t)n * sizeof(int);
    return launch_dyn_lds(k_lu_unblocked_inplace, items ? nitems : nbatch, lds, stream, n, (double2*)A, maps, info, items);
}

hipError_t launch_null_iterate(int n, const double* A_lu, const int* rowmaps, int nb, const int* items, int nitems,
                               const int* lu_info, double* vecs, int* info, int max_sweeps, hipStream_t stream) {
    NullArgs P;
    P.n = n, P.nb = nb, P.nblk = (n + nb - 1) / nb;
    P.A = (const double2*)A_lu;
    P.maps = rowmaps;
    P.items = items;
    P.lu_info = lu_info;
    P.vecs = (double2*)vecs;
    P.info = info;
    P.max_sweeps = max_sweeps;
    return launch_dyn_lds(k_null_iterate, nitems, null_iterate_lds(n), stream, P);
}

}  // namespace emme
