// tri_solve.hpp -- the frame of a workgroup that solves on an in-place partial-pivot LU (P M = L U, rows never moved):
// k_null_iterate (nullspace.hip), the two step kernels of eigpair.hip, k_fold_solve (linstep_fold.hip) and
// k_eigpair_fold_half (eigpair_fold.hip).  Device code, one 512-thread workgroup per matrix.  What the five share stands
// here once: the LDS layout and its size (Frame, frame_lds), the item pick, the row-map load, the start vector, the NaN
// fill, the workgroup sum (block_sum), the host launch with dynamic LDS (launch_dyn_lds), and below them the pipelined
// one-vector triangular solves.
//
// One right-hand side is a chain of n dependent steps whatever one does; what can be taken OFF that chain is
// everything else.  Per stage (one block of 16 unknowns) the workgroup splits into
//   wave 0   the chain: rhs of the block's 16 equations (already updated with all blocks but the previous one),
//            minus the previous block's coupling (16 x 16, the previous solution still in its registers, read with
//            v_readlane), then the 16 x 16 triangle -- 32 readlane steps, operands from LDS;
//   wave 1   stages the NEXT stage's two 16 x 16 coefficient blocks from the factors (global memory) into LDS;
//   others   apply the PREVIOUS block's solution to all equations beyond the next block;
// and ONE barrier ends the stage.  (The first version had wave 0 wait for the other waves' dots and the other
// waves wait for wave 0's triangle, two barriers and a global-memory latency per block on the chain: 0.3 ms per
// sweep at n = 256, 19 ms for the 128 matrices of the headline search, eight of which are not singular and take
// all 60 sweeps.)
#pragma once
#include <hip/hip_runtime.h>

#include "emme_device.hpp"

namespace emme {
namespace trisolve {

constexpr int NT = 512;  // (256 vector registers per thread: the chain wave holds two 16 x 16 coefficient rows)
constexpr int NW = NT / 64;
constexpr int TB = 16;  // rows per block of the triangular solves

__device__ __forceinline__ cd ld2(const double2* p) {
    const double2 v = *p;
    return mk(v.x, v.y);
}
__device__ __forceinline__ double2 d2(cd v) { return make_double2(v.x, v.y); }
__device__ __forceinline__ cd conj_(cd a) { return mk(a.x, -a.y); }
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ cd readlane_c(cd x, int k) {
    const long long bx = __double_as_longlong(x.x), by = __double_as_longlong(x.y);
    const unsigned xl = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)bx, k), xh = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(bx >> 32), k);
    const unsigned yl = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)by, k), yh = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(by >> 32), k);
    return mk(__longlong_as_double((long long)(((unsigned long long)xh << 32) | xl)), __longlong_as_double((long long)(((unsigned long long)yh << 32) | yl)));
}

// bytes of LDS behind the three vectors that the row map takes (rounded to whole double2)
__host__ __device__ constexpr size_t rowmap_slots(int n) { return ((size_t)n * sizeof(int) + 15) / 16; }

// What a solve reads: the factors of one matrix, its row order (LDS: logical row x = physical row rowmap[x]) and the
// staging blocks.  coef(i, j) = coefficient of unknown j in equation i:  M(i, j) = a[rowmap[i] n + j] of the factor, or
// conj M(j, i) for the transposed systems; LOWER = unit diagonal (L, L^H), else divide by coef(i, i) (U, U^H).
struct Factors {
    int n;
    const double2* a;   // [n][n] P M = L U in place
    const int* rowmap;  // LDS, n ints
    double2* bA;        // LDS [2][TB][TB + 1] coupling with the previous block
    double2* bD;        // LDS [2][TB][TB + 1] the block's own triangle
};

// ---- the frame ------------------------------------------------------------------------------------------------------
// The dynamic LDS of a solve workgroup on a matrix of order n: three vectors of n complex, the row map, the four staged
// 16 x 16 coefficient blocks.  frame_lds(n) is its size in bytes (null_iterate_lds(n) of launch.hpp, for host code).
__host__ __device__ constexpr size_t frame_lds(int n) {
    return (3 * (size_t)n + rowmap_slots(n) + 4 * TB * (TB + 1)) * sizeof(double2);
}
struct Frame {
    double2 *x0, *x1, *x2;  // the three vectors
    int* rowmap;
    Factors F;  // on `a`, this row map and the staging blocks
    __device__ __forceinline__ Frame(double2* sm, int n, const double2* a) {
        x0 = sm, x1 = sm + n, x2 = sm + 2 * (size_t)n;
        rowmap = reinterpret_cast<int*>(sm + 3 * (size_t)n);
        F.n = n, F.a = a, F.rowmap = rowmap;
        F.bA = sm + 3 * (size_t)n + rowmap_slots(n);
        F.bD = F.bA + 2 * TB * (TB + 1);
    }
    // the row order of a finished factorisation from its panel snapshots (maps_of_item: [ceil(n / nb)][n], nb rows per
    // snapshot): logical row x is where the snapshot of its own panel has it.  No barrier.  (Runs once, at most four
    // trips: not worth the unrolled copies of the integer division.)
    __device__ __forceinline__ void load_rowmap(const int* maps_of_item, int nb) const {
#pragma unroll 1
        for (int x = threadIdx.x; x < F.n; x += NT) rowmap[x] = maps_of_item[(size_t)(x / nb) * F.n + x];
    }
};

// the batch item of this workgroup: the launch's list, or the workgroup's own index
__device__ __forceinline__ int pick_item(const int* items) { return items ? items[blockIdx.x] : blockIdx.x; }
// s of include/emme_hip.h (the start vector of the host version, host_driver.cpp): no symmetry that a null vector of M
// could be orthogonal to
__device__ __forceinline__ double2 start_vector(int i) { return make_double2(1.0 + 0.37 * sin(1.0 + i), 0.21 * cos(2.0 * i)); }
// out[0 .. count) = NaN: what an item without a factorisation leaves behind
__device__ __forceinline__ void nan_out(double2* out, int count) {
    const double qnan = __builtin_nan("");
    for (int i = threadIdx.x; i < count; i += NT) out[i] = make_double2(qnan, qnan);
}

// t[q] = the total of v[q] over the waves of the workgroup, q < K, added in wave order, to every thread.  v: this
// wave's numbers (lane 0's are taken: the caller has summed over the lanes, wave_sum).  s_red: K * NW doubles of LDS.
// Barriers: ONE, between the waves' writes and everybody's reads.  Before the call the caller owes s_red a barrier that
// every thread has passed since the previous block_sum on it returned (any __syncthreads(), a solve's included); after
// it the totals are in registers and no barrier has been passed since the reads -- LDS written before the call is
// visible to every thread, what a thread writes after it is not until the caller's next barrier.
template <int K>
__device__ __forceinline__ void block_sum(double* s_red, const double (&v)[K], double (&t)[K]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int q = 0; q < K; ++q) s_red[q * NW + wave] = v[q];
    __syncthreads();
    for (int q = 0; q < K; ++q) {
        t[q] = 0.0;
        for (int k = 0; k < NW; ++k) t[q] += s_red[q * NW + k];
    }
}

// Host: launch `kernel` on `grid` workgroups of NT threads with `lds` bytes of dynamic LDS -- not above 150 KiB
// (hipErrorNotSupported), the attribute set beyond the default limit of 48 KiB only.
template <class... Params, class... Args>
hipError_t launch_dyn_lds(void (*kernel)(Params...), int grid, size_t lds, hipStream_t stream, Args... args) {
    if (lds > 150 * 1024) return hipErrorNotSupported;
    if (lds > 48 * 1024) {
        const hipError_t ea = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ea != hipSuccess) return ea;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), lds, stream, args...);
    return hipGetLastError();
}

// x: right-hand side on entry, solution on exit (LDS, indexed by equation = unknown).  Called by all NT threads; ends
// on a barrier.
template <bool TRANS, bool LOWER>
__device__ __forceinline__ void solve_tri(const Factors& F, double2* x) {
    const int n = F.n;
    const double2* a = F.a;
    const int* rowmap = F.rowmap;
    double2* bA = F.bA;
    double2* bD = F.bD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = (n + TB - 1) / TB;
    constexpr bool FWD = LOWER != TRANS;
    auto blk0 = [&](int s) { return (FWD ? s : B - 1 - s) * TB; };   // first unknown of the block of stage s
    auto blkn = [&](int s) { return min(TB, n - blk0(s)); };
    // stage the coefficient blocks of stage s (equations of block s x unknowns of block s - 1 / of block s)
    auto stage_blocks = [&](int s) {
        const int r1 = blk0(s), n1 = blkn(s);
        const int rp = s > 0 ? blk0(s - 1) : 0, np = s > 0 ? blkn(s - 1) : 0;
        double2* dA = bA + (s & 1) * TB * (TB + 1);
        double2* dD = bD + (s & 1) * TB * (TB + 1);
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int e = it * 64 + lane;
            // (contiguous in memory along the fast index: columns of a row for the plain systems, rows for the transposed)
            const int l = TRANS ? (e & 15) : (e >> 4), kk = TRANS ? (e >> 4) : (e & 15);
            double2 va = make_double2(0.0, 0.0), vd = make_double2(0.0, 0.0);
            if (l < n1 && kk < n1) {
                vd = TRANS ? a[(size_t)rowmap[r1 + kk] * n + r1 + l] : a[(size_t)rowmap[r1 + l] * n + r1 + kk];
                if (TRANS) vd.y = -vd.y;
            }
            if (l < n1 && kk < np) {
                va = TRANS ? a[(size_t)rowmap[rp + kk] * n + r1 + l] : a[(size_t)rowmap[r1 + l] * n + rp + kk];
                if (TRANS) va.y = -va.y;
            }
            dA[l * (TB + 1) + kk] = va, dD[l * (TB + 1) + kk] = vd;
        }
    };
    if (wave == 1) stage_blocks(0);
    __syncthreads();
    cd xprev = mk(0.0, 0.0);  // wave 0: the previous block's solution, unknown kk in lane kk
    for (int s = 0; s < B; ++s) {
        const int r0 = blk0(s), nbk = blkn(s);
        if (wave == 0) {
            const double2* dA = bA + (s & 1) * TB * (TB + 1) + (lane & 15) * (TB + 1);
            const double2* dD = bD + (s & 1) * TB * (TB + 1) + (lane & 15) * (TB + 1);
            const bool on = lane < nbk;
            cd sv = on ? mk(x[r0 + lane].x, x[r0 + lane].y) : mk(0.0, 0.0);
            cd ca[TB], cdg[TB];
#pragma unroll
            for (int kk = 0; kk < TB; ++kk) ca[kk] = mk(dA[kk].x, dA[kk].y), cdg[kk] = mk(dD[kk].x, dD[kk].y);
            if (s > 0) {
#pragma unroll
                for (int kk = 0; kk < TB; ++kk) sv = sv - ca[kk] * readlane_c(xprev, kk);  // (rows beyond the block hold zeros)
            }
#pragma unroll
            for (int q = 0; q < TB; ++q) {
                const int kk = FWD ? q : TB - 1 - q;
                if (kk < nbk) {  // uniform
                    if (!LOWER && lane == kk) sv = sv * rcp(cdg[kk]);
                    const cd xk = readlane_c(sv, kk);
                    if (on && (FWD ? lane > kk : lane < kk)) sv = sv - cdg[kk] * xk;
                }
            }
            if (on) x[r0 + lane] = make_double2(sv.x, sv.y);
            xprev = sv;
        } else if (wave == 1) {
            if (s + 1 < B) stage_blocks(s + 1);
        } else if (s > 0) {
            // apply the previous block's solution (final in x since the last barrier) to the equations beyond this block
            const int rp = blk0(s - 1), np = blkn(s - 1);
            const int lo = FWD ? r0 + nbk : 0, hi = FWD ? n : r0;  // equations [lo, hi)
            if (!TRANS) {
                // 16 contiguous coefficients per equation: four equations per wave and trip, 16-lane sums
                const int kk = lane & 15;
                const cd xk = kk < np ? mk(x[rp + kk].x, x[rp + kk].y) : mk(0.0, 0.0);
                for (int i = lo + (wave - 2) * 4 + (lane >> 4); i < hi; i += (NW - 2) * 4) {
                    const cd c = kk < np ? ld2(&a[(size_t)rowmap[i] * n + rp + kk]) : mk(0.0, 0.0);
                    const cd pr = c * xk;
                    const double sx = row16_sum(pr.x), sy = row16_sum(pr.y);
                    if (kk == 0) x[i] = make_double2(x[i].x - sx, x[i].y - sy);
                }
            } else {
                // coefficients of one unknown are contiguous along the equations: an equation per thread
                for (int i = lo + (wave - 2) * 64 + lane; i < hi; i += (NW - 2) * 64) {
                    cd acc = mk(x[i].x, x[i].y);
#pragma unroll
                    for (int kk = 0; kk < TB; ++kk)
                        if (kk < np) acc = acc - conj_(ld2(&a[(size_t)rowmap[rp + kk] * n + i])) * mk(x[rp + kk].x, x[rp + kk].y);
                    x[i] = make_double2(acc.x, acc.y);
                }
            }
        }
        __syncthreads();
    }
}

// y = M^-1 b:  c = P b, L c' = c, U y = c'.  b in `v`, y in `t` (v is left as it was); ends on a barrier.
__device__ __forceinline__ void solve_plain(const Factors& F, const double2* v, double2* t) {
    const int tid = threadIdx.x;
    for (int r = tid; r < F.n; r += NT) t[r] = v[F.rowmap[r]];
    __syncthreads();
    solve_tri<false, true>(F, t);
    solve_tri<false, false>(F, t);
}

}  // namespace trisolve
}  // namespace emme
