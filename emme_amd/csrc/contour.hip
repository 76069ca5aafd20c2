// contour.hip -- the device half of the contour eigensolver and its two C entry points:
// emme_contour_moments_batch (moments of caller matrices) and emme_find_roots_in_contour (every root inside an
// ellipse: Beyn's method, W.-J. Beyn, Linear Algebra Appl. 436 (2012) 3839-3863, seeded into the Newton search).
//
// The nodes' matrices are factored once by the nullSpace factorisation (lu_factor_batch: P M = L U in place, row
// order in panel snapshots) and kept for the whole call.  Three small kernels read the factors:
//   k_contour_solve    X = M^-1 V for a group of G right-hand sides per workgroup: permute, then forward (L) and
//                      back (U) substitution in blocks of 16 rows -- the rows' coupling to every finished block in dot
//                      form (a wave per row, rows are contiguous), then the block's 16 x 16 triangle with 16 lanes
//                      per column (a row each, the solved unknown broadcast by a shuffle), coefficients in LDS;
//   k_contour_logdet   log det M = sum log u_ii + i pi (parity of the row order), fixed-order reductions;
//   k_contour_moments  A0 = sum_j w_j X_j, A1 = sum_j w_j z_j X_j: a thread per entry, the nodes summed in order
//                      (no atomics: two calls on the same inputs are bit-identical).
// The probes V come from a counter-based hash of (row, column) with a fixed seed (k_contour_probes), so that the
// first L columns do not depend on L and doubling L solves only the new ones.
// Over many (parameter set, contour) items at once: emme_find_roots_in_contours_sets walks the round
// plan of host_contour.cpp (ContourRounds) with one fill over sets, one factorisation, one log-det and one restricted
// solve (k_contour_solve<G, true>: a list of matrices, each with its own column range) per round, the moments per item
// by k_contour_moments_groups; emme_contour_moments_groups is that kernel on caller matrices.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ctx.hpp"
#include "emme_device.hpp"
#include "host_contour.hpp"

namespace emme {

namespace {

constexpr int CT = 256;  // threads of the solve / log-det workgroups
constexpr int CW = CT / 64;
constexpr int TB = 16;   // rows per block of the triangular solves
constexpr int LCAP = 64; // most probes a call uses
constexpr unsigned long long PROBE_SEED = 0x454D4D45ull;

__device__ __forceinline__ cd cdiv(cd a, cd b) {
    const double d = b.x * b.x + b.y * b.y;
    return mk((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}
__device__ __forceinline__ double wsum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

struct SolveArgs {
    int n, map_nb, nblk;   // order; rows per row-order snapshot and snapshots per matrix
    const double2* A;      // [nmat][n][n]  P M = L U in place
    const int* maps;       // [nmat][nblk][n]
    const int* lu_info;    // [nmat]
    const double2* V;      // [n][ldv] probes
    int ldv, l0, nl;       // columns l0 .. l0 + nl - 1 of V and X
    double2* X;            // [nmat][n][ldx]
    int ldx;
    const struct SolveItem* list;  // the restricted solve: one entry per workgroup row of the grid (below)
};

// The restricted solve: matrix q of the launch is any factored matrix of the call, with its own
// column range -- when one item of a search over (set, contour) items doubles L, only its nodes get the new columns.
// The matrices of a call live in one buffer per node round, so an entry carries the matrix's own pointers.
struct SolveItem {
    const double2* A;    // [n][n] factors
    const int* maps;     // [nblk][n]
    const int* lu_info;  // its info
    double2* X;          // [n][ldx]
    int map_nb, l0, nl;  // rows per row-order snapshot; columns l0 .. l0 + nl - 1
};

// one workgroup per (matrix, group of G columns).  LISTED = false: matrix blockIdx.x of P.A, columns P.l0 .. of every
// matrix; LISTED = true: the matrix and columns of P.list[blockIdx.x] (a sibling kernel read from the same text: the
// arithmetic of a column is the same in both)
template <int G, bool LISTED>
__global__ __launch_bounds__(CT) void k_contour_solve(SolveArgs P) {
    extern __shared__ double2 sm[];
    const int n = P.n, b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int l0 = P.l0, nl = P.nl, map_nb = P.map_nb, nblk = P.nblk;
    double2* out = P.X + (size_t)b * n * P.ldx;
    const double2* a = P.A + (size_t)b * n * n;
    const int* maps = P.maps + (size_t)b * P.nblk * n;
    const int* lu_info = P.lu_info + b;
    if constexpr (LISTED) {
        const SolveItem it = P.list[b];
        l0 = it.l0, nl = it.nl, map_nb = it.map_nb, nblk = (n + map_nb - 1) / map_nb;
        out = it.X, a = it.A, maps = it.maps, lu_info = it.lu_info;
        if ((int)blockIdx.y * G >= nl) return;  // (the grid is as deep as the widest range of the list)
    }
    const int c0 = l0 + blockIdx.y * G;  // first column of the group
    const int gn = min(G, l0 + nl - c0);
    if (*lu_info != 0) {  // no factors: no solution
        for (int e = tid; e < n * gn; e += CT) out[(size_t)(e / gn) * P.ldx + c0 + e % gn] = make_double2(__builtin_nan(""), __builtin_nan(""));
        return;
    }
    double2* x = sm;                                  // [n][G]
    double2* tri = sm + (size_t)n * G;                // [TB][TB + 1] the block's own triangle
    int* rowmap = reinterpret_cast<int*>(tri + TB * (TB + 1));
    for (int r = tid; r < n; r += CT) rowmap[r] = maps[(size_t)(r / map_nb) * n + r];
    __syncthreads();
    for (int e = tid; e < n * G; e += CT) {  // c = P v
        const int r = e / G, g = e % G;
        x[e] = g < gn ? P.V[(size_t)rowmap[r] * P.ldv + c0 + g] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    const int B = (n + TB - 1) / TB;
    for (int pass = 0; pass < 2; ++pass) {  // 0: L c' = c (unit diagonal), 1: U y = c'
        const bool fwd = pass == 0;
        for (int s = 0; s < B; ++s) {
            const int r0 = (fwd ? s : B - 1 - s) * TB, nbk = min(TB, n - r0);
            const int jlo = fwd ? 0 : r0 + nbk, jhi = fwd ? r0 : n;  // finished unknowns
            // the block's equations minus their coupling to every finished unknown: a wave per row
            for (int l = wave; l < nbk; l += CW) {
                const double2* row = a + (size_t)rowmap[r0 + l] * n;
                cd acc[G];
#pragma unroll
                for (int g = 0; g < G; ++g) acc[g] = mk(0.0, 0.0);
                for (int j = jlo + lane; j < jhi; j += 64) {
                    const double2 cf = row[j];
                    const cd c = mk(cf.x, cf.y);
#pragma unroll
                    for (int g = 0; g < G; ++g) acc[g] = acc[g] + c * mk(x[(size_t)j * G + g].x, x[(size_t)j * G + g].y);
                }
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const double sx = wsum(acc[g].x), sy = wsum(acc[g].y);
                    if (lane == 0) {
                        double2& xv = x[(size_t)(r0 + l) * G + g];
                        xv = make_double2(xv.x - sx, xv.y - sy);
                    }
                }
            }
            for (int e = tid; e < TB * TB; e += CT) {
                const int l = e / TB, kk = e % TB;
                tri[l * (TB + 1) + kk] = l < nbk && kk < nbk ? a[(size_t)rowmap[r0 + l] * n + r0 + kk] : make_double2(0.0, 0.0);
            }
            __syncthreads();
            // the 16 x 16 triangle: 16 lanes per column (lane l holds row l of the block), the finished unknown of each
            // step broadcast within the 16-lane group; G <= 16 columns use at most the 256 threads
            {
                const int g = tid >> 4, l = tid & 15;
                if (g < G) {
                    double2* xp = &x[(size_t)(r0 + min(l, nbk - 1)) * G + g];
                    cd xl = l < nbk ? mk(xp->x, xp->y) : mk(0.0, 0.0);
                    const double2* trow = tri + l * (TB + 1);
                    if (fwd) {
                        for (int q = 0; q < TB - 1; ++q) {
                            const cd xq = mk(__shfl(xl.x, q, 16), __shfl(xl.y, q, 16));
                            if (l > q) xl = xl - mk(trow[q].x, trow[q].y) * xq;
                        }
                    } else {
                        for (int q = TB - 1; q >= 0; --q) {
                            if (l == q && q < nbk) xl = cdiv(xl, mk(trow[q].x, trow[q].y));
                            const cd xq = mk(__shfl(xl.x, q, 16), __shfl(xl.y, q, 16));
                            if (l < q) xl = xl - mk(trow[q].x, trow[q].y) * xq;
                        }
                    }
                    if (l < nbk) *xp = make_double2(xl.x, xl.y);
                }
            }
            __syncthreads();
        }
    }
    for (int e = tid; e < n * gn; e += CT) {
        const int r = e / gn, g = e % gn;
        out[(size_t)r * P.ldx + c0 + g] = x[(size_t)r * G + g];
    }
}

// log det M = sum_i log u_ii + i pi parity(row order): (log|det|, arg det in (-pi, pi]); a matrix without factors gets
// (-inf, NaN)
__global__ __launch_bounds__(CT) void k_contour_logdet(int n, const double2* A, const int* maps, int map_nb, int nblk,
                                                       const int* lu_info, double2* logdet) {
    __shared__ double s_re[CT], s_im[CT];
    extern __shared__ int s_map[];  // [n] row order, then [n] visited flags
    const int b = blockIdx.x, tid = threadIdx.x;
    if (lu_info[b] != 0) {
        if (tid == 0) logdet[b] = make_double2(-__builtin_inf(), __builtin_nan(""));
        return;
    }
    const double2* a = A + (size_t)b * n * n;
    const int* mp = maps + (size_t)b * nblk * n;
    int* seen = s_map + n;
    double lr = 0.0, li = 0.0;
    for (int r = tid; r < n; r += CT) {
        const int pr = mp[(size_t)(r / map_nb) * n + r];
        s_map[r] = pr, seen[r] = 0;
        const double2 u = a[(size_t)pr * n + r];
        lr += log(hypot(u.x, u.y)), li += atan2(u.y, u.x);
    }
    s_re[tid] = lr, s_im[tid] = li;
    __syncthreads();
    for (int w = CT / 2; w >= 1; w >>= 1) {
        if (tid < w) s_re[tid] += s_re[tid + w], s_im[tid] += s_im[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        int cycles = 0;  // parity of a permutation = (n - cycles) mod 2
        for (int r = 0; r < n; ++r) {
            if (seen[r]) continue;
            ++cycles;
            for (int q = r; !seen[q]; q = s_map[q]) seen[q] = 1;
        }
        const double arg = remainder(s_im[0] + ((n - cycles) & 1 ? M_PI : 0.0), 2.0 * M_PI);
        logdet[b] = make_double2(s_re[0], arg);
    }
}

// A0[i][l] = sum_j w_j X_j[i][l], A1[i][l] = sum_j w_j z_j X_j[i][l], j in order; nodes with info != 0 left out
__global__ void k_contour_moments(int n, int L, int nq, const double2* X, int ldx, const double2* wz, const int* info,
                                  double2* A0, double2* A1) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * L) return;
    const int i = e / L, l = e % L;
    cd s0 = mk(0.0, 0.0), s1 = mk(0.0, 0.0);
    for (int j = 0; j < nq; ++j) {
        if (info[j] != 0) continue;
        const double2 xv = X[((size_t)j * n + i) * ldx + l];
        const double2 w = wz[2 * j], z = wz[2 * j + 1];
        const cd t = mk(w.x, w.y) * mk(xv.x, xv.y);
        s0 = s0 + t, s1 = s1 + t * mk(z.x, z.y);
    }
    A0[e] = make_double2(s0.x, s0.y), A1[e] = make_double2(s1.x, s1.y);
}

// The same sums per group: group g (blockIdx.y) sums the nodes idx[off[g]] .. idx[off[g + 1] - 1] in
// that order, with its own column count Ls[g] (null: L for every group), into A0 / A1 + g * ostride.  A thread per
// (group, entry), consecutive threads on consecutive l of a row of X; no atomics, so two calls on the same inputs are
// bit-identical and a group's sum runs in the order k_contour_moments uses on the group alone.  Xn[node]: the node's X
// ([n][ldx]); wz[2 node], wz[2 node + 1]: its w and z; info (nullable): nodes with info != 0 are left out.
__global__ void k_contour_moments_groups(int n, int L, const int* Ls, const int* off, const int* idx,
                                         const double2* const* Xn, int ldx, const double2* wz, const int* info, double2* A0,
                                         double2* A1, size_t ostride) {
    const int g = blockIdx.y, Lg = Ls ? Ls[g] : L;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * Lg) return;
    const int i = e / Lg, l = e % Lg;
    cd s0 = mk(0.0, 0.0), s1 = mk(0.0, 0.0);
    for (int q = off[g]; q < off[g + 1]; ++q) {
        const int j = idx[q];
        if (info && info[j] != 0) continue;
        const double2 xv = Xn[j][(size_t)i * ldx + l];
        const double2 w = wz[2 * j], z = wz[2 * j + 1];
        const cd t = mk(w.x, w.y) * mk(xv.x, xv.y);
        s0 = s0 + t, s1 = s1 + t * mk(z.x, z.y);
    }
    A0[g * ostride + e] = make_double2(s0.x, s0.y), A1[g * ostride + e] = make_double2(s1.x, s1.y);
}

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long k) {
    unsigned long long z = PROBE_SEED + (k + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// V[i][l] (l < LCAP): real and imaginary parts uniform in [-1, 1) from counters 2 (i LCAP + l) and 2 (i LCAP + l) + 1
__global__ void k_contour_probes(int n, double2* V) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * LCAP) return;
    const double s = 0x1.0p-53;
    const double re = (double)(splitmix64(2ull * e) >> 11) * s, im = (double)(splitmix64(2ull * e + 1) >> 11) * s;
    V[e] = make_double2(2.0 * re - 1.0, 2.0 * im - 1.0);
}

size_t solve_lds(int n, int G) { return ((size_t)n * G + TB * (TB + 1)) * sizeof(double2) + (size_t)n * sizeof(int); }

// columns per workgroup: as many as fit 64 KiB of LDS, at most 16, and no more than leave at least one workgroup per
// compute unit (a workgroup's blocks are a chain of 2 ceil(n / 16) steps: parallelism comes from the grid)
int solve_group(int n, int nl, int nmat, int n_cu) {
    int G = 16;
    while (G > 1 && (solve_lds(n, G) > 64 * 1024 || G / 2 >= nl || (long)nmat * ((nl + G - 1) / G) < n_cu)) G /= 2;
    return G;
}

template <int G, bool LISTED>
hipError_t launch_solve_g(const SolveArgs& P, int nmat, hipStream_t st) {
    const size_t lds = solve_lds(P.n, G);
    if (lds > 150 * 1024) return hipErrorNotSupported;
    if (lds > 48 * 1024) {
        const hipError_t ea = hipFuncSetAttribute((const void*)k_contour_solve<G, LISTED>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ea != hipSuccess) return ea;
    }
    hipLaunchKernelGGL((k_contour_solve<G, LISTED>), dim3(nmat, (P.nl + G - 1) / G), dim3(CT), lds, st, P);
    return hipGetLastError();
}

// P.list null: columns P.l0 .. P.l0 + P.nl - 1 of the nmat matrices of P.A; else the nmat entries of P.list, P.nl the
// widest of their column ranges
template <bool LISTED>
hipError_t launch_contour_solve_as(const SolveArgs& P, int nmat, int n_cu, hipStream_t st) {
    switch (solve_group(P.n, P.nl, nmat, n_cu)) {
        case 16: return launch_solve_g<16, LISTED>(P, nmat, st);
        case 8: return launch_solve_g<8, LISTED>(P, nmat, st);
        case 4: return launch_solve_g<4, LISTED>(P, nmat, st);
        case 2: return launch_solve_g<2, LISTED>(P, nmat, st);
        default: return launch_solve_g<1, LISTED>(P, nmat, st);
    }
}
hipError_t launch_contour_solve(const SolveArgs& P, int nmat, int n_cu, hipStream_t st) {
    return P.list ? launch_contour_solve_as<true>(P, nmat, n_cu, st) : launch_contour_solve_as<false>(P, nmat, n_cu, st);
}

// matrices factored in one batch, with their own copy of the row order (the factorisation's scratch is reused)
struct NodeSet {
    int first = 0, count = 0, map_nb = 1;
    DeviceBuffer<double> A;  // factors
    DeviceBuffer<int> maps;
};

struct ContourState {
    emme_ctx* c;
    int n;
    int ldx;
    DeviceBuffer<double> X, logdet, V, wz, A0, A1;
    DeviceBuffer<int> info;
    std::vector<NodeSet> sets;
    int ldv = LCAP;
    const double2* Vp() const { return (const double2*)V.get(); }
};

// factor set.A in place (count matrices from node index set.first), keep the row order and info, log det
int factor_set(ContourState& S, NodeSet& set, const char* who) {
    emme_ctx* c = S.c;
    const int n = S.n;
    LuScratch scr;
    int map_nb = 1;
    const size_t per_map_max = (size_t)n * ((n + trace_solve_nb() - 1) / trace_solve_nb());  // (the unblocked LU: one)
    HIP_TRY(set.maps.grow(sizeof(int) * per_map_max * set.count));
    const int rc = lu_factor_batch(c, n, set.count, set.A, scr, who,
                                   [&](int b0, int nb, const int* maps, int mnb, const int* lu_info) -> hipError_t {
                                       map_nb = mnb;
                                       const size_t per = (size_t)n * ((n + mnb - 1) / mnb);
                                       hipError_t e = hipMemcpyAsync(set.maps + per * b0, maps, sizeof(int) * per * nb,
                                                                     hipMemcpyDeviceToDevice, c->stream);
                                       if (e == hipSuccess)
                                           e = hipMemcpyAsync(S.info + set.first + b0, lu_info, sizeof(int) * nb,
                                                              hipMemcpyDeviceToDevice, c->stream);
                                       return e;
                                   });
    if (rc) return rc;
    set.map_nb = map_nb;
    ScopedSpan sp(c, K_OTHER);
    hipLaunchKernelGGL(k_contour_logdet, dim3(set.count), dim3(CT), 2 * sizeof(int) * n, c->stream, n,
                       (const double2*)set.A.get(), set.maps.get(), map_nb, (n + map_nb - 1) / map_nb,
                       S.info + set.first, (double2*)S.logdet.get() + set.first);
    HIP_TRY(hipGetLastError());
    return EMME_OK;
}

// X columns [l0, l0 + nl) of every node of the set
int solve_set(ContourState& S, const NodeSet& set, int l0, int nl) {
    SolveArgs P;
    P.n = S.n, P.map_nb = set.map_nb, P.nblk = (S.n + set.map_nb - 1) / set.map_nb;
    P.A = (const double2*)set.A.get();
    P.maps = set.maps;
    P.lu_info = S.info + set.first;
    P.V = S.Vp(), P.ldv = S.ldv, P.l0 = l0, P.nl = nl;
    P.X = (double2*)S.X.get() + (size_t)set.first * S.n * S.ldx;
    P.ldx = S.ldx;
    P.list = nullptr;
    ScopedSpan sp(S.c, K_OTHER);
    HIP_TRY(launch_contour_solve(P, set.count, S.c->n_cu, S.c->stream));
    return EMME_OK;
}

// moments over nodes [0, nq) with weights wz (host, (w_j, z_j) per node) into host A0, A1 (n x L)
int moments(ContourState& S, int nq, const std::vector<double>& wz, int L, double* A0, double* A1) {
    emme_ctx* c = S.c;
    HIP_TRY(hipMemcpyAsync(S.wz, wz.data(), sizeof(double) * 4 * nq, hipMemcpyHostToDevice, c->stream));
    {
        ScopedSpan sp(c, K_OTHER);
        const int ne = S.n * L;
        hipLaunchKernelGGL(k_contour_moments, dim3((ne + 255) / 256), dim3(256), 0, c->stream, S.n, L, nq,
                           (const double2*)S.X.get(), S.ldx, (const double2*)S.wz.get(), S.info.get(),
                           (double2*)S.A0.get(), (double2*)S.A1.get());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(A0, S.A0, sizeof(double) * 2 * S.n * L, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(A1, S.A1, sizeof(double) * 2 * S.n * L, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EMME_OK;
}

// X, log det and info of `nodes` matrices
int alloc_nodes(ContourState& S, int nodes, int ldx) {
    S.ldx = ldx;
    HIP_TRY(S.X.grow(sizeof(double) * 2 * (size_t)nodes * S.n * ldx));
    HIP_TRY(S.logdet.grow(sizeof(double) * 2 * nodes));
    HIP_TRY(S.info.grow(sizeof(int) * nodes));
    return EMME_OK;
}

int alloc_state(ContourState& S, int nodes, int ldx) {
    EMME_TRY(alloc_nodes(S, nodes, ldx));
    HIP_TRY(S.wz.grow(sizeof(double) * 4 * nodes));
    HIP_TRY(S.A0.grow(sizeof(double) * 2 * (size_t)S.n * LCAP));
    HIP_TRY(S.A1.grow(sizeof(double) * 2 * (size_t)S.n * LCAP));
    return EMME_OK;
}

int make_probes(ContourState& S) {
    HIP_TRY(S.V.grow(sizeof(double) * 2 * (size_t)S.n * LCAP));
    S.ldv = LCAP;
    hipLaunchKernelGGL(k_contour_probes, dim3((S.n * LCAP + 255) / 256), dim3(256), 0, S.c->stream, S.n, (double2*)S.V.get());
    HIP_TRY(hipGetLastError());
    return EMME_OK;
}

// what the two building blocks share: caller matrices M (nq of order n, host or device) factored, log det taken and
// X = M^-1 V solved for L columns (V null: the internal probes), all in S
int solve_caller_matrices(emme_ctx* c, ContourState& S, const char* who, int n, int nq, const double* M, int L, const double* V) {
    HIP_TRY(hipSetDevice(c->device));
    EMME_TRY(ensure_batch(c, nq));
    S.c = c, S.n = n;
    EMME_TRY(alloc_state(S, nq, L));
    if (V) {
        HIP_TRY(S.V.grow(sizeof(double) * 2 * (size_t)n * L));
        S.ldv = L;
        HIP_TRY(hipMemcpyAsync(S.V, V, sizeof(double) * 2 * (size_t)n * L,
                               is_device_ptr(V) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    } else {
        EMME_TRY(make_probes(S));
    }
    S.sets.emplace_back();
    NodeSet& set = S.sets.back();
    set.first = 0, set.count = nq;
    const size_t mbytes = sizeof(double) * 2 * (size_t)n * n * nq;
    HIP_TRY(set.A.grow(mbytes));
    HIP_TRY(hipMemcpyAsync(set.A, M, mbytes, is_device_ptr(M) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    EMME_TRY(factor_set(S, set, who));
    return solve_set(S, set, 0, L);
}

// device images of the lists of a grouped-moments launch, and its sums
struct GroupBuffers {
    DeviceBuffer<int> ints;  // off | idx | Ls
    DeviceBuffer<const double2*> Xn;
    DeviceBuffer<double> wz, A0, A1;
};

// Moments per group (k_contour_moments_groups) into host A0, A1 (ngroups blocks of ostride complex entries each, a
// group's n x L_g sums packed at the start of its block).  off / idx: the groups' node lists; Xn, wz: X and (w, z) of
// every node; Ls null: L columns for every group; d_info (device, nullable): nodes to leave out.
int moments_groups(emme_ctx* c, int n, int L, const std::vector<int>* Ls, const std::vector<int>& off,
                   const std::vector<int>& idx, const std::vector<const double2*>& Xn, int ldx, const std::vector<double>& wz,
                   const int* d_info, GroupBuffers& G, size_t ostride, double* A0, double* A1) {
    const int ng = (int)off.size() - 1;
    int Lmax = L;
    if (Ls) Lmax = *std::max_element(Ls->begin(), Ls->end());
    std::vector<int> ints(off);
    ints.insert(ints.end(), idx.begin(), idx.end());
    if (Ls) ints.insert(ints.end(), Ls->begin(), Ls->end());
    HIP_TRY(G.ints.grow(sizeof(int) * ints.size()));
    HIP_TRY(G.Xn.grow(sizeof(double2*) * std::max<size_t>(Xn.size(), 1)));
    HIP_TRY(G.wz.grow(sizeof(double) * std::max<size_t>(wz.size(), 1)));
    HIP_TRY(G.A0.grow(sizeof(double) * 2 * ostride * ng));
    HIP_TRY(G.A1.grow(sizeof(double) * 2 * ostride * ng));
    HIP_TRY(hipMemcpyAsync(G.ints, ints.data(), sizeof(int) * ints.size(), hipMemcpyHostToDevice, c->stream));
    if (!Xn.empty()) HIP_TRY(hipMemcpyAsync(G.Xn, Xn.data(), sizeof(double2*) * Xn.size(), hipMemcpyHostToDevice, c->stream));
    if (!wz.empty()) HIP_TRY(hipMemcpyAsync(G.wz, wz.data(), sizeof(double) * wz.size(), hipMemcpyHostToDevice, c->stream));
    {
        ScopedSpan sp(c, K_OTHER);
        const int* d_off = G.ints;
        const int* d_idx = d_off + off.size();
        hipLaunchKernelGGL(k_contour_moments_groups, dim3((n * Lmax + 255) / 256, ng), dim3(256), 0, c->stream, n, L,
                           Ls ? d_idx + idx.size() : nullptr, d_off, d_idx, G.Xn.get(), ldx, (const double2*)G.wz.get(),
                           d_info, (double2*)G.A0.get(), (double2*)G.A1.get(), ostride);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(A0, G.A0, sizeof(double) * 2 * ostride * ng, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(A1, G.A1, sizeof(double) * 2 * ostride * ng, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EMME_OK;
}

// one restricted solve (k_contour_solve<G, true>) for the entries of `list`
int solve_listed(emme_ctx* c, int n, const double2* V, int ldv, const std::vector<SolveItem>& list,
                 DeviceBuffer<SolveItem>& d_list) {
    if (list.empty()) return EMME_OK;
    HIP_TRY(d_list.grow(sizeof(SolveItem) * list.size()));
    HIP_TRY(hipMemcpyAsync(d_list, list.data(), sizeof(SolveItem) * list.size(), hipMemcpyHostToDevice, c->stream));
    SolveArgs P{};
    P.n = n, P.V = V, P.ldv = ldv, P.ldx = LCAP, P.list = d_list;
    for (const SolveItem& it : list) P.nl = std::max(P.nl, it.nl);
    ScopedSpan sp(c, K_OTHER);
    HIP_TRY(launch_contour_solve(P, (int)list.size(), c->n_cu, c->stream));
    return EMME_OK;
}

}  // namespace
}  // namespace emme

using namespace emme;

extern "C" {

int emme_contour_moments_batch(emme_ctx_t* c, int n, int nq, const double* M, const double* z, const double* w, int L,
                               const double* V, double* A0, double* A1, double* logdet, int* info) {
    if (!c || !M || !z || !w || !A0 || !A1 || !logdet || !info || n < 1 || nq < 1 || L < 1 || L > LCAP) {
        set_error("emme_contour_moments_batch: need M, z, w, A0, A1, logdet, info, n >= 1, nq >= 1 and 1 <= L <= 64");
        return EMME_EINVAL;
    }
    if (n > 2048) {
        set_error("emme_contour_moments_batch: order above 2048 is not supported (the factorisation's range)");
        return EMME_ECONFIG;
    }
    ContourState S;
    int rc = solve_caller_matrices(c, S, "emme_contour_moments_batch", n, nq, M, L, V);
    if (rc) return rc;
    std::vector<double> wz(4 * (size_t)nq);
    for (int j = 0; j < nq; ++j) wz[4 * j] = w[2 * j], wz[4 * j + 1] = w[2 * j + 1], wz[4 * j + 2] = z[2 * j], wz[4 * j + 3] = z[2 * j + 1];
    rc = moments(S, nq, wz, L, A0, A1);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(logdet, S.logdet, sizeof(double) * 2 * nq, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(info, S.info, sizeof(int) * nq, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EMME_OK;
}

int emme_contour_moments_groups(emme_ctx_t* c, int n, int nq, const double* M, const int* group, int ngroups,
                                const double* z, const double* w, int L, const double* V, double* A0, double* A1,
                                double* logdet, int* info) {
    if (!c || !M || !group || !z || !w || !A0 || !A1 || !logdet || !info || n < 1 || nq < 1 || L < 1 || L > LCAP ||
        ngroups < 1 || ngroups > 65535) {
        set_error("emme_contour_moments_groups: need M, group, z, w, A0, A1, logdet, info, n >= 1, nq >= 1, 1 <= L <= 64 and "
                  "1 <= ngroups <= 65535");
        return EMME_EINVAL;
    }
    for (int j = 0; j < nq; ++j)
        if (group[j] < 0 || group[j] >= ngroups) {
            set_error("emme_contour_moments_groups: group[" + std::to_string(j) + "] = " + std::to_string(group[j]) +
                      " is outside [0, " + std::to_string(ngroups) + ")");
            return EMME_EINVAL;
        }
    if (n > 2048) {
        set_error("emme_contour_moments_groups: order above 2048 is not supported (the factorisation's range)");
        return EMME_ECONFIG;
    }
    ContourState S;
    EMME_TRY(solve_caller_matrices(c, S, "emme_contour_moments_groups", n, nq, M, L, V));
    // the groups' node lists, ascending j inside a group
    std::vector<int> off(ngroups + 1, 0), idx(nq);
    for (int j = 0; j < nq; ++j) ++off[group[j] + 1];
    for (int g = 0; g < ngroups; ++g) off[g + 1] += off[g];
    std::vector<int> at(off.begin(), off.end() - 1);
    for (int j = 0; j < nq; ++j) idx[at[group[j]]++] = j;
    std::vector<const double2*> Xn(nq);
    std::vector<double> wz(4 * (size_t)nq);
    for (int j = 0; j < nq; ++j) {
        Xn[j] = (const double2*)S.X.get() + (size_t)j * n * L;
        wz[4 * j] = w[2 * j], wz[4 * j + 1] = w[2 * j + 1], wz[4 * j + 2] = z[2 * j], wz[4 * j + 3] = z[2 * j + 1];
    }
    GroupBuffers G;
    EMME_TRY(moments_groups(c, n, L, nullptr, off, idx, Xn, L, wz, S.info, G, (size_t)n * L, A0, A1));
    HIP_TRY(hipMemcpyAsync(logdet, S.logdet, sizeof(double) * 2 * nq, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(info, S.info, sizeof(int) * nq, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EMME_OK;
}

int emme_find_roots_in_contours_sets(emme_ctx_t* c, int nitems, const int* set, const emme_contour_t* contours, int exact,
                                     double tol, int step_limit, int max_roots, double* roots, int* iters, int* info,
                                     int* n_roots, int* winding, int* points_used, int* status) {
    const std::string who = "emme_find_roots_in_contours_sets";
    if (nitems < 1 || nitems > 65535) {
        set_error(who + ": nitems must lie in 1 .. 65535");
        return EMME_EINVAL;
    }
    if (!c || !set || !contours || !roots || !iters || !info || !n_roots || !winding || !points_used || !status ||
        max_roots < 1 || step_limit < 0 || !(tol > 0.0)) {
        set_error(who + ": need a context, sets, contours, tol > 0, step_limit >= 0, max_roots >= 1 and every output");
        return EMME_EINVAL;
    }
    for (int k = 0; k < nitems; ++k)
        if (const char* bad = contour_arg_error(&contours[k])) {
            set_error(who + ": item " + std::to_string(k) + ": " + bad);
            return EMME_EINVAL;
        }
    EMME_TRY(check_set_indices(c, set, nitems, who.c_str()));
    const int n = c->dim;
    if (n > 2048) {
        set_error(who + ": dim above 2048 is not supported (the factorisation's range)");
        return EMME_ECONFIG;
    }
    HIP_TRY(hipSetDevice(c->device));
    ContourRounds plan(nitems, set, contours);
    ContourState probes;  // (only V: every item reads the same probes)
    probes.c = c, probes.n = n;
    EMME_TRY(make_probes(probes));
    std::vector<ContourState> rounds;    // the nodes of a node round: factors, X, log det, info
    std::vector<SolveItem> node;         // every node's factors and X, columns unset
    std::vector<const double2*> Xn;
    std::vector<double> ld;              // log det and info of every node, by node
    std::vector<int> h_info;
    std::vector<SolveItem> list;
    DeviceBuffer<SolveItem> d_list;
    std::string first_error;
    auto drop = [&](int item, int rc, const std::string& msg) {
        plan.drop(item, rc);
        if (first_error.empty()) first_error = who + ": item " + std::to_string(item) + ": " + msg;
    };
    // ---- node rounds: one fill, one factorisation, one log-det and one solve launch for the new nodes of all items
    while (plan.plan_nodes()) {
        const int cnt = (int)plan.r_item.size(), first = plan.r_first;
        EMME_TRY(ensure_batch(c, cnt));
        rounds.emplace_back();
        ContourState& S = rounds.back();
        S.c = c, S.n = n;
        EMME_TRY(alloc_nodes(S, cnt, LCAP));
        S.sets.emplace_back();
        NodeSet& ns = S.sets.back();
        ns.first = 0, ns.count = cnt;
        const size_t msize = 2 * (size_t)n * n;
        HIP_TRY(ns.A.grow(sizeof(double) * msize * cnt));
        EMME_TRY(upload_set_indices(c, plan.r_set.data(), cnt));
        EMME_TRY(upload_omega(c, plan.r_omega.data(), cnt));
        EMME_TRY(reset_fill_counters(c, cnt));
        FillRequest rq(cnt, c->d_omega, ns.A);
        rq.host_omega = plan.r_omega.data();
        rq.d_set = c->d_set, rq.host_set = plan.r_set.data();
        EMME_TRY(fill(c, rq));
        std::vector<unsigned long long> iv;
        std::vector<int> stv;
        EMME_TRY(queue_fill_counters(c, cnt, iv, &stv));
        HIP_TRY(hipStreamSynchronize(c->stream));
        (void)fold_fill_counters(c, iv, nullptr);
        for (int q = 0; q < cnt; ++q) {
            if (stv[q] == 0) continue;
            // the item leaves; its node is factored as a zero matrix (info != 0) and never read
            char buf[160];
            snprintf(buf, sizeof buf, "the fill of the node omega = %.17g%+.17gi failed (quadrature depth cap or non-finite integral)",
                     plan.r_omega[2 * q], plan.r_omega[2 * q + 1]);
            drop(plan.r_item[q], EMME_ENUMERIC, buf);
            HIP_TRY(hipMemsetAsync(ns.A + msize * q, 0, sizeof(double) * msize, c->stream));
        }
        EMME_TRY(factor_set(S, ns, who.c_str()));
        const size_t per_map = (size_t)n * ((n + ns.map_nb - 1) / ns.map_nb);
        list.clear();
        for (int q = 0; q < cnt; ++q) {
            SolveItem e{};
            e.A = (const double2*)ns.A.get() + (size_t)n * n * q, e.maps = ns.maps + per_map * q, e.lu_info = S.info + q;
            e.X = (double2*)S.X.get() + (size_t)q * n * LCAP, e.map_nb = ns.map_nb;
            node.push_back(e), Xn.push_back(e.X);
            const ContourRounds::Item& it = plan.items[plan.r_item[q]];
            if (it.dropped) continue;
            e.l0 = 0, e.nl = it.L;
            list.push_back(e);
        }
        EMME_TRY(solve_listed(c, n, probes.Vp(), probes.ldv, list, d_list));
        ld.resize(2 * (size_t)plan.nodes()), h_info.resize(plan.nodes());
        // (in order on the context's stream, which may be a non-blocking one: not a null-stream copy)
        HIP_TRY(hipMemcpyAsync(&ld[2 * (size_t)first], S.logdet, sizeof(double) * 2 * cnt, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(&h_info[first], S.info, sizeof(int) * cnt, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        plan.take_logdets(ld.data());
    }
    // ---- Beyn: moments per item with the trapezoid weights of its final N; L doubles per item while its A0 keeps full
    // numerical rank, and only the nodes of such an item get the new columns solved
    std::vector<int> which, off, idx, Ls;
    std::vector<double> wz, A0, A1, mu(2 * LCAP), sig(LCAP);
    std::vector<std::vector<double>> guesses(nitems);
    GroupBuffers G;
    const size_t ostride = (size_t)n * LCAP;
    while (plan.plan_moments(h_info.data(), which, off, idx, wz)) {
        const int ng = (int)which.size();
        Ls.resize(ng);
        for (int g = 0; g < ng; ++g) Ls[g] = plan.items[which[g]].L;
        A0.resize(2 * ostride * ng), A1.resize(2 * ostride * ng);
        EMME_TRY(moments_groups(c, n, 0, &Ls, off, idx, Xn, LCAP, wz, nullptr, G, ostride, A0.data(), A1.data()));
        list.clear();
        for (int g = 0; g < ng; ++g) {
            const int item = which[g];
            const emme_contour_t& ct = plan.items[item].ct;
            int k = 0, l0 = 0, nl = 0;
            const int rc = emme_contour_eigs(n, Ls[g], &A0[2 * ostride * g], &A1[2 * ostride * g], ct.rank_tol, LCAP, mu.data(),
                                             &k, sig.data());
            if (rc) {
                drop(item, rc, emme_last_error());
                continue;
            }
            if (std::getenv("EMME_DEBUG"))
                fprintf(stderr, "[emme] contours: item %d N %d L %d k %d W %d\n", item, plan.items[item].N, Ls[g], k,
                        plan.items[item].W);
            if (!plan.take_rank(item, k, &l0, &nl)) {
                // the candidates (normalised radius below 1.5: the others are no eigenvalues inside)
                contour_candidates(ct, k, mu.data(), guesses[item]);
                continue;
            }
            for (int nd : plan.items[item].nodes) {
                SolveItem e = node[nd];
                e.l0 = l0, e.nl = nl;
                list.push_back(e);
            }
        }
        EMME_TRY(solve_listed(c, n, probes.Vp(), probes.ldv, list, d_list));
    }
    // ---- one search over sets polishes the candidates of all items: items in order, an item's in the order of mu
    std::vector<double> g_all;
    std::vector<int> g_set, g_first(nitems + 1, 0);
    for (int k = 0; k < nitems; ++k) {
        if (!plan.items[k].dropped) {
            g_all.insert(g_all.end(), guesses[k].begin(), guesses[k].end());
            g_set.insert(g_set.end(), guesses[k].size() / 2, set[k]);
        }
        g_first[k + 1] = (int)g_set.size();
    }
    const int ng = (int)g_set.size();
    std::vector<double> r(2 * (size_t)ng), path(2 * (size_t)ng * (step_limit + 1));
    std::vector<int> its(ng), inf(ng);
    if (ng > 0)
        EMME_TRY(emme_solve_roots_sets(c, g_set.data(), g_all.data(), ng, exact, tol, step_limit, r.data(), its.data(),
                                       inf.data(), path.data()));
    else
        c->last_n = 0;  // (no polish: emme_ctx_get_matrix has nothing to refer to)
    for (int k = 0; k < nitems; ++k) {
        const ContourRounds::Item& it = plan.items[k];
        const int o = g_first[k], cnt = g_first[k + 1] - o;
        std::vector<ContourRoot> found;
        if (cnt > 0)
            found = contour_keep_roots(it.ct, tol, step_limit, cnt, &r[2 * (size_t)o], &its[o], &inf[o],
                                       &path[2 * (size_t)o * (step_limit + 1)]);
        for (int q = 0; q < std::min((int)found.size(), max_roots); ++q) {
            const size_t at = (size_t)k * max_roots + q;
            roots[2 * at] = found[q].re, roots[2 * at + 1] = found[q].im, iters[at] = found[q].it, info[at] = found[q].inf;
        }
        n_roots[k] = (int)found.size(), winding[k] = it.W, points_used[k] = it.N, status[k] = it.status;
    }
    if (!first_error.empty()) set_error(first_error);
    return EMME_OK;
}

int emme_find_roots_in_contour(emme_ctx_t* c, const emme_contour_t* ct, double tol, int step_limit, int max_roots,
                               double* roots, int* iters, int* info, int* n_roots, int* winding, int* points_used) {
    if (!c || !ct || !roots || !iters || !info || !n_roots || !winding || !points_used || max_roots < 1 || step_limit < 0 ||
        !(tol > 0.0)) {
        set_error("emme_find_roots_in_contour: need a context, a contour, tol > 0, step_limit >= 0, max_roots >= 1 and every output");
        return EMME_EINVAL;
    }
    if (const char* bad = contour_arg_error(ct)) {
        set_error(std::string("emme_find_roots_in_contour: ") + bad);
        return EMME_EINVAL;
    }
    const double cx = ct->center[0], cy = ct->center[1], ea = ct->semi_axes[0], eb = ct->semi_axes[1];
    const int n = c->dim;
    if (n > 2048) {
        set_error("emme_find_roots_in_contour: dim above 2048 is not supported (the factorisation's range)");
        return EMME_ECONFIG;
    }
    HIP_TRY(hipSetDevice(c->device));
    const int cap = ct->max_points;
    ContourState S;
    S.c = c, S.n = n;
    int rc = alloc_state(S, cap, LCAP);
    if (rc) return rc;
    rc = make_probes(S);
    if (rc) return rc;
    const double rho = std::max(ea, eb);
    std::vector<int> node_m;  // node k sits at t = 2 pi node_m[k] / cap
    auto omega_at = [&](int m, double* o) {
        const double t = 2.0 * M_PI * m / cap;
        o[0] = cx + ea * std::cos(t), o[1] = cy + eb * std::sin(t);
    };
    int L = ct->probes;
    // fill, factor and solve a batch of new nodes
    auto add_nodes = [&](const std::vector<int>& ms) -> int {
        const int cnt = (int)ms.size();
        int r = ensure_batch(c, cnt);
        if (r) return r;
        std::vector<double> om(2 * (size_t)cnt);
        for (int k = 0; k < cnt; ++k) omega_at(ms[k], &om[2 * k]);
        S.sets.emplace_back();
        NodeSet& set = S.sets.back();
        set.first = (int)node_m.size(), set.count = cnt;
        HIP_TRY(set.A.grow(sizeof(double) * 2 * (size_t)n * n * cnt));
        r = upload_omega(c, om.data(), cnt);
        if (r) return r;
        r = reset_fill_counters(c, cnt);
        if (r) return r;
        FillRequest nodes(cnt, c->d_omega, set.A);
        nodes.host_omega = om.data();
        r = fill(c, nodes);
        if (r) return r;
        int k = 0;
        r = collect_fill_status(c, cnt, nullptr, &k);
        if (r == EMME_ENUMERIC) {
            char buf[200];
            snprintf(buf, sizeof buf, "emme_find_roots_in_contour: the fill of the node omega = %.17g%+.17gi failed "
                     "(quadrature depth cap or non-finite integral)", om[2 * k], om[2 * k + 1]);
            set_error(buf);
        }
        if (r) return r;
        for (int m : ms) node_m.push_back(m);
        r = factor_set(S, set, "emme_find_roots_in_contour");
        if (r) return r;
        return solve_set(S, set, 0, L);
    };
    int N = ct->points;
    {
        std::vector<int> ms(N);
        for (int j = 0; j < N; ++j) ms[j] = j * (cap / N);
        rc = add_nodes(ms);
        if (rc) return rc;
    }
    // argument principle on the nodes; N doubles by the midpoints while the count is unresolved
    int W = -1;
    for (;;) {
        std::vector<double> ld(2 * node_m.size());
        // (in order on the context's stream, which may be a non-blocking one: not a null-stream copy)
        HIP_TRY(hipMemcpyAsync(ld.data(), S.logdet, sizeof(double) * ld.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        std::vector<int> ord(node_m.size());
        for (size_t k = 0; k < ord.size(); ++k) ord[k] = (int)k;
        std::sort(ord.begin(), ord.end(), [&](int x, int y) { return node_m[x] < node_m[y]; });
        std::vector<double> args(ord.size());
        for (size_t k = 0; k < ord.size(); ++k) args[k] = ld[2 * ord[k] + 1];
        bool resolved = false;
        const int w = contour_winding(args.data(), N, 0.5 * M_PI, &resolved, nullptr);
        if (resolved) {
            W = w;
            break;
        }
        if (2 * N > cap) break;
        std::vector<int> ms(N);
        for (int j = 0; j < N; ++j) ms[j] = (2 * j + 1) * (cap / (2 * N));
        rc = add_nodes(ms);
        if (rc) return rc;
        N *= 2;
    }
    // Beyn: moments with the trapezoid weights of the final N, L doubled while A0 keeps full numerical rank
    const int nq = (int)node_m.size();
    std::vector<double> wz(4 * (size_t)nq);
    for (int k = 0; k < nq; ++k) {
        const double t = 2.0 * M_PI * node_m[k] / cap;
        // w = omega'(t) / (i N), z = (omega - c) / rho
        const double dre = -ea * std::sin(t), dim_ = eb * std::cos(t);
        wz[4 * k] = dim_ / N, wz[4 * k + 1] = -dre / N;
        wz[4 * k + 2] = ea * std::cos(t) / rho, wz[4 * k + 3] = eb * std::sin(t) / rho;
    }
    std::vector<double> A0(2 * (size_t)n * LCAP), A1(2 * (size_t)n * LCAP), mu(2 * LCAP), sig(LCAP);
    int k = 0;
    for (;;) {
        rc = moments(S, nq, wz, L, A0.data(), A1.data());
        if (rc) return rc;
        rc = emme_contour_eigs(n, L, A0.data(), A1.data(), ct->rank_tol, LCAP, mu.data(), &k, sig.data());
        if (rc) return rc;
        if (std::getenv("EMME_DEBUG")) {
            fprintf(stderr, "[emme] contour N %d L %d k %d W %d sigma:", N, L, k, W);
            for (int l = 0; l < L; ++l) fprintf(stderr, " %.3e", sig[l]);
            fprintf(stderr, "\n");
        }
        if (k < L || L >= LCAP) break;
        const int L2 = std::min(2 * L, LCAP);
        for (const NodeSet& set : S.sets) {
            rc = solve_set(S, set, L, L2 - L);
            if (rc) return rc;
        }
        L = L2;
    }
    // the candidates (normalised radius below 1.5: the others are no eigenvalues inside) seed the Newton search
    std::vector<double> guesses;
    contour_candidates(*ct, k, mu.data(), guesses);
    const int ng = (int)guesses.size() / 2;
    std::vector<ContourRoot> found;
    if (ng > 0) {
        std::vector<double> r(2 * ng), path(2 * (size_t)ng * (step_limit + 1));
        std::vector<int> its(ng), inf(ng);
        rc = emme_solve_roots(c, guesses.data(), ng, tol, step_limit, r.data(), its.data(), inf.data(), path.data());
        if (rc) return rc;
        found = contour_keep_roots(*ct, tol, step_limit, ng, r.data(), its.data(), inf.data(), path.data());
    }
    for (int q = 0; q < std::min((int)found.size(), max_roots); ++q)
        roots[2 * q] = found[q].re, roots[2 * q + 1] = found[q].im, iters[q] = found[q].it, info[q] = found[q].inf;
    *n_roots = (int)found.size();
    *winding = W;
    *points_used = N;
    return EMME_OK;
}

}  // extern "C"
