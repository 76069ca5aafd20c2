// contour.hip -- the device half of the contour eigensolver and its C entry points: the moments
// of caller matrices (emme_contour_moments_batch, emme_contour_moments_groups) and the region search (every root inside
// an ellipse: Beyn's method, W.-J. Beyn, Linear Algebra Appl. 436 (2012) 3839-3863, seeded into the Newton search) on
// one contour (emme_find_roots_in_contour) or on many (parameter set, contour) items at once
// (emme_find_roots_in_contours_sets); emme_find_eigenpairs_in_contour and emme_find_eigenpairs_in_contours_sets are the
// same searches returning every root with its eigenvector and residual.
//
// The nodes' matrices are factored once by the nullSpace factorisation (lu_factor_batch: P M = L U in place, row
// order in panel snapshots) and kept for the whole call.  Three small kernels read the factors:
//   k_contour_solve    X = M^-1 V for a group of G right-hand sides per workgroup, the matrices of a launch from a
//                      list, each with its own column range: permute, then forward (L) and back (U) substitution in
//                      blocks of 16 rows -- the rows' coupling to every finished block in dot form (a wave per row,
//                      rows are contiguous), then the block's 16 x 16 triangle with 16 lanes per column (a row each,
//                      the solved unknown broadcast by a shuffle), coefficients in LDS;
//   k_contour_logdet   log det M = sum log u_ii + i pi (parity of the row order), fixed-order reductions;
//   k_contour_moments_groups  A0 = sum_j w_j X_j, A1 = sum_j w_j z_j X_j per group of nodes: a thread per entry, a
//                      group's nodes summed in order (no atomics: two calls on the same inputs are bit-identical).
// The probes V come from a counter-based hash of (row, column) with a fixed seed (k_contour_probes), so that the
// first L columns do not depend on L and doubling L solves only the new ones.
// Both searches are search_contours, which walks the round plan of host_contour.cpp (ContourRounds) with one fill, one
// factorisation, one log-det and one solve launch per node round and takes the moments per item; the search on one
// contour is its one-item case without a parameter set.
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

// Matrix q of a solve launch is any factored matrix of the call, with its own column range: when one
// item of a search doubles L, only its nodes get the new columns.  The matrices of a call live in one buffer per node
// round, so an entry carries the matrix's own pointers.
struct SolveItem {
    const double2* A;    // [n][n]  P M = L U in place
    const int* maps;     // [nblk][n]
    const int* lu_info;  // its info
    double2* X;          // [n][ldx]
    int map_nb, l0, nl;  // rows per row-order snapshot; columns l0 .. l0 + nl - 1 of V and X
};

struct SolveArgs {
    int n;
    const double2* V;       // [n][ldv] probes
    int ldv, ldx, nl;       // nl: the widest column range of the list
    const SolveItem* list;  // one entry per workgroup row of the grid
};

// one workgroup per (matrix, group of G columns): the matrix and columns of P.list[blockIdx.x]
template <int G>
__global__ __launch_bounds__(CT) void k_contour_solve(SolveArgs P) {
    extern __shared__ double2 sm[];
    const int n = P.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SolveItem it = P.list[blockIdx.x];
    const int l0 = it.l0, nl = it.nl, map_nb = it.map_nb;
    double2* out = it.X;
    const double2* a = it.A;
    const int* maps = it.maps;
    const int* lu_info = it.lu_info;
    if ((int)blockIdx.y * G >= nl) return;  // (the grid is as deep as the widest range of the list)
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

// A0[i][l] = sum_j w_j X_j[i][l], A1[i][l] = sum_j w_j z_j X_j[i][l] per group: group g (blockIdx.y)
// sums the nodes idx[off[g]] .. idx[off[g + 1] - 1] in that order, with its own column count Ls[g] (null: L for every
// group), into A0 / A1 + g * ostride.  A thread per (group, entry), consecutive threads on consecutive l of a row of X;
// no atomics, so two calls on the same inputs are bit-identical and a group's sum does not depend on the other groups.
// Xn[node]: the node's X ([n][ldx]); wz[2 node], wz[2 node + 1]: its w and z; info (nullable): nodes with info != 0 are
// left out.
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

template <int G>
hipError_t launch_solve_g(const SolveArgs& P, int nmat, hipStream_t st) {
    const size_t lds = solve_lds(P.n, G);
    if (lds > 150 * 1024) return hipErrorNotSupported;
    if (lds > 48 * 1024) {
        const hipError_t ea = hipFuncSetAttribute((const void*)k_contour_solve<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ea != hipSuccess) return ea;
    }
    hipLaunchKernelGGL((k_contour_solve<G>), dim3(nmat, (P.nl + G - 1) / G), dim3(CT), lds, st, P);
    return hipGetLastError();
}

// the nmat entries of P.list, P.nl the widest of their column ranges
hipError_t launch_contour_solve(const SolveArgs& P, int nmat, int n_cu, hipStream_t st) {
    switch (solve_group(P.n, P.nl, nmat, n_cu)) {
        case 16: return launch_solve_g<16>(P, nmat, st);
        case 8: return launch_solve_g<8>(P, nmat, st);
        case 4: return launch_solve_g<4>(P, nmat, st);
        case 2: return launch_solve_g<2>(P, nmat, st);
        default: return launch_solve_g<1>(P, nmat, st);
    }
}

// the right-hand sides of a call: the internal probes, or a caller's V
struct Probes {
    DeviceBuffer<double> V;
    int ld = LCAP;
};

int make_probes(emme_ctx* c, int n, Probes& pr) {
    HIP_TRY(pr.V.grow(sizeof(double) * 2 * (size_t)n * LCAP));
    pr.ld = LCAP;
    hipLaunchKernelGGL(k_contour_probes, dim3((n * LCAP + 255) / 256), dim3(256), 0, c->stream, n, (double2*)pr.V.get());
    HIP_TRY(hipGetLastError());
    return EMME_OK;
}

// `count` matrices factored in one batch and what the call keeps of each: the factors, their own copy of the row order
// (the factorisation's scratch is reused), X, log det and info.  One device allocation holds all five: a call frees as
// many buffers as it has node rounds, and a region search on a context of its own (create, search, destroy) is as
// fast as it was with one buffer set per call (five allocations per round cost it 5 % at n = 64)
struct ContourState {
    emme_ctx* c = nullptr;
    int n = 0, count = 0, ldx = 0, map_nb = 1;
    DeviceBuffer<char> mem;  // A | X | logdet | maps | info
    double *A = nullptr, *X = nullptr, *logdet = nullptr;
    int *maps = nullptr, *info = nullptr;
    // matrix q with the columns [l0, l0 + nl)
    SolveItem item(int q, int l0, int nl) const {
        const size_t per_map = (size_t)n * ((n + map_nb - 1) / map_nb);
        SolveItem e{};
        e.A = (const double2*)A + (size_t)n * n * q, e.maps = maps + per_map * q, e.lu_info = info + q;
        e.X = (double2*)X + (size_t)q * n * ldx, e.map_nb = map_nb, e.l0 = l0, e.nl = nl;
        return e;
    }
};

int alloc_nodes(ContourState& S, emme_ctx* c, int n, int count, int ldx) {
    S.c = c, S.n = n, S.count = count, S.ldx = ldx;
    const size_t nA = 2 * (size_t)n * n * count, nX = 2 * (size_t)count * n * ldx, nld = 2 * (size_t)count;
    // (the row order of the unblocked LU has one snapshot; the most any branch writes is one per trace_solve_nb() rows)
    const size_t nmaps = (size_t)n * ((n + trace_solve_nb() - 1) / trace_solve_nb()) * count;
    HIP_TRY(S.mem.grow(sizeof(double) * (nA + nX + nld) + sizeof(int) * (nmaps + count)));
    S.A = (double*)S.mem.get(), S.X = S.A + nA, S.logdet = S.X + nX;
    S.maps = (int*)(S.logdet + nld), S.info = S.maps + nmaps;
    return EMME_OK;
}

// factor S.A in place, keep the row order and info, log det
int factor_nodes(ContourState& S, const char* who) {
    emme_ctx* c = S.c;
    const int n = S.n;
    LuScratch scr;
    int map_nb = 1;
    const int rc = lu_factor_batch(c, n, S.count, S.A, scr, who,
                                   [&](int b0, int nb, const int* maps, int mnb, const int* lu_info) -> hipError_t {
                                       map_nb = mnb;
                                       const size_t per = (size_t)n * ((n + mnb - 1) / mnb);
                                       hipError_t e = hipMemcpyAsync(S.maps + per * b0, maps, sizeof(int) * per * nb,
                                                                     hipMemcpyDeviceToDevice, c->stream);
                                       if (e == hipSuccess)
                                           e = hipMemcpyAsync(S.info + b0, lu_info, sizeof(int) * nb, hipMemcpyDeviceToDevice,
                                                              c->stream);
                                       return e;
                                   });
    if (rc) return rc;
    S.map_nb = map_nb;
    ScopedSpan sp(c, K_OTHER);
    hipLaunchKernelGGL(k_contour_logdet, dim3(S.count), dim3(CT), 2 * sizeof(int) * n, c->stream, n,
                       (const double2*)S.A, S.maps, map_nb, (n + map_nb - 1) / map_nb, S.info,
                       (double2*)S.logdet);
    HIP_TRY(hipGetLastError());
    return EMME_OK;
}

// one solve launch for the entries of `list` (X of every entry [n][ldx])
int solve_listed(emme_ctx* c, int n, const Probes& pr, int ldx, const std::vector<SolveItem>& list,
                 DeviceBuffer<SolveItem>& d_list) {
    if (list.empty()) return EMME_OK;
    HIP_TRY(d_list.grow(sizeof(SolveItem) * list.size()));
    HIP_TRY(hipMemcpyAsync(d_list, list.data(), sizeof(SolveItem) * list.size(), hipMemcpyHostToDevice, c->stream));
    SolveArgs P{};
    P.n = n, P.V = (const double2*)pr.V.get(), P.ldv = pr.ld, P.ldx = ldx, P.list = d_list;
    for (const SolveItem& it : list) P.nl = std::max(P.nl, it.nl);
    ScopedSpan sp(c, K_OTHER);
    HIP_TRY(launch_contour_solve(P, (int)list.size(), c->n_cu, c->stream));
    return EMME_OK;
}

// device images of the lists of a moments launch, and its sums
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

// What emme_contour_moments_groups and emme_contour_moments_batch (group null: every matrix in group 0) are: caller
// matrices M (nq of order n, host or device) factored, log det taken, X = M^-1 V solved for L columns (V null: the
// internal probes) and summed per group, ascending j inside a group; a matrix with info != 0 is left out on the device
int caller_moments(emme_ctx* c, const char* who, int n, int nq, const double* M, const int* group, int ngroups,
                   const double* z, const double* w, int L, const double* V, double* A0, double* A1, double* logdet,
                   int* info) {
    HIP_TRY(hipSetDevice(c->device));
    EMME_TRY(ensure_batch(c, nq));
    Probes pr;
    if (V) {
        HIP_TRY(pr.V.grow(sizeof(double) * 2 * (size_t)n * L));
        pr.ld = L;
        HIP_TRY(hipMemcpyAsync(pr.V, V, sizeof(double) * 2 * (size_t)n * L,
                               is_device_ptr(V) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    } else {
        EMME_TRY(make_probes(c, n, pr));
    }
    ContourState S;
    EMME_TRY(alloc_nodes(S, c, n, nq, L));
    HIP_TRY(hipMemcpyAsync(S.A, M, sizeof(double) * 2 * (size_t)n * n * nq,
                           is_device_ptr(M) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    EMME_TRY(factor_nodes(S, who));
    std::vector<SolveItem> list(nq);
    std::vector<const double2*> Xn(nq);
    std::vector<double> wz(4 * (size_t)nq);
    std::vector<int> off(ngroups + 1, 0), idx(nq);
    for (int j = 0; j < nq; ++j) {
        list[j] = S.item(j, 0, L), Xn[j] = list[j].X;
        wz[4 * j] = w[2 * j], wz[4 * j + 1] = w[2 * j + 1], wz[4 * j + 2] = z[2 * j], wz[4 * j + 3] = z[2 * j + 1];
        ++off[(group ? group[j] : 0) + 1];
    }
    DeviceBuffer<SolveItem> d_list;
    EMME_TRY(solve_listed(c, n, pr, L, list, d_list));
    for (int g = 0; g < ngroups; ++g) off[g + 1] += off[g];
    std::vector<int> at(off.begin(), off.end() - 1);
    for (int j = 0; j < nq; ++j) idx[at[group ? group[j] : 0]++] = j;
    GroupBuffers G;
    EMME_TRY(moments_groups(c, n, L, nullptr, off, idx, Xn, L, wz, S.info, G, (size_t)n * L, A0, A1));
    HIP_TRY(hipMemcpyAsync(logdet, S.logdet, sizeof(double) * 2 * nq, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(info, S.info, sizeof(int) * nq, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EMME_OK;
}

// where a region search puts what it found: item k's roots at roots[k max_roots ..], one of everything else per item
// vecs / resid (both or neither): the search returns eigenpairs -- item k's unit vectors at vecs[k max_roots dim ..],
// their residuals at resid[k max_roots ..]
struct SearchOutputs {
    double* roots;
    int *iters, *info, *n_roots, *winding, *points_used, *status;
    double *vecs = nullptr, *resid = nullptr;
};

// The region search on nitems (set, contour) items in lock step: the round plan of host_contour.cpp
// (ContourRounds) with one fill, one factorisation, one log-det and one solve launch per node round, moment passes
// while L doubles, one polish.  set null is the single search of emme_find_roots_in_contour, one item
// on the context's own parameters: its fills carry no set (so they may go through the node cache), its polish is
// emme_solve_roots with the context's method (`exact` is not read), and an error of the item is the call's error,
// named without an item number.
// With out.vecs (emme_find_eigenpairs_in_contour, emme_find_eigenpairs_in_contours_sets) only the last stage differs:
// the Beyn step of the final L pass keeps the eigenvector v_c = U_k y_c beside every mu_c (emme_contour_eigpairs: mu, k
// and sigma are emme_contour_eigs' bit for bit, so nodes, counts and L passes are the same), the candidates carry
// them, and the polish is an eigenpair search started from them -- exact = 0: emme_solve_eigenpairs_secant (plain
// fills only), exact = 1: emme_solve_eigenpairs -- with or without sets; every kept root comes back with its unit
// vector and its residual.
int search_contours(emme_ctx* c, const std::string& who, int nitems, const int* set, const emme_contour_t* contours,
                    int exact, double tol, int step_limit, int max_roots, const SearchOutputs& out) {
    const int n = c->dim;
    if (n > 2048) {
        set_error(who + ": dim above 2048 is not supported (the factorisation's range)");
        return EMME_ECONFIG;
    }
    HIP_TRY(hipSetDevice(c->device));
    ContourRounds plan(nitems, set, contours);
    Probes probes;  // (every item reads the same probes)
    EMME_TRY(make_probes(c, n, probes));
    std::vector<ContourState> rounds;    // the nodes of a node round: factors, X, log det, info
    std::vector<SolveItem> node;         // every node's factors and X, columns unset
    std::vector<const double2*> Xn;
    std::vector<double> ld;              // log det and info of every node, by node
    std::vector<int> h_info;
    std::vector<SolveItem> list;
    DeviceBuffer<SolveItem> d_list;
    std::string first_error;
    auto label = [&](int item) { return set ? who + ": item " + std::to_string(item) + ": " : who + ": "; };
    auto drop = [&](int item, int rc, const std::string& msg) {
        plan.drop(item, rc);
        if (first_error.empty()) first_error = msg;
    };
    // ---- node rounds: one fill, one factorisation, one log-det and one solve launch for the new nodes of all items
    while (plan.plan_nodes()) {
        const int cnt = (int)plan.r_item.size(), first = plan.r_first;
        EMME_TRY(ensure_batch(c, cnt));
        rounds.emplace_back();
        ContourState& S = rounds.back();
        EMME_TRY(alloc_nodes(S, c, n, cnt, LCAP));
        const size_t msize = 2 * (size_t)n * n;
        EMME_TRY(upload_omega(c, plan.r_omega.data(), cnt));
        EMME_TRY(reset_fill_counters(c, cnt));
        FillRequest rq(cnt, c->d_omega, S.A);
        rq.host_omega = plan.r_omega.data();
        rq.may_mirror = false;  // (a context whose first cached call is a region search keeps the full pair list)
        if (set) {
            EMME_TRY(upload_set_indices(c, plan.r_set.data(), cnt));
            rq.d_set = c->d_set, rq.host_set = plan.r_set.data();
        }
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
            drop(plan.r_item[q], EMME_ENUMERIC, label(plan.r_item[q]) + buf);
            HIP_TRY(hipMemsetAsync(S.A + msize * q, 0, sizeof(double) * msize, c->stream));
        }
        EMME_TRY(factor_nodes(S, who.c_str()));
        list.clear();
        for (int q = 0; q < cnt; ++q) {
            const ContourRounds::Item& it = plan.items[plan.r_item[q]];
            node.push_back(S.item(q, 0, it.L)), Xn.push_back(node.back().X);
            if (!it.dropped) list.push_back(node.back());
        }
        EMME_TRY(solve_listed(c, n, probes, LCAP, list, d_list));
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
    const bool pairs = out.vecs != nullptr;
    std::vector<double> beyn;                        // (pairs) the vectors of one Beyn step, min(k, LCAP) rows of n
    std::vector<std::vector<double>> seeds(nitems);  // ... and those of an item's candidates, in the candidates' order
    std::vector<int> kept;
    if (pairs) beyn.resize(2 * (size_t)n * LCAP);
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
            const int rc = pairs ? emme_contour_eigpairs(n, Ls[g], &A0[2 * ostride * g], &A1[2 * ostride * g], ct.rank_tol, LCAP,
                                                         mu.data(), beyn.data(), &k, sig.data())
                                 : emme_contour_eigs(n, Ls[g], &A0[2 * ostride * g], &A1[2 * ostride * g], ct.rank_tol, LCAP,
                                                     mu.data(), &k, sig.data());
            if (rc) {
                drop(item, rc, set ? label(item) + emme_last_error() : emme_last_error());
                continue;
            }
            if (std::getenv("EMME_DEBUG")) {
                fprintf(stderr, "[emme] contour item %d N %d L %d k %d W %d sigma:", item, plan.items[item].N, Ls[g], k,
                        plan.items[item].W);
                for (int l = 0; l < Ls[g]; ++l) fprintf(stderr, " %.3e", sig[l]);
                fprintf(stderr, "\n");
            }
            if (!plan.take_rank(item, k, &l0, &nl)) {
                // the candidates (normalised radius below 1.5: the others are no eigenvalues inside)
                kept.clear();
                contour_candidates(ct, k, mu.data(), guesses[item], &kept);
                if (pairs)
                    for (int q : kept) seeds[item].insert(seeds[item].end(), &beyn[2 * (size_t)q * n], &beyn[2 * (size_t)(q + 1) * n]);
                continue;
            }
            for (int nd : plan.items[item].nodes) {
                SolveItem e = node[nd];
                e.l0 = l0, e.nl = nl;
                list.push_back(e);
            }
        }
        EMME_TRY(solve_listed(c, n, probes, LCAP, list, d_list));
    }
    // ---- one search polishes the candidates of all items: items in order, an item's in the order of mu
    std::vector<double> g_all, v_all;
    std::vector<int> g_set, g_first(nitems + 1, 0);
    for (int k = 0; k < nitems; ++k) {
        if (!plan.items[k].dropped) {
            g_all.insert(g_all.end(), guesses[k].begin(), guesses[k].end());
            g_set.insert(g_set.end(), guesses[k].size() / 2, plan.items[k].set);
            v_all.insert(v_all.end(), seeds[k].begin(), seeds[k].end());
        }
        g_first[k + 1] = (int)g_set.size();
    }
    const int ng = (int)g_set.size();
    std::vector<double> r(2 * (size_t)ng), path(2 * (size_t)ng * (step_limit + 1));
    std::vector<int> its(ng), inf(ng);
    std::vector<double> vec, res;  // (pairs) the polished chains' vectors and residuals
    if (ng > 0 && pairs) {
        vec.resize(2 * (size_t)ng * n), res.resize(ng);
        const int* st = set ? g_set.data() : nullptr;
        EMME_TRY(exact ? emme_solve_eigenpairs(c, st, g_all.data(), ng, v_all.data(), tol, step_limit, r.data(), vec.data(),
                                               res.data(), its.data(), inf.data(), path.data())
                       : emme_solve_eigenpairs_secant(c, st, g_all.data(), ng, v_all.data(), tol, step_limit, r.data(),
                                                      vec.data(), res.data(), its.data(), inf.data(), path.data()));
        // The one rule this form adds: a chain can stop on its step without M being singular ("chains
        // that stop without a root"; from a spurious candidate's vector the secant polish does, with residuals of
        // 5e-4 .. 7e-4 where roots have 1e-11 or less).  The root form cannot see that; here the residual tells, and
        // what is no eigenpair to sqrt(eps) is dropped like a chain that failed.
        for (int q = 0; q < ng; ++q)
            if (inf[q] == 0 && !(res[q] <= 1e-8)) inf[q] = EMME_ENUMERIC;
    } else if (ng > 0)
        EMME_TRY(set ? emme_solve_roots_sets(c, g_set.data(), g_all.data(), ng, exact, tol, step_limit, r.data(), its.data(),
                                             inf.data(), path.data())
                     : emme_solve_roots(c, g_all.data(), ng, tol, step_limit, r.data(), its.data(), inf.data(), path.data()));
    else if (set)
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
            out.roots[2 * at] = found[q].re, out.roots[2 * at + 1] = found[q].im, out.iters[at] = found[q].it,
                           out.info[at] = found[q].inf;
            if (pairs) {
                const size_t chain = (size_t)o + found[q].chain;
                std::copy(&vec[2 * chain * n], &vec[2 * (chain + 1) * n], out.vecs + 2 * at * n);
                out.resid[at] = res[chain];
            }
        }
        out.n_roots[k] = (int)found.size(), out.winding[k] = it.W, out.points_used[k] = it.N, out.status[k] = it.status;
    }
    if (!first_error.empty()) set_error(first_error);
    return EMME_OK;
}

}  // namespace
}  // namespace emme

using namespace emme;

namespace {

// The argument rules of the region searches, all before the device is looked for; pairs: the eigenpair forms, which
// need vecs and resid as well
int region_search_sets(emme_ctx* c, const std::string& who, bool pairs, int nitems, const int* set,
                       const emme_contour_t* contours, int exact, double tol, int step_limit, int max_roots,
                       const SearchOutputs& out) {
    if (nitems < 1 || nitems > 65535) {
        set_error(who + ": nitems must lie in 1 .. 65535");
        return EMME_EINVAL;
    }
    if (!c || !set || !contours || !out.roots || !out.iters || !out.info || !out.n_roots || !out.winding || !out.points_used ||
        !out.status || (pairs && (!out.vecs || !out.resid)) || max_roots < 1 || step_limit < 0 || !(tol > 0.0)) {
        set_error(who + ": need a context, sets, contours, tol > 0, step_limit >= 0, max_roots >= 1 and every output");
        return EMME_EINVAL;
    }
    for (int k = 0; k < nitems; ++k)
        if (const char* bad = contour_arg_error(&contours[k])) {
            set_error(who + ": item " + std::to_string(k) + ": " + bad);
            return EMME_EINVAL;
        }
    EMME_TRY(check_set_indices(c, set, nitems, who.c_str()));
    return search_contours(c, who, nitems, set, contours, exact, tol, step_limit, max_roots, out);
}

int region_search_one(emme_ctx* c, const std::string& who, bool pairs, const emme_contour_t* ct, int exact, double tol,
                      int step_limit, int max_roots, SearchOutputs out) {
    if (!c || !ct || !out.roots || !out.iters || !out.info || !out.n_roots || !out.winding || !out.points_used ||
        (pairs && (!out.vecs || !out.resid)) || max_roots < 1 || step_limit < 0 || !(tol > 0.0)) {
        set_error(who + ": need a context, a contour, tol > 0, step_limit >= 0, max_roots >= 1 and every output");
        return EMME_EINVAL;
    }
    if (const char* bad = contour_arg_error(ct)) {
        set_error(who + ": " + bad);
        return EMME_EINVAL;
    }
    // one item on the context's own parameters; what takes the item out of the search is the call's error
    int status = EMME_OK;
    out.status = &status;
    const int rc = search_contours(c, who, 1, nullptr, ct, exact, tol, step_limit, max_roots, out);
    return rc ? rc : status;
}

}  // namespace

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
    return caller_moments(c, "emme_contour_moments_batch", n, nq, M, nullptr, 1, z, w, L, V, A0, A1, logdet, info);
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
    return caller_moments(c, "emme_contour_moments_groups", n, nq, M, group, ngroups, z, w, L, V, A0, A1, logdet, info);
}

int emme_find_roots_in_contours_sets(emme_ctx_t* c, int nitems, const int* set, const emme_contour_t* contours, int exact,
                                     double tol, int step_limit, int max_roots, double* roots, int* iters, int* info,
                                     int* n_roots, int* winding, int* points_used, int* status) {
    return region_search_sets(c, "emme_find_roots_in_contours_sets", false, nitems, set, contours, exact, tol, step_limit,
                              max_roots, {roots, iters, info, n_roots, winding, points_used, status});
}

int emme_find_roots_in_contour(emme_ctx_t* c, const emme_contour_t* ct, double tol, int step_limit, int max_roots,
                               double* roots, int* iters, int* info, int* n_roots, int* winding, int* points_used) {
    return region_search_one(c, "emme_find_roots_in_contour", false, ct, 0, tol, step_limit, max_roots,
                             {roots, iters, info, n_roots, winding, points_used, nullptr});
}

int emme_find_eigenpairs_in_contours_sets(emme_ctx_t* c, int nitems, const int* set, const emme_contour_t* contours,
                                          int exact, double tol, int step_limit, int max_roots, double* roots, double* vecs,
                                          double* resid, int* iters, int* info, int* n_roots, int* winding, int* points_used,
                                          int* status) {
    return region_search_sets(c, "emme_find_eigenpairs_in_contours_sets", true, nitems, set, contours, exact, tol, step_limit,
                              max_roots, {roots, iters, info, n_roots, winding, points_used, status, vecs, resid});
}

int emme_find_eigenpairs_in_contour(emme_ctx_t* c, const emme_contour_t* ct, int exact, double tol, int step_limit,
                                    int max_roots, double* roots, double* vecs, double* resid, int* iters, int* info,
                                    int* n_roots, int* winding, int* points_used) {
    return region_search_one(c, "emme_find_eigenpairs_in_contour", true, ct, exact, tol, step_limit, max_roots,
                             {roots, iters, info, n_roots, winding, points_used, nullptr, vecs, resid});
}

}  // extern "C"
