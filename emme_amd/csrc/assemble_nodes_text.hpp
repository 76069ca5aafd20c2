// assemble_nodes_text.hpp -- the ONE text of the lanes-are-nodes fills that carry neither LIST mode nor the node cache:
// a lane group of 16 (GK15) or 32 (GK31) lanes per (pair, moment) item, lane = node, group_sum, the flattened
// accept / split state machine, blockIdx.y = batch item, the caps EMME_MAX_DEPTH / EMME_MAX_INTERVALS, the `active`
// skip, the interval and status counters.  Two macros select the regions that differ:
//
//   EMME_NODES_DERIV  0: M alone;  1: M and the exact dM/domega of the same discretised integrals -- each
//                     lane also evaluates F' at its node (integrand_d) and the group sums K' beside K and G.  Only K and
//                     G decide accept / split, so the trees, the interval counts and M are the plain kernel's bit for bit.
//   EMME_NODES_SETS   0: ONE parameter set per launch, DevParams by value in the kernel argument, one eta | g | b table;
//                     1: batch item b belongs to set s = set[b] of the sets bound to the context
//                     (emme_ctx_bind_param_sets): its scalars are sets[s], its tables tabs + s * 3N.
//
//   SETS  DERIV   read by                    yields
//    1     0      assemble_sets.hip          k_assemble_sets<PTS>, launch_assemble_sets
//    1     1      assemble_sets_deriv.hip    k_assemble_sets_deriv<PTS>, launch_assemble_sets_deriv
//    0     1      assemble.hip               k_assemble_deriv<PTS>(AsmArgs, Md), where that kernel stood
//    0     0      nobody: k_assemble<PTS, LIST> of assemble.hip keeps its own text, because it also carries LIST mode
//                 and the node-cache reads.  That text is this one's plain reading statement by statement -- a change
//                 to the accept / split rule, the walk or the scatter in one belongs in the other.
//
// Each reading's compiler sees the token stream of a kernel written on its own, so each kernel keeps its own register
// allocation (as assemble_tile_text.hpp).  No fused secant in any reading (a root search takes
// M' with k_secant_copy_sym).
//
// The sets readings are whole translation units: includes, namespaces, argument struct and launcher are under
// EMME_NODES_SETS here.  assemble.hip reads the kernel alone, inside its anonymous namespace, below AsmArgs and
// EMME_ASM_MIN_WAVES.
//
// Sets: s is uniform per workgroup and the set's scalars are read ONCE, before the kernel's first store, into a
// by-value copy: the address is uniform and nothing can have clobbered it, so the compiler reads the struct with scalar
// loads and keeps it in SGPRs, where k_assemble has its kernel argument.  (A reference into `sets` would be read again
// after the stores to M, by vector loads, once per use.)  All sets of a launch share N, nm (whether beta_e == 0), the
// quadrature rule and the pair list (the shape); everything else in DevParams and the tables may differ
// from item to item.
//
// No include guard: a text, not a header of declarations.
#if !defined(EMME_NODES_DERIV) || !defined(EMME_NODES_SETS)
#error "assemble_nodes_text.hpp is read by assemble_sets.hip, assemble_sets_deriv.hip and assemble.hip only, with EMME_NODES_SETS and EMME_NODES_DERIV set"
#endif
#if !EMME_NODES_SETS && !EMME_NODES_DERIV
#error "assemble_nodes_text.hpp has no plain one-set reading: that kernel is k_assemble<PTS, LIST> of assemble.hip"
#endif

#if EMME_NODES_SETS
#include <hip/hip_runtime.h>

#include "assemble_common.hpp"
#include "launch.hpp"
#include "launch_grid.hpp"

namespace emme {

namespace {

#if EMME_NODES_DERIV
struct SetsDerivArgs {
#else
struct SetsArgs {
#endif
    const DevParams* sets;  // [nsets]: the scalars of every bound parameter set
    const double* tabs;     // [nsets][3N]: eta | g | b of every set
    const int* set;         // [nbatch]: the set of every batch item
    const ushort2* pairs;   // (i, j), i < j, ordered by j - i
    int npairs;
    const double2* omega;   // [nbatch]
    const int* active;      // [nbatch] or null: item skipped when 0
    double2* M;             // [nbatch][dim][dim]
#if EMME_NODES_DERIV
    double2* Md;            // [nbatch][dim][dim]
#endif
    unsigned long long* intervals;  // [nbatch], atomically accumulated (may be null)
    int* status;                    // [nbatch], set non-zero on depth-cap / non-finite
};

#ifndef EMME_ASM_MIN_WAVES
#define EMME_ASM_MIN_WAVES 3
#endif
#endif  // EMME_NODES_SETS

template <int PTS>
#if !EMME_NODES_SETS
__global__ __launch_bounds__(256, EMME_ASM_MIN_WAVES) void k_assemble_deriv(AsmArgs A, double2* Md) {
#elif EMME_NODES_DERIV
__global__ __launch_bounds__(256, EMME_ASM_MIN_WAVES) void k_assemble_sets_deriv(SetsDerivArgs A) {
#else
__global__ __launch_bounds__(256, EMME_ASM_MIN_WAVES) void k_assemble_sets(SetsArgs A) {
#endif
    constexpr int GW = PTS == 15 ? 16 : 32;
    constexpr int GROUPS_PER_BLOCK = 256 / GW;
    constexpr int MAXD = EMME_MAX_DEPTH;  // bisection depth the LDS interval stack can hold
    extern __shared__ double lds_tab[];  // eta | g | b  (3N doubles) | per-group (mid, r) stack

#if EMME_NODES_SETS
    const int b = blockIdx.y;
    if (A.active && A.active[b] == 0) return;
    const int s = A.set[b];       // uniform per workgroup
    const DevParams P = A.sets[s];  // by value, before the first store: scalar loads (see the header)
    const int N = P.N, dim = P.dim;

    const double* tab = A.tabs + (size_t)s * 3 * N;
#else
    const DevParams& P = A.P;
    const int b = blockIdx.y;
    if (A.active && A.active[b] == 0) return;
    const int N = P.N, dim = P.dim;

    const double* tab = A.tab;
#endif
    for (int k = threadIdx.x; k < 3 * N; k += blockDim.x) lds_tab[k] = tab[k];
    __syncthreads();
    const double* eta = lds_tab;
    const double* gtab = lds_tab + N;
    const double* btab = lds_tab + 2 * N;
    // (mid, r) of every split ancestor of the current interval, one stack per lane group.  All lanes of a group store
    // the same value to the same slot and later read it back, so plain per-thread program order is enough
    double2* stk = reinterpret_cast<double2*>(lds_tab + 3 * N + (3 * N & 1)) + (threadIdx.x / GW) * MAXD;

    double2* Mb = A.M + (size_t)b * dim * dim;
#if !EMME_NODES_SETS  // (Mdb here, before omega is read, in this reading and below it in the other: DESIGN.md 12.2.2)
    double2* Mdb = Md + (size_t)b * dim * dim;
#endif
    OmegaConst oc;
    oc.omega = mk(A.omega[b].x, A.omega[b].y);
    oc.omi = -copysign(1.0, oc.omega.x);
    const cd zero = mk(0.0, 0.0);
#if EMME_NODES_DERIV
#if EMME_NODES_SETS
    double2* Mdb = A.Md + (size_t)b * dim * dim;
#endif
    // an entry of M and the same entry of M'
    auto store = [&](int r, int c, cd v, cd vd) {
        store_entry_twin(Mb, Mdb, (size_t)r * dim + c, v, vd);
    };
#else
    auto store = [&](int r, int c, cd v) {
        store_entry_secant(Mb, nullptr, nullptr, zero, (size_t)r * dim + c, v);
    };
#endif

    // diagonal (include/solver.h:442-443, 465-470): block 0 of each batch item; constant in omega, so 0 in M'
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < N; i += blockDim.x) {
#if EMME_NODES_DERIV
            store(i, i, mk(P.diag_a, 0.0), zero);
            if (P.nm == 3) {
                store(i, i + N, zero, zero);
                store(i + N, i, zero, zero);
                store(i + N, i + N, mk(P.diag_d * btab[i], 0.0), zero);
            }
#else
            store(i, i, mk(P.diag_a, 0.0));
            if (P.nm == 3) {
                store(i, i + N, zero);
                store(i + N, i, zero);
                store(i + N, i + N, mk(P.diag_d * btab[i], 0.0));
            }
#endif
        }
    }

    const int lane_in_group = threadIdx.x % GW;
    const int group = blockIdx.x * GROUPS_PER_BLOCK + threadIdx.x / GW;
    const int ngroups = gridDim.x * GROUPS_PER_BLOCK;
    const GkLane gk = gk_lane<PTS>(lane_in_group);

    const double qa = 0.0, qb = M_PI / 2.0;  // include/functions.h:319 / :328
    const double inv_scale = 2. / (qb - qa);
    const int nitems = A.npairs * P.nm;

    // ---- group state ------------------------------------------------------------
    int item = group;
    bool live = item < nitems;
    int i = 0, j = 0, m = 0;
    PairConst pc{};
    double dg = 0.0;
    int depth = 0;
    unsigned long long path = 0;  // index of the current interval at this depth
    double l = qa, r = qb;        // the current interval
    double abs_tol = 0.0;
    cd sum = zero;
#if EMME_NODES_DERIV
    cd sum_d = zero;  // accepted intervals' scale * K'
#endif
    unsigned long long my_intervals = 0;
    int item_intervals = 0;  // safety valve: no integral may run away (every wave must exit)
    int bad = 0;

    auto load_item = [&]() {
        const int p = item / P.nm;
        m = item - p * P.nm;
        const ushort2 ij = A.pairs[p];
        i = ij.x, j = ij.y;
        dg = gtab[i] - gtab[j];
        pc = make_pair_const(P, eta[i], eta[j], btab[i], btab[j], dg);
        depth = 0, path = 0, abs_tol = 0.0;
        l = qa, r = qb;
        item_intervals = 0;
        sum = zero;
#if EMME_NODES_DERIV
        sum_d = zero;
#endif
    };
    if (live) load_item();

    while (live) {
        const double mid = (r + l) / 2;
        const double scale = (r - l) / 2;
        // abscissa scale * x + mid, rounded like the reference (no FMA contraction)
        const double x = __dadd_rn(__dmul_rn(scale, gk.x), mid);

#if EMME_NODES_DERIV
        cd fd;
        const cd f = integrand_d(x, P, pc, oc, m, fd);
#else
        const cd f = integrand(x, P, pc, oc, m);
#endif
        const double Kx = group_sum<GW>(gk.wk * f.x), Ky = group_sum<GW>(gk.wk * f.y);
        const double Gx = group_sum<GW>(gk.wg * f.x), Gy = group_sum<GW>(gk.wg * f.y);
#if EMME_NODES_DERIV
        const double Kdx = group_sum<GW>(gk.wk * fd.x), Kdy = group_sum<GW>(gk.wk * fd.y);
#endif
        ++my_intervals;
        ++item_intervals;

        // (the derivative kernels: the plain kernel's rule, on K and G alone)
        const cd integral = mk(Kx * scale, Ky * scale);
        bool split = gk_split(mk(Kx, Ky), mk(Gx, Gy), scale, inv_scale, depth, P, abs_tol);
        if (split && (depth >= MAXD || item_intervals >= EMME_MAX_INTERVALS)) {  // flag and accept
            split = false;
            bad = 1;
        }
        if (split) {
            // left half first (the reference pushes [mid,r] then [l,mid]); remember the
            // right half's bounds for when the walk comes back up
            stk[depth] = make_double2(mid, r);
            r = mid;
            ++depth;
            path <<= 1;
        } else {
            sum = sum + integral;
#if EMME_NODES_DERIV
            sum_d = sum_d + mk(Kdx * scale, Kdy * scale);
#endif
            ++path;
            while (depth > 0 && !(path & 1)) {
                path >>= 1;
                --depth;
            }
            if (depth == 0) {
                // integral finished: kappa = -i pref sum (src/Parameters.cpp:182-183)
                cd kap = mk(P.pref * sum.y, -(P.pref * sum.x));
                if (kappa_bad(kap)) bad = 1;
                kap = kap + kappa_e(m, P, pc.de, dg, oc.omega);
#if EMME_NODES_DERIV
                // kappa' = -i pref sum' + kappa_e', scattered like kappa
                cd kd = mk(P.pref * sum_d.y, -(P.pref * sum_d.x));
                if (kappa_bad(kd)) bad = 1;
                kd = kd + kappa_e_d(m, P, pc.de, dg, oc.omega);
                if (lane_in_group == 0) {
                    if (m == 0) {
                        const double w = -(pair_weight(i, j, N) * P.dx);
                        const cd v = w * kap, vd = w * kd;
                        store(i, j, v, vd);
                        store(j, i, v, vd);
                    } else if (m == 1) {
                        const cd v = P.dx * kap, vd = P.dx * kd;
                        store(i, j + N, v, vd);
                        store(j, i + N, -v, -vd);
                        store(i + N, j, -v, -vd);
                        store(j + N, i, v, vd);
                    } else {
                        const cd v = P.dx * kap, vd = P.dx * kd;
                        store(i + N, j + N, v, vd);
                        store(j + N, i + N, v, vd);
                    }
                }
#else
                if (lane_in_group == 0) {
                    if (m == 0) {
                        // A_ij = -kappa_all(0) W_ij dx (include/solver.h:448-453)
                        const double w = pair_weight(i, j, N);
                        const cd v = (-(w * P.dx)) * kap;
                        store(i, j, v);
                        store(j, i, v);
                    } else if (m == 1) {
                        // B block and its mirrors (include/solver.h:480-504)
                        const cd v = P.dx * kap;
                        store(i, j + N, v);
                        store(j, i + N, -v);
                        store(i + N, j, -v);
                        store(j + N, i, v);
                    } else {
                        const cd v = P.dx * kap;
                        store(i + N, j + N, v);
                        store(j + N, i + N, v);
                    }
                }
#endif
                item += ngroups;
                live = item < nitems;
                if (live) load_item();
            } else {
                // right sibling of the ancestor that was split at depth-1
                const double2 pr = stk[depth - 1];
                l = pr.x;
                r = pr.y;
            }
        }
    }

    if (lane_in_group == 0) {
        if (A.intervals && my_intervals) atomicAdd(&A.intervals[b], my_intervals);
        if (bad) A.status[b] = 1;
    }
}

#if EMME_NODES_SETS
}  // namespace

// L describes the batch as for launch_assemble (L.P: the context's own set, read for the shape -- N, nm -- only; L.tab
// is not read); sets / tabs / set are device arrays (see the argument struct).  The grid, the block and the LDS are
// launch_assemble's.
#if EMME_NODES_DERIV
hipError_t launch_assemble_sets_deriv(const AssembleLaunch& L, const DevParams* sets, const double* tabs, const int* set,
                                      hipStream_t stream) {
    if (!L.Md || L.Mold) return hipErrorInvalidValue;  // (no fused secant)
    SetsDerivArgs A;
    A.Md = (double2*)L.Md;
#else
hipError_t launch_assemble_sets(const AssembleLaunch& L, const DevParams* sets, const double* tabs, const int* set,
                                hipStream_t stream) {
    if (L.Md) return hipErrorNotSupported;
    if (L.Mold) return hipErrorInvalidValue;  // (no fused secant)
    SetsArgs A;
#endif
    if (!sets || !tabs || !set) return hipErrorInvalidValue;
    A.sets = sets;
    A.tabs = tabs;
    A.set = set;
    A.pairs = (const ushort2*)L.pairs;
    A.npairs = L.npairs;
    A.omega = (const double2*)L.omega;
    A.active = L.active;
    A.M = (double2*)L.M;
    A.intervals = L.intervals;
    A.status = L.status;
    const int groups_per_block = 256 / (L.gk_points == 15 ? 16 : 32);
    const long nitems = (long)L.npairs * L.P.nm;
    dim3 grid(lane_group_grid_x(nitems, L.items_per_group, groups_per_block), (unsigned)L.nbatch), block(256);
    const size_t lds = tables_stack_lds_bytes(L.P.N, groups_per_block);
#if EMME_NODES_DERIV
    if (L.gk_points == 15)
        hipLaunchKernelGGL((k_assemble_sets_deriv<15>), grid, block, lds, stream, A);
    else
        hipLaunchKernelGGL((k_assemble_sets_deriv<31>), grid, block, lds, stream, A);
#else
    if (L.gk_points == 15)
        hipLaunchKernelGGL((k_assemble_sets<15>), grid, block, lds, stream, A);
    else
        hipLaunchKernelGGL((k_assemble_sets<31>), grid, block, lds, stream, A);
#endif
    return hipGetLastError();
}

}  // namespace emme
#endif  // EMME_NODES_SETS
