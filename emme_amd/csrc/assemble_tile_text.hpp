// assemble_tile_text.hpp -- the ONE text of the table-free tile fill for electrostatic GK15 batches that have no node
// cache, compiled once per translation unit: assemble_tile.hip sets EMME_TILE_DERIV to 0 and gets k_assemble_tile
// (M, with the fused secant quotient), assemble_tile_deriv.hip sets it to 1 and gets k_assemble_tile_deriv (M and the
// exact dM/domega).  The preprocessor selects the regions that differ, so each unit's compiler sees
// the token stream of a kernel written on its own (a body shared through templates changed the
// register allocation of the plain kernels).
//
// assemble_dense.hip reads both operands of its small complex GEMMs from HBM: the 8-KB tile block Q[p, 2n] = e^{A0} Q1,
// Q[p, 2n + 1] = e^{A0} Q0 of 16 pairs and one interval (node cache) and the 4-KB phase block E'[n, w] = wk_n exp(T_n w)
// (k_btab).  A batch without a cache -- node_cache_gb = 0, a cache that does not fit (npoints 1024), a one-shot call
// below cache_min_batch, the minority contour class of a call -- went through k_assemble_wl, which shares the node data
// of a (pair, interval) between 16 omega lanes but still spends one complex exponential per (pair, node, omega).  Here
// one wave BUILDS both operands of an interval in LDS -- 16 pairs x 15 nodes of node_data for the tile block, 15 nodes x
// <= 16 omegas of exp for the phase block (T = i t~ depends on the abscissa and the contour sense only) -- and then runs
// the dense fill's 48 v_mfma_f64_16x16x4_f64 and its per-element decisions.  One wave owns (tile of 16 pairs, chunk of
// <= 16 omegas of ONE contour class, plan_tile_chunks) = 256 integrals and walks the union of their trees level by level
// exactly as k_assemble_dense<1, 15, 1> does; the walk, the decisions and the epilogue are that kernel's text, copied
// (DESIGN.md 12.2).  Only MFMA rounds exist: a column that does not need an interval costs the matrix cores nothing, and
// pairs that no element needs are not evaluated.
//
// The derivative: from F' = exp(A0 + T w)(T (w Q1 + Q0) + Q1)
//     K'[p, w] = sum_n Q1[p, n] (E'_n + w D'_n) + Q0[p, n] D'_n,     D'_n = T_n E'_n:
// the SAME A operand against B rows that a lane forms in registers from the phase block and the T of its node slot.
// No twin columns (assemble_dense_deriv.hip): there they cost a second read of a cached record block, here they would
// cost a second BUILD of the tile block per omega.  The chunks keep <= 16 omegas, the operands are built once per
// entry, K and G decide as in the plain kernel -- so M, every accept / split decision and every interval count are that
// kernel's, bit for bit -- and on entries where at least one element accepted a second GEMM (32
// v_mfma_f64_16x16x4_f64, no Gauss part) reads the operands again and gives K'; an accepting element adds scale K' to a
// second pair of sums.
//
// Same preconditions as the dense fill (electrostatic, GK15, integration_accuracy >= 1e-9: the GEMM cannot apply the
// safe_exp clamp per (pair, node, omega)), same rounding-level differences from the reference, same interval sets.
// An element whose split does not fit the next 64-entry level list, or that meets a (pair, interval) whose folded
// amplitude is not representable, goes whole to the work list; the host finishes the list from scratch
// (launch_assemble_list without a cache view; launch_assemble_deriv_list for M and M').
//
// Parameter sets: EMME_TILE_SETS 1 is the reading for batches whose items carry their own parameter
// set (emme_ctx_bind_param_sets).  A chunk holds omegas of ONE set as well as of one class (plan_tile_chunks with
// host_set), so the set s of a workgroup is uniform: its scalars are read ONCE, before the kernel's first store, into a
// by-value copy -- scalar loads into SGPRs, where the one-set reading has its kernel argument (assemble_nodes_text.hpp)
// -- and its tables are tabs + s * 3N.  The work list has one segment and one counter per set, so that the list
// kernels (assemble_sets_list_text.hpp) keep the set uniform per workgroup too.  No fused secant.  The walk, the
// decisions, the caps, the counters and the epilogue are the one-set reading's.
//
//   SETS  DERIV   read by                         yields
//    0     0      assemble_tile.hip               k_assemble_tile, launch_assemble_tile
//    0     1      assemble_tile_deriv.hip         k_assemble_tile_deriv, launch_assemble_tile_deriv
//    1     0      assemble_tile_sets.hip          k_assemble_tile_sets, launch_assemble_tile_sets
//    1     1      assemble_tile_sets_deriv.hip    k_assemble_tile_sets_deriv, launch_assemble_tile_sets_deriv
//
// No include guard: a text, not a header of declarations.  The including unit defines EMME_TILE_DERIV and
// EMME_TILE_SETS and nothing else.
#if !defined(EMME_TILE_DERIV) || !defined(EMME_TILE_SETS)
#error "assemble_tile_text.hpp is included by assemble_tile.hip, assemble_tile_deriv.hip, assemble_tile_sets.hip and assemble_tile_sets_deriv.hip only, with EMME_TILE_DERIV and EMME_TILE_SETS set"
#endif
#include <hip/hip_runtime.h>

#include "assemble_common.hpp"
#include "launch.hpp"
#include "node_cache.hpp"

namespace emme {

namespace {

#if EMME_TILE_SETS && EMME_TILE_DERIV
struct TileSetsDerivArgs {
#elif EMME_TILE_SETS
struct TileSetsArgs {
#elif EMME_TILE_DERIV
struct TileDerivArgs {
#else
struct TileArgs {
#endif
#if EMME_TILE_SETS
    const DevParams* sets;  // [nsets]: the scalars of every bound parameter set
    const double* tabs;     // [nsets][3N]: eta | g | b of every set
    const int* set;         // [nbatch]: the set of every batch item
    const int* seg;         // [nsets]: where the work-list segment of every set begins
#else
    DevParams P;
    const double* tab;  // eta | g | b
#endif
    const ushort2* pairs;
    int npairs;
    unsigned long long* worklist;
    unsigned int* worklist_count;  // (sets: one counter per set)
    const int* act_idx;
    const int2* chunks;  // (first position, size <= 16) of every omega chunk; one contour class per chunk
    int nchunks;
    const double2* omega;
    double2* M;
#if EMME_TILE_DERIV
    double2* Md;
#elif !EMME_TILE_SETS
    const double2* Mold;
    double2* Mp;
    const double2* domega;
#endif
    unsigned long long* intervals;
    int* status;
    unsigned long long* stats;  // [0] MFMA rounds (the K' GEMMs are not counted), [3] tile tasks
    int skip_lost;              // columns whose matrix is already flagged (status) are left alone
};

// LDS of one wave: the two GEMM operands of the current entry, the pair constants of the tile and the sums of its 256
// elements
struct TileWaveLds {
    double2 q[TILE_BLOCK / 2];   // tile block: tile_index(2 sn + which, p)
    double2 e[BTAB_BLOCK / 2];   // phase block: E'[sn][column]
    double2 t[16];               // T per node slot
    double wk[16];               // Kronrod weight per node slot (slot 15: 0)
    double pc[TILE_PAIRS][8];    // PairConst of the tile's pairs
    double sumx[64][4], sumy[64][4], abstol[64][4];  // per element [lane][r]: accepted pieces, abs_tol of the root
#if EMME_TILE_DERIV
    double sumdx[64][4], sumdy[64][4];               // accepted pieces of K'
#endif
};

// TW: waves (tiles) per workgroup.
#if EMME_TILE_DERIV
// A wave holds 23 936 B of LDS: four of them leave room for ONE workgroup per CU (4 resident waves); two per workgroup
// let three workgroups share a CU, 6 resident waves.
constexpr int TW = 2;
constexpr int TW_WG_PER_CU = 6 / TW;
constexpr size_t TW_WG_LDS = TW * sizeof(TileWaveLds) + 16 * sizeof(unsigned long long) + 4 * sizeof(unsigned int) + 16;
static_assert(sizeof(TileWaveLds) == 23936, "LDS of a wave: DESIGN.md 12.3");
static_assert(TW_WG_PER_CU * TW_WG_LDS <= 163840, "the intended workgroups per CU do not fit the CU's LDS");

#if EMME_TILE_SETS
__global__ __launch_bounds__(64 * TW, 2) void k_assemble_tile_sets_deriv(TileSetsDerivArgs A) {
#else
__global__ __launch_bounds__(64 * TW, 2) void k_assemble_tile_deriv(TileDerivArgs A) {
#endif
#else
constexpr int TW = 4;
#ifndef EMME_TILE_MIN_WAVES
#define EMME_TILE_MIN_WAVES 2
#endif

#if EMME_TILE_SETS
__global__ __launch_bounds__(64 * TW, EMME_TILE_MIN_WAVES) void k_assemble_tile_sets(TileSetsArgs A) {
#else
__global__ __launch_bounds__(64 * TW, EMME_TILE_MIN_WAVES) void k_assemble_tile(TileArgs A) {
#endif
#endif
    constexpr int KS = 8, GKS = 4;  // k-steps of K, k-steps that feed G too
#if EMME_TILE_SETS
    // the set of the workgroup's chunk (its first column's; below: blockIdx.x / ntg is the chunk), and that set's
    // scalars by value before the first store: scalar loads (see the header)
    const int set_chunk = blockIdx.x / (((A.npairs + TILE_PAIRS - 1) / TILE_PAIRS + TW - 1) / TW);
    const int s = __builtin_amdgcn_readfirstlane(A.set[A.act_idx[A.chunks[set_chunk].x]]);
    const DevParams P = A.sets[s];
    const double* const tab = A.tabs + (size_t)s * 3 * P.N;
    const int seg = A.seg[s];
#else
    const DevParams& P = A.P;
#endif
    const int N = P.N, dim = P.dim;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, rho = lane >> 4;
    // chunk-major, the most expensive chunk first (plan_tile_chunks): its tasks are the longest and all start at once
    const int ntiles = (A.npairs + TILE_PAIRS - 1) / TILE_PAIRS;
    const int ntg = (ntiles + TW - 1) / TW;  // tile groups: TW tiles (one per wave) per workgroup
    const int chunk = blockIdx.x / ntg;
    const int tile = (blockIdx.x - chunk * ntg) * TW + wave;
    // Counters leave the workgroup once: its waves add them up in LDS and the last one to finish carries the sums to
    // memory (assemble_dense.hip).
    __shared__ unsigned long long s_iv[16];
    __shared__ unsigned int s_st[4];
    __shared__ int s_arrived;
    __shared__ TileWaveLds s_w[TW];
    if (threadIdx.x < 16) s_iv[threadIdx.x] = 0ull;
    if (threadIdx.x < 4) s_st[threadIdx.x] = 0u;
    if (threadIdx.x == 0) s_arrived = 0;
    __syncthreads();
    if (tile >= ntiles) return;
    const int waves_here = min(TW, ntiles - (tile - wave));  // waves of this workgroup that own a tile
    TileWaveLds& W = s_w[wave];

    const int2 ch = A.chunks[chunk];
    const bool in_chunk = col < ch.y;
    const int wpos = ch.x + (in_chunk ? col : 0);
    const int b = A.act_idx[wpos];
    const double2 omw = A.omega[b];  // this lane's column omega
    const int cls = -copysign(1.0, omw.x) > 0.0 ? 0 : 1;
    // the chunk's contour class is its first column's; a column of the other class (the planner never makes one)
    // is not filled and flags its matrix
    const int ccls = __builtin_amdgcn_readfirstlane(cls);
#if EMME_TILE_SETS
    // ... and so does a column of another set than the chunk's
    const bool wrong_class = in_chunk && (cls != ccls || A.set[b] != s);
#else
    const bool wrong_class = in_chunk && cls != ccls;
#endif
    if (wrong_class) A.status[b] = 1;
    // A matrix that already holds a non-finite integral is lost: nobody works on it any more (assemble_dense.hip)
    const bool has_w = in_chunk && !wrong_class && !(A.skip_lost && A.status[b] != 0);
    const double omi = ccls == 0 ? 1.0 : -1.0;  // -copysign(1, Re omega)
    // an entry v of M and what goes with it, vx: the same entry of M' (derivative), or rdw = 1 / domega of the fused
    // secant quotient (plain)
    auto store = [&](int r, int c, cd v, cd vx) {
        const size_t idx = (size_t)b * dim * dim + (size_t)r * dim + c;
#if EMME_TILE_DERIV
        store_entry_twin(A.M, A.Md, idx, v, vx);
#elif EMME_TILE_SETS
        store_entry_secant(A.M, nullptr, nullptr, vx, idx, v);
#else
        store_entry_secant(A.M, A.Mold, A.Mp, vx, idx, v);
#endif
    };
    if (tile == 0 && has_w) {  // diagonal (include/solver.h:442-443): constant in omega, so 0 in M'
#if EMME_TILE_DERIV || EMME_TILE_SETS
        const cd vx0 = mk(0.0, 0.0);
#else
        const cd vx0 = A.Mold ? rcp(mk(A.domega[b].x, A.domega[b].y)) : mk(0.0, 0.0);
#endif
        for (int i = rho; i < N; i += 4) store(i, i, mk(P.diag_a, 0.0), vx0);
    }

    // ---- what does not change during the task: the pair constants of the tile's 16 pairs, the node weights ----
    const GkLane gk = gk_lane<15>(col);            // build phase: lane = (pair row rho, node lane col)
    const int sn = slotnode_of_lane_t<15>(col);    // its node slot (Gauss nodes first, slot 15 padding)
    if (lane < 16) {
        const int pidx = tile * TILE_PAIRS + lane;
        const ushort2 ij = A.pairs[pidx < A.npairs ? pidx : 0];
        const int i = ij.x, j = ij.y;
#if EMME_TILE_SETS
        const PairConst pc = make_pair_const(P, tab[i], tab[j], tab[2 * N + i], tab[2 * N + j], tab[N + i] - tab[N + j]);
#else
        const PairConst pc = make_pair_const(P, A.tab[i], A.tab[j], A.tab[2 * N + i], A.tab[2 * N + j], A.tab[N + i] - A.tab[N + j]);
#endif
        pair_const_to_row(W.pc[lane], pc);
        W.wk[sn] = gk.wk;  // (lane 15 is the padding lane: weight 0 into slot 15)
    }
    wave_lds_sync();

    const double inv_scale = 2. / (M_PI / 2.0);
    // (wg / wk) of this lane's rows as MFMA A operand (row 4 ks + (lane >> 4), ks < 4)
    double grat[GKS];
#pragma unroll
    for (int ks = 0; ks < GKS; ++ks) grat[ks] = gauss_ratio<15>((4 * ks + (lane >> 4)) >> 1);
    const int loff = tile_index(lane >> 4, lane & 15);  // this lane's element of an MFMA operand load, k-step 0
    const int eoff = (lane >> 5) * 16 + (lane & 15);    // the same for the phase block: node 2 ks + (rho >> 1)
    // ---- the wave's 256 integrals: element r of this lane = (pair tile*16 + rho + 4 r, omega col) -----
    unsigned long long mcur[4], mnext[4];  // entries of the current / next level this element needs
    // (sums and tolerances live in LDS, touched only by their owner lane: 24 vector registers less across node_data)
    double* const sumx = W.sumx[lane];
    double* const sumy = W.sumy[lane];
    double* const abstol = W.abstol[lane];
#if EMME_TILE_DERIV
    double* const sumdx = W.sumdx[lane];
    double* const sumdy = W.sumdy[lane];
#endif
    int count[4];
    bool deferred[4], alive[4];
    // level lists: entry e of a level = its path in lane e of (E_lo, E_hi)
    unsigned int ecur_lo = 0, ecur_hi = 0, enext_lo = 0, enext_hi = 0;
    int n_cur = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int pidx = tile * TILE_PAIRS + rho + 4 * r;
        alive[r] = has_w && pidx < A.npairs;
        mcur[r] = alive[r] ? 1ull : 0ull, mnext[r] = 0ull;  // level 0: the root interval
        abstol[r] = 0.0, sumx[r] = 0.0, sumy[r] = 0.0, count[r] = 0, deferred[r] = false;
#if EMME_TILE_DERIV
        sumdx[r] = 0.0, sumdy[r] = 0.0;
#endif
    }
    if (__ballot(has_w) != 0ull) n_cur = 1;
    unsigned int n_dense = 0;
    int bad = 0;

    // (no record of the interval an element left at: there is no cache to grow around it)
    auto defer = [&](int r) {
#if EMME_TILE_SETS
        // (the segment of the chunk's set: it holds every integral of the set's items of this launch)
        const unsigned int slot = atomicAdd(A.worklist_count + s, 1u);
        A.worklist[(size_t)seg + slot] = ((unsigned long long)b << 32) | (unsigned int)(tile * TILE_PAIRS + rho + 4 * r);
#else
        const unsigned int slot = atomicAdd(A.worklist_count, 1u);
        A.worklist[slot] = ((unsigned long long)b << 32) | (unsigned int)(tile * TILE_PAIRS + rho + 4 * r);
#endif
        deferred[r] = true, alive[r] = false;
        mcur[r] = 0ull, mnext[r] = 0ull;
    };

    for (int depth = 0; n_cur > 0; ++depth) {
        int n_next = 0;
        for (int e = 0; e < n_cur; ++e) {
            // (entry e: lane e of the list -- e is wave-uniform)
            const unsigned int elo = (unsigned)__builtin_amdgcn_readlane((int)ecur_lo, e);
            const unsigned int ehi = (unsigned)__builtin_amdgcn_readlane((int)ecur_hi, e);
            const unsigned long long path = (((unsigned long long)ehi) << 32) | elo;
            bool match[4];
            unsigned long long mb[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) match[r] = ((mcur[r] >> e) & 1ull) != 0ull, mb[r] = __ballot(match[r]);
            const unsigned long long need = mb[0] | mb[1] | mb[2] | mb[3];
            if (need == 0ull) continue;  // (its owners were deferred meanwhile)
            const unsigned int colmask = (unsigned int)((need | (need >> 16) | (need >> 32) | (need >> 48)) & 0xffffull);

            // ---- the interval and this lane's abscissa (k_node_cache_tiled's form) ----
            double l, rr;
            interval_bounds_d(depth, path, l, rr);
            const double mid = (rr + l) / 2, scale = (rr - l) / 2;
            const double x = __dadd_rn(__dmul_rn(scale, gk.x), mid);

            // ---- tile block: pass r = pairs rho + 4 r, lane = node; a pair that no element needs is not evaluated ----
            bool have_t = false;
            cd tn = mk(0.0, 0.0);
#pragma unroll 1
            for (int r = 0; r < 4; ++r) {
                const int p = rho + 4 * r;
                const unsigned long long mbr = r == 0 ? mb[0] : r == 1 ? mb[1] : r == 2 ? mb[2] : mb[3];
                const bool wanted = ((mbr >> (lane & 48)) & 0xffffull) != 0ull;  // (uniform over the row of 16 lanes)
                cd q1 = mk(0.0, 0.0), q0 = mk(0.0, 0.0);
                bool over = false;
                if (wanted) {
                    const NodeData d = node_data(x, P, pair_const_of_row(W.pc[p]), omi, 0);
                    tn = d.T, have_t = true;
                    if (col < 15) {
                        double sa, ca;
                        sincos(d.A0.y, &sa, &ca);
                        const double ea = exp(d.A0.x);
                        const cd ex = mk(ea * ca, ea * sa);
                        q1 = ex * d.Q1, q0 = ex * d.Q0;
                        if (!(isfinite(q1.x) && isfinite(q1.y) && isfinite(q0.x) && isfinite(q0.y))) {
                            // Re A0 << 0: exp(A0) = 0 against an overflowing amplitude -- the reference's clamp makes the
                            // node contribute exactly 0.  Otherwise the folded amplitude is not representable: the
                            // (pair, interval) is POISONED (k_node_cache_tiled)
                            over = d.A0.x > -700.0;
                            q1 = mk(0.0, 0.0), q0 = mk(0.0, 0.0);
                        }
                    }
                }
                // poisoned (pair, interval): its records are zeroed (the GEMM of the tile's other pairs stays finite) and
                // every element of the pair that needs the interval goes to the work list
                const bool poisoned = ((__ballot(over) >> (lane & 48)) & 0xffffull) != 0ull;
                if (poisoned) q1 = mk(0.0, 0.0), q0 = mk(0.0, 0.0);
                W.q[tile_index(2 * sn, p)] = make_double2(q1.x, q1.y);
                W.q[tile_index(2 * sn + 1, p)] = make_double2(q0.x, q0.y);
                if (poisoned) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q == r && match[q]) defer(q), match[q] = false;
                }
            }
            // T of the node slots: pair-independent, the same bits in every row that evaluated a pair
            if (have_t) W.t[sn] = make_double2(tn.x, tn.y);
            wave_lds_sync();

            // ---- phase block: lane = (slots rho, rho + 4, rho + 8, rho + 12; column col), k_btab's rule ----
            const bool col_on = has_w && ((colmask >> col) & 1u) != 0u;
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                const int s = rho + 4 * k;
                cd bv = mk(0.0, 0.0);
                if (col_on && s < 15) bv = weighted_phase(&W.t[s], &omw, &W.wk[s]);
                W.e[s * 16 + col] = make_double2(bv.x, bv.y);
            }
            wave_lds_sync();

            // ---- the two GEMMs (assemble_dense.hip: dense round) ----
            v4d Kre = {0.0, 0.0, 0.0, 0.0}, Kim = Kre, Gre = Kre, Gim = Kre;
            {
                ++n_dense;
                v4d K2re = {0.0, 0.0, 0.0, 0.0}, K2im = K2re, G2re = K2re, G2im = K2re;
                const double2* a2 = W.q;
                const double2* b2 = W.e;
                double2 av[KS], ev[KS];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) av[ks] = a2[64 * ks + loff], ev[ks] = b2[32 * ks + eoff];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    // (B rows 4 ks + rho belong to node 2 ks + (rho >> 1): row rho even = omega E', odd = E')
                    const double2 a = av[ks], ep = ev[ks];
                    const double2 bk = (rho & 1) ? ep : make_double2(fma(omw.x, ep.x, -(omw.y * ep.y)), fma(omw.x, ep.y, omw.y * ep.x));
                    Kre = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, bk.x, Kre, 0, 0, 0);
                    Kim = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, bk.y, Kim, 0, 0, 0);
                    K2re = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, -bk.y, K2re, 0, 0, 0);
                    K2im = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, bk.x, K2im, 0, 0, 0);
                    if (ks < GKS) {  // G = sum_k (rho_k Q[p][k]) BK[k][w]: the A operand scaled, the same B
                        const double gx = a.x * grat[ks], gy = a.y * grat[ks];
                        Gre = __builtin_amdgcn_mfma_f64_16x16x4f64(gx, bk.x, Gre, 0, 0, 0);
                        Gim = __builtin_amdgcn_mfma_f64_16x16x4f64(gx, bk.y, Gim, 0, 0, 0);
                        G2re = __builtin_amdgcn_mfma_f64_16x16x4f64(gy, -bk.y, G2re, 0, 0, 0);
                        G2im = __builtin_amdgcn_mfma_f64_16x16x4f64(gy, bk.x, G2im, 0, 0, 0);
                    }
                }
                Kre += K2re, Kim += K2im, Gre += G2re, Gim += G2im;
            }
#if !EMME_TILE_DERIV
            // (the operands are in registers: the next entry may overwrite the blocks)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#endif

            // ---- every element that owns the interval decides for itself; an entry somebody splits puts its two
            // children on the next level's list
            bool split[4] = {false, false, false, false};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (match[r]) {
                    const int cnt = count[r] + 1;
                    count[r] = cnt;
                    bool sp = gk_split<SqrtSeeded>(mk(Kre[r], Kim[r]), mk(Gre[r], Gim[r]), scale, inv_scale, depth, P, abstol[r]);
                    if (sp && (depth >= EMME_MAX_DEPTH || cnt >= EMME_MAX_INTERVALS)) {
                        sp = false;
                        bad = 1;
                    }
                    if (!sp) {
                        sumx[r] += Kre[r] * scale;
                        sumy[r] += Kim[r] * scale;
                    }
                    split[r] = sp;
                }
            }
#if EMME_TILE_DERIV

            // ---- K' of the entry, where at least one element accepted: the operands once more from LDS (the blocks
            // are still those of this entry), the B rows formed in registers -- node 2 ks + (rho >> 1): row rho even =
            // E' + omega D', odd = D' = T E'.  (Slot 15 is the padding slot: its E' is 0 and its T the centre's.)
            if (__ballot((match[0] && !split[0]) || (match[1] && !split[1]) || (match[2] && !split[2]) ||
                         (match[3] && !split[3])) != 0ull) {
                v4d Dre = {0.0, 0.0, 0.0, 0.0}, Dim = Dre, D2re = Dre, D2im = Dre;
                const double2* a2 = W.q;
                const double2* b2 = W.e;
                double2 av[KS], ev[KS], tv[KS];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    av[ks] = a2[64 * ks + loff], ev[ks] = b2[32 * ks + eoff], tv[ks] = W.t[2 * ks + (lane >> 5)];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const double2 a = av[ks], ep = ev[ks], t = tv[ks];
                    const double2 dp = make_double2(fma(t.x, ep.x, -(t.y * ep.y)), fma(t.x, ep.y, t.y * ep.x));
                    const double2 bk = (rho & 1) ? dp
                                                 : make_double2(fma(omw.x, dp.x, fma(-omw.y, dp.y, ep.x)),
                                                                fma(omw.x, dp.y, fma(omw.y, dp.x, ep.y)));
                    Dre = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, bk.x, Dre, 0, 0, 0);
                    Dim = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, bk.y, Dim, 0, 0, 0);
                    D2re = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, -bk.y, D2re, 0, 0, 0);
                    D2im = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, bk.x, D2im, 0, 0, 0);
                }
                Dre += D2re, Dim += D2im;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (match[r] && !split[r]) {
                        sumdx[r] += Dre[r] * scale;
                        sumdy[r] += Dim[r] * scale;
                    }
                }
            }
            // (the operands have been read for the last time: the next entry may overwrite the blocks)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();

#endif
            if (__ballot(split[0] || split[1] || split[2] || split[3]) != 0ull) {
                if (n_next + 2 <= 64) {
                    const unsigned long long c0 = path << 1;
                    // (values and positions are wave-uniform: a lane-select writes lanes n_next and n_next + 1)
                    const int nl = n_next;
                    enext_lo = lane == nl ? (unsigned)c0 : (lane == nl + 1 ? (unsigned)(c0 | 1ull) : enext_lo);
                    enext_hi = (lane == nl || lane == nl + 1) ? (unsigned)(c0 >> 32) : enext_hi;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (split[r]) mnext[r] |= 3ull << nl;
                    n_next += 2;
                } else {
                    // the next level's list is full: these integrals start over in the list kernel
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (split[r]) defer(r);
                }
            }
        }
        ecur_lo = enext_lo, ecur_hi = enext_hi;
        n_cur = n_next;
#pragma unroll
        for (int r = 0; r < 4; ++r) mcur[r] = mnext[r], mnext[r] = 0ull;
    }

    // ---- results (include/solver.h:448-455: mat(i,j) = -kappa W_ij dx, mirrored; the same with sum' in M') -------
    unsigned long long my_intervals = 0;
#if EMME_TILE_SETS && !EMME_TILE_DERIV
    const cd rdw = mk(0.0, 0.0);
#elif !EMME_TILE_DERIV
    const cd rdw = A.Mold ? rcp(mk(A.domega[b].x, A.domega[b].y)) : mk(0.0, 0.0);
#endif
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int pidx = tile * TILE_PAIRS + rho + 4 * r;
        if (has_w && pidx < A.npairs && !deferred[r]) {
            my_intervals += (unsigned long long)count[r];
            const ushort2 ij = A.pairs[pidx];
            const int i = ij.x, j = ij.y;
            const cd kap = mk(P.pref * sumy[r], -(P.pref * sumx[r]));  // -i pref sum, Parameters.cpp:182
            if (kappa_bad(kap)) bad = 1;
#if EMME_TILE_DERIV
            const cd kd = mk(P.pref * sumdy[r], -(P.pref * sumdx[r]));
            if (kappa_bad(kd)) bad = 1;
            const double w = pair_entry_weight(i, j, N, P.dx);
            const cd v = w * kap, vd = w * kd;
            store(i, j, v, vd);
            store(j, i, v, vd);
#else
            const cd v = pair_entry_weight(i, j, N, P.dx) * kap;
            store(i, j, v, rdw);
            store(j, i, v, rdw);
#endif
        }
    }
    // interval count of this wave's 16 pairs per omega column: the four row lanes of a column, then the
    // workgroup's sum in LDS
    my_intervals += __shfl_xor(my_intervals, 16);
    my_intervals += __shfl_xor(my_intervals, 32);
    if (has_w) {
        if (my_intervals && rho == 0) atomicAdd(&s_iv[col], my_intervals);
        if (bad) A.status[b] = 1;
    }
    if (lane == 0) {
        atomicAdd(&s_st[0], n_dense);
        atomicAdd(&s_st[3], 1u);
    }
    __threadfence_block();
    int arrived = 0;
    if (lane == 0) arrived = atomicAdd(&s_arrived, 1) + 1;  // (LDS operations of a wave are performed in order)
    arrived = __builtin_amdgcn_readfirstlane(arrived);
    if (arrived == waves_here) {
        // the last wave of the workgroup: the sums go out (the lanes of row 0 hold the columns' items; every wave of
        // a workgroup serves the same chunk)
        __threadfence_block();
        if (lane < 16 && has_w && A.intervals && s_iv[lane] != 0ull) atomicAdd(&A.intervals[b], s_iv[lane]);
        if (A.stats && lane < 4) atomicAdd(&A.stats[lane], (unsigned long long)s_st[lane]);
    }
}

}  // namespace

// (sets: L.P is the context's own set, read for the shape only -- L.tab, L.Mold / L.Mp are not used; sets / tabs / set
// and seg are device arrays, see the argument struct; worklist_count has one counter per set)
#if EMME_TILE_SETS && EMME_TILE_DERIV
hipError_t launch_assemble_tile_sets_deriv(const AssembleLaunch& L, const DevParams* sets, const double* tabs,
                                           const int* set, const int* seg, unsigned long long* worklist,
                                           unsigned int* worklist_count, const int* act_idx, const void* chunks,
                                           int nchunks, unsigned long long* stats, hipStream_t stream) {
    if (L.gk_points != 15 || L.P.dim != L.P.N || !L.Md || L.Mold || !sets || !tabs || !set || !seg) return hipErrorInvalidValue;
    TileSetsDerivArgs A;
    A.Md = (double2*)L.Md;
#elif EMME_TILE_SETS
hipError_t launch_assemble_tile_sets(const AssembleLaunch& L, const DevParams* sets, const double* tabs, const int* set,
                                     const int* seg, unsigned long long* worklist, unsigned int* worklist_count,
                                     const int* act_idx, const void* chunks, int nchunks, unsigned long long* stats,
                                     hipStream_t stream) {
    if (L.gk_points != 15 || L.P.dim != L.P.N || L.Md) return hipErrorNotSupported;
    if (L.Mold || !sets || !tabs || !set || !seg) return hipErrorInvalidValue;  // (no fused secant)
    TileSetsArgs A;
#elif EMME_TILE_DERIV
hipError_t launch_assemble_tile_deriv(const AssembleLaunch& L, unsigned long long* worklist, unsigned int* worklist_count,
                                      const int* act_idx, const void* chunks, int nchunks, unsigned long long* stats,
                                      hipStream_t stream) {
    // (no fused secant: a derivative fill has M' itself)
    if (L.gk_points != 15 || L.P.dim != L.P.N || !L.Md || L.Mold) return hipErrorInvalidValue;
    TileDerivArgs A;
    A.Md = (double2*)L.Md;
#else
hipError_t launch_assemble_tile(const AssembleLaunch& L, unsigned long long* worklist, unsigned int* worklist_count,
                                const int* act_idx, const void* chunks, int nchunks, unsigned long long* stats,
                                hipStream_t stream) {
    if (L.gk_points != 15 || L.P.dim != L.P.N || L.Md) return hipErrorNotSupported;
    TileArgs A;
    A.Mold = (const double2*)L.Mold;
    A.Mp = (double2*)L.Mp;
    A.domega = (const double2*)L.domega;
#endif
    if (nchunks < 1) return hipSuccess;
#if EMME_TILE_SETS
    A.sets = sets;
    A.tabs = tabs;
    A.set = set;
    A.seg = seg;
#else
    A.P = L.P;
    A.tab = L.tab;
#endif
    A.pairs = (const ushort2*)L.pairs;
    A.npairs = L.npairs;
    A.worklist = worklist;
    A.worklist_count = worklist_count;
    A.act_idx = act_idx;
    A.chunks = (const int2*)chunks;
    A.nchunks = nchunks;
    A.omega = (const double2*)L.omega;
    A.M = (double2*)L.M;
    A.intervals = L.intervals;
    A.status = L.status;
    A.stats = stats;
    A.skip_lost = L.skip_lost;
    const int ntiles = (L.npairs + TILE_PAIRS - 1) / TILE_PAIRS;
    const int ntg = (ntiles + TW - 1) / TW;
#if EMME_TILE_SETS && EMME_TILE_DERIV
    hipLaunchKernelGGL(k_assemble_tile_sets_deriv, dim3((unsigned)((long)ntg * nchunks)), dim3(64 * TW), 0, stream, A);
#elif EMME_TILE_SETS
    hipLaunchKernelGGL(k_assemble_tile_sets, dim3((unsigned)((long)ntg * nchunks)), dim3(64 * TW), 0, stream, A);
#elif EMME_TILE_DERIV
    hipLaunchKernelGGL(k_assemble_tile_deriv, dim3((unsigned)((long)ntg * nchunks)), dim3(64 * TW), 0, stream, A);
#else
    hipLaunchKernelGGL(k_assemble_tile, dim3((unsigned)((long)ntg * nchunks)), dim3(64 * TW), 0, stream, A);
#endif
    return hipGetLastError();
}

}  // namespace emme
