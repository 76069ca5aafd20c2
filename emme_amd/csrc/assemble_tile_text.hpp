// assemble_tile_text.hpp -- the ONE text of every table-free tile fill kernel, compiled once per translation unit.
// Three selectors, all set by the including unit; the preprocessor selects the regions that differ, so each unit's
// compiler sees the token stream of a kernel written on its own (a body shared through templates or
// functions changed the register allocation of the kernels; 12.2.1 has the table of what was tried):
//
//   SHAPE SETS DERIV   read by                          yields
//     0    0    0      assemble_tile.hip                k_assemble_tile, launch_assemble_tile
//     0    0    1      assemble_tile_deriv.hip          k_assemble_tile_deriv, launch_assemble_tile_deriv
//     0    1    0      assemble_tile_sets.hip           k_assemble_tile_sets, launch_assemble_tile_sets
//     0    1    1      assemble_tile_sets_deriv.hip     k_assemble_tile_sets_deriv, launch_assemble_tile_sets_deriv
//     1    0    0      assemble_tile_shape.hip          k_assemble_tile_shape<PTS, NM>, launch_assemble_tile_shape
//     1    0    1      assemble_tile_shape_deriv.hip    k_assemble_tile_shape_deriv<PTS, NM>, launch_assemble_tile_shape_deriv
//     1    1    0      assemble_tile_shape_sets.hip     k_assemble_tile_shape_sets<PTS, NM>, launch_assemble_tile_shape_sets
//     1    1    1      assemble_tile_shape_sets_deriv.hip  k_assemble_tile_shape_sets_deriv<PTS, NM>,
//                                                       launch_assemble_tile_shape_sets_deriv
//
// EMME_TILE_SHAPE 0 is electrostatic GK15 (no template: PTS = 15 and NM = 1 are constants inside the kernel);
// EMME_TILE_SHAPE 1 is a template over (PTS, NM) = (15, 3), (31, 1) and (31, 3): electromagnetic contexts (three
// velocity moments per pair) and the 31-point rule.  EMME_TILE_DERIV 0 gives M (one-set readings: with the fused secant
// quotient), 1 gives M and the exact dM/domega.  EMME_TILE_SETS 1 is the reading for batches
// whose items carry their own parameter set (DESIGN.md 13.7 for electrostatic GK15, 13.8 for the shape template): every
// combination of the three selectors is a reading, eight in all.
//
// assemble_dense.hip reads both operands of its small complex GEMMs from HBM: the tile block Q[p, 2n] = e^{A0} Q1,
// Q[p, 2n + 1] = e^{A0} Q0 of 16 pairs and one interval (node cache) and the phase block E'[n, w] = wk_n exp(T_n w)
// (k_btab).  A batch without a cache -- node_cache_gb = 0, a cache that does not fit (npoints 1024), a one-shot call
// below cache_min_batch, the minority contour class of a call -- went through k_assemble_wl, which shares the node data
// of a (pair, interval) between 16 omega lanes but still spends one complex exponential per (pair, node, omega).  Here
// one wave BUILDS both operands of an interval in LDS -- 16 pairs x PTS nodes of node_data for the tile block, PTS nodes
// x <= 16 columns of exp for the phase block (T = i t~ depends on the abscissa and the contour sense only) -- and then
// runs the dense fill's v_mfma_f64_16x16x4_f64 (48 per entry for GK15, 96 for GK31) and its per-element decisions.  One
// wave owns (tile of 16 pairs, chunk of <= 16 columns of ONE contour class, plan_tile_chunks) = 256 integrals and walks
// the union of their trees level by level exactly as k_assemble_dense<1, PTS, NM> does.  Only MFMA rounds exist: a
// column that does not need an interval costs the matrix cores nothing, and pairs that no element needs are not
// evaluated.  The leaves are assemble_common.hpp's and emme_device.hpp's.
//
// The operand shapes (those of k_assemble_dense<1, PTS, NM>):
//   PTS = 31: 32 node slots (15 Gauss nodes, the 16 Kronrod-only ones, one padding slot: slotnode_of_lane_t<31>), a
//             16-KB tile block and an 8-KB phase block, 16 k-steps of which the first 8 feed G.  A lane of the build
//             takes two node slots (gk lanes col and col + 16), one after the other.
//   NM = 3:   a chunk is <= 5 omegas x 3 moments = 15 columns, column 3 w + m (column 15 idle).  The moment factor of
//             F_m = F_0 (c_nv W)^m has a pair-independent part W^m, which sits in the phase operand (k_btab<PTS, 3>'s
//             successive products; W = node_w is computed once per node slot and entry), and the pair's real c_nv^m,
//             which multiplies the element's sums before its decision.  The tile block holds moment-0 amplitudes only.
//
// The derivative: from F' = exp(A0 + T w)(T (w Q1 + Q0) + Q1), per column with that column's omega (W = node_w does not
// depend on omega, so F'_m = F'_0 (c_nv W)^m),
//     K'[p, c] = sum_n Q1[p, n] (E'_n + omega D'_n) + Q0[p, n] D'_n,     D'_n = T_n E'_n:
// the SAME A operand against B rows that a lane forms in registers from the phase block and the T of its node slot.
// No twin columns (assemble_dense_deriv.hip): there they cost a second read of a cached record block, here they would
// cost a second BUILD of the tile block per omega.  The operands are built once per entry, K and G decide as in the
// plain kernel -- so M, every accept / split decision and every interval count are that kernel's, bit for bit -- and on
// entries where at least one element accepted a second GEMM (32 v_mfma_f64_16x16x4_f64 for GK15, 64 for GK31, no Gauss
// part) reads the operands again and gives K'; an accepting element adds scale c_nv^m K' to a second pair of sums.
//
// Same preconditions as the dense fill (integration_accuracy >= 1e-9: the GEMM cannot apply the safe_exp clamp per
// (pair, node, omega)), same rounding-level differences from the reference, same interval sets.  An element whose
// split does not fit the next 64-entry level list, or that meets a (pair, interval) whose folded amplitude is not
// representable, goes whole to the work list, as the dense fill's entry (b << 32) | (pair NM + moment); the host
// finishes the list from scratch (launch_assemble_list without a cache view; for M and M' launch_assemble_deriv_list
// or, shape, k_assemble_deriv_list_shape<PTS> of assemble_tile_shape_deriv.hip).
//
// Parameter sets: a chunk holds omegas of ONE set as well as of one class (plan_tile_chunks with host_set), so the set
// s of a workgroup is uniform: its scalars are read ONCE, before the kernel's first store, into a by-value copy --
// scalar loads into SGPRs, where the one-set reading has its kernel argument (assemble_nodes_text.hpp) -- and its
// tables are tabs + s * 3N.  The work list has one segment and one counter per set, so that the list kernels
// (assemble_sets_list_text.hpp) keep the set uniform per workgroup too.  No fused secant.  The shape sets readings take
// everything else from the one-set shape readings, token for token: node_w's parameters, the diag_d * b[i] diagonal
// block and the kappa_e terms of the electromagnetic epilogue are then the chunk's set's, through P and tab.
//
// LDS per wave and waves per workgroup: see below the wave's struct, and DESIGN.md 5.3c, 12.3, 12.4.
//
// No include guard: a text, not a header of declarations.  The including unit defines the three selectors and nothing
// else.
#if !defined(EMME_TILE_SHAPE) || !defined(EMME_TILE_SETS) || !defined(EMME_TILE_DERIV)
#error "assemble_tile_text.hpp is included by the eight assemble_tile*.hip units only, with EMME_TILE_SHAPE, EMME_TILE_SETS and EMME_TILE_DERIV set"
#endif
#include <hip/hip_runtime.h>

#include "assemble_common.hpp"
#include "launch.hpp"
#include "node_cache.hpp"

namespace emme {

namespace {

#if EMME_TILE_SHAPE && EMME_TILE_SETS && EMME_TILE_DERIV
struct TileShapeSetsDerivArgs {
#elif EMME_TILE_SHAPE && EMME_TILE_SETS
struct TileShapeSetsArgs {
#elif EMME_TILE_SHAPE && EMME_TILE_DERIV
struct TileShapeDerivArgs {
#elif EMME_TILE_SHAPE
struct TileShapeArgs {
#elif EMME_TILE_SETS && EMME_TILE_DERIV
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
    const int2* chunks;  // (first position, size <= 16 / NM) of every omega chunk; one contour class per chunk
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
#if EMME_TILE_SHAPE
template <int PTS>
struct TileShapeWaveLds {
    double2 q[tile_block_doubles(PTS) / 2];  // tile block: tile_index(2 sn + which, p)
    double2 e[btab_block_doubles(PTS) / 2];  // phase block: E'[sn][column]
    double2 t[tile_slots(PTS)];              // T per node slot
    double2 w[tile_slots(PTS)];              // W per node slot (electromagnetic)
    double wk[tile_slots(PTS)];              // Kronrod weight per node slot (padding slot: 0)
    double2 om[8];                           // omega per position of the chunk (electromagnetic: the phase build's)
#else
struct TileWaveLds {
    double2 q[TILE_BLOCK / 2];   // tile block: tile_index(2 sn + which, p)
    double2 e[BTAB_BLOCK / 2];   // phase block: E'[sn][column]
    double2 t[16];               // T per node slot
    double wk[16];               // Kronrod weight per node slot (slot 15: 0)
#endif
    double pc[TILE_PAIRS][8];    // PairConst of the tile's pairs
    double sumx[64][4], sumy[64][4], abstol[64][4];  // per element [lane][r]: accepted pieces, abs_tol of the root
#if EMME_TILE_DERIV
    double sumdx[64][4], sumdy[64][4];               // accepted pieces of K'
#endif
};

// Waves (tiles) per workgroup.
#if EMME_TILE_SHAPE
// LDS per wave, plain: 20 224 bytes for GK15, 33 152 for GK31.  GK15 workgroups have 4 waves as k_assemble_tile's
// (81 048 bytes, two per CU); GK31 workgroups have 2 (66 456 bytes), so that two of them share a CU's 160 KB and a CU is
// not held by the slowest of four tiles.  Derivative: 4 096 bytes of K' sums more, and every workgroup
// has 2 waves (four GK15 waves, 97 280 B, would leave room for ONE workgroup per CU): three GK15 workgroups or two GK31
// ones share a CU.
#if EMME_TILE_DERIV
__host__ __device__ constexpr int tile_shape_waves(int) { return 2; }
__host__ __device__ constexpr int tile_shape_wg_per_cu(int pts) { return pts == 15 ? 3 : 2; }
template <int PTS>
constexpr size_t tile_shape_wg_lds() {
    return tile_shape_waves(PTS) * sizeof(TileShapeWaveLds<PTS>) + 16 * sizeof(unsigned long long) + 4 * sizeof(unsigned int) + 16;
}
static_assert(sizeof(TileShapeWaveLds<15>) == 20224 + 4096, "LDS of a GK15 wave: DESIGN.md 12.4");
static_assert(sizeof(TileShapeWaveLds<31>) == 33152 + 4096, "LDS of a GK31 wave: DESIGN.md 12.4");
static_assert(tile_shape_wg_per_cu(15) * tile_shape_wg_lds<15>() <= 163840, "three GK15 workgroups do not fit the CU's LDS");
static_assert(tile_shape_wg_per_cu(31) * tile_shape_wg_lds<31>() <= 163840, "two GK31 workgroups do not fit the CU's LDS");
#else
__host__ __device__ constexpr int tile_shape_waves(int pts) { return pts == 15 ? 4 : 2; }
#endif
#elif EMME_TILE_DERIV
// A wave holds 23 936 B of LDS: four of them leave room for ONE workgroup per CU (4 resident waves); two per workgroup
// let three workgroups share a CU, 6 resident waves.
constexpr int TW = 2;
constexpr int TW_WG_PER_CU = 6 / TW;
constexpr size_t TW_WG_LDS = TW * sizeof(TileWaveLds) + 16 * sizeof(unsigned long long) + 4 * sizeof(unsigned int) + 16;
static_assert(sizeof(TileWaveLds) == 23936, "LDS of a wave: DESIGN.md 12.3");
static_assert(TW_WG_PER_CU * TW_WG_LDS <= 163840, "the intended workgroups per CU do not fit the CU's LDS");
#else
constexpr int TW = 4;
#ifndef EMME_TILE_MIN_WAVES
#define EMME_TILE_MIN_WAVES 2
#endif
#endif

// The kernel.  Shape: <15, 3> stays inside 256 registers without scratch, two waves per SIMD; the GK31
// builds are compiled for one.
#if EMME_TILE_SHAPE
template <int PTS, int NM>
#if EMME_TILE_SETS && EMME_TILE_DERIV
__global__ __launch_bounds__(64 * tile_shape_waves(PTS), PTS == 15 ? 2 : 1) void k_assemble_tile_shape_sets_deriv(TileShapeSetsDerivArgs A) {
#elif EMME_TILE_SETS
__global__ __launch_bounds__(64 * tile_shape_waves(PTS), PTS == 15 ? 2 : 1) void k_assemble_tile_shape_sets(TileShapeSetsArgs A) {
#elif EMME_TILE_DERIV
__global__ __launch_bounds__(64 * tile_shape_waves(PTS), PTS == 15 ? 2 : 1) void k_assemble_tile_shape_deriv(TileShapeDerivArgs A) {
#else
__global__ __launch_bounds__(64 * tile_shape_waves(PTS), PTS == 15 ? 2 : 1) void k_assemble_tile_shape(TileShapeArgs A) {
#endif
    constexpr int WPG = tile_shape_waves(PTS);
    constexpr int NH = tile_slots(PTS) / 16;  // node slots a lane of the build takes
    using WaveLds = TileShapeWaveLds<PTS>;
#else
#if EMME_TILE_SETS && EMME_TILE_DERIV
__global__ __launch_bounds__(64 * TW, 2) void k_assemble_tile_sets_deriv(TileSetsDerivArgs A) {
#elif EMME_TILE_SETS
__global__ __launch_bounds__(64 * TW, EMME_TILE_MIN_WAVES) void k_assemble_tile_sets(TileSetsArgs A) {
#elif EMME_TILE_DERIV
__global__ __launch_bounds__(64 * TW, 2) void k_assemble_tile_deriv(TileDerivArgs A) {
#else
__global__ __launch_bounds__(64 * TW, EMME_TILE_MIN_WAVES) void k_assemble_tile(TileArgs A) {
#endif
    constexpr int PTS = 15, NM = 1, WPG = TW;
    using WaveLds = TileWaveLds;
#endif
    // node slots, k-steps of K, k-steps that feed G too, omegas per chunk
    constexpr int NS = tile_slots(PTS), KS = NS / 2, GKS = KS / 2, NW = 16 / NM;
#if EMME_TILE_SETS
    // the set of the workgroup's chunk (its first column's; below: blockIdx.x / ntg is the chunk), and that set's
    // scalars by value before the first store: scalar loads (see the header)
    const int set_chunk = blockIdx.x / (((A.npairs + TILE_PAIRS - 1) / TILE_PAIRS + WPG - 1) / WPG);
    const int s = __builtin_amdgcn_readfirstlane(A.set[A.act_idx[A.chunks[set_chunk].x]]);
    const DevParams P = A.sets[s];
    const double* const tab = A.tabs + (size_t)s * 3 * P.N;
    const int seg = A.seg[s];
#else
    const DevParams& P = A.P;
    const double* const tab = A.tab;
#endif
    const int N = P.N, dim = P.dim;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, rho = lane >> 4;
    const int wcol = NM == 1 ? col : col / NM;      // omega position of this lane's column in its chunk
    const int mom = NM == 1 ? 0 : col - wcol * NM;  // its velocity moment
    // chunk-major, the most expensive chunk first (plan_tile_chunks): its tasks are the longest and all start at once
    const int ntiles = (A.npairs + TILE_PAIRS - 1) / TILE_PAIRS;
    const int ntg = (ntiles + WPG - 1) / WPG;  // tile groups: one tile per wave of a workgroup
    const int chunk = blockIdx.x / ntg;
    const int tile = (blockIdx.x - chunk * ntg) * WPG + wave;
    // Counters leave the workgroup once: its waves add them up in LDS and the last one to finish carries the sums to
    // memory (assemble_dense.hip).
    __shared__ unsigned long long s_iv[16];
    __shared__ unsigned int s_st[4];
    __shared__ int s_arrived;
    __shared__ WaveLds s_w[WPG];
    if (threadIdx.x < 16) s_iv[threadIdx.x] = 0ull;
    if (threadIdx.x < 4) s_st[threadIdx.x] = 0u;
    if (threadIdx.x == 0) s_arrived = 0;
    __syncthreads();
    if (tile >= ntiles) return;
    const int waves_here = min(WPG, ntiles - (tile - wave));  // waves of this workgroup that own a tile
    WaveLds& W = s_w[wave];

    const int2 ch = A.chunks[chunk];
    const bool in_chunk = wcol < ch.y && wcol < NW;
    const int wpos = ch.x + (in_chunk ? wcol : 0);
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
    if (tile == 0 && has_w && mom == 0) {  // diagonal (include/solver.h:442-443; electromagnetic: 465-470): 0 in M'
#if EMME_TILE_DERIV || EMME_TILE_SETS
        const cd vx0 = mk(0.0, 0.0);
#else
        const cd vx0 = A.Mold ? rcp(mk(A.domega[b].x, A.domega[b].y)) : mk(0.0, 0.0);
#endif
        for (int i = rho; i < N; i += 4) {
            store(i, i, mk(P.diag_a, 0.0), vx0);
            if (NM > 1) {
                store(i, i + N, mk(0.0, 0.0), vx0);
                store(i + N, i, mk(0.0, 0.0), vx0);
                store(i + N, i + N, mk(P.diag_d * tab[2 * N + i], 0.0), vx0);
            }
        }
    }

    // ---- what does not change during the task: the pair constants of the tile's 16 pairs, the node weights, the
    // chunk's omegas (electromagnetic) ----
#if EMME_TILE_SHAPE
    // build phase: lane = (pair row rho, gk lanes col and, GK31, col + 16); their abscissae and node slots
    const double gx0 = gk_lane<PTS>(col).x, gx1 = gk_lane<PTS>(NH > 1 ? col + 16 : col).x;
    const int sn0 = slotnode_of_lane_t<PTS>(col), sn1 = slotnode_of_lane_t<PTS>(NH > 1 ? col + 16 : col);
#else
    const GkLane gk = gk_lane<PTS>(col);            // build phase: lane = (pair row rho, node lane col)
    const int sn = slotnode_of_lane_t<PTS>(col);    // its node slot (Gauss nodes first, slot 15 padding)
#endif
    if (lane < 16) {
        const int pidx = tile * TILE_PAIRS + lane;
        const ushort2 ij = A.pairs[pidx < A.npairs ? pidx : 0];
        const int i = ij.x, j = ij.y;
        const PairConst pc = make_pair_const(P, tab[i], tab[j], tab[2 * N + i], tab[2 * N + j], tab[N + i] - tab[N + j]);
        pair_const_to_row(W.pc[lane], pc);
#if !EMME_TILE_SHAPE
        W.wk[sn] = gk.wk;  // (lane 15 is the padding lane: weight 0 into slot 15)
#endif
    }
#if EMME_TILE_SHAPE
    if (lane < NS) W.wk[slotnode_of_lane_t<PTS>(lane)] = gk_lane<PTS>(lane).wk;  // (the padding lane: weight 0)
    if (NM > 1) {
        if (rho == 0 && mom == 0 && wcol < NW) W.om[wcol] = omw;
        // (column 15 belongs to no omega: the phase build never writes it)
#pragma unroll 1
        for (int ns = lane; ns < NS; ns += 64) W.e[ns * 16 + 15] = make_double2(0.0, 0.0);
    }
#endif
    wave_lds_sync();
    // c_nv^m of pair slot q of this tile (1 for electrostatic fills); m is the column's moment
    auto moment_factor = [&](int q, int m) -> double {
        if (NM == 1) return 1.0;
        const double cv = W.pc[q][6];
        return m == 0 ? 1.0 : (m == 1 ? cv : cv * cv);
    };

    const double inv_scale = 2. / (M_PI / 2.0);
    // (wg / wk) of this lane's rows as MFMA A operand (row 4 ks + (lane >> 4), ks < GKS)
    double grat[GKS];
#pragma unroll
    for (int ks = 0; ks < GKS; ++ks) grat[ks] = gauss_ratio<PTS>((4 * ks + (lane >> 4)) >> 1);
    const int loff = tile_index(lane >> 4, lane & 15);  // this lane's element of an MFMA operand load, k-step 0
    const int eoff = (lane >> 5) * 16 + (lane & 15);    // the same for the phase block: node 2 ks + (rho >> 1)
    // ---- the wave's 256 integrals: element r of this lane = (pair tile*16 + rho + 4 r, column col) -----
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
        const unsigned int item = (unsigned int)((tile * TILE_PAIRS + rho + 4 * r) * NM + mom);
#if EMME_TILE_SETS
        // (the segment of the chunk's set: it holds every integral of the set's items of this launch)
        const unsigned int slot = atomicAdd(A.worklist_count + s, 1u);
        A.worklist[(size_t)seg + slot] = ((unsigned long long)b << 32) | item;
#else
        const unsigned int slot = atomicAdd(A.worklist_count, 1u);
        A.worklist[slot] = ((unsigned long long)b << 32) | item;
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

            // ---- the interval (k_node_cache_tiled's form) ----
            double l, rr;
            interval_bounds_d(depth, path, l, rr);
            const double mid = (rr + l) / 2, scale = (rr - l) / 2;

#if EMME_TILE_SHAPE
            // ---- moment factor W of the node slots (electromagnetic): pair-independent, once per slot and entry ----
            if (NM > 1) {
#pragma unroll 1
                for (int h = 0; h < NH; ++h) {
                    if (lane < 16) {
                        const double x = __dadd_rn(__dmul_rn(scale, h ? gx1 : gx0), mid);
                        const cd wv = node_w(x, P, omi);
                        W.w[h ? sn1 : sn0] = make_double2(wv.x, wv.y);
                    }
                }
            }

            // ---- tile block: pass r = pairs rho + 4 r, lane = node(s); a pair that no element needs is not evaluated ----
#pragma unroll 1
            for (int r = 0; r < 4; ++r) {
                const int p = rho + 4 * r;
                const unsigned long long mbr = r == 0 ? mb[0] : r == 1 ? mb[1] : r == 2 ? mb[2] : mb[3];
                const bool wanted = ((mbr >> (lane & 48)) & 0xffffull) != 0ull;  // (uniform over the row of 16 lanes)
                bool over = false;
#pragma unroll 1
                for (int h = 0; h < NH; ++h) {
                    const int sn = h ? sn1 : sn0;
                    const bool real_node = col + 16 * h < PTS;  // (the last gk lane is the padding lane)
                    cd q1 = mk(0.0, 0.0), q0 = mk(0.0, 0.0);
                    if (wanted) {
                        const double x = __dadd_rn(__dmul_rn(scale, h ? gx1 : gx0), mid);
                        const NodeData d = node_data(x, P, pair_const_of_row(W.pc[p]), omi, 0);
                        // T of the node slot: pair-independent, the same bits from every row that evaluates a pair
                        W.t[sn] = make_double2(d.T.x, d.T.y);
                        if (real_node) {
                            double sa, ca;
                            sincos(d.A0.y, &sa, &ca);
                            const double ea = exp(d.A0.x);
                            const cd ex = mk(ea * ca, ea * sa);
                            q1 = ex * d.Q1, q0 = ex * d.Q0;
                            if (!(isfinite(q1.x) && isfinite(q1.y) && isfinite(q0.x) && isfinite(q0.y))) {
                                // Re A0 << 0: exp(A0) = 0 against an overflowing amplitude -- the reference's clamp makes the
                                // node contribute exactly 0.  Otherwise the folded amplitude is not representable: the
                                // (pair, interval) is POISONED (k_node_cache_tiled)
                                over = over || d.A0.x > -700.0;
                                q1 = mk(0.0, 0.0), q0 = mk(0.0, 0.0);
                            }
                        }
                    }
                    W.q[tile_index(2 * sn, p)] = make_double2(q1.x, q1.y);
                    W.q[tile_index(2 * sn + 1, p)] = make_double2(q0.x, q0.y);
                }
                // poisoned (pair, interval): its records are zeroed (the GEMM of the tile's other pairs stays finite) and
                // every element of the pair that needs the interval goes to the work list, whatever its moment
                const bool poisoned = ((__ballot(over) >> (lane & 48)) & 0xffffull) != 0ull;
                if (poisoned) {
#pragma unroll
                    for (int h = 0; h < NH; ++h) {
                        const int sn = h ? sn1 : sn0;
                        W.q[tile_index(2 * sn, p)] = make_double2(0.0, 0.0);
                        W.q[tile_index(2 * sn + 1, p)] = make_double2(0.0, 0.0);
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q == r && match[q]) defer(q), match[q] = false;
                }
            }
            wave_lds_sync();
#else
            // ---- tile block: this lane's abscissa; pass r = pairs rho + 4 r, lane = node, T kept in a register; a pair
            // that no element needs is not evaluated (the comments of the shape region above apply) ----
            const double x = __dadd_rn(__dmul_rn(scale, gk.x), mid);
            bool have_t = false;
            cd tn = mk(0.0, 0.0);
#pragma unroll 1
            for (int r = 0; r < 4; ++r) {
                const int p = rho + 4 * r;
                const unsigned long long mbr = r == 0 ? mb[0] : r == 1 ? mb[1] : r == 2 ? mb[2] : mb[3];
                const bool wanted = ((mbr >> (lane & 48)) & 0xffffull) != 0ull;
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
                            over = d.A0.x > -700.0;
                            q1 = mk(0.0, 0.0), q0 = mk(0.0, 0.0);
                        }
                    }
                }
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
#endif

            // ---- phase block, k_btab's rule ----
            if (NM == 1) {
                // lane = (slots rho, rho + 4, ..; column col)
                const bool col_on = has_w && ((colmask >> col) & 1u) != 0u;
#pragma unroll 1
                for (int k = 0; k < NS / 4; ++k) {
                    const int ns = rho + 4 * k;  // (node slot; `s` is the chunk's set in the sets readings)
                    cd bv = mk(0.0, 0.0);
                    if (col_on && ns < PTS) {
                        // (weighted_phase's text: the call changes k_assemble_tile_shape_deriv<31, 1>)
                        const double2 t = W.t[ns];
                        const double ax = fma(t.x, omw.x, -(t.y * omw.y)), ay = fma(t.x, omw.y, t.y * omw.x);
                        cd ev;
                        if (!(ax > 700.0)) {  // (a NaN omega goes through and poisons its own column only)
                            double sa, ca;
                            sincos(ay, &sa, &ca);
                            const double ea = exp(ax);
                            ev = mk(ea * ca, ea * sa);
                        } else {
                            // exp(T omega) beyond 1e304: NaN -- an integral of this omega that uses the node ends non-finite
                            // and flags its matrix (EMME_ENUMERIC) instead of dropping the term
                            ev = mk(__builtin_nan(""), __builtin_nan(""));
                        }
                        const double wk = W.wk[ns];
                        bv = mk(wk * ev.x, wk * ev.y);
                    }
                    W.e[ns * 16 + col] = make_double2(bv.x, bv.y);
                }
#if EMME_TILE_SHAPE
            } else {
                // one exponential per (node slot, omega): item = slot * NW + omega position, its three columns
                // 3 w + m are the successive products with W
#pragma unroll 1
                for (int it = lane; it < NW * NS; it += 64) {
                    const int ns = it / NW, w = it - ns * NW;
                    cd bv = mk(0.0, 0.0), wv = mk(0.0, 0.0);
                    if (((colmask >> (NM * w)) & ((1u << NM) - 1u)) != 0u && ns < PTS) {
                        bv = weighted_phase(&W.t[ns], &W.om[w], &W.wk[ns]);  // (NaN in this omega's columns only)
                        const double2 w2 = W.w[ns];
                        wv = mk(w2.x, w2.y);
                    }
                    W.e[ns * 16 + NM * w] = make_double2(bv.x, bv.y);
#pragma unroll
                    for (int m = 1; m < NM; ++m) {
                        bv = bv * wv;
                        W.e[ns * 16 + NM * w + m] = make_double2(bv.x, bv.y);
                    }
                }
#endif
            }
            wave_lds_sync();

            // ---- the two GEMMs (assemble_dense.hip: dense round) ----
            v4d Kre = {0.0, 0.0, 0.0, 0.0}, Kim = Kre, Gre = Kre, Gim = Kre;
            {
                ++n_dense;
                v4d K2re = {0.0, 0.0, 0.0, 0.0}, K2im = K2re, G2re = K2re, G2im = K2re;
                const double2* a2 = W.q;
                const double2* b2 = W.e;
#if EMME_TILE_SHAPE
#pragma unroll
                for (int h = 0; h < KS / 8; ++h) {  // (GK31: two batches of eight k-steps, the Gauss rule in the first)
                    double2 av[8], ev[8];
#pragma unroll
                    for (int ks = 0; ks < 8; ++ks) av[ks] = a2[64 * (8 * h + ks) + loff], ev[ks] = b2[32 * (8 * h + ks) + eoff];
#pragma unroll
                    for (int ks = 0; ks < 8; ++ks) {
                        // (B rows 4 ks + rho belong to node 2 ks + (rho >> 1): row rho even = omega E', odd = E')
                        const double2 a = av[ks], ep = ev[ks];
                        const double2 bk = (rho & 1) ? ep : make_double2(fma(omw.x, ep.x, -(omw.y * ep.y)), fma(omw.x, ep.y, omw.y * ep.x));
                        Kre = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, bk.x, Kre, 0, 0, 0);
                        Kim = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, bk.y, Kim, 0, 0, 0);
                        K2re = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, -bk.y, K2re, 0, 0, 0);
                        K2im = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, bk.x, K2im, 0, 0, 0);
                        if (8 * h + ks < GKS) {  // G = sum_k (rho_k Q[p][k]) BK[k][w]: the A operand scaled, the same B
                            const double gx = a.x * grat[(8 * h + ks) % GKS], gy = a.y * grat[(8 * h + ks) % GKS];
                            Gre = __builtin_amdgcn_mfma_f64_16x16x4f64(gx, bk.x, Gre, 0, 0, 0);
                            Gim = __builtin_amdgcn_mfma_f64_16x16x4f64(gx, bk.y, Gim, 0, 0, 0);
                            G2re = __builtin_amdgcn_mfma_f64_16x16x4f64(gy, -bk.y, G2re, 0, 0, 0);
                            G2im = __builtin_amdgcn_mfma_f64_16x16x4f64(gy, bk.x, G2im, 0, 0, 0);
                        }
                    }
                }
#else
                // (one batch of KS = 8 k-steps, the shape region's k-step: its h-loop form moves the plain ES15
                // kernels' code)
                double2 av[KS], ev[KS];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) av[ks] = a2[64 * ks + loff], ev[ks] = b2[32 * ks + eoff];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const double2 a = av[ks], ep = ev[ks];
                    const double2 bk = (rho & 1) ? ep : make_double2(fma(omw.x, ep.x, -(omw.y * ep.y)), fma(omw.x, ep.y, omw.y * ep.x));
                    Kre = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, bk.x, Kre, 0, 0, 0);
                    Kim = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, bk.y, Kim, 0, 0, 0);
                    K2re = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, -bk.y, K2re, 0, 0, 0);
                    K2im = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, bk.x, K2im, 0, 0, 0);
                    if (ks < GKS) {
                        const double gx = a.x * grat[ks], gy = a.y * grat[ks];
                        Gre = __builtin_amdgcn_mfma_f64_16x16x4f64(gx, bk.x, Gre, 0, 0, 0);
                        Gim = __builtin_amdgcn_mfma_f64_16x16x4f64(gx, bk.y, Gim, 0, 0, 0);
                        G2re = __builtin_amdgcn_mfma_f64_16x16x4f64(gy, -bk.y, G2re, 0, 0, 0);
                        G2im = __builtin_amdgcn_mfma_f64_16x16x4f64(gy, bk.x, G2im, 0, 0, 0);
                    }
                }
#endif
                Kre += K2re, Kim += K2im, Gre += G2re, Gim += G2im;
            }
#if !EMME_TILE_DERIV
            // (the operands are in registers: the next entry may overwrite the blocks)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#endif

            // ---- every element that owns the interval decides for itself, on its sums times the pair's c_nv^m; an
            // entry somebody splits puts its two children on the next level's list
            bool split[4] = {false, false, false, false};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (match[r]) {
                    const int cnt = count[r] + 1;
                    count[r] = cnt;
                    const double cf = moment_factor(rho + 4 * r, mom);
                    const double kx = NM == 1 ? Kre[r] : Kre[r] * cf, ky = NM == 1 ? Kim[r] : Kim[r] * cf;
                    const double gx = NM == 1 ? Gre[r] : Gre[r] * cf, gy = NM == 1 ? Gim[r] : Gim[r] * cf;
                    bool sp = gk_split<SqrtSeeded>(mk(kx, ky), mk(gx, gy), scale, inv_scale, depth, P, abstol[r]);
                    if (sp && (depth >= EMME_MAX_DEPTH || cnt >= EMME_MAX_INTERVALS)) {
                        sp = false;
                        bad = 1;
                    }
                    if (!sp) {
                        sumx[r] += kx * scale;
                        sumy[r] += ky * scale;
                    }
                    split[r] = sp;
                }
            }
#if EMME_TILE_DERIV

            // ---- K' of the entry, where at least one element accepted: the operands once more from LDS (the blocks
            // are still those of this entry), the B rows formed in registers -- node 2 ks + (rho >> 1): row rho even =
            // E' + omega D', odd = D' = T E', with the column's omega.  (The padding slot's E' is 0 and its T the centre's.)
            if (__ballot((match[0] && !split[0]) || (match[1] && !split[1]) || (match[2] && !split[2]) ||
                         (match[3] && !split[3])) != 0ull) {
                v4d Dre = {0.0, 0.0, 0.0, 0.0}, Dim = Dre, D2re = Dre, D2im = Dre;
                const double2* a2 = W.q;
                const double2* b2 = W.e;
#pragma unroll
                for (int h = 0; h < KS / 8; ++h) {
                    double2 av[8], ev[8], tv[8];
#pragma unroll
                    for (int ks = 0; ks < 8; ++ks)
                        av[ks] = a2[64 * (8 * h + ks) + loff], ev[ks] = b2[32 * (8 * h + ks) + eoff],
                        tv[ks] = W.t[2 * (8 * h + ks) + (lane >> 5)];
#pragma unroll
                    for (int ks = 0; ks < 8; ++ks) {
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
                }
                Dre += D2re, Dim += D2im;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (match[r] && !split[r]) {
#if EMME_TILE_SHAPE
                        const double cf = moment_factor(rho + 4 * r, mom);
                        const double dx = NM == 1 ? Dre[r] : Dre[r] * cf, dy = NM == 1 ? Dim[r] : Dim[r] * cf;
                        sumdx[r] += dx * scale;
                        sumdy[r] += dy * scale;
#else  // (c_nv^m = 1; the form above swaps the operands of the Dre += D2re adds in the ES15 kernels)
                        sumdx[r] += Dre[r] * scale;
                        sumdy[r] += Dim[r] * scale;
#endif
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

    // ---- results (include/solver.h:448-455: mat(i,j) = -kappa W_ij dx, mirrored; electromagnetic: 472-509; the same
    // with kappa' in M') ---------
    unsigned long long my_intervals = 0;
    // (store's vx: the entry w kappa' of M' beside the entry w kappa of M, or rdw whatever the entry)
#if EMME_TILE_SETS && !EMME_TILE_DERIV
    const cd vx = mk(0.0, 0.0);
#elif !EMME_TILE_DERIV
    const cd vx = A.Mold ? rcp(mk(A.domega[b].x, A.domega[b].y)) : mk(0.0, 0.0);
#endif
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int pidx = tile * TILE_PAIRS + rho + 4 * r;
        if (has_w && pidx < A.npairs && !deferred[r]) {
            my_intervals += (unsigned long long)count[r];
            const ushort2 ij = A.pairs[pidx];
            const int i = ij.x, j = ij.y;
            cd kap = mk(P.pref * sumy[r], -(P.pref * sumx[r]));  // -i pref sum, Parameters.cpp:182
            if (kappa_bad(kap)) bad = 1;
#if EMME_TILE_DERIV
            cd kd = mk(P.pref * sumdy[r], -(P.pref * sumdx[r]));  // kappa' = -i pref sum' (+ kappa_e')
            if (kappa_bad(kd)) bad = 1;
#endif
            if (NM == 1) {
                const double w = pair_entry_weight(i, j, N, P.dx);
                const cd v = w * kap;
#if EMME_TILE_DERIV
                const cd vx = w * kd;
#endif
                store(i, j, v, vx);
                store(j, i, v, vx);
            } else {
                // blocks A (m = 0), B and its mirrors (m = 1), D (m = 2): include/solver.h:472-509
                const double de = tab[i] - tab[j], dg = tab[N + i] - tab[N + j];
                kap = kap + kappa_e(mom, P, de, dg, mk(omw.x, omw.y));
#if EMME_TILE_DERIV
                kd = kd + kappa_e_d(mom, P, de, dg, mk(omw.x, omw.y));
#endif
#if EMME_TILE_SHAPE && EMME_TILE_SETS && !EMME_TILE_DERIV
                // (this reading alone spells the A and D stores as ONE pair with a block offset.  With vx a constant the
                // three branches below end in stores of one form and the compiler merges the mom == 0 and mom == 2
                // tails.  The LLVM IR of that merge is right -- the columns are phis with i + N / j + N on the mom == 2
                // edge -- but the gfx950 code is not: the moves that give the mom == 2 lanes their columns run under the
                // mom == 0 exec mask, so D entries went to (i + N, j), (j + N, i), the C block (ROCm's
                // hipcc -O3, no upstream report yet).  The same values and addresses as the branches.  Guarded on the GPU
                // by tests/test_gpu_tile_shape_sets.py: test_fill_matches_the_oracle with _check_blocks, and the bits
                // against k_assemble_tile_shape; nothing on the host sees it.  To retire the special case: build this
                // unit with the #else form and run those tests.)
                if (mom != 1) {
                    const int off = mom == 0 ? 0 : N;
                    const double w = mom == 0 ? -(pair_weight(i, j, N) * P.dx) : P.dx;
                    const cd v = w * kap;
                    store(i + off, j + off, v, vx);
                    store(j + off, i + off, v, vx);
                } else {
                    const cd v = P.dx * kap;
                    store(i, j + N, v, vx);
                    store(j, i + N, -v, vx);
                    store(i + N, j, -v, vx);
                    store(j + N, i, v, vx);
                }
#else
                if (mom == 0) {
                    const double w = -(pair_weight(i, j, N) * P.dx);
                    const cd v = w * kap;
#if EMME_TILE_DERIV
                    const cd vx = w * kd;
#endif
                    store(i, j, v, vx);
                    store(j, i, v, vx);
                } else if (mom == 1) {
                    const cd v = P.dx * kap;
#if EMME_TILE_DERIV
                    const cd vx = P.dx * kd;
#endif
                    store(i, j + N, v, vx);
                    // (the mirrors change sign, and so do their derivatives)
#if EMME_TILE_DERIV
                    store(j, i + N, -v, -vx);
                    store(i + N, j, -v, -vx);
#else
                    store(j, i + N, -v, vx);
                    store(i + N, j, -v, vx);
#endif
                    store(j + N, i, v, vx);
                } else {
                    const cd v = P.dx * kap;
#if EMME_TILE_DERIV
                    const cd vx = P.dx * kd;
#endif
                    store(i + N, j + N, v, vx);
                    store(j + N, i + N, v, vx);
                }
#endif
            }
        }
    }
    // interval count of this wave's 16 pairs per column: the four row lanes of a column, then the workgroup's sum in
    // LDS (the three moment columns of an omega add to the same matrix's counter)
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

#if EMME_TILE_SHAPE
template <int PTS, int NM>
#if EMME_TILE_SETS && EMME_TILE_DERIV
void launch_shape(const TileShapeSetsDerivArgs& A, int ntiles, hipStream_t stream) {
#elif EMME_TILE_SETS
void launch_shape(const TileShapeSetsArgs& A, int ntiles, hipStream_t stream) {
#elif EMME_TILE_DERIV
void launch_shape(const TileShapeDerivArgs& A, int ntiles, hipStream_t stream) {
#else
void launch_shape(const TileShapeArgs& A, int ntiles, hipStream_t stream) {
#endif
    constexpr int WPG = tile_shape_waves(PTS);
    const int ntg = (ntiles + WPG - 1) / WPG;
#if EMME_TILE_SETS && EMME_TILE_DERIV
    hipLaunchKernelGGL((k_assemble_tile_shape_sets_deriv<PTS, NM>), dim3((unsigned)((long)ntg * A.nchunks)), dim3(64 * WPG), 0, stream, A);
#elif EMME_TILE_SETS
    hipLaunchKernelGGL((k_assemble_tile_shape_sets<PTS, NM>), dim3((unsigned)((long)ntg * A.nchunks)), dim3(64 * WPG), 0, stream, A);
#elif EMME_TILE_DERIV
    hipLaunchKernelGGL((k_assemble_tile_shape_deriv<PTS, NM>), dim3((unsigned)((long)ntg * A.nchunks)), dim3(64 * WPG), 0, stream, A);
#else
    hipLaunchKernelGGL((k_assemble_tile_shape<PTS, NM>), dim3((unsigned)((long)ntg * A.nchunks)), dim3(64 * WPG), 0, stream, A);
#endif
}

#endif
}  // namespace

// The launchers.  Plain readings refuse a derivative request (hipErrorNotSupported: the caller has another path);
// derivative readings have M' itself and take no fused secant, nor do the sets readings.  (sets: L.P is the context's
// own set, read for the shape only -- L.tab, L.Mold / L.Mp are not used; sets / tabs / set and seg are device arrays,
// see the argument struct; worklist_count has one counter per set)
#if EMME_TILE_SHAPE && EMME_TILE_SETS && EMME_TILE_DERIV
hipError_t launch_assemble_tile_shape_sets_deriv(const AssembleLaunch& L, const DevParams* sets, const double* tabs,
                                                 const int* set, const int* seg, unsigned long long* worklist,
                                                 unsigned int* worklist_count, const int* act_idx, const void* chunks,
                                                 int nchunks, unsigned long long* stats, hipStream_t stream) {
    TileShapeSetsDerivArgs A;
#elif EMME_TILE_SHAPE && EMME_TILE_SETS
hipError_t launch_assemble_tile_shape_sets(const AssembleLaunch& L, const DevParams* sets, const double* tabs,
                                           const int* set, const int* seg, unsigned long long* worklist,
                                           unsigned int* worklist_count, const int* act_idx, const void* chunks,
                                           int nchunks, unsigned long long* stats, hipStream_t stream) {
    TileShapeSetsArgs A;
#elif EMME_TILE_SHAPE && EMME_TILE_DERIV
hipError_t launch_assemble_tile_shape_deriv(const AssembleLaunch& L, unsigned long long* worklist,
                                            unsigned int* worklist_count, const int* act_idx, const void* chunks,
                                            int nchunks, unsigned long long* stats, hipStream_t stream) {
    TileShapeDerivArgs A;
#elif EMME_TILE_SHAPE
hipError_t launch_assemble_tile_shape(const AssembleLaunch& L, unsigned long long* worklist, unsigned int* worklist_count,
                                      const int* act_idx, const void* chunks, int nchunks, unsigned long long* stats,
                                      hipStream_t stream) {
    TileShapeArgs A;
#elif EMME_TILE_SETS && EMME_TILE_DERIV
hipError_t launch_assemble_tile_sets_deriv(const AssembleLaunch& L, const DevParams* sets, const double* tabs,
                                           const int* set, const int* seg, unsigned long long* worklist,
                                           unsigned int* worklist_count, const int* act_idx, const void* chunks,
                                           int nchunks, unsigned long long* stats, hipStream_t stream) {
    TileSetsDerivArgs A;
#elif EMME_TILE_SETS
hipError_t launch_assemble_tile_sets(const AssembleLaunch& L, const DevParams* sets, const double* tabs, const int* set,
                                     const int* seg, unsigned long long* worklist, unsigned int* worklist_count,
                                     const int* act_idx, const void* chunks, int nchunks, unsigned long long* stats,
                                     hipStream_t stream) {
    TileSetsArgs A;
#elif EMME_TILE_DERIV
hipError_t launch_assemble_tile_deriv(const AssembleLaunch& L, unsigned long long* worklist, unsigned int* worklist_count,
                                      const int* act_idx, const void* chunks, int nchunks, unsigned long long* stats,
                                      hipStream_t stream) {
    TileDerivArgs A;
#else
hipError_t launch_assemble_tile(const AssembleLaunch& L, unsigned long long* worklist, unsigned int* worklist_count,
                                const int* act_idx, const void* chunks, int nchunks, unsigned long long* stats,
                                hipStream_t stream) {
    TileArgs A;
#endif
    const int nm = L.P.dim == L.P.N ? 1 : 3;
#if EMME_TILE_SHAPE
    const bool my_shape = (L.gk_points == 15 || L.gk_points == 31) && !(L.gk_points == 15 && nm == 1);
#else
    const bool my_shape = L.gk_points == 15 && nm == 1;
#endif
#if EMME_TILE_DERIV
    if (!my_shape || !L.Md || L.Mold) return hipErrorInvalidValue;
    A.Md = (double2*)L.Md;
#else
    if (!my_shape || L.Md) return hipErrorNotSupported;
#endif
#if EMME_TILE_SETS
    if (L.Mold || !sets || !tabs || !set || !seg) return hipErrorInvalidValue;
    A.sets = sets;
    A.tabs = tabs;
    A.set = set;
    A.seg = seg;
#else
    A.P = L.P;
    A.tab = L.tab;
#if !EMME_TILE_DERIV
    A.Mold = (const double2*)L.Mold;
    A.Mp = (double2*)L.Mp;
    A.domega = (const double2*)L.domega;
#endif
#endif
    if (nchunks < 1) return hipSuccess;
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
#if EMME_TILE_SHAPE
    if (L.gk_points == 15)
        launch_shape<15, 3>(A, ntiles, stream);
    else if (nm == 3)
        launch_shape<31, 3>(A, ntiles, stream);
    else
        launch_shape<31, 1>(A, ntiles, stream);
#else
    const int ntg = (ntiles + TW - 1) / TW;
    const dim3 grid((unsigned)((long)ntg * nchunks)), block(64 * TW);
#if EMME_TILE_SETS && EMME_TILE_DERIV
    hipLaunchKernelGGL(k_assemble_tile_sets_deriv, grid, block, 0, stream, A);
#elif EMME_TILE_SETS
    hipLaunchKernelGGL(k_assemble_tile_sets, grid, block, 0, stream, A);
#elif EMME_TILE_DERIV
    hipLaunchKernelGGL(k_assemble_tile_deriv, grid, block, 0, stream, A);
#else
    hipLaunchKernelGGL(k_assemble_tile, grid, block, 0, stream, A);
#endif
#endif
    return hipGetLastError();
}

}  // namespace emme
