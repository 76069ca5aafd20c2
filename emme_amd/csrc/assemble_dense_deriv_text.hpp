// assemble_dense_deriv_text.hpp -- the ONE text of the cached derivative fills: M(omega) and the exact dM/domega from
// the tiled node cache, the dense fill (assemble_dense.hip: k_assemble_dense<1, PTS, NM>)
// with TWIN columns.  One selector, set by the including unit; the preprocessor selects the regions that differ, so each
// unit's compiler sees the token stream of a kernel written on its own (a body shared through templates
// or functions changed the register allocation of the kernels):
//
//   EMME_DENSE_DERIV_SHAPE 0  assemble_dense_deriv.hip: BtabDerivArgs, k_btab_deriv, DenseDerivArgs,
//                             k_assemble_dense_deriv, launch_btab_deriv, launch_assemble_dense_deriv -- electrostatic
//                             GK15 (no template: PTS = 15 and NM = 1 are constants inside the kernels), option
//                             deriv_cached
//   EMME_DENSE_DERIV_SHAPE 1  assemble_dense_shape_deriv.hip: BtabShapeDerivArgs, k_btab_shape_deriv<PTS, NM>,
//                             DenseShapeDerivArgs, k_assemble_dense_shape_deriv<PTS, NM>, dense_shape_deriv_chunk,
//                             launch_btab_shape_deriv, launch_assemble_dense_shape_deriv -- (PTS, NM) = (15, 3), (31, 1)
//                             and (31, 3): electromagnetic contexts and the 31-point rule, behind the context switch
//                             EMME_DERIV_CACHE_SHAPES_ALL (emme_ctx_set_deriv_cache_shapes)
//
// With folded records the Kronrod sum of an interval is K[p, w] = sum_n Q1[p, n] (w E'_n) + Q0[p, n] E'_n,
// E'_n = wk_n exp(T_n w), and from F' = exp(A0 + T w)(T (w Q1 + Q0) + Q1)
//     K'[p, w] = sum_n Q1[p, n] (E'_n + w D'_n) + Q0[p, n] D'_n,     D'_n = T_n E'_n:
// the SAME A operand (the cached 8-KB / 16-KB record block) against other B columns.  An electromagnetic column 3 w + m
// carries W^m in its E' (k_btab<PTS, NM>'s rule), and W does not depend on omega: the same two B-row formulas serve
// every moment column with that column's omega.
//
// Column layout: column c < 8 of the complex 16 x 16 x (32 | 64) GEMM is a K column, column c + 8 is K' of the same
// (omega, moment): one read of the record block feeds both, and the K' lanes own no accumulator of their own kind -- the
// register budget is the plain kernel's (k_assemble_dense<1, 31, 3> sits at the cap).  An electrostatic chunk holds 8
// omegas (K columns 0 .. 7); an electromagnetic chunk holds 2 omegas x 3 moments (K columns 3 w + m = 0 .. 5, columns
// 6, 7, 14, 15 idle).  The phase table of a launch (k_btab_deriv, k_btab_shape_deriv) keeps E' W^m in column NM w + m and
// D' = T E' W^m in column NM w + m + 8 of the block; a K' lane fetches its partner's E' with a DPP row rotate by 8.
//
// The walk is k_assemble_dense<1, PTS, NM>'s: level by level, 64-entry level lists, MFMA rounds and vector rounds, the
// same slot look-up, c_nv^m of the pair applied to K, G and K' before the decision, the same caps and the same poison
// rule.  Only K and G decide accept / split (the K columns: own abs_tol, own count); a K' element owns the entries of
// its partner (same pair, column - 8), adds scale c_nv^m K' to its own sum when the partner accepts and moves to the
// children when the partner splits; the Gauss products of the K' columns are computed and ignored.  Integrals that leave
// the cache (uncached intervals, poisoned tiles, a level list that would overflow) are queued whole by their K element
// in the plain kernel's entry format (b << 32) | (pair NM + moment); a list kernel evaluates M and M' of them from
// scratch (assemble_deriv_list_text.hpp: k_assemble_deriv_list in assemble_dense_deriv.hip,
// k_assemble_deriv_list_shape<PTS> in assemble_tile_shape_deriv.hip).
//
// What the regions hold (each was needed to keep a kernel's machine code): the struct names with their
// shape-only fields (tab, wtab, tile_major) and the locals that stand in for them; signature and template; the LDS
// asserts; the phase-table kernel's guard on a position past the chunk; the task order and the guard on a chunk past
// the last; the diagonal; the vector round's decision; in the launchers the precondition, the shape-only assignments
// and the launch.  Everything else appears once.  The small helpers (gauss_ratio, fsqrt_pos, lane_ptr) and the accept /
// split rule live in assemble_common.hpp.  k_assemble_dense and k_btab are not read from here: sharing text with the
// headline kernel moves its registers.
//
// No include guard: a text, not a header of declarations.  The including unit defines the selector and nothing else.
#ifndef EMME_DENSE_DERIV_SHAPE
#error "assemble_dense_deriv_text.hpp is read by assemble_dense_deriv.hip (EMME_DENSE_DERIV_SHAPE 0) and assemble_dense_shape_deriv.hip (1) only"
#endif
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "assemble_common.hpp"
#include "launch.hpp"
#include "launch_grid.hpp"
#include "node_cache.hpp"

namespace emme {

namespace {

constexpr int DENSE_DERIV_TWIN = 8;  // K columns 0 .. 7, their K' twins 8 .. 15
// omegas of a chunk (the planner's capacity, fill_plan.cpp: dense_deriv_capacity)
__host__ __device__ constexpr int dense_deriv_chunk(int nm) { return DENSE_DERIV_TWIN / nm; }
static_assert(dense_deriv_chunk(1) == 8 && dense_deriv_chunk(3) == 2, "twin columns: 8 omegas, or 2 omegas x 3 moments");

#if EMME_DENSE_DERIV_SHAPE
// LDS of a workgroup (4 waves): per element sum (re, im), abs_tol, interval count for 4 x 64 elements of every wave, c_nv
// of a wave's 16 pairs, the workgroup's counters.  Three workgroups of a CU (__launch_bounds__(256, 2) admits two)
// stay far below the CU's 160 KB.  (The electrostatic GK15 reading has no c_nv: 28 824 bytes.)
constexpr int SHAPE_DERIV_WG_LDS = (3 * 4 * 4 * 64 * 8 + 4 * 4 * 64 * 4 + 4 * 16 * 8 + 16 * 8 + 4 * 4 + 4 + 7) / 8 * 8;
static_assert(SHAPE_DERIV_WG_LDS == 29336, "LDS of a workgroup: DESIGN.md 12.5");
static_assert(3 * SHAPE_DERIV_WG_LDS <= 163840, "three workgroups do not fit the CU's LDS");
#endif

// Weighted phase tables of one derivative launch: per (interval slot, chunk) a block [sn][16] of (re, im) pairs (4 KB
// for GK15, 8 KB for GK31), column NM w + m: E' W^m = wk exp(T omega_w) W^m, column NM w + m + 8: D' = T E' W^m.  The
// clamp is k_btab's: exp(T omega) beyond 1e304 becomes NaN, in all the omega's columns.
#if EMME_DENSE_DERIV_SHAPE
struct BtabShapeDerivArgs {
    const double2* ttab[2];
    const double2* wtab[2];
#else
struct BtabDerivArgs {
    const double2* ttab[2];
#endif
    const double2* omega;
    const int* act_idx;
    const int* wmap;  // per position of the launch's omega list: chunk << 8 | position in the chunk
    int n_act, nchunks, nslots;
    double* btab;
};
#if EMME_DENSE_DERIV_SHAPE
template <int PTS, int NM>
__global__ __launch_bounds__(256) void k_btab_shape_deriv(BtabShapeDerivArgs A) {
    const double2* const* wtab = A.wtab;
#else
__global__ __launch_bounds__(256) void k_btab_deriv(BtabDerivArgs A) {
    constexpr int PTS = 15, NM = 1;
    const double2* const wtab[2] = {nullptr, nullptr};  // (no moment factors)
#endif
    constexpr int GW = tile_slots(PTS), BT = btab_block_doubles(PTS);
    const long total = (long)A.nslots * GW * A.n_act;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        // e = (slot * GW + lane) * n_act + wpos, as k_btab
        const long row = e / A.n_act;
        const int wpos = (int)(e - row * A.n_act);
        const int lane = (int)(row % GW);
        const int slot = (int)(row / GW);
        const double2 om = A.omega[A.act_idx[wpos]];
        const int cls = -copysign(1.0, om.x) > 0.0 ? 0 : 1;
        cd ev = mk(0.0, 0.0), tv = mk(0.0, 0.0);
        if (A.ttab[cls] && lane < PTS) {
            const double2 t = A.ttab[cls][(long)slot * GW + lane];
            tv = mk(t.x, t.y);
            const double ax = fma(t.x, om.x, -(t.y * om.y)), ay = fma(t.x, om.y, t.y * om.x);
            if (!(ax > 700.0)) {
                double sa, ca;
                sincos(ay, &sa, &ca);
                const double ea = exp(ax);
                ev = mk(ea * ca, ea * sa);
            } else {
                ev = mk(__builtin_nan(""), __builtin_nan(""));
            }
        }
        const GkLane gk = gk_lane<PTS>(lane);
        const int sn = slotnode_of_lane_t<PTS>(lane);
        const int wm = A.wmap[wpos];
        const int wq = wm & 255;
#if EMME_DENSE_DERIV_SHAPE  // (as common text it moves k_btab_deriv: DESIGN.md 12.2.3)
        if (wq >= dense_deriv_chunk(NM)) continue;  // (never planned: the dispatcher refuses such a chunk)
#endif
        double* blk = A.btab + ((size_t)slot * A.nchunks + (wm >> 8)) * BT;
        const int col = NM * wq;
        double2* bk = reinterpret_cast<double2*>(blk);
        cd bv = mk(gk.wk * ev.x, gk.wk * ev.y);
        cd dv = tv * bv;
        bk[sn * 16 + col] = make_double2(bv.x, bv.y);
        bk[sn * 16 + col + DENSE_DERIV_TWIN] = make_double2(dv.x, dv.y);
        if (NM > 1) {
            cd wv = mk(0.0, 0.0);
            if (wtab[cls] && lane < PTS) {
                const double2 w2 = wtab[cls][(long)slot * GW + lane];
                wv = mk(w2.x, w2.y);
            }
#pragma unroll
            for (int m = 1; m < NM; ++m) {
                bv = bv * wv;  // (k_btab's product, so that the K columns are the plain fill's bit for bit)
                dv = tv * bv;
                bk[sn * 16 + col + m] = make_double2(bv.x, bv.y);
                bk[sn * 16 + col + m + DENSE_DERIV_TWIN] = make_double2(dv.x, dv.y);
            }
        }
    }
}

#if EMME_DENSE_DERIV_SHAPE
struct DenseShapeDerivArgs {
    DevParams P;
    const double* tab;  // eta | g | b (electromagnetic fills: c_nv, kappa_e and the D diagonal)
#else
struct DenseDerivArgs {
    DevParams P;
#endif
    const ushort2* pairs;
    int npairs;
    CacheGeom geom;
    const double* recs[2];
    const double* recs_ext[2][NODE_CACHE_MAX_SUB - 1];
    const double* btab;
    const double* scale;
    unsigned long long* worklist;
    unsigned long long* defer_info;
    unsigned int* worklist_count;
    const int* act_idx;
    const int2* chunks;  // (first position, size <= 8 / NM) of every omega chunk
    int nchunks;
    const double2* omega;
    double2* M;
    double2* Md;
    unsigned long long* intervals;
    int* status;
    unsigned long long* stats;  // [0] dense rounds, [1] sparse rounds, [2] sparse columns, [3] tile tasks, [10] overflows
    const unsigned char* tile_poison[2];
    int dense_min_cols;  // K columns that must need an interval for the MFMA path
    int skip_lost;
#if EMME_DENSE_DERIV_SHAPE
    int tile_major;  // task order: the chunks of a tile group back to back on one XCD (else chunk-major)
#endif
};

// Lanes col < 8 are the K columns and behave as the lanes of k_assemble_dense<1, PTS, NM>; lanes col >= 8 (`is_d`)
// carry K' of column col - 8: same masks as the partner lane - 8, no decisions, their LDS sum slots hold sum'.
#if EMME_DENSE_DERIV_SHAPE
template <int PTS, int NM>
__global__ __launch_bounds__(256, 2) void k_assemble_dense_shape_deriv(DenseShapeDerivArgs A) {
    const double* const& tab = A.tab;  // (a reference: a copy at the top moves these kernels)
#else
__global__ __launch_bounds__(256, 2) void k_assemble_dense_deriv(DenseDerivArgs A) {
    constexpr int PTS = 15, NM = 1;
    const double* const tab = nullptr;  // (no electromagnetic blocks)
#endif
    constexpr int NS = tile_slots(PTS), KS = NS / 2, GKS = KS / 2;
    constexpr int TB = tile_block_doubles(PTS), BT = btab_block_doubles(PTS);
    constexpr int CAP = dense_deriv_chunk(NM);
    const DevParams& P = A.P;
    const int N = P.N, dim = P.dim;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, rho = lane >> 4;
    const bool is_d = col >= DENSE_DERIV_TWIN;
    const int kcol = col & (DENSE_DERIV_TWIN - 1);   // the K column this lane is, or is the twin of
    const int wcol = NM == 1 ? kcol : kcol / NM;     // omega position of the column in its chunk
    const int mom = NM == 1 ? 0 : kcol - wcol * NM;  // its velocity moment
    const int ntiles = (A.npairs + TILE_PAIRS - 1) / TILE_PAIRS;
    const int ntg = (ntiles + 3) / 4;  // tile groups: 4 tiles (one per wave) per workgroup
#if EMME_DENSE_DERIV_SHAPE
    int chunk = blockIdx.x / ntg;
    int tile = (blockIdx.x - chunk * ntg) * 4 + wave;
    if (A.tile_major) {
        // k_assemble_dense's electromagnetic task order: the chunks of a tile group run back to back on one XCD
        // (workgroup ids go round the eight XCDs), whose L2 serves the tile's record blocks to all but the first
        const int nch = A.nchunks;
        const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
        const int tg = (k / nch) * 8 + xcd;
        chunk = k % nch;
        tile = tg * 4 + wave;
    }
#else  // chunk-major task order only
    const int chunk = blockIdx.x / ntg;
    const int tile = (blockIdx.x - chunk * ntg) * 4 + wave;
#endif
    __shared__ unsigned long long s_iv[16];
    __shared__ unsigned int s_st[4];
    __shared__ int s_arrived;
    if (threadIdx.x < 16) s_iv[threadIdx.x] = 0ull;
    if (threadIdx.x < 4) s_st[threadIdx.x] = 0u;
    if (threadIdx.x == 0) s_arrived = 0;
    __syncthreads();
#if EMME_DENSE_DERIV_SHAPE  // (the XCD-grouped grid is rounded up)
    if (tile >= ntiles || chunk >= A.nchunks) return;
#else
    if (tile >= ntiles) return;
#endif
    const int waves_here = min(4, ntiles - (tile - wave));

    const int2 ch = A.chunks[chunk];
    const bool in_chunk = wcol < ch.y && wcol < CAP;
    const int wpos = ch.x + (in_chunk ? wcol : 0);
    const int b = A.act_idx[wpos];
    // (the lanes of a column and of its twin read the flag in one instruction: they agree)
    const bool has_w = in_chunk && !(A.skip_lost && A.status[b] != 0);
    const int cls = -copysign(1.0, A.omega[b].x) > 0.0 ? 0 : 1;
    // K lanes write M, K' lanes the same entries of M'
    double2* const out = (is_d ? A.Md : A.M) + (size_t)b * dim * dim;
#if EMME_DENSE_DERIV_SHAPE
    if (tile == 0 && has_w && mom == 0) {  // diagonals of all blocks: constant in omega, so 0 in M'
        for (int i = rho; i < N; i += 4) {
            out[(size_t)i * dim + i] = make_double2(is_d ? 0.0 : P.diag_a, 0.0);
            if (NM > 1) {
                out[(size_t)i * dim + i + N] = make_double2(0.0, 0.0);
                out[(size_t)(i + N) * dim + i] = make_double2(0.0, 0.0);
                out[(size_t)(i + N) * dim + i + N] = make_double2(is_d ? 0.0 : P.diag_d * tab[2 * N + i], 0.0);
            }
        }
    }
#else  // (the form above moves k_assemble_dense_deriv: DESIGN.md 12.2.3)
    if (tile == 0 && has_w) {  // diagonal: constant in omega, so 0 in M'
        const double dv = is_d ? 0.0 : P.diag_a;
        for (int i = rho; i < N; i += 4) out[(size_t)i * dim + i] = make_double2(dv, 0.0);
    }
#endif
    // electromagnetic: c_nv of the tile's 16 pairs (k_assemble_dense)
    __shared__ double s_cnv[4][16];
    if (NM > 1 && lane < 16) {
        const int pidx = tile * TILE_PAIRS + lane;
        double v = 0.0;
        if (pidx < A.npairs) {
            const ushort2 ij = A.pairs[pidx];
            v = (P.qR * (tab[ij.x] - tab[ij.y])) / P.vt;
        }
        s_cnv[wave][lane] = v;
    }
    // c_nv^m of pair slot q of this tile (1 for electrostatic fills)
    auto moment_factor = [&](int q, int m) -> double {
        if (NM == 1) return 1.0;
        const double cv = s_cnv[wave][q];
        return m == 0 ? 1.0 : (m == 1 ? cv : cv * cv);
    };

    const double inv_scale = 2. / (M_PI / 2.0);
    double grat[GKS];
#pragma unroll
    for (int ks = 0; ks < GKS; ++ks) grat[ks] = gauss_ratio<PTS>((4 * ks + (lane >> 4)) >> 1);
    const double grat_node = gauss_ratio<PTS>(col);  // (node slots 16 .. 31 of GK31 are Kronrod-only)
    const int loff = tile_index(lane >> 4, lane & 15);
    const int eoff = (lane >> 5) * 16 + (lane & 15);
    const double2 omw = A.omega[b];  // this lane's column omega (K' lanes: their partner's)
    const int g_dfull = A.geom.dfull;
    const bool g_on = lane < A.geom.nsub;
    const int gk = g_on ? lane : 0;
    const int g_rd = A.geom.rd[gk], g_dd = A.geom.dd[gk], g_base = A.geom.base[gk];
    const unsigned long long g_rp = A.geom.rp[gk];
    const double* g_ptr0 = gk == 0 ? A.recs[0] : A.recs_ext[0][gk - 1];
    const double* g_ptr1 = gk == 0 ? A.recs[1] : A.recs_ext[1][gk - 1];
    const unsigned long long g_blk_main = (unsigned long long)tile * (unsigned long long)A.geom.ni_main();
    const unsigned long long g_blk0 =
        gk == 0 ? g_blk_main + (unsigned long long)g_base : (unsigned long long)tile * (unsigned long long)((2 << (g_dd - g_rd)) - 1);
    // ---- the wave's K elements and their twins: element r of this lane = (pair tile*16 + rho + 4 r, column col)
    unsigned long long mcur[4], mnext[4];
    // per-element state in LDS, touched by the owner lane (dense rounds) or the column's decider lane (vector rounds):
    // K lanes: running sum of scale K, abs_tol, interval count; K' lanes: running sum of scale K' (the rest unused)
    __shared__ double s_sumx[4][4][64], s_sumy[4][4][64], s_abstol[4][4][64];
    __shared__ int s_count[4][4][64];
    bool deferred[4], alive[4];
    unsigned int ecur_lo = 0, ecur_hi = 0, enext_lo = 0, enext_hi = 0;
    int n_cur = 0;
    {
        const unsigned long long c0 = __ballot(has_w && cls == 0), c1 = __ballot(has_w && cls == 1);
        int e_of_cls[2] = {-1, -1};
        if (c0) e_of_cls[0] = n_cur++;
        if (c1) e_of_cls[1] = n_cur++;
        if (c1) ecur_hi = lane == e_of_cls[1] ? (1u << 30) : ecur_hi;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int pidx = tile * TILE_PAIRS + rho + 4 * r;
            alive[r] = has_w && pidx < A.npairs;
            mnext[r] = 0ull;
            mcur[r] = alive[r] ? (1ull << e_of_cls[cls]) : 0ull;
            s_abstol[wave][r][lane] = 0.0, s_sumx[wave][r][lane] = 0.0, s_sumy[wave][r][lane] = 0.0;
            s_count[wave][r][lane] = 0, deferred[r] = false;
        }
    }
    unsigned int n_dense = 0, n_sparse = 0, n_cols = 0;
    int bad = 0;

    // the integral leaves the cache: its K lane queues it in the plain kernel's entry format (the list kernel writes M
    // and M'), the twin just lets go
    auto defer = [&](int r, int depth, int ccls, unsigned long long path) {
        if (!is_d) {
            const unsigned int slot = atomicAdd(A.worklist_count, 1u);
            A.worklist[slot] = ((unsigned long long)b << 32) | (unsigned int)((tile * TILE_PAIRS + rho + 4 * r) * NM + mom);
            A.defer_info[slot] = ((unsigned long long)depth << 56) | ((unsigned long long)ccls << 55) | (path & 0x7fffffffffffffull);
        }
        deferred[r] = true, alive[r] = false;
        mcur[r] = 0ull, mnext[r] = 0ull;
    };

    // a tile that holds a poisoned block hands all its integrals of that contour class over (k_assemble_dense)
    if (has_w && A.tile_poison[cls] && A.tile_poison[cls][tile] != 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (alive[r]) defer(r, 0, cls, 0ull);
    }

    for (int depth = 0; n_cur > 0; ++depth) {
        int n_next = 0;
        for (int e = 0; e < n_cur; ++e) {
            const unsigned int elo = (unsigned)__builtin_amdgcn_readlane((int)ecur_lo, e);
            const unsigned int ehi = (unsigned)__builtin_amdgcn_readlane((int)ecur_hi, e);
            const int ccls = (int)(ehi >> 30);
            const unsigned long long path = (((unsigned long long)(ehi & 0x3fffffffu)) << 32) | elo;
            bool match[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) match[r] = ((mcur[r] >> e) & 1ull) != 0ull;
            const unsigned long long need = __ballot(match[0] || match[1] || match[2] || match[3]);
            if (need == 0ull) continue;
            int cslot;
            unsigned long long blk;
            const double* ebuf;
            if (depth <= g_dfull) {
                cslot = (1 << depth) - 1 + (int)path;
                blk = g_blk_main + (unsigned long long)cslot;
                ebuf = lane_ptr(ccls ? g_ptr1 : g_ptr0, 0);
            } else {
                const int sd = (depth - g_rd) & 63;
                const bool hit = g_on && depth <= g_dd && depth >= g_rd && (path >> sd) == g_rp;
                const unsigned long long hb = __ballot(hit);
                const int k = hb ? __builtin_ctzll(hb) : 0;
                const int rel = (int)((1u << sd) - 1u) + (int)(unsigned)(path & ((1ull << sd) - 1ull));
                cslot = hb ? __builtin_amdgcn_readlane(g_base + rel, k) : -1;
                const unsigned long long bl = g_blk0 + (unsigned long long)rel;
                blk = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(bl >> 32), k) << 32) |
                      (unsigned)__builtin_amdgcn_readlane((int)(unsigned)bl, k);
                ebuf = lane_ptr(ccls ? g_ptr1 : g_ptr0, k);
            }
            if (cslot < 0 || ebuf == nullptr) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (match[r]) defer(r, depth, ccls, path);
                continue;
            }
            const double* ablk = ebuf + blk * TB;
            const double* bblk = A.btab + ((size_t)cslot * A.nchunks + chunk) * BT;
            const double2* a2 = reinterpret_cast<const double2*>(ablk);
            const double2* b2 = reinterpret_cast<const double2*>(bblk);
            // the K columns that need the interval (a twin needs what its partner needs: the low 8 columns say it all)
            unsigned int colmask = (unsigned int)((need | (need >> 16) | (need >> 32) | (need >> 48)) & 0xffull);
            v4d Kre = {0.0, 0.0, 0.0, 0.0}, Kim = Kre, Gre = Kre, Gim = Kre;
            const bool dense_round = __popc(colmask) >= A.dense_min_cols;
            if (dense_round) {
                ++n_dense;
                v4d K2re = {0.0, 0.0, 0.0, 0.0}, K2im = K2re, G2re = K2re, G2im = K2re;
#pragma unroll
                for (int h = 0; h < KS / 8; ++h) {  // (GK31: two batches of eight k-steps, the Gauss rule in the first)
                    double2 av[8], ev[8];
#pragma unroll
                    for (int ks = 0; ks < 8; ++ks) av[ks] = a2[64 * (8 * h + ks) + loff], ev[ks] = b2[32 * (8 * h + ks) + eoff];
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int ks = 0; ks < 8; ++ks) {
                        // B rows 4 ks + rho belong to node 2 ks + (rho >> 1).  K column: row rho even = omega E', odd = E'.
                        // K' column: this lane loaded D'; its partner (lane - 8: row rotate by 8) loaded E' of the same
                        // node, omega and moment: row rho even = E' + omega D', odd = D'.
                        const double2 a = av[ks], ep = ev[ks];
                        const double px = dpp_mov<0x128>(ep.x), py = dpp_mov<0x128>(ep.y);
                        const double ax = is_d ? px : 0.0, ay = is_d ? py : 0.0;
                        const double2 bk = (rho & 1) ? ep
                                                     : make_double2(fma(omw.x, ep.x, fma(-omw.y, ep.y, ax)),
                                                                    fma(omw.x, ep.y, fma(omw.y, ep.x, ay)));
                        Kre = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, bk.x, Kre, 0, 0, 0);
                        Kim = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, bk.y, Kim, 0, 0, 0);
                        K2re = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, -bk.y, K2re, 0, 0, 0);
                        K2im = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, bk.x, K2im, 0, 0, 0);
                        if (8 * h + ks < GKS) {  // (the Gauss products of the K' columns are computed and ignored)
                            const double gx = a.x * grat[(8 * h + ks) % GKS], gy = a.y * grat[(8 * h + ks) % GKS];
                            Gre = __builtin_amdgcn_mfma_f64_16x16x4f64(gx, bk.x, Gre, 0, 0, 0);
                            Gim = __builtin_amdgcn_mfma_f64_16x16x4f64(gx, bk.y, Gim, 0, 0, 0);
                            G2re = __builtin_amdgcn_mfma_f64_16x16x4f64(gy, -bk.y, G2re, 0, 0, 0);
                            G2im = __builtin_amdgcn_mfma_f64_16x16x4f64(gy, bk.x, G2im, 0, 0, 0);
                        }
                    }
                }
                Kre += K2re, Kim += K2im, Gre += G2re, Gim += G2im;
            }
            const double scale = A.scale[cslot];
            bool split[4] = {false, false, false, false};
            // one decision (k_assemble_dense's): sums (kx, ky) / (gx, gy) of the K element whose state is slot [r][owner]
            auto decide = [&](int r, int owner, double kx, double ky, double gx, double gy, int& flag_bad) -> bool {
                const int cnt = s_count[wave][r][owner] + 1;
                s_count[wave][r][owner] = cnt;
                bool sp = gk_split<SqrtSeeded>(mk(kx, ky), mk(gx, gy), scale, inv_scale, depth, P,
                                               s_abstol[wave][r][owner]);
                if (sp && (depth >= EMME_MAX_DEPTH || cnt >= EMME_MAX_INTERVALS)) {
                    sp = false;
                    flag_bad = 1;
                }
                if (!sp) {
                    s_sumx[wave][r][owner] += kx * scale;
                    s_sumy[wave][r][owner] += ky * scale;
                }
                return sp;
            };
            if (!dense_round) {
                // ---- vector round: lane = node (sn = lane & 15; GK31: node slots col and col + 16), row rho takes pair
                // rho + 4 r; one K column at a time.  The second product q1 (E' + omega D') + q0 D' comes from the same
                // 32-byte record read: two more reductions, no Gauss term.
                ++n_sparse;
                const int sn = col;
                unsigned long long mb[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) mb[r] = __ballot(match[r]);
                while (colmask) {
                    const int c = __builtin_ctz(colmask);  // (a K column: < 8)
                    colmask &= colmask - 1;
                    ++n_cols;
                    auto lane_value = [&](double v) -> double {
                        const long long bits = __double_as_longlong(v);
                        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)bits, c);
                        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(bits >> 32), c);
                        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
                    };
                    const double wcx = lane_value(omw.x), wcy = lane_value(omw.y);
                    const int pmask = (col >= 8 ? 2 : 0) | ((col >> 2) & 1);
                    double pkx[4], pky[4], pgx[4], pgy[4], pdx[4], pdy[4];
#pragma unroll
                    for (int h = 0; h < NS / 16; ++h) {
                        const int snh = sn + 16 * h;
                        const double2 ep = b2[snh * 16 + c];                     // E' (W^m) of the node
                        const double2 dp = b2[snh * 16 + c + DENSE_DERIV_TWIN];  // D' = T E'
                        const cd bk0 = mk(ep.x, ep.y);
                        const cd bk1 = mk(fma(wcx, ep.x, -(wcy * ep.y)), fma(wcx, ep.y, wcy * ep.x));
                        const cd bd0 = mk(dp.x, dp.y);
                        const cd bd1 = mk(fma(wcx, dp.x, fma(-wcy, dp.y, ep.x)), fma(wcx, dp.y, fma(wcy, dp.x, ep.y)));
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int p = rho + 4 * (r ^ pmask);
                            const double4 ra = *reinterpret_cast<const double4*>(a2 + tile_index(2 * snh, p));  // (Q1, Q0)
                            const cd q1 = mk(ra.x, ra.y), q0 = mk(ra.z, ra.w);
                            const cd fk = mk(fma(q1.x, bk1.x, fma(-q1.y, bk1.y, fma(q0.x, bk0.x, -(q0.y * bk0.y)))),
                                             fma(q1.x, bk1.y, fma(q1.y, bk1.x, fma(q0.x, bk0.y, q0.y * bk0.x))));
                            const cd fd = mk(fma(q1.x, bd1.x, fma(-q1.y, bd1.y, fma(q0.x, bd0.x, -(q0.y * bd0.y)))),
                                             fma(q1.x, bd1.y, fma(q1.y, bd1.x, fma(q0.x, bd0.y, q0.y * bd0.x))));
                            if (h == 0) {
                                const cd fg = grat_node * fk;
                                pkx[r] = fk.x, pky[r] = fk.y, pgx[r] = fg.x, pgy[r] = fg.y, pdx[r] = fd.x, pdy[r] = fd.y;
                            } else {
                                pkx[r] += fk.x, pky[r] += fk.y, pdx[r] += fd.x, pdy[r] += fd.y;
                            }
                        }
                    }
                    auto mv_reduce = [&](const double (&v)[4]) -> double {
                        const double w0 = v[0] + dpp_mov<0x140>(v[3]), w1 = v[1] + dpp_mov<0x140>(v[2]);
                        double x = w0 + dpp_mov<0x141>(w1);
                        x = dpp_add_step<0xB1>(x);
                        return dpp_add_step<0x4E>(x);
                    };
                    const double mkx = mv_reduce(pkx), mky = mv_reduce(pky), mgx = mv_reduce(pgx), mgy = mv_reduce(pgy);
                    const double mdx = mv_reduce(pdx), mdy = mv_reduce(pdy);
                    // lane (col = 4 q, rho) decides for element (pair rho + 4 q, column c), whose state is slot q of the
                    // owner lane c + 16 rho; the twin's sum' is slot q of lane owner + 8
                    const int owner = c + 16 * rho;
                    const int dq = col >> 2;
                    const bool decider = (col & 3) == 0;
                    const unsigned long long mbq = dq == 0 ? mb[0] : dq == 1 ? mb[1] : dq == 2 ? mb[2] : mb[3];
                    int qbad = 0;
                    bool sp = false;
                    if (decider && ((mbq >> owner) & 1ull)) {
#if EMME_DENSE_DERIV_SHAPE
                        // (column c is wave-uniform, and so is its moment; the decider lane's pair slot is rho + 4 dq)
                        const double cf = moment_factor(rho + 4 * dq, NM == 1 ? 0 : c % NM);
                        sp = NM == 1 ? decide(dq, owner, mkx, mky, mgx, mgy, qbad)
                                     : decide(dq, owner, mkx * cf, mky * cf, mgx * cf, mgy * cf, qbad);
                        if (!sp) {
                            s_sumx[wave][dq][owner + DENSE_DERIV_TWIN] += (NM == 1 ? mdx : mdx * cf) * scale;
                            s_sumy[wave][dq][owner + DENSE_DERIV_TWIN] += (NM == 1 ? mdy : mdy * cf) * scale;
                        }
#else  // (c_nv^m = 1; the form above moves k_assemble_dense_deriv: DESIGN.md 12.2.3)
                        sp = decide(dq, owner, mkx, mky, mgx, mgy, qbad);
                        if (!sp) {
                            s_sumx[wave][dq][owner + DENSE_DERIV_TWIN] += mdx * scale;
                            s_sumy[wave][dq][owner + DENSE_DERIV_TWIN] += mdy * scale;
                        }
#endif
                    }
                    const unsigned long long sb = __ballot(sp), bb = __ballot(qbad != 0);
                    if (kcol == c) {  // the column's lanes and their twins take the verdicts
#pragma unroll
                        for (int r = 0; r < 4; ++r) split[r] = ((sb >> (4 * r + 16 * rho)) & 1ull) != 0ull;
                        if (!is_d && ((bb >> (16 * rho)) & 0xffffull)) bad = 1;
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned long long mbr = __ballot(match[r]);
                    if (mbr == 0ull) continue;  // wave-uniform
                    const double cf = moment_factor(rho + 4 * r, mom);
                    bool sp = false;
                    if (match[r] && !is_d)
                        sp = NM == 1 ? decide(r, lane, Kre[r], Kim[r], Gre[r], Gim[r], bad)
                                     : decide(r, lane, Kre[r] * cf, Kim[r] * cf, Gre[r] * cf, Gim[r] * cf, bad);
                    const unsigned long long sb = __ballot(sp);
                    if (is_d) {
                        // the partner's verdict: accept adds scale c_nv^m K' to this element's own sum
                        sp = ((sb >> (lane - DENSE_DERIV_TWIN)) & 1ull) != 0ull;
                        if (match[r] && !sp) {
                            s_sumx[wave][r][lane] += (NM == 1 ? Kre[r] : Kre[r] * cf) * scale;
                            s_sumy[wave][r][lane] += (NM == 1 ? Kim[r] : Kim[r] * cf) * scale;
                        }
                    }
                    split[r] = sp;
                }
            }
            if (__ballot(split[0] || split[1] || split[2] || split[3]) != 0ull) {
                if (n_next + 2 <= 64) {
                    const unsigned long long c0 = path << 1;
                    const unsigned int hi = ((unsigned)ccls << 30) | (unsigned)(c0 >> 32);
                    const int nl = n_next;
                    enext_lo = lane == nl ? (unsigned)c0 : (lane == nl + 1 ? (unsigned)(c0 | 1ull) : enext_lo);
                    enext_hi = (lane == nl || lane == nl + 1) ? hi : enext_hi;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (split[r]) mnext[r] |= 3ull << nl;
                    n_next += 2;
                } else {
                    // the next level's list is full: these integrals restart in the list kernel
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (split[r]) {
                            defer(r, depth, ccls, path);
                            if (A.stats && !is_d) atomicAdd(&A.stats[10], 1ull);
                        }
                }
            }
        }
        ecur_lo = enext_lo, ecur_hi = enext_hi;
        n_cur = n_next;
#pragma unroll
        for (int r = 0; r < 4; ++r) mcur[r] = mnext[r], mnext[r] = 0ull;
    }

    // ---- results: kappa = -i pref sum + kappa_e -> the moment's block scatter (k_assemble_dense; store_entry_twin's
    // three branches, each lane into its own matrix); the twin lane the same with sum' and kappa_e' -> M'
    unsigned long long my_intervals = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int pidx = tile * TILE_PAIRS + rho + 4 * r;
        if (has_w && pidx < A.npairs && !deferred[r]) {
            my_intervals += (unsigned long long)s_count[wave][r][lane];  // (0 in the twin lanes)
            const ushort2 ij = A.pairs[pidx];
            const int i = ij.x, j = ij.y;
            const cd sm = mk(s_sumx[wave][r][lane], s_sumy[wave][r][lane]);
            cd kap = mk(P.pref * sm.y, -(P.pref * sm.x));
            if (kappa_bad(kap)) bad = 1;
            auto put = [&](int rw, int c, cd v) { out[(size_t)rw * dim + c] = make_double2(v.x, v.y); };
            if (NM == 1) {
                const cd v = pair_entry_weight(i, j, N, P.dx) * kap;
                put(i, j, v);
                put(j, i, v);
            } else {
                const double de = tab[i] - tab[j], dg = tab[N + i] - tab[N + j];
                kap = kap + (is_d ? kappa_e_d(mom, P, de, dg, mk(omw.x, omw.y)) : kappa_e(mom, P, de, dg, mk(omw.x, omw.y)));
                if (mom == 0) {
                    const cd v = (-(pair_weight(i, j, N) * P.dx)) * kap;
                    put(i, j, v);
                    put(j, i, v);
                } else if (mom == 1) {
                    const cd v = P.dx * kap;
                    put(i, j + N, v);
                    put(j, i + N, -v);
                    put(i + N, j, -v);
                    put(j + N, i, v);
                } else {
                    const cd v = P.dx * kap;
                    put(i + N, j + N, v);
                    put(j + N, i + N, v);
                }
            }
        }
    }
    my_intervals += __shfl_xor(my_intervals, 16);
    my_intervals += __shfl_xor(my_intervals, 32);
    if (has_w) {
        if (my_intervals && rho == 0) atomicAdd(&s_iv[col], my_intervals);
        if (bad) A.status[b] = 1;
    }
    if (lane == 0) {
        atomicAdd(&s_st[0], n_dense);
        atomicAdd(&s_st[1], n_sparse);
        atomicAdd(&s_st[2], n_cols);
        atomicAdd(&s_st[3], 1u);
    }
    __threadfence_block();
    int arrived = 0;
    if (lane == 0) arrived = atomicAdd(&s_arrived, 1) + 1;
    arrived = __builtin_amdgcn_readfirstlane(arrived);
    if (arrived == waves_here) {
        __threadfence_block();
        if (lane < DENSE_DERIV_TWIN && has_w && A.intervals && s_iv[lane] != 0ull) atomicAdd(&A.intervals[b], s_iv[lane]);
        if (A.stats && lane < 4) atomicAdd(&A.stats[lane], (unsigned long long)s_st[lane]);
    }
}

}  // namespace

#if EMME_DENSE_DERIV_SHAPE
int dense_shape_deriv_chunk(int nm) { return dense_deriv_chunk(nm); }

hipError_t launch_btab_shape_deriv(int gk_points, int nm, int nslots, const NodeCacheView& cache, const double* omega,
                                   const int* act_idx, int n_act, const int* wmap, int nchunks, void* btab,
                                   hipStream_t stream) {
    BtabShapeDerivArgs A;
    A.wtab[0] = (const double2*)cache.wtab[0], A.wtab[1] = (const double2*)cache.wtab[1];
#else
hipError_t launch_btab_deriv(int nslots, const NodeCacheView& cache, const double* omega, const int* act_idx, int n_act,
                             const int* wmap, int nchunks, void* btab, hipStream_t stream) {
    constexpr int gk_points = 15;
    BtabDerivArgs A;
#endif
    A.ttab[0] = (const double2*)cache.ttab[0], A.ttab[1] = (const double2*)cache.ttab[1];
    A.omega = (const double2*)omega;
    A.act_idx = act_idx;
    A.wmap = wmap;
    A.n_act = n_act;
    A.nchunks = nchunks;
    A.nslots = nslots;
    A.btab = (double*)btab;
    const long total = (long)nslots * tile_slots(gk_points) * n_act;
    long blocks = (total + 255) / 256;
    if (blocks > 65535) blocks = 65535;
    if (blocks < 1) blocks = 1;
#if EMME_DENSE_DERIV_SHAPE
    if (gk_points == 31 && nm == 3)
        hipLaunchKernelGGL((k_btab_shape_deriv<31, 3>), dim3((unsigned)blocks), dim3(256), 0, stream, A);
    else if (gk_points == 15 && nm == 3)
        hipLaunchKernelGGL((k_btab_shape_deriv<15, 3>), dim3((unsigned)blocks), dim3(256), 0, stream, A);
    else if (gk_points == 31 && nm == 1)
        hipLaunchKernelGGL((k_btab_shape_deriv<31, 1>), dim3((unsigned)blocks), dim3(256), 0, stream, A);
    else
        return hipErrorNotSupported;
#else
    hipLaunchKernelGGL(k_btab_deriv, dim3((unsigned)blocks), dim3(256), 0, stream, A);
#endif
    return hipGetLastError();
}

#if EMME_DENSE_DERIV_SHAPE
hipError_t launch_assemble_dense_shape_deriv(const AssembleLaunch& L, const NodeCacheView& cache, const void* btab,
                                             unsigned long long* worklist, unsigned int* worklist_count,
                                             unsigned long long* defer_info, const int* act_idx, const void* chunks,
                                             int nchunks, unsigned long long* stats, hipStream_t stream) {
    const int nm = L.P.dim == L.P.N ? 1 : 3;
    if ((L.gk_points != 15 && L.gk_points != 31) || (L.gk_points == 15 && nm == 1) || !L.Md || L.Mold)
        return hipErrorInvalidValue;
    DenseShapeDerivArgs A;
    A.tab = L.tab;
#else
hipError_t launch_assemble_dense_deriv(const AssembleLaunch& L, const NodeCacheView& cache, const void* btab,
                                       unsigned long long* worklist, unsigned int* worklist_count,
                                       unsigned long long* defer_info, const int* act_idx, const void* chunks,
                                       int nchunks, unsigned long long* stats, hipStream_t stream) {
    if (L.gk_points != 15 || L.P.dim != L.P.N || !L.Md || L.Mold) return hipErrorInvalidValue;
    DenseDerivArgs A;
#endif
    A.tile_poison[0] = cache.tile_poison[0];
    A.tile_poison[1] = cache.tile_poison[1];
    A.P = L.P;
    A.pairs = (const ushort2*)L.pairs;
    A.npairs = L.npairs;
    A.geom = make_geom(*cache.geom);
    for (int c = 0; c < 2; ++c) {
        A.recs[c] = (const double*)cache.recs[c];
        for (int k = 0; k < NODE_CACHE_MAX_SUB - 1; ++k) A.recs_ext[c][k] = (const double*)cache.recs_ext[c][k];
    }
    A.btab = (const double*)btab;
    A.scale = cache.scale;
    A.worklist = worklist;
    A.worklist_count = worklist_count;
    A.defer_info = defer_info;
    A.act_idx = act_idx;
    A.chunks = (const int2*)chunks;
    A.nchunks = nchunks;
    A.omega = (const double2*)L.omega;
    A.M = (double2*)L.M;
    A.Md = (double2*)L.Md;
    A.intervals = L.intervals;
    A.status = L.status;
    A.stats = stats;
    A.dense_min_cols = L.dense_min_cols;
    A.skip_lost = L.skip_lost;
    if (nchunks < 1) return hipSuccess;
    const int ntiles = (L.npairs + TILE_PAIRS - 1) / TILE_PAIRS;
#if EMME_DENSE_DERIV_SHAPE
    // Electromagnetic launches: the plain fill's XCD-grouped task order -- twin columns make 2.5 times
    // the plain fill's chunks, each of which would fetch every 8-KB / 16-KB block of its tiles again.  Electrostatic
    // GK31: chunk-major, as the plain fill.  (experiment, EMME_EXP_SHAPE_DERIV_ORDER = 0 / 1: chunk-major / XCD-grouped
    // for every shape -- read at every launch, so that tools/dense_shape_deriv.py can alternate the two in one process)
    const char* order_env = std::getenv("EMME_EXP_SHAPE_DERIV_ORDER");
    A.tile_major = order_env ? (std::atoi(order_env) != 0) : (nm == 3);
    const dim3 grid(dense_tile_grid_x(ntiles, nchunks, A.tile_major != 0));
    if (nm == 3 && L.gk_points == 31)
        hipLaunchKernelGGL((k_assemble_dense_shape_deriv<31, 3>), grid, dim3(256), 0, stream, A);
    else if (nm == 3)
        hipLaunchKernelGGL((k_assemble_dense_shape_deriv<15, 3>), grid, dim3(256), 0, stream, A);
    else
        hipLaunchKernelGGL((k_assemble_dense_shape_deriv<31, 1>), grid, dim3(256), 0, stream, A);
#else  // chunk-major
    const dim3 grid(dense_tile_grid_x(ntiles, nchunks, false));
    hipLaunchKernelGGL(k_assemble_dense_deriv, grid, dim3(256), 0, stream, A);
#endif
    return hipGetLastError();
}

}  // namespace emme
