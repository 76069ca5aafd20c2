// launch.hpp -- host-visible launch descriptors of the device kernels (internal to the .so).
#pragma once
#include <hip/hip_runtime.h>

#include "emme_device.hpp"

namespace emme {

// HBM cache of the omega-independent node records (assemble_cached.hip): the full bisection
// tree down to depth dfull plus up to NODE_CACHE_MAX_SUB full subtrees (root depth rd, root
// path rp, down to depth dd).  Subtree 0 shares the main buffer with the full tree; the others
// are added at run time, each in its own buffer.
constexpr int NODE_CACHE_MAX_SUB = 12;
struct NodeCacheGeom {
    int dfull;
    int nsub;
    int rd[NODE_CACHE_MAX_SUB], dd[NODE_CACHE_MAX_SUB];
    unsigned long long rp[NODE_CACHE_MAX_SUB];
};
struct AssembleLaunch {
    DevParams P;
    int gk_points;       // 15 or 31
    int nbatch;
    int npairs;
    int items_per_group; // scheduling knob: integrals handled per lane group
    const double* tab;   // device: eta[N] | g[N] | b[N]
    const void* pairs;   // device: ushort2[npairs]
    const double* omega; // device: 2*nbatch
    const int* active;   // device or null
    double* M;           // device
    const double* Mold;  // device or null
    double* Mp;          // device or null
    const double* domega; // device (needed when Mold != null)
    unsigned long long* intervals;  // device or null
    int* status;         // device
    unsigned long long* rounds = nullptr;  // device [1], omega-lane kernel diagnostic
    // per-context options (include/emme_hip.h: emme_options_t)
    int skip_lost = 0;         // skip integrals of a matrix whose status flag is already set (Newton loop only)
    int union_sel = 2;         // union walk: intervals served per round
    int union_walk = 1;        // electrostatic GK15 on folded records: union-walk kernel (0: independent lanes)
    int coop_wide_min = 4096;  // deferred list: length from which the one-wave cooperative kernel takes over (-1 never)
    int defer_one_group = 0;   // deferred integrals by one lane group each
    int dense_min_cols = 3;    // dense fill: columns that must need an interval for the MFMA path
    int dense_stage = 1;       // dense fill (electrostatic GK15): operands through the LDS stage, fetched one entry ahead
    double* Md = nullptr;      // device or null: exact dM/domega beside M (Mold must be null)
    int mirror = 0;            // pairs / npairs are one pair of every mirror-image couple (the tiled cache's dense fill and
                               // its deferred pass, electrostatic GK15): entry (N-1-j, N-1-i) is written beside (i, j)
};
// What the launchers that read the node cache see of it: its geometry and, per contour class (omi = +1, -1), the
// main records, the run-time subtrees (null if absent), the T table, the moment-factor table and the tile-poison
// flags (null where the context has none), plus the half-widths of the cached intervals.
struct NodeCacheView {
    const NodeCacheGeom* geom;
    const void* recs[2];
    const void* recs_ext[2][NODE_CACHE_MAX_SUB - 1];
    const void* ttab[2];
    const void* wtab[2];
    const unsigned char* tile_poison[2];
    const double* scale;
};
// lanes-are-nodes kernel, without the node cache (L.Md set: k_assemble_deriv, M and dM/domega)
hipError_t launch_assemble(const AssembleLaunch& L, hipStream_t stream);
// omega-lane form (assemble_wl.hip, both kernels from assemble_wl_text.hpp): the n_act batch items listed in act_idx
// (device) share the omega-independent node data; L.active is ignored.  L.Md set: k_assemble_wl_deriv.
hipError_t launch_assemble_wl(const AssembleLaunch& L, const int* act_idx, int n_act,
                              hipStream_t stream);

// part -1 = main buffer (full tree + subtree 0), part k >= 0 = run-time subtree k+1
size_t node_cache_bytes(int gk_points, long nitems, const NodeCacheGeom& g, int part);
size_t node_ttab_bytes(int gk_points, int max_intervals);
int node_cache_intervals(const NodeCacheGeom& g);
// wtab != null: electromagnetic SHARED layout -- one record per (pair, interval, node), that of
// moment 0, plus the table of moment factors W (see emme_device.hpp::node_w)
hipError_t launch_node_cache(const AssembleLaunch& L, const NodeCacheGeom& g, int part, double omi,
                             void* recs, void* ttab, void* wtab, double* scale, bool folded,
                             hipStream_t stream);
// electromagnetic fill on the shared layout: a lane walks the three moments of a pair together
hipError_t launch_assemble_cached_em(const AssembleLaunch& L, const NodeCacheView& cache, const void* etab,
                                     unsigned long long* worklist, unsigned int* worklist_count,
                                     unsigned long long* defer_info, const int* act_idx, int n_act,
                                     const void* chunks, int nchunks, hipStream_t stream);
hipError_t launch_assemble_cached(const AssembleLaunch& L, const NodeCacheView& cache,
                                  const void* etab /*phase table of this launch, or null*/,
                                  unsigned long long* worklist, unsigned int* worklist_count,
                                  unsigned long long* defer_info, const int* act_idx, int n_act,
                                  const void* chunks /*int2[nchunks]: (first, size)*/, int nchunks,
                                  hipStream_t stream);
// exp(T omega) for every cached interval/node and the n_act omegas of a launch: etab is
// [n_intervals][GW][n_act] complex (the records must be in the folded form)
hipError_t launch_phase_table(int gk_points, int n_intervals, const NodeCacheView& cache,
                              const double* omega, const int* act_idx, int n_act, void* etab,
                              hipStream_t stream);
// integrals deferred by the cached kernels, recomputed by k_assemble_coop (a workgroup each); cache null: from
// scratch, without the node cache
hipError_t launch_assemble_list(const AssembleLaunch& L, const unsigned long long* worklist,
                                const unsigned int* count, const NodeCacheView* cache, bool folded,
                                hipStream_t stream, bool tiled = false);

// ---- dense (matrix-core) fill: assemble_dense.hip (electrostatic GK15; electromagnetic GK31) ------
// tiled record layout: see node_cache.hpp (gk_points 15: 8 KB per (tile, interval); 31: 16 KB)
size_t node_cache_bytes_tiled(long npairs, const NodeCacheGeom& g, int part, int gk_points = 15);
// tile_poison [ntiles] (device, zeroed once per contour class): set to 1 for every tile that gets a poisoned block;
// wtab (electromagnetic contexts): the moment factor W per (interval, node lane), written beside ttab
hipError_t launch_node_cache_tiled(const AssembleLaunch& L, const NodeCacheGeom& g, int part, double omi,
                                   void* recs, void* ttab, double* scale, hipStream_t stream,
                                   unsigned char* tile_poison = nullptr, void* wtab = nullptr);
// weighted phase tables of one launch: btab_bytes(cached intervals, chunks of the launch)
size_t btab_bytes(int nslots, int nchunks, int gk_points = 15);
// wmap[position in the omega list] = chunk << 8 | position of that omega in its chunk (its first column / nm)
hipError_t launch_btab(int gk_points, int nm, int nslots, const NodeCacheView& cache, const double* omega,
                       const int* act_idx, int n_act, const int* wmap, int nchunks, void* btab, hipStream_t stream);
// act_idx: the launch's omegas, cost-sorted; chunks: int2 (first position, size <= 16 / nm) per chunk.
// stats (nullable): counters (dense rounds, vector rounds, vector columns, tile tasks, ...)
hipError_t launch_assemble_dense(const AssembleLaunch& L, const NodeCacheView& cache, const void* btab,
                                 unsigned long long* worklist, unsigned int* worklist_count,
                                 unsigned long long* defer_info, const int* act_idx, int n_act,
                                 const void* chunks, int nchunks, unsigned long long* stats, hipStream_t stream,
                                 int n_wide = 0, unsigned int* overflow = nullptr);

// ---- M and the exact dM/domega from the tiled cache.  One text, assemble_dense_deriv_text.hpp, read by two units
// (DESIGN.md 12.2.3): EMME_DENSE_DERIV_SHAPE 0 -> assemble_dense_deriv.hip (electrostatic GK15),
// EMME_DENSE_DERIV_SHAPE 1 -> assemble_dense_shape_deriv.hip (electromagnetic, GK31).  Both launchers answer
// hipErrorInvalidValue to a shape of the other family, to a missing L.Md and to a set L.Mold. ------
// -- assemble_dense_deriv.hip: electrostatic GK15 --
// chunks hold <= 8 omegas: column c of a chunk's phase block is E' of omega c, column c + 8 its D' = T E'
// (btab_bytes(cached intervals, chunks) as for the plain fill)
hipError_t launch_btab_deriv(int nslots, const NodeCacheView& cache, const double* omega, const int* act_idx, int n_act,
                             const int* wmap, int nchunks, void* btab, hipStream_t stream);
hipError_t launch_assemble_dense_deriv(const AssembleLaunch& L, const NodeCacheView& cache, const void* btab,
                                       unsigned long long* worklist, unsigned int* worklist_count,
                                       unsigned long long* defer_info, const int* act_idx, const void* chunks,
                                       int nchunks, unsigned long long* stats, hipStream_t stream);
// the integrals that kernel handed over (work list of batch << 32 | pair): M and M' from scratch, a lane group each
hipError_t launch_assemble_deriv_list(const AssembleLaunch& L, const unsigned long long* worklist,
                                      const unsigned int* count, hipStream_t stream);

// -- assemble_dense_shape_deriv.hip: electromagnetic and GK31 contexts (DESIGN.md 12.5;
// k_assemble_dense_shape_deriv<PTS, NM> for (15, 3), (31, 1), (31, 3); launch_btab_shape_deriv answers
// hipErrorNotSupported to electrostatic GK15) --
// Twin columns: a chunk holds dense_shape_deriv_chunk(nm) omegas -- 8 electrostatic ones, or 2 x 3 moments; column
// nm w + m of a chunk's phase block is E' W^m of omega w, column nm w + m + 8 its D' = T E' W^m (btab_bytes(cached
// intervals, chunks, gk_points) as for the plain fill).  Work-list entries are the plain dense fill's,
// (b << 32) | (pair nm + moment): launch_assemble_deriv_list_shape finishes them.
int dense_shape_deriv_chunk(int nm);
hipError_t launch_btab_shape_deriv(int gk_points, int nm, int nslots, const NodeCacheView& cache, const double* omega,
                                   const int* act_idx, int n_act, const int* wmap, int nchunks, void* btab,
                                   hipStream_t stream);
hipError_t launch_assemble_dense_shape_deriv(const AssembleLaunch& L, const NodeCacheView& cache, const void* btab,
                                             unsigned long long* worklist, unsigned int* worklist_count,
                                             unsigned long long* defer_info, const int* act_idx, const void* chunks,
                                             int nchunks, unsigned long long* stats, hipStream_t stream);

// ---- table-free tile fill (no node cache).  One text, assemble_tile_text.hpp, read by one thin translation unit per
// kernel: EMME_TILE_SHAPE 0 -> assemble_tile.hip, assemble_tile_deriv.hip (electrostatic GK15),
// EMME_TILE_SHAPE 1 -> assemble_tile_shape.hip, assemble_tile_shape_deriv.hip (electromagnetic, GK31); the parameter-set
// readings are further down.  A plain launcher refuses L.Md with hipErrorNotSupported, a derivative launcher a missing
// L.Md or a set L.Mold with hipErrorInvalidValue; both answer so to a shape of the other family. ------
// -- assemble_tile.hip: electrostatic GK15, plain fills --
// act_idx: the launch's omegas; chunks: int2 (first position, size <= 16) per chunk, ONE contour class per chunk
// (plan_tile_chunks), the most expensive chunk first.  Integrals the kernel cannot finish (a full level list, a folded
// amplitude that is not representable) are queued on the work list: launch_assemble_list without a cache finishes them.
// stats (nullable): [0] MFMA rounds, [3] tile tasks
hipError_t launch_assemble_tile(const AssembleLaunch& L, unsigned long long* worklist, unsigned int* worklist_count,
                                const int* act_idx, const void* chunks, int nchunks, unsigned long long* stats,
                                hipStream_t stream);

// -- assemble_tile_shape.hip: the same for electromagnetic and GK31 contexts (k_assemble_tile_shape<PTS, NM> for
// (15, 3), (31, 1), (31, 3); hipErrorNotSupported for electrostatic GK15) --
// chunks hold <= 16 / nm omegas (column 3 w + m of an electromagnetic chunk); work-list entries are the dense fill's,
// (b << 32) | (pair nm + moment)
hipError_t launch_assemble_tile_shape(const AssembleLaunch& L, unsigned long long* worklist, unsigned int* worklist_count,
                                      const int* act_idx, const void* chunks, int nchunks, unsigned long long* stats,
                                      hipStream_t stream);

// -- assemble_tile_deriv.hip: M and the exact dM/domega, electrostatic GK15 (L.Md set, L.Mold null) --
// same lists and chunks (<= 16 omegas, no twin columns); K' comes from a second GEMM on the operands built for K.  The
// work list is finished by launch_assemble_deriv_list.  stats as above (the K' GEMMs are not counted as rounds)
hipError_t launch_assemble_tile_deriv(const AssembleLaunch& L, unsigned long long* worklist, unsigned int* worklist_count,
                                      const int* act_idx, const void* chunks, int nchunks, unsigned long long* stats,
                                      hipStream_t stream);

// -- assemble_tile_shape_deriv.hip: the same for electromagnetic and GK31 contexts (k_assemble_tile_shape_deriv<PTS, NM>
// for (15, 3), (31, 1), (31, 3); hipErrorInvalidValue for electrostatic GK15, without L.Md or with L.Mold) --
// chunks and work-list entries are launch_assemble_tile_shape's; the work list is finished by
// launch_assemble_deriv_list_shape
hipError_t launch_assemble_tile_shape_deriv(const AssembleLaunch& L, unsigned long long* worklist,
                                            unsigned int* worklist_count, const int* act_idx, const void* chunks,
                                            int nchunks, unsigned long long* stats, hipStream_t stream);
// the integrals that kernel handed over (work list of batch << 32 | pair nm + moment): M and M' from scratch, a lane
// group of 16 (GK15) or 32 (GK31) each, every moment's scatter
hipError_t launch_assemble_deriv_list_shape(const AssembleLaunch& L, const unsigned long long* worklist,
                                            const unsigned int* count, hipStream_t stream);

// ---- lanes-are-nodes fill over parameter sets: the two sets readings of assemble_nodes_text.hpp (whose
// one-set derivative reading is k_assemble_deriv of assemble.hip) -> assemble_sets.hip (M),
// assemble_sets_deriv.hip (M and the exact dM/domega: L.Md set, L.Mold null).  Batch item b reads the scalars
// sets[set[b]] and the tables tabs + set[b] * 3N (all three device arrays; every set has the shape of L.P: N, nm).
// L.tab and L.Mold / L.Mp are not used (no fused secant: hipErrorInvalidValue if L.Mold is set); the plain launcher
// refuses L.Md with hipErrorNotSupported. ------
hipError_t launch_assemble_sets(const AssembleLaunch& L, const DevParams* sets, const double* tabs, const int* set,
                                hipStream_t stream);
hipError_t launch_assemble_sets_deriv(const AssembleLaunch& L, const DevParams* sets, const double* tabs, const int* set,
                                      hipStream_t stream);

// ---- table-free tile fill over parameter sets (electrostatic GK15): the two sets readings of
// assemble_tile_text.hpp -> assemble_tile_sets.hip (M), assemble_tile_sets_deriv.hip (M and the exact dM/domega: L.Md
// set).  act_idx / chunks as for launch_assemble_tile, every chunk of ONE set and one contour class (plan_tile_chunks
// with host_set); sets / tabs / set as for launch_assemble_sets.  The work list has a segment per set: seg[s] (device)
// is where the segment of set s begins, worklist_count[s] its counter.  L.tab is not used; no fused secant
// (hipErrorInvalidValue if L.Mold is set).  The segments are finished by the two readings of
// assemble_sets_list_text.hpp -> assemble_sets_list.hip, assemble_sets_list_deriv.hip: blockIdx.y = set. ------
hipError_t launch_assemble_tile_sets(const AssembleLaunch& L, const DevParams* sets, const double* tabs, const int* set,
                                     const int* seg, unsigned long long* worklist, unsigned int* worklist_count,
                                     const int* act_idx, const void* chunks, int nchunks, unsigned long long* stats,
                                     hipStream_t stream);
hipError_t launch_assemble_tile_sets_deriv(const AssembleLaunch& L, const DevParams* sets, const double* tabs,
                                           const int* set, const int* seg, unsigned long long* worklist,
                                           unsigned int* worklist_count, const int* act_idx, const void* chunks,
                                           int nchunks, unsigned long long* stats, hipStream_t stream);
hipError_t launch_assemble_sets_list(const AssembleLaunch& L, const DevParams* sets, const double* tabs, int nsets,
                                     const unsigned long long* worklist, const int* seg, const unsigned int* counts,
                                     hipStream_t stream);
hipError_t launch_assemble_sets_deriv_list(const AssembleLaunch& L, const DevParams* sets, const double* tabs, int nsets,
                                           const unsigned long long* worklist, const int* seg, const unsigned int* counts,
                                           hipStream_t stream);

// ---- the same for electromagnetic and GK31 contexts: the two shape sets readings of
// assemble_tile_text.hpp -> assemble_tile_shape_sets.hip (M), assemble_tile_shape_sets_deriv.hip (M and the exact
// dM/domega: L.Md set); k_assemble_tile_shape_sets<PTS, NM> and its _deriv form for (15, 3), (31, 1), (31, 3).  The
// argument lists and error answers are those of the two launchers above, the shapes those of launch_assemble_tile_shape
// (hipErrorNotSupported / hipErrorInvalidValue for electrostatic GK15).  Chunks hold <= 16 / nm omegas of ONE set and one
// class; a work-list entry is (b << 32) | (pair nm + moment), so the segment of a set must hold npairs * nm entries per
// item of the set.  The segments are finished by the two shape readings of assemble_sets_list_text.hpp
// (EMME_SETS_LIST_SHAPE 1) -> assemble_sets_list_shape.hip, assemble_sets_list_shape_deriv.hip:
// k_assemble_sets_list_shape<PTS> / k_assemble_sets_deriv_list_shape<PTS>, blockIdx.y = set, a lane group of 16 (GK15)
// or 32 (GK31) per entry, every moment's scatter.  Their launchers refuse electrostatic GK15 as the two above refuse
// every other shape. ------
hipError_t launch_assemble_tile_shape_sets(const AssembleLaunch& L, const DevParams* sets, const double* tabs,
                                           const int* set, const int* seg, unsigned long long* worklist,
                                           unsigned int* worklist_count, const int* act_idx, const void* chunks,
                                           int nchunks, unsigned long long* stats, hipStream_t stream);
hipError_t launch_assemble_tile_shape_sets_deriv(const AssembleLaunch& L, const DevParams* sets, const double* tabs,
                                                 const int* set, const int* seg, unsigned long long* worklist,
                                                 unsigned int* worklist_count, const int* act_idx, const void* chunks,
                                                 int nchunks, unsigned long long* stats, hipStream_t stream);
hipError_t launch_assemble_sets_list_shape(const AssembleLaunch& L, const DevParams* sets, const double* tabs, int nsets,
                                           const unsigned long long* worklist, const int* seg,
                                           const unsigned int* counts, hipStream_t stream);
hipError_t launch_assemble_sets_deriv_list_shape(const AssembleLaunch& L, const DevParams* sets, const double* tabs,
                                                 int nsets, const unsigned long long* worklist, const int* seg,
                                                 const unsigned int* counts, hipStream_t stream);

// tr(A_b^-1 B_b) by partial-pivot LU of the augmented system [A | B]; A, B destroyed.
hipError_t launch_trace_solve(int n, int nbatch, double* A, double* B, const int* active,
                              double* tr /*2*nbatch*/, int* info, hipStream_t stream);

// dst1[b] = src[b] (and dst2[b], if given) for the active n x n matrices of the batch
hipError_t launch_copy_active(int n, int nbatch, const double* src, double* dst1, double* dst2,
                              const int* active, hipStream_t stream);

// Mp[b] = (M[b] - Mold[b]) / domega[b], Mold[b] = M[b], work[b] = M[b] (if given) for the active matrices: the secant
// of a Newton step (include/solver.h:157) and the copies of the next one, in one pass
hipError_t launch_secant_copy(int n, int nbatch, const double* M, double* Mold, double* work, double* Mp,
                              const double* domega, const int* active, hipStream_t stream);

// the same for matrices that are symmetric bit for bit (every fill kernel writes an entry with its mirror): reads the
// upper triangles only; Mold is afterwards valid in its upper triangle only
hipError_t launch_secant_copy_sym(int n, int nbatch, const double* M, double* Mold, double* work, double* Mp,
                                  const double* domega, const int* active, hipStream_t stream);

// Blocked version (linstep_blocked.hip): whole L21 panel in LDS for n <= 525 (trace_solve_blocked_lds(n) <= 150 KB),
// in chunks up to 1024.
// nwg workgroups per matrix (1: one does everything; > 1: one factors A, the others carry B's
// columns; `items` = device list of the nitems matrices to work on, null for all of them);
// `scratch` holds trace_solve_blocked_scratch(n, nbatch) bytes.
size_t trace_solve_blocked_lds(int n);
size_t trace_solve_chunked_lds(int n);  // 525 < n <= 1024: panel rows in chunks (helper workgroups required;
                                        // the launcher returns hipErrorNotSupported when it cannot)
size_t trace_solve_blocked_scratch(int n, int nbatch);
// What an LU launch turned out to be (emme_ctx_linstep_kernel_symbol): the kernel as rocprofv3 prints it and the
// workgroups each matrix got.  The launcher below decides both itself -- one workgroup per matrix where the grid of a
// split launch cannot be resident -- and fills it in only where it launches.
struct LuRoute {
    const char* symbol = "";
    int nwg = 0;
};
constexpr const char* LU_SYM_BLOCKED_ONE = "k_trace_solve_blocked<false, false>";
constexpr const char* LU_SYM_BLOCKED_SPLIT = "k_trace_solve_blocked<true, false>";
constexpr const char* LU_SYM_BLOCKED_CHUNKED = "k_trace_solve_blocked<true, true>";
constexpr const char* LU_SYM_GROUPED = "k_trace_solve_grouped";
constexpr const char* LU_SYM_UNBLOCKED = "k_trace_solve";
constexpr const char* LU_SYM_INPLACE = "k_lu_inplace";
constexpr const char* LU_SYM_INPLACE_UNBLOCKED = "k_lu_unblocked_inplace";
hipError_t launch_trace_solve_blocked(int n, int nbatch, double* A, double* B, const int* active,
                                      double* tr, int* info, int nwg, const int* items, int nitems,
                                      void* scratch, hipStream_t stream, int group_min_n = 256, int spin_limit = 0,
                                      LuRoute* route = nullptr);

// ---- the trace-secant step folded into two half-size problems (linstep_fold.hip) ---------
// For symmetric matrices of even order n = 2m that are centrosymmetric apart from their last row and column.  Half
// problem 2b is the even (+) block of chain b, 2b + 1 the odd (-) one; all pointers device memory.
// vecs [nbatch][4][m] complex: the folds of u and u'; act2 [2 nbatch]: the half problems' live flags
hipError_t launch_fold_edges(int n, int nbatch, const double* M, const double* Mold, const double* domega,
                             const int* active, double* vecs, int* act2, hipStream_t stream);
// S1 = S2 = S and D1 = D2 = S' = (S - S_old) / domega of every live chain, [2 nbatch][m][m] each, from the upper
// triangles of M and Mold; Mold_w (nullable): M_old = M there, upper triangle only.  Runs behind launch_fold_edges.
hipError_t launch_fold_pass(int n, int nbatch, const double* M, const double* Mold, double* Mold_w, double* S1, double* S2,
                            double* D1, double* D2, const double* domega, const int* active, hipStream_t stream);
// the rank-2 part of every listed half problem (items: device list of nitems, null = 0 .. nitems-1) from its factors
// S_lu / rowmaps / nb / lu_info (launch_lu_inplace), S' (Sp) and vecs: part holds fold_part_bytes(nbatch) bytes
size_t fold_part_bytes(int nbatch);
hipError_t launch_fold_solve(int m, const double* S_lu, const int* rowmaps, int nb, const int* items, int nitems,
                             const int* lu_info, const double* Sp, const double* vecs, double* part, hipStream_t stream);
// tr[b], info[b] of the live chains from tr2 / info2 [2 nbatch] of the trace kernel on [S | S'], lu_info and part
hipError_t launch_fold_combine(int n, int nbatch, const int* active, const double* tr2, const int* info2, const int* lu_info,
                               const double* part, double* tr, int* info, hipStream_t stream);

// ---- nullSpace (nullspace.hip): factorisation alone + inverse iteration --------------------------------
// P A = L U in place (multipliers left of the pivots, rows never moved), no right-hand sides; for orders whose
// panel fits one workgroup's LDS (hipErrorNotSupported otherwise).  scratch as for launch_trace_solve_blocked.
hipError_t launch_lu_inplace(int n, int nbatch, double* A, const int* items, int nitems, int* info, void* scratch,
                             hipStream_t stream);
int trace_solve_nb();  // rows per panel = rows per row-order snapshot of the blocked factorisations
// row-order snapshots inside a blocked factorisation's scratch: logical row x of matrix b is physical row
// maps[(b ceil(n / nb) + x / nb) n + x]
const int* trace_solve_rowmaps(const void* scratch, int n, int nbatch);
// any order up to ~8000: unblocked, slow; maps [nbatch][n] receives the row order (one snapshot, nb = n); items
// (device list of nitems batch indices, null = all nbatch): the matrices to factor
hipError_t launch_lu_unblocked_inplace(int n, int nbatch, double* A, int* maps, int* info, hipStream_t stream,
                                       const int* items = nullptr, int nitems = 0);
size_t null_iterate_lds(int n);  // dynamic LDS of a solve workgroup: trisolve::frame_lds(n) of tri_solve.hpp, for host code
// right singular vector of the smallest singular value of every matrix, from its in-place LU: vecs [nbatch][n]
// complex, info 0 / lu_info's code / EMME_ENUMERIC for a non-finite result
hipError_t launch_null_iterate(int n, const double* A_lu, const int* rowmaps, int nb, const int* items, int nitems,
                               const int* lu_info, double* vecs, int* info, int max_sweeps, hipStream_t stream);

// ---- Newton on the eigenpair (eigpair.hip) ------------------------------------------------
// One step per listed matrix (items: device list of nitems batch indices, null = 0 .. nitems-1; active, nullable: an
// item whose flag is 0 is left alone): resid[b] = |M v| / |M|_F on the un-factored M, u = M^-1 M' v through the factors
// A_lu / rowmaps / nb / lu_info of launch_null_iterate, tau[b] = v^H u, vecs[b] <- u / |u|.  first: v is not read but
// started at M^-1 s / |M^-1 s|, s[i] = (1 + 0.37 sin(1 + i)) + 0.21 cos(2 i) i (include/emme_hip.h).  info[b]: 0,
// lu_info's code (vector, tau and resid NaN) or EMME_ENUMERIC for a non-finite tau or u.  n <= 2048
// (null_iterate_lds(n) of LDS).  Two runs are bit-identical.
hipError_t launch_eigpair_step(int n, const double* M, const double* Mp, const double* A_lu, const int* rowmaps, int nb,
                               const int* items, int nitems, const int* active, const int* lu_info, double* vecs,
                               double* tau, double* resid, int* info, bool first, hipStream_t stream);
// The secant reading (k_eigpair_secant_step): Mold = the previous plain fill M(omega_k-1), domega (device, complex per
// batch item) = omega_k - omega_k-1, and u = M^-1 (M - Mold) v / domega with the difference taken per entry inside the
// one pass that also gives M v and |M|_F^2; no M' exists.  Everything else as launch_eigpair_step; a zero or non-finite
// domega gives EMME_ENUMERIC.
hipError_t launch_eigpair_secant_step(int n, const double* M, const double* Mold, const double* domega, const double* A_lu,
                                      const int* rowmaps, int nb, const int* items, int nitems, const int* active,
                                      const int* lu_info, double* vecs, double* tau, double* resid, int* info, bool first,
                                      hipStream_t stream);
// ---- the secant eigenpair step folded into two half-size problems (eigpair_fold.hip) -----
// Behind launch_fold_edges, launch_fold_pass and launch_lu_inplace on the first copy of S (half problem 2b: the even
// block of chain b, 2b + 1 the odd one; m = n / 2; all pointers device memory).  Per listed half problem (items: device
// list of nitems, null = 0 .. nitems-1): the fold of the chain's vector, y = S v and z = S' v from the kept copies S and
// Sp, the four solves on the factors S_lu / rowmaps / nb / lu_info, its dot products; active (nullable, per chain): a
// listed half problem or chain whose flag is 0 is left alone, as in launch_eigpair_secant_step.  hv holds
// eigpair_fold_vec_bytes(n, nbatch) bytes, part eigpair_fold_part_bytes(nbatch); null_iterate_lds(m) of LDS.
size_t eigpair_fold_vec_bytes(int n, int nbatch);
size_t eigpair_fold_part_bytes(int nbatch);
hipError_t launch_eigpair_fold_half(int n, const double* S_lu, const int* rowmaps, int nb, const int* items, int nitems,
                                    const int* active, const int* lu_info, const double* S, const double* Sp, const double* edges,
                                    const double* vecs, double* hv, double* part, hipStream_t stream);
// Per chain (items: the same list, both half problems of every chain side by side, nchains = nitems / 2; null = chains
// 0 .. nchains-1): tau[b], the new unit vector in vecs[b], resid[b] = |M v| / |M|_F before the step (the edge terms of
// |M|_F from M itself) and info[b]: 0; k > 0: the even (k <= m) or the odd block (k - m) met an exactly zero pivot
// column; n + 1: the 2 x 2 matrix of the rank-2 correction is singular or not finite; EMME_ENUMERIC: a zero or
// non-finite domega, tau or u.  Vector, tau and resid are NaN for every non-zero info.  Two runs are bit-identical.
hipError_t launch_eigpair_fold_combine(int n, const int* items, int nchains, const int* active, const double* M, const double* domega,
                                       const double* edges, const int* lu_info, const double* hv, const double* part,
                                       double* vecs, double* tau, double* resid, int* info, hipStream_t stream);
// the residual alone, in the same order of sums: no factors are read, vecs is left as it is
hipError_t launch_eigpair_resid(int n, const double* M, const int* items, int nitems, const double* vecs, double* resid,
                                hipStream_t stream);

// ---- bilinear forms on matrix differences (sym_forms.hip) ----------------------------------
// Item t (a, b, x, y: device lists of nitems; b or B null: no second matrix, y null: y = x): part receives the partial
// sums of f = x^T (A_a - B_b) y and s = |A_a - B_b|_F^2, the difference taken per entry -- 4 doubles per (item, block of
// 64 rows), sym_forms_blocks(n, split) blocks per item; launch_sym_forms_finish adds them in index order.  The bits of
// a result depend on n and the data alone.  split = false: one workgroup per item (one block; other bits), kept for
// the measurement of the split.  n <= 2048 (hipErrorNotSupported above); A, B, vecs are not modified.
int sym_forms_blocks(int n, bool split = true);
hipError_t launch_sym_forms(int n, const double* A, const double* B, const double* vecs, const int* a, const int* b,
                            const int* x, const int* y, int nitems, double* part, bool split, hipStream_t stream);
// What k_sym_forms_finish makes of the partial sums (all pointers device):
//   SYM_FORMS_PLAIN      count items: form[t] (complex), fro2[t] (nullable)
//   SYM_FORMS_BASE       count roots, root g from the items 2g = (M, v), 2g + 1 = (M', v): with r = root[g] and
//                        vnorm2[r] = |v|^2, denom[r] = v^T M' v, corr[r] = -v^T M v / denom, cond[r] = |M|_F |v|^2 /
//                        |denom|, info[r] = 0, 1 (|denom| <= 64 n eps |M'|_F |v|^2: corr NaN) or EMME_ENUMERIC (a
//                        non-finite form: everything NaN)
//   SYM_FORMS_NEIGHBOUR  count items, item t = (M+, M-, v) of root r = root[t], output slot q = slot[t]:
//                        dwdp[q] = -f / (dp[q] denom[r]); NaN where info[r] != 0 or f is not finite
enum { SYM_FORMS_PLAIN = 0, SYM_FORMS_BASE = 1, SYM_FORMS_NEIGHBOUR = 2 };
struct SymFormsFinish {
    int mode, count, nblk, n;
    const double* part;
    double *form, *fro2;
    const int *root, *slot;
    const double *vnorm2, *dp;
    double *denom, *corr, *cond, *dwdp;
    int* info;
};
hipError_t launch_sym_forms_finish(const SymFormsFinish& F, hipStream_t stream);

// QR-secant form of the step (linstep_qr.hip, reference include/solver.h:210-383): Wt holds the
// TRANSPOSE of each matrix (destroyed), Mp the secant derivative (read only); writes
// tr = t_n / R_nn so that domega = -1/tr = -R_nn / t_n; info = k > 0 when R11(k,k) == 0.
size_t qr_secant_lds(int n);
hipError_t launch_qr_secant(int n, int nbatch, double* Wt, const double* Mp, const int* active,
                            double* tr, int* info, hipStream_t stream);
// out_b = in_b^T for every active item (n x n complex, row-major)
hipError_t launch_transpose(int n, int nbatch, const double* in, double* out, const int* active,
                            hipStream_t stream);

// domega = -1/tr; omega += domega; iters += 1; active = !(|domega| < tol |omega|) && info == 0
// (include/solver.h:139-140, src/main.cpp:53-56). `iterates` (nullable) records omega.
hipError_t launch_newton_update(int nbatch, const double* tr, double* omega, double* domega,
                                int* active, int* iters, const int* info, double tol,
                                double* iterates, int iter_index, int iter_stride,
                                hipStream_t stream, double* pub_omega = nullptr /* pinned host, all omegas */,
                                const int* lost = nullptr /* status flags: a flagged chain retires with EMME_ENUMERIC */);

// active == 2 ("converged, last step done") -> 0; pub_* (pinned host, nullable): the flags, the interval
// counters and the deferred-integral count for the host to read after its next synchronisation
hipError_t launch_retire(int nbatch, int* active, hipStream_t stream, int* pub_active = nullptr,
                         const unsigned long long* intervals = nullptr, unsigned long long* pub_intervals = nullptr,
                         const unsigned int* deferred = nullptr, unsigned int* pub_deferred = nullptr,
                         unsigned int* overflow = nullptr, unsigned int* pub_overflow = nullptr);
// small integer lists from a pinned host block to device memory: dst1 <- src[0..n1), dst2 <- src[n1..n1+n2)
hipError_t launch_stage_ints(const int* src_pinned, int* dst1, int n1, int* dst2, int n2, hipStream_t stream);

// Mp = (M - Mold) / domega, elementwise (include/solver.h:54-57), for active items.
hipError_t launch_secant(int nbatch, size_t nn, const double* M, const double* Mold,
                         const double* domega, const int* active, double* Mp, hipStream_t stream);

// ---- probes (probe.hip): one building block of emme_device.hpp per thread, for tests and tooling ------------------
// bessel_miller on n complex arguments (device pointers): out[4n] = y0, y1, mu + y0, -/+ z
hipError_t launch_bessel_probe(const double* z, int n, double* out, hipStream_t stream);
// one math primitive (fn = EMME_FN_* of include/emme_hip.h) on n arguments (device pointers): one double in and out
// per item for frcp / frsqrt / fexp, one in and (sin, cos) out for fsincos, (re, im) in and out for the complex rcp
hipError_t launch_elementary_probe(int fn, const double* x, int n, double* out, hipStream_t stream);
// the pointwise integrand of n items (pair, moment, abscissa, omega; device pointers) in formulation `form`
// (EMME_FORM_*); out holds integrand_probe_doubles(form) doubles per item
struct IntegrandProbe {
    DevParams P;
    int form, n;
    const double* tab;  // eta[N] | g[N] | b[N]
    const int *i, *j, *m;
    const double* x;
    const double* omega;  // 2n
    double* out;
};
__host__ __device__ constexpr int integrand_probe_doubles(int form) {
    return form == 1 ? 4 : form == 2 ? 10 : 2;
}
hipError_t launch_integrand_probe(const IntegrandProbe& A, hipStream_t stream);

}  // namespace emme
