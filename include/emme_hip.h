/* emme_hip.h -- C ABI of the MI355X (gfx950) dispersion-matrix assembly + eigenvalue
 * search.  Plain pointers and sizes only; no C++ or torch types cross this boundary.
 *
 * The reference (ssskkkky/EMME) has no FFI; these entry points sit behind its two
 * de-facto operator seams and its solve-once driver:
 *
 *   emme_params_from_json   <- util::json::parse + Parameters::generate
 *                              (reference src/JsonParser.cpp:655-669, src/Parameters.cpp:10-66)
 *   emme_assemble_batch     <- EigenSolver<T>::matrixAssembler(matrix_type&)
 *                              (reference include/solver.h:417-515), batched over omega
 *   emme_newton_step_batch  <- EigenSolver<T>::newtonTraceSecantIteration()
 *                              (reference include/solver.h:113-160; LAPACK_zsysv call :134-136)
 *   emme_solve_roots        <- solve_once_eigen loop (reference src/main.cpp:19-80) +
 *                              EigenSolver ctor (include/solver.h:396-415), batched over guesses
 *
 * Conventions: every function returns 0 on success or a negative EMME_E* code (never
 * throws); emme_last_error() gives the text for the calling thread.  Per-item `info`
 * follows LAPACK: 0 ok, k>0 = factor U(k,k) exactly zero (include/solver.h:142-153).
 * Complex numbers are interleaved (re,im) doubles == std::complex<double> == the layout
 * of the reference's Matrix<std::complex<double>> (row-major, include/Matrix.h:43).
 * Buffers are caller-owned and may be host or device pointers (detected with
 * hipPointerGetAttributes); the context owns all device scratch.  Calls on one context
 * must be serialised by the caller; different contexts are independent.
 */
#ifndef EMME_HIP_H
#define EMME_HIP_H

#include <stddef.h>

#include "emme_params.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EMME_OK 0
#define EMME_EINVAL (-1)   /* bad argument                                        */
#define EMME_EJSON (-2)    /* JSON syntax error / missing key / wrong type        */
#define EMME_EDEVICE (-3)  /* no gfx950 device / HIP runtime failure              */
#define EMME_ENOMEM (-4)   /* device or host allocation failed                    */
#define EMME_ECONFIG (-5)  /* unsupported configuration (e.g. start points != 15|31) */
#define EMME_ENUMERIC (-6) /* quadrature depth cap hit or non-finite result       */

typedef struct emme_ctx emme_ctx_t;

/* Per-kernel device timing, filled when profiling is enabled (hipEvents recorded on the
 * context's stream around every launch). */
typedef struct emme_profile {
    double assemble_ms;       /* total time in the main fill kernel (cached / omega-lane /
                                 lanes-are-nodes, whichever the context dispatches)     */
    long assemble_launches;
    double deferred_ms;       /* fill of integrals the cached kernel deferred (work list) */
    long deferred_launches;
    double linstep_ms;        /* total time in the LU + trace kernel                */
    long linstep_launches;
    double other_ms;          /* copies / elementwise kernels                       */
    long other_launches;
    long long gk_intervals;   /* Gauss-Kronrod intervals evaluated (all launches)    */
    long long integrand_evals; /* = intervals * integration_start_points             */
    long long matrices;       /* matrices assembled                                  */
    long long union_rounds;   /* omega-lane kernel: interval rounds walked by lane groups */
    double cache_build_ms;    /* k_node_cache launches (node-record cache, once per context) */
    long cache_build_launches;
    double cache_alloc_ms;    /* host wall time spent allocating the cache buffers (hipMalloc) */
    /* dense (matrix-core) fill: interval rounds of the (16 pairs x 16 omegas) tile tasks */
    long long dense_rounds;   /* served by 48 v_mfma_f64_16x16x4_f64 each                 */
    long long sparse_rounds;  /* served on the vector ALU, one omega column at a time      */
    long long sparse_columns;
    long long tile_tasks;
    double nullspace_ms;      /* nullSpace: factorisation + inverse iteration launches (version 3) */
    long nullspace_launches;
} emme_profile_t;

/* Per-context options (version 3).  emme_options_default() fills in what emme_ctx_create uses; a caller
 * changes what it needs and passes the struct to emme_ctx_create_ex / emme_ctx_set_options.  The EMME_*
 * environment variables of earlier versions remain as DEVELOPER overrides only: they are read once, when a
 * context is created, and win over the struct (DESIGN.md appendix lists them). */
#define EMME_FILL_AUTO 0   /* dense (matrix-core) fill where it applies, else union walk / independent lanes */
#define EMME_FILL_UNION 1  /* never the dense fill: 48-byte records, union-walk kernel (electrostatic GK15)   */
#define EMME_FILL_LANES 2  /* independent lanes on 48-byte records                                            */
typedef struct emme_options {
    int size;                 /* sizeof(emme_options_t) of the caller (set by emme_options_default)      */
    /* ---- HBM node cache ---- */
    double node_cache_gb;     /* budget, both contour classes together (176); 0: never build one         */
    int cache_min_batch;      /* build the cache only for calls with at least this many omegas (8)       */
    int cache_min_depth;      /* shallowest full tree worth caching; 0 = 6 (tiled layout) / 5            */
    /* ---- fill routing (layout options are fixed once the context exists) ---- */
    int fill;                 /* EMME_FILL_*                                                             */
    int phase_table;          /* 1: folded records + per-launch phase table; 0: unfolded records         */
    int em_shared;            /* 1: electromagnetic contexts share one record per pair between moments   */
    int wl_min;               /* smallest uncached batch that takes the omega-lane kernel (4)            */
    int union_sel;            /* union walk: intervals a lane group serves per round (1, 2, 4)           */
    int union_ipg_few, union_few_chunks;  /* union walk: items per lane group in launches of few chunks  */
    int coop_wide_min;        /* deferred-list length from which the one-wave cooperative kernel takes over; -1 never */
    int defer_one_group;      /* 1: deferred integrals by one lane group each                            */
    int dense_min_cols;       /* dense fill: omega columns that must need an interval for the MFMA path   */
    int dense_min_tasks;      /* dense fill: chunk capacity is halved while a launch has fewer tile tasks */
    int tile_uncached;        /* (addition within version 4, in the four bytes that used to pad dense_cost_ratio to its
                                 alignment: every other field keeps its offset and the size is unchanged)
                                 1: plain fills of electrostatic GK15 contexts (integration_accuracy >= 1e-9) that have no
                                 node cache to read build the dense fill's operands in LDS and run on the FP64 matrix
                                 cores (k_assemble_tile) instead of the omega-lane kernel; 0 (default):
                                 the omega-lane kernel.  Together with deriv_cached = 1 the same holds for derivative
                                 fills with host omegas (k_assemble_tile_deriv); alone it leaves them
                                 on the omega-lane derivative kernel.  Not a layout option: it may change on a live
                                 context   */
    double dense_cost_ratio;  /* dense fill: a chunk ends where an omega costs less than 1/ratio of its first */
    int dense_wide;           /* dense fill, level lists of 128 instead of 64 entries: 0 = for the omegas of a root search
                                 whose lists overflowed in their previous fill, 1 = always (tests)                */
    int skip_lost;            /* 1: integrals of a matrix that already holds a non-finite entry are skipped */
    /* ---- Newton linear step ---- */
    int lu_split;             /* workgroups per matrix: 0 = by live matrices and order, k = k             */
    int lu_group_min_n;       /* smallest order that takes the grouped trailing updates (256); -1 never   */
    int lu_spin_limit;        /* polls before a hand-over wait of the multi-workgroup LU gives up         */
    int lu_unblocked;         /* 1: the unblocked LU                                                      */
    /* ---- exact derivative (addition within version 4: present if size covers it) ---- */
    int deriv_cached;         /* 1: derivative fills of electrostatic GK15 contexts with the tiled node cache read and
                                 grow that cache (k_assemble_dense_deriv): derivative fills follow the
                                 plain fills' policy.  Electromagnetic and GK31 contexts with the tiled cache do the same
                                 once emme_ctx_set_deriv_cache_shapes(EMME_DERIV_CACHE_SHAPES_ALL) is set
                                 (k_assemble_dense_shape_deriv<PTS, NM>); with the shapes at their
                                 default they keep the uncached kernels bit for bit.  Where that policy finds no cache to read (no budget, a cache that
                                 does not fit, a call below cache_min_batch, the minority contour class of a call) and
                                 tile_uncached = 1 is set as well, they go through the table-free tile fill
                                 (k_assemble_tile_deriv, DESIGN.md 12.3: electrostatic GK15, integration_accuracy >= 1e-9,
                                 at least wl_min omegas; no tiled layout or cache budget needed); alone, such fills keep
                                 the uncached kernels bit for bit.  0 (default): always the uncached vector kernels.
                                 Not a layout option: it may change on a live context                        */
    int dense_stage;          /* (addition within version 4, in the four bytes that used to pad the struct to its
                                 alignment: every other field keeps its offset and the size is unchanged)
                                 1 (default): the dense fill of electrostatic GK15 contexts takes its operand blocks
                                 through a stage in LDS that is filled one entry ahead; 0: every entry
                                 loads its own operands.  Same results bit for bit.  Not a layout option: it may
                                 change on a live context                                                    */
} emme_options_t;

const char* emme_last_error(void);
int emme_params_sizeof(void);
int emme_version(void); /* 4: emme_contour_t, emme_contour_default, emme_find_roots_in_contour,
                           emme_contour_moments_batch, emme_contour_eigs;
                           3: emme_options_t, emme_ctx_create_ex / _set_options / _get_options, emme_null_vectors_batch,
                           emme_profile_t grew nullspace_*; 2: cache_* fields, emme_comm_*, emme_gather_roots */
void emme_options_default(emme_options_t* opt);

/* JSON text -> raw + derived parameters.  Reproduces the reference parser's grammar
 * (a number token is a float only if it contains '.', else atoi; no string escapes)
 * and its "Failed to accessing key: <k>" errors.  Scan objects {head,step,tail} are
 * replaced by their head (reference src/main.cpp:174-180). */
int emme_params_from_json(const char* json_text, emme_params_t* out);
/* Fill derived members from raw ones (reference src/Parameters.cpp:36-66, 211-223). */
int emme_params_derive(emme_params_t* p);

/* Host-side tables exactly as the device uses them (for tests / tooling):
 * eta[N], g[N] = g_integration_f(eta), b[N] = bi(eta); returns dx in *dx. */
int emme_tables(const emme_params_t* p, double* eta, double* g, double* b, double* dx);
/* SingularityHandler weight W(i,j) (reference src/singularity_handler.cpp:3-24). */
double emme_weight(int n, int i, int j);

/* The Bessel helper alone, evaluated on the device exactly as the fill kernels do (tests and
 * tooling): util::bessel_i_alter_helper (reference include/functions.h:381-408) for n complex
 * arguments z (2n doubles, host); out: 8n doubles = {y0, y1, mu + y0, Re z < 0 ? z : -z} each. */
int emme_bessel_batch(const double* z, int n, double* out);

/* One context per (device, parameter set). device < 0 => current device. */
int emme_ctx_create(const emme_params_t* p, int device, emme_ctx_t** out);
/* The same with options (NULL = defaults).  EMME_EINVAL for a struct of the wrong size or values out of range. */
int emme_ctx_create_ex(const emme_params_t* p, int device, const emme_options_t* opt, emme_ctx_t** out);
/* Change the options of a live context.  Everything takes effect from the next call on, except what fixes the
 * layout of the node cache (fill, phase_table, em_shared): EMME_EINVAL if those differ once a cache exists. */
int emme_ctx_set_options(emme_ctx_t* ctx, const emme_options_t* opt);
int emme_ctx_get_options(const emme_ctx_t* ctx, emme_options_t* opt);
void emme_ctx_destroy(emme_ctx_t* ctx);
/* The node-cache buffers of destroyed contexts (up to ~170 GB) are kept in a process-wide pool
 * and reused by the next context (allocating them costs seconds, a parameter sweep creates one
 * context per parameter set); this returns them to the driver. */
void emme_release_pooled_memory(void);
/* Which shapes the option tile_uncached serves (additions within version 4, found by symbol lookup).  The table-free
 * tile fill exists for all four shapes the project fills: k_assemble_tile for electrostatic GK15, and
 * k_assemble_tile_shape<PTS, NM> for electromagnetic contexts (NM = 3: a chunk is 5 omegas x 3
 * moments) and the 31-point rule.  With EMME_TILE_SHAPES_ALL, plain fills of such contexts that have no node cache to
 * read take it under tile_uncached's other preconditions (host omegas, integration_accuracy >= 1e-9, at least wl_min
 * omegas or the minority pass).  Derivative fills follow the shapes too: with deriv_cached = 1 as well they take
 * k_assemble_tile_shape_deriv<PTS, NM>, also on contexts that have a node cache, which no derivative
 * request of these shapes reads; with deriv_cached = 0 they stay on the omega-lane derivative kernel.  No effect while
 * tile_uncached = 0.  Not a layout setting: it may change on a live context and takes effect from the next call.
 * emme_ctx_fill_mode reports 5 for either kernel.  Calls over bound parameter sets are served too:
 * with EMME_TILE_SHAPES_ALL the routing rule of emme_assemble_sets_batch / emme_solve_roots_sets holds on
 * electromagnetic and GK31 contexts as well, through k_assemble_tile_shape_sets<PTS, NM> and its _deriv form, fill
 * mode 7; with EMME_TILE_SHAPES_ES15 such calls stay on k_assemble_sets. */
#define EMME_TILE_SHAPES_ES15 0 /* default: tile_uncached serves electrostatic GK15 only */
#define EMME_TILE_SHAPES_ALL  1 /* tile_uncached serves electromagnetic and GK31 contexts as well */
int emme_ctx_set_tile_shapes(emme_ctx_t* ctx, int shapes); /* EMME_EINVAL: NULL ctx, value out of range */
int emme_ctx_get_tile_shapes(const emme_ctx_t* ctx);       /* < 0: EMME_EINVAL for NULL */
/* Which shapes the option deriv_cached sends through the node cache (additions within version 4, found by symbol
 * lookup).  The cached derivative fill exists for all four shapes of the tiled cache: k_assemble_dense_deriv for
 * electrostatic GK15 and k_assemble_dense_shape_deriv<PTS, NM> for electromagnetic
 * contexts and the 31-point rule -- K and K' of a column as twin columns of the GEMM, so that a chunk holds 8
 * electrostatic omegas or 2 omegas x 3 moments.  With EMME_DERIV_CACHE_SHAPES_ALL, derivative fills with host omegas
 * of such a context that has the tiled cache (emme_assemble_derivative_batch, emme_solve_roots_newton, the exact polish
 * of emme_find_roots_in_contour) follow the cache policy of the plain fills as electrostatic GK15 ones do under
 * deriv_cached: same interval trees, M and M' within the project's 1e-10 bar of the uncached fill, the cache may be
 * built or grown, and emme_ctx_last_deferred reports the integrals that left the cache (finished from scratch by
 * k_assemble_deriv_list_shape<PTS>).  With tile_uncached = 1 and EMME_TILE_SHAPES_ALL set as well, the cache takes what
 * its policy gives it and k_assemble_tile_shape_deriv what that policy leaves without a cache.  No effect while
 * deriv_cached = 0.  Not a layout setting: it may change on a live context and takes effect from the next call.
 * emme_ctx_fill_mode keeps naming the last plain fill.  Calls over bound parameter sets never read a node cache and
 * are not affected. */
#define EMME_DERIV_CACHE_SHAPES_ES15 0 /* default: deriv_cached serves electrostatic GK15 only */
#define EMME_DERIV_CACHE_SHAPES_ALL  1 /* deriv_cached serves electromagnetic and GK31 contexts as well */
int emme_ctx_set_deriv_cache_shapes(emme_ctx_t* ctx, int shapes); /* EMME_EINVAL: NULL ctx, value out of range */
int emme_ctx_get_deriv_cache_shapes(const emme_ctx_t* ctx);       /* < 0: EMME_EINVAL for NULL */
/* Mirror-image pairs (additions within version 4, found by symbol lookup).  On a grid that is symmetric
 * under i -> N-1-i (eta and g odd, b even to 1e-13 of the table's largest value: theta = 0) the integral of pair (i, j)
 * is that of (N-1-j, N-1-i).  An electrostatic GK15 context on the tiled layout -- with EMME_MIRROR_SHAPES_ALL (below)
 * an electromagnetic or GK31 one as well -- then lays its node cache out over one
 * pair of every such couple -- half the cache, half the integrals of the dense fill and of its deferred pass -- and
 * writes both entries, each under its own SingularityHandler weight; interval counts stay those of the full pair list.
 * The two entries agree to the rounding noise of the reference's own mirror pairs.  On by default (EMME_MIRROR=0, read
 * at creation, switches it off); a context created with deriv_cached = 1 never mirrors, and one whose mirrored cache a
 * cached derivative request reaches rebuilds the cache over the full list and stays unmirrored.  A layout setting: the
 * setter answers EMME_EINVAL once the node cache exists.  The getter says whether the cache is laid out over the half
 * list, or before it exists whether it would be; 0 on every context that is not eligible. */
int emme_ctx_set_mirror_pairs(emme_ctx_t* ctx, int on); /* EMME_EINVAL: NULL ctx, value not 0 / 1, cache exists */
int emme_ctx_get_mirror_pairs(const emme_ctx_t* ctx);   /* 0 / 1; < 0: EMME_EINVAL for NULL */
/* Which shapes run mirrored (additions within version 4, found by symbol lookup).  The symmetry above
 * holds for all three velocity moments of an electromagnetic context (kappa_e reads a pair through eta_i - eta_j and
 * g_i - g_j alone, and the mirror image keeps i < j, so block B keeps its signs) and for the 31-point rule.  With
 * EMME_MIRROR_SHAPES_ALL, electromagnetic and GK31 contexts on a symmetric grid mirror exactly as electrostatic GK15
 * does: the half pair list under the tiled cache, the dense fill k_assemble_dense<1, PTS, NM> and its deferred pass,
 * each integral stored to its mirror-image entries in the block of its moment.  Everything else of
 * emme_ctx_set_mirror_pairs holds unchanged (deriv_cached, cached derivative requests, the region searches).  A
 * mirrored electrostatic GK31 context takes the folded steps below under their own rules; a mirrored electromagnetic
 * context never folds -- its matrix is a 2 x 2 block matrix of centrosymmetric blocks, not centrosymmetric itself.
 * Default EMME_MIRROR_SHAPES_ES15: every context behaves bit for bit as without this setting.  EMME_MIRROR_SHAPES, read
 * at creation, overrides the default.  A layout setting: EMME_EINVAL once the node cache exists. */
#define EMME_MIRROR_SHAPES_ES15 0 /* default: only electrostatic GK15 contexts mirror */
#define EMME_MIRROR_SHAPES_ALL  1 /* electromagnetic and GK31 contexts on a symmetric grid mirror as well */
int emme_ctx_set_mirror_shapes(emme_ctx_t* ctx, int shapes); /* EMME_EINVAL: NULL ctx, value out of range, cache exists */
int emme_ctx_get_mirror_shapes(const emme_ctx_t* ctx);       /* < 0: EMME_EINVAL for NULL */
/* The folded trace-secant step (additions within version 4, found by symbol lookup).  Where a context
 * runs mirrored (above) its matrix is symmetric and, apart from the SingularityHandler's rule for the last row and
 * column, centrosymmetric: a trace-secant step of emme_solve_roots whose two fills both ran mirrored for every live
 * chain, on an even order, factors the even and the odd block of order dim / 2 instead of the matrix and adds the
 * exact rank-2 correction of that rule.  Every other step -- odd order, theta != 0, electromagnetic contexts (mirrored
 * or not), GK31 contexts that do not mirror (EMME_MIRROR_SHAPES_ES15),
 * the QR method, the Newton, eigenpair, sets and region searches, the step-level entry points -- is what it was.
 * Option lu_fold: 1 = on, 0 = the unfolded step bit for bit; EMME_LU_FOLD, read at creation, overrides the default.
 * (emme_options_t has no room left for a field that keeps its size: the option is a setter, as mirror_pairs is.)
 * Not a layout setting: it may change on a live context, from the next call on. */
int emme_ctx_set_lu_fold(emme_ctx_t* ctx, int on); /* EMME_EINVAL: NULL ctx, value not 0 / 1 */
int emme_ctx_get_lu_fold(const emme_ctx_t* ctx);   /* 0 / 1; < 0: EMME_EINVAL for NULL */
int emme_ctx_last_folded_steps(const emme_ctx_t* ctx); /* steps of the last emme_solve_roots that ran folded */
/* Which LU kernel the context launched last (additions within version 4, found by symbol lookup), as the fill mode says
 * it for the fills.  The symbol is the kernel's name as rocprofv3 prints it, "" before the first launch, NULL for a NULL
 * context; the string lives as long as the library.  After a trace step (emme_trace_solve_batch, the half problems of
 * the folded step, a step of emme_solve_roots): "k_trace_solve_blocked<false, false>" (one workgroup per matrix),
 * "k_trace_solve_blocked<true, false>" (several), "k_trace_solve_grouped" (several, grouped trailing updates),
 * "k_trace_solve_blocked<true, true>" (chunked panel, orders whose panel does not fit one workgroup's LDS) or
 * "k_trace_solve" (unblocked) -- what was launched, which is one workgroup per matrix or the unblocked kernel where
 * the grid of a split or chunked launch could not be resident.  After a factorisation alone (null vectors, eigenpair
 * steps, contour moments): "k_lu_inplace", "k_trace_solve_blocked<true, true>" or "k_lu_unblocked_inplace".
 * emme_ctx_last_lu_workgroups: the workgroups each matrix got; emme_ctx_last_lu_slices: the launches the batch of that
 * factorisation was cut into (1 for a trace step). */
const char* emme_ctx_linstep_kernel_symbol(const emme_ctx_t* ctx);
int emme_ctx_last_lu_workgroups(const emme_ctx_t* ctx); /* < 0: EMME_EINVAL for NULL */
int emme_ctx_last_lu_slices(const emme_ctx_t* ctx);     /* < 0: EMME_EINVAL for NULL */
/* Compute units of the context's device, from its properties: what the workgroup counts and the slices of a chunked
 * factorisation (half of them per launch) are planned with. */
int emme_ctx_compute_units(const emme_ctx_t* ctx);      /* < 0: EMME_EINVAL for NULL */
/* Launch everything on this hipStream_t (e.g. torch's current stream). NULL = default. */
int emme_ctx_set_stream(emme_ctx_t* ctx, void* hip_stream);
int emme_ctx_dim(const emme_ctx_t* ctx); /* N if beta_e == 0 else 2N */
/* Kernel family used by the last fill: 0 lanes-are-nodes, 1 omega-lane, 2 HBM node cache
 * (independent lanes), 3 HBM node cache + phase table, union walk, 4 HBM node cache (tiled) +
 * dense fill on the FP64 matrix cores, 5 table-free tile fill on the FP64 matrix cores, 6 lanes-are-nodes over
 * parameter sets (emme_assemble_sets_batch, emme_solve_roots_sets; with or without the derivative), 7 table-free
 * tile fill over parameter sets, a set per omega chunk (the same two entry points, with or without the derivative:
 * at least one (set, contour class) group of the call took it; see the routing rule there; k_assemble_tile_sets on
 * electrostatic GK15, k_assemble_tile_shape_sets<PTS, NM> on electromagnetic and GK31 contexts). */
int emme_ctx_fill_mode(const emme_ctx_t* ctx);
/* Integrals the last fill handed to the work list (the cached fills and the tile fill finish them in a second
 * launch, from scratch); 0 for fills that have no work list.  Synchronises the context's stream.  < 0: an EMME_* code. */
long long emme_ctx_last_deferred(emme_ctx_t* ctx);
/* GiB of HBM currently held by the node-record cache (0 if none). */
double emme_ctx_node_cache_gib(const emme_ctx_t* ctx);
/* The node cache grows at run time: a fill that had to hand integrals to the from-scratch kernel
 * (their trees leave the cached intervals) makes the next fill cache a subtree around the interval
 * they were missing.  An integral that moves from one kernel to the other keeps its interval count
 * but changes its rounding (summation order, folded amplitudes: ~1e-16 relative, 1e-12 at strongly
 * damped omega), so a root search on a fresh context and on a warm one differ at that level.  The
 * CANONICAL state is the settled one: emme_ctx_cache_settle fills M(omega_b) for the given omegas
 * (host, 2*nbatch doubles; results discarded) until a fill leaves the cache shape unchanged; after
 * it, fills of omegas in the same region are bit-for-bit repeatable.  fills_done (nullable): fills run. */
int emme_ctx_cache_settle(emme_ctx_t* ctx, const double* omega, int nbatch, int* fills_done);
/* Shape of the cache: depth of the fully cached tree (-1 none yet, -2 disabled / does not fit),
 * number of cached subtrees (the fixed one included), GiB held.  Any pointer may be NULL. */
int emme_ctx_cache_state(const emme_ctx_t* ctx, int* full_depth, int* subtrees, double* gib);
int emme_ctx_profile_enable(emme_ctx_t* ctx, int on);
int emme_ctx_profile_read(emme_ctx_t* ctx, emme_profile_t* out, int reset);

/* Fill M(omega_b) for b < nbatch.  omega: 2*nbatch doubles (host; a device pointer is refused with
 * EMME_EINVAL before anything is read or queued: the fill is planned on the host from the omegas'
 * values).  M: nbatch*dim*dim complex, row-major, host or device.  intervals (optional, host,
 * nbatch long long): GK intervals evaluated per item. */
int emme_assemble_batch(emme_ctx_t* ctx, const double* omega, int nbatch, double* M,
                        long long* intervals);

/* One trace-secant Newton step per item, in place (all arrays host or device, but
 * consistently one of the two: omega, domega, M, Mp and info are checked together, and a call
 * that mixes the sides returns EMME_EINVAL before anything is copied or queued):
 *   in : omega[b], M[b] = M(omega[b]), Mp[b] = M'(omega[b])
 *   out: domega[b] = -1/tr(M^-1 M'), omega[b] += domega[b], M[b] = M(new omega),
 *        Mp[b] = (M_new - M_old)/domega, info[b] (LAPACK convention).
 * method: EMME_METHOD_TRACE_SECANT as above; EMME_METHOD_QR_SECANT replaces the step by the
 * reference's newtonQRSecantIteration (include/solver.h:210-383): domega = -R_nn / (Q^H M' v)_n
 * from the column-pivoted QR of M (info[b] = k > 0: R(k,k) == 0, the ztrtrs failure). */
int emme_newton_step_batch(emme_ctx_t* ctx, double* omega, double* domega, int nbatch,
                           double* M, double* Mp, int method, int* info);

/* tr(A_b^-1 B_b) for b < nbatch by partial-pivot LU (A, B: nbatch*n*n complex, destroyed;
 * host or device).  tr: 2*nbatch doubles (host). info: nbatch ints (host): 0, k > 0 = U(k,k)
 * exactly zero (tr[b] = NaN), or EMME_EDEVICE if the cooperating workgroups of that matrix
 * gave up waiting for each other (only when something else holds compute units for seconds;
 * emme_solve_roots repairs that case itself, the step-level calls report it). */
int emme_trace_solve_batch(emme_ctx_t* ctx, int n, int nbatch, double* A, double* B, double* tr,
                           int* info);

/* The folded trace-secant step alone: tr[b] = tr(M_b^-1 (M_b - M_old_b) / domega_b) for b < nbatch,
 * whatever lu_fold says.  THE CALLER PROMISES matrices of the structure the mirrored fills write: M_b and M_old_b
 * symmetric, and centrosymmetric -- X(i, j) = X(n-1-i, n-1-j) -- apart from their last row and column.  Only the upper
 * triangles are read, and of them only the wedge between diagonal and anti-diagonal (i <= j <= n-1-i) and the last
 * column; what the promise says about the rest is taken for granted, not checked.  M, M_old (nbatch*n*n complex,
 * row-major), domega (nbatch complex), tr (nbatch complex) and info (nbatch ints) are all host or all device
 * (EMME_EINVAL otherwise); M, M_old and domega are not modified.  info[b]: 0; k > 0: the factorisation of the even
 * (k <= n/2) or of the odd block (k - n/2) met an exactly zero pivot column; n + 1: the 2 x 2 matrix of the rank-2
 * correction is singular or not finite; EMME_EDEVICE as emme_trace_solve_batch; tr[b] is NaN for every non-zero info.
 * The result of an item does not depend on the other items of the call nor on lu_split.  EMME_EINVAL for an odd n;
 * EMME_ECONFIG for n above 1050 or with lu_unblocked. */
int emme_trace_secant_folded_batch(emme_ctx_t* ctx, int n, int nbatch, const double* M, const double* M_old,
                                   const double* domega, double* tr, int* info);

/* The QR-secant quotient alone, for any square A_b, B_b (nbatch*n*n complex, row-major, host or
 * device, not modified; n <= 1024): with A P = Q R (Householder QR, LAPACK zgeqp3 pivoting),
 * R11 y = r12, v = P [-y; 1], t = Q^H (B v):  q[b] = t_n / R_nn, so that the reference's step is
 * domega = -1/q (include/solver.h:370).  q: 2*nbatch doubles (host); info: nbatch ints (host). */
int emme_qr_secant_batch(emme_ctx_t* ctx, int n, int nbatch, const double* A, const double* B,
                         double* q, int* info);

/* Batched root search: for each guess g_b run the reference's solve-once sequence
 * (omega=0.99 g; M_old=M(omega); omega+=0.01 g; M; M'; then up to step_limit+1 Newton
 * steps, stopping when |domega| < tol*|omega|).  The step is the one the context's
 * iteration_method names (trace-secant or QR-secant, src/main.cpp:45-49).  All arrays host.
 * roots: 2n doubles; iters: n ints (Newton steps done); info: n ints (0 ok, k>0 singular
 * pivot k, EMME_ENUMERIC if that chain met a non-finite integral / the depth cap).
 * iterates (optional): n*(step_limit+1)*2 doubles, omega after every step, NaN padded. */
int emme_solve_roots(emme_ctx_t* ctx, const double* guesses, int n, double tol, int step_limit,
                     double* roots, int* iters, int* info, double* iterates);
/* ---- exact derivative and true Newton (additions within version 4: find them by symbol lookup) ------------------
 * M(omega) and M'(omega) = dM/domega exactly, for the intervals the adaptive rule chose for M: the
 * derivative rides along the quadrature, the accept/split decisions and M are those of the plain fill of the same
 * kernel bit for bit.  Pointers as emme_assemble_batch (omega host or device; M and Mp both host or both device).
 * Batches of wl_min or more go through the omega-lane kernel, smaller ones through the lanes-are-nodes kernel, on
 * every context: the node cache is neither read nor grown (emme_ctx_cache_state is unchanged) unless deriv_cached is
 * set, and emme_ctx_fill_mode keeps naming the last plain fill.  With the option deriv_cached, a call with host omegas
 * on an electrostatic GK15 context with the tiled cache follows the cache policy of emme_assemble_batch instead: M and
 * M' come from the cached records (k_assemble_dense_deriv), the same interval trees, M and M' within the project's
 * 1e-10 bar of the uncached fill, and the cache may be built or grown.  Electromagnetic and GK31 contexts with the tiled
 * cache do the same once their derivative cache shapes are EMME_DERIV_CACHE_SHAPES_ALL
 * (emme_ctx_set_deriv_cache_shapes: k_assemble_dense_shape_deriv<PTS, NM>); at the default they keep the uncached
 * kernels under deriv_cached.  With deriv_cached and tile_uncached
 * both set, what that policy leaves without a cache goes through k_assemble_tile_deriv where k_assemble_tile would serve
 * the plain fill: M is the plain tile fill's bit for bit, the interval trees are the same, M' is within the same bar, and
 * emme_ctx_last_deferred reports the integrals handed to the from-scratch list kernel.  EMME_ENUMERIC as the plain fill (depth cap, non-finite
 * integral), and also when an entry of M' is non-finite or beyond the range M is held to: a fill whose M alone the
 * plain fill accepts can then fail. */
int emme_assemble_derivative_batch(emme_ctx_t* ctx, const double* omega, int nbatch, double* M, double* Mp,
                                   long long* intervals);
/* Newton's method on det M = 0 with the exact M': arguments, outputs, info codes, NaN-padded iterates and stopping
 * rule as emme_solve_roots, but starting at omega_0 = g (no 0.99 g / 0.01 g bootstrap), and every step fills M and M'
 * at the current omega of the live chains.  The step is the context's iteration_method on (M, M'): trace form
 * domega = -1/tr(M^-1 M'), QR form domega = -1/q.  emme_ctx_get_matrix and emme_null_vectors_batch(M = NULL) see the
 * last fill's M per chain afterwards.  Derivative fills count in the emme_profile_t fill counters.  With the option
 * deriv_cached the fills of the search go through the node cache where emme_assemble_derivative_batch's would
 * (electromagnetic and GK31 contexts: under EMME_DERIV_CACHE_SHAPES_ALL, emme_ctx_set_deriv_cache_shapes), and
 * with tile_uncached as well through the table-free tile fill (k_assemble_tile_deriv) where there is no cache. */
int emme_solve_roots_newton(emme_ctx_t* ctx, const double* guesses, int n, double tol, int step_limit,
                            double* roots, int* iters, int* info, double* iterates);
/* ---- parameter sets: many sets on one context (additions within version 4: find them by symbol lookup;
 * DESIGN.md §13) ----------------------------------------------------------------------------------------------
 * Every other entry point works on the ONE parameter set the context was created with.  These bind further sets to
 * the context and let every item of a batch name the set it belongs to: one launch then fills (and one search
 * iterates) items of different sets side by side, through k_assemble_sets / k_assemble_sets_deriv -- the
 * lanes-are-nodes fill, never the node cache or the omega-lane kernel.  All sets of a context share
 * its SHAPE: npoints, whether beta_e == 0, integration_start_points and iteration_method; everything else may differ,
 * conf and length included.  Entry points without `set` behave exactly as before, whether or not sets are bound.
 * Routing: with the option tile_uncached on an electrostatic GK15 context whose bound sets ALL have
 * integration_accuracy >= 1e-9, and omegas the host knows (a host `omega` pointer; a root search), the items are
 * grouped by (set, contour class) and every group of at least wl_min items goes through k_assemble_tile_sets
 * (k_assemble_tile_sets_deriv for a derivative request, which asks for deriv_cached as well) -- the table-free tile
 * fill with ONE set per omega chunk, fill mode 7.  Smaller groups of the same call, and every call that fails one of
 * the conditions, keep k_assemble_sets bit for bit (mode 6 when no group took the tile fill).  With default options
 * nothing changes.  Electromagnetic and GK31 contexts follow the same rule once their tile shapes are
 * EMME_TILE_SHAPES_ALL (emme_ctx_set_tile_shapes): k_assemble_tile_shape_sets<PTS, NM> /
 * k_assemble_tile_shape_sets_deriv<PTS, NM>, a chunk of an electromagnetic context holding 5 omegas x 3 moments of one
 * set; with the shapes at their default they stay on k_assemble_sets whatever tile_uncached says. */
/* host only, no device: EMME_OK if b has a's shape (npoints, beta_e == 0 alike, integration_start_points,
 * iteration_method), else EMME_EINVAL with emme_last_error naming the first field that differs */
int emme_params_same_shape(const emme_params_t* a, const emme_params_t* b);
/* bind nsets parameter sets (derived members filled) to a context; each must have the shape of the context's own
 * set; replaces an earlier binding; nsets = 0 unbinds.  Arguments are checked BEFORE the device is looked for. */
int emme_ctx_bind_param_sets(emme_ctx_t* ctx, const emme_params_t* sets, int nsets);
int emme_ctx_param_sets(const emme_ctx_t* ctx);          /* number bound, < 0: EMME_EINVAL */
/* M(omega_b) of parameter set set[b]; Mp nullable: the exact dM/domega of the same trees.
 * Pointer rules as emme_assemble_batch / emme_assemble_derivative_batch; set: host, nbatch ints in [0, nsets).
 * EMME_EINVAL without a binding or for a set[b] out of range; EMME_ENUMERIC as emme_assemble_batch. */
int emme_assemble_sets_batch(emme_ctx_t* ctx, const int* set, const double* omega, int nbatch,
                             double* M, double* Mp, long long* intervals);
/* emme_solve_roots (exact = 0) or emme_solve_roots_newton (exact = 1), chain b on parameter set set[b].
 * Everything else as those two (tol and step_limit are the call's, for every chain); emme_ctx_get_matrix and
 * emme_null_vectors_batch(M = NULL) work afterwards. */
int emme_solve_roots_sets(emme_ctx_t* ctx, const int* set, const double* guesses, int n, int exact,
                          double tol, int step_limit, double* roots, int* iters, int* info, double* iterates);
/* Copy M(omega_final) of item b of the last emme_solve_roots / emme_solve_roots_newton / emme_solve_roots_sets call
 * (dim*dim complex). */
int emme_ctx_get_matrix(emme_ctx_t* ctx, int b, double* M_host);

/* ---- point probes (additions within version 4: find them by symbol lookup; tests and tooling only) ---------------
 * Like emme_bessel_batch: no context, host pointers, EMME_EDEVICE without a GPU, EMME_EINVAL on bad arguments
 * (checked before the device is looked for).  Every item is evaluated by one thread, by the very device function
 * the fill kernels call.
 *
 * One math primitive of the fill per argument.  fn:                     in per item   out per item */
#define EMME_FN_RCP 0         /* frcp: hardware seed + two Newton steps     x             1/x            */
#define EMME_FN_RSQRT 1       /* frsqrt                                     x             1/sqrt(x)      */
#define EMME_FN_EXP 2         /* fexp, literal coefficients                 x             exp(x)         */
#define EMME_FN_EXP_S 3       /* fexp, coefficients in scalar registers     x             exp(x)         */
#define EMME_FN_EXP_V 4       /* fexp, coefficients in vector registers     x             exp(x)         */
#define EMME_FN_SINCOS 5      /* fsincos, three-term reduction              x             sin x, cos x   */
#define EMME_FN_SINCOS_S 6    /* fsincos, two-term, scalar registers        x             sin x, cos x   */
#define EMME_FN_SINCOS_V 7    /* fsincos, two-term, vector registers        x             sin x, cos x   */
#define EMME_FN_CRCP 8        /* complex rcp                                re, im        re, im of 1/z  */
int emme_elementary_batch(int fn, const double* x, int n, double* out);
/* The pointwise integrand F_m(tan x) / cos^2 x of the mapped integral (reference src/Parameters.cpp:120-176), per item
 * k < n: grid pair i[k] < j[k], moment m[k] (0, or 0..2 when beta_e != 0), abscissa x[k] in (0, pi/2) and
 * omega[2k], omega[2k+1]; the contour sense is that of the item's omega.  The pair constants are built by the code the
 * fill kernels use.  EMME_EINVAL also for a parameter set whose arc_coeff, vt, tau, q, R or omega_s_i is zero or not
 * finite (the kernels divide by them).  form:                                                               doubles out per item */
#define EMME_FORM_F 0         /* integrand(): F                                                    2  */
#define EMME_FORM_F_DF 1      /* integrand_d(): F, dF/domega                                       4  */
#define EMME_FORM_SPLIT 2     /* node_data(): A0, T, Q1, Q0, then node_eval of them at omega: F   10  */
#define EMME_FORM_W 3         /* node_w(): W, the moment factor (F_m = F_0 (c_nv W)^m)             2  */
int emme_integrand_batch(const emme_params_t* p, int form, int n, const int* i, const int* j, const int* m,
                         const double* x, const double* omega, double* out);

/* nullSpace (reference include/solver.h:58-112): the right singular vector of the smallest
 * singular value of the n x n complex matrix M (row-major), by inverse iteration on M^H M.
 * Same vector as the reference's SVD result up to the arbitrary complex phase. Host pointers. */
int emme_null_vector(const double* M, int n, double* vec /* 2n doubles */);
/* The same on the device, batched (nullspace.hip): ONE partial-pivot LU per matrix (the Newton step's kernels,
 * no right-hand sides) and inverse iteration v <- M^-1 (M^-H v) on its factors until the direction stops
 * moving.  M: nbatch*n*n complex, row-major, host or device, not modified; NULL = the matrices M(omega_final)
 * of the last emme_solve_roots call on this context (then n = emme_ctx_dim, nbatch <= that call's n).
 * vecs: nbatch*n complex (host), unit 2-norm, arbitrary phase.  info (host, nbatch): 0, k > 0 = column k of the
 * factorisation is exactly zero (no vector: NaN), EMME_ENUMERIC = non-finite result.  n <= 2048. */
int emme_null_vectors_batch(emme_ctx_t* ctx, int n, int nbatch, const double* M, double* vecs, int* info);

/* ---- Newton on the eigenpair (additions within version 4: find them by symbol lookup) ------------
 * Nonlinear inverse iteration on (omega, v), |v| = 1:
 *     u = M(omega_k)^-1 M'(omega_k) v_k,   omega_k+1 = omega_k - 1 / (v_k^H u),   v_k+1 = u / |u|
 * with the exact M' of emme_assemble_derivative_batch.  A step is one LU WITHOUT right-hand sides, one matrix-vector
 * product and one pair of triangular solves (the trace form factors with n right-hand sides), the convergence to a
 * simple eigenpair is quadratic, and the eigenvector and the residual |M(omega) v| / |M(omega)|_F come with the root.
 *
 * emme_solve_eigenpairs: omega_0 = g as emme_solve_roots_newton; stopping rule, iters, info codes and NaN-padded
 * iterates as there; fills routed as there (deriv_cached, tile_uncached, the shape switches, parameter sets).  The
 * context's iteration_method is NOT consulted: trace-secant and QR-secant contexts give the same result.
 *   set       NULL: the context's own parameters; else host, n ints, checked as in emme_solve_roots_sets
 *   v0        NULL: chain b starts from v_0 = M(g_b)^-1 s / |M(g_b)^-1 s| with
 *                 s[i] = (1 + 0.37 sin(1 + i)) + 0.21 cos(2 i) i,   i = 0 .. dim-1
 *             (the start vector of emme_null_vectors_batch); else host, n*dim complex, each row normalised on entry
 *             (a zero or non-finite row: EMME_EINVAL)
 *   vecs      host, n*dim complex: unit 2-norm, arbitrary phase; NaN for a failed chain (info != 0)
 *   resid     host, n: |M(omega) v| / |M(omega)|_F at the returned omega with the returned vector; NaN where there is
 *             none.  A chain that used every step keeps info = 0, as in the other searches: info = 0 says "no failure",
 *             and resid is what tells a root (rounding level, 1e-16 .. 1e-15) from a chain that merely stopped.
 * All pointer and range checks (NULL ctx / guesses / roots / vecs / resid / iters / info, n < 1, step_limit < 0,
 * tol <= 0: EMME_EINVAL) come before the device is looked for.  EMME_ECONFIG for dim > 2048.  emme_ctx_get_matrix and
 * emme_null_vectors_batch(M = NULL) work afterwards. */
int emme_solve_eigenpairs(emme_ctx_t* ctx, const int* set /* NULL: the context's own set */, const double* guesses,
                          int n, const double* v0 /* NULL, or n*dim complex */, double tol, int step_limit,
                          double* roots, double* vecs /* n*dim complex */, double* resid /* n */, int* iters, int* info,
                          double* iterates /* nullable */);
/* One such step on caller matrices (eigpair.hip): M, Mp nbatch*n*n complex, row-major, both host or both device, not
 * modified.  v (host, nbatch*n complex): in, the current vectors, taken as they are (unit 2-norm expected) -- with
 * have_v = 0 not read: the step starts from M^-1 s / |M^-1 s|, s as above; out, u / |u|.  tau[b] = v^H u (host, complex:
 * domega = -1 / tau), resid[b] = |M v| / |M|_F BEFORE the step (host).  info (host): 0, k > 0 = column k of the
 * factorisation is exactly zero (vector, tau and resid NaN), EMME_ENUMERIC = non-finite tau or u.  Two calls give the
 * same bits.  n <= 2048 (EMME_ECONFIG above); argument checks come before the device is looked for. */
int emme_eigenpair_step_batch(emme_ctx_t* ctx, int n, int nbatch, const double* M, const double* Mp,
                              double* v /* in/out, host */, int have_v, double* tau, double* resid, int* info);
/* ---- the secant reading of it (additions within version 4: find them by symbol lookup) -------------
 * The same iteration for a search that has no derivative fill, only two consecutive plain fills M = M(omega_k) and
 * M_old = M(omega_k-1) -- the reference's own iteration is a secant one, and the plain fill is this library's fastest
 * path (dense, cached, mirrored):
 *     u = M^-1 (M - M_old) v_k / (omega_k - omega_k-1),   omega_k+1 = omega_k - 1 / (v_k^H u),   v_k+1 = u / |u|.
 * The matrix M' is never formed: one pass over the rows of both matrices (k_eigpair_secant_step, eigpair.hip) takes the
 * difference entry by entry and gives (M - M_old) v, M v and |M|_F together.  Convergence to a simple eigenpair is
 * superlinear, as the secant root searches'.
 *
 * One step on caller matrices: M, M_old as M, Mp of emme_eigenpair_step_batch; domega: host, nbatch complex, the step
 * omega_k - omega_k-1 between the two fills.  v, have_v, tau (domega_next = -1 / tau), resid (of M, before the step)
 * and info as there; a zero or non-finite domega gives EMME_ENUMERIC.  Two calls give the same bits.  n <= 2048
 * (EMME_ECONFIG above); argument checks come before the device is looked for. */
int emme_eigenpair_secant_step_batch(emme_ctx_t* ctx, int n, int nbatch, const double* M, const double* M_old,
                                     const double* domega /* host, nbatch complex */, double* v /* in/out, host */,
                                     int have_v, double* tau, double* resid, int* info);
/* ---- that step on mirrored grids, folded; mode parity (additions within version 4: find them by symbol lookup;
 * DESIGN.md 14.2) ----------------------------------------------------------------------------------------------------
 * Where a context runs mirrored (emme_ctx_set_mirror_pairs) its matrix is C + u e^T + e u^T, C symmetric and
 * centrosymmetric, and a secant eigenpair step whose two fills both ran mirrored for every live chain, on an even order,
 * can factor the even and the odd block of order dim / 2 instead of the matrix (ONE k_lu_inplace per block, a quarter of
 * the LU flops, four triangular solves of half the order; eigpair_fold.hip) with the exact rank-2 correction of the last
 * row and column.  Option eigpair_fold: 0 (default) = every step is the unfolded one, bit for bit; 1 = steps of
 * emme_solve_eigenpairs_secant (and of the region searches' polish with exact = 0) that qualify run folded -- all but
 * the first step of a call without v0, which also makes v_0.  Fills over parameter sets, theta != 0, odd orders, GK31
 * and electromagnetic contexts never qualify; emme_solve_eigenpairs (exact) is untouched.  EMME_EIGPAIR_FOLD, read at
 * creation, overrides the default.  Not a layout setting: it may change on a live context, from the next call on.
 * Cost: with the option on, a secant eigenpair search on a context where steps can fold (mirrored, even order, no
 * parameter sets) holds one more matrix set, n*dim*dim complex, for the half problems' secants; elsewhere nothing.
 * (emme_options_t keeps its size: the option is a setter, as lu_fold is.) */
int emme_ctx_set_eigpair_fold(emme_ctx_t* ctx, int on); /* EMME_EINVAL: NULL ctx, value not 0 / 1 */
int emme_ctx_get_eigpair_fold(const emme_ctx_t* ctx);   /* 0 / 1; < 0: EMME_EINVAL for NULL */
int emme_ctx_last_folded_eigpair_steps(const emme_ctx_t* ctx); /* steps of the last eigenpair search that ran folded */
/* The folded step alone, whatever eigpair_fold says.  THE CALLER PROMISES matrices of the structure the mirrored fills
 * write, as for emme_trace_secant_folded_batch: only the wedge between diagonal and anti-diagonal (i <= j <= n-1-i) and
 * the last column are read.  M, M_old: nbatch*n*n complex, row-major, both host or both device (EMME_EINVAL otherwise),
 * not modified; domega (host, nbatch complex); v (host, nbatch*n complex, required): in, the unit vectors; out, u / |u|;
 * tau, resid (of M, before the step) and info (host) as emme_eigenpair_secant_step_batch.  info[b]: 0; k > 0: the
 * factorisation of the even (k <= n/2) or of the odd block (k - n/2) met an exactly zero pivot column; n + 1: the 2 x 2
 * matrix of the rank-2 correction is singular or not finite; EMME_ENUMERIC: a zero or non-finite domega, tau or u;
 * vector, tau and resid are NaN for every non-zero info.  The result of an item does not depend on the other items of
 * the call; two calls give the same bits.  EMME_EINVAL for NULL arguments, n < 2 or an odd n; EMME_ECONFIG for n above
 * 1050 or with lu_unblocked; both come before the device is looked for. */
int emme_eigenpair_secant_folded_step_batch(emme_ctx_t* ctx, int n, int nbatch, const double* M, const double* M_old,
                                            const double* domega /* host */, double* v /* in/out, host, required */,
                                            double* tau, double* resid, int* info);
/* Mode parity: even[k] = |v1 + J v2|^2 / (2 |v|^2) of vector k (vecs: nvec*n complex, host), the share of the vector
 * in the subspace that is even under the flip i -> n-1-i (1: an even mode, 0: an odd one; for odd n the middle entry
 * counts as even); NaN for a zero or non-finite vector.  Plain host arithmetic: no context, no device; works on the
 * vectors of any eigenpair entry point.  EMME_EINVAL for NULL pointers, n < 1 or nvec < 1. */
int emme_vector_parity(int n, int nvec, const double* vecs, double* even);
/* The search: arguments, outputs, v0 rules, stopping rule, info codes, blanked failed chains and NaN-padded iterates as
 * emme_solve_eigenpairs, but bootstrapped as emme_solve_roots (omega_0 = 0.99 g, omega_1 = g: two plain fills; v_0 from
 * M(omega_1)^-1 s without v0), and every step costs ONE plain fill, routed exactly as emme_solve_roots' are (node cache,
 * mirrored pair list, cost order, skip_lost; parameter sets as emme_solve_roots_sets).  No derivative kernel runs and
 * no option is consulted or changed: after a call on a default context emme_ctx_get_mirror_pairs and the options are
 * what they were.  iteration_method is not consulted.  emme_ctx_get_matrix and emme_null_vectors_batch(M = NULL) work
 * afterwards. */
int emme_solve_eigenpairs_secant(emme_ctx_t* ctx, const int* set /* NULL: the context's own set */,
                                 const double* guesses, int n, const double* v0 /* NULL, or n*dim complex */, double tol,
                                 int step_limit, double* roots, double* vecs /* n*dim complex */, double* resid /* n */,
                                 int* iters, int* info, double* iterates /* nullable */);

/* ---- root sensitivities from eigenpairs (additions within version 4: find them by symbol lookup) ----
 * Every fill kernel writes an entry of M(omega; p) together with its mirror, so M = M^T bit for bit (DESIGN.md §5.0c,
 * §5.5): the left null vector of a root is the conjugate of the right one, v, that the eigenpair searches return, and
 * for a simple root
 *     d omega / d p = - v^T (dM/dp) v / (v^T M' v)          (v^T: plain transpose, no conjugation)
 * with the exact M' = dM/domega of emme_assemble_derivative_batch and dM/dp the difference of two plain fills on
 * neighbouring parameter sets at the same omega.  No factorisation, no transposed solve, no iteration: the cost of a
 * call is its fills -- the forms kernel is a single pass over matrices the fills just wrote.  The same forms give
 *     corr = - v^T M v / (v^T M' v)              the Rayleigh-functional correction: a first-order estimate of the
 *                                                distance from the returned omega to the root
 *     cond = |M|_F |v|_2^2 / |v^T M' v|          the eigenvalue condition number: how far a perturbation of M moves omega
 *
 * Building block on caller matrices (sym_forms.hip): item t < nitems computes
 *     form[t] = x^T (A_a - B_b) y   (complex; transpose, not conjugate),    fro2[t] = |A_a - B_b|_F^2
 * with a = a[t], b = b[t] (-1, or b = NULL: no second matrix), x = x[t], y = y[t] (y = NULL: y = x) -- the difference
 * taken per entry BEFORE the product, as in emme_eigenpair_secant_step_batch.  A, B: nmat*n*n complex, row-major, both
 * host or both device, not modified; vecs: host, nvec*n complex; a, b, x, y: host, their ranges ([0, nmat), b also -1,
 * [0, nvec)) checked.  form: host, nitems complex; fro2: host, nitems, nullable.  Symmetry is not assumed.  The bits of
 * a result depend on n and the data alone -- not on which items share a call or on the device's size -- and two calls
 * give the same bits.  n <= 2048 (EMME_ECONFIG above); all pointer and range checks (EMME_EINVAL) come before the
 * device is looked for. */
int emme_sym_forms_batch(emme_ctx_t* ctx, int n, int nmat, const double* A, const double* B /* nullable */,
                         int nvec, const double* vecs /* host, nvec*n complex */, int nitems, const int* a,
                         const int* b /* nullable: none */, const int* x, const int* y /* nullable: y = x */,
                         double* form /* host, nitems complex */, double* fro2 /* host, nitems; nullable */);
/* d omega / d p of nroots eigenpairs over bound parameter sets (emme_ctx_bind_param_sets).
 *   set, roots, vecs   root r is the eigenpair (roots[r], vecs[r*dim ..]) of bound set set[r], exactly as
 *                      emme_solve_eigenpairs / emme_solve_eigenpairs_secant (with `set`) and
 *                      emme_find_eigenpairs_in_contours_sets return them: their outputs can be passed straight through.
 *                      The vector need not have unit norm (the quotients do not depend on it).
 *   ndir, set_plus, set_minus, dp
 *                      direction k < ndir of root r is the pair of bound sets set_plus[r*ndir+k], set_minus[r*ndir+k],
 *                      filled at omega_r, and dp[r*ndir+k] = p+ - p-, the parameter distance between them (non-zero and
 *                      finite, else EMME_EINVAL).  The sets may differ in any continuous parameters: the direction is
 *                      whatever the caller made of it.  One-sided differences (set_minus = set[r]) and a scan line's
 *                      own neighbours (sets i-1 and i+1 around point i) are legal.  ndir = 0: only denom, corr, cond.
 *   max_items          cap of the matrices held at once (0: automatic, 1 GiB of matrices, at least 2 and at most
 *                      4096).  A cap of 1 is rounded up to one pair's two matrices, an odd cap down to whole pairs.
 *                      The neighbour fills run in chunks of whole (root, direction) pairs under the cap; the outputs
 *                      do not depend on it.
 *   dwdp               host, nroots*ndir complex;   denom[r] = v^T M' v, corr[r], cond[r] as above (host)
 *   info[r]            0;  1: |v^T M' v| <= 64 dim eps |M'|_F |v|^2, the form is at its own rounding level -- a multiple
 *                      or defective root, or not an eigenvector: dwdp and corr NaN, denom and cond still returned;
 *                      EMME_ENUMERIC: a NaN (non-finite) root or vector row -- the blanked output of a failed chain --
 *                      or a base fill that failed: every output of THAT root NaN, the others untouched.
 * A neighbour fill that fails makes only its dwdp entry NaN.  A vector that is merely not an eigenvector of a simple
 * root is NOT caught by info (it stays 0): corr, of the size of the distance to the root, and the search's resid tell.
 * Method: one derivative fill over sets for M, M' at (set[r], omega_r), plain fills over sets for the neighbour
 * matrices, routed exactly as emme_assemble_sets_batch routes them; one k_sym_forms launch per chunk and
 * k_sym_forms_finish, which forms the quotients on the device.  No option is consulted or changed beyond what
 * emme_assemble_sets_batch does: afterwards emme_ctx_get_mirror_pairs, the options and the binding are what they were.
 * EMME_EINVAL, all before the device is looked for: NULL ctx / set / roots / vecs / denom / corr / cond / info (with
 * ndir > 0 also set_plus / set_minus / dp / dwdp), nroots < 1, ndir < 0, max_items < 0, a bad dp, no binding, a set
 * index out of range, a zero vector row.  EMME_ECONFIG for dim > 2048. */
int emme_root_sensitivities_sets(emme_ctx_t* ctx, int nroots, const int* set, const double* roots, const double* vecs,
                                 int ndir, const int* set_plus, const int* set_minus, const double* dp, int max_items,
                                 double* dwdp, double* denom, double* corr, double* cond, int* info);

/* ---- region search: every root inside a contour (version 4) ---------------------------------------
 * The reference only polishes guesses (src/main.cpp:19-80).  These entry points answer "which modes lie in this part of
 * the omega plane": Beyn's contour-integral method (W.-J. Beyn, Linear Algebra Appl. 436 (2012) 3839-3863, algorithm 1)
 * turns M(omega_j)^-1 V at N quadrature nodes of an ellipse into candidates for every eigenvalue inside it, the argument
 * principle on det M(omega_j) at the same nodes counts them, and the context's Newton step (emme_solve_roots) polishes
 * the candidates to the reference's own roots.  M(omega) is analytic inside one half-plane only (the contour sense
 * omi = -sign Re omega), so an ellipse must not reach Re omega = 0. */
typedef struct emme_contour {
    int size;              /* sizeof(emme_contour_t), set by emme_contour_default */
    double center[2];      /* c */
    double semi_axes[2];   /* a along Re omega, b along Im omega; the ellipse must not reach Re omega = 0 */
    int points;            /* starting node count N (power of two) */
    int max_points;        /* cap of the nested doubling */
    int probes;            /* starting L; doubled up to 64 while A0 has full numerical rank */
    double rank_tol;       /* relative singular-value cut */
} emme_contour_t;
/* Defaults (DESIGN.md §11 gives the measurements behind them); center and semi_axes are zero and must be set. */
void emme_contour_default(emme_contour_t* c);

/* All roots of det M(omega) inside the ellipse omega(t) = c + a cos t + i b sin t, polished by the context's Newton step
 * (iteration_method), sorted by Im omega descending.  roots: 2*max_roots, iters/info: max_roots (at most max_roots are
 * written, *n_roots counts all).  *winding = argument-principle count (-1 unresolved at max_points);
 * *points_used = N at the end.  Complete iff *winding >= 0 && *n_roots == *winding.
 * The nodes t_j = 2 pi j / N are filled in one batch and factored once (partial-pivot LU, the factors are kept for the
 * whole call: N dim^2 16 bytes); N doubles by the midpoints while the count is unresolved, L doubles while A0 has full
 * numerical rank, both on the factors already held.  EMME_EINVAL: an ellipse reaching Re omega = 0, non-positive
 * semi-axes, points not a power of two >= 4, max_points < points, probes outside 1..64, rank_tol outside (0, 1);
 * EMME_ECONFIG: dim > 2048; a node whose fill fails (depth cap, non-finite) ends the call with its error, the message
 * names the node (on that return *n_roots = 0, *winding = -1 and *points_used = the nodes so far are written, as for a
 * dropped item of emme_find_roots_in_contours_sets: do not read them as a result).  Chains that did not converge (info != 0, or the last of step_limit + 1 steps still above tol) are
 * dropped. */
int emme_find_roots_in_contour(emme_ctx_t* ctx, const emme_contour_t* c, double tol, int step_limit,
                               int max_roots, double* roots, int* iters, int* info,
                               int* n_roots, int* winding, int* points_used);

/* Building block on caller matrices (host or device, nq*n*n complex, not modified):
 * X_j = M_j^-1 V, A0 = sum w_j X_j, A1 = sum w_j z_j X_j (n*L complex each, host),
 * logdet[j] = (log|det M_j|, arg det M_j), info[j] as emme_null_vectors_batch.  V NULL = internal probes
 * (V[i][l] from a counter-based hash of (i, l) with a fixed seed, DESIGN.md §11: the first L columns do not depend on L).
 * z, w: nq complex each (host).  A matrix with info != 0 has no X_j and is left out of the sums.  n <= 2048, L <= 64. */
int emme_contour_moments_batch(emme_ctx_t* ctx, int n, int nq, const double* M, const double* z,
                               const double* w, int L, const double* V, double* A0, double* A1,
                               double* logdet, int* info);

/* The same with the matrices dealt into ngroups groups (an addition within version 4: find it by symbol lookup;
 * DESIGN.md §13.9): group[j] in [0, ngroups) names the group of matrix j (host, nq ints; groups need not be
 * contiguous), and A0 / A1 hold ngroups blocks of n*L complex, block g = the sums over the matrices of group g in
 * ascending j, matrices with info != 0 left out; an empty group gives zeros.  One factorisation, one solve and one
 * moments launch for all groups.  logdet, info per matrix as above.  ngroups <= 65535. */
int emme_contour_moments_groups(emme_ctx_t* ctx, int n, int nq, const double* M, const int* group, int ngroups,
                                const double* z, const double* w, int L, const double* V, double* A0,
                                double* A1, double* logdet, int* info);

/* Region search over parameter sets (an addition within version 4: find it by symbol lookup): item k
 * is emme_find_roots_in_contour on the bound parameter set set[k] (emme_ctx_bind_param_sets) and the contour
 * contours[k], and the items advance in lock step -- per round ONE fill over sets, one factorisation, one log-det and
 * one solve launch for the new nodes of all items, then one moments launch per L pass and one emme_solve_roots_sets
 * for the candidates of all items.  Per item the node sequence (points, doubled by the midpoints up to the item's own
 * max_points), the winding rule, the L doubling from the item's own probes with its rank_tol, the candidate radius 1.5,
 * the drop rules and the sort by Im omega descending are those of the single call.  exact = 0: the polish is the
 * context's iteration_method (emme_solve_roots), exact = 1: the Newton search on the exact derivative
 * (emme_solve_roots_newton); tol and step_limit are the call's, for every item.
 * Outputs are per item: roots 2*max_roots doubles, iters / info max_roots ints (item k at offset k*max_roots roots),
 * n_roots, winding, points_used, status one int each.  status[k] = EMME_OK, or the error that took item k out of the
 * call: a node whose fill fails gives EMME_ENUMERIC, winding -1 and n_roots 0 for ITS item, the other items go on, and
 * emme_last_error names the first such item and its node.
 * The call returns EMME_EINVAL (the message names the item) without a binding, for a set[k] outside [0, nsets),
 * nitems outside 1 .. 65535 or a contour that fails emme_find_roots_in_contour's argument rules -- all checked BEFORE
 * the device is looked for; EMME_ECONFIG for dim > 2048.
 * Afterwards emme_ctx_get_matrix and emme_null_vectors_batch(M = NULL) refer to the polish, as after
 * emme_solve_roots_sets; its chains are the candidates of the items in item order and, inside an item, in the order
 * emme_contour_eigs returned them (candidates outside normalised radius 1.5 have no chain; neither have items that
 * left the call).  Memory: the factors and X of the nodes actually used, nodes * (dim^2 + 64 dim) * 16 bytes, in one
 * block per round. */
int emme_find_roots_in_contours_sets(emme_ctx_t* ctx, int nitems, const int* set, const emme_contour_t* contours,
                                     int exact, double tol, int step_limit, int max_roots, double* roots,
                                     int* iters, int* info, int* n_roots, int* winding, int* points_used,
                                     int* status);

/* Host only: the Beyn step on given moments (row-major n x L complex).  B = U_k^H A1 W_k S_k^-1 from the thin SVD
 * A0 = U S W^H (one-sided Jacobi), k = #{s_i > rank_tol s_1}; mu = eigenvalues of B (Hessenberg + shifted QR).
 * mu: 2*max_eigs (min(k, max_eigs) written), *k = numerical rank used (k == L: the probes may be too few),
 * sigma (nullable): the L singular values of A0, descending.  Returns EMME_OK, EMME_EINVAL on bad sizes. */
int emme_contour_eigs(int n, int L, const double* A0, const double* A1, double rank_tol,
                      int max_eigs, double* mu, int* k, double* sigma);
/* The same step with the eigenvectors it yields for free (an addition within version 4: find it by symbol lookup;
 * DESIGN.md §11): vecs (nullable; host, min(k, max_eigs) rows of n complex) row c = v_c = U_k y_c, the eigenvector of
 * M(omega) for mu_c, unit 2-norm, arbitrary phase; y_c is the eigenvector of B for mu_c, by inverse iteration on a kept
 * copy of B (with a perturbed shift if B - mu_c I is exactly singular).  mu, k and sigma are emme_contour_eigs' bit for
 * bit -- that function is this one with vecs = NULL. */
int emme_contour_eigpairs(int n, int L, const double* A0, const double* A1, double rank_tol, int max_eigs, double* mu,
                          double* vecs, int* k, double* sigma);

/* Region searches that return eigenpairs (additions within version 4: find them by symbol lookup):
 * emme_find_roots_in_contour / emme_find_roots_in_contours_sets with another last stage.  Nodes, count, L doubling,
 * candidate radius, drop rules, duplicate rule, order, per-item failures and argument rules are theirs (one driver);
 * the candidates carry their Beyn vectors (emme_contour_eigpairs on the moments of the final L pass), and ONE eigenpair
 * search started from those vectors polishes the candidates of all items:
 *   exact = 0   emme_solve_eigenpairs_secant (plain fills only: a default context keeps its mirrored cache)
 *   exact = 1   emme_solve_eigenpairs (exact dM/domega fills, routed as there)
 * with the items' set indices where there are sets.  Beside roots / iters / info, every kept root q of item k comes back
 * with vecs[(k max_roots + q) dim ..] (dim complex, unit 2-norm, arbitrary phase) and resid[k max_roots + q] =
 * |M(omega) v| / |M(omega)|_F; vecs holds max_roots*dim complex per item, resid max_roots.  The duplicate rule stays the
 * omega-distance one; one drop rule is added: a polished chain whose residual is above 1e-8 stopped on its step without
 * M being singular (a spurious candidate) and is dropped like a failed chain.  Afterwards emme_ctx_get_matrix and emme_null_vectors_batch(M = NULL) refer to the polish, as
 * after the root forms.  The existing searches keep their polish and their bits. */
int emme_find_eigenpairs_in_contour(emme_ctx_t* ctx, const emme_contour_t* c, int exact, double tol, int step_limit,
                                    int max_roots, double* roots, double* vecs, double* resid, int* iters, int* info,
                                    int* n_roots, int* winding, int* points_used);
int emme_find_eigenpairs_in_contours_sets(emme_ctx_t* ctx, int nitems, const int* set, const emme_contour_t* contours,
                                          int exact, double tol, int step_limit, int max_roots, double* roots,
                                          double* vecs, double* resid, int* iters, int* info, int* n_roots, int* winding,
                                          int* points_used, int* status);

/* The reference's driver (src/main.cpp:182-338) on an input.json TEXT: one solve, or a
 * parameter scan over every key written {head, step, tail}, with omega continuation.
 * matrix_dir (may be NULL): directory for the raw eigenMatrix .bin files (must exist, like the
 * reference's eigenMatrics/).  *output_text receives the output.json text (release with
 * emme_free).  Per-point failures become {"eigenvalue":"NaN","reason":...} records. */
int emme_run_json(const char* input_text, const char* matrix_dir, char** output_text);
void emme_free(void* p);
/* emme_run_json with the independent lines of the scan solved side by side; same output schema.  A line is (axis,
 * direction): round 0 solves the head of every axis, round t the t-th point of every line, each from the last
 * successful root of its own line -- one emme_solve_roots_sets call on one context per round.
 * Records, their order, file names, NaN records and reasons are the sequential driver's.  An axis whose key changes
 * the shape (npoints, beta_e through zero, integration_start_points, iteration_method) or is iteration_precision /
 * iteration_step_limit is run by the sequential driver. */
int emme_run_json_lockstep(const char* input_text, const char* matrix_dir, char** output_text);
/* The round plan of emme_run_json_lockstep for an input.json text (host only, no device).  Points are listed axis by
 * axis (input order), each axis in emme_scan_values order: axis[k], index[k] (position on its axis), round[k] (-1 on a
 * sequential axis), pred[k] (index on the same axis of the point it continues from: the previous point of its line,
 * the head for the first point of either direction; -1 for the head: initial_guess).  sequential[a] = 1 for an axis
 * left to the sequential driver.  At most max_points / max_axes entries are written (arrays nullable); *n_rounds is
 * 1 + the longest line of the axes that ride along.  Returns the number of points, or EMME_EINVAL / EMME_EJSON. */
int emme_scan_plan(const char* input_text, int max_points, int* axis, int* index, int* round, int* pred,
                   int max_axes, int* sequential, int* n_axes, int* n_rounds);
/* Values one {head, step, tail:[tail0, tail1]} axis visits, in order (reference
 * src/main.cpp:139-172); turning_flags[k] = 1 where the sweep restarts from the head in the
 * other direction.  Returns the number of values (<= max_values). */
int emme_scan_values(double head, double step, double tail0, double tail1, double* values,
                     int* turning_flags, int max_values);

/* ---- multi-GPU scan: the one collective -------------------------------------------------------
 * The (parameter set, omega guess) items of a scan are independent Newton chains.  The reference
 * walks them sequentially in one process (src/main.cpp:264-324); here item k of n_total goes to
 * rank k mod world (one process per GPU, its own context), nothing is exchanged while iterating,
 * and ONE RCCL all-gather (ncclAllGather over xGMI, 32 B per item) hands every rank all roots.
 * RCCL is bound at run time; a process that never calls these does not load it. */
#define EMME_COMM_ID_BYTES 128 /* = NCCL_UNIQUE_ID_BYTES */
typedef struct emme_comm emme_comm_t;
/* Rank 0 makes the id (ncclGetUniqueId) and hands the 128 bytes to the other ranks out of band
 * (a file, a socket, MPI, torch.distributed's store ...). */
int emme_comm_unique_id(unsigned char* id /* EMME_COMM_ID_BYTES */);
/* Collective over all `world` ranks (ncclCommInitRank). device < 0 => current device. */
int emme_comm_create(const unsigned char* id, int rank, int world, int device, emme_comm_t** out);
void emme_comm_destroy(emme_comm_t* comm);
/* Collective.  In: this rank's results in the order of its share (items rank, rank+world, ...),
 * n_local of them; n_local must be the round-robin share of n_total (EMME_EINVAL otherwise,
 * checked before the collective).  Out (host, on every rank): all n_total results in item order.
 * hip_stream: stream for the copies and the collective (NULL = default). */
int emme_gather_roots(emme_comm_t* comm, void* hip_stream, const double* roots /* 2*n_local */,
                      const int* iters, const int* info, int n_local, int n_total,
                      double* roots_all /* 2*n_total */, int* iters_all, int* info_all);
/* 0 if RCCL can be bound in this process.  NOT a collective: every rank asks before emme_comm_create, so that all
 * ranks can agree (e.g. an all-reduce over an existing process group) on the C-ABI gather or on a fall-back. */
int emme_comm_available(void);
/* The slot mapping emme_gather_roots uses, host only (no RCCL, no device): m = emme_gather_slots = ceil(n_total /
 * world) slots of 4 doubles {w_re, w_im, iters, info} per rank; emme_gather_share = items of `rank` in the
 * round-robin deal; emme_gather_pack fills a rank's 4 m doubles (NaN padded; EMME_EINVAL unless n_local is the
 * rank's share); emme_gather_unpack turns the world * 4 m doubles of the all-gather into item order. */
int emme_gather_slots(int n_total, int world);
int emme_gather_share(int n_total, int world, int rank);
int emme_gather_pack(int rank, int world, const double* roots, const int* iters, const int* info, int n_local,
                     int n_total, double* send /* 4 * slots */);
int emme_gather_unpack(int world, int n_total, const double* all /* world * 4 * slots */, double* roots_all,
                       int* iters_all, int* info_all);

#ifdef __cplusplus
}
#endif
#endif /* EMME_HIP_H */
