// assemble_wl_text.hpp -- the ONE text of the omega-lane fill (the mapping: header of assemble_wl.hip), read twice by
// assemble_wl.hip inside its anonymous namespace, below AsmWlArgs and EMME_WL_MIN_WAVES: with EMME_WL_DERIV 0 it is
// k_assemble_wl<PTS> (M, with the fused secant), with 1 k_assemble_wl_deriv<PTS> (M and the exact dM/domega of the
// same discretised integrals).  The preprocessor selects the regions that differ, so the compiler sees
// for each kernel the token stream of a kernel written on its own and each keeps its register allocation (DESIGN.md
// 12.2, 12.2.2; a template flag on k_assemble_wl changed the plain kernel's).
//
// The derivative kernel carries the Kronrod sum of F' = exp(A0 + T omega) (T (omega Q1 + Q0) + Q1) beside K -- same
// nodes, same order, same clamp.  Only K and G decide accept / split, so the trees, the interval counts and M are the
// plain kernel's bit for bit.  No fused secant there: Mold, Mp, domega are ignored.
//
// No include guard: a text, not a header of declarations.
#ifndef EMME_WL_DERIV
#error "assemble_wl_text.hpp is read by assemble_wl.hip only, with EMME_WL_DERIV 0 (k_assemble_wl) and 1 (k_assemble_wl_deriv)"
#endif

template <int PTS>
#if EMME_WL_DERIV
__global__ __launch_bounds__(256, EMME_WL_MIN_WAVES) void k_assemble_wl_deriv(AsmWlArgs A, double2* Md) {
#else
__global__ __launch_bounds__(256, EMME_WL_MIN_WAVES) void k_assemble_wl(AsmWlArgs A) {
#endif
    constexpr int GW = PTS == 15 ? 16 : 32;
    constexpr int H = (PTS + 1) / 2;
    constexpr int GROUPS_PER_BLOCK = 256 / GW;
    constexpr int GROUPS_PER_WAVE = 64 / GW;
    constexpr int MAXD = EMME_MAX_DEPTH;
    extern __shared__ double lds_raw[];  // tables | interval stacks | node slots
    __shared__ unsigned long long s_iv[GW];  // interval counts of the chunk's omegas (block_add_intervals)
    if (threadIdx.x < GW) s_iv[threadIdx.x] = 0ull;

    const DevParams& P = A.P;
    const TransConsts TC = trans_consts();
    const int N = P.N, dim = P.dim;
    for (int k = threadIdx.x; k < 3 * N; k += blockDim.x) lds_raw[k] = A.tab[k];
    __syncthreads();
    const double* eta = lds_raw;
    const double* gtab = lds_raw + N;
    const double* btab = lds_raw + 2 * N;
    const int group_in_block = threadIdx.x / GW;
    const int lane = threadIdx.x % GW;
    double2* stk = reinterpret_cast<double2*>(lds_raw + 3 * N + (3 * N & 1)) + group_in_block * MAXD;
    double2* slots = reinterpret_cast<double2*>(lds_raw + 3 * N + (3 * N & 1)) +
                     GROUPS_PER_BLOCK * MAXD + group_in_block * (GW * 4);  // 4 double2 per node

    // this lane's omega (phase 2 identity)
    const int slot_w = blockIdx.y * GW + lane;
    const bool has_w = slot_w < A.n_act;
    const int b = has_w ? A.act_idx[slot_w] : 0;
    cd omega = mk(0.0, 0.0);
#if EMME_WL_DERIV
    if (has_w) omega = mk(A.omega[b].x, A.omega[b].y);
#else
    cd rdw = mk(0.0, 0.0);
    if (has_w) {
        omega = mk(A.omega[b].x, A.omega[b].y);
        if (A.Mold) rdw = rcp(mk(A.domega[b].x, A.domega[b].y));
    }
#endif
    const double my_omi = -copysign(1.0, omega.x);
    double2* Mb = A.M + (size_t)b * dim * dim;
#if EMME_WL_DERIV
    double2* Mdb = Md + (size_t)b * dim * dim;
    // an entry of M and the same entry of M'
    auto store = [&](int r, int c, cd v, cd vd) {
        store_entry_twin(Mb, Mdb, (size_t)r * dim + c, v, vd);
    };
    const cd zero = mk(0.0, 0.0);
#else
    const double2* Moldb = A.Mold ? A.Mold + (size_t)b * dim * dim : nullptr;
    double2* Mpb = A.Mp ? A.Mp + (size_t)b * dim * dim : nullptr;

    auto store = [&](int r, int c, cd v) {
        store_entry_secant(Mb, Moldb, Mpb, rdw, (size_t)r * dim + c, v);
    };
#endif

    // diagonal (include/solver.h:442-443, 465-470): first block of every omega chunk; constant in omega, so 0 in M'
    if (blockIdx.x == 0 && has_w) {
        for (int i = group_in_block; i < N; i += GROUPS_PER_BLOCK) {
#if EMME_WL_DERIV
            store(i, i, mk(P.diag_a, 0.0), zero);
            if (P.nm == 3) {
                store(i, i + N, zero, zero);
                store(i + N, i, zero, zero);
                store(i + N, i + N, mk(P.diag_d * btab[i], 0.0), zero);
            }
#else
            store(i, i, mk(P.diag_a, 0.0));
            if (P.nm == 3) {
                store(i, i + N, mk(0.0, 0.0));
                store(i + N, i, mk(0.0, 0.0));
                store(i + N, i + N, mk(P.diag_d * btab[i], 0.0));
            }
#endif
        }
    }

    // wave-level helper: does any lane of MY group satisfy pred?
    const unsigned long long gmask =
        (GW == 64 ? ~0ull : ((1ull << GW) - 1ull)) << (((threadIdx.x & 63) / GW) * GW);
    auto group_any = [&](bool pred) -> bool { return (__ballot(pred) & gmask) != 0ull; };
    (void)GROUPS_PER_WAVE;

    const GkLane gk = gk_lane<PTS>(lane);  // phase-1 identity: node `lane`
    const double* WK = PTS == 15 ? kWk15 : kWk31;
    const double* WG = PTS == 15 ? kWg15 : kWg31;

    const double qa = 0.0, qb = M_PI / 2.0;
    const double inv_scale = 2. / (qb - qa);
    const int nitems = A.npairs * P.nm;
    const int group = blockIdx.x * GROUPS_PER_BLOCK + group_in_block;
    const int ngroups = gridDim.x * GROUPS_PER_BLOCK;

    // ---- group state (replicated in every lane of the group) ------------------------
    int item = group;
    bool live = item < nitems;
    int i = 0, j = 0, m = 0;
    PairConst pc{};
    double dg = 0.0;
    int depth = 0;
    unsigned long long path = 0;
    double l = qa, r = qb;
    // ---- lane state (phase 2: this lane's omega) -------------------------------------
    int my_depth = 0;               // next node of this omega's own tree
    unsigned long long my_path = 0;
    bool my_done = true;
    double abs_tol = 0.0;
    cd sum = mk(0.0, 0.0);
#if EMME_WL_DERIV
    cd sum_d = mk(0.0, 0.0);  // accepted intervals' scale * K'
#endif
    unsigned long long my_intervals = 0;
    int item_intervals = 0;
    int bad = 0;
    unsigned long long my_rounds = 0;

    auto load_item = [&]() {
        const int p = item / P.nm;
        m = item - p * P.nm;
        const ushort2 ij = A.pairs[p];
        i = ij.x, j = ij.y;
        dg = gtab[i] - gtab[j];
        pc = make_pair_const(P, eta[i], eta[j], btab[i], btab[j], dg);
        depth = 0, path = 0, l = qa, r = qb;
        my_depth = 0, my_path = 0, my_done = !has_w;
        abs_tol = 0.0, item_intervals = 0;
        sum = mk(0.0, 0.0);
#if EMME_WL_DERIV
        sum_d = mk(0.0, 0.0);
#endif
    };
    if (live) load_item();

    while (live) {
        const double mid = (r + l) / 2;
        const double scale = (r - l) / 2;
        const bool need = !my_done && my_depth == depth && my_path == path;
        ++my_rounds;
        bool my_split = false;

#pragma unroll 1
        for (int cls = 0; cls < 2; ++cls) {
            const double omi = cls == 0 ? 1.0 : -1.0;
            const bool mine = need && my_omi == omi;
            if (!group_any(mine)) continue;

            // ---- phase 1: lane = node ------------------------------------------------
            {
                const double x = __dadd_rn(__dmul_rn(scale, gk.x), mid);
                const NodeData d = node_data(x, P, pc, omi, m);
                double2* s = slots + lane * 4;
                s[0] = make_double2(d.A0.x, d.A0.y);
                s[1] = make_double2(d.T.x, d.T.y);
                s[2] = make_double2(d.Q1.x, d.Q1.y);
                s[3] = make_double2(d.Q0.x, d.Q0.y);
            }
            // the slots are produced and consumed inside one wave: LDS operations of a wave
            // complete in issue order; the fence keeps the compiler from moving them
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

            // ---- phase 2: lane = omega -------------------------------------------------
            if (mine) {
#if EMME_WL_DERIV
                auto eval = [&](int node, cd& fd) -> cd {
#else
                auto eval = [&](int node) -> cd {
#endif
                    const double2* s = slots + node * 4;
                    NodeData d;
                    d.A0 = mk(s[0].x, s[0].y);
                    d.T = mk(s[1].x, s[1].y);
                    d.Q1 = mk(s[2].x, s[2].y);
                    d.Q0 = mk(s[3].x, s[3].y);
#if EMME_WL_DERIV
                    return node_eval_d(d, omega, TC, fd);
#else
                    return node_eval(d, omega, TC);
#endif
                };
                // include/functions.h:186-201: centre, then f(+x_i) + f(-x_i) for i = 1..; K' alongside K
#if EMME_WL_DERIV
                cd fd0;
                const cd f0 = eval(0, fd0);
                cd K = WK[0] * f0;
                cd G = WG[0] * f0;
                cd Kd = WK[0] * fd0;
#pragma unroll 1
                for (int q = 1; q < H; ++q) {
                    cd fda, fdb;
                    const cd fa = eval(q, fda);
                    const cd f = fa + eval(q + H - 1, fdb);
                    K = K + WK[q] * f;
                    if ((q & 1) == 0) G = G + WG[q >> 1] * f;
                    Kd = Kd + WK[q] * (fda + fdb);
                }
#else
                const cd f0 = eval(0);
                cd K = WK[0] * f0;
                cd G = WG[0] * f0;
#pragma unroll 1
                for (int q = 1; q < H; ++q) {
                    const cd f = eval(q) + eval(q + H - 1);
                    K = K + WK[q] * f;
                    if ((q & 1) == 0) G = G + WG[q >> 1] * f;
                }
#endif
                ++my_intervals;
                ++item_intervals;
#if EMME_WL_DERIV
                // (gk_split of assemble_common.hpp, spelled out: calling it here renames registers in this kernel)
                const double dKx = K.x - G.x, dKy = K.y - G.y;
                const double absK = gk_modulus(K.x, K.y);
                double err = fmax(gk_modulus(dKx, dKy), absK * (2.0 * 2.220446049250313e-16));
                const cd integral = mk(K.x * scale, K.y * scale);
                err *= scale;
                const double rel_abs = P.rel_tol * (absK * scale);
                if (abs_tol == 0.0) abs_tol = rel_abs;
                my_split = depth < P.max_sub && err > abs_tol * inv_scale + P.prec_goal &&
                           err > rel_abs + P.prec_goal;
#else
                const cd integral = mk(K.x * scale, K.y * scale);
                my_split = gk_split(K, G, scale, inv_scale, depth, P, abs_tol);
#endif
                if (my_split && (depth >= MAXD || item_intervals >= EMME_MAX_INTERVALS)) {
                    my_split = false;
                    bad = 1;
                }
#if EMME_WL_DERIV
                if (!my_split) {
                    sum = sum + integral;
                    sum_d = sum_d + mk(Kd.x * scale, Kd.y * scale);
                }
#else
                if (!my_split) sum = sum + integral;
#endif
            }
            // phase-2 reads must finish before the next class / round overwrites the slots
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }

        // ---- successor of the current interval in pre-order (group-uniform) -------------
        unsigned long long spath = path + 1;
        int sdepth = depth;
        while (sdepth > 0 && !(spath & 1)) {
            spath >>= 1;
            --sdepth;
        }
        // ---- lane bookkeeping ------------------------------------------------------------
        if (need) {
            if (my_split) {
                my_depth = depth + 1;
                my_path = path << 1;
            } else if (sdepth == 0) {
                // this omega's integral is complete: kappa = -i pref sum, + kappa_e, scatter
                my_done = true;
                cd kap = mk(P.pref * sum.y, -(P.pref * sum.x));
                if (kappa_bad(kap)) bad = 1;
                kap = kap + kappa_e(m, P, pc.de, dg, omega);
#if EMME_WL_DERIV
                // kappa' = -i pref sum' + kappa_e', scattered like kappa
                cd kd = mk(P.pref * sum_d.y, -(P.pref * sum_d.x));
                if (kappa_bad(kd)) bad = 1;
                kd = kd + kappa_e_d(m, P, pc.de, dg, omega);
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
#else
                if (m == 0) {
                    const cd v = (-(pair_weight(i, j, N) * P.dx)) * kap;
                    store(i, j, v);
                    store(j, i, v);
                } else if (m == 1) {
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
#endif
            } else {
                my_depth = sdepth;
                my_path = spath;
            }
        }
        // ---- group walk over the union tree ----------------------------------------------
        if (group_any(my_split)) {
            stk[depth] = make_double2(mid, r);  // bounds of the right half, for the way back
            r = mid;
            ++depth;
            path <<= 1;
        } else if (sdepth == 0) {
            item += ngroups;
            live = item < nitems;
            if (live) load_item();
        } else {
            depth = sdepth;
            path = spath;
            const double2 pr = stk[depth - 1];
            l = pr.x;
            r = pr.y;
        }
    }

    if (A.rounds && lane == 0 && my_rounds) atomicAdd(A.rounds, my_rounds);
    block_add_intervals(s_iv, A.intervals, lane, has_w, has_w && group_in_block == 0, b, my_intervals);
    if (has_w && bad) A.status[b] = 1;
}
