// assemble_deriv_list_text.hpp -- the ONE text of the kernels that finish, from scratch, the integrals a derivative
// fill handed over: the LIST form of k_assemble_deriv (assemble_nodes_text.hpp), as k_assemble<PTS, true> is the LIST
// form of k_assemble.  A lane group per work-list entry (batch << 32 | item), integrand_d per lane, M and M' of the
// integral.  Read inside the including unit's anonymous namespace, once per unit:
//
//   EMME_DERIV_LIST_SHAPE 0  assemble_dense_deriv.hip: DerivListArgs, k_assemble_deriv_list -- electrostatic GK15 only:
//                            no template, GW = 16, __launch_bounds__(256, 3), item = pair, moment 0, no kappa_e (it
//                            is zero there), the four m = 0 stores as plain text with pair_entry_weight
//                            (store_entry_twin reorders them in this kernel)
//   EMME_DERIV_LIST_SHAPE 1  assemble_tile_shape_deriv.hip: DerivListShapeArgs, k_assemble_deriv_list_shape<PTS> --
//                            electromagnetic and GK31 contexts: bounds (256, 2), item = pair nm + moment, kappa_e and
//                            kappa_e', all three moments scattered like k_assemble_deriv through store_entry_twin
//
// Two readings, not one kernel as an instantiation of the other: that changes launch bounds and results.  The walk and
// the spelled-out accept / split rule appear once (gk_split of assemble_common.hpp, spelled out: calling it here
// renames registers in these kernels).  The launchers stay in the units.
//
// No include guard: a text, not a header of declarations.
#ifndef EMME_DERIV_LIST_SHAPE
#error "assemble_deriv_list_text.hpp is read by assemble_dense_deriv.hip (EMME_DERIV_LIST_SHAPE 0) and assemble_tile_shape_deriv.hip (1) only"
#endif

#if EMME_DERIV_LIST_SHAPE
struct DerivListShapeArgs {
#else
struct DerivListArgs {
#endif
    DevParams P;
    const double* tab;
    const ushort2* pairs;
    const double2* omega;
    double2* M;
    double2* Md;
    unsigned long long* intervals;
    int* status;
    const unsigned long long* worklist;
    const unsigned int* worklist_count;
    int skip_lost;
};

#if EMME_DERIV_LIST_SHAPE
template <int PTS>
__global__ __launch_bounds__(256, 2) void k_assemble_deriv_list_shape(DerivListShapeArgs A) {
    constexpr int GW = PTS == 15 ? 16 : 32, GROUPS_PER_BLOCK = 256 / GW, MAXD = EMME_MAX_DEPTH;
#else
__global__ __launch_bounds__(256, 3) void k_assemble_deriv_list(DerivListArgs A) {
    constexpr int PTS = 15, GW = 16, GROUPS_PER_BLOCK = 256 / GW, MAXD = EMME_MAX_DEPTH;
#endif
    extern __shared__ double lds_tab[];  // eta | g | b (3N doubles) | per-group (mid, r) stack

    const DevParams& P = A.P;
#if EMME_DERIV_LIST_SHAPE
    const int N = P.N, dim = P.dim, nm = P.nm;
#else
    const int N = P.N, dim = P.dim;
#endif
    const int nitems = (int)*A.worklist_count;
    if ((int)(blockIdx.x * GROUPS_PER_BLOCK) >= nitems) return;  // (block-uniform: no tables for an empty share)
    for (int k = threadIdx.x; k < 3 * N; k += blockDim.x) lds_tab[k] = A.tab[k];
    __syncthreads();
    const double* eta = lds_tab;
    const double* gtab = lds_tab + N;
    const double* btab = lds_tab + 2 * N;
    double2* stk = reinterpret_cast<double2*>(lds_tab + 3 * N + (3 * N & 1)) + (threadIdx.x / GW) * MAXD;

    const int lane_in_group = threadIdx.x % GW;
    const int group = blockIdx.x * GROUPS_PER_BLOCK + threadIdx.x / GW;
    const int ngroups = gridDim.x * GROUPS_PER_BLOCK;
    const GkLane gk = gk_lane<PTS>(lane_in_group);
    const double qa = 0.0, qb = M_PI / 2.0;
    const double inv_scale = 2. / (qb - qa);
    const cd zero = mk(0.0, 0.0);

    for (int item = group; item < nitems; item += ngroups) {
        const unsigned long long e = A.worklist[item];
#if EMME_DERIV_LIST_SHAPE
        const int it = (int)(e & 0xffffffffull), b = (int)(e >> 32);
        if (A.skip_lost && A.status[b] != 0) continue;  // (the matrix is lost already: uniform per group)
        const int p = it / nm, m = it - p * nm;
#else
        const int p = (int)(e & 0xffffffffull), b = (int)(e >> 32);
        if (A.skip_lost && A.status[b] != 0) continue;  // (the matrix is lost already: uniform per group)
        constexpr int m = 0;
#endif
        OmegaConst oc;
        oc.omega = mk(A.omega[b].x, A.omega[b].y);
        oc.omi = -copysign(1.0, oc.omega.x);
        const ushort2 ij = A.pairs[p];
        const int i = ij.x, j = ij.y;
#if EMME_DERIV_LIST_SHAPE
        const double dg = gtab[i] - gtab[j];
        const PairConst pc = make_pair_const(P, eta[i], eta[j], btab[i], btab[j], dg);
#else  // (no named dg here: it moves registers in this kernel)
        const PairConst pc = make_pair_const(P, eta[i], eta[j], btab[i], btab[j], gtab[i] - gtab[j]);
#endif
        int depth = 0, item_intervals = 0, bad = 0;
        unsigned long long path = 0;
        double l = qa, r = qb, abs_tol = 0.0;
        cd sum = zero, sum_d = zero;
        for (;;) {
            const double mid = (r + l) / 2;
            const double scale = (r - l) / 2;
            const double x = __dadd_rn(__dmul_rn(scale, gk.x), mid);
            cd fd;
            const cd f = integrand_d(x, P, pc, oc, m, fd);
            const double Kx = group_sum<GW>(gk.wk * f.x), Ky = group_sum<GW>(gk.wk * f.y);
            const double Gx = group_sum<GW>(gk.wg * f.x), Gy = group_sum<GW>(gk.wg * f.y);
            const double Kdx = group_sum<GW>(gk.wk * fd.x), Kdy = group_sum<GW>(gk.wk * fd.y);
            ++item_intervals;
            // (gk_split, spelled out)
            const double dKx = Kx - Gx, dKy = Ky - Gy;
            const double absK = gk_modulus(Kx, Ky);
            double err = fmax(gk_modulus(dKx, dKy), absK * (2.0 * 2.220446049250313e-16));
            const cd integral = mk(Kx * scale, Ky * scale);
            err *= scale;
            const double rel_abs = P.rel_tol * (absK * scale);
            if (abs_tol == 0.0) abs_tol = rel_abs;
            bool split = depth < P.max_sub && err > abs_tol * inv_scale + P.prec_goal && err > rel_abs + P.prec_goal;
            if (split && (depth >= MAXD || item_intervals >= EMME_MAX_INTERVALS)) {
                split = false;
                bad = 1;
            }
            if (split) {
                stk[depth] = make_double2(mid, r);
                r = mid;
                ++depth;
                path <<= 1;
                continue;
            }
            sum = sum + integral;
            sum_d = sum_d + mk(Kdx * scale, Kdy * scale);
            ++path;
            while (depth > 0 && !(path & 1)) {
                path >>= 1;
                --depth;
            }
            if (depth == 0) break;
            const double2 pr = stk[depth - 1];
            l = pr.x;
            r = pr.y;
        }
#if EMME_DERIV_LIST_SHAPE
        cd kap = mk(P.pref * sum.y, -(P.pref * sum.x));
        cd kd = mk(P.pref * sum_d.y, -(P.pref * sum_d.x));
        if (kappa_bad(kap) || kappa_bad(kd)) bad = 1;
        kap = kap + kappa_e(m, P, pc.de, dg, oc.omega);
        kd = kd + kappa_e_d(m, P, pc.de, dg, oc.omega);  // kappa' = -i pref sum' + kappa_e'
        if (lane_in_group == 0) {
            double2* Mb = A.M + (size_t)b * dim * dim;
            double2* Mdb = A.Md + (size_t)b * dim * dim;
            auto store = [&](int rw, int c, cd v, cd vd) { store_entry_twin(Mb, Mdb, (size_t)rw * dim + c, v, vd); };
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
        const cd kap = mk(P.pref * sum.y, -(P.pref * sum.x));
        const cd kd = mk(P.pref * sum_d.y, -(P.pref * sum_d.x));
        if (kappa_bad(kap) || kappa_bad(kd)) bad = 1;
        if (lane_in_group == 0) {
            const double w = pair_entry_weight(i, j, N, P.dx);
            const cd v = w * kap, vd = w * kd;
            double2* Mb = A.M + (size_t)b * dim * dim;
            double2* Mdb = A.Md + (size_t)b * dim * dim;
            Mb[(size_t)i * dim + j] = make_double2(v.x, v.y);
            Mb[(size_t)j * dim + i] = make_double2(v.x, v.y);
            Mdb[(size_t)i * dim + j] = make_double2(vd.x, vd.y);
            Mdb[(size_t)j * dim + i] = make_double2(vd.x, vd.y);
#endif
            if (A.intervals) atomicAdd(&A.intervals[b], (unsigned long long)item_intervals);
            if (bad) A.status[b] = 1;
        }
    }
}
