// eigpair_fold.hip -- the secant eigenpair step (eigpair.hip) on mirror-symmetric matrices, folded
// into the even and the odd block of order m = n / 2 (notation of linstep_fold.hip).
// M = C + u e^T + e u^T with C symmetric and centrosymmetric, e = e_{n-1}; folds are unnormalised (x+- = x1 +- J x2, so
// every bilinear or sesquilinear form of two folds is twice the form of the vectors; unfold: x1 = (x+ + x-) / 2,
// x2 = J (x+ - x-) / 2).  With S+-, S'+-, u+-, u'+- of k_fold_pass / k_fold_edges and ONE factorisation of each S_s
// (k_lu_inplace) a step is, per half problem s,
//   y_s = S_s v_s,  z_s = S'_s v_s,  c_s = S_s^-1 z_s,  a_s = S_s^-1 u_s,  a'_s = S_s^-1 u'_s,  b_s = S_s^-1 e_s
// and per chain, with v_last = v[n-1],
//   x  = c + v_last a' + <u', v> b                      (= C^-1 (M - M_old) v / domega)
//   K  = I + [[<e, a>, <e, b>], [<u, a>, <u, b>]],  (g1, g2)^T = K^-1 (<e, x>, <u, x>)^T
//   u^ = x - g1 a - g2 b                                (= M^-1 (M - M_old) v / domega, Woodbury)
//   tau = v^H u^,  v <- unfold(u^) / |u^|,  (M v)+- = y+- + v_last u+- + <u, v> e+-,  resid = |M v| / |M|_F.
//   k_eigpair_fold_half     one workgroup per live half problem: the fold of v, one pass over the kept copies of S_s
//                           and S'_s (rows to waves, columns to lanes, as k_eigpair_secant_step), the four solves
//                           (tri_solve.hpp), this half's dot products
//   k_eigpair_fold_combine  one workgroup per live chain: K, g, u^, tau, the new vector, the residual, info
// (which half a workgroup has, the merge of the halves' codes and K: fold_combine.hpp, shared with linstep_fold.hip)
// Every sum is taken in a fixed order (xor shuffles, then the waves in order), nothing is atomic, and a chain reads
// nothing of another chain: two runs give the same bits, alone or in a batch.
#include <hip/hip_runtime.h>

#include <cmath>

#include "emme_device.hpp"
#include "fold_combine.hpp"
#include "launch.hpp"

namespace emme {

namespace {

using namespace trisolve;
using namespace fold;

constexpr int NHV = 5;    // vectors a half problem leaves behind: c, a, a', b, y
constexpr int NHP = 8;    // ... and its sums: u.a, u.b, u.c, u.a', u'.v, u.v, (|S|_F^2, |v_s|^2), unused

struct EigFoldHalfArgs {
    int n, m, nb, nblk;   // order of the chain's matrix and of a half problem; rows per panel snapshot and snapshots per
                          // matrix of the half problems' factorisation
    const double2* A;     // [2 nbatch][m][m] P S = L U in place
    const int* maps;      // [2 nbatch][nblk][m] row-order snapshots
    const int* items;     // half problems of this launch (null: 0 .. grid-1)
    const int* active;    // nullable, per chain: a half problem whose chain's flag is 0 is left alone
    const int* lu_info;   // per half problem: 0, or the column at which the factorisation stopped
    const double2* S;     // [2 nbatch][m][m] the kept copy of S
    const double2* D;     // [2 nbatch][m][m] the kept copy of S'
    const double2* edges; // [nbatch][4][m] u+, u-, u'+, u'- (k_fold_edges)
    const double2* vecs;  // [nbatch][n] the chains' unit vectors
    double2* hv;          // [2 nbatch][NHV][m]
    double2* part;        // [2 nbatch][NHP]
};

__global__ __launch_bounds__(NT) void k_eigpair_fold_half(EigFoldHalfArgs P) {
    extern __shared__ double2 sm[];
    __shared__ double s_red[6 * NW];
    const int n = P.n, m = P.m;
    const int h = pick_item(P.items);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (P.active && P.active[h >> 1] == 0) return;  // uniform
    double2* out = P.part + (size_t)h * NHP;
    if (P.lu_info[h] != 0) return nan_out(out, NHP);  // no factorisation: the chain's step fails (k_eigpair_fold_combine)
    const Half H(h, P.edges, m);
    const double sgn = H.sgn;
    const double2 *u = H.u, *ud = H.ud;
    const double2* v = P.vecs + (size_t)H.b * n;
    double2* hv = P.hv + (size_t)h * NHV * m;
    const Frame fr(sm, m, P.A + (size_t)h * m * m);
    const Factors& F = fr.F;
    double2* vs = fr.x0;   // v_s
    double2* rhs = fr.x1;  // the right-hand side of the solve at hand
    double2* sol = fr.x2;  // its solution
    fr.load_rowmap(P.maps + (size_t)h * P.nblk * m, P.nb);
    for (int x = tid; x < m; x += NT) vs[x] = d2(ld2(&v[x]) + sgn * ld2(&v[n - 1 - x]));
    __syncthreads();
    // ---- one pass over S_s and S'_s: y = S v_s (left behind), z = S' v_s (the first right-hand side), |S|_F^2 ----
    const double2* S = P.S + (size_t)h * m * m;
    const double2* D = P.D + (size_t)h * m * m;
    double fro = 0.0;
    for (int r = wave; r < m; r += NW) {
        const double2* row = S + (size_t)r * m;
        const double2* row_d = D + (size_t)r * m;
        cd acc = mk(0.0, 0.0), acc_d = mk(0.0, 0.0);
#pragma unroll 4
        for (int c = lane; c < m; c += 64) {
            const cd s = ld2(&row[c]), d = ld2(&row_d[c]);
            const cd xc = mk(vs[c].x, vs[c].y);
            acc_d = acc_d + d * xc;
            acc = acc + s * xc;
            fro += norm2(s);
        }
        acc.x = wave_sum(acc.x), acc.y = wave_sum(acc.y);
        acc_d.x = wave_sum(acc_d.x), acc_d.y = wave_sum(acc_d.y);
        if (lane == 0) hv[4 * (size_t)m + r] = d2(acc), rhs[r] = d2(acc_d);
    }
    __syncthreads();
    // ---- the four solves; each solution goes out, its dot product with u stays in this thread ----
    // (one copy of the solves' code: four inlined copies spill)
    cd dot_c = mk(0.0, 0.0), dot_a = dot_c, dot_ap = dot_c, dot_b = dot_c;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        if (k > 0) {
            for (int x = tid; x < m; x += NT)
                rhs[x] = k == 1 ? u[x] : k == 2 ? ud[x] : make_double2(x == 0 ? sgn : 0.0, 0.0);  // u_s, u'_s, e_s
            __syncthreads();
        }
        solve_plain(F, rhs, sol);
        cd acc = mk(0.0, 0.0);
        for (int x = tid; x < m; x += NT) {
            const cd sx = mk(sol[x].x, sol[x].y);
            hv[(size_t)k * m + x] = sol[x];
            acc = acc + ld2(&u[x]) * sx;
        }
        if (k == 0) dot_c = acc;  // u.c, u.a, u.a', u.b
        else if (k == 1) dot_a = acc;
        else if (k == 2) dot_ap = acc;
        else dot_b = acc;
    }
    cd uv = mk(0.0, 0.0), dv = uv;
    double v2 = 0.0;
    for (int x = tid; x < m; x += NT) {
        const cd vx = mk(vs[x].x, vs[x].y);
        uv = uv + ld2(&u[x]) * vx, dv = dv + ld2(&ud[x]) * vx;
        v2 += norm2(vx);
    }
    // (s_red: the solves' barriers stand before the first sum, one of the kernel's own before each of the others)
    double t[6], t2[2];
    {
        const double w[6] = {wave_sum(dot_a.x), wave_sum(dot_a.y), wave_sum(dot_b.x), wave_sum(dot_b.y),
                             wave_sum(dot_c.x), wave_sum(dot_c.y)};
        block_sum(s_red, w, t);
    }
    if (tid == 0) out[0] = make_double2(t[0], t[1]), out[1] = make_double2(t[2], t[3]), out[2] = make_double2(t[4], t[5]);
    __syncthreads();
    {
        const double w[6] = {wave_sum(dot_ap.x), wave_sum(dot_ap.y), wave_sum(dv.x), wave_sum(dv.y), wave_sum(uv.x), wave_sum(uv.y)};
        block_sum(s_red, w, t);
    }
    if (tid == 0) out[3] = make_double2(t[0], t[1]), out[4] = make_double2(t[2], t[3]), out[5] = make_double2(t[4], t[5]);
    __syncthreads();
    {
        const double w[2] = {wave_sum(fro), wave_sum(v2)};
        block_sum(s_red, w, t2);
    }
    if (tid == 0) out[6] = make_double2(t2[0], t2[1]), out[7] = make_double2(0.0, 0.0);
}

struct EigFoldCombineArgs {
    int n, m;
    const int* items;      // the live half problems, two per chain (null: chain = workgroup)
    const int* active;     // nullable, per chain: a chain whose flag is 0 is left alone
    const double2* M;      // [nbatch][n][n]: row 0, the last column and two diagonal entries are read (|M|_F)
    const double2* domega; // [nbatch]
    const double2* edges;  // [nbatch][4][m]
    const int* lu_info;    // [2 nbatch]
    const double2* hv;     // [2 nbatch][NHV][m]
    const double2* part;   // [2 nbatch][NHP]
    double2* vecs;         // [nbatch][n] in: v_k, out: v_k+1
    double2* tau;          // [nbatch]
    double* resid;         // [nbatch]
    int* info;             // [nbatch]
};

// info: a stopped factorisation's column (in the odd block plus m), n + 1 where det K is zero or not finite,
// EMME_ENUMERIC for a zero or non-finite domega, tau or u^; the vector, tau and resid are NaN for every non-zero info
__global__ __launch_bounds__(NT) void k_eigpair_fold_combine(EigFoldCombineArgs P) {
    extern __shared__ double2 sm[];
    __shared__ double s_red[5 * NW];
    const int n = P.n, m = P.m;
    double2* up = sm;      // u^+
    double2* um = sm + m;  // u^-
    const int b = P.items ? P.items[2 * blockIdx.x] >> 1 : blockIdx.x;
    if (P.active && P.active[b] == 0) return;  // uniform
    const int tid = threadIdx.x;
    double2* out = P.vecs + (size_t)b * n;
    const double qnan = __builtin_nan("");
    auto fail = [&](int code) {
        nan_out(out, n);
        if (tid == 0) P.info[b] = code, P.tau[b] = make_double2(qnan, qnan), P.resid[b] = qnan;
    };
    const int inf = merge_half_info(P.lu_info[2 * b], P.lu_info[2 * b + 1], m);
    if (inf != 0) return fail(inf);  // uniform
    const double2* pp = P.part + (size_t)(2 * b) * NHP;
    const double2* pm = pp + NHP;
    const double2* hp = P.hv + (size_t)(2 * b) * NHV * m;  // c, a, a', b, y of the even block
    const double2* hm = hp + (size_t)NHV * m;              // ... of the odd block
    const double2* ue = P.edges + (size_t)b * 4 * m;       // u+, then u-
    // (a form of two unnormalised folds is twice the form of the vectors; e+ = e_0, e- = -e_0)
    auto first = [&](int k) { return 0.5 * (ld2(&hp[(size_t)k * m]) - ld2(&hm[(size_t)k * m])); };
    const cd ua = both(pp, pm, 0), ub = both(pp, pm, 1), uc = both(pp, pm, 2), uap = both(pp, pm, 3), upv = both(pp, pm, 4);
    const cd uv = both(pp, pm, 5);
    const cd ec = first(0), ea = first(1), eap = first(2), eb = first(3);
    const cd vlast = ld2(&out[n - 1]);
    const cd ex = ec + vlast * eap + upv * eb, ux = uc + vlast * uap + upv * ub;
    const WoodburyK K(ea, eb, ua, ub);
    if (!K.ok) return fail(n + 1);  // uniform
    const cd rdet = rcp(K.det);
    const cd g1 = (K.k22 * ex - K.k12 * ux) * rdet, g2 = (K.k11 * ux - K.k21 * ex) * rdet;
    // ---- u^+-, tau, |u^|^2, |M v|^2 and the edge terms of |M|_F^2 ----
    const double2* Mb = P.M + (size_t)b * n * n;
    cd tau = mk(0.0, 0.0);
    double u2 = 0.0, mv2 = 0.0, edge = 0.0;
    for (int i = tid; i < m; i += NT) {
        const cd v1 = ld2(&out[i]), v2 = ld2(&out[n - 1 - i]);
        const cd vp = v1 + v2, vm = v1 - v2;
        const cd xp = ld2(&hp[i]) + vlast * ld2(&hp[2 * (size_t)m + i]) + upv * ld2(&hp[3 * (size_t)m + i]);
        const cd xm = ld2(&hm[i]) + vlast * ld2(&hm[2 * (size_t)m + i]) + upv * ld2(&hm[3 * (size_t)m + i]);
        const cd wp = xp - g1 * ld2(&hp[(size_t)m + i]) - g2 * ld2(&hp[3 * (size_t)m + i]);
        const cd wm = xm - g1 * ld2(&hm[(size_t)m + i]) - g2 * ld2(&hm[3 * (size_t)m + i]);
        up[i] = d2(wp), um[i] = d2(wm);
        tau = tau + conj_(vp) * wp + conj_(vm) * wm;
        u2 += norm2(wp) + norm2(wm);
        const double e0 = i == 0 ? 1.0 : 0.0;
        const cd yp = ld2(&hp[4 * (size_t)m + i]) + vlast * ld2(&ue[i]) + e0 * uv;
        const cd ym = ld2(&hm[4 * (size_t)m + i]) + vlast * ld2(&ue[m + i]) - e0 * uv;
        mv2 += norm2(yp) + norm2(ym);
    }
    for (int i = 1 + tid; i < n - 1; i += NT) edge += norm2(ld2(&Mb[(size_t)i * n + n - 1])) - norm2(ld2(&Mb[n - 1 - i]));
    double t[5];
    {
        const double w[5] = {wave_sum(tau.x), wave_sum(tau.y), wave_sum(u2), wave_sum(mv2), wave_sum(edge)};
        block_sum(s_red, w, t);
    }
    const double tx = 0.5 * t[0], ty = 0.5 * t[1];
    const double r = 1.0 / sqrt(0.5 * t[2]);
    const double fro2 = pp[6].x + pm[6].x + 2.0 * t[4] + norm2(ld2(&Mb[(size_t)(n - 1) * n + n - 1])) - norm2(ld2(&Mb[0]));
    const double res = sqrt(0.5 * t[3]) / sqrt(fro2);
    const double2 dw = P.domega[b];
    bool finite = isfinite(dw.x) && isfinite(dw.y) && (dw.x != 0.0 || dw.y != 0.0) && isfinite(tx) && isfinite(ty) &&
                  (tx != 0.0 || ty != 0.0) && isfinite(r);
    // (every read of v_k lies before block_sum's barrier)
    const double hr = 0.5 * r;
    for (int i = tid; i < m; i += NT) {
        const cd wp = mk(up[i].x, up[i].y), wm = mk(um[i].x, um[i].y);
        const double2 o1 = d2(hr * (wp + wm)), o2 = d2(hr * (wp - wm));
        out[i] = o1, out[n - 1 - i] = o2;
        finite = finite && isfinite(o1.x) && isfinite(o1.y) && isfinite(o2.x) && isfinite(o2.y);
    }
    const int bad = __syncthreads_or(!finite);
    if (bad) return fail(-6 /* EMME_ENUMERIC */);  // uniform
    if (tid == 0) P.tau[b] = make_double2(tx, ty), P.resid[b] = res, P.info[b] = 0;
}

}  // namespace

size_t eigpair_fold_vec_bytes(int n, int nbatch) { return sizeof(double2) * NHV * (size_t)(n / 2) * 2 * nbatch; }
size_t eigpair_fold_part_bytes(int nbatch) { return sizeof(double2) * NHP * 2 * (size_t)nbatch; }

hipError_t launch_eigpair_fold_half(int n, const double* S_lu, const int* rowmaps, int nb, const int* items, int nitems,
                                    const int* active, const int* lu_info, const double* S, const double* Sp, const double* edges,
                                    const double* vecs, double* hv, double* part, hipStream_t stream) {
    if (nitems < 1) return hipSuccess;
    const int m = n / 2;
    EigFoldHalfArgs P;
    P.n = n, P.m = m, P.nb = nb, P.nblk = (m + nb - 1) / nb;
    P.A = (const double2*)S_lu, P.maps = rowmaps, P.items = items, P.active = active, P.lu_info = lu_info;
    P.S = (const double2*)S, P.D = (const double2*)Sp, P.edges = (const double2*)edges, P.vecs = (const double2*)vecs;
    P.hv = (double2*)hv, P.part = (double2*)part;
    return launch_dyn_lds(k_eigpair_fold_half, nitems, frame_lds(m), stream, P);
}

hipError_t launch_eigpair_fold_combine(int n, const int* items, int nchains, const int* active, const double* M, const double* domega,
                                       const double* edges, const int* lu_info, const double* hv, const double* part,
                                       double* vecs, double* tau, double* resid, int* info, hipStream_t stream) {
    if (nchains < 1) return hipSuccess;
    EigFoldCombineArgs P;
    P.n = n, P.m = n / 2, P.items = items, P.active = active, P.M = (const double2*)M, P.domega = (const double2*)domega;
    P.edges = (const double2*)edges, P.lu_info = lu_info, P.hv = (const double2*)hv, P.part = (const double2*)part;
    P.vecs = (double2*)vecs, P.tau = (double2*)tau, P.resid = resid, P.info = info;
    const size_t lds = sizeof(double2) * 2 * (size_t)P.m;  // (17 KiB at the half problems' own limit, m = 525)
    hipLaunchKernelGGL(k_eigpair_fold_combine, dim3(nchains), dim3(NT), lds, stream, P);
    return hipGetLastError();
}

}  // namespace emme
