// linstep_fold.hip -- the trace-secant step on mirror-symmetric matrices, folded into two half-size problems
// (DESIGN.md 5.4c).  On a grid symmetric under i -> N-1-i the electrostatic matrix is M = C + E: C symmetric and
// centrosymmetric, E = u e^T + e u^T (e = e_{n-1}) the SingularityHandler's "-1/2 on the last column" (pair_weight,
// assemble_common.hpp).  For even n = 2m the orthogonal map Q = 2^-1/2 [[I, I], [J, -J]] splits C into
//   S+ = A11 + A12 J,  S- = A11 - A12 J   (order m: the even and the odd modes),
// the same holds for the secant C' = (C - C_old) / domega, and Sherman-Morrison-Woodbury gives
//   tr(M^-1 M') = tr(S+^-1 S+') + tr(S-^-1 S-') + 2 b^T u' - tr(K^-1 G),
//   a = C^-1 u, b = C^-1 e, K = I + [[e^T a, e^T b], [u^T a, u^T b]], G = [[b^T M' a, b^T M' b], [a^T M' a, a^T M' b]].
// The kernels of this file are what stands around the two factorisations of every half problem (the blocked trace kernel
// on [S | S'], k_lu_inplace on a second copy of S: linstep_blocked.hip):
//   k_fold_edges    u and u' of M and M_old, folded (unnormalised: v+ = v1 + J v2, v- = v1 - J v2; every bilinear form
//                   of two folded vectors is then twice its value, exactly); the live flags of the half problems
//   k_fold_pass     one coalesced pass over the upper triangles of M and M_old: S+-, S+-' (each twice: the copy a
//                   factorisation destroys and the one that is read afterwards) and M_old = M
//   k_fold_solve    per half problem: a+- and b+- from the factors of k_lu_inplace (tri_solve.hpp), the three forms
//                   with S' and the six dot products
//   k_fold_combine  per chain: K, G, the sum, info
// (which half a workgroup has, the merge of the halves' codes and K: fold_combine.hpp, shared with eigpair_fold.hip)
// C is defined from what the pass reads -- for i <= j < m the entries (i, j) and (i, n-1-j) of the upper triangle, the
// wedge between the diagonal and the anti-diagonal, each once -- so it is centrosymmetric by construction; E is M - C on
// the last row and column: u_i = M(i, n-1) - M(0, n-1-i), u_{n-1} = (M(n-1, n-1) - M(0, 0)) / 2.
#include <hip/hip_runtime.h>

#include "emme_device.hpp"
#include "fold_combine.hpp"
#include "launch.hpp"

namespace emme {

namespace {

using namespace trisolve;
using namespace fold;

constexpr int FT = 32;  // tile edge of the fold pass

// u(k) of one matrix X (upper triangle): the part of column n-1 that the mirror image of row 0 does not explain
__device__ __forceinline__ cd edge_u(const double2* X, int n, int k) {
    if (k == n - 1) return 0.5 * (ld2(&X[(size_t)(n - 1) * n + n - 1]) - ld2(&X[0]));
    return ld2(&X[(size_t)k * n + n - 1]) - ld2(&X[n - 1 - k]);
}

// vecs[b][4][m]: u+, u-, u'+, u'- (unnormalised folds); act2[2b], act2[2b + 1]: the half problems' live flags
__global__ __launch_bounds__(256) void k_fold_edges(int n, const double2* M, const double2* Mold, const double2* domega,
                                                    const int* active, double2* vecs, int* act2) {
    const int b = blockIdx.x;
    const int live = active ? active[b] != 0 : 1;
    if (threadIdx.x == 0) act2[2 * b] = live, act2[2 * b + 1] = live;
    if (!live) return;
    const int m = n / 2;
    const cd rdw = rcp(mk(domega[b].x, domega[b].y));
    const double2* X = M + (size_t)b * n * n;
    const double2* O = Mold + (size_t)b * n * n;
    double2* v = vecs + (size_t)b * 4 * m;
    for (int i = threadIdx.x; i < m; i += 256) {
        const int i2 = n - 1 - i;
        const cd u1 = edge_u(X, n, i), u2 = edge_u(X, n, i2);
        const cd d1 = (u1 - edge_u(O, n, i)) * rdw, dd2 = (u2 - edge_u(O, n, i2)) * rdw;
        v[i] = d2(u1 + u2), v[m + i] = d2(u1 - u2);
        v[2 * m + i] = d2(d1 + dd2), v[3 * m + i] = d2(d1 - dd2);
    }
}

// blockIdx.x < nfold: tile (I, J), I <= J, of the m x m grid of S: entry (i, j), i <= j, from P = X(i, j) and
// Q = X(i, n-1-j); S+- = P +- Q and the secants likewise, written with their mirror images (S is symmetric) for the half
// problems 2b (+) and 2b + 1 (-): S to S1 and S2, S' to D1 and D2.  M_old = M at both places, if Mold_w is given.
// Beyond: the tiles of the n x n grid for what is left of the upper triangle -- right of the anti-diagonal -- M_old = M.
__global__ __launch_bounds__(256) void k_fold_pass(int n, int nfold, const double2* M, const double2* Mold, double2* Mold_w,
                                                   double2* S1, double2* S2, double2* D1, double2* D2,
                                                   const double2* domega, const int* active) {
    const int b = blockIdx.y;
    if (active && active[b] == 0) return;
    __shared__ double2 s_p[FT][FT + 1], s_m[FT][FT + 1];
    const int m = n / 2;
    const size_t base = (size_t)b * n * n;
    const int tx = threadIdx.x & (FT - 1), ty = threadIdx.x / FT;  // 32 x 8 threads, 4 rows each
    const bool copy_tile = (int)blockIdx.x >= nfold;
    const int nt = ((copy_tile ? n : m) + FT - 1) / FT;
    int I = 0, rem = copy_tile ? blockIdx.x - nfold : blockIdx.x;
    while (rem >= nt - I) rem -= nt - I, ++I;
    const int J = I + rem;
    if (copy_tile) {
        if (I * FT + J * FT + 2 * (FT - 1) <= n - 1) return;  // the whole tile lies left of the anti-diagonal
        for (int rr = ty; rr < FT; rr += 256 / FT) {
            const int r = I * FT + rr, c = J * FT + tx;
            if (r < n && c < n && r <= c && c > n - 1 - r) Mold_w[base + (size_t)r * n + c] = M[base + (size_t)r * n + c];
        }
        return;
    }
    const cd rdw = rcp(mk(domega[b].x, domega[b].y));
    cd dp[FT / 8], dm[FT / 8];
#pragma unroll
    for (int q = 0; q < FT / 8; ++q) {
        const int rr = ty + 8 * q;
        const int i = I * FT + rr, j = J * FT + tx;
        cd sp = mk(0.0, 0.0), sm = sp;
        dp[q] = sp, dm[q] = sp;
        if (i < m && j < m && (I != J || rr <= tx)) {
            const size_t ip = base + (size_t)i * n + j, iq = base + (size_t)i * n + (n - 1 - j);
            const double2 vp = M[ip], vq = M[iq];
            const cd P = mk(vp.x, vp.y), Q = mk(vq.x, vq.y);
            const cd Pd = (P - ld2(&Mold[ip])) * rdw, Qd = (Q - ld2(&Mold[iq])) * rdw;
            if (Mold_w) Mold_w[ip] = vp, Mold_w[iq] = vq;
            sp = P + Q, sm = P - Q;
            dp[q] = Pd + Qd, dm[q] = Pd - Qd;
        }
        s_p[rr][tx] = d2(sp), s_m[rr][tx] = d2(sm);
    }
    // tile (I, J) itself (a diagonal tile takes its lower half from the transposed upper half) and its mirror image
    auto write_out = [&](double2* out1, double2* out2) {
        double2* p1 = out1 + (size_t)(2 * b) * m * m;
        double2* p2 = out2 + (size_t)(2 * b) * m * m;
        const size_t minus = (size_t)m * m;  // the - half follows the + half
        for (int rr = ty; rr < FT; rr += 256 / FT) {
            const int r = I * FT + rr, c = J * FT + tx;
            if (r < m && c < m) {
                const bool lower = I == J && rr > tx;
                const size_t idx = (size_t)r * m + c;
                const double2 vp = lower ? s_p[tx][rr] : s_p[rr][tx], vm = lower ? s_m[tx][rr] : s_m[rr][tx];
                p1[idx] = vp, p2[idx] = vp, p1[minus + idx] = vm, p2[minus + idx] = vm;
            }
        }
        if (I != J) {
            for (int rr = ty; rr < FT; rr += 256 / FT) {
                const int r = J * FT + rr, c = I * FT + tx;
                if (r < m && c < m) {
                    const size_t idx = (size_t)r * m + c;
                    const double2 vp = s_p[tx][rr], vm = s_m[tx][rr];
                    p1[idx] = vp, p2[idx] = vp, p1[minus + idx] = vm, p2[minus + idx] = vm;
                }
            }
        }
    };
    __syncthreads();
    write_out(S1, S2);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < FT / 8; ++q) s_p[ty + 8 * q][tx] = d2(dp[q]), s_m[ty + 8 * q][tx] = d2(dm[q]);
    __syncthreads();
    write_out(D1, D2);
}

constexpr int NPART = 9;  // per half problem: e.a, e.b, u.a, u.b, u'.a, u'.b, b^T S' a, a^T S' a, b^T S' b

struct FoldSolveArgs {
    int m, nb, nblk;     // order of a half problem; rows per panel snapshot and snapshots per matrix of its factorisation
    const double2* A;    // [2 nbatch][m][m] P S = L U in place
    const int* maps;     // [2 nbatch][nblk][m] row-order snapshots
    const int* items;    // half problems of this launch (null: 0 .. grid-1)
    const int* lu_info;  // per half problem: 0, or the column at which the factorisation stopped
    const double2* D;    // [2 nbatch][m][m] S'
    const double2* vecs; // [nbatch][4][m] (k_fold_edges)
    double2* part;       // [2 nbatch][NPART]
};

// One 512-thread workgroup per half problem h = 2b + s: a = S^-1 u_s, b = S^-1 e_s (e+ = e_0, e- = -e_0: the folds of
// e_{n-1}), then one pass over S' for the forms.  Every sum is taken in a fixed order.
__global__ __launch_bounds__(NT) void k_fold_solve(FoldSolveArgs P) {
    extern __shared__ double2 sm[];
    __shared__ double s_red[6 * NW];
    const int m = P.m;
    const int h = pick_item(P.items);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double2* out = P.part + (size_t)h * NPART;
    if (P.lu_info[h] != 0) return nan_out(out, NPART);  // no factorisation: the chain's step fails (k_fold_combine)
    const Half H(h, P.vecs, m);
    const double sgn = H.sgn;
    const double2 *u = H.u, *ud = H.ud;
    const Frame fr(sm, m, P.A + (size_t)h * m * m);
    double2* x0 = fr.x0;  // the right-hand side
    double2* xa = fr.x1;  // a
    double2* xb = fr.x2;  // b
    fr.load_rowmap(P.maps + (size_t)h * P.nblk * m, P.nb);
    for (int x = tid; x < m; x += NT) x0[x] = u[x];
    __syncthreads();
    solve_plain(fr.F, x0, xa);
    for (int x = tid; x < m; x += NT) x0[x] = make_double2(x == 0 ? sgn : 0.0, 0.0);
    __syncthreads();
    solve_plain(fr.F, x0, xb);
    // the three forms with S': row r by wave r mod NW, the lanes' partial sums by xor shuffles
    const double2* D = P.D + (size_t)h * m * m;
    cd fba = mk(0.0, 0.0), faa = fba, fbb = fba;
    for (int r = wave; r < m; r += NW) {
        const double2* row = D + (size_t)r * m;
        cd ya = mk(0.0, 0.0), yb = ya;
        for (int c = lane; c < m; c += 64) {
            const cd d = ld2(&row[c]);
            ya = ya + d * mk(xa[c].x, xa[c].y);
            yb = yb + d * mk(xb[c].x, xb[c].y);
        }
        ya.x = wave_sum(ya.x), ya.y = wave_sum(ya.y), yb.x = wave_sum(yb.x), yb.y = wave_sum(yb.y);
        const cd ar = mk(xa[r].x, xa[r].y), br = mk(xb[r].x, xb[r].y);
        fba = fba + br * ya, faa = faa + ar * ya, fbb = fbb + br * yb;
    }
    double t[6], t2[2];
    {
        const double v[6] = {fba.x, fba.y, faa.x, faa.y, fbb.x, fbb.y};  // (every lane of a wave holds the wave's sums)
        block_sum(s_red, v, t);
    }
    if (tid == 0) {
        out[6] = make_double2(t[0], t[1]), out[7] = make_double2(t[2], t[3]), out[8] = make_double2(t[4], t[5]);
        out[0] = make_double2(sgn * xa[0].x, sgn * xa[0].y), out[1] = make_double2(sgn * xb[0].x, sgn * xb[0].y);
    }
    // the dot products with u and u'
    cd ua = mk(0.0, 0.0), ub = ua, da = ua, db = ua;
    for (int x = tid; x < m; x += NT) {
        const cd a = mk(xa[x].x, xa[x].y), bb = mk(xb[x].x, xb[x].y), uu = ld2(&u[x]), dd = ld2(&ud[x]);
        ua = ua + uu * a, ub = ub + uu * bb, da = da + dd * a, db = db + dd * bb;
    }
    __syncthreads();  // (s_red is read no more)
    {
        const double v[6] = {wave_sum(ua.x), wave_sum(ua.y), wave_sum(ub.x), wave_sum(ub.y), wave_sum(da.x), wave_sum(da.y)};
        block_sum(s_red, v, t);
    }
    if (tid == 0) out[2] = make_double2(t[0], t[1]), out[3] = make_double2(t[2], t[3]), out[4] = make_double2(t[4], t[5]);
    __syncthreads();
    {
        const double v[2] = {wave_sum(db.x), wave_sum(db.y)};
        block_sum(s_red, v, t2);
    }
    if (tid == 0) out[5] = make_double2(t2[0], t2[1]);
}

// tr[b] and info[b] of every live chain from its two half problems: tr2 / info2 of the trace kernel, lu_info of the
// second factorisation, part of k_fold_solve.  info: a half's own code (a stopped factorisation: its column, in the -
// half plus m; a hand-over time-out as it is), n + 1 where det K is zero or not finite; tr is NaN then.
__global__ void k_fold_combine(int n, int nbatch, const int* active, const double2* tr2, const int* info2,
                               const int* lu_info, const double2* part, double2* tr, int* info) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nbatch) return;
    if (active && active[b] == 0) return;
    auto half_info = [&](int s) { return info2[2 * b + s] != 0 ? info2[2 * b + s] : lu_info[2 * b + s]; };
    int inf = merge_half_info(half_info(0), half_info(1), n / 2);
    const double2* pp = part + (size_t)(2 * b) * NPART;
    const double2* pm = pp + NPART;
    const cd ea = both(pp, pm, 0), eb = both(pp, pm, 1), ua = both(pp, pm, 2), ub = both(pp, pm, 3);
    const cd au = both(pp, pm, 4), bu = both(pp, pm, 5), fba = both(pp, pm, 6), faa = both(pp, pm, 7), fbb = both(pp, pm, 8);
    const cd g11 = fba + bu * ea + eb * au;  // b^T M' a = b^T C' a + (b.u')(e.a) + (b.e)(u'.a)
    const cd g12 = fbb + 2.0 * (bu * eb);    // b^T M' b
    const cd g21 = faa + 2.0 * (au * ea);    // a^T M' a
    const WoodburyK K(ea, eb, ua, ub);
    if (inf == 0 && !K.ok) inf = n + 1;
    const cd trkg = (K.k22 * g11 - K.k12 * g21 - K.k21 * g12 + K.k11 * g11) * rcp(K.det);
    const cd t = ld2(&tr2[2 * b]) + ld2(&tr2[2 * b + 1]) + 2.0 * bu - trkg;
    const double qnan = __builtin_nan("");
    tr[b] = inf != 0 ? make_double2(qnan, qnan) : d2(t);
    info[b] = inf;
}

}  // namespace

size_t fold_part_bytes(int nbatch) { return sizeof(double2) * NPART * 2 * (size_t)nbatch; }

hipError_t launch_fold_edges(int n, int nbatch, const double* M, const double* Mold, const double* domega,
                             const int* active, double* vecs, int* act2, hipStream_t stream) {
    hipLaunchKernelGGL(k_fold_edges, dim3(nbatch), dim3(256), 0, stream, n, (const double2*)M, (const double2*)Mold,
                       (const double2*)domega, active, (double2*)vecs, act2);
    return hipGetLastError();
}

hipError_t launch_fold_pass(int n, int nbatch, const double* M, const double* Mold, double* Mold_w, double* S1, double* S2,
                            double* D1, double* D2, const double* domega, const int* active, hipStream_t stream) {
    const int m = n / 2;
    const int ntm = (m + FT - 1) / FT, ntn = (n + FT - 1) / FT;
    const int nfold = ntm * (ntm + 1) / 2, ncopy = Mold_w ? ntn * (ntn + 1) / 2 : 0;
    hipLaunchKernelGGL(k_fold_pass, dim3((unsigned)(nfold + ncopy), nbatch), dim3(256), 0, stream, n, nfold,
                       (const double2*)M, (const double2*)Mold, (double2*)Mold_w, (double2*)S1, (double2*)S2, (double2*)D1,
                       (double2*)D2, (const double2*)domega, active);
    return hipGetLastError();
}

hipError_t launch_fold_solve(int m, const double* S_lu, const int* rowmaps, int nb, const int* items, int nitems,
                             const int* lu_info, const double* Sp, const double* vecs, double* part, hipStream_t stream) {
    FoldSolveArgs P;
    P.m = m, P.nb = nb, P.nblk = (m + nb - 1) / nb;
    P.A = (const double2*)S_lu, P.maps = rowmaps, P.items = items, P.lu_info = lu_info;
    P.D = (const double2*)Sp, P.vecs = (const double2*)vecs, P.part = (double2*)part;
    return launch_dyn_lds(k_fold_solve, nitems, frame_lds(m), stream, P);
}

hipError_t launch_fold_combine(int n, int nbatch, const int* active, const double* tr2, const int* info2, const int* lu_info,
                               const double* part, double* tr, int* info, hipStream_t stream) {
    hipLaunchKernelGGL(k_fold_combine, dim3((nbatch + 63) / 64), dim3(64), 0, stream, n, nbatch, active, (const double2*)tr2,
                       info2, lu_info, (const double2*)part, (double2*)tr, info);
    return hipGetLastError();
}

}  // namespace emme
