// sym_forms.hip -- batched bilinear forms on matrix differences: per item t
//     f[t] = x_t^T (A_a - B_b) y_t   (complex; transpose, not conjugate),   s[t] = |A_a - B_b|_F^2,
// the difference taken entry by entry BEFORE it meets the vectors, as in k_eigpair_secant_step (eigpair.hip): x^T A y
// and x^T B y of two neighbouring fills are each O(1) with an O(delta) difference, while single entries of A and B
// agree in most digits.  b[t] < 0: no second matrix.  Nothing here assumes symmetry; a symmetric caller passes x = y.
//
// k_sym_forms: the work unit is (item, block of `rows` rows), one 512-thread workgroup per unit.  y is staged in LDS;
// inside a unit a wave takes a row at a time, rows dealt to the waves in a fixed order (row r0 + w, r0 + w + 8, ...),
// columns strided over the lanes with 16-byte loads, the lanes' sums by xor shuffles, a wave's rows added in row order
// and the waves' sums in wave order.  Every unit writes its partial (f, s) to part[item][block];
// k_sym_forms_finish adds an item's blocks in index order.  With rows = 64 the bits of a result therefore depend on n
// and the data alone -- not on the grid, on which items share a launch, or on the device -- nothing is atomic, and two
// runs are bit-identical.  (rows = n, one workgroup per item, is the unsplit form that tools/sensitivities_vs_resolve.py
// times against it; its sums group differently.)
//
// k_sym_forms_finish has three readings: the plain one (form, fro2 per item), and the two of
// emme_root_sensitivities_sets, which form the quotients on the device -- `base`: items (M_g, v_g), (M'_g, v_g) per
// root give denom, corr, cond and info; `neighbour`: item (M+, M-, v) of (root, direction) gives dw/dp.
#include <hip/hip_runtime.h>

#include <cmath>

#include "emme_device.hpp"
#include "launch.hpp"
#include "sens_plan.hpp"
#include "tri_solve.hpp"

namespace emme {

namespace {

using namespace trisolve;

struct FormsArgs {
    int n, rows, nblk;  // order; rows per unit; units per item = ceil(n / rows)
    const double2* A;   // [..][n][n]
    const double2* B;   // [..][n][n], null when no item names one
    const double2* vecs;  // [nvec][n]
    const int *a, *b, *x, *y;  // per item (device); b null: none, y null: y = x
    double* part;  // [nitems][nblk][4]: Re f, Im f, s, 0
};

__global__ __launch_bounds__(NT) void k_sym_forms(FormsArgs P) {
    extern __shared__ double2 sm[];  // y
    __shared__ double s_red[3 * NW];
    const int n = P.n;
    const int t = blockIdx.x / P.nblk, blk = blockIdx.x % P.nblk;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ia = P.a[t], ib = P.b ? P.b[t] : -1, ix = P.x[t], iy = P.y ? P.y[t] : ix;
    const double2* xv = P.vecs + (size_t)ix * n;
    const double2* yv = P.vecs + (size_t)iy * n;
    for (int i = tid; i < n; i += NT) sm[i] = yv[i];
    __syncthreads();
    const int r0 = blk * P.rows, r1 = min(n, r0 + P.rows);
    const double2* matA = P.A + (size_t)ia * n * n;
    cd f = mk(0.0, 0.0);
    double fro = 0.0;
    if (ib >= 0) {  // uniform
        const double2* matB = P.B + (size_t)ib * n * n;
        for (int r = r0 + wave; r < r1; r += NW) {
            const double2* rowA = matA + (size_t)r * n;
            const double2* rowB = matB + (size_t)r * n;
            cd acc = mk(0.0, 0.0);
#pragma unroll 4
            for (int c = lane; c < n; c += 64) {
                const cd d = ld2(&rowA[c]) - ld2(&rowB[c]);
                acc = acc + d * mk(sm[c].x, sm[c].y);
                fro += norm2(d);
            }
            acc.x = wave_sum(acc.x), acc.y = wave_sum(acc.y);
            f = f + ld2(&xv[r]) * acc;
        }
    } else {
        for (int r = r0 + wave; r < r1; r += NW) {
            const double2* rowA = matA + (size_t)r * n;
            cd acc = mk(0.0, 0.0);
#pragma unroll 4
            for (int c = lane; c < n; c += 64) {
                const cd d = ld2(&rowA[c]);
                acc = acc + d * mk(sm[c].x, sm[c].y);
                fro += norm2(d);
            }
            acc.x = wave_sum(acc.x), acc.y = wave_sum(acc.y);
            f = f + ld2(&xv[r]) * acc;
        }
    }
    // (after the xor shuffles every lane of a wave holds the same f; fro is still per lane)
    fro = wave_sum(fro);
    if (lane == 0) s_red[wave] = f.x, s_red[NW + wave] = f.y, s_red[2 * NW + wave] = fro;
    __syncthreads();
    if (tid == 0) {
        double fx = 0.0, fy = 0.0, s = 0.0;
#pragma unroll
        for (int k = 0; k < NW; ++k) fx += s_red[k], fy += s_red[NW + k], s += s_red[2 * NW + k];
        double* out = P.part + ((size_t)t * P.nblk + blk) * 4;
        out[0] = fx, out[1] = fy, out[2] = s, out[3] = 0.0;
    }
}

// an item's blocks in index order
__device__ __forceinline__ void sum_blocks(const double* part, int nblk, int t, cd& f, double& s) {
    f = mk(0.0, 0.0), s = 0.0;
    const double* p = part + (size_t)t * nblk * 4;
    for (int k = 0; k < nblk; ++k) f.x += p[4 * k], f.y += p[4 * k + 1], s += p[4 * k + 2];
}

__device__ __forceinline__ cd cdiv(cd a, cd b) {
    const double d = b.x * b.x + b.y * b.y;
    const cd q = a * mk(b.x, -b.y);
    return mk(q.x / d, q.y / d);
}

__global__ __launch_bounds__(256) void k_sym_forms_finish(SymFormsFinish F) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F.count) return;
    const double qnan = __builtin_nan("");
    cd f;
    double s;
    if (F.mode == SYM_FORMS_PLAIN) {
        sum_blocks(F.part, F.nblk, i, f, s);
        F.form[2 * i] = f.x, F.form[2 * i + 1] = f.y;
        if (F.fro2) F.fro2[i] = s;
    } else if (F.mode == SYM_FORMS_BASE) {
        // items 2 i, 2 i + 1: v^T M v with |M|_F^2, v^T M' v with |M'|_F^2
        cd fp;
        double sp;
        sum_blocks(F.part, F.nblk, 2 * i, f, s);
        sum_blocks(F.part, F.nblk, 2 * i + 1, fp, sp);
        const int r = F.root[i];
        const double vn2 = F.vnorm2[r];
        const double ad = hypot(fp.x, fp.y);
        cd corr = mk(qnan, qnan);
        double cond = qnan;
        int info = 0;
        if (!(isfinite(f.x) && isfinite(f.y) && isfinite(s) && isfinite(fp.x) && isfinite(fp.y) && isfinite(sp))) {
            info = -6;  // EMME_ENUMERIC: a non-finite base fill
            fp = mk(qnan, qnan);
        } else {
            cond = sqrt(s) * vn2 / ad;
            if (sens_form_at_rounding(ad, F.n, sqrt(sp), vn2))
                info = 1;
            else
                corr = -cdiv(f, fp);
        }
        F.denom[2 * r] = fp.x, F.denom[2 * r + 1] = fp.y;
        F.corr[2 * r] = corr.x, F.corr[2 * r + 1] = corr.y;
        F.cond[r] = cond;
        F.info[r] = info;
    } else {
        // item i: v^T (M+ - M-) v of (root, direction) = slot
        sum_blocks(F.part, F.nblk, i, f, s);
        const int r = F.root[i], q = F.slot[i];
        cd d = mk(qnan, qnan);
        if (F.info[r] == 0 && isfinite(f.x) && isfinite(f.y)) {
            const cd den = F.dp[q] * mk(F.denom[2 * r], F.denom[2 * r + 1]);
            d = -cdiv(f, den);
        }
        F.dwdp[2 * q] = d.x, F.dwdp[2 * q + 1] = d.y;
    }
}

}  // namespace

int sym_forms_blocks(int n, bool split) { return split ? (n + 63) / 64 : 1; }

hipError_t launch_sym_forms(int n, const double* A, const double* B, const double* vecs, const int* a, const int* b,
                            const int* x, const int* y, int nitems, double* part, bool split, hipStream_t stream) {
    if (nitems < 1) return hipSuccess;
    if (n < 1 || n > 2048) return hipErrorNotSupported;
    FormsArgs P{};
    P.n = n, P.rows = split ? 64 : n, P.nblk = sym_forms_blocks(n, split);
    P.A = (const double2*)A, P.B = (const double2*)B, P.vecs = (const double2*)vecs;
    P.a = a, P.b = B ? b : nullptr, P.x = x, P.y = y, P.part = part;
    const size_t lds = sizeof(double2) * (size_t)n;  // <= 32 KB
    hipLaunchKernelGGL(k_sym_forms, dim3((unsigned)nitems * (unsigned)P.nblk), dim3(NT), lds, stream, P);
    return hipGetLastError();
}

hipError_t launch_sym_forms_finish(const SymFormsFinish& F, hipStream_t stream) {
    if (F.count < 1) return hipSuccess;
    hipLaunchKernelGGL(k_sym_forms_finish, dim3((F.count + 255) / 256), dim3(256), 0, stream, F);
    return hipGetLastError();
}

}  // namespace emme
