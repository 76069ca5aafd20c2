// ctx_sens.hip -- root sensitivities from eigenpairs, above sym_forms.hip: the entry points
// emme_sym_forms_batch (the forms on caller matrices) and emme_root_sensitivities_sets (d omega / d p of roots over
// bound parameter sets, with the Rayleigh-functional correction and the eigenvalue condition number).  The chunk plan
// is plain C++ (sens_plan.cpp); the fills are emme_assemble_sets_batch's, request for request.
#include "ctx.hpp"
#include "sens_plan.hpp"

using namespace emme;

namespace {

// One fill over sets as emme_assemble_sets_batch issues it: items (set[b], omega[b]) into dM (and, dMp given, the exact
// dM/domega beside it).  set and omega are host arrays.  The status flags and interval counts are queued into st / iv,
// valid after the caller's next synchronisation.
int fill_sets(emme_ctx* c, const int* set, const double* omega, int nbatch, double* dM, double* dMp,
              std::vector<unsigned long long>& iv, std::vector<int>& st) {
    EMME_TRY(ensure_batch(c, nbatch));
    EMME_TRY(upload_set_indices(c, set, nbatch));
    EMME_TRY(upload_omega(c, omega, nbatch, hipMemcpyDefault));
    EMME_TRY(reset_fill_counters(c, nbatch));
    FillRequest r(nbatch, c->d_omega, dM);
    r.d_Md = dMp, r.d_set = c->d_set, r.host_set = set, r.host_omega = omega;
    EMME_TRY(fill(c, r));
    return queue_fill_counters(c, nbatch, iv, &st);
}

bool index_range_ok(const int* idx, int count, int lo, int hi, const char* name, const std::string& who) {
    for (int t = 0; t < count; ++t)
        if (idx[t] < lo || idx[t] >= hi) {
            set_error(who + ": " + name + "[" + std::to_string(t) + "] = " + std::to_string(idx[t]) + " is outside [" +
                      std::to_string(lo) + ", " + std::to_string(hi) + ")");
            return false;
        }
    return true;
}

// the unsplit form of k_sym_forms, for the one measurement of the split (tools/sensitivities_vs_resolve.py)
bool forms_split() {
    const char* e = std::getenv("EMME_SYM_FORMS_SPLIT");
    return !(e && e[0] == '0');
}

}  // namespace

extern "C" {

int emme_sym_forms_batch(emme_ctx_t* c, int n, int nmat, const double* A, const double* B, int nvec, const double* vecs,
                         int nitems, const int* a, const int* b, const int* x, const int* y, double* form, double* fro2) {
    const std::string who = "emme_sym_forms_batch";
    if (!c || !A || !vecs || !a || !x || !form || n < 1 || nmat < 1 || nvec < 1 || nitems < 1) {
        set_error(who + ": a required pointer is NULL, or n, nmat, nvec or nitems < 1");
        return EMME_EINVAL;
    }
    if (b && !B) {
        set_error(who + ": b names second matrices but B is NULL");
        return EMME_EINVAL;
    }
    if (!index_range_ok(a, nitems, 0, nmat, "a", who) || (b && !index_range_ok(b, nitems, -1, nmat, "b", who)) ||
        !index_range_ok(x, nitems, 0, nvec, "x", who) || (y && !index_range_ok(y, nitems, 0, nvec, "y", who)))
        return EMME_EINVAL;
    if (n > 2048) {
        set_error(who + ": order above 2048 is not supported");
        return EMME_ECONFIG;
    }
    HIP_TRY(hipSetDevice(c->device));
    const size_t mbytes = batch_bytes(n, nmat);
    const double *dA = A, *dB = B;
    DeviceBuffer<double> t_a, t_b;
    if (B) {
        bool dev = false;
        EMME_TRY(same_side(A, B, "A and B", &dev));
        if (!dev) {
            HIP_TRY(t_a.grow(mbytes));
            HIP_TRY(t_b.grow(mbytes));
            HIP_TRY(hipMemcpyAsync(t_a, A, mbytes, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(t_b, B, mbytes, hipMemcpyHostToDevice, c->stream));
            dA = t_a, dB = t_b;
        }
    } else if (!is_device_ptr(A)) {
        HIP_TRY(t_a.grow(mbytes));
        HIP_TRY(hipMemcpyAsync(t_a, A, mbytes, hipMemcpyHostToDevice, c->stream));
        dA = t_a;
    }
    const bool split = forms_split();
    const int nblk = sym_forms_blocks(n, split);
    // device scratch of this call: vectors, the four index lists, the partial sums, the results
    DeviceBuffer<double> t_v, t_part, t_out;
    DeviceBuffer<int> t_idx;
    const size_t vbytes = sizeof(double) * 2 * (size_t)n * nvec;
    HIP_TRY(t_v.grow(vbytes));
    HIP_TRY(t_idx.grow(sizeof(int) * 4 * (size_t)nitems));
    HIP_TRY(t_part.grow(sizeof(double) * 4 * (size_t)nitems * nblk));
    HIP_TRY(t_out.grow(sizeof(double) * 3 * (size_t)nitems));
    HIP_TRY(hipMemcpyAsync(t_v, vecs, vbytes, hipMemcpyHostToDevice, c->stream));
    const int* lists[4] = {a, b, x, y};
    int* d_lists[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 4; ++k)
        if (lists[k]) {
            d_lists[k] = t_idx + (size_t)k * nitems;
            HIP_TRY(hipMemcpyAsync(d_lists[k], lists[k], sizeof(int) * (size_t)nitems, hipMemcpyHostToDevice, c->stream));
        }
    {
        ScopedSpan sp(c, K_OTHER);
        HIP_TRY(launch_sym_forms(n, dA, dB, t_v, d_lists[0], d_lists[1], d_lists[2], d_lists[3], nitems, t_part, split,
                                 c->stream));
        SymFormsFinish F{};
        F.mode = SYM_FORMS_PLAIN, F.count = nitems, F.nblk = nblk, F.n = n, F.part = t_part;
        F.form = t_out, F.fro2 = t_out + 2 * (size_t)nitems;
        HIP_TRY(launch_sym_forms_finish(F, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(form, t_out, sizeof(double) * 2 * (size_t)nitems, hipMemcpyDeviceToHost, c->stream));
    if (fro2)
        HIP_TRY(hipMemcpyAsync(fro2, t_out + 2 * (size_t)nitems, sizeof(double) * (size_t)nitems, hipMemcpyDeviceToHost,
                               c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return EMME_OK;
}

int emme_root_sensitivities_sets(emme_ctx_t* c, int nroots, const int* set, const double* roots, const double* vecs,
                                 int ndir, const int* set_plus, const int* set_minus, const double* dp, int max_items,
                                 double* dwdp, double* denom, double* corr, double* cond, int* info) {
    const std::string who = "emme_root_sensitivities_sets";
    if (!c || !set || !roots || !vecs || !denom || !corr || !cond || !info || nroots < 1 || ndir < 0 || max_items < 0 ||
        (ndir > 0 && (!set_plus || !set_minus || !dp || !dwdp))) {
        set_error(who + ": a required pointer is NULL, nroots < 1, ndir < 0 or max_items < 0");
        return EMME_EINVAL;
    }
    const size_t nslots = (size_t)nroots * ndir;
    for (size_t q = 0; q < nslots; ++q)
        if (!(dp[q] != 0.0) || !std::isfinite(dp[q])) {
            set_error(who + ": dp[" + std::to_string(q) + "] is zero or not finite");
            return EMME_EINVAL;
        }
    // (a negative index needs no context to be wrong)
    for (int r = 0; r < nroots; ++r)
        if (set[r] < 0) {
            set_error(who + ": set[" + std::to_string(r) + "] = " + std::to_string(set[r]) + " is negative");
            return EMME_EINVAL;
        }
    for (size_t q = 0; q < nslots; ++q)
        if (set_plus[q] < 0 || set_minus[q] < 0) {
            set_error(who + ": set_plus / set_minus[" + std::to_string(q) + "] is negative");
            return EMME_EINVAL;
        }
    EMME_TRY(check_set_indices(c, set, nroots, who.c_str()));
    if (ndir > 0) {
        EMME_TRY(check_set_indices(c, set_plus, (int)nslots, (who + " (set_plus)").c_str()));
        EMME_TRY(check_set_indices(c, set_minus, (int)nslots, (who + " (set_minus)").c_str()));
    }
    const int dim = c->dim;
    if (dim > 2048) {
        set_error(who + ": matrix dimension above 2048 is not supported");
        return EMME_ECONFIG;
    }
    // the eigenpairs: a NaN (or otherwise non-finite) root or vector row is the blanked output of a failed chain and
    // takes ITS root out of the call; a zero vector is a caller's mistake
    std::vector<int> good;
    std::vector<double> vnorm2(nroots, 0.0);
    for (int r = 0; r < nroots; ++r) {
        const double* row = vecs + 2 * (size_t)r * dim;
        bool finite = std::isfinite(roots[2 * r]) && std::isfinite(roots[2 * r + 1]);
        double s2 = 0.0;
        for (int i = 0; i < 2 * dim; ++i) finite = finite && std::isfinite(row[i]), s2 += row[i] * row[i];
        finite = finite && std::isfinite(s2);
        if (finite && !(s2 > 0.0)) {
            set_error(who + ": vector row " + std::to_string(r) + " is zero");
            return EMME_EINVAL;
        }
        vnorm2[r] = s2;
        if (finite) good.push_back(r);
    }
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    std::fill(denom, denom + 2 * (size_t)nroots, qnan);
    std::fill(corr, corr + 2 * (size_t)nroots, qnan);
    std::fill(cond, cond + nroots, qnan);
    if (ndir > 0) std::fill(dwdp, dwdp + 2 * nslots, qnan);
    std::fill(info, info + nroots, (int)EMME_ENUMERIC);
    const int ng = (int)good.size();
    if (ng == 0) return EMME_OK;

    HIP_TRY(hipSetDevice(c->device));
    const SensPlan plan = sens_plan(ng, ndir, max_items, dim);
    // the matrices of the largest chunk, all in d_M: M | M' of a base chunk's roots, (M+, M-) of a neighbour chunk's pairs
    const int per = (int)std::min<size_t>((size_t)plan.cap / 2, (size_t)ng * (size_t)std::max(ndir, 1));
    EMME_TRY(ensure_mats(c, 2 * per, 1));
    const bool split = forms_split();
    const int nblk = sym_forms_blocks(dim, split);
    // device scratch of this call: the vectors, |v|^2, dp, the results (denom | corr | cond | dwdp), info, and per
    // chunk the index lists (a | b | x | root | slot) and the partial sums
    const size_t max_forms = 2 * (size_t)per;
    DeviceBuffer<double> t_v, t_vn, t_dp, t_res, t_part;
    DeviceBuffer<int> t_info, t_idx;
    const size_t vbytes = sizeof(double) * 2 * (size_t)dim * nroots;
    const size_t nres = 5 * (size_t)nroots + 2 * nslots;
    HIP_TRY(t_v.grow(vbytes));
    HIP_TRY(t_vn.grow(sizeof(double) * nroots));
    HIP_TRY(t_res.grow(sizeof(double) * nres));
    HIP_TRY(t_info.grow(sizeof(int) * nroots));
    HIP_TRY(t_idx.grow(sizeof(int) * 5 * max_forms));
    HIP_TRY(t_part.grow(sizeof(double) * 4 * max_forms * nblk));
    HIP_TRY(hipMemcpyAsync(t_v, vecs, vbytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(t_vn, vnorm2.data(), sizeof(double) * nroots, hipMemcpyHostToDevice, c->stream));
    if (ndir > 0) {
        HIP_TRY(t_dp.grow(sizeof(double) * nslots));
        HIP_TRY(hipMemcpyAsync(t_dp, dp, sizeof(double) * nslots, hipMemcpyHostToDevice, c->stream));
    }
    double* d_denom = t_res;
    double* d_corr = d_denom + 2 * (size_t)nroots;
    double* d_cond = d_corr + 2 * (size_t)nroots;
    double* d_dwdp = d_cond + nroots;
    // what the chunks' fills report, read after the one synchronisation at the end
    struct ChunkFlags {
        std::vector<unsigned long long> iv;
        std::vector<int> st;
    };
    std::vector<ChunkFlags> base_flags(plan.base.size()), pair_flags(plan.pairs.size());
    // host images of a chunk's lists, kept until the stream has read them
    std::vector<std::vector<int>> kept_idx;
    std::vector<std::vector<double>> kept_w;
    auto stage_lists = [&](const std::vector<int>& idx) -> int {
        // (the previous chunk's kernels may still read t_idx: the copy is ordered behind them on the stream)
        HIP_TRY(hipMemcpyAsync(t_idx, idx.data(), sizeof(int) * idx.size(), hipMemcpyHostToDevice, c->stream));
        return EMME_OK;
    };

    // ---- M and M' at (set[r], omega_r): v^T M v, v^T M' v and the two Frobenius norms ----
    for (size_t k = 0; k < plan.base.size(); ++k) {
        const SensChunk ch = plan.base[k];
        std::vector<int> st(ch.count);
        std::vector<double> w(2 * (size_t)ch.count);
        const size_t L = 2 * (size_t)ch.count;  // forms of the chunk: item 2g of M_g, item 2g + 1 of M'_g
        std::vector<int> idx(3 * L);            // a | x | root (one per root)
        for (int g = 0; g < ch.count; ++g) {
            const int r = good[ch.first + g];
            st[g] = set[r], w[2 * g] = roots[2 * r], w[2 * g + 1] = roots[2 * r + 1];
            idx[2 * g] = g, idx[2 * g + 1] = ch.count + g;  // (M' of the chunk lies behind its M, below)
            idx[L + 2 * g] = r, idx[L + 2 * g + 1] = r;
            idx[2 * L + g] = r;
        }
        kept_idx.push_back(std::move(idx)), kept_w.push_back(std::move(w));
        double* dMp = c->d_M + (size_t)ch.count * dim * dim * 2;
        EMME_TRY(fill_sets(c, st.data(), kept_w.back().data(), ch.count, c->d_M, dMp, base_flags[k].iv, base_flags[k].st));
        EMME_TRY(stage_lists(kept_idx.back()));
        ScopedSpan sp(c, K_OTHER);
        HIP_TRY(launch_sym_forms(dim, c->d_M, nullptr, t_v, t_idx, nullptr, t_idx + L, nullptr, (int)L, t_part, split,
                                 c->stream));
        SymFormsFinish F{};
        F.mode = SYM_FORMS_BASE, F.count = ch.count, F.nblk = nblk, F.n = dim, F.part = t_part;
        F.root = t_idx + 2 * L, F.vnorm2 = t_vn;
        F.denom = d_denom, F.corr = d_corr, F.cond = d_cond, F.info = t_info;
        HIP_TRY(launch_sym_forms_finish(F, c->stream));
    }
    // ---- the neighbour matrices at (set+-, omega_r): v^T (M+ - M-) v, the difference per entry ----
    for (size_t k = 0; k < plan.pairs.size(); ++k) {
        const SensChunk ch = plan.pairs[k];
        const size_t L = (size_t)ch.count;
        std::vector<int> st(2 * L);
        std::vector<double> w(4 * L);
        std::vector<int> idx(5 * L);
        for (int j = 0; j < ch.count; ++j) {
            const int pair = ch.first + j, r = good[pair / ndir], q = r * ndir + pair % ndir;
            st[2 * j] = set_plus[q], st[2 * j + 1] = set_minus[q];
            w[4 * j] = w[4 * j + 2] = roots[2 * r], w[4 * j + 1] = w[4 * j + 3] = roots[2 * r + 1];
            idx[j] = 2 * j, idx[L + j] = 2 * j + 1, idx[2 * L + j] = r, idx[3 * L + j] = r, idx[4 * L + j] = q;
        }
        kept_idx.push_back(std::move(idx)), kept_w.push_back(std::move(w));
        EMME_TRY(fill_sets(c, st.data(), kept_w.back().data(), 2 * ch.count, c->d_M, nullptr, pair_flags[k].iv, pair_flags[k].st));
        EMME_TRY(stage_lists(kept_idx.back()));
        ScopedSpan sp(c, K_OTHER);
        HIP_TRY(launch_sym_forms(dim, c->d_M, c->d_M, t_v, t_idx, t_idx + L, t_idx + 2 * L, nullptr, ch.count, t_part, split,
                                 c->stream));
        SymFormsFinish F{};
        F.mode = SYM_FORMS_NEIGHBOUR, F.count = ch.count, F.nblk = nblk, F.n = dim, F.part = t_part;
        F.root = t_idx + 3 * L, F.slot = t_idx + 4 * L, F.dp = t_dp;
        F.denom = d_denom, F.dwdp = d_dwdp, F.info = t_info;
        HIP_TRY(launch_sym_forms_finish(F, c->stream));
    }
    // ---- one small copy returns everything ----
    std::vector<double> res(nres);
    std::vector<int> h_info(nroots);
    HIP_TRY(hipMemcpyAsync(res.data(), t_res, sizeof(double) * nres, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h_info.data(), t_info, sizeof(int) * nroots, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const double* h_denom = res.data();
    const double* h_corr = h_denom + 2 * (size_t)nroots;
    const double* h_cond = h_corr + 2 * (size_t)nroots;
    const double* h_dwdp = h_cond + nroots;
    for (size_t k = 0; k < plan.base.size(); ++k) {
        (void)fold_fill_counters(c, base_flags[k].iv, nullptr);
        for (int g = 0; g < plan.base[k].count; ++g) {
            const int r = good[plan.base[k].first + g];
            if (base_flags[k].st[g] != 0) continue;  // a fill that hit the depth cap or was not finite: EMME_ENUMERIC stays
            info[r] = h_info[r];
            denom[2 * r] = h_denom[2 * r], denom[2 * r + 1] = h_denom[2 * r + 1];
            corr[2 * r] = h_corr[2 * r], corr[2 * r + 1] = h_corr[2 * r + 1];
            cond[r] = h_cond[r];
        }
    }
    for (size_t k = 0; k < plan.pairs.size(); ++k) {
        (void)fold_fill_counters(c, pair_flags[k].iv, nullptr);
        for (int j = 0; j < plan.pairs[k].count; ++j) {
            const int pair = plan.pairs[k].first + j, r = good[pair / ndir];
            const size_t q = (size_t)r * ndir + pair % ndir;
            if (info[r] != 0 || pair_flags[k].st[2 * j] != 0 || pair_flags[k].st[2 * j + 1] != 0) continue;  // NaN stays
            dwdp[2 * q] = h_dwdp[2 * q], dwdp[2 * q + 1] = h_dwdp[2 * q + 1];
        }
    }
    return EMME_OK;
}

}  // extern "C"
