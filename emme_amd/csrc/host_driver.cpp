// host_driver.cpp -- the solve-once / parameter-scan driver above the C ABI, and the null
// vector of the converged matrix.
//
// Mirrors reference src/main.cpp: solve_once_eigen (:19-80), the {head, step, tail} scan
// generator with its two-direction sweep and 0.01*step fuzz (:139-172), filter_input
// (:174-180), the scan loop with omega continuation and the NaN fall-back (:223-325), the
// output.json schema (:208-221, 246-262, 270-321) and the raw eigenMatrics/<key>Eq<v>.bin files
// (:255-257, 295-299, 61-63).  nullSpace (include/solver.h:58-112) runs on the device
// (emme_null_vectors_batch, nullspace.hip); the host version below (inverse iteration on M^H M with a
// partial-pivot LU of a complex SYMMETRIC M) is emme_null_vector: a second opinion for tests and tools.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/emme_hip.h"
#include "host_json.hpp"
#include "scan_plan.hpp"

namespace emme {
void set_error(const std::string& msg);
int params_from_value(const JsonValue& root, emme_params_t* out);
}

namespace {

using emme::JsonValue;
using emme::ScanGen;  // get_scan_generator, src/main.cpp:139-172 (scan_plan.hpp)
using cplx = std::complex<double>;

// ---- null vector: the right singular vector of the smallest singular value, by inverse iteration -------
// (M^H M)^-1 is applied as M^-1 M^-H through ONE LU of M itself (M complex symmetric => M^-H v =
// conj(M^-1 conj(v))): M^H M is never formed, so the factorisation sees cond(M), not its square; the
// convergence factor per sweep is (s_n / s_n-1)^2, four sweeps.
struct Lu {
    int n;
    std::vector<cplx> a;
    std::vector<int> piv;
    bool factor(const cplx* m, int n_) {
        n = n_;
        a.assign(m, m + (size_t)n * n);
        piv.resize(n);
        for (int k = 0; k < n; ++k) {
            int p = k;
            double best = std::abs(a[(size_t)k * n + k]);
            for (int r = k + 1; r < n; ++r) {
                const double v = std::abs(a[(size_t)r * n + k]);
                if (v > best) best = v, p = r;
            }
            piv[k] = p;
            if (p != k)
                for (int c = 0; c < n; ++c) std::swap(a[(size_t)k * n + c], a[(size_t)p * n + c]);
            cplx d = a[(size_t)k * n + k];
            if (d == cplx(0.0)) d = a[(size_t)k * n + k] = cplx(1e-300);  // exactly singular: perturb
            for (int r = k + 1; r < n; ++r) {
                const cplx f = a[(size_t)r * n + k] / d;
                a[(size_t)r * n + k] = f;
                if (f == cplx(0.0)) continue;
                for (int c = k + 1; c < n; ++c) a[(size_t)r * n + c] -= f * a[(size_t)k * n + c];
            }
        }
        return true;
    }
    void solve(std::vector<cplx>& x) const {
        for (int k = 0; k < n; ++k) {
            std::swap(x[k], x[piv[k]]);
            for (int r = k + 1; r < n; ++r) x[r] -= a[(size_t)r * n + k] * x[k];
        }
        for (int r = n - 1; r >= 0; --r) {
            cplx s = x[r];
            for (int c = r + 1; c < n; ++c) s -= a[(size_t)r * n + c] * x[c];
            x[r] = s / a[(size_t)r * n + r];
        }
    }
};

void null_vector_of(const cplx* m, int n, cplx* out) {
    Lu lu;
    lu.factor(m, n);
    std::vector<cplx> v(n);
    for (int i = 0; i < n; ++i) v[i] = cplx(1.0 + 0.37 * std::sin(1.0 + i), 0.21 * std::cos(2.0 * i));
    auto normalise = [&](std::vector<cplx>& x) {
        double s = 0;
        for (auto& e : x) s += std::norm(e);
        s = 1.0 / std::sqrt(s);
        for (auto& e : x) e *= s;
    };
    normalise(v);
    for (int it = 0; it < 4; ++it) {
        // u = M^-H v = conj(M^-1 conj(v));  v = M^-1 u
        for (auto& e : v) e = std::conj(e);
        lu.solve(v);
        for (auto& e : v) e = std::conj(e);
        normalise(v);
        lu.solve(v);
        normalise(v);
    }
    for (int i = 0; i < n; ++i) out[i] = v[i];
}

// ---- driver ---------------------------------------------------------------------------------
std::string date_string() {
    // reference src/functions.cpp:8-20: %FT%T%z with a colon inserted in the zone offset
    std::time_t t = std::time(nullptr);
    std::tm tm = *std::localtime(&t);
    char buf[64];
    std::strftime(buf, sizeof buf, "%FT%T%z", &tm);
    std::string s(buf);
    if (s.size() >= 5) {
        const char c = s[s.size() - 5];
        if (c == '+' || c == '-') s.insert(s.size() - 2, ":");
    }
    return s;
}

JsonValue filter_input(const JsonValue& all) {
    JsonValue in = all;
    for (auto& m : in.members)
        if (m.second.is_object()) m.second = JsonValue(m.second.at("head"));
    return in;
}

// What a search's per-chain info code becomes in a scan record: the text of the exception that turns the point into
// {"eigenvalue":"NaN","reason":...} (src/main.cpp:311-318); empty for info == 0.
std::string search_failure_text(int info) {
    if (info > 0) {
        // include/solver.h:142-153.  The reference prints zsysv's index of the singular block of its LDL^T
        // factorisation; the step here is a partial-pivot LU, whose index of the zero pivot is a different
        // number for the same verdict: the reference's sentence without a number it would not print, and
        // this library's index marked as such.
        std::ostringstream oss;
        oss << "Linear solve failed. The factorization has been completed, but the "
            << "block diagonal matrix D is exactly singular"
            << ", so the solution could not be computed. [emme_amd: partial-pivot LU, zero pivot in column " << info << "]";
        return oss.str();
    }
    if (info < 0) {
        // Failures the reference does not have a code for.  It would carry a non-finite integral
        // into M, where zsysv fails (the message above), or into omega and end with a NaN eigenvalue;
        // either way the scan records {"eigenvalue":"NaN","reason":...} (src/main.cpp:311-318) and does NOT
        // continue the next scan point from this omega.  Same here.
        return info == EMME_ENUMERIC
                   ? "Linear solve failed. The matrix holds a non-finite integral, or the quadrature depth cap was reached "
                     "(EMME_ENUMERIC), so the solution could not be computed."
                   : "Linear solve failed on the device (EMME_EDEVICE).";
    }
    return std::string();
}

// M(omega_final) as the reference writes it (src/main.cpp:61-63); an empty path writes nothing
bool write_matrix_file(const std::string& path, const std::vector<cplx>& M) {
    if (path.empty()) return false;
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(M.data()), (std::streamsize)(sizeof(cplx) * M.size()));
    return (bool)f;
}

// the record of one solved point: eigenvalue, eigenvector, iterations
JsonValue point_record(const double root[2], const cplx* vec, int dim, int iters) {
    JsonValue res = JsonValue::make_object();
    JsonValue ev = JsonValue::make_array();
    ev.items.push_back(JsonValue::make(root[0]));
    ev.items.push_back(JsonValue::make(root[1]));
    res["eigenvalue"] = ev;
    JsonValue evec = JsonValue::make_array();
    for (int i = 0; i < dim; ++i) {
        JsonValue pr = JsonValue::make_array();
        pr.items.push_back(JsonValue::make(vec[i].real()));
        pr.items.push_back(JsonValue::make(vec[i].imag()));
        evec.items.push_back(pr);
    }
    res["eigenvector"] = evec;
    res["iterations"] = JsonValue::make(iters);
    return res;
}

JsonValue nan_record(const std::string& reason) {
    JsonValue err = JsonValue::make_object();
    err["eigenvalue"] = JsonValue::make(std::string("NaN"));
    err["reason"] = JsonValue::make(reason);
    return err;
}

// solve_once_eigen on an input object whose scan keys have been replaced by scalars
JsonValue solve_once(const JsonValue& input, cplx& omega, const std::string& matrix_path, bool& file_ok) {
    emme_params_t p;
    if (emme::params_from_value(input, &p) != EMME_OK) throw std::runtime_error(emme_last_error());
    emme_ctx_t* ctx = nullptr;
    if (emme_ctx_create(&p, -1, &ctx) != EMME_OK) throw std::runtime_error(emme_last_error());
    struct Guard {
        emme_ctx_t* c;
        ~Guard() { emme_ctx_destroy(c); }
    } guard{ctx};
    const double g[2] = {omega.real(), omega.imag()};
    double root[2];
    int iters = 0, info = 0;
    if (emme_solve_roots(ctx, g, 1, p.iteration_precision, p.iteration_step_limit, root, &iters, &info,
                         nullptr) != EMME_OK)
        throw std::runtime_error(emme_last_error());
    if (info != 0) throw std::runtime_error(search_failure_text(info));
    const int dim = emme_ctx_dim(ctx);
    std::vector<cplx> M((size_t)dim * dim), vec(dim);
    if (emme_ctx_get_matrix(ctx, 0, reinterpret_cast<double*>(M.data())) != EMME_OK)
        throw std::runtime_error(emme_last_error());
    file_ok = write_matrix_file(matrix_path, M);
    // nullSpace (include/solver.h:58-112, src/main.cpp:73-76) on the device, from M(omega_final) as the search left it
    int vinfo = 0;
    if (emme_null_vectors_batch(ctx, dim, 1, nullptr, reinterpret_cast<double*>(vec.data()), &vinfo) != EMME_OK)
        throw std::runtime_error(emme_last_error());
    JsonValue res = point_record(root, vec.data(), dim, iters);
    omega = cplx(root[0], root[1]);  // continuation, src/main.cpp:78
    return res;
}

// ---- the lock-step scan driver -------------------------------------------------------------
// One axis that cannot ride along (ScanAxis::sequential), point after point through solve_once -- a context per
// point, as the sequential driver walks it (src/main.cpp:264-324; emme_run_json's axis loop, which stays as it is).
JsonValue sequential_unit(const JsonValue& all, const emme::ScanAxis& ax, const cplx guess0, const std::string& dir) {
    JsonValue input = filter_input(all);
    ScanGen gen(ax.head, ax.step, ax.t0, ax.t1);
    bool cont, turning;
    double value;
    gen.next(cont, turning, value);
    JsonValue values = JsonValue::make_array(), arr = JsonValue::make_array();
    cplx omega = guess0;
    while (cont) {
        input[ax.key] = ax.head_is_int ? JsonValue::make((int)value) : JsonValue::make(value);
        values.items.push_back(JsonValue::make(value));
        if (turning) {  // second direction restarts from the head's root (:282-291)
            const JsonValue& first = arr.items.at(0).at("eigenvalue");
            omega = first.is_string() ? guess0 : cplx(first.at((size_t)0).number(), first.at((size_t)1).number());
        }
        const std::string fname = dir.empty() ? "" : dir + "/" + ax.key + "Eq" + std::to_string(value) + ".bin";
        try {
            bool ok = false;
            JsonValue one = solve_once(input, omega, fname, ok);
            one["eigenMatrix"] = JsonValue::make(ok ? fname : "Can not open '" + fname + "' for write.");
            one["scan_value"] = JsonValue::make(value);
            arr.items.push_back(one);
        } catch (const std::exception& e) {
            arr.items.push_back(nan_record(e.what()));
        }
        gen.next(cont, turning, value);
    }
    JsonValue unit = JsonValue::make_object();
    unit["scan_key"] = JsonValue::make(ax.key);
    unit["scan_values"] = values;
    unit["scan_result"] = arr;
    return unit;
}

// The axes that ride along, round by round on ONE context: the points of a round become the parameter sets bound to
// it, one emme_solve_roots_sets call finds their roots side by side, one emme_null_vectors_batch their vectors.
// units[a] receives the unit of riding axis a.  Throws (before any record exists) if the context cannot be made: the
// caller then falls back to the sequential driver, whose records carry the reason point by point.
void lockstep_units(const JsonValue& all, const emme::ScanPlan& plan, const cplx guess0, const std::string& dir,
                    std::vector<JsonValue>& units) {
    const JsonValue base = filter_input(all);
    emme_params_t p0;
    if (emme::params_from_value(base, &p0) != EMME_OK) throw std::runtime_error(emme_last_error());
    emme_ctx_t* ctx = nullptr;
    if (emme_ctx_create(&p0, -1, &ctx) != EMME_OK) throw std::runtime_error(emme_last_error());
    struct Guard {
        emme_ctx_t* c;
        ~Guard() { emme_ctx_destroy(c); }
    } guard{ctx};
    const int dim = emme_ctx_dim(ctx);
    const size_t naxes = plan.axes.size();
    std::vector<std::vector<JsonValue>> records(naxes);
    std::vector<JsonValue> values(naxes, JsonValue::make_array());
    // per line: the omega its next point continues from (solve_once's `omega`); per axis: the head's root, if any
    std::vector<cplx> cont0(naxes, guess0), cont1(naxes, guess0), head_root(naxes, guess0);
    for (const emme::ScanPoint& pt : plan.points)
        if (pt.round >= 0) {
            records[pt.axis].resize(records[pt.axis].size() + 1);
            values[pt.axis].items.push_back(JsonValue::make(pt.value));
        }
    struct Item {
        const emme::ScanPoint* pt;
        std::string fname;
    };
    for (int t = 0; t < plan.nrounds; ++t) {
        std::vector<Item> items;
        std::vector<emme_params_t> sets;
        std::vector<double> guesses;
        for (const emme::ScanPoint& pt : plan.points) {
            if (pt.round != t) continue;
            const emme::ScanAxis& ax = plan.axes[pt.axis];
            if (pt.line == 1 && pt.pred == 0) cont1[pt.axis] = head_root[pt.axis];  // src/main.cpp:282-291
            JsonValue input = base;
            input[ax.key] = ax.head_is_int ? JsonValue::make((int)pt.value) : JsonValue::make(pt.value);
            emme_params_t p;
            if (emme::params_from_value(input, &p) != EMME_OK) {
                records[pt.axis][pt.index] = nan_record(emme_last_error());
                continue;
            }
            const cplx g = pt.line == 1 ? cont1[pt.axis] : cont0[pt.axis];
            items.push_back({&pt, dir.empty() ? "" : dir + "/" + ax.key + "Eq" + std::to_string(pt.value) + ".bin"});
            sets.push_back(p);
            guesses.push_back(g.real()), guesses.push_back(g.imag());
        }
        const int n = (int)items.size();
        if (n == 0) continue;
        std::vector<int> set(n), iters(n, 0), info(n, 0), vinfo(n, 0);
        for (int b = 0; b < n; ++b) set[b] = b;
        std::vector<double> roots(2 * (size_t)n);
        std::vector<cplx> vecs((size_t)n * dim), M((size_t)dim * dim);
        std::string failed;  // a failure of the whole call: every point of the round records it, as solve_once would
        if (emme_ctx_bind_param_sets(ctx, sets.data(), n) != EMME_OK ||
            emme_solve_roots_sets(ctx, set.data(), guesses.data(), n, 0, p0.iteration_precision, p0.iteration_step_limit,
                                  roots.data(), iters.data(), info.data(), nullptr) != EMME_OK)
            failed = emme_last_error();
        bool any_ok = false;
        for (int b = 0; b < n; ++b) any_ok |= info[b] == 0;
        std::string vec_failed;
        if (failed.empty() && any_ok &&
            emme_null_vectors_batch(ctx, dim, n, nullptr, reinterpret_cast<double*>(vecs.data()), vinfo.data()) != EMME_OK)
            vec_failed = emme_last_error();
        for (int b = 0; b < n; ++b) {
            const emme::ScanPoint& pt = *items[b].pt;
            JsonValue& rec = records[pt.axis][pt.index];
            if (!failed.empty() || info[b] != 0) {
                rec = nan_record(failed.empty() ? search_failure_text(info[b]) : failed);
                continue;
            }
            if (emme_ctx_get_matrix(ctx, b, reinterpret_cast<double*>(M.data())) != EMME_OK) {
                rec = nan_record(emme_last_error());
                continue;
            }
            const bool ok = write_matrix_file(items[b].fname, M);
            if (!vec_failed.empty()) {
                rec = nan_record(vec_failed);
                continue;
            }
            rec = point_record(&roots[2 * (size_t)b], vecs.data() + (size_t)b * dim, dim, iters[b]);
            rec["eigenMatrix"] = JsonValue::make(ok ? items[b].fname : "Can not open '" + items[b].fname + "' for write.");
            rec["scan_value"] = JsonValue::make(pt.value);
            const cplx w(roots[2 * (size_t)b], roots[2 * (size_t)b + 1]);  // continuation, src/main.cpp:78
            (pt.line == 1 ? cont1 : cont0)[pt.axis] = w;
            if (pt.index == 0) head_root[pt.axis] = w;
        }
    }
    for (size_t a = 0; a < naxes; ++a) {
        if (plan.axes[a].sequential) continue;
        JsonValue unit = JsonValue::make_object();
        unit["scan_key"] = JsonValue::make(plan.axes[a].key);
        JsonValue arr = JsonValue::make_array();
        arr.items = records[a];
        unit["scan_values"] = values[a];
        unit["scan_result"] = arr;
        units[a] = unit;
    }
}

}  // namespace

extern "C" {

int emme_null_vector(const double* M, int n, double* vec) {
    if (!M || !vec || n < 1) return EMME_EINVAL;
    null_vector_of(reinterpret_cast<const cplx*>(M), n, reinterpret_cast<cplx*>(vec));
    return EMME_OK;
}

void emme_free(void* p) { std::free(p); }

int emme_scan_values(double head, double step, double tail0, double tail1, double* values,
                     int* turning_flags, int max_values) {
    // the value sequence the scan loop of src/main.cpp:264-324 visits for one axis
    ScanGen gen(head, step, tail0, tail1);
    bool cont, turning;
    double v;
    int n = 0;
    gen.next(cont, turning, v);
    while (cont && n < max_values) {
        if (values) values[n] = v;
        if (turning_flags) turning_flags[n] = turning ? 1 : 0;
        ++n;
        gen.next(cont, turning, v);
    }
    return n;
}

int emme_run_json(const char* input_text, const char* matrix_dir, char** output_text) {
    if (!input_text || !output_text) return EMME_EINVAL;
    *output_text = nullptr;
    try {
        const JsonValue all = emme::json_parse(input_text, "input.json");
        const std::string method = all.at("method").str();
        if (method != "eigen") {
            std::ostringstream oss;
            oss << "Method '" << method << "' is not supported, yet.\n";  // src/main.cpp:193-196
            throw std::runtime_error(oss.str());
        }
        const JsonValue& guess = all.at("initial_guess");
        const cplx guess0(guess.at((size_t)0).number(), guess.at((size_t)1).number());
        const std::string dir = matrix_dir ? std::string(matrix_dir) : std::string();

        JsonValue result = JsonValue::make_object();
        result["input"] = all;
        result["run_time"] = JsonValue::make(date_string());
        JsonValue results = JsonValue::make_object();

        // scan axes: every top-level key whose value is an object (src/main.cpp:225-242)
        struct Axis {
            std::string key;
            double head, step, t0, t1;
            bool head_is_int;
        };
        std::vector<Axis> axes;
        for (const auto& m : all.members) {
            if (!m.second.is_object()) continue;
            Axis a;
            a.key = m.first;
            a.head = m.second.at("head").number();
            a.head_is_int = m.second.at("head").kind == JsonValue::Int;
            a.step = m.second.at("step").number();
            const JsonValue& tail = m.second.at("tail");
            if (tail.is_array()) {
                a.t0 = tail.at((size_t)0).number();
                a.t1 = tail.at((size_t)1).number();
            } else {
                a.t0 = tail.number();
                a.t1 = a.head + .5 * std::copysign(a.step, a.head - a.t0);
            }
            axes.push_back(a);
        }

        if (axes.empty()) {
            JsonValue unit = JsonValue::make_object();
            unit["scan_key"] = JsonValue::make(std::string("(None)"));
            JsonValue arr = JsonValue::make_array();
            cplx omega = guess0;
            bool ok = false;
            arr.items.push_back(solve_once(all, omega, dir.empty() ? "" : dir + "/eigenMatrix.bin", ok));
            unit["scan_result"] = arr;
            results["(None)"] = unit;
        } else {
            for (const Axis& ax : axes) {
                JsonValue input = filter_input(all);
                ScanGen gen(ax.head, ax.step, ax.t0, ax.t1);
                bool cont, turning;
                double value;
                gen.next(cont, turning, value);
                JsonValue unit = JsonValue::make_object();
                unit["scan_key"] = JsonValue::make(ax.key);
                JsonValue values = JsonValue::make_array();
                JsonValue arr = JsonValue::make_array();
                cplx omega = guess0;
                while (cont) {
                    // Value::operator=(double) keeps the category of the head value: an
                    // INTEGER head truncates every scan value (include/JsonParser.h:176-186)
                    input[ax.key] = ax.head_is_int ? JsonValue::make((int)value) : JsonValue::make(value);
                    values.items.push_back(JsonValue::make(value));
                    if (turning) {  // second direction restarts from the head's root (:282-291)
                        const JsonValue& first = arr.items.at(0).at("eigenvalue");
                        if (first.is_string())
                            omega = guess0;
                        else
                            omega = cplx(first.at((size_t)0).number(), first.at((size_t)1).number());
                    }
                    const std::string fname =
                        dir.empty() ? "" : dir + "/" + ax.key + "Eq" + std::to_string(value) + ".bin";
                    try {
                        bool ok = false;
                        JsonValue one = solve_once(input, omega, fname, ok);
                        one["eigenMatrix"] = JsonValue::make(ok ? fname : "Can not open '" + fname + "' for write.");
                        one["scan_value"] = JsonValue::make(value);
                        arr.items.push_back(one);
                    } catch (const std::exception& e) {
                        JsonValue err = JsonValue::make_object();
                        err["eigenvalue"] = JsonValue::make(std::string("NaN"));
                        err["reason"] = JsonValue::make(std::string(e.what()));
                        arr.items.push_back(err);
                    }
                    gen.next(cont, turning, value);
                }
                unit["scan_values"] = values;
                unit["scan_result"] = arr;
                results[ax.key] = unit;
            }
        }
        result["result"] = results;
        const std::string text = result.dump(0);
        *output_text = static_cast<char*>(std::malloc(text.size() + 1));
        if (!*output_text) return EMME_ENOMEM;
        std::memcpy(*output_text, text.c_str(), text.size() + 1);
        return EMME_OK;
    } catch (const std::exception& e) {
        emme::set_error(e.what());
        return EMME_EJSON;
    }
}

int emme_run_json_lockstep(const char* input_text, const char* matrix_dir, char** output_text) {
    if (!input_text || !output_text) return EMME_EINVAL;
    *output_text = nullptr;
    try {
        const JsonValue all = emme::json_parse(input_text, "input.json");
        const emme::ScanPlan plan = emme::make_scan_plan(all);
        // nothing to put side by side (no axis, or none that rides along), an input the sequential driver refuses, or
        // no context for the rounds: the sequential driver, whose output says why point by point
        if (plan.nrounds == 0 || all.at("method").str() != "eigen") return emme_run_json(input_text, matrix_dir, output_text);
        const JsonValue& guess = all.at("initial_guess");
        const cplx guess0(guess.at((size_t)0).number(), guess.at((size_t)1).number());
        std::vector<JsonValue> units(plan.axes.size());
        const std::string dir = matrix_dir ? std::string(matrix_dir) : std::string();
        try {
            lockstep_units(all, plan, guess0, dir, units);
        } catch (const std::exception&) {
            return emme_run_json(input_text, matrix_dir, output_text);
        }
        JsonValue result = JsonValue::make_object();
        result["input"] = all;
        result["run_time"] = JsonValue::make(date_string());
        JsonValue results = JsonValue::make_object();
        for (size_t a = 0; a < plan.axes.size(); ++a)
            results[plan.axes[a].key] =
                plan.axes[a].sequential ? sequential_unit(all, plan.axes[a], guess0, dir) : units[a];
        result["result"] = results;
        const std::string text = result.dump(0);
        *output_text = static_cast<char*>(std::malloc(text.size() + 1));
        if (!*output_text) return EMME_ENOMEM;
        std::memcpy(*output_text, text.c_str(), text.size() + 1);
        return EMME_OK;
    } catch (const std::exception& e) {
        emme::set_error(e.what());
        return EMME_EJSON;
    }
}

}  // extern "C"
