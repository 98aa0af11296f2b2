// Stand-alone driver of figh_chain_host_tail for AddressSanitizer / UBSan runs of the tail unit ON THE CPU (no device, no
// Python): the shapes of tests/test_host_tail_native.py, every output array allocated at exactly the documented size so that
// an index past it is caught.  Build and run, from the repository root:
//   hipcc -O1 -g -std=c++17 -Iinclude -Ifigaroh_plus_amd/csrc -Xarch_host -fsanitize=address,undefined
//         -Xarch_host -fno-sanitize-recover=undefined --offload-arch=gfx950 tools/host_tail_sanitize.cpp
//         figaroh_plus_amd/csrc/figh_host_tail.hip -o build/host_tail_sanitize && build/host_tail_sanitize   (mkdir -p build first: it is git-ignored)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "figh.h"

namespace figh {
void set_error(const std::string &msg) { std::fprintf(stderr, "libfigh: %s\n", msg.c_str()); }
}  // namespace figh

static int failures = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

struct Case {
    int n, with_tau;
    std::vector<int> dep;
    std::vector<double> rows;  // (nc + 1) x nc
    std::vector<int> base;
};

// rows_k of an upper-triangular regrouped factor with a well-conditioned R1 (diagonal 10 .. 20, entries of R2 = R1 times
// coefficients of three decimals) and a plain diagonal with 1e-13 at the dependent columns
static Case make_case(int n, std::vector<int> dep, int with_tau, unsigned seed) {
    std::mt19937 gen(seed);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    Case c{n, with_tau, dep, {}, {}};
    const int nc = n + with_tau;
    c.rows.assign((size_t)(nc + 1) * nc, 0.0);
    std::vector<char> is_dep(n, 0);
    for (int d : dep) is_dep[d] = 1;
    for (int k = 0; k < n; ++k)
        if (!is_dep[k]) c.base.push_back(k);
    const int r = (int)c.base.size();
    std::vector<double> R1((size_t)r * r, 0.0);
    for (int a = 0; a < r; ++a)
        for (int b = a; b < r; ++b) R1[(size_t)a * r + b] = a == b ? 15.0 + 5.0 * u(gen) : u(gen);
    for (int a = 0; a < r; ++a) {
        double *row = &c.rows[(size_t)c.base[a] * nc];
        for (int b = 0; b < r; ++b) row[c.base[b]] = b >= a ? R1[(size_t)a * r + b] : 1e-15 * u(gen);  // residues below
        if (with_tau) row[n] = 30.0 * u(gen);
    }
    for (int d : dep) {
        std::vector<double> coef(r, 0.0);
        for (int b = 0; b < r; ++b)
            if (c.base[b] < d && d - c.base[b] <= 4) coef[b] = std::round(2000.0 * u(gen)) / 1000.0;
        for (int a = 0; a < r; ++a) {
            double s = 0.0;
            for (int b = a; b < r; ++b) s += R1[(size_t)a * r + b] * coef[b];
            c.rows[(size_t)c.base[a] * nc + d] = s;
        }
    }
    if (with_tau) c.rows[(size_t)n * nc + n] = 0.7;
    for (int k = 0; k < n; ++k) c.rows[(size_t)nc * nc + k] = is_dep[k] ? 1e-13 : 12.0 + k;
    if (with_tau) c.rows[(size_t)nc * nc + n] = 0.7;
    return c;
}

struct Out {
    std::vector<int32_t> idx, cached;
    std::vector<double> absdiag, beta, phi_ls, phi_b, bounds;
    figh_host_tail_t t;
};

static int run(const Case &c, Out &o, double tol, int64_t total_rows, int null_rule, bool keep_cache = false) {
    const int n = c.n, r = (int)c.base.size(), d = n - r;
    // exact sizes: beta r x d, phi r, idx n, bounds n + 2 (at least one element each, so that the pointers are valid)
    o.idx.assign(n, -1);
    o.absdiag.assign(n, 0.0);
    o.beta.assign((size_t)std::max(1, r * d), 0.0);
    o.phi_ls.assign(std::max(1, r), 0.0);
    o.phi_b.assign(std::max(1, r), 0.0);
    if (!keep_cache) {
        o.bounds.assign(n + 2, 0.0);
        o.cached.assign(n, 0);
    }
    figh_host_tail_t &t = o.t;
    t.rows_k = c.rows.data();
    t.n = n;
    t.with_tau = c.with_tau;
    t.tol_qr = tol;
    t.total_rows = total_rows;
    t.pieces = 1;
    t.null_rule = null_rule;
    if (!keep_cache) t.n_cached_base = -1;
    t.cached_base = o.cached.data();
    t.bounds = o.bounds.data();
    t.idx = o.idx.data();
    t.absdiag = o.absdiag.data();
    t.beta = o.beta.data();
    t.phi_ls = o.phi_ls.data();
    t.phi_b = o.phi_b.data();
    return figh_chain_host_tail(&t);
}

// R1 beta = R2 and R1 phi = z up to the rounding to six decimals
static void check_solution(const Case &c, const Out &o) {
    const int n = c.n, nc = n + c.with_tau, r = o.t.n_base, d = n - r;
    for (int a = 0; a < r; ++a) {
        const double *row = &c.rows[(size_t)o.idx[a] * nc];
        double rowsum = 0.0;
        for (int b = a; b < r; ++b) rowsum += std::fabs(row[o.idx[b]]);
        for (int j = 0; j < d; ++j) {
            double s = 0.0;
            for (int b = a; b < r; ++b) s += row[o.idx[b]] * o.beta[(size_t)b * d + j];
            EXPECT(std::fabs(s - row[o.idx[r + j]]) <= 0.5e-6 * rowsum + 1e-9);
        }
        if (c.with_tau) {
            double s = 0.0;
            for (int b = a; b < r; ++b) s += row[o.idx[b]] * o.phi_ls[b];
            EXPECT(std::fabs(s - row[n]) <= 1e-10 * (1.0 + std::fabs(row[n])));
            EXPECT(std::fabs(o.phi_b[a] - o.phi_ls[a]) <= 0.5e-6 + 1e-12);
        }
    }
}

int main() {
    const double tol = 1e-8;
    struct Shape {
        const char *name;
        int n, with_tau;
        std::vector<int> dep;
    };
    const std::vector<Shape> shapes = {
        {"n = 1 without tau", 1, 0, {}},
        {"n = 3 with tau", 3, 1, {1}},
        {"no dependent column", 5, 1, {}},
        {"one base column, the rest dependent", 4, 1, {1, 2, 3}},
        {"UR10's shape (49 + tau, 36 base)", 49, 1, {6, 9, 13, 16, 20, 23, 27, 30, 34, 37, 41, 44, 47}},
        {"80 columns with tau", 80, 1, {79}},
    };
    unsigned seed = 1;
    for (const Shape &s : shapes) {
        std::printf("%s\n", s.name);
        Case c = make_case(s.n, s.dep, s.with_tau, seed++);
        Out o;
        EXPECT(run(c, o, tol, 240, 1) == FIGH_OK);
        EXPECT(o.t.status == FIGH_TAIL_OK && o.t.n_base == (int)c.base.size() && o.t.bounds_recomputed == 1);
        EXPECT(o.t.certified == 1);
        for (size_t k = 0; k < c.base.size(); ++k) EXPECT(o.idx[k] == c.base[k]);
        check_solution(c, o);
        // the cached bounds handed back
        for (int k = 0; k < o.t.n_base; ++k) o.cached[k] = o.idx[k];
        o.t.n_cached_base = o.t.n_base;
        EXPECT(run(c, o, tol, 240, 1, true) == FIGH_OK && o.t.bounds_recomputed == 0 && o.t.certified == 1);
        EXPECT(run(c, o, tol, 240, 0) == FIGH_OK && o.t.certified == 0);
    }
    {
        std::printf("a zero and a NaN pivot, dependent pivots around tol / 8, a base pivot around the sqrt(T) margin\n");
        Case c = make_case(6, {2, 4}, 1, 40);
        const size_t diag = (size_t)7 * 7;
        Out o;
        c.rows[diag + 2] = 0.0;
        EXPECT(run(c, o, tol, 240, 1) == FIGH_OK && o.t.n_base == 4 && o.t.certified == 1);
        c.rows[diag + 4] = std::nan("");
        EXPECT(run(c, o, tol, 240, 1) == FIGH_OK && o.t.n_base == 4 && o.t.certified == 0 && std::isnan(o.absdiag[4]));
        check_solution(c, o);
        c.rows[diag + 4] = tol / 8.0 * (1.0 + 1e-9);
        EXPECT(run(c, o, tol, 240, 1) == FIGH_OK && o.t.certified == 0);
        c.rows[diag + 4] = tol / 8.0 * (1.0 - 1e-9);
        EXPECT(run(c, o, tol, 240, 1) == FIGH_OK && o.t.certified == 1);
        const double margin = (1.0 + o.bounds[3]) * (2.0 * tol / 64.0) * std::sqrt(4000000.0 / 32.0 + 1.0);
        c.rows[diag + 5] = tol + margin * (1.0 - 1e-6);
        EXPECT(run(c, o, tol, 4000000, 1) == FIGH_OK && o.t.n_base == 4 && o.t.certified == 0);
        c.rows[diag + 5] = tol + margin * (1.0 + 1e-6);
        EXPECT(run(c, o, tol, 4000000, 1) == FIGH_OK && o.t.n_base == 4 && o.t.certified == 1);
    }
    {
        std::printf("a singular R1, bad arguments\n");
        Case c = make_case(5, {3}, 1, 41);
        c.rows[(size_t)1 * 6 + 1] = 0.0;
        Out o;
        EXPECT(run(c, o, tol, 240, 1) == FIGH_OK && o.t.status == FIGH_TAIL_SINGULAR && o.t.certified == 0);
        EXPECT(o.bounds[5 + 1] == 0.0);
        o.t.n = 81;
        EXPECT(figh_chain_host_tail(&o.t) == FIGH_ERR_INVALID);
        EXPECT(figh_chain_host_tail(nullptr) == FIGH_ERR_INVALID);
    }
    std::printf(failures ? "%d check(s) FAILED\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
