// Host tail of a pass on the n x n numbers the device returns (n <= 80): the rank decision, R1^-1, the regrouping
// coefficients, the least-squares solution and the certificate of the null-pivot rule.  No device code and no HIP call
// lives here: figh_chain_host_tail runs on a machine without a GPU.
//
// The semantics are those of IdentificationPipeline._finish (its n <= 80 branch), _host.null_rule_bounds and
// _host.null_rule_certified, condition for condition; qrdecomposition.py:215-244 of the reference is what they mirror.
// Expression strings are not formed here (tools/qrdecomposition._expressions): native code never formats a float.
#include <cmath>
#include <cstring>

#include "figh_internal.h"

namespace figh {

static constexpr int kTailMax = 80;
static constexpr double kNullRuleFold = 64.0;  // the rule folds at most tol_qr / 64 of a column's norm (figh.h)

// np.around(x, 6): rint(x * 1e6) / 1e6 in the default rounding mode (round half to even)
static inline double round6(double x) { return std::nearbyint(x * 1e6) / 1e6; }

// _host.null_rule_triangles
static inline double tail_triangles(int64_t rows, int64_t pieces) {
    const int64_t t = (rows + 31) / 32 + (pieces > 1 ? pieces : 1);  // (-(-rows // 32): rows >= 0)
    return (double)(t > 1 ? t : 1);
}

int host_tail(figh_host_tail_t *t) {
    FIGH_REQUIRE(t && t->rows_k && t->idx && t->absdiag && t->beta && t->phi_ls && t->phi_b && t->bounds,
                 "figh_chain_host_tail: NULL pointer");
    const int n = t->n, with_tau = t->with_tau ? 1 : 0, nc = n + with_tau;
    FIGH_REQUIRE(n >= 1 && n <= kTailMax, "figh_chain_host_tail: 1 .. 80 columns");
    FIGH_REQUIRE(t->n_cached_base < 0 || t->cached_base, "figh_chain_host_tail: cached bounds without their base columns");
    const double *rows = t->rows_k, *diag = rows + (size_t)nc * nc;
    const double tol = t->tol_qr;
    // the rank decision on the plain diagonal (a NaN pivot compares false: not base)
    int base[kTailMax], rest[kTailMax], r = 0, d = 0;
    for (int k = 0; k < n; ++k) {
        const double a = std::fabs(diag[k]);
        t->absdiag[k] = a;
        if (a > tol) base[r++] = k;
        else rest[d++] = k;
    }
    for (int k = 0; k < r; ++k) t->idx[k] = base[k];
    for (int k = 0; k < d; ++k) t->idx[r + k] = rest[k];
    t->n_base = r;
    t->status = FIGH_TAIL_OK;
    t->certified = 0;
    t->bounds_recomputed = 0;
    t->residual_norm = with_tau ? std::fabs(rows[(size_t)n * nc + n]) : 0.0;

    // R1 (its upper triangle; below it the device leaves rounding residues) and [R2 | Q1^T tau], gathered once
    static thread_local double U[kTailMax * kTailMax], X[kTailMax * kTailMax], B[kTailMax * (kTailMax + 1)];
    const int nb = d + with_tau;  // right-hand sides: the dependent columns, then tau
    for (int a = 0; a < r; ++a) {
        const double *row = rows + (size_t)base[a] * nc;
        for (int b = a; b < r; ++b) U[a * kTailMax + b] = row[base[b]];
        for (int c = 0; c < d; ++c) B[a * (kTailMax + 1) + c] = row[rest[c]];
        if (with_tau) B[a * (kTailMax + 1) + d] = row[n];
    }
    auto R1 = [&](int a, int b) { return U[a * kTailMax + b]; };  // a <= b
    // X = R1^-1 by back substitution, column by column: X_jj = 1 / R_jj, X_ij = -(sum_{i < k <= j} R_ik X_kj) / R_ii
    bool singular = false, finite = true;
    for (int k = 0; k < r; ++k) singular = singular || R1(k, k) == 0.0;
    if (!singular) {
        for (int j = 0; j < r; ++j) {
            double *x = X + (size_t)j * kTailMax;  // column j of X, entries 0 .. j
            x[j] = 1.0 / R1(j, j);
            for (int i = j - 1; i >= 0; --i) {
                const double *u = U + i * kTailMax;
                double s = 0.0;
                for (int k = i + 1; k <= j; ++k) s += u[k] * x[k];
                x[i] = -s / u[i];
            }
            for (int i = 0; i <= j; ++i) finite = finite && std::isfinite(x[i]);
        }
    }
    auto Xe = [&](int i, int j) { return X[(size_t)j * kTailMax + i]; };  // i <= j
    // row i of R1^-1 [R2 | z]: sum over k >= i of X_ik B_k.
    auto product_row = [&](int i, double *out) {
        for (int c = 0; c < nb; ++c) out[c] = 0.0;
        for (int k = i; k < r; ++k) {
            const double x = Xe(i, k);
            const double *b = B + k * (kTailMax + 1);
            for (int c = 0; c < nb; ++c) out[c] += x * b[c];
        }
    };

    // the certificate's coefficient sums (_host.null_rule_bounds): kept while the base set stays the same
    double *A_base = t->bounds, *A_dep = t->bounds + r, *xnorm = t->bounds + n, *valid = t->bounds + n + 1;
    if (t->null_rule) {
        bool cached = t->n_cached_base == r;
        for (int k = 0; cached && k < r; ++k) cached = t->cached_base[k] == base[k];
        if (!cached) {
            t->bounds_recomputed = 1;
            if (singular || !finite) {
                *valid = 0.0;  // (None: the pass cannot be certified)
            } else {
                double rowsum[kTailMax];
                for (int i = 0; i < r; ++i) rowsum[i] = 0.0;
                for (int k = 0; k < r; ++k) {
                    double s = 0.0;
                    for (int i = 0; i < k; ++i) s += std::fabs(Xe(i, k));
                    A_base[k] = std::fabs(R1(k, k)) * s;
                    for (int i = 0; i <= k; ++i) rowsum[i] += std::fabs(Xe(i, k));
                }
                double xn = 0.0;
                for (int i = 0; i < r; ++i) xn = rowsum[i] > xn ? rowsum[i] : xn;
                double prod[kTailMax + 1];
                for (int c = 0; c < d; ++c) A_dep[c] = 0.0;
                for (int i = 0; i < r; ++i) {
                    product_row(i, prod);
                    for (int c = 0; c < d; ++c) A_dep[c] += std::fabs(prod[c]);
                }
                *xnorm = r ? xn : 0.0;
                *valid = 1.0;
            }
        }
    }
    if (singular) {
        t->status = FIGH_TAIL_SINGULAR;  // (np.linalg.LinAlgError in the caller, like LAPACK's info > 0)
        return FIGH_OK;
    }

    // beta = around(R1^-1 R2, 6), phi = R1^-1 Q1^T tau
    for (int i = 0; i < r; ++i) {
        double prod[kTailMax + 1];
        product_row(i, prod);
        for (int c = 0; c < d; ++c) t->beta[(size_t)i * d + c] = round6(prod[c]);
        if (with_tau) {
            t->phi_ls[i] = prod[d];
            t->phi_b[i] = round6(prod[d]);
        }
    }

    if (!t->null_rule) return FIGH_OK;
    // _host.null_rule_certified (safety = 2)
    if (*valid == 0.0) return FIGH_OK;
    const double fold = 2.0 * tol / kNullRuleFold;
    if (with_tau) {
        double sum = 0.0, mx = 0.0;
        for (int i = 0; i < r; ++i) {
            const double p = std::fabs(t->phi_ls[i]);
            if (!std::isfinite(p)) return FIGH_OK;
            sum += p;
            mx = p > mx ? p : mx;
        }
        if (*xnorm * (tol / kNullRuleFold) * sum > 1e-7 * (mx > 1.0 ? mx : 1.0)) return FIGH_OK;
    }
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(t->absdiag[k])) return FIGH_OK;
    for (int c = 0; c < d; ++c)
        if (t->absdiag[rest[c]] > tol / 8.0) return FIGH_OK;
    const double fold_base = fold * std::sqrt(tail_triangles(t->total_rows, t->pieces));
    for (int k = 0; k < r; ++k)
        if (!(t->absdiag[base[k]] - tol > (1.0 + A_base[k]) * fold_base)) return FIGH_OK;
    for (int c = 0; c < d; ++c)
        if (!(tol - t->absdiag[rest[c]] > (1.0 + A_dep[c]) * fold)) return FIGH_OK;
    t->certified = 1;
    return FIGH_OK;
}

}  // namespace figh

extern "C" int figh_chain_host_tail(figh_host_tail_t *t) { return figh::host_tail(t); }
