// The parts of the exact certificate (certify.hip) that do not care where the p-adic digits came from: the integer scaling of an
// LP, the row-scaled integer basis, the assembly of the digits with the combined-unknown rational reconstruction and the exact
// substitution, the sign checks with the reduced costs of all non-basic columns, and the exact objective.  `certify_basis` (one
// LP, a chain of launches) and the batched certificate of relp_many (many_certify.hip: one launch for all LPs) call the same
// functions; what differs between them is only who produced the digits.
#pragma once
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "bigint.hpp"
#include "certify.hpp"
#include "device_columns.hpp"

namespace relp {

// v mod p for v < 2^64; p = 2^31 - 1 (the first trial prime) folds instead of dividing
__device__ __forceinline__ uint32_t reduce64(uint64_t v, uint32_t p) {
    if (p == 0x7fffffffu) {
        v = (v & 0x7fffffffu) + (v >> 31);   // < 2^34
        v = (v & 0x7fffffffu) + (v >> 31);   // < 2^31 + 8
        uint32_t r = (uint32_t)v;
        return r >= p ? r - p : r;
    }
    return (uint32_t)(v % p);
}

// the trial primes of the modular inverse, in the order they are tried
constexpr uint32_t CERTIFY_PRIMES[4] = {2147483647u, 2147483629u, 2147483587u, 2147483579u};

// diagnostic timeline (RELP_TIME_CERTIFY=1): where the certificate's wall time goes
struct CertifyTimes {
    double device_digits = 0.0, host_assemble = 0.0, inverse = 0.0, setup = 0.0, checks = 0.0, reconstruct = 0.0, parallel = 0.0;
    double unpack = 0.0, horner = 0.0, combine = 0.0, numerators = 0.0, verify = 0.0, normalise = 0.0;  // parts of host_assemble
    int digit_launches = 0, solves = 0, reconstructs = 0;
};

struct IntegerBasis {          // row-scaled integer basis, both orientations
    int m = 0;
    std::vector<int> col_start, row_index;   // CSC (columns = basis positions)
    std::vector<long long> value;
    std::vector<int> row_start, col_index;   // CSR
    std::vector<long long> row_value;
};

struct ExactVector {           // numer[i] / denom
    std::vector<BigInt> numer;
    BigInt denom = BigInt(1);
};

// The exact vectors a certificate proved its verdict with (declared in certify.hpp), in the terms of the caller's LP.  Big integers
// over one denominator per vector; the "num/den" texts are made on demand (exact_witness_values).  A certificate only KEEPS what
// the witnesses are made of -- most results are never asked for theirs: the row and cost multipliers of the integer scaling are
// folded into y by the first exact_witness_values (under `finish_guard`: accessors may come from several threads), and x is
// shared with the kept exact primal solution where there is one, not copied.
struct ExactWitnesses {
    int mode = 0;               // as certify_basis: 0 FINITE_OPTIMUM, 1 INFEASIBLE, 2 UNBOUNDED; 3: a lower bound of the dual simplex
                                // (certify_dual_bound: y alone, finished, no x and no ray)
    std::vector<int> basis;     // the basis that was finally proved: provider column per row (-1-k: artificial k)
    int entering = -1;          // mode 2: the provider column q of the ray
    ExactVector x;              // x_B[k] = x.numer[k] / x.denom ...
    std::shared_ptr<const ExactPrimal> shared_x;  // ... unless this is set: then x is the kept primal solution's (same basis, same values)
    mutable ExactVector y;      // once finished: y_i = y.numer[i] / y.denom per row: the dual solution (mode 1: the Farkas vector)
    ExactVector alpha;          // mode 2: alpha = B^-1 a_q, d_{basis[k]} = -alpha_k
    mutable std::mutex finish_guard;
    mutable bool finished = false;      // false: y is still the solution of the scaled system, and these wait to be folded in:
    std::vector<i128> row_mult;
    i128 cost_mult = 1;
};

// What depends on the loaded LP only (kept by the handle between certificates, CertifyScratch::statics).
struct CertifyStatic {
    std::vector<SparseColumn> columns;
    std::vector<Rat> rhs;
    std::vector<i128> row_mult;
    i128 cost_mult = 1;        // 0: the cost scaling overflows 128 bits (only the phase-one certificate can do without)
    DeviceColumns cols;
    std::vector<BigInt> rhs_big;
    BigInt rhs_den = BigInt(1);
};

// Integer scaling of the LP: row multipliers (lcm of the denominators of the row's coefficients), cost multiplier, and the
// right-hand side over its own common denominator.  Null with `message` set when the row scaling overflows 128 bits.
std::shared_ptr<const CertifyStatic> certify_static(const StandardForm& form, std::string* message);

// The basis in integers: B (CSC and CSR), the scaled basic costs (`mode` 1: the phase-one costs) and the membership flags of the
// provider columns.  An artificial column -1-k is the unit column of its row scaled by the row multiplier.  False with `message`
// set when an entry does not fit 62 bits.  `rows` >= 0: the first `rows` rows of the LP only, with a basis of that many columns (the
// constraint rows of an LP held on implicit bounds: a bounded column loses its entry on its bound row).
bool certify_integer_basis(const CertifyStatic& statics, const MatrixData& md, const std::vector<int>& basis, int mode, IntegerBasis* B,
                           std::vector<long long>* cost_basis, std::vector<char>* in_basis, std::string* message, int rows = -1);

// From the first digits.size() p-adic digits of the solution of A z = rhs (transpose 0: A = B, 1: A = B'): the numerators over one
// common denominator (one rational reconstruction of a random integer combination of the unknowns, then one per entry that
// brings a factor the combination lost), VERIFIED by exact substitution A numer == denom rhs.  False when the digits do not
// suffice (or are wrong).  `parallel`: the entries are spread over the certificate's worker pool; else they run on the caller.
bool dixon_reconstruct(const IntegerBasis& B, const std::vector<long long>& rhs, int transpose, uint32_t p,
                       const std::vector<const uint32_t*>& digits, bool parallel, ExactVector* out, CertifyTimes& times);

// Sign checks of a basis with exact x_B = x.numer / x.denom (denom > 0) and y: the most negative basic value and, from the
// reduced costs of ALL non-basic columns (`dhat`, over one positive denominator), the most negative of those; -1 where there is
// none.  False with `message` set when an artificial variable is positive (modes 0 and 2).
struct CertifySigns {
    int worst_row = -1, worst_col = -1;
    std::vector<BigInt> dhat;
};
bool certify_signs(const CertifyStatic& statics, const MatrixData& md, const std::vector<int>& basis, const std::vector<char>& in_basis,
                   int mode, const ExactVector& x, const ExactVector& y, bool parallel, CertifySigns* signs, std::string* message);

// objective = (sum_k cost_basis[k] X_k) / (cost_mult * Dx) + fixed cost, reduced, as "num/den"
std::string certify_objective(const StandardForm& form, const CertifyStatic& statics, const std::vector<long long>& cost_basis,
                              const ExactVector& x);

// ---- the final checks of the two other verdicts (after certify_signs with the same `mode`) -------------------------------------
// Mode 1, INFEASIBLE: the final phase-one basis is optimal (no negative x_B, no negative reduced cost under the phase-one costs) and
// its optimum, the sum of the basic artificial variables, is positive.  *objective: that optimum, reduced, as "num/den".
bool certify_infeasible(const CertifySigns& signs, const std::vector<long long>& cost_basis, const ExactVector& x, std::string* objective,
                        std::string* message);
// Mode 2, UNBOUNDED, before the ray is solved for: x_B >= 0 and the provider column `entering` is non-basic with cbar_q < 0.
bool certify_unbounded_entering(const CertifySigns& signs, const std::vector<char>& in_basis, int entering, std::string* message);
// Provider column j scaled by the row multipliers, dense (the right-hand side of B alpha = a_q).  False with `message` set when an
// entry does not fit 62 bits.
bool certify_scaled_column(const CertifyStatic& statics, int j, std::vector<long long>* out, std::string* message);
// Mode 2, the ray: alpha = B^-1 a_q <= 0, and exactly zero on a row whose basic variable is an artificial.  *objective: "-inf".
bool certify_unbounded_ray(const std::vector<int>& basis, const ExactVector& alpha, std::string* objective, std::string* message);

// ---- what a proved certificate hands out ----------------------------------------------------------------------------------------
// `x` as the checks saw it (x.denom holds rhs_den already); `y` is the solution of the SCALED system (diag(r) B)' y^ = mu c_B with the
// row multipliers r and the cost multiplier mu (mode 1: the phase-one costs, mu = 1), so the dual solution of the caller's LP is
// y_i = r_i y^_i / mu: B' (r . y^) = mu c_B.  x and alpha do not see the row scaling.  The vectors are moved from.
// `shared_x` (may be null): the kept exact primal solution of the same basis; x is then taken from there (and may have been moved from).
std::shared_ptr<const ExactWitnesses> make_exact_witnesses(const CertifyStatic& statics, int mode, const std::vector<int>& basis, int entering,
                                                          ExactVector& x, ExactVector& y, ExactVector& alpha,
                                                          std::shared_ptr<const ExactPrimal> shared_x = nullptr);

}  // namespace relp
