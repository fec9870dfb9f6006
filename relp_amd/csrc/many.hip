// Many small independent LPs in one launch, one workgroup per LP (relp_many_*, include/relp_amd.h).
//
// The `Solver` handle runs one LP as a device-wide pipeline (two or three kernels per pivot over the whole chip).  For an LP of a
// few dozen to a few hundred rows each pivot then costs the launch boundaries while nearly every CU is idle.  Here a workgroup owns
// one LP for its whole two-phase solve -- `solve_relaxation` of two_phase/mod.rs:25-109 with the loops of phase_one.rs:134-178 and
// phase_two.rs:36-58 -- inside ONE ordinary launch: no grid barrier, no cooperative launch, no communication between workgroups.
//
// Per LP the host builds what `Solver::load` builds (the same `StandardForm` / `MatrixData`, artificial columns first, then the
// provider columns; the reference's initial slack pivots, artificials on the other rows), so that bases, pivot counts and index
// spaces compare directly with a `Solver`'s.  Each step restates the single-LP f64 path (kernels.hip):
//   pricing + steepest-edge update   price_kernel          (pivot_rule.rs:190-296, tableau/mod.rs:106-112)
//   FTRAN, two-pass ratio test       pivot_fused_kernel    (tableau/mod.rs:126-130, 287-313; Harris or the textbook rule)
//   x_B, -pi, objective update       pivot_fused_kernel    (carry/mod.rs:295-349)
//   product-form inverse update      pivot_fused_kernel    (basis_inverse_rows.rs:36-70, 123-137)
//   -pi and gamma at a phase start   pi_kernel, gamma_init_kernel   (carry/mod.rs:499-525, pivot_rule.rs:202-219)
//   zero-level pivots                row_scan_kernel + a forced pivot (phase_one.rs:232-278)
// The explicit inverse is re-inverted from the basis columns by Gauss-Jordan with partial pivoting every `polish_period` pivots and
// before every verdict (the role of `BasisInverse::invert`, lower_upper/mod.rs:78-92).
//
// Two tiers of storage for B^-1 (f64, column-major, ld = m), one kernel source: `many_kernel<true, .>` keeps it in the workgroup's
// LDS, `many_kernel<false, .>` in a per-LP slab of global memory.  Everything else of the LP's state -- x_B, -pi, rho_p, w, alpha, the
// basis -- is in LDS in both.  Columns, costs, steepest-edge weights and column positions stay in global memory.
//
// Implicit upper bounds (`many_kernel<., true>`, relp_many_config.implicit_bounds): the device LP has the constraint rows only and
// the bounds of the structurals and the ranges of the range slacks are kept by the bounded-variable ratio test, as a `Solver` with
// relp_options.implicit_bounds does (kernels.hip, ftran_ratio_fast_kernel): complemented columns (`flipped`, pos -2) priced and
// entered with the opposite sign, rows with alpha_i < 0 leaving at the upper bound of their basic variable, bound flips of the
// entering variable, zero-width columns never priced (pos -3).  Two more vectors per LP in LDS: `xub` (the bound of the variable
// basic in row i) and the mutable right-hand side b' = b - sum over the complemented columns of u_j a_j; 8 m words instead of 6 m, so
// the LDS tier of a bounded LP ends at 138 rows.  `flipped` and `ub` are in global memory beside `pos`.  An LP without a finite bound
// runs the plain instantiation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "exact_values.hpp"
#include "launch.hpp"
#include "many_certify.hpp"
#include "options.hpp"
#include "pivot_step.hpp"
#include "price_step.hpp"
#include "solver.hpp"
#include "wave_ops.hpp"

namespace relp {

constexpr int MANY_THREADS = 512;
constexpr int MANY_WAVES = MANY_THREADS / WAVE;
constexpr int MANY_MAX_ROWS = 512;
constexpr size_t MANY_LDS_BYTES = 160 * 1024;        // a CU of gfx950
constexpr size_t MANY_STATIC_LDS = 1024;             // the kernel's __shared__ scalars (below), rounded up
constexpr double MANY_RESIDUAL_BOUND = 1e-6;         // max |B B^-1 - I| a fresh inversion must reach, else RELP_ERR_NUMERICAL
constexpr int MANY_TIERS = 4;                        // launch groups per instantiation: three LDS sizes and the global tier
constexpr int MANY_GROUPS = 2 * MANY_TIERS;          // ... of the plain and of the bounded kernel
constexpr double MANY_ZERO_LEVEL_TOL = 1e-7;         // row scan of a zero-level pivot (as Solver::drive_out_artificials)

// Words (8 bytes) of the per-LP vectors in LDS: x_B, -pi, rho_p, w, alpha, then the basis and the pivot rows of the inversion
// (2 m ints), with implicit bounds xub and b' too, and in the LDS tier the m x m inverse.
__host__ __device__ constexpr size_t many_vector_words(int m, bool bounded = false) { return (size_t)(bounded ? 8 : 6) * m; }
__host__ __device__ constexpr size_t many_lds_bytes(int m, bool inverse_in_lds, bool bounded = false) {
    return 8 * (many_vector_words(m, bounded) + (inverse_in_lds ? (size_t)m * m : 0));
}
// Largest m whose LDS tier fits a CU: 139 rows (139 x 139 x 8 + 6 x 139 x 8 = 161 240 bytes, plus the static part); with implicit
// bounds 138 rows (138 x 138 x 8 + 8 x 138 x 8 = 161 184 bytes; 139 rows would need 163 464).
constexpr int many_lds_tier_rows(bool bounded = false) {
    int m = 1;
    while (m < MANY_MAX_ROWS && many_lds_bytes(m + 1, true, bounded) + MANY_STATIC_LDS <= MANY_LDS_BYTES) ++m;
    return m;
}
static_assert(many_lds_tier_rows() == 139, "the documented cut-off of the LDS tier");
static_assert(many_lds_tier_rows(true) == 138, "the documented cut-off of the LDS tier with implicit bounds");

struct ManyLP {
    int m, n, n_art, textbook;
    long long col_off;   // n + 1 column starts (relative to nz_off)
    long long nz_off;    // row indices, values
    long long c_off;     // n: costs of phase two, steepest-edge weights, column positions
    long long r_off;     // m: right-hand side, initial basis, final basis, final x_B
    long long inv_off;   // m * m: the global tier's inverse (unused in the LDS tier)
    long long max_pivots;
};

struct ManyOut {
    int status;        // relp_status
    int kind;          // relp_result_kind
    int entering;      // device column of the ray (UNBOUNDED)
    int redundant;     // rows left on a zero-level artificial
    long long pivots_phase_one, pivots_phase_two, reinversions;
    long long bound_flips;  // implicit bounds: iterations that moved the entering variable to its other bound (counted in the pivots too)
    double minus_obj;
    double max_residual;
};

struct ManyArgs {
    const ManyLP* lps;
    const int* order;  // workgroup -> LP, longest estimated solve first
    const int* col_start;
    const int* row_index;
    const double* value;
    const double* cost2;
    const double* rhs;
    const int* basis0;
    double* gamma;
    int* pos;
    const double* ub;  // implicit bounds: [n] per LP beside `pos` (+inf: none), and which columns are held in complemented form
    int* flipped;
    double* inverse;
    int* basis_out;
    double* xb_out;
    ManyOut* out;
    int rule;
    int polish_period;
    double tol_dual, tol_pivot, harris_delta, tol_feasible;
};

enum : int { MANY_PIVOTED = 0, MANY_NO_ENTERING = 1, MANY_UNBOUNDED = 2 };

template <bool LDS_INVERSE, bool BOUNDED>
__global__ void __launch_bounds__(MANY_THREADS) many_kernel(ManyArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double s_akey[MANY_WAVES];
    __shared__ unsigned long long s_arank[MANY_WAVES];
    __shared__ double s_red[MANY_WAVES + 2];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const ManyLP L = a.lps[a.order[blockIdx.x]];
    const int m = L.m, n = L.n, n_art = L.n_art, ld = m;
    const int* cs = a.col_start + L.col_off;
    const int* ri = a.row_index + L.nz_off;
    const double* va = a.value + L.nz_off;
    const double* cost2 = a.cost2 + L.c_off;
    const double* rhs = a.rhs + L.r_off;
    double* gamma = a.gamma + L.c_off;
    int* pos = a.pos + L.c_off;
    double* xb = smem;
    double* mpi = xb + m;
    double* rho = mpi + m;
    double* w = rho + m;
    double* alpha = w + m;
    int* basis = reinterpret_cast<int*>(alpha + m);
    int* pivot_row = basis + m;
    // implicit bounds: the bound of the variable basic in row i, the right-hand side b' of the complemented LP; per column the bound
    // and whether the column is held in complemented form (x'_j = u_j - x_j, column and cost negated)
    double* xub = BOUNDED ? smem + many_vector_words(m) : nullptr;
    double* bprime = BOUNDED ? xub + m : nullptr;
    const double* ub = BOUNDED ? a.ub + L.c_off : nullptr;
    int* flipped = BOUNDED ? a.flipped + L.c_off : nullptr;
    double* inv = LDS_INVERSE ? smem + many_vector_words(m, BOUNDED) : a.inverse + L.inv_off;
    const bool steepest = a.rule == RELP_PIVOT_STEEPEST_EDGE;
    const double slack = L.textbook ? 0.0 : a.harris_delta;

    int phase = n_art > 0 ? 1 : 2;
    auto cost = [&](int j) { return phase == 1 ? (j < n_art ? 1.0 : 0.0) : cost2[j]; };
    // cost and entries of a column as the basis holds it: a complemented column with the opposite sign (cb_kernel, invert_kernel)
    auto basic_cost = [&](int j) {
        if constexpr (BOUNDED) return flipped[j] ? -cost(j) : cost(j);
        else return cost(j);
    };
    auto basic_value = [&](int j, int e) {
        if constexpr (BOUNDED) return flipped[j] ? -va[e] : va[e];
        else return va[e];
    };
    auto block_sum = [&](double v) { return block_reduce<0>(v, s_red); };
    auto block_max = [&](double v) { return -block_reduce<1>(-v, s_red); };

    // ---- Tableau::new over Partially (partially.rs:125-205): B = I, artificial k on its row, slack pivots on the others ----
    if constexpr (BOUNDED) {  // nothing is complemented; a variable whose two bounds coincide is never priced (-3)
        for (int j = tid; j < n; j += MANY_THREADS) {
            pos[j] = ub[j] == 0.0 ? -3 : -1;
            flipped[j] = 0;
        }
    } else {
        for (int j = tid; j < n; j += MANY_THREADS) pos[j] = -1;
    }
    for (int i = tid; i < m; i += MANY_THREADS) {
        basis[i] = a.basis0[L.r_off + i];
        xb[i] = rhs[i];
        rho[i] = w[i] = 0.0;
        if constexpr (BOUNDED) {  // (the initial basic variables, artificials and slacks, have no upper bound)
            xub[i] = INFINITY;
            bprime[i] = rhs[i];
        }
    }
    __syncthreads();
    for (int i = tid; i < m; i += MANY_THREADS) pos[basis[i]] = i;
    for (int j = wave; j < m; j += MANY_WAVES)
        for (int i = lane; i < m; i += WAVE) inv[(size_t)j * ld + i] = i == j ? 1.0 : 0.0;
    __syncthreads();

    double minus_obj = 0.0, max_residual = 0.0;
    long long pivots[2] = {0, 0}, reinversions = 0, since = 0, bound_flips = 0;
    int pending = 0, leaving = -1, status = RELP_OK, kind = RELP_RESULT_NONE, entering = -1, redundant = 0;
    double gamma_q = 1.0, alpha_pq = 1.0;

    // -pi = -c_B' B^-1 (pi_kernel) and the objective (cb_kernel), from the costs of the current phase
    auto refresh_pi = [&]() {
        for (int j = wave; j < m; j += MANY_WAVES) {
            double acc = 0.0;
            for (int i = lane; i < m; i += WAVE) acc += basic_cost(basis[i]) * inv[(size_t)j * ld + i];
            acc = wave_sum(acc);
            if (lane == LAST) mpi[j] = -acc;
        }
        double v = 0.0;
        for (int i = tid; i < m; i += MANY_THREADS) v += xb[i] * basic_cost(basis[i]);
        if constexpr (BOUNDED)  // the constant of the complemented variables: sum u_j c_j
            for (int j = tid; j < n; j += MANY_THREADS)
                if (flipped[j]) v += ub[j] * cost(j);
        minus_obj = -block_sum(v);  // (its barriers publish -pi too)
    };
    // x_B = B^-1 b (xb_kernel); with implicit bounds b is b'
    auto refresh_xb = [&]() {
        const double* b = BOUNDED ? bprime : rhs;
        for (int i = tid; i < m; i += MANY_THREADS) {
            double acc = 0.0;
            for (int j = 0; j < m; ++j) acc += inv[(size_t)j * ld + i] * b[j];
            xb[i] = acc;
        }
        __syncthreads();
    };
    // `Carry::from_artificial` hand-over / phase start: -pi and the weights gamma_j = 1 + |B^-1 a_j|^2 (gamma_init_kernel)
    auto set_phase = [&](int new_phase) {
        phase = new_phase;
        refresh_pi();
        if (steepest)
            for (int j = n_art + tid; j < n; j += MANY_THREADS) {
                if (pos[j] >= 0) {
                    gamma[j] = 1.0;
                    continue;
                }
                double acc = 0.0;
                for (int i = 0; i < m; ++i) {
                    double v = 0.0;
                    for (int e = cs[j]; e < cs[j + 1]; ++e) v += inv[(size_t)ri[e] * ld + i] * va[e];
                    acc += v * v;
                }
                gamma[j] = 1.0 + acc;
            }
        pending = 0;
        __syncthreads();
    };
    // max |B B^-1 - I| over the basis columns (residual_kernel)
    auto residual = [&]() {
        double worst = 0.0;
        for (int i = tid; i < m; i += MANY_THREADS)
            for (int k = 0; k < m; ++k) {
                const int col = basis[k];
                double acc = i == k ? 1.0 : 0.0;
                for (int e = cs[col]; e < cs[col + 1]; ++e) acc -= basic_value(col, e) * inv[(size_t)ri[e] * ld + i];
                worst = fmax(worst, fabs(acc));
                if (acc != acc) worst = INFINITY;  // (NaN)
            }
        return block_max(worst);
    };
    // `BasisInverse::invert` (lower_upper/mod.rs:78-92): B^-1 from the basis columns by Gauss-Jordan with partial pivoting, in place;
    // then x_B, -pi and the objective from it.  false: singular, or the fresh inverse misses MANY_RESIDUAL_BOUND.
    auto reinvert = [&]() -> bool {
        max_residual = fmax(max_residual, residual());
        ++reinversions;
        since = 0;
        for (int j = wave; j < m; j += MANY_WAVES)
            for (int i = lane; i < m; i += WAVE) inv[(size_t)j * ld + i] = 0.0;
        __syncthreads();
        for (int k = wave; k < m; k += MANY_WAVES) {
            const int col = basis[k];
            for (int e = cs[col] + lane; e < cs[col + 1]; e += WAVE) inv[(size_t)k * ld + ri[e]] = basic_value(col, e);
        }
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            double key = 0.0;
            unsigned long long rank = RANK_NONE;
            for (int i = k + tid; i < m; i += MANY_THREADS) {
                const double mag = fabs(inv[(size_t)k * ld + i]);
                if (mag > 0.0 && (rank == RANK_NONE || mag > key)) {  // (ascending i: ties keep the lowest row)
                    key = mag;
                    rank = (unsigned long long)i;
                }
            }
            block_argbest(key, rank, s_akey, s_arank);
            if (rank == RANK_NONE) return false;  // singular
            const int r = (int)rank;
            if (r != k)
                for (int j = tid; j < m; j += MANY_THREADS) {
                    const double t = inv[(size_t)j * ld + k];
                    inv[(size_t)j * ld + k] = inv[(size_t)j * ld + r];
                    inv[(size_t)j * ld + r] = t;
                }
            if (tid == 0) pivot_row[k] = r;
            __syncthreads();
            const double piv = inv[(size_t)k * ld + k];
            for (int i = tid; i < m; i += MANY_THREADS) alpha[i] = inv[(size_t)k * ld + i];  // column k before the step
            __syncthreads();
            for (int j = tid; j < m; j += MANY_THREADS) inv[(size_t)j * ld + k] = (j == k ? 1.0 : inv[(size_t)j * ld + k]) / piv;
            __syncthreads();
            for (int j = wave; j < m; j += MANY_WAVES) {
                const double rk = inv[(size_t)j * ld + k];
                for (int i = lane; i < m; i += WAVE)
                    if (i != k) inv[(size_t)j * ld + i] = (j == k ? 0.0 : inv[(size_t)j * ld + i]) - alpha[i] * rk;
            }
            __syncthreads();
        }
        for (int k = m - 1; k >= 0; --k) {  // the row interchanges, undone as column interchanges
            const int r = pivot_row[k];
            if (r == k) continue;
            for (int i = tid; i < m; i += MANY_THREADS) {
                const double t = inv[(size_t)k * ld + i];
                inv[(size_t)k * ld + i] = inv[(size_t)r * ld + i];
                inv[(size_t)r * ld + i] = t;
            }
            __syncthreads();
        }
        __syncthreads();
        const double fresh = residual();
        if (!(fresh <= MANY_RESIDUAL_BOUND)) return false;
        refresh_xb();
        refresh_pi();
        return true;
    };
    // One pricing pass (with the pending steepest-edge update) and, unless `forced_q` >= 0, the entering column; then FTRAN, the
    // ratio test (or the given row) and the basis change.  Returns MANY_PIVOTED / MANY_NO_ENTERING / MANY_UNBOUNDED.
    // The ratio test and the step decision are those of pivot_step.hpp; a bound flip is MANY_PIVOTED without a basis change.
    auto ratio_row = [&](int i, double al) {
        return row_room(al, xb[i], [&] { return xub[i]; }, !(phase == 2 && basis[i] < n_art), BOUNDED, a.tol_pivot);
    };
    auto pivot = [&](int forced_q, int forced_p) -> int {
        double key = 0.0;
        unsigned long long rank = RANK_NONE;
        for (int j = n_art + tid; j < n; j += MANY_THREADS) {
            const int pos_j = pos[j];
            if (!column_priced(pos_j, BOUNDED)) continue;
            double d_pi = 0.0, d_rho = 0.0, d_w = 0.0;
            for (int e = cs[j]; e < cs[j + 1]; ++e) {
                const int r = ri[e];
                const double v = va[e];
                d_pi += v * mpi[r];
                if (pending) {
                    d_rho += v * rho[r];
                    d_w += v * w[r];
                }
            }
            const double cbar = column_sign(pos_j, BOUNDED) * (cost(j) + d_pi);
            double g = 1.0;
            if (steepest) {
                g = gamma[j];
                if (pending) gamma[j] = g = weight_after_pivot(g, d_rho, d_w, gamma_q, alpha_pq, j == leaving);
            }
            bool candidate;
            const double k = steepest ? price_key<RELP_PIVOT_STEEPEST_EDGE>(cbar, a.tol_dual, g, j, -1, n, candidate)
                                      : price_key<RELP_PIVOT_DANTZIG>(cbar, a.tol_dual, g, j, -1, n, candidate);
            if (candidate) {  // (one workgroup prices every column: slot 0)
                if (steepest) offer_entering<RELP_PIVOT_STEEPEST_EDGE>(k, j, 0, key, rank);
                else offer_entering<RELP_PIVOT_DANTZIG>(k, j, 0, key, rank);
            }
        }
        pending = 0;
        int block = 0;
        const int winner = steepest ? entering_winner<RELP_PIVOT_STEEPEST_EDGE>(key, rank, s_akey, s_arank, block)
                                    : entering_winner<RELP_PIVOT_DANTZIG>(key, rank, s_akey, s_arank, block);
        int q = forced_q;
        if (q < 0) {
            if (winner < 0) return MANY_NO_ENTERING;
            q = winner;
        }
        double cbar_q = reduced_cost_of(cost(q), cs, ri, va, mpi, q);  // (every thread: the same sum in the same order as the pricing pass)
        double sgn_q = 1.0, ub_q = INFINITY;
        if constexpr (BOUNDED) {
            sgn_q = flipped[q] ? -1.0 : 1.0;
            ub_q = ub[q];
            cbar_q *= sgn_q;
        }
        // FTRAN: alpha = B^-1 a_q (of the complemented column: with the opposite sign)
        double sumsq = 0.0, theta = INFINITY;
        for (int i = tid; i < m; i += MANY_THREADS) {
            double acc = 0.0;
            for (int e = cs[q]; e < cs[q + 1]; ++e) acc += inv[(size_t)ri[e] * ld + i] * va[e];
            if constexpr (BOUNDED) acc *= sgn_q;
            alpha[i] = acc;
            sumsq += acc * acc;
            const RowRoom row = ratio_row(i, acc);
            if (row.eligible) theta = fmin(theta, harris_pass1(row.room, slack, acc));
        }
        gamma_q = 1.0 + block_sum(sumsq);  // pivot_rule.rs:258
        const double theta_max = block_reduce<1>(theta, s_red);
        // Harris pass 2: the largest eligible pivot within theta_max (the textbook rule: every ratio at the minimum), ties by the
        // lowest leaving column, then the lowest row
        key = 0.0;
        rank = RANK_NONE;
        for (int i = tid; i < m; i += MANY_THREADS) {
            const double al = alpha[i];
            const RowRoom row = ratio_row(i, al);
            const double mag = fabs(al);
            if (forced_p >= 0 ? i == forced_p : (row.eligible && harris_accepts(row.room, mag, theta_max)))
                keep_better(harris_key(L.textbook, mag), leaving_rank(basis[i], i), key, rank);
        }
        block_argbest(key, rank, s_akey, s_arank);
        const int p = leaving_row(rank);
        const double alpha_p = p >= 0 ? alpha[p] : 1.0;
        const double xb_p = p >= 0 ? xb[p] : 0.0;
        const Step step = step_decision(BOUNDED, forced_p >= 0, p, alpha_p, xb_p, p >= 0 ? ratio_row(p, alpha_p).room : 0.0, ub_q);
        if constexpr (BOUNDED) {
            if (step.flip) {
                // bound flip: x_q runs from 0 to u_q and is complemented so that it sits at 0 again; the basis does not change, so
                // neither the inverse nor -pi nor the weights do
                __syncthreads();  // (x_B read by every thread)
                for (int i = tid; i < m; i += MANY_THREADS) xb[i] -= alpha[i] * ub_q;
                for (int e = cs[q] + tid; e < cs[q + 1]; e += MANY_THREADS) bprime[ri[e]] -= ub_q * sgn_q * va[e];
                if (tid == 0) flip_column(pos, flipped, q, sgn_q);
                minus_obj -= cbar_q * ub_q;
                ++pivots[phase - 1];
                ++bound_flips;
                ++since;
                __syncthreads();
                return MANY_PIVOTED;
            }
        }
        if (p < 0) {
            entering = q;
            return MANY_UNBOUNDED;
        }
        alpha_pq = alpha_p;
        if (alpha_pq == 0.0) {
            entering = q;
            return MANY_UNBOUNDED;  // (a forced row whose element vanished: never from the ratio test, which needs alpha > tol_pivot)
        }
        leaving = basis[p];
        const double xp = step.xp;
        int leaving_flipped = 0;
        if constexpr (BOUNDED) leaving_flipped = flipped[leaving];
        __syncthreads();  // x_B[p], basis[p] and flipped[leaving] read by every thread
        for (int i = tid; i < m; i += MANY_THREADS) xb[i] = i == p ? xp : xb[i] - alpha[i] * xp;
        if constexpr (BOUNDED)
            if (step.leaves_at_upper) {  // the leaving variable reached its upper bound: it is held in complemented form from now on
                const double sgn_l = leaving_flipped ? -1.0 : 1.0;
                for (int e = cs[leaving] + tid; e < cs[leaving + 1]; e += MANY_THREADS) bprime[ri[e]] -= step.ub_leaving * sgn_l * va[e];
            }
        minus_obj -= cbar_q * xp;
        // rank-one update of B^-1 by columns, with rho_p, w = alpha' B^-1_old and -pi (pivot_fused_kernel)
        for (int j = wave; j < m; j += MANY_WAVES) {
            double* col = inv + (size_t)j * ld;
            const double r_j = col[p] / alpha_pq;
            double w_j = 0.0;
            for (int i = lane; i < m; i += WAVE) {
                const double o = col[i], al = alpha[i];
                w_j += al * o;
                col[i] = i == p ? r_j : (al != 0.0 ? o - al * r_j : o);
            }
            w_j = wave_sum(w_j);
            if (lane == LAST) {
                w[j] = w_j;
                rho[j] = r_j;
                mpi[j] -= cbar_q * r_j;
            }
        }
        if (tid == 0) {
            basis[p] = q;
            exchange_columns(pos, flipped, xub, BOUNDED, q, p, leaving, leaving_flipped, step.leaves_at_upper, ub_q);
        }
        pending = steepest ? 1 : 0;
        ++pivots[phase - 1];
        ++since;
        __syncthreads();
        return MANY_PIVOTED;
    };

    const long long cap = L.max_pivots;
    set_phase(phase);
    auto numerical = [&]() { status = RELP_ERR_NUMERICAL; };
    // phase one, then phase two (phase_one.rs:134-178, phase_two.rs:36-58)
    while (status == RELP_OK && kind == RELP_RESULT_NONE) {
        if (a.polish_period > 0 && since >= a.polish_period && !reinvert()) { numerical(); break; }
        if (pivots[0] + pivots[1] >= cap) { kind = RELP_RESULT_ITERATION_LIMIT; break; }
        const int step = pivot(-1, -1);
        if (step == MANY_PIVOTED) continue;
        if (since > 0) {  // a verdict is drawn from a fresh inverse only: re-invert and look again
            if (!reinvert()) numerical();
            continue;
        }
        if (step == MANY_UNBOUNDED) {
            if (phase == 1) numerical();  // "Artificial cost can not be unbounded." (phase_one.rs:151)
            else kind = RELP_RESULT_UNBOUNDED;  // phase_two.rs:53
            break;
        }
        if (phase == 2) { kind = RELP_RESULT_FINITE_OPTIMUM; break; }
        // end of phase one: infeasible when the artificial objective stays positive (phase_one.rs:171-173)
        double sum = 0.0;
        for (int i = tid; i < m; i += MANY_THREADS) sum += fabs(xb[i]);
        const double scale = 1.0 + block_sum(sum);
        if (-minus_obj > a.tol_feasible * scale) { kind = RELP_RESULT_INFEASIBLE; break; }
        // zero-level artificials leave by forced pivots; a row without a candidate is redundant and keeps its artificial
        for (int r = 0; r < m && status == RELP_OK; ++r) {
            if (basis[r] >= n_art) continue;
            unsigned long long first = RANK_NONE;
            for (int j = n_art + tid; j < n; j += MANY_THREADS) {
                if (BOUNDED ? pos[j] >= 0 : pos[j] != -1) continue;  // (every non-basic column, as row_scan_kernel: fixed ones too)
                double acc = 0.0;
                for (int e = cs[j]; e < cs[j + 1]; ++e) acc += va[e] * inv[(size_t)ri[e] * ld + r];
                if (fabs(acc) > MANY_ZERO_LEVEL_TOL && first == RANK_NONE) first = (unsigned long long)j;
            }
            double one = 1.0;
            block_argbest(one, first, s_akey, s_arank);
            if (first == RANK_NONE) {
                ++redundant;
                continue;
            }
            if (tid == 0) xb[r] = 0.0;  // the artificial that leaves is zero: no residue is divided by a small pivot
            __syncthreads();
            if (pivot((int)first, r) != MANY_PIVOTED) numerical();
        }
        if (status != RELP_OK) break;
        if (since > 0 && !reinvert()) { numerical(); break; }
        set_phase(2);
    }
    __syncthreads();
    if constexpr (BOUNDED) {
        // A fixed variable sits at both of its bounds at once; which of the two the reference's formulation sees is decided by its
        // reduced cost (Solver::resolve_fixed_columns): negative -> at the upper bound (-2), else the bound slack is basic (-1).
        for (int j = n_art + tid; j < n; j += MANY_THREADS) {
            if (pos[j] != -3) continue;
            double cbar = cost(j);
            for (int e = cs[j]; e < cs[j + 1]; ++e) cbar += va[e] * mpi[ri[e]];
            pos[j] = cbar < 0.0 ? -2 : -1;
        }
    }
    for (int i = tid; i < m; i += MANY_THREADS) {
        a.basis_out[L.r_off + i] = basis[i];
        a.xb_out[L.r_off + i] = xb[i];
    }
    if (tid == 0) {
        ManyOut o;
        o.status = status;
        o.kind = kind;
        o.entering = entering;
        o.redundant = redundant;
        o.pivots_phase_one = pivots[0];
        o.pivots_phase_two = pivots[1];
        o.reinversions = reinversions;
        o.bound_flips = bound_flips;
        o.minus_obj = minus_obj;
        o.max_residual = max_residual;
        a.out[a.order[blockIdx.x]] = o;
    }
}

namespace {
double many_now() {
    using clock = std::chrono::steady_clock;
    return std::chrono::duration<double>(clock::now().time_since_epoch()).count();
}
// the switches that select kernels of the generated incidence columns of the graph providers: this path materialises every column
constexpr unsigned MANY_REFUSED_SWITCHES = RELP_SW_ELL_WIDE | RELP_SW_PRICE_UNIT_PAIRS | RELP_SW_NO_RHO_BITS | RELP_SW_NETWORK_STATS;
}  // namespace

// One LP as the device sees it (the index space and the data a `Solver` with the explicit carry has, with or without implicit
// bounds), and what is this path's own: the tier, the launch group and the work estimate.
struct ManyHostLP {
    int m = 0, n = 0, n_art = 0, textbook = 0, lds = 0, bucket = 0, bounded = 0;
    DeviceColumns cols;
    DeviceMatrix data;
    std::vector<double> ub;  // bounded: [n] upper bound of each device column, +inf where there is none
    double work = 0.0;  // estimated solve time, for the launch order
};

// Rows of the device LP: with implicit bounds the constraint rows of an LP that has a bound, else every row of the standard form.
int many_device_rows(const MatrixData& md, bool implicit_bounds) {
    return implicit_bounds && md.nr_variable_bounds() > 0 ? md.nr_constraints() : md.nr_rows();
}

ManyHostLP many_host_lp(const StandardForm& form, const relp_options& o, bool implicit_bounds) {
    ManyHostLP lp;
    const MatrixData& md = form.data;
    // as for a Solver (kernel_path.hpp): an LP without a finite bound is not a bounded one; a bounded one has the constraint rows and the
    // first four column groups, and the bounds of the structurals and the ranges of the range slacks per column
    lp.bounded = implicit_bounds && md.nr_variable_bounds() > 0;
    lp.cols = device_columns(md, lp.bounded);
    lp.data = DeviceMatrix(lp.cols, md);
    const int m = lp.m = lp.cols.m, n = lp.n = lp.cols.n();
    lp.n_art = lp.cols.n_art;
    if (lp.bounded) lp.ub = implicit_upper_bounds(md, lp.cols);
    // (every LP here has at most 512 rows: the kernels have the textbook rule)
    lp.textbook = resolves_to_textbook(o, lp.data, true);
    lp.lds = m <= many_lds_tier_rows(lp.bounded) && !(o.switches & RELP_SW_MANY_GLOBAL_TIER);
    // launch groups: three LDS sizes (7, 2 and 1 workgroups per CU) and the global tier; the bounded LPs in four groups of their own
    lp.bucket = (!lp.lds ? 3 : m <= 48 ? 0 : m <= 96 ? 1 : 2) + (lp.bounded ? MANY_TIERS : 0);
    lp.work = (double)(m + n) * m * ((double)m + (double)lp.data.row_index.size() / std::max(1, n));
    return lp;
}

}  // namespace relp

using namespace relp;

struct relp_many {
    relp_options options;
    std::vector<StandardForm> forms;
    std::vector<ManyHostLP> lps;
    int device = 0;
    // device arrays
    ManyLP* d_lps = nullptr;
    int *d_order = nullptr, *d_col_start = nullptr, *d_row_index = nullptr, *d_basis0 = nullptr, *d_pos = nullptr, *d_basis_out = nullptr;
    double *d_value = nullptr, *d_cost2 = nullptr, *d_rhs = nullptr, *d_gamma = nullptr, *d_inverse = nullptr, *d_xb_out = nullptr;
    double* d_ub = nullptr;     // implicit bounds (allocated when an LP of the list is bounded)
    int* d_flipped = nullptr;
    ManyOut* d_out = nullptr;
    bool implicit_bounds = false;     // relp_many_config.implicit_bounds
    bool any_bounded = false;
    std::vector<int> order;           // LP indices, grouped by bucket, longest first within a bucket
    int bucket_first[MANY_GROUPS + 1] = {};
    int bucket_rows[MANY_GROUPS] = {};  // largest m of each bucket
    hipStream_t streams[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_start = nullptr, ev_stop = nullptr, ev_done[4] = {nullptr, nullptr, nullptr, nullptr};
    DeviceAllocations memory;  // every device array above
    CertifyScratch certify_scratch;
    // results of the last solve
    bool solved = false;
    std::vector<relp_many_result> results;
    std::vector<long long> bound_flips;
    std::vector<std::vector<int>> bases;      // provider codes (DeviceColumns::to_provider); bounded: of the reference's formulation
    std::vector<std::vector<double>> solutions;  // every column of MatrixData
    std::vector<std::string> exact;
    std::vector<int> entering;                // device column a verdict of UNBOUNDED names (the ray of its certificate)
    std::vector<std::array<int32_t, 3>> certificate_digits;  // of the last relp_many_certify: primal, dual, ray (empty before one)
    bool keep_witnesses = false;              // relp_many_keep_witnesses
    bool witnesses_kept = false;              // the last relp_many_certify ran with the switch on
    std::vector<std::shared_ptr<const ExactWitnesses>> witnesses;  // of that call, per LP (null: not certified); empty with the switch off
    std::string error;

    void release() {
        (void)hipSetDevice(device);
        certify_scratch.release();
        memory.free_all();
        for (hipStream_t& s : streams)
            if (s) (void)hipStreamDestroy(s);
        for (hipEvent_t e : {ev_start, ev_stop, ev_done[0], ev_done[1], ev_done[2], ev_done[3]})
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {
void many_set_error(char* error, int32_t capacity, const std::string& text) {
    if (!error || capacity <= 0) return;
    const size_t n = std::min<size_t>(text.size(), (size_t)capacity - 1);
    std::memcpy(error, text.data(), n);
    error[n] = 0;
}
template <class T>
T* many_upload(DeviceAllocations& memory, const std::vector<T>& host) {
    T* p = memory.alloc<T>(host.size());
    if (!host.empty()) RELP_HIP(hipMemcpy(p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return p;
}
// (with implicit bounds the explicit basis proves an optimum; the two other verdicts stay uncertified, as on a handle)
bool many_serial_certificate_applies(const relp_many& many, int k) {
    const relp_many_result& res = many.results[k];
    return res.status == RELP_OK && (res.kind == RELP_RESULT_FINITE_OPTIMUM ||
                                     (!many.lps[k].bounded && (res.kind == RELP_RESULT_INFEASIBLE || res.kind == RELP_RESULT_UNBOUNDED)));
}

// The certificate of model k's verdict in certify_basis's terms: its mode, and for UNBOUNDED the provider column of the ray (-1: none).
void many_certificate_kind(const relp_many& many, int k, int* mode, int* ray) {
    const ManyHostLP& lp = many.lps[k];
    const int kind = many.results[k].kind;
    const int entering = many.entering[k];
    *mode = kind == RELP_RESULT_INFEASIBLE ? 1 : kind == RELP_RESULT_UNBOUNDED ? 2 : 0;
    *ray = kind == RELP_RESULT_UNBOUNDED && entering >= lp.n_art && entering < lp.n ? entering - lp.n_art : -1;
}

// The exact certificate of relp_solve_relaxation for model k of the last solve (certify_basis: its other primes and its exact repair
// pivots included).  Sets results[k].certified and certify_seconds, and exact[k].
bool many_serial_certificate(relp_many& many, int k, long long* repairs, std::shared_ptr<const ExactWitnesses>* witnesses = nullptr) {
    relp_many_result& res = many.results[k];
    const double t0 = many_now();
    bool ok = false;
    std::string message;
    int mode = 0, ray = -1;
    many_certificate_kind(many, k, &mode, &ray);
    many.certify_scratch.statics.reset();  // (what it keeps belongs to one LP)
    many.certify_scratch.digit_hints[0] = many.certify_scratch.digit_hints[1] = 0;
    *repairs = 0;
    try {
        certify_basis(many.forms[k], many.bases[k], many.device, many.streams[0], &many.exact[k], &ok, repairs, &message, mode, ray, nullptr,
                      &many.certify_scratch, witnesses);
    } catch (const RatOverflow& e) {  // the f64 result stands, uncertified
        ok = false;
        message = std::string("exact certificate: ") + e.what();
    }
    if (!ok) {
        many.exact[k].clear();
        if (many.error.empty()) many.error = "model " + std::to_string(k) + ": " + message;
    }
    res.certified = ok ? 1 : 0;
    res.certify_seconds = many_now() - t0;
    return ok;
}

// The options this path honours; the message names the first one it cannot.
std::string many_refusal(const relp_options& o) {
    if (o.carry != RELP_CARRY_EXPLICIT) return "relp_many keeps an explicit inverse: carry must be RELP_CARRY_EXPLICIT";
    if (o.implicit_bounds) return "relp_many has no implicit bounds (implicit_bounds must be 0)";
    if (o.crash) return "relp_many starts from the reference's initial basis (crash must be 0)";
    if (o.pivot_rule != RELP_PIVOT_STEEPEST_EDGE && o.pivot_rule != RELP_PIVOT_DANTZIG)
        return "relp_many implements RELP_PIVOT_STEEPEST_EDGE and RELP_PIVOT_DANTZIG only";
    if (o.ratio_rule < RELP_RATIO_HARRIS || o.ratio_rule > RELP_RATIO_AUTO) return "unknown ratio_rule";
    if (o.switches & MANY_REFUSED_SWITCHES) return "relp_many materialises every column: the switches of the generated graph columns do not apply";
    return std::string();
}
}  // namespace

extern "C" {

int32_t relp_many_create(const relp_model* const* models, int32_t n_models, const relp_options* options, relp_many** out, char* error,
                         int32_t error_capacity) {
    return relp_many_create_with(models, n_models, options, nullptr, out, error, error_capacity);
}

int32_t relp_many_create_with(const relp_model* const* models, int32_t n_models, const relp_options* options, const relp_many_config* config,
                              relp_many** out, char* error, int32_t error_capacity) {
    if (out) *out = nullptr;
    if (!models || n_models <= 0 || !out) {
        many_set_error(error, error_capacity, "models, n_models > 0 and out are required");
        return RELP_ERR_ARGUMENT;
    }
    relp_options adopted;
    if (adopt_options(options, &adopted) != RELP_OK) {
        many_set_error(error, error_capacity, "relp_options.struct_size is not a size this library's header ever had");
        return RELP_ERR_ARGUMENT;
    }
    const std::string refused = many_refusal(adopted);
    if (!refused.empty()) {
        many_set_error(error, error_capacity, refused);
        return RELP_ERR_ARGUMENT;
    }
    if (config && config->struct_size != (int32_t)sizeof(relp_many_config)) {  // (the one size this struct has had)
        many_set_error(error, error_capacity, "relp_many_config.struct_size is not a size this library's header ever had");
        return RELP_ERR_ARGUMENT;
    }
    if (config && config->implicit_bounds != 0 && config->implicit_bounds != 1) {
        many_set_error(error, error_capacity, "relp_many_config.implicit_bounds must be 0 or 1");
        return RELP_ERR_ARGUMENT;
    }
    const bool implicit_bounds = config && config->implicit_bounds == 1;
    // every model is checked before the device is touched
    for (int32_t k = 0; k < n_models; ++k) {
        if (!models[k]) {
            many_set_error(error, error_capacity, "model " + std::to_string(k) + ": null");
            return RELP_ERR_ARGUMENT;
        }
        const int rows = many_device_rows(models[k]->form.data, implicit_bounds);
        if (rows < 1 || rows > MANY_MAX_ROWS) {
            many_set_error(error, error_capacity, "model " + std::to_string(k) + ": " + std::to_string(rows) +
                                                      (implicit_bounds ? " constraint rows" : " rows in standard form") + "; relp_many takes 1 to " +
                                                      std::to_string(MANY_MAX_ROWS));
            return RELP_ERR_ARGUMENT;
        }
    }
    auto many = std::make_unique<relp_many>();
    many->options = adopted;
    many->implicit_bounds = implicit_bounds;
    many->device = adopted.device;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || adopted.device < 0 || adopted.device >= count ||
        hipSetDevice(adopted.device) != hipSuccess) {
        (void)hipGetLastError();
        many_set_error(error, error_capacity, "no usable HIP device (the product has no CPU fallback)");
        return RELP_ERR_DEVICE;
    }
    try {
        const int n = n_models;
        many->forms.reserve(n);
        for (int k = 0; k < n; ++k) many->forms.push_back(models[k]->form);
        for (int k = 0; k < n; ++k) many->lps.push_back(many_host_lp(many->forms[k], adopted, implicit_bounds));
        for (const ManyHostLP& lp : many->lps) many->any_bounded |= lp.bounded != 0;
        // pack: CSC, costs, right-hand sides, initial bases; per-LP offsets
        std::vector<ManyLP> desc(n);
        std::vector<int> col_start, row_index, basis0;
        std::vector<double> value, cost2, rhs, ub;
        long long inverse_words = 0;
        for (int k = 0; k < n; ++k) {
            const ManyHostLP& lp = many->lps[k];
            ManyLP& d = desc[k];
            d.m = lp.m;
            d.n = lp.n;
            d.n_art = lp.n_art;
            d.textbook = lp.textbook;
            d.col_off = (long long)col_start.size();
            d.nz_off = (long long)row_index.size();
            d.c_off = (long long)cost2.size();
            d.r_off = (long long)rhs.size();
            d.inv_off = lp.lds ? 0 : inverse_words;
            if (!lp.lds) inverse_words += (long long)lp.m * lp.m;
            d.max_pivots = adopted.max_pivots > 0 ? adopted.max_pivots : 200LL * (lp.m + lp.n) + 100000;
            col_start.insert(col_start.end(), lp.data.col_start.begin(), lp.data.col_start.end());
            row_index.insert(row_index.end(), lp.data.row_index.begin(), lp.data.row_index.end());
            value.insert(value.end(), lp.data.value.begin(), lp.data.value.end());
            cost2.insert(cost2.end(), lp.data.cost2.begin(), lp.data.cost2.end());
            rhs.insert(rhs.end(), lp.data.rhs.begin(), lp.data.rhs.end());
            basis0.insert(basis0.end(), lp.cols.basis0.begin(), lp.cols.basis0.end());
            if (many->any_bounded) {  // (one entry per column of every LP, as `pos`: a plain LP's are not read)
                if (lp.bounded) ub.insert(ub.end(), lp.ub.begin(), lp.ub.end());
                else ub.insert(ub.end(), (size_t)lp.n, std::numeric_limits<double>::infinity());
            }
        }
        // launch order: by bucket, then the longest estimated solve first (ties: the caller's order)
        std::vector<int> order(n);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
            const ManyHostLP &a = many->lps[x], &b = many->lps[y];
            if (a.bucket != b.bucket) return a.bucket < b.bucket;
            return a.work > b.work;
        });
        many->order = order;
        for (int b = 0; b < MANY_GROUPS; ++b) {
            many->bucket_first[b + 1] = many->bucket_first[b];
            for (int k : order)
                if (many->lps[k].bucket == b) {
                    many->bucket_first[b + 1] += 1;
                    many->bucket_rows[b] = std::max(many->bucket_rows[b], many->lps[k].m);
                }
        }
        many->d_lps = many_upload(many->memory, desc);
        many->d_order = many_upload(many->memory, order);
        many->d_col_start = many_upload(many->memory, col_start);
        many->d_row_index = many_upload(many->memory, row_index);
        many->d_value = many_upload(many->memory, value);
        many->d_cost2 = many_upload(many->memory, cost2);
        many->d_rhs = many_upload(many->memory, rhs);
        many->d_basis0 = many_upload(many->memory, basis0);
        many->d_gamma = many->memory.alloc<double>(cost2.size());
        many->d_pos = many->memory.alloc<int>(cost2.size());
        if (many->any_bounded) {
            many->d_ub = many_upload(many->memory, ub);
            many->d_flipped = many->memory.alloc<int>(cost2.size());
        }
        many->d_inverse = many->memory.alloc<double>((size_t)inverse_words);
        many->d_basis_out = many->memory.alloc<int>(rhs.size());
        many->d_xb_out = many->memory.alloc<double>(rhs.size());
        many->d_out = many->memory.alloc<ManyOut>((size_t)n);
        for (hipStream_t& s : many->streams) RELP_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        RELP_HIP(hipEventCreate(&many->ev_start));
        RELP_HIP(hipEventCreate(&many->ev_stop));
        for (hipEvent_t& e : many->ev_done) RELP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        static PerDeviceOnce once;
        allow_full_lds_once(once, &many_kernel<true, false>, &many_kernel<true, true>);
    } catch (const DeviceError& e) {
        many_set_error(error, error_capacity, e.what());
        many->release();
        return RELP_ERR_DEVICE;
    } catch (const std::exception& e) {
        many_set_error(error, error_capacity, e.what());
        many->release();
        return RELP_ERR_STATE;
    }
    *out = many.release();
    return RELP_OK;
}

int32_t relp_many_solve(relp_many* many, relp_many_result* results, double* kernel_seconds) {
    if (!many) return RELP_ERR_ARGUMENT;
    try {
        RELP_HIP(hipSetDevice(many->device));
        const relp_options& o = many->options;
        const int n = (int)many->lps.size();
        ManyArgs args;
        args.lps = many->d_lps;
        args.order = many->d_order;
        args.col_start = many->d_col_start;
        args.row_index = many->d_row_index;
        args.value = many->d_value;
        args.cost2 = many->d_cost2;
        args.rhs = many->d_rhs;
        args.basis0 = many->d_basis0;
        args.gamma = many->d_gamma;
        args.pos = many->d_pos;
        args.ub = many->d_ub;
        args.flipped = many->d_flipped;
        args.inverse = many->d_inverse;
        args.basis_out = many->d_basis_out;
        args.xb_out = many->d_xb_out;
        args.out = many->d_out;
        args.rule = o.pivot_rule;
        args.polish_period = o.polish_period;
        args.tol_dual = o.tol_dual;
        args.tol_pivot = o.tol_pivot;
        args.harris_delta = o.harris_delta;
        args.tol_feasible = o.tol_feasible;
        RELP_HIP(hipEventRecord(many->ev_start, many->streams[0]));
        for (int t = 0; t < MANY_TIERS; ++t) {  // a stream per tier: its plain group, then its bounded group
            hipStream_t s = many->streams[t];
            if (t > 0) RELP_HIP(hipStreamWaitEvent(s, many->ev_start, 0));
            for (int b : {t, t + MANY_TIERS}) {
                const int blocks = many->bucket_first[b + 1] - many->bucket_first[b];
                if (blocks == 0) continue;
                ManyArgs part = args;
                part.order = many->d_order + many->bucket_first[b];
                const bool lds = t < 3, bounded = b >= MANY_TIERS;
                const size_t bytes = many_lds_bytes(many->bucket_rows[b], lds, bounded);
                if (lds && bounded) hipLaunchKernelGGL((many_kernel<true, true>), dim3(blocks), dim3(MANY_THREADS), bytes, s, part);
                else if (lds) hipLaunchKernelGGL((many_kernel<true, false>), dim3(blocks), dim3(MANY_THREADS), bytes, s, part);
                else if (bounded) hipLaunchKernelGGL((many_kernel<false, true>), dim3(blocks), dim3(MANY_THREADS), bytes, s, part);
                else hipLaunchKernelGGL((many_kernel<false, false>), dim3(blocks), dim3(MANY_THREADS), bytes, s, part);
                check_launch("many_kernel");
            }
            if (t > 0) {
                RELP_HIP(hipEventRecord(many->ev_done[t], s));
                RELP_HIP(hipStreamWaitEvent(many->streams[0], many->ev_done[t], 0));
            }
        }
        RELP_HIP(hipEventRecord(many->ev_stop, many->streams[0]));
        RELP_HIP(hipEventSynchronize(many->ev_stop));
        float ms = 0.f;
        RELP_HIP(hipEventElapsedTime(&ms, many->ev_start, many->ev_stop));
        if (kernel_seconds) *kernel_seconds = ms * 1e-3;
        std::vector<ManyOut> outs(n);
        const size_t rows = many->lps.empty() ? 0 : (size_t)std::accumulate(many->lps.begin(), many->lps.end(), 0, [](int s, const ManyHostLP& lp) { return s + lp.m; });
        std::vector<int> basis(rows);
        std::vector<double> xb(rows);
        RELP_HIP(hipMemcpy(outs.data(), many->d_out, n * sizeof(ManyOut), hipMemcpyDeviceToHost));
        RELP_HIP(hipMemcpy(basis.data(), many->d_basis_out, rows * sizeof(int), hipMemcpyDeviceToHost));
        RELP_HIP(hipMemcpy(xb.data(), many->d_xb_out, rows * sizeof(double), hipMemcpyDeviceToHost));
        std::vector<int> all_pos, all_flipped;  // implicit bounds: per column of every LP
        if (many->any_bounded) {
            size_t columns = 0;
            for (const ManyHostLP& lp : many->lps) columns += (size_t)lp.n;
            all_pos.resize(columns);
            all_flipped.resize(columns);
            RELP_HIP(hipMemcpy(all_pos.data(), many->d_pos, columns * sizeof(int), hipMemcpyDeviceToHost));
            RELP_HIP(hipMemcpy(all_flipped.data(), many->d_flipped, columns * sizeof(int), hipMemcpyDeviceToHost));
        }
        many->bound_flips.assign(n, 0);
        many->results.assign(n, relp_many_result{});
        many->bases.assign(n, std::vector<int>());
        many->solutions.assign(n, std::vector<double>());
        many->exact.assign(n, std::string());
        many->entering.assign(n, -1);
        size_t r0 = 0, c0 = 0;
        for (int k = 0; k < n; ++k) {
            const ManyHostLP& lp = many->lps[k];
            const StandardForm& form = many->forms[k];
            const ManyOut& oc = outs[k];
            relp_many_result& res = many->results[k];
            res.status = oc.status;
            res.kind = oc.kind;
            res.inverse_in_lds = lp.lds;
            res.pivots_phase_one = oc.pivots_phase_one;
            res.pivots_phase_two = oc.pivots_phase_two;
            res.reinversions = oc.reinversions;
            res.max_residual = oc.max_residual;
            many->bound_flips[k] = oc.bound_flips;
            res.objective = (oc.status == RELP_OK && oc.kind == RELP_RESULT_FINITE_OPTIMUM) ? -oc.minus_obj + form.fixed_cost.to_double()
                                                                                           : std::nan("");
            // Carry::current_bfs + reconstruct_solution (carry/mod.rs:636-645, matrix_data.rs:402-411); device values are checked first
            std::vector<int>& provider_basis = many->bases[k];
            std::vector<double>& x = many->solutions[k];
            provider_basis.assign(lp.m, 0);
            x.assign(form.data.nr_columns(), 0.0);
            for (int i = 0; i < lp.m; ++i) {
                const int dev = basis[r0 + i];
                if (dev < 0 || dev >= lp.n) throw std::runtime_error("model " + std::to_string(k) + ": the device returned an invalid basis");
                provider_basis[i] = lp.cols.to_provider(dev);
                if (!lp.bounded && dev >= lp.n_art) x[dev - lp.n_art] = xb[r0 + i];
            }
            if (lp.bounded) {  // back to the reference's formulation, as a handle with implicit bounds reports it
                const std::vector<int> device_basis(basis.begin() + r0, basis.begin() + r0 + lp.m);
                const std::vector<int> pos(all_pos.begin() + c0, all_pos.begin() + c0 + lp.n);
                const std::vector<int> flipped(all_flipped.begin() + c0, all_flipped.begin() + c0 + lp.n);
                provider_basis = explicit_basis(form.data, lp.cols, device_basis, pos);
                explicit_solution(form.data, lp.cols, device_basis, xb.data() + r0, flipped, pos, lp.ub, x);
            }
            r0 += lp.m;
            c0 += lp.n;
            many->entering[k] = oc.entering;
            if (o.certify && many_serial_certificate_applies(*many, k)) {
                long long repairs = 0;
                many_serial_certificate(*many, k, &repairs);
            }
        }
        many->solved = true;
        many->certificate_digits.clear();
        many->witnesses.clear();
        many->witnesses_kept = false;
        if (results) std::copy(many->results.begin(), many->results.end(), results);
        return RELP_OK;
    } catch (const DeviceError& e) {
        many->error = e.what();
        return RELP_ERR_DEVICE;
    } catch (const std::exception& e) {
        many->error = e.what();
        return RELP_ERR_STATE;
    }
}

int32_t relp_many_certify_lds_rows(void) { return many_certify_lds_rows(); }

int32_t relp_many_certify(relp_many* many, int32_t mode, relp_many_certificate* out, double* device_seconds, double* wall_seconds) {
    if (device_seconds) *device_seconds = 0.0;
    if (wall_seconds) *wall_seconds = 0.0;
    // (`out` and its size first: nothing of the handle is read for a caller built against another header)
    if (!out || out[0].struct_size != (int32_t)sizeof(relp_many_certificate)) return RELP_ERR_ARGUMENT;  // (the one size this struct has had)
    if (mode != RELP_MANY_CERTIFY_OPTIMA && mode != RELP_MANY_CERTIFY_SERIAL && mode != RELP_MANY_CERTIFY_ALL_KINDS) return RELP_ERR_ARGUMENT;
    if (!many) return RELP_ERR_ARGUMENT;
    if (!many->solved) {
        many->error = "relp_many_certify needs the results of a relp_many_solve";
        return RELP_ERR_STATE;
    }
    try {
        const double t_begin = many_now();
        RELP_HIP(hipSetDevice(many->device));
        const int n = (int)many->lps.size();
        many->error.clear();
        for (int k = 0; k < n; ++k) {
            out[k] = relp_many_certificate{};
            out[k].struct_size = (int32_t)sizeof(relp_many_certificate);
            many->exact[k].clear();
            many->results[k].certified = 0;
        }
        many->certificate_digits.assign(n, std::array<int32_t, 3>{0, 0, 0});
        many->witnesses.clear();
        many->witnesses_kept = false;
        const bool keep = many->keep_witnesses;
        if (keep) many->witnesses.assign(n, nullptr);
        // the batched stage takes the optima, and in RELP_MANY_CERTIFY_ALL_KINDS the two other verdicts that have a certificate;
        // everything else that has one keeps the serial certificate
        std::vector<int> batched;
        std::vector<ManyCertifyItem> items;
        std::vector<ManyCertifyOutcome> outcomes;
        if (mode != RELP_MANY_CERTIFY_SERIAL) {
            for (int k = 0; k < n; ++k) {
                const bool optimum = many->results[k].status == RELP_OK && many->results[k].kind == RELP_RESULT_FINITE_OPTIMUM;
                if (!optimum && !(mode == RELP_MANY_CERTIFY_ALL_KINDS && many_serial_certificate_applies(*many, k))) continue;
                ManyCertifyItem item{&many->forms[k], &many->bases[k]};
                many_certificate_kind(*many, k, &item.mode, &item.ray);
                batched.push_back(k);
                items.push_back(item);
            }
            many_certify_batched(items, many->device, many->streams, &outcomes, device_seconds, keep);
        }
        std::vector<int> slot(n, -1);
        for (size_t s = 0; s < batched.size(); ++s) slot[batched[s]] = (int)s;
        for (int k = 0; k < n; ++k) {
            relp_many_certificate& c = out[k];
            if (!many_serial_certificate_applies(*many, k)) continue;  // path 0: nothing to prove
            if (slot[k] >= 0) {
                const ManyCertifyOutcome& oc = outcomes[slot[k]];
                c.fallback_reason = oc.reason;
                c.host_seconds = oc.host_seconds;
                if (oc.reason == MANY_CERTIFY_NONE) {
                    c.certified = 1;
                    c.path = 1;
                    c.digits_primal = oc.digits_primal;
                    c.digits_dual = oc.digits_dual;
                    many->certificate_digits[k] = {oc.digits_primal, oc.digits_dual, oc.digits_ray};
                    many->exact[k] = oc.objective;
                    many->results[k].certified = 1;
                    many->results[k].certify_seconds = oc.host_seconds;
                    if (keep) many->witnesses[k] = oc.witnesses;
                    continue;
                }
            } else if (mode == RELP_MANY_CERTIFY_OPTIMA) {
                c.fallback_reason = MANY_CERTIFY_KIND;
            }
            long long repairs = 0;
            c.certified = many_serial_certificate(*many, k, &repairs, keep ? &many->witnesses[k] : nullptr) ? 1 : 0;
            c.path = 2;
            c.repair_pivots = repairs;
            c.host_seconds += many->results[k].certify_seconds;
        }
        many->witnesses_kept = keep;
        if (wall_seconds) *wall_seconds = many_now() - t_begin;
        return RELP_OK;
    } catch (const DeviceError& e) {
        many->error = e.what();
        return RELP_ERR_DEVICE;
    } catch (const std::exception& e) {
        many->error = e.what();
        return RELP_ERR_STATE;
    }
}

int32_t relp_many_get_certificate_digits(const relp_many* many, int32_t model, int32_t digits[3]) {
    if (!many || !digits || model < 0 || model >= (int32_t)many->lps.size()) return RELP_ERR_ARGUMENT;
    if (!many->solved || many->certificate_digits.size() != many->lps.size()) return RELP_ERR_STATE;
    std::copy(many->certificate_digits[model].begin(), many->certificate_digits[model].end(), digits);
    return RELP_OK;
}

int32_t relp_many_keep_witnesses(relp_many* many, int32_t on) {
    if (!many || (on != 0 && on != 1)) return RELP_ERR_ARGUMENT;
    many->keep_witnesses = on == 1;
    return RELP_OK;
}

// The witnesses of model `model` when the last relp_many_certify kept them and certified it; else null with the reason in many.error.
static const ExactWitnesses* many_kept_witnesses(const relp_many* many, int32_t model) {
    std::string& error = const_cast<relp_many*>(many)->error;
    if (!many->solved || many->certificate_digits.size() != many->lps.size())
        error = "no exact witnesses: there is no relp_many_certify of the last relp_many_solve";
    else if (!many->witnesses_kept)
        error = "no exact witnesses: relp_many_keep_witnesses was off when relp_many_certify ran";
    else if (!many->witnesses[model] || !many->results[model].certified)
        error = "no exact witnesses: model " + std::to_string(model) + " is not certified";
    else
        return many->witnesses[model].get();
    return nullptr;
}

int32_t relp_many_get_witness_exact(const relp_many* many, int32_t model, int32_t which, int32_t capacity, int32_t* count, int32_t* index,
                                    char* buffer, int64_t buffer_capacity, int64_t* length) {
    if (!many || model < 0 || model >= (int32_t)many->lps.size() || !count || capacity < 0 || buffer_capacity < 0 ||
        which < RELP_WITNESS_PRIMAL || which > RELP_WITNESS_RAY)
        return RELP_ERR_ARGUMENT;
    const ExactWitnesses* kept = many_kept_witnesses(many, model);
    if (!kept) return RELP_ERR_STATE;
    const std::string refusal = witness_refusal(many->results[model].kind, which);
    if (!refusal.empty()) {
        const_cast<relp_many*>(many)->error = "model " + std::to_string(model) + ": " + refusal;
        return RELP_ERR_STATE;
    }
    try {
        return return_exact_values(exact_witness_values(*kept, which), capacity, count, index, buffer, buffer_capacity, length);
    } catch (const std::exception& e) {
        const_cast<relp_many*>(many)->error = e.what();
        return RELP_ERR_NUMERICAL;
    }
}

int32_t relp_many_get_solution_exact(const relp_many* many, int32_t model, int32_t original, int32_t capacity, int32_t* count, int32_t* index,
                                     char* buffer, int64_t buffer_capacity, int64_t* length) {
    if (!many || model < 0 || model >= (int32_t)many->lps.size() || !count || capacity < 0 || buffer_capacity < 0) return RELP_ERR_ARGUMENT;
    const ExactWitnesses* kept = many_kept_witnesses(many, model);
    if (!kept) return RELP_ERR_STATE;
    if (many->results[model].kind != RELP_RESULT_FINITE_OPTIMUM) {
        const_cast<relp_many*>(many)->error = "model " + std::to_string(model) + ": no exact solution (not a certified finite optimum)";
        return RELP_ERR_STATE;
    }
    try {
        const ExactValues values = exact_solution_values(many->forms[model], exact_witness_values(*kept, RELP_WITNESS_PRIMAL), original != 0);
        return return_exact_values(values, capacity, count, index, buffer, buffer_capacity, length);
    } catch (const std::exception& e) {
        const_cast<relp_many*>(many)->error = e.what();
        return RELP_ERR_NUMERICAL;
    }
}

int32_t relp_many_get_basis(const relp_many* many, int32_t model, int32_t* basis) {
    if (!many || !basis || model < 0 || model >= (int32_t)many->lps.size()) return RELP_ERR_ARGUMENT;
    if (!many->solved) return RELP_ERR_STATE;
    const std::vector<int>& b = many->bases[model];
    std::copy(b.begin(), b.end(), basis);
    return RELP_OK;
}

int32_t relp_many_get_solution(const relp_many* many, int32_t model, double* x_structural) {
    if (!many || !x_structural || model < 0 || model >= (int32_t)many->lps.size()) return RELP_ERR_ARGUMENT;
    if (!many->solved) return RELP_ERR_STATE;
    const int n_struct = many->forms[model].data.nr_normal_variables();
    for (int j = 0; j < n_struct; ++j) x_structural[j] = many->solutions[model][j];
    return RELP_OK;
}

int32_t relp_many_get_objective_exact(const relp_many* many, int32_t model, char* buffer, int32_t capacity, int32_t* length) {
    if (!many || model < 0 || model >= (int32_t)many->lps.size()) return RELP_ERR_ARGUMENT;
    const std::string s = many->solved ? many->exact[model] : std::string();
    if (length) *length = (int32_t)s.size();
    if (s.empty()) return RELP_ERR_STATE;
    if (buffer && capacity > 0) {
        const int32_t nbytes = std::min<int32_t>((int32_t)s.size(), capacity - 1);
        std::memcpy(buffer, s.data(), nbytes);
        buffer[nbytes] = 0;
    }
    return RELP_OK;
}

int32_t relp_many_dimensions(const relp_many* many, int32_t model, int32_t* nr_rows, int32_t* nr_structural) {
    if (!many || model < 0 || model >= (int32_t)many->lps.size()) return RELP_ERR_ARGUMENT;
    if (nr_rows) *nr_rows = many->forms[model].data.nr_rows();
    if (nr_structural) *nr_structural = many->forms[model].data.nr_normal_variables();
    return RELP_OK;
}

int32_t relp_many_get_bound_flips(const relp_many* many, int32_t model, int64_t* bound_flips) {
    if (!many || !bound_flips || model < 0 || model >= (int32_t)many->lps.size()) return RELP_ERR_ARGUMENT;
    if (!many->solved) return RELP_ERR_STATE;
    *bound_flips = many->bound_flips[model];
    return RELP_OK;
}

const char* relp_many_last_error(const relp_many* many) { return many ? many->error.c_str() : "null handle"; }

int32_t relp_many_free(relp_many* many) {
    if (!many) return RELP_ERR_ARGUMENT;
    many->release();
    delete many;
    return RELP_OK;
}

}  // extern "C"
