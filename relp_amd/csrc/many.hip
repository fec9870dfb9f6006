// Many small independent LPs in one launch, one workgroup per LP (relp_many_*, include/relp_amd.h).
//
// The `Solver` handle runs one LP as a device-wide pipeline (two or three kernels per pivot over the whole chip).  For an LP of a
// few dozen to a few hundred rows each pivot then costs the launch boundaries while nearly every CU is idle.  Here a workgroup owns
// one LP for its whole two-phase solve -- `solve_relaxation` of two_phase/mod.rs:25-109 with the loops of phase_one.rs:134-178 and
// phase_two.rs:36-58 -- inside ONE ordinary launch: no grid barrier, no cooperative launch, no communication between workgroups.
//
// Per LP the host builds what `Solver::upload` builds (the same `StandardForm` / `MatrixData`, artificial columns first, then the
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
// Two tiers of storage for B^-1 (f64, column-major, ld = m), one kernel source: `many_kernel<true>` keeps it in the workgroup's LDS,
// `many_kernel<false>` in a per-LP slab of global memory.  Everything else of the LP's state -- x_B, -pi, rho_p, w, alpha, the basis
// -- is in LDS in both.  Columns, costs, steepest-edge weights and column positions stay in global memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "solver.hpp"
#include "wave_ops.hpp"

namespace relp {

constexpr int MANY_THREADS = 512;
constexpr int MANY_WAVES = MANY_THREADS / WAVE;
constexpr int MANY_MAX_ROWS = 512;
constexpr size_t MANY_LDS_BYTES = 160 * 1024;        // a CU of gfx950
constexpr size_t MANY_STATIC_LDS = 1024;             // the kernel's __shared__ scalars (below), rounded up
constexpr double MANY_RESIDUAL_BOUND = 1e-6;         // max |B B^-1 - I| a fresh inversion must reach, else RELP_ERR_NUMERICAL
constexpr double MANY_ZERO_LEVEL_TOL = 1e-7;         // row scan of a zero-level pivot (as Solver::drive_out_artificials)

// Words (8 bytes) of the per-LP vectors in LDS: x_B, -pi, rho_p, w, alpha, then the basis and the pivot rows of the inversion
// (2 m ints), and in the LDS tier the m x m inverse.
__host__ __device__ constexpr size_t many_vector_words(int m) { return (size_t)6 * m; }
__host__ __device__ constexpr size_t many_lds_bytes(int m, bool inverse_in_lds) {
    return 8 * (many_vector_words(m) + (inverse_in_lds ? (size_t)m * m : 0));
}
// Largest m whose LDS tier fits a CU: 139 rows (139 x 139 x 8 + 6 x 139 x 8 = 161 240 bytes, plus the static part).
constexpr int many_lds_tier_rows() {
    int m = 1;
    while (m < MANY_MAX_ROWS && many_lds_bytes(m + 1, true) + MANY_STATIC_LDS <= MANY_LDS_BYTES) ++m;
    return m;
}
static_assert(many_lds_tier_rows() == 139, "the documented cut-off of the LDS tier");

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
    double* inverse;
    int* basis_out;
    double* xb_out;
    ManyOut* out;
    int rule;
    int polish_period;
    double tol_dual, tol_pivot, harris_delta, tol_feasible;
};

enum : int { MANY_PIVOTED = 0, MANY_NO_ENTERING = 1, MANY_UNBOUNDED = 2 };

template <bool LDS_INVERSE>
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
    double* inv = LDS_INVERSE ? smem + many_vector_words(m) : a.inverse + L.inv_off;
    const bool steepest = a.rule == RELP_PIVOT_STEEPEST_EDGE;
    const double slack = L.textbook ? 0.0 : a.harris_delta;

    int phase = n_art > 0 ? 1 : 2;
    auto cost = [&](int j) { return phase == 1 ? (j < n_art ? 1.0 : 0.0) : cost2[j]; };
    auto block_sum = [&](double v) { return block_reduce<0>(v, s_red); };
    auto block_max = [&](double v) { return -block_reduce<1>(-v, s_red); };

    // ---- Tableau::new over Partially (partially.rs:125-205): B = I, artificial k on its row, slack pivots on the others ----
    for (int j = tid; j < n; j += MANY_THREADS) pos[j] = -1;
    for (int i = tid; i < m; i += MANY_THREADS) {
        basis[i] = a.basis0[L.r_off + i];
        xb[i] = rhs[i];
        rho[i] = w[i] = 0.0;
    }
    __syncthreads();
    for (int i = tid; i < m; i += MANY_THREADS) pos[basis[i]] = i;
    for (int j = wave; j < m; j += MANY_WAVES)
        for (int i = lane; i < m; i += WAVE) inv[(size_t)j * ld + i] = i == j ? 1.0 : 0.0;
    __syncthreads();

    double minus_obj = 0.0, max_residual = 0.0;
    long long pivots[2] = {0, 0}, reinversions = 0, since = 0;
    int pending = 0, leaving = -1, status = RELP_OK, kind = RELP_RESULT_NONE, entering = -1, redundant = 0;
    double gamma_q = 1.0, alpha_pq = 1.0;

    // -pi = -c_B' B^-1 (pi_kernel) and the objective (cb_kernel), from the costs of the current phase
    auto refresh_pi = [&]() {
        for (int j = wave; j < m; j += MANY_WAVES) {
            double acc = 0.0;
            for (int i = lane; i < m; i += WAVE) acc += cost(basis[i]) * inv[(size_t)j * ld + i];
            acc = wave_sum(acc);
            if (lane == LAST) mpi[j] = -acc;
        }
        double v = 0.0;
        for (int i = tid; i < m; i += MANY_THREADS) v += xb[i] * cost(basis[i]);
        minus_obj = -block_sum(v);  // (its barriers publish -pi too)
    };
    // x_B = B^-1 b (xb_kernel)
    auto refresh_xb = [&]() {
        for (int i = tid; i < m; i += MANY_THREADS) {
            double acc = 0.0;
            for (int j = 0; j < m; ++j) acc += inv[(size_t)j * ld + i] * rhs[j];
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
                for (int e = cs[col]; e < cs[col + 1]; ++e) acc -= va[e] * inv[(size_t)ri[e] * ld + i];
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
            for (int e = cs[col] + lane; e < cs[col + 1]; e += WAVE) inv[(size_t)k * ld + ri[e]] = va[e];
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
    auto pivot = [&](int forced_q, int forced_p) -> int {
        double key = 0.0;
        unsigned long long rank = RANK_NONE;
        for (int j = n_art + tid; j < n; j += MANY_THREADS) {
            if (pos[j] != -1) continue;
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
            const double cbar = cost(j) + d_pi;
            double g = 1.0;
            if (steepest) {
                g = gamma[j];
                if (pending) {
                    if (j == leaving) {
                        g = gamma_q / (alpha_pq * alpha_pq);  // pivot_rule.rs:294-295
                    } else {
                        const double sq = d_rho * d_rho;  // pivot_rule.rs:262-288 (Goldfarb-Reid)
                        g = fmax(g - 2.0 * d_rho * d_w + sq * gamma_q, 1.0 + sq);
                    }
                    gamma[j] = g;
                }
            }
            if (cbar < -a.tol_dual) {
                // steepest edge: cbar^2 / gamma, ties to the larger column; Dantzig: -cbar, ties to the smaller one
                const double k = steepest ? cbar * cbar / g : -cbar;
                const unsigned long long r = steepest ? (unsigned long long)(0x7fffffff - j) : (unsigned long long)j;
                if (rank == RANK_NONE || k > key || (k == key && r < rank)) {
                    key = k;
                    rank = r;
                }
            }
        }
        pending = 0;
        block_argbest(key, rank, s_akey, s_arank);
        int q = forced_q;
        if (q < 0) {
            if (rank == RANK_NONE) return MANY_NO_ENTERING;
            q = steepest ? 0x7fffffff - (int)rank : (int)rank;
        }
        double cbar_q = cost(q);  // (every thread: the same sum in the same order as the pricing pass)
        for (int e = cs[q]; e < cs[q + 1]; ++e) cbar_q += va[e] * mpi[ri[e]];
        // FTRAN: alpha = B^-1 a_q
        double sumsq = 0.0, theta = INFINITY;
        for (int i = tid; i < m; i += MANY_THREADS) {
            double acc = 0.0;
            for (int e = cs[q]; e < cs[q + 1]; ++e) acc += inv[(size_t)ri[e] * ld + i] * va[e];
            alpha[i] = acc;
            sumsq += acc * acc;
            const bool eligible = acc > a.tol_pivot && !(phase == 2 && basis[i] < n_art);
            if (eligible) theta = fmin(theta, (fmax(xb[i], 0.0) + slack) / fabs(acc));
        }
        gamma_q = 1.0 + block_sum(sumsq);  // pivot_rule.rs:258
        const double theta_max = block_reduce<1>(theta, s_red);
        // Harris pass 2: the largest eligible pivot within theta_max (the textbook rule: every ratio at the minimum), ties by the
        // lowest leaving column, then the lowest row
        key = 0.0;
        rank = RANK_NONE;
        for (int i = tid; i < m; i += MANY_THREADS) {
            const double al = alpha[i];
            const bool eligible = al > a.tol_pivot && !(phase == 2 && basis[i] < n_art);
            const double mag = fabs(al);
            const double k = L.textbook ? 1.0 : mag;
            if (forced_p >= 0 ? i == forced_p : (eligible && fmax(xb[i], 0.0) / mag <= theta_max)) {
                const unsigned long long r = ((unsigned long long)(unsigned)basis[i] << 32) | (unsigned)i;
                if (rank == RANK_NONE || k > key || (k == key && r < rank)) {
                    key = k;
                    rank = r;
                }
            }
        }
        block_argbest(key, rank, s_akey, s_arank);
        if (rank == RANK_NONE) {
            entering = q;
            return MANY_UNBOUNDED;
        }
        const int p = (int)(rank & 0xffffffffu);
        alpha_pq = alpha[p];
        if (alpha_pq == 0.0) {
            entering = q;
            return MANY_UNBOUNDED;  // (a forced row whose element vanished: never from the ratio test, which needs alpha > tol_pivot)
        }
        leaving = basis[p];
        const double xp = fmax(xb[p], 0.0) / alpha_pq;
        __syncthreads();  // x_B[p] and basis[p] read by every thread
        for (int i = tid; i < m; i += MANY_THREADS) xb[i] = i == p ? xp : xb[i] - alpha[i] * xp;
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
            pos[q] = p;
            pos[leaving] = -1;
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
                if (pos[j] != -1) continue;
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

// One LP as the device sees it (the index space and the data a `Solver` with the explicit carry and no implicit bounds has), and
// what is this path's own: the tier, the launch group and the work estimate.
struct ManyHostLP {
    int m = 0, n = 0, n_art = 0, textbook = 0, lds = 0, bucket = 0;
    DeviceColumns cols;
    DeviceMatrix data;
    double work = 0.0;  // estimated solve time, for the launch order
};

ManyHostLP many_host_lp(const StandardForm& form, const relp_options& o) {
    ManyHostLP lp;
    lp.cols = DeviceColumns(form.data);
    lp.data = DeviceMatrix(lp.cols, form.data);
    const int m = lp.m = lp.cols.m, n = lp.n = lp.cols.n();
    lp.n_art = lp.cols.n_art;
    // RELP_RATIO_AUTO as Solver::upload resolves it (every LP here has at most 512 rows: the kernels have the textbook rule)
    lp.textbook = o.ratio_rule == RELP_RATIO_TEXTBOOK || (o.ratio_rule == RELP_RATIO_AUTO && lp.data.small_integer_data());
    lp.lds = m <= many_lds_tier_rows() && !(o.switches & RELP_SW_MANY_GLOBAL_TIER);
    // launch groups: three LDS sizes (7, 2 and 1 workgroups per CU) and the global tier
    lp.bucket = !lp.lds ? 3 : m <= 48 ? 0 : m <= 96 ? 1 : 2;
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
    ManyOut* d_out = nullptr;
    std::vector<int> order;           // LP indices, grouped by bucket, longest first within a bucket
    int bucket_first[5] = {0, 0, 0, 0, 0};
    int bucket_rows[4] = {0, 0, 0, 0};  // largest m of each bucket
    hipStream_t streams[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_start = nullptr, ev_stop = nullptr, ev_done[4] = {nullptr, nullptr, nullptr, nullptr};
    DeviceAllocations memory;  // every device array above
    CertifyScratch certify_scratch;
    // results of the last solve
    bool solved = false;
    std::vector<relp_many_result> results;
    std::vector<std::vector<int>> bases;      // provider codes (DeviceColumns::to_provider)
    std::vector<std::vector<double>> solutions;  // every column of MatrixData
    std::vector<std::string> exact;
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
    // every model is checked before the device is touched
    for (int32_t k = 0; k < n_models; ++k) {
        if (!models[k]) {
            many_set_error(error, error_capacity, "model " + std::to_string(k) + ": null");
            return RELP_ERR_ARGUMENT;
        }
        const int rows = models[k]->form.data.nr_rows();
        if (rows < 1 || rows > MANY_MAX_ROWS) {
            many_set_error(error, error_capacity, "model " + std::to_string(k) + ": " + std::to_string(rows) +
                                                      " rows in standard form; relp_many takes 1 to " + std::to_string(MANY_MAX_ROWS));
            return RELP_ERR_ARGUMENT;
        }
    }
    auto many = std::make_unique<relp_many>();
    many->options = adopted;
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
        for (int k = 0; k < n; ++k) many->lps.push_back(many_host_lp(many->forms[k], adopted));
        // pack: CSC, costs, right-hand sides, initial bases; per-LP offsets
        std::vector<ManyLP> desc(n);
        std::vector<int> col_start, row_index, basis0;
        std::vector<double> value, cost2, rhs;
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
        for (int b = 0; b < 4; ++b) {
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
        many->d_inverse = many->memory.alloc<double>((size_t)inverse_words);
        many->d_basis_out = many->memory.alloc<int>(rhs.size());
        many->d_xb_out = many->memory.alloc<double>(rhs.size());
        many->d_out = many->memory.alloc<ManyOut>((size_t)n);
        for (hipStream_t& s : many->streams) RELP_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        RELP_HIP(hipEventCreate(&many->ev_start));
        RELP_HIP(hipEventCreate(&many->ev_stop));
        for (hipEvent_t& e : many->ev_done) RELP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        static PerDeviceOnce once;
        once.run([] {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(&many_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(MANY_LDS_BYTES - MANY_STATIC_LDS)) != hipSuccess)
                (void)hipGetLastError();
        });
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
        for (int b = 0; b < 4; ++b) {
            const int blocks = many->bucket_first[b + 1] - many->bucket_first[b];
            hipStream_t s = many->streams[b];
            if (b > 0) RELP_HIP(hipStreamWaitEvent(s, many->ev_start, 0));
            if (blocks > 0) {
                ManyArgs part = args;
                part.order = many->d_order + many->bucket_first[b];
                const bool lds = b < 3;
                const size_t bytes = many_lds_bytes(many->bucket_rows[b], lds);
                if (lds) hipLaunchKernelGGL(many_kernel<true>, dim3(blocks), dim3(MANY_THREADS), bytes, s, part);
                else hipLaunchKernelGGL(many_kernel<false>, dim3(blocks), dim3(MANY_THREADS), bytes, s, part);
                RELP_HIP(hipGetLastError());
            }
            if (b > 0) {
                RELP_HIP(hipEventRecord(many->ev_done[b], s));
                RELP_HIP(hipStreamWaitEvent(many->streams[0], many->ev_done[b], 0));
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
        many->results.assign(n, relp_many_result{});
        many->bases.assign(n, std::vector<int>());
        many->solutions.assign(n, std::vector<double>());
        many->exact.assign(n, std::string());
        size_t r0 = 0;
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
                if (dev >= lp.n_art) x[dev - lp.n_art] = xb[r0 + i];
            }
            r0 += lp.m;
            if (o.certify && oc.status == RELP_OK &&
                (oc.kind == RELP_RESULT_FINITE_OPTIMUM || oc.kind == RELP_RESULT_INFEASIBLE || oc.kind == RELP_RESULT_UNBOUNDED)) {
                const double t0 = many_now();
                bool ok = false;
                long long repairs = 0;
                std::string message;
                const int mode = oc.kind == RELP_RESULT_INFEASIBLE ? 1 : oc.kind == RELP_RESULT_UNBOUNDED ? 2 : 0;
                const int ray = oc.kind == RELP_RESULT_UNBOUNDED && oc.entering >= lp.n_art && oc.entering < lp.n ? oc.entering - lp.n_art : -1;
                many->certify_scratch.statics.reset();  // (what it keeps belongs to one LP)
                many->certify_scratch.digit_hints[0] = many->certify_scratch.digit_hints[1] = 0;
                try {
                    certify_basis(form, provider_basis, many->device, many->streams[0], &many->exact[k], &ok, &repairs, &message, mode, ray,
                                  nullptr, &many->certify_scratch);
                } catch (const RatOverflow& e) {  // the f64 result stands, uncertified
                    ok = false;
                    message = std::string("exact certificate: ") + e.what();
                }
                if (!ok) {
                    many->exact[k].clear();
                    if (many->error.empty()) many->error = "model " + std::to_string(k) + ": " + message;
                }
                res.certified = ok ? 1 : 0;
                res.certify_seconds = many_now() - t0;
            }
        }
        many->solved = true;
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
    if (nr_rows) *nr_rows = many->lps[model].m;
    if (nr_structural) *nr_structural = many->forms[model].data.nr_normal_variables();
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
