// Dual simplex from a given dual-feasible basis: the five kernels of one dual pivot (gfx950, wave64), the two that keep the weights of
// the steepest-edge leaving rule, the kernel that starts a child LP from its parent's inverse, and their launch helpers.
//
// The primal kernels cannot leave a primal-infeasible basis (step_decision clamps the leaving value at zero), and the rules of
// pivot_step.hpp are shared with the fused pivot, so the dual loop is a set of kernels of its own over the same device state
// (dual.hpp).  The textbook method: the leaving row is the most infeasible one (or, as an option, the one with the largest
// x_B[i]^2 / |row i of the inverse|^2: dual steepest edge), the entering column the one whose relative cost
// reaches zero first along row p of the tableau, found by a two-pass ratio test of the same shape as the primal Harris test
// (pass 1: the largest dual step that keeps every relative cost above -tol_dual; pass 2: the largest |alpha_pj| within it).
// Candidates go through per-workgroup slots that one workgroup folds, as in the primal loop; no floating-point atomics, every
// reduction in a fixed order.
//
// Implicit upper bounds (DeviceLP::ub, the state the bounded primal kernels keep): the leave, row and pivot kernels have a BOUNDED
// instantiation each that states the same method on the held representation -- every column held as x_j or as u_j - x_j, a basic
// variable infeasible below 0 or above xub[i] -- and dual_choose_kernel and dual_update_kernel serve both, since they only see the
// signed row (abar_j, d_j) and the signed column alpha_q.  The instantiations without bounds are the kernels as they were.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "pivot_step.hpp"
#include "solver.hpp"
#include "wave_ops.hpp"

namespace relp {

namespace {

constexpr int DL_THREADS = 1024;      // the two single-workgroup kernels
constexpr int DL_U = 8;               // rows per thread in flight together (K2_U of ftran_ratio_kernel)
constexpr int DL_COL_CHUNK = 1024;    // entries of the entering column staged per pass
constexpr int DU_THREADS = 256;       // dual_update_kernel: four waves, a column pair each
constexpr int DU_CPW = 2;
constexpr int DI_THREADS = 256;       // dual_inherit_kernel: four waves, a column of the child's inverse each
constexpr int DW_THREADS = 256;       // dual_weights_kernel: four waves over one tile of 64 rows, a quarter of the slice's columns each
constexpr int DW_U = 16;              // its columns in flight per lane

// Implicit upper bounds: the side of a basic variable with the value x and the upper bound `up` (+inf: none).  +1: it is (or would be)
// infeasible below 0 and has to rise; -1: above `up` and has to fall.  The three BOUNDED kernels form it from x_B[p] and xub[p].
__device__ __forceinline__ double dual_side(double x, double up) { return x - up > -x ? -1.0 : 1.0; }

// ---------------------------------------------------------------------------------------------------
// 1. The leaving row: key = -x_B[i] among the rows with x_B[i] < -delta, ties to the lowest basic column, then the lowest row.
//    Then rho = row p of the inverse (m strided loads of the column-major inverse, as btran_vec_kernel does for a unit vector).
//    Also the budget check of the chain: the four kernels behind this one only look at the status.
// ---------------------------------------------------------------------------------------------------
//    STEEPEST (relp_options.dual_pricing = RELP_DUAL_PRICING_STEEPEST_EDGE): key = x_B[i]^2 / beta[i] among the same rows, the same ties.
//    The instantiation of rule 0 never reads `beta`: its instructions are those of the kernel before the second rule existed.
//    BOUNDED: the violation of row i is v_i = max(-x_B[i], x_B[i] - xub[i]) (xub = +inf: no upper side), the rows with v_i > delta are
//    eligible, key v_i or v_i^2 / beta[i].  The side of the leaving row is not stored: dual_side of (x_B[p], xub[p]), which no kernel
//    writes between this one and dual_pivot_kernel.
//    CUTOFF (Solver::set_dual_cutoff): in front of the budget check, so before anything is scanned, the objective of the basis the chain
//    stands on -- dual feasible, so a lower bound of the LP -- against `cutoff_carry`, the caller's cutoff less the fixed cost: reached,
//    the chain stops with ST_CUTOFF and Ctl::p is left alone.  Uniform: every thread reads the same control block.  The instantiations
//    without it never read `cutoff_carry`: their instructions are those of the kernel before the cutoff existed.
template <bool STEEPEST, bool BOUNDED, bool CUTOFF>
__global__ void __launch_bounds__(DL_THREADS) dual_leave_kernel(DeviceLP lp, double delta, const double* __restrict__ beta, double cutoff_carry) {
    __shared__ double s_key[DL_THREADS / WAVE];
    __shared__ unsigned long long s_rank[DL_THREADS / WAVE];
    Ctl* ctl = lp.ctl;
    if (ctl->status != ST_RUNNING) return;
    if constexpr (CUTOFF) {
        if (-ctl->minus_obj >= cutoff_carry) {
            if (threadIdx.x == 0) {
                ctl->status = ST_CUTOFF;
                ctl->pending = 0;
            }
            return;
        }
    }
    if (ctl->iters >= ctl->budget) {
        if (threadIdx.x == 0) ctl_budget(*ctl);
        return;
    }
    const int m = lp.m, ld = lp.ld;
    double key = 0.0;
    unsigned long long rank = RANK_NONE;
    for (int i0 = threadIdx.x; i0 < m; i0 += DL_U * DL_THREADS) {
        double xbv[DL_U], betav[DL_U], upv[DL_U];
        int basv[DL_U];
#pragma unroll
        for (int u = 0; u < DL_U; ++u) {
            const int i = i0 + u * DL_THREADS;
            xbv[u] = i < m ? lp.xB[i] : 0.0;
            basv[u] = i < m ? lp.basis[i] : 0;
            if (STEEPEST) betav[u] = i < m ? beta[i] : 1.0;
            if (BOUNDED) upv[u] = i < m ? lp.xub[i] : INFINITY;
        }
#pragma unroll
        for (int u = 0; u < DL_U; ++u) {
            const int i = i0 + u * DL_THREADS;
            if constexpr (BOUNDED) {
                const double v = fmax(-xbv[u], xbv[u] - upv[u]);
                if (i < m && v > delta) keep_better(STEEPEST ? v * v / betav[u] : v, leaving_rank(basv[u], i), key, rank);
            } else {
                if (i < m && xbv[u] < -delta) keep_better(STEEPEST ? xbv[u] * xbv[u] / betav[u] : -xbv[u], leaving_rank(basv[u], i), key, rank);
            }
        }
    }
    block_argbest<true>(key, rank, s_key, s_rank);  // (the first use of the slots)
    const int p = leaving_row(rank);
    if (p < 0) {  // primal feasible
        if (threadIdx.x == 0) {
            ctl->status = ST_NO_ENTERING;
            ctl->pending = 0;
        }
        return;
    }
    for (int j0 = threadIdx.x; j0 < m; j0 += DL_U * DL_THREADS) {
        double v[DL_U];
#pragma unroll
        for (int u = 0; u < DL_U; ++u) {
            const int j = j0 + u * DL_THREADS;
            v[u] = j < m ? lp.Binv[(size_t)j * ld + p] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < DL_U; ++u) {
            const int j = j0 + u * DL_THREADS;
            if (j < m) lp.rho[j] = v[u];
        }
    }
    if (threadIdx.x == 0) ctl->p = p;
}

// ---------------------------------------------------------------------------------------------------
// 2. Row p of the tableau and the relative costs over the provider columns, one lane per column, in one pass over its entries:
//    alpha_pj = sum v rho[r], d_j = c_j + sum v (-pi)[r] (the sum of reduced_cost_of, in its order).  A basic column stores
//    alpha_pj = 0 and is never eligible.  Pass 1 of the ratio test over the columns with alpha_pj < -tol_pivot: the workgroup's
//    minimum of (max(d_j, 0) + slack) / |alpha_pj|.  LDS: rho and -pi staged in 2 m doubles of dynamic LDS.
// ---------------------------------------------------------------------------------------------------
template <bool LDS>
__global__ void __launch_bounds__(DUAL_COLUMNS_PER_BLOCK) dual_row_kernel(DeviceLP lp, DualBuffers b, double tol_pivot, double slack) {
    extern __shared__ __attribute__((aligned(16))) double s_vectors[];
    __shared__ __attribute__((aligned(16))) double s_red[DUAL_COLUMNS_PER_BLOCK / WAVE + 2];
    if (lp.ctl->status != ST_RUNNING) return;
    const int m = lp.m;
    const double* rho = lp.rho;
    const double* minus_pi = lp.minus_pi;
    if (LDS) {
        for (int i = threadIdx.x; i < m; i += DUAL_COLUMNS_PER_BLOCK) {
            s_vectors[i] = lp.rho[i];
            s_vectors[m + i] = lp.minus_pi[i];
        }
        __syncthreads();
        rho = s_vectors;
        minus_pi = s_vectors + m;
    }
    const int j = lp.n_art + blockIdx.x * DUAL_COLUMNS_PER_BLOCK + threadIdx.x;
    double theta = INFINITY;
    if (j < lp.n) {
        double a = 0.0, dj = 0.0;
        if (lp.pos[j] < 0) {
            dj = lp.cost[j];
            const int first = lp.col_start[j], last = lp.col_start[j + 1];
            for (int e = first; e < last; ++e) {
                const int r = lp.row_index[e];
                const double v = lp.value[e];
                dj += v * minus_pi[r];
                a += v * rho[r];
            }
            if (a < -tol_pivot) theta = (fmax(dj, 0.0) + slack) / fabs(a);
        }
        b.alpha_row[j] = a;
        b.d[j] = dj;
    }
    theta = block_reduce<1>(theta, s_red);
    if (threadIdx.x == 0) b.part_theta[blockIdx.x] = theta;
}

// The same on implicit upper bounds, a kernel of its own (as a second template parameter it changed the order of two instructions of
// the kernel above): over the columns with pos -1 or -2 (a fixed column, pos -3, is never priced), in the held form and towards the
// side s of the leaving row: abar_j = s sgn_j (rho . a_j), d_j = sgn_j (c_j + sum v (-pi)[r]) -- the same sums in the same order, one
// lane per column, multiplied by +-1 after them.  flipped[j] is loaded beside pos[j]; the side comes from two uniform loads behind
// Ctl::p that are on their way while rho and -pi are staged.
template <bool LDS>
__global__ void __launch_bounds__(DUAL_COLUMNS_PER_BLOCK) dual_row_bounded_kernel(DeviceLP lp, DualBuffers b, double tol_pivot, double slack) {
    extern __shared__ __attribute__((aligned(16))) double s_vectors[];
    __shared__ __attribute__((aligned(16))) double s_red[DUAL_COLUMNS_PER_BLOCK / WAVE + 2];
    if (lp.ctl->status != ST_RUNNING) return;
    const int m = lp.m;
    const int p = lp.ctl->p;
    const double side = dual_side(lp.xB[p], lp.xub[p]);
    const double* rho = lp.rho;
    const double* minus_pi = lp.minus_pi;
    if (LDS) {
        for (int i = threadIdx.x; i < m; i += DUAL_COLUMNS_PER_BLOCK) {
            s_vectors[i] = lp.rho[i];
            s_vectors[m + i] = lp.minus_pi[i];
        }
        __syncthreads();
        rho = s_vectors;
        minus_pi = s_vectors + m;
    }
    const int j = lp.n_art + blockIdx.x * DUAL_COLUMNS_PER_BLOCK + threadIdx.x;
    double theta = INFINITY;
    if (j < lp.n) {
        double a = 0.0, dj = 0.0;
        const int position = lp.pos[j];
        const int complemented = lp.flipped[j];
        if (position == -1 || position == -2) {
            dj = lp.cost[j];
            const int first = lp.col_start[j], last = lp.col_start[j + 1];
            for (int e = first; e < last; ++e) {
                const int r = lp.row_index[e];
                const double v = lp.value[e];
                dj += v * minus_pi[r];
                a += v * rho[r];
            }
            const double sgn = complemented ? -1.0 : 1.0;
            dj *= sgn;
            a *= sgn * side;
            if (a < -tol_pivot) theta = (fmax(dj, 0.0) + slack) / fabs(a);
        }
        b.alpha_row[j] = a;
        b.d[j] = dj;
    }
    theta = block_reduce<1>(theta, s_red);
    if (threadIdx.x == 0) b.part_theta[blockIdx.x] = theta;
}

// ---------------------------------------------------------------------------------------------------
// 2b. The long-step (bound-flipping) ratio test, an option of the loop on implicit bounds: one workgroup between the row kernel (either
//    variant) and dual_choose_kernel.  Along the dual ray of row p the slope of the dual objective is the violation delta = v_p; it
//    drops by ub_j |abar_j| at the ratio of every boxed candidate j, because that column can go to its other bound instead of
//    entering.  The candidates (abar_j < -tol_pivot) in the order (max(d_j, 0) / |abar_j|, j): the walk passes a candidate while the
//    slope behind it stays above harris_delta -- row p is then still a row dual_leave_kernel would call violated, on the same side --
//    and ends at one without a bound, at the last candidate of all, at the first that would take the slope to harris_delta or below,
//    and after DUAL_MAX_FLIPS passed ones (every prefix of the order that keeps the slope positive is a legal flip set).
//    The boxed candidates are compacted into LDS (ratio, ub_j |abar_j|, j; the slots in no fixed order, which no result depends on:
//    every choice below is a minimum under the total order (ratio, j)), the candidates without a bound only give their smallest
//    (ratio, j).  Then one round per passed candidate: the workgroup's arg-min over the unmarked slots, the tests above, the mark.
//    F is short (1 to 3 columns on the test family), so peeling beats a sort.  Out: flip_count[0] = |F|, flip_j in walk order,
//    alpha_row[j] = 0 on F ("not eligible" to dual_choose_kernel and to the pass below) and part_theta rewritten -- slot 0 = pass 1
//    over the candidates outside F, the other slots +inf --, so that dual_choose_kernel and the pivot kernel choose the entering
//    column outside F by their own rule.  Nothing of DeviceLP is written: the flips are applied by dual_pivot_kernel<true, true>
//    behind its guard.  More boxed candidates than slots: F is empty for this pivot (the plain rule) and flip_count[1] = 1 says so.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DL_THREADS) dual_long_step_kernel(DeviceLP lp, DualBuffers b, double tol_pivot, double slack, double harris_delta) {
    __shared__ double s_key[DL_THREADS / WAVE];
    __shared__ unsigned long long s_rank[DL_THREADS / WAVE];
    __shared__ double s_red[DL_THREADS / WAVE + 2];
    __shared__ double s_ratio[DUAL_LONG_STEP_SLOTS];
    __shared__ double s_drop[DUAL_LONG_STEP_SLOTS];  // ub_j |abar_j|: what the slope loses when j is passed
    __shared__ int s_col[DUAL_LONG_STEP_SLOTS];      // j, -1 once passed
    __shared__ int s_count[2];                       // boxed candidates, candidates without a bound
    if (lp.ctl->status != ST_RUNNING) return;
    const int p = lp.ctl->p;
    const double x_p = lp.xB[p], up_p = lp.xub[p];
    if (threadIdx.x < 2) s_count[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        b.flip_count[0] = 0;
        b.flip_count[1] = 0;
    }
    __syncthreads();
    double free_key = 0.0;  // the first candidate without a bound: the largest -ratio, ties to the lowest column
    unsigned long long free_rank = RANK_NONE;
    for (int j0 = lp.n_art + threadIdx.x; j0 < lp.n; j0 += DL_U * DL_THREADS) {
        double av[DL_U], dv[DL_U], widthv[DL_U];  // DL_U columns per thread in flight together: one round trip up to 8192 columns
#pragma unroll
        for (int u = 0; u < DL_U; ++u) {
            const int j = j0 + u * DL_THREADS;
            av[u] = j < lp.n ? b.alpha_row[j] : 0.0;
            dv[u] = j < lp.n ? b.d[j] : 0.0;
            widthv[u] = j < lp.n ? lp.ub[j] : INFINITY;
        }
#pragma unroll
        for (int u = 0; u < DL_U; ++u) {
            const int j = j0 + u * DL_THREADS;
            if (!(av[u] < -tol_pivot)) continue;  // (a column past the end has alpha 0)
            const double mag = fabs(av[u]), ratio = fmax(dv[u], 0.0) / mag;
            if (widthv[u] < INFINITY) {
                const int slot = atomicAdd(&s_count[0], 1);  // (an integer counter in LDS; the slot order is free, see above)
                if (slot < DUAL_LONG_STEP_SLOTS) {
                    s_ratio[slot] = ratio;
                    s_drop[slot] = widthv[u] * mag;
                    s_col[slot] = j;
                }
            } else {
                atomicAdd(&s_count[1], 1);
                keep_better(-ratio, (unsigned long long)(unsigned)j, free_key, free_rank);
            }
        }
    }
    block_argbest<true>(free_key, free_rank, s_key, s_rank);  // (the slots' first use; its barrier also publishes s_count and the slots)
    const int boxed = s_count[0], candidates = boxed + s_count[1];
    if (boxed == 0) return;
    if (boxed > DUAL_LONG_STEP_SLOTS) {
        if (threadIdx.x == 0) b.flip_count[1] = 1;
        return;
    }
    double slope = fmax(-x_p, x_p - up_p);
    int passed = 0;
    while (passed < DUAL_MAX_FLIPS && passed + 1 < candidates) {  // (the last candidate of all is never passed: it enters)
        double key = 0.0;
        unsigned long long rank = RANK_NONE;
        for (int e = threadIdx.x; e < boxed; e += DL_THREADS) {
            const int j = s_col[e];
            if (j >= 0) keep_better(-s_ratio[e], ((unsigned long long)(unsigned)j << 32) | (unsigned)e, key, rank);
        }
        block_argbest(key, rank, s_key, s_rank);
        if (rank == RANK_NONE) break;
        const int j = (int)(rank >> 32), e = (int)(rank & 0xffffffffu);
        if (free_rank != RANK_NONE && (free_key > key || (free_key == key && (int)free_rank < j))) break;  // a candidate without a bound comes first
        const double behind = slope - s_drop[e];
        if (!(behind > harris_delta)) break;
        if (threadIdx.x == 0) {  // (every thread scanned s_col in front of block_argbest's barriers)
            s_col[e] = -1;
            b.flip_j[passed] = j;
            b.alpha_row[j] = 0.0;
        }
        slope = behind;
        passed += 1;
        __syncthreads();  // the mark, and alpha_row[j] = 0, for every thread
    }
    if (passed == 0) return;
    double theta = INFINITY;
    for (int j0 = lp.n_art + threadIdx.x; j0 < lp.n; j0 += DL_U * DL_THREADS) {
        double av[DL_U], dv[DL_U];
#pragma unroll
        for (int u = 0; u < DL_U; ++u) {
            const int j = j0 + u * DL_THREADS;
            av[u] = j < lp.n ? b.alpha_row[j] : 0.0;
            dv[u] = j < lp.n ? b.d[j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < DL_U; ++u)
            if (av[u] < -tol_pivot) theta = fmin(theta, (fmax(dv[u], 0.0) + slack) / fabs(av[u]));
    }
    theta = block_reduce<1>(theta, s_red);
    for (int k = threadIdx.x; k < b.blocks; k += DL_THREADS) b.part_theta[k] = k == 0 ? theta : INFINITY;
    if (threadIdx.x == 0) b.flip_count[0] = passed;
}

// ---------------------------------------------------------------------------------------------------
// 3. theta_max = the minimum of the partial minima (every workgroup folds them itself, in the same order), then pass 2: among the
//    eligible columns with max(d_j, 0) / |alpha_pj| <= theta_max the largest |alpha_pj| (key 1 under the textbook rule), ties to the
//    lowest column.  One candidate per workgroup.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DUAL_COLUMNS_PER_BLOCK) dual_choose_kernel(DeviceLP lp, DualBuffers b, double tol_pivot, int textbook) {
    __shared__ double s_red[DUAL_COLUMNS_PER_BLOCK / WAVE + 2];
    __shared__ double s_key[DUAL_COLUMNS_PER_BLOCK / WAVE];
    __shared__ unsigned long long s_rank[DUAL_COLUMNS_PER_BLOCK / WAVE];
    if (lp.ctl->status != ST_RUNNING) return;
    double theta = INFINITY;
    for (int k = threadIdx.x; k < b.blocks; k += DUAL_COLUMNS_PER_BLOCK) theta = fmin(theta, b.part_theta[k]);
    const double theta_max = block_reduce<1>(theta, s_red);
    const int j = lp.n_art + blockIdx.x * DUAL_COLUMNS_PER_BLOCK + threadIdx.x;
    double key = 0.0;
    unsigned long long rank = RANK_NONE;
    if (j < lp.n) {
        const double a = b.alpha_row[j];
        if (a < -tol_pivot) {
            const double mag = fabs(a);
            if (fmax(b.d[j], 0.0) / mag <= theta_max) {
                key = textbook ? 1.0 : mag;
                rank = (unsigned long long)(unsigned)j;
            }
        }
    }
    block_argbest<true>(key, rank, s_key, s_rank);  // (the slots' first use; block_reduce has its own)
    if (threadIdx.x == 0) {
        b.cand_j[blockIdx.x] = rank == RANK_NONE ? -1 : (int)rank;
        b.cand_key[blockIdx.x] = key;
    }
}

// ---------------------------------------------------------------------------------------------------
// 4. The entering column q from the candidates (none: the dual is unbounded, the LP infeasible), alpha_q = Binv a_q with the column
//    staged through LDS as in ftran_ratio_kernel, the check that alpha_q[p] agrees with the row's value (ST_REFACTOR otherwise),
//    then the step theta = x_B[p] / alpha_q[p] -- the FTRAN value of the pivot, used
//    below and by the update of the inverse alike --, x_B, basis, pos and the control block.
// ---------------------------------------------------------------------------------------------------
//    BOUNDED: alpha_q = Binv (sgn_q a_q); the pivot is usable when s alpha_q[p] < -tol_pivot; theta = (x_B[p] - bound) / alpha_q[p] with
//    bound = 0 or xub[p] by the side s.  A column that leaves at its upper bound is held complemented from then on (rhs moves over
//    its entries as in ftran_ratio_kernel; exchange_columns of pivot_step.hpp); one of width 0 gets pos -3 and never enters again.
//    The entering value may exceed ub[q]: that is an infeasible row for a later pivot.
//    LONG (BOUNDED only; the long-step ratio test, behind dual_long_step_kernel): the columns of the flip set F go to their other bound
//    in the same launch, behind the same guard.  In front of the barrier, where nothing but scratch is written: w = Binv Delta with
//    Delta = sum over F of ub_j sgn_j a_j, one column after the other in flip order through the staging of the entering column, into
//    DualBuffers::flip_w.  Behind the guard: theta = (x_B[p] - w[p] - bound) / alpha_q[p], x_B = (x_B - w) - theta alpha_q in the one
//    pass, rhs -= Delta column by column, the complement marks of F, flip_cost, the objective and the two totals.  With F empty
//    every value is the one the instantiation without LONG computes (x - 0 is x).
template <bool BOUNDED, bool LONG = false>
__global__ void __launch_bounds__(DL_THREADS) dual_pivot_kernel(DeviceLP lp, DualBuffers b, double tol_pivot) {
    static_assert(BOUNDED || !LONG, "the long step flips boxed columns: implicit bounds only");
    __shared__ double s_key[DL_THREADS / WAVE];
    __shared__ unsigned long long s_rank[DL_THREADS / WAVE];
    __shared__ int s_rows[DL_COL_CHUNK];
    __shared__ double s_vals[DL_COL_CHUNK];
    __shared__ double s_pivot[BOUNDED ? (LONG ? 4 : 3) : 2];  // alpha_q[p], x_B[p], (xub[p]), (w[p])
    __shared__ int s_flip_j[LONG ? DUAL_MAX_FLIPS : 1];          // LONG: the flip set and ub_j sgn_j of each, read here in front of
    __shared__ double s_flip_scale[LONG ? DUAL_MAX_FLIPS : 1];   // the barrier: flipped[j] is rewritten at the end
    Ctl* ctl = lp.ctl;
    if (ctl->status != ST_RUNNING) return;
    const int m = lp.m, ld = lp.ld;
    const int p = ctl->p;
    double key = 0.0;
    unsigned long long rank = RANK_NONE;
    for (int k = threadIdx.x; k < b.blocks; k += DL_THREADS) {
        const int j = b.cand_j[k];
        if (j >= 0) keep_better(b.cand_key[k], (unsigned long long)(unsigned)j, key, rank);
    }
    block_argbest<true>(key, rank, s_key, s_rank);  // (the first use of the slots)
    if (rank == RANK_NONE) {
        if (threadIdx.x == 0) {
            ctl->status = ST_UNBOUNDED;
            ctl->q = -1;
            ctl->p = -1;
            ctl->pending = 0;
        }
        return;
    }
    const int q = (int)rank;
    const int ca = lp.col_start[q], cb = lp.col_start[q + 1];
    const bool single = (cb - ca) <= DL_COL_CHUNK;
    double sgn_q = 1.0, ub_q = INFINITY;
    if constexpr (BOUNDED) {
        sgn_q = lp.flipped[q] ? -1.0 : 1.0;
        ub_q = lp.ub[q];
    }
    if (!single)
        for (int i = threadIdx.x; i < m; i += DL_THREADS) lp.alpha[i] = 0.0;
    for (int c0 = ca; c0 < cb; c0 += DL_COL_CHUNK) {
        const int cnt = min(DL_COL_CHUNK, cb - c0);
        __syncthreads();
        for (int e = threadIdx.x; e < cnt; e += DL_THREADS) {
            s_rows[e] = lp.row_index[c0 + e];
            s_vals[e] = lp.value[c0 + e];
        }
        __syncthreads();
        for (int i0 = threadIdx.x; i0 < m; i0 += DL_U * DL_THREADS) {
            double acc[DL_U];
#pragma unroll
            for (int u = 0; u < DL_U; ++u) {
                const int i = i0 + u * DL_THREADS;
                acc[u] = (!single && i < m) ? lp.alpha[i] : 0.0;
            }
            for (int e = 0; e < cnt; ++e) {
                const size_t off = (size_t)s_rows[e] * ld;
                const double v = s_vals[e];
#pragma unroll
                for (int u = 0; u < DL_U; ++u) {
                    const int i = i0 + u * DL_THREADS;
                    if (i < m) acc[u] += lp.Binv[off + i] * v;
                }
            }
#pragma unroll
            for (int u = 0; u < DL_U; ++u) {
                const int i = i0 + u * DL_THREADS;
                if constexpr (BOUNDED) {
                    // (the sign of the held column goes on after the last chunk's sum, not per chunk)
                    if (i < m) lp.alpha[i] = c0 + DL_COL_CHUNK >= cb ? acc[u] * sgn_q : acc[u];
                } else {
                    if (i < m) lp.alpha[i] = acc[u];  // (read again below by the thread that wrote it)
                }
            }
        }
    }
    int flips = 0;
    if constexpr (LONG) {
        flips = min(b.flip_count[0], DUAL_MAX_FLIPS);
        if (flips > 0) {
            if ((int)threadIdx.x < flips) {
                const int j = b.flip_j[threadIdx.x];
                s_flip_j[threadIdx.x] = j;
                s_flip_scale[threadIdx.x] = lp.ub[j] * (lp.flipped[j] ? -1.0 : 1.0);
            }
            for (int i = threadIdx.x; i < m; i += DL_THREADS) b.flip_w[i] = 0.0;  // (read again below by the thread that wrote it)
            __syncthreads();
            for (int f = 0; f < flips; ++f) {
                const int j = s_flip_j[f];
                const double scale = s_flip_scale[f];
                const int fa = lp.col_start[j], fb = lp.col_start[j + 1];
                for (int c0 = fa; c0 < fb; c0 += DL_COL_CHUNK) {
                    const int cnt = min(DL_COL_CHUNK, fb - c0);
                    __syncthreads();
                    for (int e = threadIdx.x; e < cnt; e += DL_THREADS) {
                        s_rows[e] = lp.row_index[c0 + e];
                        s_vals[e] = lp.value[c0 + e] * scale;
                    }
                    __syncthreads();
                    for (int i0 = threadIdx.x; i0 < m; i0 += DL_U * DL_THREADS) {
                        double acc[DL_U];
#pragma unroll
                        for (int u = 0; u < DL_U; ++u) {
                            const int i = i0 + u * DL_THREADS;
                            acc[u] = i < m ? b.flip_w[i] : 0.0;
                        }
                        for (int e = 0; e < cnt; ++e) {
                            const size_t off = (size_t)s_rows[e] * ld;
                            const double v = s_vals[e];
#pragma unroll
                            for (int u = 0; u < DL_U; ++u) {
                                const int i = i0 + u * DL_THREADS;
                                if (i < m) acc[u] += lp.Binv[off + i] * v;
                            }
                        }
#pragma unroll
                        for (int u = 0; u < DL_U; ++u) {
                            const int i = i0 + u * DL_THREADS;
                            if (i < m) b.flip_w[i] = acc[u];
                        }
                    }
                }
            }
        }
    }
    if ((p % DL_THREADS) == (int)threadIdx.x) {  // the thread that owns row p
        s_pivot[0] = lp.alpha[p];
        s_pivot[1] = lp.xB[p];
        if constexpr (BOUNDED) s_pivot[2] = lp.xub[p];
        if constexpr (LONG) s_pivot[3] = flips > 0 ? b.flip_w[p] : 0.0;
    }
    // BOUNDED: what thread 0 rewrites at the end -- basis[p], flipped[leaving] -- is read by every thread here, in front of this barrier
    int leaving = 0, leaving_flipped = 0, leaving_first = 0, leaving_last = 0;
    if constexpr (BOUNDED) {
        leaving = lp.basis[p];
        leaving_flipped = lp.flipped[leaving];
        leaving_first = lp.col_start[leaving];
        leaving_last = lp.col_start[leaving + 1];
    }
    __syncthreads();
    if constexpr (BOUNDED) {
        const double alpha_pq = s_pivot[0], x_p = s_pivot[1], up_p = s_pivot[2];
        const double side = dual_side(x_p, up_p);
        if (!(side * alpha_pq < -tol_pivot)) {  // (as below: nothing has been written)
            if (threadIdx.x == 0) {
                ctl->status = ST_REFACTOR;
                ctl->pending = 0;
            }
            return;
        }
        const bool leaves_at_upper = side < 0.0;
        double theta = (leaves_at_upper ? x_p - up_p : x_p) / alpha_pq;
        if constexpr (LONG) theta = ((leaves_at_upper ? x_p - up_p : x_p) - s_pivot[3]) / alpha_pq;  // (row p after the flips: still violated, on the same side)
        for (int i0 = threadIdx.x; i0 < m; i0 += DL_U * DL_THREADS) {
            double av[DL_U], xbv[DL_U], wv[DL_U];
#pragma unroll
            for (int u = 0; u < DL_U; ++u) {
                const int i = i0 + u * DL_THREADS;
                av[u] = i < m ? lp.alpha[i] : 0.0;
                xbv[u] = i < m ? lp.xB[i] : 0.0;
                if constexpr (LONG) wv[u] = (flips > 0 && i < m) ? b.flip_w[i] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < DL_U; ++u) {
                const int i = i0 + u * DL_THREADS;
                if constexpr (LONG) {
                    if (i < m) lp.xB[i] = i == p ? theta : (xbv[u] - wv[u]) - theta * av[u];
                } else {
                    if (i < m) lp.xB[i] = i == p ? theta : xbv[u] - theta * av[u];
                }
            }
        }
        if constexpr (LONG) {
            // rhs -= Delta, a column of F after the other (two of them may share a row), each as a column that leaves at its upper
            // bound moves it below; then the marks, one thread per column of F (no column of F is q or the leaving one)
            for (int f = 0; f < flips; ++f) {
                const int j = s_flip_j[f];
                const double scale = s_flip_scale[f];
                const int fb = lp.col_start[j + 1];
                for (int e = lp.col_start[j] + (int)threadIdx.x; e < fb; e += DL_THREADS) lp.rhs[lp.row_index[e]] -= scale * lp.value[e];
                __syncthreads();
            }
            if ((int)threadIdx.x < flips) {
                const int j = s_flip_j[threadIdx.x];
                const int now_flipped = s_flip_scale[threadIdx.x] < 0.0 ? 0 : 1;
                lp.flipped[j] = now_flipped;
                lp.pos[j] = now_flipped ? -2 : -1;
            }
        }
        if (leaves_at_upper) {  // the leaving variable stops at its upper bound: held in complemented form from now on
            const double sgn_l = leaving_flipped ? -1.0 : 1.0;
            for (int e = leaving_first + (int)threadIdx.x; e < leaving_last; e += DL_THREADS) lp.rhs[lp.row_index[e]] -= up_p * sgn_l * lp.value[e];
        }
        if (threadIdx.x == 0) {
            if constexpr (LONG) {  // the objective moves by sum d_j ub_j over F, d_j as priced at this pivot; flip_cost as in ctl_bound_flip
                double moved = 0.0, shift = 0.0;
                for (int f = 0; f < flips; ++f) {
                    const int j = s_flip_j[f];
                    const double scale = s_flip_scale[f];
                    moved += b.d[j] * fabs(scale);
                    shift += scale * lp.cost[j];  // (+ub_j c_j for a column that is complemented now, - for one that is not any more)
                }
                if (flips > 0) {
                    ctl->minus_obj = ctl->minus_obj - moved;
                    ctl->flip_cost += shift;
                }
                b.flip_count[2] += flips;
                b.flip_count[3] += b.flip_count[1];
            }
            const double d_q = b.d[q];
            lp.basis[p] = q;
            const int fl = exchange_columns(lp.pos, lp.flipped, lp.xub, true, q, p, leaving, leaving_flipped, leaves_at_upper, ub_q);
            if (leaves_at_upper) ctl->flip_cost += (fl ? 1.0 : -1.0) * up_p * lp.cost[leaving];
            if (lp.ub[leaving] == 0.0) lp.pos[leaving] = -3;  // both bounds are the same point: never priced again
            ctl->q = q;
            ctl->leaving = leaving;
            ctl->alpha_pq = alpha_pq;
            ctl->cbar_q = d_q;
            ctl->xp = theta;
            ctl->minus_obj = ctl->minus_obj - d_q * theta;
            ctl->iters = ctl->iters + 1;
            ctl->pending = 0;
        }
        return;
    }
    const double alpha_pq = s_pivot[0];
    // The column was chosen on rho_p . a_q < -tol_pivot; the FTRAN value is the same number through the other side of the inverse.
    // Where the two disagree -- the FTRAN value is no usable pivot of that sign -- the inverse has drifted: x_B, the basis and the inverse
    // are still untouched, the chain stops with ST_REFACTOR and the host polishes the inverse and asks again (Solver::iterate_dual).
    if (!(alpha_pq < -tol_pivot)) {
        if (threadIdx.x == 0) {
            ctl->status = ST_REFACTOR;
            ctl->pending = 0;
        }
        return;
    }
    const double theta = s_pivot[1] / alpha_pq;
    for (int i0 = threadIdx.x; i0 < m; i0 += DL_U * DL_THREADS) {
        double av[DL_U], xbv[DL_U];
#pragma unroll
        for (int u = 0; u < DL_U; ++u) {
            const int i = i0 + u * DL_THREADS;
            av[u] = i < m ? lp.alpha[i] : 0.0;
            xbv[u] = i < m ? lp.xB[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < DL_U; ++u) {
            const int i = i0 + u * DL_THREADS;
            if (i < m) lp.xB[i] = i == p ? theta : xbv[u] - theta * av[u];
        }
    }
    if (threadIdx.x == 0) {
        const int leaving = lp.basis[p];
        const double d_q = b.d[q];
        lp.basis[p] = q;
        lp.pos[q] = p;
        lp.pos[leaving] = -1;
        ctl->q = q;
        ctl->leaving = leaving;
        ctl->alpha_pq = alpha_pq;
        ctl->cbar_q = d_q;
        ctl->xp = theta;
        ctl->minus_obj = ctl->minus_obj - d_q * theta;
        ctl->iters = ctl->iters + 1;
        ctl->pending = 0;  // the steepest-edge weights are not maintained here: set_phase(2) recomputes them
    }
}

// ---------------------------------------------------------------------------------------------------
// 5. The inverse and -pi, a wave per pair of columns, rows coalesced: with r = c[p] / alpha_pq (row p of the new inverse),
//    c[i] -= alpha_q[i] r for i != p, c[p] = r, (-pi)[j] -= d_q r.  A column with c[p] == 0 exactly does not change.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DU_THREADS) dual_update_kernel(DeviceLP lp) {
    const Ctl* ctl = lp.ctl;
    if (ctl->status != ST_RUNNING) return;  // (still running behind dual_pivot_kernel: it has pivoted)
    const int m = lp.m, ld = lp.ld;
    const int p = ctl->p;
    const double alpha_pq = ctl->alpha_pq, d_q = ctl->cbar_q;
    const int lane = threadIdx.x & (WAVE - 1);
    const int j0 = (blockIdx.x * (DU_THREADS / WAVE) + threadIdx.x / WAVE) * DU_CPW;
    double r[DU_CPW];
#pragma unroll
    for (int c = 0; c < DU_CPW; ++c) r[c] = j0 + c < m ? lp.Binv[(size_t)(j0 + c) * ld + p] / alpha_pq : 0.0;
    if (r[0] == 0.0 && r[1] == 0.0) return;
    for (int i = lane; i < m; i += WAVE) {
        const double a = lp.alpha[i];
#pragma unroll
        for (int c = 0; c < DU_CPW; ++c) {
            if (r[c] == 0.0) continue;
            double* column = lp.Binv + (size_t)(j0 + c) * ld;
            column[i] = i == p ? r[c] : column[i] - a * r[c];
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < DU_CPW; ++c)
            if (r[c] != 0.0) lp.minus_pi[j0 + c] -= d_q * r[c];
    }
}

// ---------------------------------------------------------------------------------------------------
// The weights of the steepest-edge rule, beta_i = sum_j Binv[i, j]^2, from the column-major inverse in its first buffer.  Workgroup
// (tile, slice): rows 64 tile .. 64 tile + 63, a lane per row in each of the four waves, so every load of a wave is 64 consecutive
// doubles of one column (8-byte accesses: ld need not be even, see dual_inherit_kernel); columns [slice per_slice, (slice + 1)
// per_slice) of the m, a contiguous quarter per wave, DW_U loads in flight, the squares added in column order; then the four quarters
// in wave order through LDS.  One partial sum per (slice, row) at out[slice m + row]; with one slice `out` is beta itself, otherwise
// dual_weights_fold_kernel adds the slices in slice order.  Every sum in a fixed order and no atomics: the same bits at every run.
// `chained`: behind the launches of a pivot, a no-op unless the chain is still running, like them.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DW_THREADS) dual_weights_kernel(DeviceLP lp, double* __restrict__ out, int per_slice, int chained) {
    __shared__ double s_quarter[DW_THREADS / WAVE][WAVE];
    if (chained && lp.ctl->status != ST_RUNNING) return;
    const int m = lp.m, ld = lp.ld;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int row = blockIdx.x * WAVE + lane;
    const int per_wave = (per_slice + DW_THREADS / WAVE - 1) / (DW_THREADS / WAVE);
    const int slice_end = min(m, ((int)blockIdx.y + 1) * per_slice);
    const int first = min(slice_end, (int)blockIdx.y * per_slice + wave * per_wave), last = min(slice_end, first + per_wave);
    double sum = 0.0;
    if (row < m) {
        const double* entry = lp.Binv + row;
        for (int j0 = first; j0 < last; j0 += DW_U) {
            double v[DW_U];
#pragma unroll
            for (int u = 0; u < DW_U; ++u) v[u] = j0 + u < last ? entry[(size_t)(j0 + u) * ld] : 0.0;
#pragma unroll
            for (int u = 0; u < DW_U; ++u) sum += v[u] * v[u];  // (a column past the end adds +0: the sum is never negative)
        }
    }
    s_quarter[wave][lane] = sum;
    __syncthreads();
    if (wave == 0 && row < m) {
        double total = s_quarter[0][lane];
#pragma unroll
        for (int w = 1; w < DW_THREADS / WAVE; ++w) total += s_quarter[w][lane];
        out[(size_t)blockIdx.y * m + row] = total;
    }
}

__global__ void __launch_bounds__(DW_THREADS) dual_weights_fold_kernel(DeviceLP lp, const double* __restrict__ part, double* __restrict__ beta, int slices, int chained) {
    if (chained && lp.ctl->status != ST_RUNNING) return;
    const int m = lp.m;
    const int row = blockIdx.x * DW_THREADS + threadIdx.x;
    if (row >= m) return;
    double v[DUAL_WEIGHT_SLICES_MAX];  // every slice's partial sum in flight together, then added in slice order
#pragma unroll
    for (int s = 0; s < DUAL_WEIGHT_SLICES_MAX; ++s) v[s] = s < slices ? part[(size_t)s * m + row] : 0.0;
    double total = v[0];
#pragma unroll
    for (int s = 1; s < DUAL_WEIGHT_SLICES_MAX; ++s) total += v[s];  // (a slice past the last adds +0: the sum is never negative)
    beta[row] = total;
}

// ---------------------------------------------------------------------------------------------------
// The start from a parent's inverse (dual_inherit.hpp): the child's basis is the parent's in the first m positions and the slack of
// each of the k appended rows behind it, so its inverse is [B^-1 0; -S^-1 C B^-1  S^-1].  A wave per column j of the child's inverse.
//   j <  m: rows 0 .. m-1 are column j of the parent's inverse (lanes over rows, both sides coalesced; the leading dimensions differ
//           and neither need be even, so 8-byte accesses); then a lane per new row r, in rounds of 64: over the entries of row m + r
//           in CSR order whose column is basic at a position below m,  -(sum v parent[pos[col], j]) / s_r  with s_r the entry of the
//           row's own slack (the column at position m + r).  A fixed order, no atomics; a long cut makes its lane's loop long.
//   j >= m: the unit column scaled by 1 / s_{j-m}.
// Every entry of the child's first buffer is written: nothing is left from an earlier use of it.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DI_THREADS) dual_inherit_kernel(DeviceLP lp, const double* __restrict__ parent, int m, int parent_ld) {
    const int m_child = lp.m, ld = lp.ld;
    const int lane = threadIdx.x & (WAVE - 1);
    const int j = blockIdx.x * (DI_THREADS / WAVE) + threadIdx.x / WAVE;
    if (j >= m_child) return;
    double* out = lp.Binv + (size_t)j * ld;
    if (j < m) {
        const double* src = parent + (size_t)j * parent_ld;
        for (int i = lane; i < m; i += WAVE) out[i] = src[i];
        for (int row = m + lane; row < m_child; row += WAVE) {
            double sum = 0.0, own = 0.0;
            const int last = lp.row_start[row + 1];
            for (int e = lp.row_start[row]; e < last; ++e) {
                const int p = lp.pos[lp.col_index[e]];
                const double v = lp.row_value[e];
                if (p == row) own = v;
                else if (p >= 0 && p < m) sum += v * src[p];
            }
            out[row] = -sum / own;
        }
    } else {
        double own = 0.0;  // (every lane walks the row: the same addresses, one fetch per wave)
        const int last = lp.row_start[j + 1];
        for (int e = lp.row_start[j]; e < last; ++e)
            if (lp.pos[lp.col_index[e]] == j) own = lp.row_value[e];
        const double diagonal = 1.0 / own;
        for (int i = lane; i < m_child; i += WAVE) out[i] = i == j ? diagonal : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------
// The same start between two LPs held on implicit upper bounds (dual_bounded_inherit_refusal, dual_inherit.hpp): the child's basic
// columns are the parent's and the slack of each appended row, but at other positions and some of them complemented on one side only,
// so the identity map of dual_inherit_kernel becomes (src, sg): position i of the child holds what the parent holds at position
// src[i] >= 0, with the sign sg[i] = sgn_parent * sgn_child between the two held forms, or the slack of new row m + rho where
// src[i] = -1 - rho.  Row i of the child's inverse is sg[i] times row src[i] of the parent's, the row of a new slack is the border
// row -(sum v sgn_col inv_child[pos[col], j]) / s_r over the entries of its row in CSR order whose column is basic at an inherited
// position (sgn_col from the child's `flipped`, +1 after place_basis, and s_r the signed entry of the slack itself).  A wave per column
// j of the child's inverse, lanes over positions; the gather through src stays inside column j of the parent (8-byte accesses: neither
// leading dimension need be even).  A fixed order, no atomics; every entry of the child's first buffer is written.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DI_THREADS) dual_inherit_mapped_kernel(DeviceLP lp, const double* __restrict__ parent, int m, int parent_ld,
                                                                         const int* __restrict__ src, const int* __restrict__ sg) {
    const int m_child = lp.m, ld = lp.ld;
    const int lane = threadIdx.x & (WAVE - 1);
    const int j = blockIdx.x * (DI_THREADS / WAVE) + threadIdx.x / WAVE;
    if (j >= m_child) return;
    double* out = lp.Binv + (size_t)j * ld;
    if (j < m) {
        const double* column = parent + (size_t)j * parent_ld;
        for (int i = lane; i < m_child; i += WAVE) {
            const int from = src[i];
            if (from >= 0) {
                out[i] = (double)sg[i] * column[from];
                continue;
            }
            const int row = m - 1 - from;  // the slack of new row m + rho sits here
            double sum = 0.0, own = 0.0;
            const int last = lp.row_start[row + 1];
            for (int e = lp.row_start[row]; e < last; ++e) {
                const int c = lp.col_index[e];
                const int p = lp.pos[c];
                if (p < 0) continue;
                const double v = lp.flipped && lp.flipped[c] ? -lp.row_value[e] : lp.row_value[e];
                if (p == i) own = v;
                else if (src[p] >= 0) sum += v * ((double)sg[p] * column[src[p]]);  // (what the lane of position p writes, bit for bit)
            }
            out[i] = -sum / own;
        }
    } else {
        const int rho = j - m;
        double own = 0.0;  // (every lane walks the row: the same addresses, one fetch per wave)
        const int last = lp.row_start[j + 1];
        for (int e = lp.row_start[j]; e < last; ++e) {
            const int c = lp.col_index[e];
            const int p = lp.pos[c];
            if (p >= 0 && src[p] == -1 - rho) own = lp.flipped && lp.flipped[c] ? -lp.row_value[e] : lp.row_value[e];
        }
        const double diagonal = 1.0 / own;
        for (int i = lane; i < m_child; i += WAVE) out[i] = src[i] == -1 - rho ? diagonal : 0.0;
    }
}

}  // namespace

void launch_dual_inherit_mapped(const DeviceLP& child, const double* parent_inverse, int parent_m, int parent_ld, const int* src, const int* sg, hipStream_t s) {
    const int per_block = DI_THREADS / WAVE;
    hipLaunchKernelGGL(dual_inherit_mapped_kernel, dim3((child.m + per_block - 1) / per_block), dim3(DI_THREADS), 0, s, child, parent_inverse, parent_m, parent_ld,
                       src, sg);
}
void launch_dual_inherit(const DeviceLP& child, const double* parent_inverse, int parent_m, int parent_ld, hipStream_t s) {
    const int per_block = DI_THREADS / WAVE;
    hipLaunchKernelGGL(dual_inherit_kernel, dim3((child.m + per_block - 1) / per_block), dim3(DI_THREADS), 0, s, child, parent_inverse, parent_m, parent_ld);
}
void launch_dual_leave(const DeviceLP& d, double harris_delta, const double* beta, bool bounded, bool cutoff, double cutoff_carry, hipStream_t s) {
    auto kernel = cutoff ? (beta ? (bounded ? dual_leave_kernel<true, true, true> : dual_leave_kernel<true, false, true>)
                                 : (bounded ? dual_leave_kernel<false, true, true> : dual_leave_kernel<false, false, true>))
                         : (beta ? (bounded ? dual_leave_kernel<true, true, false> : dual_leave_kernel<true, false, false>)
                                 : (bounded ? dual_leave_kernel<false, true, false> : dual_leave_kernel<false, false, false>));
    hipLaunchKernelGGL(kernel, dim3(1), dim3(DL_THREADS), 0, s, d, harris_delta, beta, cutoff_carry);
}
int launch_dual_weights(const DeviceLP& d, const DualBuffers& b, bool chained, hipStream_t s) {
    const int m = d.m, per_slice = (m + b.slices - 1) / b.slices;
    hipLaunchKernelGGL(dual_weights_kernel, dim3((m + WAVE - 1) / WAVE, b.slices), dim3(DW_THREADS), 0, s, d, b.slices == 1 ? b.beta : b.beta_part, per_slice, chained ? 1 : 0);
    if (b.slices == 1) return 1;
    hipLaunchKernelGGL(dual_weights_fold_kernel, dim3((m + DW_THREADS - 1) / DW_THREADS), dim3(DW_THREADS), 0, s, d, b.beta_part, b.beta, b.slices, chained ? 1 : 0);
    return 2;
}
void launch_dual_row(const DeviceLP& d, const DualBuffers& b, bool lds, bool bounded, double tol_pivot, double slack, hipStream_t s) {
    static PerDeviceOnce once, once_bounded;  // more than 64 KB of dynamic LDS is an opt-in, per device and kernel
    if (bounded) allow_full_lds_once(once_bounded, &dual_row_bounded_kernel<true>);
    else allow_full_lds_once(once, &dual_row_kernel<true>);
    auto kernel = lds ? (bounded ? dual_row_bounded_kernel<true> : dual_row_kernel<true>) : (bounded ? dual_row_bounded_kernel<false> : dual_row_kernel<false>);
    hipLaunchKernelGGL(kernel, dim3(b.blocks), dim3(DUAL_COLUMNS_PER_BLOCK), lds ? 2 * (size_t)d.m * sizeof(double) : 0, s, d, b, tol_pivot, slack);
}
void launch_dual_choose(const DeviceLP& d, const DualBuffers& b, double tol_pivot, bool textbook, hipStream_t s) {
    hipLaunchKernelGGL(dual_choose_kernel, dim3(b.blocks), dim3(DUAL_COLUMNS_PER_BLOCK), 0, s, d, b, tol_pivot, textbook ? 1 : 0);
}
void launch_dual_long_step(const DeviceLP& d, const DualBuffers& b, double tol_pivot, double slack, double harris_delta, hipStream_t s) {
    hipLaunchKernelGGL(dual_long_step_kernel, dim3(1), dim3(DL_THREADS), 0, s, d, b, tol_pivot, slack, harris_delta);
}
void launch_dual_pivot(const DeviceLP& d, const DualBuffers& b, bool bounded, bool long_step, double tol_pivot, hipStream_t s) {
    if (bounded && long_step) hipLaunchKernelGGL((dual_pivot_kernel<true, true>), dim3(1), dim3(DL_THREADS), 0, s, d, b, tol_pivot);
    else if (bounded) hipLaunchKernelGGL(dual_pivot_kernel<true>, dim3(1), dim3(DL_THREADS), 0, s, d, b, tol_pivot);
    else hipLaunchKernelGGL(dual_pivot_kernel<false>, dim3(1), dim3(DL_THREADS), 0, s, d, b, tol_pivot);
}
void launch_dual_update(const DeviceLP& d, hipStream_t s) {
    const int waves = (d.m + DU_CPW - 1) / DU_CPW, per_block = DU_THREADS / WAVE;
    hipLaunchKernelGGL(dual_update_kernel, dim3((waves + per_block - 1) / per_block), dim3(DU_THREADS), 0, s, d);
}

}  // namespace relp
