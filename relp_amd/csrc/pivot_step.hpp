// The primal ratio test and the bookkeeping of a pivot, stated ONCE for every f64 kernel that makes one (kernels.hip: ftran_ratio_kernel,
// k2l_*, ftran_ratio_fast_kernel, pivot_fused_kernel; lu.hip: lu_pivot_kernel; many.hip: many_kernel; network_carry.hip through k2l_*).
//   restates  Tableau::select_primal_pivot_row                     tableau/mod.rs:287-313
//             Carry::update_b and the basis bookkeeping            carry/mod.rs:295-325,561-604
// The kernels keep what is theirs -- where alpha, x_B and the basis live, how they loop over the rows, their barriers and reductions --
// and take the rules from here.  Everything is __forceinline__ and `bounded` folds away where the caller passes a constant.
//
// The ratio test is the two-pass Harris variant (f64 needs a pivot-size preference the exact reference does not): pass 1 finds the
// largest step theta_max that leaves every basic variable within `slack` of its bound, pass 2 takes the largest |alpha_i| among the
// rows whose own ratio is within theta_max.  harris_delta < 0 selects the reference's test instead: the exact minimum ratio (slack 0,
// every row at the minimum has key 1).  Ties go to the lowest leaving column (Bland, tableau/mod.rs:295), then the lowest row.
// Implicit upper bounds (DeviceLP::ub): a basic variable may also leave at its upper bound -- rows with alpha_i < 0 whose basic
// variable has one -- and the entering variable may run into its own bound first (a "bound flip", no basis change).  A variable at
// its upper bound is held in complemented form, so its column enters with the opposite sign.
#pragma once
#include "device_lp.hpp"
#include "wave_ops.hpp"

namespace relp {

// ---- candidates: (key, rank), the larger key wins, ties to the smaller rank (entering columns: price_step.hpp) ------------------
__device__ __forceinline__ void keep_better(double key, unsigned long long rank, double& best_key, unsigned long long& best_rank) {
    if (best_rank == RANK_NONE || key > best_key || (key == best_key && rank < best_rank)) {
        best_key = key;
        best_rank = rank;
    }
}
// leaving row: the lowest basic column, then the lowest row
__device__ __forceinline__ unsigned long long leaving_rank(int basic_column, int row) {
    return ((unsigned long long)(unsigned)basic_column << 32) | (unsigned)row;
}
__device__ __forceinline__ int leaving_row(unsigned long long rank) { return rank == RANK_NONE ? -1 : (int)(rank & 0xffffffffu); }

// ---- the rules ------------------------------------------------------------------------------------------------------------------
struct HarrisRule {
    bool textbook;
    double slack;
};
__device__ __forceinline__ HarrisRule harris_rule(double harris_delta) {
    HarrisRule h;
    h.textbook = harris_delta < 0.0;
    h.slack = h.textbook ? 0.0 : harris_delta;
    return h;
}
// Row i may block the step when it is `allowed` (not an artificial row being skipped) and alpha_i is a usable pivot in the direction
// its basic variable moves.  `room`: the distance of that variable to the bound it moves towards.  `xub` is a callable, so that the
// row's upper bound is only fetched where the rule looks at it.
struct RowRoom {
    bool eligible;
    double room;
};
template <class Xub>
__device__ __forceinline__ RowRoom row_room(double a, double x, Xub xub, bool allowed, bool bounded, double tol_pivot) {
    RowRoom r;
    r.room = fmax(x, 0.0);
    r.eligible = allowed && a > tol_pivot;
    if (bounded && allowed && a < -tol_pivot) {
        const double up = xub();
        if (up < INFINITY) {
            r.eligible = true;
            r.room = fmax(up - x, 0.0);
        }
    }
    return r;
}
__device__ __forceinline__ double harris_pass1(double room, double slack, double a) { return (room + slack) / fabs(a); }
__device__ __forceinline__ bool harris_accepts(double room, double mag, double theta_max) { return room / mag <= theta_max; }
__device__ __forceinline__ double harris_key(bool textbook, double mag) { return textbook ? 1.0 : mag; }

// Step length -- to the bound of the leaving variable, or (forced zero-level pivots, phase_one.rs:232-278) as the reference computes
// it -- and what happens: the leaving variable stops at its upper bound `ub_leaving` = x_p + room_p, or the entering variable
// reaches its own bound ub_q first (`flip`).  p < 0: no row blocks.
struct Step {
    double xp;
    bool leaves_at_upper, flip;
    double ub_leaving;
};
__device__ __forceinline__ Step step_decision(bool bounded, bool forced, int p, double alpha_pq, double x_p, double room_p, double ub_q) {
    Step s;
    s.xp = (forced || !bounded) ? fmax(x_p, 0.0) / alpha_pq : room_p / fabs(alpha_pq);
    s.leaves_at_upper = bounded && !forced && p >= 0 && alpha_pq < 0.0;
    s.flip = bounded && !forced && ub_q < INFINITY && (p < 0 || ub_q <= s.xp);
    s.ub_leaving = x_p + room_p;
    return s;
}

// ---- the bookkeeping (one thread) -----------------------------------------------------------------------------------------------
// Column positions: -1 non-basic at 0 | -2 non-basic at its upper bound, held complemented.  Plain pointers: many_kernel keeps them in LDS.
// Bound flip: x_q ran from 0 to ub_q and is complemented so that it sits at 0 again.  Returns whether q is complemented now.
__device__ __forceinline__ int flip_column(int* pos, int* flipped, int q, double sgn_q) {
    const int now_flipped = sgn_q < 0.0 ? 0 : 1;
    flipped[q] = now_flipped;
    pos[q] = now_flipped ? -2 : -1;
    return now_flipped;
}
// Basis change at row p.  Returns whether the leaving column is complemented now (it is from now on when it left at its upper bound).
__device__ __forceinline__ int exchange_columns(int* pos, int* flipped, double* xub, bool bounded, int q, int p, int leaving,
                                                int leaving_flipped, bool leaves_at_upper, double ub_q) {
    pos[q] = p;
    int fl = 0;
    if (bounded) {
        fl = leaving_flipped;
        if (leaves_at_upper) flipped[leaving] = fl ^= 1;
        xub[p] = ub_q;
    }
    pos[leaving] = fl ? -2 : -1;
    return fl;
}

// The control block: against a Ctl&, so that the kernels that edit *lp.ctl in place and the fused kernel (a local copy, stored to
// the other state) share them.  `mode` as in ftran_ratio_kernel: 0 full iteration | 1 entering column only | 2 ratio test only.
__device__ __forceinline__ void ctl_budget(Ctl& c) {
    c.status = ST_BUDGET;
    c.pending = 0;
}
__device__ __forceinline__ void ctl_no_entering(Ctl& c, int mode) {
    if (mode == 0) c.status = ST_NO_ENTERING;
    c.q = -1;
    c.pending = 0;
    if (mode == 0) c.last_selected = -1;
}
__device__ __forceinline__ void ctl_entering_only(Ctl& c, int q, double cbar_q) {
    c.q = q;
    c.cbar_q = cbar_q;
    c.pending = 0;
}
__device__ __forceinline__ void ctl_unbounded(Ctl& c, int q, int mode) {
    if (mode == 0) c.status = ST_UNBOUNDED;
    c.q = q;
    c.p = -1;
    c.pending = 0;
    c.forced_q = -1;
    c.forced_p = -1;
}
__device__ __forceinline__ void ctl_ratio_only(Ctl& c, int q, int p, bool flip, double cbar_q, double gamma_q) {
    c.q = q;
    c.p = flip ? -1 : p;
    c.cbar_q = cbar_q;
    c.gamma_q = gamma_q;
    c.pending = 0;
    c.forced_q = -1;
    c.forced_p = -1;
}
// An iteration that moved x_q by `step` (a bound flip or a basis change) is complete.
__device__ __forceinline__ void ctl_iteration_done(Ctl& c, int q, double cbar_q, double step, double minus_obj, long long iters) {
    c.q = q;
    c.cbar_q = cbar_q;
    c.minus_obj = minus_obj - cbar_q * step;
    c.iters = iters + 1;
    c.forced_q = -1;
    c.forced_p = -1;
    c.last_selected = q;
}
// (minus_obj, iters: the values before this iteration -- the register-resident kernels fetched them in their first round trip)
__device__ __forceinline__ void ctl_bound_flip(const DeviceLP& lp, Ctl& c, int q, double sgn_q, double ub_q, double cbar_q,
                                               double minus_obj, long long iters) {
    const int now_flipped = flip_column(lp.pos, lp.flipped, q, sgn_q);
    c.flip_cost += (now_flipped ? 1.0 : -1.0) * ub_q * lp.cost[q];
    c.p = -1;
    c.bound_flips += 1;
    c.pending = 0;  // no basis change: no inverse update, no weight update
    ctl_iteration_done(c, q, cbar_q, ub_q, minus_obj, iters);
}
__device__ __forceinline__ void ctl_basis_change(const DeviceLP& lp, Ctl& c, bool bounded, int q, int p, int leaving, int leaving_flipped,
                                                 const Step& step, double ub_q, double cbar_q, double alpha_pq, double gamma_q,
                                                 int nz_count, double minus_obj, long long iters) {
    const int fl = exchange_columns(lp.pos, lp.flipped, lp.xub, bounded, q, p, leaving, leaving_flipped, step.leaves_at_upper, ub_q);
    if (step.leaves_at_upper) c.flip_cost += (fl ? 1.0 : -1.0) * step.ub_leaving * lp.cost[leaving];
    c.p = p;
    c.leaving = leaving;
    c.alpha_pq = alpha_pq;
    c.gamma_q = gamma_q;
    c.xp = step.xp;
    c.nz_count = nz_count;
    c.pending = 1;
    ctl_iteration_done(c, q, cbar_q, step.xp, minus_obj, iters);
}

}  // namespace relp
