// Dual simplex from a given dual-feasible basis (dual.hip): the buffers of its loop and the launch helpers Solver::iterate_dual calls.
//
// The loop works on DeviceLP as it stands outside a batch of primal pivots -- the column-major inverse in its first buffer, x_B, basis,
// pos, -pi, the CSC and the control block -- and leaves it in that form, so the primal loop, the polish and the fine-grained operations
// can take over after any dual pivot.  It does not maintain the steepest-edge weights (every dual pivot leaves Ctl::pending = 0):
// set_phase(2) recomputes them before the primal loop runs again.  Which plans take it: dual_refusal (kernel_path.hpp).
#pragma once
#include <hip/hip_runtime.h>

namespace relp {

struct DeviceLP;  // device_lp.hpp; solver.hpp includes this file for the handle's DualBuffers

// Allocated by the first begin_dual of a loaded LP, freed with the LP's other device buffers.
struct DualBuffers {
    double* alpha_row = nullptr;   // [n] alpha_pj = rho_p . a_j of the non-basic columns (0 on a basic column: never eligible)
    double* d = nullptr;           // [n] their relative costs d_j = c_j - pi . a_j
    double* part_theta = nullptr;  // [blocks] pass 1 of the ratio test: one partial minimum per workgroup of dual_row_kernel
    double* cand_key = nullptr;    // [blocks] pass 2: one candidate per workgroup of dual_choose_kernel ...
    int* cand_j = nullptr;         // ... its column, -1: none
    int blocks = 0;                // workgroups of the two grids over the provider columns [n_art, n)
    // relp_options.dual_pricing = RELP_DUAL_PRICING_STEEPEST_EDGE only (nullptr / 0 otherwise: the loop of rule 0 is what it was)
    double* beta = nullptr;        // [m] beta_i = |e_i' B^-1|^2, the squared norm of row i of the inverse
    double* beta_part = nullptr;   // [slices][m] dual_weights_kernel: the sum over one slice of columns, per row
    int slices = 0;                // column slices of its grid (dual_weight_slices)
    // The long-step ratio test only (Solver::set_dual_long_step on a plan with implicit bounds; nullptr otherwise)
    int* flip_count = nullptr;     // [4] of this pivot: |F|, 1 where the kernel fell back to F = {}; since the start: flips applied, fall-backs
    int* flip_j = nullptr;         // [DUAL_MAX_FLIPS] the columns of F in the order of the walk
    double* flip_w = nullptr;      // [m] scratch of the pivot kernel: Binv Delta, Delta = sum over F of ub_j sgn_j a_j
};

constexpr int DUAL_COLUMNS_PER_BLOCK = 256;  // dual_row_kernel, dual_choose_kernel: one lane per column
constexpr int DUAL_MAX_FLIPS = 32;           // long step: columns passed in one pivot at most (stopping early is always valid)
constexpr int DUAL_LONG_STEP_SLOTS = 2048;   // dual_long_step_kernel: boxed candidates of one pivot it holds in LDS (40 KB)
inline int dual_blocks(int n_art, int n) { return (n - n_art + DUAL_COLUMNS_PER_BLOCK - 1) / DUAL_COLUMNS_PER_BLOCK; }

// Column slices of dual_weights_kernel: at least 64 columns each (16 per wave of its workgroups), 16 at most -- at m = 2049 the grid is
// 33 row tiles x 16 slices, two workgroups per compute unit; one slice up to m = 127.
constexpr int DUAL_WEIGHT_SLICES_MAX = 16;
inline int dual_weight_slices(int m) { return m / 64 < 1 ? 1 : m / 64 > DUAL_WEIGHT_SLICES_MAX ? DUAL_WEIGHT_SLICES_MAX : m / 64; }

// One dual pivot is these five launches in this order.  Each returns at once unless Ctl::status == ST_RUNNING; dual_leave_kernel
// also stops the chain when the budget of the batch is used up (ST_BUDGET), so a batch that finishes early is a run of no-ops.
//   leave:   the leaving row p (largest infeasibility among x_B[i] < -harris_delta, or largest x_B[i]^2 / beta_i under the steepest-edge
//            rule; ties: lowest basic column, lowest row), rho = row p of the inverse; none: ST_NO_ENTERING, the basis is primal feasible;
//            with an objective cutoff, first of all: ST_CUTOFF where the objective of this basis has reached it
//   row:     alpha_pj, d_j and pass 1 of the ratio test over the non-basic provider columns (`lds`: rho and -pi staged in LDS)
//   choose:  theta_max, pass 2 (largest |alpha_pj| within theta_max, key 1 under the textbook rule; ties: lowest column)
//   pivot:   the entering column q (none: ST_UNBOUNDED, the LP is infeasible), FTRAN, x_B, basis, pos, control block; ST_REFACTOR
//            with nothing written where the FTRAN value of the pivot is not below -tol_pivot as the row's value was
//   update:  the inverse and -pi
// `bounded` (KernelPath::bounded, the loop of Solver::begin_dual_bounded): the instantiations that know implicit upper bounds, over the
// state the bounded primal kernels keep (DeviceLP::ub, xub, flipped, rhs; pos -2 / -3).  A row is infeasible below 0 or above xub[i]
// (the side s = +1 / -1); the row of the tableau is taken in the held form and towards that side, abar_j = s sgn_j rho . a_j and
// d_j = sgn_j (c_j - pi . a_j), so that choose and update are the same kernels; the pivot checks s alpha_q[p] < -tol_pivot, steps to
// the violated bound, and complements a column that leaves at its upper bound.  false: the kernels as they were.
// `cutoff` (Solver::set_dual_cutoff): the instantiations of the leave kernel that first compare the objective of the basis they stand on,
// -Ctl::minus_obj, with `cutoff_carry` (the cutoff less the fixed cost) and stop the chain with ST_CUTOFF where it is reached, in front
// of the budget check and with nothing scanned or written but the status.  false: the kernels as they were; `cutoff_carry` is not read.
void launch_dual_leave(const DeviceLP& d, double harris_delta, const double* beta, bool bounded, bool cutoff, double cutoff_carry,
                       hipStream_t s);  // beta == nullptr: rule 0
void launch_dual_row(const DeviceLP& d, const DualBuffers& b, bool lds, bool bounded, double tol_pivot, double slack, hipStream_t s);
void launch_dual_choose(const DeviceLP& d, const DualBuffers& b, double tol_pivot, bool textbook, hipStream_t s);
void launch_dual_pivot(const DeviceLP& d, const DualBuffers& b, bool bounded, bool long_step, double tol_pivot, hipStream_t s);
void launch_dual_update(const DeviceLP& d, hipStream_t s);

// The long-step (bound-flipping) ratio test of the bounded loop, a sixth launch between row and choose (b.flip_count allocated, and
// launch_dual_pivot with `long_step`): the boxed candidates whose ratios the dual step may pass while row p stays violated by more than
// harris_delta go to their other bound instead of entering (DualBuffers::flip_j), choose and pivot find the entering column among the
// rest, and the pivot kernel applies the flips behind its ST_REFACTOR guard.  `slack` as launch_dual_row's.
void launch_dual_long_step(const DeviceLP& d, const DualBuffers& b, double tol_pivot, double slack, double harris_delta, hipStream_t s);

// The steepest-edge rule of the leaving row (b.beta allocated): launch_dual_leave takes `beta` = b.beta and keys a row by
// x_B[i]^2 / beta_i; after launch_dual_update the weights are computed again from the new inverse, which they equal by construction
// (no recurrence, nothing to drift).  Returns the number of launches: 1 with one slice (the partial sums are the weights), else 2
// (dual_weights_kernel, then the fold of the partial sums in slice order).  `chained`: behind a pivot's launches, a no-op unless
// Ctl::status == ST_RUNNING like them; false from the host (the starts, after a polish), where the status says nothing about the inverse.
int launch_dual_weights(const DeviceLP& d, const DualBuffers& b, bool chained, hipStream_t s);

// The start from a parent's inverse (Solver::begin_dual_from; the relation between the two LPs: dual_inherit.hpp).  `child` has its
// pos uploaded for the basis [the parent's basis in the first parent_m positions | the slack of each appended row]; `parent_inverse`
// is the parent's column-major inverse (parent_m x parent_m, leading dimension parent_ld) on the same device.  Writes every entry of
// the child's first buffer: the parent's columns, the child.m - parent_m border rows, the scaled unit columns of the new slacks.
void launch_dual_inherit(const DeviceLP& child, const double* parent_inverse, int parent_m, int parent_ld, hipStream_t s);

// The same between two LPs held on implicit upper bounds (Solver::begin_dual_bounded_from; dual_bounded_inherit_refusal): `src` and
// `sg` are device arrays of child.m ints.  src[i] in [0, parent_m): the child's position i holds the column the parent holds at that
// position, sg[i] = +-1 the product of the signs the two held forms give it; src[i] = -1 - rho, rho in [0, child.m - parent_m), each
// once: the slack of new row parent_m + rho (sg[i] is not read).  `child` has pos and flipped uploaded for its basis.  Writes every
// entry of the child's first buffer; reads the parent's inverse only (the caller checks the ranges: the kernel trusts them).
void launch_dual_inherit_mapped(const DeviceLP& child, const double* parent_inverse, int parent_m, int parent_ld, const int* src, const int* sg, hipStream_t s);

}  // namespace relp
