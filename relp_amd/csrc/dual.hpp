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
};

constexpr int DUAL_COLUMNS_PER_BLOCK = 256;  // dual_row_kernel, dual_choose_kernel: one lane per column
inline int dual_blocks(int n_art, int n) { return (n - n_art + DUAL_COLUMNS_PER_BLOCK - 1) / DUAL_COLUMNS_PER_BLOCK; }

// One dual pivot is these five launches in this order.  Each returns at once unless Ctl::status == ST_RUNNING; dual_leave_kernel
// also stops the chain when the budget of the batch is used up (ST_BUDGET), so a batch that finishes early is a run of no-ops.
//   leave:   the leaving row p (largest infeasibility among x_B[i] < -harris_delta; ties: lowest basic column, lowest row), rho = row p
//            of the inverse; none: ST_NO_ENTERING, the basis is primal feasible
//   row:     alpha_pj, d_j and pass 1 of the ratio test over the non-basic provider columns (`lds`: rho and -pi staged in LDS)
//   choose:  theta_max, pass 2 (largest |alpha_pj| within theta_max, key 1 under the textbook rule; ties: lowest column)
//   pivot:   the entering column q (none: ST_UNBOUNDED, the LP is infeasible), FTRAN, x_B, basis, pos, control block; ST_REFACTOR
//            with nothing written where the FTRAN value of the pivot is not below -tol_pivot as the row's value was
//   update:  the inverse and -pi
void launch_dual_leave(const DeviceLP& d, double harris_delta, hipStream_t s);
void launch_dual_row(const DeviceLP& d, const DualBuffers& b, bool lds, double tol_pivot, double slack, hipStream_t s);
void launch_dual_choose(const DeviceLP& d, const DualBuffers& b, double tol_pivot, bool textbook, hipStream_t s);
void launch_dual_pivot(const DeviceLP& d, const DualBuffers& b, double tol_pivot, hipStream_t s);
void launch_dual_update(const DeviceLP& d, hipStream_t s);

// The start from a parent's inverse (Solver::begin_dual_from; the relation between the two LPs: dual_inherit.hpp).  `child` has its
// pos uploaded for the basis [the parent's basis in the first parent_m positions | the slack of each appended row]; `parent_inverse`
// is the parent's column-major inverse (parent_m x parent_m, leading dimension parent_ld) on the same device.  Writes every entry of
// the child's first buffer: the parent's columns, the child.m - parent_m border rows, the scaled unit columns of the new slacks.
void launch_dual_inherit(const DeviceLP& child, const double* parent_inverse, int parent_m, int parent_ld, hipStream_t s);

}  // namespace relp
