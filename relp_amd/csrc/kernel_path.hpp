// Which kernels a loaded LP runs, decided once from the options and the host matrix before anything is allocated (host-only: no HIP).
//
// `plan_kernel_path` is the only place that chooses; `Solver::load` keeps its answer as `path_`, and the allocation of the device arrays
// and every launch read it.  DESIGN.md section 4 lists the decisions in the order in which they depend on each other.
#pragma once
#include <string>
#include <vector>

#include "../../include/relp_amd.h"
#include "kernel_limits.hpp"

namespace relp {

struct MatrixData;  // (model.hpp; the next two device_columns.hpp: the planner's inputs, which a launcher that reads a plan does not need)
struct DeviceColumns;
struct DeviceMatrix;

// How the dense block is stored: the narrowest type that holds every entry exactly (relp_options.dense_storage may ask for a wider
// one), as tiles for the column-per-lane pricing (*_LANE), rows permuted within 1024-row chunks (I8_PERMUTED) or plain column-major.
enum class DenseStorage : int { NONE, I8_LANE, F32_LANE, F64_LANE, I8_PERMUTED, F32_ROWS, F64_ROWS };

// The template instantiations of the pivot loop.  Each names what one launch helper of kernels.hip runs when a path calls it (the LU
// and the forest carries never call launch_update, the deferred product form runs btran_pass_kernel in its place).
//   UNIT_PAIRS  price_kernel<RULE, false, 2, true>   generated columns, two lanes per arc (A/B form)
//   GENERATED   price_unit_kernel<RULE>              incidence columns generated from the arcs' endpoints (8 B per arc)
//   WIDTH_2     price_kernel<RULE, false, 2>         graph LPs: two entries per column, vectors gathered from L2
//   LDS         price_kernel<RULE, true, 8>          -pi, rho_p, w staged in LDS (price_lds bytes per workgroup)
//   GATHER      price_kernel<RULE, false, 8>
enum class PriceKernel : int { UNIT_PAIRS, GENERATED, WIDTH_2, LDS, GATHER };
// REGISTERS_R: ftran_ratio_fast_kernel<RULE, R> (R rows per thread of one workgroup of K2F_THREADS); MULTI_WORKGROUP: the chain
// k2l_ftran_kernel (k2l_preselected_kernel under the forest carry) / k2l_harris_kernel / k2l_apply_kernel; ONE_WORKGROUP: ftran_ratio_kernel.
enum class RatioKernel : int { REGISTERS_2, REGISTERS_4, REGISTERS_8, REGISTERS_16, MULTI_WORKGROUP, ONE_WORKGROUP };
inline int ratio_rows_per_thread(RatioKernel k) { return k <= RatioKernel::REGISTERS_16 ? 2 << (int)k : 0; }  // 0: not register-resident
// update_kernel<true> | update_kernel<false> on one workgroup per 8 columns | update_kernel<false> on one workgroup per column pair
enum class UpdateKernel : int { EAGER, PREDICATED, PREDICATED_SPLIT_GRID };
// gemm_mfma_kernel (v_mfma_f64_16x16x4_f64, restricted to the touched rows where they are tracked) | gemm_polish_kernel (plain FMA, every row)
enum class PolishGemm : int { MFMA, VECTOR };

// The constants of a loaded LP: written by plan_kernel_path, read everywhere else.
struct KernelPath {
    // the device LP: [n_art artificials | n_p provider columns], m rows
    int m = 0, n = 0, n_art = 0, n_p = 0;
    // carry and refactorisation
    bool bounded = false;          // implicit upper bounds are active
    bool network = false;          // spanning-forest carry
    bool lu_mode = false;          // an LU carry ...
    bool lu_inverse = false;       // ... in its inverse-factor form (lu.hpp: L^-1, U^-1 and product-form updates)
    int refactor_period = 64;
    bool device_refactor = false;  // `BasisInverse::invert` as kernels
    bool async_refactor = false;   // ... on a second stream, beside the pivots
    // dense block
    int n_dense = 0;
    int sparse_first = 0;          // device columns priced by the CSC kernel: [sparse_first, n)
    int dense_ld = 0;
    bool dense_lane = false;       // column-per-lane pricing
    bool dense_full = false;       // every dense column has m entries, rows 0 .. m-1 in order
    int dense_csc_start = 0;
    DenseStorage dense_storage = DenseStorage::NONE;
    int dense_entry_bytes() const {
        const DenseStorage s = dense_storage;
        return s == DenseStorage::I8_LANE || s == DenseStorage::I8_PERMUTED ? 1 : s == DenseStorage::F32_LANE || s == DenseStorage::F32_ROWS ? 4 : 8;
    }
    // pricing and FTRAN sizing
    int ell_w = ELL_W;
    bool generated_columns = false;  // incidence columns generated from 8 bytes per arc
    PriceKernel price_kernel = PriceKernel::GATHER;        // of the three-kernel pivot (a forced batch of a fused path too)
    PriceKernel price_kernel_fused = PriceKernel::GATHER;  // of the fused pivot's batches: read where `fused`
    int price_blocks = 0;            // sparse pricing workgroups
    int dense_blocks = 0;            // dense pricing workgroups (candidate slots follow the sparse ones)
    int vector_len = 0;              // -pi, rho, w: zero-padded to the dense block's row count when the column-per-lane pricing reads them
    size_t price_lds = 0;
    int ftran_slices = 0;            // > 0: multi-block FTRAN pipeline
    // pivot form
    bool eta_mode = false;           // deferred product form of the inverse
    int eta_cap = 0;
    bool slack_in_btran = false;     // the slack columns of the dense pipeline are priced by the BTRAN pass of the previous pivot
    std::vector<int> slack_of_row;   // [m] with slack_in_btran: that column of each row, or -1
    bool track_touched = false;
    RatioKernel ratio_kernel = RatioKernel::ONE_WORKGROUP;            // a full iteration (mode 0)
    RatioKernel ratio_kernel_no_change = RatioKernel::ONE_WORKGROUP;  // modes 1 and 2 (`price`, `ratio`): never across workgroups
    bool multi_workgroup_ratio = false;  // ratio_kernel == MULTI_WORKGROUP: k2_partd / k2_parti exist
    bool ratio_textbook = false;     // the reference's ratio test runs (relp_options.ratio_rule resolved against the data and the kernels)
    bool fused = false;              // ratio test + inverse update in one launch
    int fused_rows = 0;              // ... pivot_fused_kernel<RULE, R>: 2 or 4 rows per thread (0: not fused)
    UpdateKernel update_kernel = UpdateKernel::EAGER;
    PolishGemm polish_gemm = PolishGemm::MFMA;
    // generated columns
    int rho_words = 0;
    bool price_unit_pairs = false;

    int slots() const { return price_blocks + dense_blocks; }  // candidate slots of the pricing passes

    // What Solver::stats().launches counts for one batch of `count` pivots: a plain batch, a forced one (`bring_into_basis`, the
    // zero-level pivots: always the three-kernel form) or a batch replayed from a captured graph.  The figures are a convention that
    // tests pin, not a census of kernels.  A replayed batch counts the three-kernel pivot on every explicit path, whatever the dense
    // block, the FTRAN form and the fused pivot add or save.  No batch counts the four consolidation kernels of the deferred product
    // form (every eta_cap pivots and at the end of a batch), and outside the forest carry the multi-workgroup ratio test counts as one
    // launch though it is three.  Nothing outside a batch is counted at all: set_phase and the polish (launch_pi's three kernels
    // among them), the refactorisations and the fine-grained operations.
    int launches_per_batch(bool forced, bool replayed) const { return fused && !forced && !replayed ? 2 : 1; }  // budget (begin_batch + commit)
    int launches_per_pivot(bool forced, bool replayed) const {
        if (network) return multi_workgroup_ratio ? 7 : 5;  // pricing, path, ratio test (one kernel, or three across workgroups), update, re-hang
        if (lu_mode) return 2;                              // pricing and the single-workgroup LU kernel
        if (replayed) return 3;
        if (fused && !forced) return 2;
        return 3 + (dense_blocks > 0) + 2 * (ftran_slices > 0);
    }
    long long launches(long long count, bool forced, bool replayed) const {
        return launches_per_batch(forced, replayed) + (long long)launches_per_pivot(forced, replayed) * count;
    }
};

// Throws std::runtime_error ("LP without rows") or std::invalid_argument (a carry or a ratio rule the LP cannot have) -- before
// anything is allocated.  `column_names` (may be null) names the column in the message of the network check.
KernelPath plan_kernel_path(const relp_options& o, const MatrixData& md, const DeviceColumns& cols, const DeviceMatrix& a,
                            const std::vector<std::string>* column_names = nullptr);

// Why the dual simplex (dual.hip) does not take this plan, in words; empty: it does.  Its kernels read and write the explicit inverse
// as it stands outside a batch, one column-major buffer with every column present, and know neither bounds nor generated columns:
// they take the explicit carry without the dense pipeline, up to the row count of the single-workgroup kernels.
constexpr int DUAL_MAX_ROWS = 8192;
std::string dual_refusal(const KernelPath& p);
// ... and the loop that knows implicit upper bounds (Solver::begin_dual_bounded): dual_refusal of the plan with `bounded` cleared.  It
// takes every plan the loop above takes, with bounds or without; p.m counts the constraint rows only.
std::string dual_bounded_refusal(const KernelPath& p);

// The plan as one JSON object (relp_debug_kernel_path); slack_of_row by its length only.
std::string kernel_path_json(const KernelPath& p);

}  // namespace relp
