// Which kernels a loaded LP runs, decided once from the options and the host matrix before anything is allocated (host-only: no HIP).
//
// `plan_kernel_path` is the only place that chooses; `Solver::load` keeps its answer as `path_`, and the allocation of the device arrays
// and every launch read it.  DESIGN.md section 4 lists the decisions in the order in which they depend on each other.
#pragma once
#include <string>
#include <vector>

#include "../../include/relp_amd.h"
#include "device_columns.hpp"
#include "kernel_limits.hpp"

namespace relp {

// How the dense block is stored: the narrowest type that holds every entry exactly (relp_options.dense_storage may ask for a wider
// one), as tiles for the column-per-lane pricing (*_LANE), rows permuted within 1024-row chunks (I8_PERMUTED) or plain column-major.
enum class DenseStorage : int { NONE, I8_LANE, F32_LANE, F64_LANE, I8_PERMUTED, F32_ROWS, F64_ROWS };

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
    bool multi_workgroup_ratio = false;  // the ratio test runs across workgroups (k2_partd / k2_parti exist)
    bool ratio_textbook = false;     // the reference's ratio test runs (relp_options.ratio_rule resolved against the data and the kernels)
    bool fused = false;              // ratio test + inverse update in one launch
    // generated columns
    int rho_words = 0;
    bool price_unit_pairs = false;

    int slots() const { return price_blocks + dense_blocks; }  // candidate slots of the pricing passes
};

// Implicit upper bounds apply to an LP that has a finite bound (relp_options.implicit_bounds); the device LP then has the
// constraint rows and the first four column groups only.
inline bool implicit_bounds_apply(const relp_options& o, const MatrixData& md) { return o.implicit_bounds != 0 && md.nr_variable_bounds() > 0; }
inline DeviceColumns device_columns(const MatrixData& md, bool bounded) {
    return bounded ? DeviceColumns(md, md.nr_constraints(), md.col_end[3]) : DeviceColumns(md);
}

// `Tableau::select_primal_pivot_row` (tableau/mod.rs:287-313): which ratio test runs.  TEXTBOOK asks for the reference's rule; AUTO
// (the default) takes it where the data are small integers and the kernels of the path implement it, Harris on decimal data.
inline bool resolves_to_textbook(const relp_options& o, const DeviceMatrix& data, bool kernels_have_it) {
    return o.ratio_rule == RELP_RATIO_TEXTBOOK || (o.ratio_rule == RELP_RATIO_AUTO && data.small_integer_data() && kernels_have_it);
}

// Throws std::runtime_error ("LP without rows") or std::invalid_argument (a carry or a ratio rule the LP cannot have) -- before
// anything is allocated.  `column_names` (may be null) names the column in the message of the network check.
KernelPath plan_kernel_path(const relp_options& o, const MatrixData& md, const DeviceColumns& cols, const DeviceMatrix& a,
                            const std::vector<std::string>* column_names = nullptr);

// The plan as one JSON object (relp_debug_kernel_path); slack_of_row by its length only.
std::string kernel_path_json(const KernelPath& p);

}  // namespace relp
