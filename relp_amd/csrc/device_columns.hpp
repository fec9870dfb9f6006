// The index space of the device LP, in one place (host-only).
//
// Every solve path numbers its columns [one artificial per row without an initial pivot | provider columns]: the virtual identity
// columns of `Partially::original_column` (kind/artificial/partially.rs:52-60) first, then the columns of `MatrixData::column`
// (matrix_data.rs:308-327).  It starts from "artificial k on its row, the free slack pivot on the others"
// (`Carry::create_for_partially_artificial`, carry/mod.rs:397-442) and reports a basis in provider columns, with a negative code
// for artificial k.  `DeviceColumns` is that numbering; `DeviceMatrix` is the f64 data the f64 paths put behind it (the exact paths
// scale their own integers and need the numbering only).
#pragma once
#include <cmath>
#include <limits>
#include <vector>

#include "../../include/relp_amd.h"
#include "model.hpp"

namespace relp {

struct DeviceColumns {
    int m = 0, n_p = 0, n_art = 0;
    std::vector<int> artificial_rows;  // [n_art] row of artificial k
    std::vector<int> basis0;           // [m] device column basic in row i at the start of phase one

    DeviceColumns() = default;
    // The first `rows` rows and `provider_columns` columns of `md`: all of them, or with implicit bounds the constraint rows and the
    // first four column groups (the bound rows and their slack columns are not part of the device LP then).
    DeviceColumns(const MatrixData& md, int rows, int provider_columns) : m(rows), n_p(provider_columns) {
        std::vector<int> real_column_of_row(m, -1);
        for (auto& [row, column] : md.pivot_element_indices())
            if (row < m && column < n_p) real_column_of_row[row] = column;
        for (int i = 0; i < m; ++i)
            if (real_column_of_row[i] < 0) artificial_rows.push_back(i);
        n_art = (int)artificial_rows.size();
        basis0.resize(m);
        for (int i = 0, k = 0; i < m; ++i) basis0[i] = real_column_of_row[i] < 0 ? k++ : n_art + real_column_of_row[i];
    }
    explicit DeviceColumns(const MatrixData& md) : DeviceColumns(md, md.nr_rows(), md.nr_columns()) {}

    int n() const { return n_art + n_p; }
    std::vector<int> pos0() const {  // device column -> its row in basis0, -1 for the others
        std::vector<int> pos(n(), -1);
        for (int i = 0; i < m; ++i) pos[basis0[i]] = i;
        return pos;
    }
    // device column <-> provider code: the provider column, or -1 - k for artificial k
    int to_provider(int device_column) const { return device_column >= n_art ? device_column - n_art : -1 - device_column; }
    int to_device(int provider_code) const { return provider_code >= 0 ? n_art + provider_code : -1 - provider_code; }
    std::vector<int> to_provider(const std::vector<int>& device_basis) const {
        std::vector<int> out(device_basis.size());
        for (size_t i = 0; i < out.size(); ++i) out[i] = to_provider(device_basis[i]);
        return out;
    }
};

// f64 CSC of [artificials | provider columns] (12 bytes per virtual column, so materialising them costs nothing and makes the
// pricing pass one uniform CSC sweep), the costs of phase two and the right-hand side.
struct DeviceMatrix {
    std::vector<int> col_start, row_index;
    std::vector<double> value, cost2, rhs;

    DeviceMatrix() = default;
    DeviceMatrix(const DeviceColumns& c, const MatrixData& md) : col_start(c.n() + 1, 0), cost2(c.n(), 0.0), rhs(c.m) {
        for (int k = 0; k < c.n_art; ++k) {
            row_index.push_back(c.artificial_rows[k]);
            value.push_back(1.0);
            col_start[k + 1] = (int)row_index.size();
        }
        for (int j = 0; j < c.n_p; ++j) {
            const SparseColumn column = md.column(j);
            for (size_t e = 0; e < column.nnz(); ++e) {
                if (column.index[e] >= c.m) continue;  // the bound-row entry of a bounded column (implicit bounds)
                row_index.push_back(column.index[e]);
                value.push_back(column.value[e].to_double());
            }
            col_start[c.n_art + j + 1] = (int)row_index.size();
            cost2[c.n_art + j] = md.cost_value(j).to_double();
        }
        const auto rhs_exact = md.right_hand_side();
        for (int i = 0; i < c.m; ++i) rhs[i] = rhs_exact[i].to_double();
    }
    // RELP_RATIO_AUTO takes the reference's ratio test on such data: every entry an integer with |a| <= 64, costs and right-hand
    // side integers below 2^20.
    bool small_integer_data() const {
        bool small_integers = true;
        for (size_t e = 0; e < value.size() && small_integers; ++e) small_integers = value[e] == std::nearbyint(value[e]) && std::fabs(value[e]) <= 64.0;
        for (size_t j = 0; j < cost2.size() && small_integers; ++j) small_integers = cost2[j] == std::nearbyint(cost2[j]) && std::fabs(cost2[j]) < 1048576.0;
        for (size_t i = 0; i < rhs.size() && small_integers; ++i) small_integers = rhs[i] == std::nearbyint(rhs[i]) && std::fabs(rhs[i]) < 1048576.0;
        return small_integers;
    }
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

// ---- implicit upper bounds: between the device LP (constraint rows, the first four column groups) and the reference's formulation
// (every row of MatrixData, the VariableBound / SlackBound rows and their slack columns of matrix_data.rs:104-145 included) ----------

// Upper bound of each device column: structurals with one, range slacks (their range); +inf for the others.
inline std::vector<double> implicit_upper_bounds(const MatrixData& md, const DeviceColumns& c) {
    std::vector<double> ub(c.n(), std::numeric_limits<double>::infinity());
    for (int j = 0; j < md.nr_normal_variables(); ++j)
        if (md.variables[j].has_upper) ub[c.n_art + j] = md.variables[j].upper.to_double();
    for (int k = 0; k < md.nr_range; ++k) ub[c.n_art + md.col_end[0] + k] = md.ranges[k].to_double();
    return ub;
}

// The basis of the reference's formulation that a device state stands for (`basis`: device column per constraint row; `pos`: per
// device column, -2 = non-basic at its upper bound).  On every bound row the bound slack is basic when the variable is below its
// bound and the variable itself when it sits at it.
inline std::vector<int> explicit_basis(const MatrixData& md, const DeviceColumns& c, const std::vector<int>& basis, const std::vector<int>& pos) {
    std::vector<int> out(md.nr_rows(), -1);
    for (int i = 0; i < c.m; ++i) out[i] = c.to_provider(basis[i]);
    const int nb = (int)md.bound_to_variable.size();
    for (int k2 = 0; k2 < nb; ++k2) {
        const int j = md.bound_to_variable[k2];
        out[md.row_end[3] + k2] = pos[c.n_art + j] == -2 ? j : md.col_end[3] + k2;
    }
    for (int k2 = 0; k2 < md.nr_range; ++k2) {
        const int j = md.col_end[0] + k2;
        out[md.row_end[4] + k2] = pos[c.n_art + j] == -2 ? j : md.col_end[4] + k2;
    }
    return out;
}

// The values of every column of MatrixData (`x`, zero-filled, nr_columns() long) from x_B of the device LP: the value of a
// complemented variable is u_j - x'_j, a complemented non-basic variable sits at its upper bound, and the bound slack of a variable
// below its bound takes up the rest.
inline void explicit_solution(const MatrixData& md, const DeviceColumns& c, const std::vector<int>& basis, const double* xb, const std::vector<int>& flipped,
                              const std::vector<int>& pos, const std::vector<double>& ub, std::vector<double>& x) {
    for (int i = 0; i < c.m; ++i) {
        const int dev = basis[i];
        if (dev >= c.n_art) x[dev - c.n_art] = flipped[dev] ? ub[dev] - xb[i] : xb[i];
    }
    for (int j = c.n_art; j < c.n(); ++j)
        if (pos[j] == -2) x[j - c.n_art] = ub[j];
    const int nb = (int)md.bound_to_variable.size();
    for (int k2 = 0; k2 < nb; ++k2) {  // VariableBound rows: the bound slack of a variable below its bound
        const int j = md.bound_to_variable[k2];
        if (pos[c.n_art + j] != -2) x[md.col_end[3] + k2] = ub[c.n_art + j] - x[j];
    }
    for (int k2 = 0; k2 < md.nr_range; ++k2) {  // SlackBound rows (range slacks)
        const int j = md.col_end[0] + k2;
        if (pos[c.n_art + j] != -2) x[md.col_end[4] + k2] = ub[c.n_art + j] - x[j];
    }
}

}  // namespace relp
