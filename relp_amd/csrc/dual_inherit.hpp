// The relation between a parent LP and a child LP under which the child's dual simplex may start from the parent's inverse
// (Solver::begin_dual_from; DESIGN.md "Dual simplex: the start from the parent's inverse").  Host only, no HIP: one pure function
// over the exact data of the two models, so that it links into a stand-alone program (tests/support/dual_inherit_check.cpp).
//
// With the parent's basis B in the first m positions and the slack of each appended row behind it,
//
//   B_child = [ B  0 ]        B_child^-1 = [  B^-1          0    ]
//             [ C  S ]                     [ -S^-1 C B^-1   S^-1 ]
//
// (C: the new rows' entries on the parent's basic columns, S: the diagonal of the new slacks' own entries), so the child's inverse is
// the parent's plus k rows, each a sparse combination of rows of the parent's (dual_inherit_kernel, dual.hip).
#pragma once
#include <string>
#include <vector>

#include "model.hpp"

namespace relp {

// Why the child cannot inherit, in words that name the row or the column; empty: it can.  Both bases are provider columns by position,
// as Solver::get_basis gives them (a negative entry is an artificial's code).  Accepted when
//   - the child has k >= 0 more rows than the parent's m, and each basis has one entry per row of its model;
//   - neither basis holds an artificial;
//   - for every position i < m, the child's column child_basis[i] restricted to the rows below m equals the parent's column
//     parent_basis[i] exactly (the same rows, Rat equality): position i means the same thing in both handles;
//   - for every new row r >= m, the column child_basis[r] has exactly one entry, in row r (the slack of that row; its value is s_r).
// Costs and right-hand sides may differ anywhere.
std::string dual_inherit_refusal(const StandardForm& parent, const StandardForm& child, const std::vector<int>& parent_basis,
                                 const std::vector<int>& child_basis);

// ---- implicit upper bounds (Solver::begin_dual_bounded_from; DESIGN.md "The inherited start on implicit bounds") ----------------------

// A basis of the formulation (one column per row of MatrixData, bound rows included; -1 - k: artificial k) reduced to the device's
// constraint rows, as a plan with implicit bounds holds it: the first part of Solver::place_basis, which calls this.  A bounded variable
// whose bound slack is NOT basic sits at its upper bound: non-basic and complemented on the device; with the slack basic it is basic
// here exactly when it is basic there.  A device-basic column keeps the position of its row where that is a constraint row nobody has
// taken, the others fill the free positions in column order.  Device columns: artificial k is k, provider column c is n_art + c.
// Throws std::invalid_argument ("bad basis ...") for a list that is no such basis.
struct ReducedBasis {
    std::vector<int> basis;    // [nr_constraints()] device column per position
    std::vector<int> flipped;  // [n_art + col_end[3]] 1: non-basic at its upper bound, held complemented
};
ReducedBasis reduce_bounded_basis(const MatrixData& md, int n_art, const int* basis_columns);

// What a device column of an LP is, whatever its number: structural variable j (row -1), or the slack or surplus of constraint row i
// (the numbers of the slacks shift when rows are added).  slack_of_row: the provider column, -1 for an equality row.
struct ColumnIdentity {
    int structural = -1, row = -1;
};
ColumnIdentity column_identity(const MatrixData& md, int provider_column);  // of a column below col_end[3]
int slack_of_row(const MatrixData& md, int constraint_row);

// dual_inherit_refusal for two LPs held on implicit bounds, where a changed bound is no row: the child of a branching step keeps its
// parent's constraint rows.  Both bases are bases of the formulation, as Solver::get_basis returns them and begin_dual_bounded takes
// them; each is reduced by reduce_bounded_basis, and the relation is one of the reduced bases over the constraint rows.  With m the
// parent's constraint rows, accepted when
//   - the child has k >= 0 more constraint rows, and its first m are the parent's in order (the same kind of row at each index);
//   - neither basis holds an artificial;
//   - every device-basic column of the child is (a) the same column, by ColumnIdentity, as a device-basic column of the parent, with
//     exactly the parent's entries on the first m rows, or (b) a column with one entry on the constraint rows, in a new row r >= m,
//     no two of them on one row -- and there are exactly k of kind (b).
// Positions and complemented columns need not agree: the child's position i holds what the parent holds at some position src[i], up to
// a sign (dual_inherit_mapped_kernel).  Bounds, costs and right-hand sides may differ anywhere; an LP without a bound reduces to itself.
// `source`, if given and the pair is accepted: per position of the child's reduced basis, the PARENT's provider column of kind (a), or
// -1 - (r - m) for the column of kind (b) on new row r.
std::string dual_bounded_inherit_refusal(const StandardForm& parent, const StandardForm& child, const std::vector<int>& parent_basis,
                                         const std::vector<int>& child_basis, std::vector<int>* source = nullptr);

}  // namespace relp
