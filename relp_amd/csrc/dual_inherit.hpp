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

}  // namespace relp
