// dual_inherit_refusal (dual_inherit.hpp): host only, exact data, no device in reach.
#include "dual_inherit.hpp"

namespace relp {

namespace {

std::string basis_refusal(const char* whose, const MatrixData& md, const std::vector<int>& basis) {
    const int rows = md.nr_rows(), columns = md.nr_columns();
    if ((int)basis.size() != rows)
        return std::string("the ") + whose + "'s basis has " + std::to_string(basis.size()) + " entries for " + std::to_string(rows) + " rows";
    for (int i = 0; i < rows; ++i) {
        if (basis[i] < 0)
            return std::string("the ") + whose + "'s basis holds an artificial column (code " + std::to_string(basis[i]) + " on row " + std::to_string(i) +
                   "): only a basis of the LP's own columns is inherited";
        if (basis[i] >= columns)
            return std::string("the ") + whose + "'s basis names column " + std::to_string(basis[i]) + " on row " + std::to_string(i) + ", beyond its " +
                   std::to_string(columns) + " columns";
    }
    return "";
}

}  // namespace

std::string dual_inherit_refusal(const StandardForm& parent, const StandardForm& child, const std::vector<int>& parent_basis,
                                 const std::vector<int>& child_basis) {
    const MatrixData &pd = parent.data, &cd = child.data;
    const int m = pd.nr_rows(), m_child = cd.nr_rows();
    if (m_child < m)
        return "the child has " + std::to_string(m_child) + " rows, fewer than its parent's " + std::to_string(m) + ": rows are appended, never dropped";
    std::string refusal = basis_refusal("parent", pd, parent_basis);
    if (refusal.empty()) refusal = basis_refusal("child", cd, child_basis);
    if (!refusal.empty()) return refusal;
    for (int i = 0; i < m; ++i) {
        const SparseColumn before = pd.column(parent_basis[i]), after = cd.column(child_basis[i]);
        const std::string where = "position " + std::to_string(i) + ": column " + std::to_string(child_basis[i]) + " of the child is not column " +
                                  std::to_string(parent_basis[i]) + " of the parent on the parent's rows";
        size_t e = 0;
        for (size_t f = 0; f < after.nnz() && after.index[f] < m; ++f, ++e) {  // (rows are sorted: those below m come first)
            if (e >= before.nnz() || before.index[e] > after.index[f])
                return where + " (row " + std::to_string(after.index[f]) + ": " + to_string(after.value[f]) + " in the child, no entry in the parent)";
            if (before.index[e] < after.index[f])
                return where + " (row " + std::to_string(before.index[e]) + ": " + to_string(before.value[e]) + " in the parent, no entry in the child)";
            if (before.value[e] != after.value[f])
                return where + " (row " + std::to_string(after.index[f]) + ": " + to_string(after.value[f]) + " in the child, " + to_string(before.value[e]) +
                       " in the parent)";
        }
        if (e < before.nnz())
            return where + " (row " + std::to_string(before.index[e]) + ": " + to_string(before.value[e]) + " in the parent, no entry in the child)";
    }
    for (int r = m; r < m_child; ++r) {
        const SparseColumn slack = cd.column(child_basis[r]);
        if (slack.nnz() != 1 || slack.index[0] != r)
            return "row " + std::to_string(r) + ": column " + std::to_string(child_basis[r]) + " of the child is not the slack of that new row (it has " +
                   std::to_string(slack.nnz()) + (slack.nnz() == 1 ? " entry, in row " + std::to_string(slack.index[0]) : std::string(" entries")) +
                   "): a new row starts with its own single-entry column basic";
    }
    return "";
}

}  // namespace relp
