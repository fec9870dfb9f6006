// dual_inherit_refusal, reduce_bounded_basis and dual_bounded_inherit_refusal (dual_inherit.hpp): host only, exact data, no device in reach.
#include "dual_inherit.hpp"

#include <stdexcept>

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

// Where the child's column `after` differs from the parent's column `before` on the rows below m, in brackets; empty: nowhere.
// (Rows are sorted: those below m come first; what lies behind them -- new rows, a bound row -- is not compared.)
std::string difference_below(const SparseColumn& before, const SparseColumn& after, int m) {
    size_t e = 0, f = 0;
    for (; f < after.nnz() && after.index[f] < m; ++f, ++e) {
        if (e >= before.nnz() || before.index[e] >= m || before.index[e] > after.index[f])
            return " (row " + std::to_string(after.index[f]) + ": " + to_string(after.value[f]) + " in the child, no entry in the parent)";
        if (before.index[e] < after.index[f])
            return " (row " + std::to_string(before.index[e]) + ": " + to_string(before.value[e]) + " in the parent, no entry in the child)";
        if (before.value[e] != after.value[f])
            return " (row " + std::to_string(after.index[f]) + ": " + to_string(after.value[f]) + " in the child, " + to_string(before.value[e]) +
                   " in the parent)";
    }
    if (e < before.nnz() && before.index[e] < m)
        return " (row " + std::to_string(before.index[e]) + ": " + to_string(before.value[e]) + " in the parent, no entry in the child)";
    return "";
}

int row_kind(const MatrixData& md, int constraint_row) {  // 0 equality | 1 range | 2 <= | 3 >=
    int kind = 0;
    while (constraint_row >= md.row_end[kind]) ++kind;
    return kind;
}

std::string described(const MatrixData& md, int provider_column) {
    const ColumnIdentity id = column_identity(md, provider_column);
    return "column " + std::to_string(provider_column) +
           (id.row < 0 ? " (structural variable " + std::to_string(id.structural) + ")" : " (the slack of row " + std::to_string(id.row) + ")");
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
        const std::string difference = difference_below(pd.column(parent_basis[i]), cd.column(child_basis[i]), m);
        if (!difference.empty())
            return "position " + std::to_string(i) + ": column " + std::to_string(child_basis[i]) + " of the child is not column " +
                   std::to_string(parent_basis[i]) + " of the parent on the parent's rows" + difference;
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

ReducedBasis reduce_bounded_basis(const MatrixData& md, int n_art, const int* basis_columns) {
    const int m = md.nr_constraints(), rows_full = md.nr_rows(), cols_full = md.nr_columns(), n_dev = md.col_end[3];
    ReducedBasis out;
    out.basis.assign(m, -1);
    out.flipped.assign(n_art + n_dev, 0);
    std::vector<int> row_of(cols_full, -1);
    std::vector<int> artificial_row_of(n_art, -1);
    for (int i = 0; i < rows_full; ++i) {
        const int c = basis_columns[i];
        if (c >= 0) {
            if (c >= cols_full || row_of[c] >= 0) throw std::invalid_argument("bad basis");
            row_of[c] = i;
        } else {
            const int k = -1 - c;  // (an artificial's device column is its number)
            if (k >= n_art || artificial_row_of[k] >= 0) throw std::invalid_argument("bad basis");
            artificial_row_of[k] = i;
        }
    }
    auto bound_pair = [&](int variable, int slack) {
        if (row_of[slack] < 0) {
            if (row_of[variable] < 0) throw std::invalid_argument("bad basis: neither a bounded variable nor its bound slack is basic");
            out.flipped[n_art + variable] = 1;  // at its upper bound
            row_of[variable] = -2;              // not basic on the device
        }
    };
    for (int k2 = 0; k2 < (int)md.bound_to_variable.size(); ++k2) bound_pair(md.bound_to_variable[k2], md.col_end[3] + k2);
    for (int k2 = 0; k2 < md.nr_range; ++k2) bound_pair(md.col_end[0] + k2, md.col_end[4] + k2);
    std::vector<int> device_basic;  // device column, preferred row
    std::vector<int> wanted_row;
    for (int k = 0; k < n_art; ++k)
        if (artificial_row_of[k] >= 0) { device_basic.push_back(k); wanted_row.push_back(artificial_row_of[k]); }
    for (int c = 0; c < n_dev; ++c)
        if (row_of[c] >= 0) { device_basic.push_back(n_art + c); wanted_row.push_back(row_of[c]); }
    if ((int)device_basic.size() != m) throw std::invalid_argument("bad basis: it does not reduce to a basis of the constraint rows");
    std::vector<int> homeless;
    for (size_t t = 0; t < device_basic.size(); ++t) {
        if (wanted_row[t] < m && out.basis[wanted_row[t]] < 0) out.basis[wanted_row[t]] = device_basic[t];
        else homeless.push_back(device_basic[t]);
    }
    size_t next = 0;
    for (int i = 0; i < m; ++i)
        if (out.basis[i] < 0) out.basis[i] = homeless[next++];
    return out;
}

ColumnIdentity column_identity(const MatrixData& md, int provider_column) {
    ColumnIdentity id;
    const auto [group, k] = md.column_type(provider_column);
    if (group == 0) id.structural = k;
    else id.row = md.row_end[group - 1] + k;  // RangeSlack | UpperIneqSlack | LowerIneqSlack: the k-th row of its kind
    return id;
}

int slack_of_row(const MatrixData& md, int constraint_row) {
    const int kind = row_kind(md, constraint_row);
    return kind == 0 ? -1 : md.col_end[kind - 1] + (constraint_row - md.row_end[kind - 1]);
}

std::string dual_bounded_inherit_refusal(const StandardForm& parent, const StandardForm& child, const std::vector<int>& parent_basis,
                                         const std::vector<int>& child_basis, std::vector<int>* source) {
    static const char* kinds[] = {"an equality", "a range", "a <=", "a >="};
    const MatrixData &pd = parent.data, &cd = child.data;
    const int m = pd.nr_constraints(), m_child = cd.nr_constraints(), k = m_child - m;
    if (m_child < m)
        return "the child has " + std::to_string(m_child) + " constraint rows, fewer than its parent's " + std::to_string(m) +
               ": rows are appended, never dropped";
    for (int i = 0; i < m; ++i)
        if (row_kind(pd, i) != row_kind(cd, i))
            return "row " + std::to_string(i) + " is " + kinds[row_kind(cd, i)] + " row in the child and " + kinds[row_kind(pd, i)] +
                   " row in the parent: the child's first " + std::to_string(m) + " constraint rows are the parent's, in order";
    std::string refusal = basis_refusal("parent", pd, parent_basis);
    if (refusal.empty()) refusal = basis_refusal("child", cd, child_basis);
    if (!refusal.empty()) return refusal;
    ReducedBasis reduced_parent, reduced_child;
    try {
        reduced_parent = reduce_bounded_basis(pd, 0, parent_basis.data());
    } catch (const std::invalid_argument& e) {
        return std::string("the parent's basis: ") + e.what();
    }
    try {
        reduced_child = reduce_bounded_basis(cd, 0, child_basis.data());
    } catch (const std::invalid_argument& e) {
        return std::string("the child's basis: ") + e.what();
    }
    std::vector<char> basic_in_parent(pd.col_end[3], 0);
    for (int c : reduced_parent.basis) basic_in_parent[c] = 1;
    std::vector<int> from(m_child, 0), taken_by(k, -1);
    int n_new = 0;
    for (int i = 0; i < m_child; ++i) {
        const int c = reduced_child.basis[i];
        const SparseColumn column = cd.column(c);
        size_t below = 0, on_rows = 0;  // entries on the parent's rows, on the constraint rows (a bound row's entry lies behind them)
        while (on_rows < column.nnz() && column.index[on_rows] < m_child) {
            if (column.index[on_rows] < m) ++below;
            ++on_rows;
        }
        const std::string where = "position " + std::to_string(i) + ": " + described(cd, c) + " of the child";
        if (below == 0) {  // kind (b)
            if (on_rows != 1)
                return where + " has " + std::to_string(on_rows) + " entries on the constraint rows" +
                       (on_rows >= 2 ? " (rows " + std::to_string(column.index[0]) + " and " + std::to_string(column.index[1]) + " among them)" : std::string()) +
                       ", none of them on the parent's: the basic column of a new row has one entry, in that row";
            const int r = column.index[0];
            if (taken_by[r - m] >= 0)
                return "row " + std::to_string(r) + ": columns " + std::to_string(taken_by[r - m]) + " and " + std::to_string(c) +
                       " of the child both have their one entry in this new row";
            taken_by[r - m] = c;
            from[i] = -1 - (r - m);
            ++n_new;
            continue;
        }
        const ColumnIdentity id = column_identity(cd, c);  // kind (a)
        const int same = id.row < 0 ? (id.structural < pd.col_end[0] ? id.structural : -1) : (id.row < m ? slack_of_row(pd, id.row) : -1);
        if (same < 0 || !basic_in_parent[same])
            return where + " has " + std::to_string(below) + " of its " + std::to_string(on_rows) + " entries on the parent's rows (row " +
                   std::to_string(column.index[0]) + " the first) and is not basic in the parent: the child's basic columns are the parent's, and one single-entry column per new row";
        const std::string difference = difference_below(pd.column(same), column, m);
        if (!difference.empty()) return where + " is not " + described(pd, same) + " of the parent on the parent's rows" + difference;
        from[i] = same;
    }
    if (n_new != k)  // (cannot happen with m_child distinct columns of which at most m are the parent's; kept as the statement of the rule)
        return "the child has " + std::to_string(k) + " new rows and " + std::to_string(n_new) + " basic columns with their one entry in a new row";
    if (source) *source = from;
    return "";
}

}  // namespace relp
