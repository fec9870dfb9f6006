// Stand-alone check of reduce_bounded_basis and dual_bounded_inherit_refusal (relp_amd/csrc/dual_inherit.cpp), meant to be built with
// -fsanitize=address,undefined (tests/test_dual_bounded_inherit_host.py does): the reduction of a basis of the formulation to the
// constraint rows, the accepted pairs with the map they give, and every refusal, on models built by hand.  Prints "ok" and exits 0,
// or says which expectation failed and exits 1.
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "dual_inherit.hpp"

using relp::Rat;
using relp::ReducedBasis;
using relp::SparseColumn;
using relp::StandardForm;

namespace {

using Columns = std::vector<std::vector<std::pair<int, long long>>>;

// `equalities` "=" rows, then "<=" rows, over `columns` structural columns; upper[j] < 0: variable j has no upper bound.  The columns
// are the structurals, a slack per "<=" row, a slack per bound row; the rows are the constraint rows, then a bound row per bounded
// variable in variable order.
StandardForm bounded_form(int rows, const Columns& columns, const std::vector<long long>& b, const std::vector<long long>& upper, int equalities = 0) {
    StandardForm form;
    for (size_t j = 0; j < columns.size(); ++j) {
        SparseColumn column;
        for (const auto& [row, value] : columns[j]) column.push(row, Rat(value));
        form.data.constraints.push_back(column);
        relp::Variable variable;
        variable.cost = Rat(-1);
        if (upper[j] >= 0) {
            variable.has_upper = true;
            variable.upper = Rat(upper[j]);
        }
        form.data.variables.push_back(variable);
    }
    for (long long value : b) form.data.b.push_back(Rat(value));
    form.data.nr_equality = equalities;
    form.data.nr_upper = rows - equalities;
    form.data.finalize();
    form.nr_original = (int)columns.size();
    return form;
}

int failures = 0;
void expect(bool condition, const char* what, const std::string& text) {
    if (condition) return;
    std::printf("FAILED: %s (got \"%s\")\n", what, text.c_str());
    ++failures;
}
bool names(const std::string& text, const char* part) { return text.find(part) != std::string::npos; }
std::string listed(const std::vector<int>& values) {
    std::string out;
    for (int v : values) out += std::to_string(v) + " ";
    return out;
}
std::string thrown(const relp::MatrixData& md, int n_art, const std::vector<int>& basis) {
    try {
        relp::reduce_bounded_basis(md, n_art, basis.data());
    } catch (const std::invalid_argument& e) {
        return e.what();
    }
    return "(nothing thrown)";
}

}  // namespace

int main() {
    // parent: 3 "<=" rows (0 .. 2), structural columns 0 .. 2, slacks 3 .. 5; x0 <= 4 and x2 <= 6: bound rows 3 and 4, bound slacks 6 and 7
    const Columns parent_columns = {{{0, 2}, {1, 1}}, {{1, 3}}, {{0, 1}, {2, 5}}};
    const StandardForm parent = bounded_form(3, parent_columns, {4, 6, 10}, {4, -1, 6});
    const relp::MatrixData& pd = parent.data;
    expect(pd.nr_constraints() == 3 && pd.nr_rows() == 5 && pd.nr_columns() == 8, "the parent's shape", "");

    // ---- the reduction ----
    ReducedBasis reduced = relp::reduce_bounded_basis(pd, 0, std::vector<int>{0, 4, 2, 6, 7}.data());
    expect(reduced.basis == std::vector<int>({0, 4, 2}) && reduced.flipped == std::vector<int>(6, 0), "both bound slacks basic: the constraint rows' columns", listed(reduced.basis));
    reduced = relp::reduce_bounded_basis(pd, 0, std::vector<int>{3, 4, 2, 0, 7}.data());  // x0 on its bound row, its slack not basic: at its bound
    expect(reduced.basis == std::vector<int>({3, 4, 2}) && reduced.flipped == std::vector<int>({1, 0, 0, 0, 0, 0}), "a variable at its upper bound is complemented and not basic",
           listed(reduced.basis) + "| " + listed(reduced.flipped));
    reduced = relp::reduce_bounded_basis(pd, 0, std::vector<int>{6, 4, 2, 0, 7}.data());  // x0 basic on its bound row, the bound slack on row 0
    expect(reduced.basis == std::vector<int>({0, 4, 2}) && reduced.flipped == std::vector<int>(6, 0), "a column listed on a bound row takes the free position", listed(reduced.basis));
    reduced = relp::reduce_bounded_basis(pd, 0, std::vector<int>{6, 7, 2, 0, 5}.data());  // two of them: free positions in column order, row 2 kept
    expect(reduced.basis == std::vector<int>({0, 5, 2}), "two columns without a row of their own fill the free positions in column order", listed(reduced.basis));
    reduced = relp::reduce_bounded_basis(pd, 1, std::vector<int>{-1, 4, 2, 6, 7}.data());  // one artificial in front of the provider columns
    expect(reduced.basis == std::vector<int>({0, 5, 3}) && reduced.flipped.size() == 7, "an artificial is its own device column, the others move up", listed(reduced.basis));
    expect(names(thrown(pd, 0, {0, 0, 2, 6, 7}), "bad basis"), "a column listed twice", thrown(pd, 0, {0, 0, 2, 6, 7}));
    expect(names(thrown(pd, 0, {1, 4, 2, 3, 7}), "neither a bounded variable nor its bound slack"), "neither x0 nor its bound slack", thrown(pd, 0, {1, 4, 2, 3, 7}));
    expect(names(thrown(pd, 0, {-1, 4, 2, 6, 7}), "bad basis"), "an artificial the LP does not have", thrown(pd, 0, {-1, 4, 2, 6, 7}));
    expect(relp::column_identity(pd, 1).structural == 1 && relp::column_identity(pd, 4).row == 1 && relp::slack_of_row(pd, 2) == 5, "what a column is", "");

    // ---- the relation ----
    const std::vector<int> parent_basis = {0, 4, 2, 6, 7};
    // child: two cuts appended (constraint rows 3 and 4) over columns 0 and 2, x0 <= 3 now and x1 <= 2 new: slacks 3 .. 7, bound rows 5 .. 7, bound slacks 8 .. 10
    Columns child_columns = parent_columns;
    child_columns[0].push_back({3, 1});
    child_columns[2].push_back({3, -2});
    child_columns[2].push_back({4, 3});
    const StandardForm child = bounded_form(5, child_columns, {4, 6, 10, 1, 2}, {3, 2, 6});
    const std::vector<int> child_basis = {0, 4, 2, 6, 7, 8, 9, 10};
    std::vector<int> source;
    std::string text = relp::dual_bounded_inherit_refusal(parent, child, parent_basis, child_basis, &source);
    expect(text.empty() && source == std::vector<int>({0, 4, 2, -1, -2}), "cuts, a tightened bound and a new bound row are accepted", text + listed(source));
    // the parent holds x0 at its upper bound and slack 3 basic; the child has x2 at its bound and lists its columns in another order
    text = relp::dual_bounded_inherit_refusal(parent, child, {3, 4, 2, 0, 7}, {4, 3, 0, 6, 7, 8, 9, 2}, &source);
    expect(names(text, "position 2") && names(text, "structural variable 0") && names(text, "not basic in the parent"), "a column the parent does not hold basic", text);
    text = relp::dual_bounded_inherit_refusal(parent, child, {3, 4, 2, 0, 7}, {4, 2, 3, 6, 7, 0, 9, 10}, &source);
    expect(text.empty() && source == std::vector<int>({4, 2, 3, -1, -2}), "other positions, a variable at its bound on both sides", text + listed(source));
    const StandardForm tightened = bounded_form(3, parent_columns, {3, 6, 7}, {1, -1, 0});  // k = 0: bounds and right-hand sides only
    text = relp::dual_bounded_inherit_refusal(parent, tightened, parent_basis, parent_basis, &source);
    expect(text.empty() && source == std::vector<int>({0, 4, 2}), "a pure branch is accepted", text);
    const StandardForm free_parent = bounded_form(3, parent_columns, {4, 6, 10}, {-1, -1, -1}), free_child = bounded_form(5, child_columns, {4, 6, 10, 1, 2}, {-1, -1, -1});
    text = relp::dual_bounded_inherit_refusal(free_parent, free_child, {0, 4, 2}, {0, 4, 2, 6, 7}, &source);
    expect(text.empty() && source == std::vector<int>({0, 4, 2, -1, -2}), "a pair without bounds is accepted by the same rule", text);
    text = relp::dual_bounded_inherit_refusal(free_parent, child, {0, 4, 2}, child_basis);
    expect(text.empty(), "bounds on one side only", text);

    text = relp::dual_bounded_inherit_refusal(child, parent, child_basis, parent_basis);
    expect(names(text, "3 constraint rows, fewer than its parent's 5"), "fewer rows than the parent", text);
    Columns changed_columns = child_columns;
    changed_columns[2][0].second = 7;  // row 0 of basic column 2
    text = relp::dual_bounded_inherit_refusal(parent, bounded_form(5, changed_columns, {4, 6, 10, 1, 2}, {3, 2, 6}), parent_basis, child_basis);
    expect(names(text, "position 2") && names(text, "row 0") && names(text, "7/1 in the child, 1/1 in the parent"), "a changed coefficient of a basic column", text);
    changed_columns[2][0].second = 1;
    changed_columns[1][0].second = 9;  // ... of a column that is not basic: no matter
    text = relp::dual_bounded_inherit_refusal(parent, bounded_form(5, changed_columns, {4, 6, 10, 1, 2}, {3, 2, 6}), parent_basis, child_basis);
    expect(text.empty(), "a changed coefficient of a non-basic column", text);
    Columns swapped_columns = child_columns;  // rows 0 and 1 of the parent change places
    swapped_columns[0] = {{0, 1}, {1, 2}, {3, 1}};
    swapped_columns[1] = {{0, 3}};
    swapped_columns[2] = {{1, 1}, {2, 5}, {3, -2}, {4, 3}};
    text = relp::dual_bounded_inherit_refusal(parent, bounded_form(5, swapped_columns, {6, 4, 10, 1, 2}, {3, 2, 6}), parent_basis, child_basis);
    expect(names(text, "position 0") && names(text, "row 0") && names(text, "1/1 in the child, 2/1 in the parent"), "two of the parent's rows in the other order", text);
    text = relp::dual_bounded_inherit_refusal(parent, bounded_form(5, child_columns, {4, 6, 10, 1, 2}, {3, 2, 6}, 1), parent_basis, {0, 3, 2, 5, 6, 7, 8, 9});
    expect(names(text, "row 0 is an equality row in the child and a <= row in the parent"), "a row of another kind in front", text);
    Columns two_entries = child_columns;
    two_entries.push_back({{3, 1}, {4, 1}});  // a new structural column over the two new rows only
    const StandardForm wide = bounded_form(5, two_entries, {4, 6, 10, 1, 2}, {3, 2, 6, -1});  // slacks 4 .. 8, bound slacks 9 .. 11
    text = relp::dual_bounded_inherit_refusal(parent, wide, parent_basis, {0, 5, 2, 3, 8, 9, 10, 11});
    expect(names(text, "position 3") && names(text, "structural variable 3") && names(text, "2 entries") && names(text, "rows 3 and 4"), "a new row whose basic column has two entries", text);
    text = relp::dual_bounded_inherit_refusal(parent, wide, parent_basis, {0, 5, 2, 7, 8, 9, 10, 11});
    expect(text.empty(), "the same model with the slacks on the new rows", text);
    text = relp::dual_bounded_inherit_refusal(parent, child, parent_basis, {0, 4, 2, 1, 7, 8, 9, 10});
    expect(names(text, "position 3") && names(text, "structural variable 1") && names(text, "not basic in the parent"), "a structural column of the parent's rows on a new row", text);

    text = relp::dual_bounded_inherit_refusal(parent, child, {0, -2, 2, 6, 7}, child_basis);
    expect(names(text, "parent's basis holds an artificial") && names(text, "row 1"), "an artificial in the parent's basis", text);
    text = relp::dual_bounded_inherit_refusal(parent, child, parent_basis, {0, 4, 2, 6, 7, 8, -1, 10});
    expect(names(text, "child's basis holds an artificial") && names(text, "row 6"), "an artificial on a bound row of the child's basis", text);
    text = relp::dual_bounded_inherit_refusal(parent, child, parent_basis, {0, 4, 2, 6, 7, 8, 9});
    expect(names(text, "7 entries for 8 rows"), "a basis that is too short", text);
    text = relp::dual_bounded_inherit_refusal(parent, child, parent_basis, {0, 4, 2, 6, 7, 8, 9, 11});
    expect(names(text, "names column 11"), "a column beyond the model", text);
    text = relp::dual_bounded_inherit_refusal(parent, child, parent_basis, {1, 4, 2, 6, 7, 3, 9, 10});
    expect(names(text, "the child's basis: bad basis") && names(text, "neither a bounded variable nor its bound slack"), "a basis that does not reduce", text);

    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
