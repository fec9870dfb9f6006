// Stand-alone check of dual_inherit_refusal (relp_amd/csrc/dual_inherit.cpp), meant to be built with -fsanitize=address,undefined
// (tests/test_dual_inherit_host.py does): the accepted pairs and every refusal, on models built by hand.  Prints "ok" and exits 0,
// or says which expectation failed and exits 1.
#include <cstdio>
#include <string>
#include <vector>

#include "dual_inherit.hpp"

using relp::Rat;
using relp::SparseColumn;
using relp::StandardForm;

namespace {

// `rows` "<=" rows over `columns` structural columns: a slack per row behind them (MatrixData's UpperIneq group).
StandardForm less_form(int rows, const std::vector<std::vector<std::pair<int, long long>>>& columns, const std::vector<long long>& b) {
    StandardForm form;
    for (const auto& entries : columns) {
        SparseColumn column;
        for (const auto& [row, value] : entries) column.push(row, Rat(value));
        form.data.constraints.push_back(column);
        relp::Variable variable;
        variable.cost = Rat(-1);
        form.data.variables.push_back(variable);
    }
    for (long long value : b) form.data.b.push_back(Rat(value));
    form.data.nr_upper = rows;
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

}  // namespace

int main() {
    // parent: 3 rows, 3 structural columns (0 .. 2), slacks 3 .. 5; basis: column 0 on row 0, slack 4, column 2 on row 2
    const std::vector<std::vector<std::pair<int, long long>>> parent_columns = {{{0, 2}, {1, 1}}, {{1, 3}}, {{0, 1}, {2, 5}}};
    const StandardForm parent = less_form(3, parent_columns, {4, 6, 10});
    const std::vector<int> parent_basis = {0, 4, 2};
    // child: two cuts appended (rows 3 and 4) over columns 0 and 2; its slacks are columns 3 .. 7
    auto child_columns = parent_columns;
    child_columns[0].push_back({3, 1});
    child_columns[2].push_back({3, -2});
    child_columns[2].push_back({4, 3});
    const StandardForm child = less_form(5, child_columns, {4, 6, 10, 1, 2});
    const std::vector<int> child_basis = {0, 4, 2, 6, 7};

    std::string text = relp::dual_inherit_refusal(parent, child, parent_basis, child_basis);
    expect(text.empty(), "the cut child is accepted", text);
    const StandardForm tightened = less_form(3, parent_columns, {3, 6, 7});  // k = 0: another right-hand side only
    text = relp::dual_inherit_refusal(parent, tightened, parent_basis, parent_basis);
    expect(text.empty(), "a child that differs in its right-hand side is accepted", text);

    text = relp::dual_inherit_refusal(child, parent, child_basis, parent_basis);
    expect(names(text, "fewer than its parent's 5"), "fewer rows than the parent", text);

    auto changed_columns = child_columns;
    changed_columns[2][0].second = 7;  // row 0 of basic column 2
    const StandardForm changed = less_form(5, changed_columns, {4, 6, 10, 1, 2});
    text = relp::dual_inherit_refusal(parent, changed, parent_basis, child_basis);
    expect(names(text, "position 2") && names(text, "row 0") && names(text, "7/1") && names(text, "1/1"), "a changed coefficient of a basic column", text);
    auto dropped_columns = child_columns;
    dropped_columns[0].erase(dropped_columns[0].begin() + 1);  // row 1 of basic column 0 is gone in the child
    text = relp::dual_inherit_refusal(parent, less_form(5, dropped_columns, {4, 6, 10, 1, 2}), parent_basis, child_basis);
    expect(names(text, "position 0") && names(text, "row 1") && names(text, "no entry in the child"), "a dropped entry of a basic column", text);
    auto added_columns = child_columns;
    added_columns[0].insert(added_columns[0].begin() + 2, {2, 9});  // ... and one it did not have
    text = relp::dual_inherit_refusal(parent, less_form(5, added_columns, {4, 6, 10, 1, 2}), parent_basis, child_basis);
    expect(names(text, "position 0") && names(text, "row 2") && names(text, "no entry in the parent"), "an added entry of a basic column", text);

    text = relp::dual_inherit_refusal(parent, child, parent_basis, {2, 4, 0, 6, 7});
    expect(names(text, "position 0") && names(text, "column 2 of the child"), "two positions swapped", text);
    text = relp::dual_inherit_refusal(parent, child, parent_basis, {0, 4, 2, 1, 7});
    expect(names(text, "row 3") && names(text, "column 1") && names(text, "not the slack"), "a structural column on a new row", text);
    text = relp::dual_inherit_refusal(parent, child, parent_basis, {0, 4, 2, 7, 6});
    expect(names(text, "row 3") && names(text, "column 7") && names(text, "in row 4"), "the slack of another new row", text);

    text = relp::dual_inherit_refusal(parent, child, {0, -2, 2}, child_basis);
    expect(names(text, "parent's basis holds an artificial") && names(text, "row 1"), "an artificial in the parent's basis", text);
    text = relp::dual_inherit_refusal(parent, child, parent_basis, {0, 4, 2, -1, 7});
    expect(names(text, "child's basis holds an artificial") && names(text, "row 3"), "an artificial in the child's basis", text);
    text = relp::dual_inherit_refusal(parent, child, parent_basis, {0, 4, 2, 6});
    expect(names(text, "4 entries for 5 rows"), "a basis that is too short", text);
    text = relp::dual_inherit_refusal(parent, child, parent_basis, {0, 4, 2, 6, 8});
    expect(names(text, "names column 8"), "a column beyond the model", text);

    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
