// What the getters of exact vectors share between a handle (capi.cpp) and relp_many (many.hip): the exact back-mapping to the
// variables of the file, which witness a verdict has, and the return protocol of relp_get_solution_exact.
#pragma once
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/relp_amd.h"
#include "bigrat.hpp"
#include "model.hpp"

namespace relp {

using ExactValues = std::vector<std::pair<int, std::string>>;  // (index, "num/den" reduced, den > 0), non-zero entries, ascending

// Exact back-mapping of general_form/mod.rs:753-771, 840-934 (the f64 twin is StandardForm::original_solution).
inline std::vector<BigRat> original_solution_exact(const StandardForm& form, const std::vector<BigRat>& standardised) {
    const bool identity = form.active_to_original.empty();
    std::vector<BigRat> out((size_t)form.nr_file_variables());
    std::vector<char> known(out.size(), 0);
    for (int j = 0; j < form.nr_original; ++j) {
        BigRat x = standardised[j];
        if (j < (int)form.free_negative_part.size() && form.free_negative_part[j] >= 0) x -= standardised[form.free_negative_part[j]];
        x -= BigRat(form.data.variables[j].shift);
        if (form.data.variables[j].flipped) x = -x;
        const int original = identity ? j : form.active_to_original[j];
        out[original] = x;
        known[original] = 1;
    }
    bool progress = true;
    while (progress) {
        progress = false;
        for (const auto& [original, how] : form.removed) {
            if (known[original]) continue;
            bool ready = true;
            BigRat value(how.constant);
            if (how.function_of_others)
                for (const auto& [k, c] : how.coefficients) {
                    if (!known[k]) { ready = false; break; }
                    value -= BigRat(c) * out[k];
                }
            if (ready) {
                out[original] = value;
                known[original] = 1;
                progress = true;
            }
        }
    }
    return out;
}

// The exact solution a caller sees, from the exact values of the basic provider columns (slacks included).  original == 0:
// reconstruct_solution (matrix_data.rs:402-411), the slack columns are dropped; else the variables of the file.
inline ExactValues exact_solution_values(const StandardForm& form, const ExactValues& basics, bool original) {
    const int n_structural = form.data.nr_normal_variables();
    ExactValues values;
    if (!original) {
        for (const auto& entry : basics)
            if (entry.first < n_structural) values.push_back(entry);
        return values;
    }
    std::vector<BigRat> standardised((size_t)n_structural);
    for (const auto& [j, text] : basics)
        if (j < n_structural) standardised[j] = BigRat::parse(text);
    const std::vector<BigRat> full = original_solution_exact(form, standardised);
    for (size_t j = 0; j < full.size(); ++j)
        if (!full[j].is_zero()) values.push_back({(int)j, full[j].to_string()});
    return values;
}

// Empty when a certified result of `kind` has the witness `which` (the table of relp_witness, include/relp_amd.h); else the
// message that names the combination.
inline std::string witness_refusal(int kind, int which) {
    static const char* const names[3] = {"RELP_WITNESS_PRIMAL", "RELP_WITNESS_DUAL", "RELP_WITNESS_RAY"};
    const bool defined = which == RELP_WITNESS_PRIMAL ? (kind == RELP_RESULT_FINITE_OPTIMUM || kind == RELP_RESULT_UNBOUNDED)
                         : which == RELP_WITNESS_DUAL ? (kind == RELP_RESULT_FINITE_OPTIMUM || kind == RELP_RESULT_INFEASIBLE)
                                                      : kind == RELP_RESULT_UNBOUNDED;
    if (defined) return std::string();
    const char* result = kind == RELP_RESULT_FINITE_OPTIMUM ? "FINITE_OPTIMUM" : kind == RELP_RESULT_INFEASIBLE ? "INFEASIBLE"
                         : kind == RELP_RESULT_UNBOUNDED    ? "UNBOUNDED" : "result without a certificate";
    return std::string("a certified ") + result + " has no " + names[which];
}

// The return protocol of relp_get_solution_exact: *count, *length (bytes needed in `buffer`), then index[k] and the texts separated by
// '\n' and terminated by 0.  index == NULL and buffer == NULL: the two sizes only.
inline int32_t return_exact_values(const ExactValues& values, int32_t capacity, int32_t* count, int32_t* index, char* buffer,
                                   int64_t buffer_capacity, int64_t* length) {
    *count = (int32_t)values.size();
    int64_t needed = 0;
    for (const auto& entry : values) needed += (int64_t)entry.second.size() + 1;
    if (length) *length = needed;
    if (!index && !buffer) return RELP_OK;  // size query
    if (capacity < *count || buffer_capacity < needed || !index || !buffer) return RELP_ERR_ARGUMENT;
    int64_t at = 0;
    for (size_t k = 0; k < values.size(); ++k) {
        index[k] = values[k].first;
        std::memcpy(buffer + at, values[k].second.data(), values[k].second.size());
        at += (int64_t)values[k].second.size();
        buffer[at++] = k + 1 < values.size() ? '\n' : '\0';
    }
    return RELP_OK;
}

}  // namespace relp
