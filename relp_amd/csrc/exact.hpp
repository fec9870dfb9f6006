// The exact fixed-width simplex's interface (exact.hip) and the entry points of its unit tests.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "model.hpp"

namespace relp {

// One run of the exact fixed-width simplex kernel (exact.hip) at one width: what `relp_get_exact_counters` reports.
constexpr int EX_PROF_WORDS = 40;
struct ExactWidthRecord {
    int limbs = 0, grid = 0;
    long long pivots_total_at_end = 0;            // pivots of the solve so far when this width stopped (overflow) or finished
    double seconds = 0.0;                         // host wall time of this width (upload or widening + kernel)
    double step_seconds[10] = {0};                // the leader's time per step of the loop (x_B, pass B, arg-max, exact weights, tournament, alpha, ratio, update, bookkeeping, pass A)
    long long update_products_needed = 0;         // 64 x 64 -> 128-bit word products of the update of N: what the entries' bit bounds ask for ...
    long long update_products_issued = 0;         // ... and what the waves execute (every lane of a wave runs the longest count among its entries)
};
// exact.hip: the host driver of the exact simplex, and the entry points of its unit tests and of tools/tile_bench.py
void exact_simplex(const StandardForm& form, int device, hipStream_t stream, int first_limbs, int max_limbs, long long max_pivots,
                   int trace_capacity, int* status, int* limbs_used, long long* pivots_phase_one, long long* pivots_phase_two,
                   std::vector<int>* trace, std::string* objective, std::vector<int>* final_basis,
                   std::vector<std::pair<int, long long>>* pivots_survived, int* redundant_rows, std::vector<ExactWidthRecord>* counters, int update_mode, int forced_grid);
void exact_finish_entries(int device, int limbs, int count, const unsigned long long* T, const int* carry, const int* words, int shift, int flip,
                          unsigned long long* N_out, int* bits_out);
void exact_words_test(int device, int limbs, int mode, int count, const unsigned long long* a, const unsigned long long* b, unsigned long long* out);
double exact_tile_bench(int device, int limbs, int tiles, int nb64, int terms, int shift);
// grid_barrier_test.hip
void grid_barrier_test(int device, int grid, int rounds, int reads, int mode, long long limit_ticks, long long* out8);

}  // namespace relp
