// Pricing and the choice of the entering column, stated ONCE for every f64 kernel that prices a column or folds the pricing
// workgroups' candidates (kernels.hip: price_kernel, price_unit_kernel, price_dense_kernel, price_dense_lane_kernel,
// btran_pass_kernel's slack pricing, ftran_partial_kernel, ftran_ratio_kernel, k2l_ftran_kernel, the k2f_* front half;
// lu.hip: lu_pivot_kernel; network_carry.hip: net_ftran_kernel; many.hip: many_kernel).  The sibling of pivot_step.hpp.
//   restates  SteepestDescentAlongObjective::select_primal_pivot_column   strategy/pivot_rule.rs:221-241
//             SteepestDescentAlongObjective::after_basis_update            strategy/pivot_rule.rs:243-296
//             Tableau::relative_cost / Carry::cost_difference             tableau/mod.rs:106-112, carry/mod.rs:606-611
// The kernels keep what is theirs -- how they load a column, what they stage in LDS, how they sum a column, and the short cut
// "a weight without an entry in the pivot row does not change" where the fetch is skipped -- and take the rules from here.
// Everything is __forceinline__; RULE and `bounded` fold away where the caller passes a constant.
#pragma once
#include "../../include/relp_amd.h"
#include "pivot_step.hpp"

namespace relp {

// ---- column state (positions: pivot_step.hpp) -----------------------------------------------------------------------------------
// Priced: non-basic at 0 (-1) or at its upper bound (-2).  -3, a fixed variable, is never priced; -2 cannot occur without bounds.
__device__ __forceinline__ bool column_priced(int pos, bool bounded = true) { return pos == -1 || (bounded && pos == -2); }
// A column at its upper bound is held in complemented form: it is priced, and enters, with the opposite sign.
__device__ __forceinline__ double column_sign(int pos, bool bounded = true) { return (bounded && pos == -2) ? -1.0 : 1.0; }

// ---- the steepest-edge weight of column j after a pivot ---------------------------------------------------------------------------
// d_rho = rho_p . a_j, d_w = w . a_j; gamma_q, alpha_pq: the entering column's weight and the pivot element.  The leaving column
// takes gamma_q / alpha_pq^2 (pivot_rule.rs:294-295), every other one the Goldfarb-Reid update (pivot_rule.rs:262-288).  Two
// statements on purpose: the compiler contracts within an expression, and the kernels are tested bit for bit against each other.
__device__ __forceinline__ double weight_after_pivot(double gam, double d_rho, double d_w, double gamma_q, double alpha_pq, bool is_leaving) {
    if (is_leaving) return gamma_q / (alpha_pq * alpha_pq);
    const double sq = d_rho * d_rho;
    gam = gam - 2.0 * d_rho * d_w + sq * gamma_q;
    gam = fmax(gam, 1.0 + sq);
    return gam;
}

// ---- candidacy and key per pivot rule: the larger key wins ------------------------------------------------------------------------
// steepest edge cbar^2 / gamma | Dantzig -cbar | first profitable: the lowest column | first profitable with memory: the first
// one after `last`, the column selected before (< 0: none), wrapping round the n columns; `last` itself is no candidate.
template <int RULE>
__device__ __forceinline__ double price_key(double cbar, double tol_dual, double gam, int j, int last, int n, bool& candidate) {
    candidate = cbar < -tol_dual;
    if (RULE == RELP_PIVOT_STEEPEST_EDGE) return cbar * cbar / gam;
    if (RULE == RELP_PIVOT_DANTZIG) return -cbar;
    if (RULE == RELP_PIVOT_FIRST_PROFITABLE) return -(double)j;
    if (last >= 0 && j == last) candidate = false;
    const long long rank = (last < 0) ? j : (j > last ? (long long)j - last - 1 : (long long)j + n - last);
    return -(double)rank;
}

// ---- a candidate against a running best: equal keys go to the larger column under steepest edge (the reference keeps the last
//      maximum), to the smaller one otherwise.  (key, rank) form: `block` is the pricing workgroup that offers j (its slot).
template <int RULE>
__device__ __forceinline__ unsigned long long entering_rank(int j, int block) {
    const unsigned long long order = (RULE == RELP_PIVOT_STEEPEST_EDGE) ? (unsigned long long)(0x7fffffff - j) : (unsigned long long)j;
    return (order << 16) | (unsigned long long)block;
}
template <int RULE>
__device__ __forceinline__ int entering_column(unsigned long long rank) {
    const int order = (int)(rank >> 16);
    return (RULE == RELP_PIVOT_STEEPEST_EDGE) ? 0x7fffffff - order : order;
}
__device__ __forceinline__ int entering_block(unsigned long long rank) { return (int)(rank & 0xffff); }
template <int RULE>
__device__ __forceinline__ void offer_entering(double key, int j, int block, double& best_key, unsigned long long& best_rank) {
    if (j >= 0) keep_better(key, entering_rank<RULE>(j, block), best_key, best_rank);
}
// Cand form (the pricing kernels, whose winner carries a payload): returns "this one won", and the caller updates its payload.
__device__ __forceinline__ Cand no_candidate(int aux = 0) {
    Cand c;
    c.key = 0.0;
    c.idx = -1;
    c.aux = aux;
    return c;
}
template <int RULE>
__device__ __forceinline__ bool offer_candidate(Cand& best, double key, int j) {
    Cand c;
    c.key = key;
    c.idx = j;
    c.aux = 0;
    best = (RULE == RELP_PIVOT_STEEPEST_EDGE) ? better<TIE_LARGER_IDX>(best, c) : better<TIE_SMALLER_IDX>(best, c);
    return best.idx == j;
}
template <int RULE>
__device__ __forceinline__ Cand block_best_candidate(Cand best, Cand* s) {
    return (RULE == RELP_PIVOT_STEEPEST_EDGE) ? block_best<TIE_LARGER_IDX>(best, s) : block_best<TIE_SMALLER_IDX>(best, s);
}

// ---- the candidate slots: one per pricing workgroup --------------------------------------------------------------------------------
// cand_j = -1: the workgroup found no candidate, and nothing else of the slot is read.  Otherwise cand_key and cand_cbar are the
// column's key and (signed) reduced cost, and cand_len says where its entries are: -1, read the column from the CSC; >= 0, the
// column's length, with its first min(len, ELL_W) entries inline in cand_rows / cand_vals[slot * ELL_W ..] (padding: row 0, value 0;
// a column longer than ELL_W continues in the CSC).
__device__ __forceinline__ void publish_candidate(const DeviceLP& lp, int slot, double key, int j, double cbar, int len) {
    lp.cand_key[slot] = key;
    lp.cand_j[slot] = j;
    lp.cand_cbar[slot] = cbar;
    lp.cand_len[slot] = len;
}
__device__ __forceinline__ void publish_entry(const DeviceLP& lp, int slot, int e, int row, double val) {
    lp.cand_rows[(size_t)slot * ELL_W + e] = row;
    lp.cand_vals[(size_t)slot * ELL_W + e] = val;
}
__device__ __forceinline__ void publish_no_candidate(const DeviceLP& lp, int slot) { lp.cand_j[slot] = -1; }

// ---- the fold over the slots: this thread's best (start from key 0, rank RANK_NONE), then the workgroup's ---------------------------
template <int RULE>
__device__ __forceinline__ void fold_candidates(const int* cand_j, const double* cand_key, int n_blocks, int tid, int n_threads,
                                                double& key, unsigned long long& rank) {
    for (int b = tid; b < n_blocks; b += n_threads) offer_entering<RULE>(cand_key[b], cand_j[b], b, key, rank);
}
// s_key / s_rank: one slot per wave (block_argbest, whose SLOTS_FREE this passes on).  Returns q for every thread, -1: none; `block`:
// the slot that offered it.
template <int RULE, bool SLOTS_FREE = false>
__device__ __forceinline__ int entering_winner(double key, unsigned long long rank, double* s_key, unsigned long long* s_rank, int& block) {
    block_argbest<SLOTS_FREE>(key, rank, s_key, s_rank);
    if (rank == RANK_NONE) return -1;
    block = entering_block(rank);
    return entering_column<RULE>(rank);
}

// ---- the reduced cost of a column that was not priced (a forced entering column): c_q - pi . a_q, unsigned -- the caller applies
//      the sign of a complemented column where it needs it.  The same sum in the same order as a pricing pass over the CSC.
__device__ __forceinline__ double reduced_cost_of(double cost_q, const int* col_start, const int* row_index, const double* value,
                                                  const double* minus_pi, int q) {
    double cb = cost_q;
    for (int e = col_start[q]; e < col_start[q + 1]; ++e) cb += value[e] * minus_pi[row_index[e]];
    return cb;
}

}  // namespace relp
