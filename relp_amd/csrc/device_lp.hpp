// The device structs every kernel takes by value: the control block, the device LP and the spanning forest of the network carry.
#pragma once
#include <hip/hip_runtime.h>

#include "kernel_limits.hpp"

namespace relp {

// Device control block, written by single-workgroup kernels, polled by the host.
struct Ctl {
    int status;        // 0 running | 1 no entering column | 2 unbounded (ratio test empty) | 3 iteration budget used | 4 refactorise (LU carry)
    int q;             // entering column (device index space: artificials first)
    int p;             // pivot row
    int leaving;       // column that left the basis at row p
    int pending;       // 1: the steepest-edge update of the last pivot is applied by the next pricing pass
    int forced_q;      // >= 0: next iteration must enter this column ...
    int forced_p;      //       ... at this row (zero-level pivots of phase_one.rs:232-278)
    int last_selected; // FirstProfitableWithMemory (pivot_rule.rs:113-150)
    long long iters;   // pivots done in the current phase
    long long budget;  // stop when iters reaches this
    double cbar_q;
    double alpha_pq;
    double gamma_q;
    double xp;
    double minus_obj;  // carry/mod.rs `minus_objective`
    double residual;   // max |I - B Binv| written by the polish
    double scan_value;
    int scan_column;
    int nz_count;      // entries of the ordered non-zero list of alpha_q (written by K2, read by K3)
    int eta_count;     // deferred product form (dense pipeline): pivots not yet folded into the stored inverse
    int touched_count; // columns of the stored inverse that are not unit vectors any more (entries of DeviceLP::tlist)
    double flip_cost;  // implicit bounds: sum of ub_j c_j over the complemented variables (current phase's costs)
    long long bound_flips;  // iterations that moved the entering variable to its other bound without a basis change
    int k2_forced;     // multi-workgroup ratio test: the pivot row of this iteration was given by the caller
    int t_buf;         // fused pivot kernel: which of the two buffers holds the current inverse (0 outside a batch)
    int eta_version;   // deferred product form: pivots made; the kept columns of M live in eta_cols buffer (eta_version & 1)
    int eta_new;       // ... and whether the last pivot added a kept column (its row had none) -- both written by K2
    int rho_buf;       // generated columns: which half of DeviceLP::rho_bits the writers of rho_p mark (flipped by the kernel that decides a pivot)
};

// The control block field by field: a kernel that reads it, edits it and writes it elsewhere keeps it in registers this way (the
// struct assignment `Ctl c = *src` is made of overlapping 16-byte pieces that the compiler keeps on the stack: 176 bytes of scratch
// per lane of the fused pivot kernel).
#if defined(__HIPCC__)
#define RELP_CTL_FIELDS(X) X(status) X(q) X(p) X(leaving) X(pending) X(forced_q) X(forced_p) X(last_selected) X(iters) X(budget) X(cbar_q) \
    X(alpha_pq) X(gamma_q) X(xp) X(minus_obj) X(residual) X(scan_value) X(scan_column) X(nz_count) X(eta_count) X(touched_count) \
    X(flip_cost) X(bound_flips) X(k2_forced) X(t_buf) X(eta_version) X(eta_new) X(rho_buf)
__device__ __forceinline__ void ctl_copy(Ctl& dst, const Ctl& src) {
    static_assert(sizeof(Ctl) == 8 * 4 + 2 * 8 + 7 * 8 + 4 * 4 + 2 * 8 + 5 * 4 + 4, "a field of Ctl is missing from RELP_CTL_FIELDS");
#define RELP_CTL_COPY(f) dst.f = src.f;
    RELP_CTL_FIELDS(RELP_CTL_COPY)
#undef RELP_CTL_COPY
}
#endif

enum : int { ST_RUNNING = 0, ST_NO_ENTERING = 1, ST_UNBOUNDED = 2, ST_BUDGET = 3, ST_REFACTOR = 4, ST_REFACTOR_FAILED = 5, ST_CUTOFF = 6 };  // 4: LU carry, refactorise now;
// 5: the refactorisation kernels gave up (a capacity, a row too long for the eliminating wave): the pivots behind them are no-ops, the host factorises
// 6: the dual loop under an objective cutoff (dual_leave_kernel<.., .., true>): the objective of its basis has reached the cutoff

struct DeviceLP {
    int m = 0, n = 0, n_art = 0, ld = 0;
    // dense block: device columns [dense_first, dense_first + n_dense) also stored dense, column-major, ld = dense_ld
    int n_dense = 0, dense_first = 0, dense_ld = 0;
    double* dense_val = nullptr;
    signed char* dense_val8 = nullptr;  // the same block as signed bytes (every entry an integer in [-128, 127]); rows permuted within 1024-row chunks, dense_ld a multiple of 1024
    int dense_full = 0, dense_csc_start = 0;  // 1: every column of the dense block has m entries (rows 0 .. m-1 in order), the first of them at dense_csc_start in the CSC
    int dense_lane = 0;  // 1: dense_val8 in tiles of 16 columns x 64 rows instead (price_dense_lane_kernel), -pi / rho / w zero-padded to dense_ld
    float* dense_val32 = nullptr;  // the same block as float, when every entry is exactly representable (then dense_val is not allocated)
    double* alpha_part = nullptr;  // slices of the multi-block FTRAN, [n_slices][m]
    double* alpha_in = nullptr;    // their fixed-order sum (with the pending etas applied): what K2 reads when preselected
    // Deferred product form (eta_cap > 0, dense pipeline only).  The current inverse is  M * Binv  with
    //   M = E_k ... E_1 = I + sum_c (eta_cols[:, c] - e_{eta_rows[c]}) e_{eta_rows[c]}'        (k = ctl->eta_count <= eta_cap)
    // i.e. eta_cols[:, c] is column eta_rows[c] of M.  Binv itself is only rewritten every eta_cap pivots (one rank-k
    // update); per pivot the passes over it are read-only (FTRAN, and one BTRAN pass for rho_p and w together).
    int eta_cap = 0;
    double* eta_cols = nullptr;    // [2][eta_cap][ld]: two copies, the current one is copy ctl->eta_version & 1 (each pivot writes the other)
    int* eta_rows = nullptr;       // [eta_cap]
    int* eta_slot = nullptr;       // [m]: slot of row i in eta_rows, or -1
    double* eta_gather = nullptr;  // [eta_cap][m]: rows eta_rows[c] of Binv, gathered before the rank-k update
    double* eta_dot_part = nullptr;  // [eta_cap][ceil(m / 64)]: alpha_reduce_kernel's per-block shares of alpha' M[:, c]
    // Column j of the STORED inverse is still the unit vector e_j until a row-j pivot has been folded in (E e_j = e_j for
    // every eta of another row; the polish keeps such columns exactly).  touched[j] / tlist record the others, so that the
    // FTRAN and BTRAN passes and the rank-k update only stream columns that carry information.
    int* slack_of_row = nullptr;   // [m] dense pipeline whose sparse part is one single-entry column per row: that column (or -1); the
                                   // BTRAN pass then prices those columns itself (btran_pass_kernel) and no separate launch does
    int track_touched = 0;         // 1: touched / tlist are maintained (deferred product form, or m > 2048)
    int* touched = nullptr;        // [m] 0/1
    int* tlist = nullptr;          // [m] touched columns in the order they were folded in
    // CSC of [artificial identity columns | provider columns] (matrix_data.rs:291-329 materialised once)
    int* col_start = nullptr;
    int* row_index = nullptr;
    double* value = nullptr;
    // CSR of the same matrix (for the residual I - B Binv)
    int* row_start = nullptr;
    int* col_index = nullptr;
    double* row_value = nullptr;
    double* cost = nullptr;      // current phase (n)
    double* cost1 = nullptr;     // phase one: 1 on artificials
    double* cost2 = nullptr;     // phase two: provider costs
    double* rhs = nullptr;       // right_hand_side() (m)
    double* xB = nullptr;        // Carry::b (m)
    double* minus_pi = nullptr;  // Carry::minus_pi (m)
    int* basis = nullptr;        // Carry::basis_indices (m)
    int* pos = nullptr;          // column -> row (the Tableau's basis_columns set) (n); non-basic: -1 at 0 | -2 at its upper bound
                                 // (held complemented) | -3 fixed, both bounds coincide: never priced (implicit bounds)
    double* gamma = nullptr;     // steepest-edge weights (n)
    double* cb = nullptr;        // c_B (m): costs of the basic columns, written by cb_kernel for the -pi refresh
    int* cb_idx = nullptr;       // (m + 1) ordered non-zero positions of c_B; [m] = their number
    double* Binv = nullptr;      // explicit basis inverse, COLUMN-major: Binv(i, j) at [j*ld + i]
    double* Binv2 = nullptr;     // second buffer for the polish
    double* R = nullptr;         // residual I - B Binv
    double* alpha = nullptr;     // B^-1 a_q (m)
    double* rho = nullptr;       // row p of the NEW inverse (m)
    double* w = nullptr;         // w = alpha_q' Binv_old (m)
    int* nz_index = nullptr;     // rows with alpha_i != 0 (plus p), ascending (m)
    double* nz_alpha = nullptr;  // their alpha values (m)
    double* cand_key = nullptr;  // per pricing block
    int* cand_j = nullptr;
    double* cand_cbar = nullptr;
    int* cand_rows = nullptr;    // first ELL_W entries of each block's best column (so K2 needs no dependent fetch)
    double* cand_vals = nullptr;
    int* cand_len = nullptr;     // nnz of that column (> ELL_W: the rest comes from the CSC)
    // padded copy of the first ELL_W entries of every column (value 0 padding): no col_start dependency in K1
    int ell_w = ELL_W;           // padded width in use: 2 when no column has more than two entries and m is large, else ELL_W
    int* ell_rows = nullptr;
    double* prw = nullptr;       // ell_w == 2, columns with values: (-pi_r, rho_r, w_r, 0) packed per row, kept beside the three vectors by their writers
    // ... and the same as one BIT per row, two buffers of rho_words words: the writers of rho_p set bits in buffer Ctl::rho_buf,
    // the pricing pass copies that buffer into LDS (8 KB for config 5) and clears the other one, the kernel that decides the next
    // pivot flips Ctl::rho_buf.  Bits are only ever a superset of the non-zeros (a stale bit costs one gather of an exact zero).
    unsigned* rho_bits = nullptr;
    int price_unit_pairs = 0;  // RELP_PRICE_UNIT_PAIRS: the round-2 pricing pass (two lanes per arc, byte table), for A/B and the parity test
    int rho_words = 0;  // per buffer, a multiple of 4; 0: no bit table (too many rows for LDS: the byte table is gathered instead)
    unsigned char* rho_nz = nullptr;  // generated columns without the bit table: rho_r != 0, one byte per row (rho and w are gathered only where this says so)
    double* ell_vals = nullptr;
    // generated incidence columns (ell_w == 2, every value +-1, integer costs in [-127, 127]): ell_rows carries the sign in
    // bit 31 (0x7fffffff: no entry), ell_vals is not allocated, and pricing reads the cost as a signed byte
    signed char* cost8 = nullptr;   // current phase (n)
    signed char* cost8_2 = nullptr; // phase two (phase one: zeros on every priced column)
    // Implicit upper bounds (relp_options.implicit_bounds): the `VariableBound` / `SlackBound` rows of `MatrixData`
    // (matrix_data.rs:104-112: x_j + s = u_j) are not rows of the device LP; a variable at its upper bound is held in
    // complemented form x_j = u_j - x'_j, so every non-basic variable sits at zero and pricing is unchanged up to the
    // sign of the column: pos[j] == -2 marks a complemented non-basic column, flipped[j] the complemented ones (basic too).
    double* ub = nullptr;        // [n] upper bound of each device column (+inf without one); nullptr = mode off
    double* xub = nullptr;       // [m] upper bound of the variable that is basic in row i
    int* flipped = nullptr;      // [n] 1: the column is held in complemented form
    double* rhs0 = nullptr;      // [m] right-hand side of the file (rhs holds b minus the complemented columns' u_j a_j)
    double* k2_partd = nullptr;  // multi-workgroup ratio test (m > 8192): per-workgroup partial sums / minima / candidate keys
    int* k2_parti = nullptr;     //   ... candidate rows, their basic columns, non-zero counts and list offsets
    double* scratch = nullptr;   // m or n doubles for the fine-grained ops
    Ctl* ctl = nullptr;
    Ctl* ctl_mirror = nullptr;   // fused pivot kernel: the handle's pinned host copy of the control block, as the device addresses it; commit_kernel
                                 // writes the committed block there too, so that the host reads the end of a batch without a copy
    // fused pivot kernel (pivot_fused_kernel, small LPs): x_B, basis and control block exist twice; pivot k of a batch reads copy
    // k & 1 and writes the other (kernels.hip, K23)
    struct State {
        Ctl* ctl = nullptr;
        double* xB = nullptr;
        int* basis = nullptr;
    };
    State state[2];
    unsigned long long* dbg = nullptr;  // diagnostic builds only (-DRELP_STAMPS): per-segment cycle sums of K2
};

#ifdef __HIPCC__
// Generated incidence columns: row j of the new rho_p for the pricing pass -- its bit in this pivot's half of rho_bits (set only:
// the pricing pass clears the other half), its byte in rho_nz where that table is kept.
__device__ __forceinline__ void mark_rho_row(const DeviceLP& lp, int rho_buf, int j, double r) {
    if (lp.rho_nz) lp.rho_nz[j] = r != 0.0;
    if (r != 0.0 && lp.rho_words) atomicOr(lp.rho_bits + (size_t)rho_buf * lp.rho_words + (j >> 5), 1u << (j & 31));
}
#endif

// Spanning-forest carry (relp_options.carry == RELP_CARRY_NETWORK, network_carry.hip).  Every basis of a network LP is a spanning
// forest of the rows: a basic incidence column joins two rows, a basic single-entry column (artificial, arc at a removed vertex) is
// the root arc of its row's tree.  B^-1 (slot i, row j) = sign[child[i]] when row j lies below the arc of slot i, else 0.
struct NetTree {
    int* parent = nullptr;        // [m] row above this row in its tree (-1: a root)
    int* slot = nullptr;          // [m] basis slot of the arc to the parent (a root: its root arc)
    signed char* sign = nullptr;  // [m] entry of that basic column (negated when it is held complemented) at this row
    int* child = nullptr;         // [m] slot -> the row below its arc
    int* mark = nullptr;          // [m] walk stamps of the entering column's path search
    int* chain = nullptr;         // [m] rows of one endpoint's root path (scratch of that search)
    int* path = nullptr;          // [m] slots where alpha_in is non-zero (cleared by the next search)
    int* state = nullptr;         // [2] stamp, path length
    unsigned long long* stats = nullptr;  // [NS_WORDS] RELP_SW_NETWORK_STATS only: counters over the pivots since phase one began
};
enum : int { NS_PIVOTS = 0, NS_SUBTREE_SUM, NS_SUBTREE_MAX, NS_DEPTH_SUM, NS_DEPTH_MAX, NS_SUBTREE_NOW, NS_PATH_SUM, NS_PATH_MAX, NS_WORDS };

}  // namespace relp
