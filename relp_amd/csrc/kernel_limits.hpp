// The limits of the kernels that the load-time plan reads (kernel_path.cpp): sizes shared by the kernels that have them and the host
// code that chooses between kernels.  No HIP: constants and inline host functions only.
#pragma once
#include <cstddef>

namespace relp {

constexpr int WAVE = 64;
constexpr int ELL_W = 8;            // padded entries per column = lanes per column in the pricing kernel
constexpr int PRICE_UNIT_ARCS = 4;  // arcs per lane of price_unit_kernel
constexpr size_t PRICE_LDS_CONFIGURED = 160 * 1024 - 1024;  // the dynamic LDS a pricing workgroup may ask for (configure_lds)
inline int price_columns_per_block(int ell_w, bool generated) { return generated ? 256 * PRICE_UNIT_ARCS : 256 / ell_w; }

// column-per-lane pricing of the dense block (price_dense_lane_kernel)
constexpr int K1C_MAX_THREADS = 512, K1C_U = 4, K1C_COLS = 16, K1C_TILE_ROWS = 64;
inline int dense_lane_slots(int n_dense) { return (n_dense + K1C_COLS - 1) / K1C_COLS; }
inline int dense_lane_threads(int m) { return m > 1024 ? 512 : 256; }
inline int dense_lane_ld(int m) { const int unit = K1C_TILE_ROWS * (dense_lane_threads(m) / WAVE) * K1C_U; return (m + unit - 1) / unit * unit; }

// deferred product form (alpha_reduce_kernel, btran_pass_kernel)
constexpr int ETA_MAX = 32;
inline int eta_max() { return ETA_MAX; }
inline int btran_pass_blocks() { return 256; }

// the register-resident ratio test (ftran_ratio_fast_kernel, up to 8192 rows) and the fused pivot (pivot_fused_kernel, up to 2048)
constexpr int K2F_THREADS = 512;
constexpr int K2F_MAX_BLOCKS = 2048;
constexpr int KF_MAX_R = 4;  // rows per thread: 2 up to 1024 rows, 4 up to 2048 (as ftran_ratio_fast_kernel<RULE, R>)
constexpr int KF_MAX_M = KF_MAX_R * K2F_THREADS;
inline bool fast_k2_available(int m, int n_price_blocks) { return n_price_blocks <= K2F_MAX_BLOCKS && m <= 16 * K2F_THREADS; }
inline bool fused_pivot_available(int m, int n_price_blocks) { return m <= KF_MAX_M && n_price_blocks <= K2F_MAX_BLOCKS; }

// LU carries (lu.hip): all kernels single-workgroup
constexpr int LU_MAX_SLOTS = 64;  // one wave solves T
constexpr int LU_THREADS = 1024;
// LDS of the solve kernels: the two vectors (16 bytes per row), the mask of the replaced positions, one count per 64 rows for
// the ordered compactions, reductions, and the trailing block T with its four slot vectors.
// `inverse_vectors`: 0 = the Forrest-Tomlin form; 4 / 3 = the inverse-factor form with four vectors in LDS (a product is out of
// place and the BTRAN has two right-hand sides) or, for the rows that leaves no room for, with three (the two right-hand sides go
// through the factors one after the other: twice the passes over them).
inline size_t lu_lds_fixed_bytes(int m, int max_updates, int inverse_vectors = 0) {
    const size_t mm = (size_t)((m + 1) & ~1);
    if (inverse_vectors)  // no T / MF; the per-wave partials of M' r
        return (size_t)inverse_vectors * mm * sizeof(double) + ((size_t)(m + 31) / 32 + 2) * sizeof(int) + ((size_t)(m + 63) / 64 + 4) * sizeof(int) + 64 * sizeof(double) +
               ((size_t)4 * LU_MAX_SLOTS + (size_t)2 * (LU_THREADS / 64) * LU_MAX_SLOTS) * sizeof(double) + 256;
    return 2 * mm * sizeof(double) + ((size_t)(m + 31) / 32 + 2) * sizeof(int) + ((size_t)(m + 63) / 64 + 4) * sizeof(int) + 64 * sizeof(double) +
           ((size_t)2 * max_updates * (max_updates + 1) + 4 * LU_MAX_SLOTS) * sizeof(double) + 256;
}
constexpr size_t LU_LDS_TOTAL = 160 * 1024 - 1024;  // what a kernel may ask for (static LDS of the fused kernel comes on top)
inline int lu_inverse_vectors(int m, int max_updates) {  // 4 when they fit, else 3, else 0 (does not fit at all)
    for (int vectors = 4; vectors >= 3; --vectors)
        if (lu_lds_fixed_bytes(m, max_updates, vectors) <= LU_LDS_TOTAL - 2048) return vectors;
    return 0;
}
inline bool lu_fits_lds(int m, int max_updates, bool inverse_factors = false) {  // max_updates: the update slots the kernels will be given (T is max_updates^2 doubles of LDS)
    if (max_updates < 1) max_updates = 1;
    if (max_updates > LU_MAX_SLOTS) max_updates = LU_MAX_SLOTS;
    if (inverse_factors) return lu_inverse_vectors(m, max_updates) != 0;
    return lu_lds_fixed_bytes(m, max_updates, 0) <= LU_LDS_TOTAL - 2048;
}

}  // namespace relp
