// Launch helpers that one file defines and another calls: the f64 pipeline of kernels.hip and the forest carry's row of the inverse
// (network_carry.hip).  Included by the defining file too, so that a changed parameter list is a diagnostic and not a link error.
#pragma once
#include "device_lp.hpp"
#include "kernel_path.hpp"

namespace relp {

// kernels.hip (the limits the load-time plan reads -- dense_lane_slots, fast_k2_available, eta_max ... -- are in kernel_limits.hpp)
void launch_price(const DeviceLP& d, const KernelPath& path, PriceKernel kernel, int rule, int skip_weights, double tol, hipStream_t s);
void launch_price_dense(const DeviceLP& d, const KernelPath& path, int skip_weights, double tol, hipStream_t s);
void configure_dense_lds();
void launch_ftran_partial(const DeviceLP& d, int n_slices, int n_price_blocks, int rule, hipStream_t s);
void configure_lds();
void launch_ftran_ratio(const DeviceLP& d, const KernelPath& path, int rule, double tol_pivot, double harris_delta, int skip_artificial_rows,
                        int mode, int n_alpha_slices, hipStream_t s);
void launch_update(const DeviceLP& d, const KernelPath& path, hipStream_t s);
void launch_pivot_fused(const DeviceLP& d, const KernelPath& path, int rule, int parity, double tol_pivot, double harris_delta,
                        int skip_artificial_rows, hipStream_t s);
void launch_begin_batch(const DeviceLP& d, long long add, hipStream_t s);
void launch_commit(const DeviceLP& d, int parity, hipStream_t s);
void launch_budget(const DeviceLP& d, long long add, hipStream_t s);
void launch_pi(const DeviceLP& d, hipStream_t s);
void launch_cb(const DeviceLP& d, hipStream_t s);
void launch_k2l_preselected(const DeviceLP& d, double tol_pivot, double harris_delta, int skip_artificial_rows, hipStream_t s);
void launch_xb(const DeviceLP& d, hipStream_t s);
void launch_gamma_init(const DeviceLP& d, int identity, hipStream_t s);
void launch_identity(double* X, int m, int ld, hipStream_t s);
void launch_scatter(double* X, const long long* index, const double* value, long long count, hipStream_t s);
void launch_residual(const DeviceLP& d, const double* X, double* R, hipStream_t s);
void launch_gemm_polish(PolishGemm gemm, const double* X, const double* R, double* C, int m, int ld, const int* row_list, int n_rows, hipStream_t s);
void launch_residual_dense(const DeviceLP& d, PolishGemm gemm, double* Bd, const double* T, double* S, const int* row_list, int n_rows, hipStream_t s);
void launch_copy_rows(const double* src, double* dst, int m, int ld, const int* row_list, int n_rows, hipStream_t s);
void launch_alpha_reduce(const DeviceLP& d, int n_slices, hipStream_t s);
void configure_btran_lds();
void launch_eta_update(const DeviceLP& d, double tol_dual, hipStream_t s);
void launch_eta_consolidate(const DeviceLP& d, hipStream_t s);
void launch_mark_all_touched(const DeviceLP& d, hipStream_t s);
void launch_scaled_basis(const DeviceLP& d, double* T, double scale, hipStream_t s);
void launch_row_scan(const DeviceLP& d, int r, double tol, hipStream_t s);
void launch_ftran_vec(const DeviceLP& d, const int* rows, const double* vals, int nnz, double* out, hipStream_t s);
void launch_btran_vec(const DeviceLP& d, const int* rows, const double* vals, int nnz, double* out, hipStream_t s);
void launch_relative_cost(const DeviceLP& d, double* out, hipStream_t s);

// network_carry.hip
void launch_net_row(const DeviceLP& d, const NetTree& t, int r, double* out, hipStream_t s);

}  // namespace relp
