// Host driver of the device-resident simplex (see solver.hpp).  Replaces, for this path:
//   two_phase/mod.rs:25-109        solve_relaxation (both the generic and the FullInitialBasis route)
//   phase_one.rs:123-278           phase-one loop + zero-level pivots
//   phase_two.rs:22-59             phase-two loop
//   kind/artificial/partially.rs   virtual artificial columns (index space: artificials first)
#include "dual_inherit.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "solver.hpp"

#include <thread>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>

namespace relp {

namespace {
double now_seconds() {
    using clock = std::chrono::steady_clock;
    return std::chrono::duration<double>(clock::now().time_since_epoch()).count();
}
void check_sparse(int nnz, const int* rows, const double* values, int m) {
    if (nnz < 0 || nnz > m) throw std::invalid_argument("nnz out of range");
    if (nnz > 0 && (!rows || !values)) throw std::invalid_argument("null sparse vector");
    for (int e = 0; e < nnz; ++e)
        if (rows[e] < 0 || rows[e] >= m) throw std::invalid_argument("index out of range");
}
template <class T>
void upload_vec(T* dst, const std::vector<T>& src, hipStream_t s) {
    if (!src.empty()) RELP_HIP(hipMemcpyAsync(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, s));
}
// The dense block as the column-per-lane pricing reads it (price_dense_lane_kernel): tile (group of 16 columns, 64 rows) is
// sizeof(T) pieces of 64 lanes x 16 bytes -- one piece of 16 bytes, four of 4 floats, eight of 2 doubles; lane 16 * (row % 64 / 16) +
// column % 16 of piece (row % 16) / (entries per piece) holds the entry.  Zero where a column has no entry.
template <class T>
std::vector<T> pack_dense_lanes(const DeviceMatrix& a, int first_column, int n_dense, int groups, int dense_ld) {
    constexpr int per_piece = 16 / (int)sizeof(T), pieces = (int)sizeof(T);
    const int tiles_per_group = dense_ld / 64;
    std::vector<T> packed((size_t)groups * 16 * dense_ld, T(0));
    for (int jd = 0; jd < n_dense; ++jd)
        for (int e = a.col_start[first_column + jd]; e < a.col_start[first_column + jd + 1]; ++e) {
            const int row = a.row_index[e], within = row % 64, t = within % 16;
            packed[((((size_t)(jd / 16) * tiles_per_group + row / 64) * pieces + t / per_piece) * 64 + 16 * (within / 16) + jd % 16) * per_piece + t % per_piece] = (T)a.value[e];
        }
    return packed;
}
}  // namespace

Solver::Solver(const relp_options& options) : opt_(options) {
    int count = 0;
    hipError_t err = hipGetDeviceCount(&count);
    if (err != hipSuccess || count <= 0)
        throw DeviceError("no HIP device available (relp_amd has no CPU fallback)");
    if (opt_.device < 0 || opt_.device >= count) throw DeviceError("device ordinal out of range");
    RELP_HIP(hipSetDevice(opt_.device));
    RELP_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    RELP_HIP(hipEventCreate(&ev_a_));
    RELP_HIP(hipEventCreate(&ev_b_));
}

Solver::~Solver() {
    (void)hipSetDevice(opt_.device);
    certify_scratch_.release();
    free_device();
    destroy_graphs();
    if (ev_a_) (void)hipEventDestroy(ev_a_);
    if (ev_b_) (void)hipEventDestroy(ev_b_);
    if (ev_parent_) (void)hipEventDestroy(ev_parent_);
    if (ev_snapshot_) (void)hipEventDestroy(ev_snapshot_);
    if (ev_refactored_) (void)hipEventDestroy(ev_refactored_);
    if (refactor_stream_) (void)hipStreamDestroy(refactor_stream_);
    if (d_basis_snapshot_) (void)hipFree(d_basis_snapshot_);
    if (d_probe_) (void)hipFree(d_probe_);
    if (d_flipped_snapshot_) (void)hipFree(d_flipped_snapshot_);
    if (stream_) (void)hipStreamDestroy(stream_);
}

void Solver::free_device() {
    device_memory_.free_all();
    pinned_memory_.free_all();
    h_ctl_ = h_ctl_out_ = nullptr;
    h_flip_totals_ = nullptr;
    h_rb_basis_ = h_rb_flipped_ = h_rb_pos_ = nullptr;
    h_rb_xb_ = h_rb_ub_ = nullptr;
    d_ = DeviceLP{};
    net_ = NetTree{};
    dual_ = DualBuffers{};
    dual_ready_ = false;
    dual_bounded_ = false;
    dual_long_active_ = false;
    dual_flips_ = dual_long_skipped_ = 0;
    dual_cutoff_active_ = dual_cutoff_stopped_ = dual_bound_proved_ = false;
    dual_start_ = "none";
    d_inherit_map_ = nullptr;
    dual_inherit_complemented_ = dual_inherit_moved_ = 0;
}

void Solver::reset_stats() { stats_ = relp_stats{}; }

void Solver::load(StandardForm&& form) {
    RELP_HIP(hipSetDevice(opt_.device));
    loaded_ = false;  // a failed upload must not leave a handle that looks loaded (its device pointers are gone)
    phase_ = 0;
    free_device();
    destroy_graphs();
    form_ = std::move(form);
    certify_scratch_.digit_hints[0] = certify_scratch_.digit_hints[1] = 0;  // (a new LP: nothing is known about its certificate)
    certify_scratch_.statics.reset();
    exact_witnesses.reset();
    path_ = KernelPath{};  // (a refused load leaves no plan behind)
    try {
        upload();
    } catch (...) {
        free_device();
        throw;
    }
    loaded_ = true;
}

// Materialise [artificials | provider columns] once (CSC + CSR) and upload.  The artificial columns are the virtual
// identity columns of `Partially::original_column` (kind/artificial/partially.rs:52-60); the slack columns are the
// virtual columns of `MatrixData::column` (matrix_data.rs:308-327): 12 bytes each, so materialising them costs nothing
// and makes the pricing pass one uniform CSC sweep.  Every choice between kernels is made by plan_kernel_path
// (kernel_path.hpp) before anything is allocated; the functions below read `path_` and decide nothing.
void Solver::upload() {
    const MatrixData& md = form_.data;
    const bool timing = diagnostic("RELP_TIME_UPLOAD");  // diagnostic: where the one-off load time goes
    double t_last = now_seconds();
    auto tick = [&](const char* what) {
        if (!timing) return;
        const double t = now_seconds();
        fprintf(stderr, "[upload] %-28s %.3f s\n", what, t - t_last);
        t_last = t;
    };
    cols_ = device_columns(md, implicit_bounds_apply(opt_, md));
    host_ = DeviceMatrix(cols_, md);
    tick("columns -> CSC");
    path_ = plan_kernel_path(opt_, md, cols_, host_, &form_.column_names);
    tick("kernel path");
    const int m = path_.m, n = path_.n, n_art = path_.n_art;
    d_.m = d_.ld = m, d_.n = n, d_.n_art = d_.dense_first = n_art;  // the decisions the kernels read
    d_.n_dense = path_.n_dense, d_.dense_ld = path_.dense_ld, d_.dense_full = path_.dense_full, d_.dense_csc_start = path_.dense_csc_start;
    d_.dense_lane = path_.dense_lane, d_.ell_w = path_.ell_w, d_.eta_cap = path_.eta_cap, d_.track_touched = path_.track_touched;
    d_.price_unit_pairs = path_.price_unit_pairs, d_.rho_words = path_.rho_words;
    upload_matrix();
    tick("CSC, CSR, costs, rhs");
    upload_pricing_copy();
    tick("pricing copy");
    upload_dense_block();
    tick("dense block");
    allocate_pivot_state();
    configure_lds();
    tick("pivot state");

    stats_.price_bytes = (long long)(host_.col_start[n] - host_.col_start[path_.sparse_first]) * 12 + (long long)(n - n_art) * 24 +
                         (long long)path_.n_dense * m * path_.dense_entry_bytes();  // upper bound: every dense column non-basic
    if (path_.generated_columns) stats_.price_bytes = (long long)(n - n_art) * (8 + 1 + 4);  // endpoints, cost byte, pos (+ the weight of the few columns that need it)
    stats_.update_bytes = path_.network ? 0 : (long long)2 * m * m * 8;
    if (path_.network) net_allocate();
    h_basis_.assign(m, -1);
    h_solution_.assign(md.nr_columns(), 0.0);
    if (!(path_.lu_mode || path_.network || opt_.crash)) host_ = DeviceMatrix{};  // (nothing on the host reads it after the upload)
}

// CSC and CSR of the device LP, the costs of both phases and the right-hand side.
void Solver::upload_matrix() {
    const int m = path_.m, n = path_.n, n_art = path_.n_art;
    const std::vector<int>&col_start = host_.col_start, &row_index = host_.row_index;
    const std::vector<double>& value = host_.value;
    const size_t nnz = row_index.size();
    std::vector<int> row_start(m + 1, 0), col_index(nnz);
    std::vector<double> row_value(nnz);
    for (size_t e = 0; e < nnz; ++e) row_start[row_index[e] + 1]++;
    for (int i = 0; i < m; ++i) row_start[i + 1] += row_start[i];
    {
        std::vector<int> fill(row_start.begin(), row_start.end() - 1);
        for (int j = 0; j < n; ++j)
            for (int e = col_start[j]; e < col_start[j + 1]; ++e) {
                int dst = fill[row_index[e]]++;
                col_index[dst] = j;
                row_value[dst] = value[e];
            }
    }
    std::vector<double> cost1(n, 0.0);
    for (int k = 0; k < n_art; ++k) cost1[k] = 1.0;  // artificial::Cost::One (kind/artificial/partially.rs:42-50)
    d_.col_start = device_alloc<int>(n + 1);
    d_.row_index = device_alloc<int>(nnz);
    d_.value = device_alloc<double>(nnz);
    d_.row_start = device_alloc<int>(m + 1);
    d_.col_index = device_alloc<int>(nnz);
    d_.row_value = device_alloc<double>(nnz);
    d_.cost = device_alloc<double>(n);
    d_.cost1 = device_alloc<double>(n);
    d_.cost2 = device_alloc<double>(n);
    d_.rhs = device_alloc<double>(m);
    d_.rhs0 = device_alloc<double>(m);
    upload_vec(d_.col_start, col_start, stream_);
    upload_vec(d_.row_index, row_index, stream_);
    upload_vec(d_.value, value, stream_);
    upload_vec(d_.row_start, row_start, stream_);
    upload_vec(d_.col_index, col_index, stream_);
    upload_vec(d_.row_value, row_value, stream_);
    upload_vec(d_.cost1, cost1, stream_);
    upload_vec(d_.cost2, host_.cost2, stream_);
    upload_vec(d_.rhs, host_.rhs, stream_);
    upload_vec(d_.rhs0, host_.rhs, stream_);
    RELP_HIP(hipStreamSynchronize(stream_));
    if (opt_.crash) {  // the rows by columns too (the crash walks them)
        h_row_start_ = std::move(row_start);
        h_col_index_ = std::move(col_index);
    }
}

// What the pricing pass streams instead of the CSC: the first ell_w entries of every column, padded; generated incidence columns as
// (row | sign) and a cost byte; and, at width 2, the per-row records or tables of -pi, rho_p and w.
void Solver::upload_pricing_copy() {
    const int m = path_.m, n = path_.n, width = path_.ell_w;
    const std::vector<int>&col_start = host_.col_start, &row_index = host_.row_index;
    const std::vector<double>& value = host_.value;
    std::vector<int> er((size_t)n * width, 0);
    std::vector<double> ev((size_t)n * width, 0.0);
    for (int j = 0; j < n; ++j)
        for (int e = col_start[j], k = 0; e < col_start[j + 1] && k < width; ++e, ++k) {
            er[(size_t)j * width + k] = row_index[e];
            ev[(size_t)j * width + k] = value[e];
        }
    if (path_.generated_columns) {
        for (int j = 0; j < n; ++j)
            for (int k = 0; k < width; ++k) {
                const int len = col_start[j + 1] - col_start[j];
                er[(size_t)j * width + k] = k < len ? (int)((unsigned)row_index[col_start[j] + k] | (value[col_start[j] + k] < 0.0 ? 0x80000000u : 0u))
                                                    : 0x7fffffff;
            }
        std::vector<signed char> c8(n);
        for (int j = 0; j < n; ++j) c8[j] = (signed char)host_.cost2[j];
        d_.cost8 = device_alloc<signed char>(n);
        d_.cost8_2 = device_alloc<signed char>(n);
        upload_vec(d_.cost8_2, c8, stream_);
    } else {
        d_.ell_vals = device_alloc<double>(ev.size());
        upload_vec(d_.ell_vals, ev, stream_);
    }
    d_.ell_rows = device_alloc<int>(er.size());
    upload_vec(d_.ell_rows, er, stream_);
    if (width == 2 && !path_.generated_columns) {  // columns with values: the packed records of price_kernel<.., 2>
        d_.prw = device_alloc<double>((size_t)4 * m);
        RELP_HIP(hipMemsetAsync(d_.prw, 0, (size_t)4 * m * sizeof(double), stream_));
    } else if (path_.rho_words) {  // generated columns: -pi from its own vector, rho_p's non-zero rows as bits ...
        d_.rho_bits = device_alloc<unsigned>((size_t)2 * path_.rho_words);
        RELP_HIP(hipMemsetAsync(d_.rho_bits, 0, (size_t)2 * path_.rho_words * sizeof(unsigned), stream_));
    } else if (path_.generated_columns) {  // ... (bytes beyond LDS)
        d_.rho_nz = device_alloc<unsigned char>(m);
        RELP_HIP(hipMemsetAsync(d_.rho_nz, 0, m, stream_));
    }
    RELP_HIP(hipStreamSynchronize(stream_));
}

// The dense block in the form the plan chose (DenseStorage).
void Solver::upload_dense_block() {
    const int n_art = path_.n_art, n_dense = path_.n_dense;
    const std::vector<int>&col_start = host_.col_start, &row_index = host_.row_index;
    const std::vector<double>& value = host_.value;
    const auto put = [&](auto*& dst, const auto& block) {  // (synchronised: `block` is a temporary of the caller)
        dst = device_alloc<typename std::decay_t<decltype(block)>::value_type>(block.size());
        upload_vec(dst, block, stream_);
        RELP_HIP(hipStreamSynchronize(stream_));
    };
    std::vector<double> dense;  // plain column-major
    if (path_.dense_storage == DenseStorage::F32_ROWS || path_.dense_storage == DenseStorage::F64_ROWS) {
        dense.assign((size_t)n_dense * d_.dense_ld, 0.0);
        for (int jd = 0; jd < n_dense; ++jd)
            for (int e = col_start[n_art + jd]; e < col_start[n_art + jd + 1]; ++e) dense[(size_t)jd * d_.dense_ld + row_index[e]] = value[e];
    }
    switch (path_.dense_storage) {
    case DenseStorage::NONE: return;
    case DenseStorage::I8_LANE: put(d_.dense_val8, pack_dense_lanes<signed char>(host_, n_art, n_dense, path_.dense_blocks, d_.dense_ld)); break;
    case DenseStorage::F32_LANE: put(d_.dense_val32, pack_dense_lanes<float>(host_, n_art, n_dense, path_.dense_blocks, d_.dense_ld)); break;
    case DenseStorage::F64_LANE: put(d_.dense_val, pack_dense_lanes<double>(host_, n_art, n_dense, path_.dense_blocks, d_.dense_ld)); break;
    case DenseStorage::I8_PERMUTED: {
        std::vector<signed char> bytes((size_t)n_dense * d_.dense_ld, 0);
        for (int jd = 0; jd < n_dense; ++jd)
            for (int e = col_start[n_art + jd]; e < col_start[n_art + jd + 1]; ++e) {
                const int row = row_index[e], chunk = row / 1024, within = row % 1024;
                const int pair = within / 128, lane = (within % 128) / 2, t = 2 * pair + (within & 1);  // see price_dense_kernel
                bytes[(size_t)jd * d_.dense_ld + (size_t)chunk * 1024 + lane * 16 + t] = (signed char)value[e];
            }
        put(d_.dense_val8, bytes);
        break;
    }
    case DenseStorage::F32_ROWS: put(d_.dense_val32, std::vector<float>(dense.begin(), dense.end())); break;
    case DenseStorage::F64_ROWS: put(d_.dense_val, dense); break;
    }
    if (!path_.dense_lane) configure_dense_lds();  // (one wave per column: the vectors are in LDS)
}

// Everything a pivot reads and writes: the vectors, the inverse, the candidate slots of the pricing passes, the buffers of the
// pivot form the plan chose, the bounds of an LP with implicit bounds, and the control block.
void Solver::allocate_pivot_state() {
    const int m = path_.m, n = path_.n, vector_len = path_.vector_len, slots = path_.slots();
    d_.xB = device_alloc<double>(m);
    d_.minus_pi = device_alloc<double>(vector_len);
    RELP_HIP(hipMemsetAsync(d_.minus_pi, 0, (size_t)vector_len * sizeof(double), stream_));
    d_.basis = device_alloc<int>(m);
    d_.pos = device_alloc<int>(n);
    d_.gamma = device_alloc<double>(n);
    RELP_HIP(hipMemsetAsync(d_.gamma, 0, n * sizeof(double), stream_));
    d_.cb = device_alloc<double>(m);
    d_.cb_idx = device_alloc<int>(m + 1);
    // The second copy of the inverse and the residual matrix are only needed once a polish finds something to correct
    // (Solver::ensure_polish_buffers): at m = 65 534 each is 34 GB and about a second of hipMalloc, and the max-flow LP of
    // config 5, whose bases are unimodular, never needs them.
    if (!path_.lu_mode && !path_.network) d_.Binv = device_alloc<double>((size_t)m * d_.ld);  // the LU and the forest carries have no m x m array at all
    d_.alpha = device_alloc<double>(m);
    RELP_HIP(hipMemsetAsync(d_.alpha, 0, m * sizeof(double), stream_));
    d_.rho = device_alloc<double>(vector_len);
    RELP_HIP(hipMemsetAsync(d_.rho, 0, (size_t)vector_len * sizeof(double), stream_));
    d_.nz_index = device_alloc<int>(m);
    d_.nz_alpha = device_alloc<double>(m);
    d_.w = device_alloc<double>(vector_len);
    RELP_HIP(hipMemsetAsync(d_.w, 0, (size_t)vector_len * sizeof(double), stream_));
    d_.cand_key = device_alloc<double>(slots);
    d_.cand_j = device_alloc<int>(slots);
    d_.cand_cbar = device_alloc<double>(slots);
    d_.cand_rows = device_alloc<int>((size_t)slots * ELL_W);
    d_.cand_vals = device_alloc<double>((size_t)slots * ELL_W);
    d_.cand_len = device_alloc<int>(slots);
    RELP_HIP(hipMemsetAsync(d_.cand_rows, 0, (size_t)slots * ELL_W * sizeof(int), stream_));  // width-2 pricing writes two of the ELL_W slots
    RELP_HIP(hipMemsetAsync(d_.cand_vals, 0, (size_t)slots * ELL_W * sizeof(double), stream_));
    d_.alpha_part = device_alloc<double>((size_t)std::max(1, path_.ftran_slices) * m);
    d_.alpha_in = device_alloc<double>(m);
    if (path_.slack_in_btran) {
        d_.slack_of_row = device_alloc<int>(m);
        upload_vec(d_.slack_of_row, path_.slack_of_row, stream_);
    }
    d_.touched = device_alloc<int>(m);
    d_.tlist = device_alloc<int>(m);
    RELP_HIP(hipMemsetAsync(d_.touched, 0, m * sizeof(int), stream_));
    if (path_.eta_mode) {  // deferred product form of the inverse (alpha_reduce_kernel, btran_pass_kernel)
        d_.eta_cols = device_alloc<double>((size_t)2 * d_.eta_cap * d_.ld);
        d_.eta_dot_part = device_alloc<double>((size_t)d_.eta_cap * ((m + 63) / 64));
        d_.eta_rows = device_alloc<int>(d_.eta_cap);
        d_.eta_slot = device_alloc<int>(m);
        d_.eta_gather = device_alloc<double>((size_t)d_.eta_cap * m);
        RELP_HIP(hipMemsetAsync(d_.eta_slot, 0xff, m * sizeof(int), stream_));
        configure_btran_lds();
    }
    if (path_.bounded) {
        const std::vector<double> ub = implicit_upper_bounds(form_.data, cols_);
        zero_width_.assign(n, 0);
        for (int j = 0; j < n; ++j) zero_width_[j] = ub[j] == 0.0 ? 1 : 0;
        d_.ub = device_alloc<double>(n);
        d_.xub = device_alloc<double>(m);
        d_.flipped = device_alloc<int>(n);
        upload_vec(d_.ub, ub, stream_);
        RELP_HIP(hipStreamSynchronize(stream_));  // (`ub` is read until the copy has been made)
    }
    if (path_.multi_workgroup_ratio) {  // m > 8192
        d_.k2_partd = device_alloc<double>((size_t)8 * ((m + 1023) / 1024));
        d_.k2_parti = device_alloc<int>((size_t)4 * ((m + 1023) / 1024));
    }
    if (path_.fused) {  // x_B, the basis and the control block twice (pivot_fused_kernel)
        for (int k = 0; k < 2; ++k) {
            d_.state[k].ctl = device_alloc<Ctl>(1);
            d_.state[k].xB = device_alloc<double>(m);
            d_.state[k].basis = device_alloc<int>(m);
        }
        ensure_polish_buffers();  // the second buffer of the out-of-place update
    }
    d_.scratch = device_alloc<double>((size_t)std::max(m, n) * 3 + 16);  // fine-grained ops carve m ints + 2 m doubles out of it
    d_.ctl = device_alloc<Ctl>(1);
    // what the host and the device hand each other around the kernels lives in pinned host memory (no device bytes)
    h_ctl_ = pinned_memory_.alloc<Ctl>(1);
    h_ctl_out_ = pinned_memory_.alloc<Ctl>(1);
    *h_ctl_ = Ctl{};
    if (path_.fused) d_.ctl_mirror = PinnedAllocations::device_pointer(h_ctl_);  // (before any graph is captured: a graph keeps its kernels' arguments)
    h_rb_basis_ = pinned_memory_.alloc<int>(m);
    h_rb_xb_ = pinned_memory_.alloc<double>(m);
    if (path_.bounded) {
        h_rb_flipped_ = pinned_memory_.alloc<int>(n);
        h_rb_pos_ = pinned_memory_.alloc<int>(n);
        h_rb_ub_ = pinned_memory_.alloc<double>(n);
    }
    d_.dbg = device_alloc<unsigned long long>(64);
    RELP_HIP(hipMemsetAsync(d_.dbg, 0, 64 * sizeof(unsigned long long), stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
}

Ctl Solver::read_ctl() {
    // Every batch of launches ends in a read of the control block (never inside a stream capture): the place where a
    // rejected launch -- a grid or an LDS request the device refuses -- surfaces instead of leaving stale device state behind.
    // The copy lands in the handle's pinned mirror: a copy into pageable memory is staged through a copy kernel of the runtime.
    RELP_HIP(hipGetLastError());
    RELP_HIP(hipMemcpyAsync(h_ctl_, d_.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
    Ctl c = *h_ctl_;
    if (c.status == ST_REFACTOR_FAILED) {
        // the refactorisation kernels gave up (a capacity, a row too long for the eliminating wave): nothing has pivoted since, the
        // basis on the device is the one they were given -- factorise it on the host (which also grows what was too small)
        ++device_refactor_failures_;
        if (opt_.verbose > 0) {
            int info[LUF_INFO_WORDS];
            RELP_HIP(hipMemcpy(info, lu().device_info(), sizeof(info), hipMemcpyDeviceToHost));
            fprintf(stderr, "[lu] the device refactorisation gave up with status %d (m %d): host fallback\n", info[LUF_STATUS], d_.m);
        }
        c.status = ST_REFACTOR;
        write_ctl(c);
        refactor_lu_host(true);
        refactors_--;  // (counted once, by the attempt on the device)
        RELP_HIP(hipMemcpyAsync(h_ctl_, d_.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, stream_));
        RELP_HIP(hipStreamSynchronize(stream_));
        c = *h_ctl_;
    }
    return c;
}
// The end of a batch of pivots (Solver::iterate).  Fused path: commit_kernel, the last kernel of every batch, has stored the
// committed block into the mirror as well (DeviceLP::ctl_mirror), so nothing is enqueued -- the host waits for the stream and reads.
// The mirror is never read while a kernel may still be running.
Ctl Solver::read_ctl_after_batch() {
    if (!d_.ctl_mirror) return read_ctl();
    RELP_HIP(hipGetLastError());
    RELP_HIP(hipStreamSynchronize(stream_));
    return *h_ctl_;
}
void Solver::write_ctl(const Ctl& c) {
    *h_ctl_out_ = c;  // (the wait below: the pinned block is free again when this returns)
    RELP_HIP(hipMemcpyAsync(d_.ctl, h_ctl_out_, sizeof(Ctl), hipMemcpyHostToDevice, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
}

// `Tableau::<_, Partially<_>>::new` + `Carry::create_for_partially_artificial` (partially.rs:125-205, carry/mod.rs:397-442):
// B = I, basis = artificial k on its row / free slack pivot on the others, b = rhs.
void Solver::begin_phase_one() {
    if (!loaded_) throw std::runtime_error("no LP loaded");
    RELP_HIP(hipSetDevice(opt_.device));
    dual_ready_ = false;
    const int m = d_.m, n = d_.n, n_art = d_.n_art;
    const std::vector<int>& basis = cols_.basis0;
    std::vector<int> pos = cols_.pos0();
    if (path_.bounded)  // a variable whose two bounds coincide can never move: it is not priced (pos -3; see DeviceLP::pos)
        for (int j = n_art; j < n; ++j)
            if (zero_width_[j] && pos[j] < 0) pos[j] = -3;
    upload_vec(d_.basis, basis, stream_);
    upload_vec(d_.pos, pos, stream_);
    RELP_HIP(hipMemcpyAsync(d_.rhs, d_.rhs0, m * sizeof(double), hipMemcpyDeviceToDevice, stream_));
    if (path_.bounded) {  // nothing is complemented; the initial basic variables (artificials, <= slacks) have no upper bound
        std::vector<double> xub(m, std::numeric_limits<double>::infinity());
        upload_vec(d_.xub, xub, stream_);
        RELP_HIP(hipMemsetAsync(d_.flipped, 0, n * sizeof(int), stream_));
        RELP_HIP(hipStreamSynchronize(stream_));
    }
    RELP_HIP(hipMemcpyAsync(d_.xB, d_.rhs, m * sizeof(double), hipMemcpyDeviceToDevice, stream_));
    if (path_.lu_mode) lu_identity();
    else if (path_.network) {
        net_upload(net_build(basis, std::vector<int>()));  // every row its own root (unit columns)
        if (net_.stats) RELP_HIP(hipMemsetAsync(net_.stats, 0, NS_WORDS * sizeof(unsigned long long), stream_));
    }
    else launch_identity(d_.Binv, m, d_.ld, stream_);
    RELP_HIP(hipMemsetAsync(d_.touched, 0, m * sizeof(int), stream_));  // every column is a unit vector
    binv_identity_ = true;
    refactors_ = 0;
    device_refactor_failures_ = 0;
    refactor_seconds_ = 0.0;
    Ctl c{};
    c.forced_q = c.forced_p = -1;
    c.last_selected = -1;
    c.scan_column = std::numeric_limits<int>::max();
    write_ctl(c);
    pivots_[0] = pivots_[1] = 0;
    polishes_ = 0;
    max_residual_ = 0.0;
    since_polish_ = 0;
    polish_scale_ = 1;
    redundant_rows_.clear();
    gamma_ready_ = false;
    if (opt_.crash && n_art > 0) crash_basis();
    set_phase(n_art > 0 ? 1 : 2);
}


// Triangular crash basis (relp_options.crash; an EXTENSION: the reference starts every row without a slack pivot on an
// artificial, partially.rs:125-205, and on the max-flow LP of examples/max_flow.rs pivots all V - 2 of them out one
// degenerate pivot at a time).  Columns that have exactly ONE entry in the rows still covered by an artificial are assigned to
// that row, breadth first -- on an incidence matrix that is a spanning forest grown from s and t.  The basis is triangular
// by construction, so its inverse comes from sparse back-substitution on the host (no factorisation) and is scattered into
// the identity that `begin_phase_one` has just written; x_B, the touched-column list and the steepest-edge weights
// gamma_j = 1 + |B^-1 a_j|^2 (pivot_rule.rs:202-219) are computed from the same sparse columns.  The crash is only kept when
// it is primal feasible; phase one then starts from it (with zero artificials left it ends without a pivot).
bool Solver::crash_basis() {
    if (path_.lu_mode || path_.eta_mode || d_.n_dense > 0 || host_.col_start.empty() || h_row_start_.empty()) return false;
    const int m = d_.m, n = d_.n, n_art = d_.n_art;
    const bool timing = diagnostic("RELP_TIME_SOLVE");
    double t_last = now_seconds();
    auto tick = [&](const char* what) {
        if (!timing) return;
        const double t = now_seconds();
        fprintf(stderr, "[crash] %-28s %.3f ms\n", what, (t - t_last) * 1e3);
        t_last = t;
    };
    std::vector<int> basis(m);
    RELP_HIP(hipMemcpyAsync(basis.data(), d_.basis, m * sizeof(int), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
    const std::vector<int>& cs = host_.col_start;
    const std::vector<int>& ri = host_.row_index;
    const std::vector<double>& va = host_.value;
    std::vector<char> uncovered(m, 0);
    for (int i = 0; i < m; ++i) uncovered[i] = basis[i] < n_art ? 1 : 0;
    // rows -> columns: the CSR of the device LP kept by upload() (artificial columns included: skipped below)
    const std::vector<int>& row_start = h_row_start_;
    const std::vector<int>& row_cols = h_col_index_;
    std::vector<int> count(n, 0);
    for (int j = n_art; j < n; ++j)
        for (int e = cs[j]; e < cs[j + 1]; ++e) count[j] += uncovered[ri[e]];
    std::vector<int> queue;
    queue.reserve(n - n_art);
    std::vector<char> is_basic(n, 0);
    for (int i = 0; i < m; ++i) is_basic[basis[i]] = 1;
    for (int j = n_art; j < n; ++j)
        if (count[j] == 1 && !is_basic[j] && !(path_.bounded && zero_width_[j])) queue.push_back(j);
    std::vector<int> order_of_row(m, -1), crash_rows;  // order in which the rows were covered
    std::vector<double> diagonal(m, 1.0);
    for (size_t head = 0; head < queue.size(); ++head) {
        const int j = queue[head];
        if (count[j] != 1 || is_basic[j]) continue;
        int r = -1;
        double pivot = 0.0, largest = 0.0;
        for (int e = cs[j]; e < cs[j + 1]; ++e) {
            largest = std::max(largest, std::fabs(va[e]));
            if (uncovered[ri[e]]) { r = ri[e]; pivot = va[e]; }
        }
        if (r < 0 || std::fabs(pivot) < 0.1 * largest) continue;  // (a small diagonal would make the triangular basis ill conditioned)
        is_basic[basis[r]] = 0;
        basis[r] = j;
        is_basic[j] = 1;
        uncovered[r] = 0;
        order_of_row[r] = (int)crash_rows.size();
        crash_rows.push_back(r);
        diagonal[r] = pivot;
        for (int e = row_start[r]; e < row_start[r + 1]; ++e) {
            const int j2 = row_cols[e];
            if (j2 < n_art) continue;
            if (--count[j2] == 1 && !is_basic[j2] && !(path_.bounded && zero_width_[j2])) queue.push_back(j2);
        }
    }
    const int covered = (int)crash_rows.size();
    tick("rows by columns, BFS");
    if (covered == 0) return false;
    if (path_.network) {  // the forest carry takes the crash columns as they are: no inverse on the host
        if (!net_crash(basis)) return false;
        crash_rows_covered_ = covered;
        tick("forest, x_B, weights");
        return true;
    }
    // Inverse by back-substitution: B (rows x positions, position of a crash column = its row) is upper triangular in the
    // order [rows that kept a unit column | crash rows in covering order].  Column r of B^-1 (r a crash row) solves B v = e_r.
    const size_t entry_cap = (size_t)64 * m + (1u << 22);
    std::vector<size_t> inv_start(covered + 1, 0);
    std::vector<int> inv_pos;
    std::vector<double> inv_val;
    std::vector<double> work(m, 0.0);
    std::vector<char> in_heap(m, 0);
    std::vector<std::pair<int, int>> heap;  // (covering order, row): max-heap
    for (int k = 0; k < covered; ++k) {
        const int r = crash_rows[k];
        work[r] = 1.0;
        heap.clear();
        heap.push_back({k, r});
        in_heap[r] = 1;
        while (!heap.empty()) {
            std::pop_heap(heap.begin(), heap.end());
            const int row = heap.back().second;
            heap.pop_back();
            in_heap[row] = 0;
            const double residual = work[row];
            work[row] = 0.0;
            if (residual == 0.0) continue;
            const double v = residual / diagonal[row];
            inv_pos.push_back(row);
            inv_val.push_back(v);
            if (order_of_row[row] < 0) continue;  // a unit column: nothing to propagate
            const int j = basis[row];
            for (int e = cs[j]; e < cs[j + 1]; ++e) {
                const int r2 = ri[e];
                if (r2 == row) continue;
                work[r2] -= va[e] * v;
                if (!in_heap[r2]) {
                    in_heap[r2] = 1;
                    heap.push_back({order_of_row[r2], r2});
                    std::push_heap(heap.begin(), heap.end());
                }
            }
        }
        inv_start[k + 1] = inv_pos.size();
        if (inv_pos.size() > entry_cap) return false;  // not a sparse inverse: leave the start to phase one
    }
    tick("sparse inverse");
    // x_B = B^-1 b, must be a basic feasible solution of the phase-one problem
    std::vector<double> xb(m, 0.0);
    for (int i = 0; i < m; ++i)
        if (order_of_row[i] < 0) xb[i] = host_.rhs[i];
    for (int k = 0; k < covered; ++k) {
        const double b = host_.rhs[crash_rows[k]];
        if (b == 0.0) continue;
        for (size_t e = inv_start[k]; e < inv_start[k + 1]; ++e) xb[inv_pos[e]] += inv_val[e] * b;
    }
    std::vector<double> ub;
    if (path_.bounded) {
        ub.resize(n);
        RELP_HIP(hipMemcpyAsync(ub.data(), d_.ub, n * sizeof(double), hipMemcpyDeviceToHost, stream_));
        RELP_HIP(hipStreamSynchronize(stream_));
    }
    double scale = 1.0;
    for (int i = 0; i < m; ++i) scale = std::max(scale, std::fabs(host_.rhs[i]));
    for (int i = 0; i < m; ++i) {
        if (xb[i] < -1e-9 * scale) return false;
        if (path_.bounded && xb[i] > ub[basis[i]] + 1e-9 * scale) return false;
        if (xb[i] < 0.0) xb[i] = 0.0;
    }
    // steepest-edge weights of the non-basic columns from the sparse inverse columns
    std::vector<double> gamma(n, 1.0);
    if (opt_.pivot_rule == RELP_PIVOT_STEEPEST_EDGE) {
        // (independent columns: host threads, each with its own accumulator -- 41 ms on one core for the 1 M arcs of config 5)
        const int n_threads = (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
        auto range = [&](int first, int last) {
            std::vector<int> touched_list, mark(m, -1);
            std::vector<double> acc(m, 0.0);
            auto add = [&](int p, double v, int j) {
                if (mark[p] != j) {
                    mark[p] = j;
                    acc[p] = 0.0;
                    touched_list.push_back(p);
                }
                acc[p] += v;
            };
            for (int j = first; j < last; ++j) {
                if (is_basic[j]) continue;
                touched_list.clear();
                for (int e = cs[j]; e < cs[j + 1]; ++e) {
                    const int r = ri[e], k = order_of_row[r];
                    if (k < 0) add(r, va[e], j);
                    else
                        for (size_t t = inv_start[k]; t < inv_start[k + 1]; ++t) add(inv_pos[t], va[e] * inv_val[t], j);
                }
                double sum = 1.0;
                for (int p : touched_list) sum += acc[p] * acc[p];
                gamma[j] = sum;
            }
        };
        const int columns = n - n_art;
        if (n_threads <= 1 || columns < 65536) {
            range(n_art, n);
        } else {
            std::vector<std::thread> pool;
            const int chunk = (columns + n_threads - 1) / n_threads;
            for (int t = 0; t < n_threads; ++t) {
                const int first = n_art + t * chunk, last = std::min(n, first + chunk);
                if (first < last) pool.emplace_back(range, first, last);
            }
            for (auto& th : pool) th.join();
        }
        std::fill(work.begin(), work.end(), 0.0);
    }
    tick("x_B, weights");
    // ---- device state -------------------------------------------------------------------------------------------
    std::vector<long long> scatter_index(inv_pos.size());
    for (int k = 0; k < covered; ++k)
        for (size_t e = inv_start[k]; e < inv_start[k + 1]; ++e) scatter_index[e] = (long long)crash_rows[k] * d_.ld + inv_pos[e];
    long long* d_index = nullptr;
    double* d_value = nullptr;
    RELP_HIP(hipMalloc(reinterpret_cast<void**>(&d_index), scatter_index.size() * sizeof(long long)));
    RELP_HIP(hipMalloc(reinterpret_cast<void**>(&d_value), inv_val.size() * sizeof(double)));
    RELP_HIP(hipMemcpyAsync(d_index, scatter_index.data(), scatter_index.size() * sizeof(long long), hipMemcpyHostToDevice, stream_));
    RELP_HIP(hipMemcpyAsync(d_value, inv_val.data(), inv_val.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
    launch_scatter(d_.Binv, d_index, d_value, (long long)inv_val.size(), stream_);
    std::vector<int> pos(n, -1), touched(m, 0);
    if (path_.bounded)
        for (int j = n_art; j < n; ++j)
            if (zero_width_[j]) pos[j] = -3;
    for (int i = 0; i < m; ++i) pos[basis[i]] = i;
    for (int r : crash_rows) touched[r] = 1;
    upload_vec(d_.basis, basis, stream_);
    upload_vec(d_.pos, pos, stream_);
    upload_vec(d_.xB, xb, stream_);
    upload_vec(d_.gamma, gamma, stream_);
    upload_vec(d_.touched, touched, stream_);
    upload_vec(d_.tlist, crash_rows, stream_);
    if (path_.bounded) {
        std::vector<double> xub(m);
        for (int i = 0; i < m; ++i) xub[i] = ub[basis[i]];
        upload_vec(d_.xub, xub, stream_);
    }
    Ctl c = read_ctl();  // (also waits for the uploads)
    c.touched_count = covered;
    write_ctl(c);
    (void)hipFree(d_index);
    (void)hipFree(d_value);
    binv_identity_ = false;
    gamma_ready_ = opt_.pivot_rule == RELP_PIVOT_STEEPEST_EDGE;
    crash_rows_covered_ = covered;
    tick("uploads");
    return true;
}

// `Tableau::from_artificial` (non_artificial.rs:99-120): same basis, provider costs; -pi, -obj and the weights are
// recomputed from the resident inverse (carry/mod.rs:499-525; pivot_rule.rs:202-219).
void Solver::begin_phase_two() {
    // (set_phase reads the basis, its positions and the inverse: before begin_phase_one or set_basis has written them the kernels would
    //  index with whatever the arrays hold.  An LP without artificials starts phase two in begin_phase_one)
    if (phase_ == 0) throw std::runtime_error("begin_phase_two: no basis yet (begin_phase_one or set_basis comes first)");
    set_phase(2);
}

void Solver::set_phase(int phase) {
    const int phase_before = phase_;
    phase_ = phase;
    last_pivot_dual_ = false;
    RELP_HIP(hipMemcpyAsync(d_.cost, phase == 1 ? d_.cost1 : d_.cost2, d_.n * sizeof(double), hipMemcpyDeviceToDevice, stream_));
    if (d_.cost8) {  // generated columns: the priced columns (never the artificials) cost 0 in phase one
        if (phase == 1) RELP_HIP(hipMemsetAsync(d_.cost8, 0, d_.n, stream_));
        else RELP_HIP(hipMemcpyAsync(d_.cost8, d_.cost8_2, d_.n, hipMemcpyDeviceToDevice, stream_));
    }
    if (path_.lu_mode) launch_lu_pi(d_, lu().device(), stream_);
    else if (path_.network) net_refresh(false, true);
    else launch_pi(d_, stream_);
    // Steepest-edge weights gamma_j = 1 + |B^-1 a_j|^2 do not depend on the costs, and the recurrences that maintain them
    // are exact: what phase one leaves is what `SteepestDescentAlongObjective::new` (pivot_rule.rs:202-219) would recompute
    // for phase two.  Recomputing costs one pass over the inverse per column pair -- fine for Netlib, 1 TB for the 1 M-arc
    // max-flow LP -- so large LPs keep the weights (after flushing the update of the last zero-level pivot).
    const double carry_threshold = opt_.carry_weights_min > 0.0 ? opt_.carry_weights_min : 4e9;  // (test hook)
    // (the LU carry always keeps them: recomputing is one FTRAN per non-basic column)
    const bool carry_weights = phase == 2 && phase_before == 1 && !binv_identity_ &&
                               (path_.lu_mode || (double)(d_.n - d_.n_art) * (double)d_.m > carry_threshold);
    if (opt_.pivot_rule == RELP_PIVOT_STEEPEST_EDGE) {
        if (carry_weights) {
            Ctl pending = read_ctl();
            if (pending.pending) {
                pending.status = ST_RUNNING;
                write_ctl(pending);
                RELP_HIP(hipMemcpyAsync(d_.cost, d_.cost1, d_.n * sizeof(double), hipMemcpyDeviceToDevice, stream_));
                enqueue_price(0);  // applies the pending Goldfarb-Reid update; its candidates are discarded
                RELP_HIP(hipMemcpyAsync(d_.cost, d_.cost2, d_.n * sizeof(double), hipMemcpyDeviceToDevice, stream_));
            }
        } else if (gamma_ready_) {
            gamma_ready_ = false;  // the crash computed them on the host from its sparse inverse
        } else if (path_.lu_mode && !binv_identity_) {
            launch_lu_gamma(d_, lu().device(), stream_);
        } else if (path_.network && !binv_identity_) {
            net_set_gamma();
        } else {
            launch_gamma_init(d_, binv_identity_ ? 1 : 0, stream_);
        }
    }
    Ctl c = read_ctl();
    const double minus_obj = c.minus_obj;
    const int touched_count = c.touched_count;
    const long long bound_flips = c.bound_flips;
    c = Ctl{};
    c.minus_obj = minus_obj;
    c.touched_count = touched_count;
    c.bound_flips = bound_flips;
    c.forced_q = c.forced_p = -1;
    c.last_selected = -1;
    c.scan_column = std::numeric_limits<int>::max();
    write_ctl(c);
}

// One batch of `count` iterations of the loop of phase_one.rs:134-178 / phase_two.rs:36-58.
void Solver::launch_pivots(int count, bool forced) {
    stats_.launches += path_.launches(count, forced, false);
    stats_.price_launches += count;
    if (path_.fused && !forced) {  // two kernels per pivot; x_B, basis and control block alternate between their two copies (kernels.hip, K23)
        launch_begin_batch(d_, count, stream_);
        for (int it = 0; it < count; ++it) {
            enqueue_price_fused(it & 1);
            enqueue_pivot_fused(it & 1);
        }
        launch_commit(d_, count & 1, stream_);
        return;
    }
    launch_budget(d_, count, stream_);
    for (int it = 0; it < count; ++it) {
        enqueue_price(0, it == 0);
        enqueue_ftran_ratio(0);  // (the forest carry: its whole pivot, a linear chain of launches; the LU carry: its single-workgroup kernel)
        if (path_.network || path_.lu_mode) continue;
        enqueue_update();
        if (path_.eta_mode && ((it + 1) % d_.eta_cap == 0 || it + 1 == count)) enqueue_consolidate();
    }
}

// Pricing pass: the dense block (if any) streams through price_dense_kernel, every other column through the CSC kernel.
void Solver::enqueue_price(int skip_weights, bool first_of_batch) {
    // path_.slack_in_btran: the BTRAN pass of the previous pivot has priced the slack columns (weights included); only the first
    // pivot of a batch has no predecessor in the batch, and its pass must not apply the weight update a second time
    if (path_.price_blocks > 0 && (!path_.slack_in_btran || first_of_batch))
        launch_price(d_, path_, path_.price_kernel, opt_.pivot_rule, path_.slack_in_btran ? 1 : skip_weights, opt_.tol_dual, stream_);
    if (path_.dense_blocks > 0) launch_price_dense(d_, path_, skip_weights, opt_.tol_dual, stream_);
}

// Fused mode: the pricing pass before pivot k reads the control block of copy k & 1 (it writes nothing of the twin state).
void Solver::enqueue_price_fused(int parity) {
    DeviceLP d = d_;
    d.ctl = d_.state[parity].ctl;
    launch_price(d, path_, path_.price_kernel_fused, opt_.pivot_rule, 0, opt_.tol_dual, stream_);
}
void Solver::enqueue_pivot_fused(int parity) {
    launch_pivot_fused(d_, path_, opt_.pivot_rule, parity, opt_.tol_pivot, ratio_delta(), phase_ == 2 ? 1 : 0, stream_);
}

// The basis update: rank-one update of the explicit inverse (K3), or -- deferred product form -- the eta bookkeeping plus
// one read-only pass for rho_p, w and -pi.
void Solver::enqueue_update() {
    if (path_.eta_mode) launch_eta_update(d_, opt_.tol_dual, stream_);
    else launch_update(d_, path_, stream_);
}
// Fold the pending etas into the stored inverse (no-op kernels when there are none; runs whatever the status is, so that
// everything outside the pivot loop sees the plain explicit inverse).
void Solver::enqueue_consolidate() {
    if (path_.eta_mode) launch_eta_consolidate(d_, stream_);
}

// Entering column + FTRAN + ratio test (+ updates in mode 0).  Long (dense) columns take the multi-block FTRAN.
void Solver::enqueue_ftran_ratio(int mode) {
    const int skip_art = phase_ == 2 ? 1 : 0;
    const int slots = path_.slots();
    if (path_.network) {
        net_enqueue_pivot(mode);
        return;
    }
    if (path_.lu_mode) {
        launch_lu_pivot(d_, lu().device(), opt_.pivot_rule, slots, opt_.tol_pivot, ratio_delta(), skip_art, mode, path_.refactor_period, stream_);
        return;
    }
    if (path_.ftran_slices > 0) {
        launch_ftran_partial(d_, path_.ftran_slices, slots, opt_.pivot_rule, stream_);
        launch_alpha_reduce(d_, path_.ftran_slices, stream_);
    }
    launch_ftran_ratio(d_, path_, opt_.pivot_rule, opt_.tol_pivot, ratio_delta(), skip_art, mode, path_.ftran_slices > 0 ? 1 : 0, stream_);
}

void Solver::destroy_graphs() {
    for (int k = 0; k < 4; ++k) {
        if (graph_exec_[k]) { (void)hipGraphExecDestroy(graph_exec_[k]); graph_exec_[k] = nullptr; }
        if (graph_[k]) { (void)hipGraphDestroy(graph_[k]); graph_[k] = nullptr; }
        graph_count_[k] = 0;
    }
}

void Solver::build_graph(int count) {
    const int k = graph_index();
    if (graph_exec_[k] && graph_count_[k] == count) return;
    if (graph_exec_[k]) { (void)hipGraphExecDestroy(graph_exec_[k]); graph_exec_[k] = nullptr; }
    if (graph_[k]) { (void)hipGraphDestroy(graph_[k]); graph_[k] = nullptr; }
    long long launches = stats_.launches, price_launches = stats_.price_launches;
    RELP_HIP(hipStreamBeginCapture(stream_, hipStreamCaptureModeRelaxed));
    launch_pivots(count);
    RELP_HIP(hipStreamEndCapture(stream_, &graph_[k]));
    RELP_HIP(hipGraphInstantiate(&graph_exec_[k], graph_[k], nullptr, nullptr, 0));
    stats_.launches = launches;
    stats_.price_launches = price_launches;
    graph_count_[k] = count;
}

// Newton-Schulz polish (see kernels.hip).  Two iterations at most; the residual before the polish is recorded.
void Solver::polish(bool refresh_vectors, bool force) {
    if (path_.lu_mode) {  // the LU carry's refresh is a refactorisation
        refactor_lu(refresh_vectors);
        return;
    }
    if (path_.network) {  // the forest is exact: x_B, -pi and the objective recomputed from it
        if (since_polish_ == 0 && !force && !(opt_.switches & RELP_SW_POLISH_ALWAYS)) return;
        if (refresh_vectors) net_refresh(true, true);
        polish_scale_ = std::min(256, polish_scale_ * 4);
        polishes_++;
        since_polish_ = 0;
        return;
    }
    // nothing has changed since the inverse was last made exact (identity, crash basis, set_basis, the previous polish): at
    // m = 65 534 the residual pass and the two refresh passes are 34 GB each
    if (since_polish_ == 0 && !force && !(opt_.switches & RELP_SW_POLISH_ALWAYS)) return;
    const int m = d_.m;
    polish_rebuilt_ = false;
    dual_weights_current_ = false;  // (the inverse may be rewritten below)
    // dense pipeline: only the columns of the stored inverse that are not unit vectors take part (the corresponding
    // rows of S are zero and those columns of the polished inverse do not change): both GEMMs shrink by m / touched
    const bool by_rows = path_.track_touched && path_.polish_gemm == PolishGemm::MFMA;  // (the plain-FMA kernels compute every row)
    const int* rows = by_rows ? d_.tlist : nullptr;
    int n_rows = m;
    if (by_rows) n_rows = read_ctl().touched_count;
    if (d_.n_dense > 0) ensure_polish_buffers();  // the dense residual is a GEMM into R through Binv2
    for (int it = 0; it < 2; ++it) {
        RELP_HIP(hipMemsetAsync(&d_.ctl->residual, 0, sizeof(double), stream_));
        if (by_rows && d_.R) RELP_HIP(hipMemsetAsync(d_.R, 0, (size_t)m * d_.ld * sizeof(double), stream_));
        if (d_.n_dense > 0) launch_residual_dense(d_, path_.polish_gemm, d_.Binv2, d_.Binv, d_.R, rows, n_rows, stream_);
        else launch_residual(d_, d_.Binv, d_.R, stream_);  // R == nullptr: norm only
        Ctl c = read_ctl();  // max |I - B' T|
        if (d_.R == nullptr && c.residual >= 1e-12 && c.residual < 0.5) {  // something to correct: now S itself is needed
            ensure_polish_buffers();
            if (by_rows) RELP_HIP(hipMemsetAsync(d_.R, 0, (size_t)m * d_.ld * sizeof(double), stream_));
            RELP_HIP(hipMemsetAsync(&d_.ctl->residual, 0, sizeof(double), stream_));
            launch_residual(d_, d_.Binv, d_.R, stream_);
            c = read_ctl();
        }
        if (!(c.residual == c.residual)) throw std::runtime_error("NaN in basis inverse");
        if (it == 0) {
            polish_first_residual_ = c.residual;
            max_residual_ = std::max(max_residual_, c.residual);
            // the drift seen after this many pivots schedules the next polish: far below the working accuracy -> wait
            // twice as long (up to 16 periods), close to it -> back to the configured period
            // (an inverse that is still EXACT, as on totally unimodular bases, has not drifted at all: four times as long, up to 256)
            if (c.residual == 0.0) polish_scale_ = std::min(256, polish_scale_ * 4);
            else if (c.residual < 1e-8) polish_scale_ = std::min(std::max(16, polish_scale_), polish_scale_ * 2);
            else if (c.residual > 1e-6) polish_scale_ = 1;
        }
        if (c.residual < 1e-12) break;  // nothing to correct: skip the second GEMM
        if (c.residual >= 0.5) {  // drifted too far for the quadratic iteration: rebuild from the basis columns
            invert_from_scratch();
            polish_rebuilt_ = true;
            break;
        }
        launch_gemm_polish(path_.polish_gemm, d_.Binv, d_.R, d_.Binv2, m, d_.ld, rows, n_rows, stream_);
        ++polish_gemms_;
        if (by_rows) launch_copy_rows(d_.Binv2, d_.Binv, m, d_.ld, rows, n_rows, stream_);
        else RELP_HIP(hipMemcpyAsync(d_.Binv, d_.Binv2, (size_t)m * d_.ld * sizeof(double), hipMemcpyDeviceToDevice, stream_));
        if (c.residual < 1e-8) break;  // one quadratic step takes it to ~residual^2
    }
    binv_identity_ = false;
    polishes_++;
    since_polish_ = 0;
    if (refresh_vectors) {  // pi_kernel also rewrites minus_obj from the refreshed xB; everything stays on the stream
        launch_xb(d_, stream_);
        launch_pi(d_, stream_);
    }
}

// From-scratch inverse by Newton-Schulz from X0 = B' / (|B|_1 |B|_inf) (converges for every nonsingular B).
// Plays the role of `BasisInverse::invert` (lower_upper/mod.rs:78-92) for `from_basis` / warm starts.
void Solver::ensure_polish_buffers() {
    if (d_.Binv2 == nullptr) d_.Binv2 = device_alloc<double>((size_t)d_.m * d_.ld);
    if (d_.R == nullptr) d_.R = device_alloc<double>((size_t)d_.m * d_.ld);
}

void Solver::invert_from_scratch() {
    if (path_.lu_mode) {
        // (set_basis on a handle that never began phase one: the refactorisation kernels write into arrays that lu_identity sizes by bounds)
        if (path_.device_refactor && !lu().device_prepared()) lu_identity();
        refactor_lu(false);
        return;
    }
    if (path_.network) {  // the forest of the basis on the device, built on the host in O(m)
        net_upload(net_download());
        return;
    }
    const int m = d_.m;
    ensure_polish_buffers();
    std::vector<int> basis(m);
    RELP_HIP(hipMemcpyAsync(basis.data(), d_.basis, m * sizeof(int), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
    const MatrixData& md = form_.data;
    std::vector<double> row_sum(m, 0.0);
    double norm1 = 0.0;
    for (int k = 0; k < m; ++k) {
        double col_sum = 0.0;
        if (basis[k] < d_.n_art) {
            col_sum = 1.0;  // identity column; its row is found below through pos/CSR, the bound is enough here
        } else {
            SparseColumn c = md.column(basis[k] - d_.n_art);
            for (size_t e = 0; e < c.nnz(); ++e) {
                if (c.index[e] >= m) continue;  // the bound-row entry of a bounded column (implicit bounds)
                double v = std::fabs(c.value[e].to_double());
                col_sum += v;
                row_sum[c.index[e]] += v;
            }
        }
        norm1 = std::max(norm1, col_sum);
    }
    double norm_inf = 1.0;
    for (double v : row_sum) norm_inf = std::max(norm_inf, v);
    launch_scaled_basis(d_, d_.Binv, 1.0 / (norm1 * norm_inf), stream_);
    double previous = std::numeric_limits<double>::infinity();
    for (int it = 0; it < 200; ++it) {
        RELP_HIP(hipMemsetAsync(&d_.ctl->residual, 0, sizeof(double), stream_));
        launch_residual(d_, d_.Binv, d_.R, stream_);
        launch_gemm_polish(path_.polish_gemm, d_.Binv, d_.R, d_.Binv2, m, d_.ld, nullptr, m, stream_);
        ++polish_gemms_;
        RELP_HIP(hipMemcpyAsync(d_.Binv, d_.Binv2, (size_t)m * d_.ld * sizeof(double), hipMemcpyDeviceToDevice, stream_));
        Ctl c = read_ctl();
        if (c.residual < 1e-11) break;
        if (it > 60 && c.residual >= previous) break;
        previous = c.residual;
    }
    launch_mark_all_touched(d_, stream_);  // no column of a fresh inverse is known to be a unit vector
    binv_identity_ = false;
}

// `InverseMaintainer::from_basis` (carry/mod.rs:444-478) + `Tableau::new_with_inverse_maintainer`: phase two from a given basis.
void Solver::set_basis(const int* basis_columns) {
    place_basis(basis_columns);
    invert_from_scratch();
    if (path_.lu_mode) launch_lu_xb(d_, lu().device(), stream_);
    else if (path_.network) net_refresh(true, false);
    else launch_xb(d_, stream_);
    reset_basis_counters();
    set_phase(2);
}

// The first part of set_basis: the basis as the device holds it, pos, (implicit bounds: which columns are complemented, the
// right-hand side and the bounds of the basic variables,) and a fresh control block.  The inverse is the caller's to provide.
void Solver::place_basis(const int* basis_columns) {
    if (!loaded_) throw std::runtime_error("no LP loaded");
    RELP_HIP(hipSetDevice(opt_.device));
    dual_ready_ = false;
    const int m = d_.m, n = d_.n;
    std::vector<int> basis(m), pos(n, -1);
    if (!path_.bounded) {
        for (int i = 0; i < m; ++i) {
            int c = basis_columns[i];
            int dev = cols_.to_device(c);
            if (dev < 0 || dev >= n || pos[dev] >= 0) throw std::invalid_argument("bad basis");
            basis[i] = dev;
            pos[dev] = i;
        }
    } else {
        // Implicit bounds: `basis_columns` is a basis of the reference's formulation (one column per row of MatrixData).  A
        // bounded variable whose bound slack is NOT basic sits at its bound: non-basic and complemented on the device; with
        // the slack basic it is basic here exactly when it is basic there (reduce_bounded_basis, dual_inherit.hpp: the relation of
        // begin_dual_bounded_from reads the same reduction).
        const MatrixData& md = form_.data;
        ReducedBasis reduced = reduce_bounded_basis(md, d_.n_art, basis_columns);
        basis = std::move(reduced.basis);
        std::vector<int> flipped = std::move(reduced.flipped);
        for (int j = 0; j < n; ++j) {
            if (zero_width_[j]) flipped[j] = 0;  // both bounds are the same point
            pos[j] = zero_width_[j] ? -3 : (flipped[j] ? -2 : -1);
        }
        for (int i = 0; i < m; ++i) pos[basis[i]] = i;
        // right-hand side with the complemented columns moved over, bounds of the basic variables
        std::vector<double> ub(n), rhs(m), xub(m);
        RELP_HIP(hipMemcpyAsync(ub.data(), d_.ub, n * sizeof(double), hipMemcpyDeviceToHost, stream_));
        RELP_HIP(hipMemcpyAsync(rhs.data(), d_.rhs0, m * sizeof(double), hipMemcpyDeviceToHost, stream_));
        RELP_HIP(hipStreamSynchronize(stream_));
        for (int j = d_.n_art; j < n; ++j) {
            if (!flipped[j]) continue;
            SparseColumn column = md.column(j - d_.n_art);
            for (size_t e = 0; e < column.nnz(); ++e)
                if (column.index[e] < m) rhs[column.index[e]] -= ub[j] * column.value[e].to_double();
        }
        for (int i = 0; i < m; ++i) xub[i] = ub[basis[i]];
        upload_vec(d_.flipped, flipped, stream_);
        upload_vec(d_.rhs, rhs, stream_);
        upload_vec(d_.xub, xub, stream_);
        RELP_HIP(hipStreamSynchronize(stream_));
    }
    upload_vec(d_.basis, basis, stream_);
    upload_vec(d_.pos, pos, stream_);
    Ctl c{};
    c.forced_q = c.forced_p = -1;
    c.last_selected = -1;
    c.scan_column = std::numeric_limits<int>::max();
    write_ctl(c);
}

// ... and the last: the inverse is that of a basis given from outside, nothing has been counted on it yet.
void Solver::reset_basis_counters() {
    binv_identity_ = false;
    refactors_ = 0;
    refactor_seconds_ = 0.0;
    pivots_[0] = pivots_[1] = 0;
    polishes_ = 0;
    max_residual_ = 0.0;
    since_polish_ = 0;
    polish_scale_ = 1;
    redundant_rows_.clear();
}

long long Solver::iterate(long long count, int* stop_reason) {
    if (phase_ == 0) throw std::runtime_error("no phase started");
    RELP_HIP(hipSetDevice(opt_.device));
    long long done = 0;
    int reason = ST_BUDGET;
    long long iters_before = read_ctl().iters;  // one control-word read per batch: the next batch starts where this one ended
    // LU carry: a batch is one refactorisation cycle (period updates + the pivot that asks for the refactorisation)
    // (the refactorisation beside the pivots needs the host's attention more often than once per cycle: batches of 16 pivots)
    const int full_batch = path_.async_refactor ? (opt_.pivots_per_launch > 0 && opt_.pivots_per_launch < 64 ? opt_.pivots_per_launch : 16) : path_.lu_mode ? path_.refactor_period + 1 : std::max(1, opt_.pivots_per_launch);
    while (done < count) {
        if (async_in_flight_ && hipEventQuery(ev_refactored_) == hipSuccess) finish_async_refactor(iters_before);
        long long room = (!path_.lu_mode && opt_.polish_period > 0) ? (long long)opt_.polish_period * polish_scale_ - since_polish_ : count;
        if (room <= 0) { polish(true); continue; }  // (a polish does not touch the iteration counter)
        int batch = (int)std::min<long long>({count - done, room, (long long)full_batch});
        if (opt_.use_graph && batch == full_batch) {
            build_graph(batch);
            RELP_HIP(hipGraphLaunch(graph_exec_[graph_index()], stream_));
            stats_.launches += path_.launches(batch, false, true);
            stats_.price_launches += batch;
        } else {
            launch_pivots(batch);
        }
        const long long fallbacks_before = device_refactor_failures_;
        Ctl after = read_ctl_after_batch();  // (a refactorisation the kernels gave up on is redone by the host in here: nothing pivoted, go on)
        const bool fell_back = device_refactor_failures_ != fallbacks_before;
        long long made = after.iters - iters_before;
        iters_before = after.iters;
        done += made;
        since_polish_ += made;
        pivots_[phase_ - 1] += made;
        if (made > 0) binv_identity_ = false;  // (the phase hand-over must not take the weights of the identity basis)
        if (made > 0) last_pivot_dual_ = false;
        if (made > 0) dual_weights_current_ = false;
        if (after.status == ST_NO_ENTERING || after.status == ST_UNBOUNDED) { reason = after.status; break; }
        if (after.status == ST_REFACTOR) {  // LU carry: should_refactor (or an unstable update) -- BasisInverse::invert
            // (the new factors may be on their way on the other stream: wait for them, replay, go on; else factorise now)
            if (async_in_flight_ && finish_async_refactor(after.iters)) launch_clear_refactor_status(d_, stream_);
            else refactor_lu(true, /*settle=*/false);  // (the next batch ends in read_ctl)
            continue;
        }
        // the next factors are started early enough that the pivots made meanwhile fit the log of their etas
        if (path_.async_refactor && !async_in_flight_ && after.status == ST_RUNNING && lu().device().inverse_factors == 4 &&
            since_polish_ + LU_LOG_CAPACITY + full_batch > path_.refactor_period)
            start_async_refactor(after.iters);
        if (made == 0 && after.status == ST_RUNNING && !fell_back) break;  // defensive: nothing happened
    }
    if (stop_reason) *stop_reason = reason;
    return done;
}

// phase_one.rs:232-278.  Returns the number of redundant rows (artificials that cannot be pivoted out).
int Solver::drive_out_artificials() {
    const int m = d_.m;
    std::vector<int> basis(m);
    RELP_HIP(hipMemcpyAsync(basis.data(), d_.basis, m * sizeof(int), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
    int redundant = 0;
    for (int r = 0; r < m; ++r) {
        if (basis[r] >= d_.n_art) continue;
        Ctl c = read_ctl();
        c.scan_column = std::numeric_limits<int>::max();
        write_ctl(c);
        if (path_.lu_mode) {  // row r of the inverse by one BTRAN, then the scan of rho_r a_j over the non-basic columns
            double* rowvec = d_.scratch + (d_.m + 1) / 2 + 1 + d_.m;
            int* d_slot = reinterpret_cast<int*>(d_.scratch);
            double* d_one = d_.scratch + (d_.m + 1) / 2 + 1;
            const double one = 1.0;
            RELP_HIP(hipMemcpyAsync(d_slot, &r, sizeof(int), hipMemcpyHostToDevice, stream_));
            RELP_HIP(hipMemcpyAsync(d_one, &one, sizeof(double), hipMemcpyHostToDevice, stream_));
            launch_lu_btran(lu().device(), d_slot, d_one, 1, rowvec, stream_);
            launch_lu_row_scan(d_, rowvec, 1e-7, stream_);
        } else if (path_.network) {  // row r of the inverse from the forest, then the same scan
            double* rowvec = d_.scratch + (d_.m + 1) / 2 + 1 + d_.m;
            launch_net_row(d_, net_, r, rowvec, stream_);
            launch_lu_row_scan(d_, rowvec, 1e-7, stream_);
        } else {
            launch_row_scan(d_, r, 1e-7, stream_);
        }
        c = read_ctl();
        if (c.scan_column == std::numeric_limits<int>::max()) {
            redundant_rows_.push_back(r);
            ++redundant;
            continue;
        }
        c.forced_q = c.scan_column;
        c.forced_p = r;
        c.status = ST_RUNNING;
        write_ctl(c);
        // a zero-level pivot: the artificial that leaves IS zero (the phase-one objective vanished); whatever residue f64 left
        // in x_B[r] must not be divided by a small pivot element and spread over x_B
        RELP_HIP(hipMemsetAsync(d_.xB + r, 0, sizeof(double), stream_));
        launch_pivots(1, true);
        Ctl after = read_ctl();
        if (after.iters == c.iters) throw std::runtime_error("zero-level pivot failed");
        pivots_[0] += 1;
        since_polish_ += 1;
        if (after.status == ST_REFACTOR) refactor_lu(true);
    }
    return redundant;
}

void Solver::solve(relp_result* result) {
    if (!loaded_) throw std::runtime_error("no LP loaded");
    RELP_HIP(hipSetDevice(opt_.device));
    const double t0 = now_seconds();
    exact_objective.clear();
    exact_primal.reset();
    exact_witnesses.reset();
    const bool timing = diagnostic("RELP_TIME_SOLVE");  // diagnostic: host-side timeline of one solve
    double t_last = t0;
    auto tick = [&](const char* what) {
        if (!timing) return;
        RELP_HIP(hipStreamSynchronize(stream_));
        const double t = now_seconds();
        fprintf(stderr, "[solve] %-24s %.3f ms\n", what, (t - t_last) * 1e3);
        t_last = t;
    };
    begin_phase_one();
    tick("begin_phase_one");
    // 0: a safety cap far above anything a terminating solve needs (GREENBEA: 8349 pivots with m + n = 8776), so that an LP
    // that cycles in f64 comes back as RELP_RESULT_ITERATION_LIMIT instead of never
    const long long cap = opt_.max_pivots > 0 ? opt_.max_pivots : 200LL * (d_.m + d_.n) + 100000;
    int kind = RELP_RESULT_NONE;
    if (phase_ == 1) {
        int reason = 0;
        long long done = iterate(cap, &reason);
        (void)done;
        tick("phase one loop");
        if (reason == ST_UNBOUNDED) throw std::runtime_error("Artificial cost can not be unbounded.");  // phase_one.rs:151
        if (reason == ST_BUDGET) kind = RELP_RESULT_ITERATION_LIMIT;
        if (kind == RELP_RESULT_NONE) {
            polish(true);
            tick("polish");
            RELP_HIP(hipMemcpyAsync(h_rb_xb_, d_.xB, d_.m * sizeof(double), hipMemcpyDeviceToHost, stream_));
            Ctl c = read_ctl();  // (waits for x_B too)
            double scale = 1.0;
            for (int i = 0; i < d_.m; ++i) scale += std::fabs(h_rb_xb_[i]);
            if (-c.minus_obj > opt_.tol_feasible * scale) {
                kind = RELP_RESULT_INFEASIBLE;  // phase_one.rs:171-173
            } else {
                tick("feasibility check");
                drive_out_artificials();
                tick("drive out artificials");
                set_phase(2);
                tick("set_phase(2)");
            }
        }
    }
    if (kind == RELP_RESULT_NONE) {
        int reason = 0;
        iterate(cap - pivots_[0], &reason);
        tick("phase two loop");
        if (reason == ST_UNBOUNDED) kind = RELP_RESULT_UNBOUNDED;  // phase_two.rs:53
        else if (reason == ST_NO_ENTERING) {
            kind = RELP_RESULT_FINITE_OPTIMUM;
            polish(true);
            tick("final polish");
        } else kind = RELP_RESULT_ITERATION_LIMIT;
    }
    collect_result(kind, t0, true, tick, result);
}

// The tail of a solve (`solve`, `solve_dual`): the basis and the vertex read back, the result struct, the exact certificate.
void Solver::collect_result(int kind, double t0, bool certify_verdicts, const std::function<void(const char*)>& tick, relp_result* result) {
    relp_result res{};
    // results: Carry::current_bfs (carry/mod.rs:636-645) + reconstruct_solution (matrix_data.rs:402-411)
    const int m = d_.m;
    // (into the handle's pinned buffers, all behind the one wait of read_ctl)
    RELP_HIP(hipMemcpyAsync(h_rb_basis_, d_.basis, m * sizeof(int), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipMemcpyAsync(h_rb_xb_, d_.xB, m * sizeof(double), hipMemcpyDeviceToHost, stream_));
    if (path_.bounded) {
        RELP_HIP(hipMemcpyAsync(h_rb_flipped_, d_.flipped, d_.n * sizeof(int), hipMemcpyDeviceToHost, stream_));
        RELP_HIP(hipMemcpyAsync(h_rb_pos_, d_.pos, d_.n * sizeof(int), hipMemcpyDeviceToHost, stream_));
        RELP_HIP(hipMemcpyAsync(h_rb_ub_, d_.ub, d_.n * sizeof(double), hipMemcpyDeviceToHost, stream_));
    }
    Ctl c = read_ctl();
    const std::vector<int> basis(h_rb_basis_, h_rb_basis_ + m);
    const double* xb = h_rb_xb_;
    for (int i = 0; i < m; ++i)  // never index host arrays with an unchecked device value
        if (basis[i] < 0 || basis[i] >= d_.n) throw std::runtime_error("the device returned an invalid basis (row " + std::to_string(i) + ")");
    std::fill(h_solution_.begin(), h_solution_.end(), 0.0);
    if (!path_.bounded) {
        for (int i = 0; i < m; ++i) {
            h_basis_[i] = cols_.to_provider(basis[i]);
            if (basis[i] >= d_.n_art) h_solution_[basis[i] - d_.n_art] = xb[i];
        }
    } else {
        // back to the reference's formulation: values of complemented variables are u_j - x'_j, a complemented non-basic
        // variable sits at its upper bound, and the basis of the full MatrixData has, on every bound row, the bound slack
        // (variable below its bound) or the variable itself (variable at its bound).
        const MatrixData& md = form_.data;
        const std::vector<int> flipped(h_rb_flipped_, h_rb_flipped_ + d_.n);
        std::vector<int> pos(h_rb_pos_, h_rb_pos_ + d_.n);
        const std::vector<double> ub(h_rb_ub_, h_rb_ub_ + d_.n);
        resolve_fixed_columns(pos);
        h_basis_ = explicit_basis(basis, pos);
        explicit_solution(md, cols_, basis, xb, flipped, pos, ub, h_solution_);
    }
    if (net_.stats) {
        net_stats_.assign(NS_WORDS, 0);
        RELP_HIP(hipMemcpyAsync(net_stats_.data(), net_.stats, NS_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream_));
        RELP_HIP(hipStreamSynchronize(stream_));
    }
    res.kind = kind;
    res.pivots_phase_one = pivots_[0];
    res.pivots_phase_two = pivots_[1];
    res.polishes = polishes_;
    res.max_residual = max_residual_;
    res.refactors = refactors_;
    res.refactor_seconds = refactor_seconds_;
    res.objective = (kind == RELP_RESULT_FINITE_OPTIMUM) ? -c.minus_obj + form_.fixed_cost.to_double()
                                                         : std::numeric_limits<double>::quiet_NaN();
    tick("results");
    res.solve_seconds = now_seconds() - t0;
    // The exact certificate: optimality of the final basis; for the two other verdicts of `OptimizationResult`
    // (algorithm/mod.rs:43-47), which the reference decides exactly, a Farkas certificate / an unbounded ray.
    unbounded_column_ = kind == RELP_RESULT_UNBOUNDED ? c.q - d_.n_art : -1;
    if (opt_.certify && !path_.bounded && (kind == RELP_RESULT_FINITE_OPTIMUM || (certify_verdicts && (kind == RELP_RESULT_INFEASIBLE || kind == RELP_RESULT_UNBOUNDED))))
        certify(&res);
    else if (opt_.certify && kind == RELP_RESULT_FINITE_OPTIMUM) certify(&res);
    last_result = res;
    if (result) *result = res;
}

// Implicit bounds: the basis of the reference's formulation (all rows of MatrixData) that the device state stands for.  On
// every bound row the bound slack is basic when the variable is below its bound and the variable itself when it sits at it.
// A fixed variable (pos -3) sits at both of its bounds at once; which of the two the reference's formulation should see is
// decided by its reduced cost, exactly as the bound flips of a zero step used to do: negative -> "at the upper bound" (the
// variable itself basic on its bound row), else the bound slack.  Rewrites the -3 entries of `pos` to -2 / -1.
void Solver::resolve_fixed_columns(std::vector<int>& pos) {
    bool any = false;
    for (int j = d_.n_art; j < d_.n && !any; ++j) any = pos[j] == -3;
    if (!any) return;
    std::vector<double> cbar(d_.n);
    relative_costs(cbar.data());
    for (int j = d_.n_art; j < d_.n; ++j)
        if (pos[j] == -3) pos[j] = cbar[j] < 0.0 ? -2 : -1;
}

std::vector<int> Solver::explicit_basis(const std::vector<int>& basis, const std::vector<int>& pos) const {
    return relp::explicit_basis(form_.data, cols_, basis, pos);
}

void Solver::certify(relp_result* result) {
    if (path_.network) {  // from the forest, O(m + n) (certify_basis needs m^2 words); the other verdicts stay uncertified here
        if (result->kind == RELP_RESULT_FINITE_OPTIMUM) net_certify(result);
        else last_error = "RELP_CARRY_NETWORK certifies finite optima only";
        return;
    }
    const double t0 = now_seconds();
    bool ok = false;
    long long repairs = 0;
    std::string message;
    try {
        const int mode = result->kind == RELP_RESULT_INFEASIBLE ? 1 : result->kind == RELP_RESULT_UNBOUNDED ? 2 : 0;
        certify_basis(form_, h_basis_, opt_.device, stream_, &exact_objective, &ok, &repairs, &message, mode, unbounded_column_, &exact_primal, &certify_scratch_,
                      &exact_witnesses);
    } catch (const RatOverflow& e) {  // the f64 result stands; it is reported uncertified with the reason
        ok = false;
        message = std::string("exact certificate: ") + e.what();
    }
    result->certified = ok ? 1 : 0;
    result->exact_repair_pivots = repairs;
    result->certify_seconds = now_seconds() - t0;
    if (!ok) last_error = message;
}

// ---- dual simplex from a given basis (dual.hip) -------------------------------------------------------
// The optimal basis of an LP stays dual feasible when rows are appended or a right-hand side is tightened, and is primal infeasible
// where the change bites: the caller loads the changed LP and passes the old basis, extended by the slack of each new row.
void Solver::check_dual_start(const int* basis_columns, bool bounded_entry) const {
    if (!loaded_) throw std::runtime_error("no LP loaded");
    const std::string refusal = bounded_entry ? dual_bounded_refusal(path_) : dual_refusal(path_);
    if (!refusal.empty()) throw std::invalid_argument(refusal);
    if (!bounded_entry && dual_long_step_)
        throw std::invalid_argument("begin_dual: the long-step ratio test is switched on (relp_set_dual_long_step), and only the loop on implicit upper bounds has it: "
                                    "relp_begin_dual_bounded / relp_solve_dual_bounded take this call, or switch it off");
    const int rows = path_.bounded ? form_.data.nr_rows() : d_.m;  // (implicit bounds: a basis of the formulation, bound rows included)
    for (int i = 0; i < rows; ++i)
        if (basis_columns[i] < 0)
            throw std::invalid_argument("begin_dual: the basis holds an artificial column (code " + std::to_string(basis_columns[i]) + " on row " + std::to_string(i) +
                                        "): the dual simplex starts from a basis of the LP's own columns");
}

void Solver::begin_dual(const int* basis_columns) { start_dual_from_scratch(basis_columns, false); }
// Implicit upper bounds: the same start -- place_basis reduces the formulation's basis to the constraint rows, complements the columns
// at their upper bound and moves them over to the right-hand side -- and the loop of the BOUNDED kernels behind it (launch_dual_pivots).
void Solver::begin_dual_bounded(const int* basis_columns) { start_dual_from_scratch(basis_columns, true); }

void Solver::start_dual_from_scratch(const int* basis_columns, bool bounded_entry) {
    check_dual_start(basis_columns, bounded_entry);
    RELP_HIP(hipSetDevice(opt_.device));
    const double t0 = now_seconds();
    const long long gemms_before = polish_gemms_;
    dual_start_ = "none";
    dual_inherit_complemented_ = dual_inherit_moved_ = 0;
    set_basis(basis_columns);  // inverse from scratch, x_B, the costs of phase two, -pi; every column of the inverse marked touched
    dual_start_residual_ = -1.0;  // (no guard: the inverse was iterated to its own stopping rule)
    finish_dual_start(basis_columns, "scratch", t0, gemms_before);
}

std::vector<int> Solver::provider_basis() const {
    std::vector<int> basis(d_.m);
    RELP_HIP(hipMemcpyAsync(basis.data(), d_.basis, d_.m * sizeof(int), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
    for (int& column : basis) column = cols_.to_provider(column);
    return basis;
}

// The child of a cut loop or of a branching step: `parent` holds the inverse of all but k rows of this basis, polished, on the same
// device (dual_inherit.hpp has the block form).  Everything that can refuse does so before the first launch.
void Solver::begin_dual_from(const Solver& parent, const int* basis_columns) {
    if (!loaded_) throw std::runtime_error("no LP loaded");
    if (&parent == this) throw std::runtime_error("begin_dual_from: the parent is this handle itself (the child is loaded on a handle of its own)");
    if (!parent.loaded_) throw std::runtime_error("begin_dual_from: the parent handle has no LP loaded");
    const std::string parent_plan = dual_refusal(parent.path_);
    if (!parent_plan.empty()) throw std::invalid_argument("begin_dual_from: the parent's plan: " + parent_plan);
    check_dual_start(basis_columns);
    if (parent.opt_.device != opt_.device)
        throw std::invalid_argument("begin_dual_from: the parent is on device " + std::to_string(parent.opt_.device) + ", this handle on device " +
                                    std::to_string(opt_.device) + ": the inverse is inherited on one device");
    if (parent.phase_ == 0)
        throw std::runtime_error("begin_dual_from: the parent has no basis and inverse yet (a solve, set_basis or solve_dual on it comes first)");
    RELP_HIP(hipSetDevice(opt_.device));
    const std::string relation = dual_inherit_refusal(parent.form_, form_, parent.provider_basis(), std::vector<int>(basis_columns, basis_columns + d_.m));
    if (!relation.empty()) throw std::invalid_argument("begin_dual_from: " + relation);
    const double t0 = now_seconds();
    const long long gemms_before = polish_gemms_;
    dual_start_ = "none";
    dual_inherit_complemented_ = dual_inherit_moved_ = 0;
    place_basis(basis_columns);
    if (!ev_parent_) RELP_HIP(hipEventCreateWithFlags(&ev_parent_, hipEventDisableTiming));
    RELP_HIP(hipEventRecord(ev_parent_, parent.stream_));  // whatever the parent still has on its way to its inverse comes first
    RELP_HIP(hipStreamWaitEvent(stream_, ev_parent_, 0));
    stats_.launches += 2;
    launch_dual_inherit(d_, parent.d_.Binv, parent.d_.m, parent.d_.ld, stream_);
    launch_mark_all_touched(d_, stream_);  // no column of an inherited inverse is known to be a unit vector
    reset_basis_counters();
    // The guard: max |I - B Binv| of this basis against this LP's own matrix; below 1e-12 it adds nothing, otherwise one or two
    // Newton-Schulz steps, from 0.5 on the from-scratch inverse.  It also refreshes x_B (and -pi, which set_phase recomputes with the
    // costs of phase two in place: the copy below only keeps the polish's own -pi pass off a cost vector nothing has written yet).
    RELP_HIP(hipMemcpyAsync(d_.cost, d_.cost2, d_.n * sizeof(double), hipMemcpyDeviceToDevice, stream_));
    polish_first_residual_ = -1.0;
    polish(true, true);
    dual_start_residual_ = polish_first_residual_;
    RELP_HIP(hipStreamSynchronize(stream_));  // the parent's inverse has been read: the caller may use the parent again
    set_phase(2);
    finish_dual_start(basis_columns, polish_rebuilt_ ? "scratch_after_inherit" : "inherited", t0, gemms_before);
}

void Solver::held_state(std::vector<int>* basis, std::vector<int>* pos, std::vector<int>* flipped) const {
    basis->resize(d_.m);
    pos->resize(d_.n);
    flipped->assign(d_.n, 0);
    RELP_HIP(hipMemcpyAsync(basis->data(), d_.basis, d_.m * sizeof(int), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipMemcpyAsync(pos->data(), d_.pos, d_.n * sizeof(int), hipMemcpyDeviceToHost, stream_));
    if (path_.bounded) RELP_HIP(hipMemcpyAsync(flipped->data(), d_.flipped, d_.n * sizeof(int), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
}

// begin_dual_from between two LPs held on implicit upper bounds, step by step.  The child of a branching step keeps its parent's
// constraint rows, so its basis matrix is the parent's up to the order of the positions and the sign of the columns one side holds
// complemented: the relation (dual_bounded_inherit_refusal) names the parent's column behind every position, the parent's device state
// its position and sign there.  Everything that can refuse does so before the first launch.
void Solver::begin_dual_bounded_from(const Solver& parent, const int* basis_columns) {
    if (!loaded_) throw std::runtime_error("no LP loaded");
    if (&parent == this) throw std::runtime_error("begin_dual_bounded_from: the parent is this handle itself (the child is loaded on a handle of its own)");
    if (!parent.loaded_) throw std::runtime_error("begin_dual_bounded_from: the parent handle has no LP loaded");
    const std::string parent_plan = dual_bounded_refusal(parent.path_);
    if (!parent_plan.empty()) throw std::invalid_argument("begin_dual_bounded_from: the parent's plan: " + parent_plan);
    check_dual_start(basis_columns, true);
    for (const Solver* handle : {&parent, (const Solver*)this})
        if (!handle->path_.bounded && handle->form_.data.nr_variable_bounds() > 0)
            throw std::invalid_argument(std::string("begin_dual_bounded_from: ") + (handle == this ? "this handle" : "the parent") +
                                        " holds its upper bounds as rows of the device LP (implicit_bounds = 0): the relation is one of LPs held on implicit bounds");
    if (parent.opt_.device != opt_.device)
        throw std::invalid_argument("begin_dual_bounded_from: the parent is on device " + std::to_string(parent.opt_.device) + ", this handle on device " +
                                    std::to_string(opt_.device) + ": the inverse is inherited on one device");
    if (parent.phase_ == 0)
        throw std::runtime_error("begin_dual_bounded_from: the parent has no basis and inverse yet (a solve, set_basis or solve_dual_bounded on it comes first)");
    RELP_HIP(hipSetDevice(opt_.device));
    // the parent's basis of its formulation and where it holds each column, off its device state (copies: nothing is launched)
    std::vector<int> parent_basis, parent_pos, parent_flipped;
    parent.held_state(&parent_basis, &parent_pos, &parent_flipped);
    const std::vector<int> parent_formulation = parent.path_.bounded ? parent.explicit_basis(parent_basis, parent_pos) : parent.cols_.to_provider(parent_basis);
    std::vector<int> source;
    const std::string relation = dual_bounded_inherit_refusal(parent.form_, form_, parent_formulation,
                                                              std::vector<int>(basis_columns, basis_columns + form_.data.nr_rows()), &source);
    if (!relation.empty()) throw std::invalid_argument("begin_dual_bounded_from: " + relation);
    const int m = d_.m, m_parent = parent.d_.m;
    std::vector<int> map(2 * (size_t)m, 1);  // src | sg
    std::vector<int> parent_column(m, -1);
    for (int i = 0; i < m; ++i) {
        map[i] = source[i];
        if (source[i] < 0) continue;
        parent_column[i] = parent.cols_.to_device(source[i]);
        map[i] = parent_pos[parent_column[i]];
        if (map[i] < 0 || map[i] >= m_parent)
            throw std::runtime_error("begin_dual_bounded_from: column " + std::to_string(source[i]) + " of the parent is not basic on its device");
    }
    const double t0 = now_seconds();
    const long long gemms_before = polish_gemms_;
    dual_start_ = "none";
    dual_inherit_complemented_ = dual_inherit_moved_ = 0;
    place_basis(basis_columns);
    // the signs: the parent's as its walk left them; this handle's as place_basis has just written them (+1 on every basic column)
    std::vector<int> basis, pos, flipped;
    held_state(&basis, &pos, &flipped);
    long long complemented = 0, moved = 0;
    for (int i = 0; i < m; ++i) {
        if (map[i] < 0) continue;
        map[m + i] = (parent_flipped[parent_column[i]] ? -1 : 1) * (flipped[basis[i]] ? -1 : 1);
        complemented += map[m + i] < 0;
        moved += map[i] != i;
    }
    if (!d_inherit_map_) d_inherit_map_ = device_alloc<int>(2 * (size_t)m);
    upload_vec(d_inherit_map_, map, stream_);
    if (!ev_parent_) RELP_HIP(hipEventCreateWithFlags(&ev_parent_, hipEventDisableTiming));
    RELP_HIP(hipEventRecord(ev_parent_, parent.stream_));  // whatever the parent still has on its way to its inverse comes first
    RELP_HIP(hipStreamWaitEvent(stream_, ev_parent_, 0));
    stats_.launches += 2;
    launch_dual_inherit_mapped(d_, parent.d_.Binv, m_parent, parent.d_.ld, d_inherit_map_, d_inherit_map_ + m, stream_);
    launch_mark_all_touched(d_, stream_);  // no column of an inherited inverse is known to be a unit vector
    reset_basis_counters();
    // the guard of begin_dual_from, with its threshold
    RELP_HIP(hipMemcpyAsync(d_.cost, d_.cost2, d_.n * sizeof(double), hipMemcpyDeviceToDevice, stream_));
    polish_first_residual_ = -1.0;
    polish(true, true);
    dual_start_residual_ = polish_first_residual_;
    RELP_HIP(hipStreamSynchronize(stream_));  // the parent's inverse and the map have been read: the caller may use the parent again
    set_phase(2);
    finish_dual_start(basis_columns, polish_rebuilt_ ? "scratch_after_inherit" : "inherited", t0, gemms_before);
    dual_inherit_complemented_ = complemented;
    dual_inherit_moved_ = moved;
}

void Solver::finish_dual_start(const int* basis_columns, const char* how, double t0, long long gemms_before) {
    const int m = d_.m, n = d_.n, n_art = d_.n_art;
    if (!dual_.alpha_row) {
        dual_.blocks = dual_blocks(n_art, n);
        dual_.alpha_row = device_alloc<double>(n);
        dual_.d = device_alloc<double>(n);
        dual_.part_theta = device_alloc<double>(dual_.blocks);
        dual_.cand_key = device_alloc<double>(dual_.blocks);
        dual_.cand_j = device_alloc<int>(dual_.blocks);
    }
    if (steepest_dual() && !dual_.beta) {  // (rule 0 allocates nothing more than it did)
        dual_.slices = dual_weight_slices(m);
        dual_.beta = device_alloc<double>(m);
        if (dual_.slices > 1) dual_.beta_part = device_alloc<double>((size_t)dual_.slices * m);
    }
    dual_long_active_ = dual_long_step_ && path_.bounded;
    if (dual_long_active_ && !dual_.flip_count) {  // (with the switch off nothing more is allocated than was)
        dual_.flip_count = device_alloc<int>(4);
        dual_.flip_j = device_alloc<int>(DUAL_MAX_FLIPS);
        dual_.flip_w = device_alloc<double>(m);
        h_flip_totals_ = pinned_memory_.alloc<int>(2);
    }
    if (dual_long_active_) RELP_HIP(hipMemsetAsync(dual_.flip_count, 0, 4 * sizeof(int), stream_));
    dual_flips_ = dual_long_skipped_ = 0;
    dual_farkas_active_ = dual_farkas_;
    dual_farkas_row_ = -1;
    dual_cutoff_active_ = dual_cutoff_on_;
    dual_cutoff_read_ = dual_cutoff_;
    dual_cutoff_carry_ = dual_cutoff_ - form_.fixed_cost.to_double();  // (Ctl::minus_obj does not hold the fixed cost: collect_result adds it)
    dual_cutoff_stopped_ = dual_bound_proved_ = false;
    const size_t lds_max = opt_.price_lds_max > 0 ? (size_t)opt_.price_lds_max : (size_t)96 * 1024;
    dual_lds_ = 2 * (size_t)m * sizeof(double) <= lds_max;
    std::vector<double> cbar(n);
    relative_costs(cbar.data());
    if (path_.bounded) {  // the signed costs of the held form; a fixed column (pos -3) is never priced, a basic one is zero up to rounding
        std::vector<int> pos(n);
        RELP_HIP(hipMemcpyAsync(pos.data(), d_.pos, n * sizeof(int), hipMemcpyDeviceToHost, stream_));
        RELP_HIP(hipStreamSynchronize(stream_));
        for (int j = n_art; j < n; ++j) cbar[j] = pos[j] == -1 ? cbar[j] : pos[j] == -2 ? -cbar[j] : 0.0;
    } else {
        for (int i = 0; i < m; ++i) cbar[cols_.to_device(basis_columns[i])] = 0.0;  // (a basic column's is zero up to rounding)
    }
    for (int j = n_art; j < n; ++j)
        if (cbar[j] < -opt_.tol_dual) {
            char value[32];
            snprintf(value, sizeof(value), "%.6g", cbar[j]);
            throw std::invalid_argument("begin_dual: the basis is not dual feasible: column " + std::to_string(j - n_art) + " has the relative cost " + value +
                                        " (a primal clean-up from such a basis is not part of the dual simplex)");
        }
    dual_pivots_ = 0;
    dual_device_seconds_ = 0.0;
    dual_ready_ = true;
    dual_bounded_ = path_.bounded;
    dual_weights_current_ = false;
    refresh_dual_weights();  // (behind either start: the inverse is final here)
    RELP_HIP(hipStreamSynchronize(stream_));
    dual_start_ = how;
    dual_start_seconds_ = now_seconds() - t0;
    dual_start_gemms_ = polish_gemms_ - gemms_before;
}

// The weights of the steepest-edge leaving rule from the inverse as it stands (a no-op under rule 0, before a start, and while they are
// current): at the end of either start, and in front of the first batch of dual pivots after anything but a dual pivot has written
// the inverse -- a polish (inside iterate_dual, the forced ones of run_dual, refactor) or primal pivots.
void Solver::refresh_dual_weights() {
    if (!steepest_dual() || !dual_ready_ || dual_weights_current_) return;
    stats_.launches += launch_dual_weights(d_, dual_, false, stream_);
    dual_weights_current_ = true;
}

void Solver::dual_weights(double* out) {
    if (!loaded_) throw std::runtime_error("no LP loaded");
    if (!steepest_dual()) throw std::runtime_error("dual_weights: the handle's dual_pricing is 0 (largest infeasibility keeps no weights)");
    if (!dual_ready_) throw std::runtime_error("dual_weights: no dual loop started (begin_dual comes first)");
    RELP_HIP(hipSetDevice(opt_.device));
    refresh_dual_weights();
    RELP_HIP(hipMemcpyAsync(out, dual_.beta, d_.m * sizeof(double), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
}

// One batch: the budget, then five launches per pivot (dual.hpp) -- six with the long-step ratio test --, and behind them the one or two
// of the weights under the steepest-edge rule.  The chain is a run of no-ops from the first kernel that stops it.
void Solver::launch_dual_pivots(int count) {
    stats_.launches += 1 + (dual_long_active_ ? 6LL : 5LL) * count;
    launch_budget(d_, count, stream_);
    const bool textbook = path_.ratio_textbook;
    for (int it = 0; it < count; ++it) {
        launch_dual_leave(d_, opt_.harris_delta, dual_.beta, path_.bounded, dual_cutoff_active_, dual_cutoff_carry_, stream_);
        launch_dual_row(d_, dual_, dual_lds_, path_.bounded, opt_.tol_pivot, textbook ? 0.0 : opt_.tol_dual, stream_);
        if (dual_long_active_) launch_dual_long_step(d_, dual_, opt_.tol_pivot, textbook ? 0.0 : opt_.tol_dual, opt_.harris_delta, stream_);
        launch_dual_choose(d_, dual_, opt_.tol_pivot, textbook, stream_);
        launch_dual_pivot(d_, dual_, path_.bounded, dual_long_active_, opt_.tol_pivot, stream_);
        launch_dual_update(d_, stream_);
        if (dual_.beta) stats_.launches += launch_dual_weights(d_, dual_, true, stream_);
    }
}

long long Solver::iterate_dual(long long count, int* stop_reason) {
    if (!dual_ready_) throw std::runtime_error("iterate_dual: no dual loop started (begin_dual comes first)");
    RELP_HIP(hipSetDevice(opt_.device));
    long long done = 0;
    int reason = ST_BUDGET;
    Ctl c = read_ctl();
    if (c.status != ST_RUNNING) {  // an earlier loop stopped here: whether a row is infeasible now is for the kernels to say
        c.status = ST_RUNNING;
        write_ctl(c);
    }
    long long iters_before = c.iters;
    const int full_batch = std::max(1, opt_.pivots_per_launch);
    bool polished_for_pivot = false;
    while (done < count) {
        const long long room = opt_.polish_period > 0 ? (long long)opt_.polish_period * polish_scale_ - since_polish_ : count;
        if (room <= 0) { polish(true); continue; }
        refresh_dual_weights();  // (after a polish here, in the ST_REFACTOR path below or in run_dual, or primal pivots since the last batch)
        const int batch = (int)std::min<long long>({count - done, room, (long long)full_batch});
        RELP_HIP(hipEventRecord(ev_a_, stream_));  // the device time of the batch, for relp_get_record_json ("dual_device_seconds")
        launch_dual_pivots(batch);
        RELP_HIP(hipEventRecord(ev_b_, stream_));
        Ctl after = read_ctl();
        if (dual_long_active_) {  // the two totals since the start (dual_pivot_kernel adds to them behind its guard)
            RELP_HIP(hipMemcpyAsync(h_flip_totals_, dual_.flip_count + 2, 2 * sizeof(int), hipMemcpyDeviceToHost, stream_));  // (pinned, as the control block's mirror)
            RELP_HIP(hipStreamSynchronize(stream_));
            dual_flips_ = h_flip_totals_[0];
            dual_long_skipped_ = h_flip_totals_[1];
        }
        float batch_ms = 0.0f;
        RELP_HIP(hipEventElapsedTime(&batch_ms, ev_a_, ev_b_));
        dual_device_seconds_ += 1e-3 * batch_ms;
        const long long made = after.iters - iters_before;
        iters_before = after.iters;
        done += made;
        since_polish_ += made;
        dual_pivots_ += made;
        if (made > 0) {
            binv_identity_ = false;
            last_pivot_dual_ = true;
        }
        if (after.status == ST_NO_ENTERING || after.status == ST_UNBOUNDED) { reason = after.status; break; }
        if (after.status == ST_CUTOFF) {  // (only under set_dual_cutoff: the objective of this basis has reached the cutoff)
            dual_cutoff_stopped_ = true;
            reason = ST_CUTOFF;
            break;
        }
        if (after.status == ST_REFACTOR) {
            // dual_pivot_kernel found the FTRAN value of its pivot unusable where the row's value was usable: the inverse has drifted.
            // Nothing of that pivot was written.  A forced polish, and the loop asks again; twice in a row at one basis is an error.
            if (made == 0 && polished_for_pivot) throw std::runtime_error("iterate_dual: the pivot element of row " + std::to_string(after.p) +
                                                                          " is not usable after a polish of the inverse (an ill-conditioned basis)");
            polish(true, true);
            polished_for_pivot = true;
            after.status = ST_RUNNING;
            write_ctl(after);
            continue;
        }
        polished_for_pivot = false;
        if (made == 0) break;  // defensive: nothing happened
    }
    if (stop_reason) *stop_reason = reason;
    return done;
}

void Solver::solve_dual(const int* basis_columns, relp_result* result) { run_dual(nullptr, basis_columns, result); }
void Solver::solve_dual_from(const Solver& parent, const int* basis_columns, relp_result* result) { run_dual(&parent, basis_columns, result); }
void Solver::solve_dual_bounded(const int* basis_columns, relp_result* result) { run_dual(nullptr, basis_columns, result, true); }
void Solver::solve_dual_bounded_from(const Solver& parent, const int* basis_columns, relp_result* result) { run_dual(&parent, basis_columns, result, true); }

void Solver::run_dual(const Solver* parent, const int* basis_columns, relp_result* result, bool bounded_entry) {
    if (!loaded_) throw std::runtime_error("no LP loaded");
    RELP_HIP(hipSetDevice(opt_.device));
    const double t0 = now_seconds();
    exact_objective.clear();
    exact_primal.reset();
    exact_witnesses.reset();
    if (parent && bounded_entry) begin_dual_bounded_from(*parent, basis_columns);
    else if (parent) begin_dual_from(*parent, basis_columns);
    else start_dual_from_scratch(basis_columns, bounded_entry);
    const long long cap = opt_.max_pivots > 0 ? opt_.max_pivots : 200LL * (d_.m + d_.n) + 100000;
    int kind = RELP_RESULT_NONE;
    int reason = 0;
    iterate_dual(cap, &reason);
    // primal feasible in f64: the same question again on the polished state, while that still finds an infeasible row
    for (int round = 0; round < 3 && reason == ST_NO_ENTERING; ++round) {
        polish(true, true);
        if (iterate_dual(cap - dual_pivots_, &reason) == 0) break;
    }
    if (reason == ST_UNBOUNDED) kind = RELP_RESULT_INFEASIBLE;
    else if (reason == ST_CUTOFF) kind = RELP_RESULT_CUTOFF;  // (no primal clean-up: the basis is not primal feasible, and need not be)
    else if (reason != ST_NO_ENTERING) kind = RELP_RESULT_ITERATION_LIMIT;
    // under set_dual_cutoff the basis the dual loop itself stopped on has an objective worth reporting: a lower bound of the LP
    const bool dual_bound = dual_cutoff_active_ && (kind == RELP_RESULT_CUTOFF || kind == RELP_RESULT_ITERATION_LIMIT);
    if (kind == RELP_RESULT_NONE) {
        // the primal loop from the primal-feasible basis: the weights recomputed, the control block reset (minus_obj kept); it
        // removes relative costs that drifted below -tol_dual and normally makes no pivot
        set_phase(2);
        iterate(cap - dual_pivots_, &reason);
        if (reason == ST_UNBOUNDED) kind = RELP_RESULT_UNBOUNDED;
        else if (reason == ST_NO_ENTERING) {
            kind = RELP_RESULT_FINITE_OPTIMUM;
            polish(true);
        } else kind = RELP_RESULT_ITERATION_LIMIT;
    }
    const bool dual_unbounded = kind == RELP_RESULT_INFEASIBLE;
    collect_result(kind, t0, !dual_unbounded, [](const char*) {}, result);
    if (dual_bound) {
        last_result.objective = -read_ctl().minus_obj + form_.fixed_cost.to_double();
        if (result) *result = last_result;
        if (opt_.certify) certify_dual_lower_bound(result);
    }
    if (dual_unbounded && dual_farkas_active_ && opt_.certify) certify_dual_infeasible(result);
    else if (dual_unbounded)  // (without relp_set_dual_farkas: reported with certified = 0 whatever the options ask for)
        last_error ="the dual simplex does not certify infeasibility yet (the Farkas vector is the row of the inverse at which the dual is unbounded)";
}

// dual_pivot_kernel clears Ctl::p where it stops the loop, and nothing has written x_B, the basis or the weights since: the leaving-row
// kernel, alone and under a status that lets it run, names the row again.  The control block is put back as the loop left it.
int Solver::dual_stopped_row() {
    const Ctl stopped = read_ctl();
    if (stopped.status != ST_UNBOUNDED) return -1;
    Ctl running = stopped;
    running.status = ST_RUNNING;
    write_ctl(running);
    stats_.launches += 1;
    launch_dual_leave(d_, opt_.harris_delta, dual_.beta, path_.bounded, false, 0.0, stream_);  // (never the cutoff's: it would stop in front of the row)
    const Ctl named = read_ctl();
    write_ctl(stopped);
    return named.status == ST_RUNNING && named.p >= 0 && named.p < d_.m ? named.p : -1;
}

// The INFEASIBLE verdict of the dual loop, proved: row p of the exact inverse is the Farkas vector (certify.hpp: certify_dual_farkas).
// The basis is the one the device holds -- on implicit bounds its constraint rows, uncomplemented: the closed form over the bound rows
// does not ask where a column sits --, and the f64 state only says which sign of the row to try first.
void Solver::certify_dual_infeasible(relp_result* result) {
    const double t0 = now_seconds();
    bool ok = false;
    std::string message;
    const int p = dual_stopped_row();
    if (p < 0) {
        message = "dual Farkas: the loop does not stand at a dual unbounded row";
    } else {
        std::vector<int> basis(d_.m);
        for (int i = 0; i < d_.m; ++i) basis[i] = cols_.to_provider(h_rb_basis_[i]);  // (collect_result's read-back)
        int first_sign = -1;
        if (path_.bounded) {
            const int column = h_rb_basis_[p];
            const bool below = !(h_rb_xb_[p] - h_rb_ub_[column] > -h_rb_xb_[p]);  // (dual_side of dual.hip)
            first_sign = below != (h_rb_flipped_[column] != 0) ? -1 : 1;
        }
        try {
            certify_dual_farkas(form_, basis, p, path_.bounded, first_sign, opt_.device, stream_, &exact_objective, &ok, &message, &certify_scratch_, &exact_witnesses);
        } catch (const RatOverflow& e) {  // (as certify())
            ok = false;
            message = std::string("exact certificate: ") + e.what();
        }
        dual_farkas_row_ = p;
    }
    last_result.certified = ok ? 1 : 0;
    last_result.certify_seconds = now_seconds() - t0;
    if (result) *result = last_result;
    if (!ok) last_error = message;
}

// The lower bound of a child the dual loop left at the cutoff or at its iteration limit, proved: every basis of that loop is dual feasible
// in f64, and one transposed lifting of B'y = c_B says whether this one is in exact arithmetic (certify.hpp: certify_dual_bound).  The
// basis is the one the device holds, as certify_dual_infeasible takes it; nothing is launched on the pivot state.
void Solver::certify_dual_lower_bound(relp_result* result) {
    const double t0 = now_seconds();
    bool ok = false;
    std::string message;
    std::vector<int> basis(d_.m);
    for (int i = 0; i < d_.m; ++i) basis[i] = cols_.to_provider(h_rb_basis_[i]);  // (collect_result's read-back)
    const bool at_cutoff = last_result.kind == RELP_RESULT_CUTOFF;
    try {
        certify_dual_bound(form_, basis, path_.bounded, at_cutoff, dual_cutoff_read_, opt_.device, stream_, &exact_objective, &ok, &message, &certify_scratch_,
                           &exact_witnesses);
    } catch (const RatOverflow& e) {  // (as certify())
        ok = false;
        message = std::string("exact certificate: ") + e.what();
    }
    dual_bound_proved_ = ok;
    last_result.certified = ok ? 1 : 0;
    last_result.certify_seconds = now_seconds() - t0;
    if (result) *result = last_result;
    if (!ok) last_error = message;
}

// ---- LU carry ---------------------------------------------------------------------------------------
// `BasisInverse::identity` (lower_upper/mod.rs:67-76) for the start of phase one.
// A factorisation on its way on the second stream is given up (its basis is superseded): the handle's stream waits for it before the
// snapshot buffers and the other set of factor arrays are written again -- the next start_async_refactor would otherwise copy a new
// basis into d_basis_snapshot_ while the abandoned kernels still read the old one (advisor, round 5).
void Solver::abandon_async_flight() {
    if (async_in_flight_) RELP_HIP(hipStreamWaitEvent(stream_, ev_refactored_, 0));
    async_in_flight_ = false;
}
void Solver::lu_identity() {
    abandon_async_flight();
    const int m = d_.m;
    HostLU f;
    f.m = m;
    f.rowpos.resize(m);
    f.colpos.resize(m);
    for (int i = 0; i < m; ++i) f.rowpos[i] = f.colpos[i] = i;
    f.l_start.assign(m + 1, 0);
    f.u_start.assign(m + 1, 0);
    f.diag.assign(m, 1.0);
    // (device refactorisation: every array sized by bounds first, so that the layout -- and the captured graphs -- stay put)
    if (path_.device_refactor && lu().prepare_device(m, path_.refactor_period + 1, true, (size_t)host_.col_start.back())) destroy_graphs();
    if (lu().upload(f, path_.refactor_period + 1, stream_, path_.lu_inverse)) destroy_graphs();  // the captured batches hold the old addresses
}
// `BasisInverse::invert(basis columns)` (lower_upper/mod.rs:78-92; called by `Carry::change_basis` when `should_refactor`,
// carry/mod.rs:584-591): Markowitz factorisation of the current basis on the host, one upload, and -- `refresh_vectors` -- x_B,
// -pi and the objective recomputed from the fresh factors (what the explicit carry's polish does too).
void Solver::refactor_lu(bool refresh_vectors, bool settle) {
    abandon_async_flight();  // (factors on their way on the other stream belong to a basis this call supersedes: never swapped in)
    if (!path_.device_refactor) {
        refactor_lu_host(refresh_vectors);
        return;
    }
    // Round 4: factorisation, inversion of the two triangles and the slot records are kernels on this handle's stream -- no basis
    // read-back, no upload, the host only enqueues (its time below is launch overhead).  What the kernels cannot take comes back
    // as ST_REFACTOR_FAILED at the next read of the control block (read_ctl: host fallback).
    const double t0 = now_seconds();
    LuFactorSource src;
    src.col_start = d_.col_start;
    src.row_index = d_.row_index;
    src.value = d_.value;
    src.basis = d_.basis;
    src.flipped = path_.bounded ? d_.flipped : nullptr;
    const double threshold = opt_.lu_pivot_threshold > 0.0 ? opt_.lu_pivot_threshold : 0.1;
    // (dense tail: the last rows through a dense LU out of LDS.  It saves the factorisation its slowest rounds but makes the ends of both
    //  triangles dense, and the INVERTED triangles pay for that -- more entries per product and a serial chain in the inversion)
    const int dense_tail = opt_.luf_dense_tail > 0 ? opt_.luf_dense_tail : (opt_.luf_dense_tail < 0 ? 0 : 8);
    lu().refactor_device(src, threshold, 0, dense_tail, d_.ctl, ST_REFACTOR_FAILED, stream_);
    binv_identity_ = false;
    if (refresh_vectors) {
        launch_lu_xb(d_, lu().device(), stream_);
        launch_lu_pi(d_, lu().device(), stream_);
    }
    launch_clear_refactor_status(d_, stream_);
    refactors_++;
    since_polish_ = 0;
    refactor_seconds_ += now_seconds() - t0;
    // Kernels that gave up leave ST_REFACTOR_FAILED in the control block and half-written factors behind.  The pivot loop reads the block
    // after its next batch (whose kernels do nothing under that status); every other caller hands control back to code that may read x_B,
    // -pi or solve with the factors directly, so the host fallback of read_ctl runs before it does.
    if (settle) read_ctl();
}
// Round 5: `BasisInverse::invert` beside the pivots.  The basis is copied as it stands (stream-ordered behind the pivots made so
// far), the pivot kernel starts logging the row factors of its etas, and the factorisation kernels run on a second stream into
// the OTHER set of factor arrays, on other compute units than the one-workgroup pivot kernel.
void Solver::start_async_refactor(long long iters_now) {
    const int m = d_.m;
    LuFactors& next = lu_sets_[lu_cur_ ^ 1];
    if (!refactor_stream_) {
        RELP_HIP(hipStreamCreateWithFlags(&refactor_stream_, hipStreamNonBlocking));
        RELP_HIP(hipEventCreateWithFlags(&ev_snapshot_, hipEventDisableTiming));
        RELP_HIP(hipEventCreateWithFlags(&ev_refactored_, hipEventDisableTiming));
        RELP_HIP(hipMalloc(&d_basis_snapshot_, (size_t)m * sizeof(int)));
        RELP_HIP(hipMalloc(&d_probe_, ((size_t)2 * m + 2) * sizeof(double)));  // the guard's probe v, B^-1 v and the residual
        launch_lu_probe_fill(d_probe_, m, stream_);
        if (path_.bounded) RELP_HIP(hipMalloc(&d_flipped_snapshot_, (size_t)d_.n * sizeof(*d_.flipped)));
    }
    if (!next.device_prepared()) next.prepare_device(m, path_.refactor_period + 1, true, (size_t)host_.col_start.back());
    RELP_HIP(hipMemcpyAsync(d_basis_snapshot_, d_.basis, (size_t)m * sizeof(int), hipMemcpyDeviceToDevice, stream_));
    if (path_.bounded) RELP_HIP(hipMemcpyAsync(d_flipped_snapshot_, d_.flipped, (size_t)d_.n * sizeof(*d_.flipped), hipMemcpyDeviceToDevice, stream_));
    lu().start_log(stream_);
    RELP_HIP(hipEventRecord(ev_snapshot_, stream_));
    RELP_HIP(hipStreamWaitEvent(refactor_stream_, ev_snapshot_, 0));
    LuFactorSource src;
    src.col_start = d_.col_start;
    src.row_index = d_.row_index;
    src.value = d_.value;
    src.basis = d_basis_snapshot_;
    src.flipped = path_.bounded ? reinterpret_cast<decltype(src.flipped)>(d_flipped_snapshot_) : nullptr;
    const double threshold = opt_.lu_pivot_threshold > 0.0 ? opt_.lu_pivot_threshold : 0.1;
    const int dense_tail = opt_.luf_dense_tail > 0 ? opt_.luf_dense_tail : (opt_.luf_dense_tail < 0 ? 0 : 8);
    next.refactor_device(src, threshold, 0, dense_tail, nullptr, ST_REFACTOR_FAILED, refactor_stream_);  // (a failure stays in its info words)
    RELP_HIP(hipEventRecord(ev_refactored_, refactor_stream_));
    async_in_flight_ = true;
    async_iters_at_snapshot_ = iters_now;
    if (diagnostic("RELP_TIME_REFACTOR")) fprintf(stderr, "[async] snapshot at iteration %lld, %lld updates since the last factors, set %d -> %d\n", iters_now, since_polish_, lu_cur_, lu_cur_ ^ 1);
}
// The new factors are ready (or are waited for): replay the logged etas onto them and swap sets.  false: they cannot be used (the
// kernels gave up, or more pivots were made than the log holds) -- the handle stays on the old factors and the caller takes the
// synchronous path when the device asks for a refactorisation.
bool Solver::finish_async_refactor(long long iters_now) {
    const double t0 = now_seconds();
    async_in_flight_ = false;
    LuFactors& next = lu_sets_[lu_cur_ ^ 1];
    RELP_HIP(hipStreamWaitEvent(stream_, ev_refactored_, 0));
    int info[LUF_INFO_WORDS];
    int state[LU_STATE_WORDS];
    RELP_HIP(hipMemcpyAsync(info, next.device_info(), sizeof(info), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipMemcpyAsync(state, lu().device().state, sizeof(state), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
    const long long made = iters_now - async_iters_at_snapshot_;
    if (diagnostic("RELP_TIME_REFACTOR")) {
        fprintf(stderr, "[async] ready: status %d, pivots since the snapshot %lld, logged %d, updates on the old factors %d (kept columns %d), iters %lld\n", info[LUF_STATUS], made,
                state[LU_LOG_COUNT], state[LU_N_UPDATES], state[LU_PF_COUNT], iters_now);
    }
    // (every basis change since the snapshot must be in the log: the count the kernels kept says so, the iteration counter is a
    //  cross-check -- bound flips make iterations without basis changes)
    if (info[LUF_STATUS] != LUF_OK || state[LU_LOG_COUNT] > LU_LOG_CAPACITY || state[LU_LOG_COUNT] > made) {
        ++async_abandoned_;
        if (info[LUF_STATUS] != LUF_OK) ++device_refactor_failures_;
        return false;
    }
    next.replay_log_of(lu(), stream_);
    // the guard (see lu_basis_residual_kernel): x = B^-1 v through the new factors and the replayed etas, |B x - v| over the basis now
    launch_lu_ftran_dense(next.device(), d_probe_, d_probe_ + d_.m, stream_);
    launch_lu_basis_residual(d_.col_start, d_.row_index, d_.value, d_.basis, path_.bounded ? d_.flipped : nullptr, d_probe_ + d_.m, d_probe_, d_.m, d_probe_ + 2 * (size_t)d_.m, stream_);
    double residual = 0.0;
    RELP_HIP(hipMemcpyAsync(&residual, d_probe_ + 2 * (size_t)d_.m, sizeof(double), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
    async_worst_residual_ = std::max(async_worst_residual_, residual);
    if (diagnostic("RELP_TIME_REFACTOR")) fprintf(stderr, "[async] |B (B^-1 v) - v| through the new factors + %d replayed etas: %.3e\n", state[LU_LOG_COUNT], residual);
    if (!(residual <= 1e-8)) {  // (the chain of swaps has drifted: this cycle ends with a factorisation of the basis as it is)
        ++async_abandoned_;
        return false;
    }
    lu_cur_ ^= 1;
    launch_lu_xb(d_, lu().device(), stream_);
    launch_lu_pi(d_, lu().device(), stream_);
    binv_identity_ = false;
    refactors_++;
    async_refactors_++;
    since_polish_ = state[LU_LOG_COUNT];
    refactor_seconds_ += now_seconds() - t0;
    return true;
}
void Solver::refactor_lu_host(bool refresh_vectors) {
    abandon_async_flight();
    const double t0 = now_seconds();
    const int m = d_.m;
    std::vector<int> basis(m);
    RELP_HIP(hipMemcpyAsync(basis.data(), d_.basis, m * sizeof(int), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
    std::vector<int> cs(m + 1, 0);
    size_t total = 0;
    for (int k = 0; k < m; ++k) {
        if (basis[k] < 0 || basis[k] >= d_.n) throw std::runtime_error("the device returned an invalid basis");
        total += (size_t)(host_.col_start[basis[k] + 1] - host_.col_start[basis[k]]);
        cs[k + 1] = (int)total;
    }
    std::vector<int> rows(total);
    std::vector<double> vals(total);
    std::vector<int> flipped;
    if (path_.bounded) {  // implicit bounds: a complemented column sits in the basis with the opposite sign
        flipped.resize(d_.n);
        RELP_HIP(hipMemcpyAsync(flipped.data(), d_.flipped, d_.n * sizeof(int), hipMemcpyDeviceToHost, stream_));
        RELP_HIP(hipStreamSynchronize(stream_));
    }
    for (int k = 0; k < m; ++k) {
        const int a = host_.col_start[basis[k]], len = host_.col_start[basis[k] + 1] - a;
        std::copy(host_.row_index.begin() + a, host_.row_index.begin() + a + len, rows.begin() + cs[k]);
        std::copy(host_.value.begin() + a, host_.value.begin() + a + len, vals.begin() + cs[k]);
        if (path_.bounded && flipped[basis[k]])
            for (int e = cs[k]; e < cs[k] + len; ++e) vals[e] = -vals[e];
    }
    LuOptions lo;
    lo.threshold = opt_.lu_pivot_threshold > 0.0 ? opt_.lu_pivot_threshold : 0.1;
    static const bool time_parts = diagnostic("RELP_TIME_REFACTOR");
    thread_local double part_seconds[3] = {0.0, 0.0, 0.0};
    const double t1 = now_seconds();
    HostLU f = lu_factor(m, cs.data(), rows.data(), vals.data(), lo);
    if (f.singular) throw std::runtime_error("singular basis in the LU refactorisation");
    const double t2 = now_seconds();
    if (lu().upload(f, path_.refactor_period + 1, stream_, path_.lu_inverse)) destroy_graphs();
    if (time_parts) {
        part_seconds[0] += t1 - t0;
        part_seconds[1] += t2 - t1;
        part_seconds[2] += now_seconds() - t2;
        if ((refactors_ + 1) % 25 == 0)
            fprintf(stderr, "[refactor] %lld so far: basis fetch + gather %.2f ms, Markowitz LU %.2f ms, schedules + upload %.2f ms (sums)\n", refactors_ + 1,
                    part_seconds[0] * 1e3, part_seconds[1] * 1e3, part_seconds[2] * 1e3);
    }
    binv_identity_ = false;
    if (refresh_vectors) {
        launch_lu_xb(d_, lu().device(), stream_);
        launch_lu_pi(d_, lu().device(), stream_);  // also rewrites minus_obj from the refreshed x_B
    }
    // status: REFACTOR -> RUNNING, stream-ordered (no host round trip: the refresh kernels above are still running; whoever reads
    // the control block next synchronises anyway).  A refactorisation is only ever asked for in the RUNNING state.
    launch_clear_refactor_status(d_, stream_);
    refactors_++;
    since_polish_ = 0;
    refactor_seconds_ += now_seconds() - t0;
    if (opt_.verbose > 1)
        fprintf(stderr, "[lu] refactor %lld: nnz(L) %lld nnz(U) %lld depth %d + %d\n", refactors_, lu().nnz_l, lu().nnz_u, lu().depth_l, lu().depth_u);
}

// ---- fine-grained ops -------------------------------------------------------------------------------
void Solver::ftran(int nnz, const int* rows, const double* values, double* out) {
    int* d_rows = reinterpret_cast<int*>(d_.scratch);
    double* d_vals = d_.scratch + (d_.m + 1) / 2 + 1;
    double* d_out = d_vals + d_.m;
    check_sparse(nnz, rows, values, d_.m);
    RELP_HIP(hipSetDevice(opt_.device));
    if (path_.network) {
        std::vector<double> v(d_.m, 0.0);
        for (int e = 0; e < nnz; ++e) v[rows[e]] += values[e];
        const std::vector<double> x = net_host_solve(net_download(), false, v);
        std::copy(x.begin(), x.end(), out);
        return;
    }
    RELP_HIP(hipMemcpyAsync(d_rows, rows, nnz * sizeof(int), hipMemcpyHostToDevice, stream_));
    RELP_HIP(hipMemcpyAsync(d_vals, values, nnz * sizeof(double), hipMemcpyHostToDevice, stream_));
    if (path_.lu_mode) launch_lu_ftran(lu().device(), d_rows, d_vals, nnz, d_out, 0, stream_);
    else launch_ftran_vec(d_, d_rows, d_vals, nnz, d_out, stream_);
    RELP_HIP(hipMemcpyAsync(out, d_out, d_.m * sizeof(double), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
}
void Solver::btran(int nnz, const int* rows, const double* values, double* out) {
    int* d_rows = reinterpret_cast<int*>(d_.scratch);
    double* d_vals = d_.scratch + (d_.m + 1) / 2 + 1;
    double* d_out = d_vals + d_.m;
    check_sparse(nnz, rows, values, d_.m);
    RELP_HIP(hipSetDevice(opt_.device));
    if (path_.network) {
        std::vector<double> v(d_.m, 0.0);
        for (int e = 0; e < nnz; ++e) v[rows[e]] += values[e];
        const std::vector<double> x = net_host_solve(net_download(), true, v);
        std::copy(x.begin(), x.end(), out);
        return;
    }
    RELP_HIP(hipMemcpyAsync(d_rows, rows, nnz * sizeof(int), hipMemcpyHostToDevice, stream_));
    RELP_HIP(hipMemcpyAsync(d_vals, values, nnz * sizeof(double), hipMemcpyHostToDevice, stream_));
    if (path_.lu_mode) launch_lu_btran(lu().device(), d_rows, d_vals, nnz, d_out, stream_);
    else launch_btran_vec(d_, d_rows, d_vals, nnz, d_out, stream_);
    RELP_HIP(hipMemcpyAsync(out, d_out, d_.m * sizeof(double), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
}
void Solver::inverse_row(int row, double* out) {
    if (row < 0 || row >= d_.m) throw std::invalid_argument("row out of range");
    const double one = 1.0;
    btran(1, &row, &one, out);  // e_row' Binv: a strided read of the column-major inverse
}
void Solver::relative_costs(double* out) {
    if (phase_ == 0) throw std::runtime_error("no phase started");
    RELP_HIP(hipSetDevice(opt_.device));
    launch_relative_cost(d_, d_.scratch, stream_);
    RELP_HIP(hipMemcpyAsync(out, d_.scratch, d_.n * sizeof(double), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
}
void Solver::get_gamma(double* out) {
    RELP_HIP(hipSetDevice(opt_.device));
    // apply a pending weight update first so that the values are those the next pricing pass would use
    std::vector<int> pos(d_.n);
    RELP_HIP(hipMemcpyAsync(out, d_.gamma, d_.n * sizeof(double), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipMemcpyAsync(pos.data(), d_.pos, d_.n * sizeof(int), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
    for (int j = 0; j < d_.n; ++j)
        if (j < d_.n_art || pos[j] >= 0) out[j] = std::numeric_limits<double>::quiet_NaN();
}
// `PivotRule::select_primal_pivot_column`: the pricing kernel, then the entering-column reduction of the fused kernel
// (mode 1: stop after the choice).  Applies a pending steepest-edge update exactly like the device loop does.
void Solver::price(int* column, double* cbar) {
    if (phase_ == 0) throw std::runtime_error("no phase started");
    RELP_HIP(hipSetDevice(opt_.device));
    Ctl c = read_ctl();
    const int saved = c.status;
    c.status = ST_RUNNING;
    c.forced_q = c.forced_p = -1;
    write_ctl(c);
    enqueue_price(0);
    if (path_.lu_mode) enqueue_ftran_ratio(1);
    else launch_ftran_ratio(d_, path_, opt_.pivot_rule, opt_.tol_pivot, ratio_delta(), phase_ == 2 ? 1 : 0, 1, 0, stream_);
    c = read_ctl();
    *column = c.q;
    *cbar = c.q >= 0 ? c.cbar_q : 0.0;
    c.status = saved;
    write_ctl(c);
}
// `Tableau::generate_column` + `select_primal_pivot_row` without a basis change: the fused kernel in mode 2.
void Solver::ratio(int column, int* row, double* alpha_out) {
    if (phase_ == 0) throw std::runtime_error("no phase started");
    RELP_HIP(hipSetDevice(opt_.device));
    if (column < 0 || column >= d_.n) throw std::invalid_argument("column out of range");
    Ctl c = read_ctl();
    const Ctl before = c;  // a pending steepest-edge update still needs q, gamma_q, alpha_pq, leaving of the LAST pivot
    const int saved = c.status;
    const int saved_pending = c.pending;
    c.status = ST_RUNNING;
    c.forced_q = column;
    c.forced_p = -1;
    // the multi-block FTRAN (ftran_partial_kernel) has no mode: it computes nothing once the budget of the last batch is used up,
    // and the ratio test would then read the alpha of an earlier column
    if (path_.ftran_slices > 0) c.budget = c.iters + 1;
    write_ctl(c);
    enqueue_ftran_ratio(2);
    c = read_ctl();
    c.budget = before.budget;
    *row = c.p;
    if (alpha_out) {
        RELP_HIP(hipMemcpyAsync(alpha_out, d_.alpha, d_.m * sizeof(double), hipMemcpyDeviceToHost, stream_));
        RELP_HIP(hipStreamSynchronize(stream_));
    }
    c.status = saved;
    c.pending = saved_pending;
    c.q = before.q;
    c.p = before.p;
    c.leaving = before.leaving;
    c.cbar_q = before.cbar_q;
    c.alpha_pq = before.alpha_pq;
    c.gamma_q = before.gamma_q;
    c.forced_q = c.forced_p = -1;
    write_ctl(c);
}
void Solver::solve_exact(int first_limbs, int max_limbs, long long max_pivots, int trace_capacity, int* status, int* limbs, long long* p1,
                         long long* p2, std::vector<int>* trace, std::string* objective, std::vector<int>* basis,
                         std::vector<std::pair<int, long long>>* survived, int* redundant_rows) {
    if (!loaded_) throw std::runtime_error("no LP loaded");
    const long long cap = max_pivots > 0 ? max_pivots : 200LL * (d_.m + d_.n) + 100000;
    exact_simplex(form_, opt_.device, stream_, first_limbs, max_limbs, cap, trace_capacity, status, limbs, p1, p2, trace, objective, basis, survived,
                  redundant_rows, &exact_records_, opt_.exact_update, opt_.exact_grid);
}
void Solver::last_pivot(int* phase, int* column, int* row, int* leaving) {
    const Ctl c = read_ctl();
    const bool any = c.iters > 0 && c.p >= 0;
    *phase = last_pivot_dual_ ? 3 : phase_;
    *column = any ? c.q : -1;
    *row = any ? c.p : -1;
    *leaving = any ? c.leaving : -1;
}
// `PivotRule::after_basis_update` (strategy/pivot_rule.rs:243-296): the Goldfarb-Reid update of the steepest-edge weights for
// the last basis change.  Inside the device loop it rides on the next pricing pass; a caller that drives the loop itself can
// ask for it here (one pass over the non-basic columns, candidates discarded).  No-op when nothing is pending.
void Solver::after_basis_update() {
    if (phase_ == 0) throw std::runtime_error("no phase started");
    RELP_HIP(hipSetDevice(opt_.device));
    Ctl c = read_ctl();
    if (!c.pending) return;
    const int saved = c.status;
    c.status = ST_RUNNING;
    write_ctl(c);
    enqueue_price(0);
    c = read_ctl();
    c.pending = 0;
    c.status = saved;
    write_ctl(c);
}
// `Tableau::bring_into_basis(pivot_column, pivot_row, column)` (tableau/mod.rs:139-160) with both indices given by the
// caller: one iteration of the device loop whose pricing and ratio test are overridden (the steepest-edge weights, b,
// -pi, the objective and the inverse are updated as in any other pivot).  Same index space as `price` / `ratio`.
void Solver::bring_into_basis(int column, int row) {
    if (phase_ == 0) throw std::runtime_error("no phase started");
    if (column < 0 || column >= d_.n) throw std::invalid_argument("column out of range");
    if (row < 0 || row >= d_.m) throw std::invalid_argument("row out of range");
    Ctl c = read_ctl();
    const long long before = c.iters;
    c.status = ST_RUNNING;
    c.forced_q = column;
    c.forced_p = row;
    write_ctl(c);
    launch_pivots(1, true);
    c = read_ctl();
    if (c.iters == before) throw std::runtime_error("bring_into_basis: the pivot element is zero (or the column is basic)");
    pivots_[phase_ - 1] += 1;
    since_polish_ += 1;
    binv_identity_ = false;
    last_pivot_dual_ = false;
    dual_weights_current_ = false;
    if (c.status == ST_REFACTOR) refactor_lu(true);  // LU carry: `should_refactor` was true for this pivot
}
// `BasisInverse::should_refactor` + `invert` (lower_upper/mod.rs:78-92, 249-252) on demand: the Newton-Schulz polish of the
// resident inverse, with b, -pi and the objective recomputed from it.  Returns the residual max|I - B'T| found before.
double Solver::refactor() {
    if (phase_ == 0) throw std::runtime_error("no phase started");
    const double before = max_residual_;
    max_residual_ = 0.0;
    polish(true, true);
    const double found = max_residual_;
    max_residual_ = std::max(before, found);
    return found;
}
// Average execution time of one launch of a hot-loop kernel INSIDE the real pivot sequence (bench.py's roofline leg):
// `repetitions` further pivots of the current phase are run un-graphed, and the chosen kernel of every pivot is
// bracketed by its own start/stop event pair (hipExtLaunchKernelGGL) on this handle's stream.  The solve advances.
double Solver::profile_kernel(int which, int repetitions) {
    if (phase_ == 0) throw std::runtime_error("no phase started");
    if (path_.lu_mode && which == 2) throw std::invalid_argument("the LU carry has no separate update kernel (which = 1 covers it)");
    if (path_.fused && which == 2) throw std::invalid_argument("the update is part of kernel 1 (fused pivot kernel): which = 1 covers it");
    RELP_HIP(hipSetDevice(opt_.device));
    const int m = d_.m;
    if (which == 0) {
        // algorithmic bytes of a pricing pass at this state: the columns that are non-basic now
        std::vector<int> pos(d_.n), cs(d_.n + 1);
        RELP_HIP(hipMemcpyAsync(pos.data(), d_.pos, d_.n * sizeof(int), hipMemcpyDeviceToHost, stream_));
        RELP_HIP(hipMemcpyAsync(cs.data(), d_.col_start, (d_.n + 1) * sizeof(int), hipMemcpyDeviceToHost, stream_));
        RELP_HIP(hipStreamSynchronize(stream_));
        long long bytes = 0;
        for (int j = d_.n_art; j < d_.n; ++j) {
            if (pos[j] >= 0) continue;
            if (d_.cost8) {  // generated incidence column: 8 B of endpoints, 1 B cost, 4 B position
                bytes += 13;
                continue;
            }
            const bool dense_col = j >= d_.dense_first && j < d_.dense_first + d_.n_dense;
            bytes += dense_col ? (long long)m * path_.dense_entry_bytes() : (long long)(cs[j + 1] - cs[j]) * 12;
            bytes += 24;  // cost, gamma read + gamma write
        }
        stats_.price_bytes = bytes;
    }
    std::vector<hipEvent_t> starts(repetitions), stops(repetitions);
    for (int k = 0; k < repetitions; ++k) {
        RELP_HIP(hipEventCreate(&starts[k]));
        RELP_HIP(hipEventCreate(&stops[k]));
    }
    Ctl before = read_ctl();
    if (path_.network) {  // (the forest's kernels are bracketed by events of their own: 0 pricing, 1 path + ratio test, 2 forest update)
        launch_budget(d_, repetitions, stream_);
        for (int k = 0; k < repetitions; ++k) {
            if (which == 0) RELP_HIP(hipEventRecord(starts[k], stream_));
            enqueue_price(0);
            if (which == 0) RELP_HIP(hipEventRecord(stops[k], stream_));
            if (which == 1) RELP_HIP(hipEventRecord(starts[k], stream_));
            net_enqueue_pivot(0, 1);
            if (which == 1) RELP_HIP(hipEventRecord(stops[k], stream_));
            if (which == 2) RELP_HIP(hipEventRecord(starts[k], stream_));
            net_enqueue_pivot(0, 2);
            if (which == 2) RELP_HIP(hipEventRecord(stops[k], stream_));
        }
    } else if (path_.fused) {
        launch_begin_batch(d_, repetitions, stream_);
        for (int k = 0; k < repetitions; ++k) {
            if (which == 0) arm_launch_timer(0, starts[k], stops[k]);
            enqueue_price_fused(k & 1);
            if (which == 1) arm_launch_timer(1, starts[k], stops[k]);
            enqueue_pivot_fused(k & 1);
        }
        launch_commit(d_, repetitions & 1, stream_);
    } else {
    launch_budget(d_, repetitions, stream_);
    for (int k = 0; k < repetitions; ++k) {
        if (which == 0) arm_launch_timer(0, starts[k], stops[k]);
        enqueue_price(0, k == 0);
        if (which == 1) arm_launch_timer(1, starts[k], stops[k]);
        enqueue_ftran_ratio(0);
        if (which == 2) arm_launch_timer(2, starts[k], stops[k]);
        if (!path_.lu_mode) enqueue_update();
        if (path_.eta_mode && ((k + 1) % d_.eta_cap == 0 || k + 1 == repetitions)) enqueue_consolidate();
    }
    }
    arm_launch_timer(-1, nullptr, nullptr);
    Ctl after = read_ctl();
    // K3's algorithmic bytes at the profiled state when unit columns are skipped: read + write of (non-zero rows of alpha) x
    // (columns of the stored inverse that carry information)
    if (d_.track_touched && !path_.eta_mode) stats_.update_bytes = 16LL * std::max(1, after.nz_count) * std::max(1, after.touched_count);
    if (after.status == ST_REFACTOR) refactor_lu(true);
    const long long made = after.iters - before.iters;
    pivots_[phase_ - 1] += made;
    since_polish_ += made;
    double total_ms = 0.0;
    int counted = 0;
    for (int k = 0; k < repetitions; ++k) {
        float ms = 0.f;
        if (k < made && hipEventElapsedTime(&ms, starts[k], stops[k]) == hipSuccess) {
            total_ms += ms;
            ++counted;
        }
        (void)hipEventDestroy(starts[k]);
        (void)hipEventDestroy(stops[k]);
    }
    if (counted == 0) throw std::runtime_error("no pivot was made while profiling (phase already finished)");
    return total_ms * 1e-3 / counted;
}

void Solver::debug_stamps(unsigned long long* out64) {
    RELP_HIP(hipMemcpyAsync(out64, d_.dbg, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
}

void Solver::get_b(double* out) {
    RELP_HIP(hipSetDevice(opt_.device));
    RELP_HIP(hipMemcpyAsync(out, d_.xB, d_.m * sizeof(double), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
}
double Solver::objective() { return -read_ctl().minus_obj; }
long long Solver::bound_flips() {
    if (!path_.bounded || phase_ == 0) return 0;
    RELP_HIP(hipSetDevice(opt_.device));
    return read_ctl().bound_flips;
}

void Solver::get_basis(int* out) {
    std::vector<int> basis(d_.m);
    RELP_HIP(hipMemcpyAsync(basis.data(), d_.basis, d_.m * sizeof(int), hipMemcpyDeviceToHost, stream_));
    RELP_HIP(hipStreamSynchronize(stream_));
    if (path_.bounded) {  // in the reference's formulation: one entry per row of MatrixData, bound rows included
        std::vector<int> pos(d_.n);
        RELP_HIP(hipMemcpyAsync(pos.data(), d_.pos, d_.n * sizeof(int), hipMemcpyDeviceToHost, stream_));
        RELP_HIP(hipStreamSynchronize(stream_));
        resolve_fixed_columns(pos);
        const std::vector<int> full = explicit_basis(basis, pos);
        std::copy(full.begin(), full.end(), out);
        return;
    }
    for (int i = 0; i < d_.m; ++i) out[i] = cols_.to_provider(basis[i]);
}
void Solver::get_solution(double* x) const {
    const int n_struct = form_.data.nr_normal_variables();
    for (int j = 0; j < n_struct; ++j) x[j] = h_solution_[j];
}

}  // namespace relp

