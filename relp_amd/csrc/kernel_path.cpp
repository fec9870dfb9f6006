// plan_kernel_path: every decision of a load, in the order in which they depend on each other (kernel_path.hpp).  Host-only.
#include "kernel_path.hpp"

#include <algorithm>
#include <cmath>
#include <sstream>
#include <stdexcept>

#include "device_columns.hpp"

namespace relp {

KernelPath plan_kernel_path(const relp_options& opt_, const MatrixData& md, const DeviceColumns& cols, const DeviceMatrix& a,
                            const std::vector<std::string>* column_names) {
    KernelPath p;
    // Implicit upper bounds: the device LP has the constraint rows only (E | R | <= | >=) and the provider columns of the
    // first four groups (structurals, range slacks, <= slacks, >= slacks); the VariableBound / SlackBound rows and their
    // slack columns (matrix_data.rs:104-145) become upper bounds of the structurals and the range slacks.
    p.bounded = implicit_bounds_apply(opt_, md);
    const bool want_f64_block = opt_.dense_storage == RELP_DENSE_DOUBLE;
    const bool want_f32_block = opt_.dense_storage == RELP_DENSE_FLOAT;
    const bool product_form_off = opt_.product_form == 1;
    const int ftran_min_nnz = opt_.ftran_min_nnz > 0 ? opt_.ftran_min_nnz : 1024;
    const auto sw = [&](unsigned bit) { return (opt_.switches & bit) != 0; };
    const int m = p.m = cols.m, n_p = p.n_p = cols.n_p;
    if (m < 1) throw std::runtime_error("LP without rows");
    const int n_art = p.n_art = cols.n_art, n = p.n = cols.n();
    const std::vector<int>&col_start = a.col_start, &row_index = a.row_index;
    const std::vector<double>&value = a.value, &cost2 = a.cost2;
    p.network = opt_.carry == RELP_CARRY_NETWORK;
    if (p.network) {  // a network LP: at most two entries per column, each +-1, of opposite signs when there are two
        for (int j = n_art; j < n; ++j) {
            const int first = col_start[j], len = col_start[j + 1] - first;
            bool fits = len <= 2;
            for (int e = first; fits && e < first + len; ++e) fits = value[e] == 1.0 || value[e] == -1.0;
            if (fits && len == 2) fits = value[first] == -value[first + 1];
            if (fits) continue;
            const int c = j - n_art;
            const std::string name = column_names && c < (int)column_names->size() ? (*column_names)[c] : "slack";
            std::string hint;
            if (!p.bounded && md.nr_variable_bounds() > 0) hint = "; its upper bound is a row of the device LP: set implicit_bounds = 1";
            throw std::invalid_argument("RELP_CARRY_NETWORK: column " + std::to_string(c) + " (" + name + ") is not a network column (" + std::to_string(len) +
                                        " entries; at most two, each +-1, of opposite signs)" + hint);
        }
    }
    p.lu_mode = opt_.carry == RELP_CARRY_LU || opt_.carry == RELP_CARRY_LU_INVERSE;
    p.lu_inverse = opt_.carry == RELP_CARRY_LU_INVERSE;
    // (default: the reference's `should_refactor`, > 30 updates, for its Forrest-Tomlin form; 47 for the inverse-factor form, whose
    //  kept columns cost less per update than its refactorisation per pivot: 25FV47 63 -> 59 us per pivot, CYCLE 87 -> 81)
    p.refactor_period = std::min(opt_.refactor_period > 0 ? opt_.refactor_period : (p.lu_inverse ? 47 : 31), LU_MAX_SLOTS - 1);  // T is solved by one wave
    // `BasisInverse::invert` as kernels (lu_factor.hip, lu_device_tasks.hip: the inverse-factor form) or on one host core:
    // relp_options.lu_refactor.  AUTO is the host path today -- faster at every size measured.
    {
        int where = opt_.lu_refactor;
        p.device_refactor = p.lu_inverse && (where == RELP_REFACTOR_DEVICE || where == RELP_REFACTOR_DEVICE_ASYNC) && m <= 65535;
        p.async_refactor = p.device_refactor && where == RELP_REFACTOR_DEVICE_ASYNC;  // (only with the four-vector layout: checked where it starts)
    }
    // (a refactorisation on the device costs about twice the host's, so its period is the longest the kept columns allow: 25FV47 64.8 us
    //  per pivot at 47, 60.3 at 63; GREENBEA 154.5 -> 142.3)
    if (p.device_refactor && opt_.refactor_period <= 0) p.refactor_period = LU_MAX_SLOTS - 1;
    if (p.lu_inverse && !lu_fits_lds(m, p.refactor_period + 1, true))
        throw std::invalid_argument("the inverse-factor carry keeps its vectors in LDS (32 bytes per row, 24 beyond ~4300 rows): at most about 5800 rows (use the LU or the explicit carry beyond)");
    if (p.lu_mode && !p.lu_inverse) {
        if (!lu_fits_lds(m, p.refactor_period + 1)) throw std::invalid_argument("the LU carry keeps its two solve vectors in LDS (16 bytes per row): at most about 8000 rows with this refactor period (use the explicit carry beyond)");
    }
    // dense block: the longest run of provider columns, starting at the first one, with nnz > m/2 (config 3: all
    // structural columns); steepest edge only (the dense kernel implements that rule)
    int n_dense = 0;
    if (opt_.pivot_rule == RELP_PIVOT_STEEPEST_EDGE && m >= 64)
        while (n_dense < n_p && (col_start[n_art + n_dense + 1] - col_start[n_art + n_dense]) * 2 > m) ++n_dense;
    if (n_dense < 64 || p.bounded || p.lu_mode || p.network) n_dense = 0;  // (the dense pipeline belongs to the explicit inverse)
    p.n_dense = n_dense;
    p.dense_ld = (m + 3) & ~3;
    p.sparse_first = n_art + n_dense;
    p.price_lds = (size_t)3 * m * sizeof(double);
    {   // graph LPs (at most two entries per column) beyond the LDS-resident size: width-2 padded copy, 4x less padding to stream
        int longest = 0;
        for (int j = 0; j < n; ++j) longest = std::max(longest, col_start[j + 1] - col_start[j]);
        p.ell_w = (longest <= 2 && n_dense == 0 && p.price_lds > 160 * 1024 - 1024 && !sw(RELP_SW_ELL_WIDE)) ? 2 : ELL_W;
    }
    // incidence columns (graph providers, examples/max_flow.rs:174-200): every value +-1 and small integer costs -- the
    // pricing pass then GENERATES the column from 8 bytes per arc (row | sign) instead of streaming 24 + 8 bytes of it
    bool unit = p.ell_w == 2 && !sw(RELP_SW_NO_GENERATED_COLUMNS);
    for (size_t e = 0; unit && e < value.size(); ++e) unit = value[e] == 1.0 || value[e] == -1.0;
    for (int j = 0; unit && j < n; ++j) unit = cost2[j] == std::floor(cost2[j]) && std::fabs(cost2[j]) <= 127.0;
    p.generated_columns = unit;
    const int cpb = price_columns_per_block(p.ell_w, unit);
    p.price_blocks = std::min(p.ell_w == 2 && !unit ? 2048 : 1024, (n - p.sparse_first + cpb - 1) / cpb);
    // (the multi-block FTRAN and the slack columns below: the longest provider column)
    int max_nnz = 0;
    for (int j = n_art; j < n; ++j) max_nnz = std::max(max_nnz, col_start[j + 1] - col_start[j]);
    // Dense pipeline whose sparse columns are one single-entry column per row at most (the slack columns of config 3): the BTRAN
    // pass of a pivot prices them for the next one (btran_pass_kernel), one candidate slot per workgroup of that pass.
    std::vector<int> slack_of_row;
    {
        bool eligible = n_dense > 0 && opt_.pivot_rule == RELP_PIVOT_STEEPEST_EDGE && m % 2 == 0 && m <= 4096 &&
                        !product_form_off && !sw(RELP_SW_NO_SLACK_IN_BTRAN) && n > p.sparse_first;
        if (eligible) eligible = max_nnz > ftran_min_nnz;  // (the deferred product form needs the multi-block FTRAN: a column longer than its threshold)
        if (eligible) {
            slack_of_row.assign(m, -1);
            for (int j = p.sparse_first; eligible && j < n; ++j) {
                eligible = col_start[j + 1] - col_start[j] == 1 && slack_of_row[row_index[col_start[j]]] < 0;
                if (eligible) slack_of_row[row_index[col_start[j]]] = j;
            }
        }
        if (!eligible) slack_of_row.clear();
        else p.price_blocks = btran_pass_blocks();
    }
    p.dense_blocks = n_dense > 0 ? std::min(opt_.dense_blocks > 0 ? opt_.dense_blocks : 256, (n_dense + 15) / 16) : 0;  // 16 waves per workgroup, one workgroup per CU (96 KB of LDS each)
    bool dense_bytes = n_dense > 0 && !want_f64_block && !want_f32_block;  // narrowest exact storage type
    for (int jd = 0; dense_bytes && jd < n_dense; ++jd)
        for (int e = col_start[n_art + jd]; dense_bytes && e < col_start[n_art + jd + 1]; ++e)
            dense_bytes = value[e] >= -128.0 && value[e] <= 127.0 && value[e] == std::floor(value[e]);
    {
        bool full = n_dense > 0;
        for (int jd = 0; full && jd < n_dense; ++jd) {
            full = col_start[n_art + jd + 1] - col_start[n_art + jd] == m;
            for (int e = col_start[n_art + jd], i = 0; full && i < m; ++e, ++i) full = row_index[e] == i;
        }
        p.dense_full = full;
        p.dense_csc_start = n_dense > 0 ? col_start[n_art] : 0;
    }
    bool dense_floats = n_dense > 0 && !dense_bytes && !want_f64_block;  // float holds every entry exactly
    for (int jd = 0; dense_floats && jd < n_dense; ++jd)
        for (int e = col_start[n_art + jd]; dense_floats && e < col_start[n_art + jd + 1]; ++e) dense_floats = (double)(float)value[e] == value[e];
    p.vector_len = m;
    if (n_dense > 0 && dense_lane_slots(n_dense) <= 1024 && !sw(RELP_SW_NO_DENSE_LANE)) {
        // column-per-lane pricing: one workgroup and one candidate slot per group of 16 columns
        p.dense_lane = true;
        p.dense_ld = dense_lane_ld(m);
        p.dense_blocks = dense_lane_slots(n_dense);
        p.vector_len = p.dense_ld;
    }
    if (p.price_blocks + p.dense_blocks == 0) p.price_blocks = 1;
    // columns longer than this take the multi-block FTRAN pipeline (relp_options.ftran_min_nnz: test hook to exercise it on small LPs)
    const bool fast_k2 = fast_k2_available(m, p.slots());
    if (max_nnz > ftran_min_nnz && fast_k2) p.ftran_slices = opt_.ftran_slices > 0 ? opt_.ftran_slices : std::min(64, (max_nnz + 255) / 256);  // (4096 x 8192: 8 / 16 / 32 / 64 slices = 20.8k / 21.2k / 20.8k / 19.7k pivots/s)
    // deferred product form of the inverse: the dense pipeline (multi-block FTRAN), m even and <= 4096 (alpha_reduce_kernel, btran_pass_kernel)
    // (relp_options.product_form = 1 keeps the per-pivot rank-one update: A/B measurements)
    p.eta_mode = n_dense > 0 && p.ftran_slices > 0 && m % 2 == 0 && m <= 4096 && !product_form_off;
    p.eta_cap = p.eta_mode ? eta_max() : 0;
    p.slack_in_btran = p.eta_mode && !slack_of_row.empty();
    if (p.slack_in_btran) p.slack_of_row = std::move(slack_of_row);
    // unit columns of the inverse are tracked where skipping them pays: the dense pipeline and the larger sparse LPs
    // (below that the update kernel is latency bound and the extra indirection would cost a round trip)
    p.track_touched = (p.eta_mode || m > 2048) && !p.lu_mode && !p.network && !sw(RELP_SW_NO_TOUCHED);
    // The dense block's storage.  The row-permuted byte form keeps the padded vectors in LDS: beyond that the block goes to the
    // plain forms, whose float test looks at the padded block (its zeros are exact) and honours RELP_DENSE_DOUBLE only -- a block
    // that qualified as bytes did not have its floats scanned above.
    if (n_dense > 0) {
        const bool permuted_fits = !((size_t)3 * ((m + 1023) & ~1023) * sizeof(double) > 160 * 1024 - 4096);
        if (p.dense_lane) p.dense_storage = dense_bytes ? DenseStorage::I8_LANE : dense_floats ? DenseStorage::F32_LANE : DenseStorage::F64_LANE;
        else if (dense_bytes && permuted_fits) {
            p.dense_storage = DenseStorage::I8_PERMUTED;
            p.dense_ld = (m + 1023) & ~1023;
        } else {
            bool exact_in_float = !want_f64_block;  // relp_options.dense_storage = RELP_DENSE_DOUBLE keeps the f64 block
            for (int jd = 0; exact_in_float && jd < n_dense; ++jd)
                for (int e = col_start[n_art + jd]; exact_in_float && e < col_start[n_art + jd + 1]; ++e) exact_in_float = (double)(float)value[e] == value[e];
            p.dense_storage = exact_in_float ? DenseStorage::F32_ROWS : DenseStorage::F64_ROWS;
        }
    }
    // The ratio test: rows in registers where they fit (the smallest R with m <= R * K2F_THREADS), beyond that across workgroups for
    // a full iteration (RELP_SW_K2_SINGLE: A/B; the forest carry has no other form there) and in one workgroup for the calls that
    // make no basis change.
    p.ratio_kernel_no_change = !fast_k2 ? RatioKernel::ONE_WORKGROUP
                               : m <= 2 * K2F_THREADS ? RatioKernel::REGISTERS_2
                               : m <= 4 * K2F_THREADS ? RatioKernel::REGISTERS_4
                               : m <= 8 * K2F_THREADS ? RatioKernel::REGISTERS_8
                                                      : RatioKernel::REGISTERS_16;
    p.ratio_kernel = !fast_k2 && (!sw(RELP_SW_K2_SINGLE) || p.network) ? RatioKernel::MULTI_WORKGROUP : p.ratio_kernel_no_change;  // m > 8192
    p.multi_workgroup_ratio = p.ratio_kernel == RatioKernel::MULTI_WORKGROUP;
    // The reference's ratio rule is implemented by the register-resident ratio test (m <= 8192), the fused pivot kernel and the LU
    // pivot kernel; the multi-workgroup test beyond 8192 rows and the one-workgroup fallback implement the two-pass rule only.
    {
        // (the forest carry has the reference's rule at every size: alpha is +-1 on its path, see net_enqueue_pivot)
        const bool kernels_have_it = p.lu_mode || p.network || fast_k2;
        if (opt_.ratio_rule == RELP_RATIO_TEXTBOOK && !kernels_have_it)
            throw std::invalid_argument("RELP_RATIO_TEXTBOOK: the reference's ratio test is implemented up to 8192 rows (the multi-workgroup ratio test has the two-pass rule only)");
        p.ratio_textbook = resolves_to_textbook(opt_, a, kernels_have_it);
    }
    // small LPs: ratio test and inverse update in one launch (pivot_fused_kernel; relp_options.pivot_kernels = 1 keeps the three-kernel pivot)
    p.fused = !p.lu_mode && !p.network && !p.bounded && !p.eta_mode && n_dense == 0 && p.ftran_slices == 0 && !p.track_touched && p.ell_w == ELL_W &&
              fused_pivot_available(m, p.price_blocks) && opt_.pivot_kernels != 1;
    p.fused_rows = !p.fused ? 0 : m <= 2 * K2F_THREADS ? 2 : KF_MAX_R;
    if (p.generated_columns) {  // -pi from its own vector, rho_p's non-zero rows as bits (bytes beyond LDS)
        p.price_unit_pairs = sw(RELP_SW_PRICE_UNIT_PAIRS);
        p.rho_words = ((m + 127) / 128) * 4;
        if ((size_t)p.rho_words * 4 > 64 * 1024 || sw(RELP_SW_NO_RHO_BITS) || p.price_unit_pairs) p.rho_words = 0;
    }
    // The CSC pricing kernel.  At width 8 it stages -pi, rho_p and w in LDS (3 m doubles per workgroup) where that pays.  Not beside a
    // dense block: the CSC kernel then only sees the short slack columns, and staging would cost more than the gathers it saves.
    // (Running it on a second stream beside the dense pass was measured too: the fork/join edges of the captured graph cost 15 us per
    // pivot against the 8 us they hide.)  Not beyond 4096 rows (96 KB): a workgroup prices 32 columns and would stage 3 m doubles for
    // them, one workgroup per CU (80BAU3B, m = 5746: 486 workgroups x 138 KB = 67 MB of staging against 1.5 MB of gathers; 53.8 ->
    // 45.7 us per pivot without).  Between 2000 and 2800 rows the two forms are within the run-to-run noise (BNL2, CYCLE, GREENBEA).
    // relp_options.price_lds_max: A/B hook.  The fused pivot's batches stage whatever the CU holds.
    const auto price_kernel = [&](bool stage_in_lds) {
        if (p.ell_w == 2 && p.generated_columns && p.price_unit_pairs) return PriceKernel::UNIT_PAIRS;
        if (p.ell_w == 2 && p.generated_columns) return PriceKernel::GENERATED;
        if (p.ell_w == 2) return PriceKernel::WIDTH_2;
        return stage_in_lds ? PriceKernel::LDS : PriceKernel::GATHER;
    };
    const size_t lds_max = opt_.price_lds_max > 0 ? (size_t)opt_.price_lds_max : (size_t)96 * 1024;
    p.price_kernel = price_kernel(p.price_lds <= lds_max && p.dense_blocks == 0);
    p.price_kernel_fused = price_kernel(p.price_lds <= PRICE_LDS_CONFIGURED);
    // The rank-one update of the explicit inverse.  Up to 2048 rows it is latency bound and reads whole columns; beyond, its loads
    // are predicated on alpha_i != 0, and a full sweep runs one workgroup per column pair where the touched columns are listed (the
    // list-driven modes use the first quarter of that grid; beyond 16384 rows they dominate -- graph LPs -- and 4x the workgroups
    // only cost launch time).
    p.update_kernel = m <= 2048 ? UpdateKernel::EAGER : (p.track_touched && m <= 16384) ? UpdateKernel::PREDICATED_SPLIT_GRID : UpdateKernel::PREDICATED;
    p.polish_gemm = sw(RELP_SW_GEMM_VECTOR) ? PolishGemm::VECTOR : PolishGemm::MFMA;  // (the switch: A/B measurements)
    return p;
}

std::string dual_refusal(const KernelPath& p) {
    if (p.lu_mode) return "the dual simplex needs the explicit inverse: the LU carries (carry = 1, 2) are not supported";
    if (p.network) return "the dual simplex needs the explicit inverse: the spanning-forest carry (carry = 3) is not supported";
    if (p.bounded) return "the dual simplex does not know implicit upper bounds (implicit_bounds = 1 on an LP with a bound)";
    if (p.eta_mode) return "the dual simplex does not read the deferred product form of the inverse (the dense pipeline)";
    if (p.n_dense > 0) return "the dual simplex does not price a dense block (" + std::to_string(p.n_dense) + " dense columns)";
    if (p.ftran_slices > 0) return "the dual simplex does not run beside the multi-block FTRAN";
    if (p.generated_columns) return "the dual simplex reads the columns from the CSC: generated incidence columns are not supported";
    if (p.ell_w == 2) return "the dual simplex does not take the two-entry column layout of graph LPs";
    if (p.m > DUAL_MAX_ROWS) return "the dual simplex takes at most " + std::to_string(DUAL_MAX_ROWS) + " rows (this LP has " + std::to_string(p.m) + ")";
    return std::string();
}

std::string dual_bounded_refusal(const KernelPath& p) {
    KernelPath without_bounds = p;
    without_bounds.bounded = false;
    return dual_refusal(without_bounds);
}

std::string kernel_path_json(const KernelPath& p) {
    static const char* storage[] = {"NONE", "I8_LANE", "F32_LANE", "F64_LANE", "I8_PERMUTED", "F32_ROWS", "F64_ROWS"};
    static const char* price[] = {"UNIT_PAIRS", "GENERATED", "WIDTH_2", "LDS", "GATHER"};
    static const char* ratio[] = {"REGISTERS_2", "REGISTERS_4", "REGISTERS_8", "REGISTERS_16", "MULTI_WORKGROUP", "ONE_WORKGROUP"};
    static const char* update[] = {"EAGER", "PREDICATED", "PREDICATED_SPLIT_GRID"};
    static const char* gemm[] = {"MFMA", "VECTOR"};
    std::ostringstream out;
#define RELP_FIELD(x) << ", \"" #x "\": " << p.x
    out << std::boolalpha << "{\"m\": " << p.m RELP_FIELD(n) RELP_FIELD(n_art) RELP_FIELD(n_p) RELP_FIELD(bounded) RELP_FIELD(network) RELP_FIELD(lu_mode)
        RELP_FIELD(lu_inverse) RELP_FIELD(refactor_period) RELP_FIELD(device_refactor) RELP_FIELD(async_refactor) RELP_FIELD(n_dense) RELP_FIELD(sparse_first)
        RELP_FIELD(dense_ld) RELP_FIELD(dense_lane) RELP_FIELD(dense_full) RELP_FIELD(dense_csc_start)
        << ", \"dense_storage\": \"" << storage[(int)p.dense_storage] << "\", \"dense_entry_bytes\": " << p.dense_entry_bytes() RELP_FIELD(ell_w) RELP_FIELD(generated_columns)
        RELP_FIELD(price_blocks) RELP_FIELD(dense_blocks) RELP_FIELD(vector_len) RELP_FIELD(price_lds) RELP_FIELD(ftran_slices) RELP_FIELD(eta_mode)
        RELP_FIELD(eta_cap) RELP_FIELD(slack_in_btran) << ", \"slack_of_row_length\": " << p.slack_of_row.size() RELP_FIELD(track_touched)
        RELP_FIELD(multi_workgroup_ratio) RELP_FIELD(ratio_textbook) RELP_FIELD(fused) RELP_FIELD(rho_words) RELP_FIELD(price_unit_pairs)
        << ", \"price_kernel\": \"" << price[(int)p.price_kernel] << "\", \"price_kernel_fused\": \"" << price[(int)p.price_kernel_fused]
        << "\", \"ratio_kernel\": \"" << ratio[(int)p.ratio_kernel] << "\", \"ratio_kernel_no_change\": \"" << ratio[(int)p.ratio_kernel_no_change] << "\""
        RELP_FIELD(fused_rows) << ", \"update_kernel\": \"" << update[(int)p.update_kernel] << "\", \"polish_gemm\": \"" << gemm[(int)p.polish_gemm]
        << "\", \"launches_per_batch\": " << p.launches_per_batch(false, false) << ", \"launches_per_pivot\": " << p.launches_per_pivot(false, false)
        << ", \"launches_per_pivot_forced\": " << p.launches_per_pivot(true, false) << ", \"launches_per_pivot_replayed\": " << p.launches_per_pivot(false, true) << "}";
#undef RELP_FIELD
    return out.str();
}

}  // namespace relp
