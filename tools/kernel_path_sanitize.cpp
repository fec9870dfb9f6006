// plan_kernel_path under the host sanitizers, without a device: plans AFIRO, a dense 64 x 128 LP and the diagonal LP on each side of
// every row count at which the plan takes another kernel instantiation, under a few options each, and prints the plans.  kernel_path.cpp is compiled here, instrumented (its limits are inline in kernel_limits.hpp); the library only parses
// the models:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Irelp_amd/csrc tools/kernel_path_sanitize.cpp
//       relp_amd/csrc/kernel_path.cpp -Lrelp_amd -lrelp_amd -Wl,-rpath,$PWD/relp_amd -o kernel_path_sanitize && ./kernel_path_sanitize
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "device_columns.hpp"
#include "kernel_path.hpp"
#include "options.hpp"

using namespace relp;

static void plan(const relp_model* model, relp_options o, const char* what) {
    const MatrixData& md = model->form.data;
    const DeviceColumns cols = device_columns(md, implicit_bounds_apply(o, md));
    try {
        std::printf("%s: %s\n", what, kernel_path_json(plan_kernel_path(o, md, cols, DeviceMatrix(cols, md), &model->form.column_names)).c_str());
    } catch (const std::exception& e) {
        std::printf("%s: refused: %s\n", what, e.what());
    }
}

// adopt_options (options.hpp) on every struct size a header has had, read from a heap buffer of exactly that size (an over-read is an
// ASan report), and on what it refuses or clamps.  Returns the number of failed expectations.
static int check_adopt_options() {
    int failures = 0;
    auto expect = [&](bool ok, const char* what) {
        if (!ok) std::printf("adopt_options: %s\n", what), ++failures;
    };
    relp_options defaults, out;
    relp_options_default(&defaults);
    expect(adopt_options(nullptr, &out) == RELP_OK && std::memcmp(&out, &defaults, sizeof out) == 0, "a null pointer does not give the defaults");
    int known = 0;
    for (int32_t size = 0; size <= (int32_t)sizeof(relp_options) + 8; ++size) {
        if (!known_options_size(size)) continue;
        ++known;
        std::unique_ptr<unsigned char[]> exact(new unsigned char[size]);
        relp_options_default_sized(reinterpret_cast<relp_options*>(exact.get()), size);
        relp_options wanted;
        std::memcpy(&wanted, &defaults, sizeof wanted);  // (padding included: the results are compared as bytes)
        const int64_t max_pivots = 12345;  // (a field every size has, changed in the caller's struct)
        std::memcpy(exact.get() + offsetof(relp_options, max_pivots), &max_pivots, sizeof max_pivots);
        wanted.max_pivots = max_pivots;
        expect(adopt_options(reinterpret_cast<const relp_options*>(exact.get()), &out) == RELP_OK, "a known size is refused");
        expect(out.struct_size == (int32_t)sizeof(relp_options) && std::memcmp(&out, &wanted, sizeof out) == 0,
               "a known size does not give the caller's fields and the defaults behind them");
    }
    expect(known == 2, "the sizes relp_options has had are not two");
    relp_options odd = defaults;
    odd.struct_size = (int32_t)sizeof(relp_options) - 4;
    expect(adopt_options(&odd, &out) == RELP_ERR_ARGUMENT, "an unknown size is accepted");
    relp_options wide = defaults;
    wide.ftran_slices = 1000, wide.price_lds_max = 1 << 30;
    expect(adopt_options(&wide, &out) == RELP_OK && out.ftran_slices == 64 && out.price_lds_max == 160 * 1024, "ftran_slices / price_lds_max above their range");
    wide.ftran_slices = -5, wide.price_lds_max = -1;
    expect(adopt_options(&wide, &out) == RELP_OK && out.ftran_slices == 0 && out.price_lds_max == 0, "ftran_slices / price_lds_max below their range");
    return failures;
}

int main() {
    if (check_adopt_options() != 0) return 1;
    relp_options o;
    relp_options_default(&o);
    char error[512];
    relp_model* afiro = nullptr;
    if (relp_model_from_mps_ex("data/netlib/AFIRO.SIF", 1, 0, &afiro, error, 512) != RELP_OK) return std::printf("%s\n", error), 1;
    plan(afiro, o, "afiro");
    relp_options lu = o;
    lu.carry = RELP_CARRY_LU_INVERSE, lu.lu_refactor = RELP_REFACTOR_DEVICE;
    plan(afiro, lu, "afiro, inverse-factor carry");
    relp_options net = o;
    net.carry = RELP_CARRY_NETWORK;
    plan(afiro, net, "afiro, network carry");
    // dense_lp(64, 128): A[i][j] = 1 + (i * 131 + j * 17) % 100 stands in for the generator's draws (same shape, same value range)
    const int m = 64, n = 128;
    std::vector<int64_t> start(n + 1), num, den, b(m, 100000), one(n > m ? n : m, 1), cost(n, -1), zero(n, 0);
    std::vector<int32_t> rows, kind(m, 2);
    std::vector<uint8_t> has_l(n, 1), has_u(n, 0);
    for (int j = 0; j < n; ++j) {
        for (int i = 0; i < m; ++i) rows.push_back(i), num.push_back(1 + (i * 131 + j * 17) % 100), den.push_back(1);
        start[j + 1] = (int64_t)rows.size();
    }
    relp_model* dense = nullptr;
    if (relp_model_from_general_form(0, m, n, start.data(), rows.data(), num.data(), den.data(), kind.data(), zero.data(), one.data(), b.data(), one.data(),
                                     cost.data(), one.data(), has_l.data(), zero.data(), one.data(), has_u.data(), zero.data(), one.data(), 0, 1, 0, &dense, error, 512) != RELP_OK)
        return std::printf("%s\n", error), 1;
    plan(dense, o, "dense 64 x 128");
    relp_options eta = o;
    eta.ftran_min_nnz = 16;
    plan(dense, eta, "dense 64 x 128, multi-block FTRAN");
    relp_options rows_form = o;
    rows_form.switches = RELP_SW_NO_DENSE_LANE, rows_form.dense_storage = RELP_DENSE_FLOAT;
    plan(dense, rows_form, "dense 64 x 128, float rows");
    // the diagonal LP of tools/record_kernel_paths.py (row i: x_i - z_i = b_i, min sum x) around 1024, 2048, 4096 and 8192 rows
    for (const int rows_d : {1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193}) {
        const int cols_d = 2 * rows_d;
        std::vector<int64_t> d_start(cols_d + 1), d_num(cols_d), d_den(cols_d, 1), d_b(rows_d), d_cost(cols_d), d_one(cols_d, 1), d_zero(cols_d, 0);
        std::vector<int32_t> d_rows(cols_d), d_kind(rows_d, 0);
        std::vector<uint8_t> d_has_l(cols_d, 1), d_has_u(cols_d, 0);
        for (int j = 0; j < cols_d; ++j) d_start[j + 1] = j + 1, d_rows[j] = j % rows_d, d_num[j] = j < rows_d ? 1 : -1, d_cost[j] = j < rows_d ? 1 : 0;
        for (int i = 0; i < rows_d; ++i) d_b[i] = i % 100 == 0 ? 1 : 0;
        relp_model* diagonal = nullptr;
        if (relp_model_from_general_form(0, rows_d, cols_d, d_start.data(), d_rows.data(), d_num.data(), d_den.data(), d_kind.data(), d_zero.data(), d_one.data(),
                                         d_b.data(), d_one.data(), d_cost.data(), d_one.data(), d_has_l.data(), d_zero.data(), d_one.data(), d_has_u.data(),
                                         d_zero.data(), d_one.data(), 0, 1, 0, &diagonal, error, 512) != RELP_OK)
            return std::printf("%s\n", error), 1;
        char what[96];
        std::snprintf(what, sizeof what, "diagonal %d", rows_d);
        plan(diagonal, o, what);
        if (rows_d <= 2048) {
            relp_options three = o;
            three.pivot_kernels = 1;
            std::snprintf(what, sizeof what, "diagonal %d, three-kernel pivot", rows_d);
            plan(diagonal, three, what);
        }
        if (rows_d == 8193) {
            relp_options single = o;
            single.switches = RELP_SW_K2_SINGLE;
            plan(diagonal, single, "diagonal 8193, one-workgroup ratio test");
            plan(diagonal, net, "diagonal 8193, network carry");
        }
        relp_model_free(diagonal);
    }
    relp_model_free(afiro);
    relp_model_free(dense);
    return 0;
}
