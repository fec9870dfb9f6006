// The exact certificate of every LP of a relp_many launch in ONE further launch, one workgroup per LP (relp_many_certify).
//
// `certify_basis` (certify.hip) proves one basis with a chain of launches: a modular inverse of B, then two kernels per p-adic
// digit and a stream synchronisation per round of digit doubling, with host big-integer work in between.  For an LP of at most 512
// rows the whole device part fits one workgroup, which needs no grid barrier and nothing from the other LPs -- the shape of
// `many_kernel`.  Per LP the host prepares what `certify_basis` prepares (certify_parts.hpp: the row-scaled integer basis in CSR and
// CSC, the scaled right-hand side and basic costs, a prime) and FIXES the number of digits of both solves before the launch from
// Hadamard's bound, so nothing is retried inside the batch.  The workgroup
//   a. reduces B mod p into a dense m x m u32 work matrix and inverts it in place by Gauss-Jordan mod p, the pivot of a column
//      being its FIRST non-zero (any non-zero pivot is exact in Z_p); without one the LP's "singular mod p" flag is set and the
//      workgroup ends;
//   b. lifts B x = b and B' y = c_B (Dixon): per digit x_s = C (r mod p) mod p, r <- (r - B x_s) / p exactly in 128-bit
//      accumulators, with the "not divisible" and "overflow" flags of dixon_residual_kernel kept per LP.  Between the two solves the
//      work matrix is transposed in place, so both run the same wave-per-row product.  An UNBOUNDED result has a third solve, the
//      ray B alpha = a_q of the entering column the solve named: it runs against the untransposed matrix, after the primal lifting
//      and before the transpose, through the same vectors of LDS.
// The costs of the dual solve are the phase-two costs for an optimum and an unbounded LP and the phase-one costs (1 on a basic
// artificial, 0 elsewhere) for an infeasible one, whose basis is the final phase-one basis: the kernel does not know the difference.
// No atomics; every reduction runs in a fixed order (a wave's butterfly, then the waves in order), so the digits of an LP do not
// depend on the launch it is in.  Digits go to global memory as digits[lp][solve][s][i], the solves in the order primal, dual, ray.
//
// Two tiers, one source: `many_certify_kernel<true>` keeps the work matrix in LDS (4 m^2 bytes beside 28 m bytes of vectors: up to
// 198 rows), `many_certify_kernel<false>` in a per-LP slab of global memory (199 to 512 rows).
//
// After the one launch and one download every LP is finished on the host by the functions `certify_basis` uses (assembly of the
// digits, combined-unknown rational reconstruction, VERIFICATION BY EXACT SUBSTITUTION, sign checks, reduced costs of all non-basic
// columns, exact objective; for the two other verdicts the final checks of certify_parts.hpp: a positive phase-one optimum, the
// signs of the ray), on at most 16 threads, results written by index.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <thread>

#include "certify_parts.hpp"
#include "launch.hpp"
#include "many_certify.hpp"

namespace relp {

namespace {

using u32 = uint32_t;
using u64 = uint64_t;
using i64 = long long;

constexpr int MC_THREADS = 512;
constexpr int MC_WAVES = MC_THREADS / 64;
constexpr int MC_MAX_ROWS = 512;
constexpr size_t MC_LDS_BYTES = 160 * 1024;   // a CU of gfx950
constexpr size_t MC_STATIC_LDS = 1024;        // the kernel's __shared__ scalars, rounded up
constexpr int MC_TIERS = 4;                   // launch groups: three LDS sizes and the global tier
// Digits per solve an LP may ask for.  The digit buffer of an LP is then at most 3 x 512 digits x 512 rows x 4 bytes = 3 MiB, and
// the buffer of a launch is kept within MC_DIGIT_BUDGET: an LP that would pass it falls back (DIGITS) like one above the cap.
constexpr int MC_MAX_DIGITS = 512;
constexpr size_t MC_DIGIT_BUDGET = (size_t)1 << 30;
static_assert(MC_MAX_DIGITS >= 256, "the cap on the digits of a solve");

// LDS of one LP: r (i64), then r mod p, the digit, the pivot column, the pivot row (u32) and the row interchanges (int); in the LDS
// tier the m x m work matrix (u32) behind them.
__host__ __device__ constexpr size_t mc_vector_bytes(int m) { return (size_t)28 * m; }
__host__ __device__ constexpr size_t mc_lds_bytes(int m, bool matrix_in_lds) { return mc_vector_bytes(m) + (matrix_in_lds ? (size_t)4 * m * m : 0); }
// Largest m whose work matrix fits a CU: 198 rows (198 x 198 x 4 + 28 x 198 = 162 360 bytes, plus the static part; 199 rows: 163 976).
constexpr int mc_lds_tier_rows() {
    int m = 1;
    while (m < MC_MAX_ROWS && mc_lds_bytes(m + 1, true) + MC_STATIC_LDS <= MC_LDS_BYTES) ++m;
    return m;
}
static_assert(mc_lds_tier_rows() == 198, "the documented cut-off of the LDS tier of the batched certificate");

struct ManyCertLP {
    int m;
    u32 p;
    int k_primal, k_dual;   // digits of B x = b and of B' y = c_B (0: the right-hand side is zero, nothing to lift)
    int k_ray;              // digits of B alpha = a_q (0: no ray solve -- not UNBOUNDED, or an entering column without entries)
    long long start_off;    // row_start / col_start of this LP (m + 1 entries each)
    long long nz_off;       // its entries in col_index / row_value and row_index / value
    long long vec_off;      // rhs / cost / ray (m entries each)
    long long digit_off;    // digits: k_primal x m, then k_dual x m, then k_ray x m
    long long slab_off;     // global tier: the work matrix in `slab`
};

struct ManyCertArgs {
    const ManyCertLP* lps;
    const int* order;       // the LPs of this launch group
    const int *row_start, *col_index, *col_start, *row_index;
    const i64 *row_value, *value, *rhs, *cost, *ray;
    u32* digits;
    u32* slab;
    int* flags;             // [lp][4]: singular mod p, residual not divisible, residual overflow, unused
};

__device__ __forceinline__ u32 mc_mul(u32 a, u32 b, u32 p) { return reduce64((u64)a * b, p); }

// a^(p-2) mod p (Fermat): the inverse of a pivot
__device__ __forceinline__ u32 mc_inverse(u32 a, u32 p) {
    u32 result = 1, base = a;
    for (u32 e = p - 2; e != 0; e >>= 1) {
        if (e & 1u) result = mc_mul(result, base, p);
        base = mc_mul(base, base, p);
    }
    return result;
}

// K digits of A z = r0 for A = B (C holds B^-1 mod p; the rows of B by `start`, `index`, `val`), r0 in s_r.
__device__ __forceinline__ void mc_lift(const u32* C, int m, u32 p, int K, const int* start, const int* index, const i64* val, i64* s_r,
                                        u32* s_rmod, u32* s_x, u32* digits, int* s_flags) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 two32 = (1ull << 32) % p;
    for (int s = 0; s < K; ++s) {
        for (int j = tid; j < m; j += MC_THREADS) {
            i64 v = s_r[j] % (i64)p;
            if (v < 0) v += p;
            s_rmod[j] = (u32)v;
        }
        __syncthreads();
        // x_s = C (r mod p) mod p: a wave per row, the products summed in two 64-bit halves and reduced once
        for (int i = wave; i < m; i += MC_WAVES) {
            const u32* row = C + (size_t)i * m;
            u64 lo = 0, hi = 0;
            for (int j = lane; j < m; j += 64) {
                const u64 prod = (u64)row[j] * s_rmod[j];
                lo += prod & 0xffffffffu;
                hi += prod >> 32;
            }
            for (int off = 32; off > 0; off >>= 1) {
                lo += __shfl_down(lo, off);
                hi += __shfl_down(hi, off);
            }
            if (lane == 0) {
                const u32 x = reduce64((u64)reduce64(hi, p) * two32 + reduce64(lo, p), p);
                s_x[i] = x;
                digits[(size_t)s * m + i] = x;
            }
        }
        __syncthreads();
        // r <- (r - A x_s) / p exactly: |A_ij| < 2^62, x_j < 2^31, a row of at most 512 entries -- 128 bits hold it
        for (int i = tid; i < m; i += MC_THREADS) {
            __int128 acc = s_r[i];
            for (int e = start[i]; e < start[i + 1]; ++e) acc -= (__int128)val[e] * (i64)s_x[index[e]];
            const bool negative = acc < 0;
            unsigned __int128 mag = negative ? (unsigned __int128)(-acc) : (unsigned __int128)acc;
            u64 rem = 0;
            unsigned __int128 quotient = 0;
#pragma unroll
            for (int part = 3; part >= 0; --part) {  // (no 128-bit divide on the device: four 64 / 32-bit steps)
                const u64 cur = (rem << 32) | (u64)(u32)(mag >> (32 * part));
                quotient = (quotient << 32) | (cur / p);
                rem = cur % p;
            }
            if (rem != 0) s_flags[1] = 1;  // cannot happen when C is the inverse of B modulo p
            if (quotient > (unsigned __int128)0x3fffffffffffffffULL) s_flags[2] = 1;  // overflow guard
            s_r[i] = negative ? -(i64)(u64)quotient : (i64)(u64)quotient;
        }
        __syncthreads();
    }
}

template <bool LDS_MATRIX>
__global__ void __launch_bounds__(MC_THREADS) many_certify_kernel(ManyCertArgs a) {
    extern __shared__ __align__(16) unsigned char mc_smem[];
    __shared__ int s_wave_first[MC_WAVES];
    __shared__ int s_flags[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lp_index = a.order[blockIdx.x];
    const ManyCertLP lp = a.lps[lp_index];
    const int m = lp.m;
    const u32 p = lp.p;
    i64* s_r = reinterpret_cast<i64*>(mc_smem);
    u32* s_rmod = reinterpret_cast<u32*>(s_r + m);
    u32* s_x = s_rmod + m;
    u32* s_f = s_x + m;      // the pivot column before the elimination
    u32* s_rowk = s_f + m;   // the pivot row
    int* s_perm = reinterpret_cast<int*>(s_rowk + m);
    u32* C = LDS_MATRIX ? reinterpret_cast<u32*>(s_perm + m) : a.slab + lp.slab_off;
    const int* row_start = a.row_start + lp.start_off;
    const int* col_start = a.col_start + lp.start_off;
    const int* col_index = a.col_index + lp.nz_off;
    const int* row_index = a.row_index + lp.nz_off;
    const i64* row_value = a.row_value + lp.nz_off;
    const i64* value = a.value + lp.nz_off;
    if (tid < 4) s_flags[tid] = 0;

    // ---- a. C = B mod p, dense, then its inverse in place ---------------------------------------------------------------------
    for (size_t e = tid; e < (size_t)m * m; e += MC_THREADS) C[e] = 0;
    __syncthreads();
    for (int i = tid; i < m; i += MC_THREADS)
        for (int e = row_start[i]; e < row_start[i + 1]; ++e) {
            i64 v = row_value[e] % (i64)p;
            if (v < 0) v += p;
            C[(size_t)i * m + col_index[e]] = (u32)v;  // (a basis column has a row once)
        }
    __syncthreads();
    for (int k = 0; k < m; ++k) {
        // the first non-zero of column k at or below the diagonal: per thread ascending rows, the wave's minimum, the waves' minimum
        int first = INT_MAX;
        for (int i = k + tid; i < m; i += MC_THREADS)
            if (C[(size_t)i * m + k] != 0) {
                first = i;
                break;
            }
        for (int off = 32; off > 0; off >>= 1) first = min(first, __shfl_xor(first, off));
        if (lane == 0) s_wave_first[wave] = first;
        __syncthreads();
        int piv = s_wave_first[0];
#pragma unroll
        for (int w = 1; w < MC_WAVES; ++w) piv = min(piv, s_wave_first[w]);
        if (piv == INT_MAX) {  // (uniform: every thread read the same eight values)
            if (tid == 0) a.flags[4 * (size_t)lp_index + 0] = 1;
            return;
        }
        // the pivot column and the pivot row as they are, the interchange applied while they are read
        for (int i = tid; i < m; i += MC_THREADS) {
            const int src = i == k ? piv : i == piv ? k : i;
            s_f[i] = C[(size_t)src * m + k];
            s_rowk[i] = C[(size_t)piv * m + i];
        }
        if (tid == 0) s_perm[k] = piv;
        __syncthreads();
        if (piv != k)
            for (int j = tid; j < m; j += MC_THREADS) C[(size_t)piv * m + j] = C[(size_t)k * m + j];  // (row k itself is written below)
        const u32 pivinv = mc_inverse(s_f[k], p);  // (every thread the same chain: no broadcast, no barrier)
        __syncthreads();
        for (int j = tid; j < m; j += MC_THREADS) {
            const u32 v = j == k ? pivinv : mc_mul(s_rowk[j], pivinv, p);
            s_rowk[j] = v;
            C[(size_t)k * m + j] = v;
        }
        __syncthreads();
        // row i <- row i - f_i x pivot row, the column of the pivot becoming the column of the inverse; a row with f_i = 0 is skipped
        for (int i = wave; i < m; i += MC_WAVES) {
            const u32 f = s_f[i];
            if (i == k || f == 0) continue;
            const u32 minus_f = p - f;
            u32* row = C + (size_t)i * m;
            for (int j = lane; j < m; j += 64) {
                const u32 cur = j == k ? 0u : row[j];
                row[j] = reduce64((u64)minus_f * s_rowk[j] + cur, p);
            }
        }
        __syncthreads();
    }
    // the row interchanges of B are column interchanges of its inverse, undone last to first
    for (int k = m - 1; k >= 0; --k) {
        const int piv = s_perm[k];
        if (piv == k) continue;
        for (int i = tid; i < m; i += MC_THREADS) {
            u32* row = C + (size_t)i * m;
            const u32 t = row[k];
            row[k] = row[piv];
            row[piv] = t;
        }
        __syncthreads();
    }

    // ---- b. the liftings: primal, ray (UNBOUNDED only), then dual against the transposed matrix -----------------------------------
    u32* digits = a.digits + lp.digit_off;
    if (lp.k_primal > 0) {
        for (int i = tid; i < m; i += MC_THREADS) s_r[i] = a.rhs[lp.vec_off + i];
        __syncthreads();
        mc_lift(C, m, p, lp.k_primal, row_start, col_index, row_value, s_r, s_rmod, s_x, digits, s_flags);
    }
    if (lp.k_ray > 0) {  // B alpha = a_q: the rows of B again, before the work matrix is transposed
        for (int i = tid; i < m; i += MC_THREADS) s_r[i] = a.ray[lp.vec_off + i];
        __syncthreads();
        mc_lift(C, m, p, lp.k_ray, row_start, col_index, row_value, s_r, s_rmod, s_x, digits + (size_t)(lp.k_primal + lp.k_dual) * m, s_flags);
    }
    if (lp.k_dual > 0) {
        // (B')^-1 = (B^-1)': transposed in place; the rows of B' are the columns of B
        for (int i = wave; i < m; i += MC_WAVES)
            for (int j = i + 1 + lane; j < m; j += 64) {
                const u32 t = C[(size_t)i * m + j];
                C[(size_t)i * m + j] = C[(size_t)j * m + i];
                C[(size_t)j * m + i] = t;
            }
        for (int i = tid; i < m; i += MC_THREADS) s_r[i] = a.cost[lp.vec_off + i];
        __syncthreads();
        mc_lift(C, m, p, lp.k_dual, col_start, row_index, value, s_r, s_rmod, s_x, digits + (size_t)lp.k_primal * m, s_flags);
    }
    __syncthreads();
    if (tid == 1 || tid == 2)
        if (s_flags[tid]) a.flags[4 * (size_t)lp_index + tid] = 1;
}

double mc_now() {
    using clock = std::chrono::steady_clock;
    return std::chrono::duration<double>(clock::now().time_since_epoch()).count();
}

// What the host keeps of one LP between the preparation and its host stage.
struct Prepared {
    std::shared_ptr<const CertifyStatic> statics;
    IntegerBasis B;
    std::vector<i64> rhs, cost_basis, ray;  // ray: a_q scaled by the row multipliers (mode 2), else zeros
    std::vector<char> in_basis;
    int k_primal = 0, k_dual = 0, k_ray = 0;
    int slot = -1;  // index among the LPs of the launch, -1: not launched
    long long digit_off = 0;
    double work = 0.0;
    int bucket = 0;
};

// Digits of a solve A z = rhs with A = B (`transpose` 0) or B' (1).  z_i = det(A_i) / det(A) by Cramer's rule; with N and D the
// Hadamard bounds of the numerators and of the denominator (for each the smaller of the column-norm and the row-norm product) the
// rational reconstruction needs 2 N D < p^K, K = ceil(log_p(2 N D)) + 1.  The reconstruction of certify_parts.hpp asks more: it
// accepts a numerator or a denominator v with 2 bits(v) + 2 <= bits(p^K) -- both below the SAME bound sqrt(p^K) / 2 -- and it
// reconstructs an integer combination of the unknowns with weights below 2^16 first, so V = max(2^16 m N, D) takes the place of
// both and K = ceil((2 log2 V + 4) / log2 p) + 1, which is never less.  Logarithms in long double, rounded up.
int mc_digit_count(const IntegerBasis& B, const std::vector<i64>& rhs, int transpose, u32 p) {
    const int m = B.m;
    if (std::all_of(rhs.begin(), rhs.end(), [](i64 v) { return v == 0; })) return 0;
    std::vector<long double> col2(m, 0.0L), row2(m, 0.0L);  // squared norms
    for (int k = 0; k < m; ++k)
        for (int e = B.col_start[k]; e < B.col_start[k + 1]; ++e) {
            const long double v = (long double)B.value[e];
            col2[k] += v * v;
            row2[B.row_index[e]] += v * v;
        }
    const std::vector<long double>& across = transpose ? row2 : col2;  // the columns of A
    const std::vector<long double>& along = transpose ? col2 : row2;   // the rows of A
    long double rhs2 = 0.0L;
    for (i64 v : rhs) rhs2 += (long double)v * (long double)v;
    auto half_log2 = [](long double squared) { return 0.5L * log2l(std::max(squared, 1.0L)); };
    long double log_cols = 0.0L, log_rows = 0.0L, smallest_col = HUGE_VALL, log_rows_rhs = 0.0L;
    for (int k = 0; k < m; ++k) {
        log_cols += half_log2(across[k]);
        smallest_col = std::min(smallest_col, half_log2(across[k]));
        log_rows += half_log2(along[k]);
        log_rows_rhs += half_log2(along[k] + (long double)rhs[k] * (long double)rhs[k]);  // row k of A with one entry replaced by rhs_k
    }
    const long double log_d = std::min(log_cols, log_rows);
    const long double log_n = std::min(log_cols - smallest_col + half_log2(rhs2), log_rows_rhs);  // a column replaced by rhs
    const long double log_v = std::max(log_n + 16.0L + log2l((long double)m), log_d);
    const long double log_p = log2l((long double)p) - 1e-9L;
    const long double digits = ceill((2.0L * log_v + 4.0L) / log_p * (1.0L + 1e-12L)) + 1.0L;
    return digits > 1e6L ? INT_MAX : (int)digits;
}

}  // namespace

int many_certify_lds_rows() { return mc_lds_tier_rows(); }

void many_certify_batched(const std::vector<ManyCertifyItem>& items, int device, hipStream_t* streams, std::vector<ManyCertifyOutcome>* outcomes,
                          double* device_seconds, bool keep_witnesses) {
    const int n = (int)items.size();
    outcomes->assign(n, ManyCertifyOutcome{});
    if (device_seconds) *device_seconds = 0.0;
    if (n == 0) return;
    std::vector<Prepared> prepared(n);
    const int threads = std::max(1, std::min({16, n, (int)std::thread::hardware_concurrency()}));
    auto on_pool = [&](auto&& fn) {  // fn(k) for every LP, by index: the order of completion cannot show
        std::atomic<int> next{0};
        auto work = [&] {
            for (int k = next.fetch_add(1); k < n; k = next.fetch_add(1)) fn(k);
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < threads; ++t) pool.emplace_back(work);
        work();
        for (std::thread& t : pool) t.join();
    };
    const u32 p = CERTIFY_PRIMES[0];

    // ---- preparation: what certify_basis prepares, and the digit counts ----------------------------------------------------------
    on_pool([&](int k) {
        const double t0 = mc_now();
        ManyCertifyOutcome& out = (*outcomes)[k];
        Prepared& pr = prepared[k];
        try {
            const StandardForm& form = *items[k].form;
            const int mode = items[k].mode, ray = items[k].ray;
            pr.statics = certify_static(form, &out.message);
            const bool no_costs = pr.statics && mode != 1 && pr.statics->cost_mult == 0;  // (the phase-one certificate has its own costs)
            if (no_costs) out.message = "cost scaling overflows 128 bits";
            if (!pr.statics || no_costs ||
                !certify_integer_basis(*pr.statics, form.data, *items[k].basis, mode, &pr.B, &pr.cost_basis, &pr.in_basis, &out.message)) {
                out.reason = MANY_CERTIFY_WIDTH;
            } else if (mode == 2 && (ray < 0 || ray >= (int)pr.in_basis.size() || pr.in_basis[ray])) {
                out.reason = MANY_CERTIFY_KIND;
                out.message = "unbounded: no entering column";
            } else {
                const int m = pr.B.m;
                pr.ray.assign(m, 0);
                if (mode == 2 && !certify_scaled_column(*pr.statics, ray, &pr.ray, &out.message)) out.reason = MANY_CERTIFY_WIDTH;
                pr.rhs.resize(m);
                for (int i = 0; i < m && out.reason == MANY_CERTIFY_NONE; ++i) {
                    const BigInt& v = pr.statics->rhs_big[i];
                    if (v.bits() > 62) {
                        out.reason = MANY_CERTIFY_WIDTH;
                        out.message = "scaled right-hand side does not fit 62 bits";
                    } else {
                        u64 mag = 0;
                        for (size_t l = 0; l < v.mag.size() && l < 2; ++l) mag |= (u64)v.mag[l] << (32 * l);
                        pr.rhs[i] = v.sign() < 0 ? -(i64)mag : (i64)mag;
                    }
                }
                if (out.reason == MANY_CERTIFY_NONE) {
                    pr.k_primal = mc_digit_count(pr.B, pr.rhs, 0, p);
                    pr.k_dual = mc_digit_count(pr.B, pr.cost_basis, 1, p);
                    pr.k_ray = mode == 2 ? mc_digit_count(pr.B, pr.ray, 0, p) : 0;
                    if (m > MC_MAX_ROWS || pr.k_primal > MC_MAX_DIGITS || pr.k_dual > MC_MAX_DIGITS || pr.k_ray > MC_MAX_DIGITS) {
                        out.reason = MANY_CERTIFY_DIGITS;
                        out.message = "more p-adic digits than the batched certificate lifts";
                    }
                    const bool lds = m <= mc_lds_tier_rows();
                    pr.bucket = !lds ? 3 : m <= 48 ? 0 : m <= 96 ? 1 : 2;
                    pr.work = (double)m * m * m + (double)(pr.k_primal + pr.k_dual + pr.k_ray) * ((double)m * m + (double)pr.B.value.size());
                }
            }
        } catch (const RatOverflow& e) {
            out.reason = MANY_CERTIFY_WIDTH;
            out.message = std::string("exact certificate: ") + e.what();
        }
        out.host_seconds += mc_now() - t0;
    });

    // ---- pack: per-LP offsets; launch order by LDS size, longest estimated work first (ties: the caller's order) -----------------
    std::vector<ManyCertLP> desc;
    std::vector<int> lp_of_slot, row_start, col_index, col_start, row_index;
    std::vector<i64> row_value, value, rhs, cost, ray;
    long long digit_words = 0, slab_words = 0;
    for (int k = 0; k < n; ++k) {
        ManyCertifyOutcome& out = (*outcomes)[k];
        Prepared& pr = prepared[k];
        if (out.reason != MANY_CERTIFY_NONE) continue;
        const int m = pr.B.m;
        const long long own = (long long)(pr.k_primal + pr.k_dual + pr.k_ray) * m;
        if ((size_t)(digit_words + own) * sizeof(u32) > MC_DIGIT_BUDGET) {
            out.reason = MANY_CERTIFY_DIGITS;
            out.message = "the digit buffer of the launch is full";
            continue;
        }
        ManyCertLP d;
        d.m = m;
        d.p = p;
        d.k_primal = pr.k_primal;
        d.k_dual = pr.k_dual;
        d.k_ray = pr.k_ray;
        d.start_off = (long long)row_start.size();
        d.nz_off = (long long)col_index.size();
        d.vec_off = (long long)rhs.size();
        d.digit_off = pr.digit_off = digit_words;
        d.slab_off = pr.bucket == 3 ? slab_words : 0;
        digit_words += own;
        if (pr.bucket == 3) slab_words += (long long)m * m;
        pr.slot = (int)desc.size();
        desc.push_back(d);
        lp_of_slot.push_back(k);
        row_start.insert(row_start.end(), pr.B.row_start.begin(), pr.B.row_start.end());
        col_start.insert(col_start.end(), pr.B.col_start.begin(), pr.B.col_start.end());
        col_index.insert(col_index.end(), pr.B.col_index.begin(), pr.B.col_index.end());
        row_index.insert(row_index.end(), pr.B.row_index.begin(), pr.B.row_index.end());
        row_value.insert(row_value.end(), pr.B.row_value.begin(), pr.B.row_value.end());
        value.insert(value.end(), pr.B.value.begin(), pr.B.value.end());
        rhs.insert(rhs.end(), pr.rhs.begin(), pr.rhs.end());
        cost.insert(cost.end(), pr.cost_basis.begin(), pr.cost_basis.end());
        ray.insert(ray.end(), pr.ray.begin(), pr.ray.end());
    }
    const int launched = (int)desc.size();
    std::vector<u32> digits((size_t)digit_words);
    std::vector<int> flags((size_t)4 * launched, 0);
    if (launched > 0) {
        std::vector<int> order(launched);
        for (int s = 0; s < launched; ++s) order[s] = s;
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
            const Prepared &a = prepared[lp_of_slot[x]], &b = prepared[lp_of_slot[y]];
            if (a.bucket != b.bucket) return a.bucket < b.bucket;
            return a.work > b.work;
        });
        int first[MC_TIERS + 1] = {}, rows[MC_TIERS] = {};
        for (int s : order) {
            const Prepared& pr = prepared[lp_of_slot[s]];
            first[pr.bucket + 1] += 1;
            rows[pr.bucket] = std::max(rows[pr.bucket], pr.B.m);
        }
        for (int b = 0; b < MC_TIERS; ++b) first[b + 1] += first[b];

        RELP_HIP(hipSetDevice(device));
        DeviceAllocations memory;
        struct Free {
            DeviceAllocations& memory;
            ~Free() { memory.free_all(); }
        } free_at_end{memory};
        auto upload = [&](const auto& host) {
            using T = typename std::decay_t<decltype(host)>::value_type;
            T* d = memory.alloc<T>(host.size());
            if (!host.empty()) RELP_HIP(hipMemcpy(d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
            return d;
        };
        ManyCertArgs args;
        args.lps = upload(desc);
        const int* d_order = upload(order);
        args.row_start = upload(row_start);
        args.col_index = upload(col_index);
        args.col_start = upload(col_start);
        args.row_index = upload(row_index);
        args.row_value = upload(row_value);
        args.value = upload(value);
        args.rhs = upload(rhs);
        args.cost = upload(cost);
        args.ray = upload(ray);
        args.digits = memory.alloc<u32>((size_t)digit_words);
        args.slab = memory.alloc<u32>((size_t)slab_words);
        args.flags = upload(flags);  // (zeros)
        static PerDeviceOnce once;
        allow_full_lds_once(once, &many_certify_kernel<true>);
        hipEvent_t ev_start = nullptr, ev_stop = nullptr, ev_done[MC_TIERS] = {};
        struct Events {
            hipEvent_t *a, *b, *c;
            ~Events() {
                if (*a) (void)hipEventDestroy(*a);
                if (*b) (void)hipEventDestroy(*b);
                for (int t = 0; t < MC_TIERS; ++t)
                    if (c[t]) (void)hipEventDestroy(c[t]);
            }
        } events{&ev_start, &ev_stop, ev_done};
        RELP_HIP(hipEventCreate(&ev_start));
        RELP_HIP(hipEventCreate(&ev_stop));
        for (int t = 1; t < MC_TIERS; ++t) RELP_HIP(hipEventCreateWithFlags(&ev_done[t], hipEventDisableTiming));
        RELP_HIP(hipEventRecord(ev_start, streams[0]));
        for (int t = 0; t < MC_TIERS; ++t) {  // a stream per launch group
            hipStream_t s = streams[t];
            if (t > 0) RELP_HIP(hipStreamWaitEvent(s, ev_start, 0));
            const int blocks = first[t + 1] - first[t];
            if (blocks > 0) {
                ManyCertArgs part = args;
                part.order = d_order + first[t];
                const bool lds = t < 3;
                const size_t bytes = mc_lds_bytes(rows[t], lds);
                if (lds) hipLaunchKernelGGL((many_certify_kernel<true>), dim3(blocks), dim3(MC_THREADS), bytes, s, part);
                else hipLaunchKernelGGL((many_certify_kernel<false>), dim3(blocks), dim3(MC_THREADS), bytes, s, part);
                check_launch("many_certify_kernel");
            }
            if (t > 0) {
                RELP_HIP(hipEventRecord(ev_done[t], s));
                RELP_HIP(hipStreamWaitEvent(streams[0], ev_done[t], 0));
            }
        }
        RELP_HIP(hipEventRecord(ev_stop, streams[0]));
        RELP_HIP(hipEventSynchronize(ev_stop));
        float ms = 0.f;
        RELP_HIP(hipEventElapsedTime(&ms, ev_start, ev_stop));
        if (device_seconds) *device_seconds = ms * 1e-3;
        if (digit_words > 0) RELP_HIP(hipMemcpy(digits.data(), args.digits, (size_t)digit_words * sizeof(u32), hipMemcpyDeviceToHost));
        RELP_HIP(hipMemcpy(flags.data(), args.flags, flags.size() * sizeof(int), hipMemcpyDeviceToHost));
    }

    // ---- the host stage of every LP: the functions of certify_basis, one LP per thread ------------------------------------------
    on_pool([&](int k) {
        ManyCertifyOutcome& out = (*outcomes)[k];
        const Prepared& pr = prepared[k];
        if (out.reason != MANY_CERTIFY_NONE || pr.slot < 0) return;
        const double t0 = mc_now();
        out.digits_primal = pr.k_primal;
        out.digits_dual = pr.k_dual;
        out.digits_ray = pr.k_ray;
        try {
            const int m = pr.B.m;
            const int* flag = flags.data() + (size_t)4 * pr.slot;
            if (flag[0]) {
                out.reason = MANY_CERTIFY_SINGULAR_MOD_P;
                out.message = "basis singular modulo the prime of the batched certificate";
            } else if (flag[1] || flag[2]) {
                out.reason = MANY_CERTIFY_WIDTH;
                out.message = flag[2] ? "Dixon residual overflow (coefficients too large for the 128-bit path)" : "Dixon residual not divisible by p";
            } else {
                CertifyTimes times;
                ExactVector x, y, alpha;
                auto solve = [&](const std::vector<i64>& r, int transpose, int K, const u32* base, ExactVector* z) {
                    z->numer.assign(m, BigInt(0));
                    z->denom = BigInt(1);
                    if (K == 0) return true;  // (a zero right-hand side)
                    std::vector<const u32*> rows(K);
                    for (int s = 0; s < K; ++s) rows[s] = base + (size_t)s * m;
                    return dixon_reconstruct(pr.B, r, transpose, p, rows, false, z, times);
                };
                const u32* base = digits.data() + pr.digit_off;
                const StandardForm& form = *items[k].form;
                const std::vector<int>& basis = *items[k].basis;
                const int mode = items[k].mode;
                CertifySigns signs;
                if (!solve(pr.rhs, 0, pr.k_primal, base, &x) || !solve(pr.cost_basis, 1, pr.k_dual, base + (size_t)pr.k_primal * m, &y) ||
                    !solve(pr.ray, 0, pr.k_ray, base + (size_t)(pr.k_primal + pr.k_dual) * m, &alpha)) {
                    out.reason = MANY_CERTIFY_DIGITS;
                    out.message = "the reconstruction from the digits of the batched certificate failed its exact verification";
                } else {
                    x.denom = x.denom * pr.statics->rhs_den;  // x_B = numer / (denom * rhs_den); the sign checks only need denom > 0
                    bool holds = certify_signs(*pr.statics, form.data, basis, pr.in_basis, mode, x, y, false, &signs, &out.message);
                    if (holds && mode == 0) {
                        holds = signs.worst_row < 0 && signs.worst_col < 0;
                        if (holds) out.objective = certify_objective(form, *pr.statics, pr.cost_basis, x);
                        else out.message = "the basis is not optimal in exact arithmetic";
                    } else if (holds && mode == 1) {
                        holds = certify_infeasible(signs, pr.cost_basis, x, &out.objective, &out.message);
                    } else if (holds) {
                        holds = certify_unbounded_entering(signs, pr.in_basis, items[k].ray, &out.message) &&
                                certify_unbounded_ray(basis, alpha, &out.objective, &out.message);
                    }
                    if (!holds) out.reason = MANY_CERTIFY_SIGN;  // (modes 1 and 2 have no repair pivots: the serial certificate says the same)
                    else if (keep_witnesses) out.witnesses = make_exact_witnesses(*pr.statics, mode, basis, items[k].ray, x, y, alpha);
                }
            }
        } catch (const RatOverflow& e) {
            out.reason = MANY_CERTIFY_WIDTH;
            out.message = std::string("exact certificate: ") + e.what();
        }
        out.host_seconds += mc_now() - t0;
    });
}

}  // namespace relp
