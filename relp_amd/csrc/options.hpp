// The options plumbing (host-only: no HIP): the caller's relp_options adopted into the library's struct, and the calling thread's tuning.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/relp_amd.h"

namespace relp {

// The calling thread's A/B switches and sizes (relp_options.switches and the fields beside it): set by the C ABI from the handle's
// options for the duration of a call (capi.cpp `guarded`), read by the launch helpers that have no handle in reach (lu_factor.hip,
// lu_device_tasks.hip, certify.hip).  Round 5: these were getenv calls; nothing that changes a kernel or a result reads the
// environment any more.
struct Tuning {
    unsigned switches = 0;
    int certify_threads = 0, luf_dense_tail = 0, luf_slack = 0, luf_lds = 0, luf_lds_arena = 0, luf_arena_cap = 0;
    bool has(unsigned bit) const { return (switches & bit) != 0; }
};
inline Tuning& thread_tuning() {
    static thread_local Tuning tuning;
    return tuning;
}
inline Tuning tuning_of(const relp_options& o) {
    Tuning t;
    t.switches = o.switches;
    t.certify_threads = o.certify_threads;
    t.luf_dense_tail = o.luf_dense_tail;
    t.luf_slack = o.luf_slack;
    t.luf_lds = o.luf_lds;
    t.luf_lds_arena = o.luf_lds_arena;
    t.luf_arena_cap = o.luf_arena_cap;
    return t;
}
// The sizes relp_options has had: round 4 (through lu_refactor), round 5 / 6 (through carry_weights_min), round 7 (through
// reserved_round7).  A struct of any other size was not written by a header of this library.
inline bool known_options_size(int32_t size) {
    const int32_t round4_size = (int32_t)(offsetof(relp_options, lu_refactor) + sizeof(int32_t));
    const int32_t round5_size = (int32_t)(offsetof(relp_options, carry_weights_min) + sizeof(double));
    const int32_t round7_size = (int32_t)(offsetof(relp_options, reserved_round7) + sizeof(int32_t));
    static_assert(offsetof(relp_options, reserved_round7) + sizeof(int32_t) == sizeof(relp_options), "a field was appended: give its round a size here");
    static_assert(offsetof(relp_options, dual_pricing) == offsetof(relp_options, carry_weights_min) + sizeof(double), "round 7 grew the struct by exactly 8 bytes");
    return size == round4_size || size == round5_size || size == round7_size;
}
// The caller's options into the library's struct: as many bytes as the caller's header had (relp_options.struct_size, one of the known
// sizes), the defaults for the rest.  RELP_ERR_ARGUMENT when the struct was not initialised by relp_options_default(_sized) or comes
// from a newer header, names no relp_dual_pricing or has a non-zero reserved field.  The tuning fields are clamped to what their
// comments promise.
inline int32_t adopt_options(const relp_options* options, relp_options* out) {
    relp_options_default_sized(out, (int32_t)sizeof(relp_options));
    if (!options) return RELP_OK;
    if (!known_options_size(options->struct_size)) return RELP_ERR_ARGUMENT;
    std::memcpy(out, options, (size_t)options->struct_size);
    out->struct_size = (int32_t)sizeof(relp_options);
    out->ftran_slices = std::max(0, std::min(64, out->ftran_slices));
    out->price_lds_max = std::max(0, std::min(160 * 1024, out->price_lds_max));  // (a CU of gfx950 has 160 KB of LDS)
    if (out->dual_pricing != RELP_DUAL_PRICING_INFEASIBILITY && out->dual_pricing != RELP_DUAL_PRICING_STEEPEST_EDGE) return RELP_ERR_ARGUMENT;
    if (out->reserved_round7 != 0) return RELP_ERR_ARGUMENT;
    return RELP_OK;
}
struct TuningScope {  // the thread's tuning for the lifetime of the object
    Tuning saved;
    explicit TuningScope(const Tuning& t) : saved(thread_tuning()) { thread_tuning() = t; }
    ~TuningScope() { thread_tuning() = saved; }
};

}  // namespace relp
