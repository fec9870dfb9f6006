// The batched exact certificate of relp_many (many_certify.hip): what relp_many_certify (many.hip) hands over and gets back.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "model.hpp"

namespace relp {

struct ExactWitnesses;  // x, y and the ray of a proved certificate (certify.hpp, certify_parts.hpp)

// Why the batched stage did not prove an LP (relp_many_certificate.fallback_reason, include/relp_amd.h)
enum ManyCertifyReason {
    MANY_CERTIFY_NONE = 0,
    MANY_CERTIFY_KIND = 1,
    MANY_CERTIFY_WIDTH = 2,
    MANY_CERTIFY_SINGULAR_MOD_P = 3,
    MANY_CERTIFY_DIGITS = 4,
    MANY_CERTIFY_SIGN = 5
};

struct ManyCertifyItem {  // a result and the basis it ended on (provider columns, -1-k for artificial k)
    const StandardForm* form = nullptr;
    const std::vector<int>* basis = nullptr;
    int mode = 0;   // as certify_basis: 0 FINITE_OPTIMUM, 1 INFEASIBLE (the final phase-one basis), 2 UNBOUNDED
    int ray = -1;   // mode 2: the provider column the solve named as entering (-1: none, the item falls back with KIND)
};

struct ManyCertifyOutcome {
    int reason = MANY_CERTIFY_NONE;  // NONE: proved, `objective` is the exact optimum (mode 1: of phase one; mode 2: "-inf")
    int digits_primal = 0, digits_dual = 0, digits_ray = 0;
    double host_seconds = 0.0;
    std::string objective;
    std::string message;
    std::shared_ptr<const ExactWitnesses> witnesses;  // proved and asked for: the vectors of the proof, else null
};

// Rows up to which the work matrix of the batched certificate lives in LDS.
int many_certify_lds_rows();

// One launch (a group per LDS size, as relp_many_solve launches) for all items, one download, then the host stage of every item on
// at most 16 threads.  `streams`: four streams of the handle.  *device_seconds: the launch (HIP events).  `keep_witnesses`: the
// host stage keeps the reconstructed vectors of every proved item in its outcome instead of dropping them.
void many_certify_batched(const std::vector<ManyCertifyItem>& items, int device, hipStream_t* streams, std::vector<ManyCertifyOutcome>* outcomes,
                          double* device_seconds, bool keep_witnesses = false);

}  // namespace relp
