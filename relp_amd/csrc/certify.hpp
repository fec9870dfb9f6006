// The exact certificate's interface (certify.hip): what a handle keeps between its certificates, the certificate itself and the
// exact vectors it was proved with.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "model.hpp"

namespace relp {

// Exact primal solution of a certified basis: x_B[k] = numer[k] / denom for the provider column basis[k] (certify.hip).
struct ExactPrimal;
// The three exact vectors of a proved certificate, in the terms of the caller's LP (certify_parts.hpp): x_B, the dual solution y (the
// Farkas vector of an INFEASIBLE verdict) and alpha = B^-1 a_q of an UNBOUNDED one.
struct ExactWitnesses;
// What a handle keeps between its certificates (certify.hip): the second stream of the dual lifting (creating and destroying a
// stream costs 4 + 2 ms, as much as the rest of a certificate), the host thread that drives it (creating one costs 0.1 ms), the
// device buffers (returned to the handle, not to the driver), the pinned staging arena the uploads are packed into and the digits
// are downloaded into (a copy from or to pageable memory goes through a copy kernel of the runtime and blocks), and the p-adic digit
// counts the last certificate of the loaded LP needed.  Nothing of it is shared between handles.
struct CertifyScratch {
    hipStream_t second = nullptr;
    std::shared_ptr<void> worker;  // certify.hip: CertifyWorker, made by the first certificate; joined by release() or with the scratch
    struct Block {
        void* ptr;
        size_t bytes;
        bool busy;
    };
    std::vector<Block> blocks;
    std::vector<Block> pinned;    // the staging arena: pinned host blocks, handed out and taken back like the device blocks
    void* take_pinned(size_t bytes);
    void give_back_pinned(void* ptr);
    int digit_hints[2] = {0, 0};  // (primal, dual); 0: unknown.  Reset when another LP is loaded.
    std::shared_ptr<const void> statics;  // the LP's integer scaling (certify.hip: CertifyStatic); reset when another LP is loaded
    void* take(size_t bytes);     // smallest free block that fits, else a new allocation
    void give_back(void* ptr);
    void release();               // frees everything (the handle's destructor; device must be current)
};
// (provider column, "num/den" reduced) for every basic provider column with a non-zero exact value, ascending column
std::vector<std::pair<int, std::string>> exact_primal_values(const ExactPrimal& primal);
// The exact primal values of a certificate made elsewhere (network_carry.hip: the forest's): provider column and value, over one
// common denominator.
std::shared_ptr<const ExactPrimal> make_exact_primal(const std::vector<int>& columns, const std::vector<Rat>& values);
// The mode (as certify_basis) of the certificate the witnesses belong to.
int exact_witness_mode(const ExactWitnesses& witnesses);
// (index, "num/den" reduced, den > 0) of the non-zero entries of one witness, ascending index.  `which` (relp_witness): PRIMAL by
// provider column (a basic artificial has value 0 and is not reported), DUAL by row, RAY by provider column: 1 on the entering
// column, -alpha_k on basis[k].  The caller has checked that the mode has this witness.
std::vector<std::pair<int, std::string>> exact_witness_values(const ExactWitnesses& witnesses, int which);
// The exact certificate of a basis given in provider columns (certify.hip, where the modes are described).  `witnesses` (may be
// null): the vectors the verdict was proved with, set only when *certified.
void certify_basis(const StandardForm& form, const std::vector<int>& basis_provider_columns, int device, hipStream_t stream,
                   std::string* objective, bool* certified, long long* repair_pivots, std::string* message, int mode, int entering,
                   std::shared_ptr<const ExactPrimal>* primal, CertifyScratch* scratch,
                   std::shared_ptr<const ExactWitnesses>* witnesses = nullptr);
// The exact proof of the INFEASIBLE verdict the dual simplex stops with (certify.hip): `basis` is the basis as the device holds it, in
// provider columns by row -- every row of the standard form, or with `bounded` (an LP held on implicit upper bounds) the constraint
// rows only --, `row` the row p at which the loop found the dual unbounded.  One transposed lifting gives row p of the inverse exactly;
// the Farkas vector is its negative, or on a bounded handle either sign of it extended over the bound rows in closed form
// (`first_sign`: -1 tries -rho_p first, +1 the other one; both are tried).  *certified with *objective = y'b > 0 and the witnesses of an
// INFEASIBLE certificate (mode 1: y by row of the standard form), or *message names the exact inequality that failed.  No repair pivots.
void certify_dual_farkas(const StandardForm& form, const std::vector<int>& basis_provider_columns, int row, bool bounded, int first_sign,
                         int device, hipStream_t stream, std::string* objective, bool* certified, std::string* message,
                         CertifyScratch* scratch, std::shared_ptr<const ExactWitnesses>* witnesses);
// The exact lower bound of a basis the dual simplex stopped on, at its objective cutoff or at its iteration limit (certify.hip): `basis`
// and `bounded` as certify_dual_farkas takes them.  One transposed lifting of B'y = c_B, then d_j = c_j - y'a_j for every provider column
// in exact integers: every d_j >= 0, or on a bounded handle min(0, d_j) on the bound row of a column that has one and d_j >= 0 for the
// rest.  *objective = z = y'b + fixed cost (bounded: y_c'b_c + sum_j min(0, d_j) u_j + fixed cost).  `at_cutoff`: certified only if also
// z >= cutoff, the double taken as the exact rational it is (-inf: always; the result of a loop that stopped at the cutoff); otherwise z
// is certified whatever its size.  *certified with the witnesses of mode 3 (y by row of the standard form, bound rows included, and
// nothing else), or *message names the provider column that prices negative, the two numbers, or the refusal of the optimum's
// certificate ("cost scaling overflows 128 bits").  No repair pivots.
void certify_dual_bound(const StandardForm& form, const std::vector<int>& basis_provider_columns, bool bounded, bool at_cutoff, double cutoff,
                        int device, hipStream_t stream, std::string* objective, bool* certified, std::string* message,
                        CertifyScratch* scratch, std::shared_ptr<const ExactWitnesses>* witnesses);

}  // namespace relp
