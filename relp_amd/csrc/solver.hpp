// Device-resident two-phase revised simplex for one LP: host-side class (one handle = one stream on one GPU).
//
// Mirrors the reference's `Tableau<Carry<F, BI>, Kind>` + `PivotRule` state (tableau/mod.rs:25-39,
// carry/mod.rs:46-66, strategy/pivot_rule.rs:190-193) but keeps every array in HBM for the whole solve:
// the host only enqueues kernels and polls a control word once per `pivots_per_launch` pivots.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/relp_amd.h"
#include "certify.hpp"
#include "device_columns.hpp"
#include "device_lp.hpp"
#include "device_memory.hpp"
#include "dual.hpp"
#include "exact.hpp"
#include "kernel_path.hpp"
#include "lu.hpp"
#include "model.hpp"

namespace relp {

// Host copy of the forest (set_basis, crash, the fine-grained operations, the certificate): `order` lists every row after its parent.
struct HostTree {
    std::vector<int> parent, slot, child, order, depth;
    std::vector<signed char> sign;
};

class Solver {
public:
    explicit Solver(const relp_options& options);
    ~Solver();

    void load(StandardForm&& form);
    bool loaded() const { return loaded_; }
    bool ratio_textbook() const { return path_.ratio_textbook; }

    void solve(relp_result* result);
    void begin_phase_one();
    void begin_phase_two();
    void set_basis(const int* basis_columns);
    long long iterate(long long count, int* stop_reason);
    // Dual simplex from a dual-feasible basis of the loaded LP, given as set_basis takes it (dual.hpp; DESIGN.md "Dual simplex from a
    // given basis").  begin_dual: the refusals (std::invalid_argument: a plan the dual kernels do not take, an artificial in the basis,
    // a basis that is not dual feasible), set_basis, the loop's buffers; no pivot.  iterate_dual: up to `count` dual pivots; the stop
    // reasons are ST_NO_ENTERING (no infeasible row is left), ST_UNBOUNDED (the LP is infeasible) and ST_BUDGET.  solve_dual: both,
    // then the primal loop from the primal-feasible basis (it normally makes no pivot) and the result as `solve` reports it.
    void begin_dual(const int* basis_columns);
    long long iterate_dual(long long count, int* stop_reason);
    void solve_dual(const int* basis_columns, relp_result* result);
    // The same from the inverse of `parent`, a handle on the same device whose LP this one extends (dual_inherit.hpp: the parent's
    // basis in the first positions, the slack of each appended row behind it; costs and right-hand sides may differ).  The refusals
    // come before anything is launched: std::invalid_argument for a plan the dual kernels do not take (either handle), a parent on
    // another device and a non-empty dual_inherit_refusal; std::runtime_error for a parent that has no LP, or no basis and inverse
    // yet, or is this handle.  Then the child's inverse is written from the parent's by one kernel (dual_inherit_kernel) behind an
    // event on the parent's stream, and a forced polish guards it: its residual pass measures the child's basis against the child's
    // own matrix, corrects what it finds and rebuilds from scratch by itself from 0.5 on.  The parent is only read.
    void begin_dual_from(const Solver& parent, const int* basis_columns);
    void solve_dual_from(const Solver& parent, const int* basis_columns, relp_result* result);
    // The same loop on a plan with implicit upper bounds (the BOUNDED instantiations of dual.hip), and on every plan begin_dual takes
    // (then with the kernels begin_dual runs): dual_bounded_refusal.  `basis_columns` is a basis of the reference's formulation, one
    // column per row of MatrixData with the bound rows included, as get_basis returns it; a basic variable above its upper bound is what
    // the loop repairs, not an error.  begin_dual, solve_dual and the _from pair keep refusing a bounded plan.
    void begin_dual_bounded(const int* basis_columns);
    void solve_dual_bounded(const int* basis_columns, relp_result* result);
    bool dual_bounded() const { return dual_bounded_; }  // the last start ran the loop with implicit upper bounds
    // begin_dual_bounded with the inverse written from the one `parent` holds, as begin_dual_from does it for plans without implicit
    // bounds: the relation is dual_bounded_inherit_refusal over the two formulations' bases (the parent's read off its device state),
    // the kernel dual_inherit_mapped_kernel, which takes the positions and the complemented columns of either side as they are.  The
    // refusals come before anything is launched, with the classes of begin_dual_from: std::invalid_argument for dual_bounded_refusal of
    // either plan, a plan that holds its bounds as rows (implicit_bounds = 0 on an LP with a bound), a parent on another device and a
    // non-empty relation; std::runtime_error for a parent without LP, without basis and inverse, or this handle.  The same guard.
    void begin_dual_bounded_from(const Solver& parent, const int* basis_columns);
    void solve_dual_bounded_from(const Solver& parent, const int* basis_columns, relp_result* result);
    // Of the last start (0 after any other than begin_dual_bounded_from): inherited positions whose column the two handles hold with
    // opposite signs, and inherited positions that are not the parent's.
    long long dual_inherit_complemented() const { return dual_inherit_complemented_; }
    long long dual_inherit_moved() const { return dual_inherit_moved_; }
    // The long-step (bound-flipping) ratio test of that loop (dual.hpp: launch_dual_long_step), off by default.  The switch holds until
    // changed and is read by begin_dual_bounded / solve_dual_bounded; while it is on, begin_dual, solve_dual and the _from pair refuse
    // (std::invalid_argument).  On a bounded-entry plan without bounds there is no boxed column and it changes nothing.
    void set_dual_long_step(bool on) { dual_long_step_ = on; }
    bool dual_long_step() const { return dual_long_active_; }  // the last start ran the loop with it
    long long dual_flips() const { return dual_flips_; }  // columns it sent to their other bound, over the dual pivots since that start
    long long dual_long_step_skipped() const { return dual_long_skipped_; }  // pivots at which it held too many candidates and made none
    // The exact proof of an INFEASIBLE verdict of solve_dual / solve_dual_from / solve_dual_bounded / solve_dual_bounded_from
    // (certify.hpp: certify_dual_farkas), off by default.  The switch holds until changed, is read by every start and takes effect where
    // relp_options.certify is set and the loop ends dual unbounded: the result is then certified with the Farkas vector as its dual
    // witness and y'b as its exact objective, or uncertified with the exact inequality that failed in last_error.
    void set_dual_farkas(bool on) { dual_farkas_ = on; }
    bool dual_farkas() const { return dual_farkas_active_; }  // the switch as the last start read it
    int dual_farkas_row() const { return dual_farkas_row_; }  // the row of the basis the last proof used, -1 where there was none
    // An objective cutoff for the dual loop, off by default, in the units of relp_result.objective (the fixed cost included).  The switch
    // holds until changed and is read by every start, the stepwise ones included.  On, the leave kernel stops the chain with ST_CUTOFF at
    // the first basis whose objective has reached the cutoff (iterate_dual: stop reason 6; run_dual: RELP_RESULT_CUTOFF), and a
    // solve_dual* that ends there, or at the iteration limit of the dual loop, reports the f64 objective of that basis and -- with
    // relp_options.certify set -- proves it as a lower bound of the LP (certify.hpp: certify_dual_bound).
    void set_dual_cutoff(bool on, double cutoff) { dual_cutoff_on_ = on; dual_cutoff_ = cutoff; }
    bool dual_cutoff_active() const { return dual_cutoff_active_; }  // the switch as the last start read it ...
    double dual_cutoff() const { return dual_cutoff_read_; }         // ... and its value
    bool dual_cutoff_stopped() const { return dual_cutoff_stopped_; }  // the loop since that start has stopped at the cutoff
    bool dual_bound_proved() const { return dual_bound_proved_; }      // the last solve_dual* ended with a proved lower bound
    long long dual_pivots() const { return dual_pivots_; }  // of the last solve_dual / since begin_dual
    // relp_options.dual_pricing = RELP_DUAL_PRICING_STEEPEST_EDGE: the m weights the next dual pivot would read (the squared row norms
    // of the inverse).  std::runtime_error under rule 0 and before a begin_dual.
    void dual_weights(double* out);
    // How the last begin_dual / begin_dual_from got its inverse ("none" before the first): "scratch", "inherited", or
    // "scratch_after_inherit" where the guard of an inherited inverse rebuilt it; the wall time of that call (the stream synchronised
    // at its end), the GEMMs of the polish and the from-scratch inverse inside it, and the guard's first residual (-1: no guard ran).
    const char* dual_start() const { return dual_start_; }
    double dual_start_seconds() const { return dual_start_seconds_; }
    long long dual_start_gemms() const { return dual_start_gemms_; }
    double dual_start_residual() const { return dual_start_residual_; }
    double dual_device_seconds() const { return dual_device_seconds_; }  // ... and the device time of their batches (stream events)

    // fine-grained ops (trait parity)
    void ftran(int nnz, const int* rows, const double* values, double* out);
    void btran(int nnz, const int* rows, const double* values, double* out);
    void inverse_row(int row, double* out);
    void price(int* column, double* cbar);
    void relative_costs(double* out);
    void get_gamma(double* out);
    void ratio(int column, int* row, double* alpha_out);
    void bring_into_basis(int column, int row);
    void after_basis_update();
    void solve_exact(int first_limbs, int max_limbs, long long max_pivots, int trace_capacity, int* status, int* limbs, long long* p1,
                     long long* p2, std::vector<int>* trace, std::string* objective, std::vector<int>* basis,
                     std::vector<std::pair<int, long long>>* survived, int* redundant_rows = nullptr);
    size_t device_bytes() const { return device_memory_.bytes(); }  // bytes this handle has allocated on the device
    bool network_carry() const { return path_.network; }
    const std::vector<unsigned long long>& network_stats() const { return net_stats_; }  // RELP_SW_NETWORK_STATS: NS_* of the last solve
    const std::vector<ExactWidthRecord>& exact_records() const { return exact_records_; }  // of the last solve_exact, one per width tried
    void last_pivot(int* phase, int* column, int* row, int* leaving);
    double refactor();
    void get_b(double* out);
    double objective();
    void get_basis(int* out);
    long long bound_flips();  // implicit bounds: Ctl::bound_flips since begin_phase_one
    void get_solution(double* x) const;
    double profile_kernel(int which, int repetitions);
    void debug_stamps(unsigned long long* out64);

    const StandardForm& form() const { return form_; }
    const DeviceLP& device() const { return d_; }
    const relp_stats& stats() const { return stats_; }
    void reset_stats();
    int n_art() const { return d_.n_art; }
    bool refactors_on_device() const { return path_.device_refactor; }
    long long device_refactor_fallbacks() const { return device_refactor_failures_; }
    bool refactors_asynchronously() const { return path_.async_refactor; }
    long long async_refactors() const { return async_refactors_; }
    long long async_refactors_abandoned() const { return async_abandoned_; }
    double async_worst_residual() const { return async_worst_residual_; }
    std::string exact_objective;  // filled by certify()
    // exact x_B of the certified optimal basis (certify.hip keeps the big integers; strings are made on demand)
    std::shared_ptr<const ExactPrimal> exact_primal;
    // x, y and the ray of the last certified verdict (certify_basis; none under RELP_CARRY_NETWORK, whose proof comes from the forest)
    std::shared_ptr<const ExactWitnesses> exact_witnesses;
    std::string last_error;
    relp_result last_result{};

private:
    // The constants of the loaded LP: which kernels it runs and how its arrays are sized (kernel_path.hpp).  Assigned once per load(),
    // at the top of upload(), before anything is allocated.
    KernelPath path_;
    void upload();                // plan, then one function per group of arrays (none of them decides anything)
    void upload_matrix();         // CSC / CSR, costs, right-hand side
    void upload_pricing_copy();   // ELL copy, generated columns, prw / rho_bits / rho_nz
    void upload_dense_block();    // one form per DenseStorage
    void allocate_pivot_state();  // vectors, candidate slots, eta buffers, touched lists, K2 partials, fused twin state, bounds, ctl
    void free_device();
    void set_phase(int phase);
    void launch_pivots(int count, bool forced = false);
    void enqueue_price_fused(int parity);
    void enqueue_pivot_fused(int parity);  // forced: the caller set forced_q / forced_p (three-kernel pivot)
    void enqueue_price(int skip_weights, bool first_of_batch = true);
    void enqueue_ftran_ratio(int mode);
    void enqueue_update();
    void enqueue_consolidate();
    void build_graph(int count);
    void polish(bool refresh_vectors, bool force = false);
    void invert_from_scratch();
    std::vector<int> explicit_basis(const std::vector<int>& basis, const std::vector<int>& pos) const;  // implicit bounds -> basis of the reference's formulation
    void resolve_fixed_columns(std::vector<int>& pos);
    std::vector<char> zero_width_;  // implicit bounds: device columns with upper bound 0 (fixed variables)
    void ensure_polish_buffers();  // second inverse + residual matrix, allocated when a polish first has something to correct
    Ctl read_ctl();                // an explicit copy of the device's control block into the pinned mirror, behind a stream synchronise
    Ctl read_ctl_after_batch();    // the same after a batch of pivots: the fused path's commit_kernel has written the mirror itself
    void write_ctl(const Ctl& c);
    // Pinned, host-mapped memory of the loaded LP (sized at load, freed with the device buffers): the mirror of the control block,
    // the block write_ctl copies out of (every write_ctl waits for the stream, so it is never reused before it has been consumed), and
    // the read-backs of a solve.  Read only behind a hipStreamSynchronize of stream_.
    PinnedAllocations pinned_memory_;
    Ctl* h_ctl_ = nullptr;
    Ctl* h_ctl_out_ = nullptr;
    int* h_rb_basis_ = nullptr;     // [m]
    double* h_rb_xb_ = nullptr;     // [m]
    int* h_rb_flipped_ = nullptr;   // [n] implicit bounds only, like the next two
    int* h_rb_pos_ = nullptr;       // [n]
    double* h_rb_ub_ = nullptr;     // [n]
    int drive_out_artificials();
    // The tail of a solve: read-backs, h_basis_, h_solution_, the objective and the exact certificate (`certify_verdicts`: of the
    // INFEASIBLE and UNBOUNDED verdicts too, where the options ask for one) into last_result and *result.
    void collect_result(int kind, double t0, bool certify_verdicts, const std::function<void(const char*)>& tick, relp_result* result);
    void certify(relp_result* result);
    // the dual loop (dual.hip)
    DualBuffers dual_;
    bool dual_lds_ = false;         // its row kernel stages rho and -pi in LDS (2 m doubles within relp_options.price_lds_max)
    bool dual_ready_ = false;       // begin_dual has run on the loaded LP
    bool last_pivot_dual_ = false;  // the last pivot was a dual one: last_pivot reports phase 3
    long long dual_pivots_ = 0;
    double dual_device_seconds_ = 0.0;
    void launch_dual_pivots(int count);
    bool steepest_dual() const { return opt_.dual_pricing == RELP_DUAL_PRICING_STEEPEST_EDGE; }
    void refresh_dual_weights();
    bool dual_weights_current_ = false;  // DualBuffers::beta holds the row norms of the inverse as it stands
    // set_basis in three parts, shared with begin_dual_from: basis, pos and the control block; (the inverse); the handle's counters
    void place_basis(const int* basis_columns);
    void reset_basis_counters();
    // the refusals every start shares: the plan (`bounded_entry`: dual_bounded_refusal instead of dual_refusal), an artificial in any row
    // of the basis as it is given (a bounded plan: every row of the formulation)
    void check_dual_start(const int* basis_columns, bool bounded_entry = false) const;
    void start_dual_from_scratch(const int* basis_columns, bool bounded_entry);  // begin_dual and begin_dual_bounded
    bool dual_bounded_ = false;
    bool dual_long_step_ = false;    // the switch
    bool dual_long_active_ = false;  // ... as the last start read it, on a plan with implicit bounds
    long long dual_flips_ = 0, dual_long_skipped_ = 0;
    int* h_flip_totals_ = nullptr;   // pinned: DualBuffers::flip_count[2..3] after a batch
    bool dual_farkas_ = false;         // the switch
    bool dual_farkas_active_ = false;  // ... as the last start read it
    int dual_farkas_row_ = -1;
    int dual_stopped_row();                            // the row at which the loop stands dual unbounded (one launch of the leaving-row kernel)
    void certify_dual_infeasible(relp_result* result);  // behind collect_result, which has read the basis and x_B back
    bool dual_cutoff_on_ = false;      // the switch and its value
    double dual_cutoff_ = 0.0;
    bool dual_cutoff_active_ = false;  // ... as the last start read them; the kernel gets dual_cutoff_read_ less the fixed cost
    double dual_cutoff_read_ = 0.0, dual_cutoff_carry_ = 0.0;
    bool dual_cutoff_stopped_ = false, dual_bound_proved_ = false;
    void certify_dual_lower_bound(relp_result* result);  // behind collect_result, like the one above: the bound of the basis the loop stopped on
    // ... and their tail behind set_phase(2): the loop's buffers, the dual-feasibility check that names the column, the counters
    void finish_dual_start(const int* basis_columns, const char* how, double t0, long long gemms_before);
    void run_dual(const Solver* parent, const int* basis_columns, relp_result* result, bool bounded_entry = false);  // every solve_dual*: one loop
    std::vector<int> provider_basis() const;  // the basis on the device, provider columns by position (plans without implicit bounds)
    const char* dual_start_ = "none";
    double dual_start_seconds_ = 0.0, dual_start_residual_ = -1.0;
    long long dual_start_gemms_ = 0;
    long long polish_gemms_ = 0;            // launch_gemm_polish calls of this handle (polish, invert_from_scratch)
    double polish_first_residual_ = -1.0;   // of the last polish that measured one: its first reading ...
    bool polish_rebuilt_ = false;           // ... and whether it gave up on the quadratic step and inverted from scratch
    hipEvent_t ev_parent_ = nullptr;        // begin_dual_from: recorded on the parent's stream, waited for on this one
    int* d_inherit_map_ = nullptr;          // begin_dual_bounded_from: [2 m] src | sg of dual_inherit_mapped_kernel, allocated by its first call
    long long dual_inherit_complemented_ = 0, dual_inherit_moved_ = 0;
    // the basis, pos and (a bounded plan: else zeros) flipped of the device state, read behind the handle's stream
    void held_state(std::vector<int>* basis, std::vector<int>* pos, std::vector<int>* flipped) const;
    std::vector<double> net_host_solve(const HostTree& t, bool transposed, const std::vector<double>& v) const;  // B^-1 v or v' B^-1
    CertifyScratch certify_scratch_;
    // spanning-forest carry (network_carry.hip)
    NetTree net_;
    void net_allocate();
    HostTree net_build(const std::vector<int>& basis, const std::vector<int>& flipped) const;  // throws unless the basis is a forest
    void net_upload(const HostTree& tree);
    HostTree net_download();
    void net_refresh(bool xb, bool pi);       // x_B and / or -pi (and the objective) recomputed from the forest on the device
    void net_gamma(const HostTree& tree, const std::vector<int>& pos, std::vector<double>* gamma) const;  // 1 + path length
    void net_set_gamma();                     // ... of every non-basic column, uploaded
    bool net_crash(const std::vector<int>& basis);
    void net_certify(relp_result* result);
    void net_enqueue_pivot(int mode, int parts = 3);  // entering column + tree path, ratio test (+ forest update in mode 0)
    std::vector<unsigned long long> net_stats_;
    DeviceAllocations device_memory_;  // every buffer of the loaded LP: d_, net_ (free_device)
    template <class T>
    T* device_alloc(size_t count) { return device_memory_.alloc<T>(count); }
    // LU carry (relp_options.carry == RELP_CARRY_LU)
    void refactor_lu(bool refresh_vectors, bool settle = true);  // BasisInverse::invert of the current basis: kernels on the device (lu_factor.hip), or ...
    void refactor_lu_host(bool refresh_vectors);  // ... host Markowitz + upload (relp_options.lu_refactor; the LU + Forrest-Tomlin carry; the fallback)
    std::vector<ExactWidthRecord> exact_records_;
    long long device_refactor_failures_ = 0;
    void lu_identity();                      // BasisInverse::identity
    LuFactors lu_sets_[2];  // (two sets of factor arrays: the asynchronous refactorisation builds the next factors in the other one)
    int lu_cur_ = 0;
    LuFactors& lu() { return lu_sets_[lu_cur_]; }
    const LuFactors& lu() const { return lu_sets_[lu_cur_]; }
    // the refactorisation beside the pivots (relp_options.lu_refactor = RELP_REFACTOR_DEVICE_ASYNC; solver.hip: start_async_refactor)
    bool async_in_flight_ = false;
    hipStream_t refactor_stream_ = nullptr;
    hipEvent_t ev_snapshot_ = nullptr, ev_refactored_ = nullptr;
    long long async_iters_at_snapshot_ = 0;
    int* d_basis_snapshot_ = nullptr;
    double* d_probe_ = nullptr;          // [2 m + 2] the swap guard's probe vector, its image, the residual
    double async_worst_residual_ = 0.0;
    unsigned char* d_flipped_snapshot_ = nullptr;
    long long async_refactors_ = 0, async_abandoned_ = 0;
    void start_async_refactor(long long iters_now);
    void abandon_async_flight();
    bool finish_async_refactor(long long iters_now);  // true: the handle now runs on the new factors
    bool lu_is_identity_ = true;
    // (a negative slack selects the reference's ratio test in the kernels that implement it: the fused kernel for m <= 8192 and the LU kernel)
    double ratio_delta() const { return path_.ratio_textbook ? -1.0 : opt_.harris_delta; }
    int unbounded_column_ = -1;  // provider column of the ray when the result is UNBOUNDED
    long long refactors_ = 0;
    double refactor_seconds_ = 0.0;
    DeviceColumns cols_;  // index space of the loaded LP
    DeviceMatrix host_;   // host copy of the device CSC and right-hand side, kept where the host reads them (the refactorisation's basis columns, the forest, the crash basis)
    std::vector<int> h_row_start_, h_col_index_;  // the same matrix by rows (kept for the crash basis)
    bool crash_basis();           // relp_options.crash: triangular crash basis as the start of phase one
    bool gamma_ready_ = false;    // the next set_phase keeps the uploaded steepest-edge weights
    int crash_rows_covered_ = 0;

    relp_options opt_;
    StandardForm form_;
    DeviceLP d_;
    bool loaded_ = false;
    bool binv_identity_ = true;
    int phase_ = 0;
    hipStream_t stream_ = nullptr;
    // one captured batch of pivots per phase (the phases differ in a kernel argument); both survive across solves of the
    // same LP, so a solve pays for no capture or instantiation after the first
    hipGraph_t graph_[4] = {nullptr, nullptr, nullptr, nullptr};      // [phase + 2 * set of LU factors]
    hipGraphExec_t graph_exec_[4] = {nullptr, nullptr, nullptr, nullptr};
    int graph_count_[4] = {0, 0, 0, 0};
    int graph_index() const { return (phase_ == 2 ? 1 : 0) + 2 * lu_cur_; }
    void destroy_graphs();
    hipEvent_t ev_a_ = nullptr, ev_b_ = nullptr;
    relp_stats stats_{};
    std::vector<double> h_solution_;
    std::vector<int> h_basis_;
    std::vector<int> redundant_rows_;
    long long pivots_[2] = {0, 0};
    long long polishes_ = 0;
    double max_residual_ = 0.0;
    long long since_polish_ = 0;
    int polish_scale_ = 1;        // multiplier of polish_period, adapted to the drift measured at each polish
};

}  // namespace relp
