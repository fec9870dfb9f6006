/*
 * relp_amd -- C ABI of the MI355X-native revised-simplex hot path (drop-in boundary).
 *
 * The reference (vandenheuvel/relp, Rust) has no FFI today; its plug-in surface for this path is four generic
 * traits.  Each entry point below names the reference interface it replaces; paths are
 * relative to /root/reference/src/algorithm/two_phase/.  A Rust shim that binds these is shown in INTEGRATION.md.
 *
 * Conventions: every call returns a relp_status (0 = ok); arrays are caller-owned; indices are 0-based;
 * a handle is confined to one host thread and owns one HIP stream on one device; distinct handles are independent.
 * Provider column indices are the reference's `MatrixData` indices (matrix_data.rs:115-145): structural columns
 * first, then the five virtual slack groups.  Exact values cross the boundary as (numerator, denominator) pairs of
 * int64 -- the reference's `Rational64` input type (io/mps/number/parse.rs:46-65).
 */
#ifndef RELP_AMD_H
#define RELP_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct relp_handle relp_handle;

typedef enum relp_status {
    RELP_OK = 0,
    RELP_ERR_ARGUMENT = 1,      /* bad pointer / size / index */
    RELP_ERR_PARSE = 2,         /* io::error::{Parse, Inconsistency} (src/io/error.rs:15-237) */
    RELP_ERR_DEVICE = 3,        /* no HIP device or a HIP call failed: the product has NO CPU fallback */
    RELP_ERR_OVERFLOW = 4,      /* fixed-width exact arithmetic overflowed */
    RELP_ERR_STATE = 5,         /* call out of order (e.g. solve before load) */
    RELP_ERR_NUMERICAL = 6      /* f64 breakdown that polishing could not repair */
} relp_status;

/* algorithm/mod.rs:43-47 `OptimizationResult` plus the states a library must report instead of panicking. */
typedef enum relp_result_kind {
    RELP_RESULT_NONE = 0,
    RELP_RESULT_FINITE_OPTIMUM = 1,
    RELP_RESULT_INFEASIBLE = 2,
    RELP_RESULT_UNBOUNDED = 3,
    RELP_RESULT_ITERATION_LIMIT = 4,
    RELP_RESULT_CUTOFF = 5      /* relp_set_dual_cutoff only: the dual loop stopped at a basis whose objective has reached the cutoff */
} relp_result_kind;

/* strategy/pivot_rule.rs:86-305: the four `PivotRule` implementations. */
typedef enum relp_pivot_rule {
    RELP_PIVOT_STEEPEST_EDGE = 0,          /* SteepestDescentAlongObjective (the reference's hard-wired default) */
    RELP_PIVOT_DANTZIG = 1,                /* SteepestDescentAlongVariable */
    RELP_PIVOT_FIRST_PROFITABLE = 2,       /* FirstProfitable */
    RELP_PIVOT_FIRST_PROFITABLE_MEMORY = 3 /* FirstProfitableWithMemory */
} relp_pivot_rule;

/* The two `BasisInverse` implementations of the reference (carry/mod.rs:69-169), both resident on the device. */
typedef enum relp_carry {
    RELP_CARRY_EXPLICIT = 0,   /* `BasisInverseRows` (carry/basis_inverse_rows.rs:21-229): explicit inverse, product-form update */
    RELP_CARRY_LU = 1,         /* `LUDecomposition` (carry/lower_upper/mod.rs:36-272): P B Q = L U, Forrest-Tomlin updates,
                                  refactorisation every `refactor_period` updates */
    RELP_CARRY_LU_INVERSE = 2, /* the same factorisation (`LUDecomposition::invert`, lower_upper/mod.rs:78-92, at every
                                  refactorisation) applied through the sparse INVERSES of its two triangles: FTRAN / BTRAN
                                  (mod.rs:180-237) are two sparse matrix-vector products each instead of two level-by-level
                                  triangular solves, and the basis changes between refactorisations are kept in product form on
                                  top (the etas of `BasisInverseRows`, basis_inverse_rows.rs:96-135, as at most `refactor_period`
                                  columns) instead of Forrest-Tomlin row etas.  At most about 5800 rows (four vectors in LDS up to
                                  about 4300 rows, three beyond). */
    RELP_CARRY_NETWORK = 3     /* network LPs only (the graph providers, examples/max_flow.rs and examples/shortest_path.rs):
                                  the basis is kept as a spanning forest of the rows, O(m) memory, no m x m array.  FTRAN is
                                  the tree path of the entering arc, row p of the inverse the subtree the leaving arc cuts off.
                                  Accepts a device LP (after implicit bounds are taken out) whose every column has at most two
                                  entries, each +-1, of opposite signs when there are two; anything else fails to load with
                                  RELP_ERR_ARGUMENT naming the first such column (the max-flow provider needs implicit_bounds).
                                  The certificate (certify) is proved from the tree for finite optima; INFEASIBLE and
                                  UNBOUNDED results stay uncertified under this carry. */
} relp_carry;

/* `Tableau::select_primal_pivot_row` (tableau/mod.rs:287-313). */
typedef enum relp_ratio_rule {
    RELP_RATIO_HARRIS = 0,     /* two-pass Harris test with slack `harris_delta`, largest pivot among the near-ties (what f64
                                  needs on real data), ties to the lowest leaving column */
    RELP_RATIO_TEXTBOOK = 1,   /* the reference's rule: the exact minimum ratio, ties to the lowest leaving column (Bland).  For
                                  data on which f64 is exact (small integers); rows <= 8192 (RELP_ERR_ARGUMENT at load beyond:
                                  the multi-workgroup ratio test implements the two-pass rule only), any number of rows
                                  under RELP_CARRY_NETWORK */
    RELP_RATIO_AUTO = 2        /* the default since round 6 ("defaults reproduce the reference"): the
                                  reference's rule where the data are small integers -- every matrix entry an integer of at most
                                  64 in magnitude, every cost and right-hand side an integer below 2^20 -- and the LP has at most
                                  8192 rows (any number under RELP_CARRY_NETWORK); the two-pass Harris test otherwise (decimal data: Netlib).  The per-LP record
                                  (relp_get_record_json) says which one ran */
} relp_ratio_rule;

/* Storage type of a dense column block (`relp_options.dense_storage`). */
typedef enum relp_dense_storage {
    RELP_DENSE_NARROWEST = 0,  /* the narrowest type that holds every entry exactly: signed bytes, else float, else double */
    RELP_DENSE_FLOAT = 1,      /* float when every entry is exactly representable, else double */
    RELP_DENSE_DOUBLE = 2      /* double (SURVEY.md section 8(d)'s 8 bytes per entry) */
} relp_dense_storage;

/* Where the LU carries refactorise (`relp_options.lu_refactor`). */
typedef enum relp_lu_refactor {
    RELP_REFACTOR_AUTO = 0,    /* the faster of the two at the sizes measured so far: today the host path for every shipped LP
                                  (DESIGN.md section 2d has the table: the kernels are 7-25 % behind the host path per pivot) */
    RELP_REFACTOR_DEVICE = 1,  /* kernels on the handle's stream (lu_factor.hip, lu_device_tasks.hip): Markowitz factorisation with
                                  independent pivots per round, inversion of the two triangles, slot records -- no basis read-back, no
                                  upload; RELP_CARRY_LU_INVERSE only (the Forrest-Tomlin carry factorises on the host); what the
                                  kernels cannot take (a row of more than 256 entries, a capacity) falls back to the host path */
    RELP_REFACTOR_HOST = 2,    /* one host core: Markowitz + inversion + task lists, one upload (rounds 2-3) */
    RELP_REFACTOR_DEVICE_ASYNC = 3  /* round 5: the same kernels on a SECOND stream, into a second set of factor arrays, while the
                                  pivots go on with the old factors: the pivot kernel logs the row factors of its etas from the
                                  moment the basis is snapshotted, and when the new factors are ready a replay kernel folds the
                                  logged etas (at most 40) into their product form -- B_now^-1 = E_k ... E_1 B_snapshot^-1 -- and the
                                  handle swaps sets.  RELP_CARRY_LU_INVERSE with its four vectors in LDS (m <= ~4300); anything
                                  else, and any refactorisation the kernels give up on, takes the synchronous paths above */
} relp_lu_refactor;

/* The leaving row of a dual pivot (relp_amd/csrc/dual.hip), among the rows with x_B[i] < -harris_delta; ties go to the lowest basic
 * column, then the lowest row, under both rules. */
typedef enum relp_dual_pricing {
    RELP_DUAL_PRICING_INFEASIBILITY = 0,  /* the largest -x_B[i] (the default) */
    RELP_DUAL_PRICING_STEEPEST_EDGE = 1   /* the largest x_B[i]^2 / beta_i, beta_i = |e_i' B^-1|^2 the squared norm of row i of the
                                             inverse, recomputed from the inverse after every dual pivot (relp_get_dual_weights) */
} relp_dual_pricing;

/* A/B switches of the kernels (`relp_options.switches`; tests and measurements -- all clear = what the library would choose).
 * Round 5: these were environment variables of the same names (RELP_NO_TOUCHED ...); the library no longer reads the environment
 * for anything that changes a kernel or a result, so a caller's options cannot be overruled from outside. */
typedef enum relp_switch {
    RELP_SW_NO_TOUCHED = 1 << 0,            /* no bookkeeping of the non-unit columns of the inverse (m > 2048) */
    RELP_SW_K2_SINGLE = 1 << 1,             /* the one-workgroup ratio test beyond 8192 rows as well */
    RELP_SW_ELL_WIDE = 1 << 2,              /* graph LPs: the 8-wide padded copy of the columns */
    RELP_SW_NO_GENERATED_COLUMNS = 1 << 3,  /* graph LPs: materialised instead of generated incidence columns */
    RELP_SW_NO_SLACK_IN_BTRAN = 1 << 4,     /* dense pipeline: slack columns priced by a launch of their own */
    RELP_SW_NO_DENSE_LANE = 1 << 5,         /* dense block priced by one wave per column instead of a column per lane */
    RELP_SW_POLISH_ALWAYS = 1 << 6,         /* polish at every opportunity */
    RELP_SW_NO_RHO_BITS = 1 << 7,           /* generated columns: no bit table of rho_p's rows */
    RELP_SW_PRICE_UNIT_PAIRS = 1 << 8,      /* generated columns: the pair-per-lane pricing kernel */
    RELP_SW_CERTIFY_NO_LEVELS = 1 << 9,     /* exact certificate: modular inverse without level scheduling */
    RELP_SW_GEMM_VECTOR = 1 << 10,          /* polish: the plain-FMA GEMM instead of v_mfma_f64_16x16x4_f64 */
    RELP_SW_LUF_CLAIM_TARGETS = 1 << 11,    /* device refactorisation: target rows claimed from a counter */
    RELP_SW_LUF_NO_LDS_ARENA = 1 << 12,     /* ... the active sub-matrix in global memory throughout */
    RELP_SW_LUI_CLAIM_ROWS = 1 << 13,       /* ... inversion of the triangles: rows claimed from a counter */
    RELP_SW_BI_FACTOR_HOST = 1 << 14,       /* stand-alone BasisInverse: `invert` on a host core */
    RELP_SW_NETWORK_STATS = 1 << 15,        /* RELP_CARRY_NETWORK: count row depths, subtree and path sizes at every pivot (the record's
                                               "network_tree"; a diagnostic, it costs atomics in the forest update) */
    RELP_SW_MANY_GLOBAL_TIER = 1 << 16      /* relp_many: every LP keeps its inverse in global memory, also where it fits LDS (test hook) */
} relp_switch;

typedef struct relp_options {
    int32_t struct_size;       /* sizeof(relp_options) as the CALLER compiled it; relp_options_default() -- through the header's
                                  macro relp_options_default_sized(o, sizeof(relp_options)) -- sets it and is the only supported
                                  way to initialise the struct.  relp_create / relp_batch_create read that many bytes and take the
                                  defaults for the fields a caller built against an older header does not have; anything but
                                  a size this struct has had in some round is RELP_ERR_ARGUMENT */
    int32_t device;            /* HIP device ordinal */
    int32_t pivot_rule;        /* relp_pivot_rule */
    int32_t polish_period;     /* pivots between Newton-Schulz polishes of the explicit inverse (role of
                                  BasisInverse::should_refactor, lower_upper/mod.rs:249-252) */
    int32_t pivots_per_launch; /* pivots enqueued per host round trip (hipGraph replay length) */
    int64_t max_pivots;        /* iteration cap (the reference has none; cycling is acknowledged, tests/netlib/test.rs:221);
                                  0 = 200 (m + n) + 100 000, after which the result is RELP_RESULT_ITERATION_LIMIT */
    double tol_dual;           /* cbar_j < -tol_dual makes j a pricing candidate */
    double tol_pivot;          /* alpha_i > tol_pivot takes part in the ratio test */
    double harris_delta;       /* feasibility slack of the two-pass ratio test */
    double tol_feasible;       /* phase-one objective above tol_feasible*(1+|b|_1) => infeasible */
    int32_t certify;           /* 1: after the f64 solve, prove the basis optimal in exact arithmetic and return the
                                  exact rational objective (bit-exact with the reference's RationalBig optimum) */
    int32_t use_graph;         /* 1: replay the pivot loop from a hipGraph */
    int32_t verbose;
    int32_t implicit_bounds;   /* 1: variable upper bounds (MatrixData's VariableBound / SlackBound rows, matrix_data.rs:104-112)
                                  are handled by the bounded-variable ratio test instead of as rows: same optimum, fewer rows.
                                  relp_get_basis / relp_set_basis keep speaking the reference's formulation (one column per
                                  row of MatrixData, bound rows included); the other fine-grained trait operations refer to
                                  the reduced LP */
    int32_t carry;             /* relp_carry: which `BasisInverse` the loop maintains (the `BI` of `Carry<F, BI>`,
                                  tests/netlib/mod.rs:62) */
    int32_t refactor_period;   /* LU carry: Forrest-Tomlin updates between refactorisations (`should_refactor`,
                                  lower_upper/mod.rs:249-252: the reference refactors after 31); at most 63; 0 = the default:
                                  31, and 47 product-form updates for RELP_CARRY_LU_INVERSE */
    double lu_pivot_threshold; /* LU carry: relative pivot tolerance of the Markowitz factorisation (f64 needs one, the exact
                                  reference does not); 0 = 0.1 */
    int32_t ratio_rule;        /* relp_ratio_rule */
    int32_t crash;             /* 1: phase one starts from a triangular crash basis instead of one artificial per row without a
                                  slack pivot (an extension; the reference has none, kind/artificial/partially.rs:125-205):
                                  columns with a single entry in the rows still on an artificial are assigned breadth first
                                  -- a spanning forest on the graph providers -- and the crash is kept when it is primal
                                  feasible.  Same optimum, different (much shorter) pivot sequence; explicit carry only */
    /* ---- appended in round 4: what was reachable only through the environment before ---- */
    int32_t dense_storage;     /* relp_dense_storage: storage type of a dense column block (relp_load_dense_le; BASELINE config 3
                                  names the f64 block) */
    int32_t pivot_kernels;     /* 0 = automatic (ratio test and inverse update fused into one launch for m <= 2048, explicit
                                  carry), 1 = the three separate kernels (bit-identical results) */
    int32_t product_form;      /* dense pipeline: 0 = automatic (updates deferred in product form, one rank-k update every 32
                                  pivots), 1 = a rank-one update of the stored inverse per pivot */
    int32_t ftran_min_nnz;     /* columns longer than this take the multi-block FTRAN pipeline; 0 = 1024 */
    int32_t lu_refactor;       /* relp_lu_refactor: where `BasisInverse::invert` of the LU carries runs (lower_upper/mod.rs:78-92,
                                  decomposition/mod.rs:27-143) */
    /* ---- appended in round 5: the remaining A/B hooks (0 = the library's choice everywhere) ---- */
    uint32_t switches;         /* relp_switch bits */
    int32_t dense_blocks;      /* workgroups of the one-wave-per-column dense pricing kernel (256) */
    int32_t ftran_slices;      /* slices of the multi-block FTRAN (by the longest column, at most 64) */
    int32_t price_lds_max;     /* pricing stages -pi / rho / w in LDS up to this many bytes of the three vectors (96 KB) */
    int32_t certify_threads;   /* host threads of the exact certificate (by the core count, at most 32) */
    int32_t exact_grid;        /* relp_solve_exact: workgroups of the cooperative launch (by the work of a pivot) */
    int32_t exact_update;      /* relp_solve_exact, bits: 1 = the update of N = D B^-1 on the vector unit only (default: on the matrix
                                  cores from 16 limbs on); 4 = the update on the matrix cores in the two passes of round 5 (numerators,
                                  then carries / shift / sign by a thread per entry; default since round 6: the tiles finish their
                                  entries themselves into a second buffer of N); 2 = the pricing pass forms the products N a_j of every column that can enter
                                  exactly (default: weight estimates from the leading words, exact only where their error bound asks) */
    int32_t luf_dense_tail;    /* device refactorisation: rows of the dense tail (8); -1 = none */
    int32_t luf_slack;         /* ... Markowitz score slack of a round (16) */
    int32_t luf_lds;           /* ... 1 + the LDS level forced (1: every work array in global memory) */
    int32_t luf_lds_arena;     /* ... cap on the entries of the active sub-matrix held in LDS (test hook: spills) */
    int32_t luf_arena_cap;     /* ... cap on the words of the global arena (test hook: a basis that outgrows it) */
    double carry_weights_min;  /* steepest-edge weights carried from phase one into phase two from this many columns (4e9) */
    /* ---- appended in round 7: the leaving-row rule of the dual loop ---- */
    int32_t dual_pricing;      /* relp_dual_pricing; any other value is RELP_ERR_ARGUMENT at relp_create */
    int32_t reserved_round7;   /* must be 0 (keeps the struct a multiple of 8 bytes without tail padding) */
} relp_options;

typedef struct relp_result {
    int32_t kind;              /* relp_result_kind */
    int32_t certified;         /* 1 when the exact certificate holds */
    int64_t pivots_phase_one;  /* bring_into_basis calls: phase_one.rs:145,265 */
    int64_t pivots_phase_two;  /* phase_two.rs:47 */
    int64_t polishes;
    int64_t exact_repair_pivots;
    double objective;          /* f64 objective incl. fixed cost (general_form/mod.rs:840-851) */
    double solve_seconds;      /* wall clock of solve_relaxation only (device-resident in, result out) */
    double certify_seconds;
    double max_residual;       /* largest |I - B Binv| entry seen by a polish */
    int64_t refactors;         /* LU carry: refactorisations (`BasisInverse::invert`) made, and the host time they took */
    double refactor_seconds;
} relp_result;

typedef struct relp_stats {
    int64_t launches;          /* kernel launches issued */
    int64_t price_launches;
    double price_seconds;      /* HIP-event time spent in the pricing kernel (the dominant kernel), see bench.py */
    double update_seconds;
    double ftran_seconds;
    int64_t price_bytes;       /* algorithmic bytes of one pricing launch */
    int64_t update_bytes;
} relp_stats;

/* The defaults, written into a struct of `caller_size` bytes -- sizeof(relp_options) as the CALLER compiled it: not a byte more is
 * touched, and struct_size is set to that size, so a program built against an older, shorter header keeps working with a newer
 * library (relp_create / relp_batch_create read struct_size bytes and take the defaults for the rest).  The only supported
 * initialiser; a size no header of this library ever had is RELP_ERR_ARGUMENT.  Bindings by symbol (ctypes, Rust `extern`)
 * call this one with their own struct's size. */
int32_t relp_options_default_sized(relp_options* options, int32_t caller_size);
/* The exported symbol of rounds 1-5: assumes the LIBRARY's sizeof(relp_options) -- right only for a caller built against the header the
 * library was built with.  C and C++ callers get the sized call through the macro below without changing a line. */
int32_t relp_options_default(relp_options* options);
#define relp_options_default(options) relp_options_default_sized((options), (int32_t)sizeof(relp_options))

/* ---- host-only model: the provider without a device (usable on a machine with no GPU) ------------------------
 * `relp_model` is the `MatrixData` a provider call sequence would see; it needs no HIP device, so the host logic
 * (parser, standardisation, virtual slack columns) is testable on CPU.  relp_load_model uploads it to a handle. */
typedef struct relp_model relp_model;
int32_t relp_model_from_mps(const char* path, int32_t fixed_format, relp_model** out, char* error, int32_t error_capacity);
/* The same with `GeneralForm::presolve` (general_form/mod.rs:335-358 and general_form/presolve/ of the reference: fixed
 * variables, bound constraints, slack elimination, domain propagation) applied before `standardize()`, as the reference's
 * Netlib harness does (tests/netlib/mod.rs:58).  RELP_ERR_STATE when the presolve itself proves the problem infeasible,
 * unbounded or solves it completely (message in `error`).  The presolve computes in arbitrary precision, the host model is
 * 128-bit rationals: when a presolved value does not fit, the presolve is run again without the implied bounds that need
 * more than 126 (then 60) bits, and only if that fails as well is the LP loaded as the file states it -- never
 * RELP_ERR_OVERFLOW because of the presolve (relp_get_record_json reports the level). */
int32_t relp_model_from_mps_ex(const char* path, int32_t fixed_format, int32_t presolve, relp_model** out, char* error,
                               int32_t error_capacity);
/* The provider of a caller that builds the general form itself: `GeneralForm::new` (general_form/mod.rs:211-237) followed by
 * [`presolve` :335-463 ->] `standardize` (:325-332: split free variables, flip and shift to x >= 0 :506-587, b >= 0 :592-618,
 * minimise :623-633, rows ordered E | R | <= | >= :651-717) -> `derive_matrix_data` (:262-304).
 *   columns: CSC with ascending row indices and no explicit zeros, exact rationals value_num/value_den;
 *   row_kind[i]: 0 Equal, 1 Range (b_i - range_i <= a_i x <= b_i, range_i >= 0), 2 Less, 3 Greater
 *                (`RangedConstraintRelation`, data/linear_program/elements.rs); range_* is read for Range rows only;
 *   variable j: cost, optional lower / upper bound (`Variable`, general_form/mod.rs:140-165; shift 0, not flipped);
 *   variables are named X0, X1, ... ; relp_get_original_solution returns their values in this order. */
int32_t relp_model_from_general_form(int32_t maximize, int32_t nr_rows, int32_t nr_columns, const int64_t* column_start,
                                     const int32_t* row_index, const int64_t* value_num, const int64_t* value_den,
                                     const int32_t* row_kind, const int64_t* range_num, const int64_t* range_den,
                                     const int64_t* b_num, const int64_t* b_den, const int64_t* cost_num, const int64_t* cost_den,
                                     const uint8_t* has_lower, const int64_t* lower_num, const int64_t* lower_den,
                                     const uint8_t* has_upper, const int64_t* upper_num, const int64_t* upper_den,
                                     int64_t fixed_cost_num, int64_t fixed_cost_den, int32_t presolve, relp_model** out,
                                     char* error, int32_t error_capacity);
/* Any other `MatrixProvider` (matrix_provider/mod.rs:37-134), through the calls the reference's loops make on it: the host
 * pulls every column once (the device keeps them resident; the reference generates columns lazily per pivot).
 *   column(j): `MatrixProvider::column` -- writes at most `capacity` (row, num/den) entries, ascending rows, no zeros, and
 *              returns the number of non-zeros of the column (called again with a larger buffer if that exceeds capacity);
 *   cost_value(j): `MatrixProvider::cost_value`;  right_hand_side: `MatrixProvider::right_hand_side`, nr_rows values >= 0;
 *   pivot_element_indices: `PartialInitialBasis::pivot_element_indices` (matrix_provider/mod.rs) -- (row, column) pairs whose
 *              column is the unit vector of that row; NULL, or a count of 0, for a provider without an initial basis (phase one
 *              then starts fully artificial: `Tableau::new` over `Fully`, tableau/kind/artificial/fully.rs).
 * Variable bounds are rows of such a provider (as in examples/max_flow.rs); `implicit_bounds` has nothing to take out. */
typedef struct relp_provider {
    void* user;
    int32_t nr_rows, nr_columns;
    int32_t (*column)(void* user, int32_t j, int32_t capacity, int32_t* row, int64_t* num, int64_t* den);
    void (*cost_value)(void* user, int32_t j, int64_t* num, int64_t* den);
    void (*right_hand_side)(void* user, int64_t* num, int64_t* den);
    int32_t (*pivot_element_indices)(void* user, int32_t capacity, int32_t* rows, int32_t* columns);
} relp_provider;
int32_t relp_model_from_provider(const relp_provider* provider, relp_model** out, char* error, int32_t error_capacity);
/* Number of variables of the file and how many of them the presolve removed (0 without presolve). */
int32_t relp_model_original_variables(const relp_model* model, int32_t* nr_original, int32_t* nr_removed);
/* Graph providers (reference: examples/max_flow.rs:31-223 `Primal::new` + its MatrixProvider; examples/shortest_path.rs:20-118;
 * incidence matrix data/linear_program/network/representation.rs:24-100).  Arcs in the order the reference's column-major
 * adjacency matrix enumerates them: sorted by (tail, head), no self arcs.  `value` = capacity (max flow: arc j gets the
 * bound row V-2+j and the slack column E+j, initial pivots (V-2+j, E+j)) or length (shortest path: row of s removed,
 * b = e_t).  RELP_ERR_ARGUMENT for unsorted / duplicate / self arcs or bad terminals. */
int32_t relp_model_max_flow(int32_t nr_vertices, int32_t nr_arcs, const int32_t* tail, const int32_t* head,
                            const int64_t* capacity_num, const int64_t* capacity_den, int32_t s, int32_t t,
                            relp_model** out, char* error, int32_t error_capacity);
int32_t relp_model_shortest_path(int32_t nr_vertices, int32_t nr_arcs, const int32_t* tail, const int32_t* head,
                                 const int64_t* length_num, const int64_t* length_den, int32_t s, int32_t t,
                                 relp_model** out, char* error, int32_t error_capacity);
int32_t relp_model_free(relp_model* model);
int32_t relp_model_dimensions(const relp_model* model, int32_t* nr_rows, int32_t* nr_columns, int32_t* nr_constraints,
                              int32_t* nr_structural, int64_t* nnz, int32_t group_counts[4]);
int32_t relp_model_column(const relp_model* model, int32_t j, int32_t capacity, int32_t* count,
                          int32_t* row_index, double* value);
/* exact form of one column: values as decimal strings "num/den" joined by ';' are avoided -- int64 pairs instead;
 * returns RELP_ERR_OVERFLOW when a value does not fit int64. */
int32_t relp_model_column_exact(const relp_model* model, int32_t j, int32_t capacity, int32_t* count,
                                int32_t* row_index, int64_t* num, int64_t* den);
int32_t relp_model_cost(const relp_model* model, int32_t j, double* cost);
int32_t relp_model_right_hand_side(const relp_model* model, double* rhs);
int32_t relp_model_initial_pivots(const relp_model* model, int32_t capacity, int32_t* count, int32_t* rows, int32_t* columns);
int32_t relp_model_fixed_cost(const relp_model* model, double* fixed_cost);
/* exact forms of cost_value(j), right_hand_side() (nr_rows pairs) and the fixed cost, as relp_model_column_exact gives a column:
 * int64 pairs num/den (reduced, den > 0), RELP_ERR_OVERFLOW when a value does not fit int64.  With relp_model_column_exact they
 * are all a caller needs to check a witness of relp_get_witness_exact without parsing the file again. */
int32_t relp_model_cost_exact(const relp_model* model, int32_t j, int64_t* num, int64_t* den);
int32_t relp_model_right_hand_side_exact(const relp_model* model, int64_t* num, int64_t* den);
int32_t relp_model_fixed_cost_exact(const relp_model* model, int64_t* num, int64_t* den);

/* Lifetime.  relp_create fails with RELP_ERR_DEVICE when no MI355X/HIP device is usable. */
int32_t relp_create(const relp_options* options, relp_handle** out);
int32_t relp_destroy(relp_handle* handle);
const char* relp_last_error(const relp_handle* handle);

/* ---- provider: replaces `MatrixData::new` (matrix_provider/matrix_data.rs:172-248) -------------------------
 * constraints: CSC over the constraint rows (sorted rows per column, no zeros), values num/den;
 * b: one per constraint row (>= 0); ranges: one per range row; upper_*: per variable, has_upper[j] != 0 adds a
 * virtual bound row + slack.  Row order must be Equality | Range | <= | >= (general_form/mod.rs:651-717). */
int32_t relp_load_matrix_data(relp_handle* handle,
                              int32_t nr_constraints, int32_t nr_variables,
                              const int64_t* column_start, const int32_t* row_index,
                              const int64_t* value_num, const int64_t* value_den,
                              const int64_t* b_num, const int64_t* b_den,
                              const int64_t* cost_num, const int64_t* cost_den,
                              const uint8_t* has_upper, const int64_t* upper_num, const int64_t* upper_den,
                              const int64_t* range_num, const int64_t* range_den,
                              int32_t nr_equality, int32_t nr_range, int32_t nr_upper, int32_t nr_lower,
                              int64_t fixed_cost_num, int64_t fixed_cost_den);

/* Dense provider `A x <= b, x >= 0, b >= 0` with integer data (column-major A, m x n): every row has its slack as an
 * initial pivot, i.e. the `FullInitialBasis` route of two_phase/mod.rs:80-109 (no phase one).  BASELINE config 3. */
int32_t relp_load_dense_le(relp_handle* handle, int32_t m, int32_t n, const int64_t* a_column_major,
                           const int64_t* b, const int64_t* cost);

/* Convenience for the step before the path: `parse_fixed`/`parse_free` + `TryInto<GeneralForm>` +
 * `standardize()` + `derive_matrix_data()` (tests/netlib/mod.rs:55-61, without presolve). */
int32_t relp_load_mps(relp_handle* handle, const char* path, int32_t fixed_format);
int32_t relp_load_mps_ex(relp_handle* handle, const char* path, int32_t fixed_format, int32_t presolve);
int32_t relp_load_model(relp_handle* handle, const relp_model* model);

/* `MatrixProvider::{nr_rows, nr_columns, nr_constraints, nr_variable_bounds}` (matrix_provider/mod.rs:37-134). */
int32_t relp_get_dimensions(const relp_handle* handle, int32_t* nr_rows, int32_t* nr_columns,
                            int32_t* nr_constraints, int32_t* nr_structural, int32_t* nr_artificial, int64_t* nnz);
/* `MatrixProvider::column(j)`; returns nnz through *count (capacity entries are written at most). */
int32_t relp_get_column(const relp_handle* handle, int32_t j, int32_t capacity, int32_t* count,
                        int32_t* row_index, double* value);
int32_t relp_get_cost(const relp_handle* handle, int32_t j, double* cost);            /* cost_value(j) */
int32_t relp_get_right_hand_side(const relp_handle* handle, double* rhs);             /* right_hand_side() */
int32_t relp_get_initial_pivots(const relp_handle* handle, int32_t capacity, int32_t* count,
                                int32_t* rows, int32_t* columns);                      /* pivot_element_indices() */

/* ---- `SolveRelaxation::solve_relaxation::<Carry<_, _>>()` (algorithm/mod.rs:17-36, two_phase/mod.rs:25-109) -- */
int32_t relp_solve_relaxation(relp_handle* handle, relp_result* result);
/* OptimizationResult::FiniteOptimum(x) after `reconstruct_solution` (matrix_data.rs:402-411): structural columns. */
int32_t relp_get_solution(const relp_handle* handle, double* x_structural);
/* Values of the variables of the loaded file, in file order: un-shifted, un-flipped, free variables recombined and the
 * variables a presolve removed evaluated (`GeneralForm::compute_full_solution_with_reduced_solution`,
 * general_form/mod.rs:753-771, 840-934).  `count` receives their number; RELP_ERR_ARGUMENT if capacity is too small. */
int32_t relp_get_original_solution(const relp_handle* handle, int32_t capacity, double* x, int32_t* count);
/* Exact optimal objective "num/den" incl. fixed cost (needs options.certify); returns needed length in *length. */
int32_t relp_get_objective_exact(const relp_handle* handle, char* buffer, int32_t capacity, int32_t* length);
/* `OptimizationResult::FiniteOptimum(SparseVector<RationalBig>)` (algorithm/mod.rs:43-47) in EXACT form, from the certificate's
 * solve of B x_B = b (needs options.certify and a certified finite optimum; RELP_ERR_STATE otherwise).
 *   original == 0: the sparse vector the reference's `solve_relaxation` returns, after `reconstruct_solution`
 *                  (matrix_data.rs:402-411): index = structural column of the standard form;
 *   original != 0: the `Solution` of `GeneralForm::compute_full_solution_with_reduced_solution` (general_form/mod.rs:840-934;
 *                  asserted value by value in tests/burkardt/test.rs:60-112, 143, 185): index = variable of the file, in
 *                  file order (shifts, flips, free splits and presolve removals undone in exact arithmetic).
 * Only the non-zero values are returned, ascending index: index[k] and, in `buffer`, their "num/den" texts (reduced, den > 0)
 * separated by '\n' and terminated by 0.  *count = their number, *length = bytes needed in `buffer`; with index == NULL and
 * buffer == NULL the call only reports the two sizes. */
int32_t relp_get_solution_exact(const relp_handle* handle, int32_t original, int32_t capacity, int32_t* count, int32_t* index,
                                char* buffer, int64_t buffer_capacity, int64_t* length);
/* The exact vectors the certificate proved the last result with (needs options.certify and a certified result).  They refer to the
 * standard form relp_model_* / relp_get_* describe: min c'x, A x = b, x >= 0 over the provider columns (structural columns, then
 * slack columns: nr_columns of relp_get_dimensions; nr_rows rows).  Artificial columns are not part of that form: a basic
 * artificial has value 0 and is never reported.
 *   RELP_WITNESS_PRIMAL, by provider column, of a FINITE_OPTIMUM or UNBOUNDED result: A x = b, x >= 0; for an optimum
 *                        c'x + fixed cost = the exact objective.
 *   RELP_WITNESS_DUAL,   by row, of a FINITE_OPTIMUM: c_j - y'a_j >= 0 for EVERY provider column j and y'b + fixed cost = the exact
 *                        objective; of an INFEASIBLE result (the Farkas vector): y'a_j <= 0 for every provider column j and
 *                        y'b > 0, the value relp_get_objective_exact returns for it (the phase-one optimum).
 *   RELP_WITNESS_RAY,    by provider column, of an UNBOUNDED result: d >= 0, A d = 0, c'd < 0; d_q = 1 for the entering column,
 *                        d_basis[i] = -alpha_i where a provider column is basic, 0 elsewhere: x + t d is feasible for every t >= 0.
 * After exact repair pivots the vectors are those of the basis that was finally proved.  Any other combination, and a result that
 * is not certified, is RELP_ERR_STATE with relp_last_error naming it; a `which` outside the enum is RELP_ERR_ARGUMENT.  Under
 * RELP_CARRY_NETWORK the optimum is proved from the forest: PRIMAL is returned, DUAL is RELP_ERR_STATE.
 * Return protocol of relp_get_solution_exact: only non-zero entries, ascending index, "num/den" (reduced, den > 0) separated by
 * '\n' and terminated by 0; with index == NULL and buffer == NULL the call only reports *count and *length. */
typedef enum relp_witness {
    RELP_WITNESS_PRIMAL = 0,
    RELP_WITNESS_DUAL = 1,
    RELP_WITNESS_RAY = 2
} relp_witness;
int32_t relp_get_witness_exact(const relp_handle* handle, int32_t which, int32_t capacity, int32_t* count, int32_t* index,
                               char* buffer, int64_t buffer_capacity, int64_t* length);
/* Name of variable j of the loaded file (the `String` of `Solution::solution_values`, data/linear_program/solution.rs:15-24);
 * "Xj" for providers built without names.  *length receives the full length. */
int32_t relp_get_variable_name(const relp_handle* handle, int32_t j, char* buffer, int32_t capacity, int32_t* length);
/* One JSON object describing the last relp_solve_relaxation of this handle (the per-LP record of SURVEY.md section 5; the
 * reference has no logging at all): name, m, n, nnz, result, pivots per phase, polishes / refactorisations, wall times,
 * pivots/s, algorithmic bytes per pivot, objective (f64) and objective_exact ("num/den" when certified).  "device_bytes":
 * the handle's own device arrays (the LP, its vectors and the carry's state: the explicit inverse, the forest); the factor sets of
 * the LU carries, the certificate's scratch and transient buffers are not counted.  "network_tree" (RELP_SW_NETWORK_STATS):
 * per-pivot means and maxima of the row depth, of the subtree the leaving arc cuts off and of the entering arc's path.
 * *length receives the full length; at most capacity - 1 bytes are written. */
int32_t relp_get_record_json(const relp_handle* handle, char* buffer, int32_t capacity, int32_t* length);
/* ---- the loop in exact fixed-width integer arithmetic on the device ------------------------------------------------------
 * `solve_relaxation::<Carry<RationalBig, _>>` with the reference's arbitrary-precision rationals replaced by LIMBS x 64-bit
 * integers over a common denominator (exact.hip; int128 = 2 limbs, int256 = 4, ... up to 128 = 8192 bits): the SAME pivot sequence as the
 * reference (steepest edge with its tie rules, exact ratio test with Bland ties, zero-level pivots) for as long as the
 * numbers fit.  The solve starts with `first_limbs` limbs and restarts with twice as many whenever a value may not fit
 * (status 4 when `max_limbs` <= 128 is not enough).  For small LPs: one workgroup owns the whole solve.
 *   trace: (phase, entering column, pivot row, leaving column) per pivot, in the index space of relp_price;
 *   objective: the exact optimum "num/den" incl. fixed cost; basis: as relp_get_basis.
 * status: 1 optimal | 2 infeasible | 3 unbounded | 4 overflow | 5 pivot limit. */
typedef struct relp_exact_result {
    int32_t status;
    int32_t limbs;              /* limbs of the run that finished */
    int64_t pivots_phase_one;
    int64_t pivots_phase_two;
    int32_t trace_entries;
    int32_t objective_length;
    int32_t limbs_tried[6];     /* every width that was tried, in order ... */
    int32_t redundant_rows;     /* rows found redundant at the end of phase one: the reference removes them (`RemoveRows`), here
                                   each keeps its zero-level artificial basic (-1 - k in `basis`) and the phase-two row indices of
                                   `trace` count the remaining rows, as the reference's do */
    int32_t reserved;
    int64_t pivots_survived[6]; /* ... and the pivots it made before a value might not fit (or until it finished) */
} relp_exact_result;
int32_t relp_solve_exact(relp_handle* handle, int32_t first_limbs, int32_t max_limbs, int64_t max_pivots, relp_exact_result* result,
                         int32_t trace_capacity, int32_t* trace, char* objective, int32_t objective_capacity, int32_t* basis);
/* Measurement of the last relp_solve_exact on this handle, one record per width tried (no reference counterpart: the reference's
 * RationalBig has no fixed width).  `update_word_products_*` count the 64 x 64 -> 128-bit multiplications of the integer-preserving
 * update of N = D B^-1 (the dominant step): `needed` by the entries' bit bounds, `issued` by the waves (the integer-multiply roofline
 * of bench.py divides `needed` -- the algorithmic figure -- by `step_seconds[7]`; issued / needed is the waste of whole blocks).  step_seconds: x_B, reduced costs (y = c_B' N and every c~_j), arg-max, exact weights, tournament, entering
 * column, ratio test, update of N, bookkeeping, products N a_j and keys of the columns with c~_j < 0.  Returns the number of records through *count (at most `capacity` copied). */
typedef struct relp_exact_width_record {
    int32_t limbs;
    int32_t grid;                          /* workgroups of the cooperative launch */
    int64_t pivots_total_at_end;           /* pivots of the solve when this width stopped */
    double seconds;                        /* host wall time of this width */
    double step_seconds[10];
    int64_t update_word_products_needed;
    int64_t update_word_products_issued;
} relp_exact_width_record;
int32_t relp_get_exact_counters(const relp_handle* handle, relp_exact_width_record* records, int32_t capacity, int32_t* count);
/* `InverseMaintainer::basis_column_index_for_row` for all rows (provider indices; -1-k for artificial k). */
int32_t relp_get_basis(const relp_handle* handle, int32_t* basis);

/* ---- fine-grained trait parity (tests and the Rust shim) ---------------------------------------------------- */
/* `InverseMaintainer::from_basis` (inverse_maintenance/mod.rs:92-101): start phase two from the given basis
 * (provider column per row).  Also the checkpoint/resume entry. */
int32_t relp_set_basis(relp_handle* handle, const int32_t* basis_columns);
/* Phase-one start: `Tableau::<_, Partially<_>>::new` (kind/artificial/partially.rs:125-205). */
int32_t relp_begin_phase_one(relp_handle* handle);
/* `Tableau::from_artificial` hand-over (kind/non_artificial.rs:99-120, carry/mod.rs:499-525).  Needs a basis: RELP_ERR_STATE unless
 * relp_begin_phase_one or relp_set_basis has run on this LP (an LP without artificials starts phase two in relp_begin_phase_one). */
int32_t relp_begin_phase_two(relp_handle* handle);
/* `BasisInverse::left_multiply_by_basis_inverse` (carry/mod.rs:98-107; lower_upper/mod.rs:180-210): FTRAN. */
int32_t relp_bi_ftran(relp_handle* handle, int32_t nnz, const int32_t* row_index, const double* value, double* out_m);
/* `BasisInverse::right_multiply_by_basis_inverse` (lower_upper/mod.rs:212-237): BTRAN. */
int32_t relp_bi_btran(relp_handle* handle, int32_t nnz, const int32_t* row_index, const double* value, double* out_m);
/* `BasisInverse::basis_inverse_row` (lower_upper/mod.rs:254-272). */
int32_t relp_bi_row(relp_handle* handle, int32_t row, double* out_m);
/* `PivotRule::select_primal_pivot_column` (strategy/pivot_rule.rs:221-241): *column = -1 when none. */
int32_t relp_price(relp_handle* handle, int32_t* column, double* relative_cost);
/* `Tableau::relative_cost(j)` for every column of the current index space (tableau/mod.rs:106-112). */
int32_t relp_relative_costs(relp_handle* handle, double* out_n);
/* Steepest-edge weights gamma_j (strategy/pivot_rule.rs:190-219); NaN for basic / artificial columns. */
int32_t relp_get_gamma(relp_handle* handle, double* out_n);
/* `Tableau::generate_column` + `select_primal_pivot_row` (tableau/mod.rs:126-130, 287-313): *row = -1 when unbounded. */
int32_t relp_ratio(relp_handle* handle, int32_t column, int32_t* row, double* out_alpha_m);
/* `Tableau::bring_into_basis(pivot_column, pivot_row, ..)` (tableau/mod.rs:139-160; `InverseMaintainer::change_basis`,
 * carry/mod.rs:561-604) with the pivot given by the caller, in the index space of relp_price / relp_ratio: the inverse, b, -pi,
 * the objective and the steepest-edge weights are updated as in any pivot of the loop.  RELP_ERR_STATE when the pivot
 * element is zero. */
int32_t relp_bring_into_basis(relp_handle* handle, int32_t column, int32_t row);
/* The last basis change: `BasisChangeComputationInfo::{pivot_row_index, pivot_column_index, leaving_column_index}`
 * (tableau/mod.rs:205-234) in the index space of relp_price, and the phase it was made in.  -1 when none was made yet. */
int32_t relp_get_last_pivot(relp_handle* handle, int32_t* phase, int32_t* column, int32_t* row, int32_t* leaving);
/* relp_options.implicit_bounds: how many iterations since the last relp_begin_phase_one (a solve starts with one) moved the entering
 * variable to its other bound without a basis change.  They are counted among the pivots of relp_result too.  0 without the mode. */
int32_t relp_get_bound_flips(const relp_handle* handle, int64_t* bound_flips);
/* `PivotRule::after_basis_update(info, tableau)` (strategy/pivot_rule.rs:23-54; `SteepestDescentAlongObjective` :243-296): the
 * Goldfarb-Reid update of the steepest-edge weights for the last relp_bring_into_basis / relp_iterate pivot.  Inside the
 * device loop the update rides on the next pricing pass; this entry applies it now (no-op when none is pending, or for the
 * rules without state). */
int32_t relp_se_after_basis_update(relp_handle* handle);
/* `BasisInverse::should_refactor` + `invert` on demand (lower_upper/mod.rs:78-92, 249-252): polishes the resident inverse and
 * recomputes b, -pi and the objective from it; *residual_before = max |I - B^T T| found. */
int32_t relp_refactor(relp_handle* handle, double* residual_before);
/* One full iteration of phase_one.rs:134-178 / phase_two.rs:36-58, repeated `count` times on the device. */
int32_t relp_iterate(relp_handle* handle, int64_t count, int64_t* done, int32_t* stop_reason);
/* `InverseMaintainer::{b, get_objective_function_value}` (inverse_maintenance/mod.rs:240-264). */
int32_t relp_get_b(relp_handle* handle, double* out_m);
int32_t relp_get_objective(relp_handle* handle, double* objective);
int32_t relp_get_stats(const relp_handle* handle, relp_stats* stats);
int32_t relp_reset_stats(relp_handle* handle);
/* Measurement hook for bench.py: average execution time (seconds) of ONE launch of a hot-loop kernel INSIDE the real
 * pivot sequence: `repetitions` further pivots of the current phase are run, the chosen kernel of each one bracketed by
 * its own HIP start/stop event pair on the handle's stream (hipExtLaunchKernelGGL).  The solve advances.
 * which: 0 pricing pass (with the steepest-edge update) | 1 fused ftran/ratio | 2 inverse update. */
int32_t relp_profile_kernel(relp_handle* handle, int32_t which, int32_t repetitions, double* seconds_per_launch);

/* Diagnostic builds only (-DRELP_STAMPS): per-segment cycle sums of the fused kernel; zeros otherwise. */
int32_t relp_debug_stamps(relp_handle* handle, uint64_t* out64);
/* Which kernels a handle created with `options` would run `model` on, and how it would size their arrays: the load-time plan
 * (relp_amd/csrc/kernel_path.hpp) as one JSON object.  Host only: needs no device.  The return protocol of relp_get_record_json.
 * RELP_ERR_ARGUMENT with the plan's message in `buffer` where a load would be refused (a carry or a ratio rule the LP cannot have). */
int32_t relp_debug_kernel_path(const relp_model* model, const relp_options* options, char* buffer, int32_t capacity, int32_t* length);
/* The switches and sizes of `options` for the test hooks that take no options of their own (relp_lu_factor_device), on the calling
 * thread, until the next call.  NULL restores the defaults. */
int32_t relp_debug_set_tuning(const relp_options* options);
/* Test hook of the exact simplex's update on the matrix cores (exact.hip, finish_update_entry): `count` numerators as the MFMA tiles
 * leave them -- `limbs` words each, word-major (word w of entry e at T[w * count + e]), one carry per pair of words
 * (carry[pair * count + e], added to the pair above), words[e] of them valid (a multiple of 8) -- become the entries of N: carries run
 * through, sign-extended from 64 * words[e] bits, shifted right by `shift` bits, negated where `flip`; N_out word-major, bits_out the
 * bit length of each magnitude.  limbs in {16, 32, 64, 128}.  No reference counterpart (tests only). */
int32_t relp_debug_exact_finish(int32_t device, int32_t limbs, int32_t count, const uint64_t* T, const int32_t* carry, const int32_t* words,
                                int32_t shift, int32_t flip, uint64_t* N_out, int32_t* bits_out);
/* Test hook of the word arithmetic behind a pivot's scalars (exact.hip): `count` pairs of `limbs`-word integers (entry e at a[e * limbs ..],
 * least significant word first), mode 0: out = 1 / a modulo 2^(64 limbs) for odd a (wave_inverse_odd: the inverse of D's odd part);
 * 1: out = -(a b) modulo 2^(64 limbs) (wave_mul_lo_negated: the rows' update factors); 2: out = a b.  No reference counterpart. */
int32_t relp_debug_exact_words(int32_t device, int32_t limbs, int32_t mode, int32_t count, const uint64_t* a, const uint64_t* b, uint64_t* out);
/* Test hook of the grid barrier that lets ONE cooperative launch run a whole exact solve (grid_barrier.hpp: arrivals counted per XCD,
 * one release fence per die, a watchdog that ends the launch instead of hanging the device).  mode 0, the exchange test: `rounds`
 * rounds on `grid` workgroups of 256 threads; in each, every thread stores a fresh value, the grid meets at the barrier, every thread
 * reads the values of `reads` other workgroups (rotating through all pairs; every round reads from every die) and counts what is not
 * this round's value.  mode 1: the last workgroup leaves one barrier out -- the watchdog (`limit_ticks` of 10 ns; 0 = ten seconds)
 * has to end the launch.  out8: [0] stale values seen, [1] the first as round << 32 | reader << 16 | writer (-1: none), [2] dies in use,
 * [3] ticks of 10 ns for workgroup 0's loop, [4] rounds, [5] workgroups that ran to the end, [6] the abort word (0: nobody gave up; else the
 * barrier's number), [7] workgroups found waiting then.  No reference counterpart (relp is single-threaded). */
int32_t relp_debug_grid_barrier(int32_t device, int32_t grid, int32_t rounds, int32_t reads, int32_t mode, int64_t limit_ticks, int64_t* out8);
/* Measurement hook of the exact update's MFMA tile by itself (exact.hip, mfma_update_tile with the fused epilogue): 512 workgroups x 4 waves
 * each run `tiles` tiles of `blocks` 64-byte blocks (<= limbs / 8) and `terms` terms (1: rescaled, 2: both products) on synthetic operands,
 * results shifted by `shift` bits; *seconds of the launch (tools/tile_bench.py).  limbs in {16, 32, 64, 128}.  No reference counterpart. */
int32_t relp_debug_exact_tile_bench(int32_t device, int32_t limbs, int32_t tiles, int32_t blocks, int32_t terms, int32_t shift, double* seconds);

/* ---- `BasisInverse` as an object of its own (no LP handle needed) ------------------------------------------------------
 * The reference's trait `BasisInverse` (tableau/inverse_maintenance/carry/mod.rs:69-169) and its main implementor
 * `LUDecomposition<F>` (carry/lower_upper/mod.rs:36-272): `P B Q = L U` by Markowitz pivoting
 * (lower_upper/decomposition/{mod.rs:27-143, pivoting.rs:45-81}), FTRAN / BTRAN through the sparse triangular factors,
 * Forrest-Tomlin row-eta updates (mod.rs:94-178, eta_file.rs:14-134), refactorisation after `refactor_period` updates
 * (mod.rs:249-252: 31).  The factorisation is computed on the host (f64; `pivot_threshold` is the relative pivot
 * tolerance floating point needs and the exact reference does not; `reference_ties` = 1 with threshold 0 reproduces the
 * reference's pivot choice entry for entry) and lives on the device, where the solves and updates run.
 * Vectors cross the boundary as the reference's sparse `(index, value)` pairs in, dense arrays of m doubles out.
 * Index spaces: a column is indexed by the rows of the LP (`left_multiply_by_basis_inverse` takes a provider column); a
 * row vector by the rows of the basis, i.e. by `Carry::basis_indices` positions (`right_multiply_by_basis_inverse`). */
typedef struct relp_basis_inverse relp_basis_inverse;
typedef struct relp_bi_options {
    int32_t device;
    int32_t refactor_period;   /* `should_refactor` turns true after this many `change_basis` calls (reference: 31) */
    double pivot_threshold;    /* accept a_ij as a pivot only if |a_ij| >= threshold * max_k |a_ik| (0: any non-zero) */
    int32_t reference_ties;    /* 1: pivoting.rs:60-80 exactly (minimum Markowitz count, ties by (column, row) position) */
    int32_t switches;          /* relp_switch bits (RELP_SW_BI_FACTOR_HOST, the RELP_SW_LUF_* hooks): in force during every call on the object */
} relp_bi_options;
int32_t relp_bi_options_default(relp_bi_options* options);
/* `BasisInverse::identity(m)` (carry/mod.rs:83; lower_upper/mod.rs:67-76). */
int32_t relp_bi_identity(const relp_bi_options* options, int32_t m, relp_basis_inverse** out);
/* `BasisInverse::invert(columns)` (carry/mod.rs:89-92; lower_upper/mod.rs:78-92): m columns in basis order, CSC over the
 * LP's rows.  RELP_ERR_NUMERICAL when the columns are singular. */
int32_t relp_bi_invert(const relp_bi_options* options, int32_t m, const int64_t* column_start, const int32_t* row_index,
                       const double* value, relp_basis_inverse** out);
int32_t relp_bi_free(relp_basis_inverse* bi);
const char* relp_bi_last_error(const relp_basis_inverse* bi);  /* bi == NULL: the last constructor error of this thread */
/* `BasisInverse::m()` (carry/mod.rs:168). */
int32_t relp_bi_m(const relp_basis_inverse* bi, int32_t* m);
/* `BasisInverse::left_multiply_by_basis_inverse(column)` (carry/mod.rs:123-129; lower_upper/mod.rs:180-210): B^-1 c.  The
 * object keeps the column and its spike -- the `ColumnComputationInfo` (lower_upper/mod.rs:417-432) -- for change_basis. */
int32_t relp_bi_left_multiply(relp_basis_inverse* bi, int32_t nnz, const int32_t* row_index, const double* value, double* out_m);
/* `BasisInverse::right_multiply_by_basis_inverse(row)` (carry/mod.rs:135-141; lower_upper/mod.rs:212-237): r B^-1. */
int32_t relp_bi_right_multiply(relp_basis_inverse* bi, int32_t nnz, const int32_t* index, const double* value, double* out_m);
/* `BasisInverse::basis_inverse_row(row)` (carry/mod.rs:165; lower_upper/mod.rs:254-272). */
int32_t relp_bi_basis_inverse_row(relp_basis_inverse* bi, int32_t row, double* out_m);
/* `BasisInverse::generate_element(i, original_column)` (carry/mod.rs:150-157; lower_upper/mod.rs:239-247): element i of
 * B^-1 c; *is_some = 0 when it is zero (the reference returns `None`). */
int32_t relp_bi_generate_element(relp_basis_inverse* bi, int32_t i, int32_t nnz, const int32_t* row_index, const double* value,
                                 double* element, int32_t* is_some);
/* `BasisInverse::change_basis(pivot_row_index, column)` (carry/mod.rs:104-108; lower_upper/mod.rs:94-178): the column of the
 * last relp_bi_left_multiply replaces the basis column of row `pivot_row_index` (Forrest-Tomlin update; ONLY the inverse
 * changes -- b, -pi and the objective are `Carry`'s, carry/mod.rs:561-604).  RELP_ERR_STATE without a preceding
 * left_multiply; RELP_ERR_NUMERICAL when the new basis is singular or the update area is full (poll should_refactor). */
int32_t relp_bi_change_basis(relp_basis_inverse* bi, int32_t pivot_row_index);
/* `BasisInverse::should_refactor()` (carry/mod.rs:163; lower_upper/mod.rs:249-252). */
int32_t relp_bi_should_refactor(relp_basis_inverse* bi, int32_t* should);
/* `RemoveBasisPart::remove_basis_part(indices)` (carry/mod.rs:176-180; basis_inverse_rows.rs:212-229): rows `indices` and
 * the basis columns of those rows leave the basis (redundant rows found in phase one); the rest is refactorised. */
int32_t relp_bi_remove_basis_part(relp_basis_inverse* bi, int32_t count, const int32_t* indices);
/* Sizes of the resident factor: non-zeros of L and U at the last refactorisation, the longest dependency chain of each
 * triangular solve (= LDS round trips on the device), updates since. */
int32_t relp_bi_statistics(relp_basis_inverse* bi, int64_t* nnz_lower, int64_t* nnz_upper, int32_t* depth_lower,
                           int32_t* depth_upper, int32_t* nr_updates);
/* The factors in the reference's own layout, for parity tests against its known-answer tests (lower_upper/mod.rs:36-58):
 * row/column permutation (forward), `lower_triangular` by column (lower_start has m + 1 entries), `upper_triangular` by
 * column with the rotations of all updates applied to the indices (upper_start: m + 1), `upper_diagonal`, and the eta
 * files (pivot, entries) with the indices each one had when it was made.  Every array holds at most `capacity` entries
 * (RELP_ERR_ARGUMENT otherwise); NULL skips an output. */
int32_t relp_bi_get_factors(relp_basis_inverse* bi, int64_t capacity, int32_t* row_permutation, int32_t* column_permutation,
                            int64_t* lower_start, int32_t* lower_row, double* lower_value, int64_t* upper_start,
                            int32_t* upper_row, double* upper_value, double* upper_diagonal, int32_t* nr_updates,
                            int64_t* eta_start, int32_t* eta_pivot, int32_t* eta_index, double* eta_value);
/* Host only (no device needed): the factorisation step of relp_bi_invert by itself -- `LUDecomposition::rows`
 * (decomposition/mod.rs:27-143).  L and U come back by ROW of the position space (lower_start / upper_start: m + 1 entries),
 * strictly triangular parts, U's diagonal apart; depth_* = longest dependency chain of the two triangular solves. */
int32_t relp_lu_factor_host(int32_t m, const int64_t* column_start, const int32_t* row_index, const double* value,
                            double pivot_threshold, int32_t reference_ties, int64_t capacity, int32_t* row_permutation,
                            int32_t* column_permutation, int64_t* lower_start, int32_t* lower_column, double* lower_value,
                            int64_t* upper_start, int32_t* upper_column, double* upper_value, double* upper_diagonal,
                            int32_t* depth_lower, int32_t* depth_upper);
/* The same factorisation with both triangles inverted as sparse matrices -- what RELP_CARRY_LU_INVERSE uploads at a
 * refactorisation (`LUDecomposition::invert`, lower_upper/mod.rs:78-92, then L^-1 and U^-1): lower_* = strict part of L^-1 by rows
 * (unit diagonal implied), upper_* = U^-1 by rows with its diagonal, upper_diagonal = ones.  Host only, for tests. */
int32_t relp_lu_invert_host(int32_t m, const int64_t* column_start, const int32_t* row_index, const double* value,
                            double pivot_threshold, int64_t capacity, int32_t* row_permutation, int32_t* column_permutation,
                            int64_t* lower_start, int32_t* lower_column, double* lower_value, int64_t* upper_start,
                            int32_t* upper_column, double* upper_value, double* upper_diagonal);

/* The factorisation step as the DEVICE runs it (round 4: `BasisInverse::invert` is a kernel, relp_amd/csrc/lu_factor.hip --
 * parallel independent pivots by Markowitz score with the same threshold test; with `reference_ties` one pivot per round, the
 * reference's, so the factors equal relp_lu_factor_host's and the reference's known answers entry for entry).  Same outputs as
 * relp_lu_factor_host, produced on HIP device `device` and copied back; `dense_tail`: the last rows (at most 64; 0 = none) go
 * through a dense LU out of LDS; info[32]: status, nnz(L), nnz(U), rounds, rows of the dense tail, arena peak, nnz(B), ...
 * `inverted` = 1: the two triangles inverted on the device as well (relp_lu_invert_host's outputs). */
int32_t relp_lu_factor_device(int32_t device, int32_t m, const int64_t* column_start, const int32_t* row_index, const double* value,
                              double pivot_threshold, int32_t reference_ties, int32_t dense_tail, int32_t inverted, int64_t capacity,
                              int32_t* row_permutation, int32_t* column_permutation, int64_t* lower_start, int32_t* lower_column,
                              double* lower_value, int64_t* upper_start, int32_t* upper_column, double* upper_value,
                              double* upper_diagonal, int32_t* info);

/* ---- `BasisInverse` over EXACT rationals (round 6) -----------------------------------------------------------------------
 * The reference's `BasisInverse` is generic over the field: `Carry<RationalBig, BI>` is what its tests run (tests/netlib/mod.rs:62).
 * relp_bi_* above is the f64 instantiation; these are the nine trait methods (carry/mod.rs:69-169) for exact rationals, one operation
 * at a time, so that the reference's known-answer tests (lower_upper/mod.rs:536-939, decomposition/mod.rs:319-438) hold with `==`
 * and a Rust shim can offer `Carry<RationalBig, GpuExact>`.  The object holds N = D B^-1 on the device --
 * integer entries over ONE positive denominator, fixed-width two's complement words, the representation of relp_solve_exact -- and
 * `change_basis` is Edmonds' integer-preserving pivot (exact division by a truncated multiplication with 1 / D_odd).  A bound that
 * reaches the width doubles the words (up to 128) before anything is written; beyond that RELP_ERR_OVERFLOW.
 * Sparse vectors come in as (index, numerator, denominator > 0) -- the reference's `Rational64` input type (io/mps/number/parse.rs:46-65);
 * a result is m integer numerators of *words 64-bit words each (two's complement, least significant word first, entry e at
 * numerators[e * *words]) and one positive denominator of *words words, NOT reduced (the caller's rational type reduces).
 * `capacity_words` is the room per integer the caller's arrays have; relp_bix_result_words says what is needed now
 * (RELP_ERR_ARGUMENT with *words set when it is not enough).  `should_refactor` is always 0: nothing accumulates. */
typedef struct relp_basis_inverse_exact relp_basis_inverse_exact;
/* `BasisInverse::identity(m)` (carry/mod.rs:83). */
int32_t relp_bix_identity(int32_t device, int32_t m, relp_basis_inverse_exact** out);
/* `BasisInverse::invert(columns)` (carry/mod.rs:89-92; lower_upper/mod.rs:78-92): m columns in basis order, CSC over the LP's rows.
 * RELP_ERR_NUMERICAL when the columns are singular. */
int32_t relp_bix_invert(int32_t device, int32_t m, const int64_t* column_start, const int32_t* row_index, const int64_t* value_num,
                        const int64_t* value_den, relp_basis_inverse_exact** out);
int32_t relp_bix_free(relp_basis_inverse_exact* bi);
const char* relp_bix_last_error(const relp_basis_inverse_exact* bi);  /* bi == NULL: the last constructor error of this thread */
/* `BasisInverse::m()` (carry/mod.rs:168). */
int32_t relp_bix_m(const relp_basis_inverse_exact* bi, int32_t* m);
int32_t relp_bix_result_words(const relp_basis_inverse_exact* bi, int32_t* words);
/* `left_multiply_by_basis_inverse(column)` (carry/mod.rs:123-129): B^-1 c.  The object keeps the column for change_basis. */
int32_t relp_bix_left_multiply(relp_basis_inverse_exact* bi, int32_t nnz, const int32_t* row_index, const int64_t* value_num, const int64_t* value_den,
                               int32_t capacity_words, uint64_t* numerators, uint64_t* denominator, int32_t* words);
/* `right_multiply_by_basis_inverse(row)` (carry/mod.rs:135-141): r B^-1. */
int32_t relp_bix_right_multiply(relp_basis_inverse_exact* bi, int32_t nnz, const int32_t* index, const int64_t* value_num, const int64_t* value_den,
                                int32_t capacity_words, uint64_t* numerators, uint64_t* denominator, int32_t* words);
/* The same for a row vector whose entries are themselves results of earlier solves -- `Carry::change_basis` multiplies B^-1 a_q from the
 * left (carry/mod.rs:561-604: the work vector of the steepest-edge update), RationalBig values no int64 holds: entry e = integer of
 * `value_words` two's complement words at values[e * value_words], all over ONE positive denominator of `value_words` words (the
 * format results come in).  *words = value_words + the object's words + 2. */
int32_t relp_bix_right_multiply_words(relp_basis_inverse_exact* bi, int32_t nnz, const int32_t* index, int32_t value_words, const uint64_t* values,
                                      const uint64_t* value_denominator, int32_t capacity_words, uint64_t* numerators, uint64_t* denominator, int32_t* words);
/* `basis_inverse_row(row)` (carry/mod.rs:165). */
int32_t relp_bix_basis_inverse_row(relp_basis_inverse_exact* bi, int32_t row, int32_t capacity_words, uint64_t* numerators, uint64_t* denominator,
                                   int32_t* words);
/* `generate_element(i, original_column)` (carry/mod.rs:150-157): ONE numerator and the denominator; *is_some = 0 when it is zero. */
int32_t relp_bix_generate_element(relp_basis_inverse_exact* bi, int32_t i, int32_t nnz, const int32_t* row_index, const int64_t* value_num,
                                  const int64_t* value_den, int32_t capacity_words, uint64_t* numerators, uint64_t* denominator, int32_t* words,
                                  int32_t* is_some);
/* `change_basis(pivot_row_index, column)` (carry/mod.rs:104-108): the column of the last relp_bix_left_multiply replaces the basis column
 * of that row.  RELP_ERR_STATE without a preceding left_multiply; RELP_ERR_NUMERICAL when the pivot element is zero. */
int32_t relp_bix_change_basis(relp_basis_inverse_exact* bi, int32_t pivot_row_index);
/* `should_refactor()` (carry/mod.rs:163). */
int32_t relp_bix_should_refactor(relp_basis_inverse_exact* bi, int32_t* should);
/* `RemoveBasisPart::remove_basis_part(indices)` (carry/mod.rs:176-180; basis_inverse_rows.rs:212-229): rows `indices` and the basis
 * columns of those rows -- artificial unit columns basic on redundant rows -- leave; what is left is the inverse of the smaller basis
 * over the same denominator. */
int32_t relp_bix_remove_basis_part(relp_basis_inverse_exact* bi, int32_t count, const int32_t* indices);


/* ---- batches of independent LPs (BASELINE config 4) -------------------------------------------
 * The reference solves one LP per call on one thread (tests/netlib/mod.rs:47-71); independent LPs are the unit that shards.
 * A batch keeps every LP resident on every worker: `workers_per_device` host threads per listed device, each owning one
 * handle (= one HIP stream) per model.  relp_batch_run serves a queue of `n_tickets` tickets -- ticket t solves model
 * schedule[t] (so K passes over a suite are ONE queue and the caller chooses the order, e.g. longest first) -- drawn with an
 * atomic fetch-add, or through `next_ticket` when several processes (one rank per GPU) share one queue: it must return a
 * fresh ticket number per call (values outside [0, n_tickets) end the worker).  No data-path collective exists.
 *   entries[t]: result of ticket t (status -1: not served by this batch); workers[w]: tickets, pivots, busy / idle seconds of
 *   worker w (relp_batch_workers of them); *makespan_seconds: wall clock of the run. */
typedef struct relp_batch relp_batch;
typedef struct relp_batch_entry {
    int32_t status;            /* relp_status of relp_solve_relaxation, or -1 */
    int32_t model;             /* schedule[t] */
    int32_t worker, device;
    relp_result result;
    double start_seconds, end_seconds;  /* relative to the start of the run */
} relp_batch_entry;
typedef struct relp_batch_worker {
    int32_t device;
    int32_t tickets;
    int64_t pivots;
    double busy_seconds;       /* inside relp_solve_relaxation */
    double queue_seconds;      /* drawing tickets */
    double idle_seconds;       /* makespan - busy */
    double finish_seconds;     /* when this worker found the queue empty */
} relp_batch_worker;
int32_t relp_batch_create(const relp_model* const* models, int32_t n_models, const relp_options* options, const int32_t* devices,
                          int32_t n_devices, int32_t workers_per_device, relp_batch** out, char* error, int32_t error_capacity);
int32_t relp_batch_destroy(relp_batch* batch);
int32_t relp_batch_workers(const relp_batch* batch, int32_t* n_workers);
int32_t relp_batch_run(relp_batch* batch, const int32_t* schedule, int64_t n_tickets, int64_t (*next_ticket)(void* user), void* user,
                       relp_batch_entry* entries, relp_batch_worker* workers, double* makespan_seconds);
/* exact optimum "num/den" of ticket t of the last run (options.certify; RELP_ERR_STATE when there is none) */
int32_t relp_batch_get_objective_exact(const relp_batch* batch, int64_t ticket, char* buffer, int32_t capacity, int32_t* length);
/* the resident handle of (worker, model), e.g. for relp_get_record_json / relp_get_solution_exact after a run */
int32_t relp_batch_handle(const relp_batch* batch, int32_t worker, int32_t model, relp_handle** out);

/* ---- many small LPs in one launch, one workgroup per LP (relp_amd/csrc/many.hip) ----------------------------
 * `solve_relaxation` (two_phase/mod.rs:25-109) for each of `n_models` independent LPs of at most 512 standard-form rows.  Each LP is
 * solved by ONE workgroup for its whole two-phase solve inside one ordinary kernel launch (no grid barrier, no cooperative launch):
 * the same provider, index spaces and starting basis as a handle's (artificials first, the reference's initial slack pivots), the
 * pricing and steepest-edge update of price_kernel (pivot_rule.rs:190-296), the two-pass ratio test of the fused pivot kernel or the
 * textbook rule (tableau/mod.rs:287-313; RELP_RATIO_AUTO resolved per LP as relp_load_model does), the product-form update of the
 * explicit inverse (basis_inverse_rows.rs:36-70) and zero-level pivots for the artificials left at the end of phase one
 * (phase_one.rs:232-278; rows without one keep their artificial, as the single-LP path does).  Every `polish_period` pivots and before
 * every verdict B^-1 is re-inverted from the basis columns by Gauss-Jordan with partial pivoting (`BasisInverse::invert`,
 * lower_upper/mod.rs:78-92); a fresh inverse whose residual max |B B^-1 - I| exceeds 1e-6, or a singular basis, ends THAT LP with
 * RELP_ERR_NUMERICAL.  B^-1 lives in the workgroup's LDS up to 139 rows (the LDS tier), in a per-LP slab of global memory from 140 to
 * 512 rows (the global tier).  Results do not depend on which other LPs share the launch, nor on their order.
 * relp_many_create_with and relp_many_config.implicit_bounds = 1: the upper bounds of the variables and the ranges are not rows of
 * the device LP but kept by the bounded-variable ratio test, as a handle with relp_options.implicit_bounds does (complemented
 * columns, bound flips, leaving at the upper bound; a bounded LP walks that handle's pivot sequence, a bound flip counting as an
 * iteration of its phase).  The device LP then has the CONSTRAINT rows only: the 512-row limit applies to them, the LDS tier of an LP
 * that has a bound ends at 138 rows, and an LP without any finite bound runs exactly as without the config.  relp_many_get_basis,
 * relp_many_get_solution and relp_many_dimensions keep speaking the reference's formulation (every standard-form row, the bound
 * rows and their slacks included), as relp_get_basis does on a handle in both modes.  With options.certify a FINITE_OPTIMUM is proved
 * from that basis; INFEASIBLE and UNBOUNDED results of a bounded LP stay uncertified in this mode, as on the handle.
 * relp_options is read as relp_create reads it; refused with RELP_ERR_ARGUMENT: a carry other than RELP_CARRY_EXPLICIT,
 * implicit_bounds, crash, a pivot rule other than steepest edge and Dantzig, and the switches of the generated graph columns.
 * relp_many_create checks every model before it touches the device (RELP_ERR_ARGUMENT naming the model's index, e.g. more than 512
 * rows), then RELP_ERR_DEVICE without a usable device.  With options.certify, every FINITE_OPTIMUM, INFEASIBLE and UNBOUNDED result
 * is proved after the launch by the exact certificate of relp_solve_relaxation; its time is `certify_seconds`, outside
 * `*kernel_seconds` (the launch alone, HIP events). */
typedef struct relp_many relp_many;
typedef struct relp_many_result {
    int32_t status;            /* relp_status of this LP: 0, or RELP_ERR_NUMERICAL */
    int32_t kind;              /* relp_result_kind */
    int32_t certified;         /* options.certify and the exact certificate holds */
    int32_t inverse_in_lds;    /* 1: the LDS tier, 0: the global tier */
    int64_t pivots_phase_one;  /* zero-level pivots included, as relp_result's */
    int64_t pivots_phase_two;
    int64_t reinversions;      /* Gauss-Jordan re-inversions of B */
    double objective;          /* f64 objective incl. fixed cost (NaN unless FINITE_OPTIMUM) */
    double max_residual;       /* largest max |B B^-1 - I| found before a re-inversion */
    double certify_seconds;    /* host wall time of this LP's certificate */
} relp_many_result;
int32_t relp_many_create(const relp_model* const* models, int32_t n_models, const relp_options* options, relp_many** out, char* error,
                         int32_t error_capacity);
/* What relp_options cannot say about this path.  `config` NULL: relp_many_create.  A struct_size other than
 * sizeof(relp_many_config) of a header of this library is RELP_ERR_ARGUMENT.  relp_options.implicit_bounds stays refused: the mode
 * is switched on here. */
typedef struct relp_many_config {
    int32_t struct_size;      /* sizeof(relp_many_config) of the caller's header */
    int32_t implicit_bounds;  /* 1: bounds and ranges by the bounded-variable ratio test, not as rows */
} relp_many_config;
int32_t relp_many_create_with(const relp_model* const* models, int32_t n_models, const relp_options* options,
                              const relp_many_config* config, relp_many** out, char* error, int32_t error_capacity);
/* Solves every LP (again, from the start).  results[k]: model k, in the caller's order; *kernel_seconds: the launch. */
int32_t relp_many_solve(relp_many* many, relp_many_result* results, double* kernel_seconds);
/* As relp_get_basis (provider columns, -1-k for artificial k), relp_get_solution and relp_get_objective_exact, for model `model`. */
int32_t relp_many_get_basis(const relp_many* many, int32_t model, int32_t* basis);
int32_t relp_many_get_solution(const relp_many* many, int32_t model, double* x_structural);
int32_t relp_many_get_objective_exact(const relp_many* many, int32_t model, char* buffer, int32_t capacity, int32_t* length);
/* Standard-form rows and structural columns of model `model` (the lengths of the two arrays above). */
int32_t relp_many_dimensions(const relp_many* many, int32_t model, int32_t* nr_rows, int32_t* nr_structural);
/* Bound flips among the iterations of model `model` in the last solve (0 without implicit bounds). */
int32_t relp_many_get_bound_flips(const relp_many* many, int32_t model, int64_t* bound_flips);
/* Why the last relp_many_solve failed, or why a certificate was not obtained. */
const char* relp_many_last_error(const relp_many* many);
int32_t relp_many_free(relp_many* many);

/* ---- the exact certificate of every LP of the last relp_many_solve in one further launch (relp_amd/csrc/many_certify.hip) ----------
 * One workgroup per LP inverts the row-scaled integer basis modulo a prime and lifts B x = b and B' y = c_B for a number of p-adic
 * digits the host fixed beforehand (Hadamard's bound); after one download every LP is finished on the host by the code of the
 * serial certificate (rational reconstruction, verification by exact substitution, sign checks of x_B and of the reduced costs of
 * all non-basic columns, exact objective), on at most 16 threads.  An LP the batched stage does not take, or whose batched proof
 * does not close, goes through the serial certificate of options.certify (its other primes and exact repair pivots included) --
 * per LP, never for the launch.  relp_many_fallback_reason says why.
 * RELP_MANY_CERTIFY_ALL_KINDS puts the INFEASIBLE and UNBOUNDED results into the same launch.  INFEASIBLE: the two solves on the final
 * phase-one basis with the phase-one costs (1 on a basic artificial, 0 elsewhere); the proof is the sign checks and a positive
 * phase-one optimum, which is the proved value.  UNBOUNDED: the two solves with the phase-two costs and a third, B alpha = a_q for
 * the entering column the solve named; the proof is x_B >= 0, cbar_q < 0 and alpha <= 0 with alpha = 0 where an artificial is basic,
 * and the proved value is "-inf".  These two have no repair pivots: what the batched stage refutes, the serial certificate refutes. */
typedef enum relp_many_fallback_reason {
    RELP_MANY_FALLBACK_NONE = 0,            /* the batched stage took it */
    RELP_MANY_FALLBACK_KIND = 1,            /* INFEASIBLE or UNBOUNDED in RELP_MANY_CERTIFY_OPTIMA; in ALL_KINDS an UNBOUNDED without a usable entering column */
    RELP_MANY_FALLBACK_WIDTH = 2,           /* a scaled coefficient, cost or right-hand side entry does not fit 62 bits, or the 128-bit residual overflowed */
    RELP_MANY_FALLBACK_SINGULAR_MOD_P = 3,  /* no pivot found modulo the prime */
    RELP_MANY_FALLBACK_DIGITS = 4,          /* more digits than the cap (512 per solve), or the reconstruction failed its exact verification */
    RELP_MANY_FALLBACK_SIGN = 5             /* a sign check failed: the basis needs exact repair pivots */
} relp_many_fallback_reason;
typedef enum relp_many_certify_mode {
    RELP_MANY_CERTIFY_OPTIMA = 0,     /* batched for every FINITE_OPTIMUM; INFEASIBLE and UNBOUNDED by the serial certificate (KIND) */
    RELP_MANY_CERTIFY_SERIAL = 1,     /* every LP by the serial certificate, as options.certify does */
    RELP_MANY_CERTIFY_ALL_KINDS = 2   /* batched for every kind: optima, Farkas proofs and rays in the one launch */
} relp_many_certify_mode;
typedef struct relp_many_certificate {
    int32_t struct_size;      /* in: sizeof of the caller's header, in element 0 */
    int32_t certified;        /* the exact certificate holds */
    int32_t path;             /* 1: the batched stage proved it, 2: the serial certificate did, 0: nothing to prove (status != 0) */
    int32_t fallback_reason;  /* relp_many_fallback_reason */
    int32_t digits_primal, digits_dual;  /* p-adic digits of the two solves (0 on path 2) */
    int64_t repair_pivots;    /* exact repair pivots (serial path only) */
    double  host_seconds;     /* this LP's host stage */
} relp_many_certificate;
/* Proves the results of the last relp_many_solve; out[k]: model k.  `mode`: relp_many_certify_mode.  0: batched for the optima (one
 * launch for all of them, fallback per LP); 1: every LP by the serial certificate, as options.certify does, reported in the same
 * struct; 2: batched for every kind (results of LPs solved with implicit bounds keep path 0 for the two other verdicts).
 * *device_seconds: the batched launch (HIP events; 0 in mode 1); *wall_seconds: the whole call.  Afterwards
 * relp_many_get_objective_exact returns the proved values: the optimum, the phase-one optimum of an INFEASIBLE LP, "-inf" for an
 * UNBOUNDED one.  A NULL handle or `out`, a mode that is none of the three or a struct_size no header ever had is RELP_ERR_ARGUMENT,
 * a call before relp_many_solve RELP_ERR_STATE; both are checked before the device is touched. */
int32_t relp_many_certify(relp_many* many, int32_t mode, relp_many_certificate* out, double* device_seconds, double* wall_seconds);
/* p-adic digits of model `model` in the last relp_many_certify: digits[0] of B x = b, digits[1] of B' y = c_B, digits[2] of the ray
 * B alpha = a_q (0 unless a batched UNBOUNDED proof with a non-empty entering column).  All 0 for an LP the batched stage did not
 * prove.  RELP_ERR_STATE before a relp_many_certify of the last solve. */
int32_t relp_many_get_certificate_digits(const relp_many* many, int32_t model, int32_t digits[3]);
/* Rows up to which the batched certificate keeps its work matrix in LDS (198); a per-LP slab of global memory beyond, up to 512. */
int32_t relp_many_certify_lds_rows(void);

/* ---- what the certificate of relp_many_certify proved, handed out --------------------------------------------------------------------
 * relp_many_keep_witnesses(many, 1) BEFORE a relp_many_certify makes that call keep, per certified LP, the exact vectors of its
 * proof: those of the batched stage on path 1, those of the serial certificate on path 2 (after its repair pivots).  The default is
 * off -- three vectors of m big integers per LP are hundreds of megabytes for a few hundred 500-row LPs -- and then
 * relp_many_certify keeps and returns exactly what it did before this switch existed.  The certificates themselves do not depend on
 * the switch.  A new relp_many_solve or relp_many_certify drops what was kept.
 * relp_many_get_witness_exact: as relp_get_witness_exact, for model `model` (the same table of `which`, index spaces and return
 * protocol).  relp_many_get_solution_exact: as relp_get_solution_exact (original == 0: the structural columns; else the variables
 * of the file), for a certified FINITE_OPTIMUM.  RELP_ERR_STATE with relp_many_last_error saying why: before a relp_many_certify
 * of the last solve, after one with the switch off, for an LP that is not certified (path 0 among them: the INFEASIBLE and
 * UNBOUNDED results of an LP solved with implicit bounds), for a witness its kind of result does not have.  RELP_ERR_ARGUMENT: a
 * model index out of range, a `which` outside relp_witness, capacities that are too small. */
int32_t relp_many_keep_witnesses(relp_many* many, int32_t on);
int32_t relp_many_get_witness_exact(const relp_many* many, int32_t model, int32_t which, int32_t capacity, int32_t* count,
                                    int32_t* index, char* buffer, int64_t buffer_capacity, int64_t* length);
int32_t relp_many_get_solution_exact(const relp_many* many, int32_t model, int32_t original, int32_t capacity, int32_t* count,
                                     int32_t* index, char* buffer, int64_t buffer_capacity, int64_t* length);

/* ---- dual simplex: re-solve from a basis after cuts or tightened bounds (relp_amd/csrc/dual.hip) ------------------------------------
 * The optimal basis of an LP is still dual feasible after rows are appended or a right-hand side is tightened, and primal infeasible
 * exactly where the change bites.  The caller builds the changed LP as a new model, loads it, and passes the old basis extended by
 * the slack column of each new row (relp_model_initial_pivots names it); nothing mutates a loaded LP.  `basis_columns`: m provider
 * columns, as relp_set_basis takes them.
 * RELP_ERR_ARGUMENT, before anything is launched, with the reason in relp_last_error: a plan the dual kernels do not take
 * (relp_debug_dual_refusal), an artificial column (a negative code) in the basis, and -- after the inverse of the basis has been
 * built -- a basis that is not dual feasible (the first column with a relative cost below -tol_dual is named).
 * relp_solve_dual: dual pivots until no row is infeasible, then the primal loop from that basis (it normally makes no pivot) and
 * the result as relp_solve_relaxation reports it: the primal pivots in pivots_phase_two, the dual ones through relp_get_dual_pivots
 * and as "dual_pivots" in relp_get_record_json ("dual_device_seconds": the device time of their batches).  A finite optimum is
 * certified as options.certify asks.  RELP_RESULT_INFEASIBLE (the dual is unbounded) comes back with certified = 0 and
 * relp_last_error saying so: the dual loop does not prove infeasibility yet.  A pivot element that is unusable even after a
 * polish of the inverse (an ill-conditioned basis) ends the call with RELP_ERR_STATE.
 * relp_begin_dual / relp_iterate_dual: the same loop in steps.  Stop reasons: 1 no infeasible row is left (the basis is primal
 * feasible), 2 the dual is unbounded (the LP is infeasible), 3 `count` pivots were made, 6 (under relp_set_dual_cutoff only) the
 * objective of the basis has reached the cutoff.  relp_get_last_pivot reports phase 3 after a
 * dual pivot.  The steepest-edge weights are not maintained by the dual loop: relp_begin_phase_two recomputes them. */
int32_t relp_solve_dual(relp_handle* handle, const int32_t* basis_columns, relp_result* result);
int32_t relp_begin_dual(relp_handle* handle, const int32_t* basis_columns);
int32_t relp_iterate_dual(relp_handle* handle, int64_t count, int64_t* done, int32_t* stop_reason);
int32_t relp_get_dual_pivots(const relp_handle* handle, int64_t* dual_pivots);
/* options.dual_pricing = RELP_DUAL_PRICING_STEEPEST_EDGE: the m weights beta_i of the dual loop as the next dual pivot would read them
 * (by row of the basis).  RELP_ERR_STATE before a relp_begin_dual / relp_solve_dual on the loaded LP, and on a handle whose
 * dual_pricing is 0 (it keeps no weights).  relp_get_record_json names the rule: "dual_pricing": "infeasibility" | "steepest_edge". */
int32_t relp_get_dual_weights(relp_handle* handle, double* out /* m */);
/* Host only: the empty string if the plan of (model, options) takes the dual loop, else the reason (the protocol of
 * relp_debug_kernel_path; a load that would itself be refused returns its status and message). */
int32_t relp_debug_dual_refusal(const relp_model* model, const relp_options* options, char* buffer, int32_t capacity, int32_t* length);

/* ---- dual simplex: start a child LP from its parent's inverse on the device (dual_inherit_kernel, relp_amd/csrc/dual.hip) ---------
 * In a cut loop or a branching step the parent is solved, rows are appended or a right-hand side is tightened, and the child is
 * re-solved from the parent's basis.  relp_begin_dual builds the child's inverse from scratch; these two calls write it from the
 * inverse the parent handle still holds: with the parent's basis in the first m positions and the slack of each of the k new rows
 * behind it, B_child^-1 = [B^-1 0; -S^-1 C B^-1  S^-1] (C: the new rows on the parent's basic columns, S: the new slacks' own
 * entries) -- a copy plus k sparse combinations of rows of the parent's inverse; for k = 0 a copy.  `child` has the child LP loaded,
 * `parent` is another handle on the same device that has solved (or been given a basis for) the parent LP and is only read;
 * `basis_columns`: the child's m + k provider columns in that order (the parent's relp_get_basis in the child's columns, then the
 * slacks).  Costs and right-hand sides may differ anywhere: x_B and -pi are recomputed from the child's data, and the
 * dual-feasibility check of relp_begin_dual still runs.  A forced polish guards the inherited inverse: it measures max |I - B Binv|
 * against the child's own matrix, corrects what it finds, and rebuilds from scratch by itself from 0.5 on.
 * Refused before anything is launched, the launch counters of both handles unchanged: RELP_ERR_ARGUMENT for a plan of either handle
 * that the dual kernels do not take, a parent on another device, and a pair of LPs and bases that are not in that relation
 * (relp_debug_dual_inherit_refusal; the row or column is named); RELP_ERR_STATE for a parent without a loaded LP, a parent on which
 * no solve, relp_set_basis or relp_solve_dual has happened, and parent == child.
 * relp_solve_dual_from is relp_solve_dual with this start.  relp_get_record_json says which start the last of these calls took:
 * "dual_start": "scratch" (relp_begin_dual) | "inherited" | "scratch_after_inherit" (the guard rebuilt) | "none";
 * "dual_start_seconds": its wall time, the stream synchronised at its end; "dual_start_gemms": the m x m x m products inside it;
 * "dual_start_residual": the guard's first reading (null where no guard ran). */
int32_t relp_begin_dual_from(relp_handle* child, const relp_handle* parent, const int32_t* basis_columns);
int32_t relp_solve_dual_from(relp_handle* child, const relp_handle* parent, const int32_t* basis_columns, relp_result* result);
/* Host only: the empty string if `child` with `basis_columns` can inherit from `parent` with `parent_basis` (both bases as
 * relp_get_basis gives them) under `options`, else the reason: relp_debug_dual_refusal of either model, or the relation above with
 * the row or column named (the protocol of relp_debug_dual_refusal). */
int32_t relp_debug_dual_inherit_refusal(const relp_model* parent, const relp_model* child, const int32_t* parent_basis,
                                        const int32_t* basis_columns, const relp_options* options, char* buffer, int32_t capacity,
                                        int32_t* length);

/* ---- dual simplex on implicit upper bounds: re-solve a branched child (the BOUNDED kernels of relp_amd/csrc/dual.hip) ---------------
 * A branch is a changed variable bound.  With options.implicit_bounds = 1 the bounds are no rows of the device LP, so the child of a
 * branching step has the parent's constraint rows and the dual loop's cost per pivot stays that of the constraint rows.  These two
 * calls are relp_begin_dual / relp_solve_dual for such a plan, and for every plan those two take (there they run the same kernels):
 * relp_debug_dual_bounded_refusal is relp_debug_dual_refusal of the plan without its bounds, the 8192 rows counted on the constraint
 * rows.  `basis_columns`: a basis of the formulation, one column per row of the model with the bound rows included, as relp_get_basis
 * returns it in both modes: the parent's basis plus the slack of every row the child's formulation gained (a new bound is such a row).
 * RELP_ERR_ARGUMENT before anything is launched for a refused plan and for an artificial column in any of those rows; after the
 * inverse has been built for a basis that is not dual feasible: the signed relative cost sgn_j (c_j - pi . a_j) of a non-basic column
 * (sgn_j = -1 where it sits at its upper bound) is below -tol_dual; the column is named, a fixed variable (both bounds equal) is
 * never priced.  A basic variable above its upper bound is no error: like one below zero it is a row the loop repairs.
 * One dual pivot: the leaving row has the largest violation max(-x_i, x_i - u_i) (options.dual_pricing = 1: its square over the row
 * norm of the inverse); the entering column is found by the ratio test of relp_solve_dual on the signed row; the leaving variable
 * stops at the bound it violated, and one that the branch fixed does not enter again.  An entering variable that overshoots its own
 * bound is a violated row for a later pivot; the bound-flipping ("long-step") ratio test is an option, relp_set_dual_long_step below.
 * relp_iterate_dual, relp_get_dual_pivots, relp_get_dual_weights and the record keys are shared with relp_begin_dual;
 * relp_get_record_json adds "dual_bounded": true where the last start ran the loop on implicit bounds.  A finite optimum is
 * certified as a cold solve with implicit bounds is; RELP_RESULT_INFEASIBLE comes back with certified = 0 and the relp_last_error of
 * relp_solve_dual (relp_set_dual_farkas below: proved instead).  relp_begin_dual, relp_solve_dual, relp_begin_dual_from and relp_solve_dual_from keep refusing a plan with
 * implicit bounds; the inherited start of such a plan is relp_begin_dual_bounded_from below. */
int32_t relp_solve_dual_bounded(relp_handle* handle, const int32_t* basis_columns, relp_result* result);
int32_t relp_begin_dual_bounded(relp_handle* handle, const int32_t* basis_columns);
int32_t relp_debug_dual_bounded_refusal(const relp_model* model, const relp_options* options, char* buffer, int32_t capacity, int32_t* length);

/* ---- ... started from the parent's inverse (dual_inherit_mapped_kernel, relp_amd/csrc/dual.hip) -------------------------------------
 * relp_begin_dual_from for two LPs held on implicit bounds.  The child of a pure branch has the parent's constraint rows, so its basis
 * matrix is the parent's up to the order of the positions and a sign per column: a column that one handle holds complemented
 * (x_j = u_j - x'_j) and the other does not.  `parent` holds its basis wherever its own pivots left it; `basis_columns` is the child's
 * basis of the formulation as relp_begin_dual_bounded takes it (the parent's relp_get_basis in the child's columns, plus the slack of
 * every row the child's formulation gained).  The relation is decided on the two bases reduced to the constraint rows: the child has
 * k >= 0 more constraint rows than the parent's m, its first m are the parent's in order; neither reduced basis holds an artificial;
 * every basic column of the child is either the same column as a basic column of the parent -- structural j, or the slack or surplus
 * of constraint row i, whatever its number -- with exactly the parent's entries on those m rows, or a column with one entry, in a new
 * row, one per new row.  Bounds, costs and right-hand sides may differ anywhere.  Position i of the child then holds what the parent
 * holds at a position src[i], and row i of the child's inverse is +-(row src[i] of the parent's); the k rows of the new slacks are
 * sparse combinations of those, as in relp_begin_dual_from.  The same guard follows, and the dual-feasibility check of
 * relp_begin_dual_bounded on the signed costs.  The long-step switch is read as relp_begin_dual_bounded reads it.
 * Refused before anything is launched, the launch counters of both handles unchanged: RELP_ERR_ARGUMENT where
 * relp_debug_dual_bounded_refusal names the plan of either handle, where a handle holds the bounds of its LP as rows
 * (options.implicit_bounds = 0 on an LP with a bound), for a parent on another device and for a pair outside the relation
 * (relp_debug_dual_bounded_inherit_refusal; the row or column is named); RELP_ERR_STATE for a parent without a loaded LP, a parent
 * without basis and inverse, and parent == child.  The parent is only read.
 * relp_solve_dual_bounded_from is relp_solve_dual_bounded with this start.  relp_get_record_json: "dual_start" and its companions as
 * after relp_begin_dual_from, "dual_bounded" as after relp_begin_dual_bounded, and "dual_inherit_complemented" / "dual_inherit_moved":
 * the inherited positions whose column the two handles hold with opposite signs, and those with src[i] != i (both 0 after any other
 * start). */
int32_t relp_begin_dual_bounded_from(relp_handle* child, const relp_handle* parent, const int32_t* basis_columns);
int32_t relp_solve_dual_bounded_from(relp_handle* child, const relp_handle* parent, const int32_t* basis_columns, relp_result* result);
/* Host only, the protocol and the arguments of relp_debug_dual_inherit_refusal, both bases as bases of the formulation: the empty
 * string, or relp_debug_dual_bounded_refusal of either model, or the relation above with the row or column named. */
int32_t relp_debug_dual_bounded_inherit_refusal(const relp_model* parent, const relp_model* child, const int32_t* parent_basis,
                                                const int32_t* basis_columns, const relp_options* options, char* buffer, int32_t capacity,
                                                int32_t* length);

/* The long-step (bound-flipping) ratio test of that loop, a switch on the handle (relp_options has no field for it): `on` = 1 or 0,
 * off on a new handle; any other value is RELP_ERR_ARGUMENT, a null handle answers as relp_begin_dual does.  It holds until changed
 * and is read by relp_begin_dual_bounded / relp_solve_dual_bounded.  With it on, the candidates of the ratio test are walked in the
 * order of their ratios, and a candidate with a finite upper bound whose ratio the dual step can pass -- the leaving row stays violated
 * by more than options.harris_delta with the column at its other bound -- goes to that bound instead of entering (at most 32 per
 * pivot); the entering column is the one the ratio test of the loop chooses among the rest, by the same rule (textbook or Harris) and
 * ties.  One more launch per dual pivot, and no further basis change.  With it off every launch and result is what it was.  On a plan
 * without implicit bounds the switch changes nothing; while it is on, relp_begin_dual, relp_solve_dual, relp_begin_dual_from and
 * relp_solve_dual_from return RELP_ERR_ARGUMENT (their loop has no boxed column to flip).
 * relp_get_record_json: "dual_long_step" (the last start ran the loop with it), "dual_flips" (columns sent to their other bound over
 * the dual pivots since that start) and "dual_long_step_skipped" (pivots whose boxed candidates, more than 2048, did not fit the
 * kernel: the plain rule there). */
int32_t relp_set_dual_long_step(relp_handle* handle, int32_t on);

/* The exact proof of an INFEASIBLE child, a switch on the handle like the one above: `on` = 1 or 0, off on a new handle; any other
 * value is RELP_ERR_ARGUMENT, a null handle answers as relp_set_dual_long_step does.  It holds until changed and is read by
 * relp_solve_dual, relp_solve_dual_from, relp_solve_dual_bounded and relp_solve_dual_bounded_from; it takes effect only with
 * options.certify != 0 and where the loop ends dual unbounded (RELP_RESULT_INFEASIBLE).  With it off, or with options.certify = 0,
 * that verdict comes back with certified = 0 and the relp_last_error it always had, and every launch, result and record key is what
 * it was.  With it on, row p of the exact inverse of the final basis -- p: the row at which the loop found the dual unbounded; one
 * transposed p-adic lifting with a unit right-hand side on the kernels of the optimum's certificate -- is checked as a Farkas vector
 * in exact integers: y = -rho_p, y'a_j <= 0 for every provider column and y'b > 0.  On a handle with options.implicit_bounds = 1 the
 * basis spans the constraint rows only, and either sign of rho_p is extended over the bound rows in closed form: with r_j = y'a_j
 * over the constraint rows, the bound row of column j gets -max(0, r_j), a column without a bound must have r_j <= 0, and
 * y'b = y_c'b_c - sum_j max(0, r_j) u_j must be positive.
 * Proved: result.certified = 1 with certify_seconds filled, relp_get_objective_exact returns y'b, and
 * relp_get_witness_exact(RELP_WITNESS_DUAL) returns y by row of the loaded model's standard form (bound rows included), indexed as
 * the Farkas vector of a cold INFEASIBLE solve; RELP_WITNESS_PRIMAL and RELP_WITNESS_RAY are not defined for this result.  Not proved:
 * certified = 0 and relp_last_error names the exact inequality that failed (the provider column that prices positive, or "y'b is
 * not positive"); no exact repair pivots follow.  One more launch (the leaving-row kernel names the row again) precedes the proof.
 * relp_get_record_json: "dual_farkas" (the switch as the last start read it) and "dual_farkas_row" (the row p the last proof used,
 * -1 where there was none).  relp_begin_dual / relp_iterate_dual and relp_many do not read the switch. */
int32_t relp_set_dual_farkas(relp_handle* handle, int32_t on);

/* An objective cutoff for the dual loop, a switch on the handle like the two above: `on` = 1 or 0, off on a new handle; any other value
 * is RELP_ERR_ARGUMENT, and so is a NaN `cutoff`; a null handle answers as relp_set_dual_farkas does.  +-inf are ordinary values: +inf
 * never stops the loop and only asks for the proof at the iteration limit, -inf stops it at the start basis.  `cutoff` is in the units
 * of relp_result.objective: the minimised standard-form objective with the fixed cost included.  The switch holds until changed and is
 * read by every start of the dual loop, relp_begin_dual, relp_begin_dual_from, relp_begin_dual_bounded and relp_begin_dual_bounded_from
 * included.  With it off every launch, result, message and record key is what it was.
 * Every basis of the dual loop is dual feasible, so its objective is a lower bound of the LP.  With the switch on, the kernel that
 * chooses the leaving row first compares the objective of the basis it stands on with the cutoff, before the iteration budget and
 * before anything is scanned, and stops the loop where objective >= cutoff: relp_iterate_dual reports stop reason 6, the four
 * relp_solve_dual* calls RELP_RESULT_CUTOFF, without the primal clean-up.  A start basis already at the cutoff makes 0 pivots; a basis
 * that is optimal and at the cutoff reports the cutoff, not the optimum.  result.objective is then the f64 objective of that basis
 * instead of NaN -- for RELP_RESULT_CUTOFF, and for a RELP_RESULT_ITERATION_LIMIT where the dual loop itself ran out of
 * options.max_pivots (strong branching: relp_set_dual_cutoff(handle, 1, +inf) and a small max_pivots).
 * With options.certify != 0 both results are proved by the dual half of the optimum's certificate: one transposed p-adic lifting of
 * B'y = c_B on its kernels, then d_j = c_j - y'a_j >= 0 for every provider column in exact integers and z = y'b + fixed cost.  On a
 * handle with options.implicit_bounds = 1 the basis spans the constraint rows: the bound row of column j gets min(0, d_j), a column
 * without a bound must have d_j >= 0, and z = y_c'b_c + sum_j min(0, d_j) u_j + fixed cost.  A RELP_RESULT_CUTOFF also needs z >= cutoff,
 * the double compared as the exact rational it is; at the iteration limit z is certified whatever its size.
 * Proved: result.certified = 1 with certify_seconds filled, relp_get_objective_exact returns z, and
 * relp_get_witness_exact(RELP_WITNESS_DUAL) returns y by row of the loaded model's standard form (bound rows included);
 * RELP_WITNESS_PRIMAL and RELP_WITNESS_RAY are RELP_ERR_STATE.  Not proved: certified = 0 and relp_last_error names the provider
 * column that prices negative (under the Harris ratio test a relative cost may be negative by less than tol_dual, and a column without
 * a bound cannot absorb that), or gives the exact bound and the cutoff it falls short of, or repeats the refusal of the optimum's
 * certificate; no exact repair pivots follow and the loop is not resumed.
 * relp_get_record_json: "dual_cutoff" (the value as the last start read it, "inf" / "-inf" as strings, null with the switch off),
 * "dual_cutoff_stopped" (the loop since that start stopped at the cutoff), "dual_bound_proved"; "result" may be "cutoff".
 * relp_many does not read the switch; relp_iterate_dual stops at the cutoff but has no result to certify. */
int32_t relp_set_dual_cutoff(relp_handle* handle, int32_t on, double cutoff);

/* Version / build info ("relp_amd <ver> gfx950"). */
const char* relp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RELP_AMD_H */
