/*
 * dlp.h — C ABI of the MI355X-native dense-tableau fp64 simplex (libdlp.so).
 *
 * This is the drop-in boundary for the per-iteration solver core of
 * shidanxu/DistributedLPSolver.  The reference has no FFI:
 * its surface is in-process C++ (namespace distributed_solver).  Each entry
 * point below names the reference interface it replaces; R/ is
 * /root/reference/DistributedLPSolver/DistributedLPSolver/.
 *
 *   reference                                         this ABI
 *   ------------------------------------------------  ---------------------------------
 *   Instance::Instance(A, I, slots, sparsity, ...)     dlp_problem_create_adalloc
 *     R/instance.h:41-42, R/instance.cpp:15-30
 *   Instance::GenerateInstance()  R/instance.h:46      dlp_problem_create_adalloc (bids
 *     R/instance.cpp:32-57                             regenerated bit-exactly, glibc rand)
 *   (no reference: dense LP input)                     dlp_problem_create_dense / _random
 *   Instance::RunMultiplicativeWeights(...)            dlp_solve  (exact simplex instead of
 *     R/instance.h:52-53, R/instance.cpp:117-134       the epsilon-approximate MW loop)
 *   GlobalProblem::ConstructPrimal per-iteration core  dlp_session_step_* (one pivot)
 *     R/global_problem.cpp:257-323                     dlp_session_run   (K pivots)
 *   AllocationMW::RunAllocationMW: the same            dlp_session_set_objective + dlp_session_run
 *     constraints re-weighted and solved again on      (warm re-solve from the resident basis
 *     every iteration  R/allocation_mw.cpp:271-326     instead of a cold one)
 *   the same loop over all the per-impression          dlp_batch_create_dense once, then per
 *     subproblems  R/global_problem.cpp:270-274         iteration dlp_batch_resolve(new weights):
 *     re-weighted by R/allocation_mw.cpp:271-326       every LP warm from its resident basis
 *   (no reference: budgets / capacities moved          dlp_batch_resolve_rhs(new b): dual simplex
 *     between runs, the same subproblems)              from every LP's resident basis
 *   (no reference: the same change on the one          dlp_session_set_rhs + dlp_session_run (dual
 *     global LP, R/global_problem.cpp:257-323)          pivots from the session's resident basis)
 *   (no reference: new constraints on the same         dlp_batch_add_rows(G, h): rows added in the
 *     subproblems: cuts, new capacities)               current basis, then the dual simplex
 *   (no reference: the same on the one global LP:      dlp_session_add_rows(G, h) + dlp_session_run
 *     a cutting-plane or lazy-constraint loop)         (the resident tableau grown, dual pivots)
 *   (no reference: a new advertiser or bid in the      dlp_batch_add_cols(P, d): columns added in the
 *     same subproblems; a priced-out column)           current basis, then the primal simplex
 *   (no reference: the same on the one global LP:      dlp_session_add_cols(P, d) + dlp_session_run
 *     column generation, advertisers / bids arriving)  (the resident tableau widened, primal pivots)
 *   Instance::solution_ (private, no getter)           dlp_result_x / dlp_result_y
 *     R/instance.h:34
 *   "Dual Value" stdout  R/global_problem.cpp:320-322  dlp_result_objective
 *
 * Conventions (build conventions):
 *   - every function returns int status: DLP_OK (0) or a code below; no C++
 *     exception ever crosses this boundary;
 *   - the library owns problems, sessions and results; the caller frees them
 *     with the matching *_free;
 *   - a handle is not thread-safe; concurrent solves on distinct handles are;
 *   - all arrays are plain host pointers unless the name says "dev";
 *   - fp64 everywhere (the reference computes in x87 long double; see DESIGN.md
 *     for what "parity" therefore means).
 *
 * Pivot rule (identical in oracle/ and on the GPU):
 *   maximise c^T x  s.t.  A x <= b, x >= 0, b >= 0, slack starting basis.
 *   Tableau T is (m+1) x (N+1), N = n + m, row-major, leading dimension
 *   ld = roundup(N+1, 16); row m is the objective (z_j, initially -c_j).
 *   price   : Dantzig q = argmin_{j<N} z_j (ties -> smallest j), optimal when
 *             z_q >= -tol_dj; in Bland mode q = smallest j with z_j < -tol_dj.
 *             Bland mode is entered after a degenerate pivot (r_p == 0) and
 *             left after a non-degenerate one (DLP_PRICING_DANTZIG_BLAND), or
 *             always on (DLP_PRICING_BLAND).
 *   ratio   : rows i<m with T[i][q] > tol_piv; r_i = max(T[i][N],0) / T[i][q]
 *             (IEEE division); p = argmin r_i, exact ties -> smallest basis[i];
 *             unbounded when no row qualifies.
 *   update  : prow_j = T[p][j] / T[p][q]; for i != p with T[i][q] != 0:
 *             T[i][j] = fma(-T[i][q], prow_j, T[i][j]); row p := prow; rows with
 *             T[i][q] == 0 are left untouched.
 */
#ifndef DLP_H
#define DLP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------- */
#define DLP_OK              0   /* optimal (or the step/run completed) */
#define DLP_INFEASIBLE      1   /* general LPs: Phase I ended with artificials > tol_feas */
#define DLP_UNBOUNDED       2
#define DLP_PIVOT_LIMIT     3
#define DLP_RUNNING         4   /* session has pivots left to do */
#define DLP_ERR_ARG        -1
#define DLP_ERR_OOM        -2
#define DLP_ERR_HIP        -3
#define DLP_ERR_RCCL       -4
#define DLP_ERR_NODEVICE   -5
#define DLP_ERR_STATE      -6
#define DLP_ERR_UNSUPPORTED -7

/* ---- enums ------------------------------------------------------------ */
#define DLP_PRICING_DANTZIG_BLAND 0
#define DLP_PRICING_BLAND         1

/* Synthetic instance families. */
#define DLP_GEN_DENSE       0   /* A,x0,c ~ U[0,1); b = A x0 + U[0,1)          */
#define DLP_GEN_DEGENERATE  1   /* ~50% "cone" rows: A in [-1,1), b_i = 0      */

/* Exchange buffers of a rank session (dlp_session_buffer). */
#define DLP_BUF_CAND_SEND   0   /* 1 x dlp_candidate, device                   */
#define DLP_BUF_CAND_RECV   1   /* nranks x dlp_candidate, device              */
#define DLP_BUF_PROW_SEND   2   /* ld x int64 (fp64 bits or INT64_MIN), device */
#define DLP_BUF_PROW_RECV   3   /* ld x int64, device                          */

/* Timing phases (dlp_session_timings, milliseconds, HIP events). */
#define DLP_PHASE_RATIO     0   /* pricing reduce + ratio test kernel          */
#define DLP_PHASE_EXCHANGE  1   /* candidate all-gather + select (nranks > 1)  */
#define DLP_PHASE_PROW      2   /* pivot-row normalise (+ all-reduce)          */
#define DLP_PHASE_UPDATE    3   /* rank-1 elimination kernel                   */
#define DLP_NUM_PHASES      4

typedef struct dlp_problem dlp_problem;
typedef struct dlp_session dlp_session;
typedef struct dlp_result  dlp_result;

/* 32-byte ratio-test candidate exchanged between ranks (all-gather). */
typedef struct dlp_candidate {
    double  ratio;      /* r_i */
    int32_t basis_var;  /* basis[i] (tie-break) */
    int32_t row;        /* global row index */
    int32_t valid;      /* 0 = no eligible row on that rank */
    int32_t pad0;
    double  pivot;      /* T[row][q], the pivot element if this row wins */
} dlp_candidate;

/* 32-byte pivot-log entry: the parity artifact. */
typedef struct dlp_pivot {
    int32_t q;          /* entering column */
    int32_t p;          /* pivot row (global) */
    int32_t leaving;    /* basis[p] before the pivot */
    int32_t pad;
    double  ratio;      /* r_p */
    double  objective;  /* T[m][N] after the pivot */
} dlp_pivot;

typedef struct dlp_options {
    int32_t device;          /* HIP device ordinal (default 0) */
    int32_t pricing;         /* DLP_PRICING_* */
    double  tol_dj;          /* reduced-cost tolerance (default 1e-9) */
    double  tol_piv;         /* pivot-element tolerance (default 1e-9) */
    int64_t max_pivots;      /* pivot limit (default 1000000) */
    int32_t log_pivots;      /* keep the pivot log (default 1) */
    int32_t check_interval;  /* pivots between host status polls (default 64) */
    int32_t timing;          /* 0 none, 1 update kernel, 2 every phase */
    int32_t nontemporal;     /* update kernel nt loads/stores: 1/0, -1 = auto (default) */
    int32_t rows_per_block;  /* update-kernel rows per workgroup band (0 = auto, default) */
    int32_t use_graph;       /* replay each poll window as a hipGraph (default 1) */
    int32_t update_variant;  /* rank-1 kernel variant 0..dlp_update_variants()-1, -1 = auto (default) */
    int32_t ld_align;        /* tableau row stride alignment in doubles, multiple of 16, 0 = auto
                                (default: when a row has >= 4096 columns, 128 for a deferred
                                session on a tableau > 1 GiB and 512 otherwise; else 16); the
                                kernels only touch the first roundup(N+1,16) columns */
    int32_t small_lp;        /* one-launch LDS solve for small LPs (dlp_cluster.hip): 0 = auto
                                (default: single-rank dense / random / ad-allocation problems
                                whose tableau is under 32 MiB and fits the LDS of the device's
                                CUs), 1 = whenever it fits, -1 = never */
    double  tol_feas;        /* general LPs: infeasible when the Phase I optimum is below
                                -tol_feas * (1 + max_i b'_i) (default 1e-9) */
    int32_t defer;           /* pivots per tableau pass (deferred rank-k update, results
                                bit-identical to rank-1): 1 = eager rank-1 per pivot, 2..64 =
                                block size, 0 = auto (default: 64 on a tableau > 1 GiB, 16
                                from 32 MiB, eager below 32 MiB and for multi-rank sessions
                                without an RCCL id, whose exchange the caller drives
                                through dlp_session_step_*; a single-rank session driven
                                through the step API keeps the size-based choice) */
    int32_t n_gpus;          /* dlp_solve only: 0 (default) = one GPU, no communicator;
                                N >= 1 = a row-block solve on devices [device, device+N) of
                                this process: one host thread and one RCCL communicator
                                rank per device (ncclCommInitAll); N = 1 runs that path on
                                a 1-rank communicator.  Sessions ignore it (one process per
                                GPU: dlp_session_create_rank). */
    int32_t lookahead;       /* deferred sessions: select block b+1 while the pass of block b
                                runs, on a second tableau buffer (results unchanged, bit for
                                bit; 2x the tableau memory): 1 = on where supported, 0 = off,
                                -1 = auto (default: K = 64 on a streaming (> 1 GiB) tableau
                                that fits twice, single-rank or a row-block rank once it runs
                                the peer exchange, never with RCCL; at K = 64 the selections
                                replay up to 127 steps) */
    int32_t exchange;        /* row-block exchange of dlp_solve(n_gpus = N) and of rank sessions
                                created with an RCCL id: DLP_XCHG_DEFAULT (0, the default) = the
                                peer exchange where every rank pair connects (peer access + IPC
                                open, agreed by all ranks), else RCCL (the reason:
                                dlp_session_exchange_reason); DLP_XCHG_RCCL = RCCL candidate
                                all-gather + pivot-row MAX all-reduce; DLP_XCHG_PEER = owner-
                                rooted peer stores, an error when the ranks cannot connect.
                                dlp_solve(n_gpus) with DLP_XCHG_DEFAULT: a run that fails on the
                                peer exchange is rerun from the start over RCCL
                                (dlp_result_exchange reports it) */
    int32_t condensed;       /* deferred sessions (defer > 1) of dense / random / ad-allocation LPs:
                                store only the n nonbasic columns + the RHS, the m basic columns
                                being exact unit vectors (results, pivots and
                                read-outs bit-identical to the full tableau, the read-outs up
                                to the sign of a zero in a basic variable's column: there the
                                full tableau keeps a caller's -0 that the rule left untouched,
                                the condensed read-out gives the unit vector's +0): 1 = on where
                                supported, -1 = off, 0 = auto (default: on; DLP_CONDENSED=0/1
                                overrides auto) */
} dlp_options;
/* Auto tuning (MI355X measurements): a local tableau > 1 GiB streams
 * from HBM -> row-serial kernel capped at 4 workgroups/CU, 8-row bands, nt;
 * otherwise it is partly Infinity-Cache resident -> uncapped, 4-row bands. */

/* ---- library ---------------------------------------------------------- */
void        dlp_options_default(dlp_options* opt);
const char* dlp_status_string(int status);
const char* dlp_last_error(void);          /* thread-local message of the last failure */
int         dlp_device_count(int* count);
/* Row partition of m constraint rows over nranks: [first, first+count). */
int         dlp_rank_rows(int64_t m, int rank, int nranks, int64_t* first, int64_t* count);
/* Deterministic winner of nranks candidates (same rule as the device select). */
int         dlp_candidate_select(const dlp_candidate* cands, int n, int* winner);
int64_t     dlp_tableau_ld(int64_t m, int64_t n);   /* roundup(N+1,16); sessions may pad more */
int         dlp_update_variants(void);               /* number of rank-1 update variants */
/* Sessions return their small buffers (<= 32 MiB each, <= 512 MiB in all) and streams to a
 * per-process cache for the next session, and dlp_batched_solve keeps one context per device
 * (stream, events, tableau / output buffers sized by the largest batch so far).  This frees the
 * cached buffers, pooled streams and batch contexts of `device` (-1: every device and the pinned host
 * buffers);
 * *bytes (may be NULL) = device bytes freed.  A session allocation that fails frees its device's
 * cached session buffers and retries by itself; that hipFree may synchronise the device, so it
 * waits for work other sessions have in flight on it (call this between runs to avoid that). */
int         dlp_release_cached_memory(int device, int64_t* bytes);

/* ---- problems ------------------------------------------------------------ */
/* Dense LP: A is m x n row-major; inputs are copied. Requires b >= 0. */
int dlp_problem_create_dense(int64_t m, int64_t n, const double* A, const double* b,
                             const double* c, dlp_problem** out);
/* Synthetic LP generated on the device (no host copy of A). */
int dlp_problem_create_random(int kind, int64_t m, int64_t n, uint64_t seed, dlp_problem** out);
/* The reference's ad-allocation LP (R/instance.cpp:32-57, R/allocation_mw.cpp:163-171):
 * max sum b_ai x_ai  s.t.  sum_i b_ai x_ai <= B_a (A rows),  sum_a x_ai <= 1 (I rows). */
int dlp_problem_create_adalloc(int num_advertisers, int num_impressions, int num_slots,
                               double bid_sparsity, double scaling_factor, dlp_problem** out);
/* ---- general LPs: row/column bounds + two-phase -------
 *   minimise (sense = DLP_MINIMIZE) or maximise (DLP_MAXIMIZE)  c^T x + c0
 *   s.t.  row_lo <= A x <= row_hi,  col_lo <= x <= col_hi,
 * A dense m x n row-major; any bound may be infinite (|v| >= 1e30 counts as
 * infinite).  No reference interface: the reference only builds its own
 * ad-allocation LP in memory (R/instance.cpp:32-57).  Netlib-style inputs come
 * through dlp_problem_create_mps.
 *
 * Canonical standard form (the rule spec; oracle/oracle.cpp restates it):
 *  columns: user variable j in order -> lo finite: x_j = lo + x' (one column;
 *           plus a bound row x' <= hi - lo when hi is finite); lo = -inf, hi
 *           finite: x_j = hi - x' (column -A_j, cost -c_j); both infinite:
 *           x_j = x'+ - x'- (two adjacent columns +A_j, -A_j).
 *  rows:    user rows in order, then the bound rows in column order.  shift_i
 *           = fma-chain over j ascending of A_ij * const_j (const = lo or hi).
 *           lo == hi -> E row (rhs lo - shift); only hi finite -> L row; only lo
 *           finite -> G row; both finite -> L row (hi) then G row (lo); both
 *           infinite -> dropped.  A row with rhs < 0 is negated (L <-> G); a G
 *           row with rhs == 0 is negated into an L row; rhs -0.0 becomes +0.0.
 *  tableau: [structural | one slack (+1, L) / surplus (-1, G) column per L/G
 *           row, in row order | one artificial (+1) column per G/E row, in row
 *           order | RHS].  Pricing covers structural + slack/surplus columns
 *           only (artificials never enter).  Basis: slack of L rows,
 *           artificial of G/E rows.  Objective (max form) c' = -c for minimise.
 *  phase I  (only when there are artificials): objective row z_j = sum over
 *           artificial rows i ascending of (-T[i][j]) for every non-artificial
 *           column j and the RHS (left fold from 0.0, z_j - T[i][j]); the
 *           phase II objective (-c', 0 elsewhere) rides along as an extra
 *           tableau row (global row m', owned by the last rank, never in the
 *           ratio test).  Pivot rule exactly as above.  At the Phase I optimum:
 *           infeasible if z_N < -tol_feas (1 + max b'); else every row whose
 *           basic variable is artificial, ascending, is pivoted on its first
 *           column q < n_price with |T[i][q]| > tol_piv (a logged pivot with
 *           ratio 0; a row without one is redundant and keeps its artificial);
 *           then the carried row becomes the objective row and Phase II runs
 *           in the pricing mode of the options (Bland state reset).
 *  results: x in user variables; y[i] = d(user objective)/d(bound of user row
 *           i) (HiGHS / scipy "marginals" sign convention), summed over the
 *           two rows of a ranged row; objective in the user's sense incl. c0. */
#define DLP_MINIMIZE   1
#define DLP_MAXIMIZE  -1
int dlp_problem_create_general(int64_t m, int64_t n, const double* A, const double* row_lo,
                               const double* row_hi, const double* col_lo, const double* col_hi,
                               const double* c, double c0, int sense, dlp_problem** out);
/* Free- or fixed-format MPS file (whitespace-separated fields; names without
 * blanks): NAME, OBJSENSE (MIN/MAX), ROWS (N/L/G/E; the first N row is the
 * objective, later N rows are dropped), COLUMNS (MARKER lines ignored: integer
 * columns are relaxed; repeated entries are summed), RHS (an objective-row RHS
 * v sets c0 = -v), RANGES (standard L/G/E semantics), BOUNDS (UP LO FX FR MI
 * PL BV LI UI; UP < 0 with lower 0 sets lower = -inf), ENDATA. */
int dlp_problem_create_mps(const char* path, dlp_problem** out);
/* The general form of any non-random problem (arrays may be NULL). */
int dlp_problem_get_general(const dlp_problem* prob, double* A, double* row_lo, double* row_hi,
                            double* col_lo, double* col_hi, double* c, double* c0, int* sense);
/* Standard-form sizes: constraint rows m' (the tableau adds the carried row
 * when nart > 0), total columns N, priced columns, artificial columns.  For
 * dense / random / ad-allocation problems: m' = m, N = n_price = n + m, 0. */
int dlp_problem_std_dims(const dlp_problem* prob, int64_t* m_std, int64_t* ncols,
                         int64_t* nprice, int64_t* nart);

int dlp_problem_dims(const dlp_problem* prob, int64_t* m, int64_t* n);
/* Dense copy of the problem data (A m x n row-major, b, c); NULL pointers skipped. */
int dlp_problem_get_dense(const dlp_problem* prob, double* A, double* b, double* c);
/* Ad-allocation bid list in variable order: (advertiser, impression, bid) triples. */
int dlp_problem_adalloc_bids(const dlp_problem* prob, int64_t* nnz, int32_t* adv,
                             int32_t* imp, double* bid);
void dlp_problem_free(dlp_problem* prob);

/* ---- one-shot solve (one GPU, or opt->n_gpus GPUs of this process) -------- */
int dlp_solve(const dlp_problem* prob, const dlp_options* opt, dlp_result** out);

/* ---- sessions: tableau resident in HBM ---------------------------------- */
/* Single GPU (rank 0 of 1). */
int dlp_session_create(const dlp_problem* prob, const dlp_options* opt, dlp_session** out);
/* Row-block rank of a multi-GPU solve; exchange through RCCL when
 * rccl_unique_id != NULL (128 bytes from dlp_comm_unique_id, identical on every
 * rank), or through caller-driven dlp_session_step_* when it is NULL.  With
 * nranks == 1 and an id, the RCCL exchange path runs on a 1-rank communicator
 * (same results; used to exercise that path on one GPU). */
int dlp_session_create_rank(const dlp_problem* prob, const dlp_options* opt, int rank,
                            int nranks, const void* rccl_unique_id, dlp_session** out);
int dlp_comm_unique_id(void* out128);
/* Launch up to max_pivots more pivots; returns DLP_OK / DLP_UNBOUNDED /
 * DLP_PIVOT_LIMIT / DLP_RUNNING (pivot budget of this call spent). */
int dlp_session_run(dlp_session* s, int64_t max_pivots, int64_t* pivots_done);
/* Caller-driven pivot (external communicator), in this order per pivot:
 *   step_candidate -> all-gather CAND_SEND into CAND_RECV (nranks x 32 B)
 *   step_select    -> all-reduce(MAX, int64) PROW_SEND into PROW_RECV (ld x 8 B)
 *   step_update.   With nranks == 1 no exchange is needed. */
int dlp_session_step_candidate(dlp_session* s);
int dlp_session_step_select(dlp_session* s);
int dlp_session_step_update(dlp_session* s);
/* Replace the objective of a live session by max c^T x (n doubles, host pointer) and make the
 * session runnable again from its current basis (a warm re-solve: the resident tableau is a
 * basic feasible tableau for every objective).  *kernel_ms (may be NULL): device time of the
 * objective-row rebuild.
 *
 * Sessions: single-GPU sessions of dense, random and ad-allocation problems, on every storage
 * path (eager, deferred full or condensed, lookahead, the one-launch small-LP path), at any time
 * between runs and whatever the status (running, optimal, unbounded, stopped by a run budget).
 *
 * The rule (part of the parity definition).  basis[i] is the basic variable of
 * row i; cB_i = c[basis[i]] if basis[i] < n, else +0.0 (slacks cost nothing).  For every stored
 * column j, the RHS column included:
 *   1. acc = -c_j for a structural variable j < n; acc = +0.0 for a slack and for the RHS (the
 *      cold build's start values);
 *   2. for rows i = 0, 1, ..., m-1 ascending, rows with cB_i == 0.0 skipped:
 *      acc = acc + (cB_i * T[i][j]), the product rounded, then the sum rounded (no fma);
 *   3. z_j = acc, except z_j = +0.0 for every basic variable j.
 * One ascending fold per column: no atomics, no tree over rows, no row bands; the result does
 * not depend on grid shape, tuning or layout.  Constraint rows, RHS, basis, pivot log and the
 * pivot count are untouched.  Afterwards the status is DLP_RUNNING, the Bland state is reset as
 * at the Phase II switch (Dantzig for DLP_PRICING_DANTZIG_BLAND, Bland for DLP_PRICING_BLAND),
 * the pricing partials are rebuilt, options.max_pivots keeps counting pivots over the session's
 * life and the pivot log is appended to.
 *
 * Errors, each leaving the session exactly as it was (everything is validated before anything
 * is enqueued): DLP_ERR_ARG: s or c NULL, n differs from the problem's n, a c_j that is not
 * finite; DLP_ERR_UNSUPPORTED (text in dlp_last_error): a general or MPS problem, a session
 * created with nranks > 1 or an RCCL id; DLP_ERR_STATE: a failed session, a caller-driven step
 * in progress (step_candidate done, step_update not yet), or a dual phase that is pending or
 * ended DLP_INFEASIBLE (dlp_session_set_rhs: the RHS has negative entries).
 * Not covered: changes of A (changes of b: dlp_session_set_rhs below for eager sessions,
 * dlp_session_set_rhs_in_place for every storage path), a
 * device-pointer c, multi-rank sessions, general LPs.  (Batches: dlp_batch_resolve applies this
 * rule to every resident LP.) */
int dlp_session_set_objective(dlp_session* s, const double* c, int64_t n, double* kernel_ms);
/* Replace the right-hand side of a live session by b (m doubles, host pointer; any finite value,
 * negative ones included) and put the session into a dual phase: the resident
 * tableau of an optimal session is dual feasible for every b, so the dual simplex continues from
 * its basis; it pays when b moves a little (budgets, capacities) and the basis mostly stays.  The
 * call rebuilds the RHS column, the objective entry included, and returns DLP_OK with the session
 * status DLP_RUNNING; *kernel_ms (may be NULL): device time of the rebuild kernel alone.
 * dlp_session_run then does dual pivots under its usual budget and window rules and ends
 * DLP_OK (no row is eligible: primal and dual feasible), DLP_INFEASIBLE (no entering column),
 * DLP_PIVOT_LIMIT or DLP_RUNNING (the life-time limit or the call's budget is spent).
 *
 * The rule is dlp_batch_resolve_rhs's (below), on the session's full-layout tableau:
 *   RHS rebuild: for every stored row r = 0 .. m: acc = +0.0; for l = 0 .. m-1 ascending:
 *     acc = acc + (T[r][n+l] * b_l), the product rounded, then the sum (no fma); T[r][N] = acc.
 *     One ascending fold per row, independent of grid and tuning.
 *   Leaving row: rows with T[i][N] < -tol_feas (absolute; dlp_options.tol_feas of creation); the
 *     most negative, exact ties to the smallest basis[i]; in Bland mode the eligible row with the
 *     smallest basis[i].  No eligible row -> DLP_OK; this test comes before the budget test.
 *   Entering column: columns j < N with a = T[p][j] < -tol_piv; r_j = zc / (-a) by IEEE division,
 *     zc = z_j if z_j > 0 else +0.0; the smallest, ties to the smallest j.  (A basic column's entry
 *     in row p is 0 or 1, never below -tol_piv: no mask is needed.)  None -> DLP_INFEASIBLE.
 *   Update: the eager update of the pivot rule above, unchanged, with the negative pivot.
 *   Log entry: q, p, leaving, ratio = r_q, objective after the pivot; appended to the session's log,
 *     npivots goes on counting (options.max_pivots counts pivots over the session's life).
 *   Bland state: reset at the call (on for DLP_PRICING_BLAND, else off), entered after a pivot
 *     with r_q == 0 and left after one with r_q > 0.
 *   The dual phase never falls through into a primal phase.
 *
 * Sessions: single-GPU sessions of dense, random and ad-allocation problems whose tableau is the
 * full layout in HBM between launches: the eager path (defer = 1) and the one-launch small-LP path
 * (the dual phase runs the HBM kernels on its tableau; a later primal run goes back to the one
 * launch).  The call is allowed at any time between runs.
 *
 * Errors, each leaving the session bit for bit as it was (everything is validated before anything
 * is enqueued), checked in this order:
 *   1. DLP_ERR_ARG: s or b NULL, m differs from the session's m (the problem's m plus the rows
 *      dlp_session_add_rows added), a b_i that is not finite;
 *   2. DLP_ERR_UNSUPPORTED (text in dlp_last_error): a general or MPS problem; a session created
 *      with nranks > 1 or an RCCL id; a deferred session (defer > 1, full or condensed, with or
 *      without lookahead): call dlp_session_set_rhs_in_place, or create the session with defer = 1;
 *   3. DLP_ERR_STATE: a failed session; a caller-driven step in progress; a tableau that is not
 *      dual feasible, some nonbasic z_j < -tol_dj (a session stopped inside a primal solve, or an
 *      unbounded one).
 * State around the dual phase: while it is pending (budget spent) or has ended DLP_INFEASIBLE the
 *   RHS has negative entries; dlp_session_set_rhs is accepted again (the slack columns are still
 *   B^-1 and a new b may be feasible), dlp_session_set_objective and dlp_session_step_* return
 *   DLP_ERR_STATE.  After DLP_OK the session is an ordinary optimal session (dlp_session_run
 *   returns DLP_OK with 0 pivots; set_objective and set_rhs work).  dlp_session_run continues from
 *   the tableau as it stands and folds nothing again, so budgets of any size give the pivots of one
 *   unbounded call.  dlp_session_result reads x, y and the basis from the tableau as it stands, for
 *   every status.  A negative pivot leaves -0 where a +0 stood in the basic columns of the pivot row;
 *   no comparison of the rule sees the sign of a zero.
 * Not covered by this call: deferred sessions (dlp_session_set_rhs_in_place below accepts them and
 * runs the dual phase on their own path; dlp_session_set_defer(s, 1, ...) moves a live deferred
 * session to the eager path and back), changes of A, a device-pointer b, multi-rank sessions,
 * general LPs. */
int dlp_session_set_rhs(dlp_session* s, const double* b, int64_t m, double* kernel_ms);
/* dlp_session_set_rhs for every storage path: the dual phase runs on the path the session is on
 * (DESIGN.md §24).  On an eager or small-LP session it is dlp_session_set_rhs itself: the same
 * code, the same results.  A deferred session (defer = 2..64, full or condensed) is accepted: the
 * call rebuilds the RHS column by the rule above (on the condensed layout over the stored slots:
 * the coefficient of slack n+l in row r is T[r][slot] when the slack is nonbasic, 1.0 when it is
 * basis[r], else +0.0, whose term cannot change a bit and is skipped), resets the Bland state and
 * sets the status DLP_RUNNING; dlp_session_run then does dual pivots in blocks of `defer`, one
 * tableau pass per block through the session's pass kernels, and ends DLP_OK, DLP_INFEASIBLE,
 * DLP_PIVOT_LIMIT or DLP_RUNNING exactly as above ("no eligible row" comes before every budget
 * test).  Every result is the one the route set_defer(1), set_rhs, run, set_defer back gives: status,
 * pivot count, log, basis, x, y and objective bit for bit, the tableau read-out byte for byte on
 * the full layout and up to the sign of a zero in a basic variable's column on the condensed one;
 * nothing depends on defer, the pass form, the row band, check_interval, use_graph or the budgets.
 *   Lookahead: a session with lookahead on is accepted; the call drains the lookahead and turns it
 *     off (as the step API does), dlp_session_get_lookahead then reports 0.  Turn it on again with
 *     dlp_session_set_defer(s, K, condensed, 1) once the dual phase has ended DLP_OK.
 *   On the condensed layout the entering ratio's ties go to the smaller variable index (never the
 *     slot); the RHS slot and the padding are never candidates; dual feasibility is checked per
 *     stored slot (every stored slot holds a nonbasic variable).
 * Errors: dlp_session_set_rhs's, in its order, without the "deferred session" refusal; each leaves
 * the session bit for bit as it was.  The state rules around the phase are those above: while it
 * is pending or ended DLP_INFEASIBLE, dlp_session_set_objective, _step_* and _set_defer return
 * DLP_ERR_STATE and both set_rhs calls are accepted again; after DLP_OK the session is an ordinary
 * optimal deferred session (set_objective, a primal run, another set_rhs_in_place and set_defer
 * work).  A dual phase starts and ends on an applied block.
 * Not covered: a dual block beside a lookahead pass, multi-rank and general-LP sessions, a
 * device-pointer b. */
int dlp_session_set_rhs_in_place(dlp_session* s, const double* b, int64_t m, double* kernel_ms);
/* Move a live single-GPU session to another storage path, between runs: the eager
 * full layout (defer = 1), or a deferred one with `defer` pivots per tableau pass, full or
 * condensed, with or without lookahead.  A session can so solve cold on the deferred path, switch
 * to eager for dlp_session_set_rhs and its dual phase, and switch back (dlp_session_set_rhs_in_place
 * runs that dual phase without the switch); or change K between phases.
 *   defer      1 = eager, 2..64 = pivots per pass, 0 = auto: creation's size rule for this tableau;
 *   condensed  -1 / 0 / 1 as dlp_options.condensed (DLP_CONDENSED overrides the auto choice);
 *              ignored when the target is eager;
 *   lookahead  -1 / 0 / 1 as dlp_options.lookahead: auto is on at K = 64 on a tableau > 1 GiB, 1 is
 *              on where it applies (it silently stays off elsewhere, as at creation); ignored when
 *              the target is eager;
 *   *kernel_ms (may be NULL): device time of the relayout kernel alone, 0 when no layout changed.
 * Unchanged by the call, bit for bit: the status (an optimal session stays optimal: the next
 * dlp_session_run returns DLP_OK with 0 pivots; a running one continues), the pivot count, the
 * pivot log, the basis, the Bland state, options.max_pivots' life-time count, tolerances and
 * pricing, the requested update variant, rows_per_block and non-temporal setting.  The tableau as
 * read out (dlp_session_tableau / _read_rows / _result) is byte-identical before and after, but for
 * the condensed layout's known caveat: its read-out gives +0 in a basic column where the full
 * layout may hold a -0 (after a dual phase's negative pivots).
 * After the call dlp_session_storage, _get_defer_tuning, _get_lookahead and _chain_cus report the
 * new path; the pass form is creation's choice for the new K (dlp_session_set_defer_tuning
 * overrides it afterwards) and the fused pivot is off, as at creation; graph windows captured on
 * the old geometry are dropped.  Every later pivot is bit-identical to the pivot a session created
 * on either path would do.  After a switch to defer = 1, dlp_session_set_rhs is accepted; after a
 * dual phase that ended DLP_OK, a switch back to a deferred path is accepted.
 * A layout that stays (full <-> full, e.g. eager <-> condensed = -1) keeps its buffer and stride and
 * nothing is copied; a new layout takes creation's stride rule for the session's ld_align.  The
 * nonbasic variables enter a new condensed layout ascending by index in slots 0..n-1 (the slot
 * order is not observable).  The old and the new tableau coexist during the call.
 * A call that asks for the path the session already runs returns DLP_OK and touches nothing.
 * Errors, each validated before anything is enqueued or allocated and leaving the session bit for
 * bit as it was, checked in this order:
 *   1. DLP_ERR_ARG: s NULL; defer outside 0..64; condensed or lookahead outside -1..1; defer > 1
 *      with an update variant that is not a 512-column one;
 *   2. DLP_ERR_UNSUPPORTED (text in dlp_last_error): a general or MPS problem; a session created
 *      with nranks > 1 or an RCCL id; a session on the one-launch small-LP path
 *      (dlp_session_small_lp = 1);
 *   3. DLP_ERR_STATE: a failed session; a caller-driven step in progress; a dual phase that is
 *      pending or ended DLP_INFEASIBLE (the RHS has negative entries, which no deferred primal path
 *      may see);
 *   4. DLP_ERR_OOM: the new buffers do not fit; they are allocated before anything is changed.
 * Not covered: multi-rank and general-LP sessions.  (A deferred dual pivot: dlp_session_set_rhs_in_place.) */
int dlp_session_set_defer(dlp_session* s, int defer, int condensed, int lookahead, double* kernel_ms);
/* Add r constraint rows G x <= h to a live session and put it into a dual phase: a
 * cut, a capacity that did not exist, a lazily generated constraint, without a new dlp_problem, a
 * new upload and a cold solve.  G is r x n row-major, h has r entries (host pointers; any finite
 * value, negative h included); n must be the session's n.  m becomes m + r; n and every existing
 * variable index stay.  New row t is row m + t; its slack is variable n + m + t, basic in that row.
 * Afterwards the session is exactly as after dlp_session_set_rhs_in_place: status DLP_RUNNING, the
 * Bland state reset from the pricing option; dlp_session_run does dual pivots on the path the
 * session is on and ends DLP_OK / DLP_INFEASIBLE / DLP_PIVOT_LIMIT / DLP_RUNNING ("no eligible row"
 * comes before every budget test, so rows the optimum already satisfies give DLP_OK with 0 pivots).
 * *kernel_ms (may be NULL): device time of the two kernels of the call together (the grow copy and
 * the row fold, dlp_addrows.hip).  r == 0 returns DLP_OK and touches nothing (G, h may be NULL).
 *
 * The row rule is dlp_batch_add_rows's (below), on the session's layouts.  For new
 * row t with g = row t of G, and the old rows i < m: gB_i = g[basis[i]] if basis[i] < n, else +0.0.
 *   For every stored column (variable v) and for the RHS: acc = g_v (structural v < n), +0.0 (a
 *     slack), h_t (the RHS); for i = 0 .. m-1 ascending, rows with gB_i == 0.0 skipped:
 *     acc = acc - (gB_i * T[i][v]), the product rounded, then the difference (no fma).  One
 *     ascending chain per entry over the old rows only (the new rows do not see each other); no
 *     atomics, no tree over rows, nothing that depends on grid, K, layout or tuning.
 *   Full layout, new row: every column of a currently basic variable is exact +0.0 (not folded); the
 *     row's own slack column is 1.0; the other new slack columns and the padding are +0.0.
 *     Elsewhere: the old rows and the objective row get +0.0 in the new slack columns; the objective
 *     row becomes row m + r.  Old constraint rows and the objective row keep their bits, the RHS too.
 *   Condensed layout: only the stored slots and the RHS slot exist; the slots keep their variables,
 *     the new slacks are basic; basis[m+t] = n + m + t.
 *   Strides: the full layout's RHS moves from column N to N + r and the stride follows creation's
 *     rule for the session's ld_align at the new width; the condensed stride does not change.
 *
 * Sessions: single-GPU sessions of dense, random and ad-allocation problems on the eager path and on
 * every deferred path (defer 2..64, full or condensed).  A session with lookahead on is accepted:
 * it is drained and turned off, as by dlp_session_set_rhs_in_place; dlp_session_set_defer(s, K,
 * condensed, 1) turns it on again after the phase ended DLP_OK.  A session whose earlier dual
 * phase is pending or ended DLP_INFEASIBLE is accepted (the rule holds for any basis); a block the
 * step API left open is applied first.  The tableau must be dual feasible (dlp_session_set_rhs's
 * check).
 *
 * What follows the new shape: everything sized by m, N or a stride is rebuilt by creation's rules
 * (the tableau, basis, slot maps, block arrays, selection plans, the pass band; captured graph
 * windows are dropped; pricing partials and the RHS cache are regathered).  What stays: the
 * session's size class as decided at creation (streaming or cache-resident, ld_align, the update
 * variant, the non-temporal setting: a handful of rows does not move a tableau across those
 * limits), K, the pass form, tolerances, pricing, the pivot log, its capacity and the life-time
 * pivot count.  dlp_session_info, _storage, _tableau, _read_rows and _result report the grown LP (y
 * and basis have m + r entries).  The dlp_problem handle is not touched, so the session no longer
 * has its problem's m: dlp_session_set_rhs and _set_rhs_in_place take m + r entries,
 * dlp_session_set_objective and _set_defer work as on any session of that shape, and so does a
 * second dlp_session_add_rows.  The old and the new tableau coexist during the call.
 *
 * Errors, each leaving the session bit for bit as it was (everything is validated, and every new
 * buffer allocated, before anything is changed), checked in this order:
 *   1. DLP_ERR_ARG: s NULL; r < 0; r > 0 with G or h NULL; n differs from the session's n; a G or h
 *      entry that is not finite (dlp_last_error names it); n + m + r + 1 beyond the int32 range of
 *      creation;
 *   2. DLP_ERR_UNSUPPORTED (text in dlp_last_error): a general or MPS problem; a session created
 *      with nranks > 1 or an RCCL id; a session on the one-launch small-LP path (create it with
 *      small_lp = -1: its LDS plan is tied to the shape);
 *   3. DLP_ERR_STATE: a failed session; a caller-driven step in progress; a tableau that is not dual
 *      feasible (dlp_session_set_rhs's test and message);
 *   4. DLP_ERR_OOM: the grown buffers do not fit beside the old ones.  The shape, every buffer, the
 *      status, the basis and the tableau are as before, with one difference: a lookahead that was on
 *      has been drained and turned off (that happens before the allocation;
 *      dlp_session_get_lookahead reports 0, dlp_session_set_defer turns it on again).
 * A HIP error during the growth itself (DLP_ERR_HIP) puts the old shape and buffers back as well.
 * Any r that passes check 1 is handled: the row fold takes one launch per 262,140 rows.
 * Not covered: removing rows, changing entries of existing rows (columns: dlp_session_add_cols,
 * below); device-pointer G /
 * h; small-LP, multi-rank and general-LP sessions; spare rows that would avoid the reallocation; a
 * dual block beside a lookahead pass. */
int dlp_session_add_rows(dlp_session* s, int64_t r, const double* G, const double* h, int64_t n,
                         double* kernel_ms);
/* Add k variables (columns) to a live session and put it into a primal phase: a
 * priced-out column, a new advertiser or bid, a new activity, without a new dlp_problem, a new upload
 * of [A | P] and a cold solve.  P is m x k row-major (column t = the constraint column of new variable
 * t), d has k entries (its costs); host pointers; any finite value, negative entries and costs
 * included.  m must be the session's live row count (rows from dlp_session_add_rows included).  The LP
 * becomes  max [c d]^T [x; w]  s.t.  [A | P] [x; w] <= b.  n becomes n + k; the new variables are
 * n .. n+k-1 (nonbasic at 0, so the basis stays primal feasible); slack i is renamed from n + i to
 * n + k + i (dlp_batch_add_cols's renaming: it preserves the order of the old variables, so every tie
 * rule by variable index decides among them as before).  m, the RHS, the objective value and every old
 * entry keep their bits.  k == 0 returns DLP_OK and touches nothing (P, d may be NULL).
 * *kernel_ms (may be NULL): device time of the two kernels of the call together (the widening copy and
 * the column fold, dlp_addcols.hip).
 *
 * Afterwards: status DLP_RUNNING, a primal phase (as after dlp_session_set_objective), the Bland state
 * reset from the pricing option, no entering column chosen, an empty block, the pricing partials
 * rebuilt, on K > 1 the RHS cache regathered.  dlp_session_run then does primal pivots on the path
 * the session is on and ends DLP_OK / DLP_UNBOUNDED / DLP_PIVOT_LIMIT / DLP_RUNNING; the pivot budget
 * counts from this call.  Pivot-log entries written before the call keep the variable numbers of
 * their time (a slack logged as n + i then is n + k + i now); entries written afterwards use the new
 * numbers.
 *
 * The column rule is dlp_batch_add_cols's (below), on the session's layouts.  For new
 * variable t with column p and every stored row r = 0 .. m (the objective row included):
 *     acc = +0.0;  for l = 0 .. m-1 ascending: acc = acc + (Tfull[r][n+l] * p_l),
 *   the product rounded, then the sum (no fma).  Constraint rows store acc, the objective row
 *   acc - d_t (one more rounded subtraction).  One ascending chain per entry; the k columns do not see
 *   each other; no atomics, no tree, nothing that depends on grid, K, layout or tuning.  A +-0
 *   coefficient or a +-0 p_l changes no bit of acc (it starts at +0.0 and is never -0.0), so such
 *   terms may be skipped and no select is needed (unlike the row rule).
 *   Full layout: Tfull[r][n+l] is the stored entry of column n + l (a basic slack's column is its
 *     row's unit vector, objective entry +0.0).
 *   Condensed layout: Tfull[r][n+l] is the entry of slack l's slot when it is nonbasic; 1.0 in the row
 *     where it is basic; +0.0 otherwise, the objective row included (dlp_session_set_rhs_in_place's
 *     RHS rule).
 * Layouts afterwards.  Full: columns [0, n) stay, the new variables are columns [n, n + k), the slack
 *   block moves from [n, N) to [n + k, N + k), the RHS from N to N + k; the stride follows creation's
 *   rule for the session's ld_align at the new width.  Condensed: slots [0, n) stay, the new variables
 *   take slots n .. n+k-1 (nonbasic: var_of[n+t] = n + t, slot_of[n+t] = n + t), the RHS slot moves
 *   from n to n + k, the stride becomes round16(n + k + 1) (by ld_align); every index >= n in var_of,
 *   slot_of and basis is raised by k; no restart is pending (every block has been applied).
 *
 * Sessions: single-GPU sessions of dense, random and ad-allocation problems on the eager path and on
 * every deferred path (defer 2..64, full or condensed), in every state but the three of check 3:
 * optimal, unbounded, or stopped by a budget inside a primal phase (no dual-feasibility check
 * applies).  A session with lookahead on is accepted: it is drained and turned off, as by
 * dlp_session_add_rows; dlp_session_set_defer(s, K, condensed, 1) turns it on again.  A block the
 * step API left open is applied first.
 *
 * What follows the new shape: everything sized by n, N, the width or a stride is rebuilt by
 * creation's rules (the tableau, basis, slot maps, block arrays, selection plans, the pass band, the
 * cost buffer of dlp_session_set_objective; captured graph windows are dropped).  What stays: the
 * size class decided at creation, K, the pass form, the caller's band rows, tolerances, pricing, the
 * pivot log, its capacity and the life-time pivot count.  The dlp_problem handle is not touched, so
 * the session no longer has its problem's n: dlp_session_set_objective takes n + k costs,
 * dlp_session_add_rows G with n + k columns, dlp_session_result returns x with n + k entries, and
 * dlp_session_info, _storage, _tableau, _read_rows, _set_rhs, _set_rhs_in_place, _set_defer and a
 * second dlp_session_add_cols work as on any session of that shape.  The old and the new tableau
 * coexist during the call.
 *
 * Errors, each leaving the session bit for bit as it was (everything is validated, and every new
 * buffer allocated, before anything is changed), checked in this order:
 *   1. DLP_ERR_ARG: s NULL; k < 0; k > 0 with P or d NULL; m differs from the session's m;
 *      n + k + m + 1 beyond the int32 range of creation (checked before P is read); a P or d entry
 *      that is not finite (dlp_last_error names it);
 *   2. DLP_ERR_UNSUPPORTED (text in dlp_last_error): a general or MPS problem; a session created
 *      with nranks > 1 or an RCCL id; a session on the one-launch small-LP path (create it with
 *      small_lp = -1: its LDS plan is tied to the shape);
 *   3. DLP_ERR_STATE: a failed session; a caller-driven step in progress; a dual phase that is
 *      pending or ended DLP_INFEASIBLE (the RHS has negative entries, which the primal rule must not
 *      pivot on: finish it with dlp_session_run or call dlp_session_set_rhs);
 *   4. DLP_ERR_OOM: the widened buffers do not fit beside the old ones.  The shape, every buffer, the
 *      status, the basis and the tableau are as before, with one difference: a lookahead that was on
 *      has been drained and turned off (that happens before the allocation;
 *      dlp_session_get_lookahead reports 0, dlp_session_set_defer turns it on again).
 * A HIP error during the widening itself (DLP_ERR_HIP) puts the old shape and buffers back as well.
 * Any k that passes check 1 is handled: the column fold takes one launch per 262,140 columns.
 * Not covered: removing columns, changing entries of existing columns; device-pointer P / d;
 * small-LP, multi-rank and general-LP sessions; spare slots that would avoid the reallocation;
 * keeping the lookahead across the call. */
int dlp_session_add_cols(dlp_session* s, int64_t k, const double* P, const double* d, int64_t m,
                         double* kernel_ms);
int dlp_session_buffer(dlp_session* s, int which, void** dev_ptr, size_t* bytes);
/* Synchronous host copies of an exchange buffer (for host-side communicators). */
int dlp_session_read_buffer(dlp_session* s, int which, void* host, size_t bytes);
int dlp_session_write_buffer(dlp_session* s, int which, const void* host, size_t bytes);
int dlp_session_sync(dlp_session* s);
int dlp_session_status(dlp_session* s, int* status, int64_t* npivots);
int dlp_session_timings(dlp_session* s, double* ms_out /* DLP_NUM_PHASES */, int64_t* nsamples);
/* Update-kernel launches timed (timing >= 1) and their total device time: one
 * rank-1 update per pivot (defer = 1) or one rank-k tableau pass per block. */
int dlp_session_update_stats(dlp_session* s, int64_t* launches, double* ms, int* defer);
int dlp_session_reset_timings(dlp_session* s);
/* Retune the rank-1 update between pivots (results are bit-identical for every
 * setting): variant 0..7 (rows in flight x doubles per lane x colq staging),
 * rows per workgroup band (0 = auto, <= 256), non-temporal loads/stores. */
int dlp_session_set_tuning(dlp_session* s, int update_variant, int rows_per_block, int nontemporal);
int dlp_session_get_tuning(dlp_session* s, int* update_variant, int* rows_per_block, int* nontemporal);
/* 1 when the session solves in the one-launch LDS path (options.small_lp), else 0. */
int dlp_session_small_lp(dlp_session* s, int* small_lp);
/* Lookahead sessions: the CUs the selection chain runs on, the pass on the others (0 = both
 * unmasked).  Auto from the rank's rows; DLP_CHAIN_CUS=n overrides. */
int dlp_session_chain_cus(dlp_session* s, int* cus);
/* Deferred sessions: workgroups per CU allowed for the tableau pass (LDS
 * reservation; 0 = no cap, the default) and its form (-1 = keep):
 *   LDS-staged coefficients: 0 = 2 doubles per lane (K <= 32), 1 / 2 = 1 double
 *   per lane x 2 / 4 rows per iteration;
 *   scalar-load coefficients: 3 = 1 double x 4 rows, 4 = 2 doubles x 2 rows
 *   (K <= 32), 5 = 1 double x 8 rows;
 *   streamed (buffer ops, dense-group ring; K < 16 runs form 3): 6-9 = XCD
 *   band-group order, 10-13 = tile-fastest order, 16-19 = XCD tile-range order,
 *   each as {2 doubles x 2 rows, ring 4 (K <= 32); 2 x 2, ring 2 (K <= 32);
 *   1 x 4, ring 4; 1 x 4, ring 2};
 *   14 = form 4 for full blocks + the streamed partial-block kernel (K <= 32),
 *   15 = the same with the full-block kernel held to 3 waves per SIMD,
 *   20 = form 4 with a 3-deep row prefetch ring (K <= 32),
 *   21 = DPP-broadcast coefficients, 1 double x 2 rows, K = 64 exactly (other K
 *   run form 3),
 *   22 = the same block on the matrix cores (v_mfma_f64_16x16x4f64), K = 64 exactly,
 *   23 = form 21's arithmetic with the rows and coefficients staged through a per-wave
 *   LDS ring by LDS-DMA (4 two-row groups in flight per wave), K = 64 exactly.
 * Default: 21 at K = 64 on a tableau > 1 GiB, 4 at K = 32 there and at K = 16
 * below, else 3.
 * rows_per_block (set_tuning) is the pass's row band (0 = auto: 768 rows at
 * K = 64 on a tableau > 1 GiB, 256 at smaller K there, 64 below).  Results are
 * bit-identical for every setting. */
int dlp_session_set_defer_tuning(dlp_session* s, int occupancy, int form);
/* Deferred single-rank sessions (K <= 32): run the ratio test, the selection
 * and the pivot row as one fused launch per pivot (1) or as two launches (0,
 * the default: the in-launch hand-off costs what the kernel boundary does).
 * Bit-identical either way; timing >= 2 (per-phase events) always uses two
 * launches. */
int dlp_session_set_fused_pivot(dlp_session* s, int on);
/* *on = 1 when the session runs lookahead (dlp_options.lookahead): block b+1 selected
 * while the pass of block b runs on a second tableau buffer.  The step API and pass
 * forms other than 3, 4, 5, 20, 21, 22 and 23 turn it off for the rest of the session. */
int dlp_session_get_lookahead(dlp_session* s, int* on);
/* ---- peer exchange -----------------------------------------------
 * Instead of the RCCL all-gather of the candidates and the int64 MAX all-reduce of the
 * pivot row, the ranks store their candidate into every rank's exchange block and the
 * pivot-row owner stores its row into every rank's block (xGMI peer writes between
 * devices), each message followed by a flag; the waits run inside the select / commit
 * kernels and are bounded.  Results are bit-identical to every other exchange.
 *   one process, any devices (incl. several ranks on ONE device):
 *     dlp_sessions_connect(ranks) once; then dlp_session_run per rank on its own host
 *     thread (distinct devices), or dlp_sessions_run(ranks) from one thread (required
 *     when ranks share a device: it enqueues every rank's sends before any rank's waits);
 *   one process per GPU: dlp_session_exchange_handle (64 B) on every rank, an all-gather
 *     of the handles by the caller, dlp_session_connect_ipc(handles[nranks]); or, with
 *     an RCCL id, dlp_session_set_exchange(s, DLP_XCHG_PEER) does that over RCCL.
 * dlp_session_set_exchange switches between the two on a session that has both (every
 * rank at the same point, between runs). */
#define DLP_XCHG_DEFAULT 0   /* dlp_options.exchange: peer where every rank pair connects, else RCCL */
#define DLP_XCHG_RCCL    1
#define DLP_XCHG_PEER    2
#define DLP_XCHG_HOST    3   /* dlp_session_get_exchange: caller-driven (dlp_session_step_*) */
int dlp_sessions_connect(dlp_session* const* ranks, int nranks);
int dlp_session_exchange_handle(dlp_session* s, void* out64);
int dlp_session_connect_ipc(dlp_session* s, const void* handles /* nranks x 64 B, rank order */);
/* The same connect from records that also carry each rank's device (PCI bus id): ranks that
 * share a device then split the lookahead's chain CUs into disjoint slices (dlp_session_chain_cus;
 * slices under 32 CUs turn the masks off for those ranks), which several rank processes on one
 * GPU need.  dlp_session_exchange_record fills DLP_XREC_BYTES (the exchange
 * block's IPC handle, the bus id); the caller all-gathers them in rank order.  The RCCL-agreed
 * connect (dlp_session_set_exchange / DLP_XCHG_DEFAULT) all-gathers the same records itself.
 * dlp_session_colocated: ranks of the session's exchange on its device (itself included) and its
 * index among them (1, 0 before a connect and after dlp_session_connect_ipc). */
#define DLP_XREC_BYTES 256
int dlp_session_exchange_record(dlp_session* s, void* out /* DLP_XREC_BYTES */);
int dlp_session_connect_records(dlp_session* s, const void* records /* nranks x DLP_XREC_BYTES, rank order */);
int dlp_session_colocated(dlp_session* s, int* n, int* index);
/* The tableau as stored: row stride, RHS column (N, or n when condensed) and whether it is the
 * condensed tableau.  dlp_session_info / _tableau / _read_rows always give the
 * full layout (N + 1 columns, basic columns as unit vectors). */
int dlp_session_storage(dlp_session* s, int64_t* ld, int64_t* ncols, int* condensed);
int dlp_session_set_exchange(dlp_session* s, int mode);
int dlp_session_get_exchange(dlp_session* s, int* mode);
/* Why an auto exchange (DLP_XCHG_DEFAULT) fell back to RCCL ("" when it did not). */
int dlp_session_exchange_reason(dlp_session* s, char* buf, size_t cap);
int dlp_sessions_run(dlp_session* const* ranks, int nranks, int64_t max_pivots, int64_t* pivots_done);

/* Failure containment on the exchange.  A session with an exchange
 * never blocks in a wait that a peer must end: its window waits poll the stream,
 * ncclCommGetAsyncError and an abort word; on an RCCL error, an abort request, a
 * peer-exchange wait that timed out, or a window not complete after `seconds` (the
 * exchange timeout: default 600; 0 = no limit) it raises the device abort word, calls
 * ncclCommAbort and dlp_session_run returns DLP_ERR_RCCL, the status of every exchange
 * failure (the session is then unusable; free it).  A device error returns DLP_ERR_HIP.
 * Each peer-exchange wait on the device is bounded by the same timeout + 5 s.
 * dlp_solve(n_gpus = N) aborts every rank's exchange when one rank fails and returns
 * that rank's error (with the auto exchange, after a failed peer run, the error of the
 * RCCL rerun).  dlp_session_abort may be called from any thread.
 * dlp_session_inject_fault (tests): the (after_polls+1)-th window wait fails as if the
 * exchange had died.
 * Freeing connected ranks: a rank's exchange block receives its peers' stores, so a
 * connected rank session may be freed only after every rank's stream has drained
 * (e.g. a barrier after the last run / result on every rank). */
int dlp_session_set_exchange_timeout(dlp_session* s, double seconds);
int dlp_session_abort(dlp_session* s);
int dlp_session_inject_fault(dlp_session* s, int64_t after_polls);
/* Current deferred-pass settings (K = 1: form -1). */
int dlp_session_get_defer_tuning(dlp_session* s, int* occupancy, int* form, int* K);
int dlp_session_info(dlp_session* s, int64_t* rows_local, int64_t* row_first, int64_t* ld,
                     int64_t* ncols);
/* Copy the local tableau (rows_local+1 rows x ld, objective last) to the host. */
int dlp_session_tableau(dlp_session* s, double* host);
/* Copy local rows [first, first+count) (row rows_local = objective) to the host. */
int dlp_session_read_rows(dlp_session* s, int64_t first, int64_t count, double* host);
int dlp_session_result(dlp_session* s, dlp_result** out);
/* One result for a row-block solve whose rank sessions all live in this
 * process (any order): x covers every basic variable (a single rank's
 * dlp_session_result covers its own rows only). */
int dlp_sessions_result(dlp_session* const* ranks, int nranks, dlp_result** out);
void dlp_session_free(dlp_session* s);

/* ---- batched small LPs ------------------
 * nlp independent LPs of size m x n, LP k generated on the device with seed
 * (seed + k) by the DLP_GEN_* family `kind`; one workgroup per LP solves it
 * with its whole tableau resident in LDS (rule as above, bit-identical to a
 * single-LP solve).  Per-LP outputs (NULL to skip): objective[nlp],
 * status[nlp], npivots[nlp], basis[nlp*m], logs[nlp*log_cap] (first log_cap
 * pivots of each LP).  *kernel_ms gets the solve kernel's device time.
 * Reference analog: the independent per-impression subproblems solved in a
 * loop, R/global_problem.cpp:270-274. */
int dlp_batched_solve(int kind, int64_t nlp, int64_t m, int64_t n, uint64_t seed,
                      const dlp_options* opt, double* objective, int32_t* status,
                      int64_t* npivots, int32_t* basis, dlp_pivot* logs, int64_t log_cap,
                      double* kernel_ms);
/* The same batch solve on the caller's own LPs: nlp independent problems
 *   max c_k^T x  s.t.  A_k x <= b_k, x >= 0, b_k >= 0,
 * all of one shape m x n (the per-impression subproblems themselves, not a
 * generated stand-in).  Pivot rule, tolerances and options are those of
 * dlp_batched_solve; every LP's pivot sequence is bit-identical to a
 * single-LP solve (dlp_problem_create_dense + dlp_solve).  The kernels read
 * A, b and c directly; no full-layout tableau is built in device memory.
 *
 * Inputs: A_k is m x n row-major without padding, LP k's arrays start
 * strideA / strideb / stridec doubles after LP k-1's.  A stride of 0 shares
 * one array between all LPs; any other stride must be at least m*n, m, n
 * (else DLP_ERR_ARG).  device = 0: host pointers (copied to the device on
 * every call: at 4096 x (64 x 128) that copy is 268 MB and costs far more
 * than the solve); device = 1: device pointers on opt->device whose contents
 * are complete when the call is made (the solve runs on the library's own
 * stream).
 *
 * Outputs: host pointers, NULL to skip.  objective, status, npivots, basis,
 * logs + log_cap and kernel_ms (the solve kernel's device time alone) as in
 * dlp_batched_solve; x[nlp*n] and y[nlp*m] with dlp_result_x / dlp_result_y's
 * meaning (x_j: the RHS of the row whose basic variable is j, else 0; y_i:
 * the reduced cost of slack n+i, 0 when it is basic), taken from the tableau
 * as it stands for every status, DLP_UNBOUNDED and DLP_PIVOT_LIMIT included.
 *
 * An LP with some b_i that is not >= 0 (negative or NaN) is not solved:
 * status[k] = DLP_ERR_ARG, npivots[k] = 0, objective[k] and its x and y NaN,
 * its basis the slack basis; the other LPs are solved and the call returns
 * DLP_OK.  Call-level errors, in this order: DLP_ERR_ARG (sizes, strides,
 * NULL inputs, nlp > 65535*16), DLP_ERR_NODEVICE, DLP_ERR_UNSUPPORTED (the
 * tableau does not fit 160 KiB of LDS). */
typedef struct dlp_batch_dense_in {
    const double* A;       /* nlp (or 1) x m x n */
    const double* b;       /* nlp (or 1) x m */
    const double* c;       /* nlp (or 1) x n */
    int64_t strideA, strideb, stridec;   /* doubles between consecutive LPs; 0 = shared */
    int32_t device;        /* 0 host pointers, 1 device pointers on opt->device */
    int32_t pad_;
} dlp_batch_dense_in;
typedef struct dlp_batch_out {
    double*    objective;  /* [nlp] */
    int32_t*   status;     /* [nlp] */
    int64_t*   npivots;    /* [nlp] */
    int32_t*   basis;      /* [nlp*m] */
    dlp_pivot* logs;       /* [nlp*log_cap] */
    int64_t    log_cap;
    double*    x;          /* [nlp*n] */
    double*    y;          /* [nlp*m] */
    double*    kernel_ms;  /* [1] */
} dlp_batch_out;
int dlp_batched_solve_dense(int64_t nlp, int64_t m, int64_t n, const dlp_batch_dense_in* in,
                            const dlp_options* opt, const dlp_batch_out* out);
/* The batch kernel dlp_batched_solve runs for m x n LPs on `device`: lanes per LP, LPs one CU
 * holds at once (VGPR / LDS occupancy) and whether it is the register-resident kernel (m = 64,
 * n <= 192) or the LDS one.  C5 is bound by per-pivot serial latency x this residency. */
int dlp_batched_occupancy(int64_t m, int64_t n, int device, int32_t* lps_per_cu,
                          int32_t* threads_per_lp, int32_t* register_kernel);

/* ---- resident batch: re-solve the same LPs after new objectives --------
 * The reference re-weights the objective of all its per-impression subproblems on every
 * iteration (R/allocation_mw.cpp:271-326 over R/global_problem.cpp:270-274).  A dlp_batch keeps
 * every LP's final state (condensed tableau, basis, Bland flag, status) on the device between
 * calls, so an iteration re-optimises each LP from its current basis instead of solving it
 * cold, and A is uploaded once.  Every LP stays bit-identical to the single-LP path: a cold
 * dlp_solve, then dlp_session_set_objective + dlp_session_run.
 *
 * Rejected LPs: an LP rejected at creation (some b_i not >= 0) stays DLP_ERR_ARG with NaN
 *   objective, x and y and the slack basis in every later call.
 * Non-finite c_k: a c_k with an entry that is not finite makes that LP alone report
 *   DLP_ERR_ARG with NaN objective, x and y (0 pivots, its basis as it stands) for this call;
 *   its resident state is left exactly as it was and the other LPs run.  The kernel checks
 *   this, for host and device c alike (a device input cannot be checked on the host).
 * Call-level errors are validated before anything is enqueued and leave the batch unchanged:
 *   DLP_ERR_ARG (NULL batch, a stride that is neither 0 nor >= n, c_is_device not 0 / 1,
 *   negative max_pivots or log_cap); at creation also DLP_ERR_OOM when the state does not fit
 *   in device memory.
 * max_pivots == 0 with a c rebuilds the objective rows and does no pivot: status
 *   DLP_PIVOT_LIMIT, as every batch kernel reports a zero budget.
 * Handles: a handle is not thread-safe.  Its state buffers belong to the handle
 *   (dlp_batch_info's device_bytes); dlp_release_cached_memory does not touch them. */
typedef struct dlp_batch dlp_batch;

/* Cold solve exactly as dlp_batched_solve_dense (same inputs, options, outputs, per-LP
 * DLP_ERR_ARG for a b_i that is not >= 0, same call-level errors in the same order), and keep
 * every LP's final state on the device.  out may be NULL.  A, b and c are not read after the
 * call returns. */
int dlp_batch_create_dense(int64_t nlp, int64_t m, int64_t n, const dlp_batch_dense_in* in,
                           const dlp_options* opt, const dlp_batch_out* out, dlp_batch** batch);
/* Continue every LP from its resident basis for up to max_pivots more pivots (per LP, this call).
 *   c != NULL: first replace LP k's objective by max c_k^T x (c_k at c + k*stridec, n doubles;
 *     stridec 0 = one c for all LPs, else >= n; c_is_device 0 host / 1 device pointer on the
 *     batch's device, complete when the call is made) by the rule of dlp_session_set_objective
 *     applied to LP k's tableau, reset the Bland state as that call does, status RUNNING
 *     whatever it was (optimal, unbounded, pivot limit).
 *   c == NULL: resume with the objective row and Bland state as they stand; an LP that is
 *     optimal or unbounded does 0 pivots and reports that status again.
 * out as in dlp_batched_solve_dense (may be NULL); npivots and logs are this call's pivots;
 * objective, x, y, basis from the tableau as it stands afterwards.  Tolerances, pricing and
 * device are those of creation. */
int dlp_batch_resolve(dlp_batch* batch, const double* c, int64_t stridec, int c_is_device,
                      int64_t max_pivots, const dlp_batch_out* out);
/* Re-solve every resident LP after new right-hand sides, by the dual simplex.
 * After a primal solve the resident tableau is dual feasible for every b, so the dual simplex
 * continues from it; it pays when b moves a little (budgets, capacities) and the basis mostly
 * stays.  LP k's new right-hand side is b_k at b + k*strideb, m doubles (strideb 0 = one b for
 * all LPs, else >= m; b_is_device 0 host / 1 device pointer on the batch's device, complete when
 * the call is made).  Any finite value is allowed, negative ones included.  Tolerances, pricing
 * and device are those of creation.  out as in dlp_batch_resolve: npivots and logs are this
 * call's pivots; objective, x, y and basis come from the tableau as it stands afterwards.
 *
 * RHS rebuild.  In the full layout the slack columns are B^-1.  For every stored row
 *   r = 0 .. m (the objective row included: its entry is the new objective value):
 *     acc = +0.0;  for l = 0 .. m-1 ascending: acc = acc + (Tfull[r][n+l] * b_l)
 *     (the product rounded, then the sum: no fma);  T[r][N] = acc.
 *   Tfull[.][n+l] is slack l's stored slot when it is nonbasic, the unit vector of its row with
 *   objective entry +0.0 when it is basic.  (A term whose coefficient is +-0 cannot change a
 *   bit: acc starts at +0.0, and a sum is -0.0 only if both operands are.)  One ascending fold
 *   per row: the result depends on nothing but the variable indices.
 * Dual pivot.  Every nonbasic variable (stored slot) is a candidate.
 *   Leaving row: row i < m is eligible when T[i][N] < -tol_feas (dlp_options.tol_feas of
 *     creation, absolute here).  p = argmin T[i][N] over the eligible rows, exact ties to the
 *     smallest basis[i]; in Bland mode the eligible row with the smallest basis[i].
 *   Stops: no eligible row -> DLP_OK (dual and primal feasible).  This test comes before the
 *     budget test: max_pivots == 0 reports DLP_OK on an LP that needs no pivot and
 *     DLP_PIVOT_LIMIT on one that needs some.
 *   Entering slot: slots s with a = T[p][s] < -tol_piv; r_s = zc / (-a) by IEEE division, where
 *     zc = z_s if z_s > 0 else +0.0 (the primal's clamp of its RHS); q = argmin r_s, exact ties
 *     to the smallest variable index.  No such slot -> DLP_INFEASIBLE.
 *   Update: exactly the primal one with the negative pivot T[p][q] (division for the pivot row,
 *     fma elimination, rows with T[i][q] == 0 untouched, the entering slot takes the leaving
 *     variable's column, var and basis swapped).
 *   Log entry: q, p, leaving, ratio = r_q, objective after the pivot.
 *   Bland state: reset at the call (on for DLP_PRICING_BLAND, else off), entered after a pivot
 *     with r_q == 0 and left after one with r_q > 0.
 *   The dual phase does not fall through into a primal phase.
 * Per-LP outcomes, checked in the kernel (host and device b alike) in this order; each leaves
 *   that LP's resident state bit for bit as it was, and the other LPs run:
 *   1. rejected at creation: DLP_ERR_ARG, NaN objective / x / y, the slack basis;
 *   2. a b_k entry that is not finite: DLP_ERR_ARG, NaN values, 0 pivots, the basis as it stands;
 *   3. not dual feasible, some stored slot has z_s < -tol_dj (an LP stopped inside a primal
 *      solve, or unbounded): DLP_ERR_STATE, NaN values, 0 pivots, the basis as it stands.
 * State afterwards: an LP left DLP_INFEASIBLE, or stopped by the budget inside the dual phase
 *   (reported DLP_PIVOT_LIMIT), has negative RHS entries.  dlp_batch_resolve (with or without c)
 *   reports DLP_ERR_STATE for it (NaN values, 0 pivots, the basis as it stands, state
 *   untouched); dlp_batch_resolve_rhs accepts it again: a later b may make it feasible, more
 *   budget may finish it.  After DLP_OK, dlp_batch_resolve behaves as after any optimal solve.
 * Continuation: an LP whose dual phase the budget stopped, handed the very b_k of that call
 *   again (every entry bit for bit; the batch keeps each LP's last accepted b_k), goes on from
 *   its RHS column and its Bland state as they stand, without a rebuild: budgets of any size
 *   give the pivots, basis and objective bits of one unbounded call.  (A rebuilt column equals
 *   the updated one only up to rounding.)  Any other b_k, and every LP that is not pending,
 *   takes the rebuild and the reset above.
 * Call-level errors (validated before anything is enqueued, the batch unchanged): DLP_ERR_ARG
 *   for a NULL batch or b, a stride that is neither 0 nor >= m, b_is_device not 0 / 1, negative
 *   max_pivots or log_cap.
 * Kernel: at m = 64, n <= 192 the call runs the register-resident kernel, as creation and
 *   dlp_batch_resolve do; at every other shape, or with DLP_BATCH_LDS=1 or
 *   DLP_BATCH_RHS_LDS=1 in the environment, the LDS kernel.  Both give the same bits;
 *   dlp_batch_rhs_kernel says which one runs.
 * Not covered: changes of A other than new rows and new columns (dlp_batch_add_rows,
 * dlp_batch_add_cols, below), c and b in one call, general LPs.  (Single sessions:
 * dlp_session_set_rhs applies this rule to an eager session's tableau, dlp_session_set_rhs_in_place
 * to a session on any storage path.) */
int dlp_batch_resolve_rhs(dlp_batch* batch, const double* b, int64_t strideb, int b_is_device,
                          int64_t max_pivots, const dlp_batch_out* out);
/* The kernel dlp_batch_resolve_rhs runs for this batch: *register_kernel 1 the register-resident
 * kernel, 0 the LDS kernel; how many LPs one CU of the batch's device holds of it at once (the
 * occupancy query on that very instantiation) and its threads per LP.  NULL outputs are skipped;
 * a NULL batch is DLP_ERR_ARG.  (dlp_batch_info's register_kernel stays the kernel of creation
 * and of dlp_batch_resolve; both follow the grown shape after dlp_batch_add_rows and
 * dlp_batch_add_cols.) */
int dlp_batch_rhs_kernel(const dlp_batch* batch, int32_t* register_kernel, int32_t* lps_per_cu,
                         int32_t* threads_per_lp);
/* Add r constraint rows to every resident LP and re-solve warm by the dual simplex (DESIGN.md
 * §25): LP k gains G_k x <= h_k, G_k r x n row-major at G + k*strideG (strideG 0 = one G for all
 * LPs, else >= r*n), h_k r doubles at h + k*strideh (0 = shared, else >= r); rows_are_device 0
 * host / 1 device pointers on the batch's device, complete when the call is made.  Any finite
 * value is allowed, negative h included.  The batch's m becomes m + r; n and every existing
 * variable index stay.  New row t is row m + t, its slack variable n + m + t, basic in that row
 * (no column is added: the record's row stride n + 1 stays).  Then the dual simplex of
 * dlp_batch_resolve_rhs continues from the tableau as it then stands: its leaving-row rule,
 * entering-slot rule, update, log entry, Bland rule and stops ("no eligible row" before the
 * budget, never a primal phase), with the tol_feas, tol_piv, tol_dj and pricing of creation.
 * out as in dlp_batch_resolve_rhs: basis and y have m + r entries per LP, npivots and the logs
 * are this call's.
 *
 * Row rule.  For LP k and new row t let g be row t of G_k and, for the old rows i < m,
 *   gB_i = g[basis[i]] if basis[i] < n, else +0.0.  For every stored slot s (variable v = var[s])
 *   and for the RHS:
 *     acc = g_v for a structural v < n, +0.0 for a slack, h_t for the RHS;
 *     for i = 0 .. m-1 ascending, rows with gB_i == 0.0 skipped: acc = acc - (gB_i * T[i][s])
 *     (the product rounded, then the difference: no fma);  T[m+t][s] = acc.
 *   One ascending fold per entry, over the OLD rows only (the new rows do not see each other):
 *   no atomics, no tree, nothing that depends on the launch.  Old constraint rows and the
 *   objective row keep their bits; the objective row becomes row m + r.  basis[m+t] = n + m + t;
 *   var[] is unchanged.  In dlp_batch_read's layout (now (m+r+1) x dlp_tableau_ld(m+r, n)) a new
 *   row has +0.0 in every basic column and 1.0 at its own slack, old rows +0.0 in the new slack
 *   columns.  The Bland state is reset as dlp_batch_resolve_rhs resets it.
 * r == 0 (G, h may be NULL) adds nothing and continues every LP's dual phase from the tableau as
 *   it stands: a pending LP with its stored Bland state, the others with a reset one.  A budget
 *   of 1 followed by r == 0 calls gives the pivots, basis and objective bits of one unbounded
 *   call.  r > 0 invalidates the record of each LP's last b_k (no finite b matches it): a later
 *   dlp_batch_resolve_rhs always rebuilds, from a b of m + r entries.
 * Per-LP outcomes, checked in the kernel in this order:
 *   1. rejected at creation: stays rejected in the new shape (DLP_ERR_ARG, NaN values, the slack
 *      basis of length m + r);
 *   2. not dual feasible, some stored z_s < -tol_dj (an LP stopped inside a primal solve, or
 *      unbounded): the rows are still added by the rule (it holds for any basis), no pivot is
 *      done, this call reports DLP_ERR_STATE with NaN values and the basis as it stands.  If no
 *      new RHS entry lies below -tol_feas the stored status stays as it was, so dlp_batch_resolve
 *      can continue or restart its primal solve on the larger LP; otherwise the record is stored
 *      pending and both later resolve calls refuse it: such an LP is solved cold;
 *   3. DLP_INFEASIBLE or pending from an earlier dual phase: accepted, the rows are added and
 *      the dual phase runs again.
 * Call-level errors leave the batch bit for bit as it was and out untouched, in this order:
 *   DLP_ERR_ARG (NULL batch, r < 0, r > 0 with NULL G or h, a stride that is neither 0 nor
 *   >= r*n / r, rows_are_device not 0 / 1, negative max_pivots or log_cap); DLP_ERR_UNSUPPORTED
 *   (the grown tableau does not fit 160 KiB of LDS by the launch's formula); DLP_ERR_OOM (the new
 *   buffers do not fit); DLP_ERR_ARG with the first offending LP named in dlp_last_error when a
 *   G_k / h_k entry is not finite (checked in the kernel, host and device rows alike: the kernel
 *   writes the grown records into new buffers, which the handle takes only when no LP raised
 *   the flag, so a shape change is all or nothing).
 * Afterwards dlp_batch_info reports m + r and the new device_bytes, and its register_kernel and
 *   dlp_batch_rhs_kernel follow the new shape: a batch grown from m = 64 leaves the register
 *   kernel for its later resolve calls (it pays the LDS kernel's per-pivot cost from then on), one
 *   grown from 63 to 64 rows gains it (both kernels share the record layout).  This call itself
 *   always runs the LDS kernel.
 * Not covered: removing rows, changing entries of existing rows, general LPs.  (Adding columns:
 * dlp_batch_add_cols, below.) */
int dlp_batch_add_rows(dlp_batch* batch, int64_t r, const double* G, int64_t strideG, const double* h,
                       int64_t strideh, int rows_are_device, int64_t max_pivots, const dlp_batch_out* out);
/* Add k structural variables (columns) to every resident LP and re-solve warm by the primal
 * simplex: LP j becomes  max [c d]^T [x; w]  s.t.  [A_j | P_j][x; w] <= b_j,
 * P_j m x k row-major at P + j*strideP (A's layout: concatenating A_j and P_j along the columns
 * gives the stacked LP; strideP 0 = one P for all LPs, else >= m*k), d_j k doubles at
 * d + j*strided (0 = shared, else >= k); cols_are_device 0 host / 1 device pointers on the
 * batch's device, complete when the call is made.  Any finite value is allowed, negative entries
 * and costs included.  m is the batch's current m (after any dlp_batch_add_rows).  The batch's n
 * becomes n + k and the batch is from then on exactly a batch of shape m x (n + k): structural
 * indices 0 .. n-1 keep their meaning, the new variables are n .. n+k-1, slack i is renamed from
 * n + i to n + k + i (order-preserving: every tie rule by variable index keeps its order among
 * the old variables).  dlp_batch_read gives (m+1) x dlp_tableau_ld(m, n+k) with the new columns
 * at n .. n+k-1.  A new variable enters nonbasic at 0, so the resident basis stays primal
 * feasible, and the primal loop of dlp_batch_resolve(c = NULL) continues on the widened tableau:
 * every accepted LP starts with status DLP_RUNNING whatever it was (optimal, unbounded, pivot
 * limit), the Bland state reset from the pricing option, the tolerances of creation.  A budget
 * stop reports DLP_PIVOT_LIMIT and dlp_batch_resolve(NULL) continues it: a budget of 1 followed
 * by dlp_batch_resolve(NULL) calls gives the bits of one unbounded call.  out as in
 * dlp_batch_resolve: x has n + k entries per LP, y and basis m; npivots and the logs are this call's.
 *
 * Column rule.  For LP j and new variable t let p be column t of P_j.  For every stored row
 *   r = 0 .. m (the objective row included):
 *     acc = +0.0;  for l = 0 .. m-1 ascending: acc = acc + (Tfull[r][n+l] * p_l)
 *     (the product rounded, then the sum: no fma), Tfull[.][n+l] slack l's stored slot when it is
 *     nonbasic, its row's unit vector with objective entry +0.0 when it is basic (as in
 *     dlp_batch_resolve_rhs's RHS rule; a +-0 coefficient changes no bit and may be skipped);
 *     constraint rows: T[r][new] = acc;  objective row: z_new = acc - d_t (one more rounded
 *     subtraction), so on the slack basis the column is p and z = -d_t up to the sign of a zero.
 *   One ascending chain per entry: no atomics, no tree, nothing that depends on the launch; the
 *   new columns do not see each other.  Old slots, the RHS, the objective value, the basis and
 *   every LP's last b_k keep their bits; in var[] and basis[] every index >= the old n goes up
 *   by k; the new variables take the new slots n .. n+k-1 of the record (row stride n + k + 1).
 * k == 0 (P, d may be NULL) is dlp_batch_resolve(batch, NULL, 0, 0, max_pivots, out) exactly.
 * Per-LP outcomes, checked in the kernel in this order (the record is always written in the new
 *   shape: a shape change is all or nothing):
 *   1. rejected at creation: stays DLP_ERR_ARG, NaN values, the slack basis with the renamed
 *      indices;
 *   2. stored status DLP_INFEASIBLE or a pending dual phase (the RHS has negative entries): the
 *      columns are added by the rule (it holds for any basis), no pivot is done, this call
 *      reports DLP_ERR_STATE with NaN values and the basis as it stands.  The stored status, the
 *      Bland state and the last b_k stay, so dlp_batch_resolve_rhs or dlp_batch_add_rows(r = 0)
 *      continue the dual phase on the wider LP if it is still dual feasible, and refuse it by
 *      their own rule otherwise.
 * Call-level errors leave the batch bit for bit as it was and out untouched, in this order:
 *   DLP_ERR_ARG (NULL batch, k < 0, k > 0 with NULL P or d, a stride that is neither 0 nor
 *   >= m*k / k, cols_are_device not 0 / 1, negative max_pivots or log_cap); DLP_ERR_UNSUPPORTED
 *   (the m x (n+k) tableau does not fit 160 KiB of LDS by the launch's formula); DLP_ERR_OOM (the
 *   new buffers do not fit); DLP_ERR_ARG with the first offending LP named in dlp_last_error when
 *   a P_j / d_j entry is not finite (checked in the kernel, host and device columns alike, by
 *   dlp_batch_add_rows's mechanism: new buffers, taken by the handle only when no LP raised the
 *   flag).
 * Afterwards dlp_batch_info reports n + k and the new device_bytes, and its register_kernel and
 *   dlp_batch_rhs_kernel follow the new shape: a batch with m = 64 keeps the register kernel for
 *   its later resolve calls while n + k <= 192 and leaves it beyond.  This call itself always
 *   runs the LDS kernel.
 * Not covered: removing columns, changing entries of existing columns, general LPs.  (A single
 * session: dlp_session_add_cols.) */
int dlp_batch_add_cols(dlp_batch* batch, int64_t k, const double* P, int64_t strideP, const double* d,
                       int64_t strided, int cols_are_device, int64_t max_pivots, const dlp_batch_out* out);
/* LP k's resident tableau in the full layout of dlp_session_tableau ((m+1) x dlp_tableau_ld(m,n),
 * basic columns as exact unit vectors, their objective entries +0.0, padding +0.0) and its
 * basis (m entries).  Either pointer may be NULL. */
int  dlp_batch_read(dlp_batch* batch, int64_t k, double* T, int32_t* basis);
int  dlp_batch_info(const dlp_batch* batch, int64_t* nlp, int64_t* m, int64_t* n,
                    int32_t* register_kernel, int64_t* device_bytes);
void dlp_batch_free(dlp_batch* batch);   /* NULL is a no-op */

/* ---- multiplicative-weights path ------------------
 * The reference's own epsilon-approximate MW loop (R/allocation_mw.cpp:271-326,
 * sort or binary-search mode) on the GPU for an ad-allocation problem (dlp_problem_create_adalloc),
 * with the fp64 spec of DESIGN.md §9 (fixed tie orders, fixed-order sums,
 * deterministic exp): per impression an upper envelope (wave-level bitonic
 * sort + monotone chain), a global slope sort (hipCUB radix sort), a blocked
 * budget prefix, primal construction, per-advertiser slacks and weights.
 * Scales to the reference's 100k x 1M x 1e-4 scenario, where a dense tableau
 * cannot exist.  Replaces Instance::RunMultiplicativeWeights(T, tol, binary[, scale,
 * intervals]) (R/instance.h:52-55, R/instance.cpp:117-141). */
typedef struct dlp_mw dlp_mw;
typedef struct dlp_mw_options {
    int32_t device;
    int32_t binary;        /* 0 sort mode (R/global_problem.cpp:224-255); 1 threshold search
                              (R/global_problem.cpp:46-222, the mode R/main.cpp:36 runs) with the
                              fp64 stop of DESIGN.md §9 (1e-16 is below fp64 resolution) */
    double  epsilon;       /* default 0.01 (R/main.cpp:33) */
    double  tolerance;     /* numerical_accuracy_tolerance, default 1e-18; tight-set test uses max(tol, 1e-12) */
    double  scale;         /* binary: cr_transition_scale; <= 0 -> 1 - epsilon * 0.001 (R/main.cpp:38) */
    int32_t intervals;     /* binary: critical ratios per level, 1..8, default 3 (R/main.cpp:37) */
    int32_t pad_;
} dlp_mw_options;
typedef struct dlp_mw_iter {   /* per-iteration report (the reference's stdout, R/global_problem.cpp:320,
                                  R/allocation_mw.cpp:214-220,264-268) */
    double  dual_value;
    double  max_infeasibility;
    int32_t infeasible_advertiser;
    int32_t search_levels;     /* binary mode: threshold-search levels this iteration; 0 in sort mode */
    double  min_weight, max_weight, weighted_budget;
} dlp_mw_iter;
void dlp_mw_options_default(dlp_mw_options* opt);
/* Refused before the device is touched (text in dlp_last_error): DLP_ERR_ARG for a problem that
 * is not an ad-allocation problem, one without impressions or without bids (bid_sparsity 0),
 * binary mode with intervals outside 1..8, epsilon outside (0, 1); DLP_ERR_UNSUPPORTED for an
 * impression with more than 1023 bids (1024 points with the origin). */
int  dlp_mw_create(const dlp_problem* adalloc, const dlp_mw_options* opt, dlp_mw** out);
/* Run `iterations` more MW iterations; log (may be NULL) gets one entry per iteration;
 * *kernel_ms (may be NULL) the device time of the run. */
int  dlp_mw_run(dlp_mw* mw, int iterations, dlp_mw_iter* log, double* kernel_ms);
/* Averaged and last-iteration primal x in the problem's variable order
 * (dlp_problem_adalloc_bids), and the advertiser weights; NULL pointers skipped. */
int  dlp_mw_solution(dlp_mw* mw, double* x_avg, double* x_current, double* weights);
void dlp_mw_free(dlp_mw* mw);

/* ---- results ------------------------------------------------------------- */
int     dlp_result_status(const dlp_result* r);
double  dlp_result_objective(const dlp_result* r);
int64_t dlp_result_num_pivots(const dlp_result* r);
/* x (n, this rank's basic rows only when nranks > 1), y (m, duals), basis
 * (m_basis).  Dense problems: y_i = z_{n+i}, the max-form dual of row i. */
int dlp_result_x(const dlp_result* r, double* x, int64_t n);
int dlp_result_y(const dlp_result* r, double* y, int64_t m);
int dlp_result_basis(const dlp_result* r, int32_t* basis, int64_t m /* = m_basis */);
/* m_basis: basis length (standard-form rows; m for dense problems);
 * phase1_pivots: pivots of Phase I incl. the artificial drive-out (0 without). */
int dlp_result_info(const dlp_result* r, int64_t* m_basis, int64_t* phase1_pivots);
int dlp_result_pivot_log(const dlp_result* r, dlp_pivot* log, int64_t cap, int64_t* count);
int dlp_result_timings(const dlp_result* r, double* ms_out /* DLP_NUM_PHASES */);
/* dlp_solve(n_gpus >= 1) only: the exchange the result came from (DLP_XCHG_PEER or
 * DLP_XCHG_RCCL; DLP_XCHG_DEFAULT for every other result) and, into reason (cap bytes, NUL
 * terminated), why it is not the peer exchange: the auto exchange could not connect the
 * devices, or the peer run failed and the solve was rerun from the start over RCCL. */
int dlp_result_exchange(const dlp_result* r, int* mode, char* reason, int64_t cap);
void dlp_result_free(dlp_result* r);

#ifdef __cplusplus
}
#endif
#endif /* DLP_H */
