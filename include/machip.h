/*
 * machip.h -- C ABI of libmachip.so, the MI355X (gfx950) implementation of the
 * Frank-Wolfe / Fiedler hot path of MarineRoboticsGroup/mac.
 *
 * Plain C, no torch / numpy types: pointers + sizes only.  Host pointers are
 * borrowed for the duration of a call; all device memory is owned by the
 * handle.  Every function returns a machip_status (0 = OK) and never throws;
 * machip_last_error() gives the text of the last failure on this thread.
 * A handle is not thread-safe; distinct handles are independent (one HIP
 * stream each).
 *
 * Each entry point names the reference interface it replaces (paths relative
 * to the reference repository; "nx:" = networkx 3.4.2
 * networkx/linalg/algebraicconnectivity.py, the third-party module the
 * reference delegates the eigen-solve to).  The reference-side binding is
 * shown in INTEGRATION.md.
 */
#ifndef MACHIP_H
#define MACHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MACHIP_ABI_VERSION 21   /* 21: GreedyKirchhoff on the dense machip_esp handle (machip_esp_kirchhoff_select, _gains, _eval: greedy A-optimal selection and the total effective resistance of any selection); 20: option pairs_precond (preconditioned deflated columns of machip_lowest_pairs), machip_lowest_pairs_info, machip_lowest_pairs_csr2; 19: machip_lowest_pairs, machip_lowest_pairs_csr (the q lowest non-trivial eigenpairs, every one converged to the stop rule; option pairs_vcap), machip_lowest_pairs_time, machip_gradient_block; 18: machip_eig_exchange_free (the exchange on lambda_2 on MACHIP_EIG_MATRIX_FREE / _TREE handles; option eig_xch_free_swaps), machip_eig_history; 17: MACHIP_EIG_MATRIX_FREE_TREE (GreedyEig on any connected fixed graph without a dense Sigma; machip_eig_seeds); 16: MACHIP_EIG_MATRIX_FREE (GreedyEig on a chain without a dense Sigma; options eig_free_rows, eig_free_split); 15: machip_eig_exchange (best-swap local search on lambda_2; option eig_xch_max_mb); 14: machip_esp_exchange_edge (the exchange in the candidates' space on MACHIP_ESP_EDGE_RELAX / MACHIP_ESP_EDGE_RELAX_TREE handles); 13: machip_esp_exchange (best-swap local search on the log tree count; options esp_xch_lds_kb, esp_xch_max_mb, esp_xch_profile); 12: MACHIP_ESP_EDGE_RELAX (the relaxation in the candidates' space on a chain-fixed graph; machip_esp_relax_info); 11: MACHIP_ESP_SPANNING_TREE (the matrix-free route of GreedyESP for any connected fixed graph; machip_esp_tree_plan, machip_esp_seeds); 10: MACHIP_ESP_MATRIX_FREE (GreedyESP on a chain without a dense Sigma, option esp_free_split); 9: the relaxation of GreedyESP's problem (machip_esp_relax_*); 8: GreedyEig handle (machip_eig_*); 7: GreedyESP handle (machip_esp_*); 6: machip_solve_stats.drift, machip_panel_plan fills 12 entries; 5: per-handle option table (machip_set_option), machip_comm_drop_ipc; 4: inter-process communicator */

typedef enum machip_status {
    MACHIP_OK = 0,
    MACHIP_NOT_CONVERGED = 1, /* iteration cap hit (the reference would spin, nx:236)     */
    MACHIP_DISCONNECTED = 2,  /* lambda_2 ~ 0: graph not connected (reference: SuperLU
                                 "Factor is exactly singular" RuntimeError)               */
    MACHIP_BAD_ARG = 3,       /* reference: AssertionError (mac.py:47,52,183; fiedler.py:35) */
    MACHIP_HIP_ERROR = 4,
    MACHIP_RCCL_ERROR = 5,
    MACHIP_NO_DEVICE = 6
} machip_status;

typedef struct machip_problem machip_problem; /* one MAC instance (mac/solvers/mac.py:16)  */

/* Statistics of the last eigen-solve (n_mv, n_vec counters). */
typedef struct machip_solve_stats {
    int64_t lanczos_steps; /* Lanczos steps the solve used: up to the analysis point it ended at
                            * (a function of the records alone, round 5); steps_timed counts the
                            * launches, a few more when the queue ran past that point              */
    int64_t spmv_total;    /* + SpMVs of the explicit residual checks                      */
    int64_t vec_passes;    /* length-n vector reads+writes outside the SpMV                */
    int64_t restarts;
    int64_t nnz;           /* nnz of the assembled L(x) (diagonal included)                */
    int64_t support;       /* |{k : x_k > min_selection_weight_tol}|                       */
    double residual;       /* ||L v - lambda v||_1 / ||L||_inf  (the reference's stop rule,
                              nx:232,246)                                                  */
    double lnorm;          /* ||L||_inf                                                    */
    double gpu_ms;         /* device time of the solve (hipEvents on the handle's stream)  */
    double step_ms;        /* ... of which the Krylov chunks alone (events bracketing the
                              step kernels; explicit checks / Ritz vector excluded)        */
    int64_t steps_timed;   /* steps covered by step_ms: step_ms / steps_timed = in-solve
                              duration of one fused step launch                            */
    int64_t steps_lowp;    /* of lanczos_steps, those run with fp32 storage
                              (machip_set_precision(1)); the rest are fp64                 */
    double drift;          /* column-panel steps with an 8-byte operand (mac_amd/csrc/panel_u.h):
                              largest accumulated factor by which a rounding error of the
                              recurred product L v_j was carried forward, from the tridiagonal
                              records (0: the solve took no such step); beyond option
                              "panel_u_amp" (1e5) the sequence ends and the solve goes on
                              in the two-kernel form                                        */
} machip_solve_stats;

int machip_version(void);
int machip_sizeof_stats(void);             /* sizeof(machip_solve_stats): binding layout check */
int machip_device_count(void);            /* 0 when no GPU is visible                      */
const char* machip_last_error(void);

/* MAC.__init__ (mac/solvers/mac.py:22-72): fixed + candidate edge lists (SoA,
 * int32 node ids in [0,n)), n nodes.  Builds the union sparsity pattern once and
 * keeps weights / edge lists resident in HBM.  Duplicate pairs are summed exactly
 * as coo->csr does (mac/utils/graphs.py:48,98). */
int machip_create(int device, int64_t n,
                  int64_t n_fixed, const int32_t* fi, const int32_t* fj, const double* fw,
                  int64_t m, const int32_t* ci, const int32_t* cj, const double* cw,
                  double min_selection_weight_tol, machip_problem** out);
void machip_destroy(machip_problem* p);

/* x <- host vector (m doubles); x -> host.  (The reference passes x by value
 * into MAC.laplacian / problem / evaluate_objective, mac.py:74,91,104.) */
int machip_set_x(machip_problem* p, const double* x);
int machip_get_x(machip_problem* p, double* x);

/* MAC.laplacian(x) (mac.py:74-89): assemble L(x) = L_fixed + sum_{x_k>tol} x_k w_k L_k
 * on the device as CSR.  nnz_out may be NULL. */
int machip_assemble(machip_problem* p, int64_t* nnz_out);
/* Copy the assembled CSR to the host (indptr n+1, indices nnz, data nnz; the
 * diagonal is the first entry of each row, the rest sorted by column). */
int machip_get_laplacian(machip_problem* p, int32_t* indptr, int32_t* indices, double* data);

/* find_fiedler_pair on the assembled L(x) (mac/utils/fiedler.py:9-44 ->
 * nx:151-256).  Stop rule identical to the reference: ||L v - lambda v||_1 /
 * ||L||_inf < tol.  x0: optional start vector (n doubles, host) -- the drop-in
 * passes column 0 of the reference's RandomState(7) block; NULL + warm_start!=0
 * reuses the previous Fiedler vector resident on the device (the working form of
 * MAC.Cache, mac.py:17-20); NULL + warm_start==0 uses a fixed device-side
 * pseudo-random vector.  v_out (n) and X_out (n*q, column-major) may be NULL;
 * q in [1,4] columns are produced when X_out != NULL.  ONLY COLUMN 0 OBEYS THE STOP RULE
 * (it is v_out).  Columns 1..q-1 are what the reference's block X carries along (fiedler.py:44,
 * nx:238) -- there q vectors converge together; here they are the next Ritz vectors of the LAST
 * Krylov sequence of the solve, orthonormalised against column 0 and against 1: guaranteed
 * orthonormal, orthogonal to the constant vector, with Rayleigh quotients >= lambda_2; how close
 * they are to v_3, v_4, ... depends on that sequence alone -- after a few hundred steps they are
 * accurate to 1e-3 .. 1e-7 (tests: er2000_x0), after a short sequence (a restart from an almost
 * converged vector, 33 steps on er300_x0) or after the preconditioned / exact modes, which keep
 * no Krylov basis, they are an arbitrary orthonormal completion.  A caller that needs more than
 * the Fiedler pair must not take them for eigenvectors: machip_lowest_pairs (below) returns q
 * eigenpairs that each obey the stop rule. */
int machip_fiedler(machip_problem* p, double tol, int max_steps, const double* x0, int warm_start,
                   double* lambda2, double* v_out, double* X_out, int q,
                   machip_solve_stats* stats);

/* The q lowest non-trivial eigenpairs of the assembled L(x), 1 <= q <= min(16, n - 1): EVERY column obeys the stop rule
 * ||L v - lambda v||_1 / ||L||_inf < tol with ||v||_2 = 1; the values ascend, the vectors are mutually orthonormal and orthogonal to
 * the constant vector.  Column 0 is what machip_fiedler computes for the same start vector and tolerance (same mode choice, same
 * bits); columns 1 .. q-1 come one after the other from a Lanczos recurrence on L restricted to the complement of the constant
 * vector and the columns found so far (mac_amd/csrc/solver_pairs.h; fp64 whatever machip_set_precision says, no
 * preconditioner), each from a fresh start vector, so exact multiplicities come out.  The q values are then sorted (stable).  If
 * column 0 did not end up first, the Fiedler solve had returned a true but higher eigenpair: *reordered_out = 1 and
 * *first_rank_out = the number of columns whose value lies below column 0's by more than tol ||L||_inf (0 otherwise) -- lambda_out[0]
 * is the smallest value found either way.  The outputs are sorted by exact value, so among the members of a multiple lambda_2, which
 * differ in their last bits, the Fiedler solve's vector can stand at any of their ranks with reordered = 0: output column 0 is the
 * vector machip_fiedler returns only while reordered = 0 AND lambda_2 is simple at that resolution.  What this does NOT
 * prove: that nothing lies below lambda_out[0] (a start vector with a negligible component along an eigenvector misses it here as
 * in any Krylov method).
 * X0: n x q column-major start block, or NULL: the stored start vector (machip_set_start; warm_start as in machip_fiedler) for
 * column 0 and columns 1 .. q-1 of RandomState(7).normal(size=(q, n)).T, the reference's block (fiedler.py:27-32) continued.
 * max_steps: per column (0: the library's defaults).  Outputs, by rank: lambda_out (q), V_out (n x q column-major), residual_out
 * (q: the measured ||L v - lambda v||_1 / ||L||_inf), steps_out, restarts_out, status_out (q: MACHIP_OK or MACHIP_NOT_CONVERGED --
 * a column that reached its step cap says so and carries its measured residual; if column 0 itself missed the rule the others are
 * not attempted: NOT_CONVERGED, lambda NaN, residual +inf).  All but lambda_out may be NULL.  Returns MACHIP_OK when the columns
 * were run (their statuses tell), MACHIP_DISCONNECTED as machip_fiedler does, MACHIP_BAD_ARG for q out of range, a start vector
 * inside the span of the columns before it, an evaluation lane or a handle that belongs to a communicator (one GPU, one rank).
 * Option pairs_vcap: most basis columns a deflated sequence fills before it restarts from its Ritz vector (0: the basis budget).
 * Option pairs_precond (0, the default: the deflated Lanczos above, bit for bit; 1: opt in): on a chain-like graph in fp64 with
 * n <= 2^21, columns 1 .. q-1 run a block-size-1 LOBPCG in the complement of the columns found so far, preconditioned as the Fiedler
 * solve's modes 6 / 7 are (mac_amd/csrc/solver_pairs_lob.h; the preconditioner is column 0's when that solve ran
 * mode 6 / 7, else built once per call).  steps_out then counts iterations.  A column whose iteration ends without a passing check
 * (breakdown, the cap, patience) is finished by the deflated Lanczos from the last checked vector, its steps added; max_steps caps
 * the sum.  On any other handle the option changes nothing.  machip_lowest_pairs_info tells which route produced each column.
 * The handle's Fiedler state (vector, gradient, warm start) is afterwards what the column-0 solve alone would have left. */
int machip_lowest_pairs(machip_problem* p, int q, double tol, int max_steps, const double* X0, int warm_start,
                        double* lambda_out, double* V_out, double* residual_out, int32_t* steps_out, int32_t* restarts_out,
                        int32_t* status_out, int32_t* reordered_out, int32_t* first_rank_out);
/* The same for an arbitrary CSR Laplacian, on the handle machip_fiedler_csr keeps. */
int machip_lowest_pairs_csr(int device, int64_t n, const int32_t* indptr, const int32_t* indices, const double* data,
                            int q, double tol, int max_steps, const double* X0, int warm_start,
                            double* lambda_out, double* V_out, double* residual_out, int32_t* steps_out, int32_t* restarts_out,
                            int32_t* status_out, int32_t* reordered_out, int32_t* first_rank_out);
/* machip_lowest_pairs_csr with option pairs_precond for this call (-1: the process default) and machip_lowest_pairs_info's outputs. */
int machip_lowest_pairs_csr2(int device, int64_t n, const int32_t* indptr, const int32_t* indices, const double* data,
                             int q, double tol, int max_steps, const double* X0, int warm_start,
                             double* lambda_out, double* V_out, double* residual_out, int32_t* steps_out, int32_t* restarts_out,
                             int32_t* status_out, int32_t* reordered_out, int32_t* first_rank_out,
                             int pairs_precond, int32_t* method_out, int32_t* closures_out, double* build_ms_out);
/* How the columns of the handle's last machip_lowest_pairs call were produced, by rank.  method_out (q): the solver mode -- the
 * Fiedler solve's own (machip_solve_mode) for the column it produced; 1 deflated Lanczos; 6 / 7 LOBPCG preconditioned by the
 * tridiagonal chain / the exact chain + closures inverse; 9 such iterations, then finished by the deflated Lanczos.  *closures_out:
 * closures of the exact preconditioner the deflated columns ran with (0: none did).  *build_ms_out: device ms of the one-off
 * preconditioner build (0 when column 0's was reused or none was built).  Each may be NULL. */
int machip_lowest_pairs_info(machip_problem* p, int q, int32_t* method_out, int32_t* closures_out, double* build_ms_out);
/* Device time, in ms and by rank, of the columns of the handle's last machip_lowest_pairs call (hipEvents on its stream around each
 * column: its steps, the host's looks at the records between chunks, Ritz vectors and checks; column 0: the Fiedler solve's gpu_ms). */
int machip_lowest_pairs_time(machip_problem* p, int q, double* ms_out);
/* Supergradients of q given vectors (V: n x q column-major, host): G_out (m x q column-major), column c = g_k of machip_gradient
 * for V's column c -- the same kernel, bit-exact given the vector.  Leaves the handle's own gradient alone. */
int machip_gradient_block(machip_problem* p, int q, const double* V, double* G_out);

/* Store the cold-start vector (n doubles) used by every later machip_fiedler /
 * machip_fw_step call that passes x0 = NULL and warm_start = 0: the drop-in sends the
 * first column of the reference's RandomState(7) block (fiedler.py:27-32) once. */
int machip_set_start(machip_problem* p, const double* x0);

/* Supergradient g_k = (w_k (v_i - v_j)) (v_i - v_j) for all m candidates from the
 * device-resident Fiedler vector (mac.py:117-124).  g_out (m) may be NULL. */
int machip_gradient(machip_problem* p, double* g_out);

/* solve_subset_box_lp(g, k) (mac/optimization/constraints.py:12-22 ->
 * mac/utils/rounding.py:21-28): s = indicator of the k largest g.  Ties at the
 * k-th value go to the lowest indices (the reference's argpartition leaves them
 * unspecified).  s_out (m doubles) may be NULL. */
int machip_lp_topk(machip_problem* p, int64_t k, double* s_out);

/* One Frank-Wolfe iteration, device-resident (mac/optimization/frankwolfe.py:53-76
 * with problem = MAC.problem, solve_lp = solve_subset_box_lp):
 *   assemble L(x); (f, v) = Fiedler pair; g = supergradient; s = top-k(g);
 *   dual = f + g.(s - x); gnorm = ||g||_2; x_next = x + 2/(iter+2) (s - x).
 * x_next is staged; machip_fw_commit() makes it current (the caller applies the
 * reference's stop tests first: on a stop the reference returns the pre-update
 * x, frankwolfe.py:65-74).  Only scalars cross PCIe. */
int machip_fw_step(machip_problem* p, int64_t k, int iter, double tol, int max_steps, int warm_start,
                   double* f, double* dual, double* gnorm, machip_solve_stats* stats);
int machip_fw_commit(machip_problem* p);
/* The loop itself (mac/optimization/frankwolfe.py:53-76 as mac/solvers/mac.py:196-200 calls it) without returning to the caller
 * between iterations: for i = first_iter .. first_iter + max_iters - 1: machip_fw_step; upper = min(upper, dual); stop when
 * ||g|| < grad_tol (the current x stays) or (upper - f) < gap_tol |f|; else machip_fw_commit.  *upper_inout carries the dual
 * bound in and out (start: +inf).  Optional per-iteration outputs (max_iters entries each, NULL to skip): f_traj, dual_traj,
 * gnorm_traj, stats, modes (2 ints per iteration: machip_solve_mode and its closure count).  *iters_done = iterations run.
 * Between two iterations a Python caller of machip_fw_step / machip_fw_commit leaves the GPU idle for ~50 us (measured,
 * profiles/r5_c4_gaps.txt); this entry point is what MAC.solve and bench.py drive. */
int machip_fw_run(machip_problem* p, int64_t k, int first_iter, int max_iters, double gap_tol, double grad_tol, double tol,
                  int max_steps, int warm_start, double* upper_inout, double* f_traj, double* dual_traj, double* gnorm_traj,
                  machip_solve_stats* stats, int* modes, int* iters_done);

/* round_nearest(w, k, weights, break_ties_decimal_tol) on the device-resident x
 * (mac/utils/rounding.py:7-42, called at mac/solvers/mac.py:209): indicator of the k largest
 * entries under the lexicographic key (round(x, decimals), candidate weight); decimals < 0 =
 * plain top-k of x (rounding.py:21-28).  Full ties (equal rounded x and equal weight) go to the
 * highest indices (the reference's argpartition leaves them unspecified).  rounded_out: m doubles. */
int machip_round_nearest(machip_problem* p, int64_t k, int decimals, double* rounded_out);

/* find_fiedler_pair(L) for an arbitrary scipy CSR Laplacian
 * (mac/utils/fiedler.py:9, called that way by tests/utils/test_fiedler.py:32). */
int machip_fiedler_csr(int device, int64_t n, const int32_t* indptr, const int32_t* indices,
                       const double* data, double tol, int max_steps, const double* x0,
                       double* lambda2, double* v_out, double* X_out, int q,
                       machip_solve_stats* stats);

/* y = L(x) v on the device CSR (host vectors, n doubles): parity probe for the
 * SpMV kernel. variant: 0 = auto, 1 = LDS row-tile ("stream"), 2 = sub-wave vector. */
int machip_spmv(machip_problem* p, const double* v, double* y, int variant);

/* Landscape of L(x) behind the cold start of a Lanczos solve (late round 5): u after `sweeps` Jacobi sweeps
 * u <- u + D^-1 (1 - L u) from u = D^-1 (n doubles to the host).  A cold start multiplies the start vector
 * (machip_set_start: the reference's RandomState(7) column, mac/utils/fiedler.py:27-32) entry by entry by
 * (u / max u)^p -- options start_land (sweeps, default 3, 0 = off) and start_pow (p, default 128): the Fiedler
 * vector of a sparse random graph is localised on the peaks of u, and the reference's start block is only a
 * first guess (nx:151-256 iterates it to the same stop rule).  A caller's own start vector (x0 of
 * machip_fiedler / machip_fiedler_csr: the X argument of find_fiedler_pair) and a warm start are never
 * touched.  Parity probe for the k_land_* kernels and a diagnostic. */
int machip_landscape(machip_problem* p, int sweeps, double* u_out);

/* Average duration (microseconds, hipEvents on the handle's stream) of `reps`
 * back-to-back launches of the fused Lanczos SpMV kernel on the assembled L(x),
 * and its algorithmic bytes per launch (SURVEY section 8(d) B_spmv + the fused vector
 * traffic).  Used by bench.py for the roofline object. */
int machip_profile_spmv(machip_problem* p, int reps, double* avg_us, double* bytes_per_launch);

/* Multi-GPU: candidates are sharded in contiguous ranges over
 * nranks processes (one GPU each); each rank evaluates the supergradient of its
 * range and one RCCL all-gather over xGMI rebuilds the full m-vector on every
 * rank.  unique_id: the 128-byte ncclUniqueId from machip_comm_unique_id() on
 * rank 0, distributed by the caller. */
int machip_comm_unique_id(void* id128);
int machip_comm_init(machip_problem* p, int rank, int nranks, const void* id128);
/* The same split inside ONE process (the ncclCommInitAll style of SURVEY section 8(e)): `nranks` handles of the
 * same problem -- one per GPU, or several on one GPU -- become ranks 0..nranks-1 of an in-process communicator;
 * each handle is then driven by its own host thread and machip_fw_step / machip_gradient on every handle is
 * collective (all handles must call it).  The all-gather is peer-to-peer device copies between the handles'
 * gradient buffers bracketed by a host barrier; shard arithmetic and call site are those of the RCCL path.
 * Destroying one handle releases peers blocked in the collective with MACHIP_RCCL_ERROR. */
int machip_comm_init_local(machip_problem** handles, int nranks);
/* Communicator between PROCESSES (one per GPU: what `bench.py --gpus N` / torch.distributed.run launch) whose EIGEN-SOLVE is
 * row-partitioned (SURVEY section 8(e) "Expected scaling ... unless the eigen-solve is also parallelised"; the reference is a
 * single process, there is no reference line to match).  Every rank exports IPC handles of its Lanczos record buffers,
 * partial sums, Ritz staging vector, gradient and flag words (machip_ipc_export -> a blob of machip_ipc_blob_bytes() bytes), the
 * caller distributes the blobs (mac_amd.dist.FileGroup), every rank maps the peers' buffers (machip_comm_init_ipc: blobs =
 * nranks blobs in rank order; hipIpcOpenMemHandle, peer access across devices).  A rank then launches its share of every
 * fused Lanczos step's workgroups and writes records / partial sums into every rank's copy; steps are ordered ON THE
 * DEVICE by flag words (no host, no cross-stream edge; bounded waits: a stalled or dead peer makes the call return
 * MACHIP_RCCL_ERROR after timeout_s, default 10); every rank runs the same deterministic host logic, so results are bit-identical
 * to a single rank's.  Composes with machip_comm_init: with an RCCL communicator the gradient shards travel by ncclAllGather,
 * without one (ranks sharing a GPU) by peer writes through the mapped buffers.  machip_comm_close_ipc before machip_destroy
 * marks an orderly exit (a handle destroyed without it raises abort on its peers). */
/* First-contact helpers (round 4).  machip_comm_init and the communicator's FIRST ncclAllGather run under a watchdog
 * (MACHIP_RCCL_TIMEOUT_S, default 600 s): a peer that never arrives / a fabric that cannot carry the collective returns
 * MACHIP_RCCL_ERROR naming the rank instead of hanging the job.  machip_selftest_watchdog exercises that watchdog with a
 * sleeping stand-in (no GPU needed: MACHIP_OK when work_ms < limit_ms, MACHIP_RCCL_ERROR otherwise); machip_peer_access =
 * hipDeviceCanAccessPeer (1 / 0, -1 on error), what `bench.py --gpus N --dry` prints as a matrix. */
int machip_selftest_watchdog(int work_ms, int limit_ms);
int machip_peer_access(int device_a, int device_b);
int machip_ipc_blob_bytes(void);
int machip_ipc_export(machip_problem* p, void* blob, int blob_bytes);
int machip_comm_init_ipc(machip_problem* p, int rank, int nranks, const void* blobs, double timeout_s);
int machip_comm_close_ipc(machip_problem* p);
/* Leave the inter-process communicator again (mappings closed, flag words freed, rank 0 of 1): the way back to a replicated
 * solve when the attach succeeded here but failed on a peer (mac_amd.dist.attach_ipc).  Collective in spirit: call it on
 * every rank, behind a barrier, before anybody launches another step. */
int machip_comm_drop_ipc(machip_problem* p);
/* Leave whatever inter-process communicator the handle belongs to (RCCL: ncclCommAbort; IPC: as above): the handle is a
 * single-rank handle again.  For a first contact that failed on SOME rank: every rank drops, behind an agreement exchange. */
int machip_comm_drop(machip_problem* p);
/* Device time of the last sharded gradient of this handle (hipEvents on its stream): the gradient kernel over this rank's
 * candidate range, and the exchange behind it (ncclAllGather, or the IPC publish / wait pair) -- SURVEY section 8(e)'s two
 * terms, measured per Frank-Wolfe iteration by bench.py --gpus N. */
int machip_comm_timing(machip_problem* p, double* grad_us, double* exchange_us);
/* Which launch group the steps of the last eigen-solve were: 1 fused gather step (k_pipe_vec), 2 column-panel step
 * (k_pan_mul + k_pan_fin), 3 padded fixed-width step, 4 single-workgroup kernel (k_lan_persist), 5 classic two-kernel step,
 * 6 LOBPCG preconditioned by the chain, 7 exact chain + closures mode (*closures = size of its capacitance matrix),
 * 8 fp32 sequence + fp64 refinement.  bench.py prices the roofline of THAT group. */
int machip_solve_mode(machip_problem* p, int64_t* closures);
/* With 2..8 handles the in-process communicator also ROW-PARTITIONS THE EIGEN-SOLVE (MACHIP_SHARD_EIG=0 turns that off):
 * inside machip_fw_step rank 0's solver drives every rank's stream; per Lanczos step each rank launches its share of
 * the step's workgroups on its own copy of L(x) and of the gather operand and writes the records / partial sums it
 * produces into every rank's copy (peer-mapped device pointers across xGMI; plain device memory when ranks share a
 * GPU), steps ordered by HIP events; the Krylov basis is sharded by rows.  Workgroup w of the partitioned step does
 * exactly what workgroup w of a single rank's launch does, so lambda_2, the Fiedler vector and everything after them
 * are bit-identical to a single-rank run.
 * machip_comm_mode: 0 = no communicator, 1 = RCCL (candidate shard, eigen-solve replicated), 2 = in-process with a
 * replicated eigen-solve, 3 = in-process with the row-partitioned eigen-solve, 4 = inter-process (machip_comm_init_ipc) with
 * the row-partitioned eigen-solve enabled, 5 = ... and the LAST eigen-solve really ran row-partitioned (the fused Lanczos step;
 * other solver modes run replicated on every rank), 6 = inter-process, gradient exchange only (MACHIP_SHARD_EIG=0). */
int machip_comm_mode(machip_problem* p);
/* The candidate range [lo, hi) of `rank` and the padded shard length (host arithmetic only, no GPU needed):
 * shard = ceil(m / nranks), lo = min(m, rank shard), hi = min(m, lo + shard). */
int machip_shard_plan(int64_t m, int nranks, int rank, int64_t* lo, int64_t* hi, int64_t* shard);

/* MAC.evaluate_objective for B selection vectors at once (mac/solvers/mac.py:91-102 as called in a loop by
 * round_madow(value_fn=evaluate_objective, max_iters > 1), mac/utils/rounding.py:63-75, and by the budget sweep of
 * examples/g2o_experiment.py:347-376).  X: B x m row-major on the host; lambda2: B doubles; status (may be NULL): B
 * machip_status values (OK / NOT_CONVERGED / DISCONNECTED per entry).  The handle keeps up to MACHIP_LANES (default 16 for
 * single-workgroup solves, 4 otherwise) evaluation lanes -- own x, CSR buffers, eigen-solver state and stream, sharing the pattern and the candidate
 * arrays -- driven by one host thread each, so the small latency-bound solves of a pose graph overlap on the GPU.
 * Cold starts from the handle's start vector (machip_set_start), solver mode / precision of the handle; the
 * handle's own x, gradient and Fiedler vector are not touched.  Returns the first hard error, else MACHIP_OK. */
int machip_eval_batch(machip_problem* p, int B, const double* X, double tol, int max_steps, double* lambda2,
                      int* status);

/* Frank-Wolfe on B problems of the same graph AT ONCE -- the reference's real workload is a sweep of budgets over one
 * pose graph (examples/g2o_experiment.py:306-336: 10 budgets x MAC.solve(max_iters = 20)), each a chain of small,
 * latency-bound launches that leaves most of the chip idle.  Problem b runs the loop of
 * mac/optimization/frankwolfe.py:53-76 as mac/solvers/mac.py:196-200 calls it -- problem = MAC.problem, solve_lp =
 * top-ks[b], gamma_i = 2/(i+2), dual bound from the pre-update x, stop when ||g|| < grad_tol or
 * (upper - f) < gap_tol |f|, at most max_iters iterations -- from X0[b] (B x m row-major, host), on one of the handle's
 * evaluation lanes (own x / gradient / CSR / eigen-solver state / stream, sharing pattern and candidate arrays; up to
 * MACHIP_LANES run concurrently, one host thread each, each stream on a hardware queue of its own).  Every problem starts
 * from a clean solver state and the handle's start vector: its results are bit-identical to a fresh handle running
 * machip_fw_step / machip_fw_commit in a loop IN THE SAME SOLVER MODE (machip_set_solver(1), the Lanczos path, on both: under
 * the automatic mode a standalone handle may take the exact chain + closures mode -- small pose graphs up to 700 closures, larger
 * ones on a long forecast -- which a lane keeps to 256 closures so as not to starve the other lanes; the two then agree to the
 * solver tolerance, not bit for bit), whatever lane takes it -- as long as no single Krylov sequence outgrows the
 * lane's basis (a lane holds MACHIP_LANE_VBUDGET_MB = 1/8 of the handle's basis budget: 6 710 columns against 10 010 at
 * n = 1e4, 671 against 5 368 at n = 1e5); a longer sequence restarts earlier on a lane than on the handle and then agrees
 * with it to the solver tolerance, not bit for bit.
 * Outputs (host): X_out B x m final relaxed x (what MAC.solve returns as `unrounded`); R_out (may be NULL) B x m
 * round_nearest(x, ks[b], weights, round_decimals) as machip_round_nearest computes it; upper[B] dual upper bounds;
 * f_traj (may be NULL) B x max_iters lambda_2 per iteration; iters[B] iterations done; status[B] per problem
 * (OK / NOT_CONVERGED / DISCONNECTED).  Returns the first hard error, else MACHIP_OK. */
int machip_fw_sweep(machip_problem* p, int B, const int64_t* ks, const double* X0, int max_iters, double gap_tol,
                    double grad_tol, double tol, int max_steps, int warm_start, int round_decimals, double* X_out,
                    double* R_out, double* upper, double* f_traj, int* iters, int* status);

/* Eigen-solver selection -- the reference's `fiedler_method` string (mac/solvers/mac.py:23,68;
 * mac/utils/fiedler.py:38-42 dispatches 'tracemin_pcg' | 'tracemin_lu' | 'tracemin_cholesky', all
 * computing the same pair).  mode 0 = automatic (default), 1 = Lanczos on L restricted to 1-perp,
 * 2 = preconditioned (LOBPCG with a tridiagonal odometry-chain solve; the drop-in maps
 * 'tracemin_pcg' here).  Mode 2 falls back to mode 1 when it does not apply (n <= 256) or
 * stagnates; results obey the same stop rule either way. */
int machip_set_solver(machip_problem* p, int mode);

/* Arithmetic of the Krylov iterate (BASELINE.json configs[4], SURVEY section 8(b) `precision`):
 * 0 = fp64 throughout (default, what the reference computes in, mac/utils/fiedler.py:27-44);
 * 1 = fp32 Lanczos iterate (fp32 matrix values, 8-byte {t, v} float2 gather records, fp64
 *     accumulation of every inner product) followed by fp64 refinement: the Ritz vector is
 *     re-orthogonalised, its Rayleigh quotient and the reference's residual test are evaluated in
 *     fp64 on the fp64 L(x), and fp64 steps continue from it until the test passes.  The returned
 *     pair therefore obeys the same stop rule and the same 1e-8 parity bound as mode 0. */
int machip_set_precision(machip_problem* p, int precision);

/* Per-handle option table (round 5; replaces the MACHIP_* environment knobs of rounds 1-4).  The reference's only selector is
 * one string, `fiedler_method` (mac/utils/fiedler.py:38-42 -> machip_set_solver above); everything else this library can
 * vary -- launch shapes, thresholds of the automatic mode, test hooks that force a code path onto a small graph -- is an entry
 * of the handle's table, named as listed by machip_option_name(i) (mac_amd/csrc/options.h): e.g. "panel" (-1 automatic, 0 off,
 * 1 forced), "chunk", "lanes", "woodbury".  value = MACHIP_OPTION_AUTO restores the measured default.
 * p == NULL edits the PROCESS defaults: what handles created afterwards (and the handle machip_fiedler_csr keeps) start
 * from.  Those defaults are initialised from the environment once, when the library is first used (MACHIP_<NAME>, developer
 * use: sweeps under tools/); nothing reads the environment after that.  Options consumed when a handle is created
 * ("asm_g", "vbudget_mb", "vcap", ...) must be set as process defaults before machip_create.  An evaluation lane runs on its
 * owner's table.  Unknown name -> MACHIP_BAD_ARG.  Not thread-safe against a running call on the same handle. */
#define MACHIP_OPTION_AUTO INT64_MIN
int machip_set_option(machip_problem* p, const char* name, int64_t value);
int machip_get_option(machip_problem* p, const char* name, int64_t* value);   /* MACHIP_OPTION_AUTO when not set */
const char* machip_option_name(int i);    /* i = 0, 1, ...; NULL past the last one */

int machip_synchronize(machip_problem* p);

/* Measurement helpers (no counterpart in the reference; bench.py and the CPU tests use them).
 * machip_membench: achieved HBM bandwidth on `device` in GB/s -- a read-only pass and the STREAM triad
 * a = b + s c (two reads + one write per element) over arrays of `bytes` bytes each, `reps` back-to-back
 * launches timed with HIP events.  SURVEY section 8(d): the roofline object of bench.py reports this measured
 * peak next to the nominal 8 TB/s.
 * machip_host_tridiag_smallest: host only, no GPU -- smallest eigenpair (theta, s[J]) of the J x J symmetric
 * tridiagonal with diagonal a[0..J) and off-diagonal b[1..J) (b[0] unused): the O(J) analysis the Lanczos driver
 * runs on every chunk of steps; exported so that `-m "not gpu"` tests can check it against LAPACK. */
int machip_membench(int device, int64_t bytes, int reps, double* read_gbs, double* triad_gbs);
/* Host only, no GPU: the shape the column-panel Lanczos step (mac_amd/csrc/panel.h) would use for a matrix of n rows, nnz
 * entries and longest row maxlen -- out12 = {on, NP panels, C columns per panel, NB row blocks, NTB 64-row tiles per block,
 * TWW tiles per worker wave, RPT records per worker thread (record form), workgroups of the row kernel, u (1: the shifted
 * recurrence with an 8-byte operand, mac_amd/csrc/panel_u.h), LPT 16-byte operand loads per worker thread, TWT tiles per worker
 * wave its kernel instantiation holds, row blocks per workgroup} -- under the process-default options ("panel", "panel_u" etc.).
 * For CPU tests of the shape arithmetic (coverage of all rows / columns, LDS and register limits). */
int machip_panel_plan(int64_t n, int64_t nnz, int maxlen, int* out12);
/* machip_fiedler_csr keeps one CSR-only handle (stream, device buffers, chunk graphs) between calls and reuses it when
 * device and n match and the matrix fits -- every solve still starts from a clean solver state.  This frees it (the
 * Python layer calls it at interpreter exit). */
void machip_release_cache(void);
int machip_host_tridiag_smallest(const double* a, const double* b, int J, double* theta, double* s);
/* Host only, no GPU: the rule a Lanczos solve ends by (mac_amd/csrc/follow.h; round 5, streamed records) applied to a finished
 * record array.  tri3 = interleaved (alpha_j, beta_j, ||v_j||_1) triples valid through beta_J; e_target = the residual estimate
 * (||r||_1, not yet divided by ||L||_inf) a check needs; tiny_l = ||L||_inf; jcap = basis capacity (0: none).  Out: the analysis
 * points visited (a function of the records alone), the order of the tridiagonal the sequence ends on (-1: not within J) and
 * the estimate there.  The reference's counterpart is the per-iteration test of nx:246. */
int machip_host_follow_records(const double* tri3, int J, int n, double e_target, double tiny_l, int jcap, int* points, int cap,
                               int* npoints, int* jeff, double* est);

/* GreedyESP (mac/solvers/greedy_esp.py of the reference: the greedy k-edge selection by weighted effective resistance,
 * Khosoussi et al.; mac_amd/csrc/esp.h).  Node 0 pinned, L_red = the fixed graph's reduced Laplacian, Sigma = (L_red + beta I)^-1
 * kept dense on the device.  Every step selects the unselected candidate of largest w_e r_e (r_e = a_e^T Sigma a_e; ties: lowest
 * index, exact fp64 equality) and adds it by a rank-1 update.  beta: 0 when the fixed graph is connected; otherwise
 * MACHIP_DISCONNECTED when a node other than 0 has no fixed edge, else 1e-4.  Limits: n <= 32768 when the fixed edges are
 * exactly the chain (i, i+1) (closed-form Sigma), n <= 16384 otherwise (dense Gauss-Jordan inverse); beyond them MACHIP_BAD_ARG. */
typedef struct machip_esp machip_esp;
#define MACHIP_ESP_DENSE_INVERSE 1   /* flags: build Sigma by the dense inverse even for a chain (cross-checks) */
/* flags: no Sigma at all (mac_amd/csrc/esp_free.h).  Only when the fixed edges are exactly the connected chain (i, i+1), parallel
 * links summed (MACHIP_BAD_ARG otherwise, and together with MACHIP_ESP_DENSE_INVERSE): Sigma0's entries come from the chain's
 * prefix resistances and every pick's rank-1 update stays in a history of ld x K doubles (ld = n - 1 rounded up to 64) that
 * machip_esp_select allocates, or grows, for its largest budget; nothing of size ld x ld is ever allocated.  Nothing is ever folded:
 * `fold` must be 0 with this flag (MACHIP_BAD_ARG otherwise -- an argument without a meaning is refused, not ignored).
 * No limit on n but memory and int32 node ids; a K whose history does not fit in free device memory is MACHIP_BAD_ARG, decided
 * before anything is allocated.  Pick j streams 8 ld j bytes (about 4 ld K^2 over a run): the route is for K << n.  Same rule, tie
 * rule and per-entry arithmetic as the dense forms; the sums over the history run in a fixed order that depends on (ld, j, option
 * esp_free_split) alone, so runs repeat bit for bit and agree with the dense chain form to rounding.  machip_esp_relax_* (unless
 * the handle was made with MACHIP_ESP_EDGE_RELAX as well) and machip_eig_create (unless MACHIP_EIG_MATRIX_FREE is given as well)
 * answer MACHIP_BAD_ARG on this route. */
#define MACHIP_ESP_MATRIX_FREE 2
/* flags, valid only together with MACHIP_ESP_MATRIX_FREE (MACHIP_BAD_ARG alone, with MACHIP_ESP_DENSE_INVERSE or with fold != 0):
 * the matrix-free route for ANY connected fixed graph (mac_amd/csrc/esp_tree.h).  Sigma0 is that of the spanning tree T that
 * machip_esp_tree_plan builds -- Sigma0(T)_ab = R[lca(a, b)], R the resistance from node 0 along T -- and each of the r fixed links
 * not in T ("seeds") is a rank-1 update kept as one of the first r columns of the history, before the first pick; the seeds make
 * no entry in order_out / gain_out.  The history holds r + K columns (8 ld (r + K) bytes): the route is for r << n, K << n.  A fixed
 * graph that is not connected is MACHIP_BAD_ARG (the route has no beta), as are fixed links whose summed weight is not positive;
 * all argument errors are decided on the host before a device is touched.  Exact for any connected fixed graph; on a chain it
 * feeds the history's sums the doubles MACHIP_ESP_MATRIX_FREE alone feeds them and returns the same bits.  machip_esp_relax_* (unless
 * the handle was made with MACHIP_ESP_EDGE_RELAX_TREE as well) and machip_eig_create answer MACHIP_BAD_ARG on this route. */
#define MACHIP_ESP_SPANNING_TREE 8
/* flags, valid only together with MACHIP_ESP_MATRIX_FREE (MACHIP_BAD_ARG alone, with MACHIP_ESP_DENSE_INVERSE, with
 * MACHIP_ESP_SPANNING_TREE, or on a fixed graph that is not the connected chain): the handle is a MACHIP_ESP_MATRIX_FREE handle
 * -- machip_esp_select and machip_esp_weighted_resistances work exactly as without this flag -- on which machip_esp_relax_* run in
 * the space of the m candidates instead of the n - 1 nodes (mac_amd/csrc/esp_relax_edge.h; the text above machip_esp_relax_eval). */
#define MACHIP_ESP_EDGE_RELAX 16
/* flags, valid only as MACHIP_ESP_MATRIX_FREE | MACHIP_ESP_SPANNING_TREE | MACHIP_ESP_EDGE_RELAX_TREE (without both partners
 * MACHIP_BAD_ARG "unknown flags ..."; with MACHIP_ESP_EDGE_RELAX or MACHIP_ESP_DENSE_INVERSE MACHIP_BAD_ARG naming the pair; all
 * decided on the host before a device is touched): the handle is a spanning-tree handle -- machip_esp_select and
 * machip_esp_weighted_resistances work exactly as without this flag -- on which machip_esp_relax_* run in the space of the m
 * candidates and the r seeds (mac_amd/csrc/esp_relax_edge_tree.h; the text above machip_esp_relax_eval).  Bit 4 stays unknown. */
#define MACHIP_ESP_EDGE_RELAX_TREE 32
/* fold: pending rank-1 updates folded into Sigma every `fold` steps (1..256; 0 = 64).  Builds Sigma0. */
int machip_esp_create(int device, int64_t n, int64_t n_fixed, const int32_t* fi, const int32_t* fj, const double* fw,
                      int64_t m, const int32_t* ci, const int32_t* cj, const double* cw, int fold, int flags, machip_esp** out);
void machip_esp_destroy(machip_esp* h);
/* One greedy run from Sigma0 up to K = ks[nb-1] selections (ks positive, non-decreasing, K <= m): order_out[K] = candidate
 * indices in selection order, gain_out[K] = the score s* of each pick (sum log(1 + gain) = logdet growth), t_ms_out[nb] = device
 * time from the call's start until budget ks[i] was reached.  Any output may be NULL. */
int machip_esp_select(machip_esp* h, int nb, const int64_t* ks, int32_t* order_out, double* gain_out, double* t_ms_out);
/* w_e r_e of every candidate (m doubles) in the current graph: F plus the last machip_esp_select's selections.  (Matrix-free
 * route: every candidate is rescored from the chain and the history, m K gathered pairs.) */
int machip_esp_weighted_resistances(machip_esp* h, double* r_out);
/* info4 = {form (0 chain, 1 dense inverse, 2 chain without Sigma, 3 spanning tree without Sigma), leading dimension of Sigma, fold,
 * updates pending since the last fold (form 2: the columns of the history; form 3: the picks in it, seeds not counted)}; beta. */
int machip_esp_info(machip_esp* h, int32_t* info4, double* beta);
/* The host side of MACHIP_ESP_SPANNING_TREE, no device needed.  Parallel fixed edges are summed in list order ((a, b) and (b, a)
 * are one link), self-loops dropped.  T = the BFS tree from node 0, the neighbours of a node visited in order of first appearance
 * in the fixed list.  Outputs by node (n entries each): parent (-1 for node 0), R[v] = R[parent] + 1 / w (R[0] = 0; on a chain
 * the prefix sums, same order of additions), pre = preorder number (children in the order BFS attached them), end = the last
 * preorder number of v's subtree (a is an ancestor of b iff pre[a] <= pre[b] <= end[a]).  The links not in T, in order of first
 * appearance and oriented as first given, are the seeds: *n_seeds of them into su, sv, sw (room for n_fixed entries each).
 * MACHIP_BAD_ARG when the fixed graph is not connected or a link's summed weight is not positive. */
int machip_esp_tree_plan(int64_t n, int64_t n_fixed, const int32_t* fi, const int32_t* fj, const double* fw, int32_t* parent,
                         double* R, int32_t* pre, int32_t* end, int64_t* n_seeds, int32_t* su, int32_t* sv, double* sw);
/* *seeds_out = the seeds of a MACHIP_ESP_SPANNING_TREE handle (distinct fixed links - (n - 1)); 0 on every other handle. */
int machip_esp_seeds(machip_esp* h, int64_t* seeds_out);

/* GreedyKirchhoff: greedy A-optimal selection on the same handle (mac_amd/csrc/kirchhoff.h).  The criterion is tr L^+ of the whole
 * graph's Laplacian (the total effective resistance; Kirchhoff index / n) = tr Sigma - (1^T Sigma 1) / n; adding candidate e lowers it
 * by gain_e = w_e (|z_e|^2 - (1^T z_e)^2 / n) / (1 + s_e), z_e = Sigma a_e padded with 0 for node 0, s_e its weighted resistance.
 * All three work on the dense forms only (info4[0] = 0 or 1) and refuse, before any device work, with MACHIP_BAD_ARG a handle made
 * with MACHIP_ESP_MATRIX_FREE (alone or with MACHIP_ESP_SPANNING_TREE / MACHIP_ESP_EDGE_RELAX*: the criterion needs Sigma) and with
 * MACHIP_DISCONNECTED a handle whose beta != 0 (a disconnected fixed graph has an infinite index).
 * One greedy run from Sigma0 up to K = ks[nb-1] picks, arguments as machip_esp_select (every output required): each step takes
 * the unselected candidate of largest gain (ties: lowest index); gain_out[k] = the pick's gain, so that the sum of the gains is
 * tr L^+ before the run minus tr L^+ after it.  Per pick the run streams Sigma once (8 ld^2 bytes).  Results repeat bit for bit. */
int machip_esp_kirchhoff_select(machip_esp* h, int nb, const int64_t* ks, int32_t* order_out, double* gain_out, double* t_ms_out);
/* gain_e of every candidate (m doubles; selected ones included) re-scored exactly from Sigma of the current graph -- F plus the
 * last run's selections, whose pending updates are folded first; F alone on a fresh handle. */
int machip_esp_kirchhoff_gains(machip_esp* h, double* gains_out);
/* Scores a selection of any origin: restarts from Sigma0, applies the nsel candidates idx[] (distinct, in [0, m); nsel = 0: none)
 * as forced picks in the given order, folds, and returns out2 = {tr L^+ of the fixed graph, tr L^+ with the selection}, both by a
 * two-stage reduction over Sigma (not from summed gains).  Afterwards the handle's current graph is F plus the selection. */
int machip_esp_kirchhoff_eval(machip_esp* h, int64_t nsel, const int32_t* idx, double* out2);

/* The convex relaxation of GreedyESP's problem on the same handle (mac_amd/csrc/esp_relax.h).  For x in [0, 1]^m:
 *     M(x) = L_red + beta I + sum_e x_e w_e a_e a_e^T,   F(x) = log det M(x) - log det M(0)   (nats; F(0) = 0 exactly; for a 0/1 x
 *     the sum of log(1 + gain) over its edges in machip_esp_select's convention),   dF/dx_e = w_e a_e^T M(x)^-1 a_e.
 * F is concave: F(x) + dF(x).(s - x), s the top-k vertex of dF(x) (ties at the k-th value: lowest indices, as machip_lp_topk),
 * is an upper bound on F over {x in [0, 1]^m, sum x <= k}, so on every k-edge selection.  Every evaluation assembles the dense
 * M(x), inverts it by the blocked Gauss-Jordan elimination and takes log det from the same elimination's pivots; results are
 * bit-identical from run to run.  The chain closed form does not apply to M(x): n <= 16384 whatever the fixed edges are,
 * MACHIP_BAD_ARG beyond.  The first relaxation call on a handle allocates a third ld x ld buffer (Sigma0 stays untouched:
 * machip_esp_select afterwards returns what it returns on a fresh handle) and evaluates log det M(0).  A relaxation call
 * overwrites the working copy of the last selection run: machip_esp_weighted_resistances then refers to the fixed graph again.
 * x outside [0, 1] or not finite, k <= 0, k > m: MACHIP_BAD_ARG (machip_last_error says which).
 *
 * On a handle made with MACHIP_ESP_EDGE_RELAX the same three entry points work in edge space.  With R[v] the chain's resistance
 * from node 0 to v, candidate e oriented lo_e <= hi_e, G_ef = max(0, R[min(hi_e, hi_f)] - R[max(lo_e, lo_f)]) (the resistance of
 * the overlap of two chain intervals), D = diag(w_e x_e) and N(x) = I + G D (m x m, not symmetric, leading principal minors
 * positive on all of [0, 1]^m):
 *     F(x) = log det N(x)   (the matrix determinant lemma; F(0) = log 1 = 0 exactly),   dF/dx_e = w_e [N(x)^-1 G]_ee.
 * Every evaluation assembles N(x) (leading dimension m rounded up to 64, identity beyond m), inverts it by the same blocked
 * Gauss-Jordan elimination and takes F from its pivots; the LP vertex, the step, the stop rules, the tie rule, the argument
 * checks and the outputs are those above, and runs repeat bit for bit.  Limit: m <= 16384 (MACHIP_BAD_ARG at the first relaxation
 * call, before anything is allocated); none on n.  The first call allocates two ld x ld buffers; nothing of size n is allocated and
 * nothing the greedy keeps (its history, what machip_esp_weighted_resistances reports) is touched.
 *
 * On a handle made with MACHIP_ESP_EDGE_RELAX_TREE they work in edge space over the spanning tree T of machip_esp_tree_plan, for
 * any connected fixed graph.  M = m + r columns: [0, m) the candidates, [m, M) the r seeds in the plan's order.  With Rt the root
 * resistances along T,
 *     G_ef = (Rt[lca(u_e, u_f)] + Rt[lca(v_e, v_f)]) - (Rt[lca(u_e, v_f)] + Rt[lca(v_e, u_f)])      (this association; G_ef = G_fe
 *     to the bit, a self-loop's row and column exact zeros),   d_j = w_j x_j (j < m), w_seed (j >= m),   N(x) = I + G diag(d),
 *     F(x) = log det N(x) - log det N(0)   (N(0): the seeds alone, evaluated once per handle by the same kernels: F(0) = 0 exactly),
 *     dF/dx_e = w_e sum_{j < M} N(x)^-1[e, j] G[j, e]   (e < m).
 * G is built once, at the first relaxation call, and kept (ld x ld, ld = M rounded up to 64); every evaluation assembles N(x) from
 * it, inverts it by the same elimination and takes the gradient from rows of N^-1 and G.  The LP vertex, the step, the stop rules,
 * the tie rule, the argument checks and the outputs range over the m candidates and are those above; runs repeat bit for bit.
 * Limit: m + r <= 16384 (MACHIP_BAD_ARG naming m and r at the first relaxation call, before anything is allocated; the handle's
 * greedy keeps working); none on n.  The first call allocates three ld x ld buffers (24 ld^2 bytes); nothing of size n is allocated
 * beyond the tree's tables and nothing the greedy keeps is written -- the seeds need not have been run. */
/* F(x) and, when grad_out is not NULL, the gradient (m doubles). */
int machip_esp_relax_eval(machip_esp* h, const double* x, double* F_out, double* grad_out);
/* Frank-Wolfe from x_inout with the open-loop step 2 / (2 + t), t = 0, 1, ...: per iteration F, the dual value F + g.(s - x)
 * and |g|_2 (f_traj / dual_traj / gnorm_traj, max_iters entries each, any may be NULL); *upper_out = the smallest dual value
 * seen.  Stops after the iteration at which |g|_2 < grad_tol or (upper - F) < gap_tol |F| (the iterate is then the one the test
 * was evaluated at, not yet moved), or after max_iters.  x_inout returns the last iterate, *iters_out the iterations evaluated. */
int machip_esp_relax_run(machip_esp* h, int64_t k, int max_iters, double gap_tol, double grad_tol, double* x_inout,
                         double* f_traj, double* dual_traj, double* gnorm_traj, int* iters_out, double* upper_out);
/* *out = sum_e a_e b_e (m doubles each, host), summed on the device in exactly the order machip_esp_relax_run sums g.(s - x): a
 * Frank-Wolfe driver on the host that evaluates F and the gradient with machip_esp_relax_eval and forms the dual value as
 * F + inner(g, s - x) reproduces machip_esp_relax_run's dual values, and with them its upper bound, bit for bit (a host dot
 * product sums in another order and agrees to rounding only). */
int machip_esp_relax_inner(machip_esp* h, const double* a, const double* b, double* out);
/* info2 = {the space the relaxation of this handle works in (0: nodes, M(x); 1: candidates, N(x), MACHIP_ESP_EDGE_RELAX;
 * 2: candidates and seeds over the spanning tree, MACHIP_ESP_EDGE_RELAX_TREE), the leading dimension of the matrix it inverts
 * (0 before the first relaxation call on a node-space handle)}. */
int machip_esp_relax_info(machip_esp* h, int32_t* info2);
/* The stored Gram matrix of a MACHIP_ESP_EDGE_RELAX_TREE handle, M x M row-major into G_out (M = m + r, built if no relaxation
 * call has built it yet).  MACHIP_BAD_ARG on every other kind of handle and when M is not m + r. */
int machip_esp_relax_gram(machip_esp* h, double* G_out, int64_t M);

/* The Fedorov exchange on the log tree count (mac_amd/csrc/esp_exchange.h): best-swap local search from the k-edge selection
 * sel_in (k distinct candidate indices, any order).  With S the selection, Sigma = (L_red + sum_{e in S} w_e a_e a_e^T)^-1,
 * s_e = w_e a_e^T Sigma a_e and r_ef = a_e^T Sigma a_f, taking e in S out and putting f outside S in multiplies the tree count by
 *     Delta(e, f) = (1 - s_e)(1 + s_f) + w_e w_f r_ef^2.
 * A round evaluates all k (m - k) pairs and takes the largest Delta (ties, exact equality: lowest e, then lowest f); the call
 * stops with *converged = 1 when Delta - 1 <= min_gain, or with *converged = 0 after max_swaps swaps (max_swaps = 0 is legal:
 * the selection is loaded and returned).  The swap is applied as two rank-1 updates of Sigma, the removal with
 * c = -w_e / (1 - s_e), the insertion with c = w_f / (1 + s_f'), s_f' the score after the removal.  Outputs: sel_out[k] the final
 * selection ascending; out_idx[t], in_idx[t], ratio[t] = (1 - s_e)(1 + s_f') for swap t < *n_swaps (max_swaps entries each; they
 * may be NULL when max_swaps = 0; sum log ratio = the growth of the log tree count); t_ms (6 doubles, may be NULL): device time of
 * the call, and -- only with option esp_xch_profile = 1, else 0 -- of the load with T's build, the pair passes, T's updates, the
 * forced steps with their score updates, the folds.  Results are a function of the inputs alone: runs repeat bit for bit.
 * The call keeps k rows of Sigma (8 k ld bytes, allocated by the first call, freed by machip_esp_destroy) and reads one 24-byte
 * record per round.  Option esp_xch_lds_kb (KiB; default 48, at most 152; a launch the runtime refuses falls back to global rows): a pair pass holds its row in LDS when 8 ld bytes fit, else
 * reads it from global memory -- the same bits either way.
 * MACHIP_BAD_ARG (machip_last_error names the reason): NULL pointers; k < 1 or k >= m; an index outside [0, m); a repeated index;
 * max_swaps < 0; min_gain < 0 or not finite; a MACHIP_ESP_MATRIX_FREE handle (no Sigma to exchange on); a handle with beta != 0
 * (disconnected fixed graph: 1 - s_e can be of the order of beta); 8 k ld bytes beyond the device's free memory (or option
 * esp_xch_max_mb, MiB) or k ld >= 2^31.  MACHIP_NOT_CONVERGED: a removal's 1 - s_e was not positive.
 * Afterwards machip_esp_weighted_resistances refers to the fixed graph plus sel_out; machip_esp_select and machip_esp_relax_* return
 * what they return on a fresh handle. */
int machip_esp_exchange(machip_esp* h, int64_t k, const int32_t* sel_in, int64_t max_swaps, double min_gain, int32_t* sel_out,
                        int32_t* out_idx, int32_t* in_idx, double* ratio, int64_t* n_swaps, int32_t* converged, double* t_ms);
/* The same exchange carried out in the space of the candidates (mac_amd/csrc/esp_exchange_edge.h), on a handle made with
 * MACHIP_ESP_EDGE_RELAX or MACHIP_ESP_EDGE_RELAX_TREE: any num_nodes, m + r <= 16384 (r the seeds of a tree handle, 0 on a chain).
 * With G the Gram matrix of the m + r columns the relaxation of the handle works with and S' the selection plus the seeds,
 * R = A^T Sigma(S') A is (m + r) x (m + r) and s_f = w_f R[f][f], r_ef = R[e][f]; a pick or a removal of column e is
 * R -= c R[:, e] R[e, :] with the coefficients above.  Arguments, outputs, stop rule, tie rule, the meaning of max_swaps = 0 and the
 * layout of t_ms are machip_esp_exchange's; results are a function of the inputs alone.  R lives in the relaxation's own N buffer
 * (the relaxation's state is made if this is the first call on the handle; a tree handle's G is built if it was not); the call keeps
 * k rows of R (8 k ld bytes, ld = m + r rounded up to 64) and a view of m + r columns, made by the first call, freed by
 * machip_esp_destroy.  The greedy's history, scores, flags and pending count are never written.
 * After an insertion the entering column's own score is written in closed form, 1 - 1 / (1 + s), instead of s - w c z_e^2 (G's
 * entries grow with the length of a chain, the scores of the selected stay below 1); exact duplicates of the column get its bits.
 * MACHIP_BAD_ARG (machip_last_error names the reason): what machip_esp_exchange refuses except the matrix-free clause; a handle made
 * without MACHIP_ESP_EDGE_RELAX / MACHIP_ESP_EDGE_RELAX_TREE; m + r > 16384; 8 k ld bytes beyond the device's free memory (or option
 * esp_xch_max_mb).  MACHIP_NOT_CONVERGED: a removal's 1 - s_e was not positive, or a round had no finite Delta.
 * Afterwards machip_esp_relax_*, machip_esp_select and machip_esp_weighted_resistances return what they return on a fresh handle. */
int machip_esp_exchange_edge(machip_esp* h, int64_t k, const int32_t* sel_in, int64_t max_swaps, double min_gain, int32_t* sel_out,
                             int32_t* out_idx, int32_t* in_idx, double* ratio, int64_t* n_swaps, int32_t* converged, double* t_ms);

/* GreedyEig (mac/solvers/greedy_eig.py of the reference: the greedy k-edge selection by algebraic connectivity; mac_amd/csrc/eig.h).
 * Every pick evaluates lambda_2(L_cur + w_e a_e a_e^T) for the unselected candidates whose supergradient bound
 * u_e = lambda_2 + w_e (v_i - v_j)^2 is not below a value already established, in batches that share the dense inverse of the
 * reduced Laplacian (the state of machip_esp), and takes the best by the reference's scan (candidate-index order, a candidate
 * replaces the running best only if it exceeds it by more than 1e-8).  Every reported lambda_2 satisfies the stop rule
 * ||L_e v - lambda v||_1 / ||L_e||_inf < 1e-8 (||v||_2 = 1), evaluated with the sparse Laplacian.  The fixed graph must be connected
 * (MACHIP_DISCONNECTED otherwise); size limits and flags as machip_esp_create, except that MACHIP_ESP_MATRIX_FREE is taken only together
 * with MACHIP_EIG_MATRIX_FREE and MACHIP_ESP_SPANNING_TREE not at all (MACHIP_BAD_ARG; the spanning-tree route of GreedyEig has a flag of
 * its own, MACHIP_EIG_MATRIX_FREE_TREE, and no size limit but memory). */
typedef struct machip_eig machip_eig;
/* flags of machip_eig_create only (machip_esp_create answers "unknown flags"), valid only as MACHIP_ESP_MATRIX_FREE |
 * MACHIP_EIG_MATRIX_FREE: GreedyEig without a dense Sigma (mac_amd/csrc/eig_free.h).  The fixed edges must be exactly the connected
 * chain (i, i+1), parallel links summed.  The preconditioner is applied as Sigma0 Q by two scans over the chain's prefix resistances
 * minus the rank-j correction of the picks, which stay in the history of the MACHIP_ESP_MATRIX_FREE handle underneath (8 ld K bytes,
 * sized by machip_eig_select for its budget; a K that does not fit in free device memory is MACHIP_BAD_ARG before anything is
 * allocated, as are batch arrays -- about 8 (6 ldv + 3 ld) ldq bytes -- that do not fit, at create).  Nothing of size ld x ld exists:
 * no limit on n but memory and int32 node ids.  One application costs 4 ld j B flop plus three passes over the batch instead of
 * 2 ld^2 B.  Every lambda_2, stop rule and pick is decided by the sparse L_cur as on the dense route; the order of every sum depends on
 * (ld, j, the batch, options eig_free_rows / eig_free_split) alone, so runs repeat bit for bit.  MACHIP_BAD_ARG, decided on the host
 * before a device is touched: the flag alone, with MACHIP_ESP_DENSE_INVERSE, with fold != 0 (nothing is folded: an argument without
 * a meaning is refused, not ignored), or a fixed graph that is not the chain.  machip_eig_exchange answers MACHIP_BAD_ARG on such a
 * handle (machip_eig_exchange_free is its form here).  The stop rule is relative to ||L_e||_inf: on a long chain (lambda_2 / ||L||_inf ~ pi^2 / 4 n^2 < 1e-8 from n ~ 16 000 on) it
 * certifies little more than the sign of lambda_2 -- on this route as on the dense one. */
#define MACHIP_EIG_MATRIX_FREE 64
/* flag of machip_eig_create only (machip_esp_create answers "unknown flags"), valid only as MACHIP_ESP_MATRIX_FREE |
 * MACHIP_EIG_MATRIX_FREE | MACHIP_EIG_MATRIX_FREE_TREE with fold = 0: the route above for ANY connected fixed graph
 * (mac_amd/csrc/eig_free_tree.h).  machip_eig_create takes the spanning tree T and the r seeds of MACHIP_ESP_SPANNING_TREE itself (a
 * caller's MACHIP_ESP_SPANNING_TREE stays refused): Sigma0(T)_ab = Rt[lca(a, b)] is applied to a batch by four sweeps over T in preorder
 * (suffix sums, then a prefix along the Euler tour) -- a fixed number of launches whatever the depth of T --, the r fixed links outside
 * T are the history's columns [0, r) before the first pick, and the picks follow: the history takes 8 ld (r + K) bytes, the batch
 * arrays about 8 (6 ldv + 4 ld) ldq.  Both refusals of the chain route apply, with r named in the message; the spanning-tree plan's own
 * arrive with their messages (a fixed graph that is not connected, links whose summed weight is not positive), all before a device is
 * touched.  Nothing of size ld x ld exists.  The difference of suffix sums in the sweeps loses about n eps: it costs the
 * preconditioner nothing that decides (every lambda_2 and pick is the sparse L_cur's).  The order of every sum depends on (ld, the
 * tree, j, the batch, options eig_free_rows / eig_free_split) alone.  machip_eig_exchange answers MACHIP_BAD_ARG (machip_eig_exchange_free runs).  The stop rule's caveat
 * above holds for chain-like trees. */
#define MACHIP_EIG_MATRIX_FREE_TREE 128
/* fold: as machip_esp_create (0 = 16; must be 0 with MACHIP_EIG_MATRIX_FREE); batch: columns solved together (1..4096; 0 = 512).
 * Builds Sigma0 (unless matrix-free) and the fixed graph's Fiedler pair. */
int machip_eig_create(int device, int64_t n, int64_t n_fixed, const int32_t* fi, const int32_t* fj, const double* fw,
                      int64_t m, const int32_t* ci, const int32_t* cj, const double* cw, int fold, int batch, int flags, machip_eig** out);
void machip_eig_destroy(machip_eig* h);
/* One greedy run from the fixed graph, k picks (1 <= k <= m): order_out[k] = candidate indices in pick order, lambda2_out[k] =
 * lambda_2 after each pick, t_ms_out[k] = wall time from the start of the run until each pick was made.  Any output may be NULL. */
int machip_eig_select(machip_eig* h, int64_t k, int32_t* order_out, double* lambda2_out, double* t_ms_out);
/* lambda_2(L_cur + e) of every candidate (m doubles; NaN for the selected), L_cur = the fixed graph plus the last run's picks. */
int machip_eig_candidate_lambda2(machip_eig* h, double* out);
/* the bounds u_e (m doubles; NaN for the selected) from the current Fiedler pair. */
int machip_eig_candidate_bounds(machip_eig* h, double* out);
/* info6 = {form (0 chain, 1 dense inverse, 2 chain without Sigma: MACHIP_EIG_MATRIX_FREE, 3 spanning tree without Sigma:
 * MACHIP_EIG_MATRIX_FREE_TREE), leading dimension of Sigma, fold (forms 2, 3: 0), batch, pending updates (form 2: the history's
 * columns; form 3: r seeds + picks), picks of the last run};
 * beta_lambda2 = {beta (always 0), current lambda_2}; per pick of the last run (at most cap entries): candidates solved exactly and
 * operator applications (summed over the columns). */
int machip_eig_info(machip_eig* h, int32_t* info6, double* beta_lambda2, int64_t cap, int32_t* solved_out, int32_t* applies_out);
/* *seeds_out = the seeds r of a MACHIP_EIG_MATRIX_FREE_TREE handle (distinct fixed links - (n - 1)); 0 on every other handle. */
int machip_eig_seeds(machip_eig* h, int64_t* seeds_out);
/* Best-swap local search on lambda_2 (mac_amd/csrc/eig_exchange.h) from the k-edge selection sel_in (k distinct candidate
 * indices, any order).  With S the selection and L_S the fixed graph plus S, a round
 *   1. solves the K removal pairs (lambda_2(S \ e), v^-e), e in S, as columns of the batch solver (a removal is the candidate with
 *      weight -w_e; the downdate coefficient is -w_e / (1 - w_e s_e));
 *   2. bounds every pair: u(e, f) = lambda_2(S \ e) + w_f (v^-e_i - v^-e_j)^2 >= lambda_2(S \ e + f) (concavity; one kernel, K x m);
 *   3. solves exactly, row after row in decreasing order of the row's largest bound and inside a row in decreasing order of the
 *      bound, only what can still exceed max(tau, top): tau = lambda_2(S) + min_gain, top the largest value solved in the round;
 *   4. scans the solved pairs in (e, f) order: a pair replaces the running value (initially tau) only if it exceeds it by more than
 *      1e-8.  No pair: *converged = 1 and the call returns.  Else the swap is applied (two columns of the low-rank block, folded when
 *      due) and the new Fiedler pair polished.
 * The call stops with *converged = 0 after max_swaps swaps (max_swaps = 0 is legal: the selection is loaded, lambda2_out[0]
 * reported).  Every accepted swap raises lambda_2 by more than 1e-8; every reported lambda_2 obeys GreedyEig's stop rule.
 * Outputs, any of which may be NULL: sel_out[k] the final selection ascending; out_idx[t], in_idx[t] the edges of swap
 * t < *n_swaps (max_swaps entries each); lambda2_out[max_swaps + 1]: entry 0 is lambda_2 of sel_in, entry t + 1 lambda_2 after swap
 * t; counts[3 max_swaps]: per round r < *n_swaps + *converged the triple {pairs solved exactly, operator applications summed over
 * all columns of the round, removal pairs solved}; t_ms[2] = {wall time of the call, device time between its first and last
 * command}.  Results are a function of the inputs alone: runs repeat bit for bit.  The call keeps k Fiedler vectors and k rows of
 * bounds (8 k (ldv + ldm) bytes; ldv = n rounded up to 64, ldm = m rounded up to 4), made by the first call, freed by
 * machip_eig_destroy.
 * MACHIP_BAD_ARG, decided on the host (machip_last_error names the reason): NULL handle or sel_in; k < 1 or k >= m; an index
 * outside [0, m); a repeated index; max_swaps < 0; min_gain < 0 or not finite; 8 k (ldv + ldm) bytes beyond the device's free
 * memory (or option eig_xch_max_mb, MiB); a MACHIP_EIG_MATRIX_FREE handle (no Sigma to exchange on: machip_eig_exchange_free).  MACHIP_NOT_CONVERGED: a Fiedler solve missed the stop rule (the handle is reset).
 * Afterwards machip_eig_candidate_lambda2, machip_eig_candidate_bounds and machip_eig_info (its per-pick arrays: per round) refer
 * to the fixed graph plus sel_out; machip_eig_select resets as it always has. */
int machip_eig_exchange(machip_eig* h, int64_t k, const int32_t* sel_in, int64_t max_swaps, double min_gain, int32_t* sel_out,
                        int32_t* out_idx, int32_t* in_idx, double* lambda2_out, int64_t* n_swaps, int32_t* converged, int32_t* counts,
                        double* t_ms);
/* machip_eig_exchange on a MACHIP_EIG_MATRIX_FREE or MACHIP_EIG_MATRIX_FREE_TREE handle (mac_amd/csrc/eig_exchange_free.h): the same
 * rounds, rule, scan, tie tolerance, stop rule and outputs, with the history of the route in the place of Sigma and its pending
 * block.  The selection is loaded into the history in blocks of 64 columns (the history is read once per block, not once per edge);
 * a round's trial column is history column `pending` and is dropped after the row; a swap appends two columns (the downdate of e,
 * then f).  The history is sized for k + 2 C + 1 columns after the handle's seeds, C = min(max_swaps, option eig_xch_free_swaps:
 * 1..4096, unset 32), refused with machip_eig_select's message before the state is touched when that does not fit.  When a round
 * would not fit (pending + 3 > seeds + k + 2 C + 1) the history is compacted first: back to the seeds, then the current selection
 * loaded again, ascending; the Fiedler pair is untouched and nothing is solved again.  *n_compactions (may be NULL) counts them.
 * No sum's order depends on anything but the inputs and the options: runs repeat bit for bit.  MACHIP_BAD_ARG: machip_eig_exchange's,
 * by the same messages, except that here a handle with the dense inverse is the one refused (the message names machip_eig_exchange). */
int machip_eig_exchange_free(machip_eig* h, int64_t k, const int32_t* sel_in, int64_t max_swaps, double min_gain, int32_t* sel_out,
                             int32_t* out_idx, int32_t* in_idx, double* lambda2_out, int64_t* n_swaps, int32_t* converged, int32_t* counts,
                             double* t_ms, int64_t* n_compactions);
/* The history of a MACHIP_EIG_MATRIX_FREE / _TREE handle as it stands, to the host: *cols = its columns (machip_eig_info's pending;
 * _TREE: the seeds first); Z[ld * *cols] the columns, ld doubles each, column-major as stored (rows n - 1 .. ld are 0), c[*cols] their
 * coefficients: Sigma_cur = Sigma0 - Z diag(c) Z^T, Sigma0 the inverse of the chain's (the spanning tree's) reduced Laplacian.  Z and
 * c both NULL: only *cols.  MACHIP_BAD_ARG: NULL handle, a handle with the dense inverse, cap_cols below the columns held. */
int machip_eig_history(machip_eig* h, int64_t cap_cols, double* Z, double* c, int64_t* cols);

#ifdef __cplusplus
}
#endif
#endif /* MACHIP_H */
