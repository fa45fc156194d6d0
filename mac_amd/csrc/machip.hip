// machip.hip -- C ABI of libmachip.so (see include/machip.h).  gfx950 only.  An entry point checks its arguments, sets the device
// and calls one function of the family's headers; what the ABI returns by pointer is copied out here where that is all there is to do.
#include <climits>

#include "mac_lanes.h"
#include "esp.h"
#include "esp_free.h"
#include "esp_tree.h"
#include "esp_select.h"
#include "kirchhoff.h"
#include "esp_relax.h"
#include "esp_exchange.h"
#include "esp_exchange_edge.h"
#include "eig_exchange.h"
#include "eig_routes.h"

namespace machip {
thread_local std::string g_err;
}
using namespace machip;

// ------------------------------------------------------------------------------------------
extern "C" {

int machip_version(void) { return MACHIP_ABI_VERSION; }
int machip_sizeof_stats(void) { return (int)sizeof(machip_solve_stats); }

int machip_device_count(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

const char* machip_last_error(void) { return g_err.c_str(); }

// ---- MAC (mac.h; the communicators: mac_comm.h; Frank-Wolfe: mac_fw.h; the lanes: mac_lanes.h) ----

int machip_create(int device, int64_t n, int64_t n_fixed, const int32_t* fi, const int32_t* fj, const double* fw,
                  int64_t m, const int32_t* ci, const int32_t* cj, const double* cw, double min_sel_tol,
                  machip_problem** out) {
    if (!out) return fail(MACHIP_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (n < 2 || n > 2000000000ll) return fail(MACHIP_BAD_ARG, "num_nodes must be in [2, 2e9]");
    if (n_fixed < 0 || m < 0 || m > 2000000000ll) return fail(MACHIP_BAD_ARG, "bad edge counts");
    if ((n_fixed && (!fi || !fj || !fw)) || (m && (!ci || !cj || !cw))) return fail(MACHIP_BAD_ARG, "NULL edge array");
    // mac/solvers/mac.py:46-52
    if (n_fixed + m < n - 1) return fail(MACHIP_BAD_ARG, "fewer than n-1 edges: no spanning tree possible");
    if ((double)(n_fixed + m) > 0.5 * (double)n * (double)(n - 1)) return fail(MACHIP_BAD_ARG, "more edges than the complete graph");
    if (machip_device_count() <= 0) return fail(MACHIP_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    return create_handle(device, n, n_fixed, fi, fj, fw, m, ci, cj, cw, min_sel_tol, out);
}

void machip_destroy(machip_problem* p) { if (p) destroy_handle(p); }

int machip_set_x(machip_problem* p, const double* x) {
    if (!p || !x || p->csr_only) return fail(MACHIP_BAD_ARG, "machip_set_x: bad handle or NULL x");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemcpyAsync(p->x, x, sizeof(double) * (size_t)p->m, hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->assembled = false; p->xb_valid = false;
    return MACHIP_OK;
}

int machip_get_x(machip_problem* p, double* x) {
    if (!p || !x || p->csr_only) return fail(MACHIP_BAD_ARG, "machip_get_x: bad handle or NULL x");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemcpyAsync(x, p->x, sizeof(double) * (size_t)p->m, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return MACHIP_OK;
}

int machip_assemble(machip_problem* p, int64_t* nnz_out) {
    if (!p) return fail(MACHIP_BAD_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(p->device));
    ST_TRY(assemble(p));
    if (nnz_out) *nnz_out = p->nnz;
    return MACHIP_OK;
}

int machip_get_laplacian(machip_problem* p, int32_t* indptr, int32_t* indices, double* data) {
    if (!p || !indptr || !indices || !data) return fail(MACHIP_BAD_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(p->device));
    if (!p->assembled) ST_TRY(assemble(p));
    HIP_TRY(hipMemcpyAsync(indptr, p->rowptr, sizeof(int) * ((size_t)p->n + 1), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipMemcpyAsync(indices, p->col, sizeof(int) * (size_t)p->nnz, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipMemcpyAsync(data, p->val, sizeof(double) * (size_t)p->nnz, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return MACHIP_OK;
}

int machip_fiedler(machip_problem* p, double tol, int max_steps, const double* x0, int warm_start,
                   double* lambda2, double* v_out, double* X_out, int q, machip_solve_stats* stats) {
    if (!p || !lambda2) return fail(MACHIP_BAD_ARG, "NULL argument");
    if (X_out && (q < 1 || q > 4)) return fail(MACHIP_BAD_ARG, "q must be in [1,4]");
    HIP_TRY(hipSetDevice(p->device));
    const int st = run_fiedler(p, tol, max_steps, x0, warm_start, lambda2, stats);
    if (!completed(st)) return st;
    const std::string keep = g_err;
    if (v_out) {
        HIP_TRY(hipMemcpyAsync(v_out, p->sol.yvec, sizeof(double) * (size_t)p->n, hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
    }
    if (X_out) ST_TRY(p->sol.ritz_block(q, X_out));
    g_err = keep;
    return st;
}

int machip_set_start(machip_problem* p, const double* x0) {
    if (!p || !x0) return fail(MACHIP_BAD_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemcpyAsync(p->sol.start, x0, sizeof(double) * (size_t)p->n, hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->sol.have_start = true;
    ++p->start_version;
    return MACHIP_OK;
}

int machip_gradient(machip_problem* p, double* g_out) {
    if (!p || p->csr_only) return fail(MACHIP_BAD_ARG, "bad handle");
    return gradient(p, g_out);      // (sets the device itself, under its guard)
}

int machip_lp_topk(machip_problem* p, int64_t k, double* s_out) {
    if (!p || p->csr_only) return fail(MACHIP_BAD_ARG, "bad handle");
    HIP_TRY(hipSetDevice(p->device));
    return lp_topk(p, k, s_out);
}

int machip_fw_step(machip_problem* p, int64_t k, int iter, double tol, int max_steps, int warm_start,
                   double* f, double* dual, double* gnorm, machip_solve_stats* stats) {
    if (!p || p->csr_only || !f || !dual || !gnorm) return fail(MACHIP_BAD_ARG, "bad argument");
    return fw_step(p, k, iter, tol, max_steps, warm_start, f, dual, gnorm, stats);      // (sets the device itself, under its guard)
}

int machip_fw_run(machip_problem* p, int64_t k, int first_iter, int max_iters, double gap_tol, double grad_tol, double tol, int max_steps,
                  int warm_start, double* upper_inout, double* f_traj, double* dual_traj, double* gnorm_traj, machip_solve_stats* stats,
                  int* modes, int* iters_done) {
    if (!p || p->csr_only || max_iters < 0 || first_iter < 0 || !upper_inout || !iters_done) return fail(MACHIP_BAD_ARG, "machip_fw_run: bad argument");
    machip_solve_stats st;      // (every step sets the device)
    return fw_loop(p, k, first_iter, max_iters, gap_tol, grad_tol, tol, max_steps, warm_start, &st, upper_inout, iters_done,
                   [&](int i, double f, double dual, double gn, const machip_solve_stats* s) {
                       if (f_traj) f_traj[i] = f;
                       if (dual_traj) dual_traj[i] = dual;
                       if (gnorm_traj) gnorm_traj[i] = gn;
                       if (stats) stats[i] = *s;
                       if (modes) { modes[2 * i] = p->sol.last_mode; modes[2 * i + 1] = (int)p->sol.last_wb_s; }
                   });
}

int machip_round_nearest(machip_problem* p, int64_t k, int decimals, double* rounded_out) {
    if (!p || p->csr_only || !rounded_out) return fail(MACHIP_BAD_ARG, "bad argument");
    ST_TRY(decimals_ok(decimals));
    HIP_TRY(hipSetDevice(p->device));
    return round_nearest(p, k, decimals, rounded_out);
}

int machip_fw_commit(machip_problem* p) {
    if (!p || p->csr_only) return fail(MACHIP_BAD_ARG, "bad handle");
    fw_commit(p);
    return MACHIP_OK;
}

int machip_fiedler_csr(int device, int64_t n, const int32_t* indptr, const int32_t* indices, const double* data,
                       double tol, int max_steps, const double* x0, double* lambda2, double* v_out, double* X_out,
                       int q, machip_solve_stats* stats) {
    if (!indptr || !indices || !data || !lambda2) return fail(MACHIP_BAD_ARG, "NULL argument");
    if (n < 2 || n > 2000000000ll) return fail(MACHIP_BAD_ARG, "n must be in [2, 2e9]");
    if (X_out && (q < 1 || q > 4)) return fail(MACHIP_BAD_ARG, "q must be in [1,4]");
    return fiedler_csr(device, n, indptr, indices, data, tol, max_steps, x0, lambda2, v_out, X_out, q, stats);      // (validates the matrix on the host, then sets the device)
}

static int pairs_args(int64_t n, int q, const double* lambda_out) {
    if (!lambda_out) return fail(MACHIP_BAD_ARG, "machip_lowest_pairs: lambda_out is NULL");
    if (q < 1 || q > 16 || (int64_t)q > n - 1) return fail(MACHIP_BAD_ARG, "machip_lowest_pairs: q must be in [1, min(16, n - 1)]");
    return MACHIP_OK;
}

int machip_lowest_pairs(machip_problem* p, int q, double tol, int max_steps, const double* X0, int warm_start, double* lambda_out,
                        double* V_out, double* residual_out, int32_t* steps_out, int32_t* restarts_out, int32_t* status_out,
                        int32_t* reordered_out, int32_t* first_rank_out) {
    if (!p) return fail(MACHIP_BAD_ARG, "machip_lowest_pairs: NULL handle");
    ST_TRY(pairs_args(p->n, q, lambda_out));
    if (p->is_lane || p->comm || p->lgroup || p->ipcg || p->nranks > 1)
        return fail(MACHIP_BAD_ARG, "machip_lowest_pairs: one GPU, one rank -- not on an evaluation lane or a handle that belongs to a communicator");
    HIP_TRY(hipSetDevice(p->device));
    return lowest_pairs(p, q, tol, max_steps, X0, warm_start, lambda_out, V_out, residual_out, steps_out, restarts_out, status_out, reordered_out, first_rank_out);
}

int machip_lowest_pairs_csr(int device, int64_t n, const int32_t* indptr, const int32_t* indices, const double* data, int q, double tol,
                            int max_steps, const double* X0, int warm_start, double* lambda_out, double* V_out, double* residual_out,
                            int32_t* steps_out, int32_t* restarts_out, int32_t* status_out, int32_t* reordered_out, int32_t* first_rank_out) {
    if (!indptr || !indices || !data) return fail(MACHIP_BAD_ARG, "NULL argument");
    if (n < 2 || n > 2000000000ll) return fail(MACHIP_BAD_ARG, "n must be in [2, 2e9]");
    ST_TRY(pairs_args(n, q, lambda_out));
    return with_csr_handle(device, n, indptr, indices, data, [&](machip_problem* p) {      // (validates the matrix on the host, then sets the device)
        return lowest_pairs(p, q, tol, max_steps, X0, warm_start, lambda_out, V_out, residual_out, steps_out, restarts_out, status_out, reordered_out, first_rank_out);
    });
}

int machip_lowest_pairs_csr2(int device, int64_t n, const int32_t* indptr, const int32_t* indices, const double* data, int q, double tol,
                             int max_steps, const double* X0, int warm_start, double* lambda_out, double* V_out, double* residual_out,
                             int32_t* steps_out, int32_t* restarts_out, int32_t* status_out, int32_t* reordered_out, int32_t* first_rank_out,
                             int pairs_precond, int32_t* method_out, int32_t* closures_out, double* build_ms_out) {
    if (!indptr || !indices || !data) return fail(MACHIP_BAD_ARG, "NULL argument");
    if (n < 2 || n > 2000000000ll) return fail(MACHIP_BAD_ARG, "n must be in [2, 2e9]");
    ST_TRY(pairs_args(n, q, lambda_out));
    return with_csr_handle(device, n, indptr, indices, data, [&](machip_problem* p) {
        if (pairs_precond >= 0) p->sol.opt.v[kOpt_pairs_precond] = pairs_precond;      // (else: the process default, as every option of this handle)
        const int st = lowest_pairs(p, q, tol, max_steps, X0, warm_start, lambda_out, V_out, residual_out, steps_out, restarts_out, status_out, reordered_out, first_rank_out);
        if (st == MACHIP_OK) lowest_pairs_info(*p->sol.pairs, q, method_out, closures_out, build_ms_out);
        return st;
    });
}

int machip_lowest_pairs_info(machip_problem* p, int q, int32_t* method_out, int32_t* closures_out, double* build_ms_out) {
    if (!p || !p->sol.pairs || q < 1 || q > p->sol.pairs->last_q) return fail(MACHIP_BAD_ARG, "machip_lowest_pairs_info: no machip_lowest_pairs call of at least q columns on this handle");
    lowest_pairs_info(*p->sol.pairs, q, method_out, closures_out, build_ms_out);
    return MACHIP_OK;
}

int machip_lowest_pairs_time(machip_problem* p, int q, double* ms_out) {
    if (!p || !ms_out || !p->sol.pairs || q < 1 || q > p->sol.pairs->last_q) return fail(MACHIP_BAD_ARG, "machip_lowest_pairs_time: no machip_lowest_pairs call of at least q columns on this handle");
    for (int r = 0; r < q; ++r) ms_out[r] = p->sol.pairs->last_ms[r];
    return MACHIP_OK;
}

int machip_gradient_block(machip_problem* p, int q, const double* V, double* G_out) {
    if (!p || p->csr_only || q < 1 || !V || (!G_out && p->m)) return fail(MACHIP_BAD_ARG, "machip_gradient_block: bad handle, q < 1 or NULL block");
    if (p->nranks > 1) return fail(MACHIP_BAD_ARG, "machip_gradient_block: not on a handle that belongs to a communicator");
    HIP_TRY(hipSetDevice(p->device));
    return gradient_block(p, q, V, G_out);
}

void machip_release_cache(void) { release_cache(); }

int machip_spmv(machip_problem* p, const double* v, double* y, int variant) {
    if (!p || !v || !y) return fail(MACHIP_BAD_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(p->device));
    if (!p->assembled) ST_TRY(assemble(p));
    HIP_TRY(hipMemcpyAsync(p->sol.y_raw, v, sizeof(double) * (size_t)p->n, hipMemcpyHostToDevice, p->stream));
    const SpmvPlan pl = plan_spmv(p->sol.opt, p->n, p->nnz, variant);
    OpPlain op{p->sol.w2};
    launch_spmv(pl, p->stream, p->csr(), p->sol.y_raw, op);
    HIP_TRY(hipMemcpyAsync(y, p->sol.w2, sizeof(double) * (size_t)p->n, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return MACHIP_OK;
}

int machip_landscape(machip_problem* p, int sweeps, double* u_out) {
    if (!p || !u_out || sweeps < 0 || sweeps > 16) return fail(MACHIP_BAD_ARG, "bad argument (0 <= sweeps <= 16)");
    HIP_TRY(hipSetDevice(p->device));
    if (!p->assembled) ST_TRY(assemble(p));
    const SpmvPlan pl = p->sol.landscape_plan(p->nnz);
    const double* f = p->sol.landscape_field(p->csr(), pl, sweeps);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(u_out, f, sizeof(double) * (size_t)p->n, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return MACHIP_OK;
}

int machip_profile_spmv(machip_problem* p, int reps, double* avg_us, double* bytes_per_launch) {
    if (!p || !avg_us || reps < 1) return fail(MACHIP_BAD_ARG, "bad argument");
    HIP_TRY(hipSetDevice(p->device));
    return profile_spmv(p, reps, avg_us, bytes_per_launch);
}

int machip_comm_unique_id(void* id128) {
    if (!id128) return fail(MACHIP_BAD_ARG, "NULL id buffer");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is expected to be 128 bytes");
    ncclUniqueId id;
    NCCL_TRY(ncclGetUniqueId(&id));
    memcpy(id128, &id, sizeof(id));
    return MACHIP_OK;
}

int machip_comm_init(machip_problem* p, int rank, int nranks, const void* id128) {
    if (!p || p->csr_only || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(MACHIP_BAD_ARG, "bad argument");
    if (nranks > 64) return fail(MACHIP_BAD_ARG, "at most 64 ranks");
    if (p->comm || p->lgroup) return fail(MACHIP_BAD_ARG, "machip_comm_init: handle already belongs to a communicator");
    HIP_TRY(hipSetDevice(p->device));
    return comm_init(p, rank, nranks, id128);
}

int machip_ipc_blob_bytes(void) { return (int)sizeof(IpcBlob); }

int machip_ipc_export(machip_problem* p, void* blob, int blob_bytes) {
    if (!p || p->csr_only || !blob || blob_bytes < (int)sizeof(IpcBlob)) return fail(MACHIP_BAD_ARG, "machip_ipc_export: bad argument");
    if (p->lgroup || p->ipcg) return fail(MACHIP_BAD_ARG, "machip_ipc_export: handle already belongs to a communicator");
    HIP_TRY(hipSetDevice(p->device));
    return ipc_export(p, blob);
}

int machip_comm_init_ipc(machip_problem* p, int rank, int nranks, const void* blobs, double timeout_s) {
    if (!p || p->csr_only || !blobs || nranks < 2 || nranks > kMaxPeers || rank < 0 || rank >= nranks)
        return fail(MACHIP_BAD_ARG, "machip_comm_init_ipc: 2..8 ranks, a blob per rank");
    if (!p->ipcg || p->ipcg->nranks) return fail(MACHIP_BAD_ARG, "machip_comm_init_ipc: call machip_ipc_export first (once)");
    if (p->lgroup) return fail(MACHIP_BAD_ARG, "machip_comm_init_ipc: handle already belongs to an in-process communicator");
    HIP_TRY(hipSetDevice(p->device));
    return comm_init_ipc(p, rank, nranks, blobs, timeout_s);
}

int machip_comm_close_ipc(machip_problem* p) {
    if (!p || !p->ipcg) return fail(MACHIP_BAD_ARG, "machip_comm_close_ipc: no inter-process communicator");
    p->ipcg->clean_exit = true;
    return MACHIP_OK;
}

int machip_comm_init_local(machip_problem** handles, int nranks) {
    if (!handles || nranks < 1 || nranks > 64) return fail(MACHIP_BAD_ARG, "machip_comm_init_local: 1..64 handles");
    for (int r = 0; r < nranks; ++r) {
        machip_problem* p = handles[r];
        if (!p || p->csr_only || p->comm || p->lgroup) return fail(MACHIP_BAD_ARG, "machip_comm_init_local: NULL, CSR-only or already attached handle");
        if (p->m != handles[0]->m || p->n != handles[0]->n) return fail(MACHIP_BAD_ARG, "machip_comm_init_local: handles of different problems");
    }
    return comm_init_local(handles, nranks);      // (sets each handle's device in turn)
}

int machip_selftest_watchdog(int work_ms, int limit_ms) {
    // (test hook, no GPU needed: the watchdog around the RCCL first-contact calls, exercised with a sleeping stand-in)
    return run_with_watchdog([=]() -> int { std::this_thread::sleep_for(std::chrono::milliseconds(work_ms)); return MACHIP_OK; },
                             1e-3 * (double)limit_ms, "watchdog self-test (" + std::to_string(work_ms) + " ms of work)");
}

int machip_peer_access(int device_a, int device_b) {
    int can = 0;
    if (device_a == device_b) return 1;
    if (hipDeviceCanAccessPeer(&can, device_a, device_b) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return can;
}

int machip_comm_mode(machip_problem* p) {
    if (!p) return -1;
    if (p->ipcg && p->ipcg->nranks) return p->sol.ipc ? (p->sol.last_seq_sharded ? 5 : 4) : (p->comm ? 1 : 6);
    if (p->comm) return 1;
    if (p->lgroup) return p->lgroup->shard_eig ? 3 : 2;
    return 0;
}

int machip_panel_plan(int64_t n, int64_t nnz, int maxlen, int* out12) {
    if (n < 1 || n > 2000000000ll || nnz < 0 || !out12) return fail(MACHIP_BAD_ARG, "machip_panel_plan: bad argument");
    const Options& opt = default_options();
    const PanPlan pp = plan_panel(opt, (int)n, (long)nnz, maxlen, true, -1, false, OPT(stream, 1) != 0);
    out12[0] = pp.on ? 1 : 0; out12[1] = pp.NP; out12[2] = pp.C; out12[3] = pp.NB; out12[4] = pp.NTB; out12[5] = pp.TWW; out12[6] = pp.RPT; out12[7] = pp.grid2;
    out12[8] = pp.u ? 1 : 0; out12[9] = pp.LPT; out12[10] = pp.TWT; out12[11] = pp.cells;
    return MACHIP_OK;
}

#ifdef PAN_CLOCKS
// developer build (MACHIP_BUILD_FLAGS=-DPAN_CLOCKS, tools/pan_clocks.py): the 16 wall-clock stamps (100 MHz) every workgroup of the
// LAST column-panel matrix launch left
extern "C" int machip_debug_pan_clocks(machip_problem* p, long long* out, int groups) {
    if (!p || !out || groups < 1 || groups > kMaxGrid || !p->sol.panv.clk) return fail(MACHIP_BAD_ARG, "machip_debug_pan_clocks: no clock buffer");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    HIP_TRY(hipMemcpy(out, p->sol.panv.clk, sizeof(long long) * 16 * (size_t)groups, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(p->sol.panv.clk, 0, sizeof(long long) * 16 * (size_t)kMaxGrid));      // (the next read sees one launch shape only)
    return MACHIP_OK;
}
#endif

int machip_shard_plan(int64_t m, int nranks, int rank, int64_t* lo, int64_t* hi, int64_t* shard) {
    if (m < 0 || nranks < 1 || rank < 0 || rank >= nranks || !lo || !hi || !shard) return fail(MACHIP_BAD_ARG, "machip_shard_plan: bad argument");
    long a, b, c;
    shard_plan((long)m, nranks, rank, &a, &b, &c);
    *lo = a; *hi = b; *shard = c;
    return MACHIP_OK;
}

int machip_eval_batch(machip_problem* p, int B, const double* X, double tol, int max_steps, double* lambda2, int* status) {
    if (!p || p->csr_only || p->is_lane || B < 0 || (B && (!X || !lambda2))) return fail(MACHIP_BAD_ARG, "machip_eval_batch: bad argument");
    if (B == 0) return MACHIP_OK;
    HIP_TRY(hipSetDevice(p->device));
    return eval_batch(p, B, X, tol, max_steps, lambda2, status);
}

int machip_fw_sweep(machip_problem* p, int B, const int64_t* ks, const double* X0, int max_iters, double gap_tol,
                    double grad_tol, double tol, int max_steps, int warm_start, int round_decimals, double* X_out,
                    double* R_out, double* upper, double* f_traj, int* iters, int* status) {
    if (!p || p->csr_only || p->is_lane || B < 0 || max_iters < 0 || (B && (!ks || !X0 || !X_out || !upper || !iters || !status)))
        return fail(MACHIP_BAD_ARG, "machip_fw_sweep: bad argument");
    if (p->nranks > 1) return fail(MACHIP_BAD_ARG, "machip_fw_sweep: not on a handle that belongs to a communicator");
    if (B == 0) return MACHIP_OK;
    HIP_TRY(hipSetDevice(p->device));
    return fw_sweep(p, B, ks, X0, max_iters, gap_tol, grad_tol, tol, max_steps, warm_start, round_decimals, X_out, R_out, upper, f_traj, iters, status);
}

int machip_set_option(machip_problem* p, const char* name, int64_t value) {
    const int id = option_id(name);
    if (id < 0) return fail(MACHIP_BAD_ARG, std::string("machip_set_option: unknown option '") + (name ? name : "(null)") + "'");
    const long v = value == INT64_MIN ? kOptAuto : (long)value;
    if (!p) default_options().v[id] = v;
    else set_option(p, id, v);
    return MACHIP_OK;
}

int machip_get_option(machip_problem* p, const char* name, int64_t* value) {
    const int id = option_id(name);
    if (id < 0 || !value) return fail(MACHIP_BAD_ARG, "machip_get_option: unknown option or NULL output");
    const long v = p ? p->sol.opt.v[id] : default_options().v[id];
    *value = v == kOptAuto ? INT64_MIN : (int64_t)v;
    return MACHIP_OK;
}

const char* machip_option_name(int i) { return (i >= 0 && i < kNumOpts) ? option_names()[i] : nullptr; }

int machip_comm_timing(machip_problem* p, double* grad_us, double* exchange_us) {
    if (!p || !grad_us || !exchange_us) return fail(MACHIP_BAD_ARG, "machip_comm_timing: NULL argument");
    *grad_us = 0.0; *exchange_us = 0.0;
    if (!p->ev_g_valid) return fail(MACHIP_BAD_ARG, "machip_comm_timing: no sharded gradient has been computed on this handle");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipEventSynchronize(p->ev_g2));
    float a = 0.f, b = 0.f;
    HIP_TRY(hipEventElapsedTime(&a, p->ev_g0, p->ev_g1));
    HIP_TRY(hipEventElapsedTime(&b, p->ev_g1, p->ev_g2));
    *grad_us = 1e3 * (double)a; *exchange_us = 1e3 * (double)b;
    return MACHIP_OK;
}

int machip_solve_mode(machip_problem* p, int64_t* closures) {
    if (!p) return -1;
    if (closures) *closures = p->sol.last_wb_s;
    return p->sol.last_mode;
}

int machip_comm_drop(machip_problem* p) {
    if (!p) return fail(MACHIP_BAD_ARG, "machip_comm_drop: NULL handle");
    if (p->lgroup) return fail(MACHIP_BAD_ARG, "machip_comm_drop: in-process communicators end with their handles");
    HIP_TRY(hipSetDevice(p->device));
    return comm_drop(p);
}

int machip_comm_drop_ipc(machip_problem* p) {
    if (!p || !p->ipcg) return fail(MACHIP_BAD_ARG, "machip_comm_drop_ipc: no inter-process communicator");
    HIP_TRY(hipSetDevice(p->device));
    return comm_drop_ipc(p);
}

int machip_set_solver(machip_problem* p, int mode) {
    if (!p || mode < 0 || mode > 2) return fail(MACHIP_BAD_ARG, "machip_set_solver: mode must be 0 (auto), 1 (Lanczos) or 2 (preconditioned)");
    p->sol.solver_mode = mode;
    return MACHIP_OK;
}

int machip_set_precision(machip_problem* p, int precision) {
    if (!p || precision < 0 || precision > 1) return fail(MACHIP_BAD_ARG, "machip_set_precision: 0 (f64) or 1 (f32 iterate + f64 refinement)");
    p->sol.precision = precision;
    return MACHIP_OK;
}

int machip_synchronize(machip_problem* p) {
    if (!p) return fail(MACHIP_BAD_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return MACHIP_OK;
}

int machip_membench(int device, int64_t bytes, int reps, double* read_gbs, double* triad_gbs) {
    if (bytes < (1 << 20) || reps < 1 || !read_gbs || !triad_gbs) return fail(MACHIP_BAD_ARG, "machip_membench: bytes >= 1 MiB, reps >= 1, non-NULL outputs");
    if (machip_device_count() <= 0) return fail(MACHIP_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    return membench(bytes, reps, read_gbs, triad_gbs);
}

// Host-only helper exported for CPU tests of the tridiagonal analysis (not part of the
// reference surface): smallest eigenpair of the J x J symmetric tridiagonal (a, b[1..J)).
int machip_host_tridiag_smallest(const double* a, const double* b, int J, double* theta, double* s) {
    if (!a || !b || J < 1 || !theta || !s) return fail(MACHIP_BAD_ARG, "bad argument");
    tri::Smallest sm;
    std::vector<double> wk;
    tri::smallest_eigpair(a, b, J, nullptr, 0, 0.0, sm, wk);
    *theta = sm.theta;
    for (int i = 0; i < J; ++i) s[i] = sm.s[(size_t)i];
    return MACHIP_OK;
}

// Host-only: the deterministic reading of a Lanczos sequence (follow.h) over a finished record array -- tri3 = interleaved
// (alpha_j, beta_j, ||v_j||_1) triples valid through beta_J.  points[0..*npoints) = the analysis points visited (at most cap are
// stored), *jeff = order of the tridiagonal the sequence ends on (-1: the estimate never fell below e_target within J),
// *est = the estimate at the last point.  For the `-m "not gpu"` tests of the rule the solver ends its solves by.
int machip_host_follow_records(const double* tri3, int J, int n, double e_target, double tiny_l, int jcap, int* points, int cap,
                               int* npoints, int* jeff, double* est) {
    if (!tri3 || J < 1 || n < 2 || !npoints || !jeff || !est || !(e_target > 0.0) || cap < 0 || (cap > 0 && !points))
        return fail(MACHIP_BAD_ARG, "bad argument");
    std::vector<double> ha, hb, hl1, guess, wk;
    tri::Smallest sm;
    FollowCfg fc;
    fc.n = n; fc.jcap = jcap > 0 ? (jcap & ~1) : INT_MAX; fc.tiny_l = tiny_l > 0 ? tiny_l : 1.0;
    Follower F(fc, e_target, ha, hb, hl1, guess, sm, wk);
    *npoints = 0; *jeff = -1; *est = 0.0;
    while (F.next_a <= J) {
        const int a = F.next_a;
        if (!F.analyse(tri3, a)) return fail(MACHIP_BAD_ARG, "start vector is constant, zero or not finite");
        if (*npoints < cap) points[*npoints] = a;
        ++*npoints;
        *est = F.est;
        if (F.triggered()) { *jeff = F.Jeff; break; }
        if (a >= fc.jcap) break;
    }
    return MACHIP_OK;
}

// ---- GreedyESP (esp.h; the routes without Sigma: esp_free.h, esp_tree.h; the three together: esp_select.h) ----

// machip_esp_create; tplan: the spanning-tree plan the handle's tables are made from (MACHIP_ESP_SPANNING_TREE), left to the caller
static int esp_create(int device, int64_t n, int64_t n_fixed, const int32_t* fi, const int32_t* fj, const double* fw, int64_t m,
                      const int32_t* ci, const int32_t* cj, const double* cw, int fold, int flags, machip_esp** out, EspTreePlan& tplan) {
    if (!out) return fail(MACHIP_BAD_ARG, "out is NULL");
    *out = nullptr;
    ST_TRY(esp_create_check(n, n_fixed, fi, fj, fw, m, ci, cj, cw, fold, flags));
    const bool mfree = (flags & MACHIP_ESP_MATRIX_FREE) != 0, tree = (flags & MACHIP_ESP_SPANNING_TREE) != 0;
    EspFixedClass fixed;
    ST_TRY(esp_classify_fixed(n, n_fixed, fi, fj, fw, flags, fixed));
    if (tree) ST_TRY(esp_tree_plan(n, n_fixed, fi, fj, fw, tplan));
    if (machip_device_count() <= 0) return fail(MACHIP_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipSetDevice(device));
    machip_esp* h = new machip_esp();
    h->device = device; h->n = (int)n; h->np = (int)n - 1; h->m = (int)m; h->fold = mfree ? 0 : fold; h->beta = fixed.beta;
    h->form = tree ? kEspFormTree : mfree ? kEspFormFree : fixed.chain ? 0 : 1;
    h->relax_space = (flags & MACHIP_ESP_EDGE_RELAX_TREE) ? kEspRelaxEdgeTree : (flags & MACHIP_ESP_EDGE_RELAX) ? kEspRelaxEdge : kEspRelaxNode;
    h->free_split = (int)std::max(0l, std::min<long>(default_options().get(kOpt_esp_free_split, 0), kEspFreeMaxSplit));
    h->ld = (h->np + kGjT - 1) / kGjT * kGjT;
    h->hfi.assign(fi, fi + n_fixed); h->hfj.assign(fj, fj + n_fixed); h->hfw.assign(fw, fw + n_fixed);
    h->hci.assign(ci, ci + m); h->hcj.assign(cj, cj + m); h->hcw.assign(cw, cw + m);
    int st = esp_alloc(h);
    if (st == MACHIP_OK)      // Sigma0: the tree's tables (the seeds run at the first use), the chain's closed form, the dense inverse
        st = tree ? esp_tree_upload(h, tplan) : fixed.chain ? esp_sigma0_chain(h, fixed.link) : esp_sigma0_dense(h);
    if (st != MACHIP_OK) { machip_esp_destroy(h); return st; }
    *out = h;
    return MACHIP_OK;
}

int machip_esp_create(int device, int64_t n, int64_t n_fixed, const int32_t* fi, const int32_t* fj, const double* fw,
                      int64_t m, const int32_t* ci, const int32_t* cj, const double* cw, int fold, int flags, machip_esp** out) {
    EspTreePlan tplan;
    return esp_create(device, n, n_fixed, fi, fj, fw, m, ci, cj, cw, fold, flags, out, tplan);
}

void machip_esp_destroy(machip_esp* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    esp_relax_release(h);
    esp_tree_release(h);
    esp_xch_release(h->xc);
    esp_xe_release(h->xe);
    esp_kir_release(h);
    void* bufs[] = {h->bufA, h->bufB, h->cu, h->cv, h->sel, h->pi, h->order, h->bad, h->cw, h->s, h->Zb, h->cb, h->pv, h->gain, h->piv, h->best, h->R, h->part};
    for (void* q : bufs) if (q) (void)hipFree(q);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int machip_esp_tree_plan(int64_t n, int64_t n_fixed, const int32_t* fi, const int32_t* fj, const double* fw, int32_t* parent,
                         double* R, int32_t* pre, int32_t* end, int64_t* n_seeds, int32_t* su, int32_t* sv, double* sw) {
    if (!parent || !R || !pre || !end || !n_seeds || (n_fixed > 0 && (!su || !sv || !sw))) return fail(MACHIP_BAD_ARG, "NULL output");
    EspTreePlan P;
    ST_TRY(esp_tree_plan(n, n_fixed, fi, fj, fw, P));
    std::copy(P.parent.begin(), P.parent.end(), parent);
    std::copy(P.R.begin(), P.R.end(), R);
    std::copy(P.pre.begin(), P.pre.end(), pre);
    std::copy(P.end.begin(), P.end.end(), end);
    *n_seeds = (int64_t)P.sw.size();
    std::copy(P.su.begin(), P.su.end(), su);
    std::copy(P.sv.begin(), P.sv.end(), sv);
    std::copy(P.sw.begin(), P.sw.end(), sw);
    return MACHIP_OK;
}

int machip_esp_seeds(machip_esp* h, int64_t* seeds_out) {
    if (!h || !seeds_out) return fail(MACHIP_BAD_ARG, "NULL handle or output");
    *seeds_out = h->tr ? h->tr->seeds : 0;
    return MACHIP_OK;
}

int machip_esp_info(machip_esp* h, int32_t* info4, double* beta) {
    if (!h) return fail(MACHIP_BAD_ARG, "NULL handle");
    if (info4) { info4[0] = h->form; info4[1] = h->ld; info4[2] = h->fold; info4[3] = h->live ? h->pending : 0; }
    if (beta) *beta = h->beta;
    return MACHIP_OK;
}

int machip_esp_select(machip_esp* h, int nb, const int64_t* ks, int32_t* order_out, double* gain_out, double* t_ms_out) {
    if (!h || nb < 1 || !ks) return fail(MACHIP_BAD_ARG, "NULL handle, no budgets or ks is NULL");
    if (ks[0] <= 0) return fail(MACHIP_BAD_ARG, "budgets must be positive");
    for (int i = 0; i + 1 < nb; ++i) if (ks[i] > ks[i + 1]) return fail(MACHIP_BAD_ARG, "budgets must be monotonically increasing");
    if (ks[nb - 1] > h->m) return fail(MACHIP_BAD_ARG, "not enough candidate edges to satisfy the largest budget");
    HIP_TRY(hipSetDevice(h->device));
    return esp_select(h, nb, ks, order_out, gain_out, t_ms_out);
}

int machip_esp_weighted_resistances(machip_esp* h, double* r_out) {
    if (!h || (!r_out && h->m)) return fail(MACHIP_BAD_ARG, "NULL handle or output");
    HIP_TRY(hipSetDevice(h->device));
    return esp_resistances(h, r_out);
}

// ---- GreedyKirchhoff on GreedyESP's dense handle (kirchhoff.h) ----

int machip_esp_kirchhoff_select(machip_esp* h, int nb, const int64_t* ks, int32_t* order_out, double* gain_out, double* t_ms_out) {
    if (!h || nb < 1 || !ks) return fail(MACHIP_BAD_ARG, "NULL handle, no budgets or ks is NULL");
    if (!order_out || !gain_out || !t_ms_out) return fail(MACHIP_BAD_ARG, "NULL output");
    if (ks[0] <= 0) return fail(MACHIP_BAD_ARG, "budgets must be positive");
    for (int i = 0; i + 1 < nb; ++i) if (ks[i] > ks[i + 1]) return fail(MACHIP_BAD_ARG, "budgets must be monotonically increasing");
    if (ks[nb - 1] > h->m) return fail(MACHIP_BAD_ARG, "not enough candidate edges to satisfy the largest budget");
    ST_TRY(kir_check(h));
    HIP_TRY(hipSetDevice(h->device));
    return kir_select(h, nb, ks, order_out, gain_out, t_ms_out);
}

int machip_esp_kirchhoff_gains(machip_esp* h, double* gains_out) {
    if (!h || (!gains_out && h->m)) return fail(MACHIP_BAD_ARG, "NULL handle or output");
    ST_TRY(kir_check(h));
    HIP_TRY(hipSetDevice(h->device));
    return kir_gains(h, gains_out);
}

int machip_esp_kirchhoff_eval(machip_esp* h, int64_t nsel, const int32_t* idx, double* out2) {
    if (!h || !out2) return fail(MACHIP_BAD_ARG, "NULL handle or output");
    ST_TRY(kir_eval_check(h, nsel, idx));
    ST_TRY(kir_check(h));
    HIP_TRY(hipSetDevice(h->device));
    return kir_eval(h, nsel, idx, out2);
}

// ---- the exchange on GreedyESP's handle (esp_exchange.h) and in the candidates' space (esp_exchange_edge.h) ----

int machip_esp_exchange(machip_esp* h, int64_t k, const int32_t* sel_in, int64_t max_swaps, double min_gain, int32_t* sel_out,
                        int32_t* out_idx, int32_t* in_idx, double* ratio, int64_t* n_swaps, int32_t* converged, double* t_ms) {
    std::vector<int> rowe;
    ST_TRY(esp_xch_check(h, k, sel_in, max_swaps, min_gain, sel_out, out_idx, in_idx, ratio, n_swaps, converged, rowe));
    *n_swaps = 0;
    *converged = 0;
    HIP_TRY(hipSetDevice(h->device));
    return esp_exchange(h, k, rowe, max_swaps, min_gain, sel_out, out_idx, in_idx, ratio, n_swaps, converged, t_ms);
}

int machip_esp_exchange_edge(machip_esp* h, int64_t k, const int32_t* sel_in, int64_t max_swaps, double min_gain, int32_t* sel_out,
                             int32_t* out_idx, int32_t* in_idx, double* ratio, int64_t* n_swaps, int32_t* converged, double* t_ms) {
    std::vector<int> rowe;
    ST_TRY(esp_xch_check(h, k, sel_in, max_swaps, min_gain, sel_out, out_idx, in_idx, ratio, n_swaps, converged, rowe, true));
    *n_swaps = 0;
    *converged = 0;
    ST_TRY(esp_relax_limits(h));
    HIP_TRY(hipSetDevice(h->device));
    return esp_exchange_edge(h, k, rowe, max_swaps, min_gain, sel_out, out_idx, in_idx, ratio, n_swaps, converged, t_ms);
}

// ---- the relaxation of GreedyESP's problem (esp_relax.h; its first call sets the device) ----

int machip_esp_relax_eval(machip_esp* h, const double* x, double* F_out, double* grad_out) {
    if (!h || !F_out) return fail(MACHIP_BAD_ARG, "NULL handle or F_out");
    return esp_relax_eval(h, x, F_out, grad_out);
}

int machip_esp_relax_run(machip_esp* h, int64_t k, int max_iters, double gap_tol, double grad_tol, double* x_inout,
                         double* f_traj, double* dual_traj, double* gnorm_traj, int* iters_out, double* upper_out) {
    if (!h || !iters_out || !upper_out || max_iters < 0) return fail(MACHIP_BAD_ARG, "NULL handle or output, or max_iters < 0");
    *iters_out = 0;
    *upper_out = INFINITY;
    return esp_relax_run(h, k, max_iters, gap_tol, grad_tol, x_inout, f_traj, dual_traj, gnorm_traj, iters_out, upper_out);
}

int machip_esp_relax_inner(machip_esp* h, const double* a, const double* b, double* out) {
    if (!h || !out || (h->m && (!a || !b))) return fail(MACHIP_BAD_ARG, "NULL handle, vector or output");
    return esp_relax_inner(h, a, b, out);
}

int machip_esp_relax_info(machip_esp* h, int32_t* info2) {
    if (!h || !info2) return fail(MACHIP_BAD_ARG, "NULL handle or output");
    return esp_relax_info(h, info2);
}

int machip_esp_relax_gram(machip_esp* h, double* G_out, int64_t M) {
    if (!h || !G_out) return fail(MACHIP_BAD_ARG, "NULL handle or output");
    return esp_relax_gram(h, G_out, M);
}

// ---- GreedyEig (eig.h; the routes without Sigma: eig_free.h, eig_free_tree.h; the three together: eig_routes.h) ----

int machip_eig_create(int device, int64_t n, int64_t n_fixed, const int32_t* fi, const int32_t* fj, const double* fw,
                      int64_t m, const int32_t* ci, const int32_t* cj, const double* cw, int fold, int batch, int flags, machip_eig** out) {
    if (!out) return fail(MACHIP_BAD_ARG, "out is NULL");
    *out = nullptr;
    ST_TRY(eig_create_check(fold, batch, flags));      // (flags: the machip_esp's from here on)
    machip_esp* base = nullptr;
    EspTreePlan tplan;
    ST_TRY(esp_create(device, n, n_fixed, fi, fj, fw, m, ci, cj, cw, fold, flags, &base, tplan));
    return eig_create_build(base, tplan, batch, out);
}

void machip_eig_destroy(machip_eig* h) {
    if (!h) return;
    (void)hipSetDevice(h->base->device);
    if (h->base->stream) (void)hipStreamSynchronize(h->base->stream);
    eig_xch_release(h->xc);
    eig_free_release(h->fr);
    h->release();
    machip_esp_destroy(h->base);
    delete h;
}

int machip_eig_select(machip_eig* h, int64_t k, int32_t* order_out, double* lambda2_out, double* t_ms_out) {
    if (!h || k < 1) return fail(MACHIP_BAD_ARG, "NULL handle or k < 1");
    if (k > h->m) return fail(MACHIP_BAD_ARG, "not enough candidate edges to satisfy the budget");
    HIP_TRY(hipSetDevice(h->base->device));
    return h->select((int)k, order_out, lambda2_out, t_ms_out);
}

int machip_eig_exchange(machip_eig* h, int64_t k, const int32_t* sel_in, int64_t max_swaps, double min_gain, int32_t* sel_out,
                        int32_t* out_idx, int32_t* in_idx, double* lambda2_out, int64_t* n_swaps, int32_t* converged, int32_t* counts, double* t_ms) {
    std::vector<int> rowe;
    ST_TRY(eig_xch_check(h, k, sel_in, max_swaps, min_gain, rowe));
    if (n_swaps) *n_swaps = 0;
    if (converged) *converged = 0;
    HIP_TRY(hipSetDevice(h->base->device));
    return eig_exchange(h, rowe, max_swaps, min_gain, sel_out, out_idx, in_idx, lambda2_out, n_swaps, converged, counts, t_ms);
}

int machip_eig_exchange_free(machip_eig* h, int64_t k, const int32_t* sel_in, int64_t max_swaps, double min_gain, int32_t* sel_out,
                             int32_t* out_idx, int32_t* in_idx, double* lambda2_out, int64_t* n_swaps, int32_t* converged, int32_t* counts, double* t_ms,
                             int64_t* n_compactions) {
    std::vector<int> rowe;
    ST_TRY(eig_xch_check(h, k, sel_in, max_swaps, min_gain, rowe, true));
    if (n_swaps) *n_swaps = 0;
    if (converged) *converged = 0;
    if (n_compactions) *n_compactions = 0;
    HIP_TRY(hipSetDevice(h->base->device));
    return eig_exchange(h, rowe, max_swaps, min_gain, sel_out, out_idx, in_idx, lambda2_out, n_swaps, converged, counts, t_ms, n_compactions);
}

int machip_eig_history(machip_eig* h, int64_t cap_cols, double* Z, double* c, int64_t* cols) {
    if (!h) return fail(MACHIP_BAD_ARG, "NULL handle");
    if (!h->matrix_free()) return fail(MACHIP_BAD_ARG, "machip_eig_history: only a MACHIP_EIG_MATRIX_FREE handle keeps a history");
    HIP_TRY(hipSetDevice(h->base->device));
    return eig_free_history_read(h, cap_cols, Z, c, cols);
}

int machip_eig_candidate_lambda2(machip_eig* h, double* out) {
    if (!h || (!out && h->m)) return fail(MACHIP_BAD_ARG, "NULL handle or output");
    HIP_TRY(hipSetDevice(h->base->device));
    return h->all_lambda2(out);
}

int machip_eig_candidate_bounds(machip_eig* h, double* out) {
    if (!h || (!out && h->m)) return fail(MACHIP_BAD_ARG, "NULL handle or output");
    HIP_TRY(hipSetDevice(h->base->device));
    std::vector<double> u;
    ST_TRY(h->bounds(u));
    for (int e = 0; e < h->m; ++e) out[e] = h->sel[(size_t)e] ? NAN : u[(size_t)e];
    return MACHIP_OK;
}

int machip_eig_seeds(machip_eig* h, int64_t* seeds_out) {
    if (!h || !seeds_out) return fail(MACHIP_BAD_ARG, "NULL handle or output");
    *seeds_out = h->seeds;
    return MACHIP_OK;
}

int machip_eig_info(machip_eig* h, int32_t* info6, double* beta_lambda2, int64_t cap, int32_t* solved_out, int32_t* applies_out) {
    if (!h) return fail(MACHIP_BAD_ARG, "NULL handle");
    if (info6) {
        info6[0] = h->base->form; info6[1] = h->base->ld; info6[2] = h->base->fold; info6[3] = h->batch; info6[4] = h->base->pending;
        info6[5] = (int)h->solved.size();
    }
    if (beta_lambda2) { beta_lambda2[0] = h->base->beta; beta_lambda2[1] = h->lamcur; }
    for (int64_t i = 0; i < cap && i < (int64_t)h->solved.size(); ++i) {
        if (solved_out) solved_out[i] = h->solved[(size_t)i];
        if (applies_out) applies_out[i] = h->applies[(size_t)i];
    }
    return MACHIP_OK;
}

}  // extern "C"
