// mac_amd/csrc/mac_fw.h -- Frank-Wolfe on a MAC handle: the LP vertex (lp_topk), one iteration (fw_step: assemble, eigen-solve,
// gradient -> top-K -> bookkeeping, riding behind the solve's passing check where they can), the commit, the rounding on the device,
// and the ONE loop over iterations (fw_loop) that machip_fw_run and the sweep's lanes (mac_lanes.h) both run.  DESIGN sections 4.6, 6.
#pragma once
#include "mac_comm.h"

namespace machip {

// machip_lp_topk after its handle check, on the handle's device
inline int lp_topk(machip_problem* p, int64_t k, double* s_out) {
    ST_TRY(select_topk(p, (long)k));
    const int grid = (int)std::min<long>(kMaxGrid, (p->m + kBlock - 1) / kBlock);
    k_fw_final<<<std::max(grid, 1), kBlock, 0, p->stream>>>(p->g, nullptr, p->m, p->sel, 0.0, nullptr, p->s, p->part_fw);
    if (s_out) HIP_TRY(hipMemcpyAsync(s_out, p->s, sizeof(double) * (size_t)p->m, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return MACHIP_OK;
}

// machip_fw_step after its argument check
inline int fw_step(machip_problem* p, int64_t k, int iter, double tol, int max_steps, int warm_start,
                   double* f, double* dual, double* gnorm, machip_solve_stats* stats) {
    GroupGuard guard{p};
    HIP_TRY(hipSetDevice(p->device));
    ST_TRY(assemble(p));
    double lam = 0.0;
    const int grid = std::max(1, (int)std::min<long>(kMaxGrid, (p->m + kBlock - 1) / kBlock));
    const double gamma = 2.0 / ((double)iter + 2.0);   // frankwolfe.py:7-8
    // gradient -> top-K -> bookkeeping, on the vector in yvec
    int epi_status = MACHIP_OK;
    auto epilogue = [&](bool speculative) {
        bool fused = false;
        int st = compute_gradient(p, speculative, (long)k, &fused);
        if (st == MACHIP_OK) st = select_topk(p, (long)k, fused);
        if (st == MACHIP_OK) {
            k_fw_final<<<grid, kBlock, 0, p->stream>>>(p->g, p->x, p->m, p->sel, gamma, p->x_next, nullptr, p->d_hdbl, p->tol_sel, p->xb_next);   // partials: host only
            p->xb_next_valid = true;
            if (hipGetLastError() != hipSuccess) st = fail(MACHIP_HIP_ERROR, "k_fw_final launch failed");
        }
        epi_status = st;
    };
    bool done = false;
    // A soft status (step cap reached, disconnected selection) reaches every rank of a communicator alike -- replicated solves
    // are deterministic, the row-partitioned one hands the leader's status round -- and nobody is left in a barrier: the group
    // stays usable (a retry with a larger max_steps, the next iteration).  Only hard errors shut it down.
    if (p->lgroup && p->lgroup->shard_eig) {
        const int st = group_fiedler(p, tol, max_steps, warm_start, &lam, stats);
        if (st != MACHIP_OK) { guard.ok = completed(st); return st; }
    } else {
        // single rank: the epilogue rides behind the solve's explicit check (solver.h, after_check) -- no exchange step in it
        const bool spec = p->nranks <= 1 && p->sol.opt.get(kOpt_spec_epilogue, 1) != 0;
        if (spec) p->sol.after_check = [&] { epilogue(true); };
        const int st = run_fiedler(p, tol, max_steps, nullptr, warm_start, &lam, stats);
        p->sol.after_check = nullptr;
        if (st != MACHIP_OK) { guard.ok = completed(st); return st; }
        done = spec && p->sol.hook_seq == p->sol.final_check_seq && epi_status == MACHIP_OK;     // (the passing check's wait covered it)
    }
    if (!done) {
        epilogue(false);
        if (epi_status != MACHIP_OK) return epi_status;
        HIP_TRY(hipStreamSynchronize(p->stream));
    }
    if (p->ipcg) ST_TRY(p->sol.ipc_check_err("gradient exchange"));
    double d = 0.0, q2 = 0.0;
    for (int b = 0; b < grid; ++b) { d += p->h_dbl[b]; q2 += p->h_dbl[kMaxGrid + b]; }
    *f = lam;
    *dual = lam + d;
    *gnorm = std::sqrt(q2);
    guard.ok = true;
    return MACHIP_OK;
}

// frankwolfe.py:76: the iterate the last step left in x_next, with its support bitmap, becomes x
inline void fw_commit(machip_problem* p) {
    std::swap(p->x, p->x_next);
    std::swap(p->xb, p->xb_next);
    p->xb_valid = p->xb_next_valid; p->xb_next_valid = false;
    p->assembled = false;
}

// The loop of frankwolfe.py:53-76 from iteration first_iter on, at most max_iters steps: the step (warm-started from the second
// iteration of a solve on), u = min(u, dual), the two stop rules -- x stays the current iterate at either -- and the commit.
// on_iter(i, f, dual, gnorm, stats) sees every completed iteration, i counted from 0; stats is the caller's scratch record, filled
// by the step, or NULL.  A step that does not return MACHIP_OK ends the loop with its status; *upper_inout and *iters_done are
// written either way.
template <class OnIter>
int fw_loop(machip_problem* p, int64_t k, int first_iter, int max_iters, double gap_tol, double grad_tol, double tol, int max_steps,
            int warm_start, machip_solve_stats* stats, double* upper_inout, int* iters_done, OnIter&& on_iter) {
    double u = *upper_inout;
    int done = 0, rc = MACHIP_OK;
    for (int i = 0; i < max_iters; ++i) {
        double f = 0.0, dual = 0.0, gn = 0.0;
        if (stats) memset(stats, 0, sizeof(*stats));
        rc = fw_step(p, k, first_iter + i, tol, max_steps, (warm_start && (first_iter + i) > 0) ? 1 : 0, &f, &dual, &gn, stats);
        if (rc != MACHIP_OK) break;
        u = std::min(u, dual);                                      // frankwolfe.py:62
        on_iter(i, f, dual, gn, stats);
        done = i + 1;
        if (gn < grad_tol) break;                                   // frankwolfe.py:65-68 (x stays the current iterate)
        if ((u - f) < gap_tol * std::fabs(f)) break;                // frankwolfe.py:70-74
        fw_commit(p);                                               // frankwolfe.py:76
    }
    *upper_inout = u; *iters_done = done;
    return rc;
}

// machip_round_nearest after its handle check, on the handle's device (decimals_ok: its range check, made before the device is set)
inline int decimals_ok(int decimals) { return decimals > 15 ? fail(MACHIP_BAD_ARG, "decimals must be <= 15") : (int)MACHIP_OK; }
inline int round_nearest(machip_problem* p, int64_t k, int decimals, double* rounded_out) {
    ST_TRY(decimals_ok(decimals));
    const long m = p->m;
    if (m == 0) return MACHIP_OK;
    if (!p->scratch_m) ST_TRY(dev_alloc(&p->scratch_m, (size_t)m + 64));
    const int grid = std::max(1, (int)std::min<long>(kMaxGrid, (m + kBlock - 1) / kBlock));
    double* r = p->s;                       // rounded selection weights (or x itself)
    const bool tb = decimals >= 0;
    if (tb) k_round_keys<<<grid, kBlock, 0, p->stream>>>(p->x, m, std::pow(10.0, decimals), r);
    else HIP_TRY(hipMemcpyAsync(r, p->x, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, p->stream));
    ST_TRY(select_on(p, r, (long)k, p->sel, 1));
    int two = 0;
    if (tb && k > 0 && k < m) {
        SelState h;
        HIP_TRY(hipMemcpyAsync(&h, p->sel, sizeof(SelState), hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        if (h.kk < h.cnt_eq) {              // more candidates tie at the k-th rounded value than fit
            k_tie_keys<<<grid, kBlock, 0, p->stream>>>(r, p->cw, m, p->sel, p->scratch_m);
            ST_TRY(select_on(p, p->scratch_m, (long)h.kk, p->sel + 1, 1));
            two = 1;
        }
    }
    k_round_mark<<<grid, kBlock, 0, p->stream>>>(r, p->scratch_m, m, p->sel, p->sel + 1, two, r);
    HIP_TRY(hipMemcpyAsync(rounded_out, r, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return MACHIP_OK;
}

}  // namespace machip
