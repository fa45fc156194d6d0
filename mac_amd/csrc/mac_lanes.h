// mac_amd/csrc/mac_lanes.h -- evaluation lanes of a MAC handle: lightweight copies that share the pattern and the candidate arrays
// and solve on streams (and solver states) of their own.  A lane's stream and buffers, the lanes a batch gets (prepare_lanes), the
// ONE worker pool that hands the entries of a batch to the lanes (run_on_lanes), and the two batches: machip_eval_batch (lambda_2
// of B vectors) and machip_fw_sweep (B Frank-Wolfe solves, each mac_fw.h's fw_loop).  DESIGN section 6.
#pragma once
#include <atomic>
#include <limits>
#include <thread>

#include "mac_fw.h"

namespace machip {

// ROCm maps a process's HIP streams onto GPU_MAX_HW_QUEUES hardware queues (default 4); kernels of streams that share a queue
// run one after another.  The concurrent budget sweep keeps up to 12 single-CU solves in flight (machip_fw_sweep, one stream per
// lane): on 4 shared queues it saturates at ~2.8x, with a queue per lane at 5-7x (intel 1 764 -> 4 155 it/s).  Round 3 raised
// the process-wide variable when the library was loaded -- a side effect on every other HIP user of the process, and silently
// ineffective once HIP was initialised.  Round 4: a lane's stream is created WITH A CU MASK (all CUs enabled): the runtime
// gives a CU-masked stream a hardware queue of its own (the mask is a property of the queue) instead of one from the shared
// pool -- per stream, no environment, no effect on anybody else.  MACHIP_LANE_QUEUES=shared takes plain streams.
inline int create_lane_stream(const Options& opt, int device, hipStream_t* out) {
    if (OPT(lane_queues, 0) == 0) {      // 0: CU-masked stream with a hardware queue of its own; 1: plain stream on the shared pool
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) {
            const int words = (prop.multiProcessorCount + 31) / 32;
            std::vector<uint32_t> mask((size_t)words, 0xffffffffu);
            if (prop.multiProcessorCount % 32) mask.back() = (1u << (prop.multiProcessorCount % 32)) - 1u;
            if (hipExtStreamCreateWithCUMask(out, (uint32_t)words, mask.data()) == hipSuccess) return MACHIP_OK;
            (void)hipGetLastError();     // (no such queue available: a plain stream serves, more slowly)
        }
    }
    HIP_TRY(hipStreamCreateWithFlags(out, hipStreamNonBlocking));
    return MACHIP_OK;
}

inline int make_lane(machip_problem* p, machip_problem** out) {
    machip_problem* q = new machip_problem();
    q->is_lane = true;
    q->device = p->device; q->n = p->n; q->m = p->m; q->m_pad = p->m; q->tol_sel = p->tol_sel;
    q->prow = p->prow; q->pcol = p->pcol; q->pk = p->pk; q->pw = p->pw; q->P = p->P;
    q->asm_G = p->asm_G; q->asm_rpb = p->asm_rpb; q->asm_grid = p->asm_grid;
    q->ci = p->ci; q->cj = p->cj; q->cw = p->cw;
    auto body = [&]() -> int {
        ST_TRY(create_lane_stream(p->sol.opt, q->device, &q->stream));
        ST_TRY(dev_alloc(&q->x, (size_t)q->m + 64));
        ST_TRY(alloc_assembly(q));
        // every lane keeps its own Krylov basis: a share of the handle's budget each (MACHIP_LANE_VBUDGET_MB, default
        // MACHIP_VBUDGET_MB / 8 = 512 MB: 16 lanes together hold twice what the handle itself holds; a sequence longer than
        // the lane's share restarts earlier than it would on the handle -- include/machip.h states the guarantee accordingly)
        const Options& opt = p->sol.opt;
        q->sol.opt = opt;                     // a lane runs on its owner's options
        ST_TRY(alloc_common(q, std::max(16, OPT(lane_vbudget_mb, std::max(16, OPT(vbudget_mb, 4096) / 8)))));
        q->sol.pat = q->pattern();
        q->sol.pan_allowed = p->sol.pan_allowed;
        q->sol.chain_like = p->sol.chain_like; q->sol.chain_edges = p->sol.chain_edges;
        return MACHIP_OK;
    };
    const int st = body();
    if (st != MACHIP_OK) { destroy_handle(q); return st; }
    *out = q;
    return MACHIP_OK;
}

// FW state of a lane (gradient, LP vertex, next iterate, select scratch): only the sweep needs it
inline int ensure_lane_fw(machip_problem* q) {
    if (q->lane_fw_ready) return MACHIP_OK;
    const size_t mp = (size_t)q->m + 64 * 8;
    ST_TRY(alloc_fw(q)); ST_TRY(alloc_fw_select(q));
    HIP_TRY(hipMemsetAsync(q->g, 0, sizeof(double) * mp, q->stream));     // (never the legacy stream: another lane's thread may be capturing a graph)
    HIP_TRY(hipStreamSynchronize(q->stream));
    q->lane_fw_ready = true;
    return MACHIP_OK;
}

// Lanes [0, *nl_out) of the handle, created on demand, on the handle's solver mode / precision / start vector.
inline int prepare_lanes(machip_problem* p, int B, bool fw, int* nl_out) {
    // Lanes: 16 where a solve is the single-workgroup kernel (one CU each; every lane's stream has a hardware queue of its own,
    // see create_lane_stream at the top of this file), 4 where the solves launch chip-filling step kernels -- more than
    // four hardware queues of those at once collapse (city10000 sweep: 647 it/s with 4 lanes, 277 with 8, 240 with 12).
    const bool small = p->sol.chain_like && persist_fits(p->n, std::max(0l, (long)p->P - 2 * p->sol.chain_edges));   // (P: off-diagonal slots of the union pattern)
    const Options& opt = p->sol.opt;
    // Round 5 (profiles/r5_bench_c4s.json, r5_bench_c2s.json): problems whose every step fills the chip for 7-17 us (ER sizes: union
    // pattern beyond ~400 000 slots) gain from ONE more problem in flight -- 2 lanes 1.27x (configs[3]) / 1.48x (configs[1]) the
    // one-at-a-time rate, 4 lanes 1.03x / 0.95x: two problems already cover each other's launch gaps, more only thrash the L2s.
    // Later in round 5 (tools/r5_eager3.sh): that was the captured chunks -- a lane's hipGraph executables take hardware queues away from
    // the other lanes.  Lanes launch eagerly now (Solver::use_graph) and 4 lanes win at the ER sizes too: configs[3] 267 (2 lanes) ->
    // 293 it/s (4), configs[1] 943 -> 1 180.  Beyond 4 lanes the queues are shared whatever the launch form (city10000 sweep: 1 099 it/s
    // with 4 lanes, 733 with 8, 474 with 12).
    int nl = std::max(1, std::min(B, std::min(16, OPT(lanes, small ? 16 : 4))));
    while ((int)p->lanes.size() < nl) {
        machip_problem* q = nullptr;
        const int st = make_lane(p, &q);
        if (st != MACHIP_OK) {
            // out of device memory for another lane: carry on with the lanes there are (the batch then takes longer, it
            // does not fail); without any lane the error stands
            if (p->lanes.empty()) return st;
            (void)hipGetLastError();
            nl = (int)p->lanes.size();
            break;
        }
        p->lanes.push_back(q);
    }
    HIP_TRY(hipStreamSynchronize(p->stream));
    for (int l = 0; l < nl; ++l) {
        machip_problem* q = p->lanes[(size_t)l];
        q->sol.solver_mode = p->sol.solver_mode; q->sol.precision = p->sol.precision;
        q->sol.opt = p->sol.opt;
        q->sol.throughput_lane = true;
        if (p->sol.have_start && q->seen_start_version != p->start_version) {     // per lane: a batch may use fewer lanes than exist
            HIP_TRY(hipMemcpyAsync(q->sol.start, p->sol.start, sizeof(double) * (size_t)p->n, hipMemcpyDeviceToDevice, q->stream));
            HIP_TRY(hipStreamSynchronize(q->stream));
            q->sol.have_start = true;
            q->seen_start_version = p->start_version;
        }
    }
    if (fw) for (int l = 0; l < nl; ++l) ST_TRY(ensure_lane_fw(p->lanes[(size_t)l]));
    *nl_out = nl;
    return MACHIP_OK;
}

// The worker pool of a batch of B entries on lanes [0, nl): one host thread per lane (lane 0 on the caller's), each on the lane's
// device, taking the next entry off one ticket counter until none is left.  body(q, b) runs entry b on lane q and returns its
// status; a hard status stops that lane, and the first lane that stopped so is the batch's error.
template <class Body>
int run_on_lanes(machip_problem* p, int nl, int B, Body&& body) {
    std::atomic<int> next{0};
    std::vector<int> lane_status((size_t)nl, MACHIP_OK);
    std::vector<std::string> lane_err((size_t)nl);
    auto work = [&](int l) {
        machip_problem* q = p->lanes[(size_t)l];
        if (hipSetDevice(q->device) != hipSuccess) { lane_status[(size_t)l] = MACHIP_HIP_ERROR; lane_err[(size_t)l] = "hipSetDevice failed"; return; }
        for (int b = next.fetch_add(1); b < B; b = next.fetch_add(1)) {
            const int st = body(q, b);
            if (!completed(st)) {
                lane_status[(size_t)l] = st; lane_err[(size_t)l] = g_err;     // hard failure: stop this lane
                return;
            }
        }
    };
    std::vector<std::thread> th;
    for (int l = 1; l < nl; ++l) th.emplace_back(work, l);
    work(0);
    for (auto& t : th) t.join();
    for (int l = 0; l < nl; ++l)
        if (lane_status[(size_t)l] != MACHIP_OK) return fail((machip_status)lane_status[(size_t)l], lane_err[(size_t)l]);
    return MACHIP_OK;
}

// machip_eval_batch after its argument check, on the handle's device
inline int eval_batch(machip_problem* p, int B, const double* X, double tol, int max_steps, double* lambda2, int* status) {
    int nl = 0;
    ST_TRY(prepare_lanes(p, B, false, &nl));
    return run_on_lanes(p, nl, B, [&](machip_problem* q, int b) {
        int st = MACHIP_OK;
        double lam = 0.0;
        if (hipMemcpyAsync(q->x, X + (size_t)b * (size_t)q->m, sizeof(double) * (size_t)q->m, hipMemcpyHostToDevice, q->stream) != hipSuccess ||
            hipStreamSynchronize(q->stream) != hipSuccess) {
            st = fail(MACHIP_HIP_ERROR, "machip_eval_batch: copy of x failed");
        } else {
            q->assembled = false; q->xb_valid = false;
            st = assemble(q);
            // clean solver state per entry (no step-count history from whatever this lane solved before: the automatic
            // mode choice reads it): an entry's result does not depend on the lane that takes it or on its place in the batch
            q->sol.forget_history();
            if (st == MACHIP_OK) st = run_fiedler(q, tol, max_steps, nullptr, 0, &lam, nullptr);
        }
        lambda2[b] = lam;
        if (status) status[b] = st;
        return st;
    });
}

// machip_fw_sweep after its argument checks, on the handle's device
inline int fw_sweep(machip_problem* p, int B, const int64_t* ks, const double* X0, int max_iters, double gap_tol, double grad_tol,
                    double tol, int max_steps, int warm_start, int round_decimals, double* X_out, double* R_out, double* upper,
                    double* f_traj, int* iters, int* status) {
    int nl = 0;
    ST_TRY(prepare_lanes(p, B, true, &nl));
    const size_t m = (size_t)p->m;
    return run_on_lanes(p, nl, B, [&](machip_problem* q, int b) {
        // every problem starts from a clean solver state: its result does not depend on which lane takes it or on
        // what that lane solved before (= a fresh handle running the reference's loop, frankwolfe.py:53-76)
        q->sol.forget_history();
        int st = machip_set_x(q, X0 + (size_t)b * m);
        upper[b] = std::numeric_limits<double>::infinity();
        iters[b] = 0;
        if (st == MACHIP_OK)
            st = fw_loop(q, ks[b], 0, max_iters, gap_tol, grad_tol, tol, max_steps, warm_start, nullptr, &upper[b], &iters[b],
                         [&](int i, double f, double, double, const machip_solve_stats*) {
                             if (f_traj) f_traj[(size_t)b * (size_t)max_iters + (size_t)i] = f;
                         });
        if (st == MACHIP_OK) st = machip_get_x(q, X_out + (size_t)b * m);
        if (st == MACHIP_OK && R_out) st = round_nearest(q, ks[b], round_decimals, R_out + (size_t)b * m);
        status[b] = st;
        return st;
    });
}

}  // namespace machip
