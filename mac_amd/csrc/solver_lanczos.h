// solver_lanczos.h -- the Lanczos driver: cold-start weighting, one chunk of steps in each step form (fused gather / padded / panel,
// two-kernel, single-workgroup), and solve_lanczos in its phases -- start vector, route planning, one Krylov sequence after the
// other (read step by step through streamed records, or chunk by chunk), the restart policy, the finish.  Members of Solver
// (solver.h); what a sequence's records mean is follow.h's business.
#pragma once
#include "solver.h"

namespace machip {

struct LanPending { int jend; hipEvent_t ev; int jstart; bool classic; int tailless; };   // tailless: step count of a chunk without tail kernel (0: it had one)

// What the phases of one solve_lanczos call share.
struct LanRun {
    const CsrView& A;
    long nnz;
    double lnorm, tol;
    int max_steps;
    double tiny_l;              // ||L||_inf, 1 when unknown
    bool debug;
    SpmvPlan pl, pp;            // explicit check / fused Lanczos-step kernel
    PipeView L;
    bool classic = false, pmode = false, f32_seq = false;   // the step form the next sequence takes
    bool warm = false, warm_probe = false, land_ok = false;
    const double* begin_src = nullptr;     // single-workgroup form: what k_persist_begin of the first sequence copies
    double start_overlap = -1.0;
    int chunk0 = 0, chunk_near = 0, pchunk0 = 0, jcap = 0;
    double trigger_slack = 0.0, near_factor = 0.0, f32_switch = 0.0;
    long steps_total = 0, spmv_total = 0, restarts = 0, steps_lowp = 0;
    long steps_used = 0;        // steps up to the analysis point each sequence ended at (a function of the records alone; steps_total counts launches)
    double step_ms_acc = 0.0;   // stream time of the Krylov chunks alone (step kernels + one tail kernel per chunk)
    long steps_timed_acc = 0;
    int status = MACHIP_NOT_CONVERGED;
    bool switch_out = false;    // handed over to the exact mode (solve(): switch_est_us)
    double lam = 0.0, res = 0.0;
    LanRun(const CsrView& A_, long nnz_, double lnorm_, double tol_, int max_steps_, bool debug_)
        : A(A_), nnz(nnz_), lnorm(lnorm_), tol(tol_), max_steps(max_steps_), tiny_l(lnorm_ > 0 ? lnorm_ : 1.0), debug(debug_) {}
};

// One Krylov sequence of it.
struct LanSeq {
    Follower F;                 // (follow.h: the records, the Ritz pair, the estimate; streamed records: the analysis points, the forecast)
    double seq_tol = 0.0;       // what this sequence's residual estimate aims for
    double ltarget = 0.0;
    bool stream_mode = false, feed_chunks = false, tail_ok = false;
    int J_enq = 0;              // steps enqueued in this sequence
    int J_timed = 0;            // ... of which already accounted in step_ms
    int prev_tailless = 0;      // step count of the last enqueued chunk if its records still wait for a successor's first step
    double last_check_est = 1e300, est_latest = 1e300;
    bool converged = false, need_restart = false;
    // convergence-rate tracking: (J, ln est) over a >= 64-step window predicts the steps still
    // needed, which sizes the chunks and the speculation depth (stiff chain-like graphs spend
    // thousands of steps within 1e3 of the target; random graphs a few dozen)
    std::deque<std::pair<int, double>> hist;
    double to_go = 1e18;
    int switch_votes = 0;
    std::deque<LanPending> pend;
    // streamed records
    int prog = -1;              // records up to beta_prog (alpha, l1 up to prog - 1) have landed
    int amp_at = 0;             // shifted recurrence: drift factor accumulated over the steps < amp_at (a function of the records)
    double amp = 1.0;
    int tail_at = -1;           // a tail kernel has been enqueued behind step tail_at - 1 (delivers beta_tail_at)
    int last_chunk = 0;         // steps of the last enqueued chunk (what its tail kernel advances by)
    unsigned long spins = 0;
    bool stalled = false;
    double retry_s = 0.0, amp_max = 0.0, step_us = 0.0;
    bool eager = false;
    int look_opt = 0, far_rem = 0;
    LanSeq(const FollowCfg& fc, Solver& s) : F(fc, 0.0, s.ha, s.hb, s.hl1, s.guess, s.sm, s.wk) {}
};

// Cold start: u (the stored start vector or the pseudo-random fill, already in place) is multiplied by (landscape / max)^p after
// `start_land` Jacobi sweeps (kernels.h).  Scratch: wc (diagonal), y_raw / w2 (sweeps), part_c (maxima) -- all idle until the
// first explicit check.  Deterministic (fixed-order maxima), identical on every rank of a partitioned solve.
// the landscape after `sweeps` Jacobi sweeps (in y_raw or w2; per-workgroup maxima of the last sweep in part_c[0 .. pl.grid))
// (*grid_out: how many workgroups left a maximum in part_c -- the CSR product's launch shape, or the panel row kernel's)
inline const double* Solver::landscape_field(const CsrView& A, const SpmvPlan& pl, int sweeps, int* grid_out) {
    k_land_init<<<vgrid(), kBlock, 0, stream>>>(A, wc, y_raw);
    double *src = y_raw, *dst = w2;
    const bool via_panel = pan_live && OPT(panel_ops, 1) != 0;
    for (int s = 0; s < sweeps; ++s) {
        OpLand op{src, dst, wc, part_c, 0.0};
        if (via_panel) panel_spmv(src, op, vgrid());
        else launch_spmv(pl, stream, A, src, op);
        std::swap(src, dst);
    }
    if (grid_out) *grid_out = via_panel ? vgrid() : pl.grid;
    return src;
}
inline int Solver::landscape_start(const CsrView& A, const SpmvPlan& pl) {
    const int sweeps = std::min(16, OPT(start_land, 3));
    if (sweeps <= 0) return MACHIP_OK;
    const double pw = (double)std::max(1, OPT(start_pow, 128));
    int gmax = pl.grid;
    const double* f = landscape_field(A, pl, sweeps, &gmax);
    const double floor_w = 1e-6 * (double)std::max(0, OPT(start_floor_e6, 1000));      // (every entry keeps this share of its draw: kernels.h)
    k_land_weight<<<vgrid(), kBlock, 0, stream>>>(f, part_c, gmax, u, n, pw, floor_w);
    HIP_TRY(hipGetLastError());
    return MACHIP_OK;
}

// Classic Lanczos chunk: per step one SpMV kernel (v_j = (u - mean)/||u|| with the norm taken
// from the vector itself, w = L v_j, alpha partials) and one update kernel (u <- w - alpha v_j
// - beta v_{j-1}).  Twice the launches of the pipelined form, but beta_j is computed from u_j
// directly, so it stays accurate when ||u_j|| << ||L v_j|| (restart from a good vector, Krylov
// space nearly exhausted), where the pipelined quadratic form has lost its digits.
inline void Solver::enqueue_classic(const CsrView& A, const SpmvPlan& pl, int steps) {
    OpLanczos op;
    op.L = classic_view(pl);
    const int g2 = vgrid();
    for (int s = 0; s < steps; ++s) {
        launch_spmv(pl, stream, A, op.L.u, op);
        k_lan_update<<<g2, kBlock, 0, stream>>>(op.L);
    }
    k_lan_tail<<<1, kBlock, 0, stream>>>(op.L);
}

// ---- small graphs: a whole chunk of Lanczos steps in one single-workgroup launch (persist.h) ----
// Build the packed form of A for this solve (one single-workgroup launch; the chunks then start from coalesced loads).
inline int Solver::pack_persist(const CsrView& A) {
    if (!ppack.band) {
        ST_TRY(dev_alloc(&ppack.band, 5 * (size_t)kPersistPad)); ST_TRY(dev_alloc(&ppack.cc, 2 * (size_t)kPersistPad));
        ST_TRY(dev_alloc(&ppack.crow, (size_t)kPersistPad + 1));
        ST_TRY(dev_alloc(&ppack.ccol, kPersistPackEntries)); ST_TRY(dev_alloc(&ppack.cval, kPersistPackEntries));
    }
    k_persist_pack<<<1, 1024, 0, stream>>>(A, ppack);
    HIP_TRY(hipGetLastError());
    return MACHIP_OK;
}
template <typename T>
inline void Solver::launch_persist_t(const CsrView& A, int steps) {
    const PersistViewT<T> L = persist_view<T>();
    switch ((n + kPersistThreads - 1) / kPersistThreads) {   // rows per thread (sphere2500: 5 -- every row slot costs LDS reads in every step)
        case 1: case 2: k_lan_persist<2, T><<<1, kPersistThreads, 0, stream>>>(ppack, L, steps); break;
        case 3: k_lan_persist<3, T><<<1, kPersistThreads, 0, stream>>>(ppack, L, steps); break;
        case 4: k_lan_persist<4, T><<<1, kPersistThreads, 0, stream>>>(ppack, L, steps); break;
        case 5: k_lan_persist<5, T><<<1, kPersistThreads, 0, stream>>>(ppack, L, steps); break;
        default: k_lan_persist<6, T><<<1, kPersistThreads, 0, stream>>>(ppack, L, steps); break;
    }
}
inline void Solver::launch_persist(const CsrView& A, int steps, bool f32) {
    if (f32) launch_persist_t<float>(A, steps); else launch_persist_t<double>(A, steps);
}

// ---- one chunk = `steps` step kernels + the tail kernel ------------------------------------
// tailless: no tail kernel -- the chunk's last step advances the counters and the NEXT chunk's first step (pub = this chunk's
// step count there) hands the records to the host; a chunk that turns out to have no successor gets its tail from flush_tail.
// j0 >= 0: the sequence's step index of the chunk's first step, known to the host (eager launches only: a captured chunk is replayed at any base)
inline void Solver::launch_chunk(const CsrView& A, const SpmvPlan& pl, int steps, bool f32, bool tailless, int pub, int j0) {
    if (pl.variant == kPanel && seq_ipc) { launch_chunk_ipc_pan(pl, steps, j0); return; }
    if (pl.variant == kPanel) {
        PipeView L = pview(pl);
        L.chunk = tailless ? steps : 0; L.pub = std::max(pub, 0); L.pubstep = pub < 0;
        for (int s = 0; s < steps; ++s) launch_pan_step(L, s, j0 >= 0 ? j0 + s : -1);
        if (!tailless) k_pipe_tail<<<1, 64, 0, stream>>>(L, steps);
        return;
    }
    if (shard && pl.variant == kVec && !f32) { launch_chunk_sharded(pl, steps); return; }
    if (seq_ipc && pl.variant == kVec && !f32) { launch_chunk_ipc(A, pl, steps); return; }
    if (f32) {
        PipeViewT<float> L = pview<float>(pl);
        L.chunk = tailless ? steps : 0; L.pub = std::max(pub, 0); L.pubstep = pub < 0;
        const CsrViewT<float> Af{A.n, A.rowptr, A.col, valf};
        for (int s = 0; s < steps; ++s) launch_pipe(pl, stream, Af, L, s);
        if (!tailless) k_pipe_tail<<<1, 64, 0, stream>>>(L, steps);
        return;
    }
    PipeView L = pview(pl);
    L.chunk = tailless ? steps : 0; L.pub = std::max(pub, 0); L.pubstep = pub < 0;
    const CsrView& As = pl.variant == kEll ? ell_view : A;
    for (int s = 0; s < steps; ++s) launch_pipe(pl, stream, As, L, s);
    if (!tailless) k_pipe_tail<<<1, 64, 0, stream>>>(L, steps);
}
inline void Solver::flush_tail(const SpmvPlan& pl, int steps, bool f32) {
    if (f32) k_pipe_tail<<<1, 64, 0, stream>>>(pview<float>(pl), steps);
    else k_pipe_tail<<<1, 64, 0, stream>>>(pview(pl), steps);
}
inline int Solver::enqueue_chunk(const CsrView& A, const SpmvPlan& pl, int steps, bool f32, bool tailless, int pub, int j0) {
    const bool sharded = shard && pl.variant == kVec && !f32;
    // row-partitioned chunks are launched eagerly: a captured chunk would be one graph of steps x ranks kernel nodes with
    // ranks - 1 cross-stream dependencies each (ROCm 7.2 crashes on it from 8 ranks on one device), and across devices
    // a single graph is not an option anyway
    if (!use_graph(cur_launch_us) || sharded) { launch_chunk(A, pl, steps, f32, tailless, pub, j0); HIP_TRY(hipGetLastError()); return MACHIP_OK; }
    const GraphKey key = std::make_tuple(pl.variant + (f32 ? 100 : 0) + 1000 * pl.defer + (sharded ? 100000 * (int)shard->rk.size() : 0) + (seq_ipc && pl.variant == kVec && !f32 ? 10000000 : 0), pl.width * 10 + pl.unroll, pl.grid, pl.block, steps + 1000 * (tailless ? 1 : 0) + 10000 * pub);
    // (captured without j0: a captured chunk is replayed at any base, and the one consumer of the step index -- the mixed panel mode,
    // launch_pan_step -- is launched eagerly only: lan_plan_route turns it on under eager launches alone)
    return replay_chunk(A, key, [&] { launch_chunk(A, pl, steps, f32, tailless, pub); });
}

inline int Solver::get_event(hipEvent_t* e) {
    if (!ev_pool.empty()) { *e = ev_pool.back(); ev_pool.pop_back(); return MACHIP_OK; }
    HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return MACHIP_OK;
}
// zero-copy records: poison every slot a chunk of steps [j0, hi) delivers for the first time
inline void Solver::poison_records(int j0, int hi) {
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    for (int j = j0 ? j0 + 1 : 0; j <= hi; ++j) h_tri[3 * (size_t)j + 1] = qnan;        // beta_j
    for (int j = j0; j < hi; ++j) { h_tri[3 * (size_t)j] = qnan; h_tri[3 * (size_t)j + 2] = qnan; }   // alpha_j, l1_j
}
inline bool Solver::record_landed(int j) const {
    const volatile double* t3 = h_tri;
    if (t3[3 * (size_t)j + 1] != t3[3 * (size_t)j + 1]) return false;
    if (j > 0 && (t3[3 * (size_t)(j - 1)] != t3[3 * (size_t)(j - 1)] || t3[3 * (size_t)(j - 1) + 2] != t3[3 * (size_t)(j - 1) + 2])) return false;
    return true;
}

// ---- the phases of solve_lanczos, in the order they run ----------------------------------------

// start vector: warm start, the caller's / the stored vector, the pseudo-random fill; whether a cold start gets the landscape weighting
inline int Solver::lan_start_vector(LanRun& R, int start_mode) {
    // (single-workgroup form: k_persist_begin of the first sequence copies it -- one launch less per solve)
    // LDS-resident single-workgroup form when the matrix fits (classic recurrence: also fine after restarts)
    R.pmode = OPT(persist, 1) != 0 && chain_like && persist_fits(n, R.nnz - n - 2 * chain_edges);
    // The landscape weighting moves the start to where low eigenvectors LOCALISE; it pays where they do (the Erdos-Renyi iterates:
    // participation ratio 1-5 vertices, -15 % steps) and costs its sweeps where the Fiedler vector is global (city10000: thousands of
    // vertices, 297 against 300 it/s in round 5).  Gate, round 6: what the LAST pair this handle checked looked like -- skipped when it lived on
    // more than start_land_pr_permille of the vertices (default 2 %); a handle's first solve has nothing to go by and weights.
    // A handle's FIRST solve is gated on the matrix alone: the weighting is for random-graph-like Laplacians (from ~6 entries per row), not for
    // pose graphs (3-5 entries per row: chain + a few closures), where it never paid (+-1 %) and where a floored, half-localised start flattens
    // the residual estimate's decay enough to fool the step forecast (city10000: a hand-over to the tridiagonally preconditioned mode, 26 ms
    // per iteration instead of 3.3 -- tools/floor_probe.py).
    const bool land_local = last_pr <= 0.0 || last_pr <= 0.001 * (double)std::max(1, OPT(start_land_pr_permille, 20)) * (double)n;
    const bool land_dense = 10.0 * (double)R.nnz >= (double)std::max(0, OPT(start_land_min_mean10, 60)) * (double)n;
    // (the multi-workgroup recurrence only -- a single-workgroup solve costs less than the sweeps would --, never a caller's own guess or a warm start)
    R.land_ok = !start_guess && !R.pmode && n > OPT(classic_n, 256) && OPT(start_land, 3) > 0 && land_local && land_dense;
    R.warm = start_mode == 1 && have_prev;
    if (R.warm && R.land_ok && warm_skip > 0) { --warm_skip; R.warm = false; }      // (the last warm start was no better than a random vector)
    R.warm_probe = R.warm && R.land_ok;      // this solve measures what its warm start was worth
    if (R.warm) {
        if (R.pmode) R.begin_src = yvec;
        else HIP_TRY(hipMemcpyAsync(u, yvec, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
    } else if (have_start) {
        if (R.pmode) R.begin_src = start;
        else HIP_TRY(hipMemcpyAsync(u, start, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
    } else {
        k_fill_start<<<vgrid(), kBlock, 0, stream>>>(u, n, 0x1234567ull);
    }
    // ---- landscape weighting of a cold start (kernels.h, k_land_*) ----
    pan_live = false;       // (the landscape sweeps run further down, once the panel form -- if this solve takes it -- is built: they can use it)
    return MACHIP_OK;
}

// route planning: chunk sizes, the step form (two-kernel, single-workgroup, panel, padded, gather), the mixed modes' buffers, the
// landscape weighting on the form just built, the launch-time model
inline int Solver::lan_plan_route(LanRun& R) {
    const CsrView& A = R.A;
    const long nnz = R.nnz;
    SpmvPlan& pp = R.pp;
    R.chunk0 = std::min(kMaxChunk, std::max(2, OPT(chunk, 32) & ~1));   // even: Z parity = jrel & 1
    R.chunk_near = std::min(R.chunk0, std::max(2, OPT(chunk_near, 8) & ~1));   // once the residual estimate is within 1e3 of the target
    if (R.max_steps & 1) ++R.max_steps;
    // An explicit check runs when the recurrence's own estimate of the residual is within this factor of the tolerance.  The estimate
    // predicts the measured residual to +/- 5 % (profiles/r5_c4_checks.txt), so round 1-4's factor of 1.5 bought nothing: every check
    // started between 1.1 and 1.5 x the tolerance failed (0.3 per solve at configs[3], ~100 us each: Ritz vector, product, wait) and
    // the solve went on to the same final step anyway.
    R.trigger_slack = 0.01 * OPT(trigger_pct, 110);
    R.near_factor = 0.1 * OPT(near_x10, 20);   // end game (no speculation, short chunks) from this many chunks of predicted steps to go
    R.jcap = (int)std::min<size_t>(vcap - 2, (size_t)std::max(2, n - 1) + 8) & ~1;
    R.classic = n <= OPT(classic_n, 256);
    const bool pmode = R.pmode, classic = R.classic;
    // column-panel step (panel.h) where the gather operand is too large for the caches (fp64 sequences only)
    // (shifted recurrence, panel_u.h: only where the host follows the records step by step -- its drift monitor lives there)
    pan = plan_panel(opt, n, nnz, maxlen_hint, pan_allowed && !pmode && !classic && pp.variant == kVec && !shard, (long)csr_cap,
                     false, OPT(stream, 1) != 0);   // (the in-process row-partitioned solve shards the gather step)
    pan_u = false; last_amp = 0.0; pan32 = false; pan32_from = INT_MAX;
    // between processes (round 6): the shifted recurrence partitions by the row kernel's workgroups (launch_chunk_ipc_pan) where one wave of
    // them covers every row; the record form and the multi-cell shapes are not partitioned
    if (ipc && !(pan.on && pan.u && precision == 0 && (long)pan.grid2 * pan.block2 >= (long)n && pan.grid2 >= ipc->nranks && OPT(ipc_panel, 1) != 0)) pan.on = false;
    // mixed mode: only the shifted recurrence in a shape whose fp32-tile kernel exists, launched eagerly (the step index decides which tiles
    // a launch reads); anything else keeps round 2's fp32 gather sequences
    if (precision == 1 && !(pan.on && pan.u && pan.TWT == 3 && OPT(pan32, 1) != 0)) pan.on = false;
    // padded fixed-width form for short rows (pose graphs beyond the single-workgroup kernel): no row-pointer round trip
    if (!pan.on && !pmode && !classic && !shard && !ipc && precision == 0 && pp.variant == kVec && pp.width == 4 && pp.defer < 3 &&
        maxlen_hint >= 1 && maxlen_hint <= 16 && OPT(ell, 1) != 0) {
        const int W = maxlen_hint <= 8 ? 8 : 16;
        if (!ell_col) { ST_TRY(dev_alloc(&ell_col, (size_t)n * 16)); ST_TRY(dev_alloc(&ell_val, (size_t)n * 16)); }
        k_ell_build<<<(int)std::min<long>(kMaxGrid, ((long)n * W + kBlock - 1) / kBlock), kBlock, 0, stream>>>(A, W, ell_col, ell_val);
        HIP_TRY(hipGetLastError());
        ell_view = CsrView{n, nullptr, ell_col, ell_val};
        pp.variant = kEll; pp.unroll = W / 4;
    }
    if (pan.on) {
        const bool rows_ready = pan_rows_ready && !pan.verify && pan_rows_NP == pan.NP && pan_rows_C == pan.C && pan_rows_band == pan.band;
        ST_TRY(ensure_panel(A, nnz, pan, pan.band, rows_ready));
        if (pan.verify) {        // hub rows: is every (row, panel) count within what the tiles describe?  (one sync, hub matrices only)
            int over = 0;
            HIP_TRY(hipMemcpyAsync(&over, panv.ovf, sizeof(int), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (over) pan.on = false;            // a hub row concentrated in one panel: the gather step serves this matrix
        }
    }
    if (pan.on) {
        pp.variant = kPanel; pp.grid = pan.grid2; pp.block = pan.block2;   // (grid = partial sums per quantity)
        pp.width = pan.NP * 100 + pan.RPT; pp.unroll = pan.TWW; pp.defer = pan.NB + 10000 * pan.cells + (pan.u ? 1000000 : 0);
        if (pan.u) {
            if (!pu_U0) {
                ST_TRY(dev_alloc(&pu_U0, (size_t)n + 2)); ST_TRY(dev_alloc(&pu_U1, (size_t)n + 2)); ST_TRY(dev_alloc(&pu.W, (size_t)n));
                ST_TRY(dev_alloc(&pu_sig, 2));
                pu.sig = pu_sig;
            }
            // (inter-process communicator: the operand lives in the record buffers -- 16 n bytes each, idle in this form -- which the peers
            // have mapped already: the row kernel writes its rows of the next operand into every rank's copy)
            pu.U0 = ipc ? reinterpret_cast<double*>(Z0) : pu_U0;
            pu.U1 = ipc ? reinterpret_cast<double*>(Z1) : pu_U1;
            pan_u = true;
            if (precision == 1 && !use_graph(launch_us_hist[kPanel] > 0.0 ? launch_us_hist[kPanel] : 8.0)) {
                if (pan_bv32_cap < pan_cap) {
                    HIP_TRY(hipStreamSynchronize(stream));
                    if (pan_bv32) (void)hipFree(pan_bv32);
                    pan_bv32 = nullptr; pan_bv32_cap = 0;
                    ST_TRY(dev_alloc(&pan_bv32, pan_cap));
                    pan_bv32_cap = pan_cap;
                }
                k_to_f32<<<(int)std::min<long>(kMaxGrid, ((long)pan_cap + kBlock - 1) / kBlock), kBlock, 0, stream>>>(panv.bval, pan_bv32, (long)pan_cap);
                pan32 = true;
            }
        }
    }
    pan_live = pan.on && pan_u;
    if (!R.warm && R.land_ok) ST_TRY(landscape_start(A, landscape_plan(nnz)));
    {   // eager launches or captured chunks for this solve's fused steps (use_graph)
        const int vk = std::max(0, std::min(7, (int)pp.variant));
        // (model before the first measurement: the gather step's; a panel launch never runs under ~8 us -- n >= 65 536.  A first solve must not
        // capture by mistake: on a handle with evaluation lanes, hipGraph executables take hardware queues away from the lanes'
        // streams for good -- c4s with 4 lanes 294 -> 231 it/s after ONE captured solve per lane, tools/r5_eager3.sh)
        cur_launch_us = launch_us_hist[vk] > 0.0 ? launch_us_hist[vk] : (pp.variant == kPanel ? 8.0 : 4.2 + 2e-6 * (double)nnz);
    }
    if (OPT(debug, 0)) fprintf(stderr, "[machip] fused steps: variant %d, %.2f us per launch (%s) -> %s\n", (int)pp.variant, cur_launch_us, launch_us_hist[std::max(0, std::min(7, (int)pp.variant))] > 0.0 ? "measured" : "model", use_graph(cur_launch_us) ? "captured chunks" : "eager launches");
    R.L = pview(pp);
    R.pchunk0 = std::min(kPersistMaxSteps, std::max(2, OPT(pchunk, 64)));
    // ---- mixed precision (machip_set_precision(1)): the FIRST Krylov sequence stores matrix values, records and
    // basis in fp32 (inner products accumulated in fp64).  An fp32 recurrence cannot resolve lambda_2 beyond
    // ~eps_32 ||L||, so it only runs until its residual estimate reaches f32_switch ||L||_inf (or stalls); its Ritz
    // vector is then formed with fp64 accumulation, checked in fp64 (Rayleigh quotient + the reference's residual
    // test on the fp64 matrix) and, when the test does not pass yet, fp64 sequences continue from it. ----
    R.f32_seq = precision == 1 && !classic && pp.variant == kVec;
    // (measured floor of the fp32 recurrence's TRUE residual: 8e-7 at config 2 (||L|| = 50, n = 1e4), 1e-6 on
    // sphere2500, 2e-4 on city10000 (||L|| = 1600, stiff) while its own estimate keeps falling: beyond
    // ~eps_32 sqrt(n) x 10 the fp32 steps buy nothing)
    R.f32_switch = std::max(std::max(R.tol, 1e-9 * (double)OPT(f32_switch_e9, 2000)),
                            3e-7 * std::sqrt((double)n));
    if (R.f32_seq && !pmode) {
        if (valf_cap < (size_t)nnz) {
            // cached chunk graphs carry the old pointer: drop them together with the buffer
            HIP_TRY(hipStreamSynchronize(stream));
            drop_graphs();
            if (valf) (void)hipFree(valf);
            valf = nullptr; valf_cap = 0;
            const size_t want = std::max<size_t>((size_t)nnz + (size_t)nnz / 2 + 1024, csr_cap);   // csr_cap: the most L(x) can ever hold
            ST_TRY(dev_alloc(&valf, want));
            valf_cap = want;
        }
        k_to_f32<<<(int)std::min<long>(kMaxGrid, (nnz + kBlock - 1) / kBlock), kBlock, 0, stream>>>(A.val, valf, nnz);
    }
    if (pmode) ST_TRY(pack_persist(A));
    return MACHIP_OK;
}

inline FollowCfg Solver::lan_follow_cfg(const LanRun& R) const {
    FollowCfg fc;
    fc.n = n; fc.jcap = R.jcap; fc.chunk0 = R.chunk0; fc.win_max = std::max(8, OPT(stream_window, 64));
    fc.margin = std::max(0, OPT(stream_margin, 0)); fc.tiny_l = R.tiny_l;
    return fc;
}

// ---- (re)start a Krylov sequence from u: the first records, whether its steps are row-partitioned, how the host will read it ----
inline int Solver::lan_begin_sequence(LanRun& R, LanSeq& S) {
    const SpmvPlan& pp = R.pp;
    const int g2 = vgrid();
    seq_sharded = false; seq_ipc = false;
    pan32_from = INT_MAX;
    if (R.pmode) {
        ++epoch;
        k_persist_begin<<<g2, kBlock, 0, stream>>>(persist_view(), (int)epoch, R.begin_src);
        R.begin_src = nullptr;            // (restarts continue from u)
    } else if (R.classic) {
        k_vec_sums<<<g2, kBlock, 0, stream>>>(u, n, part_u);
        k_set_state<<<1, 64, 0, stream>>>(stc, 0);
    } else if (R.f32_seq) {
        ++epoch;
        k_pipe_init<<<pp.grid, kBlock, 0, stream>>>(pview<float>(pp), u, (int)epoch);
    } else {
        ++epoch;
        if (pan_u) k_pipe_init_u<<<pp.grid, kBlock, 0, stream>>>(R.L, pu, u, (int)epoch);
        else k_pipe_init<<<pp.grid, kBlock, 0, stream>>>(R.L, u, (int)epoch);
        if (shard && pp.variant == kVec) {       // row-partitioned sequence: every rank starts from the same records
            seq_sharded = true; seq_plan = pp;
            ST_TRY(shard_broadcast_init());
        } else if (ipc && precision == 0 && ((pp.variant == kVec && pp.grid >= ipc->nranks) || (pp.variant == kPanel && pan_u))) {
            // (precision 1: the fp32 sequences run replicated on the very record / partial-sum buffers the peers of a
            // partitioned step write into, and nothing orders a rank that is still in its fp32 phase against a peer that has
            // entered the fp64 one -- the mixed mode therefore never partitions; round-4 advisor finding)
            // between processes every rank has just run k_pipe_init itself on its own copy of u: identical records
            seq_sharded = true; seq_ipc = true; seq_plan = pp;
        }
    }
    S.seq_tol = R.f32_seq ? R.f32_switch : R.tol;
    S.tail_ok = !R.pmode && !R.classic && !seq_sharded && OPT(tailless, 1) != 0;
    HIP_TRY(hipEventRecord(evs0, stream));
    ha.clear(); hb.assign(1, 0.0); hl1.assign(1, 0.0);
    guess.clear();
    S.ltarget = std::log(std::max(S.seq_tol * R.tiny_l, 1e-300));
    // ---- streamed records (round 5): where the solve ends is decided step by step, not chunk by chunk ----
    // Every step hands its (alpha_{j-1}, l1_{j-1}, beta_j) to the host as it derives them (PipeView::pubstep), so the host
    // (a) analyses T_a at a DETERMINISTIC sequence of points a_0 < a_1 < ... -- each next point a function of the analyses
    //     before it only (a third of the forecast distance to the target, at most 32 steps) -- and ends the sequence at the FIRST
    //     point whose residual estimate is below the trigger: the Ritz pair, and with it every later result, is a function
    //     of the records alone, never of timing;
    // (b) feeds the queue from the forecast: far from the end 32-step chunks one chunk ahead, then chunks of about half
    //     the predicted remainder, each enqueued only when the GPU is within `look` steps of running dry, none beyond the
    //     predicted crossing (+ margin), a one-wave tail kernel behind the last.  How many steps run BEYOND the final
    //     analysis point depends on timing; nothing reads them.
    // The chunk-granular loop (lan_chunks) overshoots the crossing by 8.7 steps per solve at configs[3] (3.6 % of 242:
    // tools/sched_probe.sh) and idles the GPU for a host round trip at each of its 2-3 end-game hops.
    // Row-partitioned sequences (every rank has to launch the same steps) and option stream = 2 feed the queue from the analyses
    // alone instead: one chunk with a tail kernel at a time, sized by the forecast once every record of its predecessor has been
    // analysed.  Same points, same rule, same final point: a partitioned solve still reproduces the single-rank one bit for bit.
    S.stream_mode = !R.pmode && !R.classic && !R.f32_seq && OPT(stream, 1) != 0;
    S.feed_chunks = seq_sharded || OPT(stream, 1) == 2 || OPT(tailless, 1) == 0;
    // what ends a sequence: the streamed loop's trigger is a share of ||L|| (1 when unknown), the chunk loop's of lnorm as given
    // (the estimate predicts the measured residual to +/- 5 %: profiles/r5_c4_checks.txt)
    S.F.e_target = S.stream_mode ? 0.01 * OPT(stream_trigger_pct, 95) * S.seq_tol * R.tiny_l : R.trigger_slack * S.seq_tol * R.lnorm;
    return MACHIP_OK;
}

// The hand-over vote (solve(): switch_est_us): the sequence is undecided at point J and its own forecast of the remaining steps
// costs more than 1.3x the exact mode's estimate -- twice in a row.  true: hand over now.
inline bool Solver::lan_vote(LanRun& R, LanSeq& S, int J, bool undecided) {
    if (switch_est_us > 0.0 && R.restarts == 0 && !R.f32_seq && undecided && J >= 128 && S.to_go < 1e17 &&
        S.to_go * (4.2 + 2e-6 * (double)R.nnz) > 1.3 * switch_est_us) {
        if (++S.switch_votes >= 2) {
            if (R.debug) fprintf(stderr, "[machip]    J=%d: forecast %.0f steps to go -- handing over to the exact chain + closures mode (estimate %.0f us)\n", J, S.to_go, switch_est_us);
            switch_to_go = S.to_go; R.switch_out = true;
            return true;
        }
    } else S.switch_votes = 0;
    return false;
}

// The explicit check of the Ritz pair of T_Jeff (sm) and its accounting: the step time up to here, lam, res, whether it passed.
inline int Solver::lan_check(LanRun& R, LanSeq& S, int Jeff, double est) {
    double rq = 0.0, r1 = 0.0;
    HIP_TRY(hipEventRecord(evs1, stream));   // everything enqueued so far = steps [J_timed, J_enq)
    spec_likely = !R.f32_seq && est < 0.01 * OPT(spec_slack_pct, 105) * S.seq_tol * R.lnorm;
    ST_TRY(explicit_check(R.A, R.pl, Jeff, sm.s.data(), &rq, &r1, R.f32_seq));   // syncs the stream: every enqueued step has run
    spec_likely = true;
    {
        float sms = 0.f;
        HIP_TRY(hipEventElapsedTime(&sms, evs0, evs1));
        R.step_ms_acc += sms; R.steps_timed_acc += S.J_enq - S.J_timed;
        S.J_timed = S.J_enq;
        HIP_TRY(hipEventRecord(evs0, stream));
    }
    R.spmv_total += 1;
    J_last = Jeff;
    S.last_check_est = std::max(est, 1e-300);
    R.lam = rq;
    R.res = R.lnorm > 0 ? r1 / R.lnorm : r1;
    S.converged = R.res < R.tol;
    if (S.converged) { R.status = MACHIP_OK; final_check_seq = check_seq; }
    return MACHIP_OK;
}

// ---- the streamed loop: (1) progress, (2) analysis, (3) feed, (4) wait ----
// (2) analysis, as soon as the records of the next point are there -- BEFORE the queue is fed: a host that cannot launch as
// fast as the GPU runs (eager launches under a profiler) would otherwise feed for ever and never look.
// *what: 0 nothing analysed, 1 analysed, 2 the sequence has ended (converged, restart or hand-over)
inline int Solver::lan_stream_analyse(LanRun& R, LanSeq& S, int* what) {
    Follower& F = S.F;
    int& next_a = F.next_a;      // the next analysis point
    int& T = F.T;                // forecast: no step >= T is wanted (INT_MAX: no forecast yet)
    const int jcap = R.jcap, J_enq = S.J_enq;
    *what = 0;
    const int a = std::min(next_a, std::min(J_enq, jcap));       // (J_enq < next_a only at the caps)
    // An analysis at a point SHORT of next_a is for the caps only (nothing more will be enqueued).  While the feeder still has
    // steps to enqueue it must come first: whether the records up to J_enq have landed before or after the loop passes here is
    // timing, and an analysis at J_enq would change every later point -- two ranks of a row-partitioned solve then disagreed
    // about where the sequence ends (2 of 30 two-rank configs[3] runs of round 5's library, 3 of 14 with the panel step:
    // tools/archive/ipc_pan_debug.py prints the first diverging trace line).
    const bool more_coming = J_enq < jcap && R.steps_total < R.max_steps && J_enq < std::max(T, next_a);
    if (!(S.prog >= a && a > 0 && (a == next_a || !more_coming))) return MACHIP_OK;
    *what = 1;
    ST_TRY(ipc_check_err("Lanczos steps"));
    const int J = a;
    if (!F.analyse(h_tri, a)) return fail(MACHIP_BAD_ARG, "start vector is constant, zero or not finite");
    const int Jeff = F.Jeff;
    const bool broke = F.broke;
    const double est = F.est;
    S.est_latest = est; S.to_go = F.to_go;
    // Mixed mode of the panel step: products may be INEXACT late in a Krylov sequence -- an error E_j in step j's product enters the
    // final residual weighted by the Ritz vector's coefficient of v_j, which is ~ the residual at that step (Simoncini 2005 /
    // Bouras & Fraysse: relaxed accuracy of matrix-vector products in projection methods) -- not early.  So the sequence starts on
    // the fp64 tiles and switches to the fp32 copy (6 bytes per entry instead of 10, relative error 6e-8) once the estimate is below
    // pan32_switch_e9 1e-9 ||L||.  Measured on the 20 configs[3] iterates (tools/pan32_probe.py, profiles/r6_pan32.md): 1e-3 passes the
    // explicit check on 19 -- residuals unchanged in the second digit -- and FAILS on the near-degenerate iterate 6 (353 steps:
    // the gap grows with 1 / (1 - convergence rate)), whose restart in the two-kernel form then costs 5 000 steps; 3e-4 (default)
    // passes on all twenty.  The switch step is a function of the records alone: 32 steps behind the analysis point that saw
    // the threshold -- as far as the feeder lets the queue run while undecided.
    if (pan32 && pan32_from == INT_MAX && est < 1e-9 * (double)std::max(1, OPT(pan32_switch_e9, 300000)) * R.tiny_l) {
        pan32_from = (J + 32 + 1) & ~1;       // (the feeder has held the queue at next_a + 32 = J + 32 until now)
        if (R.debug) fprintf(stderr, "[machip]    J=%d: estimate %.2e -- fp32 tile values from step %d on\n", J, est / R.tiny_l, pan32_from);
    }
    bool amp_trip = false;
    if (pan_u && R.pp.variant == kPanel) {
        // w_{k+1} = (L u_k - (alpha_k - alpha_{k-1}) w_k) / beta_{k+1}: what step k multiplies the difference w_k - L v_k by
        for (; S.amp_at < J; ++S.amp_at) {
            const int k = S.amp_at;
            const double ak = h_tri[3 * (size_t)k], akm = k ? h_tri[3 * (size_t)(k - 1)] : 0.0, bk1 = h_tri[3 * (size_t)(k + 1) + 1];
            S.amp = (bk1 > 0.0 ? std::fabs(ak - akm) / bk1 : 0.0) * S.amp + 1.0;
            last_amp = std::max(last_amp, S.amp);
        }
        amp_trip = !(last_amp <= S.amp_max);
        if (amp_trip && R.debug) fprintf(stderr, "[machip]    J=%d: drift factor of the shifted recurrence %.3g > %.3g -- this sequence ends here, the solve continues in the accurate form\n", J, last_amp, S.amp_max);
    }
    const bool at_cap = (J >= jcap) || (R.steps_total >= R.max_steps && J >= J_enq) || amp_trip;
    const bool trig = F.triggered();
    if (lan_vote(R, S, J, !broke && !trig && !at_cap)) { R.steps_used += J; *what = 2; return MACHIP_OK; }
    if (R.debug) fprintf(stderr, "[machip] stream J=%d Jeff=%d theta=%.15g est=%.3e to_go=%.1f T=%d next_a=%d enq=%d prog=%d broke=%d passes=%d\n", J, Jeff, sm.theta, R.lnorm > 0 ? est / R.lnorm : est, std::min(S.to_go, 1e9), T == INT_MAX ? -1 : T, next_a, J_enq, S.prog, (int)broke, sm.passes);
    if (trig || at_cap) {
        if (S.tail_at != J_enq && J_enq > 0 && S.last_chunk > 0) { flush_tail(R.pp, S.last_chunk, false); S.tail_at = J_enq; }    // (a tail-less chunk never ends a sequence: the counters move with its successor)
        ST_TRY(lan_check(R, S, Jeff, est));
        if (R.debug) fprintf(stderr, "[machip]    check J=%d rq=%.15g res=%.3e (tol %.1e) ran=%d\n", Jeff, R.lam, R.res, R.tol, J_enq);
        if (S.converged || broke || at_cap) {
            S.need_restart = !S.converged;
            R.steps_used += Jeff;
            if (pan32 && pan32_from < Jeff) R.steps_lowp += Jeff - pan32_from;      // (steps that read fp32 tile values)
            if (S.converged && R.restarts == 0 && !sm.s.empty()) R.start_overlap = std::fabs(sm.s[0]);     // <v_0, y>: what the start vector was worth
            *what = 2;
            return MACHIP_OK;
        }
        F.lower_target(S.retry_s * S.last_check_est);      // the estimate flattered the residual: further down before the next check
        T = std::max(T, J_enq + 2);
    }
    return MACHIP_OK;
}

// `chunk` more steps behind step J_enq of a streamed sequence: their record slots poisoned, the launch, the counters
inline int Solver::lan_stream_enqueue(LanRun& R, LanSeq& S, int chunk, bool tailless) {
    const int hi = S.J_enq + chunk, T = S.F.T;
    poison_records(S.J_enq, hi);
    ST_TRY(enqueue_chunk(R.A, R.pp, chunk, false, tailless, tailless ? -1 : 0, S.J_enq));
    if (R.debug && !tailless) fprintf(stderr, "[machip] chunk enqueue J=%d chunk=%d T=%d next_a=%d\n", S.J_enq, chunk, T == INT_MAX ? -1 : T, S.F.next_a);
    if (R.debug && tailless) fprintf(stderr, "[machip] stream enqueue J=%d chunk=%d prog=%d T=%d next_a=%d\n", S.J_enq, chunk, S.prog, T == INT_MAX ? -1 : T, S.F.next_a);
    S.J_enq = hi; S.last_chunk = chunk;
    if (!tailless) S.tail_at = hi;
    R.steps_total += chunk; R.spmv_total += chunk;
    return MACHIP_OK;
}

// (3) feed the queue (*fed: something was enqueued -- the loop looks at the records again before anything else)
inline int Solver::lan_stream_feed(LanRun& R, LanSeq& S, bool* fed) {
    const int jcap = R.jcap, chunk0 = R.chunk0, J_enq = S.J_enq, next_a = S.F.next_a, T = S.F.T;
    *fed = true;
    const bool room = J_enq < jcap && R.steps_total < R.max_steps;
    const int want = std::max(T, next_a);      // beta_{next_a} comes from step next_a -- or from a tail kernel when the queue ends exactly there
    if (S.feed_chunks) {
        // (decided in a state that is a function of the records: all of the queue delivered, every point up to there analysed)
        if (room && J_enq < want && S.prog >= J_enq - (J_enq == 0) && next_a > S.prog) {
            const long remaining = (long)want - J_enq;
            // (far: long chunks, a host round trip each; near: a little short of the predicted crossing -- the forecast errs on the long side)
            int chunk = remaining >= 4 * chunk0 ? std::min(kMaxChunk, 2 * chunk0) : remaining >= 2 * chunk0 ? chunk0
                        : remaining >= 12 ? (int)std::min<long>(chunk0, ((long)(0.7 * (double)remaining) + 1) & ~1L) : (int)((remaining + 1) & ~1L);
            chunk = std::min(std::max(chunk, 2), jcap - J_enq);
            chunk = (int)std::min<long>(chunk, R.max_steps - R.steps_total) & ~1;
            if (pan32 && pan32_from == INT_MAX) chunk = std::min(chunk, std::max(0, next_a + 32 - J_enq)) & ~1;
            if (chunk >= 2) return lan_stream_enqueue(R, S, chunk, false);
        }
    } else if (room && J_enq < want) {
        const long remaining = (long)want - J_enq;
        const int ahead = J_enq - std::max(S.prog, 0);
        // (the host must be back before the queue runs dry: a graph launch + one O(J) analysis of the tridiagonal)
        const int look = S.look_opt > 0 ? S.look_opt : std::max(2, std::min(24, (int)(((S.eager ? 28.0 : 36.0) + 0.07 * (double)J_enq) / S.step_us) + 1));
        int chunk = 0;
        if (remaining >= S.far_rem) { if (ahead <= 16 + look) chunk = J_enq >= 4096 ? std::min(kMaxChunk, 2 * chunk0) : chunk0; }
        else if (ahead <= look) {
            chunk = 2;
            // captured chunks: about 0.6 of the remainder, a power of two (few shapes to capture); eager launches have no
            // shapes -- two steps at a time, every decision on the latest forecast
            if (!S.eager) while (2 * chunk <= chunk0 && 5 * (long)(2 * chunk) <= 3 * remaining + 4) chunk *= 2;
        }
        // (mixed panel mode, switch step not decided yet: nothing is enqueued beyond 32 steps behind the next analysis point, so that
        // the point that sees the threshold can still name a switch step nobody has launched -- a function of the records alone)
        if (pan32 && pan32_from == INT_MAX) chunk = std::min(chunk, std::max(0, next_a + 32 - J_enq));
        if (chunk > 0) {
            chunk = std::min(chunk, jcap - J_enq);
            chunk = (int)std::min<long>(chunk, R.max_steps - R.steps_total) & ~1;
            if (chunk >= 2) return lan_stream_enqueue(R, S, chunk, true);
        }
    }
    // nothing more is wanted (or allowed) and the last record needs a tail kernel: beta_{J_enq} comes from the step that follows, or from a tail
    if (!S.feed_chunks && S.tail_at != J_enq && J_enq > 0 && (J_enq >= want || !room) && next_a >= J_enq) {
        flush_tail(R.pp, S.last_chunk, false);
        S.tail_at = J_enq;
        if (R.debug) fprintf(stderr, "[machip] stream tail at J=%d (prog=%d T=%d next_a=%d)\n", J_enq, S.prog, T == INT_MAX ? -1 : T, next_a);
        return MACHIP_OK;
    }
    *fed = false;
    return MACHIP_OK;
}

inline int Solver::lan_stream(LanRun& R, LanSeq& S) {
    S.retry_s = 0.01 * OPT(stream_retry_pct, 80);       // after a failed check: the next one when the estimate has fallen to this fraction
    // time of one step: measured in-solve on this handle's last solve in the same step form, the hand-over forecast's model before
    S.eager = !use_graph(cur_launch_us);
    S.step_us = std::max(1.0, cur_launch_us * (R.pp.variant == kPanel ? 2.0 : 1.0));
    S.look_opt = OPT(stream_look, 0);                      // steps of queued work below which the queue is fed (0: from the step-time model)
    S.far_rem = std::max(34, OPT(stream_far, 80));         // whole chunks one ahead while at least this many steps are predicted to remain
    S.amp_max = (double)std::max(2, OPT(panel_u_amp, 100000));
    for (;;) {
        // (1) how far has the GPU got?
        const int limit = std::min(S.tail_at == S.J_enq ? S.J_enq : S.J_enq - 1, R.jcap);
        while (S.prog < limit && (S.stalled || record_landed(S.prog + 1))) ++S.prog;
        int what = 0;
        ST_TRY(lan_stream_analyse(R, S, &what));
        if (what == 2) return MACHIP_OK;
        bool fed = false;
        ST_TRY(lan_stream_feed(R, S, &fed));
        if (fed) continue;
        // (4) nothing to do: wait for records
        if (what == 0) {
            if ((++S.spins & 0xfffff) == 0) {     // a device fault or a genuine NaN (non-finite input) must not hang the host
                const hipError_t q = hipStreamQuery(stream);
                if (q != hipSuccess && q != hipErrorNotReady)
                    return fail(MACHIP_HIP_ERROR, std::string("stream error while following the Lanczos steps: ") + hipGetErrorString(q));
                if (q == hipSuccess && S.prog < limit && !record_landed(S.prog + 1)) S.stalled = true;        // everything enqueued has run: the slot holds a NaN of the recurrence's own
                ST_TRY(ipc_check_err("Lanczos steps"));
            }
            __builtin_ia32_pause();
        }
    }
}

// ---- the chunk-granular loop (single-workgroup, two-kernel and fp32 sequences; option stream = 0) ----
// keep `depth` chunks in flight
inline int Solver::lan_chunk_feed(LanRun& R, LanSeq& S, bool near, int depth) {
    const bool pmode = R.pmode, classic = R.classic, f32_seq = R.f32_seq, use_classic = classic && !pmode;
    const int chunk0 = R.chunk0;
    const size_t cs = vcap + 2;   // stride of the classic alpha / beta / l1 arrays
    const bool sched = OPT(sched, 1) != 0;
    while ((int)S.pend.size() < depth && S.J_enq < R.jcap && R.steps_total < R.max_steps) {
        // (the O(J) host analysis must keep up with the GPU: longer chunks once J is large -- a function of
        // J only, so the step count at which convergence is noticed stays reproducible)
        int chunk = near ? R.chunk_near : (S.J_enq >= 4096 ? std::min(kMaxChunk, 2 * chunk0) : chunk0);
        if (near && sched && S.to_go < 1e17)   // aim a little short of the predicted crossing
            chunk = std::min(chunk0, std::max(R.chunk_near, ((int)(0.75 * S.to_go) + 1) & ~1));
        if (pmode) {   // steps cost ~0.5 us here: long chunks, so the O(J) host analysis keeps up
            chunk = R.pchunk0;
            if (S.to_go < 1e17) chunk = std::min(R.pchunk0, std::max(16, ((int)(0.9 * S.to_go) + 1) & ~1));
        }
        if (use_classic) chunk = std::min(chunk, 16);
        chunk = std::min(chunk, R.jcap - S.J_enq);
        chunk = (int)std::min<long>(chunk, R.max_steps - R.steps_total);
        if (chunk <= 0) break;
        const int hi = S.J_enq + chunk;           // records max(0, J_enq - 1)..hi inclusive
        if (pmode || !classic) poison_records(S.J_enq, hi);
        if (pmode) {
            launch_persist(R.A, chunk, f32_seq);
            HIP_TRY(hipGetLastError());   // (157 KB of static LDS: a refused launch must surface, not time out)
        } else if (classic) {
            enqueue_classic(R.A, R.pl, chunk);
            double* hp = h_pin + (vcap + 2) + 2 * kMaxGrid + 32;   // staging: 3 x (chunk+1)
            for (int q = 0; q < 3; ++q)
                HIP_TRY(hipMemcpyAsync(hp + q * (size_t)(kMaxChunk + 2), ctri + q * cs + (size_t)S.J_enq,
                                       sizeof(double) * (size_t)(chunk + 1), hipMemcpyDeviceToHost, stream));
        } else {
            // far from the end (a successor will follow): no tail kernel, the successor's first step publishes
            const bool tailless = S.tail_ok && depth >= 2 && chunk >= 2;
            ST_TRY(enqueue_chunk(R.A, R.pp, chunk, f32_seq, tailless, S.prev_tailless, S.J_enq));
            if (R.debug) fprintf(stderr, "[machip] enqueue J=%d chunk=%d tailless=%d pub=%d depth=%d near=%d\n", S.J_enq, chunk, (int)tailless, S.prev_tailless, depth, (int)near);
            S.prev_tailless = tailless ? chunk : 0;
        }
        LanPending p;
        p.tailless = (pmode || classic) ? 0 : S.prev_tailless;
        p.jstart = S.J_enq;
        p.classic = use_classic;
        p.jend = hi;
        p.ev = nullptr;
        if (use_classic) {
            ST_TRY(get_event(&p.ev));
            HIP_TRY(hipEventRecord(p.ev, stream));
        }
        S.pend.push_back(p);
        S.J_enq = hi;
        R.steps_total += chunk; R.spmv_total += chunk;
        R.steps_used += chunk;
        if (f32_seq) R.steps_lowp += chunk;
    }
    return MACHIP_OK;
}
// wait until every record of chunk p is in h_tri
inline int Solver::lan_chunk_await(const LanPending& p) {
    if (p.classic) {
        HIP_TRY(hipEventSynchronize(p.ev));
        ev_pool.push_back(p.ev);
        // scatter the staged (alpha, beta, l1) into the interleaved mirror
        const double* hp = h_pin + (vcap + 2) + 2 * kMaxGrid + 32;
        for (int i = 0; i <= p.jend - p.jstart; ++i) {
            const size_t j = (size_t)(p.jstart + i);
            h_tri[3 * j] = hp[i];
            h_tri[3 * j + 1] = hp[(kMaxChunk + 2) + i];
            h_tri[3 * j + 2] = hp[2 * (kMaxChunk + 2) + i];
        }
        return MACHIP_OK;
    }
    ST_TRY(wait_flag(((unsigned long long)epoch << 32) | (unsigned long long)(unsigned int)p.jend));
    ST_TRY(ipc_check_err("Lanczos chunk"));
    // the flag can overtake the records on their way to host memory: the beta slots of this chunk
    // were poisoned before it was enqueued, wait until every one has landed
    unsigned long budget = 5000000ul;   // ~20 ms in total: a genuine NaN (non-finite input) must not stall the solve
    auto wait_slot = [&](size_t idx) {
        volatile double* slot = h_tri + idx;
        while (*slot != *slot && budget) { --budget; __builtin_ia32_pause(); }
    };
    for (int j = p.jstart ? p.jstart + 1 : 0; j <= p.jend && budget; ++j) wait_slot(3 * (size_t)j + 1);
    for (int j = p.jstart; j < p.jend && budget; ++j) { wait_slot(3 * (size_t)j); wait_slot(3 * (size_t)j + 2); }
    return MACHIP_OK;
}
inline int Solver::lan_chunks(LanRun& R, LanSeq& S) {
    Follower& F = S.F;
    const bool pmode = R.pmode, classic = R.classic, f32_seq = R.f32_seq;
    const int chunk0 = R.chunk0;
    const double lnorm = R.lnorm;
    const bool sched = OPT(sched, 1) != 0;
    while (!S.converged && !S.need_restart) {
        // keep one chunk in flight beyond the one being analysed
        // one chunk runs ahead of the host -- except in the end game (same threshold as the
        // short chunks), where the chunk in flight is likely the last one and a speculative
        // successor would only delay the explicit residual check queued behind it
        const bool near = sched ? (S.to_go < R.near_factor * chunk0 || (S.to_go >= 1e17 && S.est_latest < 1e3 * S.seq_tol * lnorm))
                                : S.est_latest < 1e3 * S.seq_tol * lnorm;
        const int depth = ((classic && !pmode) || near) ? 1 : ((sched && S.to_go > 8.0 * chunk0) ? 3 : 2);
        ST_TRY(lan_chunk_feed(R, S, near, depth));
        if (S.pend.empty()) { S.need_restart = true; break; }
        // a tail-less chunk that gets no successor now (end game, caps): its tail kernel after all
        if (S.prev_tailless && S.pend.back().tailless && (depth == 1 || S.J_enq >= R.jcap || R.steps_total >= R.max_steps)) {
            flush_tail(R.pp, S.prev_tailless, f32_seq);
            S.pend.back().tailless = 0; S.prev_tailless = 0;
        }
        LanPending p = S.pend.front();
        S.pend.pop_front();
        if (p.tailless && S.pend.empty()) {     // (cannot happen after the test above; a lost record would stall the host)
            flush_tail(R.pp, p.tailless, f32_seq);
            S.prev_tailless = 0;
        }
        ST_TRY(lan_chunk_await(p));
        const int J = p.jend;
        if (!F.ingest(h_tri, J)) return fail(MACHIP_BAD_ARG, "start vector is constant, zero or not finite");
        const int Jeff = F.Jeff;
        const bool broke = F.broke;
        const double est = F.est;
        S.est_latest = est;
        if (!broke && est > 0.0) S.to_go = forecast_to_go(S.hist, J, est, S.ltarget, 64);
        const bool at_cap = (J >= R.jcap) || (R.steps_total >= R.max_steps && S.pend.empty());
        const bool trig = F.triggered();
        if (lan_vote(R, S, J, !broke && !trig && !at_cap)) break;

        if (R.debug) fprintf(stderr, "[machip] %s J=%d Jeff=%d theta=%.15g est=%.3e to_go=%.0f broke=%d pend=%zu passes=%d\n", pmode ? "persist" : (classic ? "classic" : "pipe"), J, Jeff, sm.theta, lnorm > 0 ? est / lnorm : est, std::min(S.to_go, 1e9), (int)broke, S.pend.size(), sm.passes);
        if ((trig && est < 0.5 * S.last_check_est) || broke || at_cap) {
            ST_TRY(lan_check(R, S, Jeff, est));
            if (R.debug) fprintf(stderr, "[machip]    check J=%d rq=%.15g res=%.3e (tol %.1e)\n", Jeff, R.lam, R.res, R.tol);
            if (!S.converged && (broke || at_cap || f32_seq)) S.need_restart = true;   // fp32 sequence: one check, then fp64
        }
    }
    return MACHIP_OK;
}

// The restart policy: what is still in flight is drained; *again: another sequence follows, from the best Ritz vector so far
inline int Solver::lan_restart(LanRun& R, LanSeq& S, bool* again) {
    *again = false;
    // streamed records: steps still in flight keep writing record slots the next sequence / mode would poison and await
    if (S.stream_mode && R.switch_out) HIP_TRY(hipStreamSynchronize(stream));
    // drain what is still in flight (its results are not needed)
    for (const LanPending& p : S.pend) {
        if (p.ev) { HIP_TRY(hipEventSynchronize(p.ev)); ev_pool.push_back(p.ev); }
    }
    if (!S.pend.empty()) HIP_TRY(hipStreamSynchronize(stream));
    S.pend.clear();
    last_seq_f32 = R.f32_seq;
    last_seq_sharded = seq_sharded;
    if (R.switch_out || S.converged || R.steps_total >= R.max_steps) return MACHIP_OK;
    // restart from the best Ritz vector found so far (it sits normalised in yvec)
    HIP_TRY(hipMemcpyAsync(u, yvec, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
    if (R.f32_seq) {
        R.f32_seq = false;   // the planned hand-over to fp64, not counted as a restart
        // a start vector this good makes the pipelined beta a difference of nearly equal terms (it would report
        // a breakdown at once, seen at config 2): continue with the classic two-kernel recurrence there
        if (R.res * R.tiny_l < 1e-4 * std::fabs(R.lam)) R.classic = true;
        *again = true;
        return MACHIP_OK;
    }
    ++R.restarts;
    R.classic = true;   // refine with the accurate form (see enqueue_classic)
    *again = R.restarts <= 64;
    return MACHIP_OK;
}

// The finish: what the next solve learns from this one (step counts, the warm-start probe, the measured launch time), the stats
inline int Solver::lan_finish(LanRun& R, double* lambda2, machip_solve_stats* stats) {
    const SpmvPlan& pp = R.pp;
    // (what most steps of this solve were: a restart's classic tail does not change that)
    last_mode = R.steps_lowp > 0 ? 8 : R.pmode ? 4 : n <= OPT(classic_n, 256) ? 5 : pp.variant == kPanel ? 2 : pp.variant == kEll ? 3 : 1;
    last_steps = R.steps_used; last_steps_lowp = R.steps_lowp;
    if (R.switch_out) return kSwitchToExact;        // (no Ritz vector was formed: have_prev keeps its value; the caller continues with the exact mode)
    have_prev = true;
    if (R.warm_probe && R.start_overlap >= 0.0) {
        if (R.start_overlap < 2.0 / std::sqrt((double)n)) { warm_skip = std::min(63, kWarmSkip << std::min(warm_fails, 4)); ++warm_fails; }    // (a random unit vector's overlap is ~1/sqrt(n))
        else warm_fails = 0;
    }
    if (OPT(debug, 0) && R.warm_probe) fprintf(stderr, "[machip] warm start: overlap of the previous vector with the result %.3f%s\n", R.start_overlap, warm_skip ? " -> the next warm requests start cold (landscape-weighted)" : "");
    if (!(ev1_at_check && R.status == MACHIP_OK)) {     // (a converged Lanczos solve ends with its explicit check: ev1 is there)
        HIP_TRY(hipEventRecord(ev1, stream));
        HIP_TRY(hipEventSynchronize(ev1));
    }
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    *lambda2 = R.lam;
    if (R.steps_timed_acc >= 16 && last_mode >= 1 && last_mode <= 3) {     // (fused forms: gather, panel, padded)
        const int vk = std::max(0, std::min(7, (int)pp.variant));
        launch_us_hist[vk] = 1e3 * R.step_ms_acc / (double)R.steps_timed_acc / (pp.variant == kPanel ? 2.0 : 1.0);
    }
    if (stats) {
        stats->lanczos_steps = R.steps_used;      // (streamed records: up to the analysis point the solve ended at; steps_timed counts what was launched)
        stats->spmv_total = R.spmv_total;
        stats->vec_passes = R.steps_total * 7;   // per step and row: Z gathered (2) + Z own-row read (2) + Z written (2) + V written (1)
        stats->restarts = R.restarts;
        stats->nnz = R.nnz;
        stats->residual = R.res;
        stats->lnorm = R.lnorm;
        stats->gpu_ms = ms;
        stats->step_ms = R.step_ms_acc;
        stats->steps_timed = R.steps_timed_acc;
        stats->steps_lowp = R.steps_lowp;
        stats->drift = last_amp;
    }
    if (R.status == MACHIP_OK && R.lam < 1e-12 * R.tiny_l)
        return fail(MACHIP_DISCONNECTED, "lambda_2 ~ 0: the graph is not connected");
    if (R.status != MACHIP_OK)
        return fail(MACHIP_NOT_CONVERGED, "Lanczos hit the step cap before the residual test passed");
    return MACHIP_OK;
}

inline int Solver::solve_lanczos(const CsrView& A, long nnz, double lnorm, double tol, int max_steps, int start_mode,
                                 int forced_variant, double* lambda2, machip_solve_stats* stats) {
    LanRun R(A, nnz, lnorm, tol, max_steps <= 0 ? 200000 : max_steps, OPT(debug, 0) != 0);
    // explicit-check kernels: run once or twice per solve, nobody re-reduces their partials per step -- at large n they may
    // use the whole chip (config 4: 84 us per check with 256 workgroups of 8 rows each)
    R.pl = plan_spmv(opt, n, nnz, forced_variant, n > 32768 ? kMaxGrid : 0);
    R.pp = plan_pipe(opt, n, nnz, maxlen_hint);            // fused Lanczos-step kernel
    HIP_TRY(hipEventRecord(ev0, stream));
    ev1_at_check = false;
    if (n < 2) { *lambda2 = 0.0; return fail(MACHIP_BAD_ARG, "graph with a single node has no Fiedler pair"); }
    ST_TRY(lan_start_vector(R, start_mode));
    ST_TRY(lan_plan_route(R));
    for (bool again = true; again;) {
        LanSeq S(lan_follow_cfg(R), *this);
        ST_TRY(lan_begin_sequence(R, S));
        ST_TRY(S.stream_mode ? lan_stream(R, S) : lan_chunks(R, S));
        ST_TRY(lan_restart(R, S, &again));
    }
    return lan_finish(R, lambda2, stats);
}

}  // namespace machip
