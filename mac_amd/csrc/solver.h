// solver.h -- device-resident Lanczos solver for the Fiedler pair of a CSR Laplacian.
//
// Algorithm (replaces nx:151-256 TraceMIN + SuperLU, which the reference calls at
// mac/utils/fiedler.py:42): plain Lanczos on L restricted to 1-perp (the mean is projected out
// of every new vector, as nx:209-213 does), no re-orthogonalisation, the whole basis kept in HBM
// (288 GB makes that free) so the Ritz vector is one tall-skinny pass at the end.  One kernel
// launch per Lanczos step (kernels.h, "pipelined" form); chunks of steps are replayed from cached
// hipGraphs and run one chunk AHEAD of the host, which meanwhile analyses the previous chunk's
// O(J) scalars (tridiag.h).  Convergence is declared by the reference's own rule evaluated
// explicitly on the device:   || L v - lambda v ||_1 / || L ||_inf < tol     (nx:232, nx:246)
//
// This file is the DRIVER's core: struct Solver with its state, allocation, the graph cache, the explicit check and solve() with the
// mode choice.  Its other members are defined in solver_lanczos.h (the Lanczos driver: solve_lanczos in its phases),
// solver_lob.h (the preconditioned and exact modes), solver_panel.h (host side of the column-panel step) and solver_shard.h
// (the row-partitioned solves) and solver_pairs.h / solver_pairs_lob.h (the deflated columns of machip_lowest_pairs: Lanczos / preconditioned), all included at the end of this file; launch shapes and the dispatch onto kernel instantiations
// are in plan.h, kernels in kernels.h / panel.h / persist.h / precond.h / woodbury.h.
#pragma once
#include <functional>
#include <dlfcn.h>

#include <array>
#include <deque>
#include <limits>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "kernels.h"
#include "persist.h"
#include "precond.h"
#include "woodbury.h"
#include "panel.h"
#include "plan.h"
#include "tridiag.h"
#include "follow.h"

namespace machip {

// (Rounds 2-3 serialised stream captures against rocBLAS / rocSOLVER calls of other threads behind a process-wide lock: those
// libraries touch the legacy stream, which HIP refuses while another thread captures.  Round 4 removed the libraries -- the dense
// inverse is hand-written, woodbury.h -- and the lock with them: captures are thread-local, every other call of this library
// names its own non-blocking stream.)

// Communicator between PROCESSES whose eigen-solve is row-partitioned (machip_comm_init_ipc; kernels.h IpcView): this rank's
// share of every Lanczos step, the peers' buffers mapped through hipIpcOpenMemHandle, ordering by flag words in device memory.
struct IpcGroup {
    int nranks = 0, rank = 0;
    IpcView view;                        // flags / counters (kernel argument)
    void* Z0[kMaxPeers] = {};            // every rank's record buffers, partial sums, Ritz-vector staging, gradient (index = rank;
    void* Z1[kMaxPeers] = {};            // my own entries are my own pointers)
    double* part[kMaxPeers] = {};
    double* yraw[kMaxPeers] = {};
    double* g[kMaxPeers] = {};
    std::vector<void*> opened;           // what hipIpcCloseMemHandle must release
    unsigned long long* flags_mem = nullptr;   // my flag words + counters (device, exported to the peers)
    int* h_err = nullptr;                // mapped pinned
    int g0 = 0, g1 = 0;                  // my workgroups of the running sequence's step launch
    bool clean_exit = false;             // the owner said goodbye (machip_comm_close_ipc): destroying the handle raises no abort
    // (every error path of machip_ipc_export / machip_comm_init_ipc ends here: mappings closed, flag words and the error word freed)
    ~IpcGroup() {
        for (void* q : opened) (void)hipIpcCloseMemHandle(q);
        if (flags_mem) (void)hipFree(flags_mem);
        if (h_err) (void)hipHostFree(h_err);
    }
};

// Row-partitioned eigen-solve of an in-process communicator (machip_comm_init_local): the LEADER's
// solver (rank 0) drives every rank's stream -- per Lanczos step one launch per rank (that rank's share of the step's
// workgroups, on that rank's copy of matrix and operand, writing next records and partial sums into every copy),
// ordered by events: step s of rank r waits for step s - 1 of every rank.  Everything else of the solve (host analysis
// of the tridiagonal, explicit residual check, restarts) runs on the leader alone; the converged vector is copied to
// the peers.  The basis V is sharded by rows: each rank keeps the rows its workgroups produced and forms its part of
// the Ritz vector.
struct ShardRank {
    int device = 0;
    hipStream_t stream = nullptr;
    Z2 *Z0 = nullptr, *Z1 = nullptr;
    double *part = nullptr, *V = nullptr, *ypart = nullptr, *sdev = nullptr, *yvec = nullptr;
    CsrView A{};                 // this rank's own assembled copy of L(x)
    hipEvent_t ev[2] = {nullptr, nullptr};
    int g0 = 0, g1 = 0;          // workgroups [g0, g1) of a step (set per solve from the plan)
};
struct ShardGroup {
    std::vector<ShardRank> rk;   // rk[0] = the leader
    hipEvent_t fork = nullptr;
    bool same_device = true;
};

struct PairsBuf;      // work space and per-column results of machip_lowest_pairs (solver_pairs.h)
struct PairsCol;
struct LanRun;        // one solve_lanczos call, one Krylov sequence of it, one chunk in flight (solver_lanczos.h)
struct LanSeq;
struct LanPending;
using GraphKey = std::tuple<int, int, int, int, int>;
// what lob_prepare leaves for the iterations on one matrix: launch shape, buffers, the product's view with permuted columns
struct LobPrep { SpmvPlan pl; LobView L; CsrView AT; bool may_escalate = false; };

struct Solver {
    Options opt = default_options();    // the handle's option table (machip_set_option); a copy of the process defaults at creation
    int n = 0;
    hipStream_t stream = nullptr;
    size_t vcap = 0;            // Lanczos vectors that fit in V
    // Krylov state
    double *u = nullptr, *V = nullptr, *tri = nullptr, *part = nullptr;
    Z2 *Z0 = nullptr, *Z1 = nullptr;
    LanState* st = nullptr;
    // explicit-check / result state (OpLanczos "column 0" machinery)
    double *y_raw = nullptr, *w2 = nullptr, *yvec = nullptr, *ypart = nullptr, *sdev = nullptr;
    double *part_c = nullptr, *part_a2 = nullptr, *part_r = nullptr, *scratch3 = nullptr, *rq_dev = nullptr;
    LanState* st2 = nullptr;
    // classic (two-kernel) Lanczos state: the accurate fallback for tiny / nearly exhausted Krylov spaces
    double *wc = nullptr, *ctri = nullptr, *part_u = nullptr, *part_a = nullptr;
    LanState* stc = nullptr;
    float* valf = nullptr;      // fp32 copy of the matrix values (mixed-precision mode)
    size_t valf_cap = 0, csr_cap = 0;   // csr_cap: capacity of the caller's CSR buffers (0 = unknown: grow on demand)
    bool last_seq_f32 = false;  // the basis V of the last sequence holds floats (ritz_block must not read it as fp64)
    long last_steps_lowp = 0;   // fp32 steps of the last Lanczos solve
    double* start = nullptr;    // persistent cold-start vector
    bool have_start = false, have_prev = false;
    int ks_max = 16;
    // pinned host staging
    double* h_tri = nullptr;    // mirror of tri (pinned, device-mapped: the tail kernel writes it)
    double* d_htri = nullptr;   // device view of h_tri
    double* d_hpin = nullptr;   // device view of h_pin (kernels write the host's small results there themselves)
    unsigned long long* h_flag = nullptr;   // pinned completion flag polled by the host
    unsigned long long* d_hflag = nullptr;
    unsigned int epoch = 0;
    double* h_pin = nullptr;    // misc
    hipEvent_t ev0 = nullptr, ev1 = nullptr, evs0 = nullptr, evs1 = nullptr;   // evs*: bracket the Krylov chunks only
    bool ev1_at_check = false;  // ev1 was recorded behind the last explicit check's kernels (and that check has been waited for)
    // Speculative epilogue: work the caller wants behind a PASSING explicit check (machip_fw_step: gradient, top-K, Frank-Wolfe
    // bookkeeping) is enqueued behind EVERY check's kernels, before the host waits for the check -- if the check passes, its
    // results are there at the same wait (one host round trip less per iteration); if not, it runs again behind the next check.
    std::function<void()> after_check;
    long check_seq = 0, hook_seq = -1, final_check_seq = -2;    // hook results are valid iff hook_seq == final_check_seq
    bool spec_likely = true;    // the check about to run is expected to pass (its residual estimate is below the tolerance): only then is the
                                // epilogue worth enqueueing behind it -- behind a failing check its kernels only delay the next chunk
    std::vector<hipEvent_t> ev_pool;
    // cached chunk graphs: (variant, width, grid, steps) -> exec
    std::map<GraphKey, std::array<hipGraphExec_t, 2>> graphs;
    unsigned graph_flip = 0;
    const void* graph_csr_key = nullptr;
    bool profiled = false;      // a rocprofiler-sdk is attached to the process (graphs are then off unless option "graph" = 1)
    // Captured chunks or eager launches (option `graph`: 1 / 0; unset = automatic).  Rounds 1-4 captured every chunk: the host had to
    // get a whole chunk out at each end-game hop.  With streamed records (round 5) the queue is fed continuously, and eager launches
    // -- no submission seam per graph -- are faster wherever a launch runs longer than the host needs to issue one (~4.4 us):
    // configs[3] 241.5 -> 246.0 it/s, configs[1] 706 -> 721, two-lane sweeps c4s 265 -> 293, c2s 923 -> 1 178; city10000's 4.2 us
    // steps lose 3.7 % and keep their graphs (tools/r5_eager.sh).  launch_us: measured in-solve time per launch of this handle's last
    // solve in the same step form, the model before there is one; either way the results are the same bits.
    double launch_us_hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // by step form (SpmvPlan::variant)
    double cur_launch_us = 0.0;                           // what the running solve's fused chunks go by
    bool use_graph(double launch_us = 0.0) const {
        if (opt.is_set(kOpt_graph)) return OPT(graph, 1) != 0;
        if (profiled) return false;
        // (evaluation lanes never capture: a lane's hipGraph executables cost the other lanes their hardware queues -- configs[1] as a
        // 4-lane sweep 1 185 -> 635 it/s after one captured solve per lane -- and city10000's lanes run as fast eagerly, 1 216 vs 1 224)
        if (throughput_lane) return false;
        return launch_us > 0.0 && launch_us < 5.2;
    }
    // host copies of T
    std::vector<double> ha, hb, hl1;
    std::vector<double> wk, guess;
    tri::Smallest sm;
    int J_last = 0;             // dimension of the Krylov space behind the current yvec
    long last_steps = 0;        // steps the previous solve needed (chunk sizing hint)
    int maxlen_hint = 0;        // longest row of the matrix about to be solved (0 = unknown)
    // preconditioned mode (precond.h): allocated on first use
    double *lx_x = nullptr, *lx_Lx = nullptr, *lx_p = nullptr, *lx_Lp = nullptr, *lx_Lw = nullptr;
    double *lx_rT = nullptr, *lx_wT = nullptr, *lx_tl = nullptr, *lx_tdinv = nullptr, *lx_tcu = nullptr;
    double *lx_ys = nullptr, *lx_pas = nullptr, *lx_as = nullptr, *lx_bs = nullptr;   // big-n solver scratch
    double* lx_maps = nullptr;   // 4 x stride chunk maps of the multi-workgroup tridiagonal solve
    double *lx_ba = nullptr, *lx_bd = nullptr, *lx_bu = nullptr;   // tridiagonal band of L in the solver's layout
    // exact chain + closures preconditioner (woodbury.h)
    int *wb_ui = nullptr, *wb_uj = nullptr, *wb_counts = nullptr;
    double *wb_uc = nullptr, *wb_g = nullptr, *wb_h = nullptr, *wb_Zt = nullptr, *wb_Cm = nullptr;
    size_t wb_Zt_cap = 0, wb_pas_cap = 0;
    double *wb_pas = nullptr, *wb_maps = nullptr;   // batched multi-workgroup column solves (n > 16 384)
    double* wb_Cm2 = nullptr;    // second buffer of the blocked Gauss-Jordan inversion (ping-pong)
    double* wb_piv = nullptr;    // 2 x (32 x 32): look-ahead inverse of the next pivot block (k_gj_step)
    WbView wb_active{};          // s > 0 while the running solve uses it
    double *lx_part = nullptr, *lx_partR = nullptr;
    int *lx_colT = nullptr, *lx_bad = nullptr;
    PersistPack ppack{};         // packed registers / LDS image of the single-workgroup kernel (persist.h), per matrix
    int* ell_col = nullptr;      // padded fixed-width copy of a short-row matrix (k_ell_build; 16 slots per row at most)
    double* ell_val = nullptr;
    CsrView ell_view{};          // {n, nullptr, ell_col, ell_val} while the current solve steps on it
    size_t lx_colT_cap = 0;
    LobState* lx_st = nullptr;
    double *h_lrec = nullptr, *d_hlrec = nullptr;
    bool lob_ready = false, last_was_lob = false;
    // what the last solve's steps were (machip_solve_mode; bench.py prices the roofline of THAT launch group):
    // 1 fused gather step (k_pipe_vec on the CSR), 2 column-panel step, 3 padded fixed-width step, 4 single-workgroup kernel,
    // 5 classic two-kernel step, 6 preconditioned by the tridiagonal chain, 7 exact chain + closures mode, 8 fp32 + fp64 sequences
    int last_mode = 0;
    long last_wb_s = 0;          // closures of the exact mode's capacitance matrix in that solve
    int solver_mode = 0;        // 0 = auto, 1 = Lanczos, 2 = preconditioned (LOBPCG + tridiagonal solve)
    bool throughput_lane = false;   // this solver serves an evaluation lane (machip_eval_batch / machip_fw_sweep): many solves run at
                                    // once, so the automatic mode keeps to kernels that occupy ONE CU per solve where it can
    int precision = 0;          // 0 = fp64; 1 = fp32 Krylov iterate + fp64 refinement (machip_set_precision)
    bool chain_like = false;    // the fixed edges contain (nearly) the whole chain (i, i+1)
    long chain_edges = 0;       // how many of them
    long support_hint = -1;     // active candidate edges of the matrix about to be solved (-1 = unknown)
    long hist_lan_steps = -1, hist_lob_iters = -1;   // steps / iterations of the last solve in each mode
    long hist_exact_iters = -1;                       // ... of the last solve the exact chain + closures preconditioner served
    // nothing learnt from an earlier problem (the cached CSR handle, an evaluation lane): no previous vector, no warm-start credit, no step counts
    void forget_history() { have_prev = false; warm_skip = 0; warm_fails = 0; last_pr = 0.0; hist_lan_steps = -1; hist_lob_iters = -1; hist_exact_iters = -1; last_steps = 0; last_steps_lowp = 0; }
    // Lanczos -> exact hand-over (solve(): chain-like graphs beyond the single-workgroup sizes with at most wb_soft() closures): the
    // Lanczos loop gives up when its own forecast of the remaining steps costs more than 1.3x the exact mode's estimate, twice in a row
    static constexpr int kSwitchToExact = 1000;       // internal status of solve_lanczos, never leaves solve()
    double switch_est_us = 0.0;                       // > 0: the hand-over is allowed, the exact mode's estimated cost
    double switch_to_go = 0.0;                        // forecast at the hand-over (history for the next solve)
    static constexpr int kLobCap = 100000;
    // column-panel step (panel.h): the panel form of the matrix being solved, rebuilt per solve from its CSR
    bool seq_sharded = false;      // the running Krylov sequence is row-partitioned (its basis is spread over the ranks)
    bool seq_ipc = false;          // ... between processes (IpcGroup): every rank runs this host loop itself
    SpmvPlan seq_plan;             // ... with this launch shape
    ShardGroup* shard = nullptr;   // set (by the leader's handle) for the duration of a row-partitioned solve
    IpcGroup* ipc = nullptr;       // set while this handle belongs to an inter-process communicator with a row-partitioned eigen-solve
    bool last_seq_sharded = false; // the basis of the last sequence is spread over the ranks (ritz_block cannot read it)
    bool pan_allowed = false;   // the CSR is one this library assembled (diagonal first, other columns ascending)
    PanPlan pan;
    PanView panv{};
    bool pan_live = false;         // the panel form (shifted-recurrence shape) of the matrix being solved is built: plain products may use it (panel_spmv)
    bool pan_u = false;            // the running sequence's panel steps are those of the shifted recurrence (panel_u.h): 8-byte operand
    PanU pu{};
    PeerSet* d_ps = nullptr; PeerSet h_ps{};      // the row-partitioned panel step's peer set, in device memory
    double *pu_sig = nullptr, *pu_U0 = nullptr, *pu_U1 = nullptr;     // (pu.U0 / U1 point at these, or at the record buffers under an inter-process communicator)
    double last_amp = 0.0;         // largest accumulated drift factor of the last solve's shifted sequences (solve stats / tests)
    // mixed mode of the panel step (machip_set_precision(1), round 6): the LATE steps of a sequence read the tile values rounded to fp32
    bool pan32 = false;            // this solve may switch (shifted recurrence, eager launches, an instantiated shape)
    int pan32_from = INT_MAX;      // ... from this step of the running sequence on (decided by the host from the records; INT_MAX: not yet)
    float* pan_bv32 = nullptr;     // the panel form's value array rounded to fp32 (same layout as panv.bval)
    size_t pan_bv32_cap = 0;
    size_t pan_cap = 0, pan_nt_cap = 0, pan_y_cap = 0, pan_band_cap = 0;
    std::array<int, 5> pan_shape_key{0, 0, 0, 0, 0};     // shape the cells' static ranges (panv.cbase) were computed for
    PatternView pat{};          // union pattern of the handle (machip_create); none on a CSR-only handle
    bool pan_rows_ready = false;     // the last assembly wrote the per-row panel tables (PanSpec) ...
    int pan_rows_NP = 0, pan_rows_C = 0; bool pan_rows_band = false;     // ... for this shape

    // budget_mb > 0: HBM budget of the Krylov basis V for this instance (evaluation lanes take a share each)
    int init(int n_, hipStream_t s, int budget_mb = 0) {
        n = n_;
        stream = s;
        size_t budget = (size_t)(budget_mb > 0 ? budget_mb : OPT(vbudget_mb, 4096)) * (size_t)(1 << 20);
        vcap = budget / (sizeof(double) * (size_t)std::max(n, 1));
        vcap = std::max<size_t>(std::min<size_t>(vcap, 16384), 64);
        vcap = std::min<size_t>(vcap, (size_t)n + 10);   // a Krylov sequence never exceeds n - 1 + 8 columns (jcap)
        vcap = std::max<size_t>(vcap, 64);
        vcap = (size_t)OPT(vcap, (int)vcap);
        // rocprofiler-sdk (ROCm 7.2) segfaults inside its HSA interception when short graphs are
        // launched in quick succession (reproduced under rocprofv3 --kernel-trace on the pose-graph
        // tests; eager launches of the same kernels are fine): with a profiler attached fall back to
        // eager launches unless MACHIP_GRAPH says otherwise.
        profiled = dlopen("librocprofiler-sdk.so", RTLD_NOLOAD | RTLD_LAZY) != nullptr ||
                   dlopen("librocprofiler-sdk.so.1", RTLD_NOLOAD | RTLD_LAZY) != nullptr;
        ST_TRY(dev_alloc(&u, n));
        ST_TRY(dev_alloc(&V, (size_t)n * vcap));
        ST_TRY(dev_alloc(&tri, 3 * (vcap + 2)));
        ST_TRY(dev_alloc(&part, 2 * kNP * kMaxGrid));
        ST_TRY(dev_alloc(&Z0, n)); ST_TRY(dev_alloc(&Z1, n));
        ST_TRY(dev_alloc(&st, 1)); ST_TRY(dev_alloc(&st2, 1));
        HIP_TRY(hipMemsetAsync(st2, 0, sizeof(LanState), stream));      // (the explicit check's "column 0" counters stay {0, 0}: nothing advances them)
        ST_TRY(dev_alloc(&y_raw, (size_t)n + 2)); ST_TRY(dev_alloc(&w2, (size_t)n + 2)); ST_TRY(dev_alloc(&yvec, n));      // (+2: a panel's 16-byte operand loads may touch one double past n)
        ST_TRY(dev_alloc(&ypart, (size_t)n * ks_max)); ST_TRY(dev_alloc(&sdev, vcap + 2));
        ST_TRY(dev_alloc(&part_c, 3 * kMaxGrid)); ST_TRY(dev_alloc(&part_a2, kMaxGrid));
        ST_TRY(dev_alloc(&part_r, kMaxGrid)); ST_TRY(dev_alloc(&scratch3, 8)); ST_TRY(dev_alloc(&rq_dev, 1));
        ST_TRY(dev_alloc(&start, n));
        ST_TRY(dev_alloc(&wc, n)); ST_TRY(dev_alloc(&ctri, 3 * (vcap + 2)));
        ST_TRY(dev_alloc(&part_u, 3 * kMaxGrid)); ST_TRY(dev_alloc(&part_a, kMaxGrid)); ST_TRY(dev_alloc(&stc, 1));
        HIP_TRY(hipHostMalloc((void**)&h_tri, 3 * (vcap + 2) * sizeof(double), hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer((void**)&d_htri, h_tri, 0));
        HIP_TRY(hipHostMalloc((void**)&h_flag, 64, hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer((void**)&d_hflag, h_flag, 0));
        *h_flag = 0;
        HIP_TRY(hipHostMalloc((void**)&h_pin, (4 * (vcap + 2) + 2 * kMaxGrid + 64) * sizeof(double), hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer((void**)&d_hpin, h_pin, 0));
        HIP_TRY(hipEventCreate(&ev0)); HIP_TRY(hipEventCreate(&ev1));
        HIP_TRY(hipEventCreate(&evs0)); HIP_TRY(hipEventCreate(&evs1));
        return MACHIP_OK;
    }
    void destroy() {
        drop_graphs();
        pairs_free();
        void* ptrs[] = {u, V, tri, part, Z0, Z1, st, st2, y_raw, w2, yvec, ypart, sdev,
                        part_c, part_a2, part_r, scratch3, rq_dev, start, wc, ctri, part_u, part_a, stc,
                        lx_x, lx_Lx, lx_p, lx_Lp, lx_Lw, lx_rT, lx_wT, lx_tl, lx_tdinv, lx_tcu, lx_part, lx_partR,
                        lx_ys, lx_pas, lx_as, lx_bs, lx_maps, lx_ba, lx_bd, lx_bu, wb_ui, wb_uj, wb_counts, wb_uc, wb_g, wb_h, wb_Zt, wb_Cm, wb_Cm2, wb_piv, wb_pas, wb_maps,
                        lx_colT, lx_bad, lx_st, valf};
        {
            void* pb[] = {panv.tptr, panv.thead, panv.bval, panv.bcol, panv.ypart, panv.coef, panv.cbase, panv.ps, panv.tick, panv.claim, panv.ovf, panv.bd, panv.bpk};
            for (void* q : pb) if (q) (void)hipFree(q);
            void* pu_[] = {pu_U0, pu_U1, pu.W, pu_sig, pan_bv32, d_ps};
            for (void* q : pu_) if (q) (void)hipFree(q);
            void* pk[] = {ppack.band, ppack.cc, ppack.crow, ppack.ccol, ppack.cval, ell_col, ell_val};
            for (void* q : pk) if (q) (void)hipFree(q);
        }
        if (h_lrec) (void)hipHostFree(h_lrec);
        for (void* p : ptrs) if (p) (void)hipFree(p);
        if (h_tri) (void)hipHostFree(h_tri);
        if (h_flag) (void)hipHostFree(h_flag);
        if (h_pin) (void)hipHostFree(h_pin);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (evs0) (void)hipEventDestroy(evs0);
        if (evs1) (void)hipEventDestroy(evs1);
        for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    }

    bool start_guess = false;   // the start vector of this solve is the caller's own guess (machip_fiedler x0): left as it is
    // A warm start (MAC.Cache made real) only pays where consecutive Fiedler vectors resemble each other.  On the localised vectors of the
    // Erdos-Renyi configs they do not (overlap < 0.005: the weak spot moves every iteration), and the weighted cold start is 13 % faster.
    // The overlap of a solve's start vector with its result is free -- |s_0|, the first Ritz coefficient -- so a warm-started solve that
    // finds it below 2 / sqrt(n) -- no better than a random vector's -- sends the next `kWarmSkip` warm requests to the weighted cold start,
    // then probes again.  (Not a larger threshold: city10000's consecutive vectors overlap by 0.03 - 0.09 only and its warm start still
    // saves 16 % of the steps -- a smooth vector is rich in the low end of the spectrum.)  A function of the records alone: every rank of
    // a partitioned solve takes the same turn.
    static constexpr int kWarmSkip = 7;      // doubled by every further probe that fails in a row (at most 63): a trajectory whose vectors keep
    int warm_skip = 0, warm_fails = 0;       // moving pays for ever fewer probes
    double last_pr = 0.0;                    // participation ratio 1 / sum v^4 of the last explicitly checked vector (0: none yet on this handle)
    // the landscape after `sweeps` Jacobi sweeps (in y_raw or w2; per-workgroup maxima of the last sweep in part_c[0 .. pl.grid))
    // (the sweeps' only per-workgroup output are the maxima in part_c, 3 x kMaxGrid doubles: their grid may exceed kMaxGrid)
    SpmvPlan landscape_plan(long nnz) const { return plan_spmv(opt, n, nnz, kAuto, 3 * kMaxGrid); }
    int vgrid() const { return (int)std::min<long>(kMaxGrid, ((long)n + kBlock - 1) / kBlock); }

    template <typename T = double>
    PipeViewT<T> pview(const SpmvPlan& pl) const {
        PipeViewT<T> L;     // T = float: records and basis live in the same buffers, read as fp32
        L.n = n; L.st = st; L.Z0 = reinterpret_cast<ZRec<T>*>(Z0); L.Z1 = reinterpret_cast<ZRec<T>*>(Z1); L.V = reinterpret_cast<T*>(V); L.tri = tri; L.htri = d_htri; L.hflag = d_hflag; L.part = part; L.P = pl.grid; L.chunk = 0; L.pub = 0; L.pubstep = 0;
        L.sig = (pl.variant == kPanel && pan_u) ? pu_sig : nullptr;      // (shifted records: panel_u.h)
        return L;
    }
    LanView check_view(const SpmvPlan& pl) const {   // "column 0" machinery for the explicit check
        LanView L;
        L.n = n; L.st = st2; L.u = y_raw; L.w = w2; L.V = yvec; L.alpha = scratch3; L.beta = scratch3 + 2;
        L.l1 = scratch3 + 4; L.part_u = part_c; L.P_u = vgrid(); L.part_a = part_a2; L.P_a = pl.grid;
        return L;
    }

    LanView classic_view(const SpmvPlan& pl) const {
        LanView L;
        L.n = n; L.st = stc; L.u = u; L.w = wc; L.V = V; L.alpha = ctri; L.beta = ctri + (vcap + 2);
        L.l1 = ctri + 2 * (vcap + 2); L.part_u = part_u; L.P_u = vgrid(); L.part_a = part_a; L.P_a = pl.grid;
        return L;
    }
    // ---- small graphs: a whole chunk of Lanczos steps in one single-workgroup launch (persist.h) ----
    template <typename T = double>
    PersistViewT<T> persist_view() const {
        PersistViewT<T> L;
        L.n = n; L.st = st; L.u = u; L.vprev = wc; L.V = reinterpret_cast<T*>(V); L.tri = tri; L.htri = d_htri; L.hflag = d_hflag;
        return L;
    }
    // y = V[:, :J] s  -> normalised into yvec; w2 = L yvec; returns (rq, ||w2 - rq yvec||_1).
    int explicit_check(const CsrView& A, const SpmvPlan& pl, int J, const double* s_host, double* rq,
                       double* res_l1, bool f32 = false) {
        if (seq_sharded && seq_ipc) { ST_TRY(ipc_ritz(seq_plan, J, s_host)); return check_vector(A, pl, rq, res_l1); }
        if (seq_sharded) { ST_TRY(shard_ritz(seq_plan, J, s_host)); return check_vector(A, pl, rq, res_l1); }
        memcpy(h_pin, s_host, sizeof(double) * (size_t)J);
        HIP_TRY(hipMemcpyAsync(sdev, h_pin, sizeof(double) * (size_t)J, hipMemcpyHostToDevice, stream));
        const int g2 = vgrid();
        const int KS = std::max(1, std::min(ks_max, J / 8));
        // (fp32 basis: the combination is accumulated in fp64; everything after it -- normalisation, L y, Rayleigh
        // quotient, the reference's residual test -- is fp64 on the fp64 matrix)
        if (f32) k_ritz_partial<float><<<dim3(g2, KS), kBlock, 0, stream>>>(reinterpret_cast<const float*>(V), n, J, sdev, ypart);
        else k_ritz_partial<<<dim3(g2, KS), kBlock, 0, stream>>>(V, n, J, sdev, ypart);
        k_ritz_combine<<<g2, kBlock, 0, stream>>>(ypart, n, KS, y_raw, part_c);
        HIP_TRY(hipGetLastError());
        return check_vector(A, pl, rq, res_l1);
    }
    // Same, for a vector already in y_raw with its sums in part_c.
    int check_vector(const CsrView& A, const SpmvPlan& pl, double* rq, double* res_l1) {
        const int g2 = vgrid();
        OpLanczos op;
        op.L = check_view(pl);
        const bool via_panel = pan_live && OPT(panel_ops, 1) != 0;
        const int pa = via_panel ? vgrid() : pl.grid;            // alpha partials: one per workgroup of the kernel that finishes the rows
        if (via_panel) { op.L.P_a = pa; panel_spmv(y_raw, op, pa); }
        else launch_spmv(pl, stream, A, y_raw, op);
        // (the partials and the Rayleigh quotient go straight into mapped pinned memory: two copy kernels less per check)
        double* hp = h_pin + (vcap + 2);
        double* dhp = d_hpin + (vcap + 2);
        k_resid_l1<<<g2, kBlock, 0, stream>>>(w2, yvec, n, part_a2, pa, dhp, rq_dev, dhp + kMaxGrid, dhp + kMaxGrid + 8);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev1, stream));     // end of the solve's device time if this check passes (no second wait then)
        ++check_seq;
        if (after_check && spec_likely) { after_check(); hook_seq = check_seq; }
        HIP_TRY(hipStreamSynchronize(stream));
        ST_TRY(ipc_check_err("explicit check"));
        ev1_at_check = true;
        double s = 0.0, q4 = 0.0;
        for (int i = 0; i < g2; ++i) { s += hp[i]; q4 += hp[kMaxGrid + 8 + i]; }
        *res_l1 = s;
        *rq = hp[kMaxGrid];
        last_pr = q4 > 0.0 ? 1.0 / q4 : (double)n;      // participation ratio of the checked (unit) vector: ~ the number of vertices it lives on
        return MACHIP_OK;
    }

    // Spin on the pinned flag the tail kernel publishes; fall back to a stream query now and then so
    // a device fault cannot hang the host.
    int wait_flag(unsigned long long want) {
        volatile unsigned long long* f = h_flag;
        for (unsigned long spins = 0;; ++spins) {
            const unsigned long long v = *f;
            if ((v >> 32) == (want >> 32) && (v & 0xffffffffull) >= (want & 0xffffffffull)) return MACHIP_OK;
            if ((spins & 0xfffff) == 0xfffff) {
                const hipError_t q = hipStreamQuery(stream);
                if (q != hipSuccess && q != hipErrorNotReady)
                    return fail(MACHIP_HIP_ERROR, std::string("stream error while waiting for a Lanczos chunk: ") + hipGetErrorString(q));
                if (q == hipSuccess) {   // stream drained: the flag must be there now
                    const unsigned long long v2 = *f;
                    if ((v2 >> 32) == (want >> 32) && (v2 & 0xffffffffull) >= (want & 0xffffffffull)) return MACHIP_OK;
                    return fail(MACHIP_HIP_ERROR, "Lanczos chunk finished without publishing its flag");
                }
            }
            __builtin_ia32_pause();
        }
    }

    // ---- the graph cache ----
    void drop_graphs() {
        for (auto& kv : graphs) for (hipGraphExec_t ge : kv.second) if (ge) (void)hipGraphExecDestroy(ge);
        graphs.clear();
    }
    // Capture this chunk once (launch() enqueues it on the stream), keep two executables, launch one.
    template <class Launch>
    int replay_chunk(const CsrView& A, const GraphKey& key, Launch&& launch) {
        if (graph_csr_key != (const void*)A.val) { drop_graphs(); graph_csr_key = (const void*)A.val; }   // different matrix buffers: cached graphs are stale
        auto it = graphs.find(key);
        if (it == graphs.end()) it = graphs.emplace(key, std::array<hipGraphExec_t, 2>{nullptr, nullptr}).first;
        // two executables per shape, used alternately: with one chunk running ahead, the same
        // hipGraphExec is never in flight twice
        hipGraphExec_t& ge = it->second[(size_t)(graph_flip++ & 1)];
        if (!ge) {
            hipGraph_t g = nullptr;
            HIP_TRY(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
            launch();
            HIP_TRY(hipStreamEndCapture(stream, &g));
            HIP_TRY(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
            (void)hipGraphDestroy(g);
        }
        HIP_TRY(hipGraphLaunch(ge, stream));
        return MACHIP_OK;
    }

    // ---- column-panel step, host side (solver_panel.h) ----
    template <class Op> void panel_spmv(const double* x, const Op& op, int grid);
    int pan_spec_prepare(PanSpec* out);
    template <class T> int pan_regrow(T** ptr, size_t count, bool* dropped);
    int pan_row_buffers(const PanPlan& pn, bool band);
    int ensure_panel(const CsrView& A, long nnz, const PanPlan& pn, bool band, bool rows_ready);
    void launch_pan_step(const PipeView& L, int s, int jhost = -1);
    // ---- row-partitioned solves (solver_shard.h) ----
    void shard_split(const SpmvPlan& pl);
    PeerSet shard_peers(const ShardRank& me, const SpmvPlan& pl) const;
    void launch_chunk_sharded(const SpmvPlan& pl, int steps);
    PeerSet ipc_peers(const SpmvPlan& pl) const;
    void ipc_split(const SpmvPlan& pl);
    void launch_chunk_ipc(const CsrView& A, const SpmvPlan& pl, int steps);
    void launch_chunk_ipc_pan(const SpmvPlan& pl, int steps, int j0);
    int ipc_ritz(const SpmvPlan& pl, int J, const double* s_host);
    int ipc_check_err(const char* where);
    int shard_broadcast_init();
    int shard_ritz(const SpmvPlan& pl, int J, const double* s_host);
    // ---- Lanczos driver (solver_lanczos.h) ----
    const double* landscape_field(const CsrView& A, const SpmvPlan& pl, int sweeps, int* grid_out = nullptr);
    int landscape_start(const CsrView& A, const SpmvPlan& pl);
    void enqueue_classic(const CsrView& A, const SpmvPlan& pl, int steps);
    int pack_persist(const CsrView& A);
    template <typename T> void launch_persist_t(const CsrView& A, int steps);
    void launch_persist(const CsrView& A, int steps, bool f32 = false);
    void launch_chunk(const CsrView& A, const SpmvPlan& pl, int steps, bool f32 = false, bool tailless = false, int pub = 0, int j0 = -1);
    void flush_tail(const SpmvPlan& pl, int steps, bool f32);
    int enqueue_chunk(const CsrView& A, const SpmvPlan& pl, int steps, bool f32 = false, bool tailless = false, int pub = 0, int j0 = -1);
    int get_event(hipEvent_t* e);
    void poison_records(int j0, int hi);
    bool record_landed(int j) const;
    int lan_start_vector(LanRun& R, int start_mode);
    int lan_plan_route(LanRun& R);
    FollowCfg lan_follow_cfg(const LanRun& R) const;
    int lan_begin_sequence(LanRun& R, LanSeq& S);
    bool lan_vote(LanRun& R, LanSeq& S, int J, bool undecided);
    int lan_check(LanRun& R, LanSeq& S, int Jeff, double est);
    int lan_stream_analyse(LanRun& R, LanSeq& S, int* what);
    int lan_stream_enqueue(LanRun& R, LanSeq& S, int chunk, bool tailless);
    int lan_stream_feed(LanRun& R, LanSeq& S, bool* fed);
    int lan_stream(LanRun& R, LanSeq& S);
    int lan_chunk_feed(LanRun& R, LanSeq& S, bool near, int depth);
    int lan_chunk_await(const LanPending& p);
    int lan_chunks(LanRun& R, LanSeq& S);
    int lan_restart(LanRun& R, LanSeq& S, bool* again);
    int lan_finish(LanRun& R, double* lambda2, machip_solve_stats* stats);
    int solve_lanczos(const CsrView& A, long nnz, double lnorm, double tol, int max_steps, int start_mode,
                      int forced_variant, double* lambda2, machip_solve_stats* stats);
    // ---- the q lowest pairs: deflated columns after the Fiedler solve (solver_pairs.h) ----
    PairsBuf* pairs = nullptr;      // allocated by the first machip_lowest_pairs call on the handle
    int pairs_alloc();
    void pairs_free();
    int pairs_fin_grid() const;
    void pairs_project(double* x, int nq, int slot);
    int pairs_column(const CsrView& A, long nnz, double lnorm, double tol, int max_steps, int c, int cap, PairsCol* out);
    int pairs_rest(const CsrView& A, long nnz, double lnorm, double tol, int max_steps, int q, PairsCol* cols);
    // ---- preconditioned and exact modes (solver_lob.h) ----
    int lob_alloc(long nnz);
    int lob_c() const;
    int lob_stride() const;
    LobView lview(const SpmvPlan& pl) const;
    // (nq: locked columns projected out of w in every iteration -- a deflated column of machip_lowest_pairs; 0: the Fiedler solve)
    template <int CMAX> void lob_launch_chunk_t(const CsrView& AT, const SpmvPlan& pl, const LobView& L, int steps, int nq);
    void lob_launch_chunk(const CsrView& AT, const SpmvPlan& pl, const LobView& L, int steps, int nq);
    int lob_enqueue_chunk(const CsrView& A, const CsrView& AT, const SpmvPlan& pl, const LobView& L, int steps, int nq);
    int wb_alloc();
    int wb_extract(const CsrView& A, int hc[2]);
    int wb_build(const LobView& L, int s);
    int lob_prepare(const CsrView& A, long nnz, double lnorm, LobPrep* P);
    int lob_iterate(const CsrView& A, const LobPrep& P, double lnorm, double tol, int max_steps, int nq, double r1,
                    double* lam, double* res, long* iters, long* spmvs, long* restarts_out);
    // ---- preconditioned deflated columns of machip_lowest_pairs (solver_pairs_lob.h) ----
    void lobq_project(const LobView& L, int nq);
    void lobq_lock(const LobView& L, int col);
    bool pairs_lob_eligible() const;
    int pairs_lob_prepare(const CsrView& A, long nnz, double lnorm, LobPrep* P, bool reuse, bool timed);
    int pairs_column_lob(const CsrView& A, long nnz, double lnorm, double tol, int max_steps, int c, LobPrep* P, PairsCol* out);
    int solve_lob(const CsrView& A, long nnz, double lnorm, double tol, int max_steps, int start_mode,
                  double* lam, double* res, long* iters, long* spmvs, long* restarts_out);

    // Most closures the exact (Woodbury) preconditioner takes: the dense s x s factorisation grows as s^3 (rocSOLVER:
    // 7 ms at 2 048), its memory as s^2 + n s; MACHIP_WB_MAX raises the default for graphs that converge no other way.
    // Two tiers: up to wb_soft() closures the exact preconditioner is built at once; between wb_soft() and wb_hard() the
    // tridiagonal one runs first and the solve ESCALATES to the exact one only when it turns out to crawl (the dense
    // factorisation then costs tens of ms -- against seconds, or no convergence at all: fuzz seed 129, n = 36 874,
    // 3 900 active closures, lambda_2 / ||L|| = 1e-10: 200 000 iterations without converging -> 27 iterations, 36 ms).
    int wb_soft() const { return std::max(64, std::min(16384, OPT(wb_max, kWbMaxS))); }
    // (evaluation lanes: 4 096 -- an s x s inverse beyond that, 2 s^3 flops on the whole chip, starves the other lanes: city10000, nine
    // budgets on four lanes, 423 it/s with escalations up to 16 384 closures against 669 with the cap; profiles/r4_exact_small.md)
    int wb_hard() const { return std::max(wb_soft(), std::min(throughput_lane ? 4096 : 16384, OPT(wb_hard, 16384))); }   // (11 600 closures on 30 000 nodes at lambda_2/||L|| = 3e-9: 0.30 s escalated against 0.75-0.9 s)
    int wb_limit_now = kWbMaxS;   // the tier this solve_lob call may use
    bool lob_escalate = false;    // set by solve_lob when it gives up early in favour of the exact preconditioner
    int wb_cap_s = 0;      // what the buffers below were sized for
    // The exact mode's cost model beyond the single-workgroup sizes, in us, from counts only (solve() has the measurements behind it):
    // set-up, the inverse, `its` iterations -- the last exact solve's count, 14 before there is one.
    double exact_cost_us() const {
        const double sd = (double)support_hint, nd = (double)n, ldw = (double)((support_hint + kGjT - 1) / kGjT * kGjT);
        const double its = hist_exact_iters > 0 ? (double)hist_exact_iters : 14.0;
        return 120.0 + 4e-6 * nd * sd + 1.1e-5 * sd * sd + (ldw / kGjB) * (13.0 + 3.5e-6 * ldw * ldw) +
               its * (45.0 + 1.2e-6 * nd * sd + 2.5e-6 * sd * sd);
    }
    // start_mode: 0 = stored cold-start vector (or device pseudo-random if none), 1 = previous
    // Fiedler vector (warm start).
    int solve(const CsrView& A, long nnz, double lnorm, double tol, int max_steps, int start_mode,
              int forced_variant, double* lambda2, machip_solve_stats* stats) {
        int mode = opt.is_set(kOpt_solver) ? OPT(solver, 0) : solver_mode;      // (option "solver" overrides machip_set_solver: 0 auto, 1 Lanczos, 2 preconditioned)
        if (mode == 3) mode = 0;      // (3 was the diagonally preconditioned LOBPCG of earlier builds: automatic now)
        // auto: chain-dominated graphs with few active closures per node (measured cross-over)
        const bool eligible = n > 256 && n <= kTriBigMaxN;
        // One preconditioned iteration costs about `ratio` Lanczos steps (three launches, one of them a
        // single workgroup).  Sparse closures: preconditioned.  Denser closures: only when the last
        // Lanczos solve of this problem was long (a stiff x) and the preconditioned mode has not been seen
        // to need more than 1/ratio of those steps.  Counts only -- never timings -- so the choice, and
        // with it every rounding of the trajectory, is reproducible run to run.
        // (where the single-workgroup Lanczos applies a step costs ~2 us instead of ~4.5: higher bar there --
        // measured: intel at 9 % closures/node 3.5 ms Lanczos vs 4.7 ms preconditioned, kitti_05 at 0.5 %: 8.6 vs 1.1)
        const bool small = n <= kPersistThreads * kPersistMaxRows;
        const long ratio = small ? 9 : 6;
        const bool sparse = (double)support_hint <= OPT(lob_density_pct, small ? 3 : 12) * 0.01 * (double)n;
        // The preconditioned mode is a block-size-1 LOBPCG preconditioned by the odometry chain: it is built for, and
        // has only been validated on (fuzz runs, every pose graph), chain-DOMINATED graphs.  On a dense random graph
        // the chain is no preconditioner at all (config 2, selected there by a mis-learnt step count: 44 us x 60-220
        // iterations against 1.1 ms of Lanczos), and a single-vector iteration has no guard against settling on a
        // higher eigenpair of a clustered spectrum, which the reference's residual test cannot tell apart.  So it is
        // confined to at most two active closures per node -- also when a caller forces it; denser graphs always take
        // the Lanczos path, which sees the whole Krylov space.
        const bool chain_dominated = support_hint < 0 || support_hint <= 2 * (long)n;
        const bool stiff = hist_lan_steps > 2500 && (hist_lob_iters < 0 || hist_lob_iters * ratio < hist_lan_steps);
        const bool slow_lob = hist_lan_steps > 0 && hist_lob_iters > 0 && hist_lob_iters * ratio > 2 * hist_lan_steps;
        // Round 4: with the hand-written inverse (woodbury.h: 0.08 ms at 157 closures, 0.28 ms at 645, where rocSOLVER took
        // 0.3-1.25 ms) and the parallel n x s product, the EXACT chain + closures preconditioner beats the single-workgroup Lanczos
        // on small pose graphs up to several hundred active closures (intel, 157-645 closures: 0.90 against 1.60 ms per solve,
        // 12 iterations against 830 steps).  Cost model in launch equivalents (~4.7 us), counts only: Lanczos = steps x 0.4
        // (single-workgroup step 1.9 us); exact = 60 (set-up, checks) + 2.7 per 32 closures (one inverse launch) + 7.5 per
        // iteration.  Without a Lanczos history the closure count alone decides (MACHIP_LOB_SMALL_S).
        const long lob_it_guess = hist_lob_iters > 0 ? hist_lob_iters : 14;
        const double cost_lob = 60.0 + 2.7 * ((double)support_hint / 32.0) + 7.5 * (double)lob_it_guess;
        // (Not on evaluation lanes: there 16 single-CU Lanczos solves run side by side -- intel sweep 4 670 it/s aggregate against
        // 2 460 when every lane launches the exact mode's chip-wide kernels; profiles/r4_exact_small.txt.)
        const bool exact_small = small && !throughput_lane && precision == 0 && support_hint >= 0 && support_hint <= OPT(lob_small_s, 700) &&
                                 support_hint <= wb_soft() && OPT(woodbury, 1) != 0 &&
                                 (hist_lan_steps <= 0 || cost_lob < 0.4 * (double)hist_lan_steps);
        // Beyond the single-workgroup sizes (n <= 16 384: the one-workgroup tridiagonal kernels the figures below were measured with)
        // the same choice needs a Lanczos history: with the look-ahead inverse (woodbury.h: 1.7 ms at 2 137 closures) the exact mode
        // solves city10000's second iterate (2 137 closures, lambda_2 = 0.0012) in 2.5 ms where 3 488 Lanczos steps take 14.3 ms.
        // Cost model in us, from counts only: set-up 120 + 4e-6 n s + 1.1e-5 s^2 (column solves, capacitance), inverse
        // (ld / 32) x (13 + 3.5e-6 ld^2), per iteration 45 + 1.2e-6 n s + 2.5e-6 s^2 (n x s and s x s products); a Lanczos step
        // 4.2 + 2e-6 nnz (tools/city_exact_probe.py, tools/ubench_gj.hip; profiles/r4_exact_big.md).
        bool exact_big = false;
        if (!small && n <= kTriMaxN && !throughput_lane && precision == 0 && support_hint > 0 && support_hint <= wb_soft() && hist_lan_steps > 0 &&
            OPT(woodbury, 1) != 0 && OPT(exact_big, 1) != 0)
            exact_big = exact_cost_us() < 0.8 * (double)hist_lan_steps * (4.2 + 2e-6 * (double)nnz);
        const bool want = chain_dominated &&
                          (mode == 2 || (mode == 0 && chain_like && support_hint >= 0 && ((sparse && !slow_lob) || stiff || exact_small || exact_big)));
        last_was_lob = false;
        final_check_seq = -2;
        // No history (or one that spoke for Lanczos): start with Lanczos, but let it hand over to the exact mode once ITS OWN forecast
        // says the rest of the solve costs more than that (city10000's first iterate: forecast > 1 000 steps from step 128 on -> 0.7 ms
        // of Lanczos + 3.0 ms exact instead of 7.3 ms).  Forecasts come from device results that are bit-reproducible: so is the choice.
        bool after_switch = false;
        long pre_steps = 0;
        if (!(eligible && want) && mode == 0 && eligible && chain_dominated && chain_like && !small && n <= kTriMaxN && !throughput_lane &&
            precision == 0 && forced_variant == 0 && support_hint > 0 && support_hint <= wb_soft() &&      // (sharded / inter-process solves too: every rank
            // holds the same tridiagonal records, takes the same decision at the same step, and runs the exact mode replicated)
            OPT(woodbury, 1) != 0 && OPT(exact_big, 1) != 0 && OPT(exact_switch, 1) != 0) {
            switch_est_us = exact_cost_us();
            const int st = solve_lanczos(A, nnz, lnorm, tol, max_steps, start_mode, forced_variant, lambda2, stats);
            switch_est_us = 0.0;
            if (st != kSwitchToExact) {
                if (st == MACHIP_OK) hist_lan_steps = last_steps - (long)(0.35 * (double)last_steps_lowp);
                return st;
            }
            after_switch = true;
            pre_steps = last_steps;
            hist_lan_steps = last_steps + (long)std::min(switch_to_go, 1e6);     // (what the solve would have taken, by its own forecast)
        }
        if ((eligible && want) || after_switch) {
            if (!after_switch) HIP_TRY(hipEventRecord(ev0, stream));      // (after a hand-over ev0 still marks the start of the Lanczos part)
            double lam = 0.0, res = 0.0;
            long iters = 0, spmvs = 0, rst = 0;
            // (evaluation lanes run many solves side by side: the exact mode's chip-wide kernels -- s column solves, the s x s inverse,
            // an n x s product per application -- are kept to the cheap cases there, the tridiagonal preconditioner serves the rest and
            // a crawling solve still escalates; city10000, 9 budgets on 4 lanes: 422 -> 664 it/s, profiles/r4_exact_small.md)
            wb_limit_now = throughput_lane ? std::min(wb_soft(), OPT(wb_lane_max, 256)) : wb_soft();
            int st = solve_lob(A, nnz, lnorm, tol, max_steps, start_mode, &lam, &res, &iters, &spmvs, &rst);
            if (st == MACHIP_NOT_CONVERGED && lob_escalate) {
                long it1 = iters, sp1 = spmvs;
                wb_limit_now = wb_hard();
                st = solve_lob(A, nnz, lnorm, tol, max_steps, start_mode, &lam, &res, &iters, &spmvs, &rst);
                iters += it1; spmvs += sp1;
            }
            if (st == MACHIP_OK) {
                HIP_TRY(hipEventRecord(ev1, stream));
                HIP_TRY(hipEventSynchronize(ev1));
                float ms = 0.f;
                HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
                last_mode = wb_active.s > 0 ? 7 : 6; last_wb_s = wb_active.s;
                have_prev = true; last_was_lob = true; last_steps = iters; J_last = 0;
                last_seq_sharded = false;        // (the final solve ran replicated, whatever a Lanczos prefix did: machip_comm_mode reports it)
                hist_lob_iters = iters;
                if (wb_active.s > 0) hist_exact_iters = iters;
                *lambda2 = lam;
                if (stats) {
                    stats->lanczos_steps = iters + pre_steps; stats->spmv_total = spmvs + pre_steps; stats->vec_passes = iters * 16 + pre_steps * 7;
                    stats->restarts = rst; stats->nnz = nnz; stats->residual = res; stats->lnorm = lnorm; stats->gpu_ms = ms;
                    stats->step_ms = ms; stats->steps_timed = iters + pre_steps; stats->steps_lowp = 0;
                }
                if (lam < 1e-12 * (lnorm > 0 ? lnorm : 1.0))
                    return fail(MACHIP_DISCONNECTED, "lambda_2 ~ 0: the graph is not connected");
                return MACHIP_OK;
            }
            if (st != MACHIP_NOT_CONVERGED) return st;
            // stagnated / T not positive definite: the Lanczos path takes over from its own start
        }
        const int st = solve_lanczos(A, nnz, lnorm, tol, max_steps, start_mode, forced_variant, lambda2, stats);
        // (mixed precision: the fp32 pre-phase inflates the count by roughly a third of its length; the learning rule
        // above is calibrated on fp64 step counts)
        if (st == MACHIP_OK) hist_lan_steps = last_steps - (long)(0.35 * (double)last_steps_lowp);
        return st;
    }

    // q Ritz vectors (column-major n x q) of the last Krylov sequence -> host buffer.  Column 0 is
    // the converged Fiedler vector in yvec; the others are the next Ritz vectors, orthonormalised
    // on the host; copies produced by Lanczos "ghost" Ritz values are skipped.
    int ritz_block(int q, double* X_host) {
        const int Jeff = std::max(1, std::min(J_last, (int)ha.size()));
        const int ncand = std::min(Jeff, q + 6);
        std::vector<double> th, S;
        if (!last_was_lob && !last_seq_f32 && !last_seq_sharded) tri::smallest_block(ha.data(), hb.data(), Jeff, ncand, th, S, wk);   // (no Krylov basis after the preconditioned mode: X is completed with orthonormal filler)
        const int g2 = vgrid();
        HIP_TRY(hipMemcpyAsync(X_host, yvec, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        int acc = 1;
        std::vector<double> col((size_t)n);
        auto orth_accept = [&](double n0) -> bool {
            for (int pass = 0; pass < 2; ++pass)
                for (int p = 0; p < acc; ++p) {
                    const double* xp = X_host + (size_t)p * n;
                    double dot = 0.0;
                    for (int i = 0; i < n; ++i) dot += xp[i] * col[(size_t)i];
                    for (int i = 0; i < n; ++i) col[(size_t)i] -= dot * xp[i];
                }
            double n2 = 0.0;
            for (int i = 0; i < n; ++i) n2 += col[(size_t)i] * col[(size_t)i];
            if (!(n2 > 1e-6 * std::max(n0, 1e-300))) return false;   // ghost copy / dependent
            const double inv = 1.0 / std::sqrt(n2);
            double* dst = X_host + (size_t)acc * n;
            for (int i = 0; i < n; ++i) dst[i] = col[(size_t)i] * inv;
            ++acc;
            return true;
        };
        for (int c = 1; c < (int)th.size() && acc < q; ++c) {
            memcpy(h_pin, S.data() + (size_t)c * Jeff, sizeof(double) * (size_t)Jeff);
            HIP_TRY(hipMemcpyAsync(sdev, h_pin, sizeof(double) * (size_t)Jeff, hipMemcpyHostToDevice, stream));
            const int KS = std::max(1, std::min(ks_max, Jeff / 8));
            k_ritz_partial<<<dim3(g2, KS), kBlock, 0, stream>>>(V, n, Jeff, sdev, ypart);
            k_ritz_combine<<<g2, kBlock, 0, stream>>>(ypart, n, KS, y_raw, part_c);
            HIP_TRY(hipMemcpyAsync(col.data(), y_raw, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            double mean = 0.0, n0 = 0.0;
            for (int i = 0; i < n; ++i) mean += col[(size_t)i];
            mean /= n;
            for (int i = 0; i < n; ++i) { col[(size_t)i] -= mean; n0 += col[(size_t)i] * col[(size_t)i]; }
            (void)orth_accept(n0);
        }
        // Krylov space exhausted (tiny or highly symmetric graph): complete the block with
        // deterministic vectors orthogonal to 1 and to the accepted columns, so X is always an
        // orthonormal n x q block like the reference's (nx:238).
        for (unsigned long long seed = 1; acc < q && seed < 64; ++seed) {
            double mean = 0.0, n0 = 0.0;
            for (int i = 0; i < n; ++i) {
                unsigned long long z = seed * 0xD1B54A32D192ED03ull + 0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1);
                z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
                z = z ^ (z >> 31);
                col[(size_t)i] = (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
                mean += col[(size_t)i];
            }
            mean /= n;
            for (int i = 0; i < n; ++i) { col[(size_t)i] -= mean; n0 += col[(size_t)i] * col[(size_t)i]; }
            (void)orth_accept(n0);
        }
        for (; acc < q; ++acc) {
            double* dst = X_host + (size_t)acc * n;
            for (int i = 0; i < n; ++i) dst[i] = 0.0;
        }
        return MACHIP_OK;
    }
};

}  // namespace machip

#include "solver_panel.h"
#include "solver_shard.h"
#include "solver_lob.h"
#include "solver_lanczos.h"
#include "solver_pairs.h"
#include "solver_pairs_lob.h"
