// solver_lob.h -- the preconditioned modes of the eigen-solver: a block-size-1 LOBPCG on L preconditioned by the tridiagonal chain
// (precond.h) or, up to wb_soft() / wb_hard() closures, by the exact chain + closures inverse (woodbury.h).  Buffers, one chunk of
// iterations, the build of the preconditioner (lob_prepare), the host loop (lob_iterate: shared with the deflated columns of
// machip_lowest_pairs, solver_pairs_lob.h) and the Fiedler solve made of the two, solve_lob.  Members of Solver (solver.h).
#pragma once
#include "solver.h"

namespace machip {

inline int Solver::lob_alloc(long nnz) {
    if (!lob_ready) {
        ST_TRY(dev_alloc(&lx_x, n)); ST_TRY(dev_alloc(&lx_Lx, n)); ST_TRY(dev_alloc(&lx_p, n));
        ST_TRY(dev_alloc(&lx_Lp, n)); ST_TRY(dev_alloc(&lx_Lw, n));
        const size_t tcap = std::max((size_t)lob_c() * (size_t)lob_stride(), (size_t)n);   // chunk-transposed, zero padded past n
        double** tr[] = {&lx_rT, &lx_wT, &lx_tl, &lx_tdinv, &lx_tcu, &lx_ba, &lx_bd, &lx_bu};
        for (double** q : tr) {
            ST_TRY(dev_alloc(q, tcap));
            HIP_TRY(hipMemsetAsync(*q, 0, sizeof(double) * tcap, stream));
        }
        if (n > kTriMaxN && n <= kTriBigMaxN) {
            const size_t fcap = (size_t)kTriThreads * (size_t)((n + kTriThreads - 1) / kTriThreads);
            ST_TRY(dev_alloc(&lx_ys, tcap)); ST_TRY(dev_alloc(&lx_pas, tcap));
            ST_TRY(dev_alloc(&lx_as, fcap)); ST_TRY(dev_alloc(&lx_bs, fcap));
            ST_TRY(dev_alloc(&lx_maps, 4 * (size_t)kMaxGrid));   // one map per workgroup and direction
        }
        ST_TRY(dev_alloc(&lx_part, (size_t)kLobNS * kMaxGrid)); ST_TRY(dev_alloc(&lx_partR, 2 * kMaxGrid));
        ST_TRY(dev_alloc(&lx_bad, 1)); ST_TRY(dev_alloc(&lx_st, 1));
        HIP_TRY(hipHostMalloc((void**)&h_lrec, sizeof(double) * 4 * (size_t)(kLobCap + kLobMaxChunk + 4), hipHostMallocMapped));
        memset(h_lrec, 0, sizeof(double) * 4 * (size_t)(kLobCap + kLobMaxChunk + 4));
        HIP_TRY(hipHostGetDevicePointer((void**)&d_hlrec, h_lrec, 0));
        lob_ready = true;
    }
    if ((size_t)nnz > lx_colT_cap) {
        if (lx_colT) { HIP_TRY(hipStreamSynchronize(stream)); (void)hipFree(lx_colT); lx_colT = nullptr; drop_graphs(); }
        lx_colT_cap = (size_t)nnz + (size_t)nnz / 2 + 1024;
        ST_TRY(dev_alloc(&lx_colT, lx_colT_cap));
    }
    return MACHIP_OK;
}
// layout of the tridiagonal solver: up to n = 16 384 one workgroup, c = ceil(n/1024) unknowns per thread;
// beyond, 4 unknowns per thread and as many 1024-thread workgroups as that takes
inline int Solver::lob_c() const { return n > kTriMaxN ? kTriBigC : (n + kTriThreads - 1) / kTriThreads; }
inline int Solver::lob_stride() const {
    if (n <= kTriMaxN) return kTriThreads;
    const int q = (n + kTriBigC - 1) / kTriBigC;
    return (q + kTriThreads - 1) / kTriThreads * kTriThreads;
}
inline LobView Solver::lview(const SpmvPlan& pl) const {
    LobView L;
    L.n = n; L.c = lob_c(); L.stride = lob_stride();
    L.mapA = lx_maps; L.mapB = lx_maps ? lx_maps + kMaxGrid : nullptr;
    L.mapA2 = lx_maps ? lx_maps + 2 * kMaxGrid : nullptr; L.mapB2 = lx_maps ? lx_maps + 3 * kMaxGrid : nullptr;
    L.x = lx_x; L.Lx = lx_Lx; L.p = lx_p; L.Lp = lx_Lp; L.Lw = lx_Lw; L.rT = lx_rT; L.wT = lx_wT;
    L.tl = lx_tl; L.tdinv = lx_tdinv; L.tcu = lx_tcu; L.part = lx_part; L.partR = lx_partR;
    L.ys = lx_ys; L.pas = lx_pas;
    L.P_c = pl.grid; L.P_a = vgrid(); L.st = lx_st; L.hrec = d_hlrec; L.hflag = d_hflag;
    return L;
}
template <int CMAX>
inline void Solver::lob_launch_chunk_t(const CsrView& AT, const SpmvPlan& pl, const LobView& L, int steps, int nq) {
    OpLob op;
    op.L = L;
    // Round 4: between two products the update of iteration s - 1, the tridiagonal solve of iteration s and g = U^T y run as ONE
    // single-workgroup launch (k_lob_fused; the same arithmetic per unknown): T W S (F W S)^(steps - 1) U instead of (T W S U)^steps
    // (small graphs only: with more unknowns per thread the one workgroup's strided reads of six vectors cost more than the two
    // launches saved -- city10000, C = 10, in the configs[4] sweep: 870 it/s fused against 1 223)
    const bool fuse = OPT(lob_fuse, 1) != 0 && CMAX <= 4;
    WbView W0 = wb_active;       // (s = 0 without the exact preconditioner: the fused kernel then skips g)
    for (int s = 0; s < steps; ++s) {
        if (s == 0 || !fuse) {
            k_tri_solve<CMAX><<<1, kTriThreads, 0, stream>>>(L, s);
            if (wb_active.s > 0) k_wb_g<<<(wb_active.s + kBlock - 1) / kBlock, kBlock, 0, stream>>>(L, wb_active);
        }
        if (wb_active.s > 0) {   // w <- y - Z C^-1 U^T y
            const WbView& W = wb_active;
            k_wb_h<<<std::min(kMaxGrid, (W.s + 3) / 4), kBlock, 0, stream>>>(W);
            k_wb_w<<<(int)std::min<size_t>(kMaxGrid, W.cap / kWbwRows), kWbwThreads, 0, stream>>>(L, W);
        }
        if (nq > 0) lobq_project(L, nq);      // (a deflated column: w <- w - Q Q^T w, solver_pairs_lob.h)
        launch_spmv(pl, stream, AT, L.wT, op);
        if (fuse && s + 1 < steps) k_lob_fused<CMAX><<<1, kTriThreads, 0, stream>>>(L, W0, s);
        else k_lob_update<<<L.P_a, kBlock, 0, stream>>>(L, s);
    }
    k_lob_tail<<<1, 64, 0, stream>>>(L, steps);
}
inline void Solver::lob_launch_chunk(const CsrView& AT, const SpmvPlan& pl, const LobView& L, int steps, int nq) {
    if (n > kTriMaxN) {
        OpLob op;
        op.L = L;
        const int gw = L.stride / kTriThreads;
        for (int s = 0; s < steps; ++s) {
            k_tri_big_fwd<<<gw, kTriThreads, 0, stream>>>(L);
            k_tri_big_mid<<<gw, kTriThreads, 0, stream>>>(L);
            k_tri_big_fin<<<gw, kTriThreads, 0, stream>>>(L);
            if (wb_active.s > 0) {
                const WbView& W = wb_active;
                k_wb_g<<<(W.s + kBlock - 1) / kBlock, kBlock, 0, stream>>>(L, W);
                k_wb_h<<<std::min(kMaxGrid, (W.s + 3) / 4), kBlock, 0, stream>>>(W);
                k_wb_w<<<(int)std::min<size_t>(kMaxGrid, W.cap / kWbwRows), kWbwThreads, 0, stream>>>(L, W);
            }
            if (nq > 0) lobq_project(L, nq);
            launch_spmv(pl, stream, AT, L.wT, op);
            k_lob_update<<<L.P_a, kBlock, 0, stream>>>(L, s);
        }
        k_lob_tail<<<1, 64, 0, stream>>>(L, steps);
        return;
    }
    with_lob_chunk(L.c, [&](auto C) { lob_launch_chunk_t<SV(C)>(AT, pl, L, steps, nq); });
}
inline int Solver::lob_enqueue_chunk(const CsrView& A, const CsrView& AT, const SpmvPlan& pl, const LobView& L, int steps, int nq) {
    // (closure count and locked-column count are baked into the launches: the cached chunk graphs stay column 0's)
    if (!use_graph() || wb_active.s > 0 || nq > 0) { lob_launch_chunk(AT, pl, L, steps, nq); return MACHIP_OK; }
    const GraphKey key = std::make_tuple(1000 + pl.variant, pl.width, pl.grid, L.c + (n > kTriMaxN ? 100 : 0), steps);
    return replay_chunk(A, key, [&] { lob_launch_chunk(AT, pl, L, steps, 0); });
}
inline int Solver::wb_alloc() {
    // sized for the closures this solve actually has (+25 %, whole 256s), not for the tier's limit: 16 384 would mean
    // a 2 GiB capacitance matrix held for the life of the handle (and of every evaluation lane)
    long need = support_hint > 0 ? support_hint + support_hint / 4 : 256;
    need = std::min<long>(wb_limit_now, std::max<long>(256, (need + 255) / 256 * 256));
    const int want = (int)need;
    if (wb_ui && wb_cap_s >= want) return MACHIP_OK;
    if (wb_ui) {
        HIP_TRY(hipStreamSynchronize(stream));
        drop_graphs();          // cached chunk graphs carry the old addresses
        void* old[] = {wb_ui, wb_uj, wb_counts, wb_uc, wb_g, wb_h, wb_Cm, wb_Cm2, wb_maps};
        for (void* q : old) if (q) (void)hipFree(q);
        wb_ui = wb_uj = wb_counts = nullptr; wb_uc = wb_g = wb_h = wb_Cm = wb_Cm2 = wb_maps = nullptr;
    }
    wb_cap_s = want;
    ST_TRY(dev_alloc(&wb_ui, (size_t)want)); ST_TRY(dev_alloc(&wb_uj, (size_t)want)); ST_TRY(dev_alloc(&wb_counts, 2));
    ST_TRY(dev_alloc(&wb_uc, (size_t)want)); ST_TRY(dev_alloc(&wb_g, (size_t)want)); ST_TRY(dev_alloc(&wb_h, (size_t)want));
    const size_t ldw = ((size_t)want + kGjT - 1) / kGjT * kGjT;      // whole 64 x 64 tiles (k_gj_step)
    ST_TRY(dev_alloc(&wb_Cm, ldw * ldw)); ST_TRY(dev_alloc(&wb_Cm2, ldw * ldw));
    return MACHIP_OK;
}
// Z = T^-1 U, C = D^-1 + U^T Z, C^-1 (rocSOLVER).  MACHIP_NOT_CONVERGED when C is not positive definite.
inline int Solver::wb_build(const LobView& L, int s) {
    const size_t cap = (size_t)L.c * (size_t)L.stride;
    if (cap * (size_t)s > wb_Zt_cap) {
        if (wb_Zt) { HIP_TRY(hipStreamSynchronize(stream)); (void)hipFree(wb_Zt); wb_Zt = nullptr; }
        wb_Zt_cap = cap * (size_t)std::min(wb_cap_s, std::max(s + s / 2, 64));
        ST_TRY(dev_alloc(&wb_Zt, wb_Zt_cap));
    }
    WbView W;
    W.s = s; W.cap = cap; W.ui = wb_ui; W.uj = wb_uj; W.uc = wb_uc; W.Zt = wb_Zt; W.Cm = wb_Cm; W.g = wb_g; W.h = wb_h;
    W.ld = (s + kGjT - 1) / kGjT * kGjT;
    if (n > kTriMaxN) {   // batched multi-workgroup solves: grid = (workgroups per system, closures)
        const int gw = L.stride / kTriThreads;
        if (cap * (size_t)s > wb_pas_cap) {
            if (wb_pas) { HIP_TRY(hipStreamSynchronize(stream)); (void)hipFree(wb_pas); wb_pas = nullptr; }
            wb_pas_cap = wb_Zt_cap;
            ST_TRY(dev_alloc(&wb_pas, wb_pas_cap));
        }
        if (!wb_maps) ST_TRY(dev_alloc(&wb_maps, (size_t)4 * kMaxGrid * (size_t)wb_cap_s));
        WbBig Bg{wb_pas, wb_maps};
        k_wb_big_fwd<<<dim3(gw, s), kTriThreads, 0, stream>>>(L, W, Bg);
        k_wb_big_mid<<<dim3(gw, s), kTriThreads, 0, stream>>>(L, W, Bg);
        k_wb_big_fin<<<dim3(gw, s), kTriThreads, 0, stream>>>(L, W, Bg);
    } else with_lob_chunk(L.c, [&](auto C) { k_wb_cols<SV(C)><<<s, kTriThreads, 0, stream>>>(L, W); });
    const int g2s = (int)std::min<long>(kMaxGrid, ((long)W.ld * W.ld + kBlock - 1) / kBlock);
    k_wb_cap<<<g2s, kBlock, 0, stream>>>(L, W);
    // C^-1: ld / 32 blocked Gauss-Jordan steps on the matrix cores, ping-pong between the two buffers (woodbury.h)
    int* info = wb_counts + 1;
    HIP_TRY(hipMemsetAsync(info, 0, sizeof(int), stream));
    const int tiles = W.ld / kGjT;
    double *src = wb_Cm, *dst = wb_Cm2;
    // (from MACHIP_GJ_LOOK_MIN = 1 024 rows on, look-ahead: the workgroup holding the next pivot block inverts it for the next launch;
    // below that all tiles run in one round of workgroups and the redundant inversion is off nobody's critical path)
    const bool look = W.ld >= OPT(gj_look_min, 1024);
    if (look && !wb_piv) ST_TRY(dev_alloc(&wb_piv, (size_t)2 * kGjB * kGjB));
    for (int kb = 0, k = 0; kb < W.ld; kb += kGjB, ++k) {
        if (look) k_gj_step<0><<<dim3(tiles, tiles), 256, 0, stream>>>(src, dst, W.ld, kb, info, k ? wb_piv + (size_t)(k & 1) * kGjB * kGjB : nullptr,
                                                                    wb_piv + (size_t)((k + 1) & 1) * kGjB * kGjB);
        else k_gj_step<0><<<dim3(tiles, tiles), 256, 0, stream>>>(src, dst, W.ld, kb, info);
        std::swap(src, dst);
    }
    HIP_TRY(hipGetLastError());
    W.Cm = src;                                  // (the last step's output)
    int hinfo = 0;
    HIP_TRY(hipMemcpyAsync(&hinfo, info, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (hinfo != 0) return MACHIP_NOT_CONVERGED;     // a non-positive pivot: C is not positive definite numerically
    wb_active = W;
    return MACHIP_OK;
}

// The off-chain entries of A into the closure arrays.  hc[0]: how many there are; hc[1]: an entry the exact form cannot take.
inline int Solver::wb_extract(const CsrView& A, int hc[2]) {
    HIP_TRY(hipMemsetAsync(lx_bad, 0, sizeof(int), stream));
    k_wb_extract<<<1, kTriThreads, 0, stream>>>(A, (n + kTriThreads - 1) / kTriThreads, wb_cap_s, wb_ui, wb_uj, wb_uc, wb_counts, lx_bad);
    HIP_TRY(hipMemcpyAsync(&hc[0], wb_counts, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&hc[1], lx_bad, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return MACHIP_OK;
}

// The preconditioner of one matrix: T factored on the device (the chain alone under the exact preconditioner), the product's
// gather indices in the solver's layout, the closures' capacitance matrix inverted -- wb_active.s > 0 then.  MACHIP_NOT_CONVERGED: the
// capacitance matrix is not positive definite numerically.  lx_bad (T not positive definite) is read by the caller, behind its first wait.
inline int Solver::lob_prepare(const CsrView& A, long nnz, double lnorm, LobPrep* P) {
    ST_TRY(lob_alloc(nnz));
    P->pl = plan_spmv(opt, n, nnz, kAuto);
    P->L = lview(P->pl);
    const LobView& L = P->L;
    const int g2 = vgrid();
    const double scale = lnorm > 0 ? lnorm : 1.0;
    // ---- exact preconditioner (woodbury.h) when the graph is chain + at most kWbMaxS closures ----
    wb_active.s = 0;
    int wb_s = 0;
    lob_escalate = false;
    const bool wb_enabled = OPT(woodbury, 1) != 0 && chain_like && support_hint >= 0;
    P->may_escalate = wb_enabled && support_hint > wb_limit_now && support_hint <= wb_hard();
    if (wb_enabled && support_hint <= wb_limit_now) {
        ST_TRY(wb_alloc());
        int hc[2] = {0, 0};
        ST_TRY(wb_extract(A, hc));
        if (hc[0] > wb_cap_s && hc[0] <= wb_limit_now && !hc[1]) {
            // more off-chain entries than the buffers were sized for (support_hint counts active CANDIDATES; fixed edges off
            // the chain are closures too): grow to what is there and extract again -- these are the stiff cases the exact
            // preconditioner exists for, it must not be skipped silently
            const long keep = support_hint;
            support_hint = hc[0];
            const int st_grow = wb_alloc();
            support_hint = keep;
            if (st_grow != MACHIP_OK) return st_grow;
            ST_TRY(wb_extract(A, hc));
        }
        if (hc[0] > 0 && hc[0] <= wb_cap_s && !hc[1]) wb_s = hc[0];
    }
    const int chain_only = wb_s > 0 ? 1 : 0;
    // ---- T = tridiag(L) + sigma I (chain Laplacian + sigma I under the exact preconditioner), factored on
    // the device; gather indices in the solver's layout ----
    const double sigma = (wb_s > 0 ? 1e-8 : 2.5e-7) * scale;
    HIP_TRY(hipMemsetAsync(lx_bad, 0, sizeof(int), stream));
    if (n > kTriMaxN) k_tri_factor_big<<<1, kTriThreads, 0, stream>>>(A, L.stride, sigma, lx_tl, lx_tdinv, lx_tcu, lx_as, lx_bs, lx_bad, chain_only);
    else {
        k_tri_band<<<g2, kBlock, 0, stream>>>(A, L.c, L.stride, lx_ba, lx_bd, lx_bu);
        with_lob_chunk(L.c, [&](auto C) { k_tri_factor<SV(C)><<<1, kTriThreads, 0, stream>>>(n, lx_ba, lx_bd, lx_bu, sigma, lx_tl, lx_tdinv, lx_tcu, lx_bad, chain_only); });
    }
    P->AT = A;
    k_lob_perm_cols<<<(int)std::min<long>(kMaxGrid, (nnz + kBlock - 1) / kBlock), kBlock, 0, stream>>>(A.col, nnz, L.c, L.stride, lx_colT);
    P->AT.col = lx_colT;
    if (wb_s > 0) {
        const int st = wb_build(L, wb_s);
        if (st != MACHIP_OK && st != MACHIP_NOT_CONVERGED) return st;
        if (st == MACHIP_NOT_CONVERGED) return MACHIP_NOT_CONVERGED;   // capacitance not SPD numerically: Lanczos takes over
    }
    return MACHIP_OK;
}

// Returns MACHIP_OK (converged: yvec, *lam, *res set), MACHIP_NOT_CONVERGED (caller falls back to
// Lanczos) or an error.
inline int Solver::solve_lob(const CsrView& A, long nnz, double lnorm, double tol, int max_steps, int start_mode,
                             double* lam, double* res, long* iters, long* spmvs, long* restarts_out) {
    LobPrep P;
    const int st_prep = lob_prepare(A, nnz, lnorm, &P);
    if (st_prep != MACHIP_OK) return st_prep;
    const SpmvPlan& pl = P.pl;
    const int g2 = vgrid();
    const double scale = lnorm > 0 ? lnorm : 1.0;
    // ---- start vector: normalised into yvec, w2 = L yvec, Rayleigh quotient ----
    const double* src = (start_mode == 1 && have_prev) ? yvec : (have_start ? start : nullptr);
    if (!src) { k_fill_start<<<g2, kBlock, 0, stream>>>(u, n, 0x1234567ull); src = u; }
    HIP_TRY(hipMemcpyAsync(y_raw, src, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
    k_vec_sums<<<g2, kBlock, 0, stream>>>(y_raw, n, part_c);
    double rq = 0.0, r1 = 0.0;
    ST_TRY(check_vector(A, pl, &rq, &r1));
    *spmvs = 1; *iters = 0; *restarts_out = 0;
    int hbad = 0;
    HIP_TRY(hipMemcpyAsync(&hbad, lx_bad, sizeof(int), hipMemcpyDeviceToHost, stream));   // (never the legacy stream: another lane's thread may be capturing a graph)
    HIP_TRY(hipStreamSynchronize(stream));
    if (hbad || !(rq == rq)) return MACHIP_NOT_CONVERGED;
    *lam = rq; *res = r1 / scale;
    if (*res < tol) return MACHIP_OK;
    return lob_iterate(A, P, lnorm, tol, max_steps, 0, r1, lam, res, iters, spmvs, restarts_out);
}

// The host loop of the preconditioned modes from a start vector that has been checked (unit norm in yvec, w2 = L yvec, its Rayleigh
// quotient in rq_dev, its residual's 1-norm r1): chunks of iterations watched through the records, the explicit check, restarts.
// nq > 0: a deflated column of machip_lowest_pairs (solver_pairs_lob.h) -- w = M^-1 r is projected against the first nq columns of
// pairs->Q in every iteration, x twice before every explicit check.  nq = 0 is the Fiedler solve.  Statuses as solve_lob's.
inline int Solver::lob_iterate(const CsrView& A, const LobPrep& P, double lnorm, double tol, int max_steps, int nq, double r1,
                               double* lam, double* res, long* iters, long* spmvs, long* restarts_out) {
    const SpmvPlan& pl = P.pl;
    const LobView& L = P.L;
    const CsrView& AT = P.AT;
    const bool may_escalate = P.may_escalate;
    const int g2 = vgrid();
    const bool debug = OPT(debug, 0) != 0;
    const double scale = lnorm > 0 ? lnorm : 1.0;
    double rq = 0.0;
    const int cap = std::min(kLobCap, max_steps > 0 ? max_steps : kLobCap);
    const int patience = std::max(64, OPT(lob_patience, 10000));   // iterations without a new best residual
    // (exact preconditioner: a handful of iterations in all, each six launches -- short chunks, no speculation)
    const bool wb = wb_active.s > 0;
    const int chunk0 = wb ? 4 : std::min(kLobMaxChunk, std::max(1, OPT(lob_chunk, 16)));
    const double ltarget = std::log(std::max(tol * scale, 1e-300));
    int it_enq = 0, restarts = 0;
    double best = r1;
    int best_it = 0;
    while (true) {
        ++epoch;
        k_lob_start<<<g2, kBlock, 0, stream>>>(L, yvec, w2, rq_dev, it_enq, epoch);
        std::deque<int> pend;
        std::deque<std::pair<int, double>> hist;
        double to_go = 1e18, est = 1e300;
        bool check = false, bad = false;
        int ramp = wb ? 2 : 4;
        while (!check) {
            const bool near = to_go < 2.0 * chunk0;
            const int depth = (near || wb) ? 1 : 2;
            while ((int)pend.size() < depth && it_enq < cap) {
                int chunk = std::min(chunk0, ramp);   // easy problems (T ~ L) converge in a handful of iterations
                ramp = std::min(chunk0, ramp * 2);
                if (near) chunk = std::min(chunk, std::max(2, (int)(0.75 * to_go) + 1));
                chunk = std::min(chunk, cap - it_enq);
                ST_TRY(lob_enqueue_chunk(A, AT, pl, L, chunk, nq));
                it_enq += chunk;
                *spmvs += chunk;
                pend.push_back(it_enq);
            }
            if (pend.empty()) { check = true; break; }
            int jend = pend.front();
            pend.pop_front();
            ST_TRY(wait_flag(((unsigned long long)epoch << 32) | (unsigned long long)(unsigned int)jend));
            const unsigned long long fv = *(volatile unsigned long long*)h_flag;
            bad = (fv & 0x80000000ull) != 0;
            {   // the flag can overtake the record on its way to host memory (seen once in ~60 solves as a
                // stale residual that triggered premature checks): wait for the record's own tag
                volatile double* rec = h_lrec + 4 * (size_t)jend;
                const double want = lob_tag(epoch, jend);
                for (unsigned long spins = 0; rec[2] != want; ++spins) {
                    if (spins > 200000000ul) return fail(MACHIP_HIP_ERROR, "preconditioned solve: iteration record never arrived");
                    __builtin_ia32_pause();
                }
                est = rec[1];
            }
            if (debug) fprintf(stderr, "[machip] lobpcg it=%d theta=%.15g est=%.3e to_go=%.0f bad=%d pend=%zu\n", jend, h_lrec[4 * (size_t)jend], est / scale, std::min(to_go, 1e9), (int)bad, pend.size());
            if (est < best) { best = est; best_it = jend; }
            if (est > 0.0) to_go = forecast_to_go(hist, jend, est, ltarget, 48);
            if (bad || !(est == est) || est < tol * scale || jend >= cap || jend - best_it > patience) check = true;
            // the tridiagonal preconditioner crawls and an exact one is affordable: hand back for the second tier
            if (!wb && may_escalate && !check && ((jend >= 1500 && to_go > 3000.0) || jend >= 6000)) {
                HIP_TRY(hipStreamSynchronize(stream));
                *iters = it_enq; *restarts_out = restarts;
                lob_escalate = true;
                if (debug) fprintf(stderr, "[machip] lobpcg it=%d: escalating to the exact preconditioner (to_go %.0f)\n", jend, std::min(to_go, 1e9));
                return MACHIP_NOT_CONVERGED;
            }
        }
        // ---- explicit check of the current x (fresh SpMV), also the refresh point of a restart ----
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipMemcpyAsync(y_raw, lx_x, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
        if (nq > 0) { pairs_project(y_raw, nq, 2); pairs_project(y_raw, nq, 2); }
        k_vec_sums<<<g2, kBlock, 0, stream>>>(y_raw, n, part_c);
        ST_TRY(check_vector(A, pl, &rq, &r1));
        *spmvs += 1;
        *iters = it_enq;
        *restarts_out = restarts;
        if (debug) fprintf(stderr, "[machip]    lobpcg check it=%d rq=%.15g res=%.3e (tol %.1e)\n", it_enq, rq, r1 / scale, tol);
        if (!(rq == rq)) { *lam = rq; return MACHIP_NOT_CONVERGED; }      // (yvec is no vector any more: the caller must not start from it)
        *lam = rq; *res = r1 / scale;
        if (*res < tol) return MACHIP_OK;
        if (it_enq >= cap || ++restarts > 12 || it_enq - best_it > patience) return MACHIP_NOT_CONVERGED;
    }
}

}  // namespace machip
