// solver_panel.h -- host side of the column-panel step (panel.h, panel_u.h): the per-row tables the assembly writes on the side,
// the panel form's buffers and its build, the launches of one step, plain products on the panel form.  Members of Solver (solver.h);
// the shapes and the tables that pick the kernel instantiations come from plan.h.
#pragma once
#include "solver.h"

namespace machip {

// y = L x for a plain vector on the panel form of the running solve (k_pan_mul8 without the recurrence's prologue + k_pan_rowop<Op>)
template <class Op>
inline void Solver::panel_spmv(const double* x, const Op& op, int grid) {
    const int g1 = pan.NB * pan.NP;
    const PipeView L = pview(SpmvPlan());
    with_pan_mul8_shape(pan.LPT, pan.TWT, [&](auto LP, auto TW) {
        k_pan_mul8<SV(LP), SV(TW), double><<<g1, kPanThreads, 0, stream>>>(x, panv.tptr, panv.thead, panv.bval, panv.bcol, panv.n, panv.C, panv.NP | (panv.TWW << 16), panv.NTB << 16, panv, L, -1);
    });
    k_pan_rowop<Op><<<grid, kBlock, 0, stream>>>(panv, x, op);
}
// ---- column-panel step (panel.h) ---------------------------------------------------------------
// What the assembly's fill pass writes on the side for the panel form (kernels.h PanSpec): the panel shape is a function of n
// (and of the handle's options) alone, so the per-row table exists before the host has seen nnz.  NP = 0: nothing to write.
inline int Solver::pan_spec_prepare(PanSpec* out) {
    *out = PanSpec();
    pan_rows_ready = false;
    if (!pan_allowed || !pat.prow) return MACHIP_OK;
    const PanPlan sh = plan_panel(opt, n, 0, 1, true, (long)csr_cap, true, OPT(stream, 1) != 0);      // (the shape solve() will plan)
    if (!sh.on) return MACHIP_OK;
    ST_TRY(pan_row_buffers(sh, sh.band));
    HIP_TRY(hipMemsetAsync(panv.ovf, 0, sizeof(int), stream));
    out->NP = sh.NP; out->C = sh.C; out->band = sh.band ? 1 : 0;
    out->ps = panv.ps; out->bd = panv.bd; out->bpk = panv.bpk; out->ovf = panv.ovf;
    pan_rows_ready = true; pan_rows_NP = sh.NP; pan_rows_C = sh.C; pan_rows_band = sh.band;
    return MACHIP_OK;
}
template <class T>
inline int Solver::pan_regrow(T** ptr, size_t count, bool* dropped) {
    if (*ptr) { if (!*dropped) { HIP_TRY(hipStreamSynchronize(stream)); drop_graphs(); *dropped = true; } (void)hipFree(*ptr); *ptr = nullptr; }
    return dev_alloc(ptr, count);
}
// per-row tables of the panel form (ps, band) and the per-panel partial products
inline int Solver::pan_row_buffers(const PanPlan& pn, bool band) {
    bool dropped = false;
    if ((size_t)pn.NP * (size_t)n > pan_y_cap) {
        ST_TRY(pan_regrow(&panv.ypart, (size_t)pn.NP * ((size_t)n + 2), &dropped));
        ST_TRY(pan_regrow(&panv.ps, ((size_t)pn.NP + 1) * (size_t)n, &dropped));
        pan_y_cap = (size_t)pn.NP * (size_t)n;
        pan_rows_ready = false;
    }
    if (!panv.ovf) ST_TRY(dev_alloc(&panv.ovf, 1));
    if (band && (size_t)n > pan_band_cap) {
        ST_TRY(pan_regrow(&panv.bd, 3 * (size_t)n, &dropped)); ST_TRY(pan_regrow(&panv.bpk, (size_t)n, &dropped));
        pan_band_cap = (size_t)n;
        pan_rows_ready = false;
    }
    return MACHIP_OK;
}
// (Re)build the panel form of A on the stream: buffers grow on demand (cached chunk graphs carry their addresses).
// rows_ready: the assembly has already written the per-row tables (ps, band) for this shape -- k_pan_rows is not needed.
inline int Solver::ensure_panel(const CsrView& A, long nnz, const PanPlan& pn, bool band, bool rows_ready) {
    const size_t cells = (size_t)pn.NB * pn.NP, NTP = (size_t)kPanWork * pn.TWW;
    const size_t NT = cells * NTP;
    bool dropped = false;
    if (NT > pan_nt_cap) {
        ST_TRY(pan_regrow(&panv.tptr, cells * (NTP + 1) + 1, &dropped)); ST_TRY(pan_regrow(&panv.thead, NT * 64, &dropped));
        pan_nt_cap = NT;
    }
    ST_TRY(pan_row_buffers(pn, band));
    if (!panv.coef) ST_TRY(dev_alloc(&panv.coef, 8));
    // band mode (Lanczos form, two launches): diagonal and chain neighbours stay out of the tiles -- k_pan_fin adds them
    panv.band = band ? 1 : 0;
    panv.rev = OPT(panel_rev, 1) != 0 ? 1 : 0;     // odd steps of the shifted form walk each wave's chunks backwards (panel_u.h: what the XCD's L2 still holds comes first); 0: forwards always
#ifdef PAN_CLOCKS
    if (!panv.clk) { ST_TRY(dev_alloc(&panv.clk, (size_t)16 * kMaxGrid)); HIP_TRY(hipMemsetAsync(panv.clk, 0, sizeof(long long) * 16 * kMaxGrid, stream)); }
#endif
    panv.n = n; panv.NP = pn.NP; panv.C = pn.C; panv.NB = pn.NB; panv.NTB = pn.NTB; panv.TWW = pn.TWW; panv.CELLS = pn.cells;
    // static ranges of the cells in the value / column arrays: pattern slots of the cell + its rows (the diagonal, when the band
    // stays in the tiles) + 64 x 128 entries of zero padding (the tile heights telescope), whole 64-entry chunks; once per shape
    const std::array<int, 5> key{pn.NP, pn.C, pn.NB, pn.NTB, pn.TWW};
    if (!panv.cbase || key != pan_shape_key) {
        HIP_TRY(hipStreamSynchronize(stream));
        if (!dropped) { drop_graphs(); dropped = true; }
        if (panv.cbase) { (void)hipFree(panv.cbase); panv.cbase = nullptr; }
        ST_TRY(dev_alloc(&panv.cbase, cells + 1));
        std::vector<int> cnt(cells + 1, 0);
        if (pat.prow) {
            HIP_TRY(hipMemsetAsync(panv.cbase, 0, sizeof(int) * (cells + 1), stream));
            k_pan_cellcap<<<(n + kBlock - 1) / kBlock, kBlock, 0, stream>>>(pat, 64 * pn.NTB, pn.C, pn.NP, panv.cbase);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(cnt.data(), panv.cbase, sizeof(int) * cells, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        } else {
            return fail(MACHIP_BAD_ARG, "column-panel form without a pattern");
        }
        std::vector<int> base(cells + 1, 0);
        size_t run = 0;
        for (size_t c = 0; c < cells; ++c) {
            base[c] = (int)run;
            run += (((size_t)cnt[c] + (size_t)64 * pn.NTB + 63) / 64) * 64 + (size_t)64 * (kPanMaxLen + 1);
            if (run > 2000000000ull) return fail(MACHIP_BAD_ARG, "column-panel form exceeds int32 indexing");
        }
        base[cells] = (int)run;
        HIP_TRY(hipMemcpyAsync(panv.cbase, base.data(), sizeof(int) * (cells + 1), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (run + kPanSlack > pan_cap) {
            ST_TRY(pan_regrow(&panv.bval, run + kPanSlack, &dropped)); ST_TRY(pan_regrow(&panv.bcol, run + kPanSlack, &dropped));
            pan_cap = run + kPanSlack;
        }
        pan_shape_key = key;
    }
    if (!rows_ready) {
        HIP_TRY(hipMemsetAsync(panv.ovf, 0, sizeof(int), stream));
        k_pan_rows<<<(n + kBlock - 1) / kBlock, kBlock, 0, stream>>>(A, panv);
        // (the per-row tables now describe THIS shape: a later solve of the same matrix in the shape the assembly had written them for
        // must not take the old flag for them -- advisor finding on round 5)
        pan_rows_ready = true; pan_rows_NP = pn.NP; pan_rows_C = pn.C; pan_rows_band = band;
    }
    const int g = pan_build_grid(pn.NB, pn.NP);      // (rows per thread of the build kernel: 1 .. 8)
    with_int<1, 8>((64 * pn.NTB + kPanThreads - 1) / kPanThreads, [&](auto R) { k_pan_build<SV(R)><<<g, kPanThreads, 0, stream>>>(A, panv); });
    HIP_TRY(hipGetLastError());
    (void)nnz;
    return MACHIP_OK;
}
#ifdef PAN_CLOCKS
#define MACHIP_FINU_CLK , (const PeerSet*)nullptr, 0, 0, panv.clk
#else
#define MACHIP_FINU_CLK
#endif
inline void Solver::launch_pan_step(const PipeView& L, int s, int jhost) {
    const int g1 = pan.NB * pan.NP;
    if (pan_u) {             // shifted recurrence (panel_u.h): 8-byte operand, no prologue in the matrix kernel; the row kernel leads
        if (pan32 && jhost >= 0 && jhost >= pan32_from)       // mixed mode: this step reads fp32 tile values (TWT = 3 shapes only: solve() checks)
            with_pan_mul8_shape(pan.LPT, 3, [&](auto LP, auto) { k_pan_mul8<SV(LP), 3, float><<<g1, kPanThreads, 0, stream>>>(PAN_MUL8_ARGS(panv, pu, L, s), pan_bv32); });
        else
            with_pan_mul8_shape(pan.LPT, pan.TWT, [&](auto LP, auto TW) { k_pan_mul8<SV(LP), SV(TW)><<<g1, kPanThreads, 0, stream>>>(PAN_MUL8_ARGS(panv, pu, L, s)); });
        with_finu_shape(pan, [&](auto B, auto M) { k_pan_finu<SV(B), SV(M)><<<pan.grid2, SV(B), 0, stream>>>(PAN_FINU_ARGS(panv, pu, L, s, jhost) MACHIP_FINU_CLK); });
        return;
    }
    if (pan.cells > 1) {     // several row blocks per workgroup, the panel loaded once (k_pan_mul_multi)
        const int gm = pan.NP * ((pan.NB + pan.cells - 1) / pan.cells);
        with_pan_rpt(pan.RPT, [&](auto R) { k_pan_mul_multi<SV(R)><<<gm, kPanThreads, 0, stream>>>(PAN_MUL_ARGS(panv, L, s)); });
    } else with_pan_rpt(pan.RPT, [&](auto R) { k_pan_mul<SV(R)><<<g1, kPanThreads, 0, stream>>>(PAN_MUL_ARGS(panv, L, s)); });
    with_block(pan.block2, [&](auto B) { k_pan_fin<SV(B)><<<pan.grid2, SV(B), 0, stream>>>(PAN_FIN_ARGS(panv, L, s)); });
}

}  // namespace machip
