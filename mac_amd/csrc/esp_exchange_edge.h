// mac_amd/csrc/esp_exchange_edge.h -- the exchange of esp_exchange.h carried out in the space of the candidates, on the handles of the
// edge-space relaxation (MACHIP_ESP_EDGE_RELAX: esp_relax_edge.h; MACHIP_ESP_EDGE_RELAX_TREE: esp_relax_edge_tree.h).  DESIGN section 19.
//
// G is the Gram matrix of the M = m + r columns (the candidates, then the r seeds of a tree handle) under Sigma0: closed form on a
// chain (esp_edge_G), stored on a tree handle.  With S' the selection plus the seeds and A the columns' incidence vectors,
//     R(S) = A^T Sigma(S) A        (M x M, independent of n)
// holds everything the exchange reads: s_f = w_f R[f][f], r_ef = R[e][f], Delta(e, f) = (1 - s_e)(1 + s_f) + w_e w_f R[e][f]^2, and
// taking column e in or out is R -= c R[:, e] R[e, :] with esp_exchange.h's coefficients.  In this space a column's incidence
// vector is a unit vector, so the greedy's and the exchange's kernels do the job unchanged through an EspView of M "candidates"
// (u = j, v = pinned) over R as their matrix: k_esp_scores reads w_j R[j][j], esp_z_entry row e of R less the pending columns,
// k_esp_update and k_esp_xch_tupdate entry e of z.  Both kernels that take a column of R read the row of that index: R need not
// stay bit-symmetric, the result is a function of the inputs alone.
//
// R lives in the relaxation's own N buffer (scratch for every evaluation; ld is the relaxation's): no ld x ld allocation here.
// Per call: R <- G (k_esp_xe_init on a chain, a copy of the stored G on a tree), the scores, the r seeds as forced picks (marked
// selected: never an f, never a row of T), the K selected candidates ascending as forced picks, T's K rows (T[row, f] = r_ef), then
// the rounds of esp_exchange.h with k_esp_xch_pairs_edge as the pair pass.  After every insertion the entering column's own score
// is set to its closed form (k_esp_xe_entered): G's entries are resistances and grow with the chain's length, the scores of the
// selected stay below 1.
#pragma once
#include <algorithm>
#include <vector>

#include "esp_exchange.h"
#include "esp_relax.h"

namespace machip {

struct EspXchEdge {
    int M = 0, ld = 0;            // columns (m + r) and the relaxation's leading dimension
    int *cu = nullptr, *cv = nullptr, *sel = nullptr, *pi = nullptr, *bad = nullptr;      // the view's arrays, ld entries each (zeros beyond M)
    double *cw = nullptr, *s = nullptr, *Zb = nullptr, *cb = nullptr, *pv = nullptr;
    EspBest* best = nullptr;
    EspXch* x = nullptr;          // the K rows of T, the partials, ratios and scale (esp_exchange.h)

    EspView view() const {
        EspView V;
        V.np = M; V.ld = ld; V.m = M; V.cu = cu; V.cv = cv; V.cw = cw; V.s = s; V.sel = sel; V.Zb = Zb; V.cb = cb;
        V.pv = pv; V.pi = pi; V.best = best; V.order = nullptr; V.gain = nullptr; V.bad = bad;
        return V;
    }
    int grid() const { return std::max(1, std::min(kEspGrid, (M + kBlock - 1) / kBlock)); }
};

// ---- R <- G, chain form: esp_edge_G per entry inside m x m, zeros beyond (k_edge_assemble without D and without the identity).
// grid = ld: workgroup i owns row i and writes it with 16-byte stores. ----
__global__ __launch_bounds__(kBlock) void k_esp_xe_init(double* __restrict__ Rm, int ld, int m, const int* __restrict__ lo,
                                                        const int* __restrict__ hi, const double* __restrict__ R) {
    const int i = blockIdx.x;
    double2* row2 = reinterpret_cast<double2*>(Rm + (size_t)i * ld);
    const bool in = i < m;
    const int li = in ? lo[i] : 0, hi_i = in ? hi[i] : 0;
    for (int j2 = threadIdx.x; j2 < ld / 2; j2 += kBlock) {
        double v[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int j = 2 * j2 + q;
            v[q] = (in && j < m) ? esp_edge_G(R, li, hi_i, lo[j], hi[j]) : 0.0;
        }
        row2[j2] = make_double2(v[0], v[1]);
    }
}

// ---- the view's columns: cu[j] = j, cv[j] = -1 (pinned), cw = the candidates' weights, then the seeds' ----
__global__ __launch_bounds__(kBlock) void k_esp_xe_columns(int* __restrict__ cu, int* __restrict__ cv, double* __restrict__ cw, int M, int m,
                                                           int ld, const double* __restrict__ w, const double* __restrict__ sw) {
    for (int j = blockIdx.x * kBlock + threadIdx.x; j < ld; j += gridDim.x * kBlock) {
        cu[j] = j < M ? j : 0;
        cv[j] = -1;
        cw[j] = j < m ? w[j] : j < M ? sw[j - m] : 0.0;
    }
}

// ---- the pair pass.  grid = (K, chunks): workgroup (row, y) owns the row of T of e = rowe[row] and the candidates
// [y per, (y + 1) per), per even.  r_ef = T[row][f]: the row is streamed contiguously, two candidates per lane and trip with
// 16-byte loads of T, s and cw and an 8-byte load of sel (the arrays hold ld entries: a pair never leaves them).  Selected
// columns and f >= m (the seeds) are skipped.  One (value, f) partial per workgroup. ----
__global__ __launch_bounds__(kBlock) void k_esp_xch_pairs_edge(EspView V, int m, const double* __restrict__ T, const int* __restrict__ rowe,
                                                               int per, double* __restrict__ pv, int* __restrict__ pf) {
    __shared__ double sv[kBlock / kWave];
    __shared__ int si[kBlock / kWave];
    const int row = blockIdx.x, e = rowe[row];
    const double2* tr2 = reinterpret_cast<const double2*>(T + (size_t)row * V.ld);      // (ld is a multiple of 64: rows are 512-byte aligned)
    const double2* s2 = reinterpret_cast<const double2*>(V.s);
    const double2* w2 = reinterpret_cast<const double2*>(V.cw);
    const int2* l2 = reinterpret_cast<const int2*>(V.sel);
    const double se = V.s[e], we = V.cw[e];
    const long f0 = (long)blockIdx.y * per;
    const int f1 = (int)min((long)m, f0 + per);
    double bv = -INFINITY;
    int bf = INT_MAX;
    for (int f = (int)f0 + 2 * threadIdx.x; f < f1; f += 2 * kBlock) {
        const int q = f >> 1;
        const double2 r = tr2[q], sf = s2[q], wf = w2[q];
        const int2 taken = l2[q];
        if (!taken.x) esp_better(bv, bf, esp_xch_delta(se, sf.x, we, wf.x, r.x), f);
        if (f + 1 < f1 && !taken.y) esp_better(bv, bf, esp_xch_delta(se, sf.y, we, wf.y, r.y), f + 1);
    }
    esp_block_argmax(bv, bf, sv, si);
    if (threadIdx.x == 0) { pv[(size_t)row * gridDim.y + blockIdx.y] = bv; pf[(size_t)row * gridDim.y + blockIdx.y] = bf; }
}

// ---- the entering column's own score after its pick.  Exactly s / (1 + s) = 1 - 1 / (1 + s); k_esp_update forms it as
// s - w c z_e^2, which cancels from s down to below 1: on a long chain s = w G_ee reaches 1e5, the rounding of eps s is then
// 1e-11 in a score whose 1 - s_e is the factor of a later removal and can be 1e-4.  One workgroup, after k_esp_update of an
// insertion (z = Zb[:, j]): s_e <- 1 - scale, scale = 1 / (1 + s) as k_esp_xch_step left it (absolute error one ulp of 1).
// A column g with the bits of e -- the same weight, z_g = z_e and the same updated score: a candidate listed twice -- is the same
// column under Sigma (R_gg = R_ee = R_eg), its score is the same closed form, and it gets the same bits: exact ties stay exact. ----
__global__ __launch_bounds__(kBlock) void k_esp_xe_entered(EspView V, int e, int j, const double* __restrict__ scale) {
    __shared__ double s_upd;
    const double* z = V.Zb + (size_t)j * V.ld;
    if (threadIdx.x == 0) s_upd = V.s[e];
    __syncthreads();                                   // (s[e] is read before any thread writes it)
    const double se = s_upd, ze = z[e], we = V.cw[e], v = 1.0 - *scale;
    for (int g = threadIdx.x; g < V.m; g += kBlock)
        if (g == e || (z[g] == ze && V.cw[g] == we && V.s[g] == se)) V.s[g] = v;
}

inline void esp_xe_release(EspXchEdge*& e) {
    if (!e) return;
    void* bufs[] = {e->cu, e->cv, e->sel, e->pi, e->bad, e->cw, e->s, e->Zb, e->cb, e->pv, e->best};
    for (void* q : bufs) if (q) (void)hipFree(q);
    esp_xch_release(e->x);
    delete e;
    e = nullptr;
}

// The view's own arrays, once per handle (the relaxation's state exists: its ld is the view's).
inline int esp_xe_prepare(machip_esp* h, EspXchEdge* e) {
    if (e->cu) return MACHIP_OK;
    e->M = h->rx->edge->M;
    e->ld = h->rx->edge->ld;
    const size_t ld = (size_t)e->ld;
    ST_TRY(dev_alloc(&e->cu, ld)); ST_TRY(dev_alloc(&e->cv, ld)); ST_TRY(dev_alloc(&e->cw, ld)); ST_TRY(dev_alloc(&e->s, ld));
    ST_TRY(dev_alloc(&e->sel, ld)); ST_TRY(dev_alloc(&e->Zb, ld * (size_t)kEspDefaultFold)); ST_TRY(dev_alloc(&e->cb, (size_t)kEspDefaultFold));
    ST_TRY(dev_alloc(&e->pv, (size_t)kEspGrid)); ST_TRY(dev_alloc(&e->pi, (size_t)kEspGrid)); ST_TRY(dev_alloc(&e->best, 1));
    ST_TRY(dev_alloc(&e->bad, 1));
    hipStream_t st = h->stream;
    HIP_TRY(hipMemsetAsync(e->s, 0, sizeof(double) * ld, st));
    HIP_TRY(hipMemsetAsync(e->Zb, 0, sizeof(double) * ld * (size_t)kEspDefaultFold, st));
    HIP_TRY(hipMemsetAsync(e->cb, 0, sizeof(double) * (size_t)kEspDefaultFold, st));
    k_esp_xe_columns<<<std::max(1, std::min(kMaxGrid, (e->ld + kBlock - 1) / kBlock)), kBlock, 0, st>>>(e->cu, e->cv, e->cw, e->M, h->m, e->ld, h->cw,
                                                                                                       h->tr ? h->tr->sw : nullptr);
    HIP_TRY(hipGetLastError());
    return MACHIP_OK;
}

// R <- G into the relaxation's N buffer (a copy of G where it is stored, the chain's closed form where not); the buffer is returned.
inline int esp_xe_load_gram(machip_esp* h, double** Rm) {
    const EspEdge* E = h->rx->edge;
    *Rm = E->bufN;
    if (E->G) HIP_TRY(hipMemcpyAsync(*Rm, E->G, sizeof(double) * (size_t)E->ld * (size_t)E->ld, hipMemcpyDeviceToDevice, h->stream));
    else k_esp_xe_init<<<E->ld, kBlock, 0, h->stream>>>(*Rm, E->ld, h->m, E->eu, E->ev, h->R);
    HIP_TRY(hipGetLastError());
    return MACHIP_OK;
}

// the edge handles' space: R from G in the relaxation's N buffer, the seeds ahead of the selection, the entering column's closed form
struct EspXchEdgeSpace : EspXchSpace {
    machip_esp* h;
    ESP_INLINE int load(double** S) { return esp_xe_load_gram(h, S); }
    ESP_INLINE void pairs() { k_esp_xch_pairs_edge<<<dim3((unsigned)K, (unsigned)chunks), kBlock, 0, h->stream>>>(V, h->m, X->T, X->rowe, per, X->pv, X->pf); }
    ESP_INLINE void entered(int e, int j) { k_esp_xe_entered<<<1, kBlock, 0, h->stream>>>(V, e, j, X->scale); }      // (s_e / (1 + s_e) without the cancellation)
    ESP_INLINE void finish(int) {}
};

// machip_esp_exchange_edge after its checks: T (refused before G is built), the relaxation's state, the view, the space, the rounds
inline int esp_exchange_edge(machip_esp* h, int64_t k, std::vector<int>& rowe, int64_t max_swaps, double min_gain, int32_t* sel_out,
                             int32_t* out_idx, int32_t* in_idx, double* ratio, int64_t* n_swaps, int32_t* converged, double* t_ms) {
    EspXchEdgeSpace sp; sp.h = h;
    const int m = h->m, ld = esp_relax_route(h).ld;
    sp.K = (int)k; sp.fold = kEspDefaultFold; sp.sel_count = ld;
    sp.chunks = std::max(1, std::min((m + kBlock - 1) / kBlock, (kEspXchTargetGroups + sp.K - 1) / sp.K));
    sp.per = ((m + sp.chunks - 1) / sp.chunks + 1) & ~1;      // (even: a chunk starts on a 16-byte boundary of its rows)
    if (!h->xe) h->xe = new EspXchEdge();
    EspXchEdge* E = h->xe;
    ST_TRY(esp_xch_prepare(E->x, (size_t)sp.K, (size_t)sp.K * (size_t)sp.chunks, (size_t)std::max<int64_t>(max_swaps, 1), (size_t)ld));
    ST_TRY(esp_relax_prepare(h));
    if (const int stp = esp_xe_prepare(h, E)) {      // (nothing half-made stays on the handle)
        esp_xe_release(h->xe);
        return stp;
    }
    sp.X = E->x; sp.V = E->view(); sp.P = E->grid(); sp.seeds = E->M - m;
    return esp_xch_run(h, sp, rowe, max_swaps, min_gain, sel_out, out_idx, in_idx, ratio, n_swaps, converged, t_ms);
}

}  // namespace machip
