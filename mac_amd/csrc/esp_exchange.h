// mac_amd/csrc/esp_exchange.h -- the Fedorov exchange on the log tree count: best-swap local search from a given K-edge selection,
// on the state of a dense machip_esp handle (esp.h).  DESIGN section 18.
//
// S the selection, M = L_red(fixed) + sum_{e in S} w_e a_e a_e^T, Sigma = M^-1, r_ab = a_a^T Sigma a_b, s_e = w_e r_ee (the scores
// the handle keeps for all m candidates).  Taking e in S out and putting f not in S in multiplies det M by
//     Delta(e, f) = (1 - s_e)(1 + s_f) + w_e w_f r_ef^2                                        (a 2 x 2 determinant).
// A round takes the largest Delta over all K (m - K) pairs -- ties, exact fp64 equality, to the lowest e and then the lowest f --
// and stops when Delta - 1 <= min_gain.  Delta comes from ONE device function in one fixed expression (esp_xch_delta) and the
// order is total, so the winner does not depend on how the pairs are spread over workgroups: runs repeat bit for bit.
//
// The cross terms need no product with Sigma: T[row, :] = (Sigma a_e)^T for the K selected edges (K rows of ld doubles) gives
// r_ef = T[row_e, u_f] - T[row_e, v_f].  T is built once after the selection is loaded (esp_z_entry for K edges) and kept current:
// every rank-1 update (c, z) of Sigma does  T[row, :] -= c (z_u - z_v) z  for the selected (u, v) of each row, and the row of the edge
// that left becomes the row of the edge that entered:  Sigma_new a_f = z_f / (1 + s_f),  z_f the column the entering step made.
//
// The swap itself is two steps of the greedy's machinery with e given instead of argmaxed (k_esp_xch_step = k_esp_z's body): the
// removal is a pick of weight -w_e, c = -w_e / (1 - s_e); the insertion c = w_f / (1 + s_f'), s_f' the score after the removal.
// Each appends its z to Zb, k_esp_update rescales all m scores, and Zb is folded into Sigma when it is full, as in machip_esp_select.
// Per round the host reads one 24-byte record (the winner: it decides termination and names the edges of the two steps).
// The load and the round loop are esp_xch_run, here for the dense handle (EspXchDense) and for esp_exchange_edge.h's space.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "esp.h"
#include "esp_tree.h"

namespace machip {

constexpr int kEspXchLdsDefaultKb = 48;       // option esp_xch_lds_kb: a row of T goes to LDS when 8 ld bytes fit (ld <= 6 144: no launch above 64 KiB of LDS by default)
constexpr int kEspXchLdsMaxKb = 152;          // 160 KiB per CU less the reduction scratch (48 bytes) and what the runtime may want
constexpr int kEspXchTargetGroups = 1024;     // workgroups of a pair pass the candidate range is cut for when K alone gives fewer

struct EspXchBest {
    double val;
    int row, e, f, pad;
};

struct EspXch {
    double* T = nullptr;          // rows x ld
    size_t rows = 0;              // rows T is allocated for
    int* rowe = nullptr;          // the selected edge of every row
    double* pv = nullptr;         // partials of the pair pass: value and f per workgroup (e is the row's)
    int* pf = nullptr;
    size_t parts = 0;
    double* ratio = nullptr;      // (1 - s_e)(1 + s_f') of every swap
    size_t swaps = 0;
    double* scale = nullptr;      // 1 / (1 + s_f') of the last insertion: the entering row is z times this
    EspXchBest* best = nullptr;
};

// Delta(e, f).  One expression, every operation rounded once, in this order -- wherever a pair is evaluated it gives these bits.
__device__ __forceinline__ double esp_xch_delta(double se, double sf, double we, double wf, double r) {
#pragma clang fp contract(off)
    const double a = (1.0 - se) * (1.0 + sf);
    const double b = ((we * wf) * r) * r;
    return a + b;
}

// (v2, e2, f2) beats (v, e, f): larger value, then lower e, then lower f.  NaN never wins.
__device__ __forceinline__ bool esp_xch_beats(double v2, int e2, int f2, double v, int e, int f) {
    return v2 > v || (v2 == v && (e2 < e || (e2 == e && f2 < f)));
}

// ---- the forced step: the z of candidate e into Zb[:, j] (k_esp_z's body, e from the argument).  grid = ceil(ld / 256).
// Workgroup 0 records it.  mode > 0: e enters, c = w / (1 + s); mode < 0: e leaves, c = -w / (1 - s).  ratio (may be NULL) gets the
// swap's realised factor: the removal stores 1 - s, the insertion multiplies 1 + s' on. ----
__global__ __launch_bounds__(kBlock) void k_esp_xch_step(EspView V, const double* __restrict__ S, int j, int e, int mode,
                                                         double* __restrict__ ratio, double* __restrict__ scale) {
    __shared__ double alpha[kEspMaxFold];
    const int u = V.cu[e], v = V.cv[e];
    esp_z_alpha(V, u, v, j, alpha);
    __syncthreads();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < V.ld) V.Zb[(size_t)j * V.ld + i] = esp_z_entry(V, S, u, v, j, alpha, i);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double s = V.s[e], w = V.cw[e];
        const double den = mode > 0 ? 1.0 + s : 1.0 - s;
        V.cb[j] = (mode > 0 ? w : -w) / den;
        V.sel[e] = mode > 0 ? 1 : 0;
        if (!(den > 0.0)) *V.bad = 1;      // (a selected bridge, or lost numerically: the caller reports it)
        if (mode > 0) *scale = 1.0 / den;
        if (ratio) *ratio = mode > 0 ? *ratio * den : den;
    }
}

// ---- T from Sigma and the pending columns: row = blockIdx.x, T[row, :] = Sigma a_e for e = rowe[row].  grid = (K, ceil(ld / 256)) ----
__global__ __launch_bounds__(kBlock) void k_esp_xch_tbuild(EspView V, const double* __restrict__ S, int j, const int* __restrict__ rowe,
                                                           double* __restrict__ T) {
    __shared__ double alpha[kEspMaxFold];
    const int e = rowe[blockIdx.x];
    const int u = V.cu[e], v = V.cv[e];
    esp_z_alpha(V, u, v, j, alpha);
    __syncthreads();
    const int i = blockIdx.y * kBlock + threadIdx.x;
    if (i < V.ld) T[(size_t)blockIdx.x * V.ld + i] = esp_z_entry(V, S, u, v, j, alpha, i);
}

// ---- T under the rank-1 update (c, z) = (cb[j], Zb[:, j]): T[row, :] -= c (z_u - z_v) z.  Row `xrow` belongs to the edge of the swap
// under way: left alone by the removal (f_in < 0), and by the insertion set to z / (1 + s_f') with rowe[xrow] = f_in.
// grid = (K, ceil(ld / 256)). ----
__global__ __launch_bounds__(kBlock) void k_esp_xch_tupdate(EspView V, double* __restrict__ T, int* __restrict__ rowe, int j, int xrow,
                                                            int f_in, const double* __restrict__ scale) {
    const int row = blockIdx.x, i = blockIdx.y * kBlock + threadIdx.x;
    if (i >= V.ld) return;
    const double* z = V.Zb + (size_t)j * V.ld;
    double* t = T + (size_t)row * V.ld + i;
    if (row == xrow) {
        if (f_in < 0) return;
        *t = z[i] * *scale;
        if (i == 0) rowe[row] = f_in;      // (no thread reads rowe[xrow] in this launch)
        return;
    }
    const int e = rowe[row];
    const int u = V.cu[e], v = V.cv[e];
    const double d = (u >= 0 ? z[u] : 0.0) - (v >= 0 ? z[v] : 0.0);
    *t = __builtin_fma(-(V.cb[j] * d), z[i], *t);
}

// ---- the pair pass.  grid = (K, chunks): workgroup (row, y) owns the row of T of e = rowe[row] and the candidates
// [y per, (y + 1) per).  LDS: the row is brought into LDS first (8 ld bytes of dynamic LDS), else it is gathered from global
// memory.  The candidates' arrays are streamed (coalesced; L2-resident).  One (value, f) partial per workgroup. ----
template <bool LDS>
__global__ __launch_bounds__(kBlock) void k_esp_xch_pairs(EspView V, const double* __restrict__ T, const int* __restrict__ rowe, int per,
                                                          double* __restrict__ pv, int* __restrict__ pf) {
    extern __shared__ __attribute__((aligned(16))) double xch_row[];
    __shared__ double sv[kBlock / kWave];
    __shared__ int si[kBlock / kWave];
    const int row = blockIdx.x, e = rowe[row];
    const double* tr = T + (size_t)row * V.ld;
    if (LDS) {
        const double2* src = reinterpret_cast<const double2*>(tr);      // (ld is a multiple of 64: rows are 512-byte aligned)
        double2* dst = reinterpret_cast<double2*>(xch_row);
        for (int i = threadIdx.x; i < V.ld / 2; i += kBlock) dst[i] = src[i];
        __syncthreads();
        tr = xch_row;
    }
    const double se = V.s[e], we = V.cw[e];
    const long f0 = (long)blockIdx.y * per;
    const int f1 = (int)min((long)V.m, f0 + per);
    double bv = -INFINITY;
    int bf = INT_MAX;
    for (int f = (int)f0 + threadIdx.x; f < f1; f += kBlock) {
        if (V.sel[f]) continue;
        const int u = V.cu[f], v = V.cv[f];
        const double r = (u >= 0 ? tr[u] : 0.0) - (v >= 0 ? tr[v] : 0.0);
        esp_better(bv, bf, esp_xch_delta(se, V.s[f], we, V.cw[f], r), f);
    }
    esp_block_argmax(bv, bf, sv, si);
    if (threadIdx.x == 0) { pv[(size_t)row * gridDim.y + blockIdx.y] = bv; pf[(size_t)row * gridDim.y + blockIdx.y] = bf; }
}

// ---- the round's winner over the P = K chunks partials: one workgroup (k_esp_argmax with the three-key order) ----
__global__ __launch_bounds__(kBlock) void k_esp_xch_argmax(EspView V, const int* __restrict__ rowe, const double* __restrict__ pv,
                                                           const int* __restrict__ pf, int P, int chunks, EspXchBest* __restrict__ best) {
    __shared__ double sv[kBlock / kWave];
    __shared__ int se[kBlock / kWave], sf[kBlock / kWave], sr[kBlock / kWave];
    double bv = -INFINITY;
    int be = INT_MAX, bf = INT_MAX, br = -1;
    for (int p = threadIdx.x; p < P; p += kBlock) {
        const int r = p / chunks, e = rowe[r];
        if (esp_xch_beats(pv[p], e, pf[p], bv, be, bf)) { bv = pv[p]; be = e; bf = pf[p]; br = r; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double v2 = __shfl_xor(bv, o, kWave);
        const int e2 = __shfl_xor(be, o, kWave), f2 = __shfl_xor(bf, o, kWave), r2 = __shfl_xor(br, o, kWave);
        if (esp_xch_beats(v2, e2, f2, bv, be, bf)) { bv = v2; be = e2; bf = f2; br = r2; }
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sv[w] = bv; se[w] = be; sf[w] = bf; sr[w] = br; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < kBlock / kWave; ++q)
            if (esp_xch_beats(sv[q], se[q], sf[q], bv, be, bf)) { bv = sv[q]; be = se[q]; bf = sf[q]; br = sr[q]; }
        if (br < 0 || be < 0 || be >= V.m || bf < 0 || bf >= V.m) {      // no finite Delta: flag it, keep the record in bounds
            *V.bad = 1;
            bv = 0.0; be = 0; bf = 0; br = 0;
        }
        best->val = bv; best->row = br; best->e = be; best->f = bf; best->pad = 0;
    }
}

inline void esp_xch_release(EspXch*& x) {
    if (!x) return;
    void* bufs[] = {x->T, x->rowe, x->pv, x->pf, x->ratio, x->scale, x->best};
    for (void* q : bufs) if (q) (void)hipFree(q);
    delete x;
    x = nullptr;
}

// The arguments, decided on the host before a device is touched.  sorted_out: the selection ascending.  edge: the call is
// machip_esp_exchange_edge (esp_exchange_edge.h), which takes the edge-space relaxation's handles and no other.
inline int esp_xch_check(const machip_esp* h, int64_t k, const int32_t* sel_in, int64_t max_swaps, double min_gain, const void* sel_out,
                         const void* out_idx, const void* in_idx, const void* ratio, const void* n_swaps, const void* converged,
                         std::vector<int>& sorted_out, bool edge = false) {
    if (!h) return fail(MACHIP_BAD_ARG, "NULL handle");
    if (!sel_in || !sel_out || !n_swaps || !converged) return fail(MACHIP_BAD_ARG, "sel_in, sel_out, n_swaps or converged is NULL");
    if (max_swaps < 0) return fail(MACHIP_BAD_ARG, "max_swaps must be >= 0 (got " + std::to_string((long long)max_swaps) + ")");
    if (max_swaps > 0 && (!out_idx || !in_idx || !ratio)) return fail(MACHIP_BAD_ARG, "out_idx, in_idx or ratio is NULL with max_swaps > 0");
    if (!(min_gain >= 0.0) || !std::isfinite(min_gain)) return fail(MACHIP_BAD_ARG, "min_gain must be finite and >= 0");
    if (edge && h->relax_space == kEspRelaxNode)
        return fail(MACHIP_BAD_ARG, "the edge-space exchange works on the relaxation's Gram matrix: the handle must be made with MACHIP_ESP_EDGE_RELAX or MACHIP_ESP_EDGE_RELAX_TREE");
    if (!edge && (h->form == kEspFormFree || h->form == kEspFormTree))
        return fail(MACHIP_BAD_ARG, "the exchange works on the dense Sigma: not available on a MACHIP_ESP_MATRIX_FREE handle");
    if (h->beta != 0.0)
        return fail(MACHIP_BAD_ARG, "the exchange needs a connected fixed graph: with beta = " + std::to_string(h->beta) +
                                        " the removal's 1 - s_e can be of the order of beta");
    if (k < 1 || k >= h->m)
        return fail(MACHIP_BAD_ARG, "k must be in [1, m - 1] (k = " + std::to_string((long long)k) + ", m = " + std::to_string(h->m) + " candidates)");
    std::vector<char> seen((size_t)h->m, 0);
    for (int64_t q = 0; q < k; ++q) {
        const int e = sel_in[q];
        if (e < 0 || e >= h->m)
            return fail(MACHIP_BAD_ARG, "sel_in[" + std::to_string((long long)q) + "] = " + std::to_string(e) + " is outside [0, m = " + std::to_string(h->m) + ")");
        if (seen[(size_t)e]) return fail(MACHIP_BAD_ARG, "sel_in names candidate " + std::to_string(e) + " more than once (a repeated index)");
        seen[(size_t)e] = 1;
    }
    sorted_out.clear();
    for (int e = 0; e < h->m; ++e) if (seen[(size_t)e]) sorted_out.push_back(e);
    return MACHIP_OK;
}

// The bookkeeping of one swap on the host's copy of the rows: row `row` held e, now holds f.
inline int esp_xch_apply(std::vector<int>& rowe, std::vector<char>& in_sel, int row, int e, int f) {
    if (row < 0 || row >= (int)rowe.size() || rowe[(size_t)row] != e || f < 0 || f >= (int)in_sel.size() || !in_sel[(size_t)e] || in_sel[(size_t)f])
        return fail(MACHIP_NOT_CONVERGED, "exchange: the round's winner does not fit the selection (row " + std::to_string(row) + ", out " +
                                         std::to_string(e) + ", in " + std::to_string(f) + ")");
    rowe[(size_t)row] = f;
    in_sel[(size_t)e] = 0;
    in_sel[(size_t)f] = 1;
    return MACHIP_OK;
}

// The call's state: K rows of T, the partials, the swaps' ratios.  Made by the first exchange call on a handle, grown by a later
// one that needs more, freed by machip_esp_destroy.  T is refused when it exceeds the device's free memory (or option
// esp_xch_max_mb, a cap in MiB).  ld: the leading dimension of T's rows (the handle's Sigma; esp_exchange_edge.h: the relaxation's).
inline int esp_xch_prepare(EspXch*& x, size_t K, size_t parts, size_t swaps, size_t ld) {
    if (!x) x = new EspXch();
    if (x->rows < K) {
        if (x->T) { (void)hipFree(x->T); x->T = nullptr; x->rows = 0; }
        if (x->rowe) { (void)hipFree(x->rowe); x->rowe = nullptr; }
        const size_t need = K * ld * sizeof(double);
        if (K * ld >= ((size_t)1 << 31))      // (the row kernels launch K x ld threads; a pair pass of that size is out of the regime anyway)
            return fail(MACHIP_BAD_ARG, "the exchange keeps one row of Sigma per selected edge and takes K x ld < 2^31: K x ld x 8 = " +
                                            std::to_string(K) + " x " + std::to_string(ld) + " x 8 = " + std::to_string(need) + " bytes is beyond it");
        size_t avail = 0, total = 0;
        HIP_TRY(hipMemGetInfo(&avail, &total));
        const long cap_mb = default_options().get(kOpt_esp_xch_max_mb, 0);
        if (cap_mb > 0) avail = std::min(avail, (size_t)cap_mb << 20);
        if (need > avail)
            return fail(MACHIP_BAD_ARG, "the exchange keeps one row of Sigma per selected edge: K x ld x 8 = " + std::to_string(K) + " x " +
                                            std::to_string(ld) + " x 8 = " + std::to_string(need) + " bytes, more than the " +
                                            std::to_string(avail) + " bytes available" + (cap_mb > 0 ? " (option esp_xch_max_mb)" : " on the device"));
        ST_TRY(dev_alloc(&x->T, K * ld));
        ST_TRY(dev_alloc(&x->rowe, K));
        x->rows = K;
    }
    if (x->parts < parts) {
        if (x->pv) { (void)hipFree(x->pv); x->pv = nullptr; }
        if (x->pf) { (void)hipFree(x->pf); x->pf = nullptr; }
        x->parts = 0;
        ST_TRY(dev_alloc(&x->pv, parts)); ST_TRY(dev_alloc(&x->pf, parts));
        x->parts = parts;
    }
    if (x->swaps < swaps) {
        if (x->ratio) { (void)hipFree(x->ratio); x->ratio = nullptr; }
        x->swaps = 0;
        ST_TRY(dev_alloc(&x->ratio, swaps));
        x->swaps = swaps;
    }
    if (!x->scale) ST_TRY(dev_alloc(&x->scale, 1));
    if (!x->best) ST_TRY(dev_alloc(&x->best, 1));
    return MACHIP_OK;
}

// Device time per phase of the exchange (option esp_xch_profile): events between the phases, read after the round's own
// synchronisation.  Interval q lies between marks q - 1 and q and belongs to the phase mark q names (-1: nobody's -- the host waited).
enum { kXchLoad = 1, kXchPairs = 2, kXchTrows = 3, kXchSteps = 4, kXchFolds = 5 };
struct XchClock {
    machip_esp* h;
    bool on;
    size_t base, used = 0;
    std::vector<int> tag;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    int mark(int phase) {
        if (!on) return MACHIP_OK;
        ST_TRY(h->events(base + used + 1));
        HIP_TRY(hipEventRecord(h->ev[base + used], h->stream));
        tag.push_back(phase);
        ++used;
        return MACHIP_OK;
    }
    int collect() {      // (the stream is idle)
        for (size_t q = 1; q < used; ++q) {
            if (tag[q] < 0) continue;
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, h->ev[base + q - 1], h->ev[base + q]));
            acc[tag[q]] += ms;
        }
        used = 0;
        tag.clear();
        return MACHIP_OK;
    }
};

// What esp_xch_run works on: the dense handle's Sigma (EspXchDense) or the relaxation's R (esp_exchange_edge.h).  Next to these
// fields a space has load(&S): the matrix at its start; pairs(): the round's pair pass; entered(e, j): after an insertion's
// update; finish(j): the handle's own bookkeeping.
struct EspXchSpace {
    EspView V;                    // the candidates (and seeds) as the kernels see them
    EspXch* X = nullptr;
    int K = 0, P = 0, fold = 0;   // rows of T, workgroups of a score pass, columns of V.Zb
    int chunks = 0, per = 0;      // the pair pass: slices of the candidates per row and their length
    int sel_count = 0;            // entries of V.sel to clear
    int seeds = 0;                // columns m .. m + seeds: forced picks ahead of the K given ones
};

// The exchange from the selection `rowe` (ascending): the load -- the matrix, the scores, the seeds and the K given edges as
// forced picks, then T -- and the rounds.  Per round the pair pass, the 24-byte read-back, and the two steps of the winning swap.
template <class Space>
inline int esp_xch_run(machip_esp* h, Space& sp, std::vector<int>& rowe, int64_t max_swaps, double min_gain, int32_t* sel_out, int32_t* out_idx,
                       int32_t* in_idx, double* ratio, int64_t* n_swaps, int32_t* converged, double* t_ms) {
    const EspView& V = sp.V; EspXch* X = sp.X;
    const int K = sp.K, m = h->m, B = sp.fold, P = sp.P, ld = V.ld, zg = esp_rows_grid(ld), tiles = ld / kGjT;
    ST_TRY(h->events(2));
    XchClock clk{h, default_options().get(kOpt_esp_xch_profile, 0) != 0, 2};
    hipStream_t st = h->stream;
    std::vector<char> in_sel((size_t)m, 0);
    for (int e : rowe) in_sel[(size_t)e] = 1;
    double* S = nullptr;
    int j = 0;      // columns of Zb pending
    // one rank-1 update: the z of e into Zb[:, j], all scores, T's rows (with_rows), the fold when Zb is full
    auto step = [&](int e, int mode, double* rt, bool with_rows, int xrow, int f_in) -> int {
        k_esp_xch_step<<<zg, kBlock, 0, st>>>(V, S, j, e, mode, rt, X->scale);
        k_esp_update<<<P, kBlock, 0, st>>>(V, j);
        if (mode > 0) sp.entered(e, j);
        if (with_rows) ST_TRY(clk.mark(kXchSteps));      // (the load is one interval, marked at its end)
        if (with_rows) {
            k_esp_xch_tupdate<<<dim3((unsigned)K, (unsigned)zg), kBlock, 0, st>>>(V, X->T, X->rowe, j, xrow, f_in, X->scale);
            ST_TRY(clk.mark(kXchTrows));
        }
        if (++j == B) {
            k_esp_fold<<<dim3(tiles, tiles), 256, 0, st>>>(S, V.Zb, V.cb, ld, B);
            j = 0;
            if (with_rows) ST_TRY(clk.mark(kXchFolds));
        }
        return MACHIP_OK;
    };
    HIP_TRY(hipEventRecord(h->ev[0], st));
    ST_TRY(clk.mark(-1));
    ST_TRY(sp.load(&S));
    HIP_TRY(hipMemsetAsync(V.sel, 0, sizeof(int) * (size_t)sp.sel_count, st));
    HIP_TRY(hipMemsetAsync(V.bad, 0, sizeof(int), st));
    HIP_TRY(hipMemcpyAsync(X->rowe, rowe.data(), sizeof(int) * (size_t)K, hipMemcpyHostToDevice, st));
    k_esp_scores<<<P, kBlock, 0, st>>>(V, S, 0);
    for (int q = 0; q < sp.seeds; ++q) ST_TRY(step(m + q, 1, nullptr, false, -1, -1));
    for (int q = 0; q < K; ++q) ST_TRY(step(rowe[(size_t)q], 1, nullptr, false, -1, -1));
    if (max_swaps > 0) k_esp_xch_tbuild<<<dim3((unsigned)K, (unsigned)zg), kBlock, 0, st>>>(V, S, j, X->rowe, X->T);
    HIP_TRY(hipGetLastError());
    ST_TRY(clk.mark(kXchLoad));
    int64_t t = 0;
    int hbad = 0;
    for (; t < max_swaps; ++t) {
        sp.pairs();
        k_esp_xch_argmax<<<1, kBlock, 0, st>>>(V, X->rowe, X->pv, X->pf, K * sp.chunks, sp.chunks, X->best);
        HIP_TRY(hipGetLastError());
        ST_TRY(clk.mark(kXchPairs));
        EspXchBest b;
        HIP_TRY(hipMemcpyAsync(&b, X->best, sizeof(b), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&hbad, V.bad, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        ST_TRY(clk.collect());
        if (hbad) break;
        if (b.val - 1.0 <= min_gain) { *converged = 1; break; }
        ST_TRY(esp_xch_apply(rowe, in_sel, b.row, b.e, b.f));
        out_idx[t] = b.e;
        in_idx[t] = b.f;
        ST_TRY(clk.mark(-1));
        ST_TRY(step(b.e, -1, X->ratio + t, true, b.row, -1));
        ST_TRY(step(b.f, +1, X->ratio + t, true, b.row, b.f));
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(h->ev[1], st));
    if (t > 0) HIP_TRY(hipMemcpyAsync(ratio, X->ratio, sizeof(double) * (size_t)t, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&hbad, V.bad, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    ST_TRY(clk.collect());
    sp.finish(j);
    if (hbad)
        return fail(MACHIP_NOT_CONVERGED, "exchange: 1 - s_e of a removal or 1 + s_f of an insertion is not positive, or no finite Delta (the selection holds a bridge of the graph, or lost numerically)");
    *n_swaps = t;
    for (int e = 0, q = 0; e < m; ++e) if (in_sel[(size_t)e]) sel_out[q++] = e;
    if (t_ms) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
        t_ms[0] = ms;
        for (int q = 1; q < 6; ++q) t_ms[q] = clk.acc[q];
    }
    return MACHIP_OK;
}

// the dense handle's space: Sigma from Sigma0; a row of T in LDS while the runtime grants it, from global memory otherwise
struct EspXchDense : EspXchSpace {
    machip_esp* h;
    size_t row_bytes;
    bool lds;
    ESP_INLINE int load(double** S) { h->live = false; h->pending = 0; *S = h->sig; return h->load_sigma0(); }      // (the handle's state: after the events exist)
    ESP_INLINE void pairs() {
        const dim3 grid((unsigned)K, (unsigned)chunks);
        if (lds) {
            k_esp_xch_pairs<true><<<grid, kBlock, row_bytes, h->stream>>>(V, X->T, X->rowe, per, X->pv, X->pf);
            if (hipGetLastError() != hipSuccess) lds = false;      // (the launch was refused, nothing ran: global-memory rows from here on)
        }
        if (!lds) k_esp_xch_pairs<false><<<grid, kBlock, 0, h->stream>>>(V, X->T, X->rowe, per, X->pv, X->pf);
    }
    ESP_INLINE void entered(int, int) {}
    ESP_INLINE void finish(int j) { h->pending = j; h->live = true; }
};

// machip_esp_exchange after its checks: T and the partials, the LDS decision, the space, the rounds
inline int esp_exchange(machip_esp* h, int64_t k, std::vector<int>& rowe, int64_t max_swaps, double min_gain, int32_t* sel_out, int32_t* out_idx,
                        int32_t* in_idx, double* ratio, int64_t* n_swaps, int32_t* converged, double* t_ms) {
    EspXchDense sp;
    sp.h = h; sp.K = (int)k; sp.P = h->grid_m(); sp.fold = h->fold; sp.sel_count = h->m;
    sp.chunks = std::max(1, std::min((h->m + kBlock - 1) / kBlock, (kEspXchTargetGroups + sp.K - 1) / sp.K));
    sp.per = (h->m + sp.chunks - 1) / sp.chunks;
    const long lds_kb = std::max(0l, std::min<long>(default_options().get(kOpt_esp_xch_lds_kb, kEspXchLdsDefaultKb), kEspXchLdsMaxKb));
    sp.row_bytes = sizeof(double) * (size_t)h->ld;
    sp.lds = sp.row_bytes <= (size_t)lds_kb * 1024;
    ST_TRY(esp_xch_prepare(h->xc, (size_t)sp.K, (size_t)sp.K * (size_t)sp.chunks, (size_t)std::max<int64_t>(max_swaps, 1), (size_t)h->ld));
    if (sp.lds && sp.row_bytes > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_esp_xch_pairs<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp.row_bytes) != hipSuccess) {
        (void)hipGetLastError();
        sp.lds = false;      // (the runtime does not grant the row: the global-memory rows give the same bits)
    }
    sp.X = h->xc; sp.V = h->view();
    return esp_xch_run(h, sp, rowe, max_swaps, min_gain, sel_out, out_idx, in_idx, ratio, n_swaps, converged, t_ms);
}

}  // namespace machip
