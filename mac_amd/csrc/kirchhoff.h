// mac_amd/csrc/kirchhoff.h -- GreedyKirchhoff: greedy A-optimal edge selection on the dense forms of a machip_esp handle.
//
// A-optimal selection minimises  tr L^+  (the total effective resistance, Kirchhoff index / n).  With node 0 pinned,
// Sigma = L_red^-1 (esp.h) and Sigma~ = Sigma padded with a zero row / column for node 0:   tr L^+ = tr Sigma - (1^T Sigma 1) / n.
// Candidate e = (u, v, w) keeps  q_e = |z_e|^2,  t_e = 1^T z_e  (z_e = Sigma~ a_e)  and GreedyESP's  s_e = w a_e^T Sigma~ a_e;
// adding it lowers tr L^+ by
//     gain_e = w_e (q_e - t_e^2 / n) / (1 + s_e).
// A step takes the unselected candidate of largest gain (ties: lowest index, esp_better).  With f the pick, z = Sigma~ a_f,
// c = w_f / (1 + s_f), y = Sigma z (Sigma BEFORE this pick's update = the folded Sigma minus the pending columns b < j) and
// d_e = z_u - z_v:
//     q_e <- q_e - 2 c d_e (y_u - y_v) + c^2 d_e^2 |z|^2,    t_e <- t_e - c d_e (1^T z),    s_e <- s_e - w_e c d_e^2,
//     Sigma <- Sigma - c z z^T   (deferred through Zb and folded every `fold` picks: esp.h's k_esp_fold).
// Per pick: k_kir_z (z into Zb[:, j], the step's record), k_kir_dots (the pending columns' c_b Zb[:, b]^T z, |z|^2 and 1^T z),
// k_kir_y (the dense symmetric product, 8 ld^2 bytes: the criterion's inherent cost), k_kir_update (the three recurrences, the
// gains and the argmax partials), k_esp_argmax.  Every reduction has a fixed order: runs repeat bit for bit.
// The same loop applies a given selection as forced picks (machip_esp_kirchhoff_eval): no product, GreedyESP's k_esp_update.
// DESIGN section 26.
#pragma once
#include "esp_select.h"

namespace machip {

constexpr int kKirRows = 4;      // rows of Sigma one wave of the product owns: every z entry it loads serves four rows

// what the criterion keeps beside GreedyESP's arrays, made by the first Kirchhoff call on a handle
struct EspKir {
    double *q = nullptr, *t = nullptr, *g = nullptr;      // per candidate: |z_e|^2, 1^T z_e, the gain
    double *y = nullptr;                                  // Sigma z of the current pick (ld)
    double *beta = nullptr;                               // c_b Zb[:, b]^T z of the pending columns (kEspMaxFold)
    double *zs = nullptr;                                 // {|z|^2, 1^T z} of the current pick
    double *rows = nullptr;                               // trace: the row sums (ld), then the diagonal (ld)
    double *tr = nullptr;                                 // trace: the two results of machip_esp_kirchhoff_eval
    int* forced = nullptr;                                // the picks of machip_esp_kirchhoff_eval (m)
};

struct KirView {
    double *q, *t, *g, *y, *beta, *zs;
    double n;      // num_nodes
};

__device__ __forceinline__ double kir_gain(double w, double q, double t, double s, double n) { return w * (q - t * t / n) / (1.0 + s); }

// ---- start pass: q_e, t_e, s_e and the gain of all m candidates from rows u, v of S (no pending block); one wave per candidate,
// lane l sums columns l, l + 64, ... < n' (the identity beyond n' stays out), then the butterfly: a pair and its reverse give the
// same bits (z -> -z exactly), a self-loop has z = 0 and gain 0.  mask != 0: partials of the argmax over the unselected.
// grid = P <= kEspGrid workgroups ----
__global__ __launch_bounds__(kBlock) void k_kir_start(EspView V, KirView Q, const double* __restrict__ S, int mask) {
    __shared__ double sv[kBlock / kWave];
    __shared__ int si[kBlock / kWave];
    const int lane = threadIdx.x & 63, nw = gridDim.x * (kBlock / kWave);
    double bv = -INFINITY;
    int bi = INT_MAX;
    for (int e = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6); e < V.m; e += nw) {
        const int u = V.cu[e], v = V.cv[e];
        const double* ru = S + (size_t)max(u, 0) * V.ld;
        const double* rv = S + (size_t)max(v, 0) * V.ld;
        double q = 0.0, t = 0.0;
        for (int i = lane; i < V.np; i += kWave) {
            const double z = (u >= 0 ? ru[i] : 0.0) - (v >= 0 ? rv[i] : 0.0);
            q = __builtin_fma(z, z, q);
            t += z;
        }
        q = wave_sum(q);
        t = wave_sum(t);
        if (lane == 0) {
            const double w = V.cw[e], s = esp_score(S, V.ld, u, v, w), g = kir_gain(w, q, t, s, Q.n);
            V.s[e] = s; Q.q[e] = q; Q.t[e] = t; Q.g[e] = g;
            if (mask && !V.sel[e]) esp_better(bv, bi, g, e);
        }
    }
    if (!mask) return;
    esp_block_argmax(bv, bi, sv, si);
    if (threadIdx.x == 0) { V.pv[blockIdx.x] = bv; V.pi[blockIdx.x] = bi; }
}

// the step's record (esp_record_step's sibling): best->val is the winner's gain, c comes from its current score
__device__ __forceinline__ void kir_record_step(const EspView& V, int e, int j, int k) {
    V.cb[j] = V.cw[e] / (1.0 + V.s[e]);
    V.order[k] = e;
    V.gain[k] = V.best->val;
    V.sel[e] = 1;
}

// ---- the z of the step's winner into Zb[:, j] (k_esp_z with this criterion's record).  grid = ceil(ld / 256) ----
__global__ __launch_bounds__(kBlock) void k_kir_z(EspView V, const double* __restrict__ S, int j, int k) {
    __shared__ double alpha[kEspMaxFold];
    const int e = V.best->idx;
    const int u = V.cu[e], v = V.cv[e];
    esp_z_alpha(V, u, v, j, alpha);
    __syncthreads();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < V.ld) V.Zb[(size_t)j * V.ld + i] = esp_z_entry(V, S, u, v, j, alpha, i);
    if (blockIdx.x == 0 && threadIdx.x == 0) kir_record_step(V, e, j, k);
}

// ---- forced pick k of machip_esp_kirchhoff_eval in the argmax's place ----
__global__ void k_kir_force(EspView V, const int* __restrict__ forced, int k) {
    if (threadIdx.x == 0) { V.best->idx = forced[k]; V.best->val = 0.0; }
}

// ---- beta_b = c_b Zb[:, b]^T z for the pending columns b < j (workgroup b), |z|^2 and 1^T z (workgroup j); z = Zb[:, j], whose
// padding rows are 0.  grid = j + 1; one workgroup per sum, thread t takes t, t + 256, ...: one fixed order ----
__global__ __launch_bounds__(kBlock) void k_kir_dots(EspView V, KirView Q, int j) {
    __shared__ double sm[kBlock / kWave];
    const double* z = V.Zb + (size_t)j * V.ld;
    const int b = blockIdx.x;
    if (b < j) {
        const double* zc = V.Zb + (size_t)b * V.ld;
        double a = 0.0;
        for (int i = threadIdx.x; i < V.ld; i += kBlock) a = __builtin_fma(zc[i], z[i], a);
        a = block_sum(a, sm);
        if (threadIdx.x == 0) Q.beta[b] = V.cb[b] * a;
    } else {
        double zz = 0.0, zt = 0.0;
        for (int i = threadIdx.x; i < V.ld; i += kBlock) {
            const double x = z[i];
            zz = __builtin_fma(x, x, zz);
            zt += x;
        }
        zz = block_sum(zz, sm);
        zt = block_sum(zt, sm);
        if (threadIdx.x == 0) { Q.zs[0] = zz; Q.zs[1] = zt; }
    }
}

// ---- y = S z - Zb[:, :j] beta: the dense symmetric product, row-major, row i of S contiguous.  A wave owns kKirRows rows
// (ld is a multiple of 64: no row is out of bounds): lane l takes the column pairs l, l + 64, ... of all of them, so a z pair
// (from L2: at ld = 32 768 z does not fit in LDS) is loaded once per four pairs of S; then the pending columns' correction, lane
// l columns l, l + 64, ...; then the butterfly.  Columns n'..ld contribute exact zeros (z is 0 there).  grid = ld / 16 ----
__global__ __launch_bounds__(kBlock) void k_kir_y(EspView V, KirView Q, const double* __restrict__ S, int j) {
    const int lane = threadIdx.x & 63;
    const int r0 = (blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6)) * kKirRows;
    const size_t ld = (size_t)V.ld;
    const double2* __restrict__ z2 = reinterpret_cast<const double2*>(V.Zb + (size_t)j * ld);
    const double2* __restrict__ s2 = reinterpret_cast<const double2*>(S + (size_t)r0 * ld);
    const int half = V.ld >> 1;
    double acc[kKirRows];
#pragma unroll
    for (int r = 0; r < kKirRows; ++r) acc[r] = 0.0;
#pragma unroll 2
    for (int c = lane; c < half; c += kWave) {
        const double2 z = z2[c];
#pragma unroll
        for (int r = 0; r < kKirRows; ++r) {
            const double2 a = s2[(size_t)r * half + c];
            acc[r] = __builtin_fma(a.x, z.x, acc[r]);
            acc[r] = __builtin_fma(a.y, z.y, acc[r]);
        }
    }
    for (int b = lane; b < j; b += kWave) {
        const double nb = -Q.beta[b];
        const double* zc = V.Zb + (size_t)b * ld + r0;
#pragma unroll
        for (int r = 0; r < kKirRows; ++r) acc[r] = __builtin_fma(nb, zc[r], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < kKirRows; ++r) {
        const double y = wave_sum(acc[r]);
        if (lane == 0) Q.y[r0 + r] = y;
    }
}

// ---- the three recurrences for all m, z = Zb[:, j], y = Q.y; the gains; partials of the argmax over the unselected ----
__global__ __launch_bounds__(kBlock) void k_kir_update(EspView V, KirView Q, int j) {
    __shared__ double sv[kBlock / kWave];
    __shared__ int si[kBlock / kWave];
    const double* z = V.Zb + (size_t)j * V.ld;
    const double c = V.cb[j], zz = Q.zs[0], zt = Q.zs[1];
    double bv = -INFINITY;
    int bi = INT_MAX;
    for (int e = blockIdx.x * kBlock + threadIdx.x; e < V.m; e += gridDim.x * kBlock) {
        const int u = V.cu[e], v = V.cv[e];
        const double d = (u >= 0 ? z[u] : 0.0) - (v >= 0 ? z[v] : 0.0);
        const double dy = (u >= 0 ? Q.y[u] : 0.0) - (v >= 0 ? Q.y[v] : 0.0);
        const double w = V.cw[e], cd = c * d;
        const double q = Q.q[e] - 2.0 * cd * dy + cd * cd * zz;
        const double t = Q.t[e] - cd * zt;
        const double s = V.s[e] - w * c * d * d;
        const double g = kir_gain(w, q, t, s, Q.n);
        Q.q[e] = q; Q.t[e] = t; V.s[e] = s; Q.g[e] = g;
        if (!V.sel[e]) esp_better(bv, bi, g, e);
    }
    esp_block_argmax(bv, bi, sv, si);
    if (threadIdx.x == 0) { V.pv[blockIdx.x] = bv; V.pi[blockIdx.x] = bi; }
}

// ---- trace, stage 1: the row sums over columns < n' and the diagonal of rows < n' of a folded S; one wave per row, lane l
// columns l, l + 64, ...  grid = ceil(n' / 4) ----
__global__ __launch_bounds__(kBlock) void k_kir_rows(const double* __restrict__ S, double* __restrict__ rows, int np, int ld) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (i >= np) return;
    const double* r = S + (size_t)i * ld;
    double a = 0.0;
    for (int c = lane; c < np; c += kWave) a += r[c];
    a = wave_sum(a);
    if (lane == 0) { rows[i] = a; rows[ld + i] = r[i]; }
}
// ---- trace, stage 2: out = tr S - (1^T S 1) / n from stage 1's arrays; one workgroup, thread t takes t, t + 256, ... ----
__global__ __launch_bounds__(kBlock) void k_kir_trace(const double* __restrict__ rows, int np, int ld, double n, double* __restrict__ out) {
    __shared__ double sm[kBlock / kWave];
    double a = 0.0, d = 0.0;
    for (int i = threadIdx.x; i < np; i += kBlock) { a += rows[i]; d += rows[ld + i]; }
    a = block_sum(a, sm);
    d = block_sum(d, sm);
    if (threadIdx.x == 0) *out = d - a / n;
}

// ---- host side ----

inline void esp_kir_release(machip_esp* h) {
    EspKir* k = h->kr;
    if (!k) return;
    void* bufs[] = {k->q, k->t, k->g, k->y, k->beta, k->zs, k->rows, k->tr, k->forced};
    for (void* p : bufs) if (p) (void)hipFree(p);
    delete k;
    h->kr = nullptr;
}

// The refusals every Kirchhoff entry point shares, decided from the handle alone: the criterion needs Sigma, and a finite index.
inline int kir_check(const machip_esp* h) {
    if (h->matrix_free())
        return fail(MACHIP_BAD_ARG, "GreedyKirchhoff needs the dense inverse Sigma: not available on a handle made with MACHIP_ESP_MATRIX_FREE "
                                    "(chain, spanning-tree or edge-relax)");
    if (h->beta != 0.0)
        return fail(MACHIP_DISCONNECTED, "the fixed graph is disconnected (beta != 0): its Kirchhoff index is infinite");
    return MACHIP_OK;
}

// the criterion's arrays, at the first call
inline int kir_state(machip_esp* h) {
    if (h->kr) return MACHIP_OK;
    h->kr = new EspKir();
    EspKir* k = h->kr;
    const size_t ms = (size_t)std::max(h->m, 1), ld = (size_t)h->ld;
    ST_TRY(dev_alloc(&k->q, ms)); ST_TRY(dev_alloc(&k->t, ms)); ST_TRY(dev_alloc(&k->g, ms)); ST_TRY(dev_alloc(&k->forced, ms));
    ST_TRY(dev_alloc(&k->y, ld)); ST_TRY(dev_alloc(&k->beta, (size_t)kEspMaxFold)); ST_TRY(dev_alloc(&k->zs, 2));
    ST_TRY(dev_alloc(&k->rows, 2 * ld)); ST_TRY(dev_alloc(&k->tr, 2));
    return MACHIP_OK;
}

inline KirView kir_view(const machip_esp* h) {
    const EspKir* k = h->kr;
    return KirView{k->q, k->t, k->g, k->y, k->beta, k->zs, (double)h->n};
}

// workgroups of the start pass (one wave per candidate)
inline int kir_start_grid(const machip_esp* h) { return std::max(1, std::min(kEspGrid, (h->m + kBlock / kWave - 1) / (kBlock / kWave))); }

// *out (device) = tr L^+ of the graph whose folded inverse is S
inline void kir_trace(machip_esp* h, const double* S, double* out) {
    k_kir_rows<<<(h->np + kBlock / kWave - 1) / (kBlock / kWave), kBlock, 0, h->stream>>>(S, h->kr->rows, h->np, h->ld);
    k_kir_trace<<<1, kBlock, 0, h->stream>>>(h->kr->rows, h->np, h->ld, (double)h->n, out);
}

// One run from Sigma0 (the caller has checked: m >= K >= 1), the shape of esp_select_run.  forced == nullptr: the greedy -- per pick
// k_kir_z, k_kir_dots, k_kir_y and, unless it is the last, k_kir_update and k_esp_argmax.  forced (device, K indices): those picks
// in that order -- k_kir_z, then k_esp_update (the scores alone decide c) and k_kir_force.  A full Zb is folded either way.
inline int kir_run(machip_esp* h, int nb, const int64_t* ks, const int* forced, int32_t* order_out, double* gain_out, double* t_ms_out) {
    const int K = (int)ks[nb - 1], B = h->fold, P = h->grid_m(), Ps = kir_start_grid(h), rg = esp_rows_grid(h->ld);
    ST_TRY(h->events((size_t)nb + 1));
    const EspView V = h->view();
    const KirView Q = kir_view(h);
    hipStream_t st = h->stream;
    h->live = false;
    HIP_TRY(hipEventRecord(h->ev[0], st));
    ST_TRY(h->load_sigma0());
    HIP_TRY(hipMemsetAsync(h->sel, 0, sizeof(int) * (size_t)h->m, st));
    HIP_TRY(hipMemsetAsync(h->bad, 0, sizeof(int), st));
    if (forced) {
        k_esp_scores<<<P, kBlock, 0, st>>>(V, h->sig, 0);
        k_kir_force<<<1, kWave, 0, st>>>(V, forced, 0);
    } else {
        k_kir_start<<<Ps, kBlock, 0, st>>>(V, Q, h->sig, 1);
        k_esp_argmax<<<1, kBlock, 0, st>>>(V, Ps);
    }
    for (int k = 0, b = 0; k < K; ++k) {
        const int j = k % B;
        k_kir_z<<<rg, kBlock, 0, st>>>(V, h->sig, j, k);
        if (k + 1 < K) {
            if (forced) {
                k_esp_update<<<P, kBlock, 0, st>>>(V, j);
                k_kir_force<<<1, kWave, 0, st>>>(V, forced, k + 1);
            } else {
                k_kir_dots<<<j + 1, kBlock, 0, st>>>(V, Q, j);
                k_kir_y<<<h->ld / (kKirRows * (kBlock / kWave)), kBlock, 0, st>>>(V, Q, h->sig, j);
                k_kir_update<<<P, kBlock, 0, st>>>(V, Q, j);
                k_esp_argmax<<<1, kBlock, 0, st>>>(V, P);
            }
        }
        if (j == B - 1) h->fold_into(h->sig, B);
        while (b < nb && ks[b] == k + 1) HIP_TRY(hipEventRecord(h->ev[1 + b++], st));
    }
    HIP_TRY(hipGetLastError());
    h->pending = K % B;
    int hbad = 0;
    if (order_out) HIP_TRY(hipMemcpyAsync(order_out, h->order, sizeof(int) * (size_t)K, hipMemcpyDeviceToHost, st));
    if (gain_out) HIP_TRY(hipMemcpyAsync(gain_out, h->gain, sizeof(double) * (size_t)K, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&hbad, h->bad, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (t_ms_out)
        for (int i = 0; i < nb; ++i) {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1 + i]));
            t_ms_out[i] = ms;
        }
    h->live = true;
    if (hbad) return fail(MACHIP_NOT_CONVERGED, "no finite gain among the unselected candidates");
    return MACHIP_OK;
}

// machip_esp_kirchhoff_select after its checks
inline int kir_select(machip_esp* h, int nb, const int64_t* ks, int32_t* order_out, double* gain_out, double* t_ms_out) {
    ST_TRY(kir_state(h));
    return kir_run(h, nb, ks, nullptr, order_out, gain_out, t_ms_out);
}

// machip_esp_kirchhoff_gains after its checks: on the last run's state (what is pending is folded) or the fixed graph
inline int kir_gains(machip_esp* h, double* gains_out) {
    ST_TRY(kir_state(h));
    double* S = h->live ? h->sig : h->sig0;
    if (h->live && h->pending) { h->fold_into(S, h->pending); h->pending = 0; }
    if (h->m) k_kir_start<<<kir_start_grid(h), kBlock, 0, h->stream>>>(h->view(), kir_view(h), S, 0);
    HIP_TRY(hipGetLastError());
    if (h->m) HIP_TRY(hipMemcpyAsync(gains_out, h->kr->g, sizeof(double) * (size_t)h->m, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MACHIP_OK;
}

// the selection of machip_esp_kirchhoff_eval, checked on the host: in range, no candidate twice
inline int kir_eval_check(const machip_esp* h, int64_t nsel, const int32_t* idx) {
    if (nsel < 0 || nsel > h->m) return fail(MACHIP_BAD_ARG, "the selection must hold between 0 and m candidates");
    if (nsel && !idx) return fail(MACHIP_BAD_ARG, "idx is NULL");
    std::vector<char> seen((size_t)std::max(h->m, 1), 0);
    for (int64_t i = 0; i < nsel; ++i) {
        if (idx[i] < 0 || idx[i] >= h->m) return fail(MACHIP_BAD_ARG, "selected candidate index out of range");
        if (seen[(size_t)idx[i]]) return fail(MACHIP_BAD_ARG, "candidate " + std::to_string(idx[i]) + " is selected twice");
        seen[(size_t)idx[i]] = 1;
    }
    return MACHIP_OK;
}

// machip_esp_kirchhoff_eval after its checks: out2 = {tr L^+ of the fixed graph, tr L^+ with the selection}, both by the trace kernels
inline int kir_eval(machip_esp* h, int64_t nsel, const int32_t* idx, double* out2) {
    ST_TRY(kir_state(h));
    double* tr = h->kr->tr;
    if (nsel) {
        HIP_TRY(hipMemcpyAsync(h->kr->forced, idx, sizeof(int) * (size_t)nsel, hipMemcpyHostToDevice, h->stream));
        ST_TRY(kir_run(h, 1, &nsel, h->kr->forced, nullptr, nullptr, nullptr));
        if (h->pending) { h->fold_into(h->sig, h->pending); h->pending = 0; }
    }
    kir_trace(h, h->sig0, tr);
    kir_trace(h, nsel ? h->sig : h->sig0, tr + 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out2, tr, sizeof(double) * 2, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MACHIP_OK;
}

}  // namespace machip
