// mac_amd/csrc/esp_free.h -- GreedyESP without a dense Sigma: the matrix-free route for chain-fixed graphs.
//
// When the fixed edges are the chain (i, i+1), Sigma0_ab = R[min(a, b)] (R = prefix sums of 1 / w_link, esp.h), so a row of
// Sigma0 needs no storage.  The rank-1 updates of the picks are never folded: all of them stay in the history Zb (ld x K, column
// b at Zb + b ld, with their c's), and the z of pick j is
//     z_i = R[min(u, i)] - R[min(v, i)] - sum_{b < j} alpha_b Zb[i, b],   alpha_b = c_b (Zb[u, b] - Zb[v, b])      (node-0 terms 0)
// -- k_esp_z's formula with the two Sigma rows taken from R and an unbounded pending count.  State: 8 ld K bytes instead of
// 2 x 8 ld^2; the price is the tall dependent product, 8 ld j bytes streamed at pick j (about 4 ld K^2 over a run).
//
// k_esp_free_z: a workgroup owns 512 rows (a double2 per lane: 16-byte loads, 1 KiB per wave instruction) and one slice of the
// columns; the alphas of the slice are staged in LDS 1 024 at a time; a row's products are one FMA chain, columns ascending, as
// esp_z_entry does.  n' = 40 000 is only 79 such workgroups, so the columns are cut into S slices (grid = row blocks x S, about
// 512 workgroups): slice 0 starts its chain from the Sigma0 term, the others from 0, the partial sums go to `part` (S x ld) and
// k_esp_free_zsum adds them in ascending slice order -- no atomics, the order is a function of (ld, j, option esp_free_split)
// alone, so runs repeat bit for bit.  With S = 1 (short histories, or esp_free_split = 1) the kernel writes z itself and the
// arithmetic per entry is that of the dense chain form with fold > K.
// Scores and updates: k_esp_free_scores is k_esp_scores with Sigma0's three entries read from R (the same three-term sum, the same
// bits); k_esp_update and k_esp_argmax are reused as they are.  k_esp_free_resist rescores every candidate from R and the history.
// Host side: esp_free_z (the sliced / unsliced launch) and esp_history_reserve, both shared with esp_tree.h; the loop is esp.h's.
#pragma once
#include <string>

#include "esp.h"
#include "plan.h"

namespace machip {

constexpr int kEspFreeRows = 2 * kBlock;     // rows of z per workgroup
constexpr int kEspFreeChunk = 1024;          // alphas staged in LDS per pass (8 KiB)
constexpr int kEspFreeUnroll = 8;            // columns in flight per lane (8 x 16 B); slices are cut at multiples of it
constexpr int kEspFreeWgs = 512;             // workgroups aimed at per pick (2 per CU, 8 KiB in flight per wave)
constexpr int kEspFreeMaxSplit = 32;         // slices of the columns at most (`part` is sized for it)
constexpr int kEspFreeMinCols = 16;          // a slice is not cut below this many columns

// Sigma0_ai = R[min(a, i)], 0 when a is node 0
__device__ __forceinline__ double esp_free_sig0(const double* __restrict__ R, int a, int i) { return a >= 0 ? R[min(a, i)] : 0.0; }

// esp_score on Sigma0 without Sigma0: uu + vv - 2 uv with uu = R[u], vv = R[v], uv = R[min(u, v)]
__device__ __forceinline__ double esp_free_score(const double* __restrict__ R, int u, int v, double w) {
    const double uu = u >= 0 ? R[u] : 0.0;
    const double vv = v >= 0 ? R[v] : 0.0;
    const double uv = (u >= 0 && v >= 0) ? R[min(u, v)] : 0.0;
    return w * (uu + vv - 2.0 * uv);
}

// ---- score pass from R alone (the fixed graph); mask != 0: partials of the argmax over the unselected ----
__global__ __launch_bounds__(kBlock) void k_esp_free_scores(EspView V, const double* __restrict__ R, int mask) {
    __shared__ double sv[kBlock / kWave];
    __shared__ int si[kBlock / kWave];
    double bv = -INFINITY;
    int bi = INT_MAX;
    for (int e = blockIdx.x * kBlock + threadIdx.x; e < V.m; e += gridDim.x * kBlock) {
        const double s = esp_free_score(R, V.cu[e], V.cv[e], V.cw[e]);
        V.s[e] = s;
        if (mask && !V.sel[e]) esp_better(bv, bi, s, e);
    }
    if (!mask) return;
    esp_block_argmax(bv, bi, sv, si);
    if (threadIdx.x == 0) { V.pv[blockIdx.x] = bv; V.pi[blockIdx.x] = bi; }
}

// ---- s_e = w_e (Sigma0 term - sum_{b < j} c_b (Zb[u, b] - Zb[v, b])^2) for all m: every candidate, selected ones included.
// A thread per candidate walks the j columns (the workgroups move through them together: a column is read from L2). ----
__global__ __launch_bounds__(kBlock) void k_esp_free_resist(EspView V, const double* __restrict__ R, int j) {
    const size_t ld = V.ld;
    for (int e = blockIdx.x * kBlock + threadIdx.x; e < V.m; e += gridDim.x * kBlock) {
        const int u = V.cu[e], v = V.cv[e];
        const double uu = u >= 0 ? R[u] : 0.0;
        const double vv = v >= 0 ? R[v] : 0.0;
        const double uv = (u >= 0 && v >= 0) ? R[min(u, v)] : 0.0;
        double acc = 0.0;
        for (int b = 0; b < j; ++b) {
            const double* zc = V.Zb + (size_t)b * ld;
            const double d = (u >= 0 ? zc[u] : 0.0) - (v >= 0 ? zc[v] : 0.0);
            acc = __builtin_fma(V.cb[b] * d, d, acc);
        }
        V.s[e] = V.cw[e] * ((uu + vv - 2.0 * uv) - acc);
    }
}

// ---- the z of the step's winner.  grid = (ceil(ld / 512), S); slice s = blockIdx.y owns the columns [s per, (s + 1) per) of the j
// in the history.  SPLIT = false (S = 1): z into Zb[:, j], workgroup 0 records the step.  SPLIT = true: the slice's partial sum
// into part[s ld ..]; k_esp_free_zsum finishes.  LOADED (esp_tree.h): `R` is not the chain's prefix sums but the Sigma0 row
// difference itself (ld doubles, written by k_esp_tree_row) and slice 0 starts its chain from that value; nothing else differs. ----
template <bool SPLIT, bool LOADED = false>
__global__ __launch_bounds__(kBlock) void k_esp_free_z(EspView V, const double* __restrict__ R, double* __restrict__ part, int j, int k,
                                                       int per) {
    __shared__ double alpha[kEspFreeChunk];
    const int e = V.best->idx;
    const int u = V.cu[e], v = V.cv[e];
    const int s = SPLIT ? (int)blockIdx.y : 0;
    const int b0 = SPLIT ? min(j, s * per) : 0, b1 = SPLIT ? min(j, b0 + per) : j;
    const size_t ld = V.ld;
    const int i = 2 * (blockIdx.x * kBlock + threadIdx.x);      // rows i, i + 1 (ld is a multiple of 64)
    const bool in = i < V.ld;
    double z0 = 0.0, z1 = 0.0;
    if (LOADED) {
        if (s == 0 && in) {
            const double2 x = *reinterpret_cast<const double2*>(R + i);
            z0 = x.x;
            z1 = x.y;
        }
    } else if (s == 0 && in) {
        if (i < V.np) z0 = esp_free_sig0(R, u, i) - esp_free_sig0(R, v, i);
        if (i + 1 < V.np) z1 = esp_free_sig0(R, u, i + 1) - esp_free_sig0(R, v, i + 1);
    }
    for (int c0 = b0; c0 < b1; c0 += kEspFreeChunk) {
        const int cn = min(kEspFreeChunk, b1 - c0);
        __syncthreads();                                         // (the previous chunk's alphas are no longer read)
        for (int b = threadIdx.x; b < cn; b += kBlock) {
            const double* zc = V.Zb + (size_t)(c0 + b) * ld;
            alpha[b] = V.cb[c0 + b] * ((u >= 0 ? zc[u] : 0.0) - (v >= 0 ? zc[v] : 0.0));
        }
        __syncthreads();
        if (!in) continue;
        const double* col = V.Zb + (size_t)c0 * ld + i;
        int b = 0;
        for (; b + kEspFreeUnroll <= cn; b += kEspFreeUnroll) {
            double2 x[kEspFreeUnroll];
#pragma unroll
            for (int q = 0; q < kEspFreeUnroll; ++q) x[q] = *reinterpret_cast<const double2*>(col + (size_t)(b + q) * ld);
#pragma unroll
            for (int q = 0; q < kEspFreeUnroll; ++q) {
                const double a = alpha[b + q];
                z0 = __builtin_fma(-a, x[q].x, z0);
                z1 = __builtin_fma(-a, x[q].y, z1);
            }
        }
        for (; b < cn; ++b) {
            const double2 x = *reinterpret_cast<const double2*>(col + (size_t)b * ld);
            const double a = alpha[b];
            z0 = __builtin_fma(-a, x.x, z0);
            z1 = __builtin_fma(-a, x.y, z1);
        }
    }
    if (SPLIT) {
        if (in) *reinterpret_cast<double2*>(part + (size_t)s * ld + i) = make_double2(z0, z1);
        return;
    }
    if (in) *reinterpret_cast<double2*>(V.Zb + (size_t)j * ld + i) = make_double2(i < V.np ? z0 : 0.0, i + 1 < V.np ? z1 : 0.0);
    if (blockIdx.x == 0 && threadIdx.x == 0) esp_record_step(V, e, j, k);
}

// ---- z = part[0] + part[1] + ... + part[S - 1] (ascending: a fixed order) into Zb[:, j], 0 in the padding rows.
// grid = ceil(ld / 512).  Workgroup 0 records the step. ----
__global__ __launch_bounds__(kBlock) void k_esp_free_zsum(EspView V, const double* __restrict__ part, int S, int j, int k) {
    const size_t ld = V.ld;
    const int i = 2 * (blockIdx.x * kBlock + threadIdx.x);
    if (i < V.ld) {
        double2 z = *reinterpret_cast<const double2*>(part + i);
        for (int s = 1; s < S; ++s) {
            const double2 p = *reinterpret_cast<const double2*>(part + (size_t)s * ld + i);
            z.x += p.x;
            z.y += p.y;
        }
        *reinterpret_cast<double2*>(V.Zb + (size_t)j * ld + i) = make_double2(i < V.np ? z.x : 0.0, i + 1 < V.np ? z.y : 0.0);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) esp_record_step(V, V.best->idx, j, k);
}

// slices of the j columns at pick j: a function of (ld, j, the handle's option) alone
inline int esp_free_slices(const machip_esp* h, int j) {
    const int zg = (h->ld + kEspFreeRows - 1) / kEspFreeRows;
    int S = h->free_split > 0 ? h->free_split : (kEspFreeWgs + zg - 1) / zg;
    S = std::min(std::min(S, kEspFreeMaxSplit), j / kEspFreeMinCols);
    return std::max(S, 1);
}

// The z of a pick through the history's first j columns into column j, recorded as pick k: k_esp_free_z, and k_esp_free_zsum
// when the columns are sliced.  LOADED = false: src = the chain's R; true (esp_tree.h): src = the Sigma0 row difference itself.
template <bool LOADED>
ESP_INLINE void esp_free_z(machip_esp* h, const EspView& V, const double* src, int j, int k) {
    const int zg = (h->ld + kEspFreeRows - 1) / kEspFreeRows;
    const int S = esp_free_slices(h, j);
    if (S == 1) {
        k_esp_free_z<false, LOADED><<<zg, kBlock, 0, h->stream>>>(V, src, nullptr, j, k, 0);
    } else {
        const int per = ((j + S - 1) / S + kEspFreeUnroll - 1) / kEspFreeUnroll * kEspFreeUnroll;
        k_esp_free_z<true, LOADED><<<dim3((unsigned)zg, (unsigned)S), kBlock, 0, h->stream>>>(V, src, h->part, j, k, per);
        k_esp_free_zsum<<<zg, kBlock, 0, h->stream>>>(V, h->part, S, j, k);
    }
}

// The history for `seeds` leading columns and K picks: Zb (ld x (seeds + K)), cb and the slices' partial sums.  Grows, never
// shrinks.  Refuses, before anything is freed or allocated, what does not fit in the device's free memory (plus what the present
// history gives back).  keep: columns [0, seeds) hold a tree handle's seeds (esp_tree.h) and are copied into the new history,
// allocated beside the old one -- which then gives nothing back, and stays (with the seeds in it) if the new one cannot be made.
// keep is apart from seeds because the columns count from the handle's creation but hold something only once the seeds have run.
// The refusal's text names the seeds on a tree handle (h->tr), r = 0 included; cols > INT_MAX can be true only there (K <= m <= 2e9).
inline int esp_history_reserve(machip_esp* h, int seeds, bool keep, int64_t K) {
    const int64_t cols = (int64_t)seeds + K;
    if ((size_t)cols <= h->zcap) return MACHIP_OK;
    const size_t ld = (size_t)h->ld;
    const double need = 8.0 * (double)ld * (double)cols;
    size_t fr = 0, tot = 0;
    HIP_TRY(hipMemGetInfo(&fr, &tot));
    // headroom: the partial sums, the c's, and 256 MiB for what the runtime and the candidate arrays of other handles take
    const double room = (double)fr + (keep ? 0.0 : 8.0 * (double)ld * (double)h->zcap) - 8.0 * (double)ld * kEspFreeMaxSplit - 8.0 * (double)cols - 268435456.0;
    if (need > room || cols > (int64_t)INT_MAX)
        return fail(MACHIP_BAD_ARG, "the matrix-free history does not fit in device memory: n = " + std::to_string(h->n) + ", K = " + std::to_string((long long)K) +
                                        (h->tr ? " and " + std::to_string(seeds) + " seeds ask for 8 ld (seeds + K) = " : " asks for 8 ld K = ") +
                                        std::to_string((unsigned long long)need) + " bytes (ld = " + std::to_string(h->ld) + "), " +
                                        std::to_string((unsigned long long)fr) + " bytes are free");
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->live = false;
    double *oldZ = h->Zb, *oldc = h->cb;
    if (!keep) {
        if (oldZ) (void)hipFree(oldZ);
        if (oldc) (void)hipFree(oldc);
        oldZ = oldc = nullptr;
    }
    h->Zb = nullptr; h->cb = nullptr; h->zcap = 0;
    if (!h->part) ST_TRY(dev_alloc(&h->part, ld * (size_t)kEspFreeMaxSplit));
    int st = dev_alloc(&h->Zb, ld * (size_t)cols);
    if (st == MACHIP_OK) st = dev_alloc(&h->cb, (size_t)cols);
    if (st == MACHIP_OK && keep) {
        hipError_t e = hipMemcpyAsync(h->Zb, oldZ, sizeof(double) * ld * (size_t)seeds, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h->cb, oldc, sizeof(double) * (size_t)seeds, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) st = fail(MACHIP_HIP_ERROR, std::string("copying the seeds' columns: ") + hipGetErrorString(e));
    }
    if (st != MACHIP_OK) {
        if (keep) {
            if (h->Zb) (void)hipFree(h->Zb);
            if (h->cb) (void)hipFree(h->cb);
            h->Zb = oldZ; h->cb = oldc; h->zcap = (size_t)seeds;
        }
        return st;
    }
    if (oldZ) (void)hipFree(oldZ);
    if (oldc) (void)hipFree(oldc);
    h->zcap = (size_t)cols;
    return MACHIP_OK;
}

}  // namespace machip
