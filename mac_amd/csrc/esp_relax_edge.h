// mac_amd/csrc/esp_relax_edge.h -- the relaxation of esp_relax.h carried out in the space of the m candidates instead of the
// n - 1 nodes, for chain-fixed graphs (MACHIP_ESP_EDGE_RELAX on a MACHIP_ESP_MATRIX_FREE handle).
//
// The fixed edges are the chain (t, t+1) with link weights c_t; R[v] = sum_{t < v} 1 / c_t is the resistance from node 0 to v, so
// Sigma0_ab = R[min(a, b)] (esp.h).  Candidate e = (lo_e <= hi_e, w_e) has the incidence column a_e, and the Gram matrix of the
// columns under Sigma0 is the resistance of the overlap of two chain intervals:
//     G_ef = a_e^T Sigma0 a_f = max(0, R[min(hi_e, hi_f)] - R[max(lo_e, lo_f)]).
// With D = diag(w_e x_e) and N(x) = I + G D (m x m):
//     F(x) = log det M(x) - log det M(0) = log det N(x)        (matrix determinant lemma; N(0) = I: F(0) = 0 exactly)
//     dF/dx_e = w_e a_e^T M(x)^-1 a_e = w_e [N(x)^-1 G]_ee = w_e sum_j N^-1[e, j] G[j, e]      (Woodbury)
// N is not symmetric, but where x > 0 it is the diagonal similarity D^-1/2 (I + D^1/2 G D^1/2) D^1/2 of an SPD matrix, and its
// leading principal minors are those of I + G_kk D_kk: positive on all of [0, 1]^m, zeros of x included.  Elimination without
// pivoting therefore meets the SPD matrix's pivots, all positive, and k_gj_step (which reads A_iK and A_Kj separately and assumes
// no symmetry) inverts N as it stands; the sum of the logs of its pivots is F itself, nothing is subtracted.
//
// Per evaluation, on the handle's stream:
//   1. k_edge_assemble: N(x), identity beyond m, into the route's own ld x ld buffer (ld = m rounded up to 64).  8 ld^2 bytes
//      written; lo, hi, w, x (24 m bytes) and the R entries they point at are read from L2;
//   2. gj_inverse_of<true> (esp.h), ping-pong with the route's second buffer and its own look-ahead pivot buffer;
//   3. k_edge_grad: row e of N^-1 against column e of G, which is built by the function step 1 built it with (the same bits);
//      8 ld m bytes read once;
//   4. the LP vertex, k_fw_final and k_relax_scalars of esp_relax.h (logdet0 = 0, ld / 32 blocks).
// State: the one EspEdge below, shared with esp_relax_edge_tree.h -- the columns' two int32 endpoint arrays (here lo, hi), two
// ld x ld buffers, 2 x 32 x 32 pivots, and no stored G: esp_edge_G is the closed form.  w is the handle's cw and R the prefix array
// the matrix-free greedy uploaded: nothing of size n is allocated here.  The greedy's history, flags and pending count are never
// written; the gradient goes to the handle's score array, which the greedy rebuilds from R (and its history) at every use.
#pragma once
#include <algorithm>
#include <vector>

#include "esp.h"
#include "plan.h"

namespace machip {

// The state of the edge-space relaxation on either route (esp_relax.h makes it, evaluates on it and releases it;
// esp_exchange_edge.h keeps its R in bufN).
struct EspEdge {
    int M = 0, ld = 0;                       // columns (chain: m; tree: m + r) and the route's leading dimension
    int *eu = nullptr, *ev = nullptr;        // the columns' endpoints, int32[M].  Chain: reduced (node - 1; -1 = node 0), eu <= ev
                                             // (lo, hi of the kernels below); tree: preorder numbers (pu, pv of esp_relax_edge_tree.h)
    double* G = nullptr;                     // the stored Gram matrix, ld x ld (tree); null on the chain, where esp_edge_G is G
    double *bufN = nullptr, *bufC = nullptr; // N(x) / its inverse, and the elimination's second buffer
    double* piv = nullptr;                   // look-ahead pivot blocks (2 x 32 x 32)
};

// R of a reduced endpoint: the resistance from node 0 (0 for node 0 itself)
__device__ __forceinline__ double esp_edge_R(const double* __restrict__ R, int a) { return a >= 0 ? R[a] : 0.0; }

// G_ef: the resistance of [max(lo_e, lo_f), min(hi_e, hi_f)], 0 when the intervals share no link.  Symmetric in (e, f) to the
// bit; the one place both kernels take G from.
__device__ __forceinline__ double esp_edge_G(const double* __restrict__ R, int lo_e, int hi_e, int lo_f, int hi_f) {
    const int a = max(lo_e, lo_f), b = min(hi_e, hi_f);
    return b > a ? esp_edge_R(R, b) - esp_edge_R(R, a) : 0.0;
}

// ---- N[i][j] = (i == j) + G_ij (w_j x_j) inside m x m, identity beyond.  grid = ld: workgroup i owns row i and writes it with
// 16-byte stores (ld is a multiple of 64: rows are 512-byte aligned).  One product, one product, one sum per entry, each rounded. ----
__global__ __launch_bounds__(kBlock) void k_edge_assemble(double* __restrict__ N, int ld, int m, const int* __restrict__ lo,
                                                          const int* __restrict__ hi, const double* __restrict__ w,
                                                          const double* __restrict__ R, const double* __restrict__ x) {
#pragma clang fp contract(off)
    const int i = blockIdx.x;
    double2* row2 = reinterpret_cast<double2*>(N + (size_t)i * ld);
    const bool in = i < m;
    const int li = in ? lo[i] : 0, hi_i = in ? hi[i] : 0;
    for (int j2 = threadIdx.x; j2 < ld / 2; j2 += kBlock) {
        double v[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int j = 2 * j2 + q;
            double a = i == j ? 1.0 : 0.0;
            if (in && j < m) a += esp_edge_G(R, li, hi_i, lo[j], hi[j]) * (w[j] * x[j]);
            v[q] = a;
        }
        row2[j2] = make_double2(v[0], v[1]);
    }
}

// ---- g_e = w_e sum_j Ninv[e][j] G[j][e].  grid = m: workgroup e streams row e once, a double2 per lane (16-byte loads, 1 KiB per
// wave instruction, contiguous); a thread adds its products in index order (no fma), block_sum adds the threads' sums in its fixed
// tree.  Columns beyond m hold zeros of the identity padding and are not read. ----
__global__ __launch_bounds__(kBlock) void k_edge_grad(const double* __restrict__ Ninv, int ld, int m, const int* __restrict__ lo,
                                                      const int* __restrict__ hi, const double* __restrict__ w,
                                                      const double* __restrict__ R, double* __restrict__ g) {
#pragma clang fp contract(off)
    __shared__ double sm[4];
    const int e = blockIdx.x;
    const double2* row2 = reinterpret_cast<const double2*>(Ninv + (size_t)e * ld);
    const int le = lo[e], he = hi[e];
    double acc = 0.0;
    for (int j2 = threadIdx.x; j2 < (m + 1) / 2; j2 += kBlock) {
        const double2 a = row2[j2];
        const int j = 2 * j2;
        acc += a.x * esp_edge_G(R, lo[j], hi[j], le, he);
        if (j + 1 < m) acc += a.y * esp_edge_G(R, lo[j + 1], hi[j + 1], le, he);
    }
    acc = block_sum(acc, sm);
    if (threadIdx.x == 0) g[e] = w[e] * acc;
}

inline void esp_edge_release(EspEdge* E) {
    if (!E) return;
    void* bufs[] = {E->eu, E->ev, E->G, E->bufN, E->bufC, E->piv};
    for (void* q : bufs) if (q) (void)hipFree(q);
    delete E;
}

// What both routes allocate for M columns at leading dimension ld (the caller owns *E and releases it on failure).
inline int esp_edge_alloc(EspEdge* E, int M, int ld, bool stored_gram) {
    E->M = M; E->ld = ld;
    const size_t l2 = (size_t)ld * (size_t)ld, Ms = (size_t)std::max(M, 1);
    ST_TRY(dev_alloc(&E->eu, Ms)); ST_TRY(dev_alloc(&E->ev, Ms));
    if (stored_gram) ST_TRY(dev_alloc(&E->G, l2));
    ST_TRY(dev_alloc(&E->bufN, l2)); ST_TRY(dev_alloc(&E->bufC, l2));
    ST_TRY(dev_alloc(&E->piv, (size_t)2 * kGjB * kGjB));
    return MACHIP_OK;
}

// The chain route's part of the state: lo, hi from the candidates' lists as given.
inline int esp_edge_chain_ends(machip_esp* h, EspEdge* E) {
    const size_t m = (size_t)h->m;
    if (!m) return MACHIP_OK;
    std::vector<int> lo(m), hi(m);
    for (size_t e = 0; e < m; ++e) {
        lo[e] = std::min(h->hci[e], h->hcj[e]) - 1;
        hi[e] = std::max(h->hci[e], h->hcj[e]) - 1;
    }
    HIP_TRY(hipMemcpyAsync(E->eu, lo.data(), sizeof(int) * m, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(E->ev, hi.data(), sizeof(int) * m, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));          // (host staging goes out of scope)
    return MACHIP_OK;
}

}  // namespace machip
