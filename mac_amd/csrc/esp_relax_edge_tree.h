// mac_amd/csrc/esp_relax_edge_tree.h -- the edge-space relaxation of esp_relax_edge.h for any connected fixed graph
// (MACHIP_ESP_EDGE_RELAX_TREE on a MACHIP_ESP_MATRIX_FREE | MACHIP_ESP_SPANNING_TREE handle).
//
// T is the spanning tree of esp_tree.h, Rt its root resistances by preorder number, Sigma0(T)_ab = Rt[lca(a, b)].  The r fixed
// links outside T (the seeds) are not eliminated first: they become r more columns.  M = m + r columns, [0, m) the candidates,
// [m, M) the seeds in the plan's order.  For columns e = (u_e, v_e), f = (u_f, v_f):
//     G_ef = (Rt[lca(u_e, u_f)] + Rt[lca(v_e, v_f)]) - (Rt[lca(u_e, v_f)] + Rt[lca(v_e, u_f)])
// in exactly this association, every sum rounded once.  The two inner sums are commutative, so G_ef = G_fe to the bit; a
// self-loop's row and column are exact zeros.  With d_j = w_j x_j (j < m), d_j = w_seed (j >= m), D = diag(d), N(x) = I + G D:
//     F(x) = log det N(x) - log det N(0),      dF/dx_e = w_e sum_{j < M} N^-1[e, j] G[j, e]      (e < m)
// N(0) carries the seeds alone; log det N(0) is taken once per handle by the kernels below in the same order, so F(0) = 0.0
// exactly.  The leading principal minors of N are det(I + G_kk D_kk) > 0 for every d >= 0: k_gj_step inverts N without pivoting,
// as in esp_relax_edge.h.
//
// G does not depend on x and costs 4 `levels` dependent gathers per entry, so it is built once per handle (the first relaxation
// call) and kept: ld x ld, ld = M rounded up to 64, zeros in the padding.  Per evaluation, on the handle's stream:
//   1. k_edge_tree_assemble: N(x) from the stored G (8 ld^2 bytes read, 8 ld^2 written), identity beyond M;
//   2. gj_inverse_of<true> (esp.h) on the route's own N / second buffer / look-ahead pivot buffer;
//   3. k_edge_tree_grad: row e of N^-1 against row e of G (= column e, G being bit-symmetric: contiguous); 16 ld m bytes read;
//   4. the LP vertex, k_fw_final and k_relax_scalars of esp_relax.h over the m candidates (logdet0 = log det N(0)).
// State: the EspEdge of esp_relax_edge.h with G stored -- three ld x ld buffers (24 ld^2 bytes), 2 x 32 x 32 pivots, the int32
// preorder endpoints of the M columns.  The candidates' weights are the handle's cw, the seeds' the tree state's sw; nothing of size
// n is allocated beyond the tree handle's tables.  The greedy's history, seeds, s0, pending count and flags are never written, and
// the seeds need not have been run; the gradient goes to the handle's score array, which the greedy rebuilds at every use.
#pragma once
#include <algorithm>

#include "esp_relax_edge.h"
#include "esp_tree.h"

namespace machip {

// ---- G, once per handle.  grid = ld: workgroup e owns row e, lanes own the columns f.  All four lifting chains start from the
// row's two endpoints (wave-uniform starts; only ancestors of u_e and v_e are ever read, so the lines stay in L2) and climb side by
// side towards the column's endpoints: 4 independent gathers in flight per lane, `levels` dependent rounds.  Padding: zeros. ----
__global__ __launch_bounds__(kBlock) void k_edge_tree_gram(double* __restrict__ G, int ld, int M, const int* __restrict__ pu,
                                                           const int* __restrict__ pv, EspTreeView T) {
#pragma clang fp contract(off)
    const int e = blockIdx.x;
    double* row = G + (size_t)e * ld;
    if (e >= M) {
        for (int f = threadIdx.x; f < ld; f += kBlock) row[f] = 0.0;
        return;
    }
    const int ue = pu[e], ve = pv[e];
    const int eu = T.tend[ue], ev = T.tend[ve];
    for (int f = threadIdx.x; f < ld; f += kBlock) {
        if (f >= M) { row[f] = 0.0; continue; }
        const int uf = pu[f], vf = pv[f];
        int xuu = ue, xvv = ve, xuv = ue, xvu = ve;
        for (int k = T.levels - 1; k >= 0; --k) {
            xuu = esp_tree_lift(T, k, xuu, uf);
            xvv = esp_tree_lift(T, k, xvv, vf);
            xuv = esp_tree_lift(T, k, xuv, vf);
            xvu = esp_tree_lift(T, k, xvu, uf);
        }
        const double uu = T.Rt[esp_tree_lift_end(T, ue, eu, xuu, uf)], vv = T.Rt[esp_tree_lift_end(T, ve, ev, xvv, vf)];
        const double uv = T.Rt[esp_tree_lift_end(T, ue, eu, xuv, vf)], vu = T.Rt[esp_tree_lift_end(T, ve, ev, xvu, uf)];
        row[f] = (uu + vv) - (uv + vu);
    }
}

// d_j: w_j x_j for a candidate, the seed's weight beyond
__device__ __forceinline__ double esp_edge_tree_d(int j, int m, const double* __restrict__ w, const double* __restrict__ sw,
                                                  const double* __restrict__ x) {
#pragma clang fp contract(off)
    return j < m ? w[j] * x[j] : sw[j - m];
}

// ---- N[i][j] = (i == j) + G[i][j] d_j inside M x M, identity beyond.  grid = ld: workgroup i owns row i, 16-byte loads of G and
// stores of N (rows are 512-byte aligned).  k_edge_assemble's rounding steps: the product d_j, the product G d, the sum. ----
__global__ __launch_bounds__(kBlock) void k_edge_tree_assemble(double* __restrict__ N, const double* __restrict__ G, int ld, int M, int m,
                                                               const double* __restrict__ w, const double* __restrict__ sw,
                                                               const double* __restrict__ x) {
#pragma clang fp contract(off)
    const int i = blockIdx.x;
    double2* row2 = reinterpret_cast<double2*>(N + (size_t)i * ld);
    const double2* g2 = reinterpret_cast<const double2*>(G + (size_t)i * ld);
    const bool in = i < M;
    for (int j2 = threadIdx.x; j2 < ld / 2; j2 += kBlock) {
        const int j = 2 * j2;
        double v0 = i == j ? 1.0 : 0.0, v1 = i == j + 1 ? 1.0 : 0.0;
        if (in && j < M) {
            const double2 g = g2[j2];
            v0 += g.x * esp_edge_tree_d(j, m, w, sw, x);
            if (j + 1 < M) v1 += g.y * esp_edge_tree_d(j + 1, m, w, sw, x);
        }
        row2[j2] = make_double2(v0, v1);
    }
}

// ---- g_e = w_e sum_{j < M} Ninv[e][j] G[e][j] (G[j][e] = G[e][j] to the bit).  grid = m: workgroup e streams the two rows once, a
// double2 per lane each; a thread adds its products in index order (no fma), block_sum adds the threads' sums in its fixed tree. ----
__global__ __launch_bounds__(kBlock) void k_edge_tree_grad(const double* __restrict__ Ninv, const double* __restrict__ G, int ld, int M,
                                                           const double* __restrict__ w, double* __restrict__ g) {
#pragma clang fp contract(off)
    __shared__ double sm[4];
    const int e = blockIdx.x;
    const double2* row2 = reinterpret_cast<const double2*>(Ninv + (size_t)e * ld);
    const double2* g2 = reinterpret_cast<const double2*>(G + (size_t)e * ld);
    double acc = 0.0;
    for (int j2 = threadIdx.x; j2 < (M + 1) / 2; j2 += kBlock) {
        const double2 a = row2[j2], b = g2[j2];
        acc += a.x * b.x;
        if (2 * j2 + 1 < M) acc += a.y * b.y;
    }
    acc = block_sum(acc, sm);
    if (threadIdx.x == 0) g[e] = w[e] * acc;
}

// ---- the columns' endpoints by preorder number, from the reduced node ids (node - 1) the handle and the tree state keep ----
__global__ __launch_bounds__(kBlock) void k_edge_tree_ends(int* __restrict__ pu, int* __restrict__ pv, int M, int m, const int* __restrict__ cu,
                                                           const int* __restrict__ cv, const int* __restrict__ su, const int* __restrict__ sv,
                                                           const int* __restrict__ pre) {
    for (int e = blockIdx.x * kBlock + threadIdx.x; e < M; e += gridDim.x * kBlock) {
        const int a = e < m ? cu[e] : su[e - m], b = e < m ? cv[e] : sv[e - m];
        pu[e] = pre[a + 1];
        pv[e] = pre[b + 1];
    }
}

// The tree route's part of the state: the columns' preorder endpoints and the Gram matrix from them.
inline int esp_edge_tree_gram(machip_esp* h, EspEdge* E) {
    const EspTreeState* t = h->tr;
    hipStream_t st = h->stream;
    if (E->M) k_edge_tree_ends<<<std::max(1, std::min(kMaxGrid, (E->M + kBlock - 1) / kBlock)), kBlock, 0, st>>>(E->eu, E->ev, E->M, h->m, h->cu, h->cv, t->su, t->sv, t->pre);
    k_edge_tree_gram<<<E->ld, kBlock, 0, st>>>(E->G, E->ld, E->M, E->eu, E->ev, t->view(h->n));
    HIP_TRY(hipGetLastError());
    return MACHIP_OK;
}

}  // namespace machip
