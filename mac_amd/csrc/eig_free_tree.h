// mac_amd/csrc/eig_free_tree.h -- GreedyEig without a dense Sigma for any connected fixed graph.
//
// eig_free.h with the chain replaced by the spanning tree T of esp_tree.h:  Sigma0(T)_ab = Rt[lca(a, b)], the r fixed links outside T
// are the history columns [0, r) (esp_tree_prepare seeds them), the picks follow from column r on.  What this file adds is
// T = Sigma0(T) Q for a batch.  In preorder, with end_p the subtree end of p and d_p = Rt[p] - Rt[parent p] = 1 / w(link above p),
//     s_p = S(p) - S(end_p + 1),   S(p) = sum_{p' >= p} q_p'        the subtree's sum as a difference of two suffix sums
//     u_p = d_p s_p
//     T_p = sum over p and its ancestors of u_a
//         = the prefix over the Euler tour of (+u_a on entering a, -u_a on leaving a), read at p's entry.
// Row p >= 1 of the batch is row node_of[p] - 1 of Q and of T (the root is the pinned node 0 and has no row).  On a chain end_p + 1 is
// past the last row and nothing is left before the end: the two scans of eig_free.h.  The difference of suffix sums cancels like
// n' eps: harmless for a preconditioner (every value is decided by the sparse L_cur), documented, not worked around.
//
// Four launches whatever the tree's depth, lanes along the batch index (a row access is one contiguous 512-byte segment per wave):
//   k_eigt_up<0>     the row chunks' sums of q (rows in preorder, `rows` per chunk)
//   k_eigt_up<1>     S, materialised (ld x ldq): a chunk's suffix carry = the later chunks' sums, added in ascending chunk order
//   k_eigt_tour<0>   the tour chunks' sums of +-u (2 rows events per chunk); u is recomputed from S, the same doubles in both launches
//   k_eigt_tour<1>   T: a chunk's prefix carry = the earlier chunks' sums, added in ascending chunk order; rows n'..ld written 0
// No atomics; the order of every sum is a function of (ld, the tree, option eig_free_rows) alone.  A 64-column group whose columns
// have all retired is skipped by every launch.  The batch's z_e = Sigma0(T) a_e - Zb alpha use the same sweeps on indicator columns
// (k_eigt_fill), then k_eigf_back<true, true> reads its base from T: one application's cost per batch instead of ld B lca walks.
#pragma once
#include <string>
#include <vector>

#include "eig_free.h"

namespace machip {

constexpr int kEigTreeLeave = INT_MIN;      // the bit of a tour entry that marks "leaving"

struct EigTreeView {
    int nev;                   // tour events: 2 n'
    const int* node_of;        // preorder number -> node
    const int* tend;           // preorder number -> last preorder number of its subtree (EspTreeState::tend)
    const int* tour;           // event -> preorder number, kEigTreeLeave set on leaving
    const double* d;           // preorder number -> Rt[p] - Rt[parent p] (d[0] = 0)
    double* S;                 // S(p) at row p - 1 (n' rows of ldq)
    double *cs, *ct;           // the row chunks' sums of q, the tour chunks' sums of +-u (chunks x ldq each)
};

// what the route keeps beside EigFree's buffers
struct EigFreeTree {
    int nev = 0;
    int *node_of = nullptr, *tour = nullptr;
    double *d = nullptr, *S = nullptr;
};

// ---- the upward sweep.  grid = (ldq / 64, chunks), one wave per workgroup: lane = a column of the batch, the chunk's preorder rows
// walked downwards.  MODE 0: cs[c] = the chunk's sum of q.  MODE 1: S.  all != 0: no column counts as retired (the batch's z_e). ----
template <int MODE>
__global__ __launch_bounds__(kWave) void k_eigt_up(EigView E, EigTreeView W, int rows, int count, int all) {
    const int col = blockIdx.x * kWave + threadIdx.x;
    const int live = (col < count && (all || E.conv[col] == 0)) ? 1 : 0;
    if (!__any(live)) return;
    const int c = blockIdx.y, nch = gridDim.y;
    const int k0 = c * rows, k1 = min(E.np, k0 + rows);
    const size_t ldq = E.ldq;
    double s = 0.0;
    if (MODE == 1)
        for (int c2 = c + 1; c2 < nch; ++c2) s += W.cs[(size_t)c2 * ldq + col];
    for (int k = k1 - 1; k >= k0; --k) {
        s += E.Q[(size_t)(W.node_of[k + 1] - 1) * ldq + col];
        if (MODE == 1) W.S[(size_t)k * ldq + col] = s;
    }
    if (MODE == 0) W.cs[(size_t)c * ldq + col] = s;
}

// +u_p on entering p, -u_p on leaving it, u_p = d_p (S(p) - S(end_p + 1)): formed the same way wherever it is needed
__device__ __forceinline__ double eigt_event(const EigTreeView& W, int np, size_t ldq, int col, int ev, int& p) {
    p = ev & ~kEigTreeLeave;
    const int en = W.tend[p];
    double s = W.S[(size_t)(p - 1) * ldq + col];
    if (en < np) s -= W.S[(size_t)en * ldq + col];
    const double u = W.d[p] * s;
    return ev < 0 ? -u : u;
}

// ---- the sweep along the tour.  grid as k_eigt_up, a chunk = 2 rows events walked upwards.  MODE 0: ct[c] = the chunk's sum of +-u.
// MODE 1: T at every entry; chunk 0 writes the rows n'..ld as 0. ----
template <int MODE>
__global__ __launch_bounds__(kWave) void k_eigt_tour(EigView E, EigTreeView W, int rows, int count, int all) {
    const int col = blockIdx.x * kWave + threadIdx.x;
    const int live = (col < count && (all || E.conv[col] == 0)) ? 1 : 0;
    if (!__any(live)) return;
    const int c = blockIdx.y;
    const int e0 = (int)min((long long)W.nev, 2ll * c * rows), e1 = (int)min((long long)W.nev, e0 + 2ll * rows);
    const size_t ldq = E.ldq;
    double t = 0.0;
    if (MODE == 1) {
        for (int c2 = 0; c2 < c; ++c2) t += W.ct[(size_t)c2 * ldq + col];
        if (c == 0)
            for (int k = E.np; k < E.ld; ++k) E.T[(size_t)k * ldq + col] = 0.0;
    }
    for (int e = e0; e < e1; ++e) {
        const int ev = W.tour[e];
        int p;
        t += eigt_event(W, E.np, ldq, col, ev, p);
        if (MODE == 1 && ev >= 0) E.T[(size_t)(W.node_of[p] - 1) * ldq + col] = t;
    }
    if (MODE == 0) W.ct[(size_t)c * ldq + col] = t;
}

// ---- Q <- the indicator columns a_e of the batch (row u: +1, row v: -1, node-0 terms none), 0 everywhere else ----
__global__ __launch_bounds__(kBlock) void k_eigt_fill(EigView E, int count) {
    const size_t ldq = E.ldq, tot = (size_t)E.ld * ldq;
    for (size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * kBlock) {
        const int k = (int)(idx / ldq), b = (int)(idx % ldq);
        double a = 0.0;
        const int e = b < count ? E.bc[b] : -1;
        if (e >= 0) a = (E.cu[e] == k ? 1.0 : 0.0) - (E.cv2[e] == k ? 1.0 : 0.0);
        E.Q[idx] = a;
    }
}

// eig_free_init, then the route's tables from the plan (node_of, the tour, d) and S.
inline int eig_tree_init(machip_eig* h, const EspTreePlan& P) {
    ST_TRY(eig_free_init(h, true));
    EigFree* F = h->fr;
    EigFreeTree* G = new EigFreeTree();
    F->tree = G;
    const machip_esp* base = h->base;
    const int N = h->n;
    const size_t n = (size_t)N;
    std::vector<int> node_of(n), tour, stack;
    std::vector<double> d(n, 0.0);
    for (int v = 0; v < N; ++v) node_of[(size_t)P.pre[(size_t)v]] = v;
    for (int p = 1; p < N; ++p) {
        const int v = node_of[(size_t)p];
        d[(size_t)p] = P.R[(size_t)v] - P.R[(size_t)P.parent[(size_t)v]];
    }
    tour.reserve(2 * n);
    for (int p = 1; p < N; ++p) {      // preorder: whatever ends before p is left before p is entered
        while (!stack.empty() && P.end[(size_t)node_of[(size_t)stack.back()]] < p) { tour.push_back(stack.back() | kEigTreeLeave); stack.pop_back(); }
        tour.push_back(p);
        stack.push_back(p);
    }
    while (!stack.empty()) { tour.push_back(stack.back() | kEigTreeLeave); stack.pop_back(); }
    G->nev = (int)tour.size();
    ST_TRY(dev_alloc(&G->S, (size_t)base->ld * (size_t)h->ldq));
    ST_TRY(dev_alloc(&G->node_of, n)); ST_TRY(dev_alloc(&G->d, n)); ST_TRY(dev_alloc(&G->tour, tour.size()));
    hipStream_t st = base->stream;
    HIP_TRY(hipMemcpyAsync(G->node_of, node_of.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(G->d, d.data(), sizeof(double) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(G->tour, tour.data(), sizeof(int) * tour.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));        // (host staging goes out of scope)
    return MACHIP_OK;
}

inline void eig_tree_release(EigFreeTree* G) {
    if (!G) return;
    void* bufs[] = {G->node_of, G->tour, G->d, G->S};
    for (void* q : bufs) if (q) (void)hipFree(q);
    delete G;
}

// T = Sigma0(T) Q: the four launches
inline int eig_tree_sweeps(machip_eig* h, int count, bool all) {
    const EigFree* F = h->fr;
    const EigFreeTree* G = F->tree;
    const machip_esp* base = h->base;
    const EigView E = h->view();
    EigTreeView W;
    W.nev = G->nev; W.node_of = G->node_of; W.tend = base->tr->tend; W.tour = G->tour; W.d = G->d; W.S = G->S; W.cs = F->cs; W.ct = F->cu;
    hipStream_t st = base->stream;
    const dim3 sg((count + kGjT - 1) / kGjT, F->nchunks);
    k_eigt_up<0><<<sg, kWave, 0, st>>>(E, W, F->rows, count, all ? 1 : 0);
    k_eigt_up<1><<<sg, kWave, 0, st>>>(E, W, F->rows, count, all ? 1 : 0);
    k_eigt_tour<0><<<sg, kWave, 0, st>>>(E, W, F->rows, count, all ? 1 : 0);
    k_eigt_tour<1><<<sg, kWave, 0, st>>>(E, W, F->rows, count, all ? 1 : 0);
    return MACHIP_OK;
}

// z_e = Sigma_cur a_e and c_e of the columns bc[0..count) into Z / cc; Q is left all zero (what machip_eig::alloc promises, and more)
inline int eig_tree_columns(machip_eig* h, int count) {
    const size_t qtot = (size_t)h->base->ld * (size_t)h->ldq;
    k_eigt_fill<<<(unsigned)std::min<size_t>(kMaxGrid, (qtot + kBlock - 1) / kBlock), kBlock, 0, h->base->stream>>>(h->view(), count);
    ST_TRY(eig_tree_sweeps(h, count, true));
    ST_TRY(eig_free_columns<true>(h, count));
    HIP_TRY(hipMemsetAsync(h->Q, 0, sizeof(double) * qtot, h->base->stream));
    return MACHIP_OK;
}

}  // namespace machip
