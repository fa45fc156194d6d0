// mac_amd/csrc/esp_tree.h -- GreedyESP's matrix-free route for any connected fixed graph.
//
// Take a spanning tree T of the fixed graph, rooted at node 0.  With R[v] the resistance from the root to v along T,
//     Sigma0(T)_ab = R[lca(a, b)]
// -- esp_free.h's R[min(a, b)] with min replaced by the lowest common ancestor (on the chain the two coincide).  Every fixed link
// that is not in T ("seed") is a rank-one update exactly like a pick: it enters the history Zb, cb as one of the columns [0, r)
// before the first pick, with c = w / (1 + w (z_u - z_v)), and makes no entry in order / gains.  Picks occupy columns r, r + 1, ...
//
// Host (esp_tree_plan): parallel fixed edges are summed in list order ((a, b) and (b, a) are one link), self-loops dropped; T is
// the BFS tree from node 0 with neighbours visited in order of first appearance in the fixed list; R[v] = R[parent] + 1 / w (on
// a chain: the prefix sums of esp.h, same order of additions, same bits); preorder numbers and subtree ends; the links not in T,
// in order of first appearance, are the seeds.
//
// Device: everything is addressed by PREORDER number p.  "a is an ancestor of b" is  p_a <= p_b <= end_a.  The lifting table
// up[k][p] = (preorder number, subtree end) of the 2^k-th ancestor of p (the root is its own parent), k < levels =
// bit_length(depth of T): an int2 per entry, so one lifting step is ONE dependent 8-byte gather (ancestor and its interval
// together) instead of two.  lca(u, i): if u is an ancestor of i it is u; else lift u past every ancestor that is not an ancestor
// of i, highest level first; the parent of where that ends is the answer.  Rt[p] = R by preorder number (Rt[0] = 0: node-0 terms
// need no special case).
//
// k_esp_tree_row: zrow_i = Rt[lca(u, i)] - Rt[lca(v, i)] for all rows.  A lane owns one row and walks the two lifting chains (u's and
// v's) side by side: 2 independent gathers in flight per lane, `levels` dependent rounds.  It is a latency chain, not a stream:
// all lanes start from the same two nodes and only ever touch ancestors of u and v, so the lines they read are few and L2-resident
// whatever the table's size.  k_esp_free_z<SPLIT, true> then starts slice 0 from zrow and runs the FMA chain over the history as on
// the chain route; k_esp_free_zsum, k_esp_update and k_esp_argmax are reused as they are.  No floating-point atomics.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "esp_free.h"

namespace machip {

// ---- host: the spanning tree and the seeds ----
struct EspTreePlan {
    std::vector<int32_t> parent, pre, end, depth;      // by node; parent[0] = -1
    std::vector<double> R;                             // by node; R[0] = 0
    std::vector<int32_t> su, sv;                       // seeds, as first given
    std::vector<double> sw;
    int maxdepth = 0;
};

inline int esp_tree_plan(int64_t n, int64_t nf, const int32_t* fi, const int32_t* fj, const double* fw, EspTreePlan& P) {
    if (n < 1 || n > (int64_t)INT_MAX - kGjT) return fail(MACHIP_BAD_ARG, "num_nodes out of range");
    if (nf < 0 || (nf && (!fi || !fj || !fw))) return fail(MACHIP_BAD_ARG, "bad fixed edge list");
    const int N = (int)n;
    // links: merged in list order, kept in order of first appearance
    std::unordered_map<uint64_t, int> at;
    at.reserve((size_t)nf * 2 + 1);
    std::vector<int32_t> la, lb;
    std::vector<double> lw;
    for (int64_t e = 0; e < nf; ++e) {
        const int a = fi[e], b = fj[e];
        if (a < 0 || a >= N || b < 0 || b >= N || !std::isfinite(fw[e])) return fail(MACHIP_BAD_ARG, "fixed edge out of range or weight not finite");
        if (a == b) continue;
        const uint64_t key = (uint64_t)std::min(a, b) * (uint64_t)N + (uint64_t)std::max(a, b);
        auto it = at.find(key);
        if (it == at.end()) {
            at.emplace(key, (int)la.size());
            la.push_back(a); lb.push_back(b); lw.push_back(fw[e]);
        } else {
            lw[(size_t)it->second] += fw[e];
        }
    }
    const size_t L = la.size();
    for (size_t l = 0; l < L; ++l)
        if (!(lw[l] > 0.0))
            return fail(MACHIP_BAD_ARG, "the spanning-tree route needs positive link weights: the fixed edges between nodes " + std::to_string(la[l]) +
                                            " and " + std::to_string(lb[l]) + " sum to " + std::to_string(lw[l]));
    // adjacency in link order
    std::vector<int> off((size_t)N + 1, 0);
    for (size_t l = 0; l < L; ++l) { ++off[(size_t)la[l] + 1]; ++off[(size_t)lb[l] + 1]; }
    for (int i = 0; i < N; ++i) off[(size_t)i + 1] += off[(size_t)i];
    std::vector<int> adj(2 * L), fill(off.begin(), off.end() - 1);
    for (size_t l = 0; l < L; ++l) { adj[(size_t)fill[(size_t)la[l]]++] = (int)l; adj[(size_t)fill[(size_t)lb[l]]++] = (int)l; }
    // BFS from node 0
    P.parent.assign((size_t)N, -1); P.depth.assign((size_t)N, 0); P.R.assign((size_t)N, 0.0);
    std::vector<char> seen((size_t)N, 0), intree(L, 0);
    std::vector<int> bfs, cstart((size_t)N, 0), ccount((size_t)N, 0);
    bfs.reserve((size_t)N);
    bfs.push_back(0);
    seen[0] = 1;
    P.maxdepth = 0;
    for (size_t q = 0; q < bfs.size(); ++q) {
        const int x = bfs[q];
        cstart[(size_t)x] = (int)bfs.size();
        for (int t = off[(size_t)x]; t < off[(size_t)x + 1]; ++t) {
            const int l = adj[(size_t)t];
            const int y = la[(size_t)l] == x ? lb[(size_t)l] : la[(size_t)l];
            if (seen[(size_t)y]) continue;
            seen[(size_t)y] = 1;
            intree[(size_t)l] = 1;
            P.parent[(size_t)y] = x;
            P.depth[(size_t)y] = P.depth[(size_t)x] + 1;
            P.maxdepth = std::max(P.maxdepth, P.depth[(size_t)y]);
            P.R[(size_t)y] = P.R[(size_t)x] + 1.0 / lw[(size_t)l];
            bfs.push_back(y);
        }
        ccount[(size_t)x] = (int)bfs.size() - cstart[(size_t)x];
    }
    if ((int)bfs.size() != N)
        return fail(MACHIP_BAD_ARG, "the spanning-tree route needs a connected fixed graph: " + std::to_string(N - (int)bfs.size()) + " of " +
                                        std::to_string(N) + " nodes are not reachable from node 0 over the fixed edges");
    // preorder (children in the order BFS attached them) and subtree ends
    P.pre.assign((size_t)N, 0); P.end.assign((size_t)N, 0);
    std::vector<int> size((size_t)N, 1), stack;
    for (size_t q = bfs.size(); q-- > 1;) size[(size_t)P.parent[(size_t)bfs[q]]] += size[(size_t)bfs[q]];
    stack.push_back(0);
    int cnt = 0;
    while (!stack.empty()) {
        const int x = stack.back();
        stack.pop_back();
        P.pre[(size_t)x] = cnt++;
        P.end[(size_t)x] = P.pre[(size_t)x] + size[(size_t)x] - 1;
        for (int c = ccount[(size_t)x]; c-- > 0;) stack.push_back(bfs[(size_t)(cstart[(size_t)x] + c)]);
    }
    P.su.clear(); P.sv.clear(); P.sw.clear();
    for (size_t l = 0; l < L; ++l)
        if (!intree[l]) { P.su.push_back(la[l]); P.sv.push_back(lb[l]); P.sw.push_back(lw[l]); }
    return MACHIP_OK;
}

// ---- device ----
struct EspTreeView {
    int n, levels;
    const int* pre;          // node -> preorder number
    const int* tend;         // preorder number -> last preorder number of its subtree
    const int2* up;          // [levels][n] by preorder number: (2^k-th ancestor, its subtree end)
    const double* Rt;        // preorder number -> resistance from the root
};

// One lifting step at level k towards the preorder number px: x moves to its 2^k-th ancestor unless that ancestor is an ancestor
// of px as well.  One dependent 8-byte gather.  The one statement of the lifting rule: every chain below is made of these.
__device__ __forceinline__ int esp_tree_lift(const EspTreeView& T, int k, int x, int px) {
    const int2 a = T.up[(size_t)k * T.n + x];
    return (a.x <= px && px <= a.y) ? x : a.x;
}

// The end of a chain that started at u = (pu, eu) and stands at x: u itself when u is an ancestor of px, else the parent of x.
__device__ __forceinline__ int esp_tree_lift_end(const EspTreeView& T, int pu, int eu, int x, int px) {
    return (pu <= px && px <= eu) ? pu : T.up[x].x;
}

// preorder number of lca(u, x) for u = (pu, eu) and the preorder number px: `levels` dependent gathers
__device__ __forceinline__ int esp_tree_lca(const EspTreeView& T, int pu, int eu, int px) {
    int x = pu;
    for (int k = T.levels - 1; k >= 0; --k) x = esp_tree_lift(T, k, x, px);
    return esp_tree_lift_end(T, pu, eu, x, px);
}

// esp_free_score with R[min(u, v)] replaced by Rt[lca(u, v)]: the same three-term sum (u, v reduced: node - 1)
__device__ __forceinline__ void esp_tree_terms(const EspTreeView& T, int u, int v, double& uu, double& vv, double& uv) {
    const int pu = T.pre[u + 1], pv = T.pre[v + 1];
    uu = T.Rt[pu];
    vv = T.Rt[pv];
    uv = T.Rt[esp_tree_lca(T, pu, T.tend[pu], pv)];
}

// ---- s = s0 (the scores after the seeds) and the partials of the argmax: the start of a selection run ----
__global__ __launch_bounds__(kBlock) void k_esp_tree_restart(EspView V, const double* __restrict__ s0) {
    __shared__ double sv[kBlock / kWave];
    __shared__ int si[kBlock / kWave];
    double bv = -INFINITY;
    int bi = INT_MAX;
    for (int e = blockIdx.x * kBlock + threadIdx.x; e < V.m; e += gridDim.x * kBlock) {
        const double s = s0[e];
        V.s[e] = s;
        esp_better(bv, bi, s, e);
    }
    esp_block_argmax(bv, bi, sv, si);
    if (threadIdx.x == 0) { V.pv[blockIdx.x] = bv; V.pi[blockIdx.x] = bi; }
}

// ---- score pass from the tree alone ----
__global__ __launch_bounds__(kBlock) void k_esp_tree_scores(EspView V, EspTreeView T) {
    for (int e = blockIdx.x * kBlock + threadIdx.x; e < V.m; e += gridDim.x * kBlock) {
        double uu, vv, uv;
        esp_tree_terms(T, V.cu[e], V.cv[e], uu, vv, uv);
        V.s[e] = V.cw[e] * (uu + vv - 2.0 * uv);
    }
}

// ---- s_e = w_e (tree term - sum_{b < j} c_b (Zb[u, b] - Zb[v, b])^2) for all m (j = seeds + picks): k_esp_free_resist's walk ----
__global__ __launch_bounds__(kBlock) void k_esp_tree_resist(EspView V, EspTreeView T, int j) {
    const size_t ld = V.ld;
    for (int e = blockIdx.x * kBlock + threadIdx.x; e < V.m; e += gridDim.x * kBlock) {
        const int u = V.cu[e], v = V.cv[e];
        double uu, vv, uv;
        esp_tree_terms(T, u, v, uu, vv, uv);
        double acc = 0.0;
        for (int b = 0; b < j; ++b) {
            const double* zc = V.Zb + (size_t)b * ld;
            const double d = (u >= 0 ? zc[u] : 0.0) - (v >= 0 ? zc[v] : 0.0);
            acc = __builtin_fma(V.cb[b] * d, d, acc);
        }
        V.s[e] = V.cw[e] * ((uu + vv - 2.0 * uv) - acc);
    }
}

// ---- the Sigma0 row difference of one edge: zrow_i = Rt[lca(u, i)] - Rt[lca(v, i)], 0 in the padding rows.  grid = ceil(ld / 256).
// SEED = false: the edge is the step's winner V.best.  SEED = true: V is the seeds' view and the edge is seed q; thread 0 makes
// it the "winner" the z kernels read. ----
template <bool SEED>
__global__ __launch_bounds__(kBlock) void k_esp_tree_row(EspView V, EspTreeView T, double* __restrict__ zrow, int q) {
    const int e = SEED ? q : V.best->idx;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (SEED && i == 0) { V.best->idx = q; V.best->val = 0.0; }
    if (i >= V.ld) return;
    if (i >= V.np) { zrow[i] = 0.0; return; }
    const int pu = T.pre[V.cu[e] + 1], pv = T.pre[V.cv[e] + 1], px = T.pre[i + 1];
    const int eu = T.tend[pu], ev = T.tend[pv];
    int xu = pu, xv = pv;
    for (int k = T.levels - 1; k >= 0; --k) {            // the two chains side by side: 2 gathers in flight per lane
        xu = esp_tree_lift(T, k, xu, px);
        xv = esp_tree_lift(T, k, xv, px);
    }
    const int lu = esp_tree_lift_end(T, pu, eu, xu, px);
    const int lv = esp_tree_lift_end(T, pv, ev, xv, px);
    zrow[i] = T.Rt[lu] - T.Rt[lv];
}

// ---- c of seed q from its z (column q): c = w / (1 + w (z_u - z_v)).  One thread. ----
__global__ void k_esp_tree_seed_c(EspView V, int q) {
    const double* z = V.Zb + (size_t)q * V.ld;
    const int u = V.cu[q], v = V.cv[q];
    const double d = (u >= 0 ? z[u] : 0.0) - (v >= 0 ? z[v] : 0.0);
    V.cb[q] = V.cw[q] / (1.0 + V.cw[q] * d);
}

// the state the route adds to a handle
struct EspTreeState {
    int seeds = 0, levels = 1;
    bool seeded = false;
    int *pre = nullptr, *tend = nullptr;
    int2* up = nullptr;
    double *Rt = nullptr, *zrow = nullptr, *s0 = nullptr;
    int *su = nullptr, *sv = nullptr, *ssel = nullptr, *sorder = nullptr;      // the seeds as a candidate list of their own
    double *sw = nullptr, *sgain = nullptr;
    EspBest* sbest = nullptr;

    EspTreeView view(int n) const {
        EspTreeView T;
        T.n = n; T.levels = levels; T.pre = pre; T.tend = tend; T.up = up; T.Rt = Rt;
        return T;
    }
    size_t table_bytes(int n) const { return (size_t)n * ((size_t)levels * sizeof(int2) + 2 * sizeof(int) + sizeof(double)); }
};

inline void esp_tree_release(machip_esp* h) {
    EspTreeState* t = h->tr;
    if (!t) return;
    void* bufs[] = {t->pre, t->tend, t->up, t->Rt, t->zrow, t->s0, t->su, t->sv, t->ssel, t->sorder, t->sw, t->sgain, t->sbest};
    for (void* q : bufs) if (q) (void)hipFree(q);
    delete t;
    h->tr = nullptr;
}

// the tables of a plan onto the device (machip_esp_create; the stream is synchronised before the host staging goes)
inline int esp_tree_upload(machip_esp* h, const EspTreePlan& P) {
    EspTreeState* t = new EspTreeState();
    h->tr = t;
    const int N = h->n;
    const size_t n = (size_t)N, r = P.sw.size(), ms = (size_t)std::max(h->m, 1);
    t->seeds = (int)r;
    t->levels = 1;
    while ((1 << t->levels) <= P.maxdepth) ++t->levels;             // bit_length(maxdepth), at least 1
    std::vector<int> node_of(n), tend(n);
    std::vector<double> Rt(n);
    for (int v = 0; v < N; ++v) node_of[(size_t)P.pre[(size_t)v]] = v;
    for (int p = 0; p < N; ++p) { tend[(size_t)p] = P.end[(size_t)node_of[(size_t)p]]; Rt[(size_t)p] = P.R[(size_t)node_of[(size_t)p]]; }
    std::vector<int2> up((size_t)t->levels * n);
    for (int p = 0; p < N; ++p) {
        const int v = node_of[(size_t)p], par = v ? P.parent[(size_t)v] : 0;
        up[(size_t)p] = make_int2(P.pre[(size_t)par], P.end[(size_t)par]);
    }
    for (int k = 1; k < t->levels; ++k)
        for (size_t p = 0; p < n; ++p) up[(size_t)k * n + p] = up[(size_t)(k - 1) * n + (size_t)up[(size_t)(k - 1) * n + p].x];
    std::vector<int> su(r), sv(r);
    for (size_t q = 0; q < r; ++q) { su[q] = P.su[q] - 1; sv[q] = P.sv[q] - 1; }
    ST_TRY(dev_alloc(&t->pre, n)); ST_TRY(dev_alloc(&t->tend, n)); ST_TRY(dev_alloc(&t->up, up.size())); ST_TRY(dev_alloc(&t->Rt, n));
    ST_TRY(dev_alloc(&t->zrow, (size_t)h->ld)); ST_TRY(dev_alloc(&t->s0, ms));
    ST_TRY(dev_alloc(&t->su, r)); ST_TRY(dev_alloc(&t->sv, r)); ST_TRY(dev_alloc(&t->sw, r));
    ST_TRY(dev_alloc(&t->ssel, r)); ST_TRY(dev_alloc(&t->sorder, r)); ST_TRY(dev_alloc(&t->sgain, r)); ST_TRY(dev_alloc(&t->sbest, 1));
    hipStream_t st = h->stream;
    HIP_TRY(hipMemcpyAsync(t->pre, P.pre.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(t->tend, tend.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(t->up, up.data(), sizeof(int2) * up.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(t->Rt, Rt.data(), sizeof(double) * n, hipMemcpyHostToDevice, st));
    if (r) {
        HIP_TRY(hipMemcpyAsync(t->su, su.data(), sizeof(int) * r, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t->sv, sv.data(), sizeof(int) * r, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t->sw, P.sw.data(), sizeof(double) * r, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return MACHIP_OK;
}

// The history sized for K picks and, once per handle, the seeds run through it: tree scores, then per seed k_esp_tree_row,
// the z product, its c, and k_esp_update over the candidates; the scores after the last seed are kept in s0.
inline int esp_tree_prepare(machip_esp* h, int64_t K) {
    EspTreeState* t = h->tr;
    ST_TRY(esp_history_reserve(h, t->seeds, t->seeded && t->seeds > 0, K));
    if (t->seeded) return MACHIP_OK;
    const EspView V = h->view();
    const EspTreeView T = t->view(h->n);
    hipStream_t st = h->stream;
    const int P = h->grid_m(), rg = esp_rows_grid(h->ld);
    h->live = false;
    HIP_TRY(hipMemsetAsync(h->sel, 0, sizeof(int) * (size_t)std::max(h->m, 1), st));
    k_esp_tree_scores<<<P, kBlock, 0, st>>>(V, T);
    EspView Vs = V;                  // the seeds as candidates: the z kernels take their edge, and leave their record, here
    Vs.m = t->seeds; Vs.cu = t->su; Vs.cv = t->sv; Vs.cw = t->sw; Vs.s = nullptr; Vs.sel = t->ssel; Vs.order = t->sorder;
    Vs.gain = t->sgain; Vs.best = t->sbest;
    for (int q = 0; q < t->seeds; ++q) {
        k_esp_tree_row<true><<<rg, kBlock, 0, st>>>(Vs, T, t->zrow, q);
        esp_free_z<true>(h, Vs, t->zrow, q, q);
        k_esp_tree_seed_c<<<1, 1, 0, st>>>(Vs, q);
        k_esp_update<<<P, kBlock, 0, st>>>(V, q);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(t->s0, h->s, sizeof(double) * (size_t)std::max(h->m, 1), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    t->seeded = true;
    return MACHIP_OK;
}

}  // namespace machip
