// mac_amd/csrc/esp.h -- GreedyESP (Khosoussi et al., "Tree-connectivity", arXiv:1604.01116, Algorithm 1) on the device.
//
// The greedy that maximises the weighted number of spanning trees: with node 0 pinned, L_red the fixed graph's reduced
// Laplacian (n' = n - 1) and  Sigma = (L_red + beta I)^-1,  every candidate e = (u, v, w) scores  s_e = w a_e^T Sigma a_e  (its
// weighted effective resistance; a_e = e_{u-1} - e_{v-1}, node-0 terms dropped).  Each step takes the argmax e* (ties: lowest
// index), then adds it to the graph by Sherman-Morrison:
//     z = Sigma a_{e*},   c = w* / (1 + s*),   Sigma <- Sigma - c z z^T,   s_e <- s_e - w_e c (z_u - z_v)^2.
// Sigma lives dense in HBM (fp64, leading dimension n' rounded up to 64).  The rank-1 updates are not applied one by one
// (16 n'^2 bytes each: 1.6 GB at n' = 10^4): the last j <= B pending z's stay in Zb (ld x B, with their c's) and the z of the
// next step is  Sigma[u,:] - Sigma[v,:] - Zb diag(c) (Zb[u,:] - Zb[v,:])^T;  every B steps  Sigma <- Sigma - Zb diag(c) Zb^T  on
// the f64 matrix cores ("fold").  Per step three launches: k_esp_z (z into Zb, order / gain), k_esp_update (all m scores +
// per-workgroup (max, lowest index) partials), k_esp_argmax (one workgroup); no host round trip until the last budget.
//
// Sigma0, the inverse of the fixed graph:
//   * chain form: F is exactly the path (i, i+1), i = 0..n-2 (parallel links summed) -> Sigma0_ij = R[min(i, j)] with R the
//     prefix sums of 1 / w_link (the resistance from node 0): one fill kernel;
//   * general form: the dense L_red + beta I inverted by the blocked Gauss-Jordan elimination of woodbury.h (k_gj_step, ld / 32
//     launches, ping-pong between the handle's two ld x ld buffers -- the second one is the working copy afterwards).
// beta (mac/solvers/greedy_esp.py of the reference: Cholesky with beta = 0, else beta = 1e-4 unless a reduced row is all zero)
// is decided on the host by a union-find over F: connected -> 0; some node other than 0 without a fixed edge -> error; else 1e-4.
// Host side, after the handle: the greedy loop of every route (esp_select_run) and machip_esp_create's pieces.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "plan.h"
#include "woodbury.h"

namespace machip {

constexpr int kEspChainMaxN = 32768;   // chain form: 2 x 8.6 GB of Sigma at the limit
constexpr int kEspDenseMaxN = 16384;   // general form: 512 Gauss-Jordan launches over 2 x 2.1 GB (k_gj_step indexes with int: ld^2 < 2^31)
constexpr int kEspFormFree = 2;        // machip_esp::form of MACHIP_ESP_MATRIX_FREE: no Sigma at all, no n limit (esp_free.h)
constexpr int kEspFormTree = 3;        // machip_esp::form of MACHIP_ESP_MATRIX_FREE | MACHIP_ESP_SPANNING_TREE (esp_tree.h)
// machip_esp::relax_space, what machip_esp_relax_info reports: the nodes (esp_relax.h), the candidates of a chain handle
// (MACHIP_ESP_EDGE_RELAX, esp_relax_edge.h), the candidates and seeds of a spanning-tree handle (MACHIP_ESP_EDGE_RELAX_TREE, esp_relax_edge_tree.h)
enum EspRelaxSpace : int { kEspRelaxNode = 0, kEspRelaxEdge = 1, kEspRelaxEdgeTree = 2 };
constexpr int kEspMaxFold = 256;
constexpr int kEspDefaultFold = 64;
constexpr int kEspGrid = 256;          // workgroups of the score / update pass (= partials of the argmax)
constexpr int kEspGjLookMin = 1024;    // look-ahead pivot blocks from this many rows on (solver_lob.h: option gj_look_min)

struct EspBest {
    double val;
    int idx;
    int pad;
};

struct EspView {
    int np, ld, m;
    const int *cu, *cv;     // reduced endpoints (node - 1; -1 = node 0)
    const double* cw;
    double* s;              // current scores w_e r_e
    int* sel;               // 1 = selected in this run
    double *Zb, *cb;        // pending columns of the low-rank block (ld x fold, column b at Zb + b ld) and their c's
    double* pv;             // per-workgroup partials of the argmax
    int* pi;
    EspBest* best;
    int* order;
    double* gain;
    int* bad;
};

// (v2, i2) beats (v, i): larger value, then lower index.  NaN never wins.
__device__ __forceinline__ void esp_better(double& v, int& i, double v2, int i2) {
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}
// Workgroup (256 threads) argmax: every thread gets the winner.  The winner of a total order does not depend on the
// reduction order -- deterministic.
__device__ __forceinline__ void esp_block_argmax(double& v, int& i, double* sv, int* si) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double v2 = __shfl_xor(v, o, kWave);
        const int i2 = __shfl_xor(i, o, kWave);
        esp_better(v, i, v2, i2);
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sv[w] = v; si[w] = i; }
    __syncthreads();
    v = sv[0]; i = si[0];
#pragma unroll
    for (int q = 1; q < kBlock / kWave; ++q) esp_better(v, i, sv[q], si[q]);
}

// ---- Sigma0, chain form: Sigma_ij = R[min(i, j)] inside n' x n', identity beyond.  grid = (ceil(ld / 256), ld) ----
__global__ __launch_bounds__(kBlock) void k_esp_chain_fill(double* __restrict__ S, const double* __restrict__ R, int np, int ld) {
    const int i = blockIdx.y, j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= ld) return;
    S[(size_t)i * ld + j] = (i < np && j < np) ? R[min(i, j)] : (i == j ? 1.0 : 0.0);
}

// ---- Sigma0, general form: the non-zeros of L_red + beta I (identity beyond n') into a zeroed ld x ld buffer ----
__global__ __launch_bounds__(kBlock) void k_esp_scatter(double* __restrict__ S, const int64_t* __restrict__ pos,
                                                        const double* __restrict__ val, int cnt) {
    for (int e = blockIdx.x * kBlock + threadIdx.x; e < cnt; e += gridDim.x * kBlock) S[pos[e]] = val[e];
}

// s_e = w (S_uu + S_vv - 2 S_uv), node-0 terms 0; the off-diagonal entry is read from the upper triangle (a pair and its
// reverse score the same bits).
__device__ __forceinline__ double esp_score(const double* __restrict__ S, int ld, int u, int v, double w) {
    const double uu = u >= 0 ? S[(size_t)u * ld + u] : 0.0;
    const double vv = v >= 0 ? S[(size_t)v * ld + v] : 0.0;
    const double uv = (u >= 0 && v >= 0) ? S[(size_t)min(u, v) * ld + max(u, v)] : 0.0;
    return w * (uu + vv - 2.0 * uv);
}

// ---- score pass: s_e for all m from S (no pending block); mask != 0: partials of the argmax over the unselected ----
__global__ __launch_bounds__(kBlock) void k_esp_scores(EspView V, const double* __restrict__ S, int mask) {
    __shared__ double sv[kBlock / kWave];
    __shared__ int si[kBlock / kWave];
    double bv = -INFINITY;
    int bi = INT_MAX;
    for (int e = blockIdx.x * kBlock + threadIdx.x; e < V.m; e += gridDim.x * kBlock) {
        const double s = esp_score(S, V.ld, V.cu[e], V.cv[e], V.cw[e]);
        V.s[e] = s;
        if (mask && !V.sel[e]) esp_better(bv, bi, s, e);
    }
    if (!mask) return;
    esp_block_argmax(bv, bi, sv, si);
    if (threadIdx.x == 0) { V.pv[blockIdx.x] = bv; V.pi[blockIdx.x] = bi; }
}

// ---- final argmax over the P partials: one workgroup ----
__global__ __launch_bounds__(kBlock) void k_esp_argmax(EspView V, int P) {
    __shared__ double sv[kBlock / kWave];
    __shared__ int si[kBlock / kWave];
    double bv = -INFINITY;
    int bi = INT_MAX;
    for (int p = threadIdx.x; p < P; p += kBlock) esp_better(bv, bi, V.pv[p], V.pi[p]);
    esp_block_argmax(bv, bi, sv, si);
    if (threadIdx.x == 0) {
        if (bi < 0 || bi >= V.m) {      // no finite score among the unselected: flag it, keep the next launch in bounds
            *V.bad = 1;
            bi = 0;
            bv = 0.0;
        }
        V.best->val = bv;
        V.best->idx = bi;
    }
}

// ---- z = Sigma a_e = S[u,:] - S[v,:] - sum_{b<j} alpha_b Zb[:,b],  alpha_b = c_b (Zb[u,b] - Zb[v,b])  (shared with eig.h) ----
// the alphas of the j pending columns into LDS (the caller synchronises before esp_z_entry)
__device__ __forceinline__ void esp_z_alpha(const EspView& V, int u, int v, int j, double* alpha) {
    for (int b = threadIdx.x; b < j; b += kBlock) {
        const double* zc = V.Zb + (size_t)b * V.ld;
        alpha[b] = V.cb[b] * ((u >= 0 ? zc[u] : 0.0) - (v >= 0 ? zc[v] : 0.0));
    }
}
// entry i of z (0 for the padding rows n'..ld: the fold reads whole tiles)
__device__ __forceinline__ double esp_z_entry(const EspView& V, const double* __restrict__ S, int u, int v, int j, const double* alpha, int i) {
    if (i >= V.np) return 0.0;
    const size_t ld = V.ld;
    double z = (u >= 0 ? S[(size_t)u * ld + i] : 0.0) - (v >= 0 ? S[(size_t)v * ld + i] : 0.0);
    for (int b = 0; b < j; ++b) z = __builtin_fma(-alpha[b], V.Zb[(size_t)b * ld + i], z);
    return z;
}

// the step's record, by one thread: winner e is pick k and column j of the low-rank block (shared with esp_free.h)
__device__ __forceinline__ void esp_record_step(const EspView& V, int e, int j, int k) {
    const double sstar = V.best->val;
    V.cb[j] = V.cw[e] / (1.0 + sstar);
    V.order[k] = e;
    V.gain[k] = sstar;
    V.sel[e] = 1;
}

// ---- the z of the step's winner into Zb[:,j].  grid = ceil(ld / 256).  Workgroup 0 records the step. ----
__global__ __launch_bounds__(kBlock) void k_esp_z(EspView V, const double* __restrict__ S, int j, int k) {
    __shared__ double alpha[kEspMaxFold];
    const int e = V.best->idx;
    const int u = V.cu[e], v = V.cv[e];
    esp_z_alpha(V, u, v, j, alpha);
    __syncthreads();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < V.ld) V.Zb[(size_t)j * V.ld + i] = esp_z_entry(V, S, u, v, j, alpha, i);
    if (blockIdx.x == 0 && threadIdx.x == 0) esp_record_step(V, e, j, k);
}

// ---- s_e <- s_e - w_e c (z_u - z_v)^2 for all m, z = Zb[:,j]; partials of the argmax over the unselected ----
__global__ __launch_bounds__(kBlock) void k_esp_update(EspView V, int j) {
    __shared__ double sv[kBlock / kWave];
    __shared__ int si[kBlock / kWave];
    const double* z = V.Zb + (size_t)j * V.ld;
    const double c = V.cb[j];
    double bv = -INFINITY;
    int bi = INT_MAX;
    for (int e = blockIdx.x * kBlock + threadIdx.x; e < V.m; e += gridDim.x * kBlock) {
        const int u = V.cu[e], v = V.cv[e];
        const double d = (u >= 0 ? z[u] : 0.0) - (v >= 0 ? z[v] : 0.0);
        const double s = V.s[e] - V.cw[e] * c * d * d;
        V.s[e] = s;
        if (!V.sel[e]) esp_better(bv, bi, s, e);
    }
    esp_block_argmax(bv, bi, sv, si);
    if (threadIdx.x == 0) { V.pv[blockIdx.x] = bv; V.pi[blockIdx.x] = bi; }
}

// ---- fold: S <- S - Zb[:, :j] diag(c) Zb[:, :j]^T on the matrix cores.  Workgroup = one 64 x 64 tile (grid = tiles x tiles),
// wave = a 32 x 32 quadrant of 2 x 2 v_mfma_f64_16x16x4_f64 blocks (the tile idiom of k_gj_step): A[i = l & 15][k = l >> 4] =
// -c_k Zb[row i, k], B[k = l >> 4][j = l & 15] = Zb[col j, k], accumulator = the tile itself in the result layout
// D[row = (l >> 4) + 4 reg][col = l & 15].  Zb's 4 columns of a k-step come from L2 (ld x j doubles, shared by all tiles). ----
__global__ __launch_bounds__(256) void k_esp_fold(double* __restrict__ S, const double* __restrict__ Zb, const double* __restrict__ cb,
                                                  int ld, int j) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int li = lane & 15, lk = lane >> 4, wr = wv >> 1, wc = wv & 1;
    const int r0 = blockIdx.y * kGjT + 32 * wr, c0 = blockIdx.x * kGjT + 32 * wc;
    gj_d4 acc[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[bi][bj][q] = S[(size_t)(r0 + 16 * bi + lk + 4 * q) * ld + c0 + 16 * bj + li];
    for (int kk = 0; kk < (j + 3) / 4; ++kk) {
        const int k = 4 * kk + lk;
        const bool ok = k < j;
        const double* zc = Zb + (size_t)(ok ? k : 0) * ld;
        const double nc = ok ? -cb[k] : 0.0;
        double a[2], b[2];
#pragma unroll
        for (int bi = 0; bi < 2; ++bi) a[bi] = ok ? nc * zc[r0 + 16 * bi + li] : 0.0;
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) b[bj] = ok ? zc[c0 + 16 * bj + li] : 0.0;
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[bi], b[bj], acc[bi][bj], 0, 0, 0);
    }
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int q = 0; q < 4; ++q) S[(size_t)(r0 + 16 * bi + lk + 4 * q) * ld + c0 + 16 * bj + li] = acc[bi][bj][q];
}

struct EspRelax;      // esp_relax.h: the state of the convex relaxation, made by the first relaxation call
struct EspTreeState;  // esp_tree.h: the spanning tree's tables and the seeds of a MACHIP_ESP_SPANNING_TREE handle
struct EspXch;        // esp_exchange.h: the rows of Sigma the exchange keeps, made by the first exchange call
struct EspXchEdge;    // esp_exchange_edge.h: the view and the rows of the edge-space exchange, made by its first call
struct EspKir;        // kirchhoff.h: the arrays of the A-optimal greedy, made by the first Kirchhoff call

}  // namespace machip

// ---- the handle (include/machip.h: machip_esp) ----
struct machip_esp {
    int device = 0;
    hipStream_t stream = nullptr;
    int n = 0, np = 0, ld = 0, m = 0, fold = machip::kEspDefaultFold;
    machip::EspRelaxSpace relax_space = machip::kEspRelaxNode;      // the space the relaxation and the edge-space exchange work in (esp_relax.h: esp_relax_route)
    int form = 0;                 // 0 chain, 1 general (dense Gauss-Jordan inverse), 2 chain without Sigma (esp_free.h), 3 spanning tree without Sigma (esp_tree.h)
    double beta = 0.0;
    double *R = nullptr, *part = nullptr;      // form 2: the chain's prefix resistances (n'); forms 2, 3: the column slices' partial sums
    size_t zcap = 0;              // forms 2, 3: columns Zb / cb are allocated for (the history of the largest budget so far; form 3: seeds included)
    int free_split = 0;           // forms 2, 3: option esp_free_split when the handle was made (0 = automatic)
    double *bufA = nullptr, *bufB = nullptr;
    double* sig0 = nullptr;       // pristine Sigma0 (one of bufA / bufB)
    double* sig = nullptr;        // working copy (the other one)
    bool live = false;            // sig holds the state after the last selection run
    int pending = 0;              // columns of Zb not yet folded into sig (form 2: the picks of the last run, never folded)
    int *cu = nullptr, *cv = nullptr, *sel = nullptr, *pi = nullptr, *order = nullptr, *bad = nullptr;
    double *cw = nullptr, *s = nullptr, *Zb = nullptr, *cb = nullptr, *pv = nullptr, *gain = nullptr, *piv = nullptr;
    machip::EspBest* best = nullptr;
    std::vector<hipEvent_t> ev;
    std::vector<int32_t> hfi, hfj, hci, hcj;      // the edge lists as given (host): esp_relax.h builds its incidence list from them
    std::vector<double> hfw, hcw;
    machip::EspRelax* rx = nullptr;
    machip::EspTreeState* tr = nullptr;
    machip::EspXch* xc = nullptr;
    machip::EspXchEdge* xe = nullptr;
    machip::EspKir* kr = nullptr;

    machip::EspView view() const {
        machip::EspView V;
        V.np = np; V.ld = ld; V.m = m; V.cu = cu; V.cv = cv; V.cw = cw; V.s = s; V.sel = sel; V.Zb = Zb; V.cb = cb;
        V.pv = pv; V.pi = pi; V.best = best; V.order = order; V.gain = gain; V.bad = bad;
        return V;
    }
    int grid_m() const { return std::max(1, std::min(machip::kEspGrid, (m + machip::kBlock - 1) / machip::kBlock)); }
    bool matrix_free() const { return form == machip::kEspFormFree || form == machip::kEspFormTree; }

    // at least n events in ev (ev[0], ev[1 + b]: a run's start and its budgets; the exchange's clock takes those from ev[2] on)
    int events(size_t n) {
        while (ev.size() < n) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            ev.push_back(e);
        }
        return MACHIP_OK;
    }
    // the working copy back to Sigma0
    int load_sigma0() {
        HIP_TRY(hipMemcpyAsync(sig, sig0, sizeof(double) * (size_t)ld * (size_t)ld, hipMemcpyDeviceToDevice, stream));
        return MACHIP_OK;
    }

    // A^-1 of the ld x ld matrix in `src`: ld / 32 blocked Gauss-Jordan steps on the matrix cores, ping-pong between src and dst,
    // look-ahead pivot blocks from 1 024 rows on -- exactly as solver_lob.h inverts the capacitance matrix (woodbury.h).  The result
    // is in `src` afterwards (the pointers are swapped per step); *bad <- 1 on a non-positive pivot.  LD: the pivot blocks'
    // log-determinants into ldet[ld / 32] as well.
    template <bool LD>
    void gj_inverse(double*& src, double*& dst, double* ldet = nullptr) { gj_inverse_of<LD>(src, dst, ld, piv, ldet); }

    // The same for a matrix of leading dimension `ldm` (a multiple of 64) with the look-ahead pivot buffer `pv2` (2 x 32 x 32
    // doubles): the handle's own (ld, piv) above, the edge-space relaxation's (esp_relax_edge.h).
    template <bool LD>
    void gj_inverse_of(double*& src, double*& dst, int ldm, double* pv2, double* ldet) {
        using namespace machip;
        const int tiles = ldm / kGjT;
        const bool look = ldm >= kEspGjLookMin;
        for (int kb = 0, k = 0; kb < ldm; kb += kGjB, ++k) {
            if (look) k_gj_step<0, LD><<<dim3(tiles, tiles), 256, 0, stream>>>(src, dst, ldm, kb, bad, k ? pv2 + (size_t)(k & 1) * kGjB * kGjB : nullptr,
                                                                               pv2 + (size_t)((k + 1) & 1) * kGjB * kGjB, ldet);
            else k_gj_step<0, LD><<<dim3(tiles, tiles), 256, 0, stream>>>(src, dst, ldm, kb, bad, nullptr, nullptr, ldet);
            std::swap(src, dst);
        }
    }

    // Sigma <- Sigma - Zb diag(c) Zb^T over the j pending columns
    void fold_into(double* S, int j) {
        if (j <= 0) return;
        const int tiles = ld / machip::kGjT;
        machip::k_esp_fold<<<dim3(tiles, tiles), 256, 0, stream>>>(S, Zb, cb, ld, j);
    }
};

namespace machip {

// a host callable of the launch-bound loops (a route's step, a space's hook): always expanded in the loop that calls it
#define ESP_INLINE __attribute__((always_inline)) inline

// workgroups of a kernel with one thread per row of an ld-row matrix or vector
inline int esp_rows_grid(int ld) { return (ld + kBlock - 1) / kBlock; }

// ---- the greedy loop of every route (esp_select.h supplies the routes) ----
// One selection run (the caller has checked the budgets: m >= K >= 1).  start(V, P): the scores and the argmax partials of the
// fixed graph; zstep(V, k): the z of pick k into the column it returns.  A handle that keeps Sigma restarts it from Sigma0 and
// folds a full Zb into it; one that does not (fold = 0) keeps every pick pending.  Per pick: the route's z, k_esp_update and
// k_esp_argmax unless it is the last, the budgets' events; then the results and the budgets' times to the host.
template <class Start, class ZStep>
inline int esp_select_run(machip_esp* h, int nb, const int64_t* ks, Start start, ZStep zstep, int32_t* order_out, double* gain_out,
                          double* t_ms_out) {
    const int K = (int)ks[nb - 1], B = h->fold, P = h->grid_m();
    ST_TRY(h->events((size_t)nb + 1));
    const EspView V = h->view();
    hipStream_t st = h->stream;
    h->live = false;
    HIP_TRY(hipEventRecord(h->ev[0], st));
    if (h->sig0) ST_TRY(h->load_sigma0());
    HIP_TRY(hipMemsetAsync(h->sel, 0, sizeof(int) * (size_t)h->m, st));
    HIP_TRY(hipMemsetAsync(h->bad, 0, sizeof(int), st));
    start(V, P);
    k_esp_argmax<<<1, kBlock, 0, st>>>(V, P);
    for (int k = 0, b = 0; k < K; ++k) {
        const int j = zstep(V, k);
        if (k + 1 < K) {
            k_esp_update<<<P, kBlock, 0, st>>>(V, j);
            k_esp_argmax<<<1, kBlock, 0, st>>>(V, P);
        }
        if (j == B - 1) h->fold_into(h->sig, B);
        while (b < nb && ks[b] == k + 1) HIP_TRY(hipEventRecord(h->ev[1 + b++], st));
    }
    HIP_TRY(hipGetLastError());
    h->pending = B ? K % B : K;
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
    if (hbad) return fail(MACHIP_NOT_CONVERGED, "no finite score among the unselected candidates");
    return MACHIP_OK;
}

// ---- machip_esp_create in pieces ----

// The refusals decided from the arguments alone, in the order the tests know.  fold: 0 becomes the default.
inline int esp_create_check(int64_t n, int64_t n_fixed, const int32_t* fi, const int32_t* fj, const double* fw, int64_t m, const int32_t* ci,
                            const int32_t* cj, const double* cw, int& fold, int flags) {
    if (n < 2) return fail(MACHIP_BAD_ARG, "num_nodes must be at least 2");
    if (n_fixed < 0 || m < 0 || m > 2000000000ll) return fail(MACHIP_BAD_ARG, "bad edge counts");
    if ((n_fixed && (!fi || !fj || !fw)) || (m && (!ci || !cj || !cw))) return fail(MACHIP_BAD_ARG, "NULL edge array");
    const int fold_given = fold;
    if (fold == 0) fold = kEspDefaultFold;
    if (fold < 1 || fold > kEspMaxFold) return fail(MACHIP_BAD_ARG, "fold must be in [1, 256]");
    if (flags & ~(MACHIP_ESP_DENSE_INVERSE | MACHIP_ESP_MATRIX_FREE | MACHIP_ESP_SPANNING_TREE | MACHIP_ESP_EDGE_RELAX | MACHIP_ESP_EDGE_RELAX_TREE))
        return fail(MACHIP_BAD_ARG, "unknown flags");
    const bool mfree = (flags & MACHIP_ESP_MATRIX_FREE) != 0, tree = (flags & MACHIP_ESP_SPANNING_TREE) != 0;
    const bool edge = (flags & MACHIP_ESP_EDGE_RELAX) != 0, etree = (flags & MACHIP_ESP_EDGE_RELAX_TREE) != 0;
    if (etree && edge)
        return fail(MACHIP_BAD_ARG, "MACHIP_ESP_EDGE_RELAX_TREE builds the Gram matrix from the spanning tree, MACHIP_ESP_EDGE_RELAX from the chain: the two cannot be combined");
    if (etree && (flags & MACHIP_ESP_DENSE_INVERSE))
        return fail(MACHIP_BAD_ARG, "MACHIP_ESP_EDGE_RELAX_TREE takes Sigma0 from the spanning tree's closed form: it cannot be combined with MACHIP_ESP_DENSE_INVERSE");
    if (etree && !(mfree && tree))      // (without its partners the bit was an unknown flag before the route existed, and stays one)
        return fail(MACHIP_BAD_ARG, "unknown flags: MACHIP_ESP_EDGE_RELAX_TREE puts the relaxation on the spanning-tree handle and is valid only together with MACHIP_ESP_MATRIX_FREE | MACHIP_ESP_SPANNING_TREE");
    if (edge && !mfree)      // (alone the bit was an unknown flag before the route existed, and stays one: the message keeps saying so)
        return fail(MACHIP_BAD_ARG, "unknown flags: MACHIP_ESP_EDGE_RELAX puts the relaxation on the chain-free handle and is valid only together with MACHIP_ESP_MATRIX_FREE");
    if (edge && (flags & MACHIP_ESP_DENSE_INVERSE))
        return fail(MACHIP_BAD_ARG, "MACHIP_ESP_EDGE_RELAX takes Sigma0 from the chain's closed form: it cannot be combined with MACHIP_ESP_DENSE_INVERSE");
    if (edge && tree)
        return fail(MACHIP_BAD_ARG, "MACHIP_ESP_EDGE_RELAX has the chain's closed form only: it cannot be combined with MACHIP_ESP_SPANNING_TREE");
    if (tree && !mfree)
        return fail(MACHIP_BAD_ARG, "MACHIP_ESP_SPANNING_TREE selects the spanning tree of the matrix-free route: it is valid only together with MACHIP_ESP_MATRIX_FREE");
    if (mfree && fold_given != 0)      // (an argument that would be ignored is refused, not dropped: nothing is ever folded here)
        return fail(MACHIP_BAD_ARG, "MACHIP_ESP_MATRIX_FREE never folds: fold has no meaning on this route and must be 0");
    if (mfree && (flags & MACHIP_ESP_DENSE_INVERSE))
        return fail(MACHIP_BAD_ARG, "MACHIP_ESP_MATRIX_FREE keeps no Sigma: it cannot be combined with MACHIP_ESP_DENSE_INVERSE");
    if (mfree && n > (int64_t)INT_MAX - kGjT) return fail(MACHIP_BAD_ARG, "node ids are int32: num_nodes is too large");
    if (!mfree && n > kEspChainMaxN) return fail(MACHIP_BAD_ARG, "GreedyESP keeps (L_red + beta I)^-1 dense: num_nodes must be <= 32768 (chain-fixed graphs), <= 16384 otherwise");
    for (int64_t e = 0; e < n_fixed; ++e)
        if (fi[e] < 0 || fi[e] >= n || fj[e] < 0 || fj[e] >= n || !std::isfinite(fw[e])) return fail(MACHIP_BAD_ARG, "fixed edge out of range or weight not finite");
    for (int64_t e = 0; e < m; ++e)
        if (ci[e] < 0 || ci[e] >= n || cj[e] < 0 || cj[e] >= n || !std::isfinite(cw[e])) return fail(MACHIP_BAD_ARG, "candidate edge out of range or weight not finite");
    return MACHIP_OK;
}

// What the fixed graph is: beta, and the chain's links when F is exactly the path (i, i+1).
struct EspFixedClass {
    double beta = 0.0;
    bool chain = false;
    std::vector<double> link;      // chain: the summed weight of link (i, i+1)
};

// beta (the reference: Cholesky with beta = 0; on failure raise if a reduced row is all zero, else beta = 1e-4), decided by a
// union-find over F; the chain form; and what the flags ask of the graph and it is not.
inline int esp_classify_fixed(int64_t n, int64_t n_fixed, const int32_t* fi, const int32_t* fj, const double* fw, int flags, EspFixedClass& C) {
    const bool mfree = (flags & MACHIP_ESP_MATRIX_FREE) != 0, tree = (flags & MACHIP_ESP_SPANNING_TREE) != 0;
    const int N = (int)n, np = N - 1;
    std::vector<int> par(N), has(N, 0);
    std::iota(par.begin(), par.end(), 0);
    auto root = [&](int a) { while (par[a] != a) { par[a] = par[par[a]]; a = par[a]; } return a; };
    int comps = N;
    for (int64_t e = 0; e < n_fixed; ++e) {
        if (fi[e] == fj[e] || fw[e] == 0.0) continue;
        has[fi[e]] = has[fj[e]] = 1;
        const int a = root(fi[e]), b = root(fj[e]);
        if (a != b) { par[a] = b; --comps; }
    }
    if (tree && comps > 1)
        return fail(MACHIP_BAD_ARG, "the spanning-tree route needs a connected fixed graph: the fixed edges leave " + std::to_string(comps) + " components");
    if (comps > 1) {
        for (int i = 1; i < N; ++i)
            if (!has[i]) return fail(MACHIP_DISCONNECTED, "node " + std::to_string(i) + " has no fixed edge: row " + std::to_string(i - 1) + " of L_fixed is all zeros");
        C.beta = 1e-4;
    }
    // chain form: F is exactly the path (i, i+1), parallel links summed
    C.link.assign((size_t)np, 0.0);
    C.chain = !(flags & MACHIP_ESP_DENSE_INVERSE) && comps == 1 && !tree;
    for (int64_t e = 0; C.chain && e < n_fixed; ++e) {
        const int a = std::min(fi[e], fj[e]), b = std::max(fi[e], fj[e]);
        if (b != a + 1) C.chain = false;
        else C.link[(size_t)a] += fw[e];
    }
    for (int i = 0; C.chain && i < np; ++i) if (!(C.link[(size_t)i] > 0.0)) C.chain = false;
    if (mfree && !tree && !C.chain)
        return fail(MACHIP_BAD_ARG, std::string("the matrix-free route needs a chain: the fixed edges must be exactly the connected path (i, i+1), i = 0..n-2 (parallel links summed)") +
                                        ((flags & MACHIP_ESP_EDGE_RELAX) ? "; MACHIP_ESP_EDGE_RELAX builds the candidates' Gram matrix from that chain's resistances" : ""));
    if (!C.chain && !tree && n > kEspDenseMaxN)
        return fail(MACHIP_BAD_ARG, "GreedyESP inverts L_red + beta I densely when the fixed edges are not exactly the chain (i, i+1): num_nodes must be <= 16384");
    return MACHIP_OK;
}

// The stream and every array of a fresh handle (n, m, ld, fold, form and the host edge lists are set); the candidates go up.
inline int esp_alloc(machip_esp* h) {
    HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    const bool mfree = h->matrix_free();
    const int64_t m = h->m;
    const size_t ld = (size_t)h->ld, ms = (size_t)std::max<int64_t>(m, 1), fold = (size_t)h->fold;
    if (!mfree) { ST_TRY(dev_alloc(&h->bufA, ld * ld)); ST_TRY(dev_alloc(&h->bufB, ld * ld)); }
    ST_TRY(dev_alloc(&h->cu, ms)); ST_TRY(dev_alloc(&h->cv, ms)); ST_TRY(dev_alloc(&h->cw, ms)); ST_TRY(dev_alloc(&h->s, ms));
    ST_TRY(dev_alloc(&h->sel, ms)); ST_TRY(dev_alloc(&h->order, ms)); ST_TRY(dev_alloc(&h->gain, ms));
    if (!mfree) { ST_TRY(dev_alloc(&h->Zb, ld * fold)); ST_TRY(dev_alloc(&h->cb, fold)); }      // (matrix-free: the select sizes the history)
    ST_TRY(dev_alloc(&h->pv, (size_t)kEspGrid)); ST_TRY(dev_alloc(&h->pi, (size_t)kEspGrid)); ST_TRY(dev_alloc(&h->best, 1));
    ST_TRY(dev_alloc(&h->bad, 1)); ST_TRY(dev_alloc(&h->piv, (size_t)2 * kGjB * kGjB));
    if (!mfree) {
        HIP_TRY(hipMemsetAsync(h->Zb, 0, sizeof(double) * ld * fold, h->stream));
        HIP_TRY(hipMemsetAsync(h->cb, 0, sizeof(double) * fold, h->stream));
    }
    HIP_TRY(hipMemsetAsync(h->bad, 0, sizeof(int), h->stream));
    if (m) {
        std::vector<int> u((size_t)m), v((size_t)m);
        for (int64_t e = 0; e < m; ++e) { u[(size_t)e] = h->hci[(size_t)e] - 1; v[(size_t)e] = h->hcj[(size_t)e] - 1; }
        HIP_TRY(hipMemcpyAsync(h->cu, u.data(), sizeof(int) * (size_t)m, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(h->cv, v.data(), sizeof(int) * (size_t)m, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(h->cw, h->hcw.data(), sizeof(double) * (size_t)m, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));     // (host staging goes out of scope)
    }
    return MACHIP_OK;
}

// Sigma0, chain form: R = the prefix sums of 1 / w_link.  A matrix-free handle keeps R and nothing else; a dense one fills bufA from it.
inline int esp_sigma0_chain(machip_esp* h, const std::vector<double>& link) {
    const int np = h->np;
    std::vector<double> R((size_t)np);
    double acc = 0.0;
    for (int i = 0; i < np; ++i) { acc += 1.0 / link[(size_t)i]; R[(size_t)i] = acc; }
    double* dR = nullptr;
    ST_TRY(dev_alloc(&dR, (size_t)np));
    HIP_TRY(hipMemcpyAsync(dR, R.data(), sizeof(double) * (size_t)np, hipMemcpyHostToDevice, h->stream));
    if (h->matrix_free()) {                           // R is all of Sigma0 this route keeps
        h->R = dR;
        HIP_TRY(hipStreamSynchronize(h->stream));
        return MACHIP_OK;
    }
    k_esp_chain_fill<<<dim3((unsigned)esp_rows_grid(h->ld), (unsigned)h->ld), kBlock, 0, h->stream>>>(h->bufA, dR, np, h->ld);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    (void)hipFree(dR);
    h->sig0 = h->bufA; h->sig = h->bufB;
    return MACHIP_OK;
}

// Sigma0, general form: dense L_red + beta I (identity beyond n'), entries summed on the host in edge order, then inverted by
// the blocked Gauss-Jordan elimination (gj_inverse).
inline int esp_sigma0_dense(machip_esp* h) {
    const int np = h->np;
    const size_t ld = (size_t)h->ld;
    std::vector<double> diag((size_t)np, h->beta);
    std::vector<std::pair<int64_t, double>> off;
    off.reserve(h->hfw.size());
    for (size_t e = 0; e < h->hfw.size(); ++e) {
        const int a = h->hfi[e] - 1, b = h->hfj[e] - 1;
        const double w = h->hfw[e];
        if (a == b) continue;
        if (a >= 0) diag[(size_t)a] += w;
        if (b >= 0) diag[(size_t)b] += w;
        if (a >= 0 && b >= 0) off.emplace_back((int64_t)std::min(a, b) * (int64_t)ld + std::max(a, b), w);
    }
    std::stable_sort(off.begin(), off.end(), [](const std::pair<int64_t, double>& x, const std::pair<int64_t, double>& y) { return x.first < y.first; });
    std::vector<int64_t> pos;
    std::vector<double> val;
    for (int i = 0; i < (int)ld; ++i) { pos.push_back((int64_t)i * (int64_t)ld + i); val.push_back(i < np ? diag[(size_t)i] : 1.0); }
    for (size_t q = 0; q < off.size();) {
        size_t r = q;
        double w = 0.0;
        for (; r < off.size() && off[r].first == off[q].first; ++r) w += off[r].second;
        const int64_t a = off[q].first / (int64_t)ld, b = off[q].first % (int64_t)ld;
        pos.push_back(a * (int64_t)ld + b); val.push_back(-w);
        pos.push_back(b * (int64_t)ld + a); val.push_back(-w);
        q = r;
    }
    int64_t* dpos = nullptr;
    double* dval = nullptr;
    ST_TRY(dev_alloc(&dpos, pos.size())); ST_TRY(dev_alloc(&dval, val.size()));
    HIP_TRY(hipMemsetAsync(h->bufA, 0, sizeof(double) * ld * ld, h->stream));
    HIP_TRY(hipMemcpyAsync(dpos, pos.data(), sizeof(int64_t) * pos.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(dval, val.data(), sizeof(double) * val.size(), hipMemcpyHostToDevice, h->stream));
    const int cnt = (int)pos.size();
    k_esp_scatter<<<std::max(1, std::min(kMaxGrid, (cnt + kBlock - 1) / kBlock)), kBlock, 0, h->stream>>>(h->bufA, dpos, dval, cnt);
    double *src = h->bufA, *dst = h->bufB;
    h->gj_inverse<false>(src, dst);
    HIP_TRY(hipGetLastError());
    int hbad = 0;
    HIP_TRY(hipMemcpyAsync(&hbad, h->bad, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    (void)hipFree(dpos); (void)hipFree(dval);
    if (hbad) return fail(MACHIP_NOT_CONVERGED, "L_red + beta I is not positive definite numerically (a non-positive Gauss-Jordan pivot)");
    h->sig0 = src; h->sig = dst;
    return MACHIP_OK;
}

}  // namespace machip
