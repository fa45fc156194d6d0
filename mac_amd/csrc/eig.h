// mac_amd/csrc/eig.h -- GreedyEig (the greedy k-edge selection by algebraic connectivity) on the device.
//
// K times: lambda_2(L_cur + w_e a_e a_e^T) of the unselected candidates e, take the best.  The supergradient bound
// u_e = lambda_2 + w_e (v_i - v_j)^2 (v the current unit Fiedler vector) orders the candidates and prunes: a candidate whose bound
// is below a value already established in the pick is never solved.  The ones that must be solved are solved in batches of B
// columns that share one inverse:  Sigma = L_red^-1 of the current graph is the state of esp.h (this handle owns a machip_esp: its
// Sigma0 by the chain fill or k_gj_step, its pending block Zb / cb, its fold kernel).  With q orthogonal to 1,
//     L_e^+ q = P (Sigma - Zb diag(cb) Zb^T - c_e z_e z_e^T)_ext q,    z_e = Sigma_cur a_e,  c_e = w_e / (1 + w_e a_e^T z_e)
// (Sherman-Morrison; _ext = a zero row / column for node 0, P = centring), so one application for the batch is the dense product
// T = Sigma Q on the f64 matrix cores (k_eig_product) plus rank-(pending + 1) corrections per column.
//
// The eigen-solver per column is the locally optimal three-term recurrence (LOBPCG with one vector) for the pencil (L_e, I) on
// 1-perp with that application as the preconditioner: Rayleigh-Ritz of L_e on span{x, L_e^+ r, p}.  Everything that decides -- the
// Rayleigh quotient lambda = x^T L_e x, the residual r = L_e x - lambda x, the 3 x 3 Gram matrix -- is computed with the sparse L_cur
// (CSR, rebuilt on the host after a pick: row-wise sums, no atomics, bit-reproducible) plus the candidate's own edge; Sigma only
// proposes search directions, so an inexact inverse costs iterations, never accuracy, and cannot certify itself.  A column retires
// when  ||r||_1 / ||L_e||_inf < 1e-8  with ||x||_2 = 1 (the stop rule of the reference's CholeskyFiedlerSolver).  Every column
// starts from the current Fiedler vector.  Per iteration three launches (k_eig_resid, k_eig_product, k_eig_rr) and one 4-byte
// read (the number of columns still active).  On a MACHIP_EIG_MATRIX_FREE handle (form 2 of the machip_esp underneath: no Sigma) k_eig_z
// and k_eig_product are replaced by the scans and history products of eig_free.h (form 3, MACHIP_EIG_MATRIX_FREE_TREE: the sweeps over a
// spanning tree of eig_free_tree.h in the place of the scans): machip_eig::columns / apply / push, which alone ask for the form
// (eig_routes.h, with the handle's creation).  The rest is shared, with eig_exchange.h too: scan, push_column, adopt_pair.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <numeric>
#include <vector>

#include "esp.h"
#include "plan.h"

namespace machip {

constexpr int kEigDefaultBatch = 512;
constexpr int kEigMaxBatch = 4096;
constexpr int kEigDefaultFold = 16;      // a fold costs two passes over Sigma, an application one: fold often, keep the block short
constexpr int kEigMaxIter = 500;
constexpr double kEigTol = 1e-8;         // stop rule (relative l1 residual) and the tie tolerance of the scan

struct EigView {
    int n, np, ld, ldv, ldq;             // nodes, n - 1, leading dimension of Sigma / Z, of node-space vectors, of Q / T (row-major)
    const int* rp; const int* cj; const double* cv; const double* deg;      // CSR of L_cur: off-diagonal weights, weighted degrees
    double maxdeg;
    const int *cu, *cv2;                 // candidates: reduced endpoints (node - 1), weights
    const double* cw;
    const int* bc;                       // candidate of column b (-1: no edge)
    double *X, *P, *W, *LX, *LW, *LP;    // ldv x B, column b at + b ldv
    double *Q, *T;                       // ld x ldq row-major: entry (k, b) at k ldq + b
    double *Z, *cc;                      // z_e of the columns (column b at + b ld), c_e
    double *lam, *res, *rbest;
    int *conv, *iters, *hasp, *stall, *nactive;
    double tol;                          // kEigTol for the candidates; 0 for the pair the next pick starts from: iterate until the residual stalls
};

// y_i = (L_cur x)_i + the candidate's edge (U, V, w) in node numbering (U == V: none)
__device__ __forceinline__ double eig_lrow(const EigView& E, const double* __restrict__ x, int i, int U, int V, double w) {
    double a = E.deg[i] * x[i];
    for (int k = E.rp[i]; k < E.rp[i + 1]; ++k) a = __builtin_fma(-E.cv[k], x[E.cj[k]], a);
    if (U != V) {
        if (i == U) a += w * (x[U] - x[V]);
        if (i == V) a -= w * (x[U] - x[V]);
    }
    return a;
}

// ---- u_e = lambda_2 + w_e (v_i - v_j)^2 for all m candidates ----
__global__ __launch_bounds__(kBlock) void k_eig_bounds(EigView E, const double* __restrict__ v, double lam, int m, double* __restrict__ out) {
    for (int e = blockIdx.x * kBlock + threadIdx.x; e < m; e += gridDim.x * kBlock) {
        const double d = v[E.cu[e] + 1] - v[E.cv2[e] + 1];
        out[e] = lam + E.cw[e] * d * d;
    }
}

// ---- z_e = Sigma_cur a_e for the columns of a batch (pending block applied), c_e.  grid = (ceil(ld / 256), columns).  dst column b
// at dst + b ld; the winner's column goes straight into Zb (dst = Zb + j ld, cdst = cb + j). ----
__global__ __launch_bounds__(kBlock) void k_eig_z(EspView V, const double* __restrict__ S, int j, const int* __restrict__ bc,
                                                  double* __restrict__ dst, double* __restrict__ cdst) {
    __shared__ double alpha[kEspMaxFold];
    const int b = blockIdx.y, e = bc[b];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (e < 0) {
        if (i < V.ld) dst[(size_t)b * V.ld + i] = 0.0;
        if (blockIdx.x == 0 && threadIdx.x == 0) cdst[b] = 0.0;
        return;
    }
    const int u = V.cu[e], v = V.cv[e];
    esp_z_alpha(V, u, v, j, alpha);
    __syncthreads();
    if (i < V.ld) dst[(size_t)b * V.ld + i] = esp_z_entry(V, S, u, v, j, alpha, i);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double s = (u >= 0 ? esp_z_entry(V, S, u, v, j, alpha, u) : 0.0) - (v >= 0 ? esp_z_entry(V, S, u, v, j, alpha, v) : 0.0);
        cdst[b] = V.cw[e] / (1.0 + V.cw[e] * s);
    }
}

// the dense routes' columns (machip_eig::columns): z_e, c_e of the batch against Sigma and the pending block
inline void eig_dense_columns(const machip_esp* base, const EspView& V, const int* bc, int count, double* Z, double* cc) {
    k_eig_z<<<dim3((base->ld + kBlock - 1) / kBlock, count), kBlock, 0, base->stream>>>(V, base->sig, base->pending, bc, Z, cc);
}

// ---- every column starts from v.  grid = (ceil(n / 256), columns) ----
__global__ __launch_bounds__(kBlock) void k_eig_init(EigView E, const double* __restrict__ v) {
    const int b = blockIdx.y, i = blockIdx.x * kBlock + threadIdx.x;
    if (i < E.n) E.X[(size_t)b * E.ldv + i] = v[i];
    if (i == 0) { E.conv[b] = 0; E.iters[b] = 0; E.hasp[b] = 0; E.stall[b] = 0; E.rbest[b] = INFINITY; }
}

// ---- lambda = x^T L_e x, r = L_e x - lambda x, the stop rule; r (nodes 1..) into column b of Q.  One workgroup per column. ----
__global__ __launch_bounds__(kBlock) void k_eig_resid(EigView E) {
    __shared__ double sm[4];
    const int b = blockIdx.x;
    if (E.conv[b]) return;
    const int e = E.bc[b];
    const int U = e >= 0 ? E.cu[e] + 1 : 0, V = e >= 0 ? E.cv2[e] + 1 : 0;
    const double w = e >= 0 ? E.cw[e] : 0.0;
    const double* x = E.X + (size_t)b * E.ldv;
    double* lx = E.LX + (size_t)b * E.ldv;
    double a = 0.0;
    for (int i = threadIdx.x; i < E.n; i += kBlock) {
        const double y = eig_lrow(E, x, i, U, V, w);
        lx[i] = y;
        a = __builtin_fma(x[i], y, a);
    }
    const double lam = block_sum(a, sm);
    double r1 = 0.0;
    for (int i = threadIdx.x; i < E.n; i += kBlock) {
        const double r = lx[i] - lam * x[i];
        r1 += fabs(r);
        if (i > 0) E.Q[(size_t)(i - 1) * E.ldq + b] = r;
    }
    r1 = block_sum(r1, sm);
    if (threadIdx.x == 0) {
        double md = E.maxdeg;
        if (U != V) md = fmax(md, fmax(E.deg[U], E.deg[V]) + w);
        const double res = r1 / (2.0 * md);
        E.lam[b] = lam;
        E.res[b] = res;
        // polishing (tol = 0): done once the stop rule holds and three iterations in a row have not halved the best residual
        int stall = E.stall[b];
        if (res < 0.5 * E.rbest[b]) { E.rbest[b] = res; stall = 0; } else ++stall;
        E.stall[b] = stall;
        if (res < E.tol || (res < kEigTol && stall >= 3)) E.conv[b] = 1;
        else if (E.iters[b] >= kEigMaxIter || !(res == res)) E.conv[b] = 2;
        else atomicAdd(E.nactive, 1);
    }
}

// ---- T = Sigma Q on the matrix cores.  Workgroup = a 64 x 64 tile of T (grid = (ldq / 64, ld / 64)), wave = a 32 x 32 quadrant of
// 2 x 2 v_mfma_f64_16x16x4_f64 blocks, operand layout of k_esp_fold: A[i = l & 15][k = l >> 4] = Sigma[k, row i] (Sigma is symmetric:
// 16 consecutive doubles per k), B[k = l >> 4][j = l & 15] = Q[k, col j], D[row = (l >> 4) + 4 reg][col = l & 15].  A tile whose 64
// columns have all retired is skipped. ----
__global__ __launch_bounds__(256) void k_eig_product(const double* __restrict__ S, EigView E, int count) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int col = blockIdx.x * kGjT + (tid & 63);
    const int live = (tid < 64 && col < count && E.conv[col] == 0) ? 1 : 0;
    if (!__syncthreads_or(live)) return;
    const int li = lane & 15, lk = lane >> 4, wr = wv >> 1, wc = wv & 1;
    const int r0 = blockIdx.y * kGjT + 32 * wr, c0 = blockIdx.x * kGjT + 32 * wc;
    const size_t ld = E.ld, ldq = E.ldq;
    gj_d4 acc[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[bi][bj][q] = 0.0;
    const double* sa = S + (size_t)lk * ld + r0 + li;
    const double* qb = E.Q + (size_t)lk * ldq + c0 + li;
    for (int kk = 0; kk < E.ld / 4; ++kk) {
        double a[2], b[2];
        a[0] = sa[0]; a[1] = sa[16];
        b[0] = qb[0]; b[1] = qb[16];
        sa += 4 * ld; qb += 4 * ldq;
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
            for (int q = 0; q < 4; ++q) E.T[(size_t)(r0 + 16 * bi + lk + 4 * q) * ldq + c0 + 16 * bj + li] = acc[bi][bj][q];
}

// Smallest eigenpair of the symmetric 3 x 3 matrix g (cyclic Jacobi); y = its unit eigenvector.
__device__ inline void eig_jacobi3(double g[3][3], double y[3]) {
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 12; ++sweep) {
        const double off = fabs(g[0][1]) + fabs(g[0][2]) + fabs(g[1][2]);
        if (off <= 1e-300 || off <= 1e-17 * (fabs(g[0][0]) + fabs(g[1][1]) + fabs(g[2][2]))) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (g[p][q] == 0.0) continue;
                const double th = (g[q][q] - g[p][p]) / (2.0 * g[p][q]);
                const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {
                    const double gkp = g[k][p], gkq = g[k][q];
                    g[k][p] = c * gkp - s * gkq; g[k][q] = s * gkp + c * gkq;
                }
                for (int k = 0; k < 3; ++k) {
                    const double gpk = g[p][k], gqk = g[q][k];
                    g[p][k] = c * gpk - s * gqk; g[q][k] = s * gpk + c * gqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq; v[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int best = 0;
    if (g[1][1] < g[best][best]) best = 1;
    if (g[2][2] < g[best][best]) best = 2;
    for (int k = 0; k < 3; ++k) y[k] = v[k][best];
}

// ---- one Rayleigh-Ritz step of a column.  w = L_e^+ r from T and the rank-(pending + 1) corrections, centred; {x, w, p}
// orthonormalised; Gram matrix of L_e; x <- the Ritz vector of the smallest Ritz value, p <- its part outside x.  One workgroup per
// column; all sums are workgroup reductions in a fixed order. ----
__global__ __launch_bounds__(kBlock) void k_eig_rr(EigView E, const double* __restrict__ Zb, const double* __restrict__ cb, int pending) {
    __shared__ double sm[4];
    __shared__ double beta[kEspMaxFold + 1];
    __shared__ double sy[3];
    const int b = blockIdx.x;
    if (E.conv[b]) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int e = E.bc[b];
    const int U = e >= 0 ? E.cu[e] + 1 : 0, V = e >= 0 ? E.cv2[e] + 1 : 0;
    const double wt = e >= 0 ? E.cw[e] : 0.0;
    const size_t ld = E.ld, ldq = E.ldq;
    const int n = E.n, np = E.np;
    double* x = E.X + (size_t)b * E.ldv;
    double* p = E.P + (size_t)b * E.ldv;
    double* w = E.W + (size_t)b * E.ldv;
    const double* lx = E.LX + (size_t)b * E.ldv;
    double* lw = E.LW + (size_t)b * E.ldv;
    double* lp = E.LP + (size_t)b * E.ldv;
    const double* z = E.Z + (size_t)b * ld;
    // beta_q = c_q (Zb[:, q] . r) for the pending columns, beta_pending = c_e (z_e . r): one wave per dot product
    for (int q = wv; q <= pending; q += kBlock / kWave) {
        const double* zc = q < pending ? Zb + (size_t)q * ld : z;
        double a = 0.0;
        for (int i = lane; i < np; i += kWave) a = __builtin_fma(zc[i], E.Q[(size_t)i * ldq + b], a);
        a = wave_sum(a);
        if (lane == 0) beta[q] = (q < pending ? cb[q] : E.cc[b]) * a;
    }
    __syncthreads();
    double s = 0.0;
    for (int i = tid; i < n; i += kBlock) {
        double t = 0.0;
        if (i > 0) {
            const int k = i - 1;
            t = E.T[(size_t)k * ldq + b];
            for (int q = 0; q < pending; ++q) t = __builtin_fma(-beta[q], Zb[(size_t)q * ld + k], t);
            t = __builtin_fma(-beta[pending], z[k], t);
        }
        w[i] = t;
        s += t;
    }
    const double mean = block_sum(s, sm) / n;
    double xw = 0.0, ww0 = 0.0;
    for (int i = tid; i < n; i += kBlock) { const double t = w[i] - mean; w[i] = t; xw = __builtin_fma(x[i], t, xw); ww0 = __builtin_fma(t, t, ww0); }
    xw = block_sum(xw, sm); ww0 = block_sum(ww0, sm);
    double ww = 0.0;
    for (int i = tid; i < n; i += kBlock) { const double t = w[i] - xw * x[i]; w[i] = t; ww = __builtin_fma(t, t, ww); }
    ww = block_sum(ww, sm);
    // w (nearly) a multiple of x -- always so for n = 2, where 1-perp is span{x}: what is left is rounding noise that would be
    // normalised into a copy of x (a singular Gram matrix, x <- x - x).  Dropped like p below.
    const double wi = ww > 1e-12 * ww0 ? 1.0 / sqrt(ww) : 0.0;
    const int hp = E.hasp[b];
    double xp = 0.0, wp = 0.0, pp0 = 0.0;
    for (int i = tid; i < n; i += kBlock) {
        const double t = w[i] * wi;
        w[i] = t;
        if (hp) { xp = __builtin_fma(x[i], p[i], xp); wp = __builtin_fma(t, p[i], wp); pp0 = __builtin_fma(p[i], p[i], pp0); }
    }
    double pi = 0.0;
    if (hp) {       // (workgroup-uniform)
        xp = block_sum(xp, sm); wp = block_sum(wp, sm); pp0 = block_sum(pp0, sm);
        double pp = 0.0;
        for (int i = tid; i < n; i += kBlock) { const double t = p[i] - xp * x[i] - wp * w[i]; p[i] = t; pp = __builtin_fma(t, t, pp); }
        pp = block_sum(pp, sm);
        pi = pp > 1e-12 * pp0 ? 1.0 / sqrt(pp) : 0.0;     // p (nearly) inside span{x, w}: what is left is rounding noise, drop it
        for (int i = tid; i < n; i += kBlock) p[i] *= pi;
    }
    __syncthreads();      // w, p complete before other threads' rows read them
    double xlw = 0.0, xlp = 0.0, wlw = 0.0, wlp = 0.0, plp = 0.0;
    for (int i = tid; i < n; i += kBlock) {
        const double yw = eig_lrow(E, w, i, U, V, wt);
        lw[i] = yw;
        xlw = __builtin_fma(lx[i], w[i], xlw);
        wlw = __builtin_fma(w[i], yw, wlw);
        if (pi != 0.0) {
            const double yp = eig_lrow(E, p, i, U, V, wt);
            lp[i] = yp;
            xlp = __builtin_fma(lx[i], p[i], xlp);
            wlp = __builtin_fma(yw, p[i], wlp);
            plp = __builtin_fma(p[i], yp, plp);
        }
    }
    xlw = block_sum(xlw, sm); wlw = block_sum(wlw, sm);
    if (pi != 0.0) { xlp = block_sum(xlp, sm); wlp = block_sum(wlp, sm); plp = block_sum(plp, sm); }
    if (tid == 0) {
        const double lam = E.lam[b];
        const double big = 4.0 * (fabs(lam) + fabs(wlw) + fabs(plp)) + 1.0;     // a dropped direction: decoupled, never the smallest
        double g[3][3] = {{lam, xlw, xlp}, {xlw, wlw, wlp}, {xlp, wlp, plp}};
        if (wi == 0.0) { g[0][1] = g[1][0] = g[1][2] = g[2][1] = 0.0; g[1][1] = big; }
        if (pi == 0.0) { g[0][2] = g[2][0] = g[1][2] = g[2][1] = 0.0; g[2][2] = big; }
        double y[3];
        eig_jacobi3(g, y);
        sy[0] = y[0]; sy[1] = y[1]; sy[2] = y[2];
    }
    __syncthreads();
    const double y0 = sy[0], y1 = sy[1], y2 = sy[2];
    double s1 = 0.0;
    for (int i = tid; i < n; i += kBlock) {
        const double d = y1 * w[i] + (pi != 0.0 ? y2 * p[i] : 0.0);
        p[i] = d;
        const double t = y0 * x[i] + d;
        x[i] = t;
        s1 += t;
    }
    const double m1 = block_sum(s1, sm) / n;
    double s2 = 0.0;
    for (int i = tid; i < n; i += kBlock) { const double t = x[i] - m1; x[i] = t; s2 = __builtin_fma(t, t, s2); }
    s2 = block_sum(s2, sm);
    const double xi = 1.0 / sqrt(s2);
    for (int i = tid; i < n; i += kBlock) x[i] *= xi;
    if (tid == 0) { E.hasp[b] = 1; E.iters[b] += 1; }
}

// the dense routes' application (machip_eig::apply): T = Sigma Q, then the step with the pending block's correction
inline void eig_dense_apply(const machip_esp* base, const EigView& E, int count) {
    k_eig_product<<<dim3((count + kGjT - 1) / kGjT, base->ld / kGjT), 256, 0, base->stream>>>(base->sig, E, count);
    k_eig_rr<<<count, kBlock, 0, base->stream>>>(E, base->Zb, base->cb, base->pending);
}

// What the bounded candidate scan (machip_eig::scan) of a pick, or of the rows of an exchange round, has established so far
struct EigScan {
    std::vector<int> ord, last;      // the candidates in decreasing order of their bound; those of the last batch solved (still in X)
    double top = -INFINITY;          // the largest value solved
    int solved = 0;                  // candidates solved
    int resident_column(int e) const {      // the column of X that holds e's vector, -1 when e was not in the last batch
        const auto it = std::find(last.begin(), last.end(), e);
        return it == last.end() ? -1 : (int)(it - last.begin());
    }
};

struct EigXch;      // eig_exchange.h: the exchange's candidate arrays, removal pairs and bound matrix, made by its first call
struct EigFree;     // eig_free.h: the scan chunks and projection buffers of the routes without Sigma (forms 2, 3 of the machip_esp underneath)

}  // namespace machip

// ---- the handle (include/machip.h: machip_eig) ----
struct machip_eig {
    machip_esp* base = nullptr;          // Sigma0 / Sigma, the pending block, the candidates, the stream
    int n = 0, m = 0, batch = 0, ldq = 0, ldv = 0;
    // L_cur on the host: adjacency of the fixed graph plus the picks, flattened to CSR after every pick
    std::vector<std::vector<std::pair<int, double>>> adj0, adj;
    std::vector<double> hdeg0, hdeg;
    std::vector<int> hci, hcj;
    std::vector<double> hcw;
    std::vector<char> sel;
    int *rp = nullptr, *cj = nullptr, *bc = nullptr, *conv = nullptr, *iters = nullptr, *hasp = nullptr, *nactive = nullptr;
    double *cv = nullptr, *deg = nullptr, *X = nullptr, *P = nullptr, *W = nullptr, *LX = nullptr, *LW = nullptr, *LP = nullptr;
    double *Q = nullptr, *T = nullptr, *Z = nullptr, *cc = nullptr, *lam = nullptr, *res = nullptr, *v0 = nullptr, *vcur = nullptr, *ub = nullptr;
    double *rbest = nullptr;
    int* stall = nullptr;
    double maxdeg = 0.0, lam0 = 0.0, lamcur = 0.0, tol = machip::kEigTol;
    size_t nnz_cap = 0;
    std::vector<int> solved, applies;    // per pick of the last run
    std::vector<int> removal;            // per round of the last exchange: removal pairs solved (eig_exchange.h)
    machip::EigXch* xc = nullptr;
    machip::EigFree* fr = nullptr;       // forms 2, 3 (MACHIP_EIG_MATRIX_FREE): no Sigma, the preconditioner of eig_free.h / eig_free_tree.h
    int seeds = 0;                       // form 3 (MACHIP_EIG_MATRIX_FREE_TREE): the history's leading columns, the fixed links outside the spanning tree
    const int *xcu = nullptr, *xcv = nullptr;      // while an exchange runs: its own candidate arrays (the m candidates, then
    const double* xcw = nullptr;                   // the negated copies of the selected ones); NULL: the greedy's
    std::vector<int> h_conv;
    std::vector<double> h_lam;

    machip::EigView view() const {
        machip::EigView E;
        E.n = n; E.np = base->np; E.ld = base->ld; E.ldv = ldv; E.ldq = ldq; E.rp = rp; E.cj = cj; E.cv = cv; E.deg = deg; E.maxdeg = maxdeg;
        E.cu = xcu ? xcu : base->cu; E.cv2 = xcv ? xcv : base->cv; E.cw = xcw ? xcw : base->cw; E.bc = bc; E.X = X; E.P = P; E.W = W; E.LX = LX; E.LW = LW; E.LP = LP;
        E.Q = Q; E.T = T; E.Z = Z; E.cc = cc; E.lam = lam; E.res = res; E.conv = conv; E.iters = iters; E.hasp = hasp; E.nactive = nactive;
        E.rbest = rbest; E.stall = stall; E.tol = tol;
        return E;
    }

    bool matrix_free() const { return base->form == machip::kEspFormFree || base->form == machip::kEspFormTree; }

    // What a route is (eig_routes.h, one switch on the form each): room for K picks; z_e, c_e of the columns bc[0..count) into Z / cc;
    // one application and step of the batch (T = Sigma_cur Q, k_eig_rr); `best`, just polished in column 0, joins the block or the history.
    int reserve(int64_t K); int columns(int count); int apply(int count); int push(int best);
    // The exchange's steps that differ by route (eig_exchange.h; C: the swaps a history is sized for, 0 on the dense routes): room for
    // the call; the selection `rows` (ascending; idx[r] on the device = rows[r]) loaded; room for a round's trial column and swap (a
    // fold, or a compaction: counted); the column of candidate *cand (on the device) joins the block or the history -- as a trial it
    // never folds and is dropped by the caller's pending = j.
    int xch_reserve(int K, int C); int xch_load(const std::vector<int>& rows, const int* idx);
    int xch_round_room(const std::vector<int>& rows, int C, int64_t* compactions); int xch_column(const int* cand, bool trial);

    machip::EspView zview() const {      // what k_eig_z reads the candidates from
        machip::EspView V = base->view();
        if (xcu) { V.cu = xcu; V.cv = xcv; V.cw = xcw; }
        return V;
    }

    int alloc() {
        using machip::dev_alloc;
        const size_t B = (size_t)ldq, ld = (size_t)base->ld, lv = (size_t)ldv;
        nnz_cap = 2 * (hci.size() + 1);
        for (auto& r : adj0) nnz_cap += r.size();
        ST_TRY(dev_alloc(&rp, (size_t)n + 1)); ST_TRY(dev_alloc(&cj, nnz_cap)); ST_TRY(dev_alloc(&cv, nnz_cap)); ST_TRY(dev_alloc(&deg, (size_t)n));
        ST_TRY(dev_alloc(&bc, B)); ST_TRY(dev_alloc(&conv, B)); ST_TRY(dev_alloc(&iters, B)); ST_TRY(dev_alloc(&hasp, B)); ST_TRY(dev_alloc(&nactive, 1));
        ST_TRY(dev_alloc(&X, lv * B)); ST_TRY(dev_alloc(&P, lv * B)); ST_TRY(dev_alloc(&W, lv * B));
        ST_TRY(dev_alloc(&LX, lv * B)); ST_TRY(dev_alloc(&LW, lv * B)); ST_TRY(dev_alloc(&LP, lv * B));
        ST_TRY(dev_alloc(&Q, ld * B)); ST_TRY(dev_alloc(&T, ld * B)); ST_TRY(dev_alloc(&Z, ld * B));
        ST_TRY(dev_alloc(&cc, B)); ST_TRY(dev_alloc(&lam, B)); ST_TRY(dev_alloc(&res, B)); ST_TRY(dev_alloc(&rbest, B)); ST_TRY(dev_alloc(&stall, B));
        ST_TRY(dev_alloc(&v0, lv)); ST_TRY(dev_alloc(&vcur, lv)); ST_TRY(dev_alloc(&ub, (size_t)std::max(m, 1)));
        HIP_TRY(hipMemsetAsync(Q, 0, sizeof(double) * ld * B, base->stream));      // rows n'..ld and the columns past a short batch stay 0
        HIP_TRY(hipMemsetAsync(bc, 0xff, sizeof(int) * B, base->stream));
        HIP_TRY(hipMemsetAsync(conv, 0, sizeof(int) * B, base->stream));
        return MACHIP_OK;
    }
    void release() {
        void* bufs[] = {rp, cj, bc, conv, iters, hasp, nactive, cv, deg, X, P, W, LX, LW, LP, Q, T, Z, cc, lam, res, v0, vcur, ub, rbest, stall};
        for (void* q : bufs) if (q) (void)hipFree(q);
    }

    // flatten adj to CSR and upload (rows in insertion order: fixed edges, then picks)
    int upload_graph() {
        std::vector<int> hrp((size_t)n + 1, 0), hcol;
        std::vector<double> hval;
        for (int i = 0; i < n; ++i) {
            for (auto& pr : adj[(size_t)i]) { hcol.push_back(pr.first); hval.push_back(pr.second); }
            hrp[(size_t)i + 1] = (int)hcol.size();
        }
        if (hcol.size() > nnz_cap) return machip::fail(MACHIP_BAD_ARG, "GreedyEig: edge storage exceeded");
        maxdeg = *std::max_element(hdeg.begin(), hdeg.end());
        hipStream_t st = base->stream;
        HIP_TRY(hipMemcpyAsync(rp, hrp.data(), sizeof(int) * hrp.size(), hipMemcpyHostToDevice, st));
        if (!hcol.empty()) {
            HIP_TRY(hipMemcpyAsync(cj, hcol.data(), sizeof(int) * hcol.size(), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(cv, hval.data(), sizeof(double) * hval.size(), hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipMemcpyAsync(deg, hdeg.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));        // (host staging goes out of scope)
        return MACHIP_OK;
    }
    void add_edge(int a, int b, double w) {
        if (a == b) return;
        adj[(size_t)a].emplace_back(b, w); adj[(size_t)b].emplace_back(a, w);
        hdeg[(size_t)a] += w; hdeg[(size_t)b] += w;
    }

    // `polish`: iterate past the stop rule until the residual stalls (the pair whose vector the next bounds are computed from).
    // Solve the columns bcand[0..count) (candidate indices; -1 = L_cur itself) from the start vector vstart.  h_lam / h_conv hold
    // the result; napp += column applications.
    int solve_batch(const int* bcand, int count, const double* vstart, int* napp, bool polish = false) {
        using namespace machip;
        tol = polish ? 0.0 : kEigTol;
        hipStream_t st = base->stream;
        HIP_TRY(hipMemcpyAsync(bc, bcand, sizeof(int) * (size_t)count, hipMemcpyHostToDevice, st));
        const EigView E = view();
        ST_TRY(columns(count));
        k_eig_init<<<dim3((n + kBlock - 1) / kBlock, count), kBlock, 0, st>>>(E, vstart);
        for (int it = 0; it <= kEigMaxIter + 1; ++it) {
            int act = 0;
            HIP_TRY(hipMemsetAsync(nactive, 0, sizeof(int), st));
            k_eig_resid<<<count, kBlock, 0, st>>>(E);
            HIP_TRY(hipMemcpyAsync(&act, nactive, sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (act == 0) break;
            if (napp) *napp += act;
            ST_TRY(apply(count));
        }
        HIP_TRY(hipGetLastError());
        h_lam.resize((size_t)count); h_conv.resize((size_t)count);
        HIP_TRY(hipMemcpyAsync(h_lam.data(), lam, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_conv.data(), conv, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int b = 0; b < count; ++b)
            if (h_conv[(size_t)b] != 1)
                return fail(MACHIP_NOT_CONVERGED, "GreedyEig: the Fiedler solve of candidate " + std::to_string(bcand[b]) + " did not reach the stop rule in " +
                                                      std::to_string(kEigMaxIter) + " iterations");
        return MACHIP_OK;
    }

    // state <- the fixed graph (Sigma0, no pending columns -- form 3: the seeds' --, its Fiedler pair)
    int reset() {
        hipStream_t st = base->stream;
        if (!matrix_free()) HIP_TRY(hipMemcpyAsync(base->sig, base->sig0, sizeof(double) * (size_t)base->ld * (size_t)base->ld, hipMemcpyDeviceToDevice, st));
        base->pending = seeds;
        adj = adj0; hdeg = hdeg0;
        std::fill(sel.begin(), sel.end(), 0);
        ST_TRY(upload_graph());
        HIP_TRY(hipMemcpyAsync(vcur, v0, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
        lamcur = lam0;
        solved.clear(); applies.clear(); removal.clear();
        return MACHIP_OK;
    }

    // the Fiedler pair of the fixed graph, from a deterministic start (a ramp plus a fixed oscillation: not orthogonal to anything special)
    int first_pair() {
        std::vector<double> x((size_t)n);
        for (int i = 0; i < n; ++i) x[(size_t)i] = (i - 0.5 * (n - 1)) / n + 0.37 * std::sin(1.0 + 2.3 * i);
        const double mean = std::accumulate(x.begin(), x.end(), 0.0) / n;
        double ss = 0.0;
        for (double& t : x) { t -= mean; ss += t * t; }
        for (double& t : x) t /= std::sqrt(ss);
        hipStream_t st = base->stream;
        HIP_TRY(hipMemcpyAsync(v0, x.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        const int none = -1;
        ST_TRY(solve_batch(&none, 1, v0, nullptr, true));
        HIP_TRY(hipMemcpyAsync(v0, X, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        lam0 = h_lam[0];
        return MACHIP_OK;
    }

    int bounds(std::vector<double>& u) {
        u.assign((size_t)m, 0.0);
        if (!m) return MACHIP_OK;
        hipStream_t st = base->stream;
        machip::k_eig_bounds<<<base->grid_m(), machip::kBlock, 0, st>>>(view(), vcur, lamcur, m, ub);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(u.data(), ub, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return MACHIP_OK;
    }

    // dense handles: the column of candidate *cand (on the device; an index into zview()'s) joins the pending block, folded when full
    void push_column(const int* cand) {
        const int j = base->pending;
        machip::eig_dense_columns(base, zview(), cand, 1, base->Zb + (size_t)j * (size_t)base->ld, base->cb + j);
        base->pending = j + 1;
        if (base->pending == base->fold) { base->fold_into(base->sig, base->pending); base->pending = 0; }
    }

    // the pair of L_cur + candidate `cand` (-1: none), polished from vstart (the next bounds are only as tight as it), becomes current
    int adopt_pair(int cand, const double* vstart, int* napp) {
        ST_TRY(solve_batch(&cand, 1, vstart, napp, true));
        HIP_TRY(hipMemcpyAsync(vcur, X, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, base->stream));
        lamcur = h_lam[0];
        return MACHIP_OK;
    }

    // The bounded scan: the unselected candidates in decreasing order of their bound u (a stable sort), solved from vstart batch after
    // batch until a batch's first bound is below max(floor, s.top): a value already established.  report(candidate, value) per solve.
    template <class Report>
    int scan(machip::EigScan& s, const std::vector<double>& u, double floor, const double* vstart, int* napp, Report report) {
        s.ord.clear();
        for (int e = 0; e < m; ++e) if (!sel[(size_t)e]) s.ord.push_back(e);
        std::stable_sort(s.ord.begin(), s.ord.end(), [&](int a, int b) { return u[(size_t)a] > u[(size_t)b]; });
        for (size_t q = 0; q < s.ord.size(); q += (size_t)batch) {
            if (u[(size_t)s.ord[q]] < std::max(floor, s.top)) break;
            const int cnt = (int)std::min(s.ord.size() - q, (size_t)batch);
            ST_TRY(solve_batch(s.ord.data() + q, cnt, vstart, napp));
            for (int b = 0; b < cnt; ++b) {
                report(s.ord[q + (size_t)b], h_lam[(size_t)b]);
                s.top = std::max(s.top, h_lam[(size_t)b]);
            }
            s.solved += cnt;
            s.last.assign(s.ord.begin() + (long)q, s.ord.begin() + (long)q + cnt);
        }
        return MACHIP_OK;
    }

    // lambda_2(L_cur + e) of every unselected candidate (NaN for the selected), no pruning: the scan in index order, no bound below anything
    int all_lambda2(double* out) {
        std::fill(out, out + m, NAN);
        machip::EigScan s;
        return scan(s, std::vector<double>((size_t)m, INFINITY), -INFINITY, vcur, nullptr, [&](int e, double val) { out[e] = val; });
    }

    int select(int K, int32_t* order_out, double* lambda2_out, double* t_ms_out) {
        using namespace machip;
        ST_TRY(reserve(K));      // (refused before the state is touched)
        ST_TRY(reset());
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<double> u, l2((size_t)m);
        std::vector<char> done((size_t)m);
        for (int k = 0; k < K; ++k) {
            ST_TRY(bounds(u));
            std::fill(done.begin(), done.end(), 0);
            EigScan s;
            int napp = 0;
            ST_TRY(scan(s, u, -INFINITY, vcur, &napp, [&](int e, double val) { l2[(size_t)e] = val; done[(size_t)e] = 1; }));
            // the reference's scan: candidate-index order, a candidate replaces the running best only if it exceeds it by more than 1e-8
            int best = -1;
            double best_l2 = 0.0;
            for (int e = 0; e < m; ++e)
                if (done[(size_t)e] && l2[(size_t)e] > best_l2 + kEigTol) { best = e; best_l2 = l2[(size_t)e]; }
            if (best < 0) return fail(MACHIP_NOT_CONVERGED, "GreedyEig: no candidate raises lambda_2 above 1e-8 at pick " + std::to_string(k));
            // the winner's pair: from its converged vector when that is still resident, else from the current one
            const int col = s.resident_column(best);
            ST_TRY(adopt_pair(best, col >= 0 ? X + (size_t)col * (size_t)ldv : vcur, &napp));
            ST_TRY(push(best));
            HIP_TRY(hipGetLastError());
            sel[(size_t)best] = 1;
            add_edge(hci[(size_t)best], hcj[(size_t)best], hcw[(size_t)best]);
            ST_TRY(upload_graph());
            solved.push_back(s.solved); applies.push_back(napp);
            if (order_out) order_out[k] = best;
            if (lambda2_out) lambda2_out[k] = lamcur;
            if (t_ms_out) t_ms_out[k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        return MACHIP_OK;
    }
};
