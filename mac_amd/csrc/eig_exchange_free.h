// mac_amd/csrc/eig_exchange_free.h -- what the exchange on lambda_2 (eig_exchange.h) needs on the routes without Sigma (eig_free.h,
// eig_free_tree.h): the blocked load of a selection into the history, and with it the compaction.  DESIGN section 23.
//
// The history holds Sigma_cur = Sigma0 - Zb diag(cb) Zb^T as the sequence of Sherman-Morrison columns z_q = Sigma_{q-1} a_q,
// c_q = w_q / (1 + w_q a_q^T z_q).  Loading K edges one column at a time reads the growing history K times; a block of B = kGjT = 64
// edges against the history as it stands (Sigma = its inverse, A the block's incidence columns, candidate indices ascending in bc):
//   1. Z0 = Sigma A            machip_eig::columns(B) as it is: the scans / sweeps and the history's part, column-major in Z
//   2. G = A^T Z0              k_eigf_gram: G[b', b] = Z0[u_b', b] - Z0[v_b', b], gathers only (node-0 terms 0)
//   3. for b = 0 .. B-1:       k_eigf_chain, one workgroup, G in LDS
//        c_b = w_b / (1 + w_b G[b, b]);  N[b, b'] = c_b G[b, b'] (b' > b);  G -= c_b g g^T, g = column b of G before the update
//      (G after b steps is A^T Sigma_b A, so row b is a_b'^T z_b: what the later columns lose to column b)
//   4. Z = Z0 (I + N)^-1       k_eigf_mix: N strictly upper triangular, so z_b = Z0[:, b] - sum_{b' < b} z_b' N[b', b]: a forward
//      substitution per row.  A lane owns a row and takes its B entries through the registers 16 at a time, N is read from LDS (every
//      lane the same address: a broadcast).  Written straight into the history's columns j .. j + B (Z and Zb share the column-major
//      layout), c into cb.
// The history is read once per block instead of once per edge.  A downdate column (a negative w) goes through unchanged.  No atomics,
// no reductions across lanes: every sum runs in index order, so two runs repeat bit for bit.  Rows n'..ld are written as 0.  A short
// block (count < B) has zeros in the rows and columns of G and N from count on and writes only its count columns.
#pragma once
#include <string>
#include <vector>

#include "eig_free_tree.h"

namespace machip {

// ---- step 2.  grid = B B / 256: thread = the entry (b', b) ----
__global__ __launch_bounds__(kBlock) void k_eigf_gram(EigView E, int count, double* __restrict__ G) {
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    const int bp = idx / kGjT, b = idx % kGjT;
    double g = 0.0;
    if (bp < count && b < count) {
        const int e = E.bc[bp];
        const int u = E.cu[e], v = E.cv2[e];
        const double* z = E.Z + (size_t)b * E.ld;
        g = (u >= 0 ? z[u] : 0.0) - (v >= 0 ? z[v] : 0.0);
    }
    G[idx] = g;
}

// ---- step 3.  One workgroup; G (32 KB) in LDS; thread t owns column k = t % 64 of the rows t / 64, t / 64 + 4, ... (16 entries).  After
// step b the rows and columns up to b are dead: only the trailing block is updated, and what a step reads (row b, column b) it does
// not write -- so a thread takes its 17 entries of column b into registers first and the 16 updates do not wait for one another. ----
__global__ __launch_bounds__(kBlock) void k_eigf_chain(EigView E, int count, const double* __restrict__ G, double* __restrict__ N,
                                                       double* __restrict__ cdst) {
    __shared__ double sG[kGjT * kGjT];
    constexpr int kRows = kBlock / kGjT, kPer = kGjT / kRows;
    const int tid = threadIdx.x, k = tid % kGjT, i0 = tid / kGjT;
    for (int idx = tid; idx < kGjT * kGjT; idx += kBlock) sG[idx] = G[idx];
    __syncthreads();
    for (int b = 0; b < kGjT; ++b) {
        double c = 0.0;
        if (b < count) {
            const double w = E.cw[E.bc[b]];
            c = w / (1.0 + w * sG[b * kGjT + b]);
        }
        const double gk = sG[k * kGjT + b];
        double gi[kPer];
#pragma unroll
        for (int q = 0; q < kPer; ++q) gi[q] = sG[(i0 + kRows * q) * kGjT + b];
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int i = i0 + kRows * q, idx = i * kGjT + k;
            if (i == b) N[idx] = k > b ? c * sG[idx] : 0.0;
            else if (i > b && k > b) sG[idx] -= c * gi[q] * gk;
        }
        if (tid == 0 && b < count) cdst[b] = c;
        __syncthreads();
    }
}

// ---- step 4.  grid = ceil(ld / 256): lane = a row of Z0, N (32 KB) in LDS.  The 64 columns go through the registers in panels of
// kEigfMixPanel = 16 (a lane that held all 64 at once, with both loops unrolled, spilled: the compiler hoists the 2 016 reads of N):
// a panel starts from its columns of Z0, loses the earlier panels' columns -- read back from dst, where this lane wrote them, one
// at a time in a rolled loop -- and is then solved in its 16 registers.  Column b still sums over q = 0 .. b - 1 in index order.
// dst = the history's column j. ----
constexpr int kEigfMixPanel = 16;

__global__ __launch_bounds__(kBlock) void k_eigf_mix(EigView E, int count, const double* __restrict__ N, double* dst) {
    __shared__ double sN[kGjT * kGjT];
    for (int idx = threadIdx.x; idx < kGjT * kGjT; idx += kBlock) sN[idx] = N[idx];
    __syncthreads();
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row >= E.ld) return;
    const size_t ld = E.ld;
    const bool in = row < E.np;      // (a row from n' on: zeros in, zeros out)
#pragma unroll 1
    for (int p0 = 0; p0 < count; p0 += kEigfMixPanel) {
        double z[kEigfMixPanel];
#pragma unroll
        for (int i = 0; i < kEigfMixPanel; ++i) z[i] = (in && p0 + i < count) ? E.Z[(size_t)(p0 + i) * ld + row] : 0.0;
        if (in) {
#pragma unroll 1
            for (int q = 0; q < p0; ++q) {
                const double zq = dst[(size_t)q * ld + row];
                const double* nq = sN + q * kGjT + p0;
#pragma unroll
                for (int i = 0; i < kEigfMixPanel; ++i) z[i] = __builtin_fma(-zq, nq[i], z[i]);
            }
        }
#pragma unroll
        for (int b = 1; b < kEigfMixPanel; ++b) {
            double a = z[b];
#pragma unroll
            for (int q = 0; q < b; ++q) a = __builtin_fma(-z[q], sN[(p0 + q) * kGjT + p0 + b], a);
            z[b] = a;
        }
#pragma unroll
        for (int i = 0; i < kEigfMixPanel; ++i)
            if (p0 + i < count) dst[(size_t)(p0 + i) * ld + row] = z[i];
    }
}

// The blocked load: the candidates `sorted` (ascending) join the history, block after block.  The caller has reserved the room.
inline int eig_xfree_load(machip_eig* h, const std::vector<int>& sorted) {
    EigFree* F = h->fr;
    machip_esp* base = h->base;
    hipStream_t st = base->stream;
    if (!F->xg) {
        ST_TRY(dev_alloc(&F->xg, (size_t)kGjT * kGjT));
        ST_TRY(dev_alloc(&F->xn, (size_t)kGjT * kGjT));
    }
    const EigView E = h->view();
    const int K = (int)sorted.size(), ld = base->ld;
    auto blocks = [&]() -> int {
        for (int q = 0; q < K; q += kGjT) {
            const int cnt = std::min(K - q, kGjT), j = base->pending;
            if ((size_t)j + (size_t)cnt > base->zcap) return fail(MACHIP_BAD_ARG, "GreedyEig: the matrix-free history is full");
            HIP_TRY(hipMemcpyAsync(h->bc, sorted.data() + q, sizeof(int) * (size_t)cnt, hipMemcpyHostToDevice, st));
            ST_TRY(h->columns(cnt));
            k_eigf_gram<<<kGjT * kGjT / kBlock, kBlock, 0, st>>>(E, cnt, F->xg);
            k_eigf_chain<<<1, kBlock, 0, st>>>(E, cnt, F->xg, F->xn, base->cb + j);
            k_eigf_mix<<<(ld + kBlock - 1) / kBlock, kBlock, 0, st>>>(E, cnt, F->xn, base->Zb + (size_t)j * (size_t)ld);
            base->pending = j + cnt;
        }
        HIP_TRY(hipGetLastError());
        return MACHIP_OK;
    };
    const int rc = blocks();
    // on every path, a failure's included: the copies read the caller's list, which may go out of scope when this returns
    const hipError_t e = hipStreamSynchronize(st);
    if (rc != MACHIP_OK) return rc;
    HIP_TRY(e);
    return MACHIP_OK;
}

// The compaction: the history back to the seeds, then the current selection (ascending) loaded again.  The pair of L_S is untouched.
inline int eig_xfree_compact(machip_eig* h, std::vector<int> rows) {
    std::sort(rows.begin(), rows.end());
    h->base->pending = h->seeds;
    return eig_xfree_load(h, rows);
}

// the history as it stands, to the host: `pending` columns of ld doubles, column-major as stored, and their coefficients
inline int eig_free_history_read(machip_eig* h, int64_t cap_cols, double* Z, double* c, int64_t* cols) {
    const machip_esp* base = h->base;
    const int j = base->pending;
    if (cols) *cols = j;
    if (!Z && !c) return MACHIP_OK;
    if (cap_cols < j)
        return fail(MACHIP_BAD_ARG, "machip_eig_history: the history holds " + std::to_string(j) + " columns, cap_cols = " + std::to_string((long long)cap_cols));
    hipStream_t st = base->stream;
    if (j > 0) {
        if (Z) HIP_TRY(hipMemcpyAsync(Z, base->Zb, sizeof(double) * (size_t)j * (size_t)base->ld, hipMemcpyDeviceToHost, st));
        if (c) HIP_TRY(hipMemcpyAsync(c, base->cb, sizeof(double) * (size_t)j, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return MACHIP_OK;
}

}  // namespace machip
