// mac_amd/csrc/eig_free.h -- GreedyEig without a dense Sigma: the matrix-free route for chain-fixed graphs.
//
// The preconditioner of eig.h is  L_e^+ q = P (Sigma0 - Zb diag(cb) Zb^T - c_e z_e z_e^T)_ext q.  When the fixed edges are the chain
// (i, i+1), Sigma0_ab = R[min(a, b)] (R = prefix sums of 1 / w_link, esp.h) and the picks' rank-1 updates stay in the history
// Zb (ld x j), cb of the machip_esp underneath (esp_free.h: never folded).  One application for the batch, T = Sigma_cur Q, is then
//   1. T = Sigma0 Q by two scans (k_eigf_scan):  with d_t = R[t] - R[t-1],  (Sigma0 q)_a = sum_{t <= a} d_t s_t,  s_t = sum_{b >= t} q_b.
//      Lanes run along the batch index; the rows are cut into chunks.  Three launches: the chunks' sums of q; the chunks' sums of
//      u_t = d_t s_t (the suffix carry of a chunk = the later chunks' sums, added in ascending chunk order by the consumer); T (the
//      prefix carry likewise).  Every launch walks its chunk downwards, so s_t and u_t are the same doubles wherever they are formed.
//   2. Y = diag(cb) Zb^T Q  (j x B) on the f64 matrix cores (k_eigf_proj): the rows are cut into slices, a workgroup owns a 64 x 64
//      tile of Y over one slice, the A operand (Zb read across its columns: stride ld) is staged through LDS 32 rows at a time;
//      k_eigf_ysum adds the slices' tiles in ascending slice order and scales by cb.
//   3. T -= Zb Y  on the matrix cores (k_eigf_back: k_eig_product's structure, Zb in the place of Sigma, the k-loop over the history
//      in steps of 4 with a zero-filled tail).
// k_eig_rr then runs with pending = 0: only the column's own c_e z_e z_e^T is left for it.  The batch's z_e = Sigma_cur a_e are the
// same back-substitution in its second output form: base R[min(u, i)] - R[min(v, i)], Y = alpha[q, b] = cb[q] (Zb[u_b, q] - Zb[v_b, q])
// (k_eigf_alpha), written column-major into Z; k_eigf_cc makes c_e.  No atomics; the order of every sum is a function of
// (ld, j, the batch, options eig_free_rows / eig_free_split) alone.
// On a spanning-tree handle (form 3, eig_free_tree.h) pass 1 is that file's four sweeps over the tree, the history starts with the r
// seeds of esp_tree.h (j = r + picks) and the batch's z_e take their base from the same sweeps; passes 2 and 3 (eig_free_history),
// eig_free_init and the z_e's history part (eig_free_columns) are shared; machip_eig::apply (eig_routes.h) runs the form's pass 1.
#pragma once
#include <string>

#include "eig.h"
#include "esp_tree.h"

namespace machip {

constexpr int kEigFreeMaxSplit = 32;     // row slices of pass 2 at most
constexpr int kEigFreePanel = 32;        // rows of Zb staged in LDS per step of pass 2
constexpr int kEigFreeLds = 80;          // row stride of the staged panel in doubles (80 = 16 mod 32): the two k-rows a half-wave reads
                                         // (ds_read_b64 is served per half-wave) fall in disjoint banks; k-rows 0 / 2 and 1 / 3 alias
constexpr int kEigFreeWgs = 256;         // workgroups aimed at in pass 2 (one per CU)
constexpr int kEigFreeMinRows = 32;      // automatic scan chunks: at least this many rows, at most kEigFreeChunks chunks
constexpr int kEigFreeChunks = 128;
constexpr int kEigFreeMaxChunks = 1024;  // option eig_free_rows is raised until the chunks are at most this many: they are gridDim.y, every wave
                                         // of launches 1 and 2 adds the other chunks' sums serially, and the sums take 2 chunks ldq doubles

// ---- pass 1.  grid = (ldq / 64, chunks), one wave per workgroup: lane = a column of the batch, the chunk's rows walked downwards.
// MODE 0: cs[c] = the chunk's sum of q.  MODE 1: cu[c] = the chunk's sum of u_t = d_t s_t.  MODE 2: T.  A 64-column group whose
// columns have all retired is skipped in every mode. ----
template <int MODE>
__global__ __launch_bounds__(kWave) void k_eigf_scan(EigView E, const double* __restrict__ R, double* __restrict__ cs, double* __restrict__ cu,
                                                     int rows, int count) {
    const int col = blockIdx.x * kWave + threadIdx.x;
    const int live = (col < count && E.conv[col] == 0) ? 1 : 0;
    if (!__any(live)) return;
    const int c = blockIdx.y, nch = gridDim.y;
    const int t0 = c * rows, t1 = min(E.ld, t0 + rows);
    const size_t ldq = E.ldq;
    if (MODE == 0) {
        double s = 0.0;
        for (int t = min(t1, E.np) - 1; t >= t0; --t) s += E.Q[(size_t)t * ldq + col];
        cs[(size_t)c * ldq + col] = s;
        return;
    }
    double s = 0.0, top = 0.0, acc = 0.0;
    for (int c2 = c + 1; c2 < nch; ++c2) s += cs[(size_t)c2 * ldq + col];
    if (MODE == 2)
        for (int c2 = 0; c2 <= c; ++c2) top += cu[(size_t)c2 * ldq + col];
    for (int t = t1 - 1; t >= t0; --t) {
        if (t >= E.np) {
            if (MODE == 2) E.T[(size_t)t * ldq + col] = 0.0;
            continue;
        }
        s += E.Q[(size_t)t * ldq + col];
        const double u = (R[t] - (t > 0 ? R[t - 1] : 0.0)) * s;
        if (MODE == 2) E.T[(size_t)t * ldq + col] = top - acc;      // sum_{t' <= t} u_t' = (the chunks up to this one) - (the rows above t)
        acc += u;
    }
    if (MODE == 1) cu[(size_t)c * ldq + col] = acc;
}

// ---- pass 2.  grid = (column groups, ceil(j / 64), slices); workgroup = a 64 x 64 tile of Zb^T Q over the rows [s per, (s + 1) per),
// wave = a 32 x 32 quadrant of 2 x 2 v_mfma_f64_16x16x4_f64 blocks: A[i = l & 15][k = l >> 4] = Zb[row k, column i] from the staged
// panel, B[k][j = l & 15] = Q[row k, col j], D[row = (l >> 4) + 4 reg][col = l & 15].  Columns of Zb from j on are staged as zeros, not
// read.  part: slice s, row q, column b at (s j64 + q) ldp + b. ----
__global__ __launch_bounds__(256) void k_eigf_proj(EigView E, const double* __restrict__ Zb, double* __restrict__ part, int j, int count,
                                                   int per, int ldp, int j64) {
    __shared__ double sA[kEigFreePanel * kEigFreeLds];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int col = blockIdx.x * kGjT + (tid & 63);
    const int live = (tid < 64 && col < count && E.conv[col] == 0) ? 1 : 0;
    if (!__syncthreads_or(live)) return;
    const int li = lane & 15, lk = lane >> 4, wr = wv >> 1, wc = wv & 1;
    const int q0 = blockIdx.y * kGjT, s = blockIdx.z;
    const int c0 = blockIdx.x * kGjT + 32 * wc;
    const size_t ld = E.ld, ldq = E.ldq;
    const int rbeg = min(E.ld, s * per), rend = min(E.ld, rbeg + per);
    gj_d4 acc[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[bi][bj][q] = 0.0;
    // staging: column q0 + sc of Zb, rows sr .. sr + 8 of the panel (64 bytes in a row, as eight 8-byte loads).  The four sr of a column
    // are 640 doubles apart in sA (0 mod 32): the staging writes are 4-way conflicted -- 8 writes per 32 operand reads, left as it is.
    const int sc = tid >> 2, sr = (tid & 3) * 8;
    const bool have = q0 + sc < j;
    const double* zsrc = Zb + (size_t)(q0 + sc) * ld + sr;
    const double* qb = E.Q + (size_t)lk * ldq + c0 + li;
    for (int r = rbeg; r < rend; r += kEigFreePanel) {
        double v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = have ? zsrc[r + i] : 0.0;
        __syncthreads();                                  // (the previous panel is no longer read)
#pragma unroll
        for (int i = 0; i < 8; ++i) sA[(sr + i) * kEigFreeLds + sc] = v[i];
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kEigFreePanel / 4; ++kk) {
            double a[2], b[2];
            a[0] = sA[(4 * kk + lk) * kEigFreeLds + 32 * wr + li];
            a[1] = sA[(4 * kk + lk) * kEigFreeLds + 32 * wr + 16 + li];
            const double* qr = qb + (size_t)(r + 4 * kk) * ldq;
            b[0] = qr[0]; b[1] = qr[16];
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[bi], b[bj], acc[bi][bj], 0, 0, 0);
        }
    }
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                part[((size_t)s * j64 + q0 + 32 * wr + 16 * bi + lk + 4 * q) * ldp + c0 + 16 * bj + li] = acc[bi][bj][q];
}

// ---- Y[q, b] = cb[q] (part[0] + part[1] + ... + part[S - 1])[q, b] (ascending: a fixed order), rows j .. j64 of Y zero ----
__global__ __launch_bounds__(kBlock) void k_eigf_ysum(const double* __restrict__ part, const double* __restrict__ cb, double* __restrict__ Y, int S,
                                                      int j, int j64, int ldp, int ldq) {
    const size_t tot = (size_t)j64 * ldp;
    for (size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * kBlock) {
        const int q = (int)(idx / ldp), b = (int)(idx % ldp);
        double a = 0.0;
        if (q < j) {
            a = part[idx];
            for (int s = 1; s < S; ++s) a += part[(size_t)s * tot + idx];
            a *= cb[q];
        }
        Y[(size_t)q * ldq + b] = a;
    }
}

// ---- alpha[q, b] = cb[q] (Zb[u_b, q] - Zb[v_b, q]) into Y (rows j .. j64, the columns without an edge and those past the batch: 0) ----
__global__ __launch_bounds__(kBlock) void k_eigf_alpha(EigView E, const double* __restrict__ Zb, const double* __restrict__ cb, double* __restrict__ Y,
                                                       int j, int j64, int count) {
    const size_t ld = E.ld, ldq = E.ldq, tot = (size_t)j64 * ldq;
    for (size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * kBlock) {
        const int q = (int)(idx / ldq), b = (int)(idx % ldq);
        double a = 0.0;
        const int e = (q < j && b < count) ? E.bc[b] : -1;
        if (e >= 0) {
            const int u = E.cu[e], v = E.cv2[e];
            const double* zc = Zb + (size_t)q * ld;
            a = cb[q] * ((u >= 0 ? zc[u] : 0.0) - (v >= 0 ? zc[v] : 0.0));
        }
        Y[idx] = a;
    }
}

// ---- pass 3: C = base - Zb Y.  grid = (column groups, ld / 64); tile, quadrants and operands as k_eig_product with Zb in the place of
// Sigma: A[i][k] = Zb[row i, column k] (16 consecutive doubles per k), B[k][j] = Y[k, col j].  Columns of Zb from j on are zeros, not
// read.  ZFORM = false: T -= Zb Y (row-major; base = pass 1's T), groups whose columns have all retired skipped.  ZFORM = true: the
// batch's z_e, column-major into Z, base R[min(u, i)] - R[min(v, i)] (node-0 terms 0), or with FROM_T (eig_free_tree.h) read from T,
// where the sweeps over the spanning tree have left Sigma0 a_e.  Rows n'..ld are written as 0. ----
template <bool ZFORM, bool FROM_T = false>
__global__ __launch_bounds__(256) void k_eigf_back(EigView E, const double* __restrict__ R, const double* __restrict__ Zb, const double* __restrict__ Y,
                                                   int j, int count) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int col = blockIdx.x * kGjT + (tid & 63);
    const int live = (tid < 64 && col < count && (ZFORM || E.conv[col] == 0)) ? 1 : 0;
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
    const double* sa = Zb + (size_t)lk * ld + r0 + li;
    const double* yb = Y + (size_t)lk * ldq + c0 + li;
    for (int q = 0; q < j; q += 4) {
        const bool in = q + lk < j;
        double a[2], b[2];
        a[0] = in ? sa[0] : 0.0; a[1] = in ? sa[16] : 0.0;
        b[0] = yb[0]; b[1] = yb[16];
        sa += 4 * ld; yb += 4 * ldq;
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
            for (int q = 0; q < 4; ++q) {
                const int row = r0 + 16 * bi + lk + 4 * q, cl = c0 + 16 * bj + li;
                if (ZFORM) {
                    if (cl >= count) continue;
                    const int e = E.bc[cl];
                    double z = 0.0;
                    if (e >= 0 && row < E.np)
                        z = (FROM_T ? E.T[(size_t)row * ldq + cl] : esp_free_sig0(R, E.cu[e], row) - esp_free_sig0(R, E.cv2[e], row)) - acc[bi][bj][q];
                    E.Z[(size_t)cl * ld + row] = z;
                } else {
                    const size_t at = (size_t)row * ldq + cl;
                    E.T[at] = row < E.np ? E.T[at] - acc[bi][bj][q] : 0.0;
                }
            }
}

// ---- c_e = w_e / (1 + w_e a_e^T z_e) of the batch's columns (0 without an edge) ----
__global__ __launch_bounds__(kBlock) void k_eigf_cc(EigView E, int count) {
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= count) return;
    const int e = E.bc[b];
    double c = 0.0;
    if (e >= 0) {
        const int u = E.cu[e], v = E.cv2[e];
        const double* z = E.Z + (size_t)b * E.ld;
        const double s = (u >= 0 ? z[u] : 0.0) - (v >= 0 ? z[v] : 0.0);
        c = E.cw[e] / (1.0 + E.cw[e] * s);
    }
    E.cc[b] = c;
}

// rows per scan chunk: a function of (ld, option eig_free_rows) alone
inline int eig_free_rows(int ld, int opt) {
    if (opt > 0) return std::min(std::max(opt, (ld + kEigFreeMaxChunks - 1) / kEigFreeMaxChunks), ld);
    return std::max(kEigFreeMinRows, (ld + kEigFreeChunks - 1) / kEigFreeChunks);
}

// row slices of pass 2: a function of (ld, j, count, option eig_free_split) alone
inline int eig_free_slices(int ld, int j, int count, int opt) {
    const int tiles = ((j + kGjT - 1) / kGjT) * ((count + kGjT - 1) / kGjT);
    int S = opt > 0 ? opt : kEigFreeWgs / std::max(tiles, 1);
    S = std::min(std::min(S, kEigFreeMaxSplit), ld / kEigFreePanel);
    return std::max(S, 1);
}

// doubles of `part` that cover every (j <= K, count <= ldq): S tiles <= max(tiles, kEigFreeWgs) without the option
inline size_t eig_free_part_elems(int K64, int ldq, int opt) {
    const size_t y = (size_t)K64 * (size_t)ldq;
    if (opt > 0) return y * (size_t)std::min(opt, kEigFreeMaxSplit);
    return std::max(y, (size_t)kEigFreeWgs * kGjT * kGjT);
}

// eig_free_tree.h -- form 3 only: the tables and S of the sweeps over the spanning tree
struct EigFreeTree;
void eig_tree_release(EigFreeTree* G);

// what the route keeps beside the batch arrays of machip_eig
struct EigFree {
    int rows = 0, nchunks = 0, split = 0;      // scan chunks; option eig_free_split when the handle was made (0 = automatic)
    double *cs = nullptr, *cu = nullptr;       // the chunks' sums (nchunks x ldq each)
    double *Y = nullptr, *part = nullptr;      // the projection (K64 x ldq) and the slices' partial tiles
    int k64 = 0;                               // history columns Y / part are sized for
    EigFreeTree* tree = nullptr;               // form 3: the spanning tree in the place of the chain (cs / cu: its row and tour chunks' sums)
    double *xg = nullptr, *xn = nullptr;       // eig_exchange_free.h: G and N of a block of the blocked load (64 x 64 each), made by its first call
};

// What both routes start from: the scan chunks and option eig_free_split, then the batch arrays' bytes (machip_eig::alloc plus the
// chunks' sums; form 3: S as well), refused when they do not fit, then the chunks' sums.  eig_tree_init adds the tree's tables.
inline int eig_free_init(machip_eig* h, bool tree = false) {
    EigFree* F = new EigFree();
    h->fr = F;
    const Options& D = default_options();
    const int ld = h->base->ld, mats = tree ? 4 : 3;
    F->rows = eig_free_rows(ld, (int)std::max(0l, std::min<long>(D.get(kOpt_eig_free_rows, 0), INT_MAX)));
    F->nchunks = (ld + F->rows - 1) / F->rows;
    F->split = (int)std::max(0l, std::min<long>(D.get(kOpt_eig_free_split, 0), kEigFreeMaxSplit));
    const double need = 8.0 * (6.0 * h->ldv + (double)mats * ld + 2.0 * F->nchunks) * (double)h->ldq;
    size_t fr = 0, tot = 0;
    HIP_TRY(hipMemGetInfo(&fr, &tot));
    if (need > (double)fr - 268435456.0)
        return fail(MACHIP_BAD_ARG, std::string("the batch arrays of MACHIP_EIG_MATRIX_FREE") + (tree ? "_TREE" : "") + " do not fit in device memory: n = " +
                                        std::to_string(h->n) + (tree ? " (r = " + std::to_string(h->seeds) + " seeds)" : "") + ", batch columns " +
                                        std::to_string(h->ldq) + " ask for 8 (6 ldv + " + std::to_string(mats) + " ld + 2 chunks) ldq = " +
                                        std::to_string((unsigned long long)need) + " bytes (ld = " + std::to_string(ld) + "), " +
                                        std::to_string((unsigned long long)fr) + " bytes are free: lower `batch`");
    ST_TRY(dev_alloc(&F->cs, (size_t)F->nchunks * (size_t)h->ldq));
    ST_TRY(dev_alloc(&F->cu, (size_t)F->nchunks * (size_t)h->ldq));
    return MACHIP_OK;
}

inline void eig_free_release(EigFree* F) {
    if (!F) return;
    eig_tree_release(F->tree);
    void* bufs[] = {F->cs, F->cu, F->Y, F->part, F->xg, F->xn};
    for (void* q : bufs) if (q) (void)hipFree(q);
    delete F;
}

// The history (esp_history_reserve: Zb, cb) and the projection buffers for K picks after the handle's r seeds (form 3; r = 0 on the
// chain).  Grows, never shrinks; a K that does not fit is refused before anything is freed or allocated.  Form 3: esp_tree_prepare
// runs the seeds through the history at its first call and copies their columns when the history grows.
inline int eig_free_reserve(machip_eig* h, int64_t K) {
    EigFree* F = h->fr;
    machip_esp* base = h->base;
    const EspTreeState* t = F->tree ? base->tr : nullptr;
    const int64_t cols = (int64_t)h->seeds + K;
    const int64_t K64 = (cols + kGjT - 1) / kGjT * kGjT;
    if (K64 > F->k64) {
        const double ld = (double)base->ld;
        const bool grow = (size_t)cols > base->zcap;
        const double hist = grow ? 8.0 * ld * (double)cols : 0.0;
        const double proj = 8.0 * ((double)K64 * h->ldq + (double)eig_free_part_elems((int)std::min<int64_t>(K64, INT_MAX), h->ldq, F->split));
        const double back = grow && !(t && t->seeded && t->seeds > 0) ? 8.0 * ld * (double)base->zcap : 0.0;      // (seeded columns are copied: old and new coexist)
        size_t fr = 0, tot = 0;
        HIP_TRY(hipMemGetInfo(&fr, &tot));
        if (hist + proj > (double)fr + back - 8.0 * ld * kEspFreeMaxSplit - 268435456.0)
            return fail(MACHIP_BAD_ARG, "the matrix-free history does not fit in device memory: n = " + std::to_string(h->n) + ", K = " + std::to_string((long long)K) +
                                            (t ? " and r = " + std::to_string(h->seeds) + " seeds ask for 8 ld (r + K) = " : " asks for 8 ld K = ") +
                                            std::to_string((unsigned long long)(8.0 * ld * (double)cols)) + " bytes (ld = " + std::to_string(base->ld) + ") and " +
                                            std::to_string((unsigned long long)proj) + " bytes of projections, " + std::to_string((unsigned long long)fr) +
                                            " bytes are free");
    }
    if (t) ST_TRY(esp_tree_prepare(base, K));
    else ST_TRY(esp_history_reserve(base, 0, false, K));
    if (K64 <= F->k64) return MACHIP_OK;
    HIP_TRY(hipStreamSynchronize(base->stream));
    if (F->Y) (void)hipFree(F->Y);
    if (F->part) (void)hipFree(F->part);
    F->Y = F->part = nullptr; F->k64 = 0;
    ST_TRY(dev_alloc(&F->Y, (size_t)K64 * (size_t)h->ldq));
    ST_TRY(dev_alloc(&F->part, eig_free_part_elems((int)K64, h->ldq, F->split)));
    F->k64 = (int)K64;
    return MACHIP_OK;
}

// z_e = Sigma_cur a_e and c_e of the columns bc[0..count) into Z / cc: Sigma0 a_e from R (form 2), or as the sweeps over the spanning
// tree left it in T (FROM_T: eig_tree_columns), minus the history's part
template <bool FROM_T = false>
inline int eig_free_columns(machip_eig* h, int count) {
    const EigFree* F = h->fr;
    const machip_esp* base = h->base;
    const EigView E = h->view();
    hipStream_t st = base->stream;
    const int j = base->pending, j64 = (j + kGjT - 1) / kGjT * kGjT;
    if (j > 0) {
        const size_t tot = (size_t)j64 * (size_t)h->ldq;
        k_eigf_alpha<<<(unsigned)std::min<size_t>(kMaxGrid, (tot + kBlock - 1) / kBlock), kBlock, 0, st>>>(E, base->Zb, base->cb, F->Y, j, j64, count);
    }
    k_eigf_back<true, FROM_T><<<dim3((count + kGjT - 1) / kGjT, base->ld / kGjT), 256, 0, st>>>(E, FROM_T ? nullptr : base->R, base->Zb, F->Y, j, count);
    k_eigf_cc<<<(count + kBlock - 1) / kBlock, kBlock, 0, st>>>(E, count);
    return MACHIP_OK;
}

// form 2, pass 1: T = Sigma0 Q for the live columns of the batch
inline void eig_free_scans(machip_eig* h, int count) {
    const EigFree* F = h->fr;
    const machip_esp* base = h->base;
    const EigView E = h->view();
    const dim3 sg((count + kGjT - 1) / kGjT, F->nchunks);
    k_eigf_scan<0><<<sg, kWave, 0, base->stream>>>(E, base->R, F->cs, F->cu, F->rows, count);
    k_eigf_scan<1><<<sg, kWave, 0, base->stream>>>(E, base->R, F->cs, F->cu, F->rows, count);
    k_eigf_scan<2><<<sg, kWave, 0, base->stream>>>(E, base->R, F->cs, F->cu, F->rows, count);
}

// both routes, passes 2 and 3: T -= Zb diag(cb) Zb^T Q, which leaves T = Sigma_cur Q
inline void eig_free_history(machip_eig* h, int count) {
    const EigFree* F = h->fr;
    const machip_esp* base = h->base;
    const int j = base->pending;
    if (j == 0) return;
    const EigView E = h->view();
    hipStream_t st = base->stream;
    const int cg = (count + kGjT - 1) / kGjT;
    const int jt = (j + kGjT - 1) / kGjT, j64 = jt * kGjT, ldp = cg * kGjT;
    const int S = eig_free_slices(base->ld, j, count, F->split);
    const int per = (base->ld / kEigFreePanel + S - 1) / S * kEigFreePanel;
    k_eigf_proj<<<dim3(cg, jt, S), 256, 0, st>>>(E, base->Zb, F->part, j, count, per, ldp, j64);
    const size_t tot = (size_t)j64 * (size_t)ldp;
    k_eigf_ysum<<<(unsigned)std::min<size_t>(kMaxGrid, (tot + kBlock - 1) / kBlock), kBlock, 0, st>>>(F->part, base->cb, F->Y, S, j, j64, ldp, h->ldq);
    k_eigf_back<false><<<dim3(cg, base->ld / kGjT), 256, 0, st>>>(E, base->R, base->Zb, F->Y, j, count);
}

// the winner's z_e, c_e (column 0 of Z / cc after its polished solve) become column j of the history
inline int eig_free_push(machip_eig* h) {
    machip_esp* base = h->base;
    const int j = base->pending;
    if ((size_t)j >= base->zcap) return fail(MACHIP_BAD_ARG, "GreedyEig: the matrix-free history is full");
    HIP_TRY(hipMemcpyAsync(base->Zb + (size_t)j * (size_t)base->ld, h->Z, sizeof(double) * (size_t)base->ld, hipMemcpyDeviceToDevice, base->stream));
    HIP_TRY(hipMemcpyAsync(base->cb + j, h->cc, sizeof(double), hipMemcpyDeviceToDevice, base->stream));
    base->pending = j + 1;
    return MACHIP_OK;
}

}  // namespace machip
