// kernels.h -- hand-written gfx950 kernels of the Frank-Wolfe / Fiedler hot path.
//
// All of this is HBM/L2-bound integer + fp64 streaming work: no MFMA (there is no dense
// contraction on the path).  Conventions: 256-thread workgroups (4 wave64), grids capped at
// kMaxGrid workgroups with grid-stride loops, reductions = wave butterfly -> 4-entry LDS ->
// one partial per workgroup, re-reduced in fixed order by the consumer kernel (bit-
// reproducible; no floating-point atomics anywhere).
#pragma once
#include <algorithm>

#include "common.h"

namespace machip {

// ------------------------------------------------------------------------------------------
// Views (passed by value as kernel arguments)
// ------------------------------------------------------------------------------------------
template <typename T>
struct CsrViewT {
    int n;
    const int* rowptr;   // n+1
    const int* col;      // nnz
    const T* val;        // nnz
};
using CsrView = CsrViewT<double>;    // float: the low-precision copy of the values used by the mixed-precision mode

// Union sparsity pattern of fixed + candidate edges (built once, machip_create):
// row r owns slots [prow[r], prow[r+1]); slot p is the off-diagonal (r, pcol[p]) fed by
// candidate pk[p] (weight pw[p] = w_k) or, when pk[p] < 0, by fixed edges (pw[p] = summed
// fixed weight).  Slots are sorted by column inside a row.
struct PatternView {
    int n;
    const int* prow;
    const int* pcol;
    const int* pk;
    const double* pw;
};

struct LanState {   // device-resident step counters: kernels take no per-step arguments,
    int jA;         // so a chunk of steps can be replayed from a hipGraph.  Fused form: jA = first
    int jB;         // step of the current chunk.  Classic form: jA is
    int epoch;      // read by the SpMV kernel, jB by k_lan_update.  epoch tags the host flag.
    int jN;         // fused form: first step of the NEXT chunk.  A chunk's first step (jrel == 0) reads jN and sets jA = jN, its other
                    // steps read jA; its last step (or its tail kernel) sets jN = jA + steps.  No launch reads a counter that
                    // a workgroup of the same launch writes (chunks have at least two steps).
};

struct LanView {
    int n;
    LanState* st;
    double* u;        // un-normalised next Lanczos vector (n)
    double* w;        // L v_j (n)
    double* V;        // Lanczos basis, column-major n x cap
    double* alpha;    // cap
    double* beta;     // cap+1; beta[j] = ||u_j|| couples v_{j-1}, v_j
    double* l1;       // cap+1; ||v_j||_1
    double* part_u;   // 3 x kMaxGrid partials of (sum u, sum u^2, sum |u|)
    int P_u;          // number of valid partials per row of part_u
    double* part_a;   // kMaxGrid partials of alpha
    int P_a;
};

// ------------------------------------------------------------------------------------------
// Laplacian assembly  (reference: MAC.laplacian, mac/solvers/mac.py:74-89, and
// weight_graph_lap_from_edges, mac/utils/graphs.py:58-98)
// ------------------------------------------------------------------------------------------
constexpr int kAsmGrid = 4096;     // most workgroups of the assembly kernels (stride of their per-workgroup result arrays)
// Which candidates are in the support: bit k of `bits` = (x_k > tol) (mac.py:85).  Written by whoever writes x -- k_fw_final for
// the next iterate (for free: one ballot per wave), k_x_bits for an x that came from the host -- and read by both assembly passes
// instead of x itself (2 M candidates = 250 KB: every gather is an L2 hit).  (Rounds 1-4 gathered x[pk] for every slot of the
// pattern in the count pass and parked x_k w_k per slot for the fill pass: 4.2 M scattered 8-byte gathers and 68 MB of parked
// values per Frank-Wolfe iteration at configs[3], whatever the support was.)
__global__ __launch_bounds__(kBlock) void k_x_bits(const double* __restrict__ x, long m, double tol, unsigned long long* __restrict__ bits) {
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < m; i += (long)gridDim.x * kBlock) {
        const unsigned long long bal = __ballot(x[i] > tol);      // (a wave covers 64 consecutive, 64-aligned candidates)
        if ((threadIdx.x & 63) == 0) bits[i >> 6] = bal;
    }
}
__device__ __forceinline__ bool x_bit(const unsigned int* __restrict__ bits32, int k) { return (bits32[k >> 5] >> (k & 31)) & 1u; }

// Pass 1: active entries per row (+1 for the diagonal) and one total per workgroup.
template <int G>
__global__ __launch_bounds__(kBlock) void k_asm_count(PatternView P, const unsigned int* __restrict__ xbits,
                                                      int rows_per_block,
                                                      int* __restrict__ cnt, int* __restrict__ blk_sum,
                                                      int* __restrict__ hsum = nullptr) {
    __shared__ int sm[4];
    constexpr int GPB = kBlock / G;
    const int lane = threadIdx.x % G, g = threadIdx.x / G;
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = min(P.n, r0 + rows_per_block);
    int local = 0, supp = 0, mx = 0;
    for (int r = r0 + g; r < r1; r += GPB) {
        const int b = P.prow[r], e = P.prow[r + 1];
        int c = 0, sc = 0;
        for (int p = b + lane; p < e; p += G) {
            const int k = P.pk[p];
            const bool cand = k >= 0;
            const bool act = cand ? x_bit(xbits, k) : true;
            c += act;
            sc += (cand && act);          // every candidate owns two slots (row i and row j): the support is half of this
        }
        c = group_sum_i<G>(c);
        sc = group_sum_i<G>(sc);
        if (lane == 0) {
            cnt[r] = c + 1;
            local += c + 1;
            supp += sc;
            mx = max(mx, c + 1);
        }
    }
    const int tot = block_sum_i(local, sm);
    const int stot = block_sum_i(supp, sm);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, kWave));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        blk_sum[blockIdx.x] = tot;
        blk_sum[kAsmGrid + blockIdx.x] = stot;                                   // active candidate slots (2 per candidate)
        const int longest = max(max(sm[0], sm[1]), max(sm[2], sm[3]));
        blk_sum[2 * kAsmGrid + blockIdx.x] = longest;                            // longest row
        if (hsum) {     // the host's copy, written straight into mapped pinned memory (no copy kernel behind the launch)
            hsum[blockIdx.x] = tot; hsum[kAsmGrid + blockIdx.x] = stot; hsum[2 * kAsmGrid + blockIdx.x] = longest;
        }
    }
}

// Pass 2: workgroup base = sum of the preceding workgroup totals; exclusive scan of the row
// counts in LDS; each G-lane group compacts the active slots of its rows (ballot + popcount,
// order preserved => columns stay sorted) behind the diagonal entry.
// Round 5: the fill pass also leaves what the column-panel form (panel.h) needs of every row -- where its entries of each column
// panel start (`ps`), its tridiagonal band (`bd`, `bpk`) -- while the row's columns are in registers anyway: k_pan_rows (one thread
// walking one row, 36 us per Frank-Wolfe iteration at configs[3]) no longer runs on matrices this library assembles.  The panel
// shape is a function of n alone, so the table is written before the host knows whether the panel step will run (NP = 0: no table).
struct PanSpec {
    int NP = 0;             // column panels (0: nothing to write)
    int C = 1;              // columns per panel
    int band = 0;           // columns r - 1 / r + 1 are kept out of the tiles
    int* ps = nullptr;      // [n][NP + 1] first off-diagonal entry of row r at or behind panel p
    double* bd = nullptr;   // [3][n] diagonal, column r - 1, column r + 1
    int* bpk = nullptr;     // [n] (CSR index of the row's first off-diagonal band entry) << 3 | how many there are
    int* ovf = nullptr;     // raised when a row holds more than 7 band entries (duplicates of a chain pair): the gather step serves the matrix
};

template <int G>
__global__ __launch_bounds__(kBlock) void k_asm_fill(PatternView P, const unsigned int* __restrict__ xbits, const double* __restrict__ x,
                                                     int rows_per_block,
                                                     const int* __restrict__ cnt,
                                                     const int* __restrict__ blk_sum,
                                                     int* __restrict__ rowptr, int* __restrict__ col,
                                                     double* __restrict__ val,
                                                     double* __restrict__ blk_lnorm, PanSpec S = PanSpec()) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    int* s_off = reinterpret_cast<int*>(smem_raw);                    // rows_per_block + 1
    __shared__ int sm_i[4];
    __shared__ double sm_d[4];
    __shared__ int s_chunk[kBlock];
    constexpr int GPB = kBlock / G;
    const int tid = threadIdx.x;
    const int lane = tid % G, g = tid / G;
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = min(P.n, r0 + rows_per_block);
    const int nr = max(0, r1 - r0);

    int acc = 0;
    for (int b = tid; b < (int)blockIdx.x; b += kBlock) acc += blk_sum[b];
    const int base = block_sum_i(acc, sm_i);

    // exclusive scan of cnt[r0..r1) -> s_off[0..nr]: per-thread runs of `per` rows, wave scans, four wave totals
    // (round 5: thread 0 used to walk the 256 per-thread sums in LDS one after the other -- a 12 us chain at the head of every workgroup)
    const int per = (nr + kBlock - 1) / kBlock;
    int csum = 0;
    for (int i = 0; i < per; ++i) {
        const int idx = tid * per + i;
        if (idx < nr) csum += cnt[r0 + idx];
    }
    {
        const int ln = tid & 63, wv = tid >> 6;
        int x = csum;
        for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o, kWave); if (ln >= o) x += y; }
        if (ln == 63) s_chunk[wv] = x;
        __syncthreads();
        int before = 0;
        for (int q = 0; q < wv; ++q) before += s_chunk[q];
        int run = before + x - csum;          // exclusive prefix of this thread's rows
        if (tid == kBlock - 1) s_off[nr] = before + x;
        for (int i = 0; i < per; ++i) {
            const int idx = tid * per + i;
            if (idx < nr) { s_off[idx] = run; run += cnt[r0 + idx]; }
        }
    }
    __syncthreads();

    double lmax = 0.0;
    for (int r = r0 + g; r < r1; r += GPB) {
        const int b = P.prow[r], e = P.prow[r + 1];
        const int out = base + s_off[r - r0];
        int pos = out + 1;
        double dsum = 0.0, asum = 0.0;
        int lastpid = 0;                        // panel of the row's last active entry so far (group-uniform)
        int hb = 0x7fffffff, hn = 0;            // band entries (columns r - 1, r + 1): first position, how many
        double vl = 0.0, vu = 0.0;
        const int gbase = ((tid & 63) / G) * G; // first lane of this group inside its wave
        for (int p0 = b; p0 < e; p0 += G) {
            const int p = p0 + lane;
            const bool in = p < e;
            const int kc = in ? P.pk[p] : -1;
            // (x_k, the support bit and the weight are requested together: behind one another they were three dependent round trips
            // per 32 slots -- 88 us per launch at configs[3])
            const double wgt = in ? P.pw[p] : 0.0;
            const double xk = kc >= 0 ? x[kc] : 1.0;
            const bool act = in && (kc < 0 || x_bit(xbits, kc));
            const double v = act ? xk * wgt : 0.0;     // x_k w_k exactly as mac.py:86 forms it (fixed slots: 1.0 x the weight)
            const unsigned long long bal = __ballot(act);
            unsigned long long gm;
            if (G == 64) gm = bal;
            else gm = (bal >> gbase) & ((1ull << (G & 63)) - 1ull);
            const unsigned long long below = gm & ((1ull << lane) - 1ull);
            const int before = __popcll(below);
            const int c = act ? P.pcol[p] : 0;
            if (act) { col[pos + before] = c; val[pos + before] = -v; }
            if (S.NP) {
                // entry at position q of panel pid, its predecessor in the row of panel ppid: the panels (ppid, pid] start at q
                const int pid = act ? c / S.C : 0;
                const int src = below ? 63 - __builtin_clzll(below) : 0;
                const int got = __shfl(pid, gbase + src, kWave);
                const int ppid = below ? got : lastpid;
                if (act) {
                    const int q = pos + before;
                    for (int pp = ppid + 1; pp <= pid; ++pp) S.ps[(size_t)r * (S.NP + 1) + pp] = q;
                    if (S.band && (c == r - 1 || c == r + 1)) {     // (accumulated: with more than G band slots -- duplicate chain pairs -- a lane meets several)
                        hb = min(hb, q); hn += 1;
                        if (c == r - 1) vl += -v; else vu += -v;
                    }
                }
                if (gm) lastpid = __shfl(pid, gbase + 63 - __builtin_clzll(gm), kWave);
            }
            pos += __popcll(gm);
            dsum += v;
            asum += fabs(v);
        }
        dsum = group_sum<G>(dsum);
        asum = group_sum<G>(asum);
        if (S.NP) {
            if (lane == 0) S.ps[(size_t)r * (S.NP + 1)] = out + 1;
            for (int pp = lastpid + 1 + lane; pp <= S.NP; pp += G) S.ps[(size_t)r * (S.NP + 1) + pp] = pos;      // panels behind the last entry
            if (S.band) {
                hn = group_sum_i<G>(hn);
                vl = group_sum<G>(vl); vu = group_sum<G>(vu);          // (one lane holds each value, the others add exact zeros)
#pragma unroll
                for (int o = G / 2; o > 0; o >>= 1) hb = min(hb, __shfl_xor(hb, o, kWave));
                if (lane == 0) {
                    S.bpk[r] = ((hn ? hb : pos) << 3) | min(hn, 7);
                    if (hn > 7) *S.ovf = 1;
                    S.bd[r] = dsum; S.bd[(size_t)P.n + r] = vl; S.bd[2 * (size_t)P.n + r] = vu;
                }
            }
        }
        if (lane == 0) {
            rowptr[r] = out;
            col[out] = r;
            val[out] = dsum;
            lmax = fmax(lmax, fabs(dsum) + asum);
        }
    }
    lmax = block_max(lmax, sm_d);
    if (tid == 0) {
        blk_lnorm[blockIdx.x] = lmax;
        if (blockIdx.x == gridDim.x - 1) rowptr[P.n] = base + s_off[nr];
    }
}

// ------------------------------------------------------------------------------------------
// CSR SpMV bodies.  Two row-to-lane mappings share one "Op" epilogue:
//   * vec<G>:   a G-lane sub-wave group per row, direct coalesced loads of (col,val) along
//               the row, butterfly reduce.  Right for long rows.
//   * stream<TPR>: the workgroup stages the products val*x[col] of a contiguous nnz tile in
//               LDS with perfectly coalesced loads, then TPR lanes per row reduce the row's
//               LDS segment ("CSR-stream" row tiles).  Right for short rows.
// Op interface: begin(sm) once per workgroup; row(r, acc) by one lane per row; end(sm).
// ------------------------------------------------------------------------------------------
template <int G, class Op>
__device__ __forceinline__ void spmv_rows_vec(const CsrView& A, const double* __restrict__ x, Op& op) {
    constexpr int GPB = kBlock / G;
    const int lane = threadIdx.x % G, g = threadIdx.x / G;
    // two rows of a group in flight (late round 5): a row is one dependent chain rowptr -> (col, val) -> gather -> butterfly, and with
    // 8 192 rows resident the 100 000 rows of configs[3] were twelve such round trips one after the other (38 us for 48 MB).  Every
    // row is still added up in the same order: same bits.
    const int stride = gridDim.x * GPB;
    for (int r = blockIdx.x * GPB + g; r < A.n; r += 2 * stride) {
        const int r2 = r + stride;
        const bool two = r2 < A.n;
        const int b = A.rowptr[r], e = A.rowptr[r + 1];
        const int b2 = two ? A.rowptr[r2] : 0, e2 = two ? A.rowptr[r2 + 1] : 0;
        double acc = 0.0, acc2 = 0.0;
        int p = b + lane, q = b2 + lane;
        while (p < e || q < e2) {
            double v1 = 0.0, x1 = 0.0, v2 = 0.0, x2 = 0.0;
            if (p < e) { v1 = A.val[p]; x1 = op.gather(x, A.col[p]); }
            if (q < e2) { v2 = A.val[q]; x2 = op.gather(x, A.col[q]); }
            if (p < e) acc += v1 * x1;
            if (q < e2) acc2 += v2 * x2;
            p += G; q += G;
        }
        acc = group_sum<G>(acc);
        acc2 = group_sum<G>(acc2);
        if (lane == 0) { op.row(r, acc); if (two) op.row(r2, acc2); }
    }
}

constexpr int kStreamTile = 2048;   // staged products per LDS tile (16 KB)

template <int TPR, class Op>
__device__ __forceinline__ void spmv_rows_stream(const CsrView& A, const double* __restrict__ x, Op& op,
                                                 double* prod, int* sptr) {
    constexpr int R = kBlock / TPR;
    const int tid = threadIdx.x;
    const int row = tid / TPR, sub = tid % TPR;
    for (int tile = blockIdx.x; tile * R < A.n; tile += gridDim.x) {
        const int r0 = tile * R;
        const int nr = min(R, A.n - r0);
        for (int i = tid; i <= nr; i += kBlock) sptr[i] = A.rowptr[r0 + i];   // nr + 1 offsets (TPR = 1: 257 > 256 threads)
        __syncthreads();
        const int p0 = sptr[0], p1 = sptr[nr];
        double acc = 0.0;
        for (int base = p0; base < p1; base += kStreamTile) {
            const int cnt = min(kStreamTile, p1 - base);
            for (int i = tid; i < cnt; i += kBlock) prod[i] = A.val[base + i] * op.gather(x, A.col[base + i]);
            __syncthreads();
            if (row < nr) {
                const int lo = max(sptr[row], base), hi = min(sptr[row + 1], base + cnt);
                for (int q = lo + sub; q < hi; q += TPR) acc += prod[q - base];
            }
            __syncthreads();
        }
        acc = group_sum<TPR>(acc);
        if (row < nr && sub == 0) op.row(r0 + row, acc);
        __syncthreads();
    }
}

// ---- plain y = A x ---------------------------------------------------------------------------
struct OpPlain {
    double* y;
    __device__ __forceinline__ void begin(double*) {}
    __device__ __forceinline__ double gather(const double* __restrict__ x, int c) const { return x[c]; }
    __device__ __forceinline__ void row(int r, double acc) { y[r] = acc; }
    __device__ __forceinline__ void end(double*) {}
};

// ---- fused Lanczos step, part 1 ---------------------------------------------------------------
// v_j = (u - mean(u)) / beta_j  (deflates the constant null vector exactly like nx:209-213's
// project(); L 1 = 0 so the SpMV can gather the raw u and scale afterwards),
// w = L v_j, alpha partial = v_j . (w - beta_j v_{j-1})   (Paige's ordering).
struct OpLanczos {
    LanView L;
    int j;
    double mu, beta, inv, ap;
    const double* vprev;
    double* vj;
    __device__ __forceinline__ void begin(double* sm) {
        j = L.st->jA;
        const double s1 = reduce_partials(L.part_u, L.P_u, sm);
        const double s2 = reduce_partials(L.part_u + kMaxGrid, L.P_u, sm);
        const double s3 = reduce_partials(L.part_u + 2 * kMaxGrid, L.P_u, sm);
        mu = s1 / (double)L.n;
        const double nrm2 = s2 - (double)L.n * mu * mu;
        beta = nrm2 > 0.0 ? sqrt(nrm2) : 0.0;
        inv = beta > 1e-290 ? 1.0 / beta : 0.0;
        ap = 0.0;
        vj = L.V + (size_t)j * (size_t)L.n;
        vprev = j > 0 ? vj - L.n : nullptr;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            L.beta[j] = beta;
            L.l1[j] = s3 * inv;
            L.st->jB = j;
        }
    }
    __device__ __forceinline__ double gather(const double* __restrict__ x, int c) const { return x[c]; }
    __device__ __forceinline__ void row(int r, double acc) {
        const double wr = acc * inv;
        const double v = (L.u[r] - mu) * inv;
        vj[r] = v;
        L.w[r] = wr;
        const double t = vprev ? wr - beta * vprev[r] : wr;
        ap += v * t;
    }
    __device__ __forceinline__ void end(double* sm) {
        const double tot = block_sum(ap, sm);
        if (threadIdx.x == 0) L.part_a[blockIdx.x] = tot;
    }
};

template <int G, class Op>
__global__ __launch_bounds__(kBlock) void k_spmv_vec(CsrView A, const double* __restrict__ x, Op op) {
    __shared__ double sm[4];
    op.begin(sm);
    spmv_rows_vec<G>(A, x, op);
    op.end(sm);
}

template <int TPR, class Op>
__global__ __launch_bounds__(kBlock) void k_spmv_stream(CsrView A, const double* __restrict__ x, Op op) {
    __shared__ double sm[4];
    __shared__ double prod[kStreamTile];
    __shared__ int sptr[kBlock / TPR + 1];
    op.begin(sm);
    spmv_rows_stream<TPR>(A, x, op, prod, sptr);
    op.end(sm);
}

// ---- landscape weighting of the cold-start vector (late round 5; solver_lanczos.h `landscape_start`) ----------------
// On sparse random graphs the Fiedler vector is LOCALISED: a handful of vertices carry it (participation ratio 1-5 on every
// iterate of configs[1] / configs[3]) -- the weakest spot of the graph, which the Frank-Wolfe update then reinforces, so the
// spot moves every iteration and the previous vector is no better a start than a random one (measured: `use_cache` +3 % steps).
// Where low eigenvectors of a Laplacian-like operator localise is predicted by its landscape function u, L u = 1
// (Filoche & Mayboroda 2012): they live on the peaks of u.  A few Jacobi sweeps u <- u + D^-1 (1 - L u) from u = D^-1 give u's
// shape over a few hops (the sweeps do not converge -- L is singular -- and need not); the start vector z is then multiplied
// entry by entry by (u / max u)^p, p ~ 100: the signs and relative sizes of z stay, the mass moves to the peaks.  Lanczos sorts
// out the rest; CPU emulation on the bench trajectories (tools/experiments/start_landscape_emulation.py): -16 % steps at
// configs[1], -17 % at configs[3], -11 % / +-1 % on city10000 / sphere2500, for k SpMV-priced launches per solve.
__global__ __launch_bounds__(kBlock) void k_land_init(CsrView A, double* __restrict__ dg, double* __restrict__ u) {
    for (int r = blockIdx.x * kBlock + threadIdx.x; r < A.n; r += gridDim.x * kBlock) {
        double d = 0.0;
        for (int p = A.rowptr[r], e = A.rowptr[r + 1]; p < e; ++p)
            if (A.col[p] == r) { d = A.val[p]; break; }        // (assembled matrices carry the diagonal first; a caller's CSR anywhere)
        dg[r] = d;
        u[r] = d > 0.0 ? 1.0 / d : 0.0;
    }
}
struct OpLand {
    const double* uin;
    double* uout;
    const double* dg;
    double* pmax;       // per-workgroup maxima of the sweep's output
    double mx;
    __device__ __forceinline__ void begin(double*) { mx = 0.0; }
    __device__ __forceinline__ double gather(const double* __restrict__ x, int c) const { return x[c]; }
    __device__ __forceinline__ void row(int r, double acc) {
        const double d = dg[r];
        double v = d > 0.0 ? uin[r] + (1.0 - acc) / d : 0.0;     // = (1 + sum_j w_rj u_j) / d_r for a Laplacian: positive
        v = v > 0.0 && v < 1e300 ? v : 0.0;                       // (a caller's matrix need not be a Laplacian)
        uout[r] = v;
        mx = fmax(mx, v);
    }
    __device__ __forceinline__ void end(double* sm) {
        const double m = block_max(mx, sm);
        if (threadIdx.x == 0) pmax[blockIdx.x] = m;
    }
};
// z_r <- z_r max((u_r / max u)^p, floor).  The maximum is re-reduced by every workgroup in the same order; a zero landscape (no positive
// diagonal at all) leaves z alone.  The FLOOR (round 6, advisor finding on round 5): (u / max u)^128 underflows to exactly 0 below
// u / max u ~ 3e-3 and is under 1e-16 below ~0.75, so the un-floored start is supported on a handful of lowest-degree vertices -- and when
// the Fiedler vector vanishes there (a weakly attached vertex at a nodal point of a symmetric graph: tests, test_landscape_start_floor)
// its overlap with the start is rounding noise, Lanczos converges to lambda_3 first, and the explicit residual test cannot tell: lambda_3 is a
// true eigenpair.  With every entry keeping >= 1e-3 of its random draw the overlap stays ~1e-3 / sqrt(n) of a random vector's: the right
// pair emerges (NumPy emulation of that graph: floor 0 and 1e-6 return lambda_3, 1e-4 .. 1e-2 return lambda_2 in as many steps as the plain start).
__global__ __launch_bounds__(kBlock) void k_land_weight(const double* __restrict__ u, const double* __restrict__ pmax, int npart,
                                                        double* __restrict__ z, int n, double p, double floor_w) {
    __shared__ double sm[4];
    double m = 0.0;
    for (int i = threadIdx.x; i < npart; i += kBlock) m = fmax(m, pmax[i]);
    m = block_max(m, sm);
    if (!(m > 0.0)) return;
    const double inv = 1.0 / m;
    for (int r = blockIdx.x * kBlock + threadIdx.x; r < n; r += gridDim.x * kBlock) {
        const double q = u[r] * inv;
        z[r] *= fmax(q > 0.0 ? exp(p * log(q)) : 0.0, floor_w);
    }
}

// ---- fused Lanczos step, part 2 ----------------------------------------------------------------
// alpha_j = sum of partials; u <- (w - alpha_j v_j) - beta_j v_{j-1}; partial sums of u for the
// next normalisation.  Advances the step counter read by part 1.
__global__ __launch_bounds__(kBlock) void k_lan_update(LanView L) {
    __shared__ double sm[4];
    const int j = L.st->jB;
    const double alpha = reduce_partials(L.part_a, L.P_a, sm);
    const double beta = L.beta[j];
    const double* vj = L.V + (size_t)j * (size_t)L.n;
    const double* vp = j > 0 ? vj - L.n : nullptr;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int r = blockIdx.x * kBlock + threadIdx.x; r < L.n; r += gridDim.x * kBlock) {
        double t = L.w[r] - alpha * vj[r];
        if (vp) t -= beta * vp[r];
        L.u[r] = t;
        s1 += t;
        s2 += t * t;
        s3 += fabs(t);
    }
    s1 = block_sum(s1, sm);
    s2 = block_sum(s2, sm);
    s3 = block_sum(s3, sm);
    if (threadIdx.x == 0) {
        L.part_u[blockIdx.x] = s1;
        L.part_u[kMaxGrid + blockIdx.x] = s2;
        L.part_u[2 * kMaxGrid + blockIdx.x] = s3;
        if (blockIdx.x == 0) {
            L.alpha[j] = alpha;
            L.st->jA = j + 1;
        }
    }
}

// One workgroup: finish the pending (beta, ||v||_1) of the vector produced by the last update so
// the host can read the residual factor without running another SpMV.
__global__ __launch_bounds__(kBlock) void k_lan_tail(LanView L) {
    __shared__ double sm[4];
    const int j = L.st->jA;
    const double s1 = reduce_partials(L.part_u, L.P_u, sm);
    const double s2 = reduce_partials(L.part_u + kMaxGrid, L.P_u, sm);
    const double s3 = reduce_partials(L.part_u + 2 * kMaxGrid, L.P_u, sm);
    if (threadIdx.x == 0) {
        const double mu = s1 / (double)L.n;
        const double nrm2 = s2 - (double)L.n * mu * mu;
        const double beta = nrm2 > 0.0 ? sqrt(nrm2) : 0.0;
        L.beta[j] = beta;
        L.l1[j] = beta > 1e-290 ? s3 / beta : 0.0;
    }
}

// ------------------------------------------------------------------------------------------
// One-kernel Lanczos step ("pipelined" form).  A kernel boundary costs ~2.3 us on this chip, every
// kernel here starts with a cold L2 (the per-XCD L2s are written back / invalidated at launch
// boundaries) and is latency-bound, so a Lanczos step is ONE launch:
//   * step j first finishes the reductions of step j-1 (alpha_{j-1}, beta_j, mean) from per-
//     workgroup partials (wave 0 of every workgroup, overlapping the other waves' CSR loads),
//   * and uses v_j without materialising it.  With Paige's intermediate
//         t_{j-1} = L v_{j-1} - beta_{j-1} v_{j-2}          (stored by step j-1, which knows beta_{j-1})
//     the new vector is   v_j[c] = ( t_{j-1}[c] - alpha_{j-1} v_{j-1}[c] - mu ) / beta_j ,
//     so the gather operand is ONE aligned 16-byte record Z[c] = {t_{j-1}, v_{j-1}}.  By linearity
//     the SpMV accumulates the two raw sums (L t)[r], (L v)[r] and combines them afterwards
//     (L 1 = 0 removes mu): the matrix/gather phase does not depend on the reduction at all.
//   * alpha_{j-1} = v.t and beta_j^2 = t.t - 2 alpha v.t + alpha^2 v.v - n mu^2 come from inner
//     products that are all MEASURED, nothing is assumed orthonormal: the quadratic form is exact
//     for the vectors actually stored, so a rounding error in beta only rescales v_j and is
//     accounted for one step later.  (Assuming |v| = 1 or dropping "tiny" terms turns that into an
//     error-feedback loop that blows up in ~20 steps -- found by emulation.)
//   * no per-step host arguments: j = jA (chunk base, device memory) + jrel (baked into the graph
//     node); chunks have an even number of steps so the Z / partial ping-pong parity is jrel & 1.
// ------------------------------------------------------------------------------------------
// Storage type T of the iterate: double, or float for the mixed-precision mode (machip_set_precision(1): fp32 matrix
// values, 8-byte records, fp32 basis; every inner product is still accumulated in fp64 and taken of the STORED,
// i.e. rounded, vectors, so the quadratic form below stays exact for what is in memory).
template <typename T> struct ZRec;
template <> struct __attribute__((aligned(16))) ZRec<double> { double t, v; };
template <> struct __attribute__((aligned(8))) ZRec<float> { float t, v; };
using Z2 = ZRec<double>;
constexpr int kNP = 6;    // partial sums per workgroup: t.t  t.v  v.v  sum(t)  sum(v)  |v|_1
constexpr int kMaxChunk = 64;
constexpr int kMaxWaves = 16;

template <typename T>
struct PipeViewT {
    int n;
    LanState* st;
    ZRec<T>* Z0;
    ZRec<T>* Z1;
    T* V;
    double* tri;      // interleaved (alpha_j, beta_j, ||v_j||_1) records
    double* htri;     // host-pinned mirror of tri, written by the tail kernel (zero-copy): the host
                      // polls hflag instead of issuing a stream-ordered copy between chunks
    unsigned long long* hflag;   // (epoch << 32) | J once records < J (and beta_J) are in htri
    double* part;     // 2 x kNP x kMaxGrid, ping-ponged like Z: a step reads half (jrel & 1) and
                      // writes the other, so a late-starting workgroup never sees partials that a
                      // fast workgroup of the SAME launch has already replaced
    int P;            // valid partials per quantity (= grid of the step kernel, <= 256)
    int chunk;        // > 0: this chunk has no tail kernel -- its last step (jrel == chunk - 1) advances jN itself, and its records
                      // reach the host through the NEXT chunk's first step (or a tail kernel the host adds when no chunk follows)
    int pub;          // > 0: the chunk before this one had `pub` steps and no tail: the first step publishes its records
    int pubstep;      // != 0: EVERY step hands its three values (alpha_{j-1}, l1_{j-1}, beta_j) to the host as it derives them (solver_lanczos.h,
                      // "streamed records": the host follows the recurrence step by step and decides where the solve ends)
    double* sig;      // != nullptr: SHIFTED records (panel_u.h, round 6): the sums are those of (u_j, v_j) with u_j = t_j - sigma_j v_j,
                      // sigma_j = alpha_{j-1}; sig[jrel & 1] = sigma_{j-1} on entry of step j, the prologue adds alpha'_{j-1} = u.v and
                      // leaves sigma_j in sig[(jrel + 1) & 1].  The tridiagonal records always carry the TRUE alpha.
#ifdef PIPE_CLOCKS
    long long* clk;   // tools/ubench5.hip: 8 wall-clock stamps (100 MHz) per workgroup
#endif
};
using PipeView = PipeViewT<double>;

#ifdef PIPE_CLOCKS   // tools/ubench5.hip: phase stamps of one worker lane and of the prologue wave per workgroup
#define PIPE_CLK(cond, i) do { if (cond) L.clk[blockIdx.x * 8 + (i)] = wall_clock64(); } while (0)
#else
#define PIPE_CLK(cond, i) do { } while (0)
#endif

struct PipeCoef { double alpha, mu, beta, inv, l1prev, atrue; };      // atrue: alpha of the un-shifted recurrence (= alpha unless PipeView::sig)

// Row-partitioned step (in-process communicator, machip_comm_init_local): rank r launches workgroups
// [first, first + gridDim.x) of the SAME `total`-workgroup launch a single rank would run -- same rows per workgroup,
// same partial sums, same order of additions, hence bit-identical results -- on its own copy of the matrix and of the
// gather operand, and writes what it produces (next records, partial sums) into every rank's copy (peer-mapped pointers
// across xGMI; plain device memory when the ranks share a GPU).  The basis column stays with the rank that owns the rows.
constexpr int kMaxPeers = 8;
struct PeerSet {
    int n = 0;            // 0: not sharded (the kernel uses blockIdx / gridDim and its own buffers only)
    int first = 0;        // global index of this launch's first workgroup
    int total = 0;        // workgroups of the whole step
    void* Z0[kMaxPeers];  // every rank's record buffers (ZRec<T>*)
    void* Z1[kMaxPeers];
    double* part[kMaxPeers];
};

// ---- device-ordered exchange between PROCESSES (round 4; machip_comm_init_ipc) ----------------------------
// Every rank maps the peers' record / partial-sum / vector / gradient buffers (hipIpcOpenMemHandle) and writes what it
// produces into every copy (PeerSet).  Ordering needs no host and no cross-stream edge: per channel (Lanczos steps, Ritz
// vector rows, gradient shards) a rank counts what it has published (`done`, its own memory) and publishes that count into a
// flag word of every peer (system-scope release, behind the producing kernel on the same stream); a consumer spins --
// bounded -- until every peer's count has reached its own.  All ranks run the same deterministic host logic on identical
// tridiagonal records, so they issue the same launches in the same order and the counts stay aligned.
constexpr int kIpcChannels = 4;          // 0 Lanczos steps, 1 Ritz-vector rows, 2 gradient shards, 3 spare
struct IpcView {
    int n = 0, rank = 0;                 // ranks in all (0: no IPC communicator), my rank
    unsigned long long* done = nullptr;              // [kIpcChannels] my publish counts
    unsigned long long* flags = nullptr;             // my flag words: [kIpcChannels][kMaxPeers], written by the peers (slot = writer's rank)
    unsigned long long* peer_flags[kMaxPeers] = {};  // every rank's flag array (mine included)
    int* err = nullptr;                  // mapped pinned host word: 1 = a wait timed out (a peer stalled or died), 2 = a peer raised abort
    long long timeout_ticks = 0;         // bound of one wait (100 MHz ticks)
};
__device__ __forceinline__ void ipc_publish(const IpcView& I, int ch) {
    const unsigned long long c = I.done[ch] + 1ull;
    I.done[ch] = c;
    __threadfence_system();              // (the producing kernel has ended; its writes are performed)
    for (int q = 0; q < I.n; ++q)
        if (q != I.rank) __hip_atomic_store(I.peer_flags[q] + ch * kMaxPeers + I.rank, c, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void ipc_wait(const IpcView& I, int ch) {
    if (*I.err) return;                  // already broken: do not spin again (a dead peer must cost ONE timeout, not one per step)
    const unsigned long long want = I.done[ch];
    const long long t0 = wall_clock64();
    for (int q = 0; q < I.n; ++q) {
        if (q == I.rank) continue;
        const unsigned long long* f = I.flags + ch * kMaxPeers + q;
        for (;;) {
            const unsigned long long v = __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);     // (relaxed poll: the consuming kernel's start is the acquire)
            if (v == ~0ull) { *I.err = 2; __threadfence_system(); return; }          // the peer raised abort
            if (v >= want) break;
            if (wall_clock64() - t0 > I.timeout_ticks) { *I.err = 1; __threadfence_system(); return; }
            __builtin_amdgcn_s_sleep(4);
        }
    }
}
__global__ void k_ipc_publish(IpcView I, int ch) { if (threadIdx.x == 0) ipc_publish(I, ch); }
__global__ void k_ipc_wait(IpcView I, int ch) { if (threadIdx.x == 0) ipc_wait(I, ch); }
// "my part of phase c is delivered" + "everybody's is": one launch between two kernels of a phase chain instead of two (round 5:
// a launch boundary, ~2.5 us, per Lanczos step of the row-partitioned solve)
__global__ void k_ipc_pubwait(IpcView I, int ch) { if (threadIdx.x == 0) { ipc_publish(I, ch); ipc_wait(I, ch); } }
__global__ void k_ipc_abort(IpcView I) {   // best effort: release the peers' waits with an error
    if (threadIdx.x != 0) return;
    for (int q = 0; q < I.n; ++q)
        if (q != I.rank)
            for (int ch = 0; ch < kIpcChannels; ++ch) __hip_atomic_store(I.peer_flags[q] + ch * kMaxPeers + I.rank, ~0ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
struct PeerVecs { int n = 0; double* v[kMaxPeers] = {}; };     // one vector per rank (y_raw, g)
// Deliveries into peer-visible copies (records, operand rows, partial sums, Ritz rows, gradient shards of a row-partitioned step) are
// WRITE-THROUGH stores at system scope, and a delivering wave waits for their acknowledgements before it ends (round 6).  Plain stores
// stay dirty in the L2 of the XCD the workgroup ran on; the flag that says "step j delivered" is published by the NEXT launch, whose
// one thread's system fence writes back ITS XCD's L2 only -- so a partial sum stored by the last instructions of a step kernel could be
// overtaken by the flag and a peer's prologue read the value of two steps before: 2 of 30 two-rank configs[3] runs ended with the ranks
// disagreeing about where a solve ends (round 5's library and round 6's alike; 3 of 14 with the panel step, whose deliveries all sit at
// the end of its row kernel; tools/archive/ipc_pan_debug.py).  MI355X_MICROARCH.md, row "publish-large": sc1 stores + vmcnt(0) + flag.
__device__ __forceinline__ void peer_store(double* p, double v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void peer_store(float* p, float v) { __hip_atomic_store(reinterpret_cast<unsigned int*>(p), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ __forceinline__ void peer_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ---- wave64 sum on the VALU (DPP row shifts + row broadcasts), ~5x faster than the
// ds_bpermute butterfly; the total lands in lane 63 and is broadcast through an SGPR. ----------
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_add(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int lo2 = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROWMASK, 0xf, false);
    const int hi2 = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROWMASK, 0xf, false);
    return v + __hiloint2double(hi2, lo2);
}
__device__ __forceinline__ double wave_total(double v) {
    v = dpp_add<0x111, 0xf>(v);   // row_shr:1
    v = dpp_add<0x112, 0xf>(v);   // row_shr:2
    v = dpp_add<0x114, 0xf>(v);   // row_shr:4
    v = dpp_add<0x118, 0xf>(v);   // row_shr:8   -> lane 15 of each row holds the row sum
    v = dpp_add<0x142, 0xa>(v);   // row_bcast:15 into rows 1,3
    v = dpp_add<0x143, 0xc>(v);   // row_bcast:31 into rows 2,3 -> lane 63 holds the wave sum
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), 63);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
    return __hiloint2double(hi, lo);
}

// N wave totals at once, stage by stage: the N chains are independent, so the DPP moves and adds of one stage issue
// back to back instead of each chain waiting out its own dependent latencies (results identical to wave_total).
template <int N>
__device__ __forceinline__ void wave_total_n(double (&v)[N]) {
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = dpp_add<0x111, 0xf>(v[q]);
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = dpp_add<0x112, 0xf>(v[q]);
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = dpp_add<0x114, 0xf>(v[q]);
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = dpp_add<0x118, 0xf>(v[q]);
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = dpp_add<0x142, 0xa>(v[q]);
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = dpp_add<0x143, 0xc>(v[q]);
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const int lo = __builtin_amdgcn_readlane(__double2loint(v[q]), 63);
        const int hi = __builtin_amdgcn_readlane(__double2hiint(v[q]), 63);
        v[q] = __hiloint2double(hi, lo);
    }
}

// Finish step j-1's reductions from the summed partials.  Identical on every workgroup.
__device__ __forceinline__ PipeCoef pipe_coefs(const double (&a)[kNP], int n) {
    PipeCoef c;
    const double tt = a[0], tv = a[1], vv = a[2];
    c.alpha = tv;                             // Paige: v.(L v - beta v_prev); 0 at j = 0 (v = 0)
    const double al = c.alpha;
    const double uu = tt - 2.0 * al * tv + al * al * vv;
    const double dn = (double)n;
    c.mu = (a[3] - al * a[4]) * __builtin_amdgcn_rcp(dn) * (2.0 - dn * __builtin_amdgcn_rcp(dn));   // one Newton step on the hardware reciprocal: the mean to 1e-15 relative without a division
    const double nrm2 = uu - dn * c.mu * c.mu;
    // ||u||^2 is a difference of O(||t||^2) terms: below ~1e-10 of their size it is rounding
    // noise, i.e. the Krylov space is (numerically) invariant -> report an exact breakdown.
    const double scale = tt + al * al * vv;
    // beta = ||u||, 1/beta through rsqrt (this chain -- it used to be a sqrt and a division, ~100 dependent fp64
    // instructions -- sits on the critical path of every step: the row waves wait for it at the barrier)
    const bool ok = nrm2 > 1e-10 * scale && nrm2 > 1e-290;
    const double rs = ok ? rsqrt(nrm2) : 0.0;
    c.beta = ok ? nrm2 * rs : 0.0;
    c.inv = c.beta > 1e-290 ? rs : 0.0;
    c.l1prev = a[5];
    return c;
}

// Prologue, run by wave 0 only: sum the P (<= 256) partials of each quantity, derive the
// coefficients, publish them to the workgroup through LDS (scoef) and -- workgroup 0 -- to the
// tridiagonal record.  The other waves go straight to their CSR loads.
// Zero-copy hand-off to the host (wave 0 of one workgroup): records [j-adv-1, j] of tri -> pinned host memory, then the flag.
template <class PV>
__device__ __forceinline__ void pipe_publish(const PV& L, const PipeCoef& c, int j, int adv) {
    const int lo = max(0, j - adv - 1);
    const int cnt = 3 * (j - lo + 1);
    // every host address is written exactly once: the three values this launch has just produced (alpha_{j-1},
    // l1_{j-1}, beta_j) go from registers, the bulk copy skips their slots (L.tri may still hold the old ones)
    const int sa = j > 0 ? 3 * (j - 1) : -1, sl = j > 0 ? 3 * (j - 1) + 2 : -1, sb = 3 * j + 1;
    for (int i = threadIdx.x; i < cnt; i += 64) {
        const int q = 3 * lo + i;
        if (q != sa && q != sl && q != sb && q < 3 * j) L.htri[q] = L.tri[q];   // (alpha_j, l1_j belong to the next chunk)
    }
    if (threadIdx.x == 0) {
        if (j > 0) { L.htri[sa] = c.atrue; L.htri[sl] = c.l1prev; }
        L.htri[sb] = c.beta;
    }
    // (round 5: no system-scope fence / release in front of the flag -- they made the one wave wait for the PCIe round trip of its
    // record stores.  The host never trusts the flag alone: every record slot of the chunk was poisoned with NaN before the chunk
    // was enqueued and is awaited individually (solver_lanczos.h lan_chunk_await), so a flag that overtakes its records costs nothing.)
    if (threadIdx.x == 0) {
        const unsigned long long epoch = (unsigned long long)(unsigned int)L.st->epoch;
        __hip_atomic_store(L.hflag, (epoch << 32) | (unsigned long long)(unsigned int)j, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// `lead`: this launch is the one of its step that advances the counters (the panel form runs the prologue in both of its launches);
// `pub_wg`: the workgroup that hands a tail-less predecessor chunk's records to the host (any workgroup can: all compute the same
// coefficients) -- the caller names one with slack.
// SIG = false: a kernel that never runs the shifted recurrence (the gather step, the record-form panel step) -- no sigma load at all: as a
// run-time test of L.sig, a field of the by-value view, it was a scalar load of the argument block, a wait and THEN the load, ~0.5 us
// behind the partial loads on the chain every row wave waits for at its first barrier (round 6).
template <bool SIG = true, class PV>
__device__ __forceinline__ PipeCoef pipe_prologue_wave0(const PV& L, int jrel, int adv_jA, double* scoef, int* j_out, int bid = -1,
                                                        bool lead = true, int pub_wg = 0) {
    // (sharded step: the tridiagonal records go to the launching rank's own arrays -- its first workgroup writes them; ranks of
    // one process share the leader's arrays and all write the same values, ranks in different processes each keep their own)
    bid = (int)blockIdx.x;
    const int lane = threadIdx.x;   // caller guarantees threadIdx.x < 64
    const int jA = *(jrel == 0 && adv_jA < 0 ? &L.st->jN : &L.st->jA);        // (requested first, consumed last: in flight together with the partial loads below)
    const double* __restrict__ pin = L.part + (size_t)(jrel & 1) * (kNP * kMaxGrid);
    // (shifted records: sigma is requested with the partials.  The load is UNCONDITIONAL -- the record form reads a partial it ignores --
    // because a branch here sat between the counter load and the 24 partial loads of every step of every form and cost the gather step
    // 0.24 us: configs[1] 6.40 -> 6.64 us, the 4-lane sweep -5 %, same-box A/B of round 5's library against round 6's first)
    double sg_prev = 0.0;
    if (SIG) { const double sg_raw = *(L.sig ? L.sig + (jrel & 1) : pin); sg_prev = L.sig ? sg_raw : 0.0; }
    double a[kNP];
    {   // The first 256 partials per quantity: 24 UNCONDITIONAL loads per lane (always in bounds: the arrays hold kMaxGrid
        // entries), masked afterwards.  Round 2, tools/ubench5.hip + the ISA: written as `i < P ? pin[..] : 0` (or as a loop
        // with a run-time trip count) the compiler emitted one predicated load + s_waitcnt per value -- 25 dependent cold
        // round trips, 3.2 us before the first partial was even requested: THE long pole of every step on matrices that
        // fit one row tile per workgroup (config 2, city10000).
        double v[kNP][4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int q = 0; q < kNP; ++q) v[q][c] = pin[q * kMaxGrid + lane + 64 * c];
#ifdef PIPE_CLOCKS
        asm volatile("" ::: "memory");
        if (lane == 0) L.clk[blockIdx.x * 8 + 3] = wall_clock64();     // (slot 3: partial loads ISSUED)
        asm volatile("" ::: "memory");
#endif
#pragma unroll
        for (int q = 0; q < kNP; ++q) {   // same order of additions as a plain loop over the workgroups
            a[q] = 0.0;
#pragma unroll
            for (int c = 0; c < 4; ++c) a[q] += (lane + 64 * c < L.P) ? v[q][c] : 0.0;
        }
    }
    for (int base = 256; base < L.P; base += 256) {   // grids beyond 256 workgroups (MACHIP_MAXGRID): same batching per 256
        double v[kNP][4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int q = 0; q < kNP; ++q) v[q][c] = pin[q * kMaxGrid + base + lane + 64 * c];    // base + 255 < kMaxGrid
#pragma unroll
        for (int q = 0; q < kNP; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c) a[q] += (base + lane + 64 * c < L.P) ? v[q][c] : 0.0;
    }
#ifdef PIPE_CLOCKS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) L.clk[blockIdx.x * 8 + 7] = wall_clock64();
#endif
    wave_total_n<kNP>(a);
    PipeCoef c = pipe_coefs(a, L.n);
    c.atrue = sg_prev + c.alpha;                // (record form: sg_prev = 0)
    const int j = jA + jrel;
    if (lane == 0) {
        scoef[0] = c.alpha; scoef[1] = c.beta; scoef[2] = c.mu; scoef[3] = c.inv; scoef[4] = (double)j; scoef[5] = c.atrue;
        if (bid == 0) {
            if (SIG && L.sig && lead && adv_jA < 0) L.sig[(jrel + 1) & 1] = c.atrue;      // sigma_j = alpha_{j-1}
            if (j > 0) { L.tri[3 * (j - 1)] = c.atrue; L.tri[3 * (j - 1) + 2] = c.l1prev; }
            L.tri[3 * j + 1] = c.beta;
            if (adv_jA >= 0) { L.st->jA = j; L.st->jN = j; }   // tail kernel: new chunk base
            else if (lead) {
                if (jrel == 0) L.st->jA = j;
                if (L.chunk > 0 && jrel == L.chunk - 1) L.st->jN = jA + L.chunk;
            }
        }
    }
    if (lead && adv_jA < 0 && jrel == 0 && L.pub > 0 && j > 0 && (int)blockIdx.x == pub_wg) pipe_publish(L, c, j, L.pub);
    if (lead && adv_jA < 0 && L.pubstep && (int)blockIdx.x == pub_wg && lane == 0) {
        // streamed records: three posted 8-byte stores into pinned host memory from ONE lane of one workgroup, ~4 us into a step --
        // acknowledged long before the launch ends.  No flag: the host awaits each (NaN-poisoned) slot.
        if (j > 0) { L.htri[3 * (j - 1)] = c.atrue; L.htri[3 * (j - 1) + 2] = c.l1prev; }
        L.htri[3 * j + 1] = c.beta;
    }
    *j_out = j;
    return c;
}

struct PipeRow {   // per-thread accumulation of the next step's partial sums
    double acc[kNP];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int q = 0; q < kNP; ++q) acc[q] = 0.0;
    }
    // raw sums (L t)[r], (L v)[r] -> w_j[r]; v_j[r] from Z[r]; store V, next Z = {t_j, v_j}.
    template <typename T>
    __device__ __forceinline__ void finish(double alpha, double beta, double mu, double inv, const ZRec<T>& z,
                                           double st, double sv, T* vj, ZRec<T>* Zn, int r, const PeerSet* PS = nullptr, int par = 0) {
        // Every product-sum below is an EXPLICIT fma (and nothing else may be fused): the generated code of two
        // instantiations of this kernel -- deferred barrier or not, row-partitioned or not -- used to differ in which of these
        // the compiler contracted, one unit in the last place apart, and the row-partitioned step must reproduce the
        // single-rank run bit for bit.
#pragma clang fp contract(off)
        const double zt = z.t, zv = z.v;
        const double w = __builtin_fma(-alpha, sv, st) * inv;
        ZRec<T> o;
        o.v = (T)((__builtin_fma(-alpha, zv, zt) - mu) * inv);
        o.t = (T)__builtin_fma(-beta, zv, w);       // Paige's intermediate for the next step
        const double v = o.v, t = o.t;              // the sums below are those of the vectors as stored
        vj[r] = o.v;
        if (PS && PS->n) {      // sharded step: the record goes into every rank's copy of the next operand
            for (int q = 0; q < PS->n; ++q) { ZRec<T>* zq = reinterpret_cast<ZRec<T>*>(par ? PS->Z0[q] : PS->Z1[q]) + r; peer_store(&zq->t, o.t); peer_store(&zq->v, o.v); }
        } else Zn[r] = o;
        acc[0] = __builtin_fma(t, t, acc[0]); acc[1] = __builtin_fma(t, v, acc[1]); acc[2] = __builtin_fma(v, v, acc[2]);
        acc[3] += t; acc[4] += v; acc[5] += fabs(v);
    }
    // One partial per quantity per workgroup.  sred: kNP x (BLOCK/64) x 64 doubles of LDS.  Round 2 (tools/ubench5.hip: "last
    // tile finished" -> "partials stored" took 1.7-2.3 us): a wave-wide fp64 total is 12 DPP moves + 6 adds, and with every
    // wave of the workgroup reducing all six quantities the SIMDs issued 6 x NW of them.  Now every lane parks its six
    // sums in LDS, and after the barrier wave q adds the NW values of its lane for quantity q and runs ONE wave total.
    template <int BLOCK, class PV>
    __device__ __forceinline__ void store(const PV& L, int jrel, double* sred, const PeerSet* PS = nullptr) {
        constexpr int NW = BLOCK / 64;
        const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
        for (int q = 0; q < kNP; ++q) sred[(q * NW + wv) * 64 + lane] = acc[q];
        __syncthreads();
        for (int q = wv; q < kNP; q += NW) {     // workgroup-uniform per wave
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < NW; ++w) s += sred[(q * NW + w) * 64 + lane];
            s = wave_total(s);
            if (lane == 0) {
                const size_t at = (size_t)((jrel + 1) & 1) * (kNP * kMaxGrid) + q * kMaxGrid;
                if (PS && PS->n) { for (int k = 0; k < PS->n; ++k) peer_store(PS->part[k] + at + PS->first + blockIdx.x, s); peer_drain(); }
                else L.part[at + blockIdx.x] = s;
            }
        }
    }
};

#define PIPE_ARGS(A, L, jrel) (A).rowptr, (A).col, (A).val, (((jrel) & 1) ? (L).Z1 : (L).Z0), (L).part, (L).st, (A).n, (jrel), (A), (L)

// ---- sub-wave vector form: G lanes per row, BLOCK threads per workgroup -------------------------
// Raw sums (L t)[r], (L v)[r] of one row by its G-lane group, and the row's own record (lane 0).
// ELLW > 0: the matrix is in padded fixed-width form (k_ell_build: ELLW slots per row, CSR order, padded with zero
// values on the row's own column), so a row's entries sit at r * ELLW -- no row-pointer load in front of the value / column
// loads, one dependent memory round trip less per step.  Zero products change nothing: the sums are those of the CSR walk.
template <int G, int UNR, typename T, int ELLW = 0>
__device__ __forceinline__ void pipe_row_sums(const CsrViewT<T>& A, const ZRec<T>* __restrict__ Zc, int r, int lane, bool mine,
                                              double& st, double& sv, ZRec<T>& zr) {
    using Z2 = ZRec<T>;
    st = 0.0; sv = 0.0;
    zr.t = 0; zr.v = 0;
    if (mine) {
        const int b = ELLW ? r * ELLW : A.rowptr[r], e = ELLW ? b + ELLW : A.rowptr[r + 1];
        if (lane == 0) zr = Zc[r];
        int p = b + lane;
        if (UNR > 1) {   // several independent (val, col, gather) chains in flight per lane
            for (; p + (UNR - 1) * G < e; p += UNR * G) {
                T vv[UNR];
                int cc[UNR];
                Z2 zz[UNR];
#pragma unroll
                for (int q = 0; q < UNR; ++q) { vv[q] = A.val[p + q * G]; cc[q] = A.col[p + q * G]; }
#pragma unroll
                for (int q = 0; q < UNR; ++q) zz[q] = Zc[cc[q]];
#pragma unroll
                for (int q = 0; q < UNR; ++q) { st = __builtin_fma((double)vv[q], (double)zz[q].t, st); sv = __builtin_fma((double)vv[q], (double)zz[q].v, sv); }
            }
        }
        for (; p < e; p += G) {
            const double vv = A.val[p];
            const Z2 z = Zc[A.col[p]];
            st = __builtin_fma(vv, (double)z.t, st); sv = __builtin_fma(vv, (double)z.v, sv);
        }
        st = group_sum<G>(st); sv = group_sum<G>(sv);
    }
}

// Round 2 (tools/ubench5.hip, wall-clock stamps per workgroup): the prologue of wave 0 -- 1 536 partials that the
// previous launch wrote from all XCDs, i.e. cold in this XCD's L2 -- is done 3.5-5.5 us after kernel entry, the first
// row tile after 1.9-4.4 us: with the barrier behind the first tile the row waves sat idle for up to 2 us per step.
// The coefficients are only needed by finish(), so the first DEFER tiles keep their raw sums in registers and the
// barrier comes after them; finish() then runs in the same row order as before (bit-identical partial sums).
template <int BLOCK, int G, int UNR = 1, bool DED = false, typename T = double, int DEFER = 3, bool SH = false, int ELLW = 0>
__global__ __launch_bounds__(BLOCK) void k_pipe_vec(const int* __restrict__ a_rowptr, const int* __restrict__ a_col, const T* __restrict__ a_val,
                                                    const ZRec<T>* __restrict__ z_cur, double* l_part, LanState* l_st, int a_n, int jrel,
                                                    CsrViewT<T> A_, PipeViewT<T> L_, PeerSet PS = PeerSet()) {
    using Z2 = ZRec<T>;
    // The pointers every wave needs for its FIRST loads come as leading scalar arguments (PIPE_ARGS): with
    // -amdgpu-kernarg-preload-count they are in SGPRs when the wave starts, instead of behind a scalar load of the argument
    // block (itself a cold round trip at the head of every step).  A_ / L_ carry the rest.
    // (Not for the padded fixed-width form: there every wave's value / column loads leave at kernel entry anyway, and having
    // them out even before wave 0's partial-sum loads measured 1.7 % slower on city10000; round 6 again: a tie.)
    // jrel is one of them (round 6): wave 0's partial-sum loads need its parity, and as a trailing argument it sat behind a scalar load
    // and a wait in front of them -- configs[1] 6.57 -> 6.33 us per step.
    const CsrViewT<T> A = ELLW ? A_ : CsrViewT<T>{a_n, a_rowptr, a_col, a_val};
    PipeViewT<T> L = L_;
    L.part = l_part; L.st = l_st;      // (the prologue's pointers are preloaded in either form: its chain is the longest)
    // SH: one rank's share of a row-partitioned step (PeerSet above); bid / gtot = this workgroup's index / the workgroup
    // count of the whole step, so that rows, partial sums and their order are those of the unsharded launch
    const int bid = SH ? PS.first + (int)blockIdx.x : (int)blockIdx.x;
    const int gtot = SH ? PS.total : (int)gridDim.x;
    const PeerSet* PSp = SH ? &PS : nullptr;
    const int par = jrel & 1;
    __shared__ double smw[kNP * BLOCK];     // epilogue scratch: six sums per lane
    __shared__ double scoef[8];
    // DED: wave 0 does nothing but the prologue (its reduction chain is then off the critical
    // path of the row work); the other waves own the rows.
    constexpr int WORK = DED ? BLOCK - 64 : BLOCK;
    constexpr int GPB = WORK / G;
    const int wt = DED ? (int)threadIdx.x - 64 : (int)threadIdx.x;
    const int lane = wt >= 0 ? wt % G : 0, g = wt >= 0 ? wt / G : 0;
    PIPE_CLK(threadIdx.x == 0, 0);
    PIPE_CLK(wt == 0, 2);
    if (threadIdx.x < 64) { int jdummy; (void)pipe_prologue_wave0<false>(L, jrel, -1, scoef, &jdummy, bid, true, (int)gridDim.x - 1); }
    PIPE_CLK(threadIdx.x == 0, 1);
    const Z2* __restrict__ Zc = ELLW ? ((jrel & 1) ? L.Z1 : L.Z0) : z_cur;
    Z2* __restrict__ Zn = (jrel & 1) ? L.Z0 : L.Z1;
    PipeRow pr;
    pr.clear();
    // ---- the first DEFER tiles: raw sums only ----
    double dst[DEFER], dsv[DEFER];
    Z2 dzr[DEFER];
#pragma unroll
    for (int i = 0; i < DEFER; ++i) {
        const int r = (bid + i * gtot) * GPB + g;
        pipe_row_sums<G, UNR, T, ELLW>(A, Zc, r, lane, wt >= 0 && r < A.n, dst[i], dsv[i], dzr[i]);
    }
    __syncthreads();     // the coefficients of wave 0 are in scoef
    PIPE_CLK(wt == 0, 4);
    const double alpha = scoef[0], beta = scoef[1], mu = scoef[2], inv = scoef[3];
    T* vj = L.V + (size_t)scoef[4] * (size_t)L.n;
#pragma unroll
    for (int i = 0; i < DEFER; ++i) {
        const int r = (bid + i * gtot) * GPB + g;
        if (wt >= 0 && r < A.n && lane == 0) pr.template finish<T>(alpha, beta, mu, inv, dzr[i], dst[i], dsv[i], vj, Zn, r, PSp, par);
    }
    // ---- remaining tiles ----
    for (int r0 = (bid + DEFER * gtot) * GPB; r0 < A.n; r0 += gtot * GPB) {
        const int r = r0 + g;
        const bool mine = wt >= 0 && r < A.n;
        double st, sv;
        Z2 zr;
        pipe_row_sums<G, UNR, T, ELLW>(A, Zc, r, lane, mine, st, sv, zr);
        if (mine && lane == 0) pr.template finish<T>(alpha, beta, mu, inv, zr, st, sv, vj, Zn, r, PSp, par);
    }
    PIPE_CLK(wt == 0, 5);
    pr.template store<BLOCK>(L, jrel, smw, PSp);
    if (SH) peer_drain();          // (every wave's deliveries -- its rows' records -- are acknowledged before the wave ends)
    PIPE_CLK(wt == 0, 6);
}

// Padded fixed-width copy of a short-row matrix (pose graphs beyond the single-workgroup kernel: city10000 has 3-13 entries
// per row): W slots per row in CSR order, the rest zero on the row's own column.
__global__ __launch_bounds__(kBlock) void k_ell_build(CsrView A, int W, int* __restrict__ ecol, double* __restrict__ eval) {
    const long tot = (long)A.n * W;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < tot; i += (long)gridDim.x * kBlock) {
        const int r = (int)(i / W), j = (int)(i - (long)r * W);
        const int b = A.rowptr[r], len = A.rowptr[r + 1] - b;
        ecol[i] = j < len ? A.col[b + j] : r;
        eval[i] = j < len ? A.val[b + j] : 0.0;
    }
}

// ---- LDS row-tile ("CSR-stream") form ------------------------------------------------------------
constexpr int kPipeTile = 1024;   // staged products per LDS tile, x2 arrays (16 KB)

template <int TPR>
__global__ __launch_bounds__(kBlock) void k_pipe_stream(CsrView A, PipeView L, int jrel) {
    __shared__ double smw[kNP * kBlock];
    __shared__ double scoef[8];
    __shared__ double pt[kPipeTile], pv[kPipeTile];
    __shared__ int sptr[kBlock / TPR + 1];
    constexpr int R = kBlock / TPR;
    const int tid = threadIdx.x;
    const int row = tid / TPR, sub = tid % TPR;
    if (tid < 64) { int jdummy; (void)pipe_prologue_wave0(L, jrel, -1, scoef, &jdummy, -1, true, (int)gridDim.x - 1); }
    const Z2* __restrict__ Zc = (jrel & 1) ? L.Z1 : L.Z0;
    Z2* __restrict__ Zn = (jrel & 1) ? L.Z0 : L.Z1;
    PipeRow pr;
    pr.clear();
    double alpha = 0.0, beta = 0.0, mu = 0.0, inv = 0.0;
    double* vj = nullptr;
    for (int tile = blockIdx.x; tile * R < A.n; tile += gridDim.x) {
        const int r0 = tile * R;
        const int nr = min(R, A.n - r0);
        for (int i = tid; i <= nr; i += kBlock) sptr[i] = A.rowptr[r0 + i];   // nr + 1 offsets (TPR = 1: 257 > 256 threads)
        Z2 zr; zr.t = 0.0; zr.v = 0.0;
        if (row < nr && sub == 0) zr = Zc[r0 + row];
        __syncthreads();
        if (!vj) {   // coefficients from wave 0 (published before the barrier above)
            alpha = scoef[0]; beta = scoef[1]; mu = scoef[2]; inv = scoef[3];
            vj = L.V + (size_t)scoef[4] * (size_t)L.n;
        }
        const int q0 = sptr[0], q1 = sptr[nr];
        double st = 0.0, sv = 0.0;
        for (int base = q0; base < q1; base += kPipeTile) {
            const int cnt = min(kPipeTile, q1 - base);
            for (int i = tid; i < cnt; i += kBlock) {     // perfectly coalesced val/col stream
                const double vv = A.val[base + i];
                const Z2 z = Zc[A.col[base + i]];
                pt[i] = vv * z.t; pv[i] = vv * z.v;
            }
            __syncthreads();
            if (row < nr) {
                const int lo = max(sptr[row], base), hi = min(sptr[row + 1], base + cnt);
                for (int q = lo + sub; q < hi; q += TPR) { st += pt[q - base]; sv += pv[q - base]; }
            }
            __syncthreads();
        }
        st = group_sum<TPR>(st); sv = group_sum<TPR>(sv);
        if (row < nr && sub == 0) pr.finish<double>(alpha, beta, mu, inv, zr, st, sv, vj, Zn, r0 + row);
    }
    pr.template store<kBlock>(L, jrel, smw);
}

// Start a sequence from u0: Z0 = (u0, 0); partials such that step 0 normalises u0.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pipe_init(PipeViewT<T> L, const double* __restrict__ u0, int epoch) {
    __shared__ double sm[4];
    double s1 = 0.0, s2 = 0.0;
    for (int r = blockIdx.x * kBlock + threadIdx.x; r < L.n; r += gridDim.x * kBlock) {
        ZRec<T> o; o.t = (T)u0[r]; o.v = 0;
        const double t = o.t;
        L.Z0[r] = o;
        s1 += t; s2 += t * t;
    }
    s1 = block_sum(s1, sm); s2 = block_sum(s2, sm);
    if (threadIdx.x == 0) {
        for (int q = 0; q < kNP; ++q) L.part[q * kMaxGrid + blockIdx.x] = 0.0;
        L.part[0 * kMaxGrid + blockIdx.x] = s2;
        L.part[3 * kMaxGrid + blockIdx.x] = s1;
        if (blockIdx.x == 0) { L.st->jA = 0; L.st->jN = 0; L.st->epoch = epoch; }
    }
}
// One wave, end of a chunk of `adv` steps: finish (alpha_{J-1}, beta_J, l1_{J-1}) for J = jA + adv
// so the host can test convergence, and advance the chunk base jA.  The step kernels only read
// jA; this kernel is alone in its launch.  Zero-copy hand-off to the host: records [J-adv-1, J]
// of tri -> pinned host memory, then the flag.
template <typename T>
__global__ __launch_bounds__(64) void k_pipe_tail(PipeViewT<T> L, int adv) {
    __shared__ double scoef[8];
    int j = 0;
    const PipeCoef c = pipe_prologue_wave0(L, adv, adv, scoef, &j);
    pipe_publish(L, c, j, adv);
}

// Partial sums (sum, sum of squares, sum of abs) of a vector -> part_u layout.
__global__ __launch_bounds__(kBlock) void k_vec_sums(const double* __restrict__ u, int n,
                                                     double* __restrict__ part) {
    __shared__ double sm[4];
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int r = blockIdx.x * kBlock + threadIdx.x; r < n; r += gridDim.x * kBlock) {
        const double t = u[r];
        s1 += t; s2 += t * t; s3 += fabs(t);
    }
    s1 = block_sum(s1, sm); s2 = block_sum(s2, sm); s3 = block_sum(s3, sm);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s1;
        part[kMaxGrid + blockIdx.x] = s2;
        part[2 * kMaxGrid + blockIdx.x] = s3;
    }
}

// fp64 -> fp32 copy of the assembled values (mixed-precision mode, once per solve).
__global__ __launch_bounds__(kBlock) void k_to_f32(const double* __restrict__ src, float* __restrict__ dst, long cnt) {
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < cnt; i += (long)gridDim.x * kBlock) dst[i] = (float)src[i];
}

__global__ void k_set_state(LanState* st, int j) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { st->jA = j; st->jB = j; st->jN = j; }
}

// Deterministic pseudo-random start vector in (-1,1) (splitmix64 of the index).
__global__ __launch_bounds__(kBlock) void k_fill_start(double* __restrict__ u, int n, unsigned long long seed) {
    for (int r = blockIdx.x * kBlock + threadIdx.x; r < n; r += gridDim.x * kBlock) {
        unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(r + 1);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z = z ^ (z >> 31);
        u[r] = (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
    }
}

// Ritz vector y = V[:, 0:J) s, split over the Krylov dimension: grid (row tiles, KS); slice ks
// accumulates columns ks, ks+KS, ... into ypart[ks*n + r].
// Rows a rank owns in a row-partitioned step (PeerSet): row tile t = r / gpb is handled by global workgroup t mod gtot.
struct RowOwner {
    int gpb = 1, gtot = 0, g0 = 0, g1 = 0;      // gtot = 0: every row
    __device__ __forceinline__ bool mine(int r) const {
        if (gtot == 0) return true;
        const int g = (r / gpb) % gtot;
        return g >= g0 && g < g1;
    }
};

template <typename T>
__global__ __launch_bounds__(kBlock) void k_ritz_partial(const T* __restrict__ V, int n, int J,
                                                         const double* __restrict__ s,
                                                         double* __restrict__ ypart, RowOwner own = RowOwner()) {
    const int KS = gridDim.y, ks = blockIdx.y;
    constexpr int U = 8;   // columns in flight per thread: the basis columns are n*8 bytes apart, so
                           // every load is a fresh DRAM page / TLB entry -- keep many outstanding
    for (int r = blockIdx.x * kBlock + threadIdx.x; r < n; r += gridDim.x * kBlock) {
        if (!own.mine(r)) continue;             // (sharded basis: the other rows live on other ranks)
        double acc = 0.0;
        for (int k0 = ks; k0 < J; k0 += U * KS) {
            double v[U], c[U];
#pragma unroll
            for (int q = 0; q < U; ++q) {
                const int k = k0 + q * KS;
                const bool ok = k < J;
                v[q] = ok ? (double)V[(size_t)k * n + r] : 0.0;
                c[q] = ok ? s[k] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < U; ++q) acc += v[q] * c[q];
        }
        ypart[(size_t)ks * n + r] = acc;
    }
}
// y = sum over the KS slices, plus the (sum, sum^2, sum|.|) partials of y.
__global__ __launch_bounds__(kBlock) void k_ritz_combine(const double* __restrict__ ypart, int n, int KS,
                                                         double* __restrict__ y, double* __restrict__ part) {
    __shared__ double sm[4];
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int r = blockIdx.x * kBlock + threadIdx.x; r < n; r += gridDim.x * kBlock) {
        double t = 0.0;
        for (int ks = 0; ks < KS; ++ks) t += ypart[(size_t)ks * n + r];
        y[r] = t;
        s1 += t; s2 += t * t; s3 += fabs(t);
    }
    s1 = block_sum(s1, sm); s2 = block_sum(s2, sm); s3 = block_sum(s3, sm);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s1;
        part[kMaxGrid + blockIdx.x] = s2;
        part[2 * kMaxGrid + blockIdx.x] = s3;
    }
}

// Sharded basis: a rank adds the KS slices of ITS rows and writes them into the leader's vector (same order of additions
// as k_ritz_combine; the leader then takes the sums of the complete vector with k_vec_sums, the same row -> workgroup
// mapping k_ritz_combine uses: bit-identical to the unsharded path).
__global__ __launch_bounds__(kBlock) void k_ritz_own_rows(const double* __restrict__ ypart, int n, int KS,
                                                          double* __restrict__ y_leader, RowOwner own, PeerVecs all = PeerVecs()) {
    for (int r = blockIdx.x * kBlock + threadIdx.x; r < n; r += gridDim.x * kBlock) {
        if (!own.mine(r)) continue;
        double t = 0.0;
        for (int ks = 0; ks < KS; ++ks) t += ypart[(size_t)ks * n + r];
        if (all.n) { for (int q = 0; q < all.n; ++q) peer_store(all.v[q] + r, t); }      // (ranks in different processes: every rank's copy)
        else y_leader[r] = t;
    }
    if (all.n) peer_drain();
}

// ||w - rq * v||_1 partials, rq = sum of the alpha partials (the Rayleigh quotient v.Lv of the
// unit vector v): the reference's convergence test numerator (nx:246).
__global__ __launch_bounds__(kBlock) void k_resid_l1(const double* __restrict__ w, const double* __restrict__ v,
                                                     int n, const double* __restrict__ part_a, int P_a,
                                                     double* __restrict__ part_out, double* __restrict__ rq_out,
                                                     double* __restrict__ rq_host = nullptr, double* __restrict__ q4_out = nullptr) {
    __shared__ double sm[4];
    const double rq = reduce_partials(part_a, P_a, sm);
    double s = 0.0, q4 = 0.0;
    for (int r = blockIdx.x * kBlock + threadIdx.x; r < n; r += gridDim.x * kBlock) {
        const double vr = v[r];
        s += fabs(w[r] - rq * vr);
        q4 += (vr * vr) * (vr * vr);       // sum v^4 of the unit vector: 1 / (its participation ratio) -- how localised the pair is (solver_lanczos.h, landscape gate)
    }
    s = block_sum(s, sm);
    q4 = block_sum(q4, sm);
    if (threadIdx.x == 0) {
        part_out[blockIdx.x] = s;
        if (q4_out) q4_out[blockIdx.x] = q4;
        if (blockIdx.x == 0) { *rq_out = rq; if (rq_host) *rq_host = rq; }
    }
}

// ------------------------------------------------------------------------------------------
// Top-k LP oracle (solve_subset_box_lp, mac/optimization/constraints.py:12-22): radix select
// of the k-th largest g on order-preserving 64-bit keys, 6 digit passes (11,11,11,11,11,9 bits),
// LDS histograms flushed with integer atomics; the last workgroup to finish a pass scans the
// 2048 bins and publishes (prefix, remaining rank) for the next pass.
// ------------------------------------------------------------------------------------------
struct SelState {
    unsigned long long prefix;   // selected high bits so far (right-aligned)
    long long kk;                // rank still to find inside the selected bucket (1-based, from the top)
    long long cnt_eq;            // after the last pass: number of keys == T
    unsigned long long T;        // after the last pass: the k-th largest key
    long long tie_limit;         // ties with index <= tie_limit are selected
    unsigned int ticket[8];
    long long k;                 // requested k
};

__device__ __forceinline__ unsigned long long f64_key(double d) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

constexpr int kBins = 2048;
constexpr int kSelRep = 16;        // replicas of the first digit's histogram when k_grad<true> counts it (hist + 6 kBins ...)

__device__ __forceinline__ int sel_shift(int pass) { return pass < 5 ? 53 - 11 * pass : 0; }
__device__ __forceinline__ int sel_bits(int pass) { return pass < 5 ? 11 : 9; }

// ------------------------------------------------------------------------------------------
// Supergradient  g_k = (w_k (v_i - v_j)) (v_i - v_j)   (mac/solvers/mac.py:117-124; same
// operation order, no fused multiply-add, so it is bit-exact with the reference given v)
// HIST (round 5): the first digit pass of the top-K select rides along -- g_k is in a register here, its top 11 key bits go
// into an LDS histogram that is flushed into hist[0 .. kBins) (zeroed by k_sel_init in front of this launch): one 8 m-byte
// pass over g and one launch less per Frank-Wolfe iteration.  Single rank only (a sharded gradient sees its own range).
// ------------------------------------------------------------------------------------------
template <bool HIST>
__global__ __launch_bounds__(kBlock) void k_grad(const int* __restrict__ ci, const int* __restrict__ cj,
                                                 const double* __restrict__ cw, const double* __restrict__ v,
                                                 long lo, long hi, double* __restrict__ g, PeerVecs all = PeerVecs(),
                                                 unsigned int* __restrict__ hist0 = nullptr) {
#pragma clang fp contract(off)   // plain operators under 'contract off': every op rounds once
    __shared__ unsigned int lh[HIST ? kBins : 1];
    if (HIST) {
        for (int i = threadIdx.x; i < kBins; i += kBlock) lh[i] = 0;
        __syncthreads();
    }
    unsigned int cur = 0xffffffffu, run = 0;
    for (long k = lo + (long)blockIdx.x * kBlock + threadIdx.x; k < hi; k += (long)gridDim.x * kBlock) {
        const double d = v[ci[k]] - v[cj[k]];
        const double t = cw[k] * d;
        const double gk = t * d;
        if (all.n) { for (int q = 0; q < all.n; ++q) peer_store(all.v[q] + k, gk); }   // (IPC communicator: the shard goes into every rank's gradient)
        else g[k] = gk;
        if (HIST) {
            const unsigned int bin = (unsigned int)(f64_key(gk) >> sel_shift(0));
            if (bin == cur) ++run;
            else { if (run) atomicAdd(&lh[cur], run); cur = bin; run = 1; }
        }
    }
    if (HIST) {
        if (run) atomicAdd(&lh[cur], run);
        __syncthreads();
        // (performed before the next launch reads them: the kernel boundary orders.  kSelRep replicas of the histogram: a gradient's
        // first digit lands in two or three bins, and 4 096 workgroups adding to the same words serialise at the memory side --
        // 33 us of a 54 us launch when first measured)
        unsigned int* hr = hist0 + (size_t)(blockIdx.x % kSelRep) * kBins;
        for (int i = threadIdx.x; i < kBins; i += kBlock)
            if (lh[i]) atomicAdd(&hr[i], lh[i]);
    }
    if (all.n) peer_drain();
}

// The scan that closes a digit pass (one workgroup of BLOCK threads): walk the bins from the top until the cumulative count reaches
// the rank still to find, publish (prefix, remaining rank) for the next pass -- or the finished threshold.
template <int BLOCK, class LoadBin>
__device__ __forceinline__ void sel_close_pass(LoadBin load_bin, int pass, unsigned long long prefix, SelState* st,
                                               unsigned int* s_w /* BLOCK / 64 words of LDS */) {
    const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
    const int sh = sel_shift(pass), nb = sel_bits(pass);
    const long long kk = pass ? st->kk : st->k;
    const int nbins = 1 << nb;
    constexpr int per = kBins / BLOCK;   // bins per thread, thread 0 owns the TOP bins
    unsigned int c[per];
    unsigned int tsum = 0;
#pragma unroll
    for (int q = 0; q < per; ++q) {
        const int bin = nbins - 1 - (tid * per + q);
        c[q] = bin >= 0 ? load_bin(bin) : 0u;
        tsum += c[q];
    }
    unsigned int x = tsum;                               // inclusive scan over the BLOCK per-thread sums (counts fit 32 bits)
    for (int o = 1; o < 64; o <<= 1) { const unsigned int y = __shfl_up(x, o, kWave); if (ln >= o) x += y; }
    __syncthreads();
    if (ln == 63) s_w[wv] = x;
    __syncthreads();
    for (int q = 0; q < wv; ++q) x += s_w[q];
    const long long pre = (long long)x;
    if (pre >= kk && pre - (long long)tsum < kk) {      // exactly one thread owns the kk-th key
        long long rem = kk - (pre - (long long)tsum);
        int q = 0;
        for (; q < per; ++q) {
            if ((long long)c[q] >= rem) break;
            rem -= c[q];
        }
        const int bin = nbins - 1 - (tid * per + q);
        st->kk = rem;
        st->prefix = (prefix << nb) | (unsigned long long)bin;
        if (pass == 5) {
            st->T = (prefix << nb) | (unsigned long long)bin;
            st->cnt_eq = (long long)c[q];
        } else if ((long long)c[q] == rem) {   // the whole bucket is selected: T = its lowest key, every "tie" counts
            st->T = ((prefix << nb) | (unsigned long long)bin) << sh;
            st->cnt_eq = rem;
            st->ticket[7] = 1u;
        }
    }
}

// Closes digit pass 0 when its histogram came from somewhere else (k_grad<true>: the supergradient kernel counts the first digit).
__global__ __launch_bounds__(1024) void k_sel_close0(unsigned int* __restrict__ hist, SelState* st) {
    __shared__ unsigned int s_w[1024 / 64];
    if (st->k <= 0) return;
    const unsigned int* rep = hist + 6 * kBins;                 // kSelRep replicas filled by k_grad<true> (complete: kernel boundary)
    sel_close_pass<1024>([rep](int bin) {
        unsigned int v[kSelRep];
#pragma unroll
        for (int r = 0; r < kSelRep; ++r) v[r] = rep[(size_t)r * kBins + bin];       // (plain loads, all in flight: written by the previous launch)
        unsigned int a = 0;
#pragma unroll
        for (int r = 0; r < kSelRep; ++r) a += v[r];
        return a; }, 0, 0ull, st, s_w);
}

// U keys per thread and round, their loads issued together: with one key per round a thread's 30 keys at 2 M candidates
// were 30 dependent memory round trips (21 us for a 16 MB pass; round 3: U = 4).  Round 5: what a pass over a dense digit costs
// is the FLUSH -- every workgroup adds its ~2 000 non-empty bins to the global histogram with returning device-scope atomics,
// 512 workgroups = a million atomics = 17 us -- so the workgroups are few and large (BLOCK = 1 024 threads on one LDS histogram).
template <int U, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_sel_pass(const double* __restrict__ g, long m, int pass,
                                                    unsigned int* __restrict__ hist /*[6][kBins]*/,
                                                    SelState* st) {
    __shared__ unsigned int lh[kBins];
    __shared__ unsigned int s_last;
    __shared__ unsigned int s_w[BLOCK / 64];
    const int tid = threadIdx.x;
    // an earlier pass found a bucket that is needed completely: the remaining digits cannot change the
    // selected set (ticket[7] is that pass's "done" mark; typical after 3 of the 6 passes on a gradient)
    if (pass && st->ticket[7]) return;
    for (int i = tid; i < kBins; i += BLOCK) lh[i] = 0;
    __syncthreads();
    const int sh = sel_shift(pass), nb = sel_bits(pass);
    const unsigned long long prefix = pass ? st->prefix : 0ull;
    const unsigned int mask = (1u << nb) - 1u;
    // the high digits of a gradient vector fall into a handful of bins: count runs of equal
    // digits in registers and touch the LDS histogram once per run, not once per key
    unsigned int cur = 0xffffffffu, run = 0;
    for (long i0 = (long)blockIdx.x * (BLOCK * U) + tid; i0 < m; i0 += (long)gridDim.x * (BLOCK * U)) {
        double gv[U];
#pragma unroll
        for (int q = 0; q < U; ++q) { const long i = i0 + (long)q * BLOCK; gv[q] = g[i < m ? i : m - 1]; }
#pragma unroll
        for (int q = 0; q < U; ++q) {
            if (i0 + (long)q * BLOCK >= m) continue;
            const unsigned long long key = f64_key(gv[q]);
            const bool match = pass == 0 || (key >> (sh + nb)) == prefix;
            if (match) {
                const unsigned int bin = (unsigned int)(key >> sh) & mask;
                if (bin == cur) ++run;
                else {
                    if (run) atomicAdd(&lh[cur], run);
                    cur = bin; run = 1;
                }
            }
        }
    }
    if (run) atomicAdd(&lh[cur], run);
    __syncthreads();
    unsigned int* gh = hist + pass * kBins;
    // The histogram lives in device-scope atomics (performed at the coherence point, never cached) and
    // is read back below with device-scope atomic loads, so no cache write-back / invalidate is needed.
    // The adds must have been PERFORMED before this workgroup takes its arrival ticket: they are issued
    // as returning atomics and the returned values are consumed, which forces the wave to wait for the
    // memory side's answer.  (Fire-and-forget adds followed by s_waitcnt vmcnt(0) were not enough: with
    // hundreds of workgroups adding to the same one or two bins -- round_nearest keys are mostly ties --
    // the last workgroup occasionally read a bin before every add had landed, and the selection came
    // out a few elements too large.  Found by tools/round_check.py.)
    unsigned int seen = 0;
    for (int i = tid; i < kBins; i += BLOCK)
        if (lh[i]) seen |= __hip_atomic_fetch_add(&gh[i], lh[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("" ::"v"(seen));
    __syncthreads();
    if (tid == 0)
        s_last = (__hip_atomic_fetch_add(&st->ticket[pass], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1);
    __syncthreads();
    if (!s_last) return;
    // last workgroup: walk the bins from the top until the cumulative count reaches kk
    sel_close_pass<BLOCK>([gh](int bin) { return __hip_atomic_load(&gh[bin], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }, pass, prefix, st, s_w);
}

// Ties at the k-th value: select the lowest indices.  One workgroup; exits at once in the
// common case (every key equal to T is needed).
// prefer_high = 0: ties with index <= tie_limit are selected (lowest indices first);
// prefer_high = 1: ties with index >= tie_limit (highest indices first; matches the stable
// lexsort order the rounding oracle uses).
__global__ __launch_bounds__(1024) void k_sel_ties(const double* __restrict__ g, long m, SelState* st, int prefer_high) {
    __shared__ int s_cnt[16];
    __shared__ long long s_found;
    const long long need = st->kk;        // ties to take (>= 1 when k >= 1)
    const long long eq = st->cnt_eq;
    if (st->k <= 0) { if (threadIdx.x == 0) st->tie_limit = prefer_high ? 0x7fffffffffffffffll : -1; return; }
    if (need >= eq) { if (threadIdx.x == 0) st->tie_limit = prefer_high ? -1 : 0x7fffffffffffffffll; return; }
    const unsigned long long T = st->T;
    const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
    if (tid == 0) s_found = -1;
    long long run = 0;
    for (long base = 0; base < m; base += 1024) {
        const long ii = base + tid;                         // position in scan order
        const long i = prefer_high ? m - 1 - ii : ii;       // element index
        const bool is = ii < m && f64_key(g[i]) == T;
        const unsigned long long bal = __ballot(is);
        __syncthreads();
        if (ln == 0) s_cnt[wv] = __popcll(bal);
        __syncthreads();
        int before = 0, tot = 0;
        for (int q = 0; q < 16; ++q) { if (q < wv) before += s_cnt[q]; tot += s_cnt[q]; }
        if (run + tot >= need) {
            const int rank = before + __popcll(bal & ((1ull << ln) - 1ull));   // 0-based among ties here
            if (is && run + rank + 1 == need) s_found = i;
            __syncthreads();
            if (tid == 0) st->tie_limit = s_found;
            return;
        }
        run += tot;
    }
    if (tid == 0) st->tie_limit = prefer_high ? -1 : 0x7fffffffffffffffll;
}

// The whole select (state reset, digit passes, tie rule) in ONE single-workgroup launch for short key vectors (pose graphs:
// 785 ... 10 688 candidates), where k_sel_init + six k_sel_pass + k_sel_ties are eight launches of 1-8 us with nothing to do.
// Same digit walk, same early exit, same tie rule: the SelState it leaves is identical to the multi-launch form's.
constexpr long kSelSmallMax = 32768;
__global__ __launch_bounds__(1024) void k_sel_small(const double* __restrict__ g, long m, long long k, SelState* st, int prefer_high) {
    __shared__ unsigned int lh[kBins];
    __shared__ unsigned int s_w[16];
    __shared__ unsigned long long s_prefix, s_T;
    __shared__ long long s_kk, s_eq, s_found;
    __shared__ int s_done, s_cnt[16];
    const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
    if (tid == 0) { s_prefix = 0; s_T = 0; s_kk = k; s_eq = 0; s_done = 0; s_found = -1; }
    __syncthreads();
    for (int pass = 0; pass < 6 && k > 0; ++pass) {
        if (s_done) break;                                   // (workgroup-uniform: read behind a barrier)
        for (int i = tid; i < kBins; i += 1024) lh[i] = 0;
        __syncthreads();
        const int sh = sel_shift(pass), nb = sel_bits(pass);
        const unsigned long long prefix = s_prefix;
        const unsigned int mask = (1u << nb) - 1u;
        unsigned int cur = 0xffffffffu, run = 0;
        for (long i = tid; i < m; i += 1024) {
            const unsigned long long key = f64_key(g[i]);
            if (pass == 0 || (key >> (sh + nb)) == prefix) {
                const unsigned int bin = (unsigned int)(key >> sh) & mask;
                if (bin == cur) ++run;
                else { if (run) atomicAdd(&lh[cur], run); cur = bin; run = 1; }
            }
        }
        if (run) atomicAdd(&lh[cur], run);
        __syncthreads();
        // walk the bins from the top until the cumulative count reaches kk: two bins per thread, thread 0 owns the top ones
        const long long kk = s_kk;
        const int nbins = 1 << nb;
        unsigned int c[2], tsum = 0;
        for (int q = 0; q < 2; ++q) { const int bin = nbins - 1 - (tid * 2 + q); c[q] = bin >= 0 ? lh[bin] : 0u; tsum += c[q]; }
        unsigned int x = tsum;                               // inclusive scan over the 1 024 per-thread sums
        for (int o = 1; o < 64; o <<= 1) { const unsigned int y = __shfl_up(x, o, kWave); if (ln >= o) x += y; }
        if (ln == 63) s_w[wv] = x;
        __syncthreads();
        for (int q = 0; q < wv; ++q) x += s_w[q];
        const long long pre = (long long)x;
        if (pre >= kk && pre - (long long)tsum < kk) {       // exactly one thread owns the kk-th key
            long long rem = kk - (pre - (long long)tsum);
            int q = 0;
            for (; q < 2; ++q) { if ((long long)c[q] >= rem) break; rem -= c[q]; }
            const int bin = nbins - 1 - (tid * 2 + q);
            s_kk = rem;
            s_prefix = (prefix << nb) | (unsigned long long)bin;
            if (pass == 5) { s_T = (prefix << nb) | (unsigned long long)bin; s_eq = (long long)c[q]; }
            else if ((long long)c[q] == rem) { s_T = ((prefix << nb) | (unsigned long long)bin) << sh; s_eq = rem; s_done = 1; }
        }
        __syncthreads();
    }
    const long long need = s_kk, eq = s_eq;
    const unsigned long long T = s_T;
    if (tid == 0) {
        st->prefix = s_prefix; st->kk = need; st->cnt_eq = eq; st->T = T; st->k = k;
        for (int i = 0; i < 7; ++i) st->ticket[i] = 0;
        st->ticket[7] = (unsigned int)s_done;
    }
    // ---- tie rule (k_sel_ties) ----
    if (k <= 0) { if (tid == 0) st->tie_limit = prefer_high ? 0x7fffffffffffffffll : -1; return; }
    if (need >= eq) { if (tid == 0) st->tie_limit = prefer_high ? -1 : 0x7fffffffffffffffll; return; }
    long long runs = 0;
    for (long base = 0; base < m; base += 1024) {
        const long ii = base + tid;
        const long i = prefer_high ? m - 1 - ii : ii;
        const bool is = ii < m && f64_key(g[i]) == T;
        const unsigned long long bal = __ballot(is);
        __syncthreads();
        if (ln == 0) s_cnt[wv] = __popcll(bal);
        __syncthreads();
        int before = 0, tot = 0;
        for (int q = 0; q < 16; ++q) { if (q < wv) before += s_cnt[q]; tot += s_cnt[q]; }
        if (runs + tot >= need) {
            const int rank = before + __popcll(bal & ((1ull << ln) - 1ull));
            if (is && runs + rank + 1 == need) s_found = i;
            __syncthreads();
            if (tid == 0) st->tie_limit = s_found;
            return;
        }
        runs += tot;
    }
    if (tid == 0) st->tie_limit = prefer_high ? -1 : 0x7fffffffffffffffll;
}

// Final fused Frank-Wolfe pass (mac/optimization/frankwolfe.py:59-76): s from the threshold,
// partials of g.(s - x) and g.g, x_next = x + gamma (s - x) (same rounding as NumPy: no fma).
__global__ __launch_bounds__(kBlock) void k_fw_final(const double* __restrict__ g, const double* __restrict__ x,
                                                     long m, const SelState* __restrict__ st, double gamma,
                                                     double* __restrict__ x_next, double* __restrict__ s_out,
                                                     double* __restrict__ part /*[2][kMaxGrid]*/,
                                                     double tol = 0.0, unsigned long long* __restrict__ xbits_next = nullptr) {
#pragma clang fp contract(off)   // x + gamma*(s - x) must round twice, like NumPy (no fma)
    __shared__ double sm[4];
    const unsigned long long T = st->T;
    const long long lim = st->tie_limit;
    const bool none = st->k <= 0;
    double d = 0.0, q = 0.0;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < m; i += (long)gridDim.x * kBlock) {
        const double gi = g[i];
        const unsigned long long key = f64_key(gi);
        const double s = (!none && (key > T || (key == T && (long long)i <= lim))) ? 1.0 : 0.0;
        if (s_out) s_out[i] = s;
        if (x) {
            const double xi = x[i];
            const double diff = s - xi;
            d += gi * diff;
            q += gi * gi;
            if (x_next) {
                const double step = gamma * diff;   // two roundings (contract off above)
                const double xn = xi + step;
                x_next[i] = xn;
                if (xbits_next) {                   // support bitmap of the next iterate (k_x_bits' rule; a wave = 64 aligned candidates)
                    const unsigned long long bal = __ballot(xn > tol);
                    if ((threadIdx.x & 63) == 0) xbits_next[i >> 6] = bal;
                }
            }
        }
    }
    d = block_sum(d, sm);
    q = block_sum(q, sm);
    if (threadIdx.x == 0) { part[blockIdx.x] = d; part[kMaxGrid + blockIdx.x] = q; }
}

// ------------------------------------------------------------------------------------------
// round_nearest with tie-break (mac/utils/rounding.py:30-42), SURVEY section 8(f) rank 2:
// top-k under the lexicographic key (round(w, decimals), edge weight).
// ------------------------------------------------------------------------------------------
// r = rint(x * f) / f  -- exactly NumPy's ndarray.round(decimals) for decimals > 0
__global__ __launch_bounds__(kBlock) void k_round_keys(const double* __restrict__ x, long m, double f,
                                                       double* __restrict__ r) {
#pragma clang fp contract(off)
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < m; i += (long)gridDim.x * kBlock) {
        const double t = x[i] * f;
        r[i] = rint(t) / f;
    }
}
// second-level keys: the edge weight where the rounded value ties with the k-th one, -inf elsewhere
__global__ __launch_bounds__(kBlock) void k_tie_keys(const double* __restrict__ r, const double* __restrict__ cw,
                                                     long m, const SelState* __restrict__ st1,
                                                     double* __restrict__ keys2) {
    const unsigned long long T = st1->T;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < m; i += (long)gridDim.x * kBlock)
        keys2[i] = f64_key(r[i]) == T ? cw[i] : -__builtin_huge_val();
}
// out = 1 where r > T1, or r == T1 and (no second level: index rule of st1 | second level: weight
// > T2, or == T2 with index >= st2.tie_limit)
__global__ __launch_bounds__(kBlock) void k_round_mark(const double* __restrict__ r, const double* __restrict__ keys2,
                                                       long m, const SelState* __restrict__ st1,
                                                       const SelState* __restrict__ st2, int two_level,
                                                       double* __restrict__ out) {
    const unsigned long long T1 = st1->T;
    const bool none = st1->k <= 0;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < m; i += (long)gridDim.x * kBlock) {
        const unsigned long long k1 = f64_key(r[i]);
        bool sel = false;
        if (!none) {
            if (k1 > T1) sel = true;
            else if (k1 == T1) {
                if (!two_level) sel = (long long)i >= st1->tie_limit;
                else {
                    const unsigned long long k2 = f64_key(keys2[i]);
                    sel = k2 > st2->T || (k2 == st2->T && (long long)i >= st2->tie_limit);
                }
            }
        }
        out[i] = sel ? 1.0 : 0.0;
    }
}

// ------------------------------------------------------------------------------------------
// Stream microbenchmarks (machip_membench; SURVEY section 8(d): "confirm the peak on the box and report both"):
// a read-only sum and the STREAM triad a = b + s c over arrays far larger than the 256 MB Infinity Cache.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_mb_read(const double2* __restrict__ a, long cnt2, double* __restrict__ out) {
    double s0 = 0.0, s1 = 0.0;
    const long stride = (long)gridDim.x * kBlock;
    long i = (long)blockIdx.x * kBlock + threadIdx.x;
    for (; i + 3 * stride < cnt2; i += 4 * stride) {      // four 16-byte loads in flight per lane
        const double2 x0 = a[i], x1 = a[i + stride], x2 = a[i + 2 * stride], x3 = a[i + 3 * stride];
        s0 += (x0.x + x1.x) + (x2.x + x3.x); s1 += (x0.y + x1.y) + (x2.y + x3.y);
    }
    for (; i < cnt2; i += stride) { const double2 x = a[i]; s0 += x.x; s1 += x.y; }
    if (s0 + s1 == 1.2345e301) out[0] = s0;               // (never true: keeps the loads alive)
}
__global__ __launch_bounds__(kBlock) void k_mb_triad(double2* __restrict__ a, const double2* __restrict__ b,
                                                      const double2* __restrict__ c, double s, long cnt2) {
    const long stride = (long)gridDim.x * kBlock;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < cnt2; i += stride) {
        const double2 x = b[i], y = c[i];
        a[i] = make_double2(x.x + s * y.x, x.y + s * y.y);
    }
}

__global__ void k_sel_init(SelState* st, long long k, unsigned int* __restrict__ hist = nullptr, int nhist = 0) {
    for (int i = threadIdx.x; i < nhist; i += blockDim.x) hist[i] = 0u;      // (was a separate fill kernel per select)
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        st->prefix = 0; st->kk = k; st->cnt_eq = 0; st->T = 0; st->tie_limit = -1; st->k = k;
        for (int i = 0; i < 8; ++i) st->ticket[i] = 0;
    }
}

// The select's launch sequence, the one place it is written: the k-th largest of keys[0..m), 0 <= k <= m, into *st (threshold,
// remaining rank, tie rule).  small_ok: short key vectors take the one-launch form (hist may then be null).  hist0_done: the
// first digit's histogram has been counted by the producer of the keys (k_grad<true>) behind a k_sel_init.
inline int sel_launch(hipStream_t stream, const double* keys, long m, long k, SelState* st, unsigned int* hist, int prefer_high,
                      bool small_ok, bool hist0_done) {
    if (m <= kSelSmallMax && small_ok) {      // short key vectors: the whole select in one launch
        k_sel_small<<<1, 1024, 0, stream>>>(keys, m, (long long)k, st, prefer_high);
        HIP_TRY(hipGetLastError());
        return MACHIP_OK;
    }
    if (!hist0_done) k_sel_init<<<1, 1024, 0, stream>>>(st, (long long)k, hist, 6 * kBins);
    if (k > 0) {
        // few, large workgroups: a dense digit costs one returning device-scope atomic per non-empty bin and workgroup (above)
        // (measured at configs[3], 16 MB of keys: 512 x 256 threads 17 us per dense pass, 128 x 1 024 threads 10 us)
        constexpr int B = 1024, U = 4;
        const int grid = (int)std::max<long>(1, std::min<long>(128, (m + (long)B * U - 1) / ((long)B * U)));
        if (hist0_done) k_sel_close0<<<1, 1024, 0, stream>>>(hist, st);
        for (int pass = hist0_done ? 1 : 0; pass < 6; ++pass) k_sel_pass<U, B><<<grid, B, 0, stream>>>(keys, m, pass, hist, st);
    }
    k_sel_ties<<<1, 1024, 0, stream>>>(keys, m, st, prefer_high);
    HIP_TRY(hipGetLastError());
    return MACHIP_OK;
}

}  // namespace machip
