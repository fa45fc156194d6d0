// solver_pairs.h -- the q lowest non-trivial eigenpairs of L by sequential deflation with locking (machip_lowest_pairs; DESIGN
// section 24).  Column 0 is the handle's own Fiedler solve (mac.h lowest_pairs calls run_fiedler); this file is everything after it:
// the kernels of the deflated Lanczos step and the driver of columns c = 1 .. q-1.
//
// Column c runs a plain three-term recurrence on L in the complement of the locked block Q = [1/sqrt(n), v_0 .. v_{c-1}].  Two
// launches per step, nothing normalised before its norm is known -- the basis keeps the UN-normalised u_j, every consumer scales by
// 1/||u_j||:
//   k_pairs_mul   t = L v_j (v_j = u_j / beta_j, beta_j from the previous launch's partials), in the row forms plan_spmv chooses;
//                 per workgroup the partial sums of t.v_j, q_i.t and q_i.v_j for the <= 16 locked columns
//   k_pairs_fin   alpha = t.v_j, h = Q^T (t - alpha v_j - beta_j v_{j-1}) from those sums (Q^T v_{j-1}: kept from the step before),
//                 u_{j+1} = t - alpha v_j - beta_j v_{j-1} - Q h  -> basis column j+1, the record (alpha_j, beta_j, ||u_j||_1), and
//                 the partials of ||u_{j+1}||^2 and ||u_{j+1}||_1 summed from u_{j+1} ITSELF (not from the expansion
//                 t.t - alpha^2 - ...: near convergence that is a difference of O(||L||^2) terms for a value of O(beta^2))
// It is the NEW vector that is projected, not L v_j alone: what v_j and v_{j-1} carry of Q is rounding noise, but the recurrence
// multiplies it by ~alpha/beta per step (the constant vector came back after 80 steps on er300_x0 when only t was projected).
// Every reduction goes through per-workgroup partials (workgroup-major: one workgroup's sums are contiguous) that every consumer
// adds up in the same fixed order; no floating-point atomics: runs repeat bit for bit.
// The host looks at the records a chunk of kPairsChunk steps at a time (no streamed records, no forecasts): smallest Ritz pair of
// T_J (tridiag.h), estimate |s_{J-1}| ||u_J||_1 of the residual's 1-norm; the Ritz vector is accepted by the explicit check on
// the true L only (Solver::check_vector).
#pragma once

namespace machip {

constexpr int kPairsMaxLock = 16;                       // the constant vector + at most 15 accepted columns are projected out
constexpr int kPairsPM = 1 + 2 * kPairsMaxLock;         // k_pairs_mul's sums per workgroup: t.v | q_i.t | q_i.v
constexpr int kPairsChunk = 16;                         // steps between two looks at the records
constexpr int kPairsModeLanczos = 1;                    // machip_lowest_pairs_info: a column of the deflated Lanczos below
constexpr int kPairsModeFinished = 9;                   // ... of preconditioned iterations (solver_pairs_lob.h) finished by it
constexpr int kPairsGrid = 256;                        // most workgroups of the vector kernels (every consumer re-reads one partial each)

struct PairsBuf {
    double *Q = nullptr;       // n x 17: the constant vector, then the accepted columns in the order they were found
    double *t = nullptr;       // L v_j
    double *xs = nullptr;      // n x 16: the start block
    double *pm = nullptr;      // kMaxGrid x kPairsPM: k_pairs_mul / k_pairs_dots partials
    double *pf = nullptr;      // 3 slots x 2 x kMaxGrid: k_pairs_fin partials (sum u^2 | sum |u|) of even steps, odd steps, projections
    double *gq = nullptr;      // 2 x 16: Q^T v_j of even / odd steps
    double *rec = nullptr;     // 3 per step: alpha_j, beta_j = ||u_j||_2, ||u_j||_1
    size_t rec_cap = 0;
    double last_ms[kPairsMaxLock] = {};      // device time per column of the last call, by rank (machip_lowest_pairs_time)
    int last_q = 0;
    // the preconditioned route (solver_pairs_lob.h; option pairs_precond)
    double *QT = nullptr;      // the locked columns in the tridiagonal solver's chunk-transposed layout, 16 x (c x stride)
    double *qpart = nullptr;   // kPairsGrid x 16: k_lobq_dots partials
    int qt_cols = 0;           // columns of QT that hold this call's locked block
    bool lob_off = false;      // this call has no preconditioner (not positive definite numerically): its columns run Lanczos
    int last_method[kPairsMaxLock] = {};     // by rank: the mode that produced each column of the last call (machip_lowest_pairs_info)
    int last_closures = 0;                   // closures of the exact preconditioner the deflated columns ran with (0: none did)
    double build_ms = 0.0;                   // device time of the one-off preconditioner build (0: column 0's was reused, or none)
};

// method: the solver mode that produced the column (solver.h last_mode; 1 deflated Lanczos, 6 / 7 preconditioned, 9 preconditioned
// iterations finished by Lanczos)
struct PairsCol { double lam = NAN, res = INFINITY, ms = 0.0; int steps = 0, restarts = 0, status = MACHIP_NOT_CONVERGED, method = 1; };

// every lane of the calling wave gets the sum of cnt partials, added in one fixed order
__device__ __forceinline__ double pairs_wave_partials(const double* part, int cnt, int stride = 1) {
    double a = 0.0;
    for (int i = threadIdx.x & 63; i < cnt; i += 64) a += part[(size_t)i * stride];
    return wave_total(a);
}
// slot q of k_pairs_mul's 33 sums is in use with nq locked columns (t.v | q_i.t | q_i.v, i < nq); OFF = 1: k_pairs_dots' 16 (q_i.x)
template <int OFF>
__device__ __forceinline__ bool pairs_used(int q, int nq) { return OFF ? q < nq : (q == 0 || ((q - 1) & (kPairsMaxLock - 1)) < nq); }
__device__ __forceinline__ double pairs_inv(double beta, double tiny) { return beta > tiny ? 1.0 / beta : 0.0; }
__device__ __forceinline__ double pairs_beta(double nrm2) { return nrm2 > 0.0 ? sqrt(nrm2) : 0.0; }

// N per-thread sums -> one per workgroup at dst[0 .. N) (red: 4 x N doubles of LDS); the slots not in use are written as zeros
// without being added up (with one locked column beside the constant vector that is 5 wave sums of 33)
template <int N, int OFF>
__device__ __forceinline__ void pairs_block_out(const double (&acc)[N], double* red, double* dst, int nq) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const double v = pairs_used<OFF>(q, nq) ? wave_total(acc[q]) : 0.0;
        if (lane == 0) red[w * N + q] = v;
    }
    __syncthreads();
    if (threadIdx.x < N) dst[threadIdx.x] = (red[threadIdx.x] + red[N + threadIdx.x]) + (red[2 * N + threadIdx.x] + red[3 * N + threadIdx.x]);
}

struct PairsMul {
    int n, nq, Pf;
    const double* Q;
    const double* uj;          // basis column j (the operand, un-normalised)
    double* t;
    double* pm;
    const double* pf;          // the partials k_pairs_fin left for column j
    double tiny;
};

struct OpPairs {
    PairsMul M;
    double inv;
    double acc[kPairsPM];
    __device__ __forceinline__ void begin(double*) {
        inv = pairs_inv(pairs_beta(pairs_wave_partials(M.pf, M.Pf)), M.tiny);
#pragma unroll
        for (int q = 0; q < kPairsPM; ++q) acc[q] = 0.0;
    }
    __device__ __forceinline__ double gather(const double* __restrict__ x, int c) const { return x[c]; }
    __device__ __forceinline__ void row(int r, double a) {
        const double t = a * inv, v = M.uj[r] * inv;
        M.t[r] = t;
        acc[0] += t * v;
#pragma unroll
        for (int i = 0; i < kPairsMaxLock; ++i)
            if (i < M.nq) {
                const double qv = M.Q[(size_t)i * M.n + r];
                acc[1 + i] += qv * t;
                acc[1 + kPairsMaxLock + i] += qv * v;
            }
    }
    __device__ __forceinline__ void end(double* red) { pairs_block_out<kPairsPM, 0>(acc, red, M.pm + (size_t)blockIdx.x * kPairsPM, M.nq); }
};

template <bool STREAM, int W>
__global__ __launch_bounds__(kBlock) void k_pairs_mul(CsrView A, PairsMul M) {
    __shared__ double red[4 * kPairsPM];
    OpPairs op;
    op.M = M;
    op.begin(red);
    if constexpr (STREAM) {
        __shared__ double prod[kStreamTile];
        __shared__ int sptr[kBlock / W + 1];
        spmv_rows_stream<W>(A, M.uj, op, prod, sptr);
    } else {
        spmv_rows_vec<W>(A, M.uj, op);
    }
    op.end(red);
}

inline void launch_pairs_mul(const SpmvPlan& pl, hipStream_t s, const CsrView& A, const PairsMul& M) {
    if (pl.variant == kStream) with_stream_width(pl.width, [&](auto W) { k_pairs_mul<true, SV(W)><<<pl.grid, kBlock, 0, s>>>(A, M); });
    else with_vec_width(pl.width, [&](auto W) { k_pairs_mul<false, SV(W)><<<pl.grid, kBlock, 0, s>>>(A, M); });
}

// Q^T x for a vector that is not a step's product (a start vector, a Ritz vector): partials in k_pairs_mul's layout (q_i.t slots)
__global__ __launch_bounds__(kBlock) void k_pairs_dots(const double* __restrict__ x, int n, const double* __restrict__ Q, int nq, double* __restrict__ pm) {
    __shared__ double red[4 * kPairsMaxLock];
    double acc[kPairsMaxLock];
#pragma unroll
    for (int i = 0; i < kPairsMaxLock; ++i) acc[i] = 0.0;
    for (int r = blockIdx.x * kBlock + threadIdx.x; r < n; r += gridDim.x * kBlock) {
        const double xr = x[r];
#pragma unroll
        for (int i = 0; i < kPairsMaxLock; ++i)
            if (i < nq) acc[i] += Q[(size_t)i * n + r] * xr;
    }
    pairs_block_out<kPairsMaxLock, 1>(acc, red, pm + (size_t)blockIdx.x * kPairsPM + 1, nq);
}

struct PairsFin {
    int n, nq, Pm, Pf, j;
    int step;                  // 1: a recurrence step; 0: a plain projection out = t - Q (Q^T t)
    const double* Q;
    const double* t;
    const double* uj;          // basis columns j and j - 1 (NULL at j = 0)
    const double* ujm1;
    double* out;               // basis column j + 1 (a projection: may be t itself)
    const double* pm;
    const double* pf_in;       // partials of u_j
    double* pf_out;            // partials of what this launch writes
    const double* g_in;        // Q^T v_{j-1} (NULL at j = 0)
    double* g_out;             // Q^T v_j
    double* rec;
    double tiny;
};

// VEC2: n is even, so every column of Q and of the basis starts on a 16-byte boundary: two rows per 16-byte load and store
template <bool VEC2>
__global__ __launch_bounds__(kBlock) void k_pairs_fin(PairsFin F) {
    __shared__ double sq[kPairsPM];
    __shared__ double sh[kPairsMaxLock];
    __shared__ double sm[4];
    const int w = threadIdx.x >> 6;
    for (int q = w; q < kPairsPM; q += 4) {      // the sums of this step that are in use, every workgroup in the same order
        if (!pairs_used<0>(q, F.nq) || (!F.step && (q == 0 || q > kPairsMaxLock))) continue;      // (a projection has the q_i.x slots only)
        const double a = pairs_wave_partials(F.pm + q, F.Pm, kPairsPM);
        if ((threadIdx.x & 63) == 0) sq[q] = a;
    }
    double alpha = 0.0, beta = 0.0, inv = 0.0, cb = 0.0;
    if (F.step) {
        beta = pairs_beta(pairs_wave_partials(F.pf_in, F.Pf));      // (the same expression k_pairs_mul scaled its operand by)
        inv = pairs_inv(beta, F.tiny);
        if (F.ujm1) cb = beta * pairs_inv(F.rec[3 * (F.j - 1) + 1], F.tiny);
    }
    __syncthreads();
    if (F.step) alpha = sq[0];
    if (threadIdx.x < kPairsMaxLock) {
        double h = 0.0;
        if ((int)threadIdx.x < F.nq) {
            h = sq[1 + threadIdx.x];
            if (F.step) h -= alpha * sq[1 + kPairsMaxLock + threadIdx.x] + (F.g_in ? beta * F.g_in[threadIdx.x] : 0.0);
        }
        sh[threadIdx.x] = h;
    }
    if (F.step && blockIdx.x == 0) {
        if ((int)threadIdx.x < F.nq) F.g_out[threadIdx.x] = sq[1 + kPairsMaxLock + threadIdx.x];
        if (w == 0) {
            const double l1 = pairs_wave_partials(F.pf_in + kMaxGrid, F.Pf);
            if (threadIdx.x == 0) { F.rec[3 * F.j] = alpha; F.rec[3 * F.j + 1] = beta; F.rec[3 * F.j + 2] = l1; }
        }
    }
    __syncthreads();
    const double ca = alpha * inv;
    double uu = 0.0, l1 = 0.0;
    if constexpr (VEC2) {
        const int n2 = F.n / 2;
        const double2* t2 = reinterpret_cast<const double2*>(F.t);
        const double2* a2 = reinterpret_cast<const double2*>(F.uj);
        const double2* b2 = reinterpret_cast<const double2*>(F.ujm1);
        double2* o2 = reinterpret_cast<double2*>(F.out);
        for (int k = blockIdx.x * kBlock + threadIdx.x; k < n2; k += gridDim.x * kBlock) {
            double2 u = t2[k];
            if (F.step) { const double2 a = a2[k]; u.x -= ca * a.x; u.y -= ca * a.y; }
            if (F.step && F.ujm1) { const double2 b = b2[k]; u.x -= cb * b.x; u.y -= cb * b.y; }
#pragma unroll 4
            for (int i = 0; i < F.nq; ++i) {
                const double2 qv = reinterpret_cast<const double2*>(F.Q + (size_t)i * F.n)[k];
                u.x -= sh[i] * qv.x; u.y -= sh[i] * qv.y;
            }
            o2[k] = u;
            uu += u.x * u.x + u.y * u.y;
            l1 += fabs(u.x) + fabs(u.y);
        }
    } else {
        for (int r = blockIdx.x * kBlock + threadIdx.x; r < F.n; r += gridDim.x * kBlock) {
            double u = F.t[r];
            if (F.step) u -= ca * F.uj[r];
            if (F.step && F.ujm1) u -= cb * F.ujm1[r];
#pragma unroll 4
            for (int i = 0; i < F.nq; ++i) u -= sh[i] * F.Q[(size_t)i * F.n + r];
            F.out[r] = u;
            uu += u * u;
            l1 += fabs(u);
        }
    }
    uu = block_sum(uu, sm);
    l1 = block_sum(l1, sm);
    if (threadIdx.x == 0) { F.pf_out[blockIdx.x] = uu; F.pf_out[kMaxGrid + blockIdx.x] = l1; }
}

// the record of the column a chunk ended on: beta_J and ||u_J||_1 are known only as partials until the next step runs
__global__ __launch_bounds__(64) void k_pairs_tail(const double* __restrict__ pf, int Pf, double* __restrict__ rec, int J) {
    const double uu = pairs_wave_partials(pf, Pf), l1 = pairs_wave_partials(pf + kMaxGrid, Pf);
    if (threadIdx.x == 0) { rec[3 * J] = 0.0; rec[3 * J + 1] = pairs_beta(uu); rec[3 * J + 2] = l1; }
}

__global__ __launch_bounds__(kBlock) void k_pairs_fill(double* __restrict__ x, int n, double v) {
    for (int r = blockIdx.x * kBlock + threadIdx.x; r < n; r += gridDim.x * kBlock) x[r] = v;
}

// ---- the driver ----

inline void Solver::pairs_free() {
    if (!pairs) return;
    void* b[] = {pairs->Q, pairs->t, pairs->xs, pairs->pm, pairs->pf, pairs->gq, pairs->rec, pairs->QT, pairs->qpart};
    for (void* q : b) if (q) (void)hipFree(q);
    delete pairs;
    pairs = nullptr;
}

inline int Solver::pairs_alloc() {
    if (pairs) return MACHIP_OK;
    pairs = new PairsBuf();
    PairsBuf& B = *pairs;
    auto body = [&]() -> int {
        ST_TRY(dev_alloc(&B.Q, (size_t)n * (kPairsMaxLock + 1) + 2)); ST_TRY(dev_alloc(&B.t, (size_t)n + 2));
        ST_TRY(dev_alloc(&B.xs, (size_t)n * kPairsMaxLock + 2));
        ST_TRY(dev_alloc(&B.pm, (size_t)kMaxGrid * kPairsPM)); ST_TRY(dev_alloc(&B.pf, 3 * 2 * kMaxGrid)); ST_TRY(dev_alloc(&B.gq, 2 * kPairsMaxLock));
        B.rec_cap = 3 * (vcap + 2);
        ST_TRY(dev_alloc(&B.rec, B.rec_cap));
        return MACHIP_OK;
    };
    const int st = body();
    if (st != MACHIP_OK) { const std::string keep = g_err; pairs_free(); g_err = keep; }      // (all of it or none: a later call allocates again)
    return st;
}

inline int Solver::pairs_fin_grid() const { return (int)std::max<long>(1, std::min<long>(kPairsGrid, (((long)n + 1) / 2 + kBlock - 1) / kBlock)); }

// x <- x - Q (Q^T x) against the first nq locked columns, in place; the sums of the result go to partial slot `slot`
inline void Solver::pairs_project(double* x, int nq, int slot) {
    PairsBuf& B = *pairs;
    const int gd = (int)std::max<long>(1, std::min<long>(kPairsGrid, ((long)n + kBlock - 1) / kBlock)), gf = pairs_fin_grid();
    k_pairs_dots<<<gd, kBlock, 0, stream>>>(x, n, B.Q, nq, B.pm);
    PairsFin F{};
    F.n = n; F.nq = nq; F.Pm = gd; F.Pf = gf; F.j = 0; F.step = 0; F.Q = B.Q; F.t = x; F.out = x; F.pm = B.pm;
    F.pf_in = B.pf; F.pf_out = B.pf + (size_t)slot * 2 * kMaxGrid; F.rec = B.rec; F.tiny = 0.0;
    if (n % 2 == 0) k_pairs_fin<true><<<gf, kBlock, 0, stream>>>(F);
    else k_pairs_fin<false><<<gf, kBlock, 0, stream>>>(F);
}

// Column c of machip_lowest_pairs, c >= 1: the locked block is columns [0, c] of pairs->Q, the start vector column c of pairs->xs.
// On return the last explicitly checked vector is in yvec (unit norm), whatever the status.
inline int Solver::pairs_column(const CsrView& A, long nnz, double lnorm, double tol, int max_steps, int c, int cap, PairsCol* out) {
    PairsBuf& B = *pairs;
    const SpmvPlan pl = plan_spmv(opt, n, nnz, kAuto);
    const int nq = c + 1, gf = pairs_fin_grid();
    const double tiny = std::max(1e-13 * lnorm, 1e-300);
    const int Jcap = std::max(1, std::min(cap - 1, n - 1 - c));      // steps one sequence can take: the basis, the complement's dimension
    const double* x = B.xs + (size_t)c * n;
    double slack = 0.25;      // the explicit check is tried once the estimate is below slack * tol * ||L||: what is locked is then well inside
                              // tol, and a later column sees little of its residual ("coupling")
    std::vector<double> hrec, a, b, wk2;
    tri::Smallest S;
    auto pf_slot = [&](int j) { return B.pf + (size_t)(j & 1) * 2 * kMaxGrid; };
    *out = PairsCol();
    for (;;) {      // one Krylov sequence
        if (out->steps >= max_steps) return MACHIP_OK;       // (status NOT_CONVERGED, the last check's figures)
        HIP_TRY(hipMemcpyAsync(V, x, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
        pairs_project(V, nq, 0);
        pairs_project(V, nq, 0);      // basis column 0 = the start vector, projected twice
        hrec.assign(3 * ((size_t)Jcap + 2), 0.0);
        int J = 0, scanned = 0;
        bool ended = false, accepted = false;
        while (!ended) {
            const int ch = std::min(kPairsChunk, std::min(Jcap - J, max_steps - out->steps));
            for (int j = J; j < J + ch; ++j) {
                double* uj = V + (size_t)j * n;
                PairsMul M{n, nq, gf, B.Q, uj, B.t, B.pm, pf_slot(j), tiny};
                launch_pairs_mul(pl, stream, A, M);
                PairsFin F{};
                F.n = n; F.nq = nq; F.Pm = pl.grid; F.Pf = gf; F.j = j; F.step = 1; F.Q = B.Q; F.t = B.t; F.uj = uj; F.ujm1 = j ? uj - n : nullptr;
                F.out = uj + n; F.pm = B.pm; F.pf_in = pf_slot(j); F.pf_out = pf_slot(j + 1);
                F.g_in = j ? B.gq + (size_t)((j - 1) & 1) * kPairsMaxLock : nullptr; F.g_out = B.gq + (size_t)(j & 1) * kPairsMaxLock;
                F.rec = B.rec; F.tiny = tiny;
                if (n % 2 == 0) k_pairs_fin<true><<<gf, kBlock, 0, stream>>>(F);
                else k_pairs_fin<false><<<gf, kBlock, 0, stream>>>(F);
            }
            const int Jn = J + ch;
            k_pairs_tail<<<1, 64, 0, stream>>>(pf_slot(Jn), gf, B.rec, Jn);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(hrec.data() + 3 * (size_t)J, B.rec + 3 * (size_t)J, sizeof(double) * 3 * (size_t)(ch + 1), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            out->steps += ch;
            if (!(hrec[1] > tiny) || !std::isfinite(hrec[1]))
                return fail(MACHIP_BAD_ARG, "machip_lowest_pairs: the start vector of column " + std::to_string(c) + " lies in the span of the constant vector and the columns before it, or is not finite");
            int Jeff = Jn;
            for (int jj = std::max(1, scanned + 1); jj <= Jn; ++jj)
                if (!(hrec[3 * (size_t)jj + 1] > tiny)) { Jeff = jj; ended = true; break; }       // breakdown: the Krylov space is invariant
            scanned = Jn;
            J = Jn;
            ended = ended || Jeff >= Jcap || out->steps >= max_steps;
            a.resize((size_t)Jeff); b.resize((size_t)Jeff + 1);
            for (int i = 0; i < Jeff; ++i) { a[(size_t)i] = hrec[3 * (size_t)i]; b[(size_t)i] = hrec[3 * (size_t)i + 1]; }
            tri::smallest_eigpair(a.data(), b.data(), Jeff, nullptr, 0, 0.0, S, wk2);
            const double est = std::fabs(S.s[(size_t)Jeff - 1]) * hrec[3 * (size_t)Jeff + 2];
            if (!ended && !(est < slack * tol * lnorm)) continue;
            // the Ritz vector from the un-normalised basis, projected twice, then the reference's rule on the true L
            for (int k = 0; k < Jeff; ++k) h_pin[k] = S.s[(size_t)k] / b[(size_t)k];
            HIP_TRY(hipMemcpyAsync(sdev, h_pin, sizeof(double) * (size_t)Jeff, hipMemcpyHostToDevice, stream));
            const int g2 = vgrid(), KS = std::max(1, std::min(ks_max, Jeff / 8));
            k_ritz_partial<<<dim3(g2, KS), kBlock, 0, stream>>>(V, n, Jeff, sdev, ypart);
            k_ritz_combine<<<g2, kBlock, 0, stream>>>(ypart, n, KS, y_raw, part_c);
            pairs_project(y_raw, nq, 2);
            pairs_project(y_raw, nq, 2);
            k_vec_sums<<<g2, kBlock, 0, stream>>>(y_raw, n, part_c);
            HIP_TRY(hipGetLastError());
            double rq = 0.0, res = 0.0;
            ST_TRY(check_vector(A, pl, &rq, &res));
            out->lam = rq; out->res = lnorm > 0.0 ? res / lnorm : res;
            if (res < tol * lnorm) { accepted = true; break; }
            if (!ended && res > 0.0 && est > 0.0) slack = std::min(slack, 0.5 * slack * est / res);      // the estimate was optimistic by res / est
        }
        if (accepted) { out->status = MACHIP_OK; return MACHIP_OK; }
        if (out->steps >= max_steps) return MACHIP_OK;
        x = yvec;                 // explicit restart from the sequence's Ritz vector
        ++out->restarts;
    }
}

// Columns 1 .. q-1 after the handle's own solve left column 0 in yvec.  X_dev: the start block is in pairs->xs already.  Results per column
// in `cols` (entry 0 is the caller's), the vectors in pairs->Q columns 1 .. q.  yvec and the participation ratio of the Fiedler solve are put
// back: the handle's next gradient, warm start or landscape gate sees what it would have seen without this call.
inline int Solver::pairs_rest(const CsrView& A, long nnz, double lnorm, double tol, int max_steps, int q, PairsCol* cols) {
    PairsBuf& B = *pairs;
    const int gd = (int)std::max<long>(1, std::min<long>(kPairsGrid, ((long)n + kBlock - 1) / kBlock));
    k_pairs_fill<<<gd, kBlock, 0, stream>>>(B.Q, n, 1.0 / std::sqrt((double)n));
    HIP_TRY(hipMemcpyAsync(B.Q + (size_t)n, yvec, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
    const double keep_pr = last_pr;
    std::function<void()> keep_hook;
    keep_hook.swap(after_check);
    int cap = (int)std::min<size_t>(vcap, B.rec_cap / 3 - 2);
    if (OPT(pairs_vcap, 0) > 0) cap = std::min(cap, OPT(pairs_vcap, 0));
    cap = std::max(cap, 4);
    const int steps_cap = max_steps > 0 ? max_steps : (int)std::min<long>(200000, std::max<long>(2000, 20l * n));
    // option pairs_precond: the columns run the preconditioned iteration of solver_pairs_lob.h where the handle is eligible; what that
    // touches of the handle beyond yvec and last_pr is put back as well
    const bool precond = OPT(pairs_precond, 0) != 0 && pairs_lob_eligible();
    const long keep_lob = hist_lob_iters, keep_exact = hist_exact_iters;
    const bool keep_prev = have_prev, keep_esc = lob_escalate;
    const int keep_limit = wb_limit_now;
    const WbView keep_wb = wb_active;
    LobPrep P;
    bool prepared = false;
    B.qt_cols = 0; B.lob_off = false; B.last_closures = 0; B.build_ms = 0.0;
    int st = MACHIP_OK;
    for (int c = 1; c < q && st == MACHIP_OK; ++c) {
        if (precond && !prepared && !B.lob_off) {      // once per call, before column 1
            const bool reuse = last_was_lob && (last_mode == 6 || last_mode == 7);
            if (!reuse) wb_limit_now = wb_soft();
            const int sp = pairs_lob_prepare(A, nnz, lnorm, &P, reuse, true);
            if (sp == MACHIP_OK) prepared = true;
            else if (sp == MACHIP_NOT_CONVERGED) B.lob_off = true;
            else { st = sp; break; }
        }
        (void)hipEventRecord(evs0, stream);
        if (precond && prepared && !B.lob_off) {
            st = pairs_column_lob(A, nnz, lnorm, tol, steps_cap, c, &P, &cols[c]);
            if (st == MACHIP_OK && cols[c].method == 7) B.last_closures = wb_active.s;
            if (st == MACHIP_OK && cols[c].status != MACHIP_OK) {
                // no check passed (breakdown, the iteration cap, patience): the deflated Lanczos finishes the column from the last
                // checked vector, as solve() finishes column 0; its steps are added to the column's count
                const PairsCol lob = cols[c];
                if (std::isfinite(lob.lam) && hipMemcpyAsync(B.xs + (size_t)c * n, yvec, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream) != hipSuccess)
                    st = fail(MACHIP_HIP_ERROR, "machip_lowest_pairs: copy of a checked vector failed");
                if (st == MACHIP_OK) st = pairs_column(A, nnz, lnorm, tol, std::max(0, steps_cap - lob.steps), c, cap, &cols[c]);
                if (cols[c].steps == 0 && std::isfinite(lob.lam)) { cols[c].lam = lob.lam; cols[c].res = lob.res; }      // (the cap left Lanczos no step: the last check's figures)
                cols[c].steps += lob.steps; cols[c].restarts += lob.restarts;
                cols[c].method = lob.steps > 0 ? kPairsModeFinished : kPairsModeLanczos;
            }
        } else st = pairs_column(A, nnz, lnorm, tol, steps_cap, c, cap, &cols[c]);
        float ms = 0.f;      // the column on the stream's clock: steps, the host's looks at the records between chunks, Ritz vectors and checks
        if (st == MACHIP_OK && hipEventRecord(evs1, stream) == hipSuccess && hipEventSynchronize(evs1) == hipSuccess &&
            hipEventElapsedTime(&ms, evs0, evs1) == hipSuccess) cols[c].ms = ms;
        if (st == MACHIP_OK) st = hipMemcpyAsync(B.Q + (size_t)(c + 1) * n, yvec, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream) == hipSuccess
                                      ? MACHIP_OK : fail(MACHIP_HIP_ERROR, "machip_lowest_pairs: copy of an accepted column failed");
    }
    hist_lob_iters = keep_lob; hist_exact_iters = keep_exact; have_prev = keep_prev; lob_escalate = keep_esc; wb_limit_now = keep_limit; wb_active = keep_wb;
    keep_hook.swap(after_check);
    last_pr = keep_pr;
    const std::string keep = g_err;
    HIP_TRY(hipMemcpyAsync(yvec, B.Q + (size_t)n, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    g_err = keep;
    return st;
}

// RandomState(7).normal(size=(q, n)).T, the reference's start block (mac/utils/fiedler.py:27-32) continued to q columns: MT19937
// seeded as numpy seeds it, 53-bit doubles, the polar method with its cached second draw -- column c is draws [c n, (c + 1) n).
struct RefBlock {
    uint32_t mt[624];
    int idx = 624;
    bool have = false;
    double saved = 0.0;
    explicit RefBlock(uint32_t seed) {
        mt[0] = seed;
        for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    }
    uint32_t next() {
        if (idx >= 624) {
            for (int i = 0; i < 624; ++i) {
                const uint32_t y = (mt[i] & 0x80000000u) | (mt[(i + 1) % 624] & 0x7fffffffu);
                mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            idx = 0;
        }
        uint32_t y = mt[idx++];
        y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
        return y;
    }
    double uniform() { const uint32_t a = next() >> 5, b = next() >> 6; return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0; }
    double normal() {
        if (have) { have = false; return saved; }
        double x1, x2, r2;
        do { x1 = 2.0 * uniform() - 1.0; x2 = 2.0 * uniform() - 1.0; r2 = x1 * x1 + x2 * x2; } while (r2 >= 1.0 || r2 == 0.0);
        const double f = std::sqrt(-2.0 * std::log(r2) / r2);
        saved = f * x1; have = true;
        return f * x2;
    }
};

}  // namespace machip
