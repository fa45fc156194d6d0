// solver_pairs_lob.h -- the deflated columns of machip_lowest_pairs, preconditioned (option pairs_precond = 1).
//
// Column c >= 1 runs the block-size-1 LOBPCG of solver_lob.h in the complement of the locked block Q = [1/sqrt(n), v_0 .. v_{c-1}]
// (columns 0 .. c of pairs->Q), preconditioned exactly as the Fiedler solve is: the same chain factor, the same Woodbury correction,
// the same Rayleigh-Ritz and update kernels, the same host loop (Solver::lob_iterate).  What is new per iteration is ONE step between
// the preconditioner and the product:
//     w <- w - Q (Q^T w)            in place, in wT's chunk-transposed layout
// so that L w is the true product of the projected w (no algebraic correction by the locked eigenvalues: the locked columns carry
// residuals up to tol ||L||, which would enter L x).  The constant vector is Q's column 0: the mean algebra of lob_rayleigh_ritz sees
// S w ~ 0 and stays as it is.  x itself is projected (twice) only before an explicit check, on the true L, and only a passing check
// accepts a column.
//   k_lobq_proj1<C>   n <= 16 384: one workgroup of 1 024 threads, thread t owns the C unknowns k_tri_solve<C> gives it, in registers;
//                     the nq dot products per thread, wave totals of the slots in use only (pairs_used), 16 waves added in wave order
//                     through LDS, w - Q h written back.  Q is read from QT, a chunk-transposed copy (one column copy per locked
//                     column, k_lobq_col): every load coalesces.  One launch per iteration.
//   k_lobq_dots       n > 16 384: per-workgroup partials, workgroup-major (k_pairs_dots' layout and reduction), at most kPairsGrid
//   k_lobq_apply      workgroups; every workgroup of the second launch adds the partials in the same fixed order.
// No floating-point atomics anywhere: two runs return the same bits.
#pragma once

namespace machip {

struct LobQ {
    int nq;
    size_t cap;                // entries per column of QT (L.c * L.stride: zero padded past n, as wT is)
    const double* QT;
    double* part;              // kPairsGrid x kPairsMaxLock (the two-launch form)
};

// column `src` (natural order) -> chunk-transposed; the padding of dst stays zero
__global__ __launch_bounds__(kBlock) void k_lobq_col(const double* __restrict__ src, int n, int c, int stride, double* __restrict__ dst) {
    for (int e = blockIdx.x * kBlock + threadIdx.x; e < n; e += gridDim.x * kBlock) dst[tri_perm(e, c, stride)] = src[e];
}

template <int CMAX>
__global__ __launch_bounds__(kTriThreads) void k_lobq_proj1(LobView L, LobQ Q) {
    __shared__ double red[(kTriThreads / 64) * kPairsMaxLock];
    __shared__ double sh[kPairsMaxLock];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    double w[CMAX], acc[kPairsMaxLock];
#pragma unroll
    for (int i = 0; i < CMAX; ++i) w[i] = L.wT[i * kTriThreads + t];      // (CMAX == L.c, stride == kTriThreads: always in bounds)
#pragma unroll
    for (int q = 0; q < kPairsMaxLock; ++q) {
        acc[q] = 0.0;
        if (q < Q.nq) {
            const double* __restrict__ col = Q.QT + (size_t)q * Q.cap;
#pragma unroll
            for (int i = 0; i < CMAX; ++i) acc[q] += col[i * kTriThreads + t] * w[i];
        }
    }
#pragma unroll
    for (int q = 0; q < kPairsMaxLock; ++q) {
        const double v = pairs_used<1>(q, Q.nq) ? wave_total(acc[q]) : 0.0;
        if (lane == 0) red[wv * kPairsMaxLock + q] = v;
    }
    __syncthreads();
    if (t < kPairsMaxLock) {
        double h = 0.0;
#pragma unroll
        for (int k = 0; k < kTriThreads / 64; ++k) h += red[k * kPairsMaxLock + t];
        sh[t] = h;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kPairsMaxLock; ++q)
        if (q < Q.nq) {
            const double* __restrict__ col = Q.QT + (size_t)q * Q.cap;
            const double h = sh[q];
#pragma unroll
            for (int i = 0; i < CMAX; ++i) w[i] -= h * col[i * kTriThreads + t];
        }
#pragma unroll
    for (int i = 0; i < CMAX; ++i) L.wT[i * kTriThreads + t] = w[i];
}

__global__ __launch_bounds__(kBlock) void k_lobq_dots(LobView L, LobQ Q) {
    __shared__ double red[4 * kPairsMaxLock];
    double acc[kPairsMaxLock];
#pragma unroll
    for (int i = 0; i < kPairsMaxLock; ++i) acc[i] = 0.0;
    for (size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x; k < Q.cap; k += (size_t)gridDim.x * kBlock) {
        const double wk = L.wT[k];
#pragma unroll
        for (int i = 0; i < kPairsMaxLock; ++i)
            if (i < Q.nq) acc[i] += Q.QT[(size_t)i * Q.cap + k] * wk;
    }
    pairs_block_out<kPairsMaxLock, 1>(acc, red, Q.part + (size_t)blockIdx.x * kPairsMaxLock, Q.nq);
}

__global__ __launch_bounds__(kBlock) void k_lobq_apply(LobView L, LobQ Q, int P) {
    __shared__ double sh[kPairsMaxLock];
    for (int q = threadIdx.x >> 6; q < Q.nq; q += kBlock / 64) {      // every workgroup: the same partials in the same order
        const double a = pairs_wave_partials(Q.part + q, P, kPairsMaxLock);
        if ((threadIdx.x & 63) == 0) sh[q] = a;
    }
    __syncthreads();
    for (size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x; k < Q.cap; k += (size_t)gridDim.x * kBlock) {
        double wk = L.wT[k];
#pragma unroll 4
        for (int i = 0; i < Q.nq; ++i) wk -= sh[i] * Q.QT[(size_t)i * Q.cap + k];
        L.wT[k] = wk;
    }
}

// w <- w - Q (Q^T w) against the first nq locked columns, between the preconditioner and the product of an iteration
inline void Solver::lobq_project(const LobView& L, int nq) {
    PairsBuf& B = *pairs;
    LobQ Q{nq, (size_t)L.c * (size_t)L.stride, B.QT, B.qpart};
    if (n <= kTriMaxN) {
        with_lob_chunk(L.c, [&](auto C) { k_lobq_proj1<SV(C)><<<1, kTriThreads, 0, stream>>>(L, Q); });
        return;
    }
    const int g = (int)std::max<size_t>(1, std::min<size_t>(kPairsGrid, (Q.cap + kBlock - 1) / kBlock));
    k_lobq_dots<<<g, kBlock, 0, stream>>>(L, Q);
    k_lobq_apply<<<g, kBlock, 0, stream>>>(L, Q, g);
}

// column `col` of pairs->Q into QT (once per locked column)
inline void Solver::lobq_lock(const LobView& L, int col) {
    PairsBuf& B = *pairs;
    const size_t cap = (size_t)L.c * (size_t)L.stride;
    const int g = (int)std::max<long>(1, std::min<long>(kPairsGrid, ((long)n + kBlock - 1) / kBlock));
    k_lobq_col<<<g, kBlock, 0, stream>>>(B.Q + (size_t)col * n, n, L.c, L.stride, B.QT + (size_t)col * cap);
}

inline bool Solver::pairs_lob_eligible() const { return chain_like && precision == 0 && !throughput_lane && n <= kTriBigMaxN; }

// The preconditioner of the call's deflated columns, once: what column 0's solve left when it ran mode 6 / 7 on this matrix (reuse),
// built as solve_lob builds it otherwise.  MACHIP_NOT_CONVERGED: there is none (T or the capacitance matrix not positive definite) --
// the columns run the deflated Lanczos.  timed: the build's device time goes to pairs->build_ms (between columns only: evs0 / evs1
// bracket the running column otherwise).
inline int Solver::pairs_lob_prepare(const CsrView& A, long nnz, double lnorm, LobPrep* P, bool reuse, bool timed) {
    PairsBuf& B = *pairs;
    if (reuse) {
        P->pl = plan_spmv(opt, n, nnz, kAuto);
        P->L = lview(P->pl);
        P->AT = A;
        P->AT.col = lx_colT;
        P->may_escalate = wb_active.s == 0 && OPT(woodbury, 1) != 0 && support_hint > wb_limit_now && support_hint <= wb_hard();
    } else {
        if (timed) (void)hipEventRecord(evs0, stream);
        const int st = lob_prepare(A, nnz, lnorm, P);
        if (st != MACHIP_OK) return st;
        int hbad = 0;
        HIP_TRY(hipMemcpyAsync(&hbad, lx_bad, sizeof(int), hipMemcpyDeviceToHost, stream));
        float ms = 0.f;
        if (timed && hipEventRecord(evs1, stream) == hipSuccess && hipEventSynchronize(evs1) == hipSuccess && hipEventElapsedTime(&ms, evs0, evs1) == hipSuccess)
            B.build_ms = ms;
        HIP_TRY(hipStreamSynchronize(stream));
        if (hbad) return MACHIP_NOT_CONVERGED;
    }
    const size_t cap = (size_t)P->L.c * (size_t)P->L.stride;
    if (!B.QT) {
        ST_TRY(dev_alloc(&B.QT, cap * kPairsMaxLock));
        HIP_TRY(hipMemsetAsync(B.QT, 0, sizeof(double) * cap * kPairsMaxLock, stream));      // (the padding past n is never written again)
        ST_TRY(dev_alloc(&B.qpart, (size_t)kPairsGrid * kPairsMaxLock));
    }
    return MACHIP_OK;
}

// Column c of machip_lowest_pairs, c >= 1, preconditioned.  On return out->status says whether a check passed; when none did, the last
// explicitly checked vector is in yvec (out->lam finite) and the caller finishes the column with the deflated Lanczos.
inline int Solver::pairs_column_lob(const CsrView& A, long nnz, double lnorm, double tol, int max_steps, int c, LobPrep* P, PairsCol* out) {
    PairsBuf& B = *pairs;
    const int nq = c + 1, g2 = vgrid();
    const double scale = lnorm > 0 ? lnorm : 1.0;
    *out = PairsCol();
    for (int i = B.qt_cols; i < nq; ++i) lobq_lock(P->L, i);
    B.qt_cols = nq;
    // the start vector: projected twice, normalised, checked -- a warm block passes here
    HIP_TRY(hipMemcpyAsync(y_raw, B.xs + (size_t)c * n, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream));
    pairs_project(y_raw, nq, 2);
    pairs_project(y_raw, nq, 2);
    k_vec_sums<<<g2, kBlock, 0, stream>>>(y_raw, n, part_c);
    HIP_TRY(hipGetLastError());
    double rq = 0.0, r1 = 0.0;
    ST_TRY(check_vector(A, P->pl, &rq, &r1));
    out->method = wb_active.s > 0 ? 7 : 6;
    out->lam = rq;
    if (!(rq == rq)) return MACHIP_OK;      // (a start vector inside span Q: the Lanczos route says so)
    out->res = r1 / scale;
    if (out->res < tol) { out->status = MACHIP_OK; return MACHIP_OK; }
    double lam = rq, res = out->res;
    long iters = 0, spmvs = 0, rst = 0;
    int st = lob_iterate(A, *P, lnorm, tol, max_steps, nq, r1, &lam, &res, &iters, &spmvs, &rst);
    if (st == MACHIP_NOT_CONVERGED && lob_escalate && lam == lam && iters < max_steps) {
        // the tridiagonal preconditioner crawls and the exact one is affordable: build it (for the remaining columns too) and go on
        // from the last checked vector -- yvec, w2 and rq_dev are that check's
        const long it1 = iters, rst1 = rst;
        wb_limit_now = wb_hard();
        const int sp = pairs_lob_prepare(A, nnz, lnorm, P, false, false);      // (inside the column's own time)
        if (sp != MACHIP_OK && sp != MACHIP_NOT_CONVERGED) return sp;
        if (sp == MACHIP_OK) {
            out->method = wb_active.s > 0 ? 7 : 6;
            st = lob_iterate(A, *P, lnorm, tol, max_steps - (int)it1, nq, res * scale, &lam, &res, &iters, &spmvs, &rst);
            iters += it1; rst += rst1;
        } else B.lob_off = true;
    }
    out->steps = (int)iters; out->restarts = (int)rst; out->lam = lam; out->res = res;
    if (st == MACHIP_OK) out->status = MACHIP_OK;
    else if (st != MACHIP_NOT_CONVERGED) return st;
    return MACHIP_OK;
}

}  // namespace machip
