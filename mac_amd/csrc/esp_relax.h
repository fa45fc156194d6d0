// mac_amd/csrc/esp_relax.h -- the convex relaxation of the k-edge tree-count problem (Khosoussi et al., arXiv:1604.01116) on
// the state of a machip_esp handle: Frank-Wolfe on the log tree count, with the dual bound every k-edge selection obeys.
//
// Node 0 pinned.  For x in [0, 1]^m, sum x <= k:
//     M(x) = L_red(fixed) + beta I + sum_e x_e w_e a_e a_e^T,   F(x) = log det M(x) - log det M(0),   dF/dx_e = w_e a_e^T M(x)^-1 a_e.
// F is concave, so F(x) + dF(x).(s - x), s the top-k vertex of dF(x), bounds F on the whole feasible set from above.
// Per evaluation, all on the handle's stream:
//   1. k_relax_assemble: the dense M(x) (identity beyond n') into the handle's working buffer.  Workgroup i owns row i: it
//      streams the row's zeros (16-byte stores), then the row's few non-zero entries, each the sum of its terms in one fixed
//      order by one thread (beta first, then the fixed edges in their order, then the candidates in index order) -- no
//      floating-point atomics; (i, j) and (j, i) sum the same terms in the same order, so M(x) is symmetric to the bit;
//   2. the blocked Gauss-Jordan inverse (esp.h: gj_inverse, k_gj_step<0, true>), ping-pong with a third ld x ld buffer that
//      the first relaxation call allocates -- Sigma0, the state of the greedy, stays where it is;
//   3. log det M(x) from that same elimination: the 32 scalar pivots of every 32 x 32 pivot block are its Schur complements,
//      the sum of their logs (block by block in ldet[], then reduced in a fixed order) is the log-determinant;
//   4. k_esp_scores(mask = 0) on the fresh inverse: the gradient;
//   5. the LP vertex: the top-k select of kernels.h (k_sel_small / k_sel_init + k_sel_pass + k_sel_ties; the tie rule of
//      machip_lp_topk: ties at the k-th value go to the lowest indices);
//   6. k_fw_final (partials of g.(s - x) and g.g, x_next = x + gamma (s - x)) and k_relax_scalars (F, dual, |g|).
// The host reads three scalars and the pivot flag per iteration (the stop tests), nothing else.
//
// On a MACHIP_ESP_EDGE_RELAX handle steps 1-4 are those of esp_relax_edge.h instead -- N(x) = I + G D in the candidates' space,
// its inverse and the gradient from it -- and steps 5-6, the reading of the scalars and the loop are the ones here.  On a
// MACHIP_ESP_EDGE_RELAX_TREE handle they are those of esp_relax_edge_tree.h: the same N(x) over the candidates and the seeds of a
// spanning tree, its Gram matrix stored, log det N(0) subtracted.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "esp.h"
#include "esp_relax_edge.h"
#include "esp_relax_edge_tree.h"
#include "kernels.h"

namespace machip {

struct EspRelax {
    double* bufC = nullptr;                  // the inverse's second buffer (the first is the handle's working copy `sig`)
    int *rowptr = nullptr, *ecol = nullptr, *tptr = nullptr, *tx = nullptr;     // incidence list by node (below)
    double* tw = nullptr;
    double *xa = nullptr, *xb = nullptr;     // iterate and next iterate
    double *part = nullptr, *ldet = nullptr, *scal = nullptr;
    SelState* st = nullptr;
    unsigned int* hist = nullptr;
    double logdet0 = 0.0;                    // log det M(0), by the same kernels in the same order (F(0) = 0 exactly)
    int ld = 0;                              // leading dimension of the matrix an evaluation inverts (node space: the handle's)
    EspEdge* ed = nullptr;                   // edge space (esp_relax_edge.h): N(x) instead of M(x); bufC .. tw above stay unused
    EspEdgeTree* et = nullptr;               // edge space over a spanning tree (esp_relax_edge_tree.h): likewise
};

// Row i of M(x): zeros, then entry q in [rowptr[i], rowptr[i + 1]) at column ecol[q] = sum over its terms t in
// [tptr[q], tptr[q + 1]) of tw[t] (tx[t] < 0: a fixed term) or tw[t] x[tx[t]].  grid = ld.
// One THREAD per entry, its terms added serially: that is the fixed order.  The diagonal of a node of degree d is a chain of
// d + 1 additions while the row's other threads idle -- pose graphs have degrees of a few tens at most and the whole assembly is
// 0.1 % of an iteration; a hub of thousands of edges would want a wave per entry with a fixed tree.
__global__ __launch_bounds__(kBlock) void k_relax_assemble(double* __restrict__ S, int ld, const int* __restrict__ rowptr,
                                                           const int* __restrict__ ecol, const int* __restrict__ tptr,
                                                           const double* __restrict__ tw, const int* __restrict__ tx,
                                                           const double* __restrict__ x) {
#pragma clang fp contract(off)   // every product and every sum rounds once: the order alone fixes the bits
    const int i = blockIdx.x;
    double* row = S + (size_t)i * ld;
    double2* row2 = reinterpret_cast<double2*>(row);         // (ld is a multiple of 64: rows are 512-byte aligned)
    for (int j = threadIdx.x; j < ld / 2; j += kBlock) row2[j] = make_double2(0.0, 0.0);
    __syncthreads();                                          // (the entries below overwrite zeros this workgroup wrote)
    for (int q = rowptr[i] + threadIdx.x; q < rowptr[i + 1]; q += kBlock) {
        double a = 0.0;
        for (int t = tptr[q]; t < tptr[q + 1]; ++t) {
            const int e = tx[t];
            const double w = tw[t];
            a += e < 0 ? w : w * x[e];
        }
        row[ecol[q]] = a;
    }
}

// a . b in the order k_fw_final sums g.(s - x): the same grid (min(1024, ceil(m / 256)) workgroups), per thread the products
// of its grid-stride elements added in index order (no fma), block_sum, one partial per workgroup; k_relax_scalars reduces them.
// machip_esp_relax_inner: a host driver that forms the dual value through it gets the bits machip_esp_relax_run gets.
__global__ __launch_bounds__(kBlock) void k_relax_inner(const double* __restrict__ a, const double* __restrict__ b, long m,
                                                        double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double sm[4];
    double d = 0.0;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < m; i += (long)gridDim.x * kBlock) d += a[i] * b[i];
    d = block_sum(d, sm);
    if (threadIdx.x == 0) { part[blockIdx.x] = d; part[kMaxGrid + blockIdx.x] = 0.0; }
}

// out[0] = F = sum(ldet) - logdet0, out[1] = F + g.(s - x), out[2] = |g|_2, out[3] = g.(s - x) from the partials of k_fw_final
// (np = 0: F only).  One workgroup, fixed order.
__global__ __launch_bounds__(kBlock) void k_relax_scalars(const double* __restrict__ ldet, int nblk, double logdet0,
                                                          const double* __restrict__ part, int np, double* __restrict__ out) {
    __shared__ double sm[4];
    const double ld = reduce_partials(ldet, nblk, sm);
    const double d = reduce_partials(part, np, sm);
    const double q = reduce_partials(part + kMaxGrid, np, sm);
    if (threadIdx.x == 0) {
        const double f = ld - logdet0;
        out[0] = f;
        out[1] = f + d;
        out[2] = sqrt(q);
        out[3] = d;
    }
}

inline void esp_relax_release(machip_esp* h) {
    EspRelax* r = h->rx;
    if (!r) return;
    void* bufs[] = {r->bufC, r->rowptr, r->ecol, r->tptr, r->tx, r->tw, r->xa, r->xb, r->part, r->ldet, r->scal, r->st, r->hist};
    for (void* q : bufs) if (q) (void)hipFree(q);
    esp_edge_release(r->ed);
    esp_edge_tree_release(r->et);
    delete r;
    h->rx = nullptr;
}

// The incidence list by node, from the edge lists the handle was made from.  Self-loops contribute nothing; node-0 terms drop out.
inline int esp_relax_build_lists(machip_esp* h, EspRelax* r) {
    struct Term { int64_t key; double w; int x; };
    const int np = h->np;
    const int64_t ld = h->ld;
    std::vector<Term> T;
    T.reserve((size_t)ld + 4 * (h->hfw.size() + h->hcw.size()));
    for (int i = 0; i < (int)ld; ++i) T.push_back({(int64_t)i * ld + i, i < np ? h->beta : 1.0, -1});
    auto add = [&](int a, int b, double w, int x) {      // reduced endpoints (-1 = node 0)
        if (a == b) return;
        if (a >= 0) T.push_back({(int64_t)a * ld + a, w, x});
        if (b >= 0) T.push_back({(int64_t)b * ld + b, w, x});
        if (a >= 0 && b >= 0) { T.push_back({(int64_t)a * ld + b, -w, x}); T.push_back({(int64_t)b * ld + a, -w, x}); }
    };
    for (size_t e = 0; e < h->hfw.size(); ++e) add(h->hfi[e] - 1, h->hfj[e] - 1, h->hfw[e], -1);
    for (size_t e = 0; e < h->hcw.size(); ++e) add(h->hci[e] - 1, h->hcj[e] - 1, h->hcw[e], (int)e);
    std::stable_sort(T.begin(), T.end(), [](const Term& a, const Term& b) { return a.key < b.key; });
    std::vector<int> rowptr((size_t)ld + 1, 0), ecol, tptr, tx(T.size());
    std::vector<double> tw(T.size());
    for (size_t t = 0; t < T.size(); ++t) {
        if (t == 0 || T[t].key != T[t - 1].key) {
            ecol.push_back((int)(T[t].key % ld));
            tptr.push_back((int)t);
            ++rowptr[(size_t)(T[t].key / ld) + 1];
        }
        tw[t] = T[t].w; tx[t] = T[t].x;
    }
    tptr.push_back((int)T.size());
    for (size_t i = 0; i < (size_t)ld; ++i) rowptr[i + 1] += rowptr[i];
    ST_TRY(dev_alloc(&r->rowptr, rowptr.size())); ST_TRY(dev_alloc(&r->ecol, ecol.size())); ST_TRY(dev_alloc(&r->tptr, tptr.size()));
    ST_TRY(dev_alloc(&r->tx, tx.size())); ST_TRY(dev_alloc(&r->tw, tw.size()));
    HIP_TRY(hipMemcpyAsync(r->rowptr, rowptr.data(), sizeof(int) * rowptr.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(r->ecol, ecol.data(), sizeof(int) * ecol.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(r->tptr, tptr.data(), sizeof(int) * tptr.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(r->tx, tx.data(), sizeof(int) * tx.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(r->tw, tw.data(), sizeof(double) * tw.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));          // (host staging goes out of scope)
    return MACHIP_OK;
}

// Steps 1-4 for the x in `x`: M(x) and its inverse in h->sig (the greedy's working copy: the last selection run's state is
// gone, Sigma0 is not touched), the blocks' log-determinants in ldet[], the gradient in h->s (want_grad).
inline int esp_relax_eval_on(machip_esp* h, const double* x, bool want_grad) {
    EspRelax* r = h->rx;
    if (r->ed) return esp_edge_eval_on(h, r->ed, x, r->ldet, want_grad);
    if (r->et) return esp_edge_tree_eval_on(h, r->et, x, r->ldet, want_grad);
    hipStream_t st = h->stream;
    h->live = false;
    h->pending = 0;
    HIP_TRY(hipMemsetAsync(h->bad, 0, sizeof(int), st));
    k_relax_assemble<<<h->ld, kBlock, 0, st>>>(h->sig, h->ld, r->rowptr, r->ecol, r->tptr, r->tw, r->tx, x);
    double *src = h->sig, *dst = r->bufC;
    h->gj_inverse<true>(src, dst, r->ldet);          // (ld / 32 is even: the inverse ends in h->sig)
    if (want_grad && h->m) k_esp_scores<<<h->grid_m(), kBlock, 0, st>>>(h->view(), src, 0);
    HIP_TRY(hipGetLastError());
    return MACHIP_OK;
}

// Step 5 on the gradient in h->s: the launch sequence of machip_lp_topk's select (machip.hip: select_on), into r->st.
inline int esp_relax_select(machip_esp* h, long k) {
    EspRelax* r = h->rx;
    const long m = h->m;
    if (m <= kSelSmallMax) {
        k_sel_small<<<1, 1024, 0, h->stream>>>(h->s, m, (long long)k, r->st, 0);
    } else {
        if (!r->hist) return fail(MACHIP_BAD_ARG, "the multi-launch select has no histogram on this handle (edge space allocates none: m <= 16384 must stay below kSelSmallMax)");
        constexpr int B = 1024, U = 4;
        const int grid = (int)std::max<long>(1, std::min<long>(128, (m + (long)B * U - 1) / ((long)B * U)));
        k_sel_init<<<1, 1024, 0, h->stream>>>(r->st, (long long)k, r->hist, 6 * kBins);
        for (int pass = 0; pass < 6; ++pass) k_sel_pass<U, B><<<grid, B, 0, h->stream>>>(h->s, m, pass, r->hist, r->st);
        k_sel_ties<<<1, 1024, 0, h->stream>>>(h->s, m, r->st, 0);
    }
    HIP_TRY(hipGetLastError());
    return MACHIP_OK;
}

// F (and the other two scalars when `np` partials of k_fw_final are there) to the host, with the pivot flag.
inline int esp_relax_read(machip_esp* h, int np, double* out3) {
    EspRelax* r = h->rx;
    int hbad = 0;
    k_relax_scalars<<<1, kBlock, 0, h->stream>>>(r->ldet, r->ld / kGjB, r->logdet0, r->part, np, r->scal);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out3, r->scal, sizeof(double) * 3, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&hbad, h->bad, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (hbad && (r->ed || r->et)) return fail(MACHIP_NOT_CONVERGED, "N(x) = I + G D has a non-positive Gauss-Jordan pivot (its leading minors are positive: lost numerically)");
    if (hbad) return fail(MACHIP_NOT_CONVERGED, "M(x) is not positive definite numerically (a non-positive Gauss-Jordan pivot)");
    return MACHIP_OK;
}

// The leading dimension an edge handle's relaxation inverts at, from the handle alone (node space: 0 -- machip_esp_relax_info's).
inline int esp_relax_ld(const machip_esp* h) {
    return h->edge_tree ? esp_edge_tree_ld((int64_t)h->m + h->tr->seeds) : h->edge_relax ? (std::max(h->m, 1) + kGjT - 1) / kGjT * kGjT : 0;
}

// the matrix an evaluation would invert is beyond the dense limit (the one statement of the three limits)
inline bool esp_relax_oversize(const machip_esp* h) {
    return h->edge_tree ? (int64_t)h->m + h->tr->seeds > kEspDenseMaxN : h->edge_relax ? h->m > kEspDenseMaxN : h->n > kEspDenseMaxN;
}

// What the relaxation cannot do on this handle, decided from the handle alone (nothing is allocated before it is asked).
inline int esp_relax_limits(const machip_esp* h) {
    if (h->edge_tree) {
        if (esp_relax_oversize(h))
            return fail(MACHIP_BAD_ARG, "MACHIP_ESP_EDGE_RELAX_TREE inverts the dense (m + r) x (m + r) N(x): candidates plus seeds must be <= 16384 (m = " +
                                            std::to_string((int64_t)h->m) + ", r = " + std::to_string((int64_t)h->tr->seeds) + ")");
        return MACHIP_OK;
    }
    if (h->edge_relax) {
        if (esp_relax_oversize(h))
            return fail(MACHIP_BAD_ARG, "MACHIP_ESP_EDGE_RELAX inverts the dense m x m N(x): the number of candidates must be <= 16384 (m = " +
                                            std::to_string(h->m) + ")");
        return MACHIP_OK;
    }
    if (h->form == kEspFormFree || h->tr)      // (tr: a MACHIP_ESP_MATRIX_FREE | MACHIP_ESP_SPANNING_TREE handle, esp_tree.h)
        return fail(MACHIP_BAD_ARG, "the relaxation inverts the dense M(x): not available on a MACHIP_ESP_MATRIX_FREE handle");
    if (esp_relax_oversize(h))
        return fail(MACHIP_BAD_ARG, "the relaxation inverts the dense M(x) (no chain closed form): num_nodes must be <= 16384");
    return MACHIP_OK;
}

// First relaxation call on a handle.  Node space: the third buffer, the incidence list, log det M(0).  Edge space: the state of
// esp_relax_edge.h (log det N(0) = log det I = 0: nothing to evaluate).  Edge space over a spanning tree: the state of
// esp_relax_edge_tree.h with its Gram matrix, and log det N(0) -- the seeds' -- by one evaluation at x = 0.
inline int esp_relax_prepare(machip_esp* h) {
    ST_TRY(esp_relax_limits(h));
    HIP_TRY(hipSetDevice(h->device));
    if (h->rx) return MACHIP_OK;
    EspRelax* r = new EspRelax();
    h->rx = r;
    auto body = [&]() -> int {
        if (h->edge_relax) {
            r->ed = new EspEdge();
            ST_TRY(esp_edge_prepare(h, r->ed));
        }
        if (h->edge_tree) {
            r->et = new EspEdgeTree();
            ST_TRY(esp_edge_tree_prepare(h, r->et));
        }
        r->ld = r->ed ? r->ed->ld : r->et ? r->et->ld : h->ld;
        const size_t ld = (size_t)r->ld, ms = (size_t)std::max(h->m, 1);
        if (!r->ed && !r->et) ST_TRY(dev_alloc(&r->bufC, ld * ld));
        ST_TRY(dev_alloc(&r->xa, ms)); ST_TRY(dev_alloc(&r->xb, ms));
        ST_TRY(dev_alloc(&r->part, (size_t)2 * kMaxGrid)); ST_TRY(dev_alloc(&r->ldet, ld / kGjB)); ST_TRY(dev_alloc(&r->scal, 4));
        ST_TRY(dev_alloc(&r->st, 1));
        if (r->ed) {                             // (m <= 16 384 is below kSelSmallMax: the multi-launch select's histogram is never used)
            // log det N(0) = 0 in every block: what k_relax_scalars sums when machip_esp_relax_inner is the handle's first call
            HIP_TRY(hipMemsetAsync(r->ldet, 0, sizeof(double) * (ld / kGjB), h->stream));
            return MACHIP_OK;
        }
        if (!r->et) {                            // (edge space over a tree: m <= 16 384 as above, no incidence list)
            ST_TRY(dev_alloc(&r->hist, (size_t)6 * kBins));
            ST_TRY(esp_relax_build_lists(h, r));
        }
        HIP_TRY(hipMemsetAsync(r->xa, 0, sizeof(double) * ms, h->stream));
        ST_TRY(esp_relax_eval_on(h, r->xa, false));
        double s3[3];
        ST_TRY(esp_relax_read(h, 0, s3));
        r->logdet0 = s3[0];
        return MACHIP_OK;
    };
    const int st = body();
    if (st != MACHIP_OK) esp_relax_release(h);
    return st;
}

inline int esp_relax_check_x(const machip_esp* h, const double* x) {
    if (h->m && !x) return fail(MACHIP_BAD_ARG, "x is NULL");
    for (int e = 0; e < h->m; ++e)
        if (!(x[e] >= 0.0 && x[e] <= 1.0))
            return fail(MACHIP_BAD_ARG, "x[" + std::to_string(e) + "] is not in [0, 1] (or not finite)");
    return MACHIP_OK;
}

// workgroups of k_fw_final and k_relax_inner over the m candidates: their partials are summed in this grid's order
inline int esp_relax_grid(const machip_esp* h) { return std::max(1, std::min(kMaxGrid, (h->m + kBlock - 1) / kBlock)); }

// machip_esp_relax_eval after its NULL checks: F(x), and the gradient when asked
inline int esp_relax_eval(machip_esp* h, const double* x, double* F_out, double* grad_out) {
    ST_TRY(esp_relax_check_x(h, x));
    ST_TRY(esp_relax_prepare(h));
    EspRelax* r = h->rx;
    if (h->m) HIP_TRY(hipMemcpyAsync(r->xa, x, sizeof(double) * (size_t)h->m, hipMemcpyHostToDevice, h->stream));
    ST_TRY(esp_relax_eval_on(h, r->xa, grad_out != nullptr));
    if (grad_out && h->m) HIP_TRY(hipMemcpyAsync(grad_out, h->s, sizeof(double) * (size_t)h->m, hipMemcpyDeviceToHost, h->stream));
    double s3[3];
    ST_TRY(esp_relax_read(h, 0, s3));
    *F_out = s3[0];
    return MACHIP_OK;
}

// machip_esp_relax_run after its NULL checks: Frank-Wolfe from x_inout, steps 1-6 and three scalars to the host per iteration
inline int esp_relax_run(machip_esp* h, int64_t k, int max_iters, double gap_tol, double grad_tol, double* x_inout, double* f_traj,
                         double* dual_traj, double* gnorm_traj, int* iters_out, double* upper_out) {
    if (esp_relax_oversize(h)) return esp_relax_prepare(h);      // (the limit's message, nothing allocated)
    if (k <= 0 || k > h->m) return fail(MACHIP_BAD_ARG, "k must be in [1, m] (m = " + std::to_string(h->m) + " candidates)");
    ST_TRY(esp_relax_check_x(h, x_inout));
    ST_TRY(esp_relax_prepare(h));
    EspRelax* r = h->rx;
    hipStream_t st = h->stream;
    const size_t mb = sizeof(double) * (size_t)h->m;
    const int grid = esp_relax_grid(h);
    HIP_TRY(hipMemcpyAsync(r->xa, x_inout, mb, hipMemcpyHostToDevice, st));
    double u = INFINITY;
    for (int it = 0; it < max_iters; ++it) {
        const double gamma = 2.0 / ((double)it + 2.0);
        ST_TRY(esp_relax_eval_on(h, r->xa, true));
        ST_TRY(esp_relax_select(h, (long)k));
        k_fw_final<<<grid, kBlock, 0, st>>>(h->s, r->xa, h->m, r->st, gamma, r->xb, nullptr, r->part);
        double s3[3];
        ST_TRY(esp_relax_read(h, grid, s3));
        u = std::min(u, s3[1]);
        if (f_traj) f_traj[it] = s3[0];
        if (dual_traj) dual_traj[it] = s3[1];
        if (gnorm_traj) gnorm_traj[it] = s3[2];
        *iters_out = it + 1;
        *upper_out = u;
        if (s3[2] < grad_tol) break;                                  // (x stays the iterate the test was evaluated at)
        if ((u - s3[0]) < gap_tol * std::fabs(s3[0])) break;          // (F >= 0; at F = 0 the test cannot fire)
        std::swap(r->xa, r->xb);
    }
    HIP_TRY(hipMemcpyAsync(x_inout, r->xa, mb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MACHIP_OK;
}

// machip_esp_relax_inner after its NULL checks: a . b through k_relax_inner and k_relax_scalars, in esp_relax_run's grid
inline int esp_relax_inner(machip_esp* h, const double* a, const double* b, double* out) {
    ST_TRY(esp_relax_prepare(h));
    EspRelax* r = h->rx;
    const size_t mb = sizeof(double) * (size_t)h->m;
    const int grid = esp_relax_grid(h);
    if (h->m) {
        HIP_TRY(hipMemcpyAsync(r->xa, a, mb, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(r->xb, b, mb, hipMemcpyHostToDevice, h->stream));
    }
    k_relax_inner<<<grid, kBlock, 0, h->stream>>>(r->xa, r->xb, h->m, r->part);
    k_relax_scalars<<<1, kBlock, 0, h->stream>>>(r->ldet, r->ld / kGjB, r->logdet0, r->part, grid, r->scal);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, r->scal + 3, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MACHIP_OK;
}

}  // namespace machip
