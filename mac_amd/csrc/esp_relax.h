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
// On a MACHIP_ESP_EDGE_RELAX handle the kernels of steps 1 and 4 are those of esp_relax_edge.h instead -- N(x) = I + G D in the
// candidates' space and the gradient from its inverse -- on a MACHIP_ESP_EDGE_RELAX_TREE handle those of esp_relax_edge_tree.h:
// the same N(x) over the candidates and the seeds of a spanning tree, its Gram matrix stored, log det N(0) subtracted.
// Everything else is written once, here.  The space is a field of the handle (machip_esp::relax_space) and EspRelaxRoute
// below is what follows from it -- columns, leading dimension, limit, messages; four places switch on it: esp_relax_limits,
// esp_relax_prepare, esp_relax_eval_on and, in esp_exchange_edge.h, the loading of the Gram matrix (by whether G is stored).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "esp.h"
#include "esp_relax_edge.h"
#include "esp_relax_edge_tree.h"
#include "kernels.h"

namespace machip {

// What follows from the space of a handle's relaxation (machip_esp::relax_space), from the handle alone: nothing is allocated
// before it is asked.  The one place that rounds up to 64, compares with the dense limit and words the spaces' messages.
struct EspRelaxRoute {
    EspRelaxSpace space;
    int64_t cols;      // what the dense limit is on: num_nodes (an evaluation inverts the n - 1 reduced columns), m, m + r
    int ld;            // leading dimension of the matrix an evaluation inverts: the handle's, or cols rounded up to 64 (at least 64)
    bool oversize() const { return cols > kEspDenseMaxN; }
    const char* lost_pivot() const {
        return space == kEspRelaxNode ? "M(x) is not positive definite numerically (a non-positive Gauss-Jordan pivot)"
                                      : "N(x) = I + G D has a non-positive Gauss-Jordan pivot (its leading minors are positive: lost numerically)";
    }
};

inline EspRelaxRoute esp_relax_route(const machip_esp* h) {
    EspRelaxRoute R{h->relax_space, h->n, h->ld};
    switch (R.space) {
    case kEspRelaxNode: return R;
    case kEspRelaxEdge: R.cols = h->m; break;
    case kEspRelaxEdgeTree: R.cols = (int64_t)h->m + h->tr->seeds; break;
    }
    R.ld = (int)((std::max<int64_t>(R.cols, 1) + kGjT - 1) / kGjT * kGjT);
    return R;
}

// What the relaxation cannot do on this handle.
inline int esp_relax_limits(const machip_esp* h) {
    const EspRelaxRoute R = esp_relax_route(h);
    // (tr: a MACHIP_ESP_MATRIX_FREE | MACHIP_ESP_SPANNING_TREE handle, esp_tree.h)
    if (R.space == kEspRelaxNode && (h->form == kEspFormFree || h->tr))
        return fail(MACHIP_BAD_ARG, "the relaxation inverts the dense M(x): not available on a MACHIP_ESP_MATRIX_FREE handle");
    if (!R.oversize()) return MACHIP_OK;
    switch (R.space) {
    case kEspRelaxEdgeTree:
        return fail(MACHIP_BAD_ARG, "MACHIP_ESP_EDGE_RELAX_TREE inverts the dense (m + r) x (m + r) N(x): candidates plus seeds must be <= 16384 (m = " +
                                        std::to_string((int64_t)h->m) + ", r = " + std::to_string((int64_t)h->tr->seeds) + ")");
    case kEspRelaxEdge:
        return fail(MACHIP_BAD_ARG, "MACHIP_ESP_EDGE_RELAX inverts the dense m x m N(x): the number of candidates must be <= 16384 (m = " +
                                        std::to_string(h->m) + ")");
    default:
        return fail(MACHIP_BAD_ARG, "the relaxation inverts the dense M(x) (no chain closed form): num_nodes must be <= 16384");
    }
}

struct EspRelax {
    EspRelaxRoute route;                     // of the handle, when the state was made
    double* bufC = nullptr;                  // the inverse's second buffer (the first is the handle's working copy `sig`)
    int *rowptr = nullptr, *ecol = nullptr, *tptr = nullptr, *tx = nullptr;     // incidence list by node (below)
    double* tw = nullptr;
    double *xa = nullptr, *xb = nullptr;     // iterate and next iterate
    double *part = nullptr, *ldet = nullptr, *scal = nullptr;
    SelState* st = nullptr;
    unsigned int* hist = nullptr;
    double logdet0 = 0.0;                    // log det M(0), by the same kernels in the same order (F(0) = 0 exactly)
    EspEdge* edge = nullptr;                 // both edge spaces (esp_relax_edge.h): N(x) instead of M(x); bufC .. tw and hist stay unused
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
    esp_edge_release(r->edge);
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

// Steps 1-4 for the x in `x`: the space's matrix and its inverse (ld / 32 is even: the inverse ends where the matrix was
// assembled), the blocks' log-determinants in ldet[], the gradient in h->s (want_grad).  Node space: in h->sig, the greedy's
// working copy -- the last selection run's state is gone, Sigma0 is not touched.  Edge spaces: in the state's own bufN; neither
// h->live nor h->pending is written, the greedy's last run stays what it was.
inline int esp_relax_eval_on(machip_esp* h, const double* x, bool want_grad) {
    EspRelax* r = h->rx;
    const EspEdge* E = r->edge;
    const EspRelaxSpace space = r->route.space;
    const int ld = r->route.ld, m = h->m;
    hipStream_t st = h->stream;
    double *src = nullptr, *dst = nullptr, *piv = nullptr;
    HIP_TRY(hipMemsetAsync(h->bad, 0, sizeof(int), st));
    switch (space) {
    case kEspRelaxNode:
        h->live = false;
        h->pending = 0;
        src = h->sig; dst = r->bufC; piv = h->piv;
        k_relax_assemble<<<ld, kBlock, 0, st>>>(src, ld, r->rowptr, r->ecol, r->tptr, r->tw, r->tx, x);
        break;
    case kEspRelaxEdge:
        src = E->bufN; dst = E->bufC; piv = E->piv;
        k_edge_assemble<<<ld, kBlock, 0, st>>>(src, ld, m, E->eu, E->ev, h->cw, h->R, x);
        break;
    case kEspRelaxEdgeTree:
        src = E->bufN; dst = E->bufC; piv = E->piv;
        k_edge_tree_assemble<<<ld, kBlock, 0, st>>>(src, E->G, ld, E->M, m, h->cw, h->tr->sw, x);
        break;
    }
    h->gj_inverse_of<true>(src, dst, ld, piv, r->ldet);
    if (want_grad && m) switch (space) {
        case kEspRelaxNode: k_esp_scores<<<h->grid_m(), kBlock, 0, st>>>(h->view(), src, 0); break;
        case kEspRelaxEdge: k_edge_grad<<<m, kBlock, 0, st>>>(src, ld, m, E->eu, E->ev, h->cw, h->R, h->s); break;
        case kEspRelaxEdgeTree: k_edge_tree_grad<<<m, kBlock, 0, st>>>(src, E->G, ld, E->M, h->cw, h->s); break;
    }
    HIP_TRY(hipGetLastError());
    return MACHIP_OK;
}

// Step 5 on the gradient in h->s, into r->st: machip_lp_topk's select and its tie rule (kernels.h: sel_launch).
inline int esp_relax_select(machip_esp* h, long k) {
    EspRelax* r = h->rx;
    if (h->m > kSelSmallMax && !r->hist) return fail(MACHIP_BAD_ARG, "the multi-launch select has no histogram on this handle (edge space allocates none: m <= 16384 must stay below kSelSmallMax)");
    return sel_launch(h->stream, h->s, h->m, k, r->st, r->hist, 0, true, false);
}

// F (and the other two scalars when `np` partials of k_fw_final are there) to the host, with the pivot flag.
inline int esp_relax_read(machip_esp* h, int np, double* out3) {
    EspRelax* r = h->rx;
    int hbad = 0;
    k_relax_scalars<<<1, kBlock, 0, h->stream>>>(r->ldet, r->route.ld / kGjB, r->logdet0, r->part, np, r->scal);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out3, r->scal, sizeof(double) * 3, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&hbad, h->bad, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (hbad) return fail(MACHIP_NOT_CONVERGED, r->route.lost_pivot());
    return MACHIP_OK;
}

// First relaxation call on a handle: the limits, then the space's own resources, the ones every space has, and log det of the
// matrix at x = 0 by one evaluation there -- except on the chain edge route, where N(0) = I: ldet is zeroed (what
// k_relax_scalars sums when machip_esp_relax_inner is the handle's first call) and the ld^3 inverse is not paid.  Neither edge
// space has a histogram or an incidence list: m <= 16 384 is below kSelSmallMax, the multi-launch select is never taken.
inline int esp_relax_prepare(machip_esp* h) {
    ST_TRY(esp_relax_limits(h));
    HIP_TRY(hipSetDevice(h->device));
    if (h->rx) return MACHIP_OK;
    EspRelax* r = new EspRelax{esp_relax_route(h)};
    h->rx = r;
    auto body = [&]() -> int {
        const EspRelaxRoute& R = r->route;
        const size_t ld = (size_t)R.ld, ms = (size_t)std::max(h->m, 1);
        bool identity_at_0 = false;
        switch (R.space) {
        case kEspRelaxNode:
            ST_TRY(dev_alloc(&r->bufC, ld * ld));
            ST_TRY(dev_alloc(&r->hist, (size_t)6 * kBins));
            ST_TRY(esp_relax_build_lists(h, r));
            break;
        case kEspRelaxEdge:
            ST_TRY(esp_edge_alloc(r->edge = new EspEdge(), (int)R.cols, R.ld, false));
            ST_TRY(esp_edge_chain_ends(h, r->edge));
            identity_at_0 = true;
            break;
        case kEspRelaxEdgeTree:
            ST_TRY(esp_edge_alloc(r->edge = new EspEdge(), (int)R.cols, R.ld, true));
            ST_TRY(esp_edge_tree_gram(h, r->edge));
            break;
        }
        ST_TRY(dev_alloc(&r->xa, ms)); ST_TRY(dev_alloc(&r->xb, ms));
        ST_TRY(dev_alloc(&r->part, (size_t)2 * kMaxGrid)); ST_TRY(dev_alloc(&r->ldet, ld / kGjB)); ST_TRY(dev_alloc(&r->scal, 4));
        ST_TRY(dev_alloc(&r->st, 1));
        if (identity_at_0) {
            HIP_TRY(hipMemsetAsync(r->ldet, 0, sizeof(double) * (ld / kGjB), h->stream));
            return MACHIP_OK;
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
    if (esp_relax_route(h).oversize()) return esp_relax_limits(h);      // (the refusal ahead of the argument checks, nothing allocated)
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
    k_relax_scalars<<<1, kBlock, 0, h->stream>>>(r->ldet, r->route.ld / kGjB, r->logdet0, r->part, grid, r->scal);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, r->scal + 3, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MACHIP_OK;
}

// machip_esp_relax_info after its NULL checks.  A node-space handle reports ld = 0 until its first relaxation call.
inline int esp_relax_info(const machip_esp* h, int32_t* info2) {
    const EspRelaxRoute R = esp_relax_route(h);
    info2[0] = R.space;
    info2[1] = R.space == kEspRelaxNode && !h->rx ? 0 : R.ld;
    return MACHIP_OK;
}

// machip_esp_relax_gram after its NULL checks: the M x M corner of the stored Gram matrix, made by the first relaxation call
inline int esp_relax_gram(machip_esp* h, double* G_out, int64_t M) {
    const EspRelaxRoute R = esp_relax_route(h);
    if (R.space != kEspRelaxEdgeTree) return fail(MACHIP_BAD_ARG, "the stored Gram matrix belongs to a MACHIP_ESP_EDGE_RELAX_TREE handle: this handle keeps none");
    if (M != R.cols)
        return fail(MACHIP_BAD_ARG, "M must be m + r = " + std::to_string((long long)R.cols) + " (m = " + std::to_string(h->m) + " candidates, r = " +
                                        std::to_string(h->tr->seeds) + " seeds), not " + std::to_string((long long)M));
    ST_TRY(esp_relax_prepare(h));
    if (!M) return MACHIP_OK;
    const EspEdge* E = h->rx->edge;
    HIP_TRY(hipMemcpy2DAsync(G_out, sizeof(double) * (size_t)M, E->G, sizeof(double) * (size_t)E->ld, sizeof(double) * (size_t)M, (size_t)M,
                             hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MACHIP_OK;
}

}  // namespace machip
