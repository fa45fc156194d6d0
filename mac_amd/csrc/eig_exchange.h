// mac_amd/csrc/eig_exchange.h -- best-swap local search on lambda_2 from a given K-edge selection, on the state of a machip_eig
// handle (eig.h).  DESIGN section 20.
//
// S the selection, L_S = fixed graph + S.  A round looks for the pair (e in S, f outside S) with the largest
// lambda_2(L_S - w_e a_e a_e^T + w_f a_f a_f^T) and takes it when it beats lambda_2(L_S) + min_gain by more than 1e-8:
//   * removal pairs: (lambda_2(S \ e), v^-e) of all K selected edges, as columns of eig.h's batch solver.  A removal is the
//     candidate edge with weight -w_e: the exchange has candidate arrays of its own, the m candidates followed by K negated copies
//     of the selected ones (row r of the exchange = the copy at m + r), which machip_eig::view / zview hand to the solver's kernels
//     while the call runs.  k_eig_z's c = w / (1 + w s) is then the downdate coefficient -w_e / (1 - w_e s_e), whose denominator is
//     positive because the fixed graph is connected.
//   * pair pass (k_eig_xch_bounds): lambda_2 is concave in the weights, so with x = v^-e (any unit vector orthogonal to 1 will do,
//     and lambda the Rayleigh quotient the solver stored with it)  u(e, f) = lambda_2(S \ e) + w_f (x_i - x_j)^2 >= lambda_2(S \ e + f).
//     K x ldm bounds, -inf for the selected f, and one maximum per workgroup.
//   * exact solves: rows in decreasing order of their largest bound while that is above max(tau, top) (tau = lambda_2(S) + min_gain,
//     top the largest value solved in the round); in a row, the greedy's own scan (machip_eig::scan) from the start vector v^-e with
//     the floor tau.  For a row the downdate column of e is appended to the pending block (and dropped afterwards: a trial never
//     folds) and the CSR of L_{S \ e} is uploaded.
//   * scan: the solved pairs in (e, f) order, a pair replaces the running value (initially tau) only if it exceeds it by more than
//     1e-8 -- GreedyEig's rule.  Nobody: converged.  Else the swap: two columns join the pending block (machip_eig::push_column), the
//     adjacency, the flags and the negated copy of the row are rewritten, the new pair is polished (machip_eig::adopt_pair).
// Everything is a function of the inputs alone: sorts are stable, reductions run in a fixed order, no floating-point atomics.
// On a matrix-free handle (machip_eig_exchange_free) the same rounds run on the route's history: the load, the room
// for a round, the trial column and the swap's columns are machip_eig::xch_* (eig_routes.h), the history's side is eig_exchange_free.h.
#pragma once
#include <chrono>
#include <string>
#include <vector>

#include "eig.h"

namespace machip {

constexpr int kEigXchTargetGroups = 1024;     // workgroups of a pair pass the candidate range is cut for when K alone gives fewer
constexpr int kEigXchFreeSwaps = 32;          // matrix-free handles: swaps the history has room for between two compactions (option
constexpr int kEigXchFreeSwapsMax = 4096;     // eig_xch_free_swaps, 1 .. 4096)

struct EigXch {
    int *cu = nullptr, *cv = nullptr;      // m + K reduced endpoints
    double* cw = nullptr;                  // m + K weights (the last K negated)
    int* sel = nullptr;                    // m flags
    size_t cand = 0;                       // entries cu / cv / cw / sel hold
    int* idx = nullptr;                    // 2 K: the edge of every row, then m + row (what k_eig_z takes its column's candidate from)
    double *Vr = nullptr, *lamr = nullptr; // K x ldv removal vectors, K values
    double* U = nullptr;                   // K x ldm bounds
    size_t rows = 0, ldm = 0;
    double* pv = nullptr;                  // K x chunks workgroup maxima
    size_t parts = 0;
};

// ---- the pair pass.  grid = (K, chunks): workgroup (row, y) owns the removal pair of row `row` and the candidates
// [y per, (y + 1) per), per a multiple of 4.  The candidates' arrays are streamed 16 bytes per lane and array (4 candidates per lane
// and step); the vector's entries are gathered (8 n bytes per row: L2).  u into U[row, :], -inf for the selected; the workgroup's
// maximum into pv[row chunks + y]. ----
__device__ __forceinline__ double eig_xch_bound(const double* __restrict__ v, double lam, int u, int w, double wt, int s) {
    const double d = v[u + 1] - v[w + 1];
    return s ? -INFINITY : lam + wt * d * d;
}

__global__ __launch_bounds__(kBlock) void k_eig_xch_bounds(const int* __restrict__ cu, const int* __restrict__ cv, const double* __restrict__ cw,
                                                           const int* __restrict__ sel, int m, const double* __restrict__ Vr, int ldv,
                                                           const double* __restrict__ lamr, int per, double* __restrict__ U, int ldm,
                                                           double* __restrict__ pv) {
    __shared__ double sv[kBlock / kWave];
    __shared__ int si[kBlock / kWave];
    const int row = blockIdx.x;
    const double* v = Vr + (size_t)row * ldv;
    const double lam = lamr[row];
    double* out = U + (size_t)row * ldm;
    const int f0 = blockIdx.y * per, f1 = min(m, f0 + per);
    double bv = -INFINITY;
    int bf = INT_MAX;
    for (int f = f0 + 4 * (int)threadIdx.x; f < f1; f += 4 * kBlock) {
        if (f + 4 <= f1) {      // (f is a multiple of 4: 16-byte aligned in every array, rows of U included)
            const int4 a = *reinterpret_cast<const int4*>(cu + f), b = *reinterpret_cast<const int4*>(cv + f);
            const int4 s = *reinterpret_cast<const int4*>(sel + f);
            const double2 w0 = *reinterpret_cast<const double2*>(cw + f), w1 = *reinterpret_cast<const double2*>(cw + f + 2);
            double2 r0, r1;
            r0.x = eig_xch_bound(v, lam, a.x, b.x, w0.x, s.x); r0.y = eig_xch_bound(v, lam, a.y, b.y, w0.y, s.y);
            r1.x = eig_xch_bound(v, lam, a.z, b.z, w1.x, s.z); r1.y = eig_xch_bound(v, lam, a.w, b.w, w1.y, s.w);
            *reinterpret_cast<double2*>(out + f) = r0;
            *reinterpret_cast<double2*>(out + f + 2) = r1;
            esp_better(bv, bf, r0.x, f); esp_better(bv, bf, r0.y, f + 1); esp_better(bv, bf, r1.x, f + 2); esp_better(bv, bf, r1.y, f + 3);
        } else {
            for (int g = f; g < f1; ++g) {
                const double r = eig_xch_bound(v, lam, cu[g], cv[g], cw[g], sel[g]);
                out[g] = r;
                esp_better(bv, bf, r, g);
            }
        }
    }
    esp_block_argmax(bv, bf, sv, si);
    if (threadIdx.x == 0) pv[(size_t)row * gridDim.y + blockIdx.y] = bv;
}

inline void eig_xch_release(EigXch*& x) {
    if (!x) return;
    void* bufs[] = {x->cu, x->cv, x->cw, x->sel, x->idx, x->Vr, x->lamr, x->U, x->pv};
    for (void* q : bufs) if (q) (void)hipFree(q);
    delete x;
    x = nullptr;
}

// The arguments, decided on the host before a device is touched.  sorted_out: the selection ascending.
// free_entry: machip_eig_exchange_free's call, where the clause on the route is the other way round.
inline int eig_xch_check(const machip_eig* h, int64_t k, const int32_t* sel_in, int64_t max_swaps, double min_gain, std::vector<int>& sorted_out,
                         bool free_entry = false) {
    if (!h) return fail(MACHIP_BAD_ARG, "NULL handle");
    if (h->matrix_free() && !free_entry)
        return fail(MACHIP_BAD_ARG, "the exchange works on the dense inverse: it is not available on a MACHIP_EIG_MATRIX_FREE handle (machip_eig_exchange_free is)");
    if (!h->matrix_free() && free_entry)
        return fail(MACHIP_BAD_ARG, "machip_eig_exchange_free works on the history of a MACHIP_EIG_MATRIX_FREE handle: a handle with the dense inverse takes machip_eig_exchange");
    if (!sel_in) return fail(MACHIP_BAD_ARG, "sel_in is NULL");
    if (max_swaps < 0) return fail(MACHIP_BAD_ARG, "max_swaps must be >= 0 (got " + std::to_string((long long)max_swaps) + ")");
    if (!(min_gain >= 0.0) || !std::isfinite(min_gain)) return fail(MACHIP_BAD_ARG, "min_gain must be finite and >= 0");
    if (k < 1 || k >= h->m)
        return fail(MACHIP_BAD_ARG, "k must be in [1, m - 1] (k = " + std::to_string((long long)k) + ", m = " + std::to_string(h->m) + " candidates)");
    std::vector<char> seen((size_t)h->m, 0);
    for (int64_t q = 0; q < k; ++q) {
        const int e = sel_in[q];
        if (e < 0 || e >= h->m)
            return fail(MACHIP_BAD_ARG, "sel_in[" + std::to_string((long long)q) + "] = " + std::to_string(e) + " is outside [0, m = " + std::to_string(h->m) + ")");
        if (seen[(size_t)e]) return fail(MACHIP_BAD_ARG, "sel_in names candidate " + std::to_string(e) + " more than once (a repeated index)");
        seen[(size_t)e] = 1;
    }
    sorted_out.clear();
    for (int e = 0; e < h->m; ++e) if (seen[(size_t)e]) sorted_out.push_back(e);
    return MACHIP_OK;
}

// The call's state: made by the first exchange call on a handle, grown by a later one that needs more, freed by
// machip_eig_destroy.  The K vectors and the K x ldm bounds are refused when they exceed the device's free memory (or option
// eig_xch_max_mb, a cap in MiB) -- before anything is allocated or launched.
inline int eig_xch_prepare(EigXch*& x, size_t m, size_t K, size_t ldv, size_t ldm, size_t parts) {
    if (!x) x = new EigXch();
    if (x->rows < K || x->ldm < ldm) {
        const size_t need = sizeof(double) * K * (ldv + ldm);
        size_t avail = 0, total = 0;
        HIP_TRY(hipMemGetInfo(&avail, &total));
        const long cap_mb = default_options().get(kOpt_eig_xch_max_mb, 0);
        if (cap_mb > 0) avail = std::min(avail, (size_t)cap_mb << 20);
        if (need > avail)
            return fail(MACHIP_BAD_ARG, "the exchange keeps one Fiedler vector and one row of bounds per selected edge: 8 x K x (ldv + ldm) = 8 x " +
                                            std::to_string(K) + " x (" + std::to_string(ldv) + " + " + std::to_string(ldm) + ") = " + std::to_string(need) +
                                            " bytes, more than the " + std::to_string(avail) + " bytes available" +
                                            (cap_mb > 0 ? " (option eig_xch_max_mb)" : " on the device"));
        void* old[] = {x->Vr, x->lamr, x->U, x->idx};
        for (void* q : old) if (q) (void)hipFree(q);
        x->Vr = x->lamr = x->U = nullptr; x->idx = nullptr; x->rows = x->ldm = 0;
        ST_TRY(dev_alloc(&x->Vr, K * ldv)); ST_TRY(dev_alloc(&x->lamr, K)); ST_TRY(dev_alloc(&x->U, K * ldm)); ST_TRY(dev_alloc(&x->idx, 2 * K));
        x->rows = K; x->ldm = ldm;
    }
    if (x->cand < m + K) {
        void* old[] = {x->cu, x->cv, x->cw, x->sel};
        for (void* q : old) if (q) (void)hipFree(q);
        x->cu = x->cv = x->sel = nullptr; x->cw = nullptr; x->cand = 0;
        ST_TRY(dev_alloc(&x->cu, m + K)); ST_TRY(dev_alloc(&x->cv, m + K)); ST_TRY(dev_alloc(&x->cw, m + K)); ST_TRY(dev_alloc(&x->sel, m + K));
        x->cand = m + K;
    }
    if (x->parts < parts) {
        if (x->pv) { (void)hipFree(x->pv); x->pv = nullptr; }
        x->parts = 0;
        ST_TRY(dev_alloc(&x->pv, parts));
        x->parts = parts;
    }
    return MACHIP_OK;
}

// the edge (a, b, w) out of the host's adjacency: the last entry that matches in both rows (equal entries are interchangeable);
// the two degrees are summed again in row order, which is the order add_edge accumulated them in -- the bits of a graph that never
// had the edge
inline int eig_xch_remove_edge(machip_eig* h, int a, int b, double w) {
    if (a == b) return MACHIP_OK;
    const int ends[2] = {a, b};
    for (int s = 0; s < 2; ++s) {
        auto& row = h->adj[(size_t)ends[s]];
        const int other = ends[1 - s];
        size_t q = row.size();
        while (q > 0 && !(row[q - 1].first == other && row[q - 1].second == w)) --q;
        if (q == 0) return fail(MACHIP_NOT_CONVERGED, "exchange: a selected edge is missing from the graph (" + std::to_string(a) + ", " + std::to_string(b) + ")");
        row.erase(row.begin() + (long)(q - 1));
        double d = 0.0;
        for (auto& pr : row) d += pr.second;
        h->hdeg[(size_t)ends[s]] = d;
    }
    return MACHIP_OK;
}

struct EigXchPair {
    int e, f, row;
    double val;
};

// The rounds.  rowe: the selection ascending.  Every output may be NULL.
inline int eig_exchange_run(machip_eig* h, std::vector<int> rowe, int64_t max_swaps, double min_gain, int32_t* sel_out, int32_t* out_idx,
                            int32_t* in_idx, double* lambda2_out, int64_t* n_swaps, int32_t* converged, int32_t* counts, double* t_ms,
                            int64_t* n_compactions) {
    machip_esp* base = h->base;
    hipStream_t st = base->stream;
    const int K = (int)rowe.size(), m = h->m, ldv = h->ldv, batch = h->batch;
    const int ldm = (m + 3) / 4 * 4;
    const int chunks = std::max(1, std::min((m + kBlock - 1) / kBlock, (kEigXchTargetGroups + K - 1) / K));
    const int per = ((m + chunks - 1) / chunks + 3) / 4 * 4;
    // the swaps a matrix-free history has room for between two compactions (option eig_xch_free_swaps, read per call)
    const int C = h->matrix_free() ? (int)std::min<int64_t>(max_swaps, std::max(1, std::min(default_options().get(kOpt_eig_xch_free_swaps, kEigXchFreeSwaps), kEigXchFreeSwapsMax))) : 0;
    ST_TRY(h->xch_reserve(K, C));      // (refused before the state is touched)
    ST_TRY(eig_xch_prepare(h->xc, (size_t)m, (size_t)K, (size_t)ldv, (size_t)ldm, (size_t)K * (size_t)chunks));
    EigXch* X = h->xc;
    while (base->ev.size() < 2) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        base->ev.push_back(e);
    }
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipEventRecord(base->ev[0], st));

    // ---- load ----
    ST_TRY(h->reset());
    std::vector<int> hu((size_t)(m + K)), hv((size_t)(m + K)), hsel((size_t)m, 0), hidx((size_t)(2 * K));
    std::vector<double> hw((size_t)(m + K));
    for (int e = 0; e < m; ++e) { hu[(size_t)e] = h->hci[(size_t)e] - 1; hv[(size_t)e] = h->hcj[(size_t)e] - 1; hw[(size_t)e] = h->hcw[(size_t)e]; }
    auto set_row = [&](int r, int e) {      // row r holds candidate e: its negated copy at m + r
        rowe[(size_t)r] = e; hidx[(size_t)r] = e; hidx[(size_t)(K + r)] = m + r;
        hu[(size_t)(m + r)] = hu[(size_t)e]; hv[(size_t)(m + r)] = hv[(size_t)e]; hw[(size_t)(m + r)] = -hw[(size_t)e];
    };
    for (int r = 0; r < K; ++r) { set_row(r, rowe[(size_t)r]); hsel[(size_t)rowe[(size_t)r]] = 1; }
    auto upload_view = [&]() -> int {      // (synchronous: the staging vectors are rewritten by the next swap)
        HIP_TRY(hipMemcpyAsync(X->cu, hu.data(), sizeof(int) * hu.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(X->cv, hv.data(), sizeof(int) * hv.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(X->cw, hw.data(), sizeof(double) * hw.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(X->sel, hsel.data(), sizeof(int) * hsel.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(X->idx, hidx.data(), sizeof(int) * hidx.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        return MACHIP_OK;
    };
    ST_TRY(upload_view());
    h->xcu = X->cu; h->xcv = X->cv; h->xcw = X->cw;
    ST_TRY(h->xch_load(rowe, X->idx));
    for (int r = 0; r < K; ++r) {
        const int e = rowe[(size_t)r];
        h->sel[(size_t)e] = 1;
        h->add_edge(h->hci[(size_t)e], h->hcj[(size_t)e], h->hcw[(size_t)e]);
    }
    HIP_TRY(hipGetLastError());
    ST_TRY(h->upload_graph());
    ST_TRY(h->adopt_pair(-1, h->v0, nullptr));
    if (lambda2_out) lambda2_out[0] = h->lamcur;

    // ---- rounds ----
    int64_t t = 0, compactions = 0;
    int conv = 0;
    std::vector<double> lamr((size_t)K), part((size_t)K * (size_t)chunks), rowmax((size_t)K), u((size_t)m);
    std::vector<int> list, rord((size_t)K);
    std::vector<EigXchPair> pairs;
    while (t < max_swaps) {
        ST_TRY(h->xch_round_room(rowe, C, &compactions));
        const double tau = h->lamcur + min_gain;
        int napp = 0;
        // removal pairs: column b of a batch is the negated copy of row q + b
        for (int q = 0; q < K; q += batch) {
            const int cnt = std::min(K - q, batch);
            list.resize((size_t)cnt);
            for (int b = 0; b < cnt; ++b) list[(size_t)b] = m + q + b;
            ST_TRY(h->solve_batch(list.data(), cnt, h->vcur, &napp));
            HIP_TRY(hipMemcpyAsync(X->Vr + (size_t)q * (size_t)ldv, h->X, sizeof(double) * (size_t)cnt * (size_t)ldv, hipMemcpyDeviceToDevice, st));
            for (int b = 0; b < cnt; ++b) lamr[(size_t)(q + b)] = h->h_lam[(size_t)b];
        }
        // pair pass
        HIP_TRY(hipMemcpyAsync(X->lamr, lamr.data(), sizeof(double) * (size_t)K, hipMemcpyHostToDevice, st));
        k_eig_xch_bounds<<<dim3((unsigned)K, (unsigned)chunks), kBlock, 0, st>>>(X->cu, X->cv, X->cw, X->sel, m, X->Vr, ldv, X->lamr, per, X->U, ldm, X->pv);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(part.data(), X->pv, sizeof(double) * part.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int r = 0; r < K; ++r) {
            double b = -INFINITY;
            for (int y = 0; y < chunks; ++y) b = std::max(b, part[(size_t)r * (size_t)chunks + (size_t)y]);
            rowmax[(size_t)r] = b;
            rord[(size_t)r] = r;
        }
        std::stable_sort(rord.begin(), rord.end(), [&](int a, int b) { return rowmax[(size_t)a] > rowmax[(size_t)b]; });
        // exact solves
        EigScan scan;      // of the round: top runs over the rows, the last batch is the last row's that solved one
        pairs.clear();
        int last_row = -1;
        bool trial_graph = false;
        for (int r : rord) {
            if (!(rowmax[(size_t)r] > std::max(tau, scan.top))) break;
            const int e = rowe[(size_t)r], a = h->hci[(size_t)e], b = h->hcj[(size_t)e];
            const int j = base->pending;
            ST_TRY(h->xch_column(X->idx + K + r, true));
            HIP_TRY(hipGetLastError());
            {      // the CSR of L_{S \ e}; the host's adjacency stays L_S
                const auto ra = h->adj[(size_t)a], rb = h->adj[(size_t)b];
                const double da = h->hdeg[(size_t)a], db = h->hdeg[(size_t)b];
                int rc = eig_xch_remove_edge(h, a, b, h->hcw[(size_t)e]);
                if (rc == MACHIP_OK) rc = h->upload_graph();
                h->adj[(size_t)a] = ra; h->adj[(size_t)b] = rb; h->hdeg[(size_t)a] = da; h->hdeg[(size_t)b] = db;
                trial_graph = true;
                if (rc != MACHIP_OK) { base->pending = j; return rc; }
            }
            HIP_TRY(hipMemcpyAsync(u.data(), X->U + (size_t)r * (size_t)ldm, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const int before = scan.solved;      // (h->sel is hsel: the scan leaves out the selected f)
            const int rc = h->scan(scan, u, tau, X->Vr + (size_t)r * (size_t)ldv, &napp, [&](int f, double val) { pairs.push_back({e, f, r, val}); });
            if (scan.solved > before) last_row = r;
            base->pending = j;      // the trial column is dropped: Sigma never saw it
            if (rc != MACHIP_OK) return rc;
        }
        // scan
        std::stable_sort(pairs.begin(), pairs.end(), [](const EigXchPair& x, const EigXchPair& y) { return x.e < y.e || (x.e == y.e && x.f < y.f); });
        int best = -1;
        double running = tau;
        for (size_t p = 0; p < pairs.size(); ++p)
            if (pairs[p].val > running + kEigTol) { best = (int)p; running = pairs[p].val; }
        if (best < 0) {
            if (trial_graph) ST_TRY(h->upload_graph());
            h->solved.push_back(scan.solved); h->applies.push_back(napp); h->removal.push_back(K);
            conv = 1;
            break;
        }
        // the swap
        const EigXchPair w = pairs[(size_t)best];
        ST_TRY(h->xch_column(X->idx + K + w.row, false));      // e leaves (the negated copy, still e's)
        set_row(w.row, w.f);
        hsel[(size_t)w.e] = 0; hsel[(size_t)w.f] = 1;
        ST_TRY(upload_view());
        ST_TRY(h->xch_column(X->idx + w.row, false));          // f enters
        HIP_TRY(hipGetLastError());
        h->sel[(size_t)w.e] = 0; h->sel[(size_t)w.f] = 1;
        ST_TRY(eig_xch_remove_edge(h, h->hci[(size_t)w.e], h->hcj[(size_t)w.e], h->hcw[(size_t)w.e]));
        h->add_edge(h->hci[(size_t)w.f], h->hcj[(size_t)w.f], h->hcw[(size_t)w.f]);
        ST_TRY(h->upload_graph());
        // the new pair, polished: from the pair's converged vector when that is still resident (it was in the last batch), else from v^-e
        const int col = last_row == w.row ? scan.resident_column(w.f) : -1;
        ST_TRY(h->adopt_pair(-1, col >= 0 ? h->X + (size_t)col * (size_t)ldv : X->Vr + (size_t)w.row * (size_t)ldv, &napp));
        h->solved.push_back(scan.solved); h->applies.push_back(napp); h->removal.push_back(K);
        if (out_idx) out_idx[t] = w.e;
        if (in_idx) in_idx[t] = w.f;
        if (lambda2_out) lambda2_out[t + 1] = h->lamcur;
        ++t;
    }
    HIP_TRY(hipEventRecord(base->ev[1], st));
    HIP_TRY(hipStreamSynchronize(st));
    if (sel_out) {
        int q = 0;
        for (int e = 0; e < m; ++e) if (h->sel[(size_t)e]) sel_out[q++] = e;
    }
    if (n_swaps) *n_swaps = t;
    if (converged) *converged = conv;
    if (n_compactions) *n_compactions = compactions;
    if (counts)
        for (size_t r = 0; r < h->solved.size(); ++r) {
            counts[3 * r] = h->solved[r]; counts[3 * r + 1] = h->applies[r]; counts[3 * r + 2] = h->removal[r];
        }
    if (t_ms) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, base->ev[0], base->ev[1]));
        t_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        t_ms[1] = ms;
    }
    return MACHIP_OK;
}

// The call after its checks: the handle leaves it with the greedy's candidate arrays and, after a failure, at the fixed graph (message kept)
inline int eig_exchange(machip_eig* h, const std::vector<int>& rowe, int64_t max_swaps, double min_gain, int32_t* sel_out, int32_t* out_idx,
                        int32_t* in_idx, double* lambda2_out, int64_t* n_swaps, int32_t* converged, int32_t* counts, double* t_ms,
                        int64_t* n_compactions = nullptr) {
    const int st = eig_exchange_run(h, rowe, max_swaps, min_gain, sel_out, out_idx, in_idx, lambda2_out, n_swaps, converged, counts, t_ms, n_compactions);
    h->xcu = h->xcv = nullptr; h->xcw = nullptr;
    if (st != MACHIP_OK) {
        const std::string msg = machip_last_error();
        if (h->reset() == MACHIP_OK) return fail((machip_status)st, msg);
    }
    return st;
}

}  // namespace machip
