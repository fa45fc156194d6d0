// mac_amd/csrc/eig_routes.h -- GreedyEig's three routes together (eig.h: the dense inverse; eig_free.h, eig_free_tree.h: no Sigma): what
// machip_eig::reserve / columns / apply / push and the exchange's xch_reserve / xch_load / xch_round_room / xch_column do, one switch on
// the machip_esp's form each, and how a handle is made.  DESIGN 12, 21, 22, 23.
#pragma once
#include "eig_exchange_free.h"

inline int machip_eig::reserve(int64_t K) { return matrix_free() ? machip::eig_free_reserve(this, K) : MACHIP_OK; }

inline int machip_eig::columns(int count) {
    switch (base->form) {
    case machip::kEspFormTree: return machip::eig_tree_columns(this, count);
    case machip::kEspFormFree: return machip::eig_free_columns<false>(this, count);
    default: machip::eig_dense_columns(base, zview(), bc, count, Z, cc); return MACHIP_OK;
    }
}

inline int machip_eig::apply(int count) {
    switch (base->form) {
    case machip::kEspFormTree: ST_TRY(machip::eig_tree_sweeps(this, count, false)); break;
    case machip::kEspFormFree: machip::eig_free_scans(this, count); break;
    default: machip::eig_dense_apply(base, view(), count); return MACHIP_OK;
    }
    machip::eig_free_history(this, count);      // the history's correction is in T then: only the column's own term is left for k_eig_rr
    machip::k_eig_rr<<<count, machip::kBlock, 0, base->stream>>>(view(), nullptr, nullptr, 0);
    return MACHIP_OK;
}

inline int machip_eig::push(int best) {
    if (matrix_free()) return machip::eig_free_push(this);      // the history, never folded: the polished solve left z, c in column 0
    HIP_TRY(hipMemcpyAsync(bc, &best, sizeof(int), hipMemcpyHostToDevice, base->stream));
    HIP_TRY(hipStreamSynchronize(base->stream));
    push_column(bc);
    return MACHIP_OK;
}

inline int machip_eig::xch_reserve(int K, int C) { return matrix_free() ? reserve((int64_t)K + 2 * (int64_t)C + 1) : MACHIP_OK; }

inline int machip_eig::xch_load(const std::vector<int>& rows, const int* idx) {
    if (matrix_free()) return machip::eig_xfree_load(this, rows);
    for (size_t r = 0; r < rows.size(); ++r) push_column(idx + r);
    return MACHIP_OK;
}

inline int machip_eig::xch_round_room(const std::vector<int>& rows, int C, int64_t* compactions) {
    if (matrix_free()) {
        if (base->pending + 3 > seeds + (int)rows.size() + 2 * C + 1) {
            ST_TRY(machip::eig_xfree_compact(this, rows));
            ++*compactions;
        }
    } else if (base->pending > 0 && base->pending + 2 > base->fold) {
        base->fold_into(base->sig, base->pending);
        base->pending = 0;
    }
    return MACHIP_OK;
}

inline int machip_eig::xch_column(const int* cand, bool trial) {
    if (matrix_free()) {      // (trial or not, the same push: nothing folds here, and the caller's pending = j drops a trial)
        HIP_TRY(hipMemcpyAsync(bc, cand, sizeof(int), hipMemcpyDeviceToDevice, base->stream));
        ST_TRY(columns(1));
        return machip::eig_free_push(this);
    }
    if (trial) {
        const int j = base->pending;
        machip::eig_dense_columns(base, zview(), cand, 1, base->Zb + (size_t)j * (size_t)base->ld, base->cb + j);
        base->pending = j + 1;
    } else push_column(cand);
    return MACHIP_OK;
}

namespace machip {

// machip_eig_create's own refusals: host only, before the machip_esp's checks, its spanning-tree plan and the first look for a device.
// fold / batch: 0 becomes the default; flags: the machip_esp's (the tree route itself asks for MACHIP_ESP_SPANNING_TREE: a caller's is refused).
inline int eig_create_check(int& fold, int& batch, int& flags) {
    const int fold_given = fold;
    if (fold == 0) fold = kEigDefaultFold;
    if (batch == 0) batch = kEigDefaultBatch;
    if (batch < 1 || batch > kEigMaxBatch) return fail(MACHIP_BAD_ARG, "batch must be in [1, 4096]");
    const bool efree = (flags & MACHIP_EIG_MATRIX_FREE) != 0, etree = (flags & MACHIP_EIG_MATRIX_FREE_TREE) != 0;
    if ((flags & MACHIP_ESP_MATRIX_FREE) && !efree)
        return fail(MACHIP_BAD_ARG, "GreedyEig solves against the dense inverse: MACHIP_ESP_MATRIX_FREE is not available here");
    if (flags & MACHIP_ESP_SPANNING_TREE)
        return fail(MACHIP_BAD_ARG, "GreedyEig solves against the dense inverse: MACHIP_ESP_SPANNING_TREE is not available here");
    if (etree && !(efree && (flags & MACHIP_ESP_MATRIX_FREE)))
        return fail(MACHIP_BAD_ARG, "MACHIP_EIG_MATRIX_FREE_TREE puts GreedyEig on the spanning-tree handle: it is valid only as MACHIP_ESP_MATRIX_FREE | MACHIP_EIG_MATRIX_FREE | MACHIP_EIG_MATRIX_FREE_TREE");
    if (efree) {
        if (!(flags & MACHIP_ESP_MATRIX_FREE))
            return fail(MACHIP_BAD_ARG, "MACHIP_EIG_MATRIX_FREE puts GreedyEig on the chain-free handle: it is valid only as MACHIP_ESP_MATRIX_FREE | MACHIP_EIG_MATRIX_FREE");
        if (flags & MACHIP_ESP_DENSE_INVERSE)
            return fail(MACHIP_BAD_ARG, "MACHIP_EIG_MATRIX_FREE keeps no Sigma: it cannot be combined with MACHIP_ESP_DENSE_INVERSE");
        if (flags & ~(MACHIP_ESP_MATRIX_FREE | MACHIP_EIG_MATRIX_FREE | MACHIP_EIG_MATRIX_FREE_TREE))
            return fail(MACHIP_BAD_ARG, "unknown flags: MACHIP_EIG_MATRIX_FREE is valid only as MACHIP_ESP_MATRIX_FREE | MACHIP_EIG_MATRIX_FREE");
        if (fold_given != 0)      // (an argument that would be ignored is refused, not dropped)
            return fail(MACHIP_BAD_ARG, "MACHIP_EIG_MATRIX_FREE never folds: fold has no meaning on this route and must be 0");
        fold = 0;
    }
    flags = (flags & ~(MACHIP_EIG_MATRIX_FREE | MACHIP_EIG_MATRIX_FREE_TREE)) | (etree ? MACHIP_ESP_SPANNING_TREE : 0);
    return MACHIP_OK;
}

// machip_eig_create after its check and the machip_esp underneath (`base`, owned from here on; tplan: the plan its tables were made
// from, form 3 only): the host's adjacency, then the route's buffers, the batch arrays, Sigma0 or the seeds, the fixed graph's pair.
inline int eig_create_build(machip_esp* base, const EspTreePlan& tplan, int batch, machip_eig** out) {
    if (base->beta != 0.0) {
        machip_esp_destroy(base);
        return fail(MACHIP_DISCONNECTED, "GreedyEig needs a connected fixed graph (lambda_2 of the fixed graph is 0 otherwise)");
    }
    machip_eig* h = new machip_eig();
    h->base = base; h->n = base->n; h->m = base->m; h->batch = batch;
    h->ldq = (batch + kGjT - 1) / kGjT * kGjT;
    h->ldv = (h->n + kGjT - 1) / kGjT * kGjT;
    h->adj.assign((size_t)h->n, {}); h->hdeg.assign((size_t)h->n, 0.0);
    for (size_t e = 0; e < base->hfw.size(); ++e) h->add_edge(base->hfi[e], base->hfj[e], base->hfw[e]);
    h->adj0 = h->adj; h->hdeg0 = h->hdeg;
    h->hci = base->hci; h->hcj = base->hcj; h->hcw = base->hcw;
    h->sel.assign((size_t)h->m, 0);
    const bool etree = base->form == kEspFormTree;
    h->seeds = etree ? base->tr->seeds : 0;
    auto body = [&]() -> int {
        if (etree) ST_TRY(eig_tree_init(h, tplan));
        else if (h->matrix_free()) ST_TRY(eig_free_init(h));
        ST_TRY(h->alloc());
        ST_TRY(h->upload_graph());
        if (!h->matrix_free()) ST_TRY(base->load_sigma0());
        if (etree) ST_TRY(eig_free_reserve(h, 0));      // the seeds into the history: the fixed graph's own pair needs them
        base->pending = h->seeds;
        ST_TRY(h->first_pair());
        return h->reset();
    };
    const int st = body();
    if (st != MACHIP_OK) { machip_eig_destroy(h); return st; }
    *out = h;
    return MACHIP_OK;
}

}  // namespace machip
