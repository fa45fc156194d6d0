// mac_amd/csrc/esp_select.h -- machip_esp_select and machip_esp_weighted_resistances on every form of handle: the dense one (esp.h),
// the chain without Sigma (esp_free.h) and the spanning tree without Sigma (esp_tree.h).  The greedy loop itself is esp.h's
// esp_select_run; a route is its start kernel and its z step.  DESIGN sections 11, 14, 15.
#pragma once
#include "esp_tree.h"

namespace machip {

// machip_esp_select after its checks: the route's history, then esp_select_run with the route's start kernel and z step
inline int esp_select(machip_esp* h, int nb, const int64_t* ks, int32_t* order_out, double* gain_out, double* t_ms_out) {
    const int K = (int)ks[nb - 1], rg = esp_rows_grid(h->ld);
    hipStream_t st = h->stream;
    if (h->form == kEspFormTree) {      // scores from s0 (after the seeds); pick k: the Sigma0 row, then column r + k of the history
        ST_TRY(esp_tree_prepare(h, K));
        const EspTreeState* t = h->tr;
        const EspTreeView T = t->view(h->n);
        return esp_select_run(h, nb, ks, [&](const EspView& V, int P) { k_esp_tree_restart<<<P, kBlock, 0, st>>>(V, t->s0); },
                              [&](const EspView& V, int k) {
                                  k_esp_tree_row<false><<<rg, kBlock, 0, st>>>(V, T, t->zrow, 0);
                                  esp_free_z<true>(h, V, t->zrow, t->seeds + k, k);
                                  return t->seeds + k;
                              }, order_out, gain_out, t_ms_out);
    }
    if (h->form == kEspFormFree) {      // scores from R; pick k: column k of the history
        ST_TRY(esp_history_reserve(h, 0, false, K));
        return esp_select_run(h, nb, ks, [&](const EspView& V, int P) { k_esp_free_scores<<<P, kBlock, 0, st>>>(V, h->R, 1); },
                              [&](const EspView& V, int k) { esp_free_z<false>(h, V, h->R, k, k); return k; }, order_out, gain_out, t_ms_out);
    }
    // dense: scores from Sigma; pick k: column k mod fold of Zb
    return esp_select_run(h, nb, ks, [&](const EspView& V, int P) { k_esp_scores<<<P, kBlock, 0, st>>>(V, h->sig, 1); },
                          [&](const EspView& V, int k) { k_esp_z<<<rg, kBlock, 0, st>>>(V, h->sig, k % h->fold, k); return k % h->fold; },
                          order_out, gain_out, t_ms_out);
}

// machip_esp_weighted_resistances after its checks: on the last run's state (a dense handle folds what is pending) or the fixed graph
inline int esp_resistances(machip_esp* h, double* r_out) {
    if (h->form == kEspFormTree) {      // the tree term and all r + j columns
        ST_TRY(esp_tree_prepare(h, 0));
        k_esp_tree_resist<<<h->grid_m(), kBlock, 0, h->stream>>>(h->view(), h->tr->view(h->n), h->tr->seeds + (h->live ? h->pending : 0));
    } else if (h->form == kEspFormFree) {
        if (h->m && h->live) k_esp_free_resist<<<h->grid_m(), kBlock, 0, h->stream>>>(h->view(), h->R, h->pending);
        else if (h->m) k_esp_free_scores<<<h->grid_m(), kBlock, 0, h->stream>>>(h->view(), h->R, 0);
    } else {
        double* S = h->live ? h->sig : h->sig0;
        if (h->live && h->pending) { h->fold_into(S, h->pending); h->pending = 0; }
        if (h->m) k_esp_scores<<<h->grid_m(), kBlock, 0, h->stream>>>(h->view(), S, 0);
    }
    HIP_TRY(hipGetLastError());
    if (h->m) HIP_TRY(hipMemcpyAsync(r_out, h->s, sizeof(double) * (size_t)h->m, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MACHIP_OK;
}

}  // namespace machip
