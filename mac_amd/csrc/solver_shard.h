// solver_shard.h -- the row-partitioned eigen-solves: a chunk of Lanczos steps, the start of a sequence and the Ritz vector with
// the rows spread over the ranks of one process (ShardGroup: streams ordered by events) or over processes (IpcGroup: each rank
// launches its own workgroups, ordered by flag words in device memory).  Members of Solver (solver.h).
#pragma once
#include "solver.h"

namespace machip {

// ---- row-partitioned chunk: per step one launch per rank, ordered by events (ShardGroup) ----
inline void Solver::shard_split(const SpmvPlan& pl) {
    const int R = (int)shard->rk.size();
    for (int r = 0; r < R; ++r) { shard->rk[(size_t)r].g0 = (int)((long)pl.grid * r / R); shard->rk[(size_t)r].g1 = (int)((long)pl.grid * (r + 1) / R); }
}
inline PeerSet Solver::shard_peers(const ShardRank& me, const SpmvPlan& pl) const {
    PeerSet PS;
    PS.n = (int)shard->rk.size(); PS.first = me.g0; PS.total = pl.grid;
    for (int q = 0; q < PS.n; ++q) { PS.Z0[q] = shard->rk[(size_t)q].Z0; PS.Z1[q] = shard->rk[(size_t)q].Z1; PS.part[q] = shard->rk[(size_t)q].part; }
    return PS;
}
inline void Solver::launch_chunk_sharded(const SpmvPlan& pl, int steps) {
    ShardGroup& G = *shard;
    const int R = (int)G.rk.size();
    shard_split(pl);
    (void)hipEventRecord(G.fork, stream);
    for (int q = 1; q < R; ++q) (void)hipStreamWaitEvent(G.rk[(size_t)q].stream, G.fork, 0);
    for (int s = 0; s < steps; ++s) {
        for (int r = 0; r < R; ++r) {
            ShardRank& me = G.rk[(size_t)r];
            if (s > 0) for (int q = 0; q < R; ++q) if (q != r) (void)hipStreamWaitEvent(me.stream, G.rk[(size_t)q].ev[(s - 1) & 1], 0);
            if (me.g1 > me.g0) {
                if (!G.same_device) (void)hipSetDevice(me.device);
                PipeView L = pview(pl);                       // the leader's counters / tridiagonal records ...
                L.Z0 = me.Z0; L.Z1 = me.Z1; L.V = me.V; L.part = me.part;   // ... this rank's operand, basis rows and partial sums
                launch_pipe_shard(pl, me.stream, me.A, L, s, shard_peers(me, pl), me.g1 - me.g0);
            }
            (void)hipEventRecord(me.ev[s & 1], me.stream);
        }
    }
    for (int q = 1; q < R; ++q) (void)hipStreamWaitEvent(stream, G.rk[(size_t)q].ev[(steps - 1) & 1], 0);
    if (!G.same_device) (void)hipSetDevice(G.rk[0].device);
    k_pipe_tail<<<1, 64, 0, stream>>>(pview(pl), steps);
}
// ---- row-partitioned chunk between processes: my workgroups only, ordered by flags in device memory (IpcGroup) ----
inline PeerSet Solver::ipc_peers(const SpmvPlan& pl) const {
    PeerSet PS;
    PS.n = ipc->nranks; PS.first = ipc->g0; PS.total = pl.grid;
    for (int q = 0; q < PS.n; ++q) { PS.Z0[q] = ipc->Z0[q]; PS.Z1[q] = ipc->Z1[q]; PS.part[q] = ipc->part[q]; }
    return PS;
}
inline void Solver::ipc_split(const SpmvPlan& pl) {
    ipc->g0 = (int)((long)pl.grid * ipc->rank / ipc->nranks);
    ipc->g1 = (int)((long)pl.grid * (ipc->rank + 1) / ipc->nranks);
}
inline void Solver::launch_chunk_ipc(const CsrView& A, const SpmvPlan& pl, int steps) {
    ipc_split(pl);
    const PipeView L = pview(pl);
    const PeerSet PS = ipc_peers(pl);
    k_ipc_wait<<<1, 64, 0, stream>>>(ipc->view, 0);              // (whatever the previous chunk / the sequence start left pending)
    for (int s = 0; s < steps; ++s) {
        launch_pipe_shard(pl, stream, A, L, s, PS, ipc->g1 - ipc->g0);
        k_ipc_pubwait<<<1, 64, 0, stream>>>(ipc->view, 0);       // mine delivered; every peer has delivered its records / partial sums of this step
    }
    k_pipe_tail<<<1, 64, 0, stream>>>(L, steps);
}
// The same for the column-panel step of the shifted recurrence (round 6): rank r owns the row kernel's workgroups [g0, g1) -- rows
// [g0 B, g1 B) -- and launches the matrix kernel for the row blocks those rows lie in, all panels each (a block that straddles two ranks
// is multiplied by both: 1 of 42 at configs[3]); the row kernel writes its rows of the next operand and its six sums into every rank's
// copy.  Cells, row sums, partial sums and their order are those of the un-partitioned launch: bit-identical.
inline void Solver::launch_chunk_ipc_pan(const SpmvPlan& pl, int steps, int j0) {
    ipc_split(pl);
    const PipeView L = pview(pl);
    const PeerSet PS = ipc_peers(pl);
    if (!d_ps) { if (dev_alloc(&d_ps, 1) != MACHIP_OK) return; }
    if (memcmp(&PS, &h_ps, sizeof(PeerSet)) != 0) {       // (the row kernel reads its peer set from device memory: panel_u.h)
        h_ps = PS;
        (void)hipMemcpyAsync(d_ps, &h_ps, sizeof(PeerSet), hipMemcpyHostToDevice, stream);
    }
    const int Rb = 64 * pan.NTB;
    const long r_lo = (long)ipc->g0 * pan.block2, r_hi = std::min<long>((long)ipc->g1 * pan.block2, (long)n);
    const int b0 = (int)(r_lo / Rb), b1 = (int)((r_hi + Rb - 1) / Rb);
    const int g1m = std::max(1, b1 - b0) * pan.NP, gf = ipc->g1 - ipc->g0;
    k_ipc_wait<<<1, 64, 0, stream>>>(ipc->view, 0);              // (whatever the previous chunk / the sequence start left pending)
    for (int s = 0; s < steps; ++s) {
        const int jhost = j0 >= 0 ? j0 + s : -1;
        with_pan_mul8_shape(pan.LPT, pan.TWT, [&](auto LP, auto TW) { k_pan_mul8<SV(LP), SV(TW), double><<<g1m, kPanThreads, 0, stream>>>(PAN_MUL8_ARGS_AT(panv, pu, L, s, b0)); });
        with_finu_shape(pan, [&](auto B, auto M) { k_pan_finu<SV(B), SV(M), true><<<gf, SV(B), 0, stream>>>(PAN_FINU_ARGS(panv, pu, L, s, jhost), d_ps, PS.first, PS.total); });
        k_ipc_pubwait<<<1, 64, 0, stream>>>(ipc->view, 0);       // mine delivered; every peer has delivered its operand rows / partial sums of this step
    }
    k_pipe_tail<<<1, 64, 0, stream>>>(L, steps);
}
// y_raw = V[:, :J] s: my rows of the basis -> my rows of EVERY rank's y_raw, then everybody holds the whole vector
inline int Solver::ipc_ritz(const SpmvPlan& pl, int J, const double* s_host) {
    const int g2 = vgrid();
    const int KS = std::max(1, std::min(ks_max, J / 8));
    memcpy(h_pin, s_host, sizeof(double) * (size_t)J);
    HIP_TRY(hipMemcpyAsync(sdev, h_pin, sizeof(double) * (size_t)J, hipMemcpyHostToDevice, stream));
    ipc_split(pl);
    RowOwner own; own.gpb = pl.variant == kPanel ? pl.block : pipe_gpb(pl); own.gtot = pl.grid; own.g0 = ipc->g0; own.g1 = ipc->g1;      // (panel form: the row kernel's workgroups own the rows)
    PeerVecs all; all.n = ipc->nranks;
    for (int q = 0; q < all.n; ++q) all.v[q] = ipc->yraw[q];
    k_ritz_partial<<<dim3(g2, KS), kBlock, 0, stream>>>(V, n, J, sdev, ypart, own);
    k_ritz_own_rows<<<g2, kBlock, 0, stream>>>(ypart, n, KS, y_raw, own, all);
    k_ipc_pubwait<<<1, 64, 0, stream>>>(ipc->view, 1);
    k_vec_sums<<<g2, kBlock, 0, stream>>>(y_raw, n, part_c);
    HIP_TRY(hipGetLastError());
    return MACHIP_OK;
}
inline int Solver::ipc_check_err(const char* where) {
    if (ipc && ipc->h_err && *(volatile int*)ipc->h_err)
        return fail(MACHIP_RCCL_ERROR, std::string("inter-process communicator: ") + (*(volatile int*)ipc->h_err == 2 ? "a peer rank raised abort" : "a peer rank did not deliver within the time limit (stalled or dead)") + " (" + where + ")");
    return MACHIP_OK;
}

// start of a sequence: the leader's k_pipe_init output (records of u, first partial sums) into every rank's copy
inline int Solver::shard_broadcast_init() {
    ShardGroup& G = *shard;
    for (size_t q = 1; q < G.rk.size(); ++q) {
        HIP_TRY(hipMemcpyAsync(G.rk[q].Z0, Z0, sizeof(Z2) * (size_t)n, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipMemcpyAsync(G.rk[q].part, part, sizeof(double) * 2 * kNP * kMaxGrid, hipMemcpyDeviceToDevice, stream));
    }
    return MACHIP_OK;
}
// y_raw = V[:, :J] s with V spread over the ranks by rows; sums of y_raw in part_c (the layout check_vector expects)
inline int Solver::shard_ritz(const SpmvPlan& pl, int J, const double* s_host) {
    ShardGroup& G = *shard;
    const int R = (int)G.rk.size(), g2 = vgrid();
    const int KS = std::max(1, std::min(ks_max, J / 8));
    memcpy(h_pin, s_host, sizeof(double) * (size_t)J);
    shard_split(pl);
    HIP_TRY(hipEventRecord(G.fork, stream));
    for (int r = 0; r < R; ++r) {
        ShardRank& me = G.rk[(size_t)r];
        if (r) HIP_TRY(hipStreamWaitEvent(me.stream, G.fork, 0));
        if (!G.same_device) HIP_TRY(hipSetDevice(me.device));
        HIP_TRY(hipMemcpyAsync(me.sdev, h_pin, sizeof(double) * (size_t)J, hipMemcpyHostToDevice, me.stream));
        RowOwner own; own.gpb = pipe_gpb(pl); own.gtot = pl.grid; own.g0 = me.g0; own.g1 = me.g1;
        k_ritz_partial<<<dim3(g2, KS), kBlock, 0, me.stream>>>(me.V, n, J, me.sdev, me.ypart, own);
        k_ritz_own_rows<<<g2, kBlock, 0, me.stream>>>(me.ypart, n, KS, y_raw, own);
        HIP_TRY(hipEventRecord(me.ev[0], me.stream));
    }
    for (int q = 1; q < R; ++q) HIP_TRY(hipStreamWaitEvent(stream, G.rk[(size_t)q].ev[0], 0));
    if (!G.same_device) HIP_TRY(hipSetDevice(G.rk[0].device));
    k_vec_sums<<<g2, kBlock, 0, stream>>>(y_raw, n, part_c);
    HIP_TRY(hipGetLastError());
    return MACHIP_OK;
}

}  // namespace machip
