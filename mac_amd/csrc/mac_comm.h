// mac_amd/csrc/mac_comm.h -- a MAC handle as a rank of a communicator: the supergradient with its exchange in the three forms (RCCL
// between processes, IPC-mapped buffers between processes, peer copies inside one process), the watchdog around RCCL's first
// contact, the collective eigen-solve of an in-process group (group_fiedler), the guard that releases the peers of a rank that
// leaves early, and the bodies of machip_comm_init*, machip_ipc_export and machip_comm_drop*.  DESIGN sections 4.6 and 7.
#pragma once
#include <unistd.h>

#include <chrono>
#include <functional>
#include <future>
#include <thread>

#include "mac.h"

namespace machip {

#define NCCL_TRY(expr)                                                                       \
    do {                                                                                     \
        ncclResult_t r__ = (expr);                                                           \
        if (r__ != ncclSuccess)                                                              \
            return fail(MACHIP_RCCL_ERROR, std::string(#expr) + ": " + ncclGetErrorString(r__)); \
    } while (0)

// First-contact watchdog (round 4): a call into RCCL that may block for ever -- ncclCommInitRank with a peer that never
// arrives, the first collective on a fabric that is not what was assumed -- runs on a helper thread; the caller waits with a
// limit (MACHIP_RCCL_TIMEOUT_S, default 600) and turns a stall into MACHIP_RCCL_ERROR with the rank in the message instead of
// a hung job.  (A helper that never returns is abandoned with its state: the process is about to report failure anyway.)
inline int run_with_watchdog(const std::function<int()>& fn, double limit_s, const std::string& what) {
    auto state = std::make_shared<std::promise<int>>();
    std::future<int> fut = state->get_future();
    std::thread([state, fn] { int r = MACHIP_HIP_ERROR; try { r = fn(); } catch (...) {} state->set_value(r); }).detach();
    if (fut.wait_for(std::chrono::duration<double>(limit_s)) != std::future_status::ready)
        return fail(MACHIP_RCCL_ERROR, what + " did not return within " + std::to_string((int)limit_s) + " s (a peer rank is missing, or the fabric / bootstrap interface is not reachable; MACHIP_RCCL_TIMEOUT_S raises the limit)");
    return fut.get();
}
inline double rccl_timeout_s() { const Options& opt = default_options(); const int t = OPT(rccl_timeout_s, 600); return t > 0 ? (double)t : 600.0; }

// What belonging to a communicator of nranks means for the handle's candidates: its rank, and the gathered vector's padded length
inline void join_ranks(machip_problem* p, int rank, int nranks) {
    long lo, hi, shard;
    shard_plan(p->m, nranks, rank, &lo, &hi, &shard);
    p->m_pad = shard * nranks;   // <= m + 63 < allocation slack
    p->rank = rank; p->nranks = nranks;
}
inline void leave_ranks(machip_problem* p) { p->rank = 0; p->nranks = 1; p->m_pad = p->m; }

// the current device may write the peer's memory (ranks on distinct devices; enabled before is as good as enabled now)
inline int enable_peer(int peer_device) {
    const hipError_t e = hipDeviceEnablePeerAccess(peer_device, 0);
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail(MACHIP_HIP_ERROR, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
    (void)hipGetLastError();
    return MACHIP_OK;
}

inline int local_allgather(machip_problem* p, long shard) {
    LocalGroup& G = *p->lgroup;
    HIP_TRY(hipStreamSynchronize(p->stream));                 // my shard is in my buffer
    if (!G.barrier()) return fail(MACHIP_RCCL_ERROR, "in-process communicator was shut down by another rank");
    for (int r = 0; r < G.nranks; ++r)
        if (r != p->rank)
            HIP_TRY(hipMemcpyAsync(p->g + shard * r, G.g[(size_t)r] + shard * r, sizeof(double) * (size_t)shard,
                                   hipMemcpyDeviceToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (!G.barrier()) return fail(MACHIP_RCCL_ERROR, "in-process communicator was shut down by another rank");   // nobody overwrites a shard a peer is still reading
    return MACHIP_OK;
}

// the FIRST collective of a communicator is awaited with a limit: a fabric that cannot carry it must surface as an
// error naming the rank, not as a job that never ends (later collectives are not polled)
inline int first_collective_wait(machip_problem* p) {
    p->first_collective_pending = false;
    const auto t0 = std::chrono::steady_clock::now();
    const double lim = rccl_timeout_s();
    for (;;) {
        const hipError_t q = hipStreamQuery(p->stream);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) return fail(MACHIP_HIP_ERROR, std::string("first ncclAllGather: ") + hipGetErrorString(q));
        ncclResult_t ar = ncclSuccess;
        if (ncclCommGetAsyncError(p->comm, &ar) == ncclSuccess && ar != ncclSuccess && ar != ncclInProgress)
            return fail(MACHIP_RCCL_ERROR, std::string("first ncclAllGather failed asynchronously: ") + ncclGetErrorString(ar));
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > lim) {
            (void)ncclCommAbort(p->comm);
            p->comm = nullptr;
            return fail(MACHIP_RCCL_ERROR, "first ncclAllGather of rank " + std::to_string(p->rank) + " of " + std::to_string(p->nranks) +
                        " did not complete within " + std::to_string((int)lim) + " s: communicator aborted");
        }
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    return MACHIP_OK;
}

// fuse_k >= 0 (single rank, long candidate lists): the first digit pass of the top-fuse_k select that follows is counted by the
// gradient kernel itself (k_grad<true>; *fused tells the caller so)
inline int compute_gradient(machip_problem* p, bool have_vec_now = false, long fuse_k = -1, bool* fused = nullptr) {
    const Options& opt = p->sol.opt;
    if (!p->have_vec && !have_vec_now) return fail(MACHIP_BAD_ARG, "no Fiedler vector on the device: call machip_fiedler first");
    const long m = p->m;
    long lo = 0, hi = m, shard = m;
    if (p->nranks > 1) shard_plan(m, p->nranks, p->rank, &lo, &hi, &shard);
    const bool ipc_gather = p->nranks > 1 && !p->comm && p->ipcg;     // no RCCL communicator (ranks sharing a GPU): shards by peer writes
    // IPC gather: my shard is written into every peer's gradient -- not before every peer is done with its gradient of the
    // previous call.  Channel 3 is that handshake: "I have arrived here" (everything this stream did with g before is complete),
    // then wait until every peer has arrived too.  Without an eigen-solve that is partitioned between the ranks nothing else
    // orders a fast rank against a slow one (round-4 advisor finding).
    if (ipc_gather) {
        k_ipc_pubwait<<<1, 64, 0, p->stream>>>(p->ipcg->view, 3);
    }
    const bool timed = p->nranks > 1;      // (communicators only: three event records per iteration)
    if (timed) {
        if (!p->ev_g0) { HIP_TRY(hipEventCreate(&p->ev_g0)); HIP_TRY(hipEventCreate(&p->ev_g1)); HIP_TRY(hipEventCreate(&p->ev_g2)); }
        p->ev_g_valid = false;
        HIP_TRY(hipEventRecord(p->ev_g0, p->stream));
    }
    if (hi > lo) {
        const int grid = (int)std::min<long>(kMaxGrid * 4, (hi - lo + kBlock - 1) / kBlock);
        PeerVecs all;
        if (ipc_gather) { all.n = p->ipcg->nranks; for (int q = 0; q < all.n; ++q) all.v[q] = p->ipcg->g[q]; }
        const bool fuse = fuse_k > 0 && p->nranks <= 1 && m > kSelSmallMax && OPT(sel_fuse, 1) != 0;
        if (fused) *fused = fuse;
        if (fuse) {
            k_sel_init<<<1, 1024, 0, p->stream>>>(p->sel, (long long)std::min(fuse_k, m), p->hist, (6 + kSelRep) * kBins);
            k_grad<true><<<grid, kBlock, 0, p->stream>>>(p->ci, p->cj, p->cw, p->sol.yvec, lo, hi, p->g, all, p->hist + 6 * kBins);
        } else k_grad<false><<<grid, kBlock, 0, p->stream>>>(p->ci, p->cj, p->cw, p->sol.yvec, lo, hi, p->g, all);
        HIP_TRY(hipGetLastError());
    }
    if (timed) HIP_TRY(hipEventRecord(p->ev_g1, p->stream));
    if (ipc_gather) {
        k_ipc_pubwait<<<1, 64, 0, p->stream>>>(p->ipcg->view, 2);
        HIP_TRY(hipGetLastError());
    } else if (p->nranks > 1) {
        if (p->comm) {
            NCCL_TRY(ncclAllGather(p->g + shard * p->rank, p->g, (size_t)shard, ncclDouble, p->comm, p->stream));
            if (p->first_collective_pending) ST_TRY(first_collective_wait(p));
        }
        else if (p->lgroup) { const int st = local_allgather(p, shard); if (st != MACHIP_OK) { p->lgroup->abort(); return st; } }
        else return fail(MACHIP_BAD_ARG, "nranks > 1 without a communicator");
    }
    if (timed) { HIP_TRY(hipEventRecord(p->ev_g2, p->stream)); p->ev_g_valid = true; }
    return MACHIP_OK;
}

// Collective eigen-solve of an in-process communicator whose step is row-partitioned: every rank has assembled the same
// L(x); rank 0's solver drives all ranks' streams (solver_shard.h, ShardGroup) and hands lambda_2, the statistics and the
// Fiedler vector to the peers.
inline int group_fiedler(machip_problem* p, double tol, int max_steps, int warm_start, double* lambda2, machip_solve_stats* stats) {
    LocalGroup& G = *p->lgroup;
    if (!G.barrier()) return fail(MACHIP_RCCL_ERROR, "in-process communicator was shut down by another rank");   // everyone's L(x) is assembled
    if (p->rank == 0) {
        for (int r = 0; r < G.nranks; ++r) {
            machip_problem* q = G.members[(size_t)r];
            ShardRank& k = G.sg.rk[(size_t)r];
            k.device = q->device; k.stream = q->stream; k.Z0 = q->sol.Z0; k.Z1 = q->sol.Z1; k.part = q->sol.part; k.V = q->sol.V;
            k.ypart = q->sol.ypart; k.sdev = q->sol.sdev; k.yvec = q->sol.yvec; k.A = q->csr();
        }
        machip_solve_stats local;
        memset(&local, 0, sizeof(local));
        p->sol.shard = &G.sg;
        int st = run_fiedler(p, tol, max_steps, nullptr, warm_start, &G.lead_lam, &local);
        p->sol.shard = nullptr;
        if (completed(st)) {
            const std::string keep = g_err;
            for (int r = 1; r < G.nranks && completed(st); ++r)
                if (hipMemcpyAsync(G.sg.rk[(size_t)r].yvec, p->sol.yvec, sizeof(double) * (size_t)p->n, hipMemcpyDeviceToDevice, p->stream) != hipSuccess)
                    st = fail(MACHIP_HIP_ERROR, "copy of the Fiedler vector to a peer failed");
            if (hipStreamSynchronize(p->stream) != hipSuccess) st = fail(MACHIP_HIP_ERROR, "stream error after the row-partitioned solve");
            else g_err = keep;
        }
        G.lead_status = st; G.lead_stats = local; G.lead_err = g_err;
    }
    if (!G.barrier()) return fail(MACHIP_RCCL_ERROR, "in-process communicator was shut down by another rank");
    const int st = G.lead_status;
    *lambda2 = G.lead_lam;
    if (stats) { *stats = G.lead_stats; stats->support = p->support; }
    if (p->rank != 0) {
        g_err = G.lead_err;
        p->have_vec = completed(st);
    }
    return st;
}

// Collective entry points of an in-process communicator: whatever makes a rank leave early (assembly, eigen-solve,
// a HIP error) must release the peers waiting in the group's barrier instead of leaving them blocked.
struct GroupGuard {
    machip_problem* p;
    bool ok = false;
    ~GroupGuard() {
        if (!ok && p && p->lgroup) p->lgroup->abort();
        if (!ok && p && p->ipcg) ipc_abort(p);
    }
};

// machip_gradient after its handle check: a collective entry point, so under the guard
inline int gradient(machip_problem* p, double* g_out) {
    GroupGuard guard{p};
    HIP_TRY(hipSetDevice(p->device));
    if (!p->have_vec) { guard.ok = true; return fail(MACHIP_BAD_ARG, "no Fiedler vector on the device: call machip_fiedler first"); }   // (argument error before any barrier: the group stays usable)
    ST_TRY(compute_gradient(p));
    if (g_out) HIP_TRY(hipMemcpyAsync(g_out, p->g, sizeof(double) * (size_t)p->m, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    guard.ok = true;
    return MACHIP_OK;
}

// machip_comm_init after its checks, on the handle's device: ncclCommInitRank under the watchdog
inline int comm_init(machip_problem* p, int rank, int nranks, const void* id128) {
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    {
        const int dev = p->device;
        auto comm_out = std::make_shared<ncclComm_t>(nullptr);
        auto err_out = std::make_shared<std::string>();
        const int st = run_with_watchdog([=]() -> int {
            if (hipSetDevice(dev) != hipSuccess) { *err_out = "hipSetDevice failed"; return MACHIP_HIP_ERROR; }
            const ncclResult_t r = ncclCommInitRank(comm_out.get(), nranks, id, rank);
            if (r != ncclSuccess) { *err_out = std::string("ncclCommInitRank: ") + ncclGetErrorString(r); return MACHIP_RCCL_ERROR; }
            return MACHIP_OK;
        }, rccl_timeout_s(), "ncclCommInitRank (rank " + std::to_string(rank) + " of " + std::to_string(nranks) + ")");
        if (st != MACHIP_OK) return err_out->empty() ? st : fail((machip_status)st, *err_out);
        p->comm = *comm_out;
    }
    p->first_collective_pending = true;
    join_ranks(p, rank, nranks);
    return MACHIP_OK;
}

// ---- communicator between processes with a row-partitioned eigen-solve (round 4) ----
// Blob a rank hands to its peers: IPC handles of its record buffers, partial sums, Ritz staging vector, gradient and flag words.
struct IpcBlob {
    unsigned long long magic;
    int n; long m; int pid; int device;
    hipIpcMemHandle_t Z0, Z1, part, yraw, g, flags;
};
constexpr unsigned long long kIpcMagic = 0x6d61636869706331ull;
constexpr size_t kIpcFlagWords = (size_t)kIpcChannels * kMaxPeers + kIpcChannels + 8;

inline int ipc_export(machip_problem* p, void* blob) {
    auto G = std::make_unique<IpcGroup>();
    ST_TRY(dev_alloc(&G->flags_mem, kIpcFlagWords));
    HIP_TRY(hipMemsetAsync(G->flags_mem, 0, sizeof(unsigned long long) * kIpcFlagWords, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    HIP_TRY(hipHostMalloc((void**)&G->h_err, 64, hipHostMallocMapped));
    *G->h_err = 0;
    IpcBlob b;
    memset(&b, 0, sizeof(b));
    b.magic = kIpcMagic; b.n = p->n; b.m = p->m; b.pid = (int)getpid(); b.device = p->device;
    HIP_TRY(hipIpcGetMemHandle(&b.Z0, p->sol.Z0)); HIP_TRY(hipIpcGetMemHandle(&b.Z1, p->sol.Z1));
    HIP_TRY(hipIpcGetMemHandle(&b.part, p->sol.part)); HIP_TRY(hipIpcGetMemHandle(&b.yraw, p->sol.y_raw));
    HIP_TRY(hipIpcGetMemHandle(&b.g, p->g)); HIP_TRY(hipIpcGetMemHandle(&b.flags, G->flags_mem));
    memcpy(blob, &b, sizeof(b));
    p->ipcg = std::move(G);
    return MACHIP_OK;
}

// machip_comm_init_ipc after its argument checks, on the handle's device
inline int comm_init_ipc(machip_problem* p, int rank, int nranks, const void* blobs, double timeout_s) {
    IpcGroup& G = *p->ipcg;
    const IpcBlob* B = static_cast<const IpcBlob*>(blobs);
    for (int q = 0; q < nranks; ++q)
        if (B[q].magic != kIpcMagic || B[q].n != p->n || B[q].m != p->m) return fail(MACHIP_BAD_ARG, "machip_comm_init_ipc: blob of a different problem / library");
    if (B[rank].pid != (int)getpid()) return fail(MACHIP_BAD_ARG, "machip_comm_init_ipc: blob[rank] is not this process's");
    auto open = [&](const hipIpcMemHandle_t& h, void** out, int peer_device) -> int {
        if (peer_device != p->device) {     // distinct devices: the peer's memory is reached over xGMI
            int can = 0;
            HIP_TRY(hipDeviceCanAccessPeer(&can, p->device, peer_device));
            if (!can) return fail(MACHIP_RCCL_ERROR, "machip_comm_init_ipc: no peer access between the ranks' devices");
            ST_TRY(enable_peer(peer_device));
        }
        const hipError_t e = hipIpcOpenMemHandle(out, h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(MACHIP_RCCL_ERROR, std::string("hipIpcOpenMemHandle: ") + hipGetErrorString(e) + " (HSA_ENABLE_IPC_MODE_LEGACY=0 set?)"); }
        G.opened.push_back(*out);
        return MACHIP_OK;
    };
    // (a failure below leaves a half-mapped group behind: it is dropped -- mappings closed by ~IpcGroup -- and a retry starts from
    // machip_ipc_export again)
    struct Rollback { machip_problem* p; bool ok = false; ~Rollback() { if (!ok) p->ipcg.reset(); } } rollback{p};
    for (int q = 0; q < nranks; ++q) {
        if (q == rank) {
            G.Z0[q] = p->sol.Z0; G.Z1[q] = p->sol.Z1; G.part[q] = p->sol.part; G.yraw[q] = p->sol.y_raw; G.g[q] = p->g;
            G.view.peer_flags[q] = G.flags_mem;
            continue;
        }
        void* t = nullptr;
        ST_TRY(open(B[q].Z0, &G.Z0[q], B[q].device)); ST_TRY(open(B[q].Z1, &G.Z1[q], B[q].device));
        ST_TRY(open(B[q].part, &t, B[q].device)); G.part[q] = (double*)t;
        ST_TRY(open(B[q].yraw, &t, B[q].device)); G.yraw[q] = (double*)t;
        ST_TRY(open(B[q].g, &t, B[q].device)); G.g[q] = (double*)t;
        ST_TRY(open(B[q].flags, &t, B[q].device)); G.view.peer_flags[q] = (unsigned long long*)t;
    }
    G.nranks = nranks; G.rank = rank;
    G.view.n = nranks; G.view.rank = rank;
    G.view.flags = G.flags_mem;
    G.view.done = G.flags_mem + (size_t)kIpcChannels * kMaxPeers;
    HIP_TRY(hipHostGetDevicePointer((void**)&G.view.err, G.h_err, 0));
    if (!(timeout_s > 0.0)) timeout_s = 10.0;
    G.view.timeout_ticks = (long long)(timeout_s * 1e8);
    join_ranks(p, rank, nranks);
    if (p->sol.opt.get(kOpt_shard_eig, 1) != 0) p->sol.ipc = &G;      // (0: the eigen-solve stays replicated, only the gradient is exchanged)
    rollback.ok = true;
    return MACHIP_OK;
}

// machip_comm_init_local after its checks of the handles
inline int comm_init_local(machip_problem** handles, int nranks) {
    auto G = std::make_shared<LocalGroup>();
    G->nranks = nranks;
    for (int r = 0; r < nranks; ++r) G->g.push_back(handles[r]->g);
    // row-partitioned eigen-solve (MACHIP_SHARD_EIG=0: every rank runs the whole solve itself, as in round 2)
    G->shard_eig = nranks > 1 && nranks <= kMaxPeers && handles[0]->sol.opt.get(kOpt_shard_eig, 1) != 0;
    if (G->shard_eig) {
        G->sg.rk.resize((size_t)nranks);
        for (int r = 0; r < nranks; ++r) {
            G->members.push_back(handles[r]);
            HIP_TRY(hipSetDevice(handles[r]->device));
            for (hipEvent_t& e : G->sg.rk[(size_t)r].ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            if (handles[r]->device != handles[0]->device) G->sg.same_device = false;
            for (int q = 0; q < nranks; ++q)          // peers write each other's operand copies
                if (handles[q]->device != handles[r]->device) ST_TRY(enable_peer(handles[q]->device));
        }
        HIP_TRY(hipSetDevice(handles[0]->device));
        HIP_TRY(hipEventCreateWithFlags(&G->sg.fork, hipEventDisableTiming));
    }
    for (int r = 0; r < nranks; ++r) {
        join_ranks(handles[r], r, nranks);
        handles[r]->lgroup = G;
    }
    return MACHIP_OK;
}

// machip_comm_drop / machip_comm_drop_ipc after their checks, on the handle's device
inline int comm_drop(machip_problem* p) {
    (void)hipStreamSynchronize(p->stream);
    if (p->ipcg) { p->sol.ipc = nullptr; p->ipcg.reset(); }
    if (p->comm) { (void)ncclCommAbort(p->comm); p->comm = nullptr; }     // (abort, not destroy: the peers may never have arrived)
    p->first_collective_pending = false; p->ev_g_valid = false;
    leave_ranks(p);
    return MACHIP_OK;
}

inline int comm_drop_ipc(machip_problem* p) {
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->sol.ipc = nullptr;
    p->ipcg.reset();
    // (an RCCL communicator attached before the IPC leg stays in charge of the gradient shards: rank, size and padding are ITS values --
    // advisor finding on round 5: the reset below used to turn such a handle into a replicated one with a dangling communicator)
    if (!p->comm) leave_ranks(p);
    return MACHIP_OK;
}

}  // namespace machip
