// ---------------------------------------------------------------------------------------------
// RCCL: one communicator per context over world_size ranks (one process per GPU).  Data-path
// collectives per MD step: the all-gather of the position slabs and, for Newton-3
// block pairs (N > 65,536), the reduce-scatter of the per-rank dense partial forces; output
// steps all-reduce a few scalars, the KDE bins and the per-ion file columns.
// ---------------------------------------------------------------------------------------------

#include <rccl/rccl.h>

#include "mdqt_ctx.hpp"

using namespace mdqt;

extern "C" int mdqt_comm_unique_id(void* out, size_t len) {
    if (!out || len < sizeof(ncclUniqueId)) return set_error("mdqt_comm_unique_id: need %zu bytes", sizeof(ncclUniqueId));
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    memcpy(out, &id, sizeof id);
    return 0;
}

extern "C" int mdqt_comm_init(mdqt_ctx* s, const void* uid, size_t len) {
    if (!s || !uid || len < sizeof(ncclUniqueId)) return set_error("mdqt_comm_init: bad arguments");
    if (s->comm) return set_error("mdqt_comm_init: communicator already initialised");
    ncclUniqueId id;
    memcpy(&id, uid, sizeof id);
    HIPCHK(hipSetDevice(s->dev));
    NCCLCHK(ncclCommInitRank(&s->comm, s->p.world_size, id, s->p.rank));
    return 0;
}

extern "C" int mdqt_comm_size(const mdqt_ctx* s, int* n) {
    if (!s || !n) return set_error("mdqt_comm_size: bad arguments");
    if (s->comm) {
        NCCLCHK(ncclCommCount(s->comm, n));
    } else {
        *n = s->local.empty() ? 1 : (int)s->local.size();
    }
    return 0;
}

// mdqt_destroy's part that needs rccl.h
void mdqt::comm_destroy(mdqt_ctx* s) {
    if (s->comm) (void)ncclCommDestroy(s->comm);
    s->comm = nullptr;
}

extern "C" int mdqt_comm_init_local(mdqt_ctx* const* ctxs, int n) {
    if (!ctxs || n < 1) return set_error("mdqt_comm_init_local: bad arguments");
    for (int r = 0; r < n; ++r) {
        if (!ctxs[r] || ctxs[r]->p.world_size != n || ctxs[r]->p.rank != r)
            return set_error("mdqt_comm_init_local: context %d is not rank %d of %d", r, r, n);
        if (ctxs[r]->S != ctxs[0]->S || ctxs[r]->N != ctxs[0]->N)
            return set_error("mdqt_comm_init_local: contexts disagree on N");
    }
    for (int r = 0; r < n; ++r) ctxs[r]->local.assign(ctxs, ctxs + n);
    return 0;
}

extern "C" int mdqt_allgather_positions(mdqt_ctx* s) {
    if (!s) return set_error("NULL context");
    if (s->p.world_size == 1) return 0;
    const size_t cnt = (size_t)3 * s->S;
    if (!s->comm && !s->local.empty()) {
        // in-process group: push this rank's slab into every peer (callers run the ranks in
        // lockstep: every rank pushes before any rank computes forces)
        HIPCHK(hipSetDevice(s->dev));
        HIPCHK(hipStreamSynchronize(s->stream));
        for (mdqt_ctx* q : s->local) {
            if (q == s) continue;
            // on the PEER's stream: ordered before the peer's next force launch (a plain
            // hipMemcpyPeer is asynchronous for device-to-device copies and races with it)
            HIPCHK(hipMemcpyPeerAsync(q->dR + (size_t)s->p.rank * cnt, q->dev, s->dR + (size_t)s->p.rank * cnt,
                                      s->dev, cnt * sizeof(double), q->stream));
        }
        return 0;
    }
    if (!s->comm) return set_error("mdqt_allgather_positions: no communicator (mdqt_comm_init)");
    HIPCHK(hipSetDevice(s->dev));
    const bool bd = force_timed_next(s) && s->use_n3b;   // (the breakdown's first stage)
    for (hipEvent_t& e : s->bd_ag)
        if (e) { s->bdfree.push_back(e); e = nullptr; }
    if (bd) s->bd_ag[0] = bd_event(s);
    NCCLCHK(ncclAllGather(s->dR + (size_t)s->p.rank * cnt, s->dR, cnt, ncclDouble, s->comm, s->stream));
    if (bd) s->bd_ag[1] = bd_event(s);
    return 0;
}

extern "C" int mdqt_allreduce_sum(mdqt_ctx* s, double* buf, size_t n) {
    if (!s || (!buf && n)) return set_error("mdqt_allreduce_sum: bad arguments");
    if (s->p.world_size == 1 || n == 0) return 0;
    if (!s->comm) return set_error("mdqt_allreduce_sum: no communicator (mdqt_comm_init)");
    HIPCHK(hipSetDevice(s->dev));
    HIPCHK(s->dComm.reserve(n));
    HIPCHK(hipMemcpyAsync(s->dComm, buf, n * sizeof(double), hipMemcpyHostToDevice, s->stream));
    NCCLCHK(ncclAllReduce(s->dComm, s->dComm, n, ncclDouble, ncclSum, s->comm, s->stream));
    HIPCHK(hipMemcpyAsync(buf, s->dComm, n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return 0;
}

// in-process rank group: the ranks' per-tile sums summed in rank order and handed to every rank,
// which then enforces on its own dense partial — the ncclAllReduce of a real group (mdqt_forces)
static int local_tail(mdqt_ctx* s) {
    bool any = false;
    for (mdqt_ctx* q : s->local) any = any || q->tail_pending;
    if (!any) return 0;
    const int T = s->tail_args.T, T4 = 4 * T;                 // per-sub-tile sums
    std::vector<double> sum((size_t)T4, 0.), h((size_t)T4);
    for (mdqt_ctx* q : s->local) {
        if (!q->tail_pending || q->tail_args.T != T) return set_error("local group: rank %d has no tail sums", q->p.rank);
        HIPCHK(hipSetDevice(q->dev));
        HIPCHK(hipMemcpyAsync(h.data(), q->tail_args.tailb, (size_t)T4 * sizeof(double), hipMemcpyDeviceToHost, q->stream));
        HIPCHK(hipStreamSynchronize(q->stream));
        for (int t = 0; t < T4; ++t) sum[t] = sum[t] + h[t];
    }
    for (mdqt_ctx* q : s->local) {
        HIPCHK(hipSetDevice(q->dev));
        HIPCHK(hipMemcpyAsync(q->tail_args.tailb, sum.data(), (size_t)T4 * sizeof(double), hipMemcpyHostToDevice, q->stream));
        if (tail_enforce(q, q->tail_args, q->dFr)) return -1;
        HIPCHK(hipStreamSynchronize(q->stream));
        q->tail_pending = false;
    }
    for (mdqt_ctx* q : s->local) {                 // every rank reacts here, at the same point
        HIPCHK(hipSetDevice(q->dev));
        if (tail_check(q)) return -1;
    }
    HIPCHK(hipSetDevice(s->dev));
    return 0;
}

// in-process rank group with block-pair Newton-3: F of this rank = the ranks' dense partials
// summed in rank order (RCCL's reduce-scatter in a real group).  Peers' force launches are
// complete: callers step the group in lockstep (all forces before any substeps).
int mdqt::local_reduce(mdqt_ctx* s) {
    if (!s->rs_pending) return 0;
    if (local_tail(s)) return -1;
    const int W = s->p.world_size;
    std::vector<const double*> h(W, nullptr);
    for (mdqt_ctx* q : s->local) {
        if (!q->dFr) return set_error("local_reduce: rank %d has no partial forces", q->p.rank);
        h[q->p.rank] = q->dFr;
        HIPCHK(hipSetDevice(q->dev));
        HIPCHK(hipStreamSynchronize(q->stream));
    }
    HIPCHK(hipSetDevice(s->dev));
    if (!s->dPeerParts) HIPCHK(s->dPeerParts.alloc((size_t)W));
    HIPCHK(hipMemcpy(s->dPeerParts, h.data(), W * sizeof(double*), hipMemcpyHostToDevice));
    HIPCHK(launch_sum_rank_chunks(s->dPeerParts, W, s->p.rank, s->S, s->dF, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    s->rs_pending = false;
    return 0;
}
