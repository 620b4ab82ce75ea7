// rt_gather.cpp — the multi-GPU frame's end: the gather plan for a frame size and world, the gather
// over RCCL (rt_comm_*, rt_gather_shards) and within one process (rt_gather_shards_local), and the
// placement of the gathered shards into the frame.  The only unit that knows RCCL.
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>

#include "rt_host.h"
#include "rt_launch.h"

using namespace rtamd;

namespace {
// A multi-GPU frame's communicator (rt_comm_create): one RCCL rank per process, bound to a context's
// device.  The gather's plan is kept for the frame size last gathered.
struct Comm {
    int ctx = -1, rank = 0, world = 1;
    int device = 0;
    ncclComm_t nc = nullptr;
    GatherPlan plan;
    ~Comm() { if (nc) (void)ncclCommDestroy(nc); }
};
// shared: rt_gather_shards keeps its communicator alive outside the lock (it waits for the other ranks)
std::map<int, std::shared_ptr<Comm>> g_comm;
int g_next_comm = 1;

// (re)build the gather plan for a frame size and world; the root's device list and receive buffer too
int gather_plan(GatherPlan& g, int nx, int ny, int world, bool root) {
    if (g.nx == nx && g.ny == ny && g.world == world && g.root == root) return 0;
    g.nx = -1;
    g.world = world;
    g.root = root;
    g.count.assign(world, 0);
    g.off.assign(world, 0);
    std::vector<uint32_t> all;
    int64_t total = 0;
    for (int r = 0; r < world; ++r) {
        const std::vector<uint32_t> pl = make_pixlist(nx, ny, PixSel{0, ny, r, world});
        g.off[r] = total;
        g.count[r] = (int64_t)pl.size();
        total += g.count[r];
        if (root) all.insert(all.end(), pl.begin(), pl.end());
    }
    if (root) {
        HIPCHK(g.pix.ensure(std::max<size_t>(1, all.size()) * sizeof(uint32_t)));
        if (!all.empty()) HIPCHK(hipMemcpy(g.pix.p, all.data(), all.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIPCHK(g.recv.ensure(std::max<size_t>(1, (size_t)g.others()) * 3 * sizeof(double)));
    }
    g.nx = nx;
    g.ny = ny;
    return 0;
}
// the root's placement: its own compact accumulator, then the received shards, into the y-up frame
int gather_place(const GatherPlan& g, const double* own, double* frame, hipStream_t st) {
    const uint32_t* pix = g.pix.as<const uint32_t>();
    if (g.count[0] > 0) HIPCHK(launch_scatter_pixels(own, pix, (uint32_t)g.count[0], frame, st));
    HIPCHK(launch_scatter_pixels(g.recv.as<const double>(), pix + g.count[0], (uint32_t)g.others(), frame, st));
    return 0;
}
}  // namespace

extern "C" {

// ---- multi-GPU frame: the frame-end gather over RCCL (include/rt.h) ----
#define NCCLCHK(expr)                                                                  \
    do {                                                                               \
        ncclResult_t r_ = (expr);                                                      \
        if (r_ != ncclSuccess) return fail(std::string(#expr) + ": " + ncclGetErrorString(r_)); \
    } while (0)

int rt_comm_unique_id(uint8_t out_id[RT_COMM_ID_BYTES]) {
    if (!out_id) return fail("null out pointer");
    static_assert(sizeof(ncclUniqueId) == RT_COMM_ID_BYTES, "RT_COMM_ID_BYTES is RCCL's unique id size");
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    std::memcpy(out_id, &id, sizeof id);
    return 0;
}

int rt_comm_create(int ctx, const uint8_t unique_id[RT_COMM_ID_BYTES], int rank, int world, int* out_comm) {
    if (!unique_id || !out_comm) return fail("null pointer");
    if (world <= 0 || rank < 0 || rank >= world) return fail("invalid rank / world size");
    int device = 0;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        Context* c = get_ctx(ctx);
        if (!c) return fail("invalid context handle");
        device = c->device;
    }
    HIPCHK(hipSetDevice(device));
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof id);
    auto m = std::make_shared<Comm>();
    m->ctx = ctx; m->rank = rank; m->world = world; m->device = device;
    // collective: returns once every rank has called it (outside the lock: it waits for the other processes)
    NCCLCHK(ncclCommInitRank(&m->nc, world, id, rank));
    std::lock_guard<std::mutex> lk(g_mu);
    const int h = g_next_comm++;
    g_comm[h] = std::move(m);
    *out_comm = h;
    return 0;
}

int rt_comm_destroy(int comm) {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_comm.find(comm);
    if (it == g_comm.end()) return fail("invalid communicator handle");
    Context* c = get_ctx(it->second->ctx);
    if (c) HIPCHK(hipSetDevice(c->device));
    g_comm.erase(it);
    return 0;
}

int rt_gather_shards(int comm, int nx, int ny, const double* accum_compact, double* frame_device, void* stream) {
    if (int rc = check_frame(nx, ny)) return rc;
    std::shared_ptr<Comm> keep;                       // alive through the call, whatever rt_comm_destroy does
    hipStream_t st = (hipStream_t)stream;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_comm.find(comm);
        if (it == g_comm.end()) return fail("invalid communicator handle");
        keep = it->second;
        Context* c = get_ctx(keep->ctx);
        if (!c) return fail("the communicator's context was destroyed");
        if (!st) st = c->stream;                      // (the context must outlive the call: rt.h)
    }
    Comm* m = keep.get();
    HIPCHK(hipSetDevice(m->device));
    if (int rc = gather_plan(m->plan, nx, ny, m->world, m->rank == 0)) return rc;
    const GatherPlan& g = m->plan;
    const int64_t mine = g.count[m->rank];
    if (mine > 0 && !accum_compact) return fail("null compact accumulator");
    if (m->rank == 0 && !frame_device) return fail("rank 0 needs the frame buffer");
    // RCCL has no gather: every other rank sends its compact accumulator (its exact size, no padding) to
    // rank 0, which posts one receive per rank into its buffer at recv_at(r), in one group.
    // The group is always closed, also after a failed call inside it (an open group poisons the thread's
    // later RCCL calls).
    if (m->world > 1) {
        ncclResult_t r0 = ncclGroupStart();
        if (r0 != ncclSuccess) return fail(std::string("ncclGroupStart: ") + ncclGetErrorString(r0));
        ncclResult_t bad = ncclSuccess;
        if (m->rank != 0) {
            if (mine > 0) bad = ncclSend(accum_compact, (size_t)(3 * mine), ncclDouble, 0, m->nc, st);
        } else {
            double* recv = g.recv.as<double>();
            for (int r = 1; r < m->world && bad == ncclSuccess; ++r)
                if (g.count[r] > 0) bad = ncclRecv(recv + g.recv_at(r), (size_t)(3 * g.count[r]), ncclDouble, r, m->nc, st);
        }
        const ncclResult_t end = ncclGroupEnd();
        if (bad != ncclSuccess) return fail(std::string("ncclSend / ncclRecv: ") + ncclGetErrorString(bad));
        if (end != ncclSuccess) return fail(std::string("ncclGroupEnd: ") + ncclGetErrorString(end));
    }
    if (m->rank == 0)                                  // place every shard's pixels into the y-up frame
        if (int rc = gather_place(g, accum_compact, frame_device, st)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int rt_gather_layout(int nx, int ny, int world, int64_t* out_count, int64_t* out_offset) {
    if (int rc = check_frame(nx, ny)) return rc;
    if (world <= 0) return fail("invalid world size");
    if (!out_count || !out_offset) return fail("null out pointer");
    GatherPlan g;
    if (int rc = gather_plan(g, nx, ny, world, false)) return rc;
    for (int r = 0; r < world; ++r) { out_count[r] = g.count[r]; out_offset[r] = g.off[r]; }
    return 0;
}

int rt_gather_shards_local(int ctx, int nx, int ny, int world, const double* const* accum_compact,
                           double* frame_device, void* stream) {
    if (int rc = check_frame(nx, ny)) return rc;
    if (world <= 0) return fail("invalid world size");
    if (!accum_compact || !frame_device) return fail("null pointer");
    LOCK_CTX(c, ctx);
    CTX_STREAM(c, st, stream);
    if (int rc = gather_plan(c->gplan, nx, ny, world, true)) return rc;
    const GatherPlan& g = c->gplan;
    for (int r = 0; r < world; ++r)
        if (g.count[r] > 0 && !accum_compact[r]) return fail("null compact accumulator for shard " + std::to_string(r));
    // what the RCCL gather's receives do: shard r's compact accumulator at recv_at(r)
    double* recv = g.recv.as<double>();
    for (int r = 1; r < world; ++r)
        if (g.count[r] > 0)
            HIPCHK(hipMemcpyAsync(recv + g.recv_at(r), accum_compact[r], (size_t)g.count[r] * 3 * sizeof(double),
                                  hipMemcpyDeviceToDevice, st));
    if (int rc = gather_place(g, accum_compact[0], frame_device, st)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
