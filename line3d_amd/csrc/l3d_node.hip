// l3d_node.hip -- the in-process all-gather of a node handle (l3d_line3d_create_node): W ranks, one per entry of a device list, run as threads
// of one process; rank r's exchange (l3d_exchange_node, the l3d_exchange_fn contract) gathers the W ranks' send slots into ITS recv_block in
// rank order with one launch of k_node_gather, which PULLS: it reads the peers' slots through peer-mapped pointers and writes local memory only.
// Ordering comes from stream events alone (no atomics, flags or spin waits on the device); the host barrier between the steps only makes sure
// that every event a stream waits for has been recorded -- and so everything it waits for queued -- before the wait is issued.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <vector>

#include "../../include/line3d_amd.h"
#include "l3d_node.hpp"

namespace l3d {

namespace {

constexpr int kNodeMaxRanks = 64;
struct NodeSources { const unsigned char* p[kNodeMaxRanks]; };

// recv + q * n <- rank q's slot (n bytes), q = blockIdx.y.  The destination is walked in 16-byte chunks from its first 16-byte boundary: the
// body is one 16-byte load and one 16-byte store per chunk and thread (the source read unaligned when the two pointers differ modulo 16:
// global memory takes unaligned vector loads); the up to 15 bytes in front of the boundary and behind the last chunk go byte by byte.
// Every access stays inside [0, n) of its slot.
__global__ __launch_bounds__(256) void k_node_gather(NodeSources src, unsigned char* __restrict__ recv, unsigned long long n)
{
    const unsigned q = blockIdx.y;
    const unsigned char* __restrict__ s = src.p[q];
    unsigned char* __restrict__ d = recv + (unsigned long long)q * n;
    const unsigned long long mis = (unsigned long long)(reinterpret_cast<uintptr_t>(d) & 15);
    const unsigned long long head = mis ? (16 - mis < n ? 16 - mis : n) : 0;
    const unsigned long long chunks = (n - head) >> 4;
    const unsigned long long tail = head + (chunks << 4);
    if (blockIdx.x == 0 && threadIdx.x < 16) {
        const unsigned t = threadIdx.x;
        if (t < head) d[t] = s[t];
        if (tail + t < n) d[tail + t] = s[tail + t];
    }
    const unsigned char* sb = s + head;
    uint4* db = reinterpret_cast<uint4*>(d + head);
    const unsigned long long stride = (unsigned long long)gridDim.x * 256;
    if ((reinterpret_cast<uintptr_t>(sb) & 15) == 0) {
        const uint4* sv = reinterpret_cast<const uint4*>(sb);
        for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += stride) db[i] = sv[i];
    } else {
        for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += stride) {
            uint4 v;
            __builtin_memcpy(&v, sb + (i << 4), 16);
            db[i] = v;
        }
    }
}

}  // namespace
}  // namespace l3d

// W ranks of one process.  Rank r is known by the stream its exchanges arrive on (l3d_node_comm_bind); the slots it publishes and the two events
// it records per exchange are read by the others only between the two barriers of that exchange.
struct l3d_node_comm {
    int world = 0;
    std::vector<int> devices;
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> send_ev, done_ev;
    std::vector<const void*> send;
    std::vector<size_t> bytes;
    std::vector<long long> calls;                 // exchanges per rank over the communicator's life (only rank r's thread counts calls[r])
    int fail_rank = -1;                           // tests: this rank's exchange number fail_at returns 1 (l3d::node_comm_fail_at)
    long long fail_at = 0;
    double timeout_s = 600.0;                     // a rank that waits this long at a barrier breaks it
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    unsigned long long generation = 0;
    std::atomic<bool> broken{ false };
    int culprit = -1;                             // the rank whose exchange broke the barrier (-1: none, or broken from outside)
};

namespace {

void comm_abort(l3d_node_comm* c, int rank)
{
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->broken) c->culprit = rank;
    c->broken = true;
    c->cv.notify_all();
}

// false: the barrier is broken (an abort, a failed rank, a timeout) -- now and for every later exchange until l3d::node_comm_rearm
bool comm_barrier(l3d_node_comm* c, int rank, int view)
{
    std::unique_lock<std::mutex> lk(c->mu);
    if (c->broken) return false;
    const unsigned long long gen = c->generation;
    if (++c->arrived == c->world) {
        c->arrived = 0;
        ++c->generation;
        c->cv.notify_all();
        return true;
    }
    const bool passed = c->cv.wait_for(lk, std::chrono::duration<double>(c->timeout_s), [&] { return c->generation != gen || c->broken; });
    if (c->generation != gen) return true;
    if (!passed) fprintf(stderr, "[l3d node] rank %d waited %.0f s for the other ranks at exchange %d: the communicator is broken\n", rank, c->timeout_s, view);
    if (!c->broken) c->culprit = rank;
    c->broken = true;
    c->cv.notify_all();
    return false;
}

int rank_of(const l3d_node_comm* c, void* stream)
{
    for (int r = 0; r < c->world; ++r)
        if (c->streams[(size_t)r] == (hipStream_t)stream) return r;
    return -1;
}

}  // namespace

namespace l3d {
void node_comm_rearm(l3d_node_comm* c)
{
    if (!c) return;
    std::lock_guard<std::mutex> lk(c->mu);
    c->arrived = 0;
    c->broken = false;
    c->culprit = -1;
}
int node_comm_culprit(l3d_node_comm* c)
{
    if (!c) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    return c->culprit;
}
void node_comm_fail_at(l3d_node_comm* c, int rank, long long k)
{
    if (!c) return;
    c->fail_rank = k > 0 ? rank : -1;
    c->fail_at = k > 0 ? c->calls[(size_t)std::max(0, std::min(rank, c->world - 1))] + k : 0;
}
}  // namespace l3d

extern "C" {

int l3d_node_comm_create(const int* devices, int n, l3d_node_comm** out)
{
    if (!out) return L3D_ERR_INVALID;
    *out = nullptr;
    if (!devices || n <= 0 || n > l3d::kNodeMaxRanks) return L3D_ERR_INVALID;
    for (int r = 0; r < n; ++r)
        if (devices[r] < 0) return L3D_ERR_INVALID;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return L3D_ERR_NODEVICE;
    for (int r = 0; r < n; ++r)
        if (devices[r] >= count) return L3D_ERR_INVALID;
    int prev = 0;
    (void)hipGetDevice(&prev);
    int rc = L3D_OK;
    // peer access for every pair of distinct devices, both ways: k_node_gather on a rank's device reads every other rank's slot
    std::vector<int> distinct;
    for (int r = 0; r < n; ++r)
        if (std::find(distinct.begin(), distinct.end(), devices[r]) == distinct.end()) distinct.push_back(devices[r]);
    for (int da : distinct)
        for (int db : distinct) {
            if (da == db || rc != L3D_OK) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, da, db) != hipSuccess || !can) {
                fprintf(stderr, "[l3d node] device %d cannot map device %d's memory (peer access refused): no node of these devices\n", da, db);
                rc = L3D_ERR_UNSUPPORTED;
                continue;
            }
            hipError_t e = hipSetDevice(da);
            if (e == hipSuccess) e = hipDeviceEnablePeerAccess(db, 0);
            if (e == hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); e = hipSuccess; }
            if (e != hipSuccess) {
                fprintf(stderr, "[l3d node] enabling peer access from device %d to device %d failed: %s\n", da, db, hipGetErrorString(e));
                rc = L3D_ERR_UNSUPPORTED;
            }
        }
    l3d_node_comm* c = nullptr;
    if (rc == L3D_OK) {
        c = new l3d_node_comm();
        c->world = n;
        c->devices.assign(devices, devices + n);
        c->streams.assign((size_t)n, nullptr);
        c->send_ev.assign((size_t)n, nullptr);
        c->done_ev.assign((size_t)n, nullptr);
        c->send.assign((size_t)n, nullptr);
        c->bytes.assign((size_t)n, 0);
        c->calls.assign((size_t)n, 0);
        for (int r = 0; r < n && rc == L3D_OK; ++r) {
            if (hipSetDevice(devices[r]) != hipSuccess || hipEventCreateWithFlags(&c->send_ev[(size_t)r], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&c->done_ev[(size_t)r], hipEventDisableTiming) != hipSuccess)
                rc = L3D_ERR_HIP;
        }
        if (rc != L3D_OK) { l3d_node_comm_destroy(c); c = nullptr; }
    }
    (void)hipSetDevice(prev);
    *out = c;
    return rc;
}

void l3d_node_comm_destroy(l3d_node_comm* c)
{
    if (!c) return;
    for (int r = 0; r < c->world; ++r) {
        (void)hipSetDevice(c->devices[(size_t)r]);
        if (c->send_ev[(size_t)r]) (void)hipEventDestroy(c->send_ev[(size_t)r]);
        if (c->done_ev[(size_t)r]) (void)hipEventDestroy(c->done_ev[(size_t)r]);
    }
    delete c;
}

int l3d_node_comm_bind(l3d_node_comm* c, int rank, void* stream)
{
    if (!c || rank < 0 || rank >= c->world || !stream) return L3D_ERR_INVALID;
    std::lock_guard<std::mutex> lk(c->mu);
    for (int q = 0; q < c->world; ++q)
        if (q != rank && c->streams[(size_t)q] == (hipStream_t)stream) return L3D_ERR_INVALID;   // one stream names one rank
    c->streams[(size_t)rank] = (hipStream_t)stream;
    return L3D_OK;
}

void l3d_node_comm_abort(l3d_node_comm* c)
{
    if (c) comm_abort(c, -1);
}

// One exchange of rank r (the rank bound to `stream`):
//   1. record send_ev[r] on the stream; publish send_slot          2. barrier
//   3. the stream waits for every peer's send_ev                     4. k_node_gather
//   5. record done_ev[r]                                             6. barrier
//   7. the stream waits for every peer's done_ev: nothing behind this exchange on the stream (the next write of the send slot) runs while a
//      peer still reads the slot.
// Every wait names an event recorded before a barrier all ranks passed.  Any failure breaks the barrier: every pending and later exchange of
// every rank returns non-zero.
int l3d_exchange_node(void* user, int view, const void* send_slot, void* recv_block, size_t slot_bytes, int world, void* stream)
{
    l3d_node_comm* c = static_cast<l3d_node_comm*>(user);
    if (!c) return 1;
    const int r = rank_of(c, stream);
    if (r < 0 || world != c->world || (slot_bytes && (!send_slot || !recv_block))) {
        fprintf(stderr, "[l3d node] exchange %d: %s\n", view, r < 0 ? "the stream is bound to no rank (l3d_node_comm_bind)" : "world or slot does not match the communicator");
        comm_abort(c, r);
        return 1;
    }
    const long long call = ++c->calls[(size_t)r];
    if (r == c->fail_rank && call == c->fail_at) {
        fprintf(stderr, "[l3d node] rank %d: exchange %d fails on request (option node_fail_at)\n", r, view);
        c->fail_rank = -1;                                          // (once)
        comm_abort(c, r);
        return 1;
    }
    if (c->broken) return 1;
    hipStream_t st = (hipStream_t)stream;
    if (hipSetDevice(c->devices[(size_t)r]) != hipSuccess || hipEventRecord(c->send_ev[(size_t)r], st) != hipSuccess) { comm_abort(c, r); return 1; }
    {
        std::lock_guard<std::mutex> lk(c->mu);
        c->send[(size_t)r] = send_slot;
        c->bytes[(size_t)r] = slot_bytes;
    }
    if (!comm_barrier(c, r, view)) return 1;
    l3d::NodeSources src{};
    bool ok = true;
    for (int q = 0; q < c->world && ok; ++q) {
        if (c->bytes[(size_t)q] != slot_bytes) {
            fprintf(stderr, "[l3d node] exchange %d: rank %d gathers %zu bytes per slot, rank %d %zu\n", view, r, slot_bytes, q, c->bytes[(size_t)q]);
            ok = false;
            break;
        }
        src.p[q] = static_cast<const unsigned char*>(c->send[(size_t)q]);
        if (q != r && hipStreamWaitEvent(st, c->send_ev[(size_t)q], 0) != hipSuccess) ok = false;
    }
    if (ok && slot_bytes) {
        const unsigned long long chunks = slot_bytes / 16 + 1;
        const unsigned gx = (unsigned)std::min<unsigned long long>(512, (chunks + 255) / 256);
        hipLaunchKernelGGL(l3d::k_node_gather, dim3(gx, (unsigned)c->world), dim3(256), 0, st, src, static_cast<unsigned char*>(recv_block),
                           (unsigned long long)slot_bytes);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { fprintf(stderr, "[l3d node] k_node_gather: %s\n", hipGetErrorString(e)); ok = false; }
    }
    if (ok && hipEventRecord(c->done_ev[(size_t)r], st) != hipSuccess) ok = false;
    if (!ok) { comm_abort(c, r); return 1; }
    if (!comm_barrier(c, r, view)) return 1;
    for (int q = 0; q < c->world; ++q)
        if (q != r && hipStreamWaitEvent(st, c->done_ev[(size_t)q], 0) != hipSuccess) { comm_abort(c, r); return 1; }
    return 0;
}

}  // extern "C"
