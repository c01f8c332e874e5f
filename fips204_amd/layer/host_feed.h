// The host-memory feed of the layers that hash raw messages where they lie in host memory (ph/hostfed.hip, mus/mus.hip): the bytes
// [msg_off[0], msg_off[n_ops]) stream through a ring of two staging chunks, cut by the chunk plan (host_chunks.h).  Chunk i + 1 is
// uploaded on the copy stream while the layer's update absorbs chunk i on the compute stream; the host waits only to get a staging
// chunk back, once per chunk.  This is the one place where host threads, two streams and four events agree on a buffer's lifetime.
// Internal linkage, as in layer_host.h.  Nothing here writes an error slot (ph's is not the scaffold's): run() hands a failure back and
// the layer reports it through its own fail / hip_failed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "host_chunks.h"
#include "layer_host.h"

namespace mldsa_layer {
namespace {

// the knee of the pre-hash layer's sweep recorded in profiles/prehash_stream_bench.jsonl; the mu-stream layer did not sweep again
constexpr size_t DEFAULT_STAGING = (size_t)64 << 20;

// page-locked (or otherwise known to the runtime) host memory is copied by DMA where it lies; anything else goes through the
// page-locked bounce chunk
bool is_pinned(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// how a run ended: a HIP runtime call of the ring failed (`hip`, in the step `step`), or the layer's update returned `rc`, or neither
struct FeedEnd {
    hipError_t hip = hipSuccess;
    const char* step = "";
    int rc = MLDSA_OK;
};

// inside run(): a HIP runtime call of the ring, or return how it failed
#define FEED_HIP(call, what)          \
    do {                              \
        end.hip = (call);             \
        if (end.hip != hipSuccess) {  \
            end.step = what;          \
            return end;               \
        }                             \
    } while (0)

struct HostFeed {
    int dev = -1;
    size_t staging = 0;
    hipStream_t copy = nullptr, compute = nullptr;  // both non-blocking; the layer's own launches and copies go on `compute`
    uint8_t* d_stage[2] = {nullptr, nullptr};
    uint8_t* h_stage[2] = {nullptr, nullptr};
    hipEvent_t copied[2] = {nullptr, nullptr};  // the chunk is in d_stage[b]
    hipEvent_t freed[2] = {nullptr, nullptr};   // the update that read d_stage[b] has finished
    bool in_flight[2] = {false, false};

    // on the current device `dev_`; staging_bytes = 0: DEFAULT_STAGING.  false: nothing is left allocated
    bool create(int dev_, size_t staging_bytes) {
        dev = dev_;
        staging = staging_bytes ? staging_bytes : DEFAULT_STAGING;
        bool ok = hipStreamCreateWithFlags(&copy, hipStreamNonBlocking) == hipSuccess &&
                  hipStreamCreateWithFlags(&compute, hipStreamNonBlocking) == hipSuccess;
        for (int b = 0; b < 2 && ok; b++)
            ok = hipMalloc((void**)&d_stage[b], staging) == hipSuccess &&
                 hipHostMalloc((void**)&h_stage[b], staging, hipHostMallocDefault) == hipSuccess &&
                 hipEventCreateWithFlags(&copied[b], hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&freed[b], hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            release();
        }
        return ok;
    }

    void release() {
        for (int b = 0; b < 2; b++) {
            if (d_stage[b]) (void)hipFree(d_stage[b]);
            if (h_stage[b]) (void)hipHostFree(h_stage[b]);
            if (copied[b]) (void)hipEventDestroy(copied[b]);
            if (freed[b]) (void)hipEventDestroy(freed[b]);
        }
        if (copy) (void)hipStreamDestroy(copy);
        if (compute) (void)hipStreamDestroy(compute);
        *this = HostFeed();
    }

    // after a failed call: nothing of it stays in flight
    void drain() {
        if (copy) (void)hipStreamSynchronize(copy);
        if (compute) (void)hipStreamSynchronize(compute);
    }

    // waits for both streams, then frees everything
    void destroy() {
        DeviceScope ds(dev);
        drain();
        release();
    }

    // Streams msgs[msg_off[0], msg_off[n_ops]) (a table mldsa_check_offsets has accepted).  For every chunk, update(chunk, d_chunk)
    // enqueues on `compute` the work that reads the chunk's bytes at d_chunk (byte chunk.lo of the batch is d_chunk[0]) and returns the
    // layer's rc; anything but MLDSA_OK ends the run and is passed through.  The work of the last chunks may still be running on return.
    template <class Update>
    FeedEnd run(const uint8_t* msgs, const uint64_t* msg_off, size_t n_ops, Update update) {
        FeedEnd end;
        const bool pinned = n_ops != 0 && msg_off[n_ops] > msg_off[0] && is_pinned(msgs + msg_off[0]);
        in_flight[0] = in_flight[1] = false;  // the call before this one ended with a wait for `compute`, or with drain()
        ChunkPlan plan(msg_off, n_ops, staging);
        Chunk c;
        for (int b = 0; plan.next(&c); b ^= 1) {
            const size_t len = (size_t)(c.hi - c.lo);
            // the only wait of the loop: the update two chunks back must be done with this buffer
            if (in_flight[b]) FEED_HIP(hipEventSynchronize(freed[b]), "wait for a staging chunk");
            const uint8_t* src = msgs + c.lo;
            if (!pinned) {
                memcpy(h_stage[b], src, len);
                src = h_stage[b];
            }
            FEED_HIP(hipMemcpyAsync(d_stage[b], src, len, hipMemcpyHostToDevice, copy), "upload of a chunk");
            FEED_HIP(hipEventRecord(copied[b], copy), "hipEventRecord");
            FEED_HIP(hipStreamWaitEvent(compute, copied[b], 0), "hipStreamWaitEvent");
            end.rc = update(c, d_stage[b]);
            if (end.rc != MLDSA_OK) return end;
            FEED_HIP(hipEventRecord(freed[b], compute), "hipEventRecord");
            in_flight[b] = true;
        }
        return end;
    }
};

#undef FEED_HIP

}  // namespace
}  // namespace mldsa_layer
