// The staging workspace of the stateless entry points: what a (thread, device) workspace (workspace.h) owns on the
// device -- an optional non-blocking stream and N grow-only buffers -- with the one binding, the one release and the one
// error rule all of them follow.  Each unit names its buffers once, in an enum that ends in the count:
//     enum { H_KPS, H_UR, ..., N_BUF };  struct PoseWs : Staging<N_BUF> {};
// so a new buffer is one new enumerator and the release covers it by construction.
#pragma once

#include <algorithm>

#include "carve.h"
#include "common.h"
#include "workspace.h"

namespace orbgpu {

template <int N> struct Staging {
    int device = -1;               // -1: unbound, owns nothing
    hipStream_t stream = nullptr;  // the host flavours' own stream; the device flavours run on the caller's
    bool pending = false;          // something was enqueued on `stream` since the last finish()
    int rc = ORBGPU_OK;            // first failure of a staging step since bind()
    DevBuf buf[N];

    Staging() = default;
    Staging(const Staging &) = delete;
    Staging &operator=(const Staging &) = delete;
    ~Staging() { release(); }

    // Every entry point calls this after select_device(device_id).  First use of this (thread, device) records the
    // device; own_stream asks for the stream as well (created once).  On failure nothing new is owned.
    int bind(int device_id, bool own_stream)
    {
        rc = ORBGPU_OK;
        if (own_stream && !stream) {
            hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
            if (e != hipSuccess) {
                stream = nullptr;
                set_error("hipStreamCreate: %s", hipGetErrorString(e));
                return ORBGPU_EHIP;
            }
        }
        device = device_id;
        return ORBGPU_OK;
    }

    // Reserve, upload, download: the first failure sticks (status()), later steps do nothing, so a run of them needs no
    // check per line -- one status() before the first launch that reads the buffers, and finish() at the end.
    template <typename T> T *as(int i) const { return buf[i].template as<T>(); }
    // the segment of buf[i] that starts `offset` bytes in (carve.h hands out the offsets)
    template <typename T> T *at(int i, size_t offset) const { return reinterpret_cast<T *>(as<char>(i) + offset); }
    template <typename T> T *at(Seg<T> s) const { return at<T>(s.buf, s.off); }
    int status() const { return rc; }
    void reserve(int i, size_t bytes)
    {
        if (rc == ORBGPU_OK)
            rc = buf[i].reserve(bytes);
    }
    // host -> buf[i] + offset on the own stream; the buffer has been reserved
    void upload(int i, const void *src, size_t bytes, size_t offset = 0) { copy(i, offset, const_cast<void *>(src), bytes, true); }
    void download(void *dst, int i, size_t bytes, size_t offset = 0) { copy(i, offset, dst, bytes, false); }
    // reserve, then upload: never less than 16 bytes (the kernels read with vector loads), nothing copied from a null
    // or empty source
    void put(int i, const void *src, size_t bytes)
    {
        reserve(i, std::max<size_t>(bytes, 16));
        if (src && bytes)
            upload(i, src, bytes);
    }
    // Waits for the own stream and returns the first failure, if any.
    int finish()
    {
        if (rc == ORBGPU_OK || pending) {
            hipError_t e = hipStreamSynchronize(stream);
            if (e != hipSuccess && rc == ORBGPU_OK) {
                set_error("hipStreamSynchronize: %s", hipGetErrorString(e));
                rc = ORBGPU_EHIP;
            }
        }
        pending = false;
        return rc;
    }

    // The error rule: a host flavour that has enqueued anything on the own stream waits for it before it returns a
    // non-OK code -- the copies read and write the caller's arrays.  The entry declares one of these once it holds the
    // workspace; a success path ends in finish(), after which this does nothing.
    struct FinishOnError {
        Staging &s;
        ~FinishOnError()
        {
            if (s.pending)
                (void)s.finish();
        }
    };

    // End of the owning thread (or of the owner of a workspace that is not the thread's), in workspace.h's order.
    // owner_hook releases what the owner keeps beside the buffers (the brute-force matcher's handle).
    template <typename Hook> void release(Hook owner_hook)
    {
        struct Ops {
            Staging &s;
            Hook &hook;
            void set_device() { (void)hipSetDevice(s.device); }
            void sync_stream() { (void)hipStreamSynchronize(s.stream); }
            void owner_hook() { hook(); }
            void free_buffers()
            {
                for (DevBuf &b : s.buf)
                    b.release();
            }
            void destroy_stream() { (void)hipStreamDestroy(s.stream); }
        } ops{*this, owner_hook};
        release_workspace(device >= 0, stream != nullptr, ops);
        device = -1, stream = nullptr, pending = false;
    }
    void release() { release([] {}); }

  private:
    void copy(int i, size_t offset, void *host, size_t bytes, bool to_device)
    {
        if (rc != ORBGPU_OK)
            return;
        if (!stream || offset + bytes > buf[i].bytes) {
            set_error("staging copy outside buffer %d (%zu + %zu of %zu bytes)", i, offset, bytes, buf[i].bytes);
            rc = ORBGPU_EINVAL;
            return;
        }
        pending = true;
        char *dev = at<char>(i, offset);
        hipError_t e = to_device ? hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, stream)
                                 : hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream);
        if (e != hipSuccess) {
            set_error("hipMemcpyAsync (staging buffer %d): %s", i, hipGetErrorString(e));
            rc = ORBGPU_EHIP;
        }
    }
};

// ---- how the solver and optimiser entry points (pose_opt.hip, sim3.hip, sim3_opt.hip, pnp.hip, initializer.hip,
// new_points.hip, local_ba.hip, essential_graph.hip) begin -------------------------------------------------------------------
// A *_batch_device entry: at most 65535 problems (the grid's y extent), each accepted by check(problem, index) -- which
// may also build what the problem needs on the host (essential_graph.hip: its index structure); then this thread's
// workspace, bound without a stream.  ws stays null for an empty batch, which only selects the device.
template <typename Ws, typename Problem, typename Check>
int batch_begin(int32_t n, const Problem *problems, Check check, int32_t device_id, Ws *&ws)
{
    ws = nullptr;
    ORBGPU_REQUIRE(n >= 0 && n <= 65535 && (n == 0 || problems), "bad arguments");
    int rc = ORBGPU_OK;
    for (int k = 0; k < n && rc == ORBGPU_OK; k++)
        rc = check(problems[k], k);
    if (rc != ORBGPU_OK || (rc = select_device(device_id)) != ORBGPU_OK || n == 0)
        return rc;
    ws = &per_device_workspace<Ws>(device_id);
    return ws->bind(device_id, false);
}

// A host flavour that stages its problem in carved blocks (sim3.hip, sim3_opt.hip, pnp.hip, initializer.hip, local_ba.hip,
// essential_graph.hip: a HostPlan's; new_points.hip: one block each way).  It runs on a stream of its own and shares the
// thread's workspace with the device flavours: whatever the thread enqueued through them on other streams must have left
// it, hence the device-wide wait (pose_opt.hip's does not wait: DESIGN.md 9.21).
template <typename Ws> int host_begin(int32_t device_id, Ws *&ws)
{
    int rc = select_device(device_id);
    if (rc != ORBGPU_OK)
        return rc;
    ORBGPU_HIP_TRY(hipDeviceSynchronize());
    ws = &per_device_workspace<Ws>(device_id);
    return ws->bind(device_id, true);
}
template <typename Ws> int host_begin(int32_t device_id, int in, size_t in_bytes, int out, size_t out_bytes, Ws *&ws)
{
    int rc = host_begin(device_id, ws);
    if (rc != ORBGPU_OK)
        return rc;
    ws->reserve(in, in_bytes);
    ws->reserve(out, out_bytes);
    return ws->status();
}
// every buffer the plan carved from, in the order of the workspace's enum
template <typename Ws, int N> int host_begin(int32_t device_id, const HostPlan<N> &plan, Ws *&ws)
{
    ORBGPU_REQUIRE(plan.ok(), "staging plan: more than %d copies", plan.MAX_SEGS);
    int rc = host_begin(device_id, ws);
    if (rc != ORBGPU_OK)
        return rc;
    for (int i = 0; i < N; i++)
        if (plan.bytes(i))
            ws->reserve(i, plan.bytes(i));
    return ws->status();
}

// ---- the two test hooks of the device optimisers (pose_opt.hip, sim3_opt.hip) -------------------------------------------
// A capacity of `max` records in LDS, lowered to k (clamped to [0, max]) while the environment variable `name` is set
// to k; read on every call, so that a test can set and clear it between calls.
inline int debug_limit(const char *name, int max)
{
    const char *s = getenv(name);
    return s ? std::min(std::max(atoi(s), 0), max) : max;
}

// The body of an *_last_spills entry point: buffer `counter` of this thread's workspace Ws, which the most recent
// optimisation zeroed and its kernel counted in, once the device has finished.
template <typename Ws> int last_spills(int32_t device_id, int counter, const char *none_recorded, int32_t *problems_spilled)
{
    ORBGPU_REQUIRE(problems_spilled, "null argument");
    int rc = select_device(device_id);
    if (rc != ORBGPU_OK)
        return rc;
    Ws &ws = per_device_workspace<Ws>(device_id);
    ORBGPU_REQUIRE(ws.buf[counter].p, "%s", none_recorded);
    ORBGPU_HIP_TRY(hipDeviceSynchronize());
    ORBGPU_HIP_TRY(hipMemcpy(problems_spilled, ws.buf[counter].p, sizeof(int32_t), hipMemcpyDeviceToHost));
    return ORBGPU_OK;
}

} // namespace orbgpu
