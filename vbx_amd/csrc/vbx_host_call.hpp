// vbx_host_call.hpp -- host runtime: the device scratch and the error state of one "one call in, result out" entry point
// (one translation unit with vbx_capi.hip, which includes it after the allocator of vbx_host_launch.hpp; not a stand-alone header)
#pragma once
namespace {

// One call's blocks, its first VBX_* error and its first hipError_t.  Every step is a no-op once something has failed, so a
// call site reads top to bottom without a test per line; kernels are launched under one `if (call.ok())` and noted with
// launched().  The destructor hands every block back on every path, and never with work in flight: the pool may belong to
// contexts with other streams (vbx_ctx::pool), whose next taker is not ordered behind this stream.
// Declare it AFTER the host buffers its copies read or write: it then goes first, and waits before they go.
// Blocks that outlive the call (vbx_scores::d_s, vbx_xvectors::d_xproj / d_fea) are not its business: dmalloc and the
// handle's destroy function, as before.
struct DeviceCall {
    vbx_ctx* ctx;
    hipStream_t st;
    int rc = VBX_OK;
    hipError_t err = hipSuccess;
    bool in_flight = false;                    // something was enqueued since the last synchronize
    std::vector<void*> blocks;

    explicit DeviceCall(vbx_ctx* ctx_) : ctx(ctx_), st(ctx_->stream) {}
    DeviceCall(const DeviceCall&) = delete;
    DeviceCall& operator=(const DeviceCall&) = delete;
    ~DeviceCall() {
        if (in_flight) (void)hipStreamSynchronize(st);
        for (void* p : blocks) ctx_free(ctx, p);
    }

    bool ok() const { return rc == VBX_OK && err == hipSuccess; }
    void note(hipError_t e) {                  // the outcome of a HIP call
        if (ok()) err = e;
    }
    void enqueued(hipError_t e) {              // ... of one that put work on the stream
        in_flight = true;
        note(e);
    }
    template <typename T> T* alloc(size_t count) {
        T* p = nullptr;
        if (ok()) rc = dmalloc(ctx, &p, count);
        if (p) blocks.push_back(p);
        return p;
    }
    template <typename T> void copy_in(T* dst, const T* src, size_t count) {      // host -> a block the call already has
        if (ok() && count) enqueued(hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyHostToDevice, st));
    }
    template <typename T> T* upload(const T* src, size_t count) {
        T* p = alloc<T>(count);
        copy_in(p, src, count);
        return p;
    }
    template <typename T> void download(T* dst, const T* src, size_t count) {
        if (ok() && count) enqueued(hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyDeviceToHost, st));
    }
    void launched() {                          // after a group of kernel launches
        if (ok()) enqueued(hipGetLastError());
    }
    void sync() {
        if (!ok()) return;
        err = hipStreamSynchronize(st);
        in_flight = false;
    }
    // the return code; a HIP failure leaves "<what>: <HIP's text>" in ctx->err (an allocation failure has left its own)
    int finish(const char* what) {
        if (rc == VBX_OK && err != hipSuccess) {
            ctx->err = std::string(what) + ": " + hipGetErrorString(err);
            rc = VBX_ERR_HIP;
        }
        return rc;
    }
};

// turns arrive as [n][2] = (begin, end); the kernels read two planes
struct TurnPlanes {
    std::vector<double> beg, end;
    TurnPlanes(const double* turns, long long n) : beg((size_t)n), end((size_t)n) {
        for (long long t = 0; t < n; ++t) {
            beg[(size_t)t] = turns[2 * t];
            end[(size_t)t] = turns[2 * t + 1];
        }
    }
};

// A speaker index is a shift count and a row on the device: spk[0 .. n) inside [0, lim)?  The first that is not is reported as
// turn t0 + its place, in the words of the entry point fn: "<fn>: <unit> <index>: speaker S of <turn> T outside [0, lim)".
inline int check_turn_speakers(vbx_ctx* ctx, const char* fn, const char* unit, int index, const char* turn, const int32_t* spk,
                               long long t0, long long n, int lim) {
    for (long long t = 0; t < n; ++t)
        if (spk[t] < 0 || spk[t] >= lim)
            FAIL(ctx, VBX_ERR_INVALID, "%s: %s %d: speaker %d of %s %lld outside [0, %d)", fn, unit, index, spk[t], turn, t0 + t, lim);
    return VBX_OK;
}

}  // namespace
