// vbx_resample.hpp -- any PCM recording to mono int16 at 8 or 16 kHz: the raw interleaved bytes of a
// batch of recordings go up as they lie in their files, the converted samples come back.
//
// A sample becomes an integer q at 24-bit scale (u8: (b - 128) << 16, s16: x << 8, s24: x, s32: x >> 8, f32: NaN -> 0, else
// rint(x 2^23) clamped to [-2^23, 2^23 - 1]); the C channels of frame j are summed, X[j] = sum_c q_c[j].  With L = sr_out / g,
// M = sr_in / g, P = 32 max(L, M) and the integer prototype hq[0 .. 2P] of audio.resample_filter, whose every phase sums to
// 2^24, output m of a recording of n frames is
//   acc[m] = sum_j X[j] hq[P + m M - j L]          over the j in [0, n) with |m M - j L| <= P
//   y[m]   = clamp(floor((2 acc + D) / (2 D)), -32768, 32767),  D = C 2^32
// for m in [0, ceil(n L / M)).  |X| <= 2^26 and sum |hq| < 2^26 over a phase: every partial sum is an integer below 2^52 and
// the int64 sum is exact in any order.
//
// The table arrives phase-major: tab[p][k] = hq[p + k L] (0 past 2P), K = 2P / L + 1 taps a phase.  Output m has the phase
// p = (P + m M) mod L and the top frame jt = (P + m M) / L, and acc[m] = sum_k tab[p][k] X[jt - k].
//
// resample_kernel: one workgroup per tile of kRsTile outputs of one recording.  The tile's frames [jt(m0) - K + 1, jt(m1)]
// are decoded, summed over their channels and staged in LDS as int32 (zero outside [0, n) of the recording: nothing of a
// neighbour is ever read into a sum).  A sample of 1 to 4 bytes starts at any byte: it is cut out of the one or two aligned
// 32-bit words that hold it.  Thread t then owns output m0 + t and walks its phase's row.  A table of at most kRsTabLds
// entries (L <= 3 for every pair built: the rates that are multiples of the target, and 8 -> 16 kHz) is staged in LDS too;
// a larger one (at most 160 KB) is read through L2.  No atomics.
#pragma once
#include "vbx_device.hpp"

namespace vbx {

constexpr int kRsTile = 256;               // outputs per workgroup: one per thread
constexpr int kRsSpan = 8192;              // frames of a tile staged in LDS (32 KB): 192 kHz -> 8 kHz needs 7681
constexpr int kRsTabLds = 1024;            // table entries staged in LDS (4 KB)
constexpr int kRsZ = 32;                   // zero crossings on either side of the prototype: P = kRsZ max(L, M)

enum { kRsU8 = 0, kRsS16 = 1, kRsS24 = 2, kRsS32 = 3, kRsF32 = 4 };

struct RsRec {
    long long boff;       // first byte in the stream
    long long ooff;       // first of its n_out outputs
    int n, n_out;
};

// the sample of `bytes` bytes that starts at byte `a` of the stream, in the low bits of the result
__device__ __forceinline__ unsigned rs_fetch(const unsigned* __restrict__ words, long long a, int bytes) {
    const long long w = a >> 2;
    const int sh = (int)(a & 3);
    const unsigned lo = words[w];
    const unsigned hi = sh + bytes > 4 ? words[w + 1] : 0u;
    return (unsigned)((((unsigned long long)hi << 32) | lo) >> (8 * sh));
}

__device__ __forceinline__ int rs_decode(unsigned raw, int fmt) {
    switch (fmt) {
    case kRsU8: return ((int)(raw & 0xffu) - 128) * 65536;
    case kRsS16: return (int)(short)(raw & 0xffffu) * 256;
    case kRsS24: return (int)(raw << 8) >> 8;
    case kRsS32: return (int)raw >> 8;
    default: {
        const float x = __uint_as_float(raw);
        if (x != x) return 0;
        return (int)fminf(fmaxf(rintf(x * 8388608.0f), -8388608.0f), 8388607.0f);      // (the product is exact in f32)
    }
    }
}

// grid = items, items[i] = {recording, first output of the tile}
template <bool kTabInLds>
__global__ __launch_bounds__(256) void resample_kernel(const unsigned* __restrict__ words, const RsRec* __restrict__ recs,
                                                       const int2* __restrict__ items, const int* __restrict__ tab, int fmt,
                                                       int bytes, int C, int L, int M, int K, short* __restrict__ out) {
    __shared__ int x_sh[kRsSpan];
    __shared__ int tab_sh[kTabInLds ? kRsTabLds : 1];
    const int2 item = items[blockIdx.x];
    const RsRec rc = recs[item.x];
    const int tid = threadIdx.x, m0 = item.y;
    const int nm = min(kRsTile, rc.n_out - m0);
    const long long P = (long long)kRsZ * max(L, M);
    const int jlo = (int)((P + (long long)m0 * M) / L) - (K - 1);                  // may be < 0
    const int jhi = (int)((P + (long long)(m0 + nm - 1) * M) / L);                 // may be >= n
    const int span = jhi - jlo + 1;                                                // <= kRsSpan: checked on the host
    for (int i = tid; i < span; i += 256) {
        const int j = jlo + i;
        int x = 0;
        if (j >= 0 && j < rc.n) {
            long long a = rc.boff + (long long)j * C * bytes;
            for (int c = 0; c < C; ++c, a += bytes) x += rs_decode(rs_fetch(words, a, bytes), fmt);
        }
        x_sh[i] = x;
    }
    if constexpr (kTabInLds)
        for (int i = tid; i < L * K; i += 256) tab_sh[i] = tab[i];
    __syncthreads();
    if (tid >= nm) return;
    const long long top = P + (long long)(m0 + tid) * M;
    const int p = (int)(top % L);
    const int* row;
    if constexpr (kTabInLds) row = tab_sh + p * K;
    else row = tab + p * K;
    const int* xs = x_sh + ((int)(top / L) - jlo);                                 // X[jt - k] = xs[-k], jt - jlo in [K - 1, span)
    long long acc = 0;
    for (int k = 0; k < K; ++k) acc += (long long)row[k] * (long long)xs[-k];
    // floor((2 acc + D) / (2 D)) with D = C 2^32: the floor of the shift, then the floor of the division by C
    const int t = (int)((2 * acc + ((long long)C << 32)) >> 33);                   // |t| < 2^20 + 1
    int y = t / C;
    if (t % C < 0) --y;
    out[rc.ooff + m0 + tid] = (short)min(max(y, -32768), 32767);
}

}  // namespace vbx

// ---- host glue (included by vbx_capi.hip after vbx_host_call.hpp) ------------------------------------------------------------
extern "C" {

int vbx_resample_pcm(vbx_ctx* ctx, int64_t n_bytes, const uint8_t* bytes, int32_t n_rec, const int64_t* rec, int32_t format,
                     int32_t channels, int32_t L, int32_t M, int32_t taps, const int32_t* table, int16_t* out, float* ms) {
    using vbx::RsRec;
    if (!ctx) return VBX_ERR_INVALID;
    if (!rec || !table || (n_bytes > 0 && !bytes))
        FAIL(ctx, VBX_ERR_INVALID, "vbx_resample_pcm: bytes, rec and table must not be NULL");
    if (n_rec <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_resample_pcm: n_rec = %d recordings, need at least one", n_rec);
    if (n_bytes < 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_resample_pcm: n_bytes = %lld", (long long)n_bytes);
    if (format < vbx::kRsU8 || format > vbx::kRsF32)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_resample_pcm: format = %d, need 0 (u8), 1 (s16), 2 (s24), 3 (s32) or 4 (f32)", format);
    if (channels < 1 || channels > 8) FAIL(ctx, VBX_ERR_INVALID, "vbx_resample_pcm: channels = %d, need 1 to 8", channels);
    if (L < 1 || L > 640 || M < 1 || M > 1024)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_resample_pcm: L = %d, M = %d, need L in [1, 640] and M in [1, 1024]", L, M);
    const long long P = (long long)vbx::kRsZ * std::max(L, M);
    if (taps != 2 * P / L + 1)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_resample_pcm: taps = %d a phase, but L = %d and M = %d give %lld", taps, L, M, 2 * P / L + 1);
    // the frames of a full tile: from the top frame of its first output less taps - 1 to the top frame of its last
    const long long span = ((long long)(vbx::kRsTile - 1) * M + L - 1) / L + taps + 1;
    if (span > vbx::kRsSpan)
        FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_resample_pcm: L = %d, M = %d need %lld frames a tile of %d outputs, at most %d are "
             "staged", L, M, span, vbx::kRsTile, vbx::kRsSpan);
    static const int kBytes[5] = {1, 2, 3, 4, 4};
    const int sb = kBytes[format];
    const long long fb = (long long)sb * channels;
    std::vector<RsRec> recs((size_t)n_rec);
    std::vector<int2> items;
    long long outputs = 0;
    for (int r = 0; r < n_rec; ++r) {
        const long long a = rec[2 * r], n = rec[2 * r + 1];
        if (n > (1LL << 30)) FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_resample_pcm: recording %d has %lld frames, at most 2^30", r, n);
        if (a < 0 || n < 0 || a > n_bytes || n * fb > n_bytes - a)
            FAIL(ctx, VBX_ERR_INVALID, "vbx_resample_pcm: recording %d (byte %lld, %lld frames of %lld bytes) outside the %lld bytes",
                 r, a, n, fb, (long long)n_bytes);
        const long long n_out = (n * L + M - 1) / M;
        if (n_out > (1LL << 30)) FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_resample_pcm: recording %d gives %lld samples, at most 2^30", r, n_out);
        recs[r] = RsRec{a, outputs, (int)n, (int)n_out};
        for (long long m0 = 0; m0 < n_out; m0 += vbx::kRsTile) items.push_back(make_int2(r, (int)m0));
        outputs += n_out;
    }
    if (items.size() > 0x7fffffffULL)
        FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_resample_pcm: %zu tiles in one call, at most 2^31 - 1", items.size());
    if (outputs > 0 && !out) FAIL(ctx, VBX_ERR_INVALID, "vbx_resample_pcm: out must not be NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // a sample is cut out of aligned 32-bit words, the second of which may lie past the last byte: the buffer ends on a
    // 16-byte chunk boundary, a whole chunk past the bytes (what lies past n_bytes is read but never used)
    const size_t n_pad = ((size_t)n_bytes + 15) / 16 * 16 + 16;
    const size_t n_tab = (size_t)L * (size_t)taps;
    DeviceCall call(ctx);
    hipStream_t st = call.st;
    const unsigned grid = (unsigned)items.size();
    unsigned char* d_bytes = call.alloc<unsigned char>(n_pad);
    RsRec* d_recs = call.alloc<RsRec>(recs.size());
    int2* d_items = call.alloc<int2>(std::max<size_t>(items.size(), 1));
    int* d_tab = call.alloc<int>(n_tab);
    short* d_out = call.alloc<short>((size_t)std::max(outputs, 1LL));
    hipEvent_t ev[3] = {};
    auto stamp = [&](int i) {
        if (ms && call.ok()) call.enqueued(hipEventRecord(ev[i], st));
    };
    for (auto& x : ev)
        if (ms && call.ok()) call.note(hipEventCreate(&x));
    stamp(0);
    call.copy_in(d_bytes, (const unsigned char*)bytes, (size_t)n_bytes);
    call.copy_in(d_recs, recs.data(), recs.size());
    call.copy_in(d_items, items.data(), items.size());
    call.copy_in(d_tab, (const int*)table, n_tab);
    stamp(1);
    if (call.ok() && grid) {
        const unsigned* d_words = reinterpret_cast<const unsigned*>(d_bytes);
        if (n_tab <= (size_t)vbx::kRsTabLds)
            hipLaunchKernelGGL((vbx::resample_kernel<true>), dim3(grid), dim3(256), 0, st, d_words, d_recs, d_items, d_tab, format, sb,
                               channels, L, M, taps, d_out);
        else
            hipLaunchKernelGGL((vbx::resample_kernel<false>), dim3(grid), dim3(256), 0, st, d_words, d_recs, d_items, d_tab, format, sb,
                               channels, L, M, taps, d_out);
        call.launched();
    }
    stamp(2);
    call.download((short*)out, d_out, (size_t)outputs);
    call.sync();
    if (ms && call.ok()) call.note(hipEventElapsedTime(&ms[0], ev[0], ev[1]));
    if (ms && call.ok()) call.note(hipEventElapsedTime(&ms[1], ev[1], ev[2]));
    for (auto& x : ev)
        if (x) (void)hipEventDestroy(x);
    return call.finish("resampling kernel failed");
}

}  // extern "C"
