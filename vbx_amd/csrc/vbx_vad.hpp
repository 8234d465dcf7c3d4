// vbx_vad.hpp -- Kaldi-style energy voice-activity detection for a batch of recordings: the int16
// samples go up once, the speech segments [a, b) in frames come back.
//
// A recording of n samples has T = (n - L) / H + 1 frames of L samples every H (400 / 160 at 16 kHz, 200 / 80 at 8 kHz; no
// dither, padding, pre-emphasis or window).  With G = gcd(L, H) = H / 2 a frame is five and a shift two sub-blocks of G
// samples, so the sums of x and x^2 over every sub-block, read once, give every frame:
//   N[t] = L sum x^2 - (sum x)^2                         int64, exact: L times the energy of the frame without its mean
//   e[t] = log(max(N[t] / L, 1))                         f64
//   theta = energy_threshold + mean_scale sum_t e[t] / T
//   raw[t] = n_hot >= n_in proportion                    n_in frames of [t - context, t + context] inside [0, T), n_hot with e > theta
// then on the maximal runs of raw: gaps shorter than min_silence close, runs shorter than min_speech drop, what is left
// grows by pad frames on both sides (clipped to [0, T)) and runs that touch become one.
//
// vad_energy: one workgroup per tile of kVadTile frames of one recording.  The tile's samples are read as aligned 16-byte
// chunks of the sample stream (eight samples; a chunk touches at most two sub-blocks since G >= 40), each thread adds its
// chunk's sums into the sub-block sums in LDS with integer atomics -- integers, so the order does not matter and N is
// exact.  Thread f then owns frame f.  The tile also leaves the sum of its e in a fixed order (block_sum: the butterfly
// of a wave, then the waves in order; a lane without a frame adds +0.0 to sums that are never negative).
// vad_theta: one workgroup per recording adds its tile sums -- thread i those of tiles i, i + 256, ... in order, then
// block_sum -- so theta depends on the recording alone: the same bits in any batch, no floating-point atomics.
// vad_raw: one thread per frame counts its window in e (clipped to the recording) and decides.
// vad_runs: one workgroup per recording.  The run boundaries by a prefix-sum compaction (kVadRunFrames frames a thread,
// 4096 a pass: a scan of the run starts places both ends, since the k-th end belongs to the k-th start), then close, drop
// and pad as three more compactions over the run list, 256 runs a pass, between two lists of (T + 1) / 2 runs.
// vad_pack: the recordings' final lists moved end to end, so that only the segments found are copied out.
//
// Every index is the recording's: a frame, a window or a run never looks past [0, T) of its own recording, and nothing is
// summed across recordings.
#pragma once
#include "vbx_device.hpp"
#include "vbx_labels_score.hpp"   // lab_block_scan

namespace vbx {

constexpr int kVadTile = 256;              // frames per energy / decision workgroup: one per thread
constexpr int kVadRunFrames = 16;          // frames a thread walks per pass of the boundary compaction
constexpr int kVadRunPass = 256 * kVadRunFrames;
static_assert(kVadTile == 256 && kLabBlock == 256, "one thread per frame of a tile, one scan entry per thread");
static_assert(kVadRunFrames + 2 <= 32, "a thread's frames and their two neighbours are one 32-bit mask");

struct VadRec {
    long long first;      // first sample in the stream
    long long foff;       // first of its T frames in N / e / raw
    long long poff;       // first of its ntiles tile sums
    long long roff;       // first of its (T + 1) / 2 run slots
    int T, ntiles;
};

// grid = items, items[i] = {recording, first frame of the tile}
template <int L, int H>
__global__ __launch_bounds__(256) void vad_energy_kernel(const short* __restrict__ samples, const VadRec* __restrict__ recs,
                                                         const int2* __restrict__ items, long long* __restrict__ Nout,
                                                         double* __restrict__ eout, double* __restrict__ part) {
    constexpr int G = H / 2, kSub = 2 * kVadTile + 3;
    static_assert(L == 5 * G && H == 2 * G && G >= 8, "five sub-blocks a frame, two a shift");
    __shared__ int sx_sh[kSub];
    __shared__ unsigned long long sq_sh[kSub];
    __shared__ double sum_sh[16];
    const int2 item = items[blockIdx.x];
    const VadRec rc = recs[item.x];
    const int tid = threadIdx.x, f0 = item.y;
    const int nf = min(kVadTile, rc.T - f0), nsub = 2 * nf + 3;
    for (int s = tid; s < nsub; s += 256) {
        sx_sh[s] = 0;
        sq_sh[s] = 0ull;
    }
    __syncthreads();
    const long long lo = rc.first + (long long)f0 * H;            // the tile is the samples [lo, lo + nsub G)
    const int nsmp = nsub * G;
    const long long c0 = lo >> 3, c1 = (lo + nsmp + 7) >> 3;      // its aligned 16-byte chunks
    const int4* chunks = reinterpret_cast<const int4*>(samples);
    for (long long c = c0 + tid; c < c1; c += 256) {
        const int4 v = chunks[c];
        const int w[4] = {v.x, v.y, v.z, v.w};
        const int rel0 = (int)(c * 8 - lo);                        // the chunk's first sample inside the tile (may be < 0)
        const int subA = max(rel0, 0) / G;
        int sa = 0, sb = 0;
        unsigned long long qa = 0, qb = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int x = (int)(short)((unsigned)w[j >> 1] >> (16 * (j & 1)));
            const int rel = rel0 + j;
            const bool in = rel >= 0 && rel < nsmp;
            const bool first = rel < (subA + 1) * G;
            const int xa = in && first ? x : 0, xb = in && !first ? x : 0;
            sa += xa;
            qa += (unsigned long long)(xa * xa);                   // (|x| <= 2^15: the square fits an int)
            sb += xb;
            qb += (unsigned long long)(xb * xb);
        }
        atomicAdd(&sx_sh[subA], sa);
        atomicAdd(&sq_sh[subA], qa);
        if (rel0 + 7 >= (subA + 1) * G && subA + 1 < nsub) {
            atomicAdd(&sx_sh[subA + 1], sb);
            atomicAdd(&sq_sh[subA + 1], qb);
        }
    }
    __syncthreads();
    double e = 0.0;
    if (tid < nf) {
        long long S = 0, Q = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            S += sx_sh[2 * tid + k];
            Q += (long long)sq_sh[2 * tid + k];
        }
        const long long N = (long long)L * Q - S * S;              // < 2^48: exact as a double too
        e = log(fmax((double)N / (double)L, 1.0));
        Nout[rc.foff + f0 + tid] = N;
        eout[rc.foff + f0 + tid] = e;
    }
    const double tot = block_sum(e, sum_sh);
    if (tid == 0) part[rc.poff + f0 / kVadTile] = tot;
}

// grid = recordings
__global__ __launch_bounds__(256) void vad_theta_kernel(const VadRec* __restrict__ recs, const double* __restrict__ part,
                                                        double energy_threshold, double mean_scale,
                                                        double* __restrict__ theta) {
    __shared__ double sum_sh[16];
    const VadRec rc = recs[blockIdx.x];
    double s = 0.0;
    for (int i = threadIdx.x; i < rc.ntiles; i += 256) s += part[rc.poff + i];
    const double tot = block_sum(s, sum_sh);
    // (each operation rounded on its own, as the host writes it; a recording without a frame has no mean: theta is the offset)
    if (threadIdx.x == 0)
        theta[blockIdx.x] = rc.T > 0 ? __dadd_rn(energy_threshold, __ddiv_rn(__dmul_rn(mean_scale, tot), (double)rc.T))
                                     : energy_threshold;
}

// grid = items of vad_energy_kernel
__global__ __launch_bounds__(256) void vad_raw_kernel(const VadRec* __restrict__ recs, const int2* __restrict__ items,
                                                      const double* __restrict__ e, const double* __restrict__ theta,
                                                      int context, double proportion, unsigned char* __restrict__ raw) {
    const int2 item = items[blockIdx.x];
    const VadRec rc = recs[item.x];
    const int t = item.y + threadIdx.x;
    if (t >= rc.T) return;
    const double th = theta[item.x];
    const int w0 = max(t - context, 0), w1 = (int)min((long long)t + context, (long long)rc.T - 1);
    const double* er = e + rc.foff;
    int hot = 0;
    for (int u = w0; u <= w1; ++u) hot += er[u] > th ? 1 : 0;
    raw[rc.foff + t] = (double)hot >= __dmul_rn((double)(w1 - w0 + 1), proportion) ? 1 : 0;
}

// runs of `in` grown by pad (clipped to [0, T)), neighbours closer than gap made one  ->  out; returns how many are left
__device__ __forceinline__ int vad_merge(const int2* in, int n, int2* out, int pad, int gap, int T, int* sh, int tid) {
    int base = 0;
    for (int k0 = 0; k0 < n; k0 += kLabBlock) {
        const int k = k0 + tid;
        int a = 0, b = 0;
        bool head = false, tail = false;
        if (k < n) {
            const int2 r = in[k];
            a = max(r.x - pad, 0);
            b = min(r.y + pad, T);
            head = k == 0 || a - min(in[k - 1].y + pad, T) >= gap;
            tail = k == n - 1 || max(in[k + 1].x - pad, 0) - b >= gap;
        }
        const int idx = base + lab_block_scan(head ? 1 : 0, sh, tid) - 1;      // the run that k ends up in
        if (head) out[idx].x = a;
        if (tail) out[idx].y = b;
        base += sh[kLabBlock - 1];
    }
    __syncthreads();                                                  // (out is read by the whole workgroup next)
    return base;
}

// runs of `in` of at least min_len frames  ->  out
__device__ __forceinline__ int vad_drop(const int2* in, int n, int2* out, int min_len, int* sh, int tid) {
    int base = 0;
    for (int k0 = 0; k0 < n; k0 += kLabBlock) {
        const int k = k0 + tid;
        int2 r = make_int2(0, 0);
        if (k < n) r = in[k];
        const bool keep = k < n && r.y - r.x >= min_len;
        const int idx = base + lab_block_scan(keep ? 1 : 0, sh, tid) - 1;
        if (keep) out[idx] = r;
        base += sh[kLabBlock - 1];
    }
    __syncthreads();
    return base;
}

// grid = recordings; run_a / run_b: (T + 1) / 2 slots each at roff; the final list is in run_b, its length in count
__global__ __launch_bounds__(256) void vad_runs_kernel(const VadRec* __restrict__ recs, const unsigned char* __restrict__ raw,
                                                       int min_silence, int min_speech, int pad, int2* run_a, int2* run_b,
                                                       int* __restrict__ count) {
    __shared__ int scan_sh[kLabBlock];
    const VadRec rc = recs[blockIdx.x];
    const int tid = threadIdx.x, T = rc.T;
    const unsigned char* rw = raw + rc.foff;
    int2* A = run_a + rc.roff;
    int2* B = run_b + rc.roff;
    int n = 0;
    for (int t0 = 0; t0 < T; t0 += kVadRunPass) {
        const int ta = t0 + tid * kVadRunFrames;
        const int len = max(min(kVadRunFrames, T - ta), 0);
        // bit 0: the frame before ta, bits 1 .. len: this thread's frames, bit len + 1: the frame after them (0 outside [0, T))
        unsigned m = 0;
        if (len > 0) {
            if (ta > 0) m |= rw[ta - 1] ? 1u : 0u;
            for (int i = 0; i < len; ++i) m |= rw[ta + i] ? 2u << i : 0u;
            if (ta + len < T) m |= rw[ta + len] ? 2u << len : 0u;
        }
        const unsigned x = m >> 1, mine = (1u << len) - 1u;
        const unsigned starts = x & ~m & mine, ends = x & ~(x >> 1) & mine;
        // the run a frame belongs to is the number of starts up to it, minus one: an end needs no scan of its own
        int c = n + lab_block_scan(__popc(starts), scan_sh, tid) - __popc(starts);
        for (int i = 0; i < len; ++i) {
            if (starts >> i & 1u) A[c++].x = ta + i;
            if (ends >> i & 1u) A[c - 1].y = ta + i + 1;
        }
        n += scan_sh[kLabBlock - 1];
    }
    __syncthreads();
    n = vad_merge(A, n, B, 0, min_silence, T, scan_sh, tid);          // close
    n = vad_drop(B, n, A, min_speech, scan_sh, tid);                  // drop
    n = vad_merge(A, n, B, pad, 1, T, scan_sh, tid);                  // pad: runs that touch or overlap have a gap < 1
    if (tid == 0) count[blockIdx.x] = n;
}

// grid = recordings: the final lists end to end, in recording order
__global__ __launch_bounds__(256) void vad_pack_kernel(const VadRec* __restrict__ recs, const int2* __restrict__ runs,
                                                       const int* __restrict__ count, int2* __restrict__ packed) {
    __shared__ int scan_sh[kLabBlock];
    const int r = blockIdx.x, tid = threadIdx.x;
    int before = 0;
    for (int q = tid; q < r; q += kLabBlock) before += count[q];
    lab_block_scan(before, scan_sh, tid);
    const int off = scan_sh[kLabBlock - 1];
    const int2* src = runs + recs[r].roff;
    for (int k = tid; k < count[r]; k += kLabBlock) packed[off + k] = src[k];
}

}  // namespace vbx

// ---- host glue (included by vbx_capi.hip after vbx_host_call.hpp) ------------------------------------------------------------
extern "C" {

int vbx_vad_energy(vbx_ctx* ctx, int64_t n_samples, const int16_t* samples, int32_t n_rec, const int64_t* rec, int32_t winlen,
                   int32_t shift, double energy_threshold, double mean_scale, int32_t context, double proportion,
                   int32_t min_silence, int32_t min_speech, int32_t pad, int32_t* counts, int32_t* segs, int64_t* N, double* e,
                   double* theta, uint8_t* raw, float* ms) {
    using vbx::VadRec;
    if (!ctx) return VBX_ERR_INVALID;
    if (!rec || !counts || !segs || (n_samples > 0 && !samples))
        FAIL(ctx, VBX_ERR_INVALID, "vbx_vad_energy: samples, rec, counts and segs must not be NULL");
    if (n_rec <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_vad_energy: n_rec = %d recordings, need at least one", n_rec);
    if (n_samples < 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_vad_energy: n_samples = %lld", (long long)n_samples);
    if (!((winlen == 400 && shift == 160) || (winlen == 200 && shift == 80)))
        FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_vad_energy: frames of %d samples every %d not built; supported: 400 / 160 (16 kHz) "
             "and 200 / 80 (8 kHz)", winlen, shift);
    if (!std::isfinite(energy_threshold) || !std::isfinite(mean_scale) || !std::isfinite(proportion))
        FAIL(ctx, VBX_ERR_INVALID, "vbx_vad_energy: energy_threshold = %g, mean_scale = %g, proportion = %g must be finite",
             energy_threshold, mean_scale, proportion);
    const int lim = 1 << 30;
    if (context < 0 || min_silence < 0 || min_speech < 0 || pad < 0 || context > lim || min_silence > lim || min_speech > lim || pad > lim)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_vad_energy: context = %d, min_silence = %d, min_speech = %d, pad = %d must lie in [0, 2^30]",
             context, min_silence, min_speech, pad);
    std::vector<VadRec> recs((size_t)n_rec);
    std::vector<int2> items;
    long long frames = 0, tiles = 0, slots = 0;
    for (int r = 0; r < n_rec; ++r) {
        const long long a = rec[2 * r], n = rec[2 * r + 1];
        if (a < 0 || n < 0 || a > n_samples || n > n_samples - a)
            FAIL(ctx, VBX_ERR_INVALID, "vbx_vad_energy: recording %d (start %lld, %lld samples) outside the %lld samples", r, a, n,
                 (long long)n_samples);
        const long long T = n >= winlen ? (n - winlen) / shift + 1 : 0;
        if (T > lim) FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_vad_energy: recording %d has %lld frames, at most 2^30", r, T);
        const int nt = (int)((T + vbx::kVadTile - 1) / vbx::kVadTile);
        recs[r] = VadRec{a, frames, tiles, slots, (int)T, nt};
        for (int i = 0; i < nt; ++i) items.push_back(make_int2(r, i * vbx::kVadTile));
        frames += T;
        tiles += nt;
        slots += (T + 1) / 2;
    }
    if (frames > 0x7fffffffLL) FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_vad_energy: %lld frames in one call, at most 2^31 - 1", frames);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the samples are read as 16-byte chunks: the buffer ends on a chunk boundary (what lies past n_samples is masked out)
    const size_t n_pad = ((size_t)n_samples + 7) / 8 * 8;
    DeviceCall call(ctx);
    hipStream_t st = call.st;
    const unsigned grid = (unsigned)items.size();
    short* d_smp = call.alloc<short>(n_pad);
    VadRec* d_recs = call.alloc<VadRec>(recs.size());
    int2* d_items = call.alloc<int2>(items.size());
    int2* d_ra = call.alloc<int2>((size_t)slots);
    int2* d_rb = call.alloc<int2>((size_t)slots);
    int2* d_pack = call.alloc<int2>((size_t)slots);
    long long* d_N = call.alloc<long long>((size_t)frames);
    double* d_e = call.alloc<double>((size_t)frames);
    double* d_part = call.alloc<double>((size_t)tiles);
    double* d_theta = call.alloc<double>((size_t)n_rec);
    unsigned char* d_raw = call.alloc<unsigned char>((size_t)frames);
    int* d_cnt = call.alloc<int>((size_t)n_rec);
    hipEvent_t ev[3] = {};
    auto stamp = [&](int i) {                                         // timing (ms given): an event in the stream, here
        if (ms && call.ok()) call.enqueued(hipEventRecord(ev[i], st));
    };
    for (auto& x : ev)
        if (ms && call.ok()) call.note(hipEventCreate(&x));
    stamp(0);
    call.copy_in(d_smp, (const short*)samples, (size_t)n_samples);    // (every block is there already: ms[0] times the uploads alone)
    call.copy_in(d_recs, recs.data(), recs.size());
    call.copy_in(d_items, items.data(), items.size());
    stamp(1);
    if (call.ok()) {
        if (grid && winlen == 400)
            hipLaunchKernelGGL((vbx::vad_energy_kernel<400, 160>), dim3(grid), dim3(256), 0, st, d_smp, d_recs, d_items, d_N, d_e, d_part);
        else if (grid)
            hipLaunchKernelGGL((vbx::vad_energy_kernel<200, 80>), dim3(grid), dim3(256), 0, st, d_smp, d_recs, d_items, d_N, d_e, d_part);
        hipLaunchKernelGGL(vbx::vad_theta_kernel, dim3((unsigned)n_rec), dim3(256), 0, st, d_recs, d_part, energy_threshold, mean_scale,
                           d_theta);
        if (grid)
            hipLaunchKernelGGL(vbx::vad_raw_kernel, dim3(grid), dim3(256), 0, st, d_recs, d_items, d_e, d_theta, context, proportion, d_raw);
        hipLaunchKernelGGL(vbx::vad_runs_kernel, dim3((unsigned)n_rec), dim3(256), 0, st, d_recs, d_raw, min_silence, min_speech, pad, d_ra,
                           d_rb, d_cnt);
        hipLaunchKernelGGL(vbx::vad_pack_kernel, dim3((unsigned)n_rec), dim3(256), 0, st, d_recs, d_rb, d_cnt, d_pack);
        call.launched();
    }
    stamp(2);
    call.download(counts, d_cnt, (size_t)n_rec);
    if (N) call.download((long long*)N, d_N, (size_t)frames);
    if (e) call.download(e, d_e, (size_t)frames);
    if (raw) call.download(raw, d_raw, (size_t)frames);
    if (theta) call.download(theta, d_theta, (size_t)n_rec);
    call.sync();                                                      // (counts has landed)
    long long total = 0;
    for (int r = 0; call.ok() && r < n_rec; ++r) total += counts[r];
    call.download((int2*)segs, d_pack, (size_t)total);
    call.sync();
    if (ms && call.ok()) call.note(hipEventElapsedTime(&ms[0], ev[0], ev[1]));
    if (ms && call.ok()) call.note(hipEventElapsedTime(&ms[1], ev[1], ev[2]));
    for (auto& x : ev)
        if (x) (void)hipEventDestroy(x);
    return call.finish("energy VAD kernels failed");
}

}  // extern "C"
