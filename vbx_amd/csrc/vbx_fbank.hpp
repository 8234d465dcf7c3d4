// vbx_fbank.hpp -- the x-vector extractor's front end (predict.py:150-178 with features.py): per VAD segment the
// mirror-padded signal is cut into frames, each frame goes through zero mean, pre-emphasis, the Povey window and a real
// DFT to a power spectrum, then a log-Mel filterbank and a floating-window CMN; the embedding model then reads windows of
// 144 frames every 24.
//
// The four linear steps of a frame are ONE f64 operator M = [cos; -sin] diag(w) P Z (2K x L, K = NFFT/2 + 1) built on the
// host (vbx_host_fbank.hpp), so the frame step is a GEMM on v_mfma_f64_16x16x4 followed by re^2 + im^2 (DESIGN section 14:
// an f32 transform puts 2e-3 on the quiet bands of a loud tone).
//
//   fbank_frame_kernel   one workgroup = 64 frames of one segment: samples staged in LDS through the mirror index map (the
//                        padded signal is never formed), frames x M^T on the matrix cores, power in LDS (f32), Mel + log
//                        accumulated in f64, log-Mel rows out in f64
//   fbank_cmn_kernel     cmvn_floating_kaldi(fea, LC, RC, norm_vars=False) per segment, cast to f32
//   fbank_gather_kernel  windows [n][64][len] (the model's [B, C, T] layout) from the CMN rows; fbank_gather_ragged_kernel:
//                        windows of mixed lengths, their [64][len_w] blocks laid end to end
//   fbank_dither_kernel  the dither before all of this (predict.py:169-170), for a caller that hands over the raw int16
//                        samples: numpy's legacy MT19937 stream, word for word, one workgroup per recording
#pragma once
#include "vbx_device.hpp"

namespace vbx {

constexpr int FB_MEL = 64;     // Mel channels (predict.py:156,162)
constexpr int FB_TILE = 64;    // frames per workgroup of the frame kernel
constexpr int FB_SKEW = 4;     // doubles of LDS padding after every SHIFT staged samples (bank spread of the A operand)

struct FbSeg {
    long long sig0;            // first sample of the segment in the (concatenated) signal
    long long row0;            // first output row of the segment
    int n;                     // samples of the segment (already clipped to the signal)
    int nframes;
};
struct FbTile {
    int seg, f0;               // frames f0 .. min(f0 + 64, nframes) of segment seg
};

// sample p of the mirror-padded segment, predict.py:173-174: seg[pre-1::-1], seg, seg[-1:-winlen//2-1:-1]
__device__ __forceinline__ int fb_mirror(int p, int pre, int n) {
    return p < pre ? pre - 1 - p : (p < pre + n ? p - pre : 2 * n + pre - 1 - p);
}

// MT [L][2 KP]: column block 32 t .. 32 t + 15 = real part of bins 16 t .. 16 t + 15, the next 16 columns their imaginary
// part (bins >= K are zero columns).  melT [64][KP] f64 with melr[m] = [first, last + 1) nonzero bin of channel m.
template <int L, int SHIFT, int KP>
__global__ __launch_bounds__(256) void fbank_frame_kernel(const double* __restrict__ sig, const FbSeg* __restrict__ segs,
                                                          const FbTile* __restrict__ tiles, const double* __restrict__ MT,
                                                          const double* __restrict__ melT, const int2* __restrict__ melr,
                                                          double* __restrict__ logmel, int pre, int post_cap) {
    using Mf = Mfma16<double>;
    using acc_t = Mf::acc_t;
    constexpr int SPAN = (FB_TILE - 1) * SHIFT + L;             // samples a tile of 64 frames covers
    constexpr int NPOS = SPAN + (SPAN / SHIFT + 1) * FB_SKEW;
    constexpr int RS = SHIFT + FB_SKEW;                         // LDS stride of one frame
    __shared__ double xs[NPOS];
    __shared__ float pw[FB_TILE][KP];
    const FbTile tl = tiles[blockIdx.x];
    const FbSeg sg = segs[tl.seg];
    const int n = sg.n, post = min(post_cap, n), padlen = pre + n + post;
    const int nf = min(FB_TILE, sg.nframes - tl.f0);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, kq = lane >> 4;
    const double* __restrict__ s = sig + sg.sig0;
    for (int r = tid; r < SPAN; r += 256) {
        const int p = tl.f0 * SHIFT + r;
        xs[r + (r / SHIFT) * FB_SKEW] = p < padlen ? s[fb_mirror(p, pre, n)] : 0.0;
    }
    __syncthreads();
    for (int t = wave; t < KP / 16; t += 4) {
        acc_t re[4], im[4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) re[rb] = im[rb] = acc_t{0, 0, 0, 0};
        const double* __restrict__ pb = MT + (long long)kq * 2 * KP + 32 * t + i;
#pragma unroll 4
        for (int k0 = 0; k0 < L; k0 += 4) {
            const double bre = pb[(long long)k0 * 2 * KP], bim = pb[(long long)k0 * 2 * KP + 16];
            const int l = k0 + kq, lp = l + (l / SHIFT) * FB_SKEW;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const double a = xs[(rb * 16 + i) * RS + lp];
                re[rb] = Mf::mma(a, bre, re[rb]);
                im[rb] = Mf::mma(a, bim, im[rb]);
            }
        }
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                pw[rb * 16 + Mf::row(lane, r)][16 * t + i] = (float)(re[rb][r] * re[rb][r] + im[rb][r] * im[rb][r]);
    }
    __syncthreads();
    const int m = tid & 63;
    const int2 br = melr[m];
    const double* __restrict__ wm = melT + m * KP;
    for (int fr = tid >> 6; fr < nf; fr += 4) {
        double acc = 0.0;
        for (int b = br.x; b < br.y; ++b) acc += (double)pw[fr][b] * wm[b];
        logmel[(sg.row0 + tl.f0 + fr) * FB_MEL + m] = log(fmax(1.0, acc));   // features.py:108
    }
}

// cmvn_floating_kaldi(x, LC, RC, norm_vars=False) (features.py:207-216) of one segment: window min(N, LC + RC + 1) frames,
// start max(min(t - LC, N - win), 0).  One workgroup = 64 frames; wave g slides one window sum per channel over 16 of them.
// blocks[b] = {segment, first frame}.
__global__ __launch_bounds__(256) void fbank_cmn_kernel(const double* __restrict__ logmel, const FbSeg* __restrict__ segs,
                                                        const FbTile* __restrict__ blocks, float* __restrict__ out, int LC,
                                                        int RC) {
    const FbTile bl = blocks[blockIdx.x];
    const FbSeg sg = segs[bl.seg];
    const int N = sg.nframes, win = min(N, LC + RC + 1), d = threadIdx.x & 63;
    const double* __restrict__ x = logmel + sg.row0 * FB_MEL + d;
    const int t0 = bl.f0 + 16 * (threadIdx.x >> 6), t1 = min(t0 + 16, N);
    double sum = 0.0;
    int ws_prev = -1;
    for (int t = t0; t < t1; ++t) {
        const int ws = max(min(t - LC, N - win), 0);
        if (ws_prev < 0) {
            for (int u = ws; u < ws + win; ++u) sum += x[(long long)u * FB_MEL];
        } else if (ws != ws_prev) {                             // the window moves by one frame at a time
            sum += x[(long long)(ws + win - 1) * FB_MEL] - x[(long long)ws_prev * FB_MEL];
        }
        ws_prev = ws;
        out[(sg.row0 + t) * FB_MEL + d] = (float)(x[(long long)t * FB_MEL] - sum / win);
    }
}

// out[w][c][t] = fea[starts[w] + t][c], t < len: a window as predict.py:68-70 hands it to the model ([1, 64, T] after the
// transpose), transposed through LDS 128 frames at a time.  One workgroup per window.
__global__ __launch_bounds__(256) void fbank_gather_kernel(const float* __restrict__ fea, const long long* __restrict__ starts,
                                                           int len, float* __restrict__ out) {
    __shared__ float tile[128][FB_MEL + 1];
    const long long w = blockIdx.x, row0 = starts[w];
    float* __restrict__ o = out + w * FB_MEL * (long long)len;
    for (int c0 = 0; c0 < len; c0 += 128) {
        const int nc = min(128, len - c0);
        for (int e = threadIdx.x; e < nc * FB_MEL; e += 256)
            tile[e >> 6][e & 63] = fea[(row0 + c0) * FB_MEL + e];
        __syncthreads();
        for (int e = threadIdx.x; e < nc * FB_MEL; e += 256) {
            const int c = e / nc, t = e - c * nc;
            o[(long long)c * len + c0 + t] = tile[t][c];
        }
        __syncthreads();
    }
}

// windows of mixed lengths, one workgroup each: window w is rows tab[w] .. + tab[2 n + w] and goes, transposed to
// [64][len], to out + 64 tab[n + w] (tab [3][n]: the first row, the frames before the window in the output, the length):
// the concatenated input of a ragged batch of the embedding network
__global__ __launch_bounds__(256) void fbank_gather_ragged_kernel(const float* __restrict__ fea, const long long* __restrict__ tab,
                                                                  int n, float* __restrict__ out) {
    __shared__ float tile[128][FB_MEL + 1];
    const long long w = blockIdx.x, row0 = tab[w];
    const int len = (int)tab[2 * (long long)n + w];
    float* __restrict__ o = out + tab[n + w] * FB_MEL;
    for (int c0 = 0; c0 < len; c0 += 128) {
        const int nc = min(128, len - c0);
        for (int e = threadIdx.x; e < nc * FB_MEL; e += 256)
            tile[e >> 6][e & 63] = fea[(row0 + c0) * FB_MEL + e];
        __syncthreads();
        for (int e = threadIdx.x; e < nc * FB_MEL; e += 256) {
            const int c = e / nc, t = e - c * nc;
            o[(long long)c * len + c0 + t] = tile[t][c];
        }
        __syncthreads();
    }
}

// ---- dither: x + level (2 rand - 1) with rand = np.random.RandomState(seed).rand ------------------------------------
// numpy's legacy generator is plain MT19937: 624 words of state, regenerated ("twisted") every 624 draws, each draw
// tempered, and a double made of two draws, r = ((a >> 5) 2^26 + (b >> 6)) / 2^53.  A twist is sequential as written,
//     new[i] = f(old[i], old[i + 1], i < 227 ? old[i + 397] : new[i - 227]),
//     f(u, v, w) = w ^ (y >> 1) ^ (y & 1 ? 0x9908b0df : 0), y = (u & 0x80000000) | (v & 0x7fffffff),
// but only through new[i - 227] and, for the last word, new[0]: words 0 .. 226 | 227 .. 453 | 454 .. 622 and 623 are
// three data-parallel phases with the same result (623 reads new[0] and new[396], both there after the second).
constexpr int MT_N = 624, MT_M = 397, MT_PAIRS = MT_N / 2;
constexpr int MT_AHEAD = 8;    // twists whose samples are in flight together (even)

struct FbRec {
    long long first, n;        // the recording's samples in the concatenated signal
    double level;
};

__device__ __forceinline__ unsigned mt_f(unsigned u, unsigned v, unsigned w) {
    const unsigned y = (u & 0x80000000u) | (v & 0x7fffffffu);
    return w ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

__device__ __forceinline__ unsigned mt_temper(unsigned y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    return y ^ (y >> 18);
}

// x + level (2 r - 1) of one sample: 2 r - 1 is exact (a multiple of 2^-52 below 1 in magnitude); the product rounds
// once for a level that is no power of two, and must then not be fused into the add, which numpy rounds separately
__device__ __forceinline__ double mt_dither(double x, double level, uint2 w) {
#pragma clang fp contract(off)
    const double r = ((double)(mt_temper(w.x) >> 5) * 67108864.0 + (double)(mt_temper(w.y) >> 6)) * (1.0 / 9007199254740992.0);
    const double d = level * (r * 2.0 - 1.0);
    return x + d;
}

// MT_AHEAD twists of the state in LDS and their doubles: twist tw0 + k reads copy k & 1 and writes the other one
// (MT_AHEAD is even), then the doubles of samples (tw0 + k) 312 + tid (and + 256 for the first 56 threads) are read from
// the written copy while the next twist already writes the one just read.  s: those samples.  FULL: all MT_AHEAD twists
// lie inside the n samples, nothing is masked (and the compiler can count the stores that follow a load).
template <bool FULL>
__device__ __forceinline__ void mt_group(unsigned (&mt)[2][MT_N], int tid, long long tw0, long long ntw, long long n,
                                         const int (&s)[MT_AHEAD][2], double level, double* __restrict__ o) {
    constexpr int P2 = MT_N - MT_M, P3 = 2 * P2;                // 227, 454: the first words of phases 2 and 3
    const bool two = tid < MT_PAIRS - 256;
#pragma unroll
    for (int k = 0; k < MT_AHEAD; ++k) {
        if (!FULL && tw0 + k >= ntw) break;                     // (the same for every thread, as the barriers need it)
        const unsigned* old = mt[k & 1];
        unsigned* nw = mt[(k & 1) ^ 1];
        if (tid < P2) nw[tid] = mt_f(old[tid], old[tid + 1], old[tid + MT_M]);
        __syncthreads();
        if (tid < P2) nw[P2 + tid] = mt_f(old[P2 + tid], old[P2 + tid + 1], nw[tid]);
        __syncthreads();
        if (tid < MT_N - 1 - P3)
            nw[P3 + tid] = mt_f(old[P3 + tid], old[P3 + tid + 1], nw[P2 + tid]);
        else if (tid == 255)
            nw[MT_N - 1] = mt_f(old[MT_N - 1], nw[0], nw[MT_M - 1]);
        __syncthreads();
        const uint2* pairs = reinterpret_cast<const uint2*>(nw);
        const long long p0 = (tw0 + k) * MT_PAIRS + tid, p1 = p0 + 256;
        if (FULL || p0 < n) o[p0] = mt_dither((double)s[k][0], level, pairs[tid]);
        if (two && (FULL || p1 < n)) o[p1] = mt_dither((double)s[k][1], level, pairs[tid + 256]);
    }
}

// sig[first + p] = raw[first + p] + level (2 rand_p - 1), p < n, for recording blockIdx.x: its stream restarts from
// states[blockIdx.x] (the 624 words init_genrand leaves, position 624: the first draw twists).  The state lives in LDS in
// two copies, a twist reads one and writes the other, so no thread overwrites a word a neighbour still reads.  Trip
// counts and barriers depend on the recording only; a twist past the end of the recording only masks its stores.
__global__ __launch_bounds__(256) void fbank_dither_kernel(const short* __restrict__ raw, const FbRec* __restrict__ recs,
                                                           const unsigned* __restrict__ states, double* __restrict__ sig) {
    __shared__ __attribute__((aligned(8))) unsigned mt[2][MT_N];
    const FbRec rc = recs[blockIdx.x];
    const int tid = threadIdx.x;
    if (rc.n <= 0) return;
    for (int i = tid; i < MT_N; i += 256) mt[0][i] = states[(long long)blockIdx.x * MT_N + i];
    __syncthreads();
    const short* __restrict__ x = raw + rc.first;
    double* __restrict__ o = sig + rc.first;
    const long long ntw = (rc.n + MT_PAIRS - 1) / MT_PAIRS;
    const long long nfull = rc.n / (MT_PAIRS * MT_AHEAD) * MT_AHEAD;   // the twists of the groups with nothing to mask
    // the samples of a group of twists are fetched together, a group ahead of the twists that use them: a twist is far
    // shorter than a trip to memory (indices past the recording are clamped into it, their results never stored)
    int sc[MT_AHEAD][2], sn[MT_AHEAD][2];                       // (a register each: packed halves would wait for their loads at once)
    auto fetch = [&](long long tw0, int (&s)[MT_AHEAD][2]) {
#pragma unroll
        for (int k = 0; k < MT_AHEAD; ++k) {
            const long long p0 = (tw0 + k) * MT_PAIRS + tid;
            s[k][0] = x[min(p0, rc.n - 1)];
            s[k][1] = x[min(tid < MT_PAIRS - 256 ? p0 + 256 : p0, rc.n - 1)];
        }
    };
    fetch(0, sc);
    long long tw0 = 0;
    for (; tw0 < nfull; tw0 += MT_AHEAD) {
        fetch(tw0 + MT_AHEAD, sn);
        mt_group<true>(mt, tid, tw0, ntw, rc.n, sc, rc.level, o);
#pragma unroll
        for (int k = 0; k < MT_AHEAD; ++k) sc[k][0] = sn[k][0], sc[k][1] = sn[k][1];
    }
    if (tw0 < ntw) mt_group<false>(mt, tid, tw0, ntw, rc.n, sc, rc.level, o);   // (fewer than MT_AHEAD twists are left)
}

}  // namespace vbx
