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

}  // namespace vbx
