// vbx_resnet.hpp -- the x-vector network of the recipes (models/resnet.py: ResNet101, Bottleneck blocks [3, 4, 23, 3],
// m = 32, feat_dim 64) for inference, with every BatchNorm folded into the convolution before it (vbx_amd/xvector.py:
// fold, in f64 on the host).  Activations are NHWC f32: [B][H][W][C], H = 64 frequency rows, W = the window's frames.
//
//   resnet_conv_kernel   implicit-GEMM convolution, M = B Ho Wo output positions x N = Cout, K = kh kw Cin, on
//                        v_mfma_f32_32x32x2_f32 (an exact k-ordered f32 fma chain per element).  A BM x BN output tile per
//                        workgroup (BM = 128: four waves of 32 rows x BN; BM = 64, for grids too small to fill the CUs: 2 x 2
//                        waves of 32 rows x BN / 2); the K loop walks 16 inputs of one tap at a time (Cin is a
//                        multiple of 16), both operand tiles staged in LDS, the next one prefetched into registers.  Padded
//                        taps and rows past M read zero.  Epilogue: + folded bias [+ residual] [ReLU].
//   resnet_stem_kernel   conv 3x3 1 -> 32 (Cin = 1, K = 9) as a direct kernel, + bias, ReLU
//   resnet_pool_kernel   mean and standard deviation over time of layer4's [B][8][W4][1024] (resnet.py:138-140), in f64
//
// The embedding Linear(16384 -> E) is resnet_conv_kernel at H = W = 1.  No atomics and no split of K: every output element
// is one thread's fixed-order chain, so a window's embedding does not depend on the batch it is run in.  ReLU keeps NaN as
// F.relu does (a NaN window must reach the embedding: predict.py skips it).
//
// Ragged batches (windows of mixed lengths in one run): at spatial level l (H_l = 64, 32, 16, 8) an activation tensor is the
// concatenation of the windows' [H_l][W_{b,l}][C] blocks, window b starting at position pos_l[b].  Every kernel is one
// body with a compile-time RAG and takes the batch's geometry as its last argument, by value: nothing or one width in
// the uniform instantiation, the level's tables in the ragged one (RnGeom for the convolutions, RnLevel for the rest).  One
// if constexpr helper each is all that differs: a row m finds its window by a search of pos (rn_window) and takes its
// widths and its input base from the tables, where the uniform instantiation divides by Ho Wo (rn_row; rn_locate and rn_span
// for the stem, the pooling and resnet_amax_kernel).  Taps, k order and zeros are the same, so every window has the bits it
// has when it is run alone.  In a profile the kernels carry their instantiation: resnet_stem_kernel<false> is the uniform
// stem, resnet_stem_kernel<true> the ragged one, and so for resnet_pool_kernel and resnet_amax_kernel.
#pragma once
#include "vbx_device.hpp"

namespace vbx {

constexpr int RN_MEL = 64;       // input rows (Mel channels)
constexpr int RN_H4 = 8;         // rows after the three stride-2 stages
constexpr int RN_C4 = 1024;      // channels out of layer4 (256 planes x 4)
constexpr int RN_POOL = 2 * RN_H4 * RN_C4;
constexpr int RN_BK = 16;        // K per LDS stage

using f32x16 = float __attribute__((ext_vector_type(16)));

// relu(v) with NaN kept: (v < 0) is false for NaN.  fmaxf(v, 0) would return 0.
__device__ __forceinline__ float rn_relu(float v) { return v < 0.0f ? 0.0f : v; }

// the row of element r of a lane's 32 x 32 D fragment (its column is lane & 31); kh = lane >> 5
__device__ __forceinline__ int rn_drow(int r, int kh) { return (r & 3) + 8 * (r >> 2) + 4 * kh; }

// a ragged batch at one convolution: window b's block starts at position pos_in[b] of the input and pos_out[b] of the
// output (both [n + 1], ascending from 0, pos[n] = M) and is wid_in[b] / wid_out[b] positions wide; every window has the
// same H.
struct RnRag {
    const long long* pos_in = nullptr;
    const long long* pos_out = nullptr;
    const int* wid_in = nullptr;
    const int* wid_out = nullptr;
    int n = 0;
};
// the last argument of both convolution kernels: the tables in the ragged instantiations, nothing in the uniform ones
template <bool RAG> struct RnGeom {};
template <> struct RnGeom<true> {
    RnRag t;
};

// the window of position m < pos[n]: the last b with pos[b] <= m (an upper bound minus one: log2 n steps)
__device__ __forceinline__ int rn_window(const long long* __restrict__ pos, int n, long long m) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pos[mid] <= m) lo = mid;
        else hi = mid;
    }
    return lo;
}

// output row m -> its window b, its position (ho, wo) there, the width W of the window's input and the input's base xb
// (floats).  A row past M (valid false) gets zeros.
struct RnRow {
    long long b, xb;
    int ho, wo, W;
};
template <bool RAG>
__device__ __forceinline__ RnRow rn_row(long long m, bool valid, int H, int W, int Cin, int Ho, int Wo, const RnGeom<RAG>& g) {
    RnRow r;
    if constexpr (RAG) {
        r.b = valid ? rn_window(g.t.pos_out, g.t.n, m) : 0;
        const int wout = g.t.wid_out[r.b], rem = valid ? (int)(m - g.t.pos_out[r.b]) : 0;
        r.ho = rem / wout;
        r.wo = rem - r.ho * wout;
        r.W = g.t.wid_in[r.b];
        r.xb = g.t.pos_in[r.b] * Cin;
    } else {
        const long long hw = (long long)Ho * Wo;
        r.b = valid ? m / hw : 0;
        const int rem = valid ? (int)(m - r.b * hw) : 0;
        r.ho = rem / Wo;
        r.wo = rem - r.ho * Wo;
        r.W = W;
        r.xb = r.b * H * W * (long long)Cin;
    }
    return r;
}

// y[m][n] = act(sum_k A[m][k] W[k][n] + bias[n] (+ res[m][n])), A[m][(r KS + s) Cin + c] = x[b][ho S - P + r][wo S - P + s][c].
// w [K][Cout] (row k = tap r KS + s, input channel c), Cout a multiple of BN; grid (ceil(M / BM), Cout / BN).
// RAG: a ragged batch g.t of windows of H rows, M = g.t.pos_out[g.t.n]; W, Ho and Wo are not read.
template <int KS, int S, int BN, int BM, bool RAG = false>
__global__ __launch_bounds__(256) void resnet_conv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, const float* __restrict__ res,
                                                          float* __restrict__ y, int H, int W, int Cin, int Ho, int Wo,
                                                          int Cout, long long M, int relu, RnGeom<RAG> g) {
    constexpr int P = KS / 2;
    constexpr int WM = BM / 32, WN = 4 / WM;                   // waves along M and N
    constexpr int NACC = BN / WN / 32;
    static_assert(NACC >= 1 && WM * WN == 4, "tile");
    constexpr int NA = BM / 64;                                // A float4 per thread
    constexpr int LDA = BM + 4, LDB = BN + 4;
    constexpr int NB4 = RN_BK * BN / 4;                        // float4 of one B stage
    constexpr int NBL = (NB4 + 255) / 256;
    __shared__ float As[RN_BK][LDA];
    __shared__ float Bs[RN_BK][LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long m0 = (long long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int K = KS * KS * Cin;
    using f4 = Vec<float>::v4;

    // A: BM rows x 16 k, NA float4 per thread: quad kq of rows (tid >> 2) + 64 p
    const int kq = tid & 3;
    int hb[NA], wb[NA], wW[NA];
    long long xb[NA];
    bool mv[NA];
#pragma unroll
    for (int p = 0; p < NA; ++p) {
        const long long m = m0 + (tid >> 2) + 64 * p;
        mv[p] = m < M;
        const RnRow row = rn_row<RAG>(m, mv[p], H, W, Cin, Ho, Wo, g);
        hb[p] = row.ho * S - P;
        wb[p] = row.wo * S - P;
        wW[p] = row.W;
        xb[p] = row.xb;
    }
    f4 ra[NA], rb[NBL];
    auto load = [&](int k0) {
        const int tap = k0 / Cin, c0 = k0 - tap * Cin, r = tap / KS, s = tap - r * KS;
#pragma unroll
        for (int p = 0; p < NA; ++p) {
            const int hi = hb[p] + r, wi = wb[p] + s, Wp = RAG ? wW[p] : W;
            ra[p] = f4{0.0f, 0.0f, 0.0f, 0.0f};
            if (mv[p] && hi >= 0 && hi < H && wi >= 0 && wi < Wp)
                ra[p] = *reinterpret_cast<const f4*>(x + xb[p] + ((long long)hi * Wp + wi) * Cin + c0 + 4 * kq);
        }
#pragma unroll
        for (int q = 0; q < NBL; ++q) {
            const int e = tid + 256 * q;
            if (e < NB4) {
                const int kk = e / (BN / 4), nq = e - kk * (BN / 4);
                rb[q] = *reinterpret_cast<const f4*>(w + (long long)(k0 + kk) * Cout + n0 + 4 * nq);
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int p = 0; p < NA; ++p)
#pragma unroll
            for (int j = 0; j < 4; ++j) As[4 * kq + j][(tid >> 2) + 64 * p] = ra[p][j];
#pragma unroll
        for (int q = 0; q < NBL; ++q) {
            const int e = tid + 256 * q;
            if (e < NB4) {
                const int kk = e / (BN / 4), nq = e - kk * (BN / 4);
                *reinterpret_cast<f4*>(&Bs[kk][4 * nq]) = rb[q];
            }
        }
    };

    f32x16 acc[NACC];
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    const int i = lane & 31, kh = lane >> 5, row0 = (wave % WM) * 32, col0 = (wave / WM) * (BN / WN);
    load(0);
    store();
    __syncthreads();
    for (int k0 = 0; k0 < K; k0 += RN_BK) {
        const bool more = k0 + RN_BK < K;
        if (more) load(k0 + RN_BK);
#pragma unroll
        for (int kk = 0; kk < RN_BK; kk += 2) {
            const float a = As[kk + kh][row0 + i];
#pragma unroll
            for (int j = 0; j < NACC; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[kk + kh][col0 + 32 * j + i], acc[j], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            store();
            __syncthreads();
        }
    }
#pragma unroll
    for (int j = 0; j < NACC; ++j) {
        const int n = n0 + col0 + 32 * j + i;
        const float bn = bias[n];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long m = m0 + row0 + rn_drow(r, kh);
            if (m < M) {
                const long long o = m * Cout + n;
                float v = acc[j][r] + bn;
                if (res) v += res[o];
                y[o] = relu ? rn_relu(v) : v;
            }
        }
    }
}

// One level of a batch as the stem, the pooling and resnet_amax_kernel take it, their last argument: every window W
// positions wide, or (RAG) the level's tables: window b starts at position pos[b] ([n + 1], pos[n] = M) and is wid[b] wide.
template <bool RAG> struct RnLevel {
    int W;
};
template <> struct RnLevel<true> {
    const long long* pos;
    const int* wid;
    int n;
};

// window b of a level of H rows: the position it starts at, how many it has, its width
struct RnSpan {
    long long start, count;
    int W;
};
template <bool RAG> __device__ __forceinline__ RnSpan rn_span(const RnLevel<RAG>& g, long long b, int H) {
    if constexpr (RAG) return RnSpan{g.pos[b], g.pos[b + 1] - g.pos[b], g.wid[b]};
    else return RnSpan{b * H * (long long)g.W, (long long)H * g.W, g.W};
}

// position m of a level of RN_MEL rows -> its window's span, its row h and its column wo there: two divisions by W, or a
// search of pos and one division
template <bool RAG> __device__ __forceinline__ RnSpan rn_locate(const RnLevel<RAG>& g, long long m, int& h, int& wo) {
    long long b;
    if constexpr (RAG) {
        b = rn_window(g.pos, g.n, m);
        const int W = g.wid[b], rem = (int)(m - g.pos[b]);
        h = rem / W;
        wo = rem - h * W;
    } else {
        wo = (int)(m % g.W);
        const long long t = m / g.W;
        h = (int)(t % RN_MEL);
        b = t / RN_MEL;
    }
    return rn_span(g, b, RN_MEL);
}

// x: the windows' [64][T_b] blocks end to end (the front end's window layout, one input channel), w [9][32] (tap r 3 + s),
// y: their [64][T_b][32] NHWC blocks; total = 32 M
template <bool RAG>
__global__ __launch_bounds__(256) void resnet_stem_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ y,
                                                          long long total, RnLevel<RAG> g) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx & 31);
    int h, wo;
    const RnSpan win = rn_locate(g, idx >> 5, h, wo);
    const int W = win.W;
    const float* __restrict__ xb = x + win.start;
    float acc = 0.0f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int hi = h + r - 1;
        if (hi < 0 || hi >= RN_MEL) continue;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int wi = wo + s - 1;
            if (wi >= 0 && wi < W) acc = fmaf(xb[(long long)hi * W + wi], w[(r * 3 + s) * 32 + c], acc);
        }
    }
    y[idx] = rn_relu(acc + bias[c]);
}

// x: the windows' [8][W4_b][1024] blocks end to end -> out [B][16384]: [h 1024 + c] = mean over time, [8192 + h 1024 + c] =
// sqrt(mean(x^2) - mean^2 + 1e-10) (resnet.py:138-140, summed in f64), every window over its own W4_b.  The embedding
// matrix's columns are permuted on the host to this order.  total = 8192 B
template <bool RAG>
__global__ __launch_bounds__(256) void resnet_pool_kernel(const float* __restrict__ x, float* __restrict__ out, long long total,
                                                          RnLevel<RAG> g) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx & (RN_C4 - 1));
    const long long bh = idx >> 10;
    const int h = (int)(bh & (RN_H4 - 1));
    const long long b = bh >> 3;
    const RnSpan win = rn_span(g, b, RN_H4);
    const int W4 = win.W;
    const float* __restrict__ p = x + (win.start + (long long)h * W4) * RN_C4 + c;
    double s = 0.0, s2 = 0.0;
    for (int t = 0; t < W4; ++t) {
        const double v = p[(long long)t * RN_C4];
        s += v;
        s2 += v * v;
    }
    const double mean = s / W4;
    float* __restrict__ o = out + b * RN_POOL + h * RN_C4 + c;
    o[0] = (float)mean;
    o[RN_POOL / 2] = (float)sqrt(s2 / W4 - mean * mean + 1e-10);
}

}  // namespace vbx
