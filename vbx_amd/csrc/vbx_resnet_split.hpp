// vbx_resnet_split.hpp -- the convolutions of the x-vector network (vbx_resnet.hpp) on the f16 matrix cores with
// error-compensated operands: the "split" mode of the network (vbx_resnet_set_gemm), the representation of vbx_split.hpp.
//
// Every f32 operand is carried as two f16 terms under an exact power-of-two scale,
//     x 2^e = hi + lo,   hi = f16(x 2^e),   lo = f16(x 2^e - hi),   e: the scaling group's largest magnitude in [2^13, 2^14)
// and a product over a k-step of 16 is three v_mfma_f32_32x32x16_f16 into the same f32 accumulators, in the fixed order
// lo hi, hi lo, hi hi (the dropped lo lo term is 2^-22 of a product), over K in order: no split of K, no atomics on
// outputs, so an output element has the same bits under every tile and in every batch.
//
//   weights       split once on the host (rn_split_weights), one scale per output channel, stored in the fragment order
//                 of the B operand: [K / 16][Cout / 32][hi | lo][lane 0..63][8], lane l = B[k = 8 (l >> 5) + j][col l & 31]
//   activations   stay f32 NHWC in HBM; the consumer splits its A tile as it stages it.  The scaling group is ONE WINDOW
//                 (one image of the batch): a batch-wide scale would make an embedding depend on its neighbours.  Every
//                 producer records max |y| per window (the bits of a non-negative float order like unsigned integers: one
//                 vector atomicMax, order-free and so deterministic; non-finite values do not count, so that the finite
//                 rest of a window that holds a NaN keeps its precision).  A slot of zero gives e = 0.
//   epilogue      acc 2^-(e_window + e_channel) (exact), + bias, + res, the NaN-keeping ReLU.
//
// A scaled product is below 2^28 and K <= 2304 in the network, so the f32 accumulators cannot overflow.  An Inf input gives
// hi = Inf, lo = Inf - Inf = NaN: the outputs it reaches are NaN where the exact mode gives Inf.
#pragma once
#include "vbx_resnet.hpp"

namespace vbx {

constexpr int RS_BK = 32;        // K per LDS stage: two k-steps of 16

// max |x| over the finite elements of every window of a level of H rows and C channels (C a multiple of 4) -> amax[window]
// (zeroed beforehand); grid = n * bpw blocks, bpw blocks share a window.  One body for uniform and ragged batches, as the
// convolution below: g (vbx_resnet.hpp: RnLevel) says where window b lies
template <bool RAG>
__global__ __launch_bounds__(256) void resnet_amax_kernel(const float* __restrict__ x, int H, int C, int bpw,
                                                          unsigned* __restrict__ amax, RnLevel<RAG> g) {
    using f4 = Vec<float>::v4;
    const long long b = blockIdx.x / bpw;
    const int part = blockIdx.x - (int)(b * bpw);
    const RnSpan win = rn_span(g, b, H);
    const f4* __restrict__ src = reinterpret_cast<const f4*>(x + win.start * C);
    const long long n4 = win.count * C >> 2;
    int m = 0;
    for (long long q = (long long)part * 256 + threadIdx.x; q < n4; q += 256LL * bpw) {
        const f4 v = src[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int a = __builtin_bit_cast(int, v[j]) & 0x7fffffff;
            m = vmax(m, a < 0x7f800000 ? a : 0);
        }
    }
    m = allreduce_max<64>(m);
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(amax + b, (unsigned)m);
}

// the window of every row of a ragged tile, kept in LDS from the prologue for the epilogue (no LDS in the uniform kernels)
template <int BM, bool RAG> __device__ __forceinline__ int* rs_row_windows() {
    if constexpr (RAG) {
        __shared__ int Ws[BM];
        return Ws;
    } else {
        return nullptr;
    }
}

// resnet_conv_kernel's contract (x, bias, res, y, geometry, grid (ceil(M / BM), Cout / BN)) with
//   amax_x [n]  max |x| per window (bits), wf / we the split weights and their per-channel exponents,
//   amax_y [n]  or null: receives max |y| per window (zeroed beforehand)
//   RAG         a ragged batch g.t (vbx_resnet.hpp); amax_x and amax_y [g.t.n]
template <int KS, int S, int BN, int BM, bool RAG = false>
__global__ __launch_bounds__(256) void resnet_conv_split_kernel(const float* __restrict__ x, const unsigned* __restrict__ amax_x,
                                                                const h8* __restrict__ wf, const int* __restrict__ we,
                                                                const float* __restrict__ bias, const float* __restrict__ res,
                                                                float* __restrict__ y, unsigned* __restrict__ amax_y, int H,
                                                                int W, int Cin, int Ho, int Wo, int Cout, long long M, int relu,
                                                                RnGeom<RAG> g) {
    constexpr int P = KS / 2;
    constexpr int WM = BM / 32, WN = 4 / WM;                   // waves along M and N
    constexpr int NACC = BN / WN / 32;
    static_assert(NACC >= 1 && WM * WN == 4, "tile");
    constexpr int NU = BM / 64;                                // A units (one row, 8 k: one lane's fragment) per thread
    constexpr int NBU = BN / 32;                               // B units (16 bytes) per thread
    constexpr int RB = BM / 32, CB = BN / 32;
    __shared__ h8 As[2 * 2 * RB * 64];                         // [k-step][hi | lo][row block][lane]
    __shared__ h8 Bs[2 * CB * 2 * 64];                         // [k-step][column block][hi | lo][lane]
    __shared__ int Es[BM];                                     // the exponent of every row's window
    int* const Ws = rs_row_windows<BM, RAG>();                 // ragged: the window itself
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long m0 = (long long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int K = KS * KS * Cin, KSTEPS = K >> 4, CBT = Cout >> 5;
    const long long hw = (long long)Ho * Wo;
    using f4 = Vec<float>::v4;

    // A: unit (row (tid >> 2) + 64 p, k-step ks_ = (tid >> 1) & 1, half kh_ = tid & 1): 8 consecutive channels of one tap
    const int ks_ = (tid >> 1) & 1, kh_ = tid & 1;
    int hb[NU], wb[NU], wW[NU], ea[NU];
    long long xb[NU];
    bool mv[NU];
#pragma unroll
    for (int p = 0; p < NU; ++p) {
        const int rl = (tid >> 2) + 64 * p;
        const long long m = m0 + rl;
        mv[p] = m < M;
        const RnRow row = rn_row<RAG>(m, mv[p], H, W, Cin, Ho, Wo, g);
        hb[p] = row.ho * S - P;
        wb[p] = row.wo * S - P;
        wW[p] = row.W;
        xb[p] = row.xb;
        ea[p] = mv[p] ? split_exponent(__builtin_bit_cast(float, amax_x[row.b])) : 0;
        if ((tid & 3) == 0) Es[rl] = ea[p];
        if constexpr (RAG)
            if ((tid & 3) == 0) Ws[rl] = (int)row.b;
    }
    f4 ra[NU][2];
    h8 rb[NBU];
    auto load = [&](int k0) {
        const int k = k0 + 16 * ks_;
        const bool kv = k < K;
        const int tap = k / Cin, c0 = k - tap * Cin + 8 * kh_, r = tap / KS, s = tap - r * KS;
#pragma unroll
        for (int p = 0; p < NU; ++p) {
            const int hi = hb[p] + r, wi = wb[p] + s, Wp = RAG ? wW[p] : W;
            ra[p][0] = ra[p][1] = f4{0.0f, 0.0f, 0.0f, 0.0f};
            if (kv && mv[p] && hi >= 0 && hi < H && wi >= 0 && wi < Wp) {
                const f4* src = reinterpret_cast<const f4*>(x + xb[p] + ((long long)hi * Wp + wi) * Cin + c0);
                ra[p][0] = src[0];
                ra[p][1] = src[1];
            }
        }
#pragma unroll
        for (int q = 0; q < NBU; ++q) {
            const int e = tid + 256 * q, cb = (e >> 7) % CB, st = (e >> 7) / CB, kstep = (k0 >> 4) + st;
            h8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (_Float16)0.0f;
            if (kstep < KSTEPS) v = wf[(((long long)kstep * CBT + (n0 >> 5) + cb) * 2 + ((e >> 6) & 1)) * 64 + (e & 63)];
            rb[q] = v;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int p = 0; p < NU; ++p) {
            const int rl = (tid >> 2) + 64 * p;
            h8 hi, lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                _Float16 a, b;
                split_f16(scale2(ra[p][j >> 2][j & 3], ea[p]), a, b);
                hi[j] = a;
                lo[j] = b;
            }
            h8* dst = As + ((ks_ * 2) * RB + (rl >> 5)) * 64 + 32 * kh_ + (rl & 31);
            dst[0] = hi;
            dst[RB * 64] = lo;
        }
#pragma unroll
        for (int q = 0; q < NBU; ++q) Bs[tid + 256 * q] = rb[q];
    };

    f32x16 acc[NACC];
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    const int i = lane & 31, kh = lane >> 5, wrb = wave % WM, wcb = (wave / WM) * NACC;
    load(0);
    store();
    lds_barrier();
    for (int k0 = 0; k0 < K; k0 += RS_BK) {
        const bool more = k0 + RS_BK < K;
        if (more) load(k0 + RS_BK);
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const h8 ah = As[((st * 2) * RB + wrb) * 64 + lane], al = As[((st * 2 + 1) * RB + wrb) * 64 + lane];
#pragma unroll
            for (int j = 0; j < NACC; ++j) {
                const h8 bh = Bs[((st * CB + wcb + j) * 2) * 64 + lane], bl = Bs[((st * CB + wcb + j) * 2 + 1) * 64 + lane];
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[j], 0, 0, 0);
            }
        }
        lds_barrier();
        if (more) {
            store();
            lds_barrier();
        }
    }
    const int row0 = wrb * 32;
    int am[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) am[r] = 0;
#pragma unroll
    for (int j = 0; j < NACC; ++j) {
        const int n = n0 + (wcb + j) * 32 + i;
        const float bn = bias[n];
        const int en = we[n];
        // the 16 residual loads of this column block go out together: one round trip, not one per row
        float rv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long m = m0 + row0 + rn_drow(r, kh);
            rv[r] = res && m < M ? res[m * Cout + n] : 0.0f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = row0 + rn_drow(r, kh);
            const long long m = m0 + rl;
            if (m < M) {
                const long long o = m * Cout + n;
                float v = scale2(acc[j][r], -(Es[rl] + en)) + bn;
                if (res) v += rv[r];
                v = relu ? rn_relu(v) : v;
                y[o] = v;
                const int a = __builtin_bit_cast(int, v) & 0x7fffffff;
                am[r] = vmax(am[r], a < 0x7f800000 ? a : 0);
            }
        }
    }
    if (amax_y && m0 + row0 < M) {                            // (wave-uniform)
        const long long mlast = m0 + row0 + 31 < M ? m0 + row0 + 31 : M - 1;
        const long long bf = RAG ? Ws[row0] : (m0 + row0) / hw;
        if (bf == (RAG ? Ws[(int)(mlast - m0)] : mlast / hw)) {   // the wave's 32 rows lie in one window
            int t = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) t = vmax(t, am[r]);
            t = allreduce_max<64>(t);
            if (lane == 0 && t > 0) atomicMax(amax_y + bf, (unsigned)t);
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int t = allreduce_max<32>(am[r]);
                const long long m = m0 + row0 + rn_drow(r, kh);
                if (i == 0 && m < M && t > 0) atomicMax(amax_y + (RAG ? Ws[(int)(m - m0)] : m / hw), (unsigned)t);
            }
        }
    }
}

}  // namespace vbx
