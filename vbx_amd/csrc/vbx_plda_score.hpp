// vbx_plda_score.hpp -- the Kaldi-recipe PLDA similarity the reference offers next to cos_similarity for the AHC stage:
//
//   kaldi_ivector_plda_scoring_dense (diarization_lib.py:59-93)   covariance of the rows, projection + Kaldi length
//                                                                  normalisation, T x T scores
//   PLDA_scoring_in_LDA_space        (diarization_lib.py:34-56)   N x M scores of rows that are already in LDA space
//
// Everything is float64 on v_mfma_f64_16x16x4, like cos_gemm_kernel (vbx_ahc.hpp).  The two eigen-decompositions and the
// inverse of the reference are D x D and stay on the host; what is O(T) or O(T^2) runs here:
//
//   covariance   column sums and (x - m)^T (x - m) over fixed chunks of kCovChunk rows, the partials added in chunk
//                order by one thread per entry: no atomics, the same input gives the same bits on every run
//   projection   y = (x - mu) M, y *= sqrt(d / sum_k y_k^2 / (acvar_k + 1)), a = y sqrt(Lambda), g = sum_k Gamma_k y_k^2
//   scores       S[i][j] = <a_i, b_j> + (r_i + c_j) + k.  With a = b and r = c the matrix is symmetric to the last bit:
//                both (i, j) and (j, i) run the same fused multiply-adds in the same k order (a product does not depend on
//                the order of its factors), and the row and the column term meet each other before they meet the dot
//                product.  The linkage kernels of vbx_ahc.hpp rely on that symmetry.
#pragma once
#include "vbx_device.hpp"

namespace vbx {

constexpr int kCovChunk = 512;             // rows of a covariance partial (fixed: the summation order is part of the result)
constexpr int kPldaMaxTiles = 16;          // 16-column tiles a projection workgroup keeps in registers: d <= 256

// part[c][j] = sum of x[t][j] over the rows of chunk c.  grid = chunks, block = 256 (thread = column, strided).
__global__ __launch_bounds__(256) void cov_colsum_kernel(const double* __restrict__ x, long long T, int D, int ld,
                                                          double* __restrict__ part) {
    const long long t0 = (long long)blockIdx.x * kCovChunk, t1 = min(t0 + kCovChunk, T);
    for (int j = threadIdx.x; j < D; j += 256) {
        double acc = 0.0;
        for (long long t = t0; t < t1; ++t) acc += x[t * ld + j];
        part[(long long)blockIdx.x * D + j] = acc;
    }
}

// mean[j] = (sum of the chunk partials, in chunk order) / T.  grid = ceil(D / 256).
__global__ __launch_bounds__(256) void cov_mean_kernel(const double* __restrict__ part, int nchunks, long long T, int D,
                                                        double* __restrict__ mean) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= D) return;
    double acc = 0.0;
    for (int c = 0; c < nchunks; ++c) acc += part[(long long)c * D + j];
    mean[j] = acc / (double)T;
}

// part[c][i][j] = sum over the rows t of chunk c of (x[t][i] - m[i]) (x[t][j] - m[j]), [Dp][Dp] per chunk, Dp = D rounded
// up to 16 (entries past D are zero).  grid = (ceil(D/64), ceil(D/64), chunks), block = 256: wave w owns the 32 x 32 sub-tile
// (w>>1, w&1) = 2 x 2 MFMA tiles; the MFMA's k runs over four rows of x, lane group g supplies row t + g.
__global__ __launch_bounds__(256) void cov_partial_kernel(const double* __restrict__ x, const double* __restrict__ mean,
                                                           long long T, int D, int ld, int Dp, double* __restrict__ part) {
    using M = Mfma16<double>;
    using acc_t = M::acc_t;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const int r0 = blockIdx.y * 64 + 32 * (wave >> 1), c0 = blockIdx.x * 64 + 32 * (wave & 1);
    const long long t0 = (long long)blockIdx.z * kCovChunk, t1 = min(t0 + kCovChunk, T);
    acc_t acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = acc_t{0, 0, 0, 0};
    int ja[2], jb[2];
    double ma[2], mb[2];
    bool oka[2], okb[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        oka[m] = r0 + 16 * m + i < D;
        okb[m] = c0 + 16 * m + i < D;
        ja[m] = min(r0 + 16 * m + i, D - 1);                 // columns past the end are clamped and contribute zero
        jb[m] = min(c0 + 16 * m + i, D - 1);
        ma[m] = mean[ja[m]];
        mb[m] = mean[jb[m]];
    }
    for (long long t = t0; t < t1; t += 4) {
        const bool live = t + g < t1;                        // rows past the end of the chunk contribute zero
        const double* __restrict__ row = x + min(t + g, T - 1) * ld;
        double a[2], b[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            a[m] = live && oka[m] ? row[ja[m]] - ma[m] : 0.0;
            b[m] = live && okb[m] ? row[jb[m]] - mb[m] : 0.0;
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[m][n] = M::mma(a[m], b[n], acc[m][n]);
    }
    double* __restrict__ dst = part + (long long)blockIdx.z * Dp * Dp;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = r0 + 16 * m + M::row(lane, r), col = c0 + 16 * n + i;
                if (row < Dp && col < Dp) dst[(long long)row * Dp + col] = acc[m][n][r];
            }
}

// C[i][j] = (sum of the chunk partials, in chunk order) * (1 / T): np.cov(x.T, bias=True).  grid = ceil(D D / 256).
__global__ __launch_bounds__(256) void cov_finish_kernel(const double* __restrict__ part, int nchunks, long long T, int D,
                                                          int Dp, double* __restrict__ C) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= D * D) return;
    const int i = e / D, j = e - i * D;
    double acc = 0.0;
    for (int c = 0; c < nchunks; ++c) acc += part[((long long)c * Dp + i) * Dp + j];
    C[e] = acc * (1.0 / (double)T);
}

// Projection into the PLDA's LDA space with Kaldi's length normalisation (diarization_lib.py:91-92) and the row terms of
// the score (diarization_lib.py:53-56).  One wavefront per 16 rows keeps all dp / 16 <= kPldaMaxTiles output tiles:
//   y = (x - mu) Mx           Mx [Dk][dp]: the host's M [D][d], zero-padded to Dk = D rounded up to 4 rows, dp = d to 16 columns
//   y *= sqrt(d / sum_k y_k^2 w_k)                      w_k = 1 / (acvar_k + 1)
//   a[t][k] = y_k sl_k  (zero for k >= d),  g[t] = sum_k gam_k y_k^2          sl = sqrt(Lambda), gam = Gamma
// w, sl and gam are [dp], zero past d.  grid = ceil(T / 16), block = 64.
__global__ __launch_bounds__(64) void plda_project_kernel(const double* __restrict__ x, long long T, int D, int ld,
                                                           const double* __restrict__ mu, const double* __restrict__ Mx,
                                                           int d, int dp, const double* __restrict__ w,
                                                           const double* __restrict__ sl, const double* __restrict__ gam,
                                                           double* __restrict__ a, double* __restrict__ gout) {
    using M = Mfma16<double>;
    using acc_t = M::acc_t;
    const int lane = threadIdx.x, i = lane & 15, g = lane >> 4;
    const long long row0 = (long long)blockIdx.x * 16;
    const int nt = dp >> 4;
    acc_t acc[kPldaMaxTiles];
#pragma unroll
    for (int n = 0; n < kPldaMaxTiles; ++n) acc[n] = acc_t{0, 0, 0, 0};
    const double* __restrict__ xr = x + min(row0 + i, T - 1) * ld;       // rows past the end are clamped, never stored
    for (int k0 = 0; k0 < D; k0 += 4) {
        const int k = k0 + g;                                              // (k < Dk: the padding rows of Mx are zero)
        const double av = k < D ? xr[k] - mu[k] : 0.0;
        const double* __restrict__ mrow = Mx + (long long)k * dp + i;
#pragma unroll
        for (int n = 0; n < kPldaMaxTiles; ++n)
            if (n < nt) acc[n] = M::mma(av, mrow[16 * n], acc[n]);
    }
    // lane (i, g) holds y[row0 + g + 4 r][16 n + i]: the sums over a row's columns run over n here and over the 16 lanes
    // of a group in the butterfly
    double ss[4] = {0, 0, 0, 0};
#pragma unroll
    for (int n = 0; n < kPldaMaxTiles; ++n)
        if (n < nt) {
            const double wk = w[16 * n + i];
#pragma unroll
            for (int r = 0; r < 4; ++r) ss[r] += acc[n][r] * acc[n][r] * wk;
        }
    double scale[4], gs[4] = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) scale[r] = sqrt((double)d / allreduce_sum<16>(ss[r]));
#pragma unroll
    for (int n = 0; n < kPldaMaxTiles; ++n)
        if (n < nt) {
            const double slk = sl[16 * n + i], gk = gam[16 * n + i];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double y = acc[n][r] * scale[r];
                gs[r] += gk * (y * y);
                const long long row = row0 + M::row(lane, r);
                if (row < T) a[row * dp + 16 * n + i] = y * slk;
            }
        }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double tot = allreduce_sum<16>(gs[r]);
        const long long row = row0 + M::row(lane, r);
        if (i == 0 && row < T) gout[row] = tot;
    }
}

// Rows that are already in LDA space (PLDA_scoring_in_LDA_space): out[t][k] = x[t][k] scale[k] (scale == nullptr: a plain
// copy), zero-padded to dp columns, and q[t] = sum_k gam[k] x[t][k]^2.  One wavefront per row, four rows per workgroup.
__global__ __launch_bounds__(256) void plda_lda_rows_kernel(const double* __restrict__ x, long long T, int D,
                                                             const double* __restrict__ scale, const double* __restrict__ gam,
                                                             int dp, double* __restrict__ out, double* __restrict__ q) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long t = (long long)blockIdx.x * 4 + wave;
    if (t >= T) return;
    double acc = 0.0;
    for (int k = lane; k < dp; k += 64) {
        const double v = k < D ? x[t * D + k] : 0.0;
        if (k < D) acc += v * v * gam[k];
        out[t * dp + k] = k < D ? (scale ? v * scale[k] : v) : 0.0;
    }
    acc = allreduce_sum<64>(acc);
    if (lane == 0) q[t] = acc;
}

// S[i][j] = <a_i, b_j> + (r_i + c_j) + kconst, S [N][M].  a [N][dp], b [M][dp], dp a multiple of 16.  The tiling of
// cos_gemm_kernel: grid = (ceil(M/64), ceil(N/64)), block = 256, wave w owns the 32 x 32 sub-tile (w>>1, w&1); lane group g
// supplies k = 16q + 4g + r for MFMA r of block q, the same k order for both operands.
__global__ __launch_bounds__(256) void plda_score_gemm_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                               const double* __restrict__ rterm, const double* __restrict__ cterm,
                                                               double kconst, double* __restrict__ S, long long N, long long Mc,
                                                               int dp) {
    using M = Mfma16<double>;
    using acc_t = M::acc_t;
    using D4 = Vec<double>::v4;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const long long r0 = (long long)blockIdx.y * 64 + 32 * (wave >> 1), c0 = (long long)blockIdx.x * 64 + 32 * (wave & 1);
    acc_t acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = acc_t{0, 0, 0, 0};
    const double* __restrict__ pa[2];
    const double* __restrict__ pb[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        pa[m] = a + min(r0 + 16 * m + i, N - 1) * dp + 4 * g;      // rows past the end are clamped, never stored
        pb[m] = b + min(c0 + 16 * m + i, Mc - 1) * dp + 4 * g;
    }
    for (int q = 0; q < dp; q += 16) {
        D4 av[2], bv[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            av[m] = *reinterpret_cast<const D4*>(pa[m] + q);
            bv[m] = *reinterpret_cast<const D4*>(pb[m] + q);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][n] = M::mma(av[m][r], bv[n][r], acc[m][n]);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const long long col = c0 + 16 * n + i;
            const double cj = cterm[min(col, Mc - 1)];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long row = r0 + 16 * m + M::row(lane, r);
                if (row < N && col < Mc) {
                    const double rc = rterm[row] + cj;            // the row and the column term meet first ...
                    S[row * Mc + col] = (acc[m][n][r] + rc) + kconst;     // ... then the dot product, then the constant
                }
            }
        }
}

}  // namespace vbx
