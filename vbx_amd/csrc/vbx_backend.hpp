// vbx_backend.hpp -- training the x-vector backend: the passes over N labelled x-vectors behind the LDA
// transform (vbhmm.py:125-129 read backwards: mean1, lda, mean2) and the Kaldi PLDA (ivector-compute-plda) that the chain reads.
//
//   y_t = l2norm(x_t - mean1)                       center_norm          f32 / f64 rows -> f64 rows, a flag where the norm is not > 0
//   sums over the rows of a class / of all rows     seg_colsum + finish  [G][D], through a by-class row index (stable, CSR offsets)
//   out[g] = sum_{t in segment g} r_t r_t^T         seg_moment + finish  [G][D][D] on v_mfma_f64_16x16x4
//   u_t = l2norm(lda^T y_t - mean2)                 xv_gemm_kernel (vbx_frontend.hpp), center_norm in place
//
// Everything is float64 and has the same bits on every run, the rule of cov_partial_kernel (vbx_plda_score.hpp): a segment is cut
// into chunks of kCovChunk rows (a chunk never spans two segments), one workgroup sums one chunk into a partial of its own, and one
// thread per output entry adds the partials of its segment in chunk order.  No atomics.  The second moment is symmetric to the last
// bit for the reason given for plda_score_gemm_kernel: (i, j) and (j, i) run the same fused multiply-adds in the same order.  So
// only the 64 x 64 blocks on and above the diagonal are computed and the finish kernel reads (j, i) for a block below it.
//
// y and u are kept as f64 rows in HBM ([N][Din] and [N][lda_dim] rounded up to 4 columns) and not recomputed inside the statistics
// kernels: the moment kernel reads every row ceil(D / 64) (ceil(D / 64) + 1) / 2 times (out of L2 after the first), and a
// recomputation would put a norm (a full-row reduction) and, for u, a Din x lda_dim product in front of each of those reads.
#pragma once
#include "vbx_device.hpp"
#include "vbx_frontend.hpp"
#include "vbx_plda_score.hpp"

namespace vbx {

constexpr int kBackendMaxDim = 1024;       // D of a second moment, as for vbx_plda_covariance

// y[t][0 .. Kp) = (x[t] - mean) / |x[t] - mean|, zero-padded to Kp; x has row stride ldx.  One wavefront per row, four rows per
// workgroup.  mean == nullptr: no centring.  In place (y == x, ldx == Kp) is allowed: a row is read completely before it is
// written.  bad[t] = 1 where the norm is not > 0 (zero, or a NaN in the row): that row of y is zero, never NaN.
template <typename XT>
__global__ __launch_bounds__(256) void backend_center_norm_kernel(const XT* x, const double* __restrict__ mean, double* y,
                                                                   long long n, int D, int ldx, int Kp, int* __restrict__ bad) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long t = (long long)blockIdx.x * 4 + wave;
    if (t >= n) return;
    double ss = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = (double)x[t * ldx + d] - (mean ? mean[d] : 0.0);
        ss += v * v;
    }
    ss = allreduce_sum<64>(ss);
    const double nrm = sqrt(ss);
    const bool good = nrm > 0.0;
    for (int d0 = 0; d0 < Kp; d0 += 64) {
        const int d = d0 + lane;
        const double v = d < D ? (double)x[t * ldx + d] - (mean ? mean[d] : 0.0) : 0.0;
        if (d < Kp) y[t * Kp + d] = good ? v / nrm : 0.0;
    }
    if (lane == 0) bad[t] = good ? 0 : 1;
}

// first[0] = the lowest t with bad[t] != 0, or -1.  One workgroup: a strided scan per thread, then a tree over LDS.
__global__ __launch_bounds__(256) void backend_first_flag_kernel(const int* __restrict__ bad, long long n, long long* __restrict__ first) {
    __shared__ long long best[256];
    constexpr long long none = 0x7fffffffffffffffll;
    long long mine = none;
    for (long long t = threadIdx.x; t < n; t += 256)
        if (bad[t]) {
            mine = t;                                          // (t ascends: the first hit of a thread is its lowest)
            break;
        }
    best[threadIdx.x] = mine;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && best[threadIdx.x + s] < best[threadIdx.x]) best[threadIdx.x] = best[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) first[0] = best[0] == none ? -1 : best[0];
}

// part[c][j] = sum over the positions p of chunk c = [cbeg[c], cend[c]) of rows[idx[p]][j] (idx == nullptr: rows[p][j]), added in
// position order.  grid = chunks, block = 256 (thread = column, strided).
template <typename XT>
__global__ __launch_bounds__(256) void backend_seg_colsum_kernel(const XT* __restrict__ rows, int ld, int D,
                                                                  const long long* __restrict__ idx, const long long* __restrict__ cbeg,
                                                                  const long long* __restrict__ cend, double* __restrict__ part) {
    const long long p0 = cbeg[blockIdx.x], p1 = cend[blockIdx.x];
    for (int j = threadIdx.x; j < D; j += 256) {
        double acc = 0.0;
        for (long long p = p0; p < p1; ++p) acc += (double)rows[(idx ? idx[p] : p) * ld + j];
        part[(long long)blockIdx.x * D + j] = acc;
    }
}

// out[g][j] = (the partials of the chunks seg_c0[g] .. seg_c0[g + 1] of segment g, added in chunk order) * scale; a segment without
// rows gives zero.  grid = ceil(G D / 256).
__global__ __launch_bounds__(256) void backend_seg_colsum_finish_kernel(const double* __restrict__ part, const long long* __restrict__ seg_c0,
                                                                         long long G, int D, double scale, double* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= G * D) return;
    const long long g = e / D;
    const int j = (int)(e - g * D);
    double acc = 0.0;
    for (long long c = seg_c0[g]; c < seg_c0[g + 1]; ++c) acc += part[c * D + j];
    out[e] = acc * scale;
}

// part[z][i][j] = sum over the rows t of chunk c = c0 + z of x[t][i] x[t][j], [Dp][Dp] per chunk, Dp = D rounded up to 16 (entries
// past D are zero), for the 64 x 64 blocks (by, bx) with bx >= by only.  grid = (nb (nb + 1) / 2, 1, chunks of this launch),
// nb = ceil(D / 64), block = 256: the tiling of cov_partial_kernel -- wave w owns the 32 x 32 sub-tile (w>>1, w&1) = 2 x 2 MFMA tiles;
// the MFMA's k runs over four rows of x, lane group g supplies row t + g.
__global__ __launch_bounds__(256) void backend_seg_moment_kernel(const double* __restrict__ x, int D, int ld, int Dp,
                                                                  const long long* __restrict__ cbeg, const long long* __restrict__ cend,
                                                                  long long c0, double* __restrict__ part) {
    using M = Mfma16<double>;
    using acc_t = M::acc_t;
    const int nb = (D + 63) >> 6;
    int by = 0, rem = blockIdx.x;
    while (rem >= nb - by) {                                     // block pair number -> (by, bx), bx >= by
        rem -= nb - by;
        ++by;
    }
    const int bx = by + rem;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const int r0 = by * 64 + 32 * (wave >> 1), cc0 = bx * 64 + 32 * (wave & 1);
    const long long t0 = cbeg[c0 + blockIdx.z], t1 = cend[c0 + blockIdx.z];    // (never empty: the host makes no chunk without rows)
    acc_t acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = acc_t{0, 0, 0, 0};
    int ja[2], jb[2];
    bool oka[2], okb[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        oka[m] = r0 + 16 * m + i < D;
        okb[m] = cc0 + 16 * m + i < D;
        ja[m] = min(r0 + 16 * m + i, D - 1);                     // columns past the end are clamped and contribute zero
        jb[m] = min(cc0 + 16 * m + i, D - 1);
    }
    for (long long t = t0; t < t1; t += 4) {
        const bool live = t + g < t1;                            // rows past the end of the chunk contribute zero
        const double* __restrict__ row = x + min(t + g, t1 - 1) * ld;
        double a[2], b[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            a[m] = live && oka[m] ? row[ja[m]] : 0.0;
            b[m] = live && okb[m] ? row[jb[m]] : 0.0;
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
                const int row = r0 + 16 * m + M::row(lane, r), col = cc0 + 16 * n + i;
                if (row < Dp && col < Dp) dst[(long long)row * Dp + col] = acc[m][n][r];
            }
}

// out[g][i][j] (+)= the partials of the chunks of segment g that lie in [c0, c1), added in chunk order, for the segments
// g0 .. g0 + ng.  A segment whose first chunk lies before c0 continues from what an earlier launch left in out; so the sum of a
// segment is ((p_0 + p_1) + p_2) + ... whatever the number of launches the partials were produced in.  grid = ceil(ng D D / 256).
__global__ __launch_bounds__(256) void backend_seg_moment_finish_kernel(const double* __restrict__ part, const long long* __restrict__ seg_c0,
                                                                         long long g0, long long ng, long long c0, long long c1, int D,
                                                                         int Dp, double* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x, DD = (long long)D * D;
    if (e >= ng * DD) return;
    const long long g = g0 + e / DD;
    const int ij = (int)(e % DD);
    int i = ij / D, j = ij - i * D;
    if ((i >> 6) > (j >> 6)) {                                   // a block below the diagonal: its mirror image was computed
        const int s = i;
        i = j;
        j = s;
    }
    const long long s0 = seg_c0[g], s1 = seg_c0[g + 1], lo = s0 > c0 ? s0 : c0, hi = s1 < c1 ? s1 : c1;
    double* __restrict__ o = out + g * DD + ij;
    double acc = s0 < c0 ? *o : 0.0;
    for (long long c = lo; c < hi; ++c) acc += part[((c - c0) * Dp + i) * Dp + j];
    *o = acc;
}

}  // namespace vbx

extern "C++" {
namespace {

// The chunks of G segments given by ascending offsets: chunk c covers the positions [cbeg[c], cend[c]) of one segment, the chunks
// of segment g are seg_c0[g] .. seg_c0[g + 1].
struct SegPlan {
    std::vector<long long> cbeg, cend, seg_c0;
    long long G = 0;
    long long chunks() const { return (long long)cbeg.size(); }
};

SegPlan seg_plan(const int64_t* off, int64_t G) {
    SegPlan p;
    p.G = G;
    p.seg_c0.resize((size_t)G + 1);
    for (int64_t g = 0; g < G; ++g) {
        p.seg_c0[(size_t)g] = p.chunks();
        for (long long t = off[g]; t < off[g + 1]; t += vbx::kCovChunk) {
            p.cbeg.push_back(t);
            p.cend.push_back(std::min<long long>(t + vbx::kCovChunk, off[g + 1]));
        }
    }
    p.seg_c0[(size_t)G] = p.chunks();
    return p;
}

// the plan on the device, in blocks of `call` (the plan outlives the call: its copies read it)
struct DevPlan {
    const long long *cbeg = nullptr, *cend = nullptr, *seg_c0 = nullptr;
};
DevPlan upload_plan(DeviceCall& call, const SegPlan& p) {
    DevPlan d;
    if (p.chunks()) {
        d.cbeg = call.upload(p.cbeg.data(), p.cbeg.size());
        d.cend = call.upload(p.cend.data(), p.cend.size());
    }
    d.seg_c0 = call.upload(p.seg_c0.data(), p.seg_c0.size());
    return d;
}

// d_out[g][j] = scale * sum over the rows of segment g, rows taken through d_idx (or in place where it is nullptr)
template <typename XT>
void launch_seg_colsum(DeviceCall& call, const XT* d_rows, int ld, int D, const long long* d_idx, const SegPlan& p, const DevPlan& dp,
                       double scale, double* d_out) {
    double* d_part = p.chunks() ? call.alloc<double>((size_t)p.chunks() * D) : nullptr;
    if (!call.ok()) return;
    if (p.chunks())
        hipLaunchKernelGGL((vbx::backend_seg_colsum_kernel<XT>), dim3((unsigned)p.chunks()), dim3(256), 0, call.st, d_rows, ld, D, d_idx,
                           dp.cbeg, dp.cend, d_part);
    hipLaunchKernelGGL(vbx::backend_seg_colsum_finish_kernel, dim3((unsigned)((p.G * D + 255) / 256)), dim3(256), 0, call.st,
                       (const double*)d_part, dp.seg_c0, p.G, D, scale, d_out);
    call.launched();
}

// d_out[g] = sum over the rows of segment g of r r^T, [G][D][D].  The partials of at most kMomentPartBytes are live at a time.
constexpr size_t kMomentPartBytes = (size_t)256 << 20;
void launch_seg_moment(DeviceCall& call, const double* d_rows, int ld, int D, const SegPlan& p, const DevPlan& dp, double* d_out) {
    const int Dp = round_up(D, 16), nb = (D + 63) / 64;
    const long long per = (long long)Dp * Dp, nch = p.chunks();
    long long batch = std::max<long long>(1, std::min<long long>(32768, (long long)(kMomentPartBytes / (sizeof(double) * per))));
    if (const char* e = experiment_env("VBX_AMD_BACKEND_BATCH_CHUNKS"))      // (the result does not depend on it: a test says so)
        if (std::atoll(e) >= 1) batch = std::min<long long>(batch, std::atoll(e));
    double* d_part = nch ? call.alloc<double>((size_t)(std::min(batch, nch) * per)) : nullptr;
    if (!call.ok()) return;
    call.enqueued(hipMemsetAsync(d_out, 0, sizeof(double) * (size_t)p.G * D * D, call.st));     // (segments without rows)
    long long g0 = 0;
    for (long long c0 = 0; c0 < nch && call.ok(); c0 += batch) {
        const long long c1 = std::min(c0 + batch, nch);
        while (p.seg_c0[(size_t)g0 + 1] <= c0) ++g0;            // the first segment with a chunk in [c0, c1) ...
        long long g1 = g0;
        while (g1 + 1 < p.G && p.seg_c0[(size_t)g1 + 1] < c1) ++g1;      // ... and the last
        const long long ng = g1 - g0 + 1;
        hipLaunchKernelGGL(vbx::backend_seg_moment_kernel, dim3((unsigned)(nb * (nb + 1) / 2), 1, (unsigned)(c1 - c0)), dim3(256), 0,
                           call.st, d_rows, D, ld, Dp, dp.cbeg, dp.cend, c0, d_part);
        hipLaunchKernelGGL(vbx::backend_seg_moment_finish_kernel, dim3((unsigned)((ng * D * D + 255) / 256)), dim3(256), 0, call.st,
                           (const double*)d_part, dp.seg_c0, g0, ng, c0, c1, D, Dp, d_out);
        call.launched();
    }
}

// class_of_row [N] in [0, K), no class without a row: counts [K], CSR offsets [K + 1] and the rows by class in archive order
// (a counting sort: stable).  The first fault is described in `msg`.
bool class_index_ok(std::string& msg, const char* fn, int64_t N, int32_t K, const int32_t* class_of_row, std::vector<int64_t>& off,
                    std::vector<long long>& order) {
    char buf[256];
    buf[0] = 0;
    off.assign((size_t)K + 1, 0);
    for (int64_t t = 0; t < N; ++t) {
        if (class_of_row[t] < 0 || class_of_row[t] >= K) {
            snprintf(buf, sizeof buf, "%s: class %d of row %lld outside [0, %d)", fn, class_of_row[t], (long long)t, K);
            msg = buf;
            return false;
        }
        ++off[(size_t)class_of_row[t] + 1];
    }
    for (int32_t k = 0; k < K; ++k) {
        if (off[(size_t)k + 1] == 0) {
            snprintf(buf, sizeof buf, "%s: class %d has no row", fn, k);
            msg = buf;
            return false;
        }
        off[(size_t)k + 1] += off[(size_t)k];
    }
    order.resize((size_t)N);
    std::vector<int64_t> at(off.begin(), off.end() - 1);
    for (int64_t t = 0; t < N; ++t) order[(size_t)at[(size_t)class_of_row[t]]++] = t;
    return true;
}

}  // namespace
}  // extern "C++"

// x-vectors and their classes resident in HBM across the two stages of the recipe
struct vbx_backend {
    vbx_ctx* ctx = nullptr;
    long long N = 0;
    int Din = 0, Kp = 0, K = 0, x_dtype = VBX_F32;
    void* d_x = nullptr;                       // [N][Din] f32 or f64, as it came
    long long* d_order = nullptr;              // rows by class, archive order inside a class
    double* d_y = nullptr;                     // [N][Kp] after stage 1
    bool have_y = false;
    std::vector<int64_t> class_off;            // [K + 1]
    SegPlan by_class, all_rows;
};

extern "C" {

int vbx_backend_destroy(vbx_backend* be) {
    if (!be) return VBX_OK;
    (void)hipSetDevice(be->ctx->device);
    (void)hipStreamSynchronize(be->ctx->stream);
    ctx_free(be->ctx, be->d_x);
    ctx_free(be->ctx, be->d_order);
    ctx_free(be->ctx, be->d_y);
    delete be;
    return VBX_OK;
}

int vbx_backend_create(vbx_ctx* ctx, int64_t N, int32_t Din, const void* x, int x_dtype, int32_t K, const int32_t* class_of_row,
                       vbx_backend** out) {
    if (!ctx) {
        g_create_error = "vbx_backend_create: NULL context";
        return VBX_ERR_INVALID;
    }
    if (!x || !class_of_row || !out) FAIL(ctx, VBX_ERR_INVALID, "vbx_backend_create: NULL input");
    *out = nullptr;
    if (N < 1 || Din < 1 || K < 1 || Din > vbx::kBackendMaxDim)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_backend_create: N=%lld rows, D=%d dimensions, K=%d classes: all must be >= 1 and D <= %d",
             (long long)N, Din, K, vbx::kBackendMaxDim);
    if (x_dtype != VBX_F32 && x_dtype != VBX_F64) FAIL(ctx, VBX_ERR_INVALID, "vbx_backend_create: x must be f32 or f64");
    std::vector<long long> order;
    std::vector<int64_t> off;
    if (!class_index_ok(ctx->err, "vbx_backend_create", N, K, class_of_row, off, order)) return VBX_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    vbx_backend* be = new vbx_backend();
    be->ctx = ctx;
    be->N = N;
    be->Din = Din;
    be->Kp = round_up(Din, 4);
    be->K = K;
    be->x_dtype = x_dtype;
    be->class_off = off;
    be->by_class = seg_plan(off.data(), K);
    const int64_t all[2] = {0, N};
    be->all_rows = seg_plan(all, 1);
    const size_t xbytes = (size_t)N * Din * (x_dtype == VBX_F64 ? 8 : 4);
    int rc;
    {
        DeviceCall call(ctx);
        char* d_x = nullptr;
        if (call.ok()) call.rc = dmalloc(ctx, &d_x, xbytes);
        be->d_x = d_x;
        if (call.ok()) call.rc = dmalloc(ctx, &be->d_order, (size_t)N);
        if (call.ok()) call.rc = dmalloc(ctx, &be->d_y, (size_t)N * be->Kp);
        call.copy_in(d_x, static_cast<const char*>(x), xbytes);
        call.copy_in(be->d_order, (const long long*)order.data(), (size_t)N);
        call.sync();
        rc = call.finish("vbx_backend_create failed");
    }
    if (rc != VBX_OK) {
        vbx_backend_destroy(be);
        return rc;
    }
    *out = be;
    return VBX_OK;
}

}  // extern "C"

extern "C++" {
namespace {

// the kernels of a stage between two events: *ms = their time on the device
struct StageClock {
    hipEvent_t a = nullptr, b = nullptr;
    DeviceCall& call;
    explicit StageClock(DeviceCall& c, bool on) : call(c) {
        if (!on) return;
        call.note(hipEventCreate(&a));
        call.note(hipEventCreate(&b));
        if (call.ok()) call.note(hipEventRecord(a, call.st));
    }
    void stop() {
        if (b && call.ok()) call.note(hipEventRecord(b, call.st));
    }
    void read(double* ms) {                                     // after the stream has been synchronized
        float t = 0.f;
        if (a && b && call.ok()) call.note(hipEventElapsedTime(&t, a, b));
        if (ms) *ms = (double)t;
    }
    ~StageClock() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

// the class sums [K][D] and the second moment [D][D] of the resident rows d_r [N][ld], into host arrays
void launch_class_stats(DeviceCall& call, vbx_backend* be, const double* d_r, int ld, int D, const DevPlan& by_class, const DevPlan& all_rows,
                        double* class_sums, double* moment) {
    double* d_cs = call.alloc<double>((size_t)be->K * D);
    double* d_m2 = call.alloc<double>((size_t)D * D);
    launch_seg_colsum<double>(call, d_r, ld, D, be->d_order, be->by_class, by_class, 1.0, d_cs);
    launch_seg_moment(call, d_r, ld, D, be->all_rows, all_rows, d_m2);
    call.download(class_sums, (const double*)d_cs, (size_t)be->K * D);
    call.download(moment, (const double*)d_m2, (size_t)D * D);
}

}  // namespace
}  // extern "C++"

extern "C" {

int vbx_backend_stage1(vbx_backend* be, double* mean1, double* class_sums, double* moment, double* kernel_ms) {
    if (!be) return VBX_ERR_INVALID;
    vbx_ctx* ctx = be->ctx;
    if (!mean1 || !class_sums || !moment) FAIL(ctx, VBX_ERR_INVALID, "vbx_backend_stage1: NULL output");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long long N = be->N;
    const int D = be->Din;
    long long first_bad = -1;
    int rc;
    {
        DeviceCall call(ctx);
        const DevPlan by_class = upload_plan(call, be->by_class), all_rows = upload_plan(call, be->all_rows);
        double* d_mean = call.alloc<double>((size_t)D);
        int* d_bad = call.alloc<int>((size_t)N);
        long long* d_first = call.alloc<long long>(1);
        StageClock clock(call, kernel_ms != nullptr);
        const dim3 rows((unsigned)((N + 3) / 4));
        if (be->x_dtype == VBX_F64) {
            launch_seg_colsum<double>(call, (const double*)be->d_x, D, D, nullptr, be->all_rows, all_rows, 1.0 / (double)N, d_mean);
            if (call.ok())
                hipLaunchKernelGGL((vbx::backend_center_norm_kernel<double>), rows, dim3(256), 0, call.st, (const double*)be->d_x,
                                   (const double*)d_mean, be->d_y, N, D, D, be->Kp, d_bad);
        } else {
            launch_seg_colsum<float>(call, (const float*)be->d_x, D, D, nullptr, be->all_rows, all_rows, 1.0 / (double)N, d_mean);
            if (call.ok())
                hipLaunchKernelGGL((vbx::backend_center_norm_kernel<float>), rows, dim3(256), 0, call.st, (const float*)be->d_x,
                                   (const double*)d_mean, be->d_y, N, D, D, be->Kp, d_bad);
        }
        if (call.ok()) {
            hipLaunchKernelGGL(vbx::backend_first_flag_kernel, dim3(1), dim3(256), 0, call.st, (const int*)d_bad, N, d_first);
            call.launched();
        }
        launch_class_stats(call, be, be->d_y, be->Kp, D, by_class, all_rows, class_sums, moment);
        clock.stop();
        call.download(mean1, (const double*)d_mean, (size_t)D);
        call.download(&first_bad, (const long long*)d_first, 1);
        call.sync();
        clock.read(kernel_ms);
        rc = call.finish("vbx_backend_stage1 failed");
    }
    if (rc != VBX_OK) return rc;
    if (first_bad >= 0)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_backend_stage1: row %lld has no length after centring (it equals the mean, or holds a NaN)", first_bad);
    be->have_y = true;
    return VBX_OK;
}

int vbx_backend_stage2(vbx_backend* be, int32_t Dl, const double* lda, const double* mean2, double* class_sums, double* moment,
                       double* kernel_ms) {
    if (!be) return VBX_ERR_INVALID;
    vbx_ctx* ctx = be->ctx;
    if (!lda || !mean2 || !class_sums || !moment) FAIL(ctx, VBX_ERR_INVALID, "vbx_backend_stage2: NULL input");
    if (Dl < 1 || Dl > be->Din) FAIL(ctx, VBX_ERR_INVALID, "vbx_backend_stage2: lda_dim=%d outside [1, %d]", Dl, be->Din);
    if (!be->have_y) FAIL(ctx, VBX_ERR_INVALID, "vbx_backend_stage2: stage 1 has not run");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long long N = be->N;
    const int Kp = be->Kp, Np = round_up(Dl, 16), Kp2 = round_up(Dl, 4);
    std::vector<double> ldap((size_t)Kp * Np, 0.0), m2p((size_t)Np, 0.0);       // lda [Kp][Np], zero-padded
    for (int k = 0; k < be->Din; ++k)
        for (int c = 0; c < Dl; ++c) ldap[(size_t)k * Np + c] = lda[(size_t)k * Dl + c];
    for (int c = 0; c < Dl; ++c) m2p[(size_t)c] = mean2[c];
    long long first_bad = -1;
    int rc;
    {
        DeviceCall call(ctx);
        const DevPlan by_class = upload_plan(call, be->by_class), all_rows = upload_plan(call, be->all_rows);
        const double* d_lda = call.upload(ldap.data(), ldap.size());
        const double* d_m2 = call.upload(m2p.data(), m2p.size());
        double* d_u = call.alloc<double>((size_t)N * Kp2);
        int* d_bad = call.alloc<int>((size_t)N);
        long long* d_first = call.alloc<long long>(1);
        StageClock clock(call, kernel_ms != nullptr);
        if (call.ok()) {
            hipLaunchKernelGGL(vbx::xv_gemm_kernel, dim3((unsigned)((N + 63) / 64)), dim3(256), 0, call.st, (const double*)be->d_y, d_lda, d_m2,
                               d_u, N, Kp, Np, (int)Dl, Kp2);
            // (in place; the columns Dl .. Kp2 become zero)
            hipLaunchKernelGGL((vbx::backend_center_norm_kernel<double>), dim3((unsigned)((N + 3) / 4)), dim3(256), 0, call.st,
                               (const double*)d_u, (const double*)nullptr, d_u, N, (int)Dl, Kp2, Kp2, d_bad);
            hipLaunchKernelGGL(vbx::backend_first_flag_kernel, dim3(1), dim3(256), 0, call.st, (const int*)d_bad, N, d_first);
            call.launched();
        }
        launch_class_stats(call, be, d_u, Kp2, Dl, by_class, all_rows, class_sums, moment);
        clock.stop();
        call.download(&first_bad, (const long long*)d_first, 1);
        call.sync();
        clock.read(kernel_ms);
        rc = call.finish("vbx_backend_stage2 failed");
    }
    if (rc != VBX_OK) return rc;
    if (first_bad >= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_backend_stage2: row %lld has no length after the projection", first_bad);
    return VBX_OK;
}

int vbx_backend_class_sums(vbx_ctx* ctx, int64_t N, int32_t D, const void* x, int x_dtype, int32_t K, const int32_t* class_of_row,
                           double* sums, int64_t* counts) {
    if (!ctx) {
        g_create_error = "vbx_backend_class_sums: NULL context";
        return VBX_ERR_INVALID;
    }
    if (!x || !class_of_row || !sums) FAIL(ctx, VBX_ERR_INVALID, "vbx_backend_class_sums: NULL input");
    if (N < 1 || D < 1 || K < 1 || D > vbx::kBackendMaxDim)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_backend_class_sums: N=%lld rows, D=%d dimensions, K=%d classes: all must be >= 1 and D <= %d",
             (long long)N, D, K, vbx::kBackendMaxDim);
    if (x_dtype != VBX_F32 && x_dtype != VBX_F64) FAIL(ctx, VBX_ERR_INVALID, "vbx_backend_class_sums: x must be f32 or f64");
    std::vector<long long> order;
    std::vector<int64_t> off;
    if (!class_index_ok(ctx->err, "vbx_backend_class_sums", N, K, class_of_row, off, order)) return VBX_ERR_INVALID;
    for (int32_t k = 0; counts && k < K; ++k) counts[k] = off[(size_t)k + 1] - off[(size_t)k];
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const SegPlan plan = seg_plan(off.data(), K);
    DeviceCall call(ctx);
    const DevPlan dp = upload_plan(call, plan);
    const char* d_x = call.upload(static_cast<const char*>(x), (size_t)N * D * (x_dtype == VBX_F64 ? 8 : 4));
    const long long* d_order = call.upload((const long long*)order.data(), (size_t)N);
    double* d_out = call.alloc<double>((size_t)K * D);
    if (x_dtype == VBX_F64)
        launch_seg_colsum<double>(call, (const double*)d_x, D, D, d_order, plan, dp, 1.0, d_out);
    else
        launch_seg_colsum<float>(call, (const float*)d_x, D, D, d_order, plan, dp, 1.0, d_out);
    call.download(sums, (const double*)d_out, (size_t)K * D);
    call.sync();
    return call.finish("vbx_backend_class_sums failed");
}

int vbx_backend_second_moments(vbx_ctx* ctx, int64_t R, int32_t D, const double* rows, int64_t G, const int64_t* offsets, double* out) {
    if (!ctx) {
        g_create_error = "vbx_backend_second_moments: NULL context";
        return VBX_ERR_INVALID;
    }
    if (!rows || !offsets || !out) FAIL(ctx, VBX_ERR_INVALID, "vbx_backend_second_moments: NULL input");
    if (R < 1 || D < 1 || G < 1 || D > vbx::kBackendMaxDim)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_backend_second_moments: R=%lld rows, D=%d dimensions, G=%lld segments: all must be >= 1 and D <= %d",
             (long long)R, D, (long long)G, vbx::kBackendMaxDim);
    if (offsets[0] < 0 || offsets[G] > R)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_backend_second_moments: offsets [%lld, %lld] leave the %lld rows", (long long)offsets[0],
             (long long)offsets[G], (long long)R);
    for (int64_t g = 0; g < G; ++g)
        if (offsets[g + 1] < offsets[g])
            FAIL(ctx, VBX_ERR_INVALID, "vbx_backend_second_moments: offsets[%lld] = %lld does not ascend (offsets[%lld] = %lld)",
                 (long long)(g + 1), (long long)offsets[g + 1], (long long)g, (long long)offsets[g]);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const SegPlan plan = seg_plan(offsets, G);
    DeviceCall call(ctx);
    const DevPlan dp = upload_plan(call, plan);
    const double* d_rows = call.upload(rows, (size_t)R * D);
    double* d_out = call.alloc<double>((size_t)G * D * D);
    launch_seg_moment(call, d_rows, D, D, plan, dp, d_out);
    call.download(out, (const double*)d_out, (size_t)G * D * D);
    call.sync();
    return call.finish("vbx_backend_second_moments failed");
}

}  // extern "C"
