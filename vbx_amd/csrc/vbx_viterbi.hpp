// vbx_viterbi.hpp -- the jointly most probable state sequence of the VB-HMM (max-product): the kernels,
// vbx_viterbi and vbx_batch_get_path.
// (one translation unit with vbx_capi.hip, which includes it after the host runtime; not a stand-alone header)
//
// The model is forward_backward's (VBx.py:98, 158-164): tr = loopProb I + (1 - loopProb) 1 pi^T, eps = 1e-8 added to tr and to
// ip before the logarithm.  With stay_j = log(loopProb + (1 - loopProb) pi_j + eps), move_j = log((1 - loopProb) pi_j + eps)
// and lip_j = log(ip_j + eps):
//   d_0(j) = lls[0][j] + lip_j
//   t >= 1:  m = max_i d_{t-1}(i),  a_t = the lowest index that attains it,
//            d_t(j) = lls[t][j] + max(d_{t-1}(j) - m + stay_j, move_j)
// stay_j >= move_j, so the maximum over i != j may run over all i: one wave-wide maximum per frame instead of an S x S
// max-plus product, and d stays of the size of one frame's log-likelihoods.  Back-pointer of (t, j): "stayed" iff
// d_{t-1}(j) - m + stay_j >= move_j (equality stays), else the path came from a_t: one bit per state and frame, one index per
// frame.  path[T-1] = the lowest index attaining max_j d_{T-1}(j); logp = the sum of the subtracted m + that last maximum.
#pragma once
#include "vbx_device.hpp"

namespace vbx {

constexpr int kVitMaxStates = 1024;   // 16 states per lane of one wavefront
constexpr int kVitLoads = 16;         // loads of one ring slot: 16 / K frames of K loads each
constexpr int kVitBlock = 64;         // frames of one back-trace block

// One recording.  `in` holds T rows of `stride` values: log-likelihoods, or (LOGB) the b = exp(l - m_t) of a batch, taken as
// log b.  Scratch: T K back-pointer words and T indices; path [T] on the device.
struct VitJob {
    const void* in;
    long long stride, T;
    int S;
    const double *pi, *ip;
    double lp;
    unsigned long long* words;
    int* amax;
    int* path;
    double* logp;             // or nullptr
};

template <bool LOGB> __device__ __forceinline__ double vit_emission(double v) { return LOGB ? log(v) : v; }
template <bool LOGB> __device__ __forceinline__ double vit_emission(float v) { return (double)(LOGB ? logf(v) : v); }

// One wavefront per recording; state s = 64 r + lane, r < K.  The frame-to-frame chain is a subtract, an add, a maximum, an
// add, the wave-wide maximum and the ballots that find a_t; nothing on it waits for memory:
//   * rows of `in` are requested two ring slots (2 * 16 / K frames, at least 2) ahead into registers -- three slots of 16 loads
//     keep the requests in flight, with the stores below, under the 63 the wait counter can tell apart;
//   * the back-pointer words and a_t of a slot's frames are gathered in one register each (lane f K + r / lane f) and leave
//     in two plain vector stores per slot that nothing waits for before the back-trace.
// The back-trace follows in the same launch: blocks of 64 frames from the end, words and indices of a block staged in
// LDS, 64 dependent steps on wave-uniform values there, the block's labels stored coalesced.
template <typename IN, bool LOGB, int K>
__global__ __launch_bounds__(64) void viterbi_kernel(VitJob job) {
    constexpr int B = kVitLoads / K;
    static_assert(B >= 1 && B * K == kVitLoads, "K divides the loads of a ring slot");
    __shared__ unsigned long long lw[kVitBlock * K];
    __shared__ int la[kVitBlock];
    const int lane = threadIdx.x;
    const IN* __restrict__ in = (const IN*)job.in;
    const long long T = job.T, stride = job.stride;
    const int S = job.S;

    double stay[K], move[K], d[K];
    int col[K];
    bool live[K];
    {
        IN e0[K];
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int s = 64 * r + lane;
            live[r] = s < S;
            col[r] = live[r] ? s : S - 1;                     // (a padded state reads the last real column and drops it)
            e0[r] = in[col[r]];
        }
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const double pj = job.pi[col[r]], ipj = job.ip[col[r]];
            move[r] = log((1.0 - job.lp) * pj + 1e-8);
            stay[r] = log(job.lp + (1.0 - job.lp) * pj + 1e-8);
            d[r] = live[r] ? vit_emission<LOGB>(e0[r]) + log(ipj + 1e-8) : -INFINITY;
        }
    }

    // the wave-wide maximum of d and the lowest state that attains it: lowest r first, then lowest lane
    auto best = [&](double& m, int& a) {
        double lm = d[0];
#pragma unroll
        for (int r = 1; r < K; ++r) lm = vmax(lm, d[r]);
        m = allreduce_max<64>(lm);
        a = 0;
#pragma unroll
        for (int r = K - 1; r >= 0; --r) {
            const unsigned long long hit = __ballot(d[r] == m);
            if (hit) a = 64 * r + (int)__builtin_ctzll(hit);
        }
    };

    double sum = 0.0, comp = 0.0;                             // logp: compensated, the sum of T terms must not cost T roundings
    auto fetch = [&](IN (&dst)[B][K], long long blk) {        // frames 1 + blk B + f; past the end: the last row again
#pragma unroll
        for (int f = 0; f < B; ++f) {
            const long long t = 1 + blk * B + f;
            const IN* __restrict__ row = in + (t < T ? t : T - 1) * stride;
#pragma unroll
            for (int r = 0; r < K; ++r) dst[f][r] = row[col[r]];
        }
    };
    auto run = [&](const IN (&src)[B][K], long long blk) {
        const long long t0 = 1 + blk * B;
        if (t0 >= T) return;
        unsigned long long wreg = 0;
        int areg = 0;
#pragma unroll
        for (int f = 0; f < B; ++f) {
            if (t0 + f < T) {
                double m;
                int a;
                best(m, a);
                const double y = m - comp, s2 = sum + y;
                comp = (s2 - sum) - y;
                sum = s2;
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    const double sv = d[r] - m + stay[r];
                    const bool stayed = sv >= move[r];
                    const unsigned long long word = __ballot(stayed);
                    if (lane == f * K + r) wreg = word;
                    const double e = live[r] ? vit_emission<LOGB>(src[f][r]) : -INFINITY;
                    d[r] = e + (stayed ? sv : move[r]);
                }
                if (lane == f) areg = a;
            }
        }
        if (lane < B * K && t0 + lane / K < T) job.words[t0 * K + lane] = wreg;
        if (lane < B && t0 + lane < T) job.amax[t0 + lane] = areg;
    };

    {
        IN b0[B][K], b1[B][K], b2[B][K];
        const long long nblk = (T - 1 + B - 1) / B;
        fetch(b0, 0);
        fetch(b1, 1);
        for (long long blk = 0; blk < nblk; blk += 3) {
            fetch(b2, blk + 2);
            run(b0, blk);
            fetch(b0, blk + 3);
            run(b1, blk + 1);
            fetch(b1, blk + 4);
            run(b2, blk + 2);
        }
    }
    double mlast;
    int p;
    best(mlast, p);
    if (job.logp && lane == 0) *job.logp = (sum + mlast) - comp;

    // ------------------------------------------------------------------------------------------ back-trace
    __threadfence();                                          // the words and indices were stored by other lanes of this wave
    p = __builtin_amdgcn_readfirstlane(p);
    for (long long lo = (T - 1) / kVitBlock * kVitBlock; lo >= 0; lo -= kVitBlock) {
        const int n = (int)(T - lo < kVitBlock ? T - lo : kVitBlock);
        for (int i = lane; i < n * K; i += 64)
            if (lo * K + i >= K) lw[i] = job.words[lo * K + i];          // (frame 0 has no back-pointers)
        if (lane < n && lo + lane >= 1) la[lane] = job.amax[lo + lane];
        __syncthreads();
        int mine = 0;
        for (int f = n - 1; f >= 0; --f) {
            if (lane == f) mine = p;
            if (lo + f == 0) break;
            const unsigned long long w = lw[f * K + (p >> 6)];
            const unsigned bit = (unsigned)(w >> (p & 63)) & 1u;
            p = __builtin_amdgcn_readfirstlane(bit ? p : la[f]);
        }
        if (lane < n) job.path[lo + lane] = mine;
        __syncthreads();
    }
}

// second[t] = the speaker of the largest gamma[t][s] among s != first[t], the lowest index among equals; -1 when S == 1
// (top2_kernel's second place with the first place given: the decoded path)
template <typename R>
__global__ __launch_bounds__(256) void second_to_path_kernel(const R* __restrict__ gamma, const int* __restrict__ first,
                                                              int* __restrict__ second, long long T, int S, int Sp) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const R* __restrict__ row = gamma + t * Sp;
    const int skip = first[t];
    int i2 = -1;
    R v2 = 0;
    for (int s = 0; s < S; ++s) {
        const R v = row[s];
        if (s != skip && (i2 < 0 || v > v2)) {
            i2 = s; v2 = v;
        }
    }
    second[t] = i2;
}

}  // namespace vbx

namespace {

// the instance for S states: K = 1, 2, 4, 8, 16 states per lane (= back-pointer words per frame)
inline int viterbi_words_per_frame(int S) {
    int k = 1;
    while (64 * k < S) k *= 2;
    return k;
}
template <typename IN, bool LOGB> void launch_viterbi(hipStream_t st, const VitJob& job) {
    (void)dispatch_int<1, 2, 4, 8, 16>(viterbi_words_per_frame(job.S), [&](auto k) {
        hipLaunchKernelGGL((viterbi_kernel<IN, LOGB, decltype(k)::value>), dim3(1), dim3(64), 0, st, job);
    });
}

// device time of the last decode of this thread between two events on its stream (vbx_viterbi_last_ms): the kernels alone,
// without the copies either side
thread_local double g_viterbi_ms = 0.0;
struct DecodeTimer {
    hipStream_t st;
    hipEvent_t a = nullptr, b = nullptr;
    explicit DecodeTimer(hipStream_t st_) : st(st_) {
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) a = b = nullptr;
    }
    ~DecodeTimer() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    void begin() { if (b) (void)hipEventRecord(a, st); }
    void end() { if (b) (void)hipEventRecord(b, st); }
    void read() {                                             // after the stream has been waited for
        float ms = 0.f;
        g_viterbi_ms = (b && hipEventElapsedTime(&ms, a, b) == hipSuccess) ? ms : 0.0;
    }
};

template <typename R> int get_path_impl(vbx_batch* b, int rec, int32_t* first, int32_t* second) {
    vbx_ctx* ctx = b->ctx;
    const RecDesc& rd = b->recs[rec];
    const long long T = rd.T;
    const int K = viterbi_words_per_frame(rd.S);
    DeviceCall call(ctx);
    VitJob job;
    job.in = (const R*)b->d_bmat + rd.row0 * b->Sp;           // b of the last E-step: in HBM under every launch plan
    job.stride = b->Sp;
    job.T = T;
    job.S = rd.S;
    job.pi = job.ip = b->d_pi_prev + (size_t)rec * b->Sp;     // the priors that E-step ran with (fin_kernel); ip = pi (VBx.py:99)
    job.lp = rd.lp;
    job.words = call.alloc<unsigned long long>((size_t)T * K);
    job.amax = call.alloc<int>((size_t)T);
    job.path = call.alloc<int>((size_t)2 * T);
    job.logp = nullptr;
    DecodeTimer timer(call.st);
    if (call.ok()) {
        timer.begin();
        launch_viterbi<R, true>(call.st, job);
        if (second)
            hipLaunchKernelGGL((second_to_path_kernel<R>), dim3((unsigned)((T + 255) / 256)), dim3(256), 0, call.st,
                               (const R*)b->d_gamma + rd.row0 * b->Sp, (const int*)job.path, job.path + T, T, rd.S, b->Sp);
        timer.end();
        call.launched();
    }
    if (first) call.download(first, (const int32_t*)job.path, (size_t)T);
    if (second) call.download(second, (const int32_t*)job.path + T, (size_t)T);
    call.sync();
    if (call.ok()) timer.read();
    return call.finish("vbx_batch_get_path: the decode failed");
}

int leaf_get_path(vbx_batch* b, int rec, int32_t* first, int32_t* second) {
    vbx_ctx* ctx = b->ctx;
    if (rec < 0 || rec >= b->n_rec) FAIL(ctx, VBX_ERR_INVALID, "recording index %d out of range", rec);
    if (!b->has_run) FAIL(ctx, VBX_ERR_STATE, "vbx_batch_get_path: the batch has not run");
    if (b->recs[rec].S > kVitMaxStates)
        FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_batch_get_path: S=%d states, the decode takes at most %d", b->recs[rec].S, kVitMaxStates);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = fetch_mirrors(b); rc != VBX_OK) return rc;
    if (b->h_state[rec].n_iters < 1)
        FAIL(ctx, VBX_ERR_STATE, "vbx_batch_get_path: recording %d has run no iteration: there is no E-step to decode", rec);
    return with_precision(b->precision, [&](auto r) { return get_path_impl<decltype(r)>(b, rec, first, second); });
}

}  // namespace

extern "C" {

int vbx_viterbi(vbx_ctx* ctx, int64_t T, int32_t S, const double* lls, const double* pi, const double* ip, double loopProb,
                int32_t* path, double* logp) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!lls || !pi) FAIL(ctx, VBX_ERR_INVALID, "vbx_viterbi: NULL lls or pi");
    if (T < 1 || S < 1) FAIL(ctx, VBX_ERR_INVALID, "vbx_viterbi: T=%lld, S=%d: both must be at least 1", (long long)T, S);
    if (!(loopProb >= 0.0 && loopProb <= 1.0)) FAIL(ctx, VBX_ERR_INVALID, "vbx_viterbi: loopProb=%g outside [0, 1]", loopProb);
    if (S > kVitMaxStates) FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_viterbi: S=%d states, the decode takes at most %d", S, kVitMaxStates);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int K = viterbi_words_per_frame(S);
    DeviceCall call(ctx);
    VitJob job;
    job.in = call.upload(lls, (size_t)T * S);
    job.stride = S;
    job.T = T;
    job.S = S;
    job.pi = call.upload(pi, (size_t)S);
    job.ip = ip ? call.upload(ip, (size_t)S) : job.pi;
    job.lp = loopProb;
    job.words = call.alloc<unsigned long long>((size_t)T * K);
    job.amax = call.alloc<int>((size_t)T);
    job.path = call.alloc<int>((size_t)T);
    job.logp = call.alloc<double>(1);
    DecodeTimer timer(call.st);
    if (call.ok()) {
        timer.begin();
        launch_viterbi<double, false>(call.st, job);
        timer.end();
        call.launched();
    }
    if (path) call.download(path, (const int32_t*)job.path, (size_t)T);
    if (logp) call.download(logp, (const double*)job.logp, (size_t)1);
    call.sync();
    if (call.ok()) timer.read();
    return call.finish("vbx_viterbi: the decode failed");
}

double vbx_viterbi_last_ms(void) { return g_viterbi_ms; }

int vbx_batch_get_path(vbx_batch* b, int rec, int32_t* first, int32_t* second) {
    if (!b) return VBX_ERR_INVALID;
    if (b->kids.empty()) return leaf_get_path(b, rec, first, second);
    if (rec < 0 || rec >= b->n_rec) FAIL(b->ctx, VBX_ERR_INVALID, "recording index %d out of range", rec);
    const int k = b->kid_of[rec];
    return kid_fail(b, k, leaf_get_path(b->kids[k], b->local_of[rec], first, second));
}

}  // extern "C"
