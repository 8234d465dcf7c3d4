// vbx_turn_init.hpp -- --init RTTM / RTTM+VB: the initial responsibilities of a recording from the speaker
// turns of a diarization that exists, resampled onto the x-vector windows on the device.
//
// All times are integer microseconds (the host parses; the device sees int64 only), so every overlap is exact and every tie a
// true tie.  Window i is [a_i, b_i), turn j is [u_j, v_j) of speaker spk_j; the turns arrive sorted by (speaker, start).
//   d[i][s] = sum over the turns j of s of max(0, min(b_i, v_j) - max(a_i, u_j)),   D_i = sum_s d[i][s]
//   D_i > 0:   w[i][s] = d[i][s] / D_i, label[i] = argmax_s d[i][s] (lowest among equals)
//   D_i == 0:  the turn with the smallest gap max(u_j - b_i, a_i - v_j) names the speaker (lowest among equal gaps): w[i] is its
//              one-hot row, label[i] that speaker
//   q[i][s] = exp(x_s - max x) / sum exp(x - max x), x = smoothing * w[i]: vbhmm.py:150-152 where a window lies in one turn
//
// turn_init_kernel: one thread per window, one launch per recording.  The turns are staged through LDS kTurnTile at a time and
// every thread walks the tile (all lanes read one address: a broadcast).  Because the turns are grouped by speaker a thread
// carries ONE running d; when the speaker changes (the same moment in every thread) it flushes d to row i of the [T][Sp]
// scratch, with zeros for the speakers without a turn in between: every (i, s) is written once, by one thread, in a fixed
// order -- no atomics.  Alongside it keeps D_i, the best (d, s) and the nearest (gap, s).  After the walk the same thread reads
// its row back twice: the sum of the exponentials in speaker order, then the quotients, written where the batch keeps its
// responsibilities (leading dimension ldq, zeros from S on).  T x N compares and 2 T S exponentials: nowhere near any roofline;
// the point is that nothing but ticks and turns goes up and that the result has the same bits on every run.
#pragma once
#include "vbx_device.hpp"

namespace vbx {

constexpr int kTurnBlock = 256;            // windows per workgroup: one per thread
constexpr int kTurnTile = 256;             // turns per LDS tile (5 KB): one load per thread

template <typename R>
__global__ __launch_bounds__(kTurnBlock) void turn_init_kernel(
    const long long* __restrict__ seg_a, const long long* __restrict__ seg_b, long long T, const long long* __restrict__ turn_u,
    const long long* __restrict__ turn_v, const int* __restrict__ turn_spk, long long N, int S, int Sp, double smoothing,
    long long* __restrict__ dscr, int* __restrict__ labels, double* __restrict__ w, R* __restrict__ q, int ldq) {
    __shared__ long long su[kTurnTile], sv[kTurnTile];
    __shared__ int ss[kTurnTile];
    const long long i = (long long)blockIdx.x * kTurnBlock + threadIdx.x;
    const bool live = i < T;                                   // (a thread past T still loads its share of every tile)
    const long long a = live ? seg_a[i] : 0, b = live ? seg_b[i] : 0;
    long long* const row = dscr + (live ? i : 0) * Sp;
    int cur = -1, best_s = 0, near_s = 0;
    long long d = 0, D = 0, best_d = 0, near_g = 0x7fffffffffffffffll;
    // speaker `cur` is complete: its d to the row, zeros for the speakers up to `next` that have no turn at all
    auto flush = [&](int next) {
        if (cur >= 0) {
            row[cur] = d;
            D += d;
            if (d > best_d) {
                best_d = d;
                best_s = cur;
            }
        }
        for (int z = cur + 1; z < next; ++z) row[z] = 0;
    };
    for (long long j0 = 0; j0 < N; j0 += kTurnTile) {
        const int n = (int)(N - j0 < kTurnTile ? N - j0 : kTurnTile);
        __syncthreads();                                       // (the tile before has been walked by everyone)
        if ((int)threadIdx.x < n) {
            su[threadIdx.x] = turn_u[j0 + threadIdx.x];
            sv[threadIdx.x] = turn_v[j0 + threadIdx.x];
            ss[threadIdx.x] = turn_spk[j0 + threadIdx.x];
        }
        __syncthreads();
        if (live)
            for (int j = 0; j < n; ++j) {
                const int s = ss[j];
                if (s != cur) {
                    flush(s);
                    cur = s;
                    d = 0;
                }
                const long long u = su[j], v = sv[j];
                const long long over = (b < v ? b : v) - (a > u ? a : u);
                if (over > 0) d += over;
                const long long g = u - b > a - v ? u - b : a - v;
                if (g < near_g) {                              // (speakers ascend: a strict test keeps the lowest among equals)
                    near_g = g;
                    near_s = s;
                }
            }
    }
    if (!live) return;
    flush(S);
    const int label = D > 0 ? best_s : near_s;
    if (labels) labels[i] = label;
    const double Dd = (double)D;
    const double wmax = D > 0 ? (double)best_d / Dd : 1.0;
    double den = 0.0;
    for (int s = 0; s < S; ++s) {
        const double ws = D > 0 ? (double)row[s] / Dd : (s == near_s ? 1.0 : 0.0);
        if (w) w[i * S + s] = ws;
        den += exp(smoothing * (ws - wmax));
    }
    if (!q) return;
    for (int s = 0; s < S; ++s) {
        const double ws = D > 0 ? (double)row[s] / Dd : (s == near_s ? 1.0 : 0.0);
        q[i * ldq + s] = (R)(exp(smoothing * (ws - wmax)) / den);
    }
    for (int s = S; s < ldq; ++s) q[i * ldq + s] = (R)0;
}

}  // namespace vbx

extern "C++" {
namespace {

// What the kernel relies on, checked on the host before anything is launched: it indexes row i of the scratch by the turns'
// speakers and assumes them grouped.  The first fault is described in `msg`.
bool turn_input_ok(std::string& msg, const char* fn, int64_t T, const int64_t* seg_a, const int64_t* seg_b, int64_t N,
                   const int64_t* turn_u, const int64_t* turn_v, const int32_t* turn_spk, int32_t S) {
    char buf[256];
    buf[0] = 0;
    if (T < 1 || N < 1) snprintf(buf, sizeof buf, "%s: T=%lld windows and N=%lld turns: both must be >= 1", fn, (long long)T, (long long)N);
    else if (S < 1 || S > VBX_MAX_SPEAKERS) snprintf(buf, sizeof buf, "%s: S=%d outside [1, %d]", fn, S, VBX_MAX_SPEAKERS);
    else if (!seg_a || !seg_b || !turn_u || !turn_v || !turn_spk) snprintf(buf, sizeof buf, "%s: NULL input", fn);
    for (int64_t i = 0; !buf[0] && i < T; ++i)
        if (seg_a[i] >= seg_b[i])
            snprintf(buf, sizeof buf, "%s: window %lld is empty: [%lld, %lld)", fn, (long long)i, (long long)seg_a[i], (long long)seg_b[i]);
    for (int64_t j = 0; !buf[0] && j < N; ++j) {
        if (turn_spk[j] < 0 || turn_spk[j] >= S)
            snprintf(buf, sizeof buf, "%s: speaker %d of turn %lld outside [0, %d)", fn, turn_spk[j], (long long)j, S);
        else if (turn_u[j] >= turn_v[j])
            snprintf(buf, sizeof buf, "%s: turn %lld is empty: [%lld, %lld)", fn, (long long)j, (long long)turn_u[j], (long long)turn_v[j]);
        else if (j > 0 && (turn_spk[j] < turn_spk[j - 1] || (turn_spk[j] == turn_spk[j - 1] && turn_u[j] < turn_u[j - 1])))
            snprintf(buf, sizeof buf, "%s: turn %lld is out of order: the turns must be sorted by (speaker, start)", fn, (long long)j);
    }
    msg = buf;
    return !buf[0];
}

// The ticks and the turns go up into blocks of `call`, the kernel runs on its stream: labels / w (either may be nullptr) and q
// (leading dimension ldq >= S, zeros from S on) are device addresses.
template <typename R>
void launch_turn_init(DeviceCall& call, int64_t T, const int64_t* seg_a, const int64_t* seg_b, int64_t N, const int64_t* turn_u,
                      const int64_t* turn_v, const int32_t* turn_spk, int S, int Sp, double init_smoothing, int* d_labels,
                      double* d_w, R* d_q, int ldq) {
    static_assert(sizeof(long long) == sizeof(int64_t), "the kernel reads the ticks as long long");
    const long long* d_a = (const long long*)call.upload(seg_a, (size_t)T);
    const long long* d_b = (const long long*)call.upload(seg_b, (size_t)T);
    const long long* d_u = (const long long*)call.upload(turn_u, (size_t)N);
    const long long* d_v = (const long long*)call.upload(turn_v, (size_t)N);
    const int* d_s = call.upload(turn_spk, (size_t)N);
    long long* d_scr = call.alloc<long long>((size_t)T * Sp);
    if (call.ok()) {
        hipLaunchKernelGGL((vbx::turn_init_kernel<R>), dim3((unsigned)((T + vbx::kTurnBlock - 1) / vbx::kTurnBlock)),
                           dim3(vbx::kTurnBlock), 0, call.st, d_a, d_b, (long long)T, d_u, d_v, d_s, (long long)N, S, Sp,
                           init_smoothing, d_scr, d_labels, d_w, d_q, ldq);
        call.launched();
    }
}

int padded_states(int S) {                                     // (leaf_create: powers of two from 16)
    int sp = 16;
    while (sp < S) sp *= 2;
    return sp;
}

}  // namespace
}  // extern "C++"

extern "C" {

int vbx_turn_weights(vbx_ctx* ctx, int64_t T, const int64_t* seg_a, const int64_t* seg_b, int64_t N, const int64_t* turn_u,
                     const int64_t* turn_v, const int32_t* turn_spk, int32_t S, double init_smoothing, int32_t* labels_host,
                     double* w_host, double* q_host) {
    std::string& err = ctx ? ctx->err : g_create_error;
    if (!turn_input_ok(err, "vbx_turn_weights", T, seg_a, seg_b, N, turn_u, turn_v, turn_spk, S)) return VBX_ERR_INVALID;
    if (!ctx) {
        err = "vbx_turn_weights: NULL context";
        return VBX_ERR_INVALID;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DeviceCall call(ctx);
    int* d_labels = labels_host ? call.alloc<int>((size_t)T) : nullptr;
    double* d_w = w_host ? call.alloc<double>((size_t)T * S) : nullptr;
    double* d_q = q_host ? call.alloc<double>((size_t)T * S) : nullptr;
    launch_turn_init<double>(call, T, seg_a, seg_b, N, turn_u, turn_v, turn_spk, S, padded_states(S), init_smoothing, d_labels, d_w,
                             d_q, S);
    if (labels_host) call.download(labels_host, (const int32_t*)d_labels, (size_t)T);
    if (w_host) call.download(w_host, (const double*)d_w, (size_t)T * S);
    if (q_host) call.download(q_host, (const double*)d_q, (size_t)T * S);
    call.sync();
    return call.finish("vbx_turn_weights failed");
}

}  // extern "C"
