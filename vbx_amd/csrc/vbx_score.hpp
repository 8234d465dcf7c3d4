// vbx_score.hpp -- confusion blocks of the responsibilities against reference labels (reference: VBx/VBx.py:134-143, DER()).
//
// DER() needs err_mx = ref_mx^T (-q) and, for the cross-entropy, ref_mx^T (-log(q + nextafter(0, 1))): two n_ref x S matrices; the
// Hungarian assignment on them is tiny and stays on the host.  The device produces, per recording and iteration,
//   C[0][r][s] = sum_{t: ref_t = r} gamma[t][s]
//   C[1][r][s] = sum_{t: ref_t = r} -log(gamma[t][s] + 4.94e-324)
// in f64, from gamma as every path of the iteration leaves it ([rows][Sp], type R of the batch), widened before anything else.
//
// Decomposition (per RECORDING, never per launch, so that a recording gives the same bits alone, in any batch and on any
// number of streams): the frames of a recording are cut into groups of kScoreGroupTiles consecutive tiles.  score_acc: one
// workgroup per (group, block of kScoreCols state columns) walks the group's frames in order with its accumulators in
// registers and writes ONE partial block per group; score_fin adds a recording's partials in group order into the history
// slot of the iteration.  Every entry is therefore a sum in frame order inside a group and in group order across groups: no
// atomics, no order that depends on the grid.
//
// score_acc, 256 threads = 8 row groups x 32 columns.  Thread (rg, col) owns the labels rg, rg + 8, ... (at most 8 of them:
// n_ref <= kScoreMaxRef = 64) of column col: per frame it adds gamma or +0.0 to each of them -- branch-free, and adding +0.0
// leaves the bits of a sum alone.  The frames come through LDS in chunks of kScoreChunk: the widened gamma and its -log are
// computed once per (frame, column) by the whole workgroup ([32][32] f64 each, 16 KB), then read back by the eight row groups
// (one address per column for every row group of a wavefront: a broadcast, no bank conflict).  LDS does not grow with S.
// A label that occurs nowhere keeps its all-zero row; padded states (s >= S) and frames behind the end are never read.
#pragma once
#include "vbx_kernels.hpp"

namespace vbx {

constexpr int kScoreGroupTiles = 8;                                   // tiles per partial block
constexpr int kScoreGroupFrames = kScoreGroupTiles * kTileFrames;     // 1024 frames
constexpr int kScoreCols = 32;                                        // state columns per workgroup
constexpr int kScoreChunk = 32;                                       // frames staged in LDS at a time
constexpr int kScoreRowGroups = 8;
constexpr int kScoreMaxRef = 64;                                      // labels the device path takes
constexpr int kScoreOwn = kScoreMaxRef / kScoreRowGroups;             // labels per thread

struct ScoreRec {
    long long part_off;   // first double of the recording's partial blocks [ngroups][2][n_ref][Sp]
    long long hist_off;   // first double of its history [max_iters][2][n_ref][Sp]
    int n_ref;            // 0: the recording has no labels
    int ngroups;
};

// grid = (items, ceil(Sp / kScoreCols)); items[i] = {recording, group}
template <typename R>
__global__ __launch_bounds__(256) void score_acc_kernel(const R* __restrict__ gamma, int Sp, const RecDesc* __restrict__ recs,
                                                        const ScoreRec* __restrict__ srec, const int* __restrict__ lab,
                                                        const int2* __restrict__ items, double* __restrict__ part) {
    __shared__ double g_sh[kScoreChunk][kScoreCols];
    __shared__ double l_sh[kScoreChunk][kScoreCols];
    __shared__ int lab_sh[kScoreChunk];
    const int2 item = items[blockIdx.x];
    const RecDesc rd = recs[item.x];
    const ScoreRec sr = srec[item.x];
    const int tid = threadIdx.x, col = tid & (kScoreCols - 1), rg = tid / kScoreCols;
    const int c = blockIdx.y * kScoreCols + col;
    const bool live = c < rd.S;                                       // (S <= Sp)
    const int t_begin = item.y * kScoreGroupFrames;
    const int t_end = min(rd.T, t_begin + kScoreGroupFrames);
    const int nown = (sr.n_ref + kScoreRowGroups - 1) / kScoreRowGroups;
    double a0[kScoreOwn], a1[kScoreOwn];
#pragma unroll
    for (int i = 0; i < kScoreOwn; ++i) a0[i] = a1[i] = 0.0;
    for (int t0 = t_begin; t0 < t_end; t0 += kScoreChunk) {
        const int nf = min(kScoreChunk, t_end - t0);
        __syncthreads();                                              // (the previous chunk has been read)
#pragma unroll
        for (int u = 0; u < kScoreChunk / kScoreRowGroups; ++u) {
            const int f = rg + kScoreRowGroups * u;
            double g = 0.0, l = 0.0;
            if (f < nf && live) {
                g = (double)gamma[(rd.row0 + t0 + f) * Sp + c];
                l = -log(g + 4.9406564584124654e-324);                // np.nextafter(0, 1), VBx.py:139
            }
            g_sh[f][col] = g;
            l_sh[f][col] = l;
        }
        if (tid < nf) lab_sh[tid] = lab[rd.row0 + t0 + tid];
        __syncthreads();
        for (int f = 0; f < nf; ++f) {
            const int q = lab_sh[f] - rg;                             // the label is rg + 8 i  <=>  q == 8 i
            const double g = g_sh[f][col], l = l_sh[f][col];
#pragma unroll
            for (int i = 0; i < kScoreOwn; ++i) {
                if (i < nown) {
                    const bool hit = q == kScoreRowGroups * i;
                    a0[i] += hit ? g : 0.0;
                    a1[i] += hit ? l : 0.0;
                }
            }
        }
    }
    if (c >= Sp) return;
    const long long plane = (long long)sr.n_ref * Sp;
    double* out = part + sr.part_off + (long long)item.y * 2 * plane;
#pragma unroll
    for (int i = 0; i < kScoreOwn; ++i) {
        const int r = rg + kScoreRowGroups * i;
        if (r < sr.n_ref) {
            out[(long long)r * Sp + c] = a0[i];
            out[plane + (long long)r * Sp + c] = a1[i];
        }
    }
}

// grid = (n_rec, blocks of 256 entries of the widest block 2 n_ref Sp); the partials of a recording in group order -> slot
// n_iters - 1 of its history (state: the latest one, after the finishing role of the iteration has run) or `slot` itself when
// there is no state (the stand-alone step)
__global__ __launch_bounds__(256) void score_fin_kernel(int Sp, int max_iters, const ScoreRec* __restrict__ srec,
                                                        const RecState* __restrict__ state, int slot,
                                                        const double* __restrict__ part, double* __restrict__ hist) {
    const int rec = blockIdx.x;
    const ScoreRec sr = srec[rec];
    if (sr.n_ref == 0) return;
    if (state) slot = state[rec].n_iters - 1;
    if (slot < 0 || slot >= max_iters) return;
    const long long block = 2ll * sr.n_ref * Sp;
    const long long e = (long long)blockIdx.y * blockDim.x + threadIdx.x;
    if (e >= block) return;
    const double* p = part + sr.part_off + e;
    double sum = 0.0;
    for (int g = 0; g < sr.ngroups; ++g) sum += p[(long long)g * block];
    hist[sr.hist_off + (long long)slot * block + e] = sum;
}

}  // namespace vbx
