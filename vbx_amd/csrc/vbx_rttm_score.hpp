// vbx_rttm_score.hpp -- md-eval diarization error of RTTM turns, for a batch of (reference, system) pairs.
//
// The recipes of the reference end in `dscore/score.py -r ref.rttm -s sys.rttm --collar 0.25 [--ignore_overlaps]`
// (run_example.sh:40); dscore wraps md-eval.  A pair is the merged reference turns and the merged system turns of one
// recording plus its cell edges: the sorted distinct turn boundaries, collar zone ends and extent ends (vbx_amd/score.py
// builds them).  Inside a cell the set of active reference speakers R, of system speakers S and the no-score flag are constant.
// The device produces, per pair, in f64,
//   tot[0] = sum w |R|             (scored reference speaker time)
//   tot[1] = sum w max(|R| - |S|, 0)   (miss)
//   tot[2] = sum w max(|S| - |R|, 0)   (false alarm)
//   tot[3] = sum w min(|R|, |S|)       (time one of the mapped speakers may claim)
//   C[r][s] = sum w [r in R][s in S]
// with w the length of a cell, or 0 where it is not scored.  The one-to-one mapping on C is tiny and stays on the host.
//
// rttm_cells: one thread per cell.  The cell's midpoint is compared (strictly) with every turn of its pair; the turns come
// through LDS in chunks of kRttmTurnChunk, so LDS does not grow with the number of turns.  The no-score zones of the collar
// are derived here from the reference turns: b - collar and b + collar are single IEEE operations, the bits the host has
// in its edges.  Out: the two 64-bit speaker masks and w of every cell.
//
// rttm_acc / rttm_fin, the scheme of score_acc_kernel / score_fin_kernel (vbx_score.hpp).  Decomposition per PAIR, never per
// launch: the cells of a pair are cut into groups of kRttmGroupCells consecutive cells.  rttm_acc: one workgroup per (pair,
// group, block of kRttmCols system speakers) walks the group's cells in order with its accumulators in registers and writes
// ONE partial block per group; rttm_fin adds a pair's partials in group order.  Every entry is a sum in cell order inside
// a group and in group order across groups: no atomics, no order that depends on the grid, so a pair gives the same bits
// alone, in any batch and at any position in it.
//
// rttm_acc, 256 threads = 8 row groups x 32 columns.  Thread (rg, col) owns the reference speakers rg, rg + 8, ... (at most
// 8: n_ref <= kRttmMaxSpk = 64) of system speaker col: per cell it adds w or +0.0 to each of them, branch-free (adding +0.0
// leaves the bits of a sum alone).  The cells come through LDS in chunks of kRttmAccChunk (masks and w: 6 KB).  Threads 0-3
// of the first column block carry tot[0..3] through the same walk.
#pragma once
#include "vbx_device.hpp"

namespace vbx {

constexpr int kRttmClsBlock = 256;         // cells per classification workgroup (one per thread)
constexpr int kRttmTurnChunk = 256;        // turns staged in LDS at a time
constexpr int kRttmGroupCells = 1024;      // cells per partial block
constexpr int kRttmAccChunk = 256;         // cells staged in LDS at a time
constexpr int kRttmCols = 32;              // system speakers per workgroup
constexpr int kRttmRowGroups = 8;
constexpr int kRttmMaxSpk = 64;            // speakers per side the device path takes (the masks are 64 bits)
constexpr int kRttmOwn = kRttmMaxSpk / kRttmRowGroups;
constexpr int kRttmTotals = 4;
static_assert(kRttmClsBlock == 256 && kRttmTurnChunk <= 256 && kRttmAccChunk <= 256, "one thread stages one entry");

struct RttmPair {
    long long edge_off;   // first of its n_cells + 1 edges
    long long cell_off;   // first of its cells in the mask / weight arrays
    long long turn_off;   // first of its turns: n_ref_turns reference turns, then n_sys_turns system turns
    long long part_off;   // first double of its partial blocks [ngroups][kRttmTotals + n_ref n_sys]
    long long out_off;    // first double of its result kRttmTotals + n_ref n_sys
    int n_cells, n_ref_turns, n_sys_turns, n_ref, n_sys, ngroups;
};

// grid = items, items[i] = {pair, block of kRttmClsBlock cells}
__global__ __launch_bounds__(256) void rttm_cells_kernel(const RttmPair* __restrict__ pairs, const int2* __restrict__ items,
                                                         const double* __restrict__ edges, const double* __restrict__ tbeg,
                                                         const double* __restrict__ tend, const int* __restrict__ tspk,
                                                         double collar, int ignore_overlaps,
                                                         unsigned long long* __restrict__ rmask,
                                                         unsigned long long* __restrict__ smask, double* __restrict__ wout) {
    __shared__ double beg_sh[kRttmTurnChunk];
    __shared__ double end_sh[kRttmTurnChunk];
    __shared__ int spk_sh[kRttmTurnChunk];
    const int2 item = items[blockIdx.x];
    const RttmPair pr = pairs[item.x];
    const int tid = threadIdx.x;
    const int c = item.y * kRttmClsBlock + tid;
    const bool live = c < pr.n_cells;
    double a = 0.0, b = 0.0, mid = 0.0;
    if (live) {
        a = edges[pr.edge_off + c];
        b = edges[pr.edge_off + c + 1];
        mid = 0.5 * (a + b);
    }
    unsigned long long R = 0, S = 0;
    bool noscore = false;
    const int nturns = pr.n_ref_turns + pr.n_sys_turns;
    for (int t0 = 0; t0 < nturns; t0 += kRttmTurnChunk) {
        const int nt = min(kRttmTurnChunk, nturns - t0);
        __syncthreads();                                              // (the previous chunk has been read)
        if (tid < nt) {
            beg_sh[tid] = tbeg[pr.turn_off + t0 + tid];
            end_sh[tid] = tend[pr.turn_off + t0 + tid];
            spk_sh[tid] = tspk[pr.turn_off + t0 + tid];
        }
        __syncthreads();
        const int nref = min(max(pr.n_ref_turns - t0, 0), nt);        // reference turns of this chunk come first
        for (int t = 0; t < nt; ++t) {
            const double tb = beg_sh[t], te = end_sh[t];
            const unsigned long long bit = (tb < mid && mid < te) ? 1ull << spk_sh[t] : 0ull;
            if (t < nref) {
                R |= bit;
                if (collar > 0.0)
                    noscore = noscore || (tb - collar < mid && mid < tb + collar) || (te - collar < mid && mid < te + collar);
            } else {
                S |= bit;
            }
        }
    }
    if (ignore_overlaps && __popcll(R) >= 2) noscore = true;
    if (live) {
        rmask[pr.cell_off + c] = R;
        smask[pr.cell_off + c] = S;
        wout[pr.cell_off + c] = noscore ? 0.0 : b - a;
    }
}

// grid = (items, column blocks); items[i] = {pair, group}
__global__ __launch_bounds__(256) void rttm_acc_kernel(const RttmPair* __restrict__ pairs, const int2* __restrict__ items,
                                                       const unsigned long long* __restrict__ rmask,
                                                       const unsigned long long* __restrict__ smask,
                                                       const double* __restrict__ w, double* __restrict__ part) {
    __shared__ unsigned long long r_sh[kRttmAccChunk];
    __shared__ unsigned long long s_sh[kRttmAccChunk];
    __shared__ double w_sh[kRttmAccChunk];
    const int2 item = items[blockIdx.x];
    const RttmPair pr = pairs[item.x];
    // a column block past the pair's system speakers has nothing to do, except that the first one carries the totals
    if (blockIdx.y > 0 && (int)blockIdx.y * kRttmCols >= pr.n_sys) return;
    const int tid = threadIdx.x, col = tid & (kRttmCols - 1), rg = tid / kRttmCols;
    const int s = blockIdx.y * kRttmCols + col;
    const int c_begin = item.y * kRttmGroupCells;
    const int c_end = min(pr.n_cells, c_begin + kRttmGroupCells);
    const int nown = (pr.n_ref + kRttmRowGroups - 1) / kRttmRowGroups;
    const int which = tid & 3;                                        // the total this thread carries (kept by tid < 4)
    double acc[kRttmOwn], tot = 0.0;
#pragma unroll
    for (int i = 0; i < kRttmOwn; ++i) acc[i] = 0.0;
    for (int c0 = c_begin; c0 < c_end; c0 += kRttmAccChunk) {
        const int nc = min(kRttmAccChunk, c_end - c0);
        __syncthreads();                                              // (the previous chunk has been read)
        if (tid < nc) {
            r_sh[tid] = rmask[pr.cell_off + c0 + tid];
            s_sh[tid] = smask[pr.cell_off + c0 + tid];
            w_sh[tid] = w[pr.cell_off + c0 + tid];
        }
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
            const unsigned long long R = r_sh[c], S = s_sh[c];
            const double wc = w_sh[c];
            const double ws = ((S >> (s & 63)) & 1ull) ? wc : 0.0;
            const unsigned long long Rr = R >> rg;
#pragma unroll
            for (int i = 0; i < kRttmOwn; ++i)
                if (i < nown) acc[i] += ((Rr >> (kRttmRowGroups * i)) & 1ull) ? ws : 0.0;
            const int nr = __popcll(R), ns = __popcll(S);
            const int k = which == 0 ? nr : which == 1 ? max(nr - ns, 0) : which == 2 ? max(ns - nr, 0) : min(nr, ns);
            tot += __dmul_rn(wc, (double)k);                          // (a product and a sum: what the host path rounds)
        }
    }
    const long long block = kRttmTotals + (long long)pr.n_ref * pr.n_sys;
    double* out = part + pr.part_off + (long long)item.y * block;
    if (blockIdx.y == 0 && tid < kRttmTotals) out[tid] = tot;
    if (s >= pr.n_sys) return;
#pragma unroll
    for (int i = 0; i < kRttmOwn; ++i) {
        const int r = rg + kRttmRowGroups * i;
        if (r < pr.n_ref) out[kRttmTotals + (long long)r * pr.n_sys + s] = acc[i];
    }
}

// grid = (pairs, blocks of 256 entries of the widest result); the partials of a pair in group order -> its result
__global__ __launch_bounds__(256) void rttm_fin_kernel(const RttmPair* __restrict__ pairs, const double* __restrict__ part,
                                                       double* __restrict__ out) {
    const RttmPair pr = pairs[blockIdx.x];
    const long long block = kRttmTotals + (long long)pr.n_ref * pr.n_sys;
    const long long e = (long long)blockIdx.y * blockDim.x + threadIdx.x;
    if (e >= block) return;
    const double* p = part + pr.part_off + e;
    double sum = 0.0;
    for (int g = 0; g < pr.ngroups; ++g) sum += p[(long long)g * block];
    out[pr.out_off + e] = sum;
}

}  // namespace vbx

// ---- host glue (included by vbx_capi.hip after vbx_host_call.hpp) ------------------------------------------------------------
namespace {

// What the three kernels run on: the pairs, the work items of rttm_cells and rttm_acc, the sizes of what they write and the
// grids of rttm_acc (ycols) and rttm_fin (widest).  vbx_rttm_score plans on turns and edges of the host, vbx_labels_score on
// those its first phase left on the device: one plan, so a pair is cut the same way whichever way it came.
struct RttmPlan {
    std::vector<vbx::RttmPair> pairs;
    std::vector<int2> cls_items, acc_items;
    long long n_cells = 0, n_part = 0, n_out = 0, widest = 0;
    int ycols = 1;
};

// the next pair: n_cells cells on the n_cells + 1 edges from edge_off; n_ref_turns, then n_sys_turns turns from turn_off
void rttm_plan_add(RttmPlan& pl, int n_cells, int n_ref_turns, int n_sys_turns, int n_ref, int n_sys, long long edge_off,
                   long long turn_off) {
    const int p = (int)pl.pairs.size();
    vbx::RttmPair pr;
    pr.edge_off = edge_off;
    pr.cell_off = pl.n_cells;
    pr.turn_off = turn_off;
    pr.part_off = pl.n_part;
    pr.out_off = pl.n_out;
    pr.n_cells = n_cells;
    pr.n_ref_turns = n_ref_turns;
    pr.n_sys_turns = n_sys_turns;
    pr.n_ref = n_ref;
    pr.n_sys = n_sys;
    pr.ngroups = (n_cells + vbx::kRttmGroupCells - 1) / vbx::kRttmGroupCells;
    const long long block = vbx::kRttmTotals + (long long)n_ref * n_sys;
    for (int b = 0; b * vbx::kRttmClsBlock < n_cells; ++b) pl.cls_items.push_back(make_int2(p, b));
    for (int g = 0; g < pr.ngroups; ++g) pl.acc_items.push_back(make_int2(p, g));
    pl.pairs.push_back(pr);
    pl.n_cells += n_cells;
    pl.n_part += block * pr.ngroups;
    pl.n_out += block;
    pl.widest = std::max(pl.widest, block);
    pl.ycols = std::max(pl.ycols, (n_sys + vbx::kRttmCols - 1) / vbx::kRttmCols);
}

// the plan goes up, the three kernels run on the edges and turns in HBM, out [n_out] comes back (enqueued, not waited for)
void rttm_plan_run(DeviceCall& call, const RttmPlan& pl, const double* d_edges, const double* d_tb, const double* d_te,
                   const int* d_spk, double collar, int ignore_overlaps, double* out) {
    const vbx::RttmPair* d_pairs = call.upload(pl.pairs.data(), pl.pairs.size());
    const int2* d_cls = call.upload(pl.cls_items.data(), pl.cls_items.size());
    const int2* d_acc = call.upload(pl.acc_items.data(), pl.acc_items.size());
    auto* d_r = call.alloc<unsigned long long>((size_t)pl.n_cells);
    auto* d_s = call.alloc<unsigned long long>((size_t)pl.n_cells);
    double* d_w = call.alloc<double>((size_t)pl.n_cells);
    double* d_part = call.alloc<double>((size_t)pl.n_part);
    double* d_out = call.alloc<double>((size_t)pl.n_out);
    if (call.ok()) {
        if (!pl.cls_items.empty())
            hipLaunchKernelGGL(vbx::rttm_cells_kernel, dim3((unsigned)pl.cls_items.size()), dim3(256), 0, call.st, d_pairs, d_cls, d_edges,
                               d_tb, d_te, d_spk, collar, ignore_overlaps ? 1 : 0, d_r, d_s, d_w);
        if (!pl.acc_items.empty())
            hipLaunchKernelGGL(vbx::rttm_acc_kernel, dim3((unsigned)pl.acc_items.size(), (unsigned)pl.ycols), dim3(256), 0, call.st, d_pairs,
                               d_acc, d_r, d_s, d_w, d_part);
        hipLaunchKernelGGL(vbx::rttm_fin_kernel, dim3((unsigned)pl.pairs.size(), (unsigned)((pl.widest + 255) / 256)), dim3(256), 0, call.st,
                           d_pairs, d_part, d_out);
        call.launched();
    }
    call.download(out, d_out, (size_t)pl.n_out);
}

}  // namespace

extern "C" {

int vbx_rttm_score(vbx_ctx* ctx, int32_t n_pairs, const int32_t* counts, const double* edges, const double* turns,
                   const int32_t* spk, double collar, int ignore_overlaps, double* out) {
    if (!ctx) return VBX_ERR_INVALID;
    if (n_pairs <= 0 || !counts || !out) FAIL(ctx, VBX_ERR_INVALID, "vbx_rttm_score: bad argument");
    if (!(collar >= 0.0) || !std::isfinite(collar)) FAIL(ctx, VBX_ERR_INVALID, "vbx_rttm_score: collar=%g is not a length", collar);
    RttmPlan pl;
    long long n_edges = 0, n_turns = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const int32_t* c = counts + 5 * (size_t)p;
        const int ne = c[0], nrt = c[1], nst = c[2], nr = c[3], ns = c[4];
        if (ne < 0 || nrt < 0 || nst < 0 || nr < 0 || ns < 0 || ne > (1 << 28) || nrt > (1 << 28) || nst > (1 << 28))
            FAIL(ctx, VBX_ERR_INVALID, "vbx_rttm_score: pair %d: negative or oversized count", p);
        if (nr > vbx::kRttmMaxSpk || ns > vbx::kRttmMaxSpk)
            FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_rttm_score: pair %d has %d reference and %d system speakers, at most %d a side", p, nr, ns, vbx::kRttmMaxSpk);
        if (nrt + nst > 0 && (!turns || !spk)) FAIL(ctx, VBX_ERR_INVALID, "vbx_rttm_score: NULL argument");
        if (int rc = check_turn_speakers(ctx, "vbx_rttm_score", "pair", p, "turn", spk + n_turns, 0, nrt, nr)) return rc;
        if (int rc = check_turn_speakers(ctx, "vbx_rttm_score", "pair", p, "turn", spk + n_turns + nrt, nrt, nst, ns)) return rc;
        rttm_plan_add(pl, ne > 0 ? ne - 1 : 0, nrt, nst, nr, ns, n_edges, n_turns);
        n_edges += ne;
        n_turns += (long long)nrt + nst;
    }
    if (n_edges && !edges) FAIL(ctx, VBX_ERR_INVALID, "vbx_rttm_score: NULL argument");
    if (pl.n_cells > 0x7fffffffLL || n_turns > 0x7fffffffLL || pl.cls_items.size() > 0x7fffffffULL)
        FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_rttm_score: %lld cells, %lld turns in one call", pl.n_cells, n_turns);
    const TurnPlanes tp(turns, n_turns);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DeviceCall call(ctx);
    const double* d_edges = call.upload(edges, (size_t)n_edges);
    const double* d_tb = call.upload(tp.beg.data(), (size_t)n_turns);
    const double* d_te = call.upload(tp.end.data(), (size_t)n_turns);
    const int* d_spk = call.upload(spk, (size_t)n_turns);
    rttm_plan_run(call, pl, d_edges, d_tb, d_te, d_spk, collar, ignore_overlaps, out);
    call.sync();
    return call.finish("RTTM score kernels failed");
}

}  // extern "C"
