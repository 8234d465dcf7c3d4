// vbx_frame_score.hpp -- the integer frame counts behind dscore's JER, B-cubed and information-theoretic columns, for a batch
// of (reference, system) pairs.
//
// dscore scores those columns on frames of `step` seconds (0.010).  Frame i exists for 0 <= i < n = int(hi / step), its time
// is the f64 product step * i, a turn [b, e) holds the frames with b <= step * i < e, and the frames with lo <= step * i < hi
// are counted (lo, hi: first turn start and last turn end of the pair).  With
//   F(x) = min(n, the first i >= 0 with step * i >= x)
// a turn holds the frames [F(b), F(e)) and the counted frames are [F(lo), F(hi)): nothing per frame is ever stored.
//
// frame_bounds: one thread per boundary (turn begins, turn ends, lo, hi).  F(x) starts from floor(x / step) and is corrected
// by comparing the rounded product step * i with x, up and down, until both neighbours agree: the candidate may be off by one
// where the quotient rounds across an integer (0.07 / 0.01 against 0.01 * 7).  __dmul_rn keeps the product a product.
// frame_sort: one thread per boundary counts the boundaries of its pair that sort before its own (smaller, or equal and
// earlier in the list), the others coming through LDS kFrmBlock at a time, and writes its value to that place.
// frame_cells: one workgroup per pair keeps the first of every run of equal values (lab_block_scan of vbx_labels_score.hpp):
// u[0] < u[1] < ... < u[nu - 1]; cell c is the frames [u[c], u[c + 1]).  Inside a cell nothing starts or ends.
// frame_masks: one thread per cell ORs the 64-bit masks of the reference and of the system speakers whose turns hold frame
// u[c], the turns coming through LDS kFrmBlock at a time.
// frame_firsts: one thread per cell finds, per side, the first cell of its pair with the same mask (a class is a set of
// speakers; the empty set is one).  frame_classes: one workgroup per pair numbers the cells that are their own first, in cell
// order: the classes in order of first appearance, with their masks.
// One small download (cells and classes per pair) sizes the result; then
// frame_acc: one thread per entry of a pair's result walks the pair's cells, which come through LDS kFrmBlock at a time, and
// adds the cell's frame count where the entry's condition holds: ref_durs[r], sys_durs[s], inter[r][s], cm[a][b], int64.
//
// No atomics and nothing that depends on the grid: every entry is one thread's sum in cell order, of integers.  A pair gives
// the same bytes alone, in any batch and at any place in it.
#pragma once
#include "vbx_device.hpp"
#include "vbx_labels_score.hpp"   // lab_block_scan

namespace vbx {

constexpr int kFrmBlock = 256;             // boundaries, cells or result entries per workgroup; turns or cells per LDS chunk
constexpr int kFrmMaxSpk = 64;             // speakers per side (the masks are 64 bits)
constexpr int kFrmMaxCls = 256;            // classes per side the device returns; a pair with more is reported, not scored
constexpr int kFrmInfo = 4;                // int32 per pair that come back: cells, reference classes, system classes, 0
static_assert(kFrmBlock == 256 && kLabBlock == kFrmBlock, "one thread stages one entry; one scan entry per thread");

struct FrmPair {
    long long turn_off;   // first of its turns: n_ref_turns reference turns, then n_sys_turns system turns
    long long bnd_off;    // first of its nb = 2 (turns) + 2 boundary slots: begins, ends, lo, hi; its cells use the same room
    long long out_off;    // first int64 of its result (phase 2)
    long long n_frames;   // int(hi / step)
    double lo, hi;
    int n_ref_turns, n_sys_turns, n_ref, n_sys;
    int n_cells, n_rcls, n_scls, pad;      // phase 2: what came back
};

__device__ __forceinline__ int frm_nb(const FrmPair& pr) { return 2 * (pr.n_ref_turns + pr.n_sys_turns) + 2; }

// F(x) = min(n, first i >= 0 with step * i >= x); step * i never decreases with i, so one boundary separates the two answers
__device__ __forceinline__ long long frm_index(double x, double step, long long n) {
    if (!(x > 0.0)) return 0;
    const double q = floor(x / step);
    long long c = q >= (double)n ? n : (long long)q;
    while (c > 0 && __dmul_rn(step, (double)(c - 1)) >= x) --c;
    while (c < n && __dmul_rn(step, (double)c) < x) ++c;
    return c;
}

// grid = items, items[i] = {pair, block of kFrmBlock boundaries}
__global__ __launch_bounds__(256) void frame_bounds_kernel(const FrmPair* __restrict__ pairs, const int2* __restrict__ items,
                                                           const double* __restrict__ tbeg, const double* __restrict__ tend,
                                                           double step, long long* __restrict__ idx) {
    const int2 item = items[blockIdx.x];
    const FrmPair pr = pairs[item.x];
    const int nt = pr.n_ref_turns + pr.n_sys_turns, nb = 2 * nt + 2;
    const int j = item.y * kFrmBlock + threadIdx.x;
    if (j >= nb) return;
    const double x = j < nt ? tbeg[pr.turn_off + j] : j < 2 * nt ? tend[pr.turn_off + j - nt] : j == 2 * nt ? pr.lo : pr.hi;
    idx[pr.bnd_off + j] = frm_index(x, step, pr.n_frames);
}

// grid = items, items[i] = {pair, block of kFrmBlock boundaries}
__global__ __launch_bounds__(256) void frame_sort_kernel(const FrmPair* __restrict__ pairs, const int2* __restrict__ items,
                                                         const long long* __restrict__ idx, long long* __restrict__ sorted) {
    __shared__ long long v_sh[kFrmBlock];
    const int2 item = items[blockIdx.x];
    const FrmPair pr = pairs[item.x];
    const int nb = frm_nb(pr), tid = threadIdx.x;
    const int j = item.y * kFrmBlock + tid;
    const bool live = j < nb;
    const long long v = live ? idx[pr.bnd_off + j] : 0;
    int pos = 0;
    for (int k0 = 0; k0 < nb; k0 += kFrmBlock) {
        const int nk = min(kFrmBlock, nb - k0);
        __syncthreads();                                              // (the previous chunk has been read)
        if (tid < nk) v_sh[tid] = idx[pr.bnd_off + k0 + tid];
        __syncthreads();
        for (int k = 0; k < nk; ++k) {
            const long long o = v_sh[k];
            pos += (o < v || (o == v && k0 + k < j)) ? 1 : 0;
        }
    }
    if (live) sorted[pr.bnd_off + pos] = v;                           // (pos < nb: a place in a total order of nb entries)
}

// grid = pairs
__global__ __launch_bounds__(256) void frame_cells_kernel(const FrmPair* __restrict__ pairs, const long long* __restrict__ sorted,
                                                          long long* __restrict__ uniq, int* __restrict__ info) {
    __shared__ int scan_sh[kLabBlock];
    const FrmPair pr = pairs[blockIdx.x];
    const int nb = frm_nb(pr), tid = threadIdx.x;
    const long long* a = sorted + pr.bnd_off;
    int base = 0;                                                     // values kept in the earlier passes
    for (int i0 = 0; i0 < nb; i0 += kLabBlock) {
        const int i = i0 + tid;
        const bool keep = i < nb && (i == 0 || a[i - 1] != a[i]);
        const int incl = base + lab_block_scan(keep ? 1 : 0, scan_sh, tid);
        if (keep) uniq[pr.bnd_off + incl - 1] = a[i];
        base += scan_sh[kLabBlock - 1];
    }
    if (tid == 0) info[(long long)blockIdx.x * kFrmInfo] = base - 1;   // cells (nb >= 2: at least one value)
}

// grid = items, items[i] = {pair, block of kFrmBlock cells} over the nb - 1 cells a pair can have
__global__ __launch_bounds__(256) void frame_masks_kernel(const FrmPair* __restrict__ pairs, const int2* __restrict__ items,
                                                          const long long* __restrict__ idx, const int* __restrict__ tspk,
                                                          const long long* __restrict__ uniq, const int* __restrict__ info,
                                                          unsigned long long* __restrict__ rmask,
                                                          unsigned long long* __restrict__ smask, long long* __restrict__ cnt) {
    __shared__ long long fb_sh[kFrmBlock];
    __shared__ long long fe_sh[kFrmBlock];
    __shared__ int spk_sh[kFrmBlock];
    const int2 item = items[blockIdx.x];
    const FrmPair pr = pairs[item.x];
    const int n_cells = info[(long long)item.x * kFrmInfo];
    if (item.y * kFrmBlock >= n_cells) return;                        // (the whole workgroup)
    const int tid = threadIdx.x, c = item.y * kFrmBlock + tid;
    const bool live = c < n_cells;
    const long long k = live ? uniq[pr.bnd_off + c] : 0;
    const int nt = pr.n_ref_turns + pr.n_sys_turns;
    unsigned long long R = 0, S = 0;
    for (int t0 = 0; t0 < nt; t0 += kFrmBlock) {
        const int n = min(kFrmBlock, nt - t0);
        __syncthreads();                                              // (the previous chunk has been read)
        if (tid < n) {
            fb_sh[tid] = idx[pr.bnd_off + t0 + tid];
            fe_sh[tid] = idx[pr.bnd_off + nt + t0 + tid];
            spk_sh[tid] = tspk[pr.turn_off + t0 + tid];
        }
        __syncthreads();
        const int nref = min(max(pr.n_ref_turns - t0, 0), n);         // reference turns of this chunk come first
        for (int t = 0; t < n; ++t) {
            const unsigned long long bit = (fb_sh[t] <= k && k < fe_sh[t]) ? 1ull << (spk_sh[t] & 63) : 0ull;
            if (t < nref) R |= bit; else S |= bit;
        }
    }
    if (live) {
        rmask[pr.bnd_off + c] = R;
        smask[pr.bnd_off + c] = S;
        cnt[pr.bnd_off + c] = uniq[pr.bnd_off + c + 1] - k;
    }
}

// grid = items of frame_masks
__global__ __launch_bounds__(256) void frame_firsts_kernel(const FrmPair* __restrict__ pairs, const int2* __restrict__ items,
                                                           const int* __restrict__ info,
                                                           const unsigned long long* __restrict__ rmask,
                                                           const unsigned long long* __restrict__ smask, int* __restrict__ rfirst,
                                                           int* __restrict__ sfirst) {
    __shared__ unsigned long long r_sh[kFrmBlock];
    __shared__ unsigned long long s_sh[kFrmBlock];
    const int2 item = items[blockIdx.x];
    const FrmPair pr = pairs[item.x];
    const int n_cells = info[(long long)item.x * kFrmInfo];
    if (item.y * kFrmBlock >= n_cells) return;
    const int tid = threadIdx.x, c = item.y * kFrmBlock + tid;
    const bool live = c < n_cells;
    const unsigned long long R = live ? rmask[pr.bnd_off + c] : 0, S = live ? smask[pr.bnd_off + c] : 0;
    int fr = c, fs = c;
    for (int k0 = 0; k0 <= item.y * kFrmBlock; k0 += kFrmBlock) {     // the cells up to and including this block
        const int nk = min(kFrmBlock, n_cells - k0);
        __syncthreads();                                              // (the previous chunk has been read)
        if (tid < nk) {
            r_sh[tid] = rmask[pr.bnd_off + k0 + tid];
            s_sh[tid] = smask[pr.bnd_off + k0 + tid];
        }
        __syncthreads();
        for (int k = 0; k < nk; ++k) {
            fr = min(fr, r_sh[k] == R ? k0 + k : fr);
            fs = min(fs, s_sh[k] == S ? k0 + k : fs);
        }
    }
    if (live) {
        rfirst[pr.bnd_off + c] = fr;
        sfirst[pr.bnd_off + c] = fs;
    }
}

// grid = pairs.  cls[c] is written for the cells that are their own first: the class their mask opens; classes [pair][2][kFrmMaxCls]
__global__ __launch_bounds__(256) void frame_classes_kernel(const FrmPair* __restrict__ pairs,
                                                            const unsigned long long* __restrict__ rmask,
                                                            const unsigned long long* __restrict__ smask,
                                                            const int* __restrict__ rfirst, const int* __restrict__ sfirst,
                                                            int* __restrict__ rcls, int* __restrict__ scls,
                                                            unsigned long long* __restrict__ classes, int* __restrict__ info) {
    __shared__ int scan_sh[kLabBlock];
    const FrmPair pr = pairs[blockIdx.x];
    const int tid = threadIdx.x;
    const int n_cells = info[(long long)blockIdx.x * kFrmInfo];
    for (int side = 0; side < 2; ++side) {
        const unsigned long long* mask = (side ? smask : rmask) + pr.bnd_off;
        const int* first = (side ? sfirst : rfirst) + pr.bnd_off;
        int* cls = (side ? scls : rcls) + pr.bnd_off;
        unsigned long long* out = classes + ((long long)blockIdx.x * 2 + side) * kFrmMaxCls;
        int base = 0;                                                 // classes opened in the earlier passes
        for (int c0 = 0; c0 < n_cells; c0 += kLabBlock) {
            const int c = c0 + tid;
            const bool opens = c < n_cells && first[c] == c;
            const int k = base + lab_block_scan(opens ? 1 : 0, scan_sh, tid) - 1;
            if (opens) {
                cls[c] = k;
                if (k < kFrmMaxCls) out[k] = mask[c];
            }
            base += scan_sh[kLabBlock - 1];
        }
        if (tid == 0) info[(long long)blockIdx.x * kFrmInfo + 1 + side] = base;
    }
}

// grid = items, items[i] = {pair, block of kFrmBlock entries of its result}: ref_durs[n_ref], sys_durs[n_sys],
// inter[n_ref][n_sys], cm[n_rcls][n_scls]
__global__ __launch_bounds__(256) void frame_acc_kernel(const FrmPair* __restrict__ pairs, const int2* __restrict__ items,
                                                        const unsigned long long* __restrict__ rmask,
                                                        const unsigned long long* __restrict__ smask,
                                                        const long long* __restrict__ cnt, const int* __restrict__ rfirst,
                                                        const int* __restrict__ sfirst, const int* __restrict__ rcls,
                                                        const int* __restrict__ scls, long long* __restrict__ out) {
    __shared__ unsigned long long r_sh[kFrmBlock];
    __shared__ unsigned long long s_sh[kFrmBlock];
    __shared__ long long n_sh[kFrmBlock];
    __shared__ int a_sh[kFrmBlock];
    __shared__ int b_sh[kFrmBlock];
    const int2 item = items[blockIdx.x];
    const FrmPair pr = pairs[item.x];
    const int tid = threadIdx.x;
    const long long n_spk = (long long)pr.n_ref + pr.n_sys, n_int = (long long)pr.n_ref * pr.n_sys;
    const long long block = n_spk + n_int + (long long)pr.n_rcls * pr.n_scls;
    const long long e = (long long)item.y * kFrmBlock + tid;
    // what the entry counts: bits of R and of S that must be set (a mask of 0 asks nothing), or a pair of classes
    unsigned long long need_r = 0, need_s = 0;
    int ca = -1, cb = -1;
    if (e < pr.n_ref) need_r = 1ull << e;
    else if (e < n_spk) need_s = 1ull << (e - pr.n_ref);
    else if (e < n_spk + n_int) {
        need_r = 1ull << ((e - n_spk) / pr.n_sys);
        need_s = 1ull << ((e - n_spk) % pr.n_sys);
    } else if (e < block) {
        ca = (int)((e - n_spk - n_int) / pr.n_scls);
        cb = (int)((e - n_spk - n_int) % pr.n_scls);
    }
    long long acc = 0;
    for (int c0 = 0; c0 < pr.n_cells; c0 += kFrmBlock) {
        const int nc = min(kFrmBlock, pr.n_cells - c0);
        __syncthreads();                                              // (the previous chunk has been read)
        if (tid < nc) {
            const long long c = pr.bnd_off + c0 + tid;
            r_sh[tid] = rmask[c];
            s_sh[tid] = smask[c];
            n_sh[tid] = cnt[c];
            a_sh[tid] = rcls[pr.bnd_off + rfirst[c]];                 // (the class of the first cell with this mask)
            b_sh[tid] = scls[pr.bnd_off + sfirst[c]];
        }
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
            const bool hit = ca >= 0 ? (a_sh[c] == ca && b_sh[c] == cb)
                                     : ((r_sh[c] & need_r) == need_r && (s_sh[c] & need_s) == need_s);
            acc += hit ? n_sh[c] : 0;
        }
    }
    if (e < block) out[pr.out_off + e] = acc;
}

}  // namespace vbx

// ---- host glue (included by vbx_capi.hip after vbx_host_call.hpp and vbx_labels_score.hpp) -----------------------------------
namespace {

// What the frame kernels run on: the pairs, the work items of the kernels that tile a pair's boundaries, cells and result
// entries, and the room they need.  vbx_frame_counts plans on turns of the host, vbx_labels_frame_counts (vbx_labels_frame.hpp)
// on those labels_turns_kernel left on the device: one plan, so a pair is cut and summed the same way whichever way it came.
struct FrmPlan {
    std::vector<vbx::FrmPair> pairs;
    std::vector<int2> bnd_items, cell_items, acc_items;
    long long n_bnd = 0, n_out = 0;
};

// what a plan's kernels read and write in HBM
struct FrmDev {
    vbx::FrmPair* pairs = nullptr;
    const int2* bitems = nullptr;
    const int2* citems = nullptr;
    long long *idx = nullptr, *sorted = nullptr, *uniq = nullptr, *cnt = nullptr;
    unsigned long long *r = nullptr, *s = nullptr, *classes = nullptr;
    int *rfirst = nullptr, *sfirst = nullptr, *rcls = nullptr, *scls = nullptr, *info = nullptr;
};

// the next pair: n_ref_turns, then n_sys_turns turns from turn_off (n_sys_turns may be an upper bound that the device
// replaces before frame_masks runs); room for its 2 (turns) + 2 boundaries and as many cells
void frm_plan_add(FrmPlan& pl, int n_ref_turns, int n_sys_turns, int n_ref, int n_sys, double lo, double hi, double step,
                  long long turn_off) {
    const int p = (int)pl.pairs.size();
    vbx::FrmPair pr = vbx::FrmPair{};
    pr.turn_off = turn_off;
    pr.bnd_off = pl.n_bnd;
    pr.n_frames = hi > 0.0 ? (long long)(hi / step) : 0;
    pr.lo = lo;
    pr.hi = hi;
    pr.n_ref_turns = n_ref_turns;
    pr.n_sys_turns = n_sys_turns;
    pr.n_ref = n_ref;
    pr.n_sys = n_sys;
    const int nb = 2 * (n_ref_turns + n_sys_turns) + 2;
    for (int b = 0; b * vbx::kFrmBlock < nb; ++b) pl.bnd_items.push_back(make_int2(p, b));
    for (int b = 0; b * vbx::kFrmBlock < nb - 1; ++b) pl.cell_items.push_back(make_int2(p, b));
    pl.pairs.push_back(pr);
    pl.n_bnd += nb;
}

bool frm_plan_fits(const FrmPlan& pl) { return pl.n_bnd <= 0x7fffffffLL && pl.bnd_items.size() <= 0x7fffffffULL; }

// the plan goes up and gets its room; cut_only: the room of frame_bounds, frame_sort and frame_cells alone
FrmDev frm_plan_upload(DeviceCall& call, const FrmPlan& pl, bool cut_only) {
    FrmDev d;
    const size_t n_bnd = (size_t)pl.n_bnd, n_pairs = pl.pairs.size();
    d.pairs = call.upload(pl.pairs.data(), n_pairs);
    d.bitems = call.upload(pl.bnd_items.data(), pl.bnd_items.size());
    if (!cut_only) d.citems = call.upload(pl.cell_items.data(), pl.cell_items.size());
    d.idx = call.alloc<long long>(n_bnd);
    d.sorted = call.alloc<long long>(n_bnd);
    d.uniq = call.alloc<long long>(n_bnd);
    if (!cut_only) {
        d.cnt = call.alloc<long long>(n_bnd);
        d.r = call.alloc<unsigned long long>(n_bnd);
        d.s = call.alloc<unsigned long long>(n_bnd);
        d.rfirst = call.alloc<int>(n_bnd);
        d.sfirst = call.alloc<int>(n_bnd);
        d.rcls = call.alloc<int>(n_bnd);
        d.scls = call.alloc<int>(n_bnd);
        d.classes = call.alloc<unsigned long long>(n_pairs * 2 * vbx::kFrmMaxCls);
    }
    d.info = call.alloc<int>(n_pairs * vbx::kFrmInfo);
    if (!cut_only && call.ok())
        call.enqueued(hipMemsetAsync(d.classes, 0, sizeof(unsigned long long) * n_pairs * 2 * vbx::kFrmMaxCls, call.st));
    return d;
}

// the sorted distinct frame indices of every pair's boundaries, from the turns in HBM: uniq and info[.][0] (enqueued)
void frm_plan_cut(DeviceCall& call, const FrmPlan& pl, const FrmDev& d, const double* d_tb, const double* d_te, double step) {
    if (!call.ok()) return;
    const dim3 nbi((unsigned)pl.bnd_items.size()), np((unsigned)pl.pairs.size()), th(256);
    hipLaunchKernelGGL(vbx::frame_bounds_kernel, nbi, th, 0, call.st, d.pairs, d.bitems, d_tb, d_te, step, d.idx);
    hipLaunchKernelGGL(vbx::frame_sort_kernel, nbi, th, 0, call.st, d.pairs, d.bitems, d.idx, d.sorted);
    hipLaunchKernelGGL(vbx::frame_cells_kernel, np, th, 0, call.st, d.pairs, d.sorted, d.uniq, d.info);
    call.launched();
}

// masks and classes of every pair's cells; what sizes the result comes back into got and classes (enqueued, not waited for)
void frm_plan_classes(DeviceCall& call, const FrmPlan& pl, const FrmDev& d, const int* d_spk, int32_t* got, uint64_t* classes) {
    if (call.ok()) {
        const dim3 nci((unsigned)pl.cell_items.size()), np((unsigned)pl.pairs.size()), th(256);
        hipLaunchKernelGGL(vbx::frame_masks_kernel, nci, th, 0, call.st, d.pairs, d.citems, d.idx, d_spk, d.uniq, d.info, d.r, d.s, d.cnt);
        hipLaunchKernelGGL(vbx::frame_firsts_kernel, nci, th, 0, call.st, d.pairs, d.citems, d.info, d.r, d.s, d.rfirst, d.sfirst);
        hipLaunchKernelGGL(vbx::frame_classes_kernel, np, th, 0, call.st, d.pairs, d.r, d.s, d.rfirst, d.sfirst, d.rcls, d.scls, d.classes,
                           d.info);
        call.launched();
    }
    call.download(got, d.info, pl.pairs.size() * vbx::kFrmInfo);
    call.download((unsigned long long*)classes, d.classes, pl.pairs.size() * 2 * vbx::kFrmMaxCls);
}

enum { kFrmSumsOk = 0, kFrmSumsInsane = 1, kFrmSumsNoRoom = 2 };

// the sums, sized by what came back in got (synchronised); a pair with more classes than kFrmMaxCls a side gets no cm.
// -> kFrmSumsInsane: what came back would index past its room; kFrmSumsNoRoom: the result has pl.n_out entries, more than
// out_cap; nothing is launched or written in either case
int frm_plan_sums(DeviceCall& call, FrmPlan& pl, const FrmDev& d, int32_t* got, int64_t* out, int64_t out_cap) {
    pl.n_out = 0;
    pl.acc_items.clear();
    if (!call.ok()) return kFrmSumsOk;
    for (size_t p = 0; p < pl.pairs.size(); ++p) {
        vbx::FrmPair& pr = pl.pairs[p];
        int32_t* g = got + p * vbx::kFrmInfo;
        const int nb = 2 * (pr.n_ref_turns + pr.n_sys_turns) + 2;
        g[3] = 0;
        if (g[0] < 0 || g[0] > nb - 1 || g[1] < 0 || g[1] > g[0] || g[2] < 0 || g[2] > g[0]) return kFrmSumsInsane;
        const bool fits = g[1] <= vbx::kFrmMaxCls && g[2] <= vbx::kFrmMaxCls;
        pr.n_cells = g[0];
        pr.n_rcls = fits ? g[1] : 0;
        pr.n_scls = fits ? g[2] : 0;
        pr.out_off = pl.n_out;
        const long long block = (long long)pr.n_ref + pr.n_sys + (long long)pr.n_ref * pr.n_sys + (long long)pr.n_rcls * pr.n_scls;
        for (long long b = 0; b * vbx::kFrmBlock < block; ++b) pl.acc_items.push_back(make_int2((int)p, (int)b));
        pl.n_out += block;
    }
    if (pl.n_out > out_cap) return kFrmSumsNoRoom;
    if (pl.n_out > 0) {
        call.copy_in(d.pairs, pl.pairs.data(), pl.pairs.size());        // (with what came back)
        const int2* d_aitems = call.upload(pl.acc_items.data(), pl.acc_items.size());
        long long* d_out = call.alloc<long long>((size_t)pl.n_out);
        if (call.ok()) {
            hipLaunchKernelGGL(vbx::frame_acc_kernel, dim3((unsigned)pl.acc_items.size()), dim3(256), 0, call.st, d.pairs, d_aitems, d.r, d.s,
                               d.cnt, d.rfirst, d.sfirst, d.rcls, d.scls, d_out);
            call.launched();
        }
        call.download((long long*)out, d_out, (size_t)pl.n_out);
        call.sync();
    }
    return kFrmSumsOk;
}

}  // namespace

extern "C" {

int vbx_frame_counts(vbx_ctx* ctx, int32_t n_pairs, const int32_t* counts, const double* extent, const double* turns,
                     const int32_t* spk, double step, int32_t* info, uint64_t* classes, int64_t* out, int64_t out_cap) {
    if (!ctx) return VBX_ERR_INVALID;
    if (n_pairs <= 0 || !counts || !extent || !info || !classes || !out || out_cap < 0)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_frame_counts: bad argument");
    if (!(step > 0.0) || !std::isfinite(step)) FAIL(ctx, VBX_ERR_INVALID, "vbx_frame_counts: step=%g is not a length", step);
    // ---- the pairs: everything the kernels index or shift with is checked here, before any launch ----
    FrmPlan pl;
    long long n_turns = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const int32_t* c = counts + 4 * (size_t)p;
        const int nrt = c[0], nst = c[1], nr = c[2], ns = c[3];
        if (nrt < 0 || nst < 0 || nr < 0 || ns < 0 || nrt > (1 << 24) || nst > (1 << 24))
            FAIL(ctx, VBX_ERR_INVALID, "vbx_frame_counts: pair %d: negative or oversized count", p);
        if (nr > vbx::kFrmMaxSpk || ns > vbx::kFrmMaxSpk)
            FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_frame_counts: pair %d has %d reference and %d system speakers, at most %d a side", p, nr, ns, vbx::kFrmMaxSpk);
        const double lo = extent[2 * (size_t)p], hi = extent[2 * (size_t)p + 1];
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo <= hi) || !(hi / step < 1099511627776.0))
            FAIL(ctx, VBX_ERR_INVALID, "vbx_frame_counts: pair %d: the extent [%g, %g] is not one of fewer than 2^40 frames", p, lo, hi);
        if (nrt + nst > 0 && (!turns || !spk)) FAIL(ctx, VBX_ERR_INVALID, "vbx_frame_counts: NULL argument");
        for (long long t = 0; t < (long long)nrt + nst; ++t) {
            const double b = turns[2 * (n_turns + t)], e = turns[2 * (n_turns + t) + 1];
            if (int rc = check_turn_speakers(ctx, "vbx_frame_counts", "pair", p, "turn", spk + n_turns + t, t, 1, t < nrt ? nr : ns)) return rc;
            if (!(lo <= b && b <= e && e <= hi)) FAIL(ctx, VBX_ERR_INVALID, "vbx_frame_counts: pair %d: turn %lld [%g, %g] outside the extent [%g, %g]", p, t, b, e, lo, hi);
        }
        frm_plan_add(pl, nrt, nst, nr, ns, lo, hi, step, n_turns);
        n_turns += (long long)nrt + nst;
    }
    if (!frm_plan_fits(pl)) FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_frame_counts: %lld turns in one call", n_turns);
    const TurnPlanes tp(turns, n_turns);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> got((size_t)n_pairs * vbx::kFrmInfo);
    DeviceCall call(ctx);                         // (after every host buffer its copies read or write)
    // ---- phase 1: cells, masks and classes of every pair ----
    const FrmDev d = frm_plan_upload(call, pl, false);
    const double* d_tb = call.upload(tp.beg.data(), (size_t)n_turns);
    const double* d_te = call.upload(tp.end.data(), (size_t)n_turns);
    const int* d_spk = call.upload(spk, (size_t)n_turns);
    frm_plan_cut(call, pl, d, d_tb, d_te, step);
    frm_plan_classes(call, pl, d, d_spk, got.data(), classes);
    call.sync();
    // ---- phase 2: the sums, sized by what came back ----
    const int sums = frm_plan_sums(call, pl, d, got.data(), out, out_cap);
    if (int rc = call.finish("frame count kernels failed")) return rc;
    if (sums == kFrmSumsInsane) FAIL(ctx, VBX_ERR_HIP, "vbx_frame_counts: the cell or class counts that came back do not fit their room");
    if (sums == kFrmSumsNoRoom) FAIL(ctx, VBX_ERR_INVALID, "vbx_frame_counts: the result has %lld entries, out has room for %lld", pl.n_out, (long long)out_cap);
    std::memcpy(info, got.data(), sizeof(int32_t) * got.size());
    return VBX_OK;
}

}  // extern "C"
