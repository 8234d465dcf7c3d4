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
extern "C" {

int vbx_frame_counts(vbx_ctx* ctx, int32_t n_pairs, const int32_t* counts, const double* extent, const double* turns,
                     const int32_t* spk, double step, int32_t* info, uint64_t* classes, int64_t* out, int64_t out_cap) {
    using vbx::FrmPair;
    if (!ctx) return VBX_ERR_INVALID;
    if (n_pairs <= 0 || !counts || !extent || !info || !classes || !out || out_cap < 0)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_frame_counts: bad argument");
    if (!(step > 0.0) || !std::isfinite(step)) FAIL(ctx, VBX_ERR_INVALID, "vbx_frame_counts: step=%g is not a length", step);
    // ---- the pairs: everything the kernels index or shift with is checked here, before any launch ----
    std::vector<FrmPair> pairs((size_t)n_pairs);
    std::vector<int2> bnd_items, cell_items;
    long long n_turns = 0, n_bnd = 0;
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
        FrmPair& pr = pairs[p];
        pr = FrmPair{};
        pr.turn_off = n_turns;
        pr.bnd_off = n_bnd;
        pr.n_frames = hi > 0.0 ? (long long)(hi / step) : 0;
        pr.lo = lo;
        pr.hi = hi;
        pr.n_ref_turns = nrt;
        pr.n_sys_turns = nst;
        pr.n_ref = nr;
        pr.n_sys = ns;
        const int nb = 2 * (nrt + nst) + 2;
        for (int b = 0; b * vbx::kFrmBlock < nb; ++b) bnd_items.push_back(make_int2(p, b));
        for (int b = 0; b * vbx::kFrmBlock < nb - 1; ++b) cell_items.push_back(make_int2(p, b));
        n_turns += (long long)nrt + nst;
        n_bnd += nb;
    }
    if (n_bnd > 0x7fffffffLL || bnd_items.size() > 0x7fffffffULL)
        FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_frame_counts: %lld turns in one call", n_turns);
    const TurnPlanes tp(turns, n_turns);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> got((size_t)n_pairs * vbx::kFrmInfo);
    std::vector<int2> acc_items;
    DeviceCall call(ctx);                         // (after every host buffer its copies read or write)
    hipStream_t st = call.st;
    const size_t n_classes = (size_t)n_pairs * 2 * vbx::kFrmMaxCls;
    // ---- phase 1: cells, masks and classes of every pair ----
    FrmPair* d_pairs = call.upload(pairs.data(), pairs.size());
    const int2* d_bitems = call.upload(bnd_items.data(), bnd_items.size());
    const int2* d_citems = call.upload(cell_items.data(), cell_items.size());
    const double* d_tb = call.upload(tp.beg.data(), (size_t)n_turns);
    const double* d_te = call.upload(tp.end.data(), (size_t)n_turns);
    const int* d_spk = call.upload(spk, (size_t)n_turns);
    long long* d_idx = call.alloc<long long>((size_t)n_bnd);
    long long* d_sorted = call.alloc<long long>((size_t)n_bnd);
    long long* d_uniq = call.alloc<long long>((size_t)n_bnd);
    long long* d_cnt = call.alloc<long long>((size_t)n_bnd);
    auto* d_r = call.alloc<unsigned long long>((size_t)n_bnd);
    auto* d_s = call.alloc<unsigned long long>((size_t)n_bnd);
    int* d_rfirst = call.alloc<int>((size_t)n_bnd);
    int* d_sfirst = call.alloc<int>((size_t)n_bnd);
    int* d_rcls = call.alloc<int>((size_t)n_bnd);
    int* d_scls = call.alloc<int>((size_t)n_bnd);
    auto* d_classes = call.alloc<unsigned long long>(n_classes);
    int* d_info = call.alloc<int>(got.size());
    if (call.ok()) call.enqueued(hipMemsetAsync(d_classes, 0, sizeof(unsigned long long) * n_classes, st));
    if (call.ok()) {
        const dim3 nbi((unsigned)bnd_items.size()), nci((unsigned)cell_items.size()), np((unsigned)n_pairs), th(256);
        hipLaunchKernelGGL(vbx::frame_bounds_kernel, nbi, th, 0, st, d_pairs, d_bitems, d_tb, d_te, step, d_idx);
        hipLaunchKernelGGL(vbx::frame_sort_kernel, nbi, th, 0, st, d_pairs, d_bitems, d_idx, d_sorted);
        hipLaunchKernelGGL(vbx::frame_cells_kernel, np, th, 0, st, d_pairs, d_sorted, d_uniq, d_info);
        hipLaunchKernelGGL(vbx::frame_masks_kernel, nci, th, 0, st, d_pairs, d_citems, d_idx, d_spk, d_uniq, d_info, d_r, d_s, d_cnt);
        hipLaunchKernelGGL(vbx::frame_firsts_kernel, nci, th, 0, st, d_pairs, d_citems, d_info, d_r, d_s, d_rfirst, d_sfirst);
        hipLaunchKernelGGL(vbx::frame_classes_kernel, np, th, 0, st, d_pairs, d_r, d_s, d_rfirst, d_sfirst, d_rcls, d_scls, d_classes,
                           d_info);
        call.launched();
    }
    call.download(got.data(), d_info, got.size());
    call.download((unsigned long long*)classes, d_classes, n_classes);
    call.sync();
    // ---- phase 2: the sums, sized by what came back; a pair with more classes than kFrmMaxCls a side gets no cm ----
    long long n_out = 0;
    bool sane = true;
    if (call.ok()) {
        for (int p = 0; p < n_pairs; ++p) {
            FrmPair& pr = pairs[p];
            int32_t* g = got.data() + (size_t)p * vbx::kFrmInfo;
            const int nb = 2 * (pr.n_ref_turns + pr.n_sys_turns) + 2;
            g[3] = 0;
            if (g[0] < 0 || g[0] > nb - 1 || g[1] < 0 || g[1] > g[0] || g[2] < 0 || g[2] > g[0]) {
                sane = false;                                         // (what came back would index past its room)
                break;
            }
            const bool fits = g[1] <= vbx::kFrmMaxCls && g[2] <= vbx::kFrmMaxCls;
            pr.n_cells = g[0];
            pr.n_rcls = fits ? g[1] : 0;
            pr.n_scls = fits ? g[2] : 0;
            pr.out_off = n_out;
            const long long block = (long long)pr.n_ref + pr.n_sys + (long long)pr.n_ref * pr.n_sys + (long long)pr.n_rcls * pr.n_scls;
            for (long long b = 0; b * vbx::kFrmBlock < block; ++b) acc_items.push_back(make_int2(p, (int)b));
            n_out += block;
        }
    }
    const bool room = n_out <= out_cap;
    if (sane && room && n_out > 0) {
        call.copy_in(d_pairs, pairs.data(), pairs.size());            // (with what came back)
        const int2* d_aitems = call.upload(acc_items.data(), acc_items.size());
        long long* d_out = call.alloc<long long>((size_t)n_out);
        if (call.ok()) {
            hipLaunchKernelGGL(vbx::frame_acc_kernel, dim3((unsigned)acc_items.size()), dim3(256), 0, st, d_pairs, d_aitems, d_r, d_s, d_cnt,
                               d_rfirst, d_sfirst, d_rcls, d_scls, d_out);
            call.launched();
        }
        call.download((long long*)out, d_out, (size_t)n_out);
        call.sync();
    }
    if (int rc = call.finish("frame count kernels failed")) return rc;
    if (!sane) FAIL(ctx, VBX_ERR_HIP, "vbx_frame_counts: the cell or class counts that came back do not fit their room");
    if (!room) FAIL(ctx, VBX_ERR_INVALID, "vbx_frame_counts: the result has %lld entries, out has room for %lld", n_out, (long long)out_cap);
    std::memcpy(info, got.data(), sizeof(int32_t) * got.size());
    return VBX_OK;
}

}  // extern "C"
