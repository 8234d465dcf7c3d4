// vbx_labels_score.hpp -- md-eval diarization error of LABEL SEQUENCES: many hypotheses per recording, the turns and the
// cell edges of every hypothesis built on the device.
//
// A grid search over Fa, Fb and loopP scores G label sequences per recording against ONE reference on ONE set of segment
// times.  vbx_rttm_score takes turns and edges the host prepared per (reference, hypothesis) pair; here the host prepares the
// reference's side once per recording and the device does per hypothesis what vbhmm.merge_adjacent_labels and score._Pair do:
//
// labels_turns (kernel A), one workgroup per hypothesis, kLabBlock segments per pass, one per thread.  Between neighbours
// i, i + 1 there is a cut where the labels differ or the segments neither overlap nor are close in numpy's sense
// (|a - b| <= 1e-8 + 1e-5 |b|, the product and the sum rounded one by one); segment i opens a turn after a cut and closes one
// before a cut.  An inclusive scan of the "opens" flags (LDS, Hillis-Steele, the count of the earlier passes carried in a
// register) numbers the turns; the thread that opens turn k writes its begin and label, the one that closes it its end.  Where
// the next turn begins before this one ends both times become (end + begin) / 2, computed by either thread from the times
// of the SEGMENTS, which is what numpy's vectorised assignment reads.  The reference turns of the recording are copied in front
// of them: rttm_cells_kernel wants the turns of a pair side by side.
//
// labels_edges (kernel B), one workgroup per hypothesis.  The host guarantees starts < ends, both non-decreasing, so the turns
// are a chain b0 <= e0 <= b1 <= e1 ...: the 2 n boundaries come out of kernel A sorted, and merged turns of one speaker
// cannot overlap (merge_turns(touching=False) would change nothing).  The reference's part of the edge list -- reference
// boundaries, collar zone ends, lo and hi, clipped, sorted, distinct -- comes from the host; lo = min(first reference begin,
// starts[0]) and hi likewise do not depend on the labels.  A system boundary is KEPT unless it equals its predecessor or a
// reference edge (binary search); the scan of kernel A over the kept flags gives its place among the kept ones, the binary
// search its place among the reference edges, the sum is its place in the union.  A reference edge goes to its own index
// plus the number of kept boundaries below it (binary search in the boundaries, exclusive prefix of the scan).  The result is
// np.unique(np.clip(concat(...), lo, hi)) of score._Pair for that hypothesis, bit for bit: nothing is computed, only placed.
// A turn WITHOUT duration (three neighbours that share both times: the two midpoints coincide) needs no special case: its
// boundary is the one of its neighbours, so it adds no edge, and rttm_cells_kernel compares strictly, so it is never active.
// Its speaker is left out of the mask of speakers with a turn of positive duration that this kernel also reduces (an OR:
// any order gives the same bits), which is how the host names the columns as score._Pair would.
//
// Totals: rttm_cells_kernel, rttm_acc_kernel, rttm_fin_kernel of vbx_rttm_score.hpp UNCHANGED, through that header's RttmPlan
// (the same planning and launch code as vbx_rttm_score), on RttmPair records whose turn_off / edge_off point into what A and
// B wrote.  Between the two phases ONE small download: (turns, edges, speaker
// mask) per hypothesis, 16 bytes each; the grids are then exact, as in vbx_rttm_score, and not an upper bound.
// No atomics anywhere: every sum and every scan runs in a fixed order, a hypothesis gives the same bytes in any batch.
#pragma once
#include "vbx_device.hpp"

namespace vbx {

constexpr int kLabBlock = 256;             // segments (kernel A) or boundaries (kernel B) per scan pass: one per thread
constexpr int kLabInfo = 4;                // int32 per hypothesis that come back: turns, edges, speaker mask low / high

struct LabRec {
    long long seg_off;    // starts[T] at seg_off, ends[T] at seg_off + T
    long long rturn_off;  // first of its n_ref_turns reference turns
    long long redge_off;  // first of its n_ref_edges reference edges
    int T, n_ref_turns, n_ref_edges, n_ref;
};

struct LabHyp {
    long long lab_off;    // first of its T labels
    long long turn_off;   // first of its turns: n_ref_turns copied reference turns, then room for T system turns
    long long edge_off;   // room for n_ref_edges + 2 T edges
    long long pre_off;    // room for 2 T + 1 exclusive prefixes of the kept flags
    int rec, n_sys;
};

// inclusive scan of one int per thread over the 256 threads of a workgroup; sh[kLabBlock - 1] holds the total afterwards
__device__ __forceinline__ int lab_block_scan(int v, int* sh, int tid) {
    __syncthreads();                                                  // (the previous scan has been read)
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < kLabBlock; d <<= 1) {
        const int add = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += add;
        __syncthreads();
    }
    return sh[tid];
}

// vbhmm.merge_adjacent_labels: is there a cut between a segment that ends at e and the next one, which starts at s?
__device__ __forceinline__ bool lab_gap(double e, double s) {
    const double tol = __dadd_rn(1e-8, __dmul_rn(1e-5, fabs(s)));     // np.isclose(e, s): atol + rtol * |s|, each rounded
    return !(fabs(e - s) <= tol || e > s);
}

// grid = hypotheses
__global__ __launch_bounds__(256) void labels_turns_kernel(const LabRec* __restrict__ recs, const LabHyp* __restrict__ hyps,
                                                           const double* __restrict__ seg, const int* __restrict__ labels,
                                                           const double* __restrict__ rtb, const double* __restrict__ rte,
                                                           const int* __restrict__ rspk, double* __restrict__ tbeg,
                                                           double* __restrict__ tend, int* __restrict__ tspk,
                                                           int* __restrict__ info) {
    __shared__ int scan_sh[kLabBlock];
    const LabHyp hy = hyps[blockIdx.x];
    const LabRec rc = recs[hy.rec];
    const int tid = threadIdx.x, T = rc.T;
    const double* starts = seg + rc.seg_off;
    const double* ends = starts + T;
    const int* lab = labels + hy.lab_off;
    for (int t = tid; t < rc.n_ref_turns; t += kLabBlock) {
        tbeg[hy.turn_off + t] = rtb[rc.rturn_off + t];
        tend[hy.turn_off + t] = rte[rc.rturn_off + t];
        tspk[hy.turn_off + t] = rspk[rc.rturn_off + t];
    }
    const long long sys_off = hy.turn_off + rc.n_ref_turns;
    int base = 0;                                                     // turns opened in the earlier passes
    for (int i0 = 0; i0 < T; i0 += kLabBlock) {
        const int i = i0 + tid;
        const bool live = i < T;
        bool opens = false, closes = false;
        double b = 0.0, e = 0.0;
        int l = 0;
        if (live) {
            b = starts[i];
            e = ends[i];
            l = lab[i];
            opens = i == 0;
            closes = i == T - 1;
            if (i > 0) {
                const double pe = ends[i - 1];
                if (lab[i - 1] != l || lab_gap(pe, b)) {
                    opens = true;
                    if (b < pe) b = (pe + b) / 2.0;                   // (the midpoint of the overlap, from the segments' times)
                }
            }
            if (i < T - 1) {
                const double ns = starts[i + 1];
                if (lab[i + 1] != l || lab_gap(e, ns)) {
                    closes = true;
                    if (ns < e) e = (e + ns) / 2.0;
                }
            }
        }
        const int k = base + lab_block_scan(opens ? 1 : 0, scan_sh, tid) - 1;      // the turn segment i belongs to
        if (opens) {
            tbeg[sys_off + k] = b;
            tspk[sys_off + k] = l;
        }
        if (closes) tend[sys_off + k] = e;
        base += scan_sh[kLabBlock - 1];
    }
    if (tid == 0) info[(long long)blockIdx.x * kLabInfo] = base;
}

// grid = hypotheses
__global__ __launch_bounds__(256) void labels_edges_kernel(const LabRec* __restrict__ recs, const LabHyp* __restrict__ hyps,
                                                           const double* __restrict__ redges, const double* __restrict__ tbeg,
                                                           const double* __restrict__ tend, const int* __restrict__ tspk,
                                                           double* __restrict__ edges, int* __restrict__ pre,
                                                           int* __restrict__ info) {
    __shared__ int scan_sh[kLabBlock];
    __shared__ unsigned long long mask_sh[kLabBlock];
    const LabHyp hy = hyps[blockIdx.x];
    const LabRec rc = recs[hy.rec];
    const int tid = threadIdx.x;
    const int n_turns = info[(long long)blockIdx.x * kLabInfo];
    const int nb = 2 * n_turns, na = rc.n_ref_edges;
    const double* A = redges + rc.redge_off;
    const double* sb = tbeg + hy.turn_off + rc.n_ref_turns;
    const double* se = tend + hy.turn_off + rc.n_ref_turns;
    const int* ss = tspk + hy.turn_off + rc.n_ref_turns;
    double* out = edges + hy.edge_off;
    int* pr = pre + hy.pre_off;
    auto bound = [&](int j) { return (j & 1) ? se[j >> 1] : sb[j >> 1]; };
    unsigned long long mask = 0;
    int base = 0;                                                     // boundaries kept in the earlier passes
    for (int j0 = 0; j0 < nb; j0 += kLabBlock) {
        const int j = j0 + tid;
        bool keep = false;
        double v = 0.0;
        int rank = 0;
        if (j < nb) {
            v = bound(j);
            int lo = 0, hi = na;                                      // rank = number of reference edges below v
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (A[mid] < v) lo = mid + 1; else hi = mid;
            }
            rank = lo;
            keep = !(rank < na && A[rank] == v) && !(j > 0 && bound(j - 1) == v);
            if (!(j & 1) && bound(j + 1) > v) mask |= 1ull << (ss[j >> 1] & 63);      // a turn of positive duration
        }
        const int incl = base + lab_block_scan(keep ? 1 : 0, scan_sh, tid);
        if (j < nb) pr[j] = incl - (keep ? 1 : 0);
        if (keep) out[rank + incl - 1] = v;
        base += scan_sh[kLabBlock - 1];
    }
    if (tid == 0) pr[nb] = base;
    mask_sh[tid] = mask;
    __syncthreads();                                                  // (and pre[] of this workgroup is visible to it)
    for (int d = kLabBlock / 2; d > 0; d >>= 1) {
        if (tid < d) mask_sh[tid] |= mask_sh[tid + d];
        __syncthreads();
    }
    for (int i = tid; i < na; i += kLabBlock) {
        const double a = A[i];
        int lo = 0, hi = nb;                                          // the first boundary not below a
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (bound(mid) < a) lo = mid + 1; else hi = mid;
        }
        out[i + pr[lo]] = a;
    }
    if (tid == 0) {
        int* o = info + (long long)blockIdx.x * kLabInfo;
        o[1] = na + base;
        o[2] = (int)(unsigned)(mask_sh[0] & 0xffffffffull);
        o[3] = (int)(unsigned)(mask_sh[0] >> 32);
    }
}

}  // namespace vbx

// ---- host glue (included by vbx_capi.hip after vbx_host_call.hpp and vbx_rttm_score.hpp, whose RttmPlan phase 2 runs) -------
extern "C" {

int vbx_labels_score(vbx_ctx* ctx, int32_t n_rec, const int32_t* rec_counts, const double* seg_times, const double* ref_turns,
                     const int32_t* ref_spk, const double* ref_edges, int32_t n_hyp, const int32_t* hyp, const int32_t* labels,
                     double collar, int ignore_overlaps, double* out, int32_t* info) {
    using vbx::LabHyp;
    using vbx::LabRec;
    if (!ctx) return VBX_ERR_INVALID;
    if (n_rec <= 0 || n_hyp <= 0 || !rec_counts || !seg_times || !ref_edges || !hyp || !labels || !out)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_score: bad argument");
    if (!(collar >= 0.0) || !std::isfinite(collar)) FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_score: collar=%g is not a length", collar);
    // ---- the recordings: everything the kernels index with is checked here, before any launch ----
    std::vector<LabRec> recs((size_t)n_rec);
    long long n_seg = 0, n_rturns = 0, n_redges = 0;
    for (int r = 0; r < n_rec; ++r) {
        const int32_t* c = rec_counts + 4 * (size_t)r;
        const int T = c[0], nrt = c[1], nr = c[2], nre = c[3];
        if (T <= 0 || nrt < 0 || nr < 0 || nre < 2 || T > (1 << 26) || nrt > (1 << 26) || nre > (1 << 28))
            FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_score: recording %d: negative or oversized count", r);
        if (nr > vbx::kRttmMaxSpk)
            FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_labels_score: recording %d has %d reference speakers, at most %d a side", r, nr, vbx::kRttmMaxSpk);
        if (nrt > 0 && (!ref_turns || !ref_spk)) FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_score: NULL argument");
        LabRec& rc = recs[r];
        rc.seg_off = 2 * n_seg;
        rc.rturn_off = n_rturns;
        rc.redge_off = n_redges;
        rc.T = T;
        rc.n_ref_turns = nrt;
        rc.n_ref_edges = nre;
        rc.n_ref = nr;
        const double* st = seg_times + rc.seg_off;
        const double* en = st + T;
        for (int i = 0; i < T; ++i) {
            // a segment without duration would be a turn merge_turns drops, and its boundary an edge score._Pair does not have
            if (!std::isfinite(st[i]) || !std::isfinite(en[i]) || !(st[i] < en[i]))
                FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_score: recording %d: segment %d [%g, %g] has no positive finite duration", r, i, st[i], en[i]);
            if (i > 0 && (st[i] < st[i - 1] || en[i] < en[i - 1]))
                FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_score: recording %d: times decrease at segment %d", r, i);
        }
        if (int bad = check_turn_speakers(ctx, "vbx_labels_score", "recording", r, "reference turn", ref_spk + n_rturns, 0, nrt, nr)) return bad;
        const double* ed = ref_edges + n_redges;
        for (int k = 0; k < nre; ++k)
            if (!std::isfinite(ed[k]) || (k > 0 && !(ed[k - 1] < ed[k])))
                FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_score: recording %d: reference edges not sorted and distinct at %d", r, k);
        if (ed[0] > st[0] || ed[nre - 1] < en[T - 1])
            FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_score: recording %d: the reference edges [%g, %g] do not span the segments [%g, %g]", r, ed[0], ed[nre - 1], st[0], en[T - 1]);
        n_seg += T;
        n_rturns += nrt;
        n_redges += nre;
    }
    // ---- the hypotheses ----
    std::vector<LabHyp> hyps((size_t)n_hyp);
    long long n_lab = 0, n_turns = 0, n_edges = 0, n_pre = 0;
    for (int h = 0; h < n_hyp; ++h) {
        const int r = hyp[2 * (size_t)h], ns = hyp[2 * (size_t)h + 1];
        if (r < 0 || r >= n_rec) FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_score: hypothesis %d names recording %d of %d", h, r, n_rec);
        if (ns <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_score: hypothesis %d: negative or oversized count", h);
        if (ns > vbx::kRttmMaxSpk)
            FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_labels_score: hypothesis %d has %d system speakers, at most %d a side", h, ns, vbx::kRttmMaxSpk);
        const LabRec& rc = recs[r];
        for (int i = 0; i < rc.T; ++i) {
            const int l = labels[n_lab + i];                          // a label is a shift count and a column on the device
            if (l < 0 || l >= ns) FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_score: hypothesis %d: label %d of segment %d outside [0, %d)", h, l, i, ns);
        }
        LabHyp& hy = hyps[h];
        hy.lab_off = n_lab;
        hy.turn_off = n_turns;
        hy.edge_off = n_edges;
        hy.pre_off = n_pre;
        hy.rec = r;
        hy.n_sys = ns;
        n_lab += rc.T;
        n_turns += (long long)rc.n_ref_turns + rc.T;
        n_edges += (long long)rc.n_ref_edges + 2LL * rc.T;
        n_pre += 2LL * rc.T + 1;
    }
    if (n_turns > 0x7fffffffLL || n_edges > 0x7fffffffLL)
        FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_labels_score: %lld edges, %lld turns in one call", n_edges, n_turns);
    const TurnPlanes rt(ref_turns, n_rturns);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> counts((size_t)n_hyp * vbx::kLabInfo);
    RttmPlan pl;
    DeviceCall call(ctx);                         // (after every host buffer its copies read or write)
    // ---- phase 1: turns and edges of every hypothesis ----
    const LabRec* d_recs = call.upload(recs.data(), recs.size());
    const LabHyp* d_hyps = call.upload(hyps.data(), hyps.size());
    const double* d_seg = call.upload(seg_times, (size_t)(2 * n_seg));
    const double* d_rb = call.upload(rt.beg.data(), (size_t)n_rturns);
    const double* d_re = call.upload(rt.end.data(), (size_t)n_rturns);
    const int* d_rspk = call.upload(ref_spk, (size_t)n_rturns);
    const double* d_redges = call.upload(ref_edges, (size_t)n_redges);
    const int* d_lab = call.upload(labels, (size_t)n_lab);
    double* d_tb = call.alloc<double>((size_t)n_turns);
    double* d_te = call.alloc<double>((size_t)n_turns);
    int* d_spk = call.alloc<int>((size_t)n_turns);
    double* d_edges = call.alloc<double>((size_t)n_edges);
    int* d_pre = call.alloc<int>((size_t)n_pre);
    int* d_info = call.alloc<int>(counts.size());
    if (call.ok()) {
        hipLaunchKernelGGL(vbx::labels_turns_kernel, dim3((unsigned)n_hyp), dim3(256), 0, call.st, d_recs, d_hyps, d_seg, d_lab, d_rb,
                           d_re, d_rspk, d_tb, d_te, d_spk, d_info);
        hipLaunchKernelGGL(vbx::labels_edges_kernel, dim3((unsigned)n_hyp), dim3(256), 0, call.st, d_recs, d_hyps, d_redges, d_tb, d_te,
                           d_spk, d_edges, d_pre, d_info);
        call.launched();
    }
    call.download(counts.data(), d_info, counts.size());
    call.sync();
    // ---- phase 2: the plan of vbx_rttm_score on what phase 1 wrote ----
    bool sane = true;
    for (int h = 0; call.ok() && sane && h < n_hyp; ++h) {
        const LabHyp& hy = hyps[h];
        const LabRec& rec = recs[hy.rec];
        const int nt = counts[(size_t)h * vbx::kLabInfo], ne = counts[(size_t)h * vbx::kLabInfo + 1];
        sane = nt >= 1 && nt <= rec.T && ne >= rec.n_ref_edges && ne <= rec.n_ref_edges + 2 * nt;   // (else it would index past its room)
        if (sane) rttm_plan_add(pl, ne - 1, rec.n_ref_turns, nt, rec.n_ref, hy.n_sys, hy.edge_off, hy.turn_off);
    }
    if (pl.n_cells > 0x7fffffffLL || pl.cls_items.size() > 0x7fffffffULL) sane = false;
    if (sane) {
        rttm_plan_run(call, pl, d_edges, d_tb, d_te, d_spk, collar, ignore_overlaps, out);
        call.sync();
    }
    if (int rc = call.finish("labels score kernels failed")) return rc;
    if (!sane) FAIL(ctx, VBX_ERR_HIP, "vbx_labels_score: the turn or edge counts that came back do not fit their room");
    if (info) std::memcpy(info, counts.data(), sizeof(int32_t) * counts.size());
    return VBX_OK;
}

}  // extern "C"
