// vbx_labels_frame.hpp -- the integer frame counts of vbx_frame_score.hpp for LABEL SEQUENCES: many hypotheses per recording,
// the turns of every hypothesis built on the device.
//
// A grid search that judges by JER, B-cubed or an information-theoretic column needs, for G label sequences per recording
// against ONE reference on ONE set of segment times, what vbx_frame_counts gives for a (reference, system) pair.  What
// depends on the recording alone is done once per recording; the rest once per hypothesis, on the device:
//
// per recording   its merged reference turns go up once.  frame_bounds, frame_sort and frame_cells of vbx_frame_score.hpp,
//                 UNCHANGED, run on "pairs" that are a recording's reference side and its extent: F(begin), F(end) of every
//                 reference turn, F(lo), F(hi), and those values sorted and distinct.  The quadratic frame_sort therefore
//                 costs 2 (reference turns) + 2 boundaries squared once per recording, whatever the number of hypotheses.
// per hypothesis  labels_turns_kernel of vbx_labels_score.hpp, UNCHANGED, writes its turns behind a copy of the
//                 recording's reference turns.  labels_frames_kernel (below), one workgroup per hypothesis, then does
//                 what frame_bounds, frame_sort and frame_cells do for a pair: F of the system boundaries; the reference's F
//                 copied, not computed again; and the union of the two sorted lists.  The host guarantees starts < ends, both
//                 non-decreasing, so the system turns are a chain b0 <= e0 <= b1 <= ..., F never decreases with its argument,
//                 and the system's frame indices come out sorted.  A system index is KEPT unless it equals its predecessor
//                 or a reference value (binary search); the scan over the kept flags gives its place among the kept, the
//                 search its place among the reference values, the sum its place in the union.  A reference value goes to
//                 its own index plus the number of kept values below it.  This is kernel B of section 18 on integers; nothing
//                 is sorted.  It also reduces the mask of the labels that have a turn of positive duration (an OR), and
//                 writes the number of turns into the hypothesis's FrmPair, which frame_masks reads next.
// then            frame_masks, frame_firsts, frame_classes, the one download that sizes the result, and frame_acc, UNCHANGED
//                 and through the FrmPlan of vbx_frame_score.hpp: a hypothesis is cut and summed as a pair is.
//
// The extent of a hypothesis is its recording's: lo = min(reference begins, starts[0]), hi = max(reference ends, ends[T - 1]);
// the system's extent is [starts[0], ends[T - 1]] whatever the labels (section 18).  Every sum and scan runs in a fixed order
// on integers and nothing is added across threads: a hypothesis gives the same bytes alone, at any place of a batch, and
// among other hypotheses of its recording.
#pragma once
#include "vbx_frame_score.hpp"

namespace vbx {

// grid = hypotheses.  rpairs / ridx / runiq / rinfo: the recordings' plan after frame_cells; pairs: the hypotheses' plan
__global__ __launch_bounds__(256) void labels_frames_kernel(const LabHyp* __restrict__ hyps, const FrmPair* __restrict__ rpairs,
                                                            FrmPair* pairs, const long long* __restrict__ ridx,
                                                            const long long* __restrict__ runiq, const int* __restrict__ rinfo,
                                                            const double* __restrict__ tbeg, const double* __restrict__ tend,
                                                            const int* __restrict__ tspk, double step, long long* idx,
                                                            long long* __restrict__ uniq, int* pre, int* linfo,
                                                            int* __restrict__ info) {
    __shared__ int scan_sh[kLabBlock];
    __shared__ unsigned long long mask_sh[kLabBlock];
    const LabHyp hy = hyps[blockIdx.x];
    const FrmPair rp = rpairs[hy.rec];
    const long long bnd_off = pairs[blockIdx.x].bnd_off, n_frames = rp.n_frames;
    const int tid = threadIdx.x;
    const int nrt = rp.n_ref_turns, n_turns = linfo[(long long)blockIdx.x * kLabInfo];
    const int nt = nrt + n_turns, nb = 2 * n_turns;
    const int na = rinfo[(long long)hy.rec * kFrmInfo] + 1;           // the recording's distinct values (cells + 1)
    const long long* A = runiq + rp.bnd_off;
    const double* sb = tbeg + hy.turn_off + nrt;
    const double* se = tend + hy.turn_off + nrt;
    const int* ss = tspk + hy.turn_off + nrt;
    long long* fb = idx + bnd_off;                                    // F(begin) of the nt turns, the reference's first
    long long* fe = fb + nt;                                          // F(end)
    long long* out = uniq + bnd_off;
    int* pr = pre + hy.pre_off;
    for (int t = tid; t < nrt; t += kLabBlock) {                      // the reference's: computed once per recording
        fb[t] = ridx[rp.bnd_off + t];
        fe[t] = ridx[rp.bnd_off + nrt + t];
    }
    unsigned long long mask = 0;
    for (int k = tid; k < n_turns; k += kLabBlock) {
        const double b = sb[k], e = se[k];
        fb[nrt + k] = frm_index(b, step, n_frames);
        fe[nrt + k] = frm_index(e, step, n_frames);
        if (e > b) mask |= 1ull << (ss[k] & 63);                      // a turn of positive duration
    }
    mask_sh[tid] = mask;
    __syncthreads();                                                  // (fb, fe of this workgroup are visible to it)
    for (int d = kLabBlock / 2; d > 0; d >>= 1) {
        if (tid < d) mask_sh[tid] |= mask_sh[tid + d];
        __syncthreads();
    }
    auto bound = [&](int j) { return (j & 1) ? fe[nrt + (j >> 1)] : fb[nrt + (j >> 1)]; };
    int base = 0;                                                     // values kept in the earlier passes
    for (int j0 = 0; j0 < nb; j0 += kLabBlock) {
        const int j = j0 + tid;
        bool keep = false;
        long long v = 0;
        int rank = 0;
        if (j < nb) {
            v = bound(j);
            int lo = 0, hi = na;                                      // rank = number of reference values below v
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (A[mid] < v) lo = mid + 1; else hi = mid;
            }
            rank = lo;
            keep = !(rank < na && A[rank] == v) && !(j > 0 && bound(j - 1) == v);
        }
        const int incl = base + lab_block_scan(keep ? 1 : 0, scan_sh, tid);
        if (j < nb) pr[j] = incl - (keep ? 1 : 0);
        if (keep) out[rank + incl - 1] = v;
        base += scan_sh[kLabBlock - 1];
    }
    if (tid == 0) pr[nb] = base;
    __syncthreads();                                                  // (pre[] of this workgroup is visible to it)
    for (int i = tid; i < na; i += kLabBlock) {
        const long long a = A[i];
        int lo = 0, hi = nb;                                          // the first system value not below a
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (bound(mid) < a) lo = mid + 1; else hi = mid;
        }
        out[i + pr[lo]] = a;
    }
    if (tid == 0) {
        pairs[blockIdx.x].n_sys_turns = n_turns;                      // (the plan held the room: T)
        info[(long long)blockIdx.x * kFrmInfo] = na + base - 1;       // cells
        int* o = linfo + (long long)blockIdx.x * kLabInfo;
        o[2] = (int)(unsigned)(mask_sh[0] & 0xffffffffull);
        o[3] = (int)(unsigned)(mask_sh[0] >> 32);
    }
}

}  // namespace vbx

// ---- host glue (included by vbx_capi.hip after vbx_labels_score.hpp and vbx_frame_score.hpp, whose FrmPlan runs) -------------
extern "C" {

int vbx_labels_frame_counts(vbx_ctx* ctx, int32_t n_rec, const int32_t* rec_counts, const double* seg_times, const double* ref_turns,
                            const int32_t* ref_spk, int32_t n_hyp, const int32_t* hyp, const int32_t* labels, double step,
                            int32_t* info, uint64_t* classes, int64_t* out, int64_t out_cap, uint64_t* label_masks) {
    using vbx::LabHyp;
    using vbx::LabRec;
    if (!ctx) return VBX_ERR_INVALID;
    if (n_rec <= 0 || n_hyp <= 0 || !rec_counts || !seg_times || !hyp || !labels || !info || !classes || !out || out_cap < 0 || !label_masks)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_frame_counts: bad argument");
    if (!(step > 0.0) || !std::isfinite(step)) FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_frame_counts: step=%g is not a length", step);
    // ---- the recordings: everything the kernels index or shift with is checked here, before any launch ----
    std::vector<LabRec> recs((size_t)n_rec);
    FrmPlan rpl, hpl;                                                 // the recordings' reference sides; the hypotheses
    long long n_seg = 0, n_rturns = 0;
    for (int r = 0; r < n_rec; ++r) {
        const int32_t* c = rec_counts + 3 * (size_t)r;
        const int T = c[0], nrt = c[1], nr = c[2];
        if (T <= 0 || nrt < 0 || nr < 0 || T > (1 << 24) || nrt > (1 << 24))
            FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_frame_counts: recording %d: negative or oversized count", r);
        if (nr > vbx::kFrmMaxSpk)
            FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_labels_frame_counts: recording %d has %d reference speakers, at most %d a side", r, nr, vbx::kFrmMaxSpk);
        if (nrt > 0 && (!ref_turns || !ref_spk)) FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_frame_counts: NULL argument");
        LabRec& rc = recs[r];
        rc = LabRec{};
        rc.seg_off = 2 * n_seg;
        rc.rturn_off = n_rturns;
        rc.T = T;
        rc.n_ref_turns = nrt;
        rc.n_ref = nr;
        const double* st = seg_times + rc.seg_off;
        const double* en = st + T;
        for (int i = 0; i < T; ++i) {
            // a segment without duration would be a turn merge_turns drops: its boundary would cut a cell numpy does not cut
            if (!std::isfinite(st[i]) || !std::isfinite(en[i]) || !(st[i] < en[i]))
                FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_frame_counts: recording %d: segment %d [%g, %g] has no positive finite duration", r, i, st[i], en[i]);
            if (i > 0 && (st[i] < st[i - 1] || en[i] < en[i - 1]))
                FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_frame_counts: recording %d: times decrease at segment %d", r, i);
        }
        if (int bad = check_turn_speakers(ctx, "vbx_labels_frame_counts", "recording", r, "reference turn", ref_spk + n_rturns, 0, nrt, nr)) return bad;
        double lo = st[0], hi = en[T - 1];
        for (long long t = n_rturns; t < n_rturns + nrt; ++t) {
            const double b = ref_turns[2 * t], e = ref_turns[2 * t + 1];
            if (!std::isfinite(b) || !std::isfinite(e) || !(b <= e))
                FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_frame_counts: recording %d: reference turn %lld [%g, %g] is not a finite interval", r, t - n_rturns, b, e);
            lo = std::min(lo, b);
            hi = std::max(hi, e);
        }
        if (!(hi / step < 1099511627776.0))
            FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_frame_counts: recording %d: the extent [%g, %g] is not one of fewer than 2^40 frames", r, lo, hi);
        frm_plan_add(rpl, nrt, 0, nr, 0, lo, hi, step, n_rturns);
        n_seg += T;
        n_rturns += nrt;
    }
    // ---- the hypotheses ----
    std::vector<LabHyp> hyps((size_t)n_hyp);
    long long n_lab = 0, n_turns = 0, n_pre = 0;
    for (int h = 0; h < n_hyp; ++h) {
        const int r = hyp[2 * (size_t)h], ns = hyp[2 * (size_t)h + 1];
        if (r < 0 || r >= n_rec) FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_frame_counts: hypothesis %d names recording %d of %d", h, r, n_rec);
        if (ns <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_frame_counts: hypothesis %d: negative or oversized count", h);
        if (ns > vbx::kFrmMaxSpk)
            FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_labels_frame_counts: hypothesis %d has %d system speakers, at most %d a side", h, ns, vbx::kFrmMaxSpk);
        const LabRec& rc = recs[r];
        for (int i = 0; i < rc.T; ++i) {
            const int l = labels[n_lab + i];                          // a label is a shift count and a column on the device
            if (l < 0 || l >= ns) FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_frame_counts: hypothesis %d: label %d of segment %d outside [0, %d)", h, l, i, ns);
        }
        LabHyp& hy = hyps[h];
        hy = LabHyp{};
        hy.lab_off = n_lab;
        hy.turn_off = n_turns;
        hy.pre_off = n_pre;
        hy.rec = r;
        hy.n_sys = ns;
        frm_plan_add(hpl, rc.n_ref_turns, rc.T, rc.n_ref, ns, rpl.pairs[r].lo, rpl.pairs[r].hi, step, n_turns);
        n_lab += rc.T;
        n_turns += (long long)rc.n_ref_turns + rc.T;
        n_pre += 2LL * rc.T + 1;
    }
    if (n_turns > 0x7fffffffLL || !frm_plan_fits(hpl) || !frm_plan_fits(rpl))
        FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_labels_frame_counts: %lld turns in one call", n_turns);
    const TurnPlanes rt(ref_turns, n_rturns);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> got((size_t)n_hyp * vbx::kFrmInfo), lgot((size_t)n_hyp * vbx::kLabInfo);
    DeviceCall call(ctx);                         // (after every host buffer its copies read or write)
    // ---- per recording: the reference's frame indices, sorted and distinct ----
    const LabRec* d_recs = call.upload(recs.data(), recs.size());
    const double* d_rb = call.upload(rt.beg.data(), (size_t)n_rturns);
    const double* d_re = call.upload(rt.end.data(), (size_t)n_rturns);
    const int* d_rspk = call.upload(ref_spk, (size_t)n_rturns);
    const FrmDev rd = frm_plan_upload(call, rpl, true);
    frm_plan_cut(call, rpl, rd, d_rb, d_re, step);
    // ---- per hypothesis: turns, cells, masks and classes ----
    const LabHyp* d_hyps = call.upload(hyps.data(), hyps.size());
    const double* d_seg = call.upload(seg_times, (size_t)(2 * n_seg));
    const int* d_lab = call.upload(labels, (size_t)n_lab);
    double* d_tb = call.alloc<double>((size_t)n_turns);
    double* d_te = call.alloc<double>((size_t)n_turns);
    int* d_spk = call.alloc<int>((size_t)n_turns);
    int* d_pre = call.alloc<int>((size_t)n_pre);
    int* d_linfo = call.alloc<int>(lgot.size());
    const FrmDev hd = frm_plan_upload(call, hpl, false);
    if (call.ok()) {
        hipLaunchKernelGGL(vbx::labels_turns_kernel, dim3((unsigned)n_hyp), dim3(256), 0, call.st, d_recs, d_hyps, d_seg, d_lab, d_rb,
                           d_re, d_rspk, d_tb, d_te, d_spk, d_linfo);
        hipLaunchKernelGGL(vbx::labels_frames_kernel, dim3((unsigned)n_hyp), dim3(256), 0, call.st, d_hyps, rd.pairs, hd.pairs, rd.idx,
                           rd.uniq, rd.info, d_tb, d_te, d_spk, step, hd.idx, hd.uniq, d_pre, d_linfo, hd.info);
        call.launched();
    }
    frm_plan_classes(call, hpl, hd, d_spk, got.data(), classes);
    call.download(lgot.data(), d_linfo, lgot.size());
    call.sync();
    // ---- the sums: the plan of vbx_frame_counts, with the turns that came back ----
    bool sane = true;
    for (int h = 0; call.ok() && sane && h < n_hyp; ++h) {
        const int nt = lgot[(size_t)h * vbx::kLabInfo];
        sane = nt >= 1 && nt <= recs[hyps[h].rec].T;                  // (else it would index past its room)
        if (sane) hpl.pairs[h].n_sys_turns = nt;
    }
    const int sums = sane ? frm_plan_sums(call, hpl, hd, got.data(), out, out_cap) : kFrmSumsInsane;
    if (int rc = call.finish("labels frame count kernels failed")) return rc;
    if (sums == kFrmSumsInsane) FAIL(ctx, VBX_ERR_HIP, "vbx_labels_frame_counts: the turn, cell or class counts that came back do not fit their room");
    if (sums == kFrmSumsNoRoom) FAIL(ctx, VBX_ERR_INVALID, "vbx_labels_frame_counts: the result has %lld entries, out has room for %lld", hpl.n_out, (long long)out_cap);
    std::memcpy(info, got.data(), sizeof(int32_t) * got.size());
    for (int h = 0; h < n_hyp; ++h)
        label_masks[h] = (uint64_t)(uint32_t)lgot[(size_t)h * vbx::kLabInfo + 2] | (uint64_t)(uint32_t)lgot[(size_t)h * vbx::kLabInfo + 3] << 32;
    return VBX_OK;
}

}  // extern "C"
