// vbx_host_set.hpp -- C ABI: the ways a batch slot is set.  Two independent choices:
//   where rho, Phi and sum G come from:  host X (the pinned slot, set_recording_impl) | resident rows (rho_from_resident) |
//                                        another slot's rows (rho_attach) | a copy of another arena's rows (rho_clone)
//   where the initial responsibilities come from:  host gamma0 (set_recording_impl) | a gamma writer on the device
//                                                  (set_slot_on_device: labels, random labels, speaker turns)
// Every leaf setter reads top to bottom: validate everything -> claim_slot -> rho -> gamma -> slot_is_set.
// (one translation unit with vbx_capi.hip, which includes it after vbx_host_group.hpp, vbx_host_ahc.hpp and
//  vbx_turn_init.hpp; not a stand-alone header)
#pragma once

// ---- validation: nothing of the batch is touched before all of it has passed ---------------------------------------------
static int check_slot_hyper(vbx_batch* b, int rec, const char* fn, double loopProb, double Fa, double Fb) {
    if (rec < 0 || rec >= b->n_rec) FAIL(b->ctx, VBX_ERR_INVALID, "%s: recording index %d out of range", fn, rec);
    if (!(loopProb >= 0.0 && loopProb <= 1.0)) FAIL(b->ctx, VBX_ERR_INVALID, "loopProb=%g outside [0,1]", loopProb);
    if (!(Fa > 0.0) || !(Fb > 0.0)) FAIL(b->ctx, VBX_ERR_INVALID, "Fa and Fb must be positive");
    return VBX_OK;
}

static int check_phi(vbx_ctx* ctx, const double* Phi, int D) {
    for (int d = 0; d < D; ++d)
        if (!(Phi[d] > 0.0)) FAIL(ctx, VBX_ERR_INVALID, "Phi[%d] must be positive", d);
    return VBX_OK;
}

// the resident rows recording `rec` is to be built from
static int check_resident_rows(vbx_batch* b, int rec, const vbx_xvectors* xv, int64_t row0, const double** d_fea) {
    *d_fea = xvectors_fea_rows(xv, row0, b->recs[rec].T, b->D, b->ctx->device);
    if (!*d_fea)
        FAIL(b->ctx, VBX_ERR_INVALID, "rows [%lld, +%d) x %d dims are not in the resident x-vectors", (long long)row0, b->recs[rec].T, b->D);
    return VBX_OK;
}

// recording `src` of `from` (nullptr: of `b` itself) as the source of the x-vectors of recording `rec` of `b`
static int check_slot_source(vbx_batch* b, int rec, vbx_batch* from, int src, const char* fn) {
    vbx_ctx* ctx = b->ctx;
    const vbx_batch* sb = from ? from : b;
    if (src < 0 || src >= sb->n_rec || (!from && src == rec)) FAIL(ctx, VBX_ERR_INVALID, "%s: recording %d / source %d out of range", fn, rec, src);
    if (!sb->is_set[src]) FAIL(ctx, VBX_ERR_STATE, "recording %d (the source of the x-vectors) has not been set", src);
    if (sb->recs[src].T != b->recs[rec].T)
        FAIL(ctx, VBX_ERR_INVALID, "recording %d has %d frames, its source %d has %d", rec, b->recs[rec].T, src, sb->recs[src].T);
    // (a source that reads the rows of `rec` itself would be unset by own_rho and leave `rec` pointing at rows that hold nothing)
    if (!from && b->share_src[src] == rec)
        FAIL(ctx, VBX_ERR_STATE, "recording %d reads the x-vectors of recording %d: it cannot be that recording's source", src, rec);
    if (from && (from->precision != b->precision || from->Dp != b->Dp || from->rsize != b->rsize))
        FAIL(ctx, VBX_ERR_STATE, "sub-batches of one group differ in layout");
    return VBX_OK;
}

// qinit_kernel and random_labels_kernel go through the staging block (whole Philox blocks are never stored past T, but the
// 16-byte stores want the block's alignment and its size checked)
static int check_labels_fit_staging(vbx_batch* b, int rec) {
    if (b->xstage_bytes < sizeof(int32_t) * (size_t)b->recs[rec].T) FAIL(b->ctx, VBX_ERR_STATE, "staging block too small for the labels");
    return VBX_OK;
}

// ---- the slot's bookkeeping ------------------------------------------------------------------------------------------------
// `rec` gets (back) a rho of its own: recordings that read its rows so far are unset, and it leaves the group it was in
static void own_rho(vbx_batch* b, int rec) {
    for (int i = 0; i < b->n_rec; ++i)
        if (i != rec && b->share_src[i] == rec) {
            b->share_src[i] = i;
            b->recs[i].rho_row0 = b->recs[i].row0;
            b->recs[i].rho_tile0 = b->recs[i].tile0;
            b->recs[i].rho_rec = i;
            b->is_set[i] = 0;
            b->order_dirty = true;
        }
    if (b->share_src[rec] != rec) b->order_dirty = true;
    b->share_src[rec] = rec;
    b->recs[rec].rho_row0 = b->recs[rec].row0;
    b->recs[rec].rho_tile0 = b->recs[rec].tile0;
    b->recs[rec].rho_rec = rec;
    b->split_dirty[rec] = 1;                                  // (every caller is about to give `rec` new x-vectors)
}

// the first change a setter makes: the hyper-parameters, and whoever shared the rows of `rec` must be set again
static void claim_slot(vbx_batch* b, int rec, double loopProb, double Fa, double Fb) {
    RecDesc& rd = b->recs[rec];
    rd.lp = loopProb;
    rd.Fa = Fa;
    rd.Fb = Fb;
    own_rho(b, rec);
}

// ... and the last
static void slot_is_set(vbx_batch* b, int rec) {
    b->is_set[rec] = 1;
    b->recs_dirty = true;
    b->mpart_valid = false;
}

// ---- rho from another recording ----------------------------------------------------------------------------------------
// the source lives on another stream, or was uploaded asynchronously: its rows, Phi and sum G must be complete before they are read
static int sync_source(vbx_batch* b, vbx_batch* sb) {
    const int rc = sync_uploads(sb);
    if (rc != VBX_OK && sb != b) b->ctx->err = sb->ctx->err;
    return rc;
}

// `rec` reads the rows of `src` of the same batch (of its owner, where `src` shares itself)
static int rho_attach(vbx_batch* b, int rec, int src) {
    const int owner = b->share_src[src];
    RecDesc& rd = b->recs[rec];
    rd.rho_row0 = b->recs[owner].row0;
    rd.rho_tile0 = b->recs[owner].tile0;
    rd.rho_rec = owner;
    b->share_src[rec] = owner;
    b->order_dirty = true;
    // the rows of rho this recording leaves unused lie behind another recording's: the last chunk of that one reads a whole
    // tile (finite values that meet gamma = 0, vbx_chunk_post.hpp), so they must not hold whatever the block held before
    HIPCHK(b->ctx, hipMemsetAsync((char*)b->d_rho + (size_t)rd.row0 * b->Dp * b->rsize, 0,
                                  (size_t)std::min(rd.T, kTileFrames) * b->Dp * b->rsize, b->ctx->stream));
    return VBX_OK;
}

// `rec` gets a COPY of the rows `src` of `from` reads -- another sub-batch of the same stream group, i.e. another device
// arena: a sweep over one recording that runs on several streams keeps one rho per stream (288 GB of HBM: a copy of 100 MB
// buys a stream of its own), shared by the points of that stream.  After sync_source(b, from).
static int rho_clone(vbx_batch* b, int rec, vbx_batch* from, int src) {
    const RecDesc& sd = from->recs[from->share_src[src]];
    const RecDesc& rd = b->recs[rec];
    HIPCHK(b->ctx, hipMemcpyAsync((char*)b->d_rho + (size_t)rd.row0 * b->Dp * b->rsize, (const char*)from->d_rho + (size_t)sd.row0 * b->Dp * b->rsize,
                                  (size_t)rd.T * b->Dp * b->rsize, hipMemcpyDeviceToDevice, b->ctx->stream));
    return VBX_OK;
}

// Phi and sum G follow the rows on the device: recording `src` of `sb` holds both (after sync_source).  The host setter's
// same-arena sharing does not come here: its source may still be on its way, and it takes them from the pinned slot
// (set_recording_impl).
static int phi_follows_on_device(vbx_batch* b, int rec, const vbx_batch* sb, int src) {
    HIPCHK(b->ctx, hipMemcpyAsync(b->d_phi + (size_t)rec * b->Dp, sb->d_phi + (size_t)src * b->Dp, sizeof(double) * b->Dp,
                                  hipMemcpyDeviceToDevice, b->ctx->stream));
    b->recs[rec].gsum = sb->recs[src].gsum;
    return VBX_OK;
}

extern "C++" {
namespace {
// ---- host X and host gamma0: the pinned slot ---------------------------------------------------------------------------
// X == nullptr: the rows are another recording's (rho_attach: Phi and sum G from the source's pinned slot or its device row)
// or in place already (share_src[rec] == rec: rho_clone and phi_follows_on_device have run).
template <typename R>
int set_recording_impl(vbx_batch* b, int rec, const void* X, int x_dtype, const double* Phi, const double* pi0,
                       const void* gamma0, int g_dtype, const double* alpha0, const double* invL0) {
    vbx_ctx* ctx = b->ctx;
    RecDesc& rd = b->recs[rec];
    const int D = b->D, Dp = b->Dp, Sp = b->Sp, S = rd.S;
    const long long T = rd.T;
    if (int rc = ensure_host_args(b); rc != VBX_OK) return rc;
    // (the pinned slot of this recording may still be the source of a copy in flight: the same recording set twice in a row)
    if (b->args_busy[rec])
        if (int rc = sync_uploads(b); rc != VBX_OK) return rc;
    const size_t per = (size_t)2 * Dp + Sp + 2;
    double* const phi = b->h_args + (size_t)rec * per;
    double* const sphi = phi + Dp;
    double* const pip = phi + 2 * Dp;
    double* const flags = phi + 2 * Dp + Sp;                  // what sync_uploads' scatter_args_kernel takes from this slot
    bool must_sync = !b->async_upload;
    if (X) {
        for (int d = 0; d < Dp; ++d) phi[d] = sphi[d] = 0.0;     // (padded dims: 0)
        for (int d = 0; d < D; ++d) {
            phi[d] = Phi[d];
            sphi[d] = std::sqrt(Phi[d]);
        }
        flags[0] = 1.0;                                       // (Phi goes to the device with the scatter of sync_uploads)
        // X -> staging -> rho, G; prep_kernel reads sqrt(Phi) from the pinned slot itself
        const size_t xbytes = (size_t)T * D * (x_dtype == VBX_F64 ? 8 : 4);
        HIPCHK(ctx, hipMemcpyAsync(b->d_xstage, X, xbytes, hipMemcpyHostToDevice, ctx->stream));
        if (x_dtype == VBX_F64) launch_prep<R, double>(b, rd, sphi); else launch_prep<R, float>(b, rd, sphi);
        HIPCHK(ctx, hipGetLastError());
        b->gsum_pending[rec] = 1;
    } else {
        const int src = b->share_src[rec];
        flags[0] = 0.0;
        if (src != rec) {
            const double* sphi_src = b->h_args + (size_t)src * per;
            if (sphi_src[per - 2] != 0.0) {                   // (the source's Phi is itself still on its way: take it from its slot)
                std::memcpy(phi, sphi_src, sizeof(double) * 2 * Dp);
                flags[0] = 1.0;
            } else {
                HIPCHK(ctx, hipMemcpyAsync(b->d_phi + (size_t)rec * Dp, b->d_phi + (size_t)src * Dp, sizeof(double) * Dp, hipMemcpyDeviceToDevice, ctx->stream));
            }
            rd.gsum = b->recs[src].gsum;                      // (if the source's is still on its way: sync_uploads copies it again)
        }
        b->gsum_pending[rec] = 0;
    }
    // gamma0 (padded speakers: 0): the rows as the caller holds them -> staging (free again: prep_kernel is ahead in the
    // stream) -> padded and converted on the device
    std::vector<R> gp;
    const size_t gbytes = (size_t)T * S * (g_dtype == VBX_F64 ? 8 : 4);
    if (gbytes <= b->xstage_bytes) {
        HIPCHK(ctx, hipMemcpyAsync(b->d_xstage, gamma0, gbytes, hipMemcpyHostToDevice, ctx->stream));
        const unsigned blocks = (unsigned)(((size_t)T * Sp + 255) / 256);
        if (g_dtype == VBX_F64)
            hipLaunchKernelGGL((vbx::pad_gamma_kernel<R, double>), dim3(blocks), dim3(256), 0, ctx->stream, (const double*)b->d_xstage,
                               (R*)b->d_gamma + rd.row0 * Sp, T, S, Sp);
        else
            hipLaunchKernelGGL((vbx::pad_gamma_kernel<R, float>), dim3(blocks), dim3(256), 0, ctx->stream, (const float*)b->d_xstage,
                               (R*)b->d_gamma + rd.row0 * Sp, T, S, Sp);
        HIPCHK(ctx, hipGetLastError());
    } else {                                                   // (more speakers than feature dims: the staging block is too small)
        if (g_dtype == VBX_F64) pack_matrix<R, double>(gp, (const double*)gamma0, T, S, Sp, (R)0);
        else pack_matrix<R, float>(gp, (const float*)gamma0, T, S, Sp, (R)0);
        HIPCHK(ctx, hipMemcpyAsync((R*)b->d_gamma + rd.row0 * Sp, gp.data(), sizeof(R) * gp.size(), hipMemcpyHostToDevice, ctx->stream));
        must_sync = true;
    }
    for (int s = 0; s < Sp; ++s) pip[s] = s < S ? pi0[s] : 0.0;
    flags[1] = 1.0;
    std::vector<R> ap, ip;
    rd.has_model = (alpha0 && invL0) ? 1 : 0;
    if (rd.has_model) {
        ap.assign((size_t)Sp * Dp, (R)0);
        ip.assign((size_t)Sp * Dp, (R)1);
        for (int s = 0; s < S; ++s)
            for (int d = 0; d < D; ++d) {
                ap[(size_t)s * Dp + d] = (R)alpha0[(size_t)s * D + d];
                ip[(size_t)s * Dp + d] = (R)invL0[(size_t)s * D + d];
            }
        HIPCHK(ctx, hipMemcpyAsync((R*)b->d_alpha + (size_t)rec * Sp * Dp, ap.data(), sizeof(R) * ap.size(), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync((R*)b->d_invL + (size_t)rec * Sp * Dp, ip.data(), sizeof(R) * ip.size(), hipMemcpyHostToDevice, ctx->stream));
        must_sync = true;
    }
    if (b->has_run) {                                         // (a fresh batch: leaf_create has zeroed the states and the flags)
        HIPCHK(ctx, hipMemsetAsync(b->d_state + rec, 0, sizeof(RecState), ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(b->d_state + b->n_rec + rec, 0, sizeof(RecState), ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(b->d_tile_done + rd.tile0, 0, sizeof(int) * rd.ntiles, ctx->stream));
    }
    b->args_busy[rec] = 1;
    b->uploads_in_flight = true;
    b->mirrors_valid = false;
    if (must_sync) return sync_uploads(b);                     // (host vectors go out of scope below)
    return VBX_OK;
}

// ---- gamma written on the device ---------------------------------------------------------------------------------------
// the host side of everything the device-side setter copies from or into: declared BEFORE its DeviceCall, which waits for the
// stream before these go
struct SlotHost {
    std::vector<double> phi, sqrt_phi, gtile, pi;
    RecState state;
    SlotHost(const vbx_batch* b, const RecDesc& rd) : phi(b->Dp, 0.0), sqrt_phi(b->Dp, 0.0), pi(b->Sp, 0.0) {
        for (int s = 0; s < rd.S; ++s) pi[s] = 1.0 / rd.S;     // (VBx.py:76: pi given as an int)
        std::memset(&state, 0, sizeof state);
    }
};

// rho, Phi and the per-tile sums of G (into h.gtile, once `call` has synchronized) of `rec` from rows already in HBM: fea [T][D] f64
template <typename R>
void rho_from_resident(DeviceCall& call, vbx_batch* b, int rec, const double* d_fea, const double* Phi, SlotHost& h) {
    const RecDesc& rd = b->recs[rec];
    for (int d = 0; d < b->D; ++d) {
        h.phi[d] = Phi[d];
        h.sqrt_phi[d] = std::sqrt(Phi[d]);
    }
    call.copy_in(b->d_phi + (size_t)rec * b->Dp, (const double*)h.phi.data(), (size_t)b->Dp);
    call.copy_in(b->d_sqrt_phi, (const double*)h.sqrt_phi.data(), (size_t)b->Dp);
    if (call.ok()) {
        LaunchScope ls(b, VBX_K_PREP);
        hipLaunchKernelGGL((prep_kernel<R, double>), dim3(rd.ntiles), dim3(256), 0, call.st, d_fea, (const double*)b->d_sqrt_phi,
                           (R*)b->d_rho + rd.row0 * b->Dp, b->d_gtile + rd.tile0, rd.T, b->D, b->Dp);
    }
    call.launched();
    h.gtile.resize(rd.ntiles);
    call.download(h.gtile.data(), (const double*)(b->d_gtile + rd.tile0), (size_t)rd.ntiles);
}

// Recording `rec` with responsibilities built on the device and pi0 = 1/S.  d_fea != nullptr: rho, Phi and sum G from these
// resident rows; d_fea == nullptr: the caller has put them in place (rho_attach / rho_clone, phi_follows_on_device).
// write_gamma(call, q) enqueues what fills q [T][Sp], the slot's rows of d_gamma.  Nothing of an upload is left pending: the
// call ends with a synchronize, and no path leaves it with a copy into or out of `h` in flight.
template <typename R, typename GammaWriter>
int set_slot_on_device(vbx_batch* b, int rec, const char* fn, const double* d_fea, const double* Phi, GammaWriter&& write_gamma) {
    RecDesc& rd = b->recs[rec];
    const int Dp = b->Dp, Sp = b->Sp;
    SlotHost h(b, rd);
    {
        DeviceCall call(b->ctx);
        if (d_fea) rho_from_resident<R>(call, b, rec, d_fea, Phi, h);
        write_gamma(call, (R*)b->d_gamma + rd.row0 * Sp);
        call.copy_in(b->d_pi + (size_t)rec * Sp, (const double*)h.pi.data(), (size_t)Sp);
        call.copy_in(b->d_state + rec, (const RecState*)&h.state, 1);
        call.copy_in(b->d_state + b->n_rec + rec, (const RecState*)&h.state, 1);
        if (call.ok()) call.enqueued(hipMemsetAsync(b->d_tile_done + rd.tile0, 0, sizeof(int) * rd.ntiles, call.st));
        call.sync();
        if (int rc = call.finish((std::string(fn) + " failed").c_str()); rc != VBX_OK) return rc;
    }
    rd.has_model = 0;
    if (d_fea) {
        double gsum = 0.0;
        for (double g : h.gtile) gsum += g;
        rd.gsum = gsum;
    }
    if (!b->gsum_pending.empty()) b->gsum_pending[rec] = 0;
    if (b->h_args) {                                          // (nothing of an earlier upload of this recording may follow)
        const size_t per = (size_t)2 * Dp + Sp + 2;
        b->h_args[(size_t)rec * per + per - 2] = b->h_args[(size_t)rec * per + per - 1] = 0.0;
    }
    b->mirrors_valid = false;
    return VBX_OK;
}

// the labels [T] in the staging block -> softmax(smoothing * onehot) rows (vbhmm.py:150-152, scipy.special.softmax:
// exp(x - max) / sum)
template <typename R>
void labels_to_gamma(DeviceCall& call, const vbx_batch* b, const RecDesc& rd, double init_smoothing, R* q) {
    const double z = std::exp(-init_smoothing), den = 1.0 + (rd.S - 1) * z;
    if (!call.ok()) return;
    hipLaunchKernelGGL((vbx::qinit_kernel<R>), dim3((unsigned)(((long long)rd.T * b->Sp + 255) / 256)), dim3(256), 0, call.st,
                       (const int*)b->d_xstage, q, (long long)rd.T, rd.S, b->Sp, 1.0 / den, z / den);
    call.launched();
}
}  // namespace
}  // extern "C++"

// ---- the six setters on one stream -------------------------------------------------------------------------------------
static int leaf_set_recording(vbx_batch* b, int rec, const void* X, int x_dtype, const double* Phi, const double* pi0,
                              const void* gamma0, int g_dtype, const double* alpha0, const double* invL0,
                              double loopProb, double Fa, double Fb) {
    if (!b) return VBX_ERR_INVALID;
    vbx_ctx* ctx = b->ctx;
    const char* fn = "vbx_batch_set_recording";
    if (int rc = check_slot_hyper(b, rec, fn, loopProb, Fa, Fb); rc != VBX_OK) return rc;
    if (!X || !Phi || !pi0 || !gamma0) FAIL(ctx, VBX_ERR_INVALID, "%s: NULL input", fn);
    if ((x_dtype != VBX_F32 && x_dtype != VBX_F64) || (g_dtype != VBX_F32 && g_dtype != VBX_F64))
        FAIL(ctx, VBX_ERR_INVALID, "bad element type");
    if (int rc = check_phi(ctx, Phi, b->D); rc != VBX_OK) return rc;
    if ((alpha0 == nullptr) != (invL0 == nullptr)) { alpha0 = nullptr; invL0 = nullptr; }   // VBx.py:94 needs both
    HIPCHK(ctx, hipSetDevice(ctx->device));
    claim_slot(b, rec, loopProb, Fa, Fb);
    int rc = with_precision(b->precision, [&](auto r) { return set_recording_impl<decltype(r)>(b, rec, X, x_dtype, Phi, pi0, gamma0, g_dtype, alpha0, invL0); });
    if (rc == VBX_OK) slot_is_set(b, rec);
    return rc;
}

// recording `rec` on the x-vectors (rho, Phi, sum G) of recording `src`: of this batch (from == nullptr: an Fa / Fb / loopProb
// sweep over one recording keeps one rho in HBM) or, as a copy, of `from`, another sub-batch of the stream group
static int leaf_set_recording_shared(vbx_batch* b, int rec, vbx_batch* from, int src, const double* pi0, const void* gamma0,
                                     int g_dtype, const double* alpha0, const double* invL0, double loopProb, double Fa, double Fb) {
    if (!b) return VBX_ERR_INVALID;
    vbx_ctx* ctx = b->ctx;
    const char* fn = "vbx_batch_set_recording_shared";
    if (int rc = check_slot_hyper(b, rec, fn, loopProb, Fa, Fb); rc != VBX_OK) return rc;
    if (int rc = check_slot_source(b, rec, from, src, fn); rc != VBX_OK) return rc;
    if (!pi0 || !gamma0) FAIL(ctx, VBX_ERR_INVALID, "%s: NULL input", fn);
    if (g_dtype != VBX_F32 && g_dtype != VBX_F64) FAIL(ctx, VBX_ERR_INVALID, "bad element type");
    if ((alpha0 == nullptr) != (invL0 == nullptr)) { alpha0 = nullptr; invL0 = nullptr; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (from)
        if (int rc = sync_source(b, from); rc != VBX_OK) return rc;
    claim_slot(b, rec, loopProb, Fa, Fb);
    int rc = from ? rho_clone(b, rec, from, src) : rho_attach(b, rec, src);
    if (rc == VBX_OK && from) rc = phi_follows_on_device(b, rec, from, src);
    if (rc == VBX_OK)
        rc = with_precision(b->precision, [&](auto r) { return set_recording_impl<decltype(r)>(b, rec, nullptr, VBX_F64, nullptr, pi0, gamma0, g_dtype, alpha0, invL0); });
    if (rc == VBX_OK) slot_is_set(b, rec);
    return rc;
}

// recording `rec` from rows already in HBM (vbx_xvectors) and the AHC labels
static int leaf_set_recording_resident(vbx_batch* b, int rec, const vbx_xvectors* xv, int64_t row0, const int32_t* labels,
                                       double init_smoothing, const double* Phi, double loopProb, double Fa, double Fb) {
    if (!b) return VBX_ERR_INVALID;
    vbx_ctx* ctx = b->ctx;
    const char* fn = "vbx_batch_set_recording_resident";
    if (int rc = check_slot_hyper(b, rec, fn, loopProb, Fa, Fb); rc != VBX_OK) return rc;
    if (!xv || !labels || !Phi) FAIL(ctx, VBX_ERR_INVALID, "%s: NULL input", fn);
    const RecDesc& rd = b->recs[rec];
    const double* d_fea = nullptr;
    if (int rc = check_resident_rows(b, rec, xv, row0, &d_fea); rc != VBX_OK) return rc;
    if (int rc = check_phi(ctx, Phi, b->D); rc != VBX_OK) return rc;
    for (long long t = 0; t < rd.T; ++t)
        if (labels[t] < 0 || labels[t] >= rd.S) FAIL(ctx, VBX_ERR_INVALID, "label %d of frame %lld outside [0, %d)", labels[t], t, rd.S);
    if (int rc = check_labels_fit_staging(b, rec); rc != VBX_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    claim_slot(b, rec, loopProb, Fa, Fb);
    int rc = with_precision(b->precision, [&](auto r) {
        using R = decltype(r);
        return set_slot_on_device<R>(b, rec, fn, d_fea, Phi, [&](DeviceCall& call, R* q) {
            // labels -> staging (the x staging block is free: fea is already on the device) -> gamma
            call.copy_in((int32_t*)b->d_xstage, labels, (size_t)rd.T);
            labels_to_gamma<R>(call, b, rd, init_smoothing, q);
        });
    });
    if (rc == VBX_OK) slot_is_set(b, rec);
    return rc;
}

// recording `rec` from random labels drawn on the device (--init random_N).  src < 0: on its own rho built
// from the resident rows of xv.  src >= 0: on the rho of recording `src` of this batch (from == nullptr: the restarts of one
// recording around one rho) or on a copy of that of recording `src` of `from`, another sub-batch of the stream group.  Written
// without the pinned argument block of the host setters, so the owner may have been set by any of the setters.
static int leaf_set_recording_random(vbx_batch* b, int rec, const vbx_xvectors* xv, int64_t row0, int src, vbx_batch* from,
                                     uint64_t seed, uint64_t name_hash, int64_t restart, double init_smoothing, const double* Phi,
                                     double loopProb, double Fa, double Fb) {
    if (!b) return VBX_ERR_INVALID;
    vbx_ctx* ctx = b->ctx;
    const char* fn = "vbx_batch_set_recording_random";
    if (int rc = check_slot_hyper(b, rec, fn, loopProb, Fa, Fb); rc != VBX_OK) return rc;
    if (restart < 0) FAIL(ctx, VBX_ERR_INVALID, "%s: restart %lld is negative", fn, (long long)restart);
    const RecDesc& rd = b->recs[rec];
    const double* d_fea = nullptr;
    if (src < 0) {
        if (!xv || !Phi) FAIL(ctx, VBX_ERR_INVALID, "%s: NULL input", fn);
        if (int rc = check_resident_rows(b, rec, xv, row0, &d_fea); rc != VBX_OK) return rc;
        if (int rc = check_phi(ctx, Phi, b->D); rc != VBX_OK) return rc;
    } else if (int rc = check_slot_source(b, rec, from, src, fn); rc != VBX_OK) {
        return rc;
    }
    if (int rc = check_labels_fit_staging(b, rec); rc != VBX_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    vbx_batch* sb = from ? from : b;
    if (src >= 0)
        if (int rc = sync_source(b, sb); rc != VBX_OK) return rc;
    claim_slot(b, rec, loopProb, Fa, Fb);
    int rc = VBX_OK;
    if (src >= 0) {
        rc = from ? rho_clone(b, rec, from, src) : rho_attach(b, rec, src);
        if (rc == VBX_OK) rc = phi_follows_on_device(b, rec, sb, from ? src : b->share_src[rec]);
    }
    if (rc == VBX_OK)
        rc = with_precision(b->precision, [&](auto r) {
            using R = decltype(r);
            return set_slot_on_device<R>(b, rec, fn, d_fea, Phi, [&](DeviceCall& call, R* q) {
                if (call.ok())
                    hipLaunchKernelGGL(vbx::random_labels_kernel, dim3((unsigned)(((rd.T + 3) / 4 + 255) / 256)), dim3(256), 0, call.st,
                                       (int*)b->d_xstage, (long long)rd.T, (unsigned long long)seed, (unsigned long long)name_hash,
                                       (unsigned long long)restart, (unsigned long long)rd.S);
                labels_to_gamma<R>(call, b, rd, init_smoothing, q);
            });
        });
    if (rc == VBX_OK) slot_is_set(b, rec);
    return rc;
}

// recording `rec` from the speaker turns of a diarization that exists (--init RTTM+VB): the
// responsibilities by turn_init_kernel where qinit_kernel writes them
static int leaf_set_recording_turns(vbx_batch* b, int rec, const vbx_xvectors* xv, int64_t row0, const int64_t* seg_a,
                                    const int64_t* seg_b, int64_t N, const int64_t* turn_u, const int64_t* turn_v,
                                    const int32_t* turn_spk, double init_smoothing, const double* Phi, double loopProb, double Fa,
                                    double Fb) {
    if (!b) return VBX_ERR_INVALID;
    vbx_ctx* ctx = b->ctx;
    const char* fn = "vbx_batch_set_recording_turns";
    if (int rc = check_slot_hyper(b, rec, fn, loopProb, Fa, Fb); rc != VBX_OK) return rc;
    if (!xv || !Phi) FAIL(ctx, VBX_ERR_INVALID, "%s: NULL input", fn);
    const RecDesc& rd = b->recs[rec];
    if (!turn_input_ok(ctx->err, fn, rd.T, seg_a, seg_b, N, turn_u, turn_v, turn_spk, rd.S)) return VBX_ERR_INVALID;
    const double* d_fea = nullptr;
    if (int rc = check_resident_rows(b, rec, xv, row0, &d_fea); rc != VBX_OK) return rc;
    if (int rc = check_phi(ctx, Phi, b->D); rc != VBX_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    claim_slot(b, rec, loopProb, Fa, Fb);
    int rc = with_precision(b->precision, [&](auto r) {
        using R = decltype(r);
        return set_slot_on_device<R>(b, rec, fn, d_fea, Phi, [&](DeviceCall& call, R* q) {
            launch_turn_init<R>(call, rd.T, seg_a, seg_b, N, turn_u, turn_v, turn_spk, rd.S, b->Sp, init_smoothing, nullptr, nullptr, q, b->Sp);
        });
    });
    if (rc == VBX_OK) slot_is_set(b, rec);
    return rc;
}

// ---- routing in a stream group ---------------------------------------------------------------------------------------
extern "C++" {
namespace {
// `rec` gets x-vectors of its own: leaf(batch, slot) sets it -- in the batch itself, or in the sub-batch it was dealt to
template <typename Leaf>
int set_own_rows(vbx_batch* b, int rec, const char* fn, Leaf&& leaf) {
    if (!b) return VBX_ERR_INVALID;
    if (b->kids.empty()) return leaf(b, rec);
    if (rec < 0 || rec >= b->n_rec) FAIL(b->ctx, VBX_ERR_INVALID, "%s: recording index %d out of range", fn, rec);
    {
        // (recordings of DIFFERENT sub-batches may be set from different host threads -- each has its own stream and arena, and
        //  a batch call uploads three times as fast that way, vbx_amd/batch.py -- so the bookkeeping they share is guarded)
        std::lock_guard<std::mutex> lock(b->group_mutex);
        b->any_set = true;
        group_new_rows(b, rec, true);
    }
    const int k = b->kid_of[rec];
    return kid_fail(b, k, leaf(b->kids[k], b->local_of[rec]));
}

// `rec` runs on the x-vectors of `src_rec`: leaf(batch, slot, from, src) sets it.  A stream group deals its recordings to
// sub-batches with a device arena each.  Sharing proper works inside one of them (from == nullptr); across two, the first
// recording of a sub-batch that asks for these x-vectors gets a COPY of the rows (device to device, from = the source's
// sub-batch) and owns it, the later ones of that sub-batch share with it: one rho per stream, not one per sweep point.
template <typename Leaf>
int group_route_source(vbx_batch* b, int rec, int src_rec, const char* fn, Leaf&& leaf) {
    if (!b) return VBX_ERR_INVALID;
    if (b->kids.empty()) return leaf(b, rec, (vbx_batch*)nullptr, src_rec);
    if (rec < 0 || rec >= b->n_rec || src_rec < 0 || src_rec >= b->n_rec || rec == src_rec)
        FAIL(b->ctx, VBX_ERR_INVALID, "%s: recording %d / source %d out of range", fn, rec, src_rec);
    const int k = b->kid_of[rec], ks = b->kid_of[src_rec];
    const int root = b->root_of[src_rec];
    if (root == rec) FAIL(b->ctx, VBX_ERR_STATE, "recording %d runs on the x-vectors of recording %d: it cannot be that recording's source", src_rec, rec);
    group_new_rows(b, rec, false);                            // (`rec` had x-vectors of its own: its dependants in other sub-batches)
    b->any_set = true;
    int local_src = ks == k ? b->local_of[src_rec] : -1;
    for (int i = 0; i < b->n_rec && local_src < 0; ++i)       // a recording of sub-batch k that already holds these x-vectors
        if (i != rec && b->kid_of[i] == k && b->root_of[i] == root && b->kids[k]->is_set[b->local_of[i]] &&
            b->kids[k]->share_src[b->local_of[i]] != b->local_of[rec])        // (not one that reads `rec`'s own copy: `rec` is
            local_src = b->local_of[i];                                       //  the clone owner being set again -> a fresh clone)
    const int rc = local_src >= 0 ? leaf(b->kids[k], b->local_of[rec], (vbx_batch*)nullptr, local_src)
                                  : leaf(b->kids[k], b->local_of[rec], b->kids[ks], b->local_of[src_rec]);
    if (rc == VBX_OK) b->root_of[rec] = root;
    return kid_fail(b, k, rc);
}
}  // namespace
}  // extern "C++"

extern "C" {

int vbx_batch_set_recording(vbx_batch* b, int rec, const void* X, int x_dtype, const double* Phi, const double* pi0,
                            const void* gamma0, int g_dtype, const double* alpha0, const double* invL0,
                            double loopProb, double Fa, double Fb) {
    return set_own_rows(b, rec, "vbx_batch_set_recording", [&](vbx_batch* leaf, int slot) {
        return leaf_set_recording(leaf, slot, X, x_dtype, Phi, pi0, gamma0, g_dtype, alpha0, invL0, loopProb, Fa, Fb);
    });
}

int vbx_batch_set_recording_shared(vbx_batch* b, int rec, int src_rec, const double* pi0, const void* gamma0, int g_dtype,
                                   const double* alpha0, const double* invL0, double loopProb, double Fa, double Fb) {
    return group_route_source(b, rec, src_rec, "vbx_batch_set_recording_shared", [&](vbx_batch* leaf, int slot, vbx_batch* from, int src) {
        return leaf_set_recording_shared(leaf, slot, from, src, pi0, gamma0, g_dtype, alpha0, invL0, loopProb, Fa, Fb);
    });
}

int vbx_batch_set_recording_resident(vbx_batch* b, int rec, const vbx_xvectors* xv, int64_t row0, const int32_t* labels,
                                     double init_smoothing, const double* Phi, double loopProb, double Fa, double Fb) {
    return set_own_rows(b, rec, "vbx_batch_set_recording_resident", [&](vbx_batch* leaf, int slot) {
        return leaf_set_recording_resident(leaf, slot, xv, row0, labels, init_smoothing, Phi, loopProb, Fa, Fb);
    });
}

int vbx_batch_set_recording_random(vbx_batch* b, int rec, const vbx_xvectors* xv, int64_t row0, int src_rec, uint64_t seed,
                                   uint64_t name_hash, int64_t restart, double init_smoothing, const double* Phi, double loopProb,
                                   double Fa, double Fb) {
    const char* fn = "vbx_batch_set_recording_random";
    if (src_rec < 0)
        return set_own_rows(b, rec, fn, [&](vbx_batch* leaf, int slot) {
            return leaf_set_recording_random(leaf, slot, xv, row0, -1, nullptr, seed, name_hash, restart, init_smoothing, Phi, loopProb, Fa, Fb);
        });
    return group_route_source(b, rec, src_rec, fn, [&](vbx_batch* leaf, int slot, vbx_batch* from, int src) {
        return leaf_set_recording_random(leaf, slot, nullptr, 0, src, from, seed, name_hash, restart, init_smoothing, nullptr, loopProb, Fa, Fb);
    });
}

int vbx_batch_set_recording_turns(vbx_batch* b, int rec, const vbx_xvectors* xv, int64_t row0, const int64_t* seg_a,
                                  const int64_t* seg_b, int64_t N, const int64_t* turn_u, const int64_t* turn_v,
                                  const int32_t* turn_spk, double init_smoothing, const double* Phi, double loopProb, double Fa,
                                  double Fb) {
    return set_own_rows(b, rec, "vbx_batch_set_recording_turns", [&](vbx_batch* leaf, int slot) {
        return leaf_set_recording_turns(leaf, slot, xv, row0, seg_a, seg_b, N, turn_u, turn_v, turn_spk, init_smoothing, Phi, loopProb, Fa, Fb);
    });
}

}  // extern "C"
