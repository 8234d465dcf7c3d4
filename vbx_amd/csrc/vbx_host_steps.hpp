// vbx_host_steps.hpp -- C ABI: step-level entry points (forward_backward, mstep, loglik) the parity tests call
// (one translation unit with vbx_capi.hip, which includes the parts in order, this one after vbx_host_call.hpp: the entry
// points without a batch behind them keep their device scratch in a DeviceCall; not a stand-alone header)
#pragma once
extern "C" {

// ---------------------------------------------------------------------------------------
// step-level entry points (parity tests)
// ---------------------------------------------------------------------------------------
extern "C++" {
namespace {
template <typename R>
int fb_step_impl(vbx_batch* b, int64_t T, int32_t S, const double* lls, double* gamma, double* tll, double* entered,
                 double* lfw, double* lbw) {
    vbx_ctx* ctx = b->ctx;
    const int Sp = b->Sp;
    std::vector<R> bm((size_t)T * Sp, (R)0), mr((size_t)T);
    for (int64_t t = 0; t < T; ++t) {
        double m = -INFINITY;
        for (int s = 0; s < S; ++s) m = std::max(m, lls[(size_t)t * S + s]);
        const R mq = (R)m;                      // the device keeps the row max in working precision
        mr[(size_t)t] = mq;
        for (int s = 0; s < S; ++s) bm[(size_t)t * Sp + s] = (R)std::exp(lls[(size_t)t * S + s] - (double)mq);
    }
    HIPCHK(ctx, hipMemcpy(b->d_bmat, bm.data(), sizeof(R) * bm.size(), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(b->d_mrow, mr.data(), sizeof(R) * mr.size(), hipMemcpyHostToDevice));
    const bool want_logs = lfw || lbw;
    if (want_logs) {
        int rc2 = dmalloc_bytes(ctx, &b->d_fw_scale, (size_t)T * sizeof(R));
        if (rc2 == VBX_OK) rc2 = dmalloc_bytes(ctx, &b->d_bw_scale, (size_t)T * sizeof(R));
        if (rc2 != VBX_OK) return rc2;
    }
    b->fuse = 0;                                  // stand-alone scan kernels: one operator per tile
    int rc = choose_fb_algo(b, want_logs);
    if (rc != VBX_OK) return rc;
    plan_iteration(b);
    rc = upload_recs(b);
    if (rc != VBX_OK) return rc;
    launch_fb<R>(b, 0.0);
    launch_post<R>(b, 0.0);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    RecState st;
    HIPCHK(ctx, hipMemcpy(&st, b->d_state + (size_t)b->state_cur * b->n_rec, sizeof st, hipMemcpyDeviceToHost));
    if (b->use_chunked) {
        std::vector<double> tp((size_t)b->ntiles_total);
        HIPCHK(ctx, hipMemcpy(tp.data(), b->d_tllpart, sizeof(double) * tp.size(), hipMemcpyDeviceToHost));
        st.tll = 0.0;
        for (double v : tp) st.tll += v;
    }
    if (tll) *tll = st.tll;
    if (gamma) {
        b->mirrors_valid = false;
        rc = leaf_get_result(b, 0, gamma, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
        if (rc != VBX_OK) return rc;
    }
    if (entered) {
        std::vector<double> ep((size_t)b->ntiles_total * Sp);
        HIPCHK(ctx, hipMemcpy(ep.data(), b->d_epart, sizeof(double) * ep.size(), hipMemcpyDeviceToHost));
        for (int s = 0; s < S; ++s) {
            double acc = 0.0;
            for (int tl = 0; tl < b->ntiles_total; ++tl) acc += ep[(size_t)tl * Sp + s];
            entered[s] = acc;
        }
    }
    if (want_logs) {
        // lfw[t] = log ahat[t] + sum_{u<=t} (log s_u + m_u);  lbw[t] = log bhat[t] + sum_{u>t} (log q_{u-1} + m_u)
        std::vector<R> ah((size_t)T * Sp), bh((size_t)T * Sp), fs((size_t)T), bs((size_t)T);
        HIPCHK(ctx, hipMemcpy(ah.data(), b->d_ahat, sizeof(R) * ah.size(), hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(bh.data(), b->d_bhat, sizeof(R) * bh.size(), hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(fs.data(), b->d_fw_scale, sizeof(R) * fs.size(), hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(bs.data(), b->d_bw_scale, sizeof(R) * bs.size(), hipMemcpyDeviceToHost));
        if (lfw) {
            double cum = 0.0;
            for (int64_t t = 0; t < T; ++t) {
                cum += std::log((double)fs[(size_t)t]) + (double)mr[(size_t)t];
                for (int s = 0; s < S; ++s) lfw[(size_t)t * S + s] = std::log((double)ah[(size_t)t * Sp + s]) + cum;
            }
        }
        if (lbw) {
            double cum = 0.0;
            for (int64_t t = T - 1; t >= 0; --t) {
                if (t < T - 1) cum += std::log((double)bs[(size_t)t]) + (double)mr[(size_t)t + 1];
                for (int s = 0; s < S; ++s) lbw[(size_t)t * S + s] = std::log((double)bh[(size_t)t * Sp + s]) + cum;
            }
        }
    }
    return VBX_OK;
}
}  // namespace
}  // extern "C++"

int vbx_forward_backward(vbx_ctx* ctx, int64_t T, int32_t S, const double* lls, const double* pi, const double* ip,
                         double loopProb, int precision, int fb_algo, double* gamma, double* tll, double* entered,
                         double* lfw, double* lbw) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!lls || !pi || T <= 0 || S <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_forward_backward: bad argument");
    if (!(loopProb >= 0.0 && loopProb <= 1.0)) FAIL(ctx, VBX_ERR_INVALID, "loopProb=%g outside [0,1]", loopProb);
    vbx_batch* b = nullptr;
    int rc = vbx_batch_create(ctx, 1, &T, &S, 32, precision, 1, &b);
    if (rc != VBX_OK) return rc;
    rc = vbx_batch_set_option(b, VBX_OPT_FB_ALGO, fb_algo);
    if (rc == VBX_OK) {
        RecDesc& rd = b->recs[0];
        rd.lp = loopProb;
        rd.Fa = rd.Fb = 1.0;
        std::vector<double> pip(b->Sp, 0.0), ipp(b->Sp, 0.0);
        for (int s = 0; s < S; ++s) {
            pip[s] = pi[s];
            ipp[s] = ip ? ip[s] : pi[s];
        }
        rc = dmalloc(ctx, &b->d_ip, (size_t)b->Sp);
        hipError_t e = hipSuccess;
        if (rc == VBX_OK) e = hipMemcpy(b->d_pi, pip.data(), sizeof(double) * b->Sp, hipMemcpyHostToDevice);
        if (rc == VBX_OK && e == hipSuccess) e = hipMemcpy(b->d_ip, ipp.data(), sizeof(double) * b->Sp, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            ctx->err = std::string("pi upload failed: ") + hipGetErrorString(e);
            rc = VBX_ERR_HIP;
        }
        b->recs_dirty = true;
    }
    if (rc == VBX_OK)
        rc = with_precision(precision, [&](auto r) { return fb_step_impl<decltype(r)>(b, T, S, lls, gamma, tll, entered, lfw, lbw); });
    vbx_batch_destroy(b);
    return rc;
}

extern "C++" {
namespace {
template <typename R>
int fb_dense_impl(vbx_ctx* ctx, int64_t T, int32_t S, const double* lls, const double* tr, const double* ip, double* gamma,
                  double* tll, double* lfw, double* lbw) {
    int Sp = 16;
    while (Sp < S && Sp < 256) Sp *= 2;
    if (S > 256) Sp = round_up(S, 64);                               // fb_dense_big_kernel: M in HBM, any S
    const size_t cells = (size_t)T * Sp;
    std::vector<R> bm(cells, (R)0), m0((size_t)Sp * Sp, (R)0), m1((size_t)Sp * Sp, (R)0), v0(Sp, (R)0);
    std::vector<double> mr((size_t)T);
    for (int64_t t = 0; t < T; ++t) {
        double m = -INFINITY;
        for (int s = 0; s < S; ++s) m = std::max(m, lls[(size_t)t * S + s]);
        mr[(size_t)t] = m;
        for (int s = 0; s < S; ++s) bm[(size_t)t * Sp + s] = (R)std::exp(lls[(size_t)t * S + s] - m);
    }
    for (int i = 0; i < S; ++i) {
        v0[i] = (R)(ip[i] + 1e-8);                                   // VBx.py:163
        for (int j = 0; j < S; ++j) {
            const R a = (R)(tr[(size_t)i * S + j] + 1e-8);           // VBx.py:158
            m0[(size_t)i * Sp + j] = a;                              // forward: M[k][o] = A[k][o]
            m1[(size_t)j * Sp + i] = a;                              // backward: M[k][o] = A[o][k]
        }
    }
    std::vector<R> ah(cells), bh(cells), fs((size_t)T), bs((size_t)T);
    DeviceCall call(ctx);
    hipStream_t st = call.st;
    const R* d_m0 = call.upload(m0.data(), m0.size());
    const R* d_m1 = call.upload(m1.data(), m1.size());
    const R* d_b = call.upload(bm.data(), cells);
    const R* d_v0 = call.upload(v0.data(), (size_t)Sp);
    R* d_ah = call.alloc<R>(cells);
    R* d_bh = call.alloc<R>(cells);
    R* d_fs = call.alloc<R>((size_t)T);
    R* d_bs = call.alloc<R>((size_t)T);
    if (call.ok()) {
#define VBX_FB_DENSE(SP_) hipLaunchKernelGGL((fb_dense_kernel<R, SP_>), dim3(2), dim3(FbDenseCfg<SP_>::kThreads), 0, st, \
                                             d_m0, d_m1, d_b, d_v0, d_ah, d_bh, d_fs, d_bs, (int)T, (int)S)
        switch (Sp) {
            case 16: VBX_FB_DENSE(16); break;
            case 32: VBX_FB_DENSE(32); break;
            case 64: VBX_FB_DENSE(64); break;
            case 128: VBX_FB_DENSE(128); break;
            case 256: VBX_FB_DENSE(256); break;
            default:      // more than 256 states (the register-resident kernel would drop them: round-3 advisor finding)
                hipLaunchKernelGGL((fb_dense_big_kernel<R>), dim3(2), dim3(1024), 0, st, d_m0, d_m1, d_b, d_v0, d_ah, d_bh,
                                   d_fs, d_bs, (int)T, (int)S, Sp);
                break;
        }
#undef VBX_FB_DENSE
        call.launched();
    }
    call.download(ah.data(), d_ah, cells);
    call.download(bh.data(), d_bh, cells);
    call.download(fs.data(), d_fs, (size_t)T);
    call.download(bs.data(), d_bs, (size_t)T);
    call.sync();
    if (int rc = call.finish("forward_backward (dense)")) return rc;
    // lfw[t] = log ahat[t] + sum_{u<=t} (log s_u + m_u);  lbw[t] = log bhat[t] + sum_{u>=t, u<T-1} log q_u + sum_{u>t} m_u
    double cum = 0.0;
    for (int64_t t = 0; t < T; ++t) {
        cum += std::log((double)fs[(size_t)t]) + mr[(size_t)t];
        if (lfw)
            for (int s = 0; s < S; ++s) lfw[(size_t)t * S + s] = std::log((double)ah[(size_t)t * Sp + s]) + cum;
    }
    if (tll) *tll = cum;
    if (lbw) {
        double back = 0.0;
        for (int64_t t = T - 1; t >= 0; --t) {
            if (t < T - 1) back += std::log((double)bs[(size_t)t]) + mr[(size_t)t + 1];
            for (int s = 0; s < S; ++s) lbw[(size_t)t * S + s] = std::log((double)bh[(size_t)t * Sp + s]) + back;
        }
    }
    if (gamma)
        for (int64_t t = 0; t < T; ++t) {
            double tot = 0.0;
            for (int s = 0; s < S; ++s) tot += (double)ah[(size_t)t * Sp + s] * (double)bh[(size_t)t * Sp + s];
            for (int s = 0; s < S; ++s)
                gamma[(size_t)t * S + s] = (double)ah[(size_t)t * Sp + s] * (double)bh[(size_t)t * Sp + s] / tot;
        }
    return VBX_OK;
}
}  // namespace
}  // extern "C++"

int vbx_forward_backward_dense(vbx_ctx* ctx, int64_t T, int32_t S, const double* lls, const double* tr, const double* ip,
                               int precision, double* gamma, double* tll, double* lfw, double* lbw) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!lls || !tr || !ip || T <= 0 || S <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_forward_backward_dense: bad argument");
    if (S > vbx::kFbDenseBigMax) FAIL(ctx, VBX_ERR_UNSUPPORTED, "forward_backward (dense): S=%d exceeds %d states", S, vbx::kFbDenseBigMax);
    if (precision != VBX_PREC_FP32 && precision != VBX_PREC_FP64) FAIL(ctx, VBX_ERR_INVALID, "unknown precision %d", precision);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return with_precision(precision, [&](auto r) { return fb_dense_impl<decltype(r)>(ctx, T, S, lls, tr, ip, gamma, tll, lfw, lbw); });
}

int vbx_mstep(vbx_ctx* ctx, int64_t T, int32_t S, int32_t D, const double* X, const double* Phi, const double* gamma,
              double Fa, double Fb, int precision, double* alpha, double* invL) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!X || !Phi || !gamma) FAIL(ctx, VBX_ERR_INVALID, "vbx_mstep: NULL input");
    vbx_batch* b = nullptr;
    int rc = vbx_batch_create(ctx, 1, &T, &S, D, precision, 1, &b);
    if (rc != VBX_OK) return rc;
    std::vector<double> pi(S, 1.0 / S);
    rc = vbx_batch_set_recording(b, 0, X, VBX_F64, Phi, pi.data(), gamma, VBX_F64, nullptr, nullptr, 0.9, Fa, Fb);
    if (rc == VBX_OK) rc = upload_recs(b);
    if (rc == VBX_OK) {
        plan_iteration(b);
        with_precision(precision, [&](auto r) { launch_mstep<decltype(r)>(b, 0.0); });
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) {
            ctx->err = std::string("mstep kernels failed: ") + hipGetErrorString(e);
            rc = VBX_ERR_HIP;
        }
    }
    if (rc == VBX_OK) rc = vbx_batch_get_result(b, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, alpha, invL);
    vbx_batch_destroy(b);
    return rc;
}

int vbx_loglik(vbx_ctx* ctx, int64_t T, int32_t S, int32_t D, const double* X, const double* Phi, const double* alpha,
               const double* invL, double Fa, int precision, double* log_p) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!X || !Phi || !alpha || !invL || !log_p) FAIL(ctx, VBX_ERR_INVALID, "vbx_loglik: NULL input");
    vbx_batch* b = nullptr;
    int rc = vbx_batch_create(ctx, 1, &T, &S, D, precision, 1, &b);
    if (rc != VBX_OK) return rc;
    std::vector<double> pi(S, 1.0 / S), g0((size_t)T * S, 1.0 / S);
    rc = vbx_batch_set_recording(b, 0, X, VBX_F64, Phi, pi.data(), g0.data(), VBX_F64, alpha, invL, 0.9, Fa, 1.0);
    if (rc == VBX_OK) rc = upload_recs(b);
    const size_t cells = (size_t)T * b->Sp;
    if (rc == VBX_OK) rc = dmalloc_bytes(ctx, &b->d_lraw, cells * b->rsize);
    if (rc == VBX_OK) {
        plan_iteration(b);
        with_precision(precision, [&](auto r) {
            launch_fin<decltype(r)>(b, 0.0, 1);
            launch_loglik<decltype(r)>(b, 0.0, true);
        });
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) {
            ctx->err = std::string("loglik kernels failed: ") + hipGetErrorString(e);
            rc = VBX_ERR_HIP;
        }
    }
    if (rc == VBX_OK) {
        // add the per-frame constant Fa*G_t of VBx.py:87,97 on the host (f64)
        rc = with_precision(precision, [&](auto r) -> int {
            using R = decltype(r);
            std::vector<R> raw(cells);
            HIPCHK(ctx, hipMemcpy(raw.data(), b->d_lraw, sizeof(R) * cells, hipMemcpyDeviceToHost));
            for (int64_t t = 0; t < T; ++t) {
                double ss = 0.0;
                for (int d = 0; d < D; ++d) ss += X[(size_t)t * D + d] * X[(size_t)t * D + d];
                const double G = -0.5 * (ss + D * std::log(2.0 * M_PI));
                for (int s = 0; s < S; ++s) log_p[(size_t)t * S + s] = (double)raw[(size_t)t * b->Sp + s] + Fa * G;
            }
            return VBX_OK;
        });
    }
    vbx_batch_destroy(b);
    return rc;
}

extern "C++" {
namespace {
template <typename R>
int score_posteriors_impl(vbx_ctx* ctx, int64_t T, int32_t S, const double* gamma, const int32_t* ref, int32_t n_ref, double* conf) {
    int Sp = 16;
    while (Sp < S) Sp *= 2;
    RecDesc rd;
    std::memset(&rd, 0, sizeof rd);
    rd.T = (int)T;
    rd.S = S;
    rd.ntiles = (rd.T + kTileFrames - 1) / kTileFrames;
    const ScoreRec sr{0, 0, n_ref, (rd.ntiles + kScoreGroupTiles - 1) / kScoreGroupTiles};
    std::vector<int2> items;
    for (int g = 0; g < sr.ngroups; ++g) items.push_back(make_int2(0, g));
    std::vector<R> gp;
    pack_matrix<R, double>(gp, gamma, T, S, Sp, (R)0);        // (fp32: rounded here, as a batch holds it)
    const size_t block = (size_t)2 * n_ref * Sp;
    std::vector<double> padded(block);
    DeviceCall call(ctx);
    R* d_gamma = call.upload(gp.data(), gp.size());
    RecDesc* d_rd = call.upload(&rd, (size_t)1);
    ScoreRec* d_sr = call.upload(&sr, (size_t)1);
    int* d_lab = call.upload(ref, (size_t)T);
    int2* d_items = call.upload(items.data(), items.size());
    double* d_part = call.alloc<double>(block * sr.ngroups);
    double* d_hist = call.alloc<double>(block);
    if (call.ok()) {
        score_launch<R>(call.st, d_gamma, Sp, 1, 1, d_rd, d_sr, d_lab, d_items, (int)items.size(), n_ref, nullptr, 0, d_part, d_hist);
        call.launched();
    }
    call.download(padded.data(), d_hist, block);
    call.sync();
    if (int rc = call.finish("score kernels failed")) return rc;
    for (size_t r = 0; r < (size_t)2 * n_ref; ++r) std::memcpy(conf + r * S, padded.data() + r * Sp, sizeof(double) * S);
    return VBX_OK;
}
}  // namespace
}  // extern "C++"

int vbx_score_posteriors(vbx_ctx* ctx, int64_t T, int32_t S, const double* gamma, const int32_t* ref, int32_t n_ref, int precision,
                         double* conf) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!gamma || !ref || !conf) FAIL(ctx, VBX_ERR_INVALID, "vbx_score_posteriors: NULL argument");
    if (T <= 0 || T > 0x7fffffffLL / 512 || S <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_score_posteriors: T=%lld, S=%d out of range", (long long)T, S);
    if (S > VBX_MAX_SPEAKERS) FAIL(ctx, VBX_ERR_UNSUPPORTED, "S=%d exceeds VBX_MAX_SPEAKERS=%d", S, VBX_MAX_SPEAKERS);
    if (n_ref < 1 || n_ref > kScoreMaxRef) FAIL(ctx, VBX_ERR_INVALID, "vbx_score_posteriors: n_ref=%d outside [1, %d]", n_ref, kScoreMaxRef);
    if (precision != VBX_PREC_FP32 && precision != VBX_PREC_FP64) FAIL(ctx, VBX_ERR_INVALID, "unknown precision %d", precision);
    for (int64_t t = 0; t < T; ++t)
        if (ref[t] < 0 || ref[t] >= n_ref) FAIL(ctx, VBX_ERR_INVALID, "vbx_score_posteriors: label %d of frame %lld outside [0, %d)", ref[t], (long long)t, n_ref);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return with_precision(precision, [&](auto r) { return score_posteriors_impl<decltype(r)>(ctx, T, S, gamma, ref, n_ref, conf); });
}

// The launch plan of the last run, for the tests that must know which instance they ran (tests/test_gpu_onestep.py): a getter
// beside vbx_batch_gemm_in_effect / vbx_batch_stream_loads_in_effect, kept in this part -- the entry points of the parity tests
// -- so that the sources an iteration is built from (vbx_amd/build.py: ITERATION_SOURCES) stay what the profiles were taken on.
int vbx_batch_plan(const vbx_batch* b, int* out, int n) {
    if (!b || (n > 0 && !out)) return VBX_ERR_INVALID;
    const vbx_batch* l = b->kids.empty() ? b : b->kids[0];     // (a batch on several streams: its first sub-batch)
    const IterPlan& p = l->plan;
    const int f[VBX_PLAN_FIELDS] = {p.fused_post, p.fused_loglik, p.half_ops, p.split, p.stream, p.small, p.lat, p.fold,
                                    p.walk_levels, p.fin_threads, l->Sp, l->use_chunked, l->sgroup, l->sgroup2};
    for (int i = 0; i < std::min(n, (int)VBX_PLAN_FIELDS); ++i) out[i] = f[i];
    return VBX_PLAN_FIELDS;
}

}  // extern "C"
