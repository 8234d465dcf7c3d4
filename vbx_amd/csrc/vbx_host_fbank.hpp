// vbx_host_fbank.hpp -- host runtime of the filterbank front end (vbx_fbank.hpp): the folded frame operator, the segment and
// tile tables, the launch sequence of one call and the copies out.  Included by vbx_capi.hip after vbx_host_launch.hpp.

struct vbx_fbank {
    vbx_ctx* ctx = nullptr;
    int L = 0, shift = 0, nfft = 0, KP = 0, pre = 0, post_cap = 0;
    double *d_MT = nullptr, *d_melT = nullptr;
    int2* d_melr = nullptr;
    // per call, grown on demand
    double *d_sig = nullptr, *d_logmel = nullptr;
    float* d_fea = nullptr;
    FbSeg* d_segs = nullptr;
    FbTile* d_tiles = nullptr;                                 // 64-frame blocks: the frame kernel's tiles and the CMN kernel's blocks
    long long* d_starts = nullptr;
    size_t cap_sig = 0, cap_logmel = 0, cap_fea = 0, cap_segs = 0, cap_tiles = 0, cap_starts = 0;
    long long rows = 0;                                        // feature rows of the last run
    hipEvent_t ev[6] = {};                                     // upload | frame | cmn of a run; gather of a windows call
};

template <typename T> static int fb_reserve(vbx_ctx* ctx, T** p, size_t* cap, size_t count) {
    if (*cap >= count && *p) return VBX_OK;
    ctx_free(ctx, *p);
    *p = nullptr;
    *cap = 0;
    const int rc = dmalloc_bytes(ctx, (void**)p, std::max<size_t>(count, 1) * sizeof(T));
    if (rc == VBX_OK) *cap = count;
    return rc;
}

extern "C" {

int vbx_fbank_destroy(vbx_fbank* fb) {
    if (!fb) return VBX_OK;
    vbx_ctx* ctx = fb->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (void* p : {(void*)fb->d_MT, (void*)fb->d_melT, (void*)fb->d_melr, (void*)fb->d_sig, (void*)fb->d_logmel, (void*)fb->d_fea,
                    (void*)fb->d_segs, (void*)fb->d_tiles, (void*)fb->d_starts})
        ctx_free(ctx, p);
    for (auto& e : fb->ev)
        if (e) (void)hipEventDestroy(e);
    delete fb;
    return VBX_OK;
}

int vbx_fbank_create(vbx_ctx* ctx, int32_t winlen, int32_t shift, int32_t nfft, int32_t n_mel, const double* window,
                     const double* mel, double preemph, vbx_fbank** out) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!out || !window || !mel) FAIL(ctx, VBX_ERR_INVALID, "vbx_fbank_create: bad argument");
    *out = nullptr;
    if (n_mel != FB_MEL || !((winlen == 400 && shift == 160 && nfft == 512) || (winlen == 200 && shift == 80 && nfft == 256)))
        FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_fbank_create: geometry (winlen %d, shift %d, nfft %d, %d channels) not built; "
             "supported: 400/160/512 (16 kHz) and 200/80/256 (8 kHz), 64 channels", winlen, shift, nfft, n_mel);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int L = winlen, K = nfft / 2 + 1, KP = round_up(K, 16);
    // M = [cos; -sin] diag(w) P Z: Z removes the frame mean, P is the pre-emphasis y[l] = z[l] - a z[max(l - 1, 0)]
    // (features.py:25, its first sample uses itself), w the window; row k of the DFT part at 2 pi k l / nfft with the
    // product k l reduced mod nfft first, so that every angle is exact
    std::vector<double> WP((size_t)L * L, 0.0);                // (diag(w) P)[l][j]
    for (int l = 0; l < L; ++l) {
        WP[(size_t)l * L + l] += window[l];
        WP[(size_t)l * L + std::max(l - 1, 0)] -= preemph * window[l];
    }
    std::vector<double> WPZ((size_t)L * L);                    // (diag(w) P Z)[l][j] = WP[l][j] - mean_j WP[l][j]
    for (int l = 0; l < L; ++l) {
        double rs = 0.0;
        for (int j = 0; j < L; ++j) rs += WP[(size_t)l * L + j];
        for (int j = 0; j < L; ++j) WPZ[(size_t)l * L + j] = WP[(size_t)l * L + j] - rs / L;
    }
    std::vector<double> cs(nfft), sn(nfft);
    for (int q = 0; q < nfft; ++q) {
        cs[q] = std::cos(2.0 * M_PI * q / nfft);
        sn[q] = std::sin(2.0 * M_PI * q / nfft);
    }
    std::vector<double> MT((size_t)L * 2 * KP, 0.0);          // MT[j][32 t + c] = re of bin 16 t + c, [j][32 t + 16 + c] = im
    for (int k = 0; k < K; ++k) {
        const size_t col = (size_t)32 * (k / 16) + (k % 16);
        for (int j = 0; j < L; ++j) {
            double re = 0.0, im = 0.0;
            for (int l = 0; l < L; ++l) {
                const int q = (int)(((long long)k * l) % nfft);
                re += cs[q] * WPZ[(size_t)l * L + j];
                im -= sn[q] * WPZ[(size_t)l * L + j];
            }
            MT[(size_t)j * 2 * KP + col] = re;
            MT[(size_t)j * 2 * KP + col + 16] = im;
        }
    }
    std::vector<double> melT((size_t)FB_MEL * KP, 0.0);
    std::vector<int2> melr(FB_MEL);
    for (int m = 0; m < FB_MEL; ++m) {
        int lo = K, hi = 0;
        for (int k = 0; k < K; ++k) {
            const double v = mel[(size_t)k * FB_MEL + m];
            melT[(size_t)m * KP + k] = v;
            if (v != 0.0) {
                lo = std::min(lo, k);
                hi = k + 1;
            }
        }
        melr[m] = make_int2(lo < hi ? lo : 0, hi);
    }
    vbx_fbank* fb = new vbx_fbank();
    fb->ctx = ctx;
    fb->L = L;
    fb->shift = shift;
    fb->nfft = nfft;
    fb->KP = KP;
    fb->pre = (winlen - shift) / 2;                            // predict.py:173: noverlap // 2 leading mirrored samples
    fb->post_cap = winlen / 2;                                 // predict.py:174: at most winlen // 2 trailing ones
    int rc = dmalloc(ctx, &fb->d_MT, MT.size());
    if (rc == VBX_OK) rc = dmalloc(ctx, &fb->d_melT, melT.size());
    if (rc == VBX_OK) rc = dmalloc_bytes(ctx, (void**)&fb->d_melr, sizeof(int2) * FB_MEL);
    hipError_t e = hipSuccess;
    if (rc == VBX_OK) {
        e = hipMemcpy(fb->d_MT, MT.data(), sizeof(double) * MT.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(fb->d_melT, melT.data(), sizeof(double) * melT.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(fb->d_melr, melr.data(), sizeof(int2) * FB_MEL, hipMemcpyHostToDevice);
        for (auto& ev : fb->ev)
            if (e == hipSuccess) e = hipEventCreate(&ev);
        if (e != hipSuccess) {
            ctx->err = std::string("vbx_fbank_create: ") + hipGetErrorString(e);
            rc = VBX_ERR_HIP;
        }
    }
    if (rc != VBX_OK) {
        vbx_fbank_destroy(fb);
        return rc;
    }
    *out = fb;
    return VBX_OK;
}

int vbx_fbank_run(vbx_fbank* fb, int64_t n_samples, const double* signal, int32_t n_seg, const int64_t* seg, int32_t cmn_lc,
                  int32_t cmn_rc, int64_t* n_frames) {
    if (!fb) return VBX_ERR_INVALID;
    vbx_ctx* ctx = fb->ctx;
    if (!signal || !seg || n_samples <= 0 || n_seg <= 0 || cmn_lc < 0 || cmn_rc < 0)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_fbank_run: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<FbSeg> segs(n_seg);
    std::vector<FbTile> tiles;
    long long rows = 0;
    for (int s = 0; s < n_seg; ++s) {
        const long long a = seg[2 * s], n = seg[2 * s + 1];
        // a segment needs one full frame and its leading mirror: predict.py only passes segments of more than 0.01 s
        if (a < 0 || n <= fb->pre || n > (1LL << 30) || a + n > n_samples)
            FAIL(ctx, VBX_ERR_INVALID, "vbx_fbank_run: segment %d (start %lld, %lld samples) outside the signal or shorter "
                 "than %d samples", s, a, n, fb->pre + 1);
        const long long padlen = fb->pre + n + std::min<long long>(fb->post_cap, n);
        if (padlen < fb->L) FAIL(ctx, VBX_ERR_INVALID, "vbx_fbank_run: segment %d is shorter than one frame", s);
        const int nf = (int)((padlen - fb->L) / fb->shift + 1);
        segs[s] = FbSeg{a, rows, (int)n, nf};
        for (int f0 = 0; f0 < nf; f0 += FB_TILE) tiles.push_back(FbTile{s, f0});
        rows += nf;
    }
    int rc = fb_reserve(ctx, &fb->d_sig, &fb->cap_sig, (size_t)n_samples);
    if (rc == VBX_OK) rc = fb_reserve(ctx, &fb->d_segs, &fb->cap_segs, segs.size());
    if (rc == VBX_OK) rc = fb_reserve(ctx, &fb->d_tiles, &fb->cap_tiles, tiles.size());
    if (rc == VBX_OK) rc = fb_reserve(ctx, &fb->d_logmel, &fb->cap_logmel, (size_t)rows * FB_MEL);
    if (rc == VBX_OK) rc = fb_reserve(ctx, &fb->d_fea, &fb->cap_fea, (size_t)rows * FB_MEL);
    if (rc != VBX_OK) return rc;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipEventRecord(fb->ev[0], st));
    HIPCHK(ctx, hipMemcpyAsync(fb->d_sig, signal, sizeof(double) * (size_t)n_samples, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(fb->d_segs, segs.data(), sizeof(FbSeg) * segs.size(), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(fb->d_tiles, tiles.data(), sizeof(FbTile) * tiles.size(), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipEventRecord(fb->ev[1], st));
    if (fb->L == 400)
        hipLaunchKernelGGL((fbank_frame_kernel<400, 160, 272>), dim3((unsigned)tiles.size()), dim3(256), 0, st, fb->d_sig,
                           fb->d_segs, fb->d_tiles, fb->d_MT, fb->d_melT, fb->d_melr, fb->d_logmel, fb->pre, fb->post_cap);
    else
        hipLaunchKernelGGL((fbank_frame_kernel<200, 80, 144>), dim3((unsigned)tiles.size()), dim3(256), 0, st, fb->d_sig,
                           fb->d_segs, fb->d_tiles, fb->d_MT, fb->d_melT, fb->d_melr, fb->d_logmel, fb->pre, fb->post_cap);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(fb->ev[2], st));
    hipLaunchKernelGGL(fbank_cmn_kernel, dim3((unsigned)tiles.size()), dim3(256), 0, st, fb->d_logmel, fb->d_segs,
                       fb->d_tiles, fb->d_fea, cmn_lc, cmn_rc);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(fb->ev[3], st));
    fb->rows = rows;
    if (n_frames) *n_frames = rows;
    // the host arrays above go out of scope: the copies from them must have landed
    HIPCHK(ctx, hipStreamSynchronize(st));
    return VBX_OK;
}

int vbx_fbank_get(vbx_fbank* fb, int which, int64_t row0, int64_t nrows, void* dst, int dst_on_device) {
    if (!fb) return VBX_ERR_INVALID;
    vbx_ctx* ctx = fb->ctx;
    if (!dst || row0 < 0 || nrows < 0 || row0 + nrows > fb->rows || (which != 0 && which != 1))
        FAIL(ctx, VBX_ERR_INVALID, "vbx_fbank_get: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t esz = which == 0 ? sizeof(float) : sizeof(double);
    const char* src = which == 0 ? (const char*)fb->d_fea : (const char*)fb->d_logmel;
    HIPCHK(ctx, hipMemcpyAsync(dst, src + (size_t)row0 * FB_MEL * esz, (size_t)nrows * FB_MEL * esz,
                               dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return VBX_OK;
}

int vbx_fbank_windows(vbx_fbank* fb, int32_t n, const int64_t* starts, int32_t len, float* dst, int dst_on_device) {
    if (!fb) return VBX_ERR_INVALID;
    vbx_ctx* ctx = fb->ctx;
    if (!starts || !dst || n <= 0 || len <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_fbank_windows: bad argument");
    for (int w = 0; w < n; ++w)
        if (starts[w] < 0 || starts[w] + len > fb->rows)
            FAIL(ctx, VBX_ERR_INVALID, "vbx_fbank_windows: window %d (rows %lld + %d) past the %lld feature rows", w,
                 (long long)starts[w], len, fb->rows);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = fb_reserve(ctx, &fb->d_starts, &fb->cap_starts, (size_t)n);
    if (rc != VBX_OK) return rc;
    const size_t bytes = sizeof(float) * (size_t)n * FB_MEL * len;
    float* out = dst;
    void* tmp = nullptr;
    if (!dst_on_device) {
        rc = dmalloc_bytes(ctx, &tmp, bytes);
        if (rc != VBX_OK) return rc;
        out = (float*)tmp;
    }
    hipError_t e = hipMemcpyAsync(fb->d_starts, starts, sizeof(long long) * n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(fb->ev[4], st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(fbank_gather_kernel, dim3((unsigned)n), dim3(256), 0, st, fb->d_fea, fb->d_starts, len, out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(fb->ev[5], st);
    if (e == hipSuccess && tmp) e = hipMemcpyAsync(dst, tmp, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    ctx_free(ctx, tmp);
    if (e != hipSuccess) FAIL(ctx, VBX_ERR_HIP, "vbx_fbank_windows: %s", hipGetErrorString(e));
    return VBX_OK;
}

int vbx_fbank_windows_ragged(vbx_fbank* fb, int32_t n, const int64_t* starts, const int32_t* lens, float* dst, int dst_on_device) {
    if (!fb) return VBX_ERR_INVALID;
    vbx_ctx* ctx = fb->ctx;
    if (!starts || !lens || !dst) FAIL(ctx, VBX_ERR_INVALID, "vbx_fbank_windows_ragged: starts, lens and dst must not be NULL");
    if (n <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_fbank_windows_ragged: n = %d windows, need at least one", n);
    std::vector<long long> tab(3 * (size_t)n);                 // the first rows | the frames before each window | the lengths
    long long frames = 0;
    for (int w = 0; w < n; ++w) {
        if (lens[w] <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_fbank_windows_ragged: window %d has lens = %d, need at least 1", w, lens[w]);
        if (starts[w] < 0 || starts[w] + lens[w] > fb->rows)
            FAIL(ctx, VBX_ERR_INVALID, "vbx_fbank_windows_ragged: window %d (rows %lld + %d) past the %lld feature rows", w,
                 (long long)starts[w], lens[w], fb->rows);
        tab[w] = starts[w];
        tab[(size_t)n + w] = frames;
        tab[2 * (size_t)n + w] = lens[w];
        frames += lens[w];
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipStreamSynchronize(st));                     // (a smaller table may still be read by queued work)
    int rc = fb_reserve(ctx, &fb->d_starts, &fb->cap_starts, tab.size());
    if (rc != VBX_OK) return rc;
    const size_t bytes = sizeof(float) * (size_t)frames * FB_MEL;
    float* out = dst;
    void* tmp = nullptr;
    if (!dst_on_device) {
        rc = dmalloc_bytes(ctx, &tmp, bytes);
        if (rc != VBX_OK) return rc;
        out = (float*)tmp;
    }
    hipError_t e = hipMemcpyAsync(fb->d_starts, tab.data(), sizeof(long long) * tab.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(fb->ev[4], st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(fbank_gather_ragged_kernel, dim3((unsigned)n), dim3(256), 0, st, fb->d_fea, fb->d_starts, n, out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(fb->ev[5], st);
    if (e == hipSuccess && tmp) e = hipMemcpyAsync(dst, tmp, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);         // (tab is pageable: its copy has left the host by now)
    ctx_free(ctx, tmp);
    if (e != hipSuccess) FAIL(ctx, VBX_ERR_HIP, "vbx_fbank_windows_ragged: %s", hipGetErrorString(e));
    return VBX_OK;
}

int vbx_fbank_times(vbx_fbank* fb, float* ms) {
    if (!fb || !ms) return VBX_ERR_INVALID;
    vbx_ctx* ctx = fb->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipEventElapsedTime(&ms[0], fb->ev[0], fb->ev[1]));
    HIPCHK(ctx, hipEventElapsedTime(&ms[1], fb->ev[1], fb->ev[2]));
    HIPCHK(ctx, hipEventElapsedTime(&ms[2], fb->ev[2], fb->ev[3]));
    if (hipEventElapsedTime(&ms[3], fb->ev[4], fb->ev[5]) != hipSuccess) ms[3] = 0.0f;   // (no windows call yet)
    return VBX_OK;
}

}  // extern "C"
