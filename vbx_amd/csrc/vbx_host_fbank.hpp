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
    // a raw run (vbx_fbank_run_raw): the int16 samples, the recording table and the generator states
    short* d_raw = nullptr;
    FbRec* d_recs = nullptr;
    unsigned* d_mt = nullptr;
    size_t cap_sig = 0, cap_logmel = 0, cap_fea = 0, cap_segs = 0, cap_tiles = 0, cap_starts = 0, cap_raw = 0, cap_recs = 0,
           cap_mt = 0;
    long long rows = 0;                                        // feature rows of the last run
    long long n_sig = 0;                                       // samples of the last run
    bool raw = false;                                          // the last run was a raw one
    hipEvent_t ev[6] = {};                                     // upload | frame | cmn of a run; gather of a windows call
    hipEvent_t evd[2] = {};                                    // the dither kernel of a raw run
};

// the recordings of a raw run: samples, their table [n_rec][2] = (first sample, samples), a seed and a level each
struct FbRaw {
    const int16_t* samples;
    int n_rec;
    const int64_t* rec;
    const uint32_t* seeds;
    const double* levels;
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
                    (void*)fb->d_segs, (void*)fb->d_tiles, (void*)fb->d_starts, (void*)fb->d_raw, (void*)fb->d_recs, (void*)fb->d_mt})
        ctx_free(ctx, p);
    for (auto& e : fb->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : fb->evd)
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
        for (auto& ev : fb->evd)
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

// one run: the signal comes up as f64 (signal), or as int16 samples that the dither kernel turns into it (raw); the tables
// and the frame and CMN launches are the same
static int fb_run(vbx_fbank* fb, const char* fn, int64_t n_samples, const double* signal, const FbRaw* raw, int32_t n_seg,
                  const int64_t* seg, int32_t cmn_lc, int32_t cmn_rc, int64_t* n_frames) {
    vbx_ctx* ctx = fb->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<FbSeg> segs(n_seg);
    std::vector<FbTile> tiles;
    long long rows = 0;
    for (int s = 0; s < n_seg; ++s) {
        const long long a = seg[2 * s], n = seg[2 * s + 1];
        // a segment needs one full frame and its leading mirror: predict.py only passes segments of more than 0.01 s
        if (a < 0 || n <= fb->pre || n > (1LL << 30) || a + n > n_samples)
            FAIL(ctx, VBX_ERR_INVALID, "%s: segment %d (start %lld, %lld samples) outside the signal or shorter "
                 "than %d samples", fn, s, a, n, fb->pre + 1);
        const long long padlen = fb->pre + n + std::min<long long>(fb->post_cap, n);
        if (padlen < fb->L) FAIL(ctx, VBX_ERR_INVALID, "%s: segment %d is shorter than one frame", fn, s);
        const int nf = (int)((padlen - fb->L) / fb->shift + 1);
        segs[s] = FbSeg{a, rows, (int)n, nf};
        for (int f0 = 0; f0 < nf; f0 += FB_TILE) tiles.push_back(FbTile{s, f0});
        rows += nf;
    }
    // a raw run: the recordings lie inside the samples and apart from each other, and each gets init_genrand(seed):
    // mt[0] = seed, mt[i] = 1812433253 (mt[i - 1] ^ (mt[i - 1] >> 30)) + i
    std::vector<FbRec> recs;
    std::vector<uint32_t> states;
    long long covered = 0;
    if (raw) {
        recs.resize(raw->n_rec);
        std::vector<int> order(raw->n_rec);
        for (int r = 0; r < raw->n_rec; ++r) {
            const long long a = raw->rec[2 * r], n = raw->rec[2 * r + 1];
            if (a < 0 || n < 0 || a > n_samples || n > n_samples - a)
                FAIL(ctx, VBX_ERR_INVALID, "%s: recording %d (start %lld, %lld samples) outside the %lld samples", fn, r, a, n,
                     (long long)n_samples);
            recs[r] = FbRec{a, n, raw->levels[r]};
            order[r] = r;
            covered += n;
        }
        std::sort(order.begin(), order.end(), [&](int p, int q) { return recs[p].first < recs[q].first; });
        for (int k = 1; k < raw->n_rec; ++k) {
            const FbRec &p = recs[order[k - 1]], &q = recs[order[k]];
            if (p.n > 0 && q.n > 0 && p.first + p.n > q.first)
                FAIL(ctx, VBX_ERR_INVALID, "%s: recordings %d (start %lld, %lld samples) and %d (start %lld) overlap", fn,
                     order[k - 1], p.first, p.n, order[k], q.first);
        }
        states.resize((size_t)raw->n_rec * MT_N);
        for (int r = 0; r < raw->n_rec; ++r) {
            uint32_t* mt = &states[(size_t)r * MT_N];
            mt[0] = raw->seeds[r];
            for (int i = 1; i < MT_N; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        }
    }
    int rc = fb_reserve(ctx, &fb->d_sig, &fb->cap_sig, (size_t)n_samples);
    if (rc == VBX_OK && raw) rc = fb_reserve(ctx, &fb->d_raw, &fb->cap_raw, (size_t)n_samples);
    if (rc == VBX_OK && raw) rc = fb_reserve(ctx, &fb->d_recs, &fb->cap_recs, recs.size());
    if (rc == VBX_OK && raw) rc = fb_reserve(ctx, &fb->d_mt, &fb->cap_mt, states.size());
    if (rc == VBX_OK) rc = fb_reserve(ctx, &fb->d_segs, &fb->cap_segs, segs.size());
    if (rc == VBX_OK) rc = fb_reserve(ctx, &fb->d_tiles, &fb->cap_tiles, tiles.size());
    if (rc == VBX_OK) rc = fb_reserve(ctx, &fb->d_logmel, &fb->cap_logmel, (size_t)rows * FB_MEL);
    if (rc == VBX_OK) rc = fb_reserve(ctx, &fb->d_fea, &fb->cap_fea, (size_t)rows * FB_MEL);
    if (rc != VBX_OK) return rc;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipEventRecord(fb->ev[0], st));
    if (raw) {
        HIPCHK(ctx, hipMemcpyAsync(fb->d_raw, raw->samples, sizeof(short) * (size_t)n_samples, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(fb->d_recs, recs.data(), sizeof(FbRec) * recs.size(), hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(fb->d_mt, states.data(), sizeof(uint32_t) * states.size(), hipMemcpyHostToDevice, st));
    } else {
        HIPCHK(ctx, hipMemcpyAsync(fb->d_sig, signal, sizeof(double) * (size_t)n_samples, hipMemcpyHostToDevice, st));
    }
    HIPCHK(ctx, hipMemcpyAsync(fb->d_segs, segs.data(), sizeof(FbSeg) * segs.size(), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(fb->d_tiles, tiles.data(), sizeof(FbTile) * tiles.size(), hipMemcpyHostToDevice, st));
    if (raw) {
        // samples that belong to no recording carry no dither and are zero
        if (covered < n_samples) HIPCHK(ctx, hipMemsetAsync(fb->d_sig, 0, sizeof(double) * (size_t)n_samples, st));
        HIPCHK(ctx, hipEventRecord(fb->evd[0], st));
        hipLaunchKernelGGL(fbank_dither_kernel, dim3((unsigned)raw->n_rec), dim3(256), 0, st, fb->d_raw, fb->d_recs, fb->d_mt,
                           fb->d_sig);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipEventRecord(fb->evd[1], st));
    }
    fb->raw = raw != nullptr;
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
    fb->n_sig = n_samples;
    if (n_frames) *n_frames = rows;
    // the host arrays above go out of scope: the copies from them must have landed
    HIPCHK(ctx, hipStreamSynchronize(st));
    return VBX_OK;
}

int vbx_fbank_run(vbx_fbank* fb, int64_t n_samples, const double* signal, int32_t n_seg, const int64_t* seg, int32_t cmn_lc,
                  int32_t cmn_rc, int64_t* n_frames) {
    if (!fb) return VBX_ERR_INVALID;
    vbx_ctx* ctx = fb->ctx;
    if (!signal || !seg || n_samples <= 0 || n_seg <= 0 || cmn_lc < 0 || cmn_rc < 0)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_fbank_run: bad argument");
    return fb_run(fb, "vbx_fbank_run", n_samples, signal, nullptr, n_seg, seg, cmn_lc, cmn_rc, n_frames);
}

int vbx_fbank_run_raw(vbx_fbank* fb, int64_t n_samples, const int16_t* samples, int32_t n_rec, const int64_t* rec,
                      const uint32_t* seeds, const double* levels, int32_t n_seg, const int64_t* seg, int32_t cmn_lc,
                      int32_t cmn_rc, int64_t* n_frames) {
    if (!fb) return VBX_ERR_INVALID;
    vbx_ctx* ctx = fb->ctx;
    if (!samples || !rec || !seeds || !levels || !seg)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_fbank_run_raw: samples, rec, seeds, levels and seg must not be NULL");
    if (n_rec <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_fbank_run_raw: n_rec = %d recordings, need at least one", n_rec);
    if (n_samples <= 0 || n_seg <= 0 || cmn_lc < 0 || cmn_rc < 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_fbank_run_raw: bad argument");
    const FbRaw raw{samples, n_rec, rec, seeds, levels};
    return fb_run(fb, "vbx_fbank_run_raw", n_samples, nullptr, &raw, n_seg, seg, cmn_lc, cmn_rc, n_frames);
}

int vbx_fbank_get_signal(vbx_fbank* fb, int64_t first, int64_t n, double* dst, int dst_on_device) {
    if (!fb) return VBX_ERR_INVALID;
    vbx_ctx* ctx = fb->ctx;
    if (!dst) FAIL(ctx, VBX_ERR_INVALID, "vbx_fbank_get_signal: dst must not be NULL");
    if (first < 0 || n < 0 || first > fb->n_sig || n > fb->n_sig - first)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_fbank_get_signal: samples %lld + %lld past the %lld of the last run", (long long)first,
             (long long)n, fb->n_sig);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(dst, fb->d_sig + first, sizeof(double) * (size_t)n,
                               dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
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
    HIPCHK(ctx, hipEventElapsedTime(&ms[0], fb->ev[0], fb->raw ? fb->evd[0] : fb->ev[1]));   // (a raw run: up to its dither kernel)
    HIPCHK(ctx, hipEventElapsedTime(&ms[1], fb->ev[1], fb->ev[2]));
    HIPCHK(ctx, hipEventElapsedTime(&ms[2], fb->ev[2], fb->ev[3]));
    if (hipEventElapsedTime(&ms[3], fb->ev[4], fb->ev[5]) != hipSuccess) ms[3] = 0.0f;   // (no windows call yet)
    return VBX_OK;
}

int vbx_fbank_dither_time(vbx_fbank* fb, float* ms) {
    if (!fb || !ms) return VBX_ERR_INVALID;
    vbx_ctx* ctx = fb->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    *ms = 0.0f;                                                 // (the last run was no raw one)
    if (fb->raw) HIPCHK(ctx, hipEventElapsedTime(ms, fb->evd[0], fb->evd[1]));
    return VBX_OK;
}

}  // extern "C"
