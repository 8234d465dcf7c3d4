// vbx_host_ahc.hpp -- C ABI: the rows next to the path -- score stage of the AHC initialisation, resident x-vectors, average linkage
// (one translation unit with vbx_capi.hip, which includes the parts in order, this one after vbx_host_call.hpp: every entry
// point here keeps its device scratch in a DeviceCall; not a stand-alone header)
#pragma once
// ---------------------------------------------------------------------------------------
// score stage of the AHC initialisation (vbhmm.py:135-138)
// ---------------------------------------------------------------------------------------

struct vbx_scores {
    vbx_ctx* ctx = nullptr;
    long long n = 0;
    double* d_s = nullptr;
};

extern "C" {

int vbx_scores_destroy(vbx_scores* sc) {
    if (!sc) return VBX_OK;
    (void)hipSetDevice(sc->ctx->device);
    ctx_free(sc->ctx, sc->d_s);
    delete sc;
    return VBX_OK;
}

int64_t vbx_scores_count(const vbx_scores* sc) { return sc ? sc->n : 0; }

// the end of every function that makes a handle: out it goes, or away where filling it failed (*out is NULL already)
static int scores_result(vbx_scores* sc, int rc, vbx_scores** out) {
    if (rc == VBX_OK) *out = sc;
    else vbx_scores_destroy(sc);
    return rc;
}

// x: host pointer (uploaded) or, with on_device, rows already resident in HBM
static int cos_similarity_impl(vbx_ctx* ctx, int64_t T, int32_t D, const double* x, bool on_device, vbx_scores** out) {
    if (T > 200000) FAIL(ctx, VBX_ERR_UNSUPPORTED, "T=%lld: the T x T score matrix would not fit the device", (long long)T);
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int Dp = round_up(D, 16);
    vbx_scores* sc = new vbx_scores();
    sc->ctx = ctx;
    sc->n = (long long)T * T;
    int rc;
    {
        DeviceCall call(ctx);
        const double* rows = on_device ? x : call.upload(x, (size_t)T * D);
        double* d_xn = call.alloc<double>((size_t)T * Dp);
        if (call.ok()) call.rc = dmalloc(ctx, &sc->d_s, (size_t)sc->n);
        if (call.ok()) {
            hipLaunchKernelGGL(vbx::cos_norm_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, call.st, rows, d_xn, (long long)T, (int)D, Dp);
            const unsigned nb = (unsigned)((T + 63) / 64);
            hipLaunchKernelGGL(vbx::cos_gemm_kernel, dim3(nb, nb), dim3(256), 0, call.st, d_xn, sc->d_s, (long long)T, Dp);
            call.launched();
        }
        call.sync();
        rc = call.finish("cos_similarity kernels failed");
    }                                             // (the scratch is back, the stream idle: the handle may go too)
    return scores_result(sc, rc, out);
}

int vbx_cos_similarity(vbx_ctx* ctx, int64_t T, int32_t D, const double* x, vbx_scores** out) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!x || !out || T <= 0 || D <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_cos_similarity: bad argument");
    return cos_similarity_impl(ctx, T, D, x, false, out);
}

// ---- x-vectors of an archive resident in HBM: projections, initial assignments, labels (vbx_frontend.hpp) ------------
struct vbx_xvectors {
    vbx_ctx* ctx = nullptr;
    long long n = 0;
    int Dl = 0, fea_dim = 0;
    double *d_xproj = nullptr, *d_fea = nullptr;
};

static const double* xvectors_fea_rows(const vbx_xvectors* xv, int64_t row0, int64_t T, int D, int device) {
    if (!xv || row0 < 0 || row0 + T > xv->n || D != xv->fea_dim || xv->ctx->device != device) return nullptr;
    return xv->d_fea + row0 * xv->fea_dim;
}

int vbx_xvectors_destroy(vbx_xvectors* xv) {
    if (!xv) return VBX_OK;
    (void)hipSetDevice(xv->ctx->device);
    (void)hipStreamSynchronize(xv->ctx->stream);
    ctx_free(xv->ctx, xv->d_xproj);
    ctx_free(xv->ctx, xv->d_fea);
    delete xv;
    return VBX_OK;
}

static_assert(sizeof(long long) == sizeof(int64_t), "row indices go up as they come");
// x: n rows on the host (uploaded), or with on_device the rows rows_host[0 .. n) (nullptr: the first n) of an array that
// already lies in HBM; everything after the first kernel is the same chain
static int xvectors_project_impl(vbx_ctx* ctx, int64_t n, int32_t Din, int32_t Dl, int32_t fea_dim, const void* x, int x_dtype,
                                 bool on_device, const int64_t* rows_host, const double* mean1, const double* lda,
                                 const double* mean2, const double* plda_mu, const double* plda_tr, vbx_xvectors** out) {
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int Kp = round_up(Din, 4), Np = round_up(Dl, 16), Kp2 = round_up(Dl, 4), Np2 = round_up(fea_dim, 16);
    // padded operands: lda [Kp][Np]; plda_tr^T [Kp2][Np2] (column k = k-th output dim); the mean of the second product
    // goes through it: (x - mu) P = x P - mu P
    std::vector<double> ldap((size_t)Kp * Np, 0.0), ptp((size_t)Kp2 * Np2, 0.0), mup(Np2, 0.0), m2p(Np, 0.0);
    for (int k = 0; k < Din; ++k)
        for (int c = 0; c < Dl; ++c) ldap[(size_t)k * Np + c] = lda[(size_t)k * Dl + c];
    for (int c = 0; c < Dl; ++c) m2p[c] = mean2[c];
    for (int k = 0; k < fea_dim; ++k) {
        double acc = 0.0;
        for (int d = 0; d < Dl; ++d) {
            ptp[(size_t)d * Np2 + k] = plda_tr[(size_t)k * Dl + d];
            acc += plda_mu[d] * plda_tr[(size_t)k * Dl + d];
        }
        mup[k] = acc;
    }
    vbx_xvectors* xv = new vbx_xvectors();
    xv->ctx = ctx;
    xv->n = n;
    xv->Dl = Dl;
    xv->fea_dim = fea_dim;
    const size_t esz = x_dtype == VBX_F64 ? 8 : 4;
    int rc;
    {
        DeviceCall call(ctx);
        hipStream_t st = call.st;
        const void* src = on_device ? x : call.upload(static_cast<const char*>(x), (size_t)n * Din * esz);
        const long long* d_rows = rows_host ? call.upload((const long long*)rows_host, (size_t)n) : nullptr;
        double* d_y1 = call.alloc<double>((size_t)n * Kp);
        const double* d_m1 = call.upload(mean1, (size_t)Din);
        const double* d_lda = call.upload(ldap.data(), ldap.size());
        const double* d_m2 = call.upload(m2p.data(), m2p.size());
        const double* d_pt = call.upload(ptp.data(), ptp.size());
        const double* d_mu = call.upload(mup.data(), mup.size());
        if (call.ok()) call.rc = dmalloc(ctx, &xv->d_xproj, (size_t)n * Kp2);
        if (call.ok()) call.rc = dmalloc(ctx, &xv->d_fea, (size_t)n * fea_dim);
        if (call.ok()) {
            const dim3 rows((unsigned)((n + 3) / 4)), blocks((unsigned)((n + 63) / 64));
            if (x_dtype == VBX_F64)
                hipLaunchKernelGGL((vbx::xv_center_norm_kernel<double>), rows, dim3(256), 0, st, (const double*)src, d_m1, d_y1, (long long)n, (int)Din, (int)Din, Kp, d_rows);
            else
                hipLaunchKernelGGL((vbx::xv_center_norm_kernel<float>), rows, dim3(256), 0, st, (const float*)src, d_m1, d_y1, (long long)n, (int)Din, (int)Din, Kp, d_rows);
            hipLaunchKernelGGL(vbx::xv_gemm_kernel, blocks, dim3(256), 0, st, d_y1, d_lda, d_m2, xv->d_xproj, (long long)n, Kp, Np, (int)Dl, Kp2);
            // (the columns Dl .. Kp2 of xproj must be zero for the second product)
            hipLaunchKernelGGL((vbx::xv_center_norm_kernel<double>), rows, dim3(256), 0, st, xv->d_xproj, (const double*)nullptr, xv->d_xproj, (long long)n, (int)Dl, Kp2, Kp2, (const long long*)nullptr);
            hipLaunchKernelGGL(vbx::xv_gemm_kernel, blocks, dim3(256), 0, st, xv->d_xproj, d_pt, d_mu, xv->d_fea, (long long)n, Kp2, Np2, (int)fea_dim, (int)fea_dim);
            call.launched();
        }
        call.sync();
        rc = call.finish("x-vector projection failed");
    }                                             // (the scratch is back, the stream idle: the handle may go too)
    if (rc != VBX_OK) {
        vbx_xvectors_destroy(xv);
        return rc;
    }
    *out = xv;
    return VBX_OK;
}

int vbx_xvectors_project(vbx_ctx* ctx, int64_t n, int32_t Din, int32_t Dl, int32_t fea_dim, const void* x, int x_dtype,
                         const double* mean1, const double* lda, const double* mean2, const double* plda_mu,
                         const double* plda_tr, vbx_xvectors** out) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!out || !x || !mean1 || !lda || !mean2 || !plda_mu || !plda_tr || n <= 0 || Din <= 0 || Dl <= 0 || fea_dim <= 0 ||
        fea_dim > Dl || (x_dtype != VBX_F32 && x_dtype != VBX_F64))
        FAIL(ctx, VBX_ERR_INVALID, "vbx_xvectors_project: bad argument");
    return xvectors_project_impl(ctx, n, Din, Dl, fea_dim, x, x_dtype, false, nullptr, mean1, lda, mean2, plda_mu, plda_tr, out);
}

// device memory of ctx's device?  (a host pointer, or an allocation of another device, is refused before any kernel reads it)
static bool on_ctx_device(vbx_ctx* ctx, const void* p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return attr.type == hipMemoryTypeDevice && attr.device == ctx->device;
}

int vbx_xvectors_project_device(vbx_ctx* ctx, int64_t n_src, int32_t Din, int32_t Dl, int32_t fea_dim, const float* d_x,
                                int64_t n, const int64_t* rows_host, const double* mean1, const double* lda,
                                const double* mean2, const double* plda_mu, const double* plda_tr, vbx_xvectors** out) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!out || !d_x || !mean1 || !lda || !mean2 || !plda_mu || !plda_tr || n <= 0 || n_src <= 0 || n > n_src || Din <= 0 ||
        Dl <= 0 || fea_dim <= 0 || fea_dim > Dl || (!rows_host && n != n_src))
        FAIL(ctx, VBX_ERR_INVALID, "vbx_xvectors_project_device: bad argument");
    *out = nullptr;
    for (int64_t i = 0; rows_host && i < n; ++i) {
        if (rows_host[i] < 0 || rows_host[i] >= n_src)
            FAIL(ctx, VBX_ERR_INVALID, "vbx_xvectors_project_device: rows[%lld] = %lld is outside the %lld source rows", (long long)i,
                 (long long)rows_host[i], (long long)n_src);
        if (i > 0 && rows_host[i] <= rows_host[i - 1])
            FAIL(ctx, VBX_ERR_INVALID, "vbx_xvectors_project_device: rows[%lld] = %lld does not increase (rows[%lld] = %lld)", (long long)i,
                 (long long)rows_host[i], (long long)(i - 1), (long long)rows_host[i - 1]);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!on_ctx_device(ctx, d_x))
        FAIL(ctx, VBX_ERR_INVALID, "vbx_xvectors_project_device: x is not device memory of device %d", ctx->device);
    return xvectors_project_impl(ctx, n, Din, Dl, fea_dim, d_x, VBX_F32, true, rows_host, mean1, lda, mean2, plda_mu, plda_tr, out);
}

int vbx_rows_nan_flags(vbx_ctx* ctx, const float* d_x, int64_t n, int32_t D, int32_t* flags_host) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!d_x || !flags_host || n <= 0 || D <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_rows_nan_flags: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!on_ctx_device(ctx, d_x)) FAIL(ctx, VBX_ERR_INVALID, "vbx_rows_nan_flags: x is not device memory of device %d", ctx->device);
    DeviceCall call(ctx);
    int* d_flags = call.alloc<int>((size_t)n);
    if (call.ok()) {
        hipLaunchKernelGGL(vbx::rows_nan_flags_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, call.st, d_x, d_flags, (long long)n, (int)D);
        call.launched();
    }
    call.download(flags_host, d_flags, (size_t)n);
    call.sync();
    return call.finish("vbx_rows_nan_flags failed");
}

int vbx_random_labels(vbx_ctx* ctx, uint64_t seed, uint64_t name_hash, int64_t restart, int64_t T, int32_t N, int32_t* labels_host) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!labels_host || T <= 0 || N <= 0 || restart < 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_random_labels: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DeviceCall call(ctx);
    int* d_labels = call.alloc<int>((size_t)T);
    if (call.ok()) {
        hipLaunchKernelGGL(vbx::random_labels_kernel, dim3((unsigned)(((T + 3) / 4 + 255) / 256)), dim3(256), 0, call.st, d_labels,
                           (long long)T, (unsigned long long)seed, (unsigned long long)name_hash, (unsigned long long)restart,
                           (unsigned long long)N);
        call.launched();
    }
    call.download(labels_host, d_labels, (size_t)T);
    call.sync();
    return call.finish("vbx_random_labels failed");
}

int vbx_xvectors_get(vbx_xvectors* xv, int which, int64_t row0, int64_t nrows, double* out) {
    if (!xv || !out || row0 < 0 || nrows < 0 || row0 + nrows > xv->n || (which != 0 && which != 1)) return VBX_ERR_INVALID;
    vbx_ctx* ctx = xv->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (which == 1) {
        HIPCHK(ctx, hipMemcpy(out, xv->d_fea + row0 * xv->fea_dim, sizeof(double) * (size_t)nrows * xv->fea_dim, hipMemcpyDeviceToHost));
    } else {
        const int ld = round_up(xv->Dl, 4);
        HIPCHK(ctx, hipMemcpy2D(out, sizeof(double) * xv->Dl, xv->d_xproj + row0 * ld, sizeof(double) * ld, sizeof(double) * xv->Dl,
                                (size_t)nrows, hipMemcpyDeviceToHost));
    }
    return VBX_OK;
}

int vbx_cos_similarity_resident(vbx_ctx* ctx, vbx_xvectors* xv, int64_t row0, int64_t T, vbx_scores** out) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!xv || !out || T <= 0 || row0 < 0 || row0 + T > xv->n || xv->ctx->device != ctx->device)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_cos_similarity_resident: bad argument");
    const int ld = round_up(xv->Dl, 4);               // (the padding columns are zero: part of the rows, no effect on the scores)
    return cos_similarity_impl(ctx, T, ld, xv->d_xproj + row0 * ld, true, out);
}

int vbx_scores_upload(vbx_ctx* ctx, int64_t n, const double* s, vbx_scores** out) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!s || !out || n <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_scores_upload: bad argument");
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    vbx_scores* sc = new vbx_scores();
    sc->ctx = ctx;
    sc->n = n;
    int rc = dmalloc(ctx, &sc->d_s, (size_t)n);
    if (rc == VBX_OK) {
        hipError_t e = hipMemcpy(sc->d_s, s, sizeof(double) * (size_t)n, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            ctx->err = std::string("score upload failed: ") + hipGetErrorString(e);
            rc = VBX_ERR_HIP;
        }
    }
    return scores_result(sc, rc, out);
}

int vbx_scores_get(vbx_scores* sc, int64_t offset, int64_t count, double* out) {
    if (!sc) return VBX_ERR_INVALID;
    if (!out || offset < 0 || count < 0 || offset + count > sc->n) FAIL(sc->ctx, VBX_ERR_INVALID, "vbx_scores_get: bad range");
    HIPCHK(sc->ctx, hipSetDevice(sc->ctx->device));
    if (count) HIPCHK(sc->ctx, hipMemcpy(out, sc->d_s + offset, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
    return VBX_OK;
}

int vbx_linkage_average(int64_t n, const double* condensed, double* Z) {
    if (n < 1 || (n > 1 && (!condensed || !Z))) return VBX_ERR_INVALID;
    if (n > 65536) return VBX_ERR_UNSUPPORTED;               // n^2 doubles of working storage
    try {
        vbx::average_linkage(n, condensed, Z);
    } catch (const std::bad_alloc&) {
        return VBX_ERR_HIP - 100;                            // host allocation failure (no ctx to carry a message)
    }
    return VBX_OK;
}

int vbx_linkage_average_fastcluster(int64_t n, const double* condensed, double* Z) {
    if (n < 1 || (n > 1 && (!condensed || !Z))) return VBX_ERR_INVALID;
    if (n > 65536) return VBX_ERR_UNSUPPORTED;
    try {
        vbx::average_linkage_fastcluster(n, condensed, Z);
    } catch (const std::bad_alloc&) {
        return VBX_ERR_HIP - 100;
    }
    return VBX_OK;
}

int64_t vbx_ark_index(const void* buf, int64_t len, int64_t cap, int64_t* key_off, int32_t* key_len, int64_t* data_off,
                      int32_t* dim, int32_t* elem_size) {
    if (!buf || len < 0 || cap < 0 || (cap > 0 && (!key_off || !key_len || !data_off || !dim || !elem_size))) return -1;
    return vbx::ark_index(static_cast<const unsigned char*>(buf), len, cap, key_off, key_len, data_off, dim, elem_size);
}

int vbx_gather_rows(const void* buf, int64_t len, const int64_t* offsets, int64_t n, int64_t row_bytes, void* out) {
    if (!buf || !out || !offsets || n < 0 || row_bytes < 0) return VBX_ERR_INVALID;
    const unsigned char* src = static_cast<const unsigned char*>(buf);
    unsigned char* dst = static_cast<unsigned char*>(out);
    for (int64_t i = 0; i < n; ++i) {
        if (offsets[i] < 0 || offsets[i] + row_bytes > len) return VBX_ERR_INVALID;
        std::memcpy(dst + i * row_bytes, src + offsets[i], (size_t)row_bytes);
    }
    return VBX_OK;
}

int vbx_fcluster_distance(int64_t n, const double* Z, double t, int32_t* labels) {
    if (n < 1 || !labels || (n > 1 && !Z)) return VBX_ERR_INVALID;
    for (int64_t k = 0; k < n - 1; ++k) {                      // children exist before their parent, ids in range
        const double a = Z[4 * k], b = Z[4 * k + 1];
        if (!(a >= 0 && b >= 0 && a < (double)(n + k) && b < (double)(n + k))) return VBX_ERR_INVALID;
    }
    try {
        vbx::fcluster_distance(n, Z, t, labels);
    } catch (const std::bad_alloc&) {
        return VBX_ERR_HIP - 100;
    }
    return VBX_OK;
}

int vbx_scores_linkage_average(vbx_scores* sc, int64_t T, double* Z) {
    if (!sc || !Z || T < 1 || (long long)T * T != sc->n || T > 0x7fffffffLL / 2) return VBX_ERR_INVALID;
    if (T == 1) return VBX_OK;
    vbx_ctx* ctx = sc->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // Two ways over the matrix (vbx_ahc.hpp):
    //   rounds  all reciprocal nearest-neighbour pairs of the current matrix merged at once, the whole chip on every pass
    //           (VBX_AMD_LINKAGE_DEVICE=rounds, the default from kRoundsFrom clusters): a few dozen rounds for 10 000 x-vectors
    //   chain   SciPy's nearest-neighbour chain on ONE persistent workgroup, bit for bit the host routine (=chain): it
    //           finishes what the rounds leave (the last kRoundsStop = 48 clusters, where a round is all launch latency: handing
    //           over at 384 / 128 / 48 / 16 clusters measured 7.6 / 5.9 / 5.8 / 6.0 ms at T = 10 000 and 3.1 / 1.4 / 1.2 / 1.1 ms
    //           at T = 1025) and is the reference the rounds are tested against
    // The chain runs in stages of n/4 merges with a compaction of the live rows and columns in between; below kStageMin
    // clusters the rest runs in one stage (there a merge costs its four round trips, not the bytes of a row).
    constexpr long long kStageMin = 4096, kRoundsFrom = 256, kRoundsStop = 48;
    const char* dev_mode = experiment_env("VBX_AMD_LINKAGE_DEVICE");           // (read per call: tests compare the two in one process)
    const bool rounds_on = !(dev_mode && std::strcmp(dev_mode, "chain") == 0);
    const bool rounds = rounds_on && T >= kRoundsFrom;
    std::vector<vbx::ChainMerge> merges((size_t)(T - 1));
    static_assert(sizeof(vbx::ChainMerge) == sizeof(vbx::ChainMergeDev), "merge record layout");
    std::vector<int> ones((size_t)T, 1), iota((size_t)T);
    for (long long i = 0; i < T; ++i) iota[(size_t)i] = (int)i;
    const int zero4[4] = {0, 0, 0, 0};
    DeviceCall call(ctx);
    hipStream_t st = call.st;
    int* d_size = call.upload(ones.data(), (size_t)T);
    int* d_chain = call.alloc<int>((size_t)T);
    int* d_orig = call.upload(iota.data(), (size_t)T);
    int* d_state = call.upload(zero4, (size_t)4);
    auto* d_merges = call.alloc<vbx::ChainMergeDev>((size_t)(T - 1));
    int* d_size2 = call.alloc<int>((size_t)T);
    int* d_orig2 = call.alloc<int>((size_t)T);
    int* d_old = call.alloc<int>((size_t)T);
    int* d_newidx = call.alloc<int>((size_t)T);
    int* d_nn = rounds ? call.alloc<int>((size_t)T) : nullptr;
    double* d_nnd = rounds ? call.alloc<double>((size_t)T) : nullptr;
    int* d_role = rounds ? call.alloc<int>((size_t)T) : nullptr;
    auto* d_pairs = rounds ? call.alloc<vbx::RnnPair>((size_t)(T / 2 + 1)) : nullptr;
    if (call.ok()) {
        hipLaunchKernelGGL(vbx::linkage_prepare_kernel, dim3((unsigned)T), dim3(256), 0, st, sc->d_s, (long long)T);
        double* cur = sc->d_s;
        int *size_c = d_size, *size_a = d_size2, *orig_c = d_orig, *orig_a = d_orig2;
        long long n_cur = T, done = 0;
        auto compact_into = [&](double* dst, long long n_new) {           // the live clusters move up, in order
            hipLaunchKernelGGL(vbx::linkage_compact_index_kernel, dim3(1), dim3(1024), 0, st, (int)n_cur, size_c, orig_c, d_chain,
                               d_state, size_a, orig_a, d_old, d_newidx);
            hipLaunchKernelGGL(vbx::linkage_compact_matrix_kernel, dim3((unsigned)n_new), dim3(256), 0, st, cur, (int)n_cur, dst,
                               (int)n_new, d_old);
            std::swap(size_c, size_a);
            std::swap(orig_c, orig_a);
            n_cur = n_new;
        };
        if (rounds) {
            // rounds of reciprocal pairs on the matrix as it lies (dead rows and columns are skipped, not removed: a
            // round reads n_live x n entries), until few clusters are left or a round hardly merges anything
            int stalled = 0;
            while (T - done > kRoundsStop && stalled < 3) {
                const int n = (int)T;
                hipLaunchKernelGGL(vbx::rnn_rowmin_kernel, dim3((unsigned)n), dim3(256), 0, st, cur, n, size_c, d_nn, d_nnd);
                hipLaunchKernelGGL(vbx::rnn_pairs_kernel, dim3(1), dim3(1024), 0, st, n, size_c, orig_c, d_nn, d_nnd, d_pairs, d_role,
                                   d_merges, d_state);
                call.launched();
                int st_host[4] = {0, 0, 0, 0};
                call.download(st_host, d_state, (size_t)4);
                call.sync();
                if (!call.ok()) break;
                const int np = st_host[3];
                if (np <= 0) break;                                        // (cannot happen: the smallest pair is reciprocal)
                hipLaunchKernelGGL(vbx::rnn_rows_kernel, dim3((unsigned)np), dim3(256), 0, st, cur, n, size_c, d_pairs);
                hipLaunchKernelGGL(vbx::rnn_cols_kernel, dim3((unsigned)n), dim3(256), 0, st, cur, n, size_c, d_role, d_pairs, d_state);
                hipLaunchKernelGGL(vbx::rnn_canon_kernel, dim3((unsigned)np), dim3(256), 0, st, cur, n, d_pairs, d_state);
                hipLaunchKernelGGL(vbx::rnn_sizes_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, size_c, d_pairs, d_state);
                call.launched();
                stalled = ((long long)np * 64 < T - done) ? stalled + 1 : 0;
                done = st_host[2];
            }
            if (call.ok() && done < T - 1) {                               // what is left goes to the chain, compacted
                const long long n_new = T - done;
                double* d_cmp = call.alloc<double>((size_t)(n_new * n_new));
                if (call.ok()) {
                    compact_into(d_cmp, n_new);
                    cur = d_cmp;
                }
            }
        }
        if (call.ok() && done < T - 1) {
            const bool stages = n_cur >= 2 * kStageMin;
            const long long n_alt = stages ? n_cur - n_cur / 4 : 0;
            double* alt = stages ? call.alloc<double>((size_t)(n_alt * n_alt)) : nullptr;
            while (call.ok() && done < T - 1) {
                const long long remaining = T - 1 - done;
                const long long m = (stages && n_cur >= 2 * kStageMin) ? std::min(remaining, n_cur / 4) : remaining;
                hipLaunchKernelGGL(vbx::nn_chain_kernel, dim3(1), dim3(1024), 0, st, cur, (int)n_cur, size_c, d_chain, orig_c, d_state,
                                   d_merges, (int)done, (int)(done + m));
                done += m;
                if (done < T - 1) {
                    compact_into(alt, n_cur - m);
                    std::swap(cur, alt);
                }
            }
        }
        call.launched();
    }
    call.download((vbx::ChainMergeDev*)merges.data(), d_merges, merges.size());
    call.sync();
    if (int rc = call.finish("device linkage failed")) return rc;
    vbx::finish_linkage(T, merges.data(), Z);
    return VBX_OK;
}

int vbx_scores_get_condensed(vbx_scores* sc, int64_t T, double scale, double* out) {
    if (!sc) return VBX_ERR_INVALID;
    vbx_ctx* ctx = sc->ctx;
    if (!out || T < 1 || (long long)T * T != sc->n) FAIL(ctx, VBX_ERR_INVALID, "vbx_scores_get_condensed: the scores are not a %lld x %lld matrix", (long long)T, (long long)T);
    if (T == 1) return VBX_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t m = (size_t)T * (size_t)(T - 1) / 2;
    DeviceCall call(ctx);
    double* d_c = call.alloc<double>(m);
    if (call.ok()) {
        hipLaunchKernelGGL(vbx::condense_kernel, dim3((unsigned)(T - 1)), dim3(256), 0, call.st, sc->d_s, d_c, (long long)T, scale);
        call.launched();
    }
    call.download(out, d_c, m);
    call.sync();
    return call.finish("vbx_scores_get_condensed");
}

int vbx_scores_two_gmm_calib(vbx_scores* sc, int32_t niters, double* threshold, double* llr) {
    if (!sc) return VBX_ERR_INVALID;
    vbx_ctx* ctx = sc->ctx;
    if (niters < 1 || !threshold) FAIL(ctx, VBX_ERR_INVALID, "vbx_scores_two_gmm_calib: niters must be >= 1");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double par[16];
    DeviceCall call(ctx);
    hipStream_t st = call.st;
    const int nb = (int)std::min<long long>(vbx::kGmmPartials, (sc->n + 255) / 256);
    double* d_par = call.alloc<double>(16);
    double* d_part = call.alloc<double>((size_t)nb * 6);
    double* d_llr = llr ? call.alloc<double>((size_t)sc->n) : nullptr;
    if (call.ok()) {
        hipLaunchKernelGGL((vbx::gmm_moment_kernel<0>), dim3(nb), dim3(256), 0, st, sc->d_s, sc->n, d_par, d_part);
        hipLaunchKernelGGL(vbx::gmm_init_kernel, dim3(1), dim3(256), 0, st, d_part, nb, sc->n, d_par, 0);
        hipLaunchKernelGGL((vbx::gmm_moment_kernel<1>), dim3(nb), dim3(256), 0, st, sc->d_s, sc->n, d_par, d_part);
        hipLaunchKernelGGL(vbx::gmm_init_kernel, dim3(1), dim3(256), 0, st, d_part, nb, sc->n, d_par, 1);
        for (int it = 0; it < niters; ++it) {
            hipLaunchKernelGGL(vbx::gmm_pass_kernel, dim3(nb), dim3(256), 0, st, sc->d_s, sc->n, d_par, d_part);
            hipLaunchKernelGGL(vbx::gmm_update_kernel, dim3(1), dim3(256), 0, st, d_part, nb, d_par);
        }
        if (llr) hipLaunchKernelGGL(vbx::gmm_llr_kernel, dim3(nb), dim3(256), 0, st, sc->d_s, sc->n, d_par, d_llr);
        call.launched();
    }
    call.download(par, d_par, (size_t)16);
    if (llr) call.download(llr, d_llr, (size_t)sc->n);
    call.sync();
    const int rc = call.finish("twoGMMcalib kernels failed");
    if (rc == VBX_OK) {
        // diarization_lib.py:30 with the final weights / means / var
        const double w0 = par[0], w1 = par[1], m0 = par[2], m1 = par[3], var = par[4];
        const double t0 = std::log(w0 * w0 / var) - m0 * m0 / var, t1 = std::log(w1 * w1 / var) - m1 * m1 / var;
        *threshold = -0.5 * (t0 - t1) / (m0 / var - m1 / var);
    }
    return rc;
}

// ---------------------------------------------------------------------------------------
// Kaldi-recipe PLDA similarity (diarization_lib.py:34-93; kernels in vbx_plda_score.hpp)
// ---------------------------------------------------------------------------------------

// diarization_lib.py:49-55 for one across-class variance
struct PldaTerms { double Lambda, Gamma, ld; };
static PldaTerms plda_terms(double ac) {
    const double iTC = 1.0 / (1.0 + ac), iWC2AC = 1.0 / (1.0 + 2.0 * ac);
    return PldaTerms{-0.5 * (iWC2AC - 1.0), -0.25 * (iWC2AC + 1.0 - 2.0 * iTC), std::log(1.0 + 2.0 * ac) - 2.0 * std::log(1.0 + ac)};
}

// x: host rows [T][D] (uploaded; ld == D) or, with on_device, rows in HBM with leading dimension ld
static int plda_covariance_impl(vbx_ctx* ctx, int64_t T, int32_t D, int ld, const double* x, bool on_device, double* mean,
                                double* cov) {
    if (D > 1024) FAIL(ctx, VBX_ERR_UNSUPPORTED, "PLDA covariance: D=%d, at most 1024 dimensions", (int)D);
    if (T > 200000) FAIL(ctx, VBX_ERR_UNSUPPORTED, "PLDA covariance: T=%lld rows, at most 200000", (long long)T);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int Dp = round_up(D, 16), nchunks = (int)((T + vbx::kCovChunk - 1) / vbx::kCovChunk);
    DeviceCall call(ctx);
    hipStream_t st = call.st;
    const double* rows = on_device ? x : call.upload(x, (size_t)T * D);
    double* d_sum = call.alloc<double>((size_t)nchunks * D);
    double* d_mean = call.alloc<double>((size_t)D);
    double* d_part = call.alloc<double>((size_t)nchunks * Dp * Dp);
    double* d_cov = call.alloc<double>((size_t)D * D);
    if (call.ok()) {
        const unsigned nb = (unsigned)((D + 63) / 64);
        hipLaunchKernelGGL(vbx::cov_colsum_kernel, dim3((unsigned)nchunks), dim3(256), 0, st, rows, (long long)T, (int)D, ld, d_sum);
        hipLaunchKernelGGL(vbx::cov_mean_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, st, d_sum, nchunks, (long long)T, (int)D, d_mean);
        hipLaunchKernelGGL(vbx::cov_partial_kernel, dim3(nb, nb, (unsigned)nchunks), dim3(256), 0, st, rows, d_mean, (long long)T, (int)D, ld, Dp, d_part);
        hipLaunchKernelGGL(vbx::cov_finish_kernel, dim3((unsigned)((D * D + 255) / 256)), dim3(256), 0, st, d_part, nchunks, (long long)T, (int)D, Dp, d_cov);
        call.launched();
    }
    call.download(mean, d_mean, (size_t)D);
    call.download(cov, d_cov, (size_t)D * D);
    call.sync();
    return call.finish("PLDA covariance kernels failed");
}

int vbx_plda_covariance(vbx_ctx* ctx, int64_t T, int32_t D, const double* x, double* mean, double* cov) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!x || !mean || !cov || T <= 0 || D <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_plda_covariance: bad argument");
    return plda_covariance_impl(ctx, T, D, D, x, false, mean, cov);
}

int vbx_plda_covariance_resident(vbx_ctx* ctx, vbx_xvectors* xv, int64_t row0, int64_t T, double* mean, double* cov) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!xv || !mean || !cov || T <= 0 || row0 < 0 || row0 + T > xv->n || xv->ctx->device != ctx->device)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_plda_covariance_resident: bad argument");
    const int ld = round_up(xv->Dl, 4);
    return plda_covariance_impl(ctx, T, xv->Dl, ld, xv->d_xproj + row0 * ld, true, mean, cov);
}

static int plda_scores_impl(vbx_ctx* ctx, int64_t T, int32_t D, int ld, const double* x, bool on_device, int32_t d,
                            const double* mu, const double* proj, const double* acvar, vbx_scores** out) {
    *out = nullptr;
    if (T > 200000) FAIL(ctx, VBX_ERR_UNSUPPORTED, "T=%lld: the T x T score matrix would not fit the device", (long long)T);
    if (d > 16 * vbx::kPldaMaxTiles) FAIL(ctx, VBX_ERR_UNSUPPORTED, "PLDA scores: d=%d, at most %d dimensions", (int)d, 16 * vbx::kPldaMaxTiles);
    const int Dk = round_up(D, 4), dp = round_up(d, 16);
    // one packed model block: mu [D] | proj padded [Dk][dp] | w [dp] | sqrt(Lambda) [dp] | Gamma [dp]
    const size_t o_proj = (size_t)D, o_w = o_proj + (size_t)Dk * dp, o_sl = o_w + dp, o_gam = o_sl + dp, n_model = o_gam + dp;
    std::vector<double> model(n_model, 0.0);
    double kconst = 0.0;
    for (int j = 0; j < D; ++j) {
        model[j] = mu[j];
        for (int k = 0; k < d; ++k) model[o_proj + (size_t)j * dp + k] = proj[(size_t)j * d + k];
    }
    for (int k = 0; k < d; ++k) {
        const PldaTerms t = plda_terms(acvar[k]);
        if (!(acvar[k] >= 0.0) || !(t.Lambda >= 0.0)) FAIL(ctx, VBX_ERR_INVALID, "PLDA scores: acvar[%d] = %g is not a variance", k, acvar[k]);
        model[o_w + k] = 1.0 / (acvar[k] + 1.0);
        model[o_sl + k] = std::sqrt(t.Lambda);
        model[o_gam + k] = t.Gamma;
        kconst += t.ld;
    }
    kconst *= -0.5;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    vbx_scores* sc = new vbx_scores();
    sc->ctx = ctx;
    sc->n = (long long)T * T;
    int rc;
    {
        DeviceCall call(ctx);
        hipStream_t st = call.st;
        const double* rows = on_device ? x : call.upload(x, (size_t)T * D);
        const double* d_model = call.upload(model.data(), n_model);
        double* d_a = call.alloc<double>((size_t)T * dp);
        double* d_g = call.alloc<double>((size_t)T);
        if (call.ok()) call.rc = dmalloc(ctx, &sc->d_s, (size_t)sc->n);
        if (call.ok()) {
            hipLaunchKernelGGL(vbx::plda_project_kernel, dim3((unsigned)((T + 15) / 16)), dim3(64), 0, st, rows, (long long)T, (int)D, ld,
                               d_model, d_model + o_proj, (int)d, dp, d_model + o_w, d_model + o_sl, d_model + o_gam, d_a, d_g);
            const unsigned nb = (unsigned)((T + 63) / 64);
            hipLaunchKernelGGL(vbx::plda_score_gemm_kernel, dim3(nb, nb), dim3(256), 0, st, d_a, d_a, d_g, d_g, kconst, sc->d_s,
                               (long long)T, (long long)T, dp);
            call.launched();
        }
        call.sync();
        rc = call.finish("PLDA score kernels failed");
    }                                             // (the scratch is back, the stream idle: the handle may go too)
    return scores_result(sc, rc, out);
}

int vbx_plda_scores(vbx_ctx* ctx, int64_t T, int32_t D, const double* x, int32_t d, const double* mu, const double* proj,
                    const double* acvar, vbx_scores** out) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!x || !mu || !proj || !acvar || !out || T <= 0 || D <= 0 || d <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_plda_scores: bad argument");
    return plda_scores_impl(ctx, T, D, D, x, false, d, mu, proj, acvar, out);
}

int vbx_plda_scores_resident(vbx_ctx* ctx, vbx_xvectors* xv, int64_t row0, int64_t T, int32_t d, const double* mu,
                             const double* proj, const double* acvar, vbx_scores** out) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!xv || !mu || !proj || !acvar || !out || T <= 0 || d <= 0 || row0 < 0 || row0 + T > xv->n || xv->ctx->device != ctx->device)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_plda_scores_resident: bad argument");
    const int ld = round_up(xv->Dl, 4);               // (the padding columns are never read: the kernels stop at Dl)
    return plda_scores_impl(ctx, T, xv->Dl, ld, xv->d_xproj + row0 * ld, true, d, mu, proj, acvar, out);
}

int vbx_plda_score_lda(vbx_ctx* ctx, int64_t N, int64_t M, int32_t D, const double* Fe, const double* Ft, const double* diagAC,
                       double* out) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!Fe || !Ft || !diagAC || !out || N <= 0 || M <= 0 || D <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_plda_score_lda: bad argument");
    if (N > 200000 || M > 200000) FAIL(ctx, VBX_ERR_UNSUPPORTED, "vbx_plda_score_lda: %lld x %lld scores would not fit the device", (long long)N, (long long)M);
    const int dp = round_up(D, 16);
    std::vector<double> terms(2 * (size_t)D);                  // Lambda [D] | Gamma [D]
    double kconst = 0.0;
    for (int k = 0; k < D; ++k) {
        const PldaTerms t = plda_terms(diagAC[k]);
        terms[k] = t.Lambda;
        terms[(size_t)D + k] = t.Gamma;
        kconst += t.ld;
    }
    kconst *= -0.5;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DeviceCall call(ctx);
    hipStream_t st = call.st;
    const double* d_fe = call.upload(Fe, (size_t)N * D);
    const double* d_ft = call.upload(Ft, (size_t)M * D);
    const double* d_terms = call.upload(terms.data(), terms.size());
    double* d_a = call.alloc<double>((size_t)N * dp);
    double* d_b = call.alloc<double>((size_t)M * dp);
    double* d_r = call.alloc<double>((size_t)N);
    double* d_c = call.alloc<double>((size_t)M);
    double* d_s = call.alloc<double>((size_t)N * (size_t)M);
    if (call.ok()) {
        hipLaunchKernelGGL(vbx::plda_lda_rows_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, d_fe, (long long)N, (int)D, d_terms,
                           d_terms + D, dp, d_a, d_r);
        hipLaunchKernelGGL(vbx::plda_lda_rows_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, d_ft, (long long)M, (int)D,
                           (const double*)nullptr, d_terms + D, dp, d_b, d_c);
        hipLaunchKernelGGL(vbx::plda_score_gemm_kernel, dim3((unsigned)((M + 63) / 64), (unsigned)((N + 63) / 64)), dim3(256), 0, st, d_a,
                           d_b, d_r, d_c, kconst, d_s, (long long)N, (long long)M, dp);
        call.launched();
    }
    call.download(out, d_s, (size_t)N * (size_t)M);
    call.sync();
    return call.finish("PLDA LDA-space score kernels failed");
}

}  // extern "C"
