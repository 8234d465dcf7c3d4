// vbx_host_resnet.hpp -- host runtime of the x-vector network (vbx_resnet.hpp): the folded parameters, the workspace and the
// launch sequence of one batch of windows.  Included by vbx_capi.hip after vbx_host_fbank.hpp (fb_reserve).
//
// Parameter blob (f32, vbx_amd/xvector.py:fold writes it in this order): for every convolution in network order -- the
// stem, then per block conv1, conv2, conv3 and, in the first block of a stage, the shortcut -- its weights [kh kw Cin][Cout]
// and its folded bias [Cout]; then the embedding [16384][E] (rows in the pooling kernel's order) and its bias [E].

struct RnConv {
    int ks, stride, cin, cout;
    size_t w, b;                                               // offsets into the parameter blob
};

struct vbx_resnet {
    vbx_ctx* ctx = nullptr;
    int E = 0, Ep = 0;                                         // embedding width, padded to 32 columns on the device
    std::vector<RnConv> convs;                                 // [0] the stem, then 3 or 4 per block
    float *d_par = nullptr, *d_emb_w = nullptr, *d_emb_b = nullptr;
    float *d_in = nullptr, *d_x[2] = {}, *d_t1 = nullptr, *d_t2 = nullptr, *d_sc = nullptr, *d_pool = nullptr, *d_out = nullptr;
    size_t cap_in = 0, cap_x[2] = {}, cap_t1 = 0, cap_t2 = 0, cap_sc = 0, cap_pool = 0, cap_out = 0;
    hipEvent_t ev[7] = {};                                     // stem | layer1 | layer2 | layer3 | layer4 | pool + embedding
};

static const int RN_BLOCKS[4] = {3, 4, 23, 3}, RN_PLANES[4] = {32, 64, 128, 256}, RN_STRIDE[4] = {1, 2, 2, 2};

static inline int rn_out(int n, int stride) { return (n - 1) / stride + 1; }

// the network's convolutions in blob order; returns the number of f32 parameters before the embedding
static size_t rn_layout(std::vector<RnConv>& convs) {
    size_t off = 0;
    auto add = [&](int ks, int stride, int cin, int cout) {
        RnConv c{ks, stride, cin, cout, off, off + (size_t)ks * ks * cin * cout};
        off = c.b + cout;
        convs.push_back(c);
    };
    add(3, 1, 1, 32);
    int cin = 32;
    for (int L = 0; L < 4; ++L)
        for (int i = 0; i < RN_BLOCKS[L]; ++i) {
            const int planes = RN_PLANES[L], s = i == 0 ? RN_STRIDE[L] : 1;
            add(1, 1, cin, planes);
            add(3, s, planes, planes);
            add(1, 1, planes, 4 * planes);
            if (i == 0) add(1, s, cin, 4 * planes);
            cin = 4 * planes;
        }
    return off;
}

template <int KS, int S>
static void rn_launch_ks(hipStream_t st, int BN, int BM, const float* x, const float* w, const float* b, const float* res,
                         float* y, int H, int W, int Cin, int Ho, int Wo, int Cout, long long M, int relu) {
    const dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)(Cout / BN)), blk(256);
    if (BN == 128 && BM == 64)
        hipLaunchKernelGGL((resnet_conv_kernel<KS, S, 128, 64>), grid, blk, 0, st, x, w, b, res, y, H, W, Cin, Ho, Wo, Cout, M, relu);
    else if (BN == 128)
        hipLaunchKernelGGL((resnet_conv_kernel<KS, S, 128, 128>), grid, blk, 0, st, x, w, b, res, y, H, W, Cin, Ho, Wo, Cout, M, relu);
    else if (BN == 64 && BM == 64)
        hipLaunchKernelGGL((resnet_conv_kernel<KS, S, 64, 64>), grid, blk, 0, st, x, w, b, res, y, H, W, Cin, Ho, Wo, Cout, M, relu);
    else if (BN == 64)
        hipLaunchKernelGGL((resnet_conv_kernel<KS, S, 64, 128>), grid, blk, 0, st, x, w, b, res, y, H, W, Cin, Ho, Wo, Cout, M, relu);
    else
        hipLaunchKernelGGL((resnet_conv_kernel<KS, S, 32, 128>), grid, blk, 0, st, x, w, b, res, y, H, W, Cin, Ho, Wo, Cout, M, relu);
}

// the BN x BM output tile of a convolution of M output positions x Cout channels (Cout a multiple of 32)
static void rn_tile(long long M, int Cout, int* bn, int* bm) {
    // (a few rows -- the embedding -- take narrow tiles: more workgroups over its long K)
    *bn = M < 4096 ? 32 : Cout % 128 == 0 ? 128 : Cout % 64 == 0 ? 64 : 32;
    // 64-row tiles where 128-row ones leave fewer than four workgroups per CU (layer3 and layer4 at 128 windows)
    *bm = *bn >= 64 && (M + 127) / 128 * (Cout / *bn) < 1024 ? 64 : 128;
}

static void rn_launch(hipStream_t st, int ks, int stride, int BN, int BM, const float* x, const float* w, const float* b,
                      const float* res, float* y, int H, int W, int Cin, int Ho, int Wo, int Cout, long long M, int relu) {
    if (ks == 1 && stride == 1) rn_launch_ks<1, 1>(st, BN, BM, x, w, b, res, y, H, W, Cin, Ho, Wo, Cout, M, relu);
    else if (ks == 1) rn_launch_ks<1, 2>(st, BN, BM, x, w, b, res, y, H, W, Cin, Ho, Wo, Cout, M, relu);
    else if (stride == 1) rn_launch_ks<3, 1>(st, BN, BM, x, w, b, res, y, H, W, Cin, Ho, Wo, Cout, M, relu);
    else rn_launch_ks<3, 2>(st, BN, BM, x, w, b, res, y, H, W, Cin, Ho, Wo, Cout, M, relu);
}

// one convolution of n images H x W x Cin -> Ho x Wo x Cout (Cout a multiple of 32, Cin of 16)
static void rn_conv(hipStream_t st, int ks, int stride, const float* x, const float* w, const float* b, const float* res, float* y,
                    int n, int H, int W, int Cin, int Cout, int relu) {
    const int Ho = rn_out(H, stride), Wo = rn_out(W, stride);
    const long long M = (long long)n * Ho * Wo;
    int BN, BM;
    rn_tile(M, Cout, &BN, &BM);
    rn_launch(st, ks, stride, BN, BM, x, w, b, res, y, H, W, Cin, Ho, Wo, Cout, M, relu);
}

// ---- step-level entry points: one kernel of the network on host arrays (the kernel tests) ----

// device copies of host f32 arrays for one step-level call; everything goes back to the ctx's blocks when it ends
struct RnStep {
    vbx_ctx* ctx;
    std::vector<float*> blocks;
    explicit RnStep(vbx_ctx* c) : ctx(c) {}
    ~RnStep() {
        (void)hipStreamSynchronize(ctx->stream);
        for (float* p : blocks) ctx_free(ctx, p);
    }
    int up(const float* host, size_t count, float** dev) {
        *dev = nullptr;
        if (!host) return VBX_OK;
        const int rc = dmalloc(ctx, dev, count);
        if (rc != VBX_OK) return rc;
        blocks.push_back(*dev);
        HIPCHK(ctx, hipMemcpyAsync(*dev, host, sizeof(float) * count, hipMemcpyHostToDevice, ctx->stream));
        return VBX_OK;
    }
    // the kernel has been launched: wait for it and bring the whole in/out buffer back
    int down(const char* what, float* host, const float* dev, size_t count) {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(host, dev, sizeof(float) * count, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            ctx->err = std::string(what) + " failed: " + hipGetErrorString(e);
            return VBX_ERR_HIP;
        }
        return VBX_OK;
    }
};

extern "C" {

int vbx_resnet_destroy(vbx_resnet* net) {
    if (!net) return VBX_OK;
    vbx_ctx* ctx = net->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (void* p : {(void*)net->d_par, (void*)net->d_emb_w, (void*)net->d_emb_b, (void*)net->d_in, (void*)net->d_x[0],
                    (void*)net->d_x[1], (void*)net->d_t1, (void*)net->d_t2, (void*)net->d_sc, (void*)net->d_pool, (void*)net->d_out})
        ctx_free(ctx, p);
    for (auto& e : net->ev)
        if (e) (void)hipEventDestroy(e);
    delete net;
    return VBX_OK;
}

int vbx_resnet_create(vbx_ctx* ctx, int32_t embed_dim, const float* params, int64_t n_params, vbx_resnet** out) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!out || !params || embed_dim <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_resnet_create: bad argument");
    *out = nullptr;
    vbx_resnet* net = new vbx_resnet();
    net->ctx = ctx;
    net->E = embed_dim;
    net->Ep = round_up(embed_dim, 32);
    const size_t nconv = rn_layout(net->convs);
    const size_t want = nconv + (size_t)RN_POOL * embed_dim + embed_dim;
    if ((size_t)n_params != want) {
        delete net;
        FAIL(ctx, VBX_ERR_INVALID, "vbx_resnet_create: %lld parameters given, ResNet101 with E = %d has %zu", (long long)n_params,
             embed_dim, want);
    }
    // the embedding padded to Ep columns (zero weights and bias: the padding columns are computed and never copied out)
    const int E = embed_dim, Ep = net->Ep;
    std::vector<float> ew((size_t)RN_POOL * Ep, 0.0f), eb(Ep, 0.0f);
    for (size_t k = 0; k < (size_t)RN_POOL; ++k)
        std::memcpy(&ew[k * Ep], params + nconv + k * E, sizeof(float) * E);
    std::memcpy(eb.data(), params + nconv + (size_t)RN_POOL * E, sizeof(float) * E);
    hipError_t e = hipSetDevice(ctx->device);
    int rc = e == hipSuccess ? dmalloc(ctx, &net->d_par, nconv) : VBX_ERR_HIP;
    if (rc == VBX_OK) rc = dmalloc(ctx, &net->d_emb_w, ew.size());
    if (rc == VBX_OK) rc = dmalloc(ctx, &net->d_emb_b, eb.size());
    if (rc == VBX_OK) {
        e = hipMemcpy(net->d_par, params, sizeof(float) * nconv, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(net->d_emb_w, ew.data(), sizeof(float) * ew.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(net->d_emb_b, eb.data(), sizeof(float) * eb.size(), hipMemcpyHostToDevice);
        for (auto& ev : net->ev)
            if (e == hipSuccess) e = hipEventCreate(&ev);
    }
    if (rc == VBX_OK && e != hipSuccess) {
        ctx->err = std::string("vbx_resnet_create: ") + hipGetErrorString(e);
        rc = VBX_ERR_HIP;
    }
    if (rc != VBX_OK) {
        vbx_resnet_destroy(net);
        return rc;
    }
    *out = net;
    return VBX_OK;
}

int vbx_resnet_input(vbx_resnet* net, int32_t n, int32_t T, float** d_in) {
    if (!net) return VBX_ERR_INVALID;
    vbx_ctx* ctx = net->ctx;
    if (!d_in || n <= 0 || T <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_resnet_input: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));            // (a smaller buffer may still be read by queued work)
    const int rc = fb_reserve(ctx, &net->d_in, &net->cap_in, (size_t)n * RN_MEL * T);
    if (rc != VBX_OK) return rc;
    *d_in = net->d_in;
    return VBX_OK;
}

int vbx_resnet_run(vbx_resnet* net, int32_t n, int32_t T, const float* x, int x_on_device, float* out, int out_on_device) {
    if (!net) return VBX_ERR_INVALID;
    vbx_ctx* ctx = net->ctx;
    if (!x || !out || n <= 0 || T <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_resnet_run: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // workspace for (n, T): every block output (ping-pong), the conv1 / conv2 outputs and the shortcut, at their largest
    size_t mx = (size_t)n * RN_MEL * T * 32, mt1 = 0, mt2 = 0, msc = 0;
    {
        int H = RN_MEL, W = T;
        for (int L = 0; L < 4; ++L)
            for (int i = 0; i < RN_BLOCKS[L]; ++i) {
                const int planes = RN_PLANES[L], s = i == 0 ? RN_STRIDE[L] : 1, Ho = rn_out(H, s), Wo = rn_out(W, s);
                mt1 = std::max(mt1, (size_t)n * H * W * planes);
                mt2 = std::max(mt2, (size_t)n * Ho * Wo * planes);
                mx = std::max(mx, (size_t)n * Ho * Wo * 4 * planes);
                if (i == 0) msc = std::max(msc, (size_t)n * Ho * Wo * 4 * planes);
                H = Ho;
                W = Wo;
            }
    }
    int rc = fb_reserve(ctx, &net->d_x[0], &net->cap_x[0], mx);
    if (rc == VBX_OK) rc = fb_reserve(ctx, &net->d_x[1], &net->cap_x[1], mx);
    if (rc == VBX_OK) rc = fb_reserve(ctx, &net->d_t1, &net->cap_t1, mt1);
    if (rc == VBX_OK) rc = fb_reserve(ctx, &net->d_t2, &net->cap_t2, mt2);
    if (rc == VBX_OK) rc = fb_reserve(ctx, &net->d_sc, &net->cap_sc, msc);
    if (rc == VBX_OK) rc = fb_reserve(ctx, &net->d_pool, &net->cap_pool, (size_t)n * RN_POOL);
    if (rc == VBX_OK) rc = fb_reserve(ctx, &net->d_out, &net->cap_out, (size_t)n * net->Ep);
    if (rc == VBX_OK && !x_on_device) rc = fb_reserve(ctx, &net->d_in, &net->cap_in, (size_t)n * RN_MEL * T);
    if (rc != VBX_OK) return rc;
    const float* xin = x;
    if (!x_on_device) {
        HIPCHK(ctx, hipMemcpyAsync(net->d_in, x, sizeof(float) * (size_t)n * RN_MEL * T, hipMemcpyHostToDevice, st));
        xin = net->d_in;
    }
    const float* P = net->d_par;
    const RnConv& c0 = net->convs[0];
    HIPCHK(ctx, hipEventRecord(net->ev[0], st));
    const long long tot0 = (long long)n * RN_MEL * T * 32;
    hipLaunchKernelGGL(resnet_stem_kernel, dim3((unsigned)((tot0 + 255) / 256)), dim3(256), 0, st, xin, P + c0.w, P + c0.b,
                       net->d_x[0], T, tot0);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(net->ev[1], st));
    int cur = 0, H = RN_MEL, W = T, k = 1;
    for (int L = 0; L < 4; ++L) {
        for (int i = 0; i < RN_BLOCKS[L]; ++i) {
            const RnConv &a = net->convs[k], &b = net->convs[k + 1], &c = net->convs[k + 2];
            const float* xs = net->d_x[cur];
            float* ys = net->d_x[cur ^ 1];
            rn_conv(st, a.ks, a.stride, xs, P + a.w, P + a.b, nullptr, net->d_t1, n, H, W, a.cin, a.cout, 1);
            rn_conv(st, b.ks, b.stride, net->d_t1, P + b.w, P + b.b, nullptr, net->d_t2, n, H, W, b.cin, b.cout, 1);
            const float* res = xs;
            if (i == 0) {
                const RnConv& sc = net->convs[k + 3];
                rn_conv(st, sc.ks, sc.stride, xs, P + sc.w, P + sc.b, nullptr, net->d_sc, n, H, W, sc.cin, sc.cout, 0);
                res = net->d_sc;
            }
            H = rn_out(H, b.stride);
            W = rn_out(W, b.stride);
            rn_conv(st, c.ks, c.stride, net->d_t2, P + c.w, P + c.b, res, ys, n, H, W, c.cin, c.cout, 1);
            HIPCHK(ctx, hipGetLastError());
            k += i == 0 ? 4 : 3;
            cur ^= 1;
        }
        HIPCHK(ctx, hipEventRecord(net->ev[2 + L], st));
    }
    const long long totp = (long long)n * RN_H4 * RN_C4;
    hipLaunchKernelGGL(resnet_pool_kernel, dim3((unsigned)((totp + 255) / 256)), dim3(256), 0, st, net->d_x[cur], net->d_pool, W,
                       totp);
    rn_conv(st, 1, 1, net->d_pool, net->d_emb_w, net->d_emb_b, nullptr, net->d_out, n, 1, 1, RN_POOL, net->Ep, 0);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(net->ev[6], st));
    HIPCHK(ctx, hipMemcpy2DAsync(out, sizeof(float) * net->E, net->d_out, sizeof(float) * net->Ep, sizeof(float) * net->E, (size_t)n,
                                 out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return VBX_OK;
}

int vbx_resnet_times(vbx_resnet* net, float* ms) {
    if (!net || !ms) return VBX_ERR_INVALID;
    vbx_ctx* ctx = net->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (int i = 0; i < 6; ++i) HIPCHK(ctx, hipEventElapsedTime(&ms[i], net->ev[i], net->ev[i + 1]));
    return VBX_OK;
}

int vbx_resnet_conv_tile(int64_t M, int32_t Cout, int32_t* bn, int32_t* bm) {
    if (!bn || !bm || M <= 0 || Cout <= 0 || Cout % 32 != 0) return VBX_ERR_INVALID;
    int BN, BM;
    rn_tile(M, Cout, &BN, &BM);
    *bn = BN;
    *bm = BM;
    return VBX_OK;
}

int vbx_resnet_conv(vbx_ctx* ctx, int32_t ks, int32_t stride, int32_t n, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                    const float* x, const float* w, const float* bias, const float* res, int relu, int32_t bn, int32_t bm,
                    float* y, int64_t pad) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!x || !w || !bias || !y) FAIL(ctx, VBX_ERR_INVALID, "vbx_resnet_conv: x, w, bias and y must not be NULL");
    if (n <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || pad < 0)
        FAIL(ctx, VBX_ERR_INVALID, "vbx_resnet_conv: n = %d, H = %d, W = %d, Cin = %d, Cout = %d must be positive, pad = %lld not negative",
             n, H, W, Cin, Cout, (long long)pad);
    if ((ks != 1 && ks != 3) || (stride != 1 && stride != 2))
        FAIL(ctx, VBX_ERR_INVALID, "vbx_resnet_conv: kernel size %d stride %d: built for 1 or 3 at stride 1 or 2", ks, stride);
    if (Cin % RN_BK != 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_resnet_conv: Cin = %d is not a multiple of %d", Cin, RN_BK);
    const int Ho = rn_out(H, stride), Wo = rn_out(W, stride);
    const long long M = (long long)n * Ho * Wo;
    int BN = bn, BM = bm;
    if (bn == 0 && bm == 0) {
        if (Cout % 32 != 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_resnet_conv: Cout = %d is not a multiple of 32", Cout);
        rn_tile(M, Cout, &BN, &BM);
    } else {
        const bool built = (bn == 128 && bm == 64) || (bn == 128 && bm == 128) || (bn == 64 && bm == 64) || (bn == 64 && bm == 128) ||
                           (bn == 32 && bm == 128);
        if (!built) FAIL(ctx, VBX_ERR_INVALID, "vbx_resnet_conv: no %d x %d tile (BN x BM: 128 x 64, 128 x 128, 64 x 64, 64 x 128, 32 x 128)", bn, bm);
        if (Cout % bn != 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_resnet_conv: Cout = %d is not a multiple of the tile's BN = %d", Cout, bn);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RnStep s(ctx);
    const size_t ny = (size_t)M * Cout + 2 * (size_t)pad;
    float *dx, *dw, *db, *dr, *dy;
    int rc = s.up(x, (size_t)n * H * W * Cin, &dx);
    if (rc == VBX_OK) rc = s.up(w, (size_t)ks * ks * Cin * Cout, &dw);
    if (rc == VBX_OK) rc = s.up(bias, (size_t)Cout, &db);
    if (rc == VBX_OK) rc = s.up(res, (size_t)M * Cout, &dr);
    if (rc == VBX_OK) rc = s.up(y, ny, &dy);
    if (rc != VBX_OK) return rc;
    rn_launch(ctx->stream, ks, stride, BN, BM, dx, dw, db, dr, dy + pad, H, W, Cin, Ho, Wo, Cout, M, relu ? 1 : 0);
    return s.down("vbx_resnet_conv", y, dy, ny);
}

int vbx_resnet_stem(vbx_ctx* ctx, int32_t n, int32_t T, const float* x, const float* w, const float* bias, float* y, int64_t pad) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!x || !w || !bias || !y || n <= 0 || T <= 0 || pad < 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_resnet_stem: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RnStep s(ctx);
    const long long total = (long long)n * RN_MEL * T * 32;
    const size_t ny = (size_t)total + 2 * (size_t)pad;
    float *dx, *dw, *db, *dy;
    int rc = s.up(x, (size_t)n * RN_MEL * T, &dx);
    if (rc == VBX_OK) rc = s.up(w, 9 * 32, &dw);
    if (rc == VBX_OK) rc = s.up(bias, 32, &db);
    if (rc == VBX_OK) rc = s.up(y, ny, &dy);
    if (rc != VBX_OK) return rc;
    hipLaunchKernelGGL(resnet_stem_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, dx, dw, db, dy + pad, T,
                       total);
    return s.down("vbx_resnet_stem", y, dy, ny);
}

int vbx_resnet_pool(vbx_ctx* ctx, int32_t n, int32_t W4, const float* x, float* out, int64_t pad) {
    if (!ctx) return VBX_ERR_INVALID;
    if (!x || !out || n <= 0 || W4 <= 0 || pad < 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_resnet_pool: bad argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RnStep s(ctx);
    const long long total = (long long)n * RN_H4 * RN_C4;
    const size_t ny = (size_t)n * RN_POOL + 2 * (size_t)pad;
    float *dx, *dy;
    int rc = s.up(x, (size_t)total * W4, &dx);
    if (rc == VBX_OK) rc = s.up(out, ny, &dy);
    if (rc != VBX_OK) return rc;
    hipLaunchKernelGGL(resnet_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, dx, dy + pad, W4, total);
    return s.down("vbx_resnet_pool", out, dy, ny);
}

}  // extern "C"
