// vbx_host_resnet.hpp -- host runtime of the x-vector network (vbx_resnet.hpp): the folded parameters, the workspace and the
// launch sequence of one batch of windows.  Included by vbx_capi.hip after vbx_host_fbank.hpp (fb_reserve).
//
// A batch's shape exists once, as an RnBatch (rn_batch builds it from one T or from T[]), for a run, for a convolution step
// and for a stem or pooling step alike; whether it is uniform or ragged becomes the kernels' RAG in rn_by_kind and nowhere
// else.
//
// Parameter blob (f32, vbx_amd/xvector.py:fold writes it in this order): for every convolution in network order -- the
// stem, then per block conv1, conv2, conv3 and, in the first block of a stage, the shortcut -- its weights [kh kw Cin][Cout]
// and its folded bias [Cout]; then the embedding [16384][E] (rows in the pooling kernel's order) and its bias [E].

struct RnConv {
    int ks, stride, cin, cout;
    size_t w, b;                                               // offsets into the parameter blob
    size_t wf = 0, we = 0;                                     // split mode: offsets (h8 units, ints) of the fragments and exponents
};

// one convolution of the launch sequence of a run (rn_plan)
enum RnBuf { RN_X0, RN_X1, RN_T1, RN_T2, RN_SC, RN_NBUF };     // the block outputs (ping-pong), conv1 / conv2 outputs, the shortcut
struct RnPlanStep {
    int conv;                                                  // index into vbx_resnet::convs
    int in, out, res;                                          // RnBuf; res: RN_NBUF for none
    int lvl, relu;                                             // the input's level (RnBatch); the output's: + 1 at stride 2
    int ain, aout;                                             // split mode: the max |.| slots of its input and (or -1) its output
    int stage;                                                 // 0 .. 3: layer1 .. layer4 (the events)
};

struct vbx_resnet {
    vbx_ctx* ctx = nullptr;
    int E = 0, Ep = 0;                                         // embedding width, padded to 32 columns on the device
    std::vector<RnConv> convs;                                 // [0] the stem, then 3 or 4 per block
    std::vector<RnPlanStep> plan;                              // the launch sequence (rn_plan)
    float *d_par = nullptr, *d_emb_w = nullptr, *d_emb_b = nullptr;
    float *d_in = nullptr, *d_buf[RN_NBUF] = {}, *d_pool = nullptr, *d_out = nullptr;
    size_t cap_in = 0, cap_buf[RN_NBUF] = {}, cap_pool = 0, cap_out = 0;
    hipEvent_t ev[7] = {};                                     // stem | layer1 | layer2 | layer3 | layer4 | pool + embedding
    // split mode (vbx_resnet_split.hpp): the weights a second time as f16 pairs in fragment order, their per-channel
    // exponents, and one max |y| slot per window for every tensor a split convolution reads
    int gemm = VBX_GEMM_EXACT, gemm_last = VBX_GEMM_EXACT;
    vbx::h8* d_wf = nullptr;
    int* d_we = nullptr;
    unsigned* d_amax = nullptr;
    size_t cap_amax = 0;
    long long* d_pos = nullptr;                                // ragged runs: RnBatch's tables
    int* d_wid = nullptr;
    size_t cap_pos = 0, cap_wid = 0;
};

constexpr int RN_BLOCKS[4] = {3, 4, 23, 3}, RN_PLANES[4] = {32, 64, 128, 256}, RN_STRIDE[4] = {1, 2, 2, 2};
constexpr int RN_NBLOCKS = RN_BLOCKS[0] + RN_BLOCKS[1] + RN_BLOCKS[2] + RN_BLOCKS[3];
constexpr int RN_AMAX_SLOTS = 1 + 3 * RN_NBLOCKS;              // the stem's output, then conv1, conv2 and the output of every block

static inline int rn_out(int n, int stride) { return (n - 1) / stride + 1; }

// the Bottleneck blocks in network order: f(stage, Cin, planes, stride, first of its stage).  The stride sits on conv2; the
// first block of a stage has the shortcut convolution.
template <class F> static void rn_for_blocks(F f) {
    int cin = 32;
    for (int L = 0; L < 4; ++L)
        for (int i = 0; i < RN_BLOCKS[L]; ++i) {
            f(L, cin, RN_PLANES[L], i == 0 ? RN_STRIDE[L] : 1, i == 0);
            cin = 4 * RN_PLANES[L];
        }
}

// the network's convolutions in blob order; returns the number of f32 parameters before the embedding
static size_t rn_layout(std::vector<RnConv>& convs) {
    size_t off = 0;
    auto add = [&](int ks, int stride, int cin, int cout) {
        RnConv c{ks, stride, cin, cout, off, off + (size_t)ks * ks * cin * cout};
        off = c.b + cout;
        convs.push_back(c);
    };
    add(3, 1, 1, 32);
    rn_for_blocks([&](int, int cin, int planes, int s, bool first) {
        add(1, 1, cin, planes);
        add(3, s, planes, planes);
        add(1, 1, planes, 4 * planes);
        if (first) add(1, s, cin, 4 * planes);
    });
    return off;
}

// The geometry of a batch of n windows, the only one there is: at level l every window has H[l] rows and the batch M[l]
// positions in all.  Uniform: every window is W[l] wide.  Ragged: window b is wid[l n + b] wide and its [H_l][W_{b,l}][C]
// block starts at position pos[l (n + 1) + b]; pos[l (n + 1) + n] = M[l] (vbx_amd/xvector.py: ragged_layout is the same in
// numpy).  A run has the network's four levels, a convolution step its input and its output, a stem or pooling step one.
constexpr int RN_LEVELS = 4;
struct RnBatch {
    int n = 0;
    bool ragged = false;
    int H[RN_LEVELS] = {}, W[RN_LEVELS] = {};                  // (W: zero in a ragged batch)
    long long M[RN_LEVELS] = {};
    std::vector<long long> pos;                                // ragged: [levels][n + 1]
    std::vector<int> wid;                                      // [levels][n]
    const long long* d_pos = nullptr;                          // their device copies
    const int* d_wid = nullptr;
    // the kernels' view of level l, and of a convolution from level li to level lo
    template <bool RAG> RnLevel<RAG> level(int l) const {
        if constexpr (RAG) return {d_pos + (size_t)l * (n + 1), d_wid + (size_t)l * n, n};
        else return {W[l]};
    }
    template <bool RAG> RnGeom<RAG> conv(int li, int lo) const {
        if constexpr (RAG) return {RnRag{level<true>(li).pos, level<true>(lo).pos, level<true>(li).wid, level<true>(lo).wid, n}};
        else return {};
    }
};

// n windows of H rows, all of them T wide or (Tv not null) window b Tv[b] wide, at `levels` levels: every level is
// rn_out(., stride) of the one before it in rows and in widths
static RnBatch rn_batch(int n, int H, int T, const int32_t* Tv, int levels, int stride = 2) {
    RnBatch g;
    g.n = n;
    g.ragged = Tv != nullptr;
    if (g.ragged) {
        g.pos.assign((size_t)levels * (n + 1), 0);
        g.wid.resize((size_t)levels * n);
    }
    for (int l = 0; l < levels; ++l) {
        g.H[l] = l == 0 ? H : rn_out(g.H[l - 1], stride);
        if (g.ragged) {
            long long* pos = &g.pos[(size_t)l * (n + 1)];
            for (int b = 0; b < n; ++b) {
                const int W = l == 0 ? Tv[b] : rn_out(g.wid[(size_t)(l - 1) * n + b], stride);
                g.wid[(size_t)l * n + b] = W;
                pos[b + 1] = pos[b] + (long long)g.H[l] * W;
            }
            g.M[l] = pos[n];
        } else {
            g.W[l] = l == 0 ? T : rn_out(g.W[l - 1], stride);
            g.M[l] = (long long)n * g.H[l] * g.W[l];
        }
    }
    return g;
}

// f(std::true_type) for a ragged batch, f(std::false_type) for a uniform one: the one place where a batch's kind becomes
// the kernels' RAG
template <class F> static void rn_by_kind(const RnBatch& g, F f) {
    if (g.ragged) f(std::true_type{});
    else f(std::false_type{});
}

// the convolutions of layer1 .. layer4 in launch order: per block conv1, conv2, the shortcut (from the block's input),
// conv3 + residual.  Slots: 3 blk the block's input, then conv1, conv2, the output.
static std::vector<RnPlanStep> rn_plan() {
    std::vector<RnPlanStep> plan;
    int lvl = 0, k = 1, x = RN_X0, s0 = 0;
    rn_for_blocks([&](int L, int, int, int s, bool first) {
        const int y = x == RN_X0 ? RN_X1 : RN_X0;
        plan.push_back({k, x, RN_T1, RN_NBUF, lvl, 1, s0, s0 + 1, L});
        plan.push_back({k + 1, RN_T1, RN_T2, RN_NBUF, lvl, 1, s0 + 1, s0 + 2, L});
        if (first) plan.push_back({k + 3, x, RN_SC, RN_NBUF, lvl, 0, s0, -1, L});
        lvl += s == 2;
        plan.push_back({k + 2, RN_T2, y, first ? RN_SC : x, lvl, 1, s0 + 2, s0 + 3, L});
        k += first ? 4 : 3;
        x = y;
        s0 += 3;
    });
    return plan;
}

// one call of a convolution kernel: the batch g from its level li to its level lo, Cin -> Cout channels (Cout a multiple of
// 32, Cin of 16).  Plain values.
struct RnCall {
    int ks, stride, Cin, Cout, relu;
    const RnBatch* g;
    int li, lo;
    const float *x = nullptr, *w = nullptr, *b = nullptr, *res = nullptr;      // w: the exact mode's weights
    float* y = nullptr;
    const unsigned* ax = nullptr;                              // split mode: the max |.| slots of x and (or null) of y,
    unsigned* ay = nullptr;
    const vbx::h8* wf = nullptr;                               // the weights' fragments and exponents
    const int* we = nullptr;
    long long M() const { return g->M[lo]; }                   // output positions
};

static RnCall rn_call(const RnConv& c, int relu, const RnBatch& g, int li, int lo) {
    return RnCall{c.ks, c.stride, c.cin, c.cout, relu, &g, li, lo};
}

// the instantiations of both convolution kernels: every (KS, S) at every BN x BM tile
constexpr int RN_KS_STRIDE[4][2] = {{1, 1}, {1, 2}, {3, 1}, {3, 2}};
constexpr int RN_TILES[5][2] = {{128, 64}, {128, 128}, {64, 64}, {64, 128}, {32, 128}};

static bool rn_tile_built(int bn, int bm) {
    for (const auto& t : RN_TILES)
        if (t[0] == bn && t[1] == bm) return true;
    return false;
}

// launches c with the BN x BM tile in the exact or the split mode; false (nothing launched) where no such kernel is built
template <int I = 0> static bool rn_launch(hipStream_t st, const RnCall& c, int BN, int BM, int mode) {
    if constexpr (I < 20) {
        constexpr int KS = RN_KS_STRIDE[I / 5][0], S = RN_KS_STRIDE[I / 5][1], bn = RN_TILES[I % 5][0], bm = RN_TILES[I % 5][1];
        if (c.ks != KS || c.stride != S || BN != bn || BM != bm) return rn_launch<I + 1>(st, c, BN, BM, mode);
        const RnBatch& g = *c.g;
        const int H = g.H[c.li], W = g.W[c.li], Ho = g.H[c.lo], Wo = g.W[c.lo];
        const long long M = c.M();
        const dim3 grid((unsigned)((M + bm - 1) / bm), (unsigned)(c.Cout / bn)), blk(256);
        rn_by_kind(g, [&](auto rag) {
            constexpr bool RAG = decltype(rag)::value;
            if (mode == VBX_GEMM_SPLIT)
                hipLaunchKernelGGL((resnet_conv_split_kernel<KS, S, bn, bm, RAG>), grid, blk, 0, st, c.x, c.ax, c.wf, c.we, c.b, c.res,
                                   c.y, c.ay, H, W, c.Cin, Ho, Wo, c.Cout, M, c.relu, g.conv<RAG>(c.li, c.lo));
            else
                hipLaunchKernelGGL((resnet_conv_kernel<KS, S, bn, bm, RAG>), grid, blk, 0, st, c.x, c.w, c.b, c.res, c.y, H, W, c.Cin,
                                   Ho, Wo, c.Cout, M, c.relu, g.conv<RAG>(c.li, c.lo));
        });
        return true;
    }
    return false;
}

// the stem over the batch g (level 0): x g.M[0] floats -> y [g.M[0]][32]
static void rn_stem(hipStream_t st, const RnBatch& g, const float* x, const float* w, const float* b, float* y) {
    const long long total = g.M[0] * 32;
    rn_by_kind(g, [&](auto rag) {
        hipLaunchKernelGGL(resnet_stem_kernel<decltype(rag)::value>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, w, b, y,
                           total, g.level<decltype(rag)::value>(0));
    });
}

// the pooling of level l of g (RN_H4 rows, RN_C4 channels): x -> out [n][RN_POOL]
static void rn_pool(hipStream_t st, const RnBatch& g, int l, const float* x, float* out) {
    const long long total = (long long)g.n * RN_H4 * RN_C4;
    rn_by_kind(g, [&](auto rag) {
        hipLaunchKernelGGL(resnet_pool_kernel<decltype(rag)::value>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, out,
                           total, g.level<decltype(rag)::value>(l));
    });
}

// max |x| per window of level l of g with C channels (a multiple of 4) into amax[n], zeroed beforehand.  Blocks per window
// from a window's floats: what every window has in a uniform batch, the mean in a ragged one.  (M / n is exact in a uniform
// batch, H W, and at least one float4 there, so the max(1, .) never bites: the grids of both kinds are what they were.)
static void rn_amax(hipStream_t st, const RnBatch& g, int l, int C, const float* x, unsigned* amax) {
    const int bpw = (int)std::max<long long>(1, std::min<long long>(64, (g.M[l] / g.n * C / 4 + 255) / 256));
    rn_by_kind(g, [&](auto rag) {
        hipLaunchKernelGGL(resnet_amax_kernel<decltype(rag)::value>, dim3((unsigned)g.n * bpw), dim3(256), 0, st, x, g.H[l], C, bpw,
                           amax, g.level<decltype(rag)::value>(l));
    });
}

// w [K][Cout] f32 (K a multiple of 16, Cout of 32) -> frag [K / 16][Cout / 32][hi | lo][64][8] f16 bits, e [Cout]: the B
// operand of vbx_resnet_split.hpp, one power-of-two scale per output channel (vbx_amd/xvector.py: pack_split_weights is the
// same in numpy)
static void rn_split_weights(const float* w, int K, int Cout, uint16_t* frag, int32_t* e) {
    for (int n = 0; n < Cout; ++n) {
        float amax = 0.0f;
        for (int k = 0; k < K; ++k) {
            const float a = std::fabs(w[(size_t)k * Cout + n]);
            if (a > amax) amax = a;                            // (a NaN does not count)
        }
        int ex = 0;
        if (amax > 0.0f && amax < INFINITY) {
            (void)std::frexp(amax, &ex);
            ex = std::max(-100, std::min(100, vbx::kSplitTop - ex));
        }
        e[n] = ex;
    }
    const int CBT = Cout / 32;
    for (int k = 0; k < K; ++k)
        for (int n = 0; n < Cout; ++n) {
            const float v = std::ldexp(w[(size_t)k * Cout + n], e[n]);
            const _Float16 hi = (_Float16)v, lo = (_Float16)(v - (float)hi);
            const size_t lane = 32 * ((k & 15) >> 3) + (n & 31);
            const size_t o = (((size_t)(k >> 4) * CBT + (n >> 5)) * 2 * 64 + lane) * 8 + (k & 7);
            std::memcpy(&frag[o], &hi, 2);
            std::memcpy(&frag[o + 64 * 8], &lo, 2);
        }
}

// the BN x BM output tile of a convolution of M output positions x Cout channels (Cout a multiple of 32)
static void rn_tile(long long M, int Cout, int* bn, int* bm) {
    // (a few rows -- the embedding -- take narrow tiles: more workgroups over its long K)
    *bn = M < 4096 ? 32 : Cout % 128 == 0 ? 128 : Cout % 64 == 0 ? 64 : 32;
    // 64-row tiles where 128-row ones leave fewer than four workgroups per CU (layer3 and layer4 at 128 windows)
    *bm = *bn >= 64 && (M + 127) / 128 * (Cout / *bn) < 1024 ? 64 : 128;
}

// one convolution at the dispatcher's tile
static bool rn_conv(hipStream_t st, const RnCall& c, int mode) {
    int BN, BM;
    rn_tile(c.M(), c.Cout, &BN, &BM);
    return rn_launch(st, c, BN, BM, mode);
}

// the split mode needs a library whose device code went through the ISA audit (vbx_amd/build.py)
static int rn_check_gemm(vbx_ctx* ctx, const char* name, int gemm) {
    if (gemm != VBX_GEMM_EXACT && gemm != VBX_GEMM_SPLIT) FAIL(ctx, VBX_ERR_INVALID, "%s: gemm must be VBX_GEMM_EXACT or VBX_GEMM_SPLIT", name);
#ifdef VBX_ISA_UNAUDITED
    if (gemm == VBX_GEMM_SPLIT)
        FAIL(ctx, VBX_ERR_UNSUPPORTED, "%s: VBX_GEMM_SPLIT: this library was built without the ISA audit (vbx_amd/build.py); rebuild with llvm-objdump available", name);
#endif
    return VBX_OK;
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
    template <class T> int up(const float* host, size_t count, T** dev) {     // (a null host array: a null device one)
        *dev = nullptr;
        return host ? up_bytes(host, sizeof(float) * count, dev) : VBX_OK;
    }
    template <class T> int up_bytes(const void* host, size_t bytes, T** dev) {   // (a null host array: zeros)
        void* p = nullptr;
        *dev = nullptr;
        const int rc = dmalloc_bytes(ctx, &p, std::max<size_t>(bytes, 4));
        if (rc != VBX_OK) return rc;
        blocks.push_back((float*)p);
        *dev = (T*)p;
        if (host) HIPCHK(ctx, hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, ctx->stream));
        else HIPCHK(ctx, hipMemsetAsync(p, 0, bytes, ctx->stream));
        return VBX_OK;
    }
    int tables(RnBatch& g) {                                   // a ragged batch's tables
        if (!g.ragged) return VBX_OK;
        long long* dpos = nullptr;
        int* dwid = nullptr;
        int rc = up_bytes(g.pos.data(), sizeof(long long) * g.pos.size(), &dpos);
        if (rc == VBX_OK) rc = up_bytes(g.wid.data(), sizeof(int) * g.wid.size(), &dwid);
        g.d_pos = dpos;
        g.d_wid = dwid;
        return rc;
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

// n and T of a ragged call
static int rn_check_lengths(vbx_ctx* ctx, const char* name, int32_t n, const int32_t* T) {
    if (n <= 0) FAIL(ctx, VBX_ERR_INVALID, "%s: n = %d windows, need at least one", name, n);
    if (!T) FAIL(ctx, VBX_ERR_INVALID, "%s: T must not be NULL", name);
    for (int b = 0; b < n; ++b)
        if (T[b] <= 0) FAIL(ctx, VBX_ERR_INVALID, "%s: window %d has T = %d frames, need at least 1", name, b, T[b]);
    return VBX_OK;
}

// ragged: g's tables to the device (the stream is idle between runs: every run ends with a synchronize)
static int rn_upload_tables(vbx_resnet* net, RnBatch& g) {
    vbx_ctx* ctx = net->ctx;
    int rc = fb_reserve(ctx, &net->d_pos, &net->cap_pos, g.pos.size());
    if (rc == VBX_OK) rc = fb_reserve(ctx, &net->d_wid, &net->cap_wid, g.wid.size());
    if (rc != VBX_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(net->d_pos, g.pos.data(), sizeof(long long) * g.pos.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(net->d_wid, g.wid.data(), sizeof(int) * g.wid.size(), hipMemcpyHostToDevice, ctx->stream));
    g.d_pos = net->d_pos;
    g.d_wid = net->d_wid;
    return VBX_OK;
}

// the network over the batch g (four levels), uniform or ragged: x is g.M[0] floats (the windows' [64][T] blocks)
static int rn_run(vbx_resnet* net, const char* name, RnBatch& g, const float* x, int x_on_device, float* out, int out_on_device) {
    vbx_ctx* ctx = net->ctx;
    const int n = g.n;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // workspace: every buffer at the largest output a step writes to it, the ping-pong pair alike (x[0] also takes the
    // stem's output)
    size_t need[RN_NBUF] = {(size_t)g.M[0] * 32};
    for (const RnPlanStep& s : net->plan) {
        const RnConv& c = net->convs[s.conv];
        need[s.out] = std::max(need[s.out], (size_t)g.M[s.lvl + (c.stride == 2)] * c.cout);
    }
    need[RN_X0] = need[RN_X1] = std::max(need[RN_X0], need[RN_X1]);
    int rc = VBX_OK;
    for (int i = 0; i < RN_NBUF && rc == VBX_OK; ++i) rc = fb_reserve(ctx, &net->d_buf[i], &net->cap_buf[i], need[i]);
    if (rc == VBX_OK) rc = fb_reserve(ctx, &net->d_pool, &net->cap_pool, (size_t)n * RN_POOL);
    if (rc == VBX_OK) rc = fb_reserve(ctx, &net->d_out, &net->cap_out, (size_t)n * net->Ep);
    if (rc == VBX_OK && !x_on_device) rc = fb_reserve(ctx, &net->d_in, &net->cap_in, (size_t)g.M[0]);
    const bool split = net->gemm == VBX_GEMM_SPLIT;
    if (rc == VBX_OK && split) rc = fb_reserve(ctx, &net->d_amax, &net->cap_amax, (size_t)RN_AMAX_SLOTS * n);
    if (rc == VBX_OK && g.ragged) rc = rn_upload_tables(net, g);
    if (rc != VBX_OK) return rc;
    net->gemm_last = net->gemm;
    if (split) HIPCHK(ctx, hipMemsetAsync(net->d_amax, 0, sizeof(unsigned) * RN_AMAX_SLOTS * (size_t)n, st));
    auto slot = [&](int s) { return split && s >= 0 ? net->d_amax + (size_t)s * n : nullptr; };
    const float* xin = x;
    if (!x_on_device) {
        HIPCHK(ctx, hipMemcpyAsync(net->d_in, x, sizeof(float) * (size_t)g.M[0], hipMemcpyHostToDevice, st));
        xin = net->d_in;
    }
    const float* P = net->d_par;
    const RnConv& c0 = net->convs[0];
    HIPCHK(ctx, hipEventRecord(net->ev[0], st));
    rn_stem(st, g, xin, P + c0.w, P + c0.b, net->d_buf[RN_X0]);
    if (split) rn_amax(st, g, 0, 32, net->d_buf[RN_X0], slot(0));  // (the stem itself stays as it is)
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(net->ev[1], st));
    int stage = 0;
    for (const RnPlanStep& s : net->plan) {
        if (s.stage != stage) HIPCHK(ctx, hipEventRecord(net->ev[2 + stage], st));
        stage = s.stage;
        const RnConv& c = net->convs[s.conv];
        RnCall call = rn_call(c, s.relu, g, s.lvl, s.lvl + (c.stride == 2));
        call.x = net->d_buf[s.in];
        call.w = P + c.w;
        call.b = P + c.b;
        call.res = s.res == RN_NBUF ? nullptr : net->d_buf[s.res];
        call.y = net->d_buf[s.out];
        call.ax = slot(s.ain);
        call.wf = net->d_wf + c.wf;
        call.we = net->d_we + c.we;
        call.ay = slot(s.aout);
        if (!rn_conv(st, call, net->gemm)) FAIL(ctx, VBX_ERR_INVALID, "%s: no kernel for convolution %d", name, s.conv);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(net->ev[2 + stage], st));
    const RnPlanStep& last = net->plan.back();
    rn_pool(st, g, RN_LEVELS - 1, net->d_buf[last.out], net->d_pool);
    const RnBatch rows = rn_batch(n, 1, 1, nullptr, 1);        // the embedding: n positions; exact in both modes
    RnCall emb = rn_call(RnConv{1, 1, RN_POOL, net->Ep}, 0, rows, 0, 0);
    emb.x = net->d_pool;
    emb.w = net->d_emb_w;
    emb.b = net->d_emb_b;
    emb.y = net->d_out;
    rn_conv(st, emb, VBX_GEMM_EXACT);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(net->ev[6], st));
    HIPCHK(ctx, hipMemcpy2DAsync(out, sizeof(float) * net->E, net->d_out, sizeof(float) * net->Ep, sizeof(float) * net->E, (size_t)n,
                                 out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return VBX_OK;
}

// vbx_resnet_stem and vbx_resnet_stem_ragged: the stem on host arrays
static int rn_stem_step(const char* name, vbx_ctx* ctx, bool ragged, int32_t n, int32_t T, const int32_t* Tv, const float* x,
                        const float* w, const float* bias, float* y, int64_t pad) {
    if (!ctx) return VBX_ERR_INVALID;
    int rc = ragged ? rn_check_lengths(ctx, name, n, Tv) : VBX_OK;
    if (rc != VBX_OK) return rc;
    const bool ok = x && w && bias && y && pad >= 0;
    if (ragged && !ok) FAIL(ctx, VBX_ERR_INVALID, "%s: x, w, bias and y must not be NULL, pad not negative", name);
    if (!ragged && (!ok || n <= 0 || T <= 0)) FAIL(ctx, VBX_ERR_INVALID, "%s: bad argument", name);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RnBatch g = rn_batch(n, RN_MEL, T, Tv, 1);                 // (outlives s and its copies)
    RnStep s(ctx);
    const size_t ny = (size_t)g.M[0] * 32 + 2 * (size_t)pad;
    float *dx, *dw, *db, *dy;
    rc = s.up(x, (size_t)g.M[0], &dx);
    if (rc == VBX_OK) rc = s.up(w, 9 * 32, &dw);
    if (rc == VBX_OK) rc = s.up(bias, 32, &db);
    if (rc == VBX_OK) rc = s.up(y, ny, &dy);
    if (rc == VBX_OK) rc = s.tables(g);
    if (rc != VBX_OK) return rc;
    rn_stem(ctx->stream, g, dx, dw, db, dy + pad);
    return s.down(name, y, dy, ny);
}

// vbx_resnet_pool and vbx_resnet_pool_ragged: the pooling on host arrays
static int rn_pool_step(const char* name, vbx_ctx* ctx, bool ragged, int32_t n, int32_t W4, const int32_t* W4v, const float* x,
                        float* out, int64_t pad) {
    if (!ctx) return VBX_ERR_INVALID;
    int rc = ragged ? rn_check_lengths(ctx, name, n, W4v) : VBX_OK;
    if (rc != VBX_OK) return rc;
    const bool ok = x && out && pad >= 0;
    if (ragged && !ok) FAIL(ctx, VBX_ERR_INVALID, "%s: x and out must not be NULL, pad not negative", name);
    if (!ragged && (!ok || n <= 0 || W4 <= 0)) FAIL(ctx, VBX_ERR_INVALID, "%s: bad argument", name);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RnBatch g = rn_batch(n, RN_H4, W4, W4v, 1);                // (outlives s and its copies)
    RnStep s(ctx);
    const size_t ny = (size_t)n * RN_POOL + 2 * (size_t)pad;
    float *dx, *dy;
    rc = s.up(x, (size_t)g.M[0] * RN_C4, &dx);
    if (rc == VBX_OK) rc = s.up(out, ny, &dy);
    if (rc == VBX_OK) rc = s.tables(g);
    if (rc != VBX_OK) return rc;
    rn_pool(ctx->stream, g, 0, dx, dy + pad);
    return s.down(name, out, dy, ny);
}

extern "C" {

int vbx_resnet_destroy(vbx_resnet* net) {
    if (!net) return VBX_OK;
    vbx_ctx* ctx = net->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (void* p : {(void*)net->d_par, (void*)net->d_emb_w, (void*)net->d_emb_b, (void*)net->d_in, (void*)net->d_pool,
                    (void*)net->d_out, (void*)net->d_wf, (void*)net->d_we, (void*)net->d_amax, (void*)net->d_pos, (void*)net->d_wid})
        ctx_free(ctx, p);
    for (float* p : net->d_buf) ctx_free(ctx, p);
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
    net->plan = rn_plan();
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
    // the split mode's copy of every convolution but the stem
    size_t nwf = 0, nwe = 0;
    for (size_t k = 1; k < net->convs.size(); ++k) {
        RnConv& c = net->convs[k];
        c.wf = nwf;
        c.we = nwe;
        nwf += (size_t)c.ks * c.ks * c.cin * c.cout / 4;       // two halfs per weight, eight per unit
        nwe += c.cout;
    }
    std::vector<uint16_t> wf(nwf * 8);
    std::vector<int32_t> we(nwe);
    for (size_t k = 1; k < net->convs.size(); ++k) {
        const RnConv& c = net->convs[k];
        rn_split_weights(params + c.w, c.ks * c.ks * c.cin, c.cout, &wf[c.wf * 8], &we[c.we]);
    }
    hipError_t e = hipSetDevice(ctx->device);
    int rc = e == hipSuccess ? dmalloc(ctx, &net->d_par, nconv) : VBX_ERR_HIP;
    if (rc == VBX_OK) rc = dmalloc(ctx, &net->d_wf, nwf);
    if (rc == VBX_OK) rc = dmalloc(ctx, &net->d_we, nwe);
    if (rc == VBX_OK) rc = dmalloc(ctx, &net->d_emb_w, ew.size());
    if (rc == VBX_OK) rc = dmalloc(ctx, &net->d_emb_b, eb.size());
    if (rc == VBX_OK) {
        e = hipMemcpy(net->d_par, params, sizeof(float) * nconv, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(net->d_emb_w, ew.data(), sizeof(float) * ew.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(net->d_emb_b, eb.data(), sizeof(float) * eb.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(net->d_wf, wf.data(), sizeof(uint16_t) * wf.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(net->d_we, we.data(), sizeof(int32_t) * we.size(), hipMemcpyHostToDevice);
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

// the network's own input buffer at `floats` or more
static int rn_input(vbx_resnet* net, size_t floats, float** d_in) {
    vbx_ctx* ctx = net->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));            // (a smaller buffer may still be read by queued work)
    const int rc = fb_reserve(ctx, &net->d_in, &net->cap_in, floats);
    if (rc != VBX_OK) return rc;
    *d_in = net->d_in;
    return VBX_OK;
}

int vbx_resnet_input(vbx_resnet* net, int32_t n, int32_t T, float** d_in) {
    if (!net) return VBX_ERR_INVALID;
    if (!d_in || n <= 0 || T <= 0) FAIL(net->ctx, VBX_ERR_INVALID, "vbx_resnet_input: bad argument");
    return rn_input(net, (size_t)n * RN_MEL * T, d_in);
}

int vbx_resnet_input_ragged(vbx_resnet* net, int32_t n, const int32_t* T, float** d_in) {
    if (!net) return VBX_ERR_INVALID;
    const int rc = rn_check_lengths(net->ctx, "vbx_resnet_input_ragged", n, T);
    if (rc != VBX_OK) return rc;
    if (!d_in) FAIL(net->ctx, VBX_ERR_INVALID, "vbx_resnet_input_ragged: d_in must not be NULL");
    size_t frames = 0;
    for (int b = 0; b < n; ++b) frames += (size_t)T[b];
    return rn_input(net, frames * RN_MEL, d_in);
}

int vbx_resnet_run(vbx_resnet* net, int32_t n, int32_t T, const float* x, int x_on_device, float* out, int out_on_device) {
    if (!net) return VBX_ERR_INVALID;
    vbx_ctx* ctx = net->ctx;
    if (!x || !out || n <= 0 || T <= 0) FAIL(ctx, VBX_ERR_INVALID, "vbx_resnet_run: bad argument");
    RnBatch g = rn_batch(n, RN_MEL, T, nullptr, RN_LEVELS);
    return rn_run(net, "vbx_resnet_run", g, x, x_on_device, out, out_on_device);
}

int vbx_resnet_run_ragged(vbx_resnet* net, int32_t n, const int32_t* T, const float* x, int x_on_device, float* out,
                          int out_on_device) {
    if (!net) return VBX_ERR_INVALID;
    vbx_ctx* ctx = net->ctx;
    const int rc = rn_check_lengths(ctx, "vbx_resnet_run_ragged", n, T);
    if (rc != VBX_OK) return rc;
    if (!x || !out) FAIL(ctx, VBX_ERR_INVALID, "vbx_resnet_run_ragged: x and out must not be NULL");
    RnBatch g = rn_batch(n, RN_MEL, 0, T, RN_LEVELS);
    return rn_run(net, "vbx_resnet_run_ragged", g, x, x_on_device, out, out_on_device);
}

int vbx_resnet_times(vbx_resnet* net, float* ms) {
    if (!net || !ms) return VBX_ERR_INVALID;
    vbx_ctx* ctx = net->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (int i = 0; i < 6; ++i) HIPCHK(ctx, hipEventElapsedTime(&ms[i], net->ev[i], net->ev[i + 1]));
    return VBX_OK;
}

int vbx_resnet_set_gemm(vbx_resnet* net, int gemm) {
    if (!net) return VBX_ERR_INVALID;
    const int rc = rn_check_gemm(net->ctx, "vbx_resnet_set_gemm", gemm);
    if (rc != VBX_OK) return rc;
    net->gemm = gemm;
    return VBX_OK;
}

int vbx_resnet_gemm_in_effect(vbx_resnet* net) { return net ? net->gemm_last : VBX_ERR_INVALID; }

int vbx_resnet_split_weights(int32_t K, int32_t Cout, const float* w, uint16_t* frag, int32_t* e) {
    if (!w || !frag || !e || K <= 0 || Cout <= 0 || K % 16 != 0 || Cout % 32 != 0) return VBX_ERR_INVALID;
    rn_split_weights(w, K, Cout, frag, e);
    return VBX_OK;
}

int vbx_resnet_conv_tile(int64_t M, int32_t Cout, int32_t* bn, int32_t* bm) {
    if (!bn || !bm || M <= 0 || Cout <= 0 || Cout % 32 != 0) return VBX_ERR_INVALID;
    rn_tile(M, Cout, bn, bm);
    return VBX_OK;
}

// vbx_resnet_conv, vbx_resnet_conv_gemm and vbx_resnet_conv_ragged: one convolution on host arrays in either mode; Wv: the
// windows' widths of a ragged batch, or null (then all of them W wide)
static int rn_conv_step(const char* name, vbx_ctx* ctx, int gemm, int32_t ks, int32_t stride, int32_t n, int32_t H, int32_t W,
                        const int32_t* Wv, int32_t Cin, int32_t Cout, const float* x, const float* w, const float* bias, const float* res, int relu,
                        int32_t bn, int32_t bm, float* y, int64_t pad, float* amax_y) {
    if (!ctx) return VBX_ERR_INVALID;
    int rc = rn_check_gemm(ctx, name, gemm);
    if (rc != VBX_OK) return rc;
    if (!x || !w || !bias || !y) FAIL(ctx, VBX_ERR_INVALID, "%s: x, w, bias and y must not be NULL", name);
    if (n <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || pad < 0)
        FAIL(ctx, VBX_ERR_INVALID, "%s: n = %d, H = %d, W = %d, Cin = %d, Cout = %d must be positive, pad = %lld not negative", name,
             n, H, W, Cin, Cout, (long long)pad);
    if ((ks != 1 && ks != 3) || (stride != 1 && stride != 2))
        FAIL(ctx, VBX_ERR_INVALID, "%s: kernel size %d stride %d: built for 1 or 3 at stride 1 or 2", name, ks, stride);
    if (Cin % RN_BK != 0) FAIL(ctx, VBX_ERR_INVALID, "%s: Cin = %d is not a multiple of %d", name, Cin, RN_BK);
    RnBatch g = rn_batch(n, H, W, Wv, 2, stride);              // (outlives the copies, as wf and we below)
    RnCall c = rn_call(RnConv{ks, stride, Cin, Cout}, relu ? 1 : 0, g, 0, 1);
    const size_t nx = (size_t)g.M[0] * Cin;
    int BN = bn, BM = bm;
    if (bn == 0 && bm == 0) {
        if (Cout % 32 != 0) FAIL(ctx, VBX_ERR_INVALID, "%s: Cout = %d is not a multiple of 32", name, Cout);
        rn_tile(c.M(), Cout, &BN, &BM);
    } else {
        if (!rn_tile_built(bn, bm)) FAIL(ctx, VBX_ERR_INVALID, "%s: no BN x BM = %d x %d tile is built (RN_TILES)", name, bn, bm);
        if (Cout % bn != 0) FAIL(ctx, VBX_ERR_INVALID, "%s: Cout = %d is not a multiple of the tile's BN = %d", name, Cout, bn);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RnStep s(ctx);
    const size_t ny = (size_t)c.M() * Cout + 2 * (size_t)pad;
    float* dy;
    rc = s.up(x, nx, &c.x);
    if (rc == VBX_OK) rc = s.tables(g);
    if (rc == VBX_OK) rc = s.up(bias, (size_t)Cout, &c.b);
    if (rc == VBX_OK) rc = s.up(res, (size_t)c.M() * Cout, &c.res);
    if (rc == VBX_OK) rc = s.up(y, ny, &dy);
    if (rc == VBX_OK && gemm == VBX_GEMM_EXACT) rc = s.up(w, (size_t)ks * ks * Cin * Cout, &c.w);
    if (rc != VBX_OK) return rc;
    c.y = dy + pad;
    const int K = ks * ks * Cin;
    std::vector<uint16_t> wf(gemm == VBX_GEMM_SPLIT ? (size_t)K * Cout * 2 : 0);     // (wf and we outlive the copies: down()
    std::vector<int32_t> we(Cout);                                                   // synchronizes)
    if (gemm == VBX_GEMM_SPLIT) {
        rn_split_weights(w, K, Cout, wf.data(), we.data());
        unsigned* dax;
        rc = s.up_bytes(wf.data(), sizeof(uint16_t) * wf.size(), &c.wf);
        if (rc == VBX_OK) rc = s.up_bytes(we.data(), sizeof(int32_t) * we.size(), &c.we);
        if (rc == VBX_OK) rc = s.up_bytes(nullptr, sizeof(unsigned) * n, &dax);
        if (rc == VBX_OK) rc = s.up_bytes(nullptr, sizeof(unsigned) * n, &c.ay);
        if (rc != VBX_OK) return rc;
        rn_amax(ctx->stream, g, 0, Cin, c.x, dax);
        c.ax = dax;
    }
    if (!rn_launch(ctx->stream, c, BN, BM, gemm)) FAIL(ctx, VBX_ERR_INVALID, "%s: no kernel for this convolution", name);
    if (c.ay && amax_y) HIPCHK(ctx, hipMemcpyAsync(amax_y, c.ay, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
    return s.down(name, y, dy, ny);
}

int vbx_resnet_conv(vbx_ctx* ctx, int32_t ks, int32_t stride, int32_t n, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                    const float* x, const float* w, const float* bias, const float* res, int relu, int32_t bn, int32_t bm,
                    float* y, int64_t pad) {
    return rn_conv_step("vbx_resnet_conv", ctx, VBX_GEMM_EXACT, ks, stride, n, H, W, nullptr, Cin, Cout, x, w, bias, res, relu, bn, bm, y, pad,
                        nullptr);
}

int vbx_resnet_conv_gemm(vbx_ctx* ctx, int gemm, int32_t ks, int32_t stride, int32_t n, int32_t H, int32_t W, int32_t Cin,
                         int32_t Cout, const float* x, const float* w, const float* bias, const float* res, int relu, int32_t bn,
                         int32_t bm, float* y, int64_t pad, float* amax_y) {
    return rn_conv_step("vbx_resnet_conv_gemm", ctx, gemm, ks, stride, n, H, W, nullptr, Cin, Cout, x, w, bias, res, relu, bn, bm, y,
                        pad, amax_y);
}

int vbx_resnet_conv_ragged(vbx_ctx* ctx, int gemm, int32_t ks, int32_t stride, int32_t n, int32_t H, const int32_t* W, int32_t Cin,
                           int32_t Cout, const float* x, const float* w, const float* bias, const float* res, int relu, int32_t bn,
                           int32_t bm, float* y, int64_t pad, float* amax_y) {
    if (!ctx) return VBX_ERR_INVALID;
    const int rc = rn_check_lengths(ctx, "vbx_resnet_conv_ragged", n, W);
    if (rc != VBX_OK) return rc;
    return rn_conv_step("vbx_resnet_conv_ragged", ctx, gemm, ks, stride, n, H, 1, W, Cin, Cout, x, w, bias, res, relu, bn, bm, y, pad,
                        amax_y);
}

int vbx_resnet_stem(vbx_ctx* ctx, int32_t n, int32_t T, const float* x, const float* w, const float* bias, float* y, int64_t pad) {
    return rn_stem_step("vbx_resnet_stem", ctx, false, n, T, nullptr, x, w, bias, y, pad);
}

int vbx_resnet_stem_ragged(vbx_ctx* ctx, int32_t n, const int32_t* T, const float* x, const float* w, const float* bias, float* y,
                           int64_t pad) {
    return rn_stem_step("vbx_resnet_stem_ragged", ctx, true, n, 0, T, x, w, bias, y, pad);
}

int vbx_resnet_pool(vbx_ctx* ctx, int32_t n, int32_t W4, const float* x, float* out, int64_t pad) {
    return rn_pool_step("vbx_resnet_pool", ctx, false, n, W4, nullptr, x, out, pad);
}

int vbx_resnet_pool_ragged(vbx_ctx* ctx, int32_t n, const int32_t* W4, const float* x, float* out, int64_t pad) {
    return rn_pool_step("vbx_resnet_pool_ragged", ctx, true, n, 0, W4, x, out, pad);
}

}  // extern "C"
