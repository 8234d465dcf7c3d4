/*
 * vbx_hip.h -- C ABI of libvbx_hip.so, the MI355X (gfx950) implementation of the VBx
 * variational-Bayes HMM E/M loop.
 *
 * The reference has no FFI: the path is the pure-Python function
 *     VBx(X, Phi, loopProb, Fa, Fb, pi, gamma, maxIters, epsilon, alphaQInit, ref, plot,
 *         return_model, alpha, invL) -> (gamma, pi, Li[, alpha, invL])
 * at /root/reference/VBx/VBx.py:27-126, called from /root/reference/VBx/vbhmm.py:154-158.
 * The entry points below are what a ctypes binding for that function binds; the Python
 * mirror of the reference interface (vbx_amd/VBx.py) is a thin marshalling layer on top.
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 on success or a negative
 *     VBX_ERR_* code and never throws; vbx_last_error() gives the message.
 *   - the caller owns every host buffer; inputs are read-only; outputs are written
 *     into caller-allocated arrays.  Device memory is owned by the ctx / batch objects.
 *   - matrices are C-contiguous row-major, exactly as NumPy hands them over:
 *     X[T][D], gamma[T][S] (frames x speakers, VBx.py:82,85), alpha/invL[S][D].
 *   - a ctx is bound to one device and one HIP stream; not thread-safe per ctx.
 *   - "recording" = one x-vector sequence = one VBx() call in the reference.
 */
#ifndef VBX_HIP_H
#define VBX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The ABI only grows within a version: entry points are added (the *_ragged ones came after 7 was set), none changes its
 * signature or its meaning. */
#define VBX_ABI_VERSION 7

/* error codes */
#define VBX_OK 0
#define VBX_ERR_INVALID (-1)     /* bad argument (shape, NULL, range)                      */
#define VBX_ERR_UNSUPPORTED (-2) /* e.g. S > VBX_MAX_SPEAKERS                              */
#define VBX_ERR_HIP (-3)         /* a HIP runtime call failed; see vbx_last_error          */
#define VBX_ERR_NO_DEVICE (-4)   /* no gfx950-class GPU visible                            */
#define VBX_ERR_STATE (-5)       /* call order violated (run before every recording is set) */

#define VBX_MAX_SPEAKERS 16384 /* states per recording (the reference: any; up to 64 fused kernels, 256 wide scan, 1024 one-wavefront
                                  walk, beyond a workgroup-wide walk: vbx_big.hpp) */

/* element types of caller buffers */
#define VBX_F32 0
#define VBX_F64 1

/* arithmetic of the device path (bench.py "dtype") */
#define VBX_PREC_FP32 0 /* f32 storage + f32 MFMA; f64 for every reduction over T and the ELBO */
#define VBX_PREC_FP64 1 /* f64 storage + f64 MFMA; matches the reference's iteration count   */

/* forward-backward algorithm selector (vbx_batch_set_option VBX_OPT_FB_ALGO) */
#define VBX_FB_AUTO 0
#define VBX_FB_SEQUENTIAL 1 /* one wavefront per direction walks all T frames           */
#define VBX_FB_CHUNKED 2    /* exact chunked parallel scan over T (transfer operators)   */

/* options for vbx_batch_set_option */
#define VBX_OPT_FB_ALGO 1
#define VBX_OPT_CHECK_EVERY 2   /* iterations launched between two convergence polls (default 4) */
#define VBX_OPT_PROFILE 3       /* 0: off; 1: bracket every kernel launch with HIP events;
                                   2*mask: only the kernel classes whose bit (1 << VBX_K_*) is set in mask */
#define VBX_OPT_CHUNK_FRAMES 4  /* frames per scan chunk for VBX_FB_CHUNKED (0 = auto)         */
#define VBX_OPT_SCAN_GROUP 6    /* chunks per group of the two-level boundary walk: 0 auto (sqrt(chunks / 5) once a
                                   recording has >= 160 chunks, or >= 32 in a batch of <= 16; at most 128 / Sp + 1 where
                                   chunk_post walks the last level itself: up to 32 padded states in a batch of <= 2048
                                   chunks; 64 < Sp <= 256: sqrt(chunks / 3.5) from 40 chunks), 1 flat chain, >= 2 explicit */
#define VBX_OPT_SCAN_GROUP2 12   /* groups per level-2 group of the THREE-level walk: 0 auto (from 300 chunks per recording --
                                   T = 38 400 -- both group sizes become (chunks / 8)^(1/3) + 1), 1 off, >= 2 explicit (on top of
                                   the VBX_OPT_SCAN_GROUP in effect).  Where chunk_post walks the last level itself and the
                                   cube root is too long for it, up to 1200 chunks: 128 / Sp + 1 and sqrt(chunks / (5 group)) */
#define VBX_OPT_THREE_LEVEL_FROM 13 /* chunk count from which VBX_OPT_SCAN_GROUP2 = 0 adds the third level            */
#define VBX_OPT_SPLIT_TILES 11  /* fused path: tiles re-run as two halves side by side (four 64-frame chains per tile instead of two
                                   128-frame ones; chunk_loglik hands the half-tile operators over).  0 = auto (on), 1 = on,
                                   2 = off                                                                                */
#define VBX_OPT_STREAMS 10      /* HIP streams of a batch: its recordings are dealt to that many sub-batches, one
                                   iteration of each is launched stream after stream, so the latency-bound launches of
                                   one overlap the bandwidth-bound ones of the others.  0 = auto (3 from 24 recordings and
                                   1536 chunks; a batch created for max_iters >= 40: min(3, recordings, chunks / 150) if
                                   that is >= 2; else 2 from 12 recordings and 768 chunks, else 1; env VBX_AMD_STREAMS overrides).  Before the
                                   first recording. */
#define VBX_OPT_TWO_LEVEL_FROM 8 /* chunk count from which VBX_OPT_SCAN_GROUP = 0 picks the two-level walk           */
#define VBX_OPT_GEMM 14         /* how the fp32 path multiplies rho alpha^T (VBx.py:97) and gamma^T rho (VBx.py:96):
                                   VBX_GEMM_EXACT (default) v_mfma_f32_16x16x4_f32, the exact f32 product at the f32 vector
                                   rate; VBX_GEMM_SPLIT v_mfma_f32_16x16x32_f16 on error-compensated f16 operand pairs
                                   (x 2^e = hi + lo, three products, f32 accumulation: 2^-22 per product; rho kept in HBM
                                   as such pairs in MFMA fragment order -- vbx_amd/csrc/vbx_split.hpp).  fp32 batches on
                                   the fused kernels (S <= 64) only; ignored elsewhere.  env VBX_AMD_GEMM=exact|split   */
#define VBX_OPT_ASYNC_UPLOAD 15 /* 1: vbx_batch_set_recording / _shared only ENQUEUE the upload (no synchronize per recording):
                                   the caller's X and gamma0 must stay valid until the next vbx_batch_run or
                                   vbx_batch_sync_uploads returns.  0 (default): every setter returns with the caller's
                                   buffers free, as in ABI <= 6.  What a batch call saves: 64 recordings of T = 10 000 go up in
                                   ONE synchronize instead of 64 (ABI 7) */
#define VBX_GEMM_EXACT 0
#define VBX_GEMM_SPLIT 1
#define VBX_OPT_STREAM_LOADS 16 /* cache policy of the loads of rho in the two fused per-chunk kernels of the split mode
                                   (VBX_OPT_GEMM): VBX_STREAM_LOADS_ON fetches the f16 copies of rho with non-temporal loads
                                   (every line of them is read once per launch), VBX_STREAM_LOADS_OFF with the default policy,
                                   VBX_STREAM_LOADS_AUTO (default) picks ON where one copy of the x-vectors that iterate
                                   together -- all sub-batches of a stream group, a shared rho counted once -- is larger than
                                   the 256 MiB Infinity Cache (vbx_stream_loads_auto): below that a batch finds rho in the
                                   caches again one iteration later and the default policy keeps it there.  64 recordings of
                                   T = 10 000: 6-8 % of the step.  Where it is in effect chunk_post leaves the last level of
                                   the boundary walk to a launch of its own (no FOLD).  Results do not depend on it, bit for
                                   bit.  Ignored where the split kernels do not run: exact f32, fp64, S > 64
                                   (vbx_batch_stream_loads_in_effect tells) */
#define VBX_STREAM_LOADS_AUTO 0
#define VBX_STREAM_LOADS_ON 1
#define VBX_STREAM_LOADS_OFF 2
#define VBX_OPT_FUSE 5          /* per-chunk fused kernels when the lattices fit in LDS: 0 none, 1 chunk_post,
                                   2 (default) chunk_post + chunk_loglik.  On the fused path the responsibilities are
                                   written once, when vbx_batch_run returns (they are not needed between iterations) */

typedef struct vbx_ctx vbx_ctx;
typedef struct vbx_batch vbx_batch;

/* kernel classes reported by vbx_batch_kernel_times (one slot per HIP kernel) */
enum {
    VBX_K_PREP = 0,       /* rho = X*sqrt(Phi), sum_t G_t            VBx.py:87-89  */
    VBX_K_MSTEP_ACC = 1,  /* gamma^T rho partial sums (MFMA)         VBx.py:96     */
    VBX_K_MSTEP_FIN = 2,  /* invL, alpha, per-speaker bias           VBx.py:95-97  */
    VBX_K_LOGLIK = 3,     /* rho alpha^T + bias, row max, exp (MFMA) VBx.py:97     */
    VBX_K_FB = 4,         /* forward-backward recursion              VBx.py:146-175 */
    VBX_K_FB_AUX = 5,     /* chunk-boundary propagation (chunked scan only)         */
    VBX_K_POST = 6,       /* gamma, pi statistics                    VBx.py:101-103,174 */
    VBX_K_ITER_FIN = 7,   /* ELBO, pi update, convergence test       VBx.py:100-105,122-125 */
    VBX_K_CHUNK_LOGLIK = 8, /* fused: log-likelihoods + chunk transfer operator  VBx.py:97,167-171 */
    VBX_K_CHUNK_POST = 9, /* fused: chunk re-run + gamma + pi statistics + next gamma^T rho  VBx.py:96,101-103,167-174 */
    VBX_K_COUNT = 10
};

int vbx_abi_version(void);

/* ---- context -------------------------------------------------------------------- */
int vbx_create(vbx_ctx** out, int device);
int vbx_destroy(vbx_ctx* ctx);
/* message of the last failure on this ctx (ctx == NULL: last failure of vbx_create). */
const char* vbx_last_error(const vbx_ctx* ctx);
/* device name (NUL-terminated, truncated to cap), compute units, HBM bytes. */
int vbx_device_info(vbx_ctx* ctx, char* name, int cap, int* compute_units, int64_t* hbm_bytes);

/* ---- batch of recordings resident in HBM -------------------------------------------
 * T[b] frames, S[b] speakers (HMM states) per recording, common feature dim D.
 * max_iters bounds the ELBO history kept on the device. */
int vbx_batch_create(vbx_ctx* ctx, int n_rec, const int64_t* T, const int32_t* S, int32_t D,
                     int precision, int max_iters, vbx_batch** out);
/* The same with the number of HIP streams (sub-batches, VBX_OPT_STREAMS) chosen at creation: 0 = the library's choice as
 * vbx_batch_create makes it (VBX_OPT_STREAMS: three streams from 24 recordings and 1536 chunks, for max_iters >= 40 also two or
 * three from 150 chunks per stream, else two from 12 recordings and 768 chunks, else one; env VBX_AMD_STREAMS overrides), 1 .. 8 = that many (at most one per recording).  A batch created on one stream by the
 * automatic choice cannot be regrouped later (VBX_OPT_STREAMS regroups stream groups only): a sweep over one long recording
 * -- few "recordings", many chunks -- asks for its streams here (vbx_batch_set_recording_shared).  ABI 6. */
int vbx_batch_create_streams(vbx_ctx* ctx, int n_rec, const int64_t* T, const int32_t* S, int32_t D,
                             int precision, int max_iters, int streams, vbx_batch** out);
int vbx_batch_destroy(vbx_batch* batch);
int vbx_batch_set_option(vbx_batch* batch, int option, int64_t value);

/* Upload one recording and its hyper-parameters; computes rho and sum_t G_t on the device.
 *   X      [T][D]  x_dtype            (VBx.py:27 "X")
 *   Phi    [D]     f64                (VBx.py:27 "Phi")
 *   pi0    [S]     f64                (VBx.py:76-77; the caller expands an int pi to ones/pi)
 *   gamma0 [T][S]  g_dtype            (VBx.py:79-85; the caller draws the RNG init)
 *   alpha0, invL0 [S][D] f64 or both NULL (VBx.py:94: skip the first M-step when given)  */
int vbx_batch_set_recording(vbx_batch* batch, int b, const void* X, int x_dtype, const double* Phi,
                            const double* pi0, const void* gamma0, int g_dtype,
                            const double* alpha0, const double* invL0, double loopProb, double Fa,
                            double Fb);

/* Recording b on the x-vectors of recording src_b of the same batch (same T; src_b set before): a sweep of Fa / Fb /
 * loopProb over one recording -- the hyper-parameter grids of DIHARD2_run.sh:42-47, AMI_run.sh:44-49,
 * CALLHOME_run.sh:42-47 around one VBx.py:87-89 rho -- keeps ONE rho in HBM, and the per-chunk kernels run the chunks that
 * read the same rows of it side by side on one XCD, so that HBM delivers them once per kernel instead of once per sweep
 * point.  Everything else (pi0, gamma0, alpha0 / invL0, results) is per recording as in vbx_batch_set_recording.  Setting
 * src_b again unsets the recordings that share with it.  In a batch that runs on several streams (VBX_OPT_STREAMS) every
 * stream's sub-batch keeps ONE copy of the rows (made device to device when its first recording asks for them), shared by
 * the sweep points dealt to that stream: the latency-bound launches of one stream (boundary walk, per-recording
 * reductions) then hide behind the per-chunk kernels of the others. */
int vbx_batch_set_recording_shared(vbx_batch* batch, int b, int src_b, const double* pi0, const void* gamma0, int g_dtype,
                                   const double* alpha0, const double* invL0, double loopProb, double Fa, double Fb);

/* Run up to max_iters VB iterations on every recording (VBx.py:91-125).  A recording
 * stops on its own when ii > 0 and ELBO - previous < epsilon (VBx.py:122-125); its state
 * is frozen from then on.  Returns after the device work has completed. */
int vbx_batch_run(vbx_batch* batch, int max_iters, double epsilon);

/* Results of recording b.  Any pointer may be NULL to skip that output.
 *   gamma [T][S] f64, pi [S] f64, Li [n_iters] f64 (ELBO per iteration, VBx.py:105),
 *   n_iters, warned (1 iff the last ELBO step was negative: the reference prints
 *   'WARNING: Value of auxiliary function has decreased!', VBx.py:123-124),
 *   alpha/invL [S][D] f64 (VBx.py:126 return_model). */
int vbx_batch_get_result(vbx_batch* batch, int b, double* gamma, double* pi, double* Li, int li_cap,
                         int* n_iters, int* warned, double* alpha, double* invL);

/* Reference labels of recording b (VBx.py:27 "ref", the diagnostic mode of VBx.py:107-110): ref [T] in [0, n_ref), n_ref <= 64,
 * else VBX_ERR_INVALID.  Call it after the recording has been set and before a run; ref = NULL clears the labels.  While any
 * recording of the batch has labels, every iteration of vbx_batch_run is followed on the device -- no synchronize, no
 * download -- by the two score kernels (vbx_score.hpp), which leave in slot n_iters - 1 of the recording's history the
 * confusion block C [2][n_ref][S] f64 of that iteration's responsibilities:
 *   C[0][r][s] = sum_{t: ref_t = r} gamma[t][s]          C[1][r][s] = sum_{t: ref_t = r} -log(gamma[t][s] + 4.94e-324)
 * i.e. -err_mx of VBx.py:139 with and without xentropy; the assignment of VBx.py:140 stays with the caller.  A label without
 * frames keeps its all-zero row.  The sums are taken per recording in a fixed order: equal responsibilities give the same bits
 * alone, in any batch and on any number of streams.  (The responsibilities themselves are those of the batch: the forward-
 * backward algorithm follows the longest recording of a sub-batch, VBX_OPT_FB_ALGO, so a short recording gets another last bit
 * of gamma -- and with it of its blocks -- alone than beside a long one unless the option pins the algorithm.)  gamma, pi and
 * the ELBO do not depend on the labels, bit for bit.  Works for recordings set with _shared and _resident.  The labels belong to
 * slot b (whose T is fixed) and stay until they are set again or cleared, also when another recording is uploaded into the
 * slot: a caller that replaces the recording replaces its labels.  Setting or clearing labels discards the history of the
 * recordings that share the stream (sub-batch) of b; the history is kept across runs otherwise.  A batch without labels launches and allocates
 * nothing of this.  The launches are timed under VBX_K_POST. */
int vbx_batch_set_reference(vbx_batch* batch, int b, const int32_t* ref, int32_t n_ref);
/* The history of recording b: conf [n_iters][2][n_ref][S] f64, unpadded, at most cap_iters blocks of it (conf may be NULL);
 * n_iters = blocks that are valid = iterations the recording has run (at most the batch's max_iters; the iteration a
 * recording stopped at has its block, as VBx.py:105-125 appends before it tests).  Iterations that ran before the labels
 * were set hold zeros.  VBX_ERR_STATE: the recording has no labels. */
int vbx_batch_get_scores(vbx_batch* batch, int b, double* conf, int cap_iters, int* n_iters);

/* Wait for the uploads enqueued under VBX_OPT_ASYNC_UPLOAD (vbx_batch_run does the same when it begins).  ABI 7. */
int vbx_batch_sync_uploads(vbx_batch* batch);

/* Results of MANY recordings with one synchronize per stream: every item is what vbx_batch_get_result takes for recording
 * `rec` (any pointer may be NULL), n_iters / warned are filled in.  The copies into `gamma`, `alpha`, `invL` are plain DMA when
 * those point into memory from vbx_host_alloc (pinned), staged and blocking otherwise.  Replaces the per-recording loop a
 * batched caller of the reference would write around VBx.py:126's return.  ABI 7. */
typedef struct {
    int32_t rec;
    double* gamma;   /* [T][S] or NULL */
    double* pi;      /* [S] or NULL */
    double* Li;      /* [li_cap] or NULL */
    int32_t li_cap;
    int32_t n_iters; /* out */
    int32_t warned;  /* out */
    double* alpha;   /* [S][D] or NULL */
    double* invL;    /* [S][D] or NULL */
} vbx_fetch;
int vbx_batch_get_results(vbx_batch* batch, int n, vbx_fetch* items);

/* Pinned (page-locked) host memory from a process-wide pool: the destination of choice for vbx_batch_get_results and a fast
 * source for vbx_batch_set_recording.  A freed block goes back to the pool (at most 2 GB are kept).  A failure's message is
 * vbx_last_error(NULL).  ABI 7. */
int vbx_host_alloc(size_t bytes, void** out);
int vbx_host_free(void* p);

/* Wall time of the last vbx_batch_run measured with HIP events on the batch's stream
 * (ms), and the number of iterations that were launched. */
int vbx_batch_last_run_ms(vbx_batch* batch, double* total_ms, int* iters_launched);
/* With VBX_OPT_PROFILE=1: summed HIP-event time (ms) and launch count per kernel class
 * for the last run; arrays of VBX_K_COUNT entries. */
int vbx_batch_kernel_times(vbx_batch* batch, double* ms, int64_t* launches);
/* Number of HIP streams (sub-batches) this batch runs on: VBX_OPT_STREAMS in effect. */
int vbx_batch_streams(const vbx_batch* b);
/* The stream (sub-batch, 0 .. vbx_batch_streams - 1) recording b was dealt to; -1: no such recording.  vbx_batch_set_recording may
 * be called from different host threads for recordings of DIFFERENT streams (each stream has its own device arena): that is
 * how a batch call keeps the host link busy.  ABI 7. */
int vbx_batch_stream_of(const vbx_batch* b, int rec);
/* VBX_GEMM_EXACT or VBX_GEMM_SPLIT: how the iterations of the last vbx_batch_run multiplied (VBX_OPT_GEMM asks, the
 * batch's precision and kernels decide: fp64 batches, S > 64 and the unfused kernels always answer VBX_GEMM_EXACT -- and so
 * does a batch that holds a recording whose frames span more than 2^10 in magnitude, which one power-of-two scale per
 * recording cannot carry at 22 bits: vbx_split.hpp.  In a batch on several streams the guard acts per sub-batch and the
 * answer is VBX_GEMM_SPLIT only if every sub-batch multiplied that way). */
int vbx_batch_gemm_in_effect(const vbx_batch* b);
/* 1 if the per-chunk kernels of the last vbx_batch_run fetched rho with non-temporal loads (VBX_OPT_STREAM_LOADS asks, the
 * batch's size and kernels decide; a batch on several streams: every sub-batch), else 0. */
int vbx_batch_stream_loads_in_effect(const vbx_batch* b);
/* The launch plan of the last vbx_batch_run, read-only: which instances of the iteration's kernels it launched.  Writes the
 * first min(n, VBX_PLAN_FIELDS) of these into out and returns VBX_PLAN_FIELDS (fields are only ever appended), or
 * VBX_ERR_INVALID:
 *    0 fused_post    chunk_post ran (gamma stays on the chip)          7 fold         chunk_post walked the last walk level (FOLD)
 *    1 fused_loglik  ... and chunk_loglik                              8 walk_levels  boundary walk: 1 flat, 2 groups, 3 groups of groups
 *    2 half_ops      ... with half-tile operators                      9 fin_threads  block size of fin_kernel
 *    3 split         f16 operand pairs (VBX_OPT_GEMM)                 10 Sp           padded state count
 *    4 stream        ... in the non-temporal instances                11 use_chunked  chunked scan (else the sequential walk)
 *    5 small         the batch does not fill the chip                 12 sgroup       chunks per group in effect (1: flat)
 *    6 lat           LAT wanted (chunk_loglik has an instance of it   13 sgroup2      groups per level-2 group in effect (1: none)
 *                    in split mode only)
 * A batch that has never run reports the all-false plan; a batch on several streams the plan of its first sub-batch.  For tests
 * and diagnostics: nothing is to be decided on it. */
#define VBX_PLAN_FIELDS 14
int vbx_batch_plan(const vbx_batch* b, int* out, int n);
/* The rule of VBX_STREAM_LOADS_AUTO as a function of the bytes of ONE copy of the x-vectors that iterate together (sum of
 * T x padded D x element size over the recordings that own their x-vectors): 1 = non-temporal loads.  Host only. */
int vbx_stream_loads_auto(int64_t rho_bytes);

/* ---- one-shot: a single recording, host buffers in / out (= one reference VBx call) ---- */
typedef struct {
    int64_t T;
    int32_t D, S;
    const void* X;        /* [T][D] */
    int32_t x_dtype;      /* VBX_F32 / VBX_F64 */
    const double* Phi;    /* [D] */
    const double* pi0;    /* [S] */
    const void* gamma0;   /* [T][S] */
    int32_t g_dtype;
    const double* alpha0; /* [S][D] or NULL */
    const double* invL0;  /* [S][D] or NULL */
    double loopProb, Fa, Fb;
    int32_t max_iters;
    double epsilon;
    int32_t precision;    /* VBX_PREC_* */
    int32_t fb_algo;      /* VBX_FB_* */
} vbx_problem;

typedef struct {
    double* gamma;   /* [T][S] */
    double* pi;      /* [S] */
    double* Li;      /* [max_iters] */
    double* alpha;   /* [S][D] or NULL */
    double* invL;    /* [S][D] or NULL */
    int32_t n_iters;
    int32_t warned;
    double run_ms;   /* device time of the iteration loop */
} vbx_result;

int vbx_run(vbx_ctx* ctx, const vbx_problem* problem, vbx_result* result);

/* ---- step-level entry points (used by the parity tests) ------------------------------
 * forward_backward (VBx.py:146-175) for transition matrices of the form VBx.py:98 builds,
 *   tr = I*loopProb + (1-loopProb)*pi      (every column j constant off the diagonal),
 * and initial-state probabilities ip (NULL: ip = pi, as VBx.py:99 passes them).
 *   lls [T][S] f64, pi [S], ip [S]  ->  gamma [T][S], tll, entered [S], lfw [T][S], lbw [T][S]
 * entered[j] = sum_{t>=1} exp(LSE_i lfw[t-1,i] + lls[t,j] + lbw[t,j] - tll) is the statistic
 * of VBx.py:101-103.  Any output pointer may be NULL. */
int vbx_forward_backward(vbx_ctx* ctx, int64_t T, int32_t S, const double* lls, const double* pi,
                         const double* ip, double loopProb, int precision, int fb_algo, double* gamma,
                         double* tll, double* entered, double* lfw, double* lbw);
/* forward_backward (VBx.py:146-175) for ANY transition matrix tr [S][S] (row i: from state i) and initial-state
 * probabilities ip [S]; eps = 1e-8 is added to both as VBx.py:158,163 do.  lls [T][S] -> gamma [T][S] (state
 * posteriors), tll, lfw [T][S], lbw [T][S]; any output pointer may be NULL.  One dependent S x S mat-vec per frame. */
int vbx_forward_backward_dense(vbx_ctx* ctx, int64_t T, int32_t S, const double* lls, const double* tr, const double* ip,
                               int precision, double* gamma, double* tll, double* lfw, double* lbw);
/* M-step (VBx.py:95-96): gamma [T][S], X [T][D], Phi [D] -> alpha, invL [S][D]. */
int vbx_mstep(vbx_ctx* ctx, int64_t T, int32_t S, int32_t D, const double* X, const double* Phi,
              const double* gamma, double Fa, double Fb, int precision, double* alpha, double* invL);
/* per-frame log-likelihoods (VBx.py:97): X, Phi, alpha, invL -> log_p [T][S] (G included). */
int vbx_loglik(vbx_ctx* ctx, int64_t T, int32_t S, int32_t D, const double* X, const double* Phi,
               const double* alpha, const double* invL, double Fa, int precision, double* log_p);

/* the confusion block of vbx_batch_set_reference for responsibilities on the host: gamma [T][S] f64 (rounded to f32 first for
 * VBX_PREC_FP32, as a batch of that precision holds them), ref [T] in [0, n_ref), n_ref <= 64 -> conf [2][n_ref][S] f64.
 * The same two kernels as in the iteration loop. */
int vbx_score_posteriors(vbx_ctx* ctx, int64_t T, int32_t S, const double* gamma, const int32_t* ref, int32_t n_ref,
                         int precision, double* conf);

/* ---- the steps of the driver either side of VBx(), for all x-vectors of an archive at once -------------------------
 * vbhmm.py:125-129  xproj = l2_norm( l2_norm(x - mean1) lda - mean2 )       [n][Dl]       input of cos_similarity
 * vbhmm.py:153      fea   = (xproj - plda_mu) plda_tr^T [:, :fea_dim]        [n][fea_dim]  input of VBx()
 * Both stay resident in HBM (vbx_xvectors); x [n][Din] x_dtype, mean1 [Din], lda [Din][Dl], mean2 [Dl],
 * plda_mu [Dl], plda_tr [Dl][Dl] (row k = k-th output dim, i.e. the array vbhmm.py:113 calls plda_tr): f64. */
typedef struct vbx_xvectors vbx_xvectors;
int vbx_xvectors_project(vbx_ctx* ctx, int64_t n, int32_t Din, int32_t Dl, int32_t fea_dim, const void* x, int x_dtype,
                         const double* mean1, const double* lda, const double* mean2, const double* plda_mu,
                         const double* plda_tr, vbx_xvectors** out);
/* The same for x-vectors that already lie in HBM (the network left them there: vbx_resnet_run with out_on_device):
 * d_x [n_src][Din] f32 on ctx's device; row i of the result is source row rows_host[i], i < n (host array, strictly
 * increasing, every index < n_src; NULL: every row in order, n == n_src).  Nothing but the n indices and the model goes
 * up; the first kernel reads its row through the index, the rest is vbx_xvectors_project's chain, so the result has the
 * bits that entry gives from a host copy of the kept rows.  Runs on ctx's stream and ends with one synchronize. */
int vbx_xvectors_project_device(vbx_ctx* ctx, int64_t n_src, int32_t Din, int32_t Dl, int32_t fea_dim, const float* d_x,
                                int64_t n, const int64_t* rows_host, const double* mean1, const double* lda,
                                const double* mean2, const double* plda_mu, const double* plda_tr, vbx_xvectors** out);
/* flags_host[t] = 1 where row t of d_x [n][D] f32 (device memory of ctx's device) holds a NaN, else 0 -- predict.py:185's
 * np.isnan(embedding).any(), an infinity is not flagged.  The n flags are all that comes back to the host. */
int vbx_rows_nan_flags(vbx_ctx* ctx, const float* d_x, int64_t n, int32_t D, int32_t* flags_host);
/* rows [row0, row0 + nrows) of xproj (which = 0, [nrows][Dl]) or fea (which = 1, [nrows][fea_dim]) to the host. */
int vbx_xvectors_get(vbx_xvectors* xv, int which, int64_t row0, int64_t nrows, double* out);
int vbx_xvectors_destroy(vbx_xvectors* xv);
/* cos_similarity (diarization_lib.py:190-213) of the resident rows [row0, row0 + T) of xproj: nothing is uploaded. */
int vbx_cos_similarity_resident(vbx_ctx* ctx, vbx_xvectors* xv, int64_t row0, int64_t T, struct vbx_scores** out);
/* Recording b of a batch from resident rows of fea and the AHC labels [T] (in [0, S[b])): the initial responsibilities
 * softmax(init_smoothing * onehot(labels)) of vbhmm.py:150-152 are built on the device, pi0 = 1/S (VBx.py:76). */
int vbx_batch_set_recording_resident(vbx_batch* batch, int b, const vbx_xvectors* xv, int64_t row0, const int32_t* labels,
                                     double init_smoothing, const double* Phi, double loopProb, double Fa, double Fb);
/* ---- --init random_N (the reference's README.md:24: random speaker labels instead of AHC's, then VBx) ----------------
 * labels_host[t] = (w[t] * N) >> 64, t < T, where w is the stream of 64-bit words Philox4x64-10 gives under the key
 * {seed, name_hash} from the counter {0, restart, 0, 0}: numpy's np.random.Philox(key=[seed, name_hash],
 * counter=[0, restart, 0, 0]).random_raw(T), i.e. word t % 4 of the block with counter {t / 4 + 1, restart, 0, 0}.  Drawn on
 * the device; N >= 1, restart >= 0.  name_hash is FNV-1a-64 of the recording's name in the driver (vbx_amd.vbhmm.name_hash). */
int vbx_random_labels(vbx_ctx* ctx, uint64_t seed, uint64_t name_hash, int64_t restart, int64_t T, int32_t N, int32_t* labels_host);
/* Recording b of a batch from those labels with N = S[b]: drawn on the device into scratch and turned into the initial
 * responsibilities softmax(init_smoothing * onehot(labels)) there, pi0 = 1/S -- what vbx_batch_set_recording_resident does with
 * labels from the host, bit for bit; no label and no responsibility crosses the bus.
 *   src_b < 0:  b owns a rho built from the resident rows [row0, row0 + T) of fea with Phi: the one path of every setter that
 *               reads resident rows (rho_from_resident, vbx_amd/csrc/vbx_host_set.hpp).
 *   src_b >= 0: b runs on the rho (and Phi) of recording src_b, under the rules of vbx_batch_set_recording_shared: same T,
 *               src_b set before (by any of the setters), one copy of the rows per stream sub-batch; xv, row0 and Phi are
 *               not read and may be 0 / NULL.  The restarts of a recording: restart 0 owns, the others share with it. */
int vbx_batch_set_recording_random(vbx_batch* batch, int b, const vbx_xvectors* xv, int64_t row0, int src_b, uint64_t seed,
                                   uint64_t name_hash, int64_t restart, double init_smoothing, const double* Phi,
                                   double loopProb, double Fa, double Fb);
/* ---- --init RTTM / RTTM+VB (the VB-HMM as the second stage of a system: it starts from a diarization that exists) -------
 * All times are integer microseconds.  Window i < T is [seg_a[i], seg_b[i]), seg_a[i] < seg_b[i]; turn j < N is
 * [turn_u[j], turn_v[j]) of speaker turn_spk[j] in [0, S), turn_u[j] < turn_v[j], and the turns are sorted by (speaker, start).
 *   d[i][s] = sum over the turns j of s of max(0, min(b_i, v_j) - max(a_i, u_j))   (exact),   D_i = sum_s d[i][s]
 *   D_i > 0:  w[i][s] = d[i][s] / D_i (one f64 division), label[i] = argmax_s d[i][s], the lowest among equals
 *   D_i == 0: the turn with the smallest gap g_j = max(u_j - b_i, a_i - v_j) names the speaker, the lowest index among equal
 *             gaps; w[i] is its one-hot row and label[i] is that speaker
 *   q[i][s] = exp(x_s - max x) / sum_s' exp(x_s' - max x), x = init_smoothing * w[i]      (summed in speaker order)
 * labels_host [T], w_host [T][S] and q_host [T][S] are computed on the device; each may be NULL.  A T or N below 1, an S
 * outside [1, VBX_MAX_SPEAKERS], a speaker outside [0, S), an empty window or turn, and turns out of order are refused with
 * VBX_ERR_INVALID before the device is touched (with ctx == NULL the message is vbx_last_error(NULL)'s). */
int vbx_turn_weights(vbx_ctx* ctx, int64_t T, const int64_t* seg_a, const int64_t* seg_b, int64_t N, const int64_t* turn_u,
                     const int64_t* turn_v, const int32_t* turn_spk, int32_t S, double init_smoothing, int32_t* labels_host,
                     double* w_host, double* q_host);
/* Recording b of a batch from those turns, S = S[b] and T = T[b] as the batch was created: rho from the resident rows
 * [row0, row0 + T) of fea with Phi on the path every setter of resident rows takes (rho_from_resident), the initial responsibilities q by the
 * kernel of vbx_turn_weights straight into the batch (padded speakers: 0), pi0 = 1/S.  Only the 2 T ticks and the N turns go
 * up; no weight and no responsibility crosses the bus. */
int vbx_batch_set_recording_turns(vbx_batch* batch, int b, const vbx_xvectors* xv, int64_t row0, const int64_t* seg_a,
                                  const int64_t* seg_b, int64_t N, const int64_t* turn_u, const int64_t* turn_v,
                                  const int32_t* turn_spk, double init_smoothing, const double* Phi, double loopProb, double Fa,
                                  double Fb);
/* vbhmm.py:160-162: np.argsort(-gamma, axis=1)[:, 0] and [:, 1] of recording b, [T] each (second: -1 when S == 1);
 * equal responsibilities keep their index order (numpy leaves the order of ties unspecified).  Either may be NULL. */
int vbx_batch_get_labels(vbx_batch* batch, int b, int32_t* first, int32_t* second);

/* ---- Viterbi decoding: the jointly most probable state sequence ------------------------------------
 * The model is vbx_forward_backward's: tr = I*loopProb + (1-loopProb)*pi, eps = 1e-8 added to tr and to ip before the
 * logarithm (VBx.py:158-164); ip NULL: ip = pi.  lls [T][S], pi [S], ip [S] are host arrays.
 *   path [T]  the state sequence q that maximises log(ip[q_0] + eps) + sum_t lls[t][q_t] + sum_{t>=1} log(tr[q_{t-1}][q_t] + eps)
 *   logp      that maximum
 * Among equal scores the lowest state index wins at the last frame and where a path enters a state; where staying in a
 * state and entering it score the same, the path stays.  Either output may be NULL.  The call takes no guard-band argument:
 * exactly T labels are written (the tests over-allocate and pass an interior pointer to see that nothing else is).
 * Refused before the device is touched: NULL lls or pi, T < 1, S < 1, loopProb outside [0, 1] (VBX_ERR_INVALID); S > 1024
 * (VBX_ERR_UNSUPPORTED, the message names S): one wavefront walks a recording with up to 16 states per lane. */
int vbx_viterbi(vbx_ctx* ctx, int64_t T, int32_t S, const double* lls, const double* pi, const double* ip, double loopProb,
                int32_t* path, double* logp);
/* The same for recording b of a batch after a run, under the model of the LAST forward-backward pass -- the one the
 * responsibilities vbx_batch_get_result returns come from: that iteration's likelihoods (the batch's b = exp(l - m_t), taken
 * as log b: a per-frame shift does not change the path), the priors that entered it, ip = pi, the recording's loopProb.
 *   first  [T]  the path
 *   second [T]  the speaker of the largest gamma[t][s] among s != first[t], the lowest index among equals; -1 when S == 1
 * Either may be NULL.  VBX_ERR_INVALID for a recording index out of range, VBX_ERR_STATE for a batch that has not run or a
 * recording that has run no iteration (no E-step to decode), VBX_ERR_UNSUPPORTED for S[b] > 1024. */
int vbx_batch_get_path(vbx_batch* batch, int b, int32_t* first, int32_t* second);
/* Device time in milliseconds of the kernels of the calling thread's last successful vbx_viterbi / vbx_batch_get_path, between
 * two events on the stream: the copies either side are not in it (tools/bench_viterbi.py). */
double vbx_viterbi_last_ms(void);

/* ---- score stage of the AHC initialisation (next row upstream of VBx(): vbhmm.py:135-138) -------------
 * cos_similarity(x)            /root/reference/VBx/diarization_lib.py:190-213
 * twoGMMcalib_lin(s, niters)   /root/reference/VBx/diarization_lib.py:13-31
 * The T x T score matrix stays resident in HBM between the two calls (vbx_scores). */
typedef struct vbx_scores vbx_scores;

/* x [T][D] f64 (rows need not be normalised) -> device-resident matrix of cosine similarities. */
int vbx_cos_similarity(vbx_ctx* ctx, int64_t T, int32_t D, const double* x, vbx_scores** out);
/* A device-resident copy of n host scores (for callers that bring their own scores). */
int vbx_scores_upload(vbx_ctx* ctx, int64_t n, const double* s, vbx_scores** out);
/* Number of scores held (T*T after vbx_cos_similarity). */
int64_t vbx_scores_count(const vbx_scores* sc);
/* Copy count scores starting at offset to the host (out [count]). */
int vbx_scores_get(vbx_scores* sc, int64_t offset, int64_t count, double* out);
/* The strict upper triangle of scale * S, row by row -- the vector form scipy.spatial.distance.squareform(m,
 * checks=False) gives -- of a T x T score matrix: vbhmm.py:139 `scr_mx = squareform(-scr_mx, checks=False)` is
 * scale = -1.  out: [T (T - 1) / 2]. */
int vbx_scores_get_condensed(vbx_scores* sc, int64_t T, double scale, double* out);

/* vbhmm.py:139-141 on the device: average linkage of the distances -S, S = the T x T matrix of similarities held by sc,
 * by a nearest-neighbour chain that one persistent workgroup walks on the matrix where it lies (no condensed copy, no
 * PCIe traffic but the T - 1 merges).  Z [T - 1][4]: the linkage matrix vbx_linkage_average gives for
 * squareform(-S), bit for bit.  CONSUMES the scores: afterwards sc holds the distances of the merged clusters. */
int vbx_scores_linkage_average(vbx_scores* sc, int64_t T, double* Z);

/* Average-linkage clustering of n observations from their condensed distance vector [n (n - 1) / 2] (host code;
 * nearest-neighbour chain, see vbx_linkage.hpp for why it is not a kernel): vbhmm.py:140-141
 * `fastcluster.linkage(scr_mx, method='average')`.  Z: [n - 1][4] = (cluster a, cluster b, distance, members), the
 * linkage matrix of scipy.cluster.hierarchy / fastcluster, bit for bit SciPy's.  Pure function, safe to call from
 * several threads at once (one recording per thread); needs no vbx_ctx. */
int vbx_linkage_average(int64_t n, const double* condensed, double* Z);
/* The same clustering in the form fastcluster 1.2 itself computes it (the package vbhmm.py:33,140-141 imports; SciPy is
 * what this repository's fixtures were made with because fastcluster is not installed): weights divided before the update
 * (d = s a + t b, s = n_a / (n_a + n_b)) and fastcluster's own chain bookkeeping (vbx_linkage.hpp).  Same tree and
 * distances equal to rounding wherever no two candidate distances tie; selected by VBX_AMD_LINKAGE=fastcluster in the
 * Python layer.  Restated from the published source -- parity with the package itself is unpinned. */
int vbx_linkage_average_fastcluster(int64_t n, const double* condensed, double* Z);
/* Flat clusters of the linkage matrix Z cut at cophenetic distance t: vbhmm.py:145-146 `fcluster(lin_mat, t,
 * criterion='distance')`.  labels: [n], numbered from 1 in SciPy's order (depth-first from the root). */
int vbx_fcluster_distance(int64_t n, const double* Z, double t, int32_t* labels);

/* Index of a binary Kaldi vector archive held in memory (vbhmm.py:117 `kaldi_io.read_vec_flt_ark`): offsets and
 * lengths of the key and of the data of every entry ('FV ' float32 / 'DV ' float64 vectors).  Returns the number
 * of entries; -1: not a well-formed binary vector archive; -2: more than `cap` entries. */
int64_t vbx_ark_index(const void* buf, int64_t len, int64_t cap, int64_t* key_off, int32_t* key_len, int64_t* data_off,
                      int32_t* dim, int32_t* elem_size);
/* n rows of row_bytes bytes each, row i starting at buf + offsets[i], packed into out (the vectors of one recording
 * out of an indexed archive: `np.array(xvecs)` of vbhmm.py:123). */
int vbx_gather_rows(const void* buf, int64_t len, const int64_t* offsets, int64_t n, int64_t row_bytes, void* out);
/* Two-Gaussian shared-variance EM over all the scores: threshold, and (llr != NULL) the linearly calibrated
 * log-odds of every score, [vbx_scores_count]. */
int vbx_scores_two_gmm_calib(vbx_scores* sc, int32_t niters, double* threshold, double* llr);
int vbx_scores_destroy(vbx_scores* sc);

/* ---- the Kaldi-recipe PLDA similarity, the alternative to cos_similarity for the AHC stage (vbx_plda_score.hpp) -------
 * kaldi_ivector_plda_scoring_dense   diarization_lib.py:59-93
 * PLDA_scoring_in_LDA_space          diarization_lib.py:34-56
 * The D x D eigen-decompositions of the reference stay with the caller; these entry points do what is O(T) and O(T^2).
 *
 * Covariance np.cov(x.T, bias=True) of the rows x [T][D] (D <= 1024): mean [D], cov [D][D] to the host.  Summed over
 * fixed chunks of rows in a fixed order: the same rows give the same bits on every run and from either entry point. */
int vbx_plda_covariance(vbx_ctx* ctx, int64_t T, int32_t D, const double* x, double* mean, double* cov);
/* ... of the resident rows [row0, row0 + T) of xproj (D = Dl). */
int vbx_plda_covariance_resident(vbx_ctx* ctx, vbx_xvectors* xv, int64_t row0, int64_t T, double* mean, double* cov);
/* Dense T x T PLDA scores of the rows x [T][D] as a vbx_scores, everything calibration and linkage take:
 *   y = (x - mu) proj,  y *= sqrt(d / sum_k y_k^2 / (acvar_k + 1)),  S = PLDA_scoring_in_LDA_space(y, y, acvar)
 * mu [D], proj [D][d] (the reference's PCA . wccn), acvar [d] >= 0, 1 <= d <= 256.  S is symmetric to the last bit. */
int vbx_plda_scores(vbx_ctx* ctx, int64_t T, int32_t D, const double* x, int32_t d, const double* mu, const double* proj,
                    const double* acvar, vbx_scores** out);
/* ... of the resident rows [row0, row0 + T) of xproj (D = Dl): nothing but the model is uploaded. */
int vbx_plda_scores_resident(vbx_ctx* ctx, vbx_xvectors* xv, int64_t row0, int64_t T, int32_t d, const double* mu,
                             const double* proj, const double* acvar, vbx_scores** out);
/* PLDA_scoring_in_LDA_space(Fe, Ft, diagAC): Fe [N][D], Ft [M][D], diagAC [D] -> out [N][M] on the host. */
int vbx_plda_score_lda(vbx_ctx* ctx, int64_t N, int64_t M, int32_t D, const double* Fe, const double* Ft,
                       const double* diagAC, double* out);

/* ---- md-eval diarization error of RTTM turns (vbx_rttm_score.hpp) ------------------------------------------------------
 * What `dscore/score.py --collar C [--ignore_overlaps]` of the reference's recipes reports, DER only, for n_pairs
 * (reference, system) pairs in one call.  Per pair p, counts[p] = {n_edges, n_ref_turns, n_sys_turns, n_ref, n_sys}:
 *   edges   its n_edges sorted distinct cell edges (n_edges - 1 cells; 0 or 1: no cell), pair after pair
 *   turns   [n_ref_turns + n_sys_turns][2] = (begin, end) of its merged reference turns, then of its system turns
 *   spk     the speaker index of every turn, in [0, n_ref) and [0, n_sys); n_ref, n_sys <= 64 (more: VBX_ERR_UNSUPPORTED)
 * A cell is scored unless its midpoint lies strictly within collar of a begin or an end of a reference turn or
 * (ignore_overlaps != 0) two or more reference speakers are active in it.  out receives per pair 4 + n_ref n_sys f64:
 * scored reference speaker time, miss, false alarm, sum of w min(|R|, |S|), then C [n_ref][n_sys].  A pair's numbers
 * are the same bits alone, in any batch and at any position in it.  Synchronises before it returns. */
int vbx_rttm_score(vbx_ctx* ctx, int32_t n_pairs, const int32_t* counts, const double* edges, const double* turns,
                   const int32_t* spk, double collar, int ignore_overlaps, double* out);

/* ---- ... of label sequences: many hypotheses per recording (vbx_labels_score.hpp) ---------------------------------------
 * What vbx_rttm_score gives for the turns of vbhmm.merge_adjacent_labels(starts, ends, labels), with the turns and the cell
 * edges of every hypothesis built on the device.  Per recording r, rec_counts[r] = {T, n_ref_turns, n_ref, n_ref_edges}:
 *   seg_times  starts[T] then ends[T], recording after recording; finite, starts[i] < ends[i], both non-decreasing
 *   ref_turns  [n_ref_turns][2] = (begin, end) of its merged reference turns, ref_spk their speakers in [0, n_ref)
 *   ref_edges  the reference's part of the cell edges, strictly increasing: reference turn boundaries, their collar zone ends,
 *              lo = min(first reference begin, starts[0]) and hi = max(last reference end, ends[T - 1]), clipped to [lo, hi]
 * Per hypothesis h, hyp[h] = {recording, n_sys} and the T labels of that recording in [0, n_sys), hypothesis after
 * hypothesis; system speaker s is label s.  n_ref, n_sys <= 64 (more: VBX_ERR_UNSUPPORTED).  out receives per hypothesis
 * 4 + n_ref n_sys f64 as vbx_rttm_score gives them (a label that never occurs: a zero column); info (or NULL) per hypothesis
 * {system turns, cell edges, low and high word of the mask of the labels that have a turn of positive duration}.
 * Everything is checked on the host before the first launch.  A hypothesis's numbers are the same bits alone, in any batch
 * and at any position in it.  Synchronises before it returns. */
int vbx_labels_score(vbx_ctx* ctx, int32_t n_rec, const int32_t* rec_counts, const double* seg_times, const double* ref_turns,
                     const int32_t* ref_spk, const double* ref_edges, int32_t n_hyp, const int32_t* hyp, const int32_t* labels,
                     double collar, int ignore_overlaps, double* out, int32_t* info);

/* ---- energy voice-activity detection (vbx_vad.hpp): the speech segments a .lab file lists ------------------------------
 * Kaldi's energy VAD rule on the front end's frames, for n_rec recordings laid end to end in samples [n_samples] int16:
 * rec [n_rec][2] = (first sample, samples) of each.  A recording of n samples has T = (n - winlen) / shift + 1 frames (0
 * if n < winlen); frame t is the samples [t shift, t shift + winlen) as they are.  winlen / shift: 400 / 160 or 200 / 80,
 * others VBX_ERR_UNSUPPORTED.  Per recording
 *   N[t]   = winlen sum x^2 - (sum x)^2, exact in int64;  e[t] = log(max(N[t] / winlen, 1)) in f64
 *   theta  = energy_threshold + mean_scale * sum_t e[t] / T   (T = 0: energy_threshold)
 *   raw[t] = n_hot >= n_in * proportion in f64: n_in the frames of [t - context, t + context] inside [0, T), n_hot those
 *            of them with e > theta
 * then, on the maximal runs of raw: every gap between two runs shorter than min_silence frames closes, every run then
 * shorter than min_speech frames goes, what is left grows by pad frames on both sides, clipped to [0, T), and runs that
 * touch or overlap become one.
 *   counts [n_rec]       the segments of every recording (0 where T = 0)
 *   segs   [sum][2]      their frames [a, b), recording after recording; the caller provides sum_r (T_r + 1) / 2 pairs,
 *                        only sum counts of them are written
 *   N, e, raw [sum T]    the frames of all recordings end to end (int64, f64, bytes), theta [n_rec]; each may be NULL
 *   ms [2]               device milliseconds of the upload and of the kernels (HIP events); may be NULL
 * A recording's numbers are the same bits alone, in any batch and at any place in it.  VBX_ERR_INVALID with a message: a
 * NULL pointer, n_rec <= 0, a recording outside the samples, a parameter that is not finite, or a count outside [0, 2^30].
 * Synchronises before it returns. */
int vbx_vad_energy(vbx_ctx* ctx, int64_t n_samples, const int16_t* samples, int32_t n_rec, const int64_t* rec, int32_t winlen,
                   int32_t shift, double energy_threshold, double mean_scale, int32_t context, double proportion,
                   int32_t min_silence, int32_t min_speech, int32_t pad, int32_t* counts, int32_t* segs, int64_t* N, double* e,
                   double* theta, uint8_t* raw, float* ms);

/* ---- frame counts behind dscore's JER, B-cubed and information-theoretic columns (vbx_frame_score.hpp) --------------------
 * dscore scores these columns on frames of `step` seconds: frame i exists for 0 <= i < int(hi / step), its time is the f64
 * product step * i, a turn [b, e) holds the frames with b <= step * i < e, and the frames with lo <= step * i < hi count.
 * For n_pairs (reference, system) pairs in one call; per pair p, counts[p] = {n_ref_turns, n_sys_turns, n_ref, n_sys}:
 *   extent  [n_pairs][2] = (lo, hi), lo <= hi finite, hi / step < 2^40
 *   turns   [n_ref_turns + n_sys_turns][2] = (begin, end) of its reference turns, then of its system turns, pair after pair;
 *           lo <= begin <= end <= hi
 *   spk     the speaker index of every turn, in [0, n_ref) and [0, n_sys); n_ref, n_sys <= 64 (more: VBX_ERR_UNSUPPORTED)
 * A frame's class on a side is the set of the side's speakers active in it (the empty set is a class); classes are numbered
 * in order of first appearance.
 *   info    [n_pairs][4] = {cells, reference classes, system classes, 0}
 *   classes [n_pairs][2][256]: the 64-bit speaker masks of the first 256 reference and of the first 256 system classes
 *   out     int64, pair after pair: ref_durs [n_ref], sys_durs [n_sys], inter [n_ref][n_sys] (frames that hold both), then
 *           cm [reference classes][system classes] -- left out for a pair with more than 256 classes on either side
 * out_cap: the int64 out has room for; a result that needs more: VBX_ERR_INVALID, nothing written.  All sums are integers,
 * no atomics: a pair's numbers are the same bytes alone, in any batch and at any place in it.  Everything the kernels index
 * with is checked on the host before the first launch.  Synchronises before it returns. */
int vbx_frame_counts(vbx_ctx* ctx, int32_t n_pairs, const int32_t* counts, const double* extent, const double* turns,
                     const int32_t* spk, double step, int32_t* info, uint64_t* classes, int64_t* out, int64_t out_cap);

/* ---- ... of label sequences: many hypotheses per recording (vbx_labels_frame.hpp) ---------------------------------------
 * What vbx_frame_counts gives for the turns of vbhmm.merge_adjacent_labels(starts, ends, labels), with the turns of every
 * hypothesis built on the device and the reference's side uploaded and cut into frames once per recording.  Per recording r,
 * rec_counts[r] = {T, n_ref_turns, n_ref}:
 *   seg_times  starts[T] then ends[T], recording after recording; finite, starts[i] < ends[i], both non-decreasing
 *   ref_turns  [n_ref_turns][2] = (begin, end) of its merged reference turns, begin <= end finite; ref_spk their speakers in
 *              [0, n_ref)
 * A hypothesis's extent is its recording's: lo = min(reference begins, starts[0]), hi = max(reference ends, ends[T - 1]);
 * hi / step < 2^40.  Per hypothesis h, hyp[h] = {recording, n_sys} and the T labels of that recording in [0, n_sys),
 * hypothesis after hypothesis; system speaker s is label s.  n_ref, n_sys <= 64 (more: VBX_ERR_UNSUPPORTED).
 *   info, classes, out, out_cap   per hypothesis what vbx_frame_counts gives per pair, in that layout (a label that never
 *              occurs: sys_durs 0 and a zero column of inter)
 *   label_masks [n_hyp]           bit s: label s has a turn of positive duration
 * All sums are integers, no atomics: a hypothesis's numbers are the same bytes alone, in any batch, at any place in it and
 * among other hypotheses of its recording, and the bytes vbx_frame_counts gives for the same turns.  Everything the kernels
 * index with is checked on the host before the first launch.  Synchronises before it returns. */
int vbx_labels_frame_counts(vbx_ctx* ctx, int32_t n_rec, const int32_t* rec_counts, const double* seg_times, const double* ref_turns,
                            const int32_t* ref_spk, int32_t n_hyp, const int32_t* hyp, const int32_t* labels, double step,
                            int32_t* info, uint64_t* classes, int64_t* out, int64_t out_cap, uint64_t* label_masks);

/* ---- any PCM recording to mono int16 at 8 or 16 kHz (vbx_resample.hpp) -------------------------------------------------
 * n_rec recordings of one sample format, channel count and rate pair, their raw interleaved little-endian frames laid end to
 * end in bytes [n_bytes] as they lie in their files: rec [n_rec][2] = (first byte, frames) of each, at any byte offset.
 *   format    0: u8, 1: s16, 2: s24, 3: s32, 4: f32;  channels 1 .. 8
 * A sample becomes an integer q at 24-bit scale: u8 (b - 128) << 16, s16 x << 8, s24 x, s32 x >> 8 (floor), f32 NaN -> 0 and
 * otherwise rint-half-even(x 2^23) clamped to [-2^23, 2^23 - 1].  X[j] = sum of q over the channels of frame j.
 *   L, M      sr_out / g and sr_in / g, g their gcd; L <= 640, M <= 1024;  P = 32 max(L, M)
 *   table     [L][taps] int32, taps = 2 P / L + 1: table[p][k] = hq[p + k L], 0 past hq[2 P], for the integer prototype
 *             hq[0 .. 2 P] whose every phase {p, p + L, ...} sums to 2^24 and sum |hq| < 2^26 (vbx_amd/audio.py)
 * A recording of n frames gives n_out = ceil(n L / M) samples,
 *   acc[m] = sum_j X[j] hq[P + m M - j L] over the j in [0, n) with |m M - j L| <= P     (exact in int64)
 *   y[m]   = clamp(floor((2 acc + D) / (2 D)), -32768, 32767),  D = channels 2^32        (round half up)
 *   out  [sum n_out]     the samples, recording after recording
 *   ms   [2]             device milliseconds of the upload and of the kernel (HIP events); may be NULL
 * A recording's samples are the same bits alone, in any batch and at any place in it; nothing is read across a recording's
 * ends.  VBX_ERR_INVALID with a message: a NULL pointer, n_rec <= 0, a format, channel count, L, M or taps outside the above,
 * a recording outside the bytes.  VBX_ERR_UNSUPPORTED: more than 2^30 frames or samples in a recording, or an L, M whose tile
 * of 256 outputs spans more than 8192 input frames (M / L above 25).  Synchronises before it returns. */
int vbx_resample_pcm(vbx_ctx* ctx, int64_t n_bytes, const uint8_t* bytes, int32_t n_rec, const int64_t* rec, int32_t format,
                     int32_t channels, int32_t L, int32_t M, int32_t taps, const int32_t* table, int16_t* out, float* ms);

/* ---- filterbank front end of the x-vector extractor (predict.py:150-204 with features.py) -----------------------
 * Per VAD segment: mirror padding (predict.py:173-174), frames of winlen samples every shift, zero mean, pre-emphasis,
 * window, |rfft(., nfft)|^2, log(max(1, P mel)) (features.py:fbank_htk with USEPOWER, ZMEANSOURCE), then
 * cmvn_floating_kaldi(., LC, RC, norm_vars=False) cast to float32.  The four linear steps run as ONE f64 operator on the
 * matrix cores (vbx_fbank.hpp).  The dither before it (predict.py:169-170, numpy's legacy generator) is either the
 * caller's, who passes the dithered f64 signal to vbx_fbank_run, or the library's: vbx_fbank_run_raw takes the int16
 * samples and draws the same MT19937 stream on the device, bit for bit. */
typedef struct vbx_fbank vbx_fbank;
/* window [winlen], mel [nfft/2 + 1][n_mel] f64 (features.mel_fbank_mx).  Geometries built: winlen / shift / nfft =
 * 400 / 160 / 512 (16 kHz) and 200 / 80 / 256 (8 kHz), n_mel = 64; others: VBX_ERR_UNSUPPORTED. */
int vbx_fbank_create(vbx_ctx* ctx, int32_t winlen, int32_t shift, int32_t nfft, int32_t n_mel, const double* window,
                     const double* mel, double preemph, vbx_fbank** out);
/* signal [n_samples] f64 (one recording or several laid end to end); seg [n_seg][2] = (first sample, samples) of every
 * segment to process, clipped to its recording and longer than (winlen - shift) / 2 samples.  The features of all
 * segments land in one device array of rows [*n_frames][n_mel], segment after segment, (padded - winlen) / shift + 1
 * rows each.  Returns once the host arrays may be reused. */
int vbx_fbank_run(vbx_fbank* fb, int64_t n_samples, const double* signal, int32_t n_seg, const int64_t* seg, int32_t cmn_lc,
                  int32_t cmn_rc, int64_t* n_frames);
/* vbx_fbank_run from the raw int16 samples [n_samples] of n_rec recordings: rec [n_rec][2] = (first sample, samples) of
 * each.  Recording r becomes x + levels[r] * (2 u - 1) in f64 with u = np.random.RandomState(seeds[r]).rand(samples), every
 * sample of it in order (not only the segments), the stream restarting from its seed for every recording; the signal
 * vbx_fbank_run would have been given, one quarter of the bytes uploaded.  Samples that belong to no recording are zero.
 * Then the launch sequence of vbx_fbank_run; returns once the host arrays may be reused.  VBX_ERR_INVALID with a message:
 * a NULL pointer, n_rec <= 0, a recording that runs past n_samples, two recordings that overlap. */
int vbx_fbank_run_raw(vbx_fbank* fb, int64_t n_samples, const int16_t* samples, int32_t n_rec, const int64_t* rec,
                      const uint32_t* seeds, const double* levels, int32_t n_seg, const int64_t* seg, int32_t cmn_lc,
                      int32_t cmn_rc, int64_t* n_frames);
/* samples [first, first + n) of the f64 signal of the last run (uploaded by vbx_fbank_run, written by vbx_fbank_run_raw).
 * Synchronises before it returns. */
int vbx_fbank_get_signal(vbx_fbank* fb, int64_t first, int64_t n, double* dst, int dst_on_device);
/* rows [row0, row0 + nrows) of the last run: which = 0 the CMN features (f32), 1 the log-Mel rows before CMN (f64).
 * dst_on_device != 0: dst is device memory of the ctx's device (e.g. a torch tensor).  Synchronises before it returns. */
int vbx_fbank_get(vbx_fbank* fb, int which, int64_t row0, int64_t nrows, void* dst, int dst_on_device);
/* n windows of len rows of the CMN features starting at rows starts[n], transposed to dst [n][n_mel][len] f32 (the
 * embedding model's [B, C, T] input, predict.py:68-70).  Synchronises before it returns. */
int vbx_fbank_windows(vbx_fbank* fb, int32_t n, const int64_t* starts, int32_t len, float* dst, int dst_on_device);
/* Windows of mixed lengths in one call: window w is lens[w] >= 1 rows from row starts[w], transposed to [n_mel][lens[w]];
 * dst receives the n blocks end to end (n_mel * sum(lens) f32): the input of vbx_resnet_run_ragged.  One kernel, one
 * synchronize, where vbx_fbank_windows needs a call per length.  VBX_ERR_INVALID with a message: n <= 0, a NULL pointer, a
 * lens[w] <= 0, a window past the feature rows. */
int vbx_fbank_windows_ragged(vbx_fbank* fb, int32_t n, const int64_t* starts, const int32_t* lens, float* dst, int dst_on_device);
/* device milliseconds (HIP events) of the last run: ms[0] upload, [1] frame kernel, [2] CMN; ms[3] the last windows call. */
int vbx_fbank_times(vbx_fbank* fb, float* ms);
/* device milliseconds of the dither kernel of the last run (between its upload and its frame kernel); 0 if that run was
 * no vbx_fbank_run_raw. */
int vbx_fbank_dither_time(vbx_fbank* fb, float* ms);
int vbx_fbank_destroy(vbx_fbank* fb);

/* ---- x-vector network ------------------------------------------------------------------------------------------------
 * models/resnet.py:ResNet101 (Bottleneck [3, 4, 23, 3], m = 32, 64 input rows) for inference, BatchNorm folded into the
 * convolutions, on the ctx's stream (the stream of vbx_fbank: windows it gathers into vbx_resnet_input's buffer need no
 * host round trip).  Convolutions are implicit GEMMs on the f32 matrix instructions (vbx_resnet.hpp) or, opt-in, on the
 * f16 matrix instructions with error-compensated operands (vbx_resnet_set_gemm); an embedding does not depend on the batch
 * its window is run in. */
typedef struct vbx_resnet vbx_resnet;
/* params: the folded network as f32 (vbx_amd/xvector.py:fold): per convolution in network order its weights
 * [kh kw Cin][Cout] and bias [Cout], then the embedding [16384][embed_dim] (pooling order) and its bias. */
int vbx_resnet_create(vbx_ctx* ctx, int32_t embed_dim, const float* params, int64_t n_params, vbx_resnet** out);
/* a device buffer of n windows [n][64][T] f32 that vbx_fbank_windows may fill; valid until the next vbx_resnet_input. */
int vbx_resnet_input(vbx_resnet* net, int32_t n, int32_t T, float** d_in);
/* embeddings [n][embed_dim] f32 of n windows x [n][64][T] (host or device memory).  Workspace grows to the largest
 * (n, T) seen.  One synchronize, after the copy out. */
int vbx_resnet_run(vbx_resnet* net, int32_t n, int32_t T, const float* x, int x_on_device, float* out, int out_on_device);
/* A ragged batch: n windows of T[b] >= 1 frames each, in any order, through the network in one walk.  x is the windows'
 * [64][T[b]] blocks end to end (64 * sum(T) f32, host or device memory); out [n][embed_dim].  At level l = 0 .. 3 (64 >> l
 * rows; a window's width W_{b,l} is (W - 1) / 2 + 1 applied l times to T[b]) an activation tensor is the windows'
 * [H_l][W_{b,l}][C] blocks end to end; the host uploads where each starts (pos [4][n + 1], int64) and how wide it is (wid
 * [4][n], int32), and a kernel row finds its window by a binary search of pos.  Nothing is padded to a common width.  Every
 * embedding has the bits vbx_resnet_run gives that window alone, in both gemm modes.  Workspace grows to the largest
 * sum seen; vbx_resnet_times and vbx_resnet_gemm_in_effect speak of it as of any run.  VBX_ERR_INVALID with a message:
 * n <= 0, a NULL pointer, a T[b] <= 0. */
int vbx_resnet_run_ragged(vbx_resnet* net, int32_t n, const int32_t* T, const float* x, int x_on_device, float* out,
                          int out_on_device);
/* vbx_resnet_input for a ragged batch: a device buffer of 64 * sum(T) f32 that vbx_fbank_windows_ragged may fill. */
int vbx_resnet_input_ragged(vbx_resnet* net, int32_t n, const int32_t* T, float** d_in);
/* device milliseconds of the last run: ms[0] stem, [1..4] layer1..layer4, [5] pooling + embedding. */
int vbx_resnet_times(vbx_resnet* net, float* ms);
int vbx_resnet_destroy(vbx_resnet* net);
/* How the convolutions of layer1 .. layer4 multiply in the runs that follow: VBX_GEMM_EXACT (default: the f32 matrix
 * instructions, bits as before) or VBX_GEMM_SPLIT (vbx_resnet_split.hpp: v_mfma_f32_32x32x16_f16 on error-compensated f16
 * operand pairs, weights split per output channel at create time, activations per window as they are staged; f32-level
 * accuracy, not the exact mode's bits).  The stem, the pooling and the embedding stay exact in both.  An embedding does not
 * depend on the batch in either mode.  A library built without the ISA audit refuses VBX_GEMM_SPLIT: VBX_ERR_UNSUPPORTED. */
int vbx_resnet_set_gemm(vbx_resnet* net, int gemm);
/* VBX_GEMM_EXACT or VBX_GEMM_SPLIT: how the last vbx_resnet_run multiplied (VBX_GEMM_EXACT before the first). */
int vbx_resnet_gemm_in_effect(vbx_resnet* net);

/* ---- step-level entry points of the network (used by the kernel tests) ----------------------------------------------
 * One kernel of vbx_resnet.hpp per call, on the ctx's stream.  Every array is a host pointer to f32; the call allocates
 * device buffers, copies in, launches, copies out, synchronizes and frees: for tests, not for speed.
 * Outputs are IN/OUT with a guard band: the array holds pad + (payload) + pad floats, all of it is uploaded, the kernel is
 * given the address of element pad, and all of it comes back.  A caller that fills it with a sentinel beforehand sees
 * stores outside the payload and payload elements the kernel never wrote.
 *
 * The BN x BM output tile the network's dispatcher uses for a convolution of M = n Ho Wo output positions and Cout
 * channels (Cout a multiple of 32).  Host code: needs no device. */
int vbx_resnet_conv_tile(int64_t M, int32_t Cout, int32_t* bn, int32_t* bm);
/* One convolution as the network launches it: ks x ks (1 or 3, padding ks / 2), stride 1 or 2, then + bias, + res (NULL:
 * none), ReLU if relu != 0 (NaN kept).  Ho = (H - 1) / stride + 1, Wo likewise, M = n Ho Wo.
 *   x [n][H][W][Cin], w [ks ks Cin][Cout] (row (r ks + s) Cin + c), bias [Cout], res [M][Cout]  ->  y [pad + M Cout + pad]
 * bn = bm = 0: the dispatcher's tile; otherwise one of BN x BM = 128 x 64, 128 x 128, 64 x 64, 64 x 128, 32 x 128 is forced.
 * VBX_ERR_INVALID, with nothing launched: ks or stride not built, Cin not a multiple of 16, Cout not a multiple of the
 * tile's BN (of 32 when the tile is not forced), a tile that is not one of the five, a size <= 0, x / w / bias / y NULL. */
int vbx_resnet_conv(vbx_ctx* ctx, int32_t ks, int32_t stride, int32_t n, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                    const float* x, const float* w, const float* bias, const float* res, int relu, int32_t bn, int32_t bm,
                    float* y, int64_t pad);
/* vbx_resnet_conv in either mode.  gemm = VBX_GEMM_SPLIT: the weights are split as vbx_resnet_create splits them, max |x| of
 * every image is measured on the device, and the split kernel of the (dispatcher's or forced) tile runs; the same guard
 * band contract and the same refusals.  amax_y (NULL: not wanted) [n] receives what the kernel records for its consumer:
 * max |y| over the finite outputs of every image (split mode only). */
int vbx_resnet_conv_gemm(vbx_ctx* ctx, int gemm, int32_t ks, int32_t stride, int32_t n, int32_t H, int32_t W, int32_t Cin,
                         int32_t Cout, const float* x, const float* w, const float* bias, const float* res, int relu, int32_t bn,
                         int32_t bm, float* y, int64_t pad, float* amax_y);
/* vbx_resnet_conv_gemm over a ragged batch: n windows of H rows and W[b] >= 1 columns.  x is the windows' [H][W[b]][Cin]
 * blocks end to end, res and the payload of y the [Ho][Wo[b]][Cout] blocks end to end (M = sum Ho Wo[b] positions), amax_y
 * [n].  The ragged kernel of the (dispatcher's, for this M, or forced) tile runs; guard band, tiles and refusals as
 * vbx_resnet_conv, and n <= 0, W NULL or a W[b] <= 0 refused with a message. */
int vbx_resnet_conv_ragged(vbx_ctx* ctx, int gemm, int32_t ks, int32_t stride, int32_t n, int32_t H, const int32_t* W, int32_t Cin,
                           int32_t Cout, const float* x, const float* w, const float* bias, const float* res, int relu, int32_t bn,
                           int32_t bm, float* y, int64_t pad, float* amax_y);
/* The split mode's weights (host code, needs no device): w [K][Cout] f32, K a multiple of 16, Cout of 32  ->  e [Cout], the
 * exponent of every output channel's power-of-two scale, and frag [K / 16][Cout / 32][hi | lo][64 lanes][8] f16 bits, the
 * fragment order of the B operand of v_mfma_f32_32x32x16_f16: lane l holds B[k = 8 (l >> 5) + j][column l & 31]. */
int vbx_resnet_split_weights(int32_t K, int32_t Cout, const float* w, uint16_t* frag, int32_t* e);
/* The stem: conv 3 x 3 of one input channel to 32, + bias, ReLU.  x [n][64][T], w [9][32] (row r 3 + s), bias [32]
 * ->  y [pad + n 64 T 32 + pad], the payload [n][64][T][32]. */
int vbx_resnet_stem(vbx_ctx* ctx, int32_t n, int32_t T, const float* x, const float* w, const float* bias, float* y, int64_t pad);
/* The stem over a ragged batch: x the [64][T[b]] blocks end to end  ->  the payload of y the [64][T[b]][32] blocks. */
int vbx_resnet_stem_ragged(vbx_ctx* ctx, int32_t n, const int32_t* T, const float* x, const float* w, const float* bias, float* y,
                           int64_t pad);
/* Statistics pooling over a ragged batch: x the [8][W4[b]][1024] blocks end to end, every window divided by its own W4[b]
 * ->  the payload [n][16384]. */
int vbx_resnet_pool_ragged(vbx_ctx* ctx, int32_t n, const int32_t* W4, const float* x, float* out, int64_t pad);
/* Statistics pooling: x [n][8][W4][1024]  ->  out [pad + n 16384 + pad], the payload [n][16384]: [h 1024 + c] the mean
 * over the W4 frames, [8192 + h 1024 + c] sqrt(mean(x^2) - mean^2 + 1e-10), summed in f64. */
int vbx_resnet_pool(vbx_ctx* ctx, int32_t n, int32_t W4, const float* x, float* out, int64_t pad);

/* ---- training the x-vector backend: the LDA transform and the Kaldi PLDA the chain reads (vbx_backend.hpp) ------------------
 * The passes over N labelled x-vectors; the D x D algebra between and after them (a generalised eigenproblem, the PLDA's EM)
 * stays with the caller (vbx_amd/backend.py).  Everything is float64, summed over fixed chunks of 512 rows in a fixed order:
 * the same input gives the same bits on every run.
 * Refused with VBX_ERR_INVALID and a message before the device is touched: a NULL pointer, N, D or K < 1, D > 1024, a class
 * outside [0, K), a class without a row, offsets that descend or leave the rows.
 *
 * sums [K][D] = the sums of the rows x [N][D] (x_dtype VBX_F32 or VBX_F64) of every class, the rows of a class added in
 * archive order; counts [K] (NULL: not wanted) = its rows. */
int vbx_backend_class_sums(vbx_ctx* ctx, int64_t N, int32_t D, const void* x, int x_dtype, int32_t K, const int32_t* class_of_row,
                           double* sums, int64_t* counts);
/* out [G][D][D], out[g] = sum over the rows t in [offsets[g], offsets[g + 1]) of rows[t] rows[t]^T, rows [R][D]; a segment
 * without rows gives zero.  Every out[g] is symmetric to the last bit. */
int vbx_backend_second_moments(vbx_ctx* ctx, int64_t R, int32_t D, const double* rows, int64_t G, const int64_t* offsets, double* out);
/* The x-vectors x [N][Din] and their classes, resident in HBM across the two stages. */
typedef struct vbx_backend vbx_backend;
int vbx_backend_create(vbx_ctx* ctx, int64_t N, int32_t Din, const void* x, int x_dtype, int32_t K, const int32_t* class_of_row,
                       vbx_backend** out);
/* mean1 [Din] = the mean of the rows; y = l2norm(x - mean1) stays in HBM; class_sums [K][Din] and moment [Din][Din] =
 * sum_t y_t y_t^T are those of y.  A row without length after centring is refused with its index (VBX_ERR_INVALID).
 * kernel_ms (NULL: not wanted): the time of the stage's kernels on the device, between two events. */
int vbx_backend_stage1(vbx_backend* be, double* mean1, double* class_sums, double* moment, double* kernel_ms);
/* u = l2norm(y lda - mean2), lda [Din][Dl], mean2 [Dl], 1 <= Dl <= Din: the rows xproj of vbx_xvectors_project.
 * class_sums [K][Dl] and moment [Dl][Dl] are those of u.  Needs stage 1. */
int vbx_backend_stage2(vbx_backend* be, int32_t Dl, const double* lda, const double* mean2, double* class_sums, double* moment,
                       double* kernel_ms);
int vbx_backend_destroy(vbx_backend* be);

#ifdef __cplusplus
}
#endif
#endif /* VBX_HIP_H */
