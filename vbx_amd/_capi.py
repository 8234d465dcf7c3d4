"""ctypes binding of libvbx_hip.so (include/vbx_hip.h).  No CPU fallback: if the library or
a gfx950 device is missing, every entry point raises."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

from . import build as _build

VBX_F32, VBX_F64 = 0, 1
PREC_FP32, PREC_FP64 = 0, 1
FB_AUTO, FB_SEQUENTIAL, FB_CHUNKED = 0, 1, 2
OPT_FB_ALGO, OPT_CHECK_EVERY, OPT_PROFILE, OPT_CHUNK_FRAMES, OPT_FUSE, OPT_SCAN_GROUP = 1, 2, 3, 4, 5, 6
OPT_TWO_LEVEL_FROM, OPT_STREAMS, OPT_SPLIT_TILES, OPT_SCAN_GROUP2, OPT_THREE_LEVEL_FROM = 8, 10, 11, 12, 13
OPT_GEMM = 14                # how the fp32 path multiplies: GEMM_EXACT (f32 MFMA) | GEMM_SPLIT (f16 operand pairs, vbx_split.hpp)
GEMM_EXACT, GEMM_SPLIT = 0, 1
GEMM_NAMES = {'exact': GEMM_EXACT, 'split': GEMM_SPLIT}
OPT_ASYNC_UPLOAD = 15        # setters only enqueue; one synchronize when the next run begins (Batch.set_async_upload)
OPT_STREAM_LOADS = 16        # non-temporal loads of rho in the per-chunk kernels: auto (by the bytes that iterate together) | on | off
STREAM_LOADS_AUTO, STREAM_LOADS_ON, STREAM_LOADS_OFF = 0, 1, 2
STREAM_LOADS_NAMES = {'auto': STREAM_LOADS_AUTO, 'on': STREAM_LOADS_ON, 'off': STREAM_LOADS_OFF}
# fields of vbx_batch_plan, in its order (include/vbx_hip.h)
PLAN_FIELDS = ['fused_post', 'fused_loglik', 'half_ops', 'split', 'stream', 'small', 'lat', 'fold', 'walk_levels', 'fin_threads',
               'Sp', 'use_chunked', 'sgroup', 'sgroup2']
PLAN_FLAGS = PLAN_FIELDS[:8] + ['use_chunked']
K_NAMES = ['prep', 'mstep_acc', 'mstep_fin', 'loglik', 'fb', 'fb_aux', 'post', 'iter_fin', 'chunk_loglik',
           'chunk_post']
MAX_SPEAKERS = 16384
MAX_DECODE_STATES = 1024      # kVitMaxStates: one wavefront walks a recording's Viterbi decode, 16 states per lane (vbx_viterbi.hpp)
PLDA_COV_CHUNK = 512         # rows of one partial of the PLDA covariance (vbx_plda_score.hpp: kCovChunk)
PLDA_MAX_DIM = 256           # dimensions the PLDA projection kernel keeps (vbx_plda_score.hpp: 16 * kPldaMaxTiles)
MAX_REF_LABELS = 64          # labels a recording can be scored against on the device (vbx_batch_set_reference)
# vbx_rttm_score.hpp: cells per classification workgroup, turns per LDS chunk, cells per partial block, cells per LDS chunk of
# the accumulation, speakers per side (kRttmClsBlock, kRttmTurnChunk, kRttmGroupCells, kRttmAccChunk, kRttmMaxSpk)
RTTM_CLS_BLOCK, RTTM_TURN_CHUNK, RTTM_GROUP_CELLS, RTTM_ACC_CHUNK, RTTM_MAX_SPEAKERS = 256, 256, 1024, 256, 64
LABELS_BLOCK = 256           # vbx_labels_score.hpp: segments / boundaries per scan pass of a workgroup (kLabBlock)
# vbx_vad.hpp: frames per energy / decision workgroup, frames per pass of the run-boundary compaction, runs per pass of the
# run-list stages (kVadTile, kVadRunPass, kLabBlock)
VAD_TILE, VAD_RUN_PASS, VAD_RUN_BLOCK = 256, 4096, 256
# vbx_frame_score.hpp: boundaries / cells / result entries per workgroup and per LDS chunk, speakers and classes per side
# (kFrmBlock, kFrmMaxSpk, kFrmMaxCls)
FRAME_BLOCK, FRAME_MAX_SPEAKERS, FRAME_MAX_CLASSES = 256, 64, 256
# vbx_resample.hpp: outputs per workgroup, input frames of a tile staged in LDS, table entries up to which the table is staged
# in LDS too (kRsTile, kRsSpan, kRsTabLds)
RESAMPLE_TILE, RESAMPLE_SPAN, RESAMPLE_TABLE_LDS = 256, 8192, 1024

ABI_SYMBOLS = [
    'vbx_abi_version', 'vbx_create', 'vbx_destroy', 'vbx_last_error', 'vbx_device_info',
    'vbx_batch_create', 'vbx_batch_create_streams', 'vbx_batch_destroy', 'vbx_batch_set_option', 'vbx_batch_set_recording',
    'vbx_batch_run', 'vbx_batch_get_result', 'vbx_batch_last_run_ms', 'vbx_batch_kernel_times',
    'vbx_run', 'vbx_forward_backward', 'vbx_forward_backward_dense', 'vbx_mstep', 'vbx_loglik',
    'vbx_cos_similarity', 'vbx_scores_upload', 'vbx_scores_count', 'vbx_scores_get', 'vbx_scores_get_condensed', 'vbx_scores_linkage_average',
    'vbx_linkage_average', 'vbx_linkage_average_fastcluster', 'vbx_fcluster_distance', 'vbx_ark_index', 'vbx_gather_rows', 'vbx_batch_streams',
    'vbx_scores_two_gmm_calib',
    'vbx_scores_destroy',
    'vbx_xvectors_project', 'vbx_xvectors_get', 'vbx_xvectors_destroy', 'vbx_cos_similarity_resident',
    'vbx_batch_set_recording_resident', 'vbx_batch_get_labels', 'vbx_batch_set_recording_shared',
    'vbx_batch_gemm_in_effect', 'vbx_batch_stream_loads_in_effect', 'vbx_stream_loads_auto', 'vbx_batch_plan',
    'vbx_batch_stream_of', 'vbx_batch_sync_uploads', 'vbx_batch_get_results', 'vbx_host_alloc', 'vbx_host_free',
    'vbx_fbank_create', 'vbx_fbank_run', 'vbx_fbank_get', 'vbx_fbank_windows', 'vbx_fbank_times', 'vbx_fbank_destroy',
    'vbx_resnet_create', 'vbx_resnet_input', 'vbx_resnet_run', 'vbx_resnet_times', 'vbx_resnet_destroy',
    'vbx_resnet_conv_tile', 'vbx_resnet_conv', 'vbx_resnet_stem', 'vbx_resnet_pool',
    'vbx_resnet_set_gemm', 'vbx_resnet_gemm_in_effect', 'vbx_resnet_conv_gemm', 'vbx_resnet_split_weights',
    'vbx_fbank_windows_ragged', 'vbx_resnet_run_ragged', 'vbx_resnet_input_ragged',
    'vbx_resnet_conv_ragged', 'vbx_resnet_stem_ragged', 'vbx_resnet_pool_ragged',
    'vbx_fbank_run_raw', 'vbx_fbank_get_signal', 'vbx_fbank_dither_time',
    'vbx_batch_set_reference', 'vbx_batch_get_scores', 'vbx_score_posteriors',
    'vbx_plda_covariance', 'vbx_plda_covariance_resident', 'vbx_plda_scores', 'vbx_plda_scores_resident', 'vbx_plda_score_lda',
    'vbx_xvectors_project_device', 'vbx_rows_nan_flags',
    'vbx_rttm_score', 'vbx_labels_score',
    'vbx_vad_energy',
    'vbx_frame_counts', 'vbx_labels_frame_counts',
    'vbx_resample_pcm',
    'vbx_random_labels', 'vbx_batch_set_recording_random',
    'vbx_turn_weights', 'vbx_batch_set_recording_turns',
    'vbx_backend_class_sums', 'vbx_backend_second_moments', 'vbx_backend_create', 'vbx_backend_stage1', 'vbx_backend_stage2',
    'vbx_backend_destroy',
    'vbx_viterbi', 'vbx_batch_get_path', 'vbx_viterbi_last_ms',
]


class VbxError(RuntimeError):
    pass


_lib = None


def library_path() -> str:
    return _build.LIB


def load():
    """Load (building if the sources are newer) the HIP library.  Raises when unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB
    if not os.path.exists(path) or (_build.is_stale() and os.environ.get('VBX_AMD_NO_REBUILD') != '1'):
        try:
            path = _build.build()
        except Exception as exc:  # a stale-but-present library is still usable on a box without hipcc
            if not os.path.exists(path):
                raise VbxError(f'libvbx_hip.so is not built and cannot be built here: {exc}') from exc
    want = os.environ.get('VBX_AMD_HW_QUEUES') or '8'       # before the HIP runtime starts (see vbx_host_state.hpp); '0': hands off
    if want != '0':
        os.environ.setdefault('GPU_MAX_HW_QUEUES', want)
    lib = C.CDLL(path)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    lib.vbx_abi_version.restype = C.c_int
    lib.vbx_create.argtypes = [C.POINTER(vp), C.c_int]
    lib.vbx_destroy.argtypes = [vp]
    lib.vbx_last_error.argtypes = [vp]
    lib.vbx_last_error.restype = C.c_char_p
    lib.vbx_device_info.argtypes = [vp, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(i64)]
    lib.vbx_batch_create.argtypes = [vp, C.c_int, C.POINTER(i64), C.POINTER(i32), i32, C.c_int, C.c_int,
                                     C.POINTER(vp)]
    lib.vbx_batch_create_streams.argtypes = [vp, C.c_int, C.POINTER(i64), C.POINTER(i32), i32, C.c_int, C.c_int, C.c_int,
                                             C.POINTER(vp)]
    lib.vbx_batch_destroy.argtypes = [vp]
    lib.vbx_batch_set_option.argtypes = [vp, C.c_int, i64]
    lib.vbx_batch_set_recording.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, dbl, dbl, dbl]
    lib.vbx_batch_run.argtypes = [vp, C.c_int, dbl]
    lib.vbx_batch_get_result.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.POINTER(C.c_int),
                                         C.POINTER(C.c_int), vp, vp]
    lib.vbx_batch_last_run_ms.argtypes = [vp, C.POINTER(dbl), C.POINTER(C.c_int)]
    lib.vbx_batch_kernel_times.argtypes = [vp, vp, vp]
    lib.vbx_batch_streams.argtypes = [vp]
    lib.vbx_batch_gemm_in_effect.argtypes = [vp]
    lib.vbx_batch_stream_loads_in_effect.argtypes = [vp]
    lib.vbx_stream_loads_auto.argtypes = [i64]
    lib.vbx_batch_plan.argtypes = [vp, vp, C.c_int]
    lib.vbx_run.argtypes = [vp, vp, vp]
    lib.vbx_forward_backward.argtypes = [vp, i64, i32, vp, vp, vp, dbl, C.c_int, C.c_int, vp, C.POINTER(dbl),
                                         vp, vp, vp]
    lib.vbx_forward_backward_dense.argtypes = [vp, i64, i32, vp, vp, vp, C.c_int, vp, C.POINTER(dbl), vp, vp]
    lib.vbx_mstep.argtypes = [vp, i64, i32, i32, vp, vp, vp, dbl, dbl, C.c_int, vp, vp]
    lib.vbx_loglik.argtypes = [vp, i64, i32, i32, vp, vp, vp, vp, dbl, C.c_int, vp]
    lib.vbx_cos_similarity.argtypes = [vp, i64, i32, vp, C.POINTER(vp)]
    lib.vbx_scores_upload.argtypes = [vp, i64, vp, C.POINTER(vp)]
    lib.vbx_scores_count.argtypes = [vp]
    lib.vbx_scores_get.argtypes = [vp, i64, i64, vp]
    lib.vbx_scores_get_condensed.argtypes = [vp, i64, dbl, vp]
    lib.vbx_scores_linkage_average.argtypes = [vp, i64, vp]
    lib.vbx_linkage_average.argtypes = [i64, vp, vp]
    lib.vbx_linkage_average_fastcluster.argtypes = [i64, vp, vp]
    lib.vbx_fcluster_distance.argtypes = [i64, vp, dbl, vp]
    lib.vbx_ark_index.argtypes = [vp, i64, i64, vp, vp, vp, vp, vp]
    lib.vbx_ark_index.restype = i64
    lib.vbx_gather_rows.argtypes = [vp, i64, vp, i64, i64, vp]
    lib.vbx_scores_two_gmm_calib.argtypes = [vp, i32, C.POINTER(dbl), vp]
    lib.vbx_scores_destroy.argtypes = [vp]
    lib.vbx_xvectors_project.argtypes = [vp, i64, i32, i32, i32, vp, C.c_int, vp, vp, vp, vp, vp, C.POINTER(vp)]
    lib.vbx_xvectors_get.argtypes = [vp, C.c_int, i64, i64, vp]
    lib.vbx_xvectors_destroy.argtypes = [vp]
    lib.vbx_cos_similarity_resident.argtypes = [vp, vp, i64, i64, C.POINTER(vp)]
    lib.vbx_batch_set_recording_resident.argtypes = [vp, C.c_int, vp, i64, vp, dbl, vp, dbl, dbl, dbl]
    lib.vbx_batch_get_labels.argtypes = [vp, C.c_int, vp, vp]
    lib.vbx_batch_get_path.argtypes = [vp, C.c_int, vp, vp]
    lib.vbx_viterbi.argtypes = [vp, i64, i32, vp, vp, vp, dbl, vp, C.POINTER(dbl)]
    lib.vbx_viterbi_last_ms.argtypes = []
    lib.vbx_batch_sync_uploads.argtypes = [vp]
    lib.vbx_batch_stream_of.argtypes = [vp, C.c_int]
    lib.vbx_batch_get_results.argtypes = [vp, C.c_int, vp]
    lib.vbx_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    lib.vbx_host_free.argtypes = [vp]
    lib.vbx_batch_set_recording_shared.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, dbl, dbl, dbl]
    lib.vbx_fbank_create.argtypes = [vp, i32, i32, i32, i32, vp, vp, dbl, C.POINTER(vp)]
    lib.vbx_fbank_run.argtypes = [vp, i64, vp, i32, vp, i32, i32, C.POINTER(i64)]
    lib.vbx_fbank_get.argtypes = [vp, C.c_int, i64, i64, vp, C.c_int]
    lib.vbx_fbank_windows.argtypes = [vp, i32, vp, i32, vp, C.c_int]
    lib.vbx_fbank_times.argtypes = [vp, vp]
    lib.vbx_fbank_destroy.argtypes = [vp]
    lib.vbx_resnet_create.argtypes = [vp, i32, vp, i64, C.POINTER(vp)]
    lib.vbx_resnet_input.argtypes = [vp, i32, i32, C.POINTER(vp)]
    lib.vbx_resnet_run.argtypes = [vp, i32, i32, vp, C.c_int, vp, C.c_int]
    lib.vbx_resnet_times.argtypes = [vp, vp]
    lib.vbx_resnet_destroy.argtypes = [vp]
    lib.vbx_resnet_conv_tile.argtypes = [i64, i32, C.POINTER(i32), C.POINTER(i32)]
    lib.vbx_resnet_conv.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, C.c_int, i32, i32, vp, i64]
    lib.vbx_resnet_stem.argtypes = [vp, i32, i32, vp, vp, vp, vp, i64]
    lib.vbx_resnet_pool.argtypes = [vp, i32, i32, vp, vp, i64]
    lib.vbx_resnet_set_gemm.argtypes = [vp, C.c_int]
    lib.vbx_resnet_gemm_in_effect.argtypes = [vp]
    lib.vbx_resnet_conv_gemm.argtypes = [vp, C.c_int, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, C.c_int, i32, i32, vp, i64, vp]
    lib.vbx_resnet_split_weights.argtypes = [i32, i32, vp, vp, vp]
    lib.vbx_fbank_windows_ragged.argtypes = [vp, i32, vp, vp, vp, C.c_int]
    lib.vbx_resnet_run_ragged.argtypes = [vp, i32, vp, vp, C.c_int, vp, C.c_int]
    lib.vbx_resnet_input_ragged.argtypes = [vp, i32, vp, C.POINTER(vp)]
    lib.vbx_resnet_conv_ragged.argtypes = [vp, C.c_int, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp, vp, C.c_int, i32, i32, vp, i64, vp]
    lib.vbx_resnet_stem_ragged.argtypes = [vp, i32, vp, vp, vp, vp, vp, i64]
    lib.vbx_resnet_pool_ragged.argtypes = [vp, i32, vp, vp, vp, i64]
    lib.vbx_fbank_run_raw.argtypes = [vp, i64, vp, i32, vp, vp, vp, i32, vp, i32, i32, C.POINTER(i64)]
    lib.vbx_fbank_get_signal.argtypes = [vp, i64, i64, vp, C.c_int]
    lib.vbx_fbank_dither_time.argtypes = [vp, C.POINTER(C.c_float)]
    lib.vbx_batch_set_reference.argtypes = [vp, C.c_int, vp, i32]
    lib.vbx_batch_get_scores.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]
    lib.vbx_score_posteriors.argtypes = [vp, i64, i32, vp, vp, i32, C.c_int, vp]
    lib.vbx_plda_covariance.argtypes = [vp, i64, i32, vp, vp, vp]
    lib.vbx_plda_covariance_resident.argtypes = [vp, vp, i64, i64, vp, vp]
    lib.vbx_plda_scores.argtypes = [vp, i64, i32, vp, i32, vp, vp, vp, C.POINTER(vp)]
    lib.vbx_plda_scores_resident.argtypes = [vp, vp, i64, i64, i32, vp, vp, vp, C.POINTER(vp)]
    lib.vbx_plda_score_lda.argtypes = [vp, i64, i64, i32, vp, vp, vp, vp]
    lib.vbx_xvectors_project_device.argtypes = [vp, i64, i32, i32, i32, vp, i64, vp, vp, vp, vp, vp, vp, C.POINTER(vp)]
    lib.vbx_rows_nan_flags.argtypes = [vp, vp, i64, i32, vp]
    lib.vbx_rttm_score.argtypes = [vp, i32, vp, vp, vp, vp, dbl, C.c_int, vp]
    lib.vbx_labels_score.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, dbl, C.c_int, vp, vp]
    lib.vbx_vad_energy.argtypes = [vp, i64, vp, i32, vp, i32, i32, dbl, dbl, i32, dbl, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.vbx_frame_counts.argtypes = [vp, i32, vp, vp, vp, vp, dbl, vp, vp, vp, i64]
    lib.vbx_labels_frame_counts.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, vp, dbl, vp, vp, vp, i64, vp]
    lib.vbx_resample_pcm.argtypes = [vp, i64, vp, i32, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.vbx_random_labels.argtypes = [vp, C.c_uint64, C.c_uint64, i64, i64, i32, vp]
    lib.vbx_batch_set_recording_random.argtypes = [vp, C.c_int, vp, i64, C.c_int, C.c_uint64, C.c_uint64, i64, dbl, vp, dbl, dbl, dbl]
    lib.vbx_turn_weights.argtypes = [vp, i64, vp, vp, i64, vp, vp, vp, i32, dbl, vp, vp, vp]
    lib.vbx_batch_set_recording_turns.argtypes = [vp, C.c_int, vp, i64, vp, vp, i64, vp, vp, vp, dbl, vp, dbl, dbl, dbl]
    lib.vbx_backend_class_sums.argtypes = [vp, i64, i32, vp, C.c_int, i32, vp, vp, vp]
    lib.vbx_backend_second_moments.argtypes = [vp, i64, i32, vp, i64, vp, vp]
    lib.vbx_backend_create.argtypes = [vp, i64, i32, vp, C.c_int, i32, vp, C.POINTER(vp)]
    lib.vbx_backend_stage1.argtypes = [vp, vp, vp, vp, C.POINTER(dbl)]
    lib.vbx_backend_stage2.argtypes = [vp, i32, vp, vp, vp, vp, C.POINTER(dbl)]
    lib.vbx_backend_destroy.argtypes = [vp]
    for name in ABI_SYMBOLS:
        fn = getattr(lib, name)          # AttributeError here = the .so does not export the ABI
        if name in ('vbx_scores_count', 'vbx_ark_index'):
            fn.restype = C.c_int64
        elif name == 'vbx_viterbi_last_ms':
            fn.restype = C.c_double
        elif name not in ('vbx_last_error', 'vbx_abi_version'):
            fn.restype = C.c_int
    _lib = lib
    return lib


class Fetch(C.Structure):
    """vbx_fetch (include/vbx_hip.h): one recording's result pointers for vbx_batch_get_results."""
    _fields_ = [('rec', C.c_int32), ('gamma', C.c_void_p), ('pi', C.c_void_p), ('Li', C.c_void_p), ('li_cap', C.c_int32),
                ('n_iters', C.c_int32), ('warned', C.c_int32), ('alpha', C.c_void_p), ('invL', C.c_void_p)]


class _PinnedBlock:
    """A block of pinned host memory from the library's pool (vbx_host_alloc); goes back to the pool with the last array on it."""

    def __init__(self, nbytes):
        p = C.c_void_p()
        rc = load().vbx_host_alloc(int(nbytes), C.byref(p))
        if rc != 0:
            raise VbxError(f'vbx_host_alloc({nbytes}) failed ({rc}): ' + (load().vbx_last_error(None) or b'').decode())
        self.ptr, self.nbytes = p.value, int(nbytes)

    def __del__(self):
        if sys.is_finalizing() or not getattr(self, 'ptr', None):
            return
        try:
            load().vbx_host_free(self.ptr)
        except Exception:
            pass
        self.ptr = None


def pinned_arrays(shapes, dtype=np.float64):
    """float64 arrays of the given shapes on ONE block of pinned host memory (the destination of choice for results: a
    copy out of HBM into such an array is a plain DMA; into ordinary memory it is staged and three to ten times slower).
    The block returns to the library's pool when the last of the arrays (or a view of one) is gone."""
    item = np.dtype(dtype).itemsize
    sizes = [int(np.prod(s)) * item for s in shapes]
    offs = np.concatenate([[0], np.cumsum([(n + 63) // 64 * 64 for n in sizes])])
    block = _PinnedBlock(max(int(offs[-1]), 64))
    raw = (C.c_char * block.nbytes).from_address(block.ptr)
    raw._vbx_owner = block                              # np.frombuffer keeps `raw` alive, `raw` keeps the block
    out = []
    for s, n, o in zip(shapes, sizes, offs):
        out.append(np.frombuffer(raw, dtype=dtype, count=n // item, offset=int(o)).reshape(s))
    return out


def experiment_env(name):
    """An environment variable that exists for A/B measurements only (second table): read only when
    VBX_AMD_EXPERIMENT=1, so that a stray variable in a production environment cannot change what the library runs."""
    return os.environ.get(name) if os.environ.get('VBX_AMD_EXPERIMENT') == '1' else None


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


SPLIT_NAMES = ('fp32-split', 'fp32s', 'f32-split')       # fp32 storage, the two GEMMs on f16 operand pairs (VBX_OPT_GEMM)


def precision_code(precision) -> int:
    if precision in (PREC_FP32, 'fp32', 'f32', 'float32', np.float32) or precision in SPLIT_NAMES:
        return PREC_FP32
    if precision in (PREC_FP64, 'fp64', 'f64', 'float64', np.float64):
        return PREC_FP64
    raise ValueError(f'unknown precision {precision!r}')


class Context:
    """One device + one HIP stream (vbx_ctx)."""

    def __init__(self, device: int = 0):
        self._lib = load()
        h = C.c_void_p()
        rc = self._lib.vbx_create(C.byref(h), int(device))
        if rc != 0:
            raise VbxError(f'vbx_create(device={device}) failed ({rc}): '
                           f'{self._lib.vbx_last_error(None).decode()}')
        self._h = h
        self.device = int(device)

    def check(self, rc: int, what: str):
        if rc != 0:
            raise VbxError(f'{what} failed ({rc}): {self._lib.vbx_last_error(self._h).decode()}')

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, hbm = C.c_int(), C.c_int64()
        self.check(self._lib.vbx_device_info(self._h, name, 256, C.byref(cus), C.byref(hbm)), 'vbx_device_info')
        return {'name': name.value.decode(), 'compute_units': cus.value, 'hbm_bytes': hbm.value}

    def close(self):
        if getattr(self, '_h', None):
            self._lib.vbx_destroy(self._h)
            self._h = None

    def __del__(self):
        if sys.is_finalizing():          # the HIP runtime may already be gone: leave the device memory to the process exit
            return
        try:
            self.close()
        except Exception:
            pass

    # ---- step-level entry points (parity tests) -------------------------------------------
    def forward_backward(self, lls, pi, loopProb, ip=None, precision='fp64', fb_algo=FB_AUTO, want_logs=False):
        lls = _f64(lls)
        T, S = lls.shape
        pi = _f64(pi)
        ip = _f64(ip)
        gamma = np.empty((T, S))
        entered = np.empty(S)
        tll = C.c_double()
        lfw = np.empty((T, S)) if want_logs else None
        lbw = np.empty((T, S)) if want_logs else None
        self.check(self._lib.vbx_forward_backward(self._h, T, S, _ptr(lls), _ptr(pi), _ptr(ip), float(loopProb),
                                                  precision_code(precision), int(fb_algo), _ptr(gamma),
                                                  C.byref(tll), _ptr(entered), _ptr(lfw), _ptr(lbw)),
                   'vbx_forward_backward')
        return gamma, tll.value, entered, lfw, lbw

    def forward_backward_dense(self, lls, tr, ip, precision='fp64', want_logs=True):
        """forward_backward (VBx.py:146-175) for any S x S transition matrix."""
        lls, tr, ip = _f64(lls), _f64(tr), _f64(ip)
        T, S = lls.shape
        assert tr.shape == (S, S) and ip.shape == (S,)
        gamma = np.empty((T, S))
        lfw = np.empty((T, S)) if want_logs else None
        lbw = np.empty((T, S)) if want_logs else None
        tll = C.c_double()
        self.check(self._lib.vbx_forward_backward_dense(self._h, T, S, _ptr(lls), _ptr(tr), _ptr(ip),
                                                        precision_code(precision), _ptr(gamma), C.byref(tll),
                                                        _ptr(lfw), _ptr(lbw)), 'vbx_forward_backward_dense')
        return gamma, tll.value, lfw, lbw

    def mstep(self, X, Phi, gamma, Fa, Fb, precision='fp64'):
        X, Phi, gamma = _f64(X), _f64(Phi), _f64(gamma)
        T, D = X.shape
        S = gamma.shape[1]
        alpha, invL = np.empty((S, D)), np.empty((S, D))
        self.check(self._lib.vbx_mstep(self._h, T, S, D, _ptr(X), _ptr(Phi), _ptr(gamma), float(Fa), float(Fb),
                                       precision_code(precision), _ptr(alpha), _ptr(invL)), 'vbx_mstep')
        return alpha, invL

    def loglik(self, X, Phi, alpha, invL, Fa, precision='fp64'):
        X, Phi, alpha, invL = _f64(X), _f64(Phi), _f64(alpha), _f64(invL)
        T, D = X.shape
        S = alpha.shape[0]
        out = np.empty((T, S))
        self.check(self._lib.vbx_loglik(self._h, T, S, D, _ptr(X), _ptr(Phi), _ptr(alpha), _ptr(invL), float(Fa),
                                        precision_code(precision), _ptr(out)), 'vbx_loglik')
        return out

    def viterbi(self, lls, pi, loopProb, ip=None):
        """(path int32 [T], logp): the most probable state sequence under forward_backward's model (vbx_viterbi)."""
        lls, pi, ip = _f64(lls), _f64(pi), _f64(ip)
        T, S = lls.shape
        assert pi.shape == (S,) and (ip is None or ip.shape == (S,))
        path = np.empty(T, dtype=np.int32)
        logp = C.c_double()
        self.check(self._lib.vbx_viterbi(self._h, T, S, _ptr(lls), _ptr(pi), _ptr(ip), float(loopProb), _ptr(path),
                                         C.byref(logp)), 'vbx_viterbi')
        return path, logp.value

    def score_posteriors(self, gamma, ref, n_ref=None, precision='fp64'):
        """Confusion block C[2][n_ref][S] of responsibilities ``gamma[T,S]`` against labels ``ref[T]`` (vbx_score_posteriors):
        C[0] = ref_mx^T gamma, C[1] = ref_mx^T -log(gamma + nextafter(0, 1)); ``n_ref`` defaults to max(ref) + 1."""
        gamma = _f64(gamma)
        ref = np.ascontiguousarray(ref, dtype=np.int32)
        T, S = gamma.shape
        assert ref.shape == (T,)
        n_ref = int(ref.max()) + 1 if n_ref is None else int(n_ref)
        conf = np.empty((2, max(n_ref, 0), S))
        self.check(self._lib.vbx_score_posteriors(self._h, T, S, _ptr(gamma), _ptr(ref), n_ref, precision_code(precision),
                                                  _ptr(conf)), 'vbx_score_posteriors')
        return conf


class XVectors:
    """The x-vectors of an archive after the driver's projections, resident in HBM (vbx_xvectors): ``xproj`` (the rows
    cos_similarity works on, vbhmm.py:125-129) and ``fea`` (the input of VBx(), vbhmm.py:153)."""

    def __init__(self, ctx: Context, x, mean1, lda, mean2, plda_mu, plda_tr, fea_dim):
        self.ctx, self._lib = ctx, ctx._lib
        x = np.ascontiguousarray(x)
        if x.dtype != np.float32:
            x = np.ascontiguousarray(x, dtype=np.float64)
        mean1, lda, mean2, plda_mu, plda_tr = _f64(mean1), _f64(lda), _f64(mean2), _f64(plda_mu), _f64(plda_tr)
        n, din = x.shape
        dl = lda.shape[1]
        assert lda.shape == (din, dl) and mean1.shape == (din,) and mean2.shape == (dl,) and plda_mu.shape == (dl,)
        assert plda_tr.shape == (dl, dl) and 0 < fea_dim <= dl
        h = C.c_void_p()
        ctx.check(self._lib.vbx_xvectors_project(ctx._h, n, din, dl, int(fea_dim), _ptr(x),
                                                 VBX_F32 if x.dtype == np.float32 else VBX_F64, _ptr(mean1), _ptr(lda),
                                                 _ptr(mean2), _ptr(plda_mu), _ptr(plda_tr), C.byref(h)),
                  'vbx_xvectors_project')
        self._h, self.n, self.dl, self.fea_dim = h, n, dl, int(fea_dim)

    @classmethod
    def from_device(cls, ctx: Context, x_ptr, n_src, Din, rows, mean1, lda, mean2, plda_mu, plda_tr, fea_dim):
        """The same from x-vectors that already lie in HBM (vbx_xvectors_project_device): f32 [n_src][Din] at the device
        address ``x_ptr``, of which the rows ``rows`` are kept (strictly increasing indices; None: all of them).  Only the
        indices go up; the result has the bits ``XVectors(ctx, x[rows], ...)`` gives from a host copy."""
        self = cls.__new__(cls)
        self.ctx, self._lib, self._h = ctx, ctx._lib, None
        mean1, lda, mean2, plda_mu, plda_tr = _f64(mean1), _f64(lda), _f64(mean2), _f64(plda_mu), _f64(plda_tr)
        n_src, din = int(n_src), int(Din)
        dl = lda.shape[1]
        assert lda.shape == (din, dl) and mean1.shape == (din,) and mean2.shape == (dl,) and plda_mu.shape == (dl,)
        assert plda_tr.shape == (dl, dl)
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        n = n_src if rows is None else rows.shape[0]
        h = C.c_void_p()
        ctx.check(self._lib.vbx_xvectors_project_device(ctx._h, n_src, din, dl, int(fea_dim), C.c_void_p(x_ptr), n, _ptr(rows),
                                                        _ptr(mean1), _ptr(lda), _ptr(mean2), _ptr(plda_mu), _ptr(plda_tr),
                                                        C.byref(h)), 'vbx_xvectors_project_device')
        self._h, self.n, self.dl, self.fea_dim = h, n, dl, int(fea_dim)
        return self

    def get(self, which, row0=0, nrows=None):
        """rows of 'xproj' (or 0) or 'fea' (or 1) as a float64 array (tests; the driver never needs them on the host)."""
        xproj = which == 'xproj' or (which is not None and not isinstance(which, str) and int(which) == 0)
        nrows = self.n - row0 if nrows is None else nrows
        out = np.empty((nrows, self.dl if xproj else self.fea_dim))
        self.ctx.check(self._lib.vbx_xvectors_get(self._h, 0 if xproj else 1, int(row0), int(nrows), _ptr(out)),
                       'vbx_xvectors_get')
        return out

    def close(self):
        if getattr(self, '_h', None):
            self._lib.vbx_xvectors_destroy(self._h)
            self._h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class FbankDevice:
    """The filterbank front end of one sample rate on one device (vbx_fbank): the folded f64 frame operator stays
    resident; every run replaces the features of the previous one."""

    def __init__(self, ctx: Context, winlen, shift, nfft, window, mel, preemph=0.97):
        self.ctx, self._lib = ctx, ctx._lib
        window, mel = _f64(window), _f64(mel)
        assert window.shape == (winlen,) and mel.shape[0] == nfft // 2 + 1
        h = C.c_void_p()
        ctx.check(self._lib.vbx_fbank_create(ctx._h, int(winlen), int(shift), int(nfft), int(mel.shape[1]), _ptr(window),
                                             _ptr(mel), float(preemph), C.byref(h)), 'vbx_fbank_create')
        self._h, self.n_mel, self.rows = h, int(mel.shape[1]), 0

    def run(self, signal, segs, lc=150, rc=149):
        """signal f64 [n]; segs int64 [n_seg][2] (first sample, samples).  Returns the number of feature rows."""
        signal = _f64(signal)
        segs = np.ascontiguousarray(segs, dtype=np.int64).reshape(-1, 2)
        rows = C.c_int64()
        self.ctx.check(self._lib.vbx_fbank_run(self._h, signal.shape[0], _ptr(signal), segs.shape[0], _ptr(segs), int(lc),
                                               int(rc), C.byref(rows)), 'vbx_fbank_run')
        self.rows = rows.value
        return self.rows

    def run_raw(self, samples, rec, seeds, levels, segs, lc=150, rc=149):
        """samples int16 [n] of the recordings rec int64 [n_rec][2] (first sample, samples), dithered on the device with
        np.random.RandomState(seeds[r])'s stream at levels[r] (vbx_fbank_run_raw); then as run()."""
        samples = np.ascontiguousarray(samples, dtype=np.int16).reshape(-1)
        rec = np.ascontiguousarray(rec, dtype=np.int64).reshape(-1, 2)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
        levels = _f64(levels).reshape(-1)
        if not (rec.shape[0] == seeds.shape[0] == levels.shape[0]):
            raise ValueError(f'run_raw: {rec.shape[0]} recordings, {seeds.shape[0]} seeds, {levels.shape[0]} levels')
        segs = np.ascontiguousarray(segs, dtype=np.int64).reshape(-1, 2)
        rows = C.c_int64()
        self.ctx.check(self._lib.vbx_fbank_run_raw(self._h, samples.shape[0], _ptr(samples), rec.shape[0], _ptr(rec),
                                                   _ptr(seeds), _ptr(levels), segs.shape[0], _ptr(segs), int(lc), int(rc),
                                                   C.byref(rows)), 'vbx_fbank_run_raw')
        self.rows = rows.value
        return self.rows

    def signal(self, first, n, dst_ptr=None):
        """samples [first, first + n) of the f64 signal of the last run; into a host array, or into device memory."""
        out = None
        if dst_ptr is None:
            out = np.empty(int(n), dtype=np.float64)
            dst_ptr = out.ctypes.data
        self.ctx.check(self._lib.vbx_fbank_get_signal(self._h, int(first), int(n), C.c_void_p(dst_ptr), int(out is None)),
                       'vbx_fbank_get_signal')
        return out

    def dither_time(self):
        """device ms of the dither kernel of the last run (0.0 after a run that was given the dithered signal)."""
        ms = C.c_float()
        self.ctx.check(self._lib.vbx_fbank_dither_time(self._h, C.byref(ms)), 'vbx_fbank_dither_time')
        return float(ms.value)

    def get(self, which, row0, nrows, dst_ptr=None):
        """rows of the CMN features ('fea', f32) or the log-Mel rows ('logmel', f64); into a host array, or into device
        memory at dst_ptr (returns None then)."""
        w = 0 if which == 'fea' else 1
        out = None
        if dst_ptr is None:
            out = np.empty((nrows, self.n_mel), dtype=np.float32 if w == 0 else np.float64)
            dst_ptr = out.ctypes.data
        self.ctx.check(self._lib.vbx_fbank_get(self._h, w, int(row0), int(nrows), C.c_void_p(dst_ptr), int(out is None)),
                       'vbx_fbank_get')
        return out

    def windows(self, starts, length, dst_ptr=None):
        """[n][n_mel][length] f32 windows of the CMN features from rows starts[n] (host array, or into device memory)."""
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        out = None
        if dst_ptr is None:
            out = np.empty((starts.shape[0], self.n_mel, int(length)), dtype=np.float32)
            dst_ptr = out.ctypes.data
        self.ctx.check(self._lib.vbx_fbank_windows(self._h, starts.shape[0], _ptr(starts), int(length), C.c_void_p(dst_ptr),
                                                   int(out is None)), 'vbx_fbank_windows')
        return out

    def windows_ragged(self, starts, lengths, dst_ptr=None):
        """Windows of mixed lengths (vbx_fbank_windows_ragged): window w is lengths[w] rows from row starts[w]; their
        [n_mel][lengths[w]] f32 blocks end to end, as one flat host array or into device memory at dst_ptr."""
        starts = np.ascontiguousarray(starts, dtype=np.int64).reshape(-1)
        lengths = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
        if starts.shape != lengths.shape:
            raise ValueError(f'windows_ragged: {starts.shape[0]} starts, {lengths.shape[0]} lengths')
        out = None
        if dst_ptr is None:
            out = np.empty(self.n_mel * int(np.maximum(lengths, 0).sum(dtype=np.int64)), dtype=np.float32)
            dst_ptr = out.ctypes.data
        self.ctx.check(self._lib.vbx_fbank_windows_ragged(self._h, starts.shape[0], _ptr(starts), _ptr(lengths),
                                                          C.c_void_p(dst_ptr), int(out is None)), 'vbx_fbank_windows_ragged')
        return out

    def times(self):
        """device ms of the last run: upload, frame kernel, CMN, and of the last windows call: gather."""
        ms = np.zeros(4, dtype=np.float32)
        self.ctx.check(self._lib.vbx_fbank_times(self._h, _ptr(ms)), 'vbx_fbank_times')
        return dict(zip(('upload', 'frame', 'cmn', 'gather'), ms.astype(float).tolist()))

    def close(self):
        if getattr(self, '_h', None):
            self._lib.vbx_fbank_destroy(self._h)
            self._h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class ResNetDevice:
    """The x-vector network resident on one device (vbx_resnet): the folded f32 parameters and a workspace that grows to
    the largest batch seen."""

    TIMES = ('stem', 'layer1', 'layer2', 'layer3', 'layer4', 'pool_embed')

    def __init__(self, ctx: Context, params, embed_dim, gemm='exact'):
        self.ctx, self._lib = ctx, ctx._lib
        if gemm not in GEMM_NAMES:
            raise ValueError(f"gemm must be 'exact' or 'split', got {gemm!r}")
        params = np.ascontiguousarray(params, dtype=np.float32)
        h = C.c_void_p()
        ctx.check(self._lib.vbx_resnet_create(ctx._h, int(embed_dim), _ptr(params), params.size, C.byref(h)),
                  'vbx_resnet_create')
        self._h, self.embed_dim = h, int(embed_dim)
        if gemm != 'exact':
            self.set_gemm(gemm)

    def set_gemm(self, gemm):
        """'exact' or 'split' for the runs that follow (vbx_resnet_set_gemm)."""
        self.ctx.check(self._lib.vbx_resnet_set_gemm(self._h, GEMM_NAMES[gemm]), 'vbx_resnet_set_gemm')

    def gemm_in_effect(self) -> str:
        """How the last run multiplied: 'exact' or 'split'."""
        return 'split' if int(self._lib.vbx_resnet_gemm_in_effect(self._h)) == GEMM_SPLIT else 'exact'

    def input_buffer(self, n, T) -> int:
        """Device address of the network's own input buffer [n][64][T] f32 (vbx_resnet_input)."""
        p = C.c_void_p()
        self.ctx.check(self._lib.vbx_resnet_input(self._h, int(n), int(T), C.byref(p)), 'vbx_resnet_input')
        return p.value

    def _run(self, name, n, shape, x, x_ptr, out_ptr):
        """One run through the C entry `name` (shape: its arguments after the handle): the host array x or device memory
        at x_ptr; into a new host array, or into device memory at out_ptr (returns None then)."""
        src, on_dev = (_ptr(x), 0) if x_ptr is None else (C.c_void_p(x_ptr), 1)
        out = None
        if out_ptr is None:
            out = np.empty((int(n), self.embed_dim), dtype=np.float32)
            out_ptr = out.ctypes.data
        self.ctx.check(getattr(self._lib, name)(self._h, *shape, src, on_dev, C.c_void_p(out_ptr), int(out is None)), name)
        return out

    def run(self, n, T, x=None, x_ptr=None, out_ptr=None):
        """Embeddings [n][E] f32 of the host array x [n][64][T], or of device memory at x_ptr; into a new host array, or
        into device memory at out_ptr (returns None then)."""
        if x_ptr is None:
            x = np.ascontiguousarray(x, dtype=np.float32)
            assert x.shape == (n, 64, T)
        return self._run('vbx_resnet_run', n, (int(n), int(T)), x, x_ptr, out_ptr)

    def input_buffer_ragged(self, lengths) -> int:
        """Device address of the network's own input buffer for a ragged batch: 64 sum(lengths) f32 (vbx_resnet_input_ragged)."""
        lengths = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
        p = C.c_void_p()
        self.ctx.check(self._lib.vbx_resnet_input_ragged(self._h, lengths.shape[0], _ptr(lengths), C.byref(p)),
                       'vbx_resnet_input_ragged')
        return p.value

    def run_ragged(self, lengths, x=None, x_ptr=None, out_ptr=None):
        """Embeddings [n][E] f32 of n windows of lengths[b] frames (vbx_resnet_run_ragged): x the flat host array of their
        [64][lengths[b]] blocks end to end, or device memory at x_ptr; into a new host array, or device memory at out_ptr."""
        lengths = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
        n = lengths.shape[0]
        if x_ptr is None:
            x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
            if x.size != 64 * int(np.maximum(lengths, 0).sum(dtype=np.int64)):
                raise ValueError(f'run_ragged: x holds {x.size} values, the lengths ask for 64 x {int(lengths.sum())}')
        return self._run('vbx_resnet_run_ragged', n, (n, _ptr(lengths)), x, x_ptr, out_ptr)

    def times(self):
        ms = np.zeros(len(self.TIMES), dtype=np.float32)
        self.ctx.check(self._lib.vbx_resnet_times(self._h, _ptr(ms)), 'vbx_resnet_times')
        return dict(zip(self.TIMES, ms.astype(float).tolist()))

    def close(self):
        if getattr(self, '_h', None):
            self._lib.vbx_resnet_destroy(self._h)
            self._h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


# ---- step-level entry points of the network (kernel tests) ------------------------------------
RN_SENTINEL = 0x7FC5A5A5     # a NaN no kernel produces, compared as uint32: a kernel may legitimately write NaN
RN_PAD = 4096                # floats of guard band either side of an output


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _guarded(count, pad):
    return np.full(int(count) + 2 * int(pad), RN_SENTINEL, dtype=np.uint32).view(np.float32)


def _unguard(buf, count, pad):
    """-> (payload, guard-band words that changed, payload words still holding the sentinel)"""
    bits = buf.view(np.uint32)
    guard = int(np.count_nonzero(bits[:pad] != RN_SENTINEL) + np.count_nonzero(bits[pad + count:] != RN_SENTINEL))
    unwritten = int(np.count_nonzero(bits[pad:pad + count] == RN_SENTINEL))
    return buf[pad:pad + count].copy(), guard, unwritten


def resnet_conv_tile(M, Cout):
    """(BN, BM) the network's dispatcher picks for M output positions x Cout channels (host code, no device)."""
    bn, bm = C.c_int32(), C.c_int32()
    rc = load().vbx_resnet_conv_tile(int(M), int(Cout), C.byref(bn), C.byref(bm))
    if rc != 0:
        raise VbxError(f'vbx_resnet_conv_tile(M={M}, Cout={Cout}) failed ({rc})')
    return bn.value, bm.value


def _pack(arrays):
    """Host arrays end to end as one flat f32 array (None: None)."""
    return None if arrays is None else np.concatenate([_f32(a).reshape(-1) for a in arrays])


def _widths(n, W):
    """The widths of n windows given as one int for all (what the uniform C entries take) or as n ints (what the *_ragged ones
    take): -> (int32 [n], the C argument)."""
    if np.ndim(W) == 0:
        return np.full(n, int(W), dtype=np.int32), int(W)
    W = np.ascontiguousarray(W, dtype=np.int32)
    return W, _ptr(W)


def _step(ctx, name, args, count, pad):
    """One step-level C entry `name` on host arrays: args(buf, pad) gives its arguments after the context, buf a guarded buffer
    for its `count` output floats.  -> (the output, flat; guard-band words the kernel changed; output words it left unwritten)."""
    buf = _guarded(count, pad)
    ctx.check(getattr(ctx._lib, name)(ctx._h, *args(_ptr(buf), int(pad))), name)
    return _unguard(buf, count, pad)


def _split(y, shapes):
    """The windows' outputs (shapes) out of y, where they lie end to end."""
    offs = np.cumsum([0] + [int(np.prod(sh)) for sh in shapes])
    return [y[offs[b]:offs[b + 1]].reshape(sh) for b, sh in enumerate(shapes)]


def _conv_step(ctx, name, gemm, n, H, W, Cin, x, w, bias, ks, stride, res, relu, tile, pad):
    """One convolution through the C entry `name` (gemm None: vbx_resnet_conv, which takes no mode and records no amax_y) of n
    windows [H][W_b][Cin], x and res (or None) flat, W as _widths takes it.  -> (y flat, the windows' output shapes
    (Ho, Wo_b, Cout), guard, unwritten, amax_y [n])."""
    x, w, bias, res = _f32(x), _f32(w), _f32(bias), _f32(res)
    widths, Warg = _widths(n, W)
    Cout = w.shape[1]
    s = max(int(stride), 1)
    shapes = [((H - 1) // s + 1, (int(Wb) - 1) // s + 1, Cout) for Wb in widths]
    count = sum(int(np.prod(sh)) for sh in shapes)
    assert w.shape == (ks * ks * Cin, Cout) and bias.shape == (Cout,) and (res is None or res.size == count)
    bn, bm = tile or (0, 0)
    amax = np.zeros(max(n, 1), dtype=np.float32)
    head, tail = ((), ()) if gemm is None else ((GEMM_NAMES[gemm],), (_ptr(amax),))

    def args(buf, pad):
        return head + (int(ks), int(stride), n, H, Warg, Cin, Cout, _ptr(x), _ptr(w), _ptr(bias), _ptr(res), int(bool(relu)),
                       int(bn), int(bm), buf, pad) + tail
    y, guard, unwritten = _step(ctx, name, args, count, pad)
    return y, shapes, guard, unwritten, amax[:n]


def _conv_stacked(ctx, name, gemm, x, w, bias, ks, stride, res, relu, tile, pad):
    """_conv_step on one array x [n][H][W][Cin] through a uniform entry: -> (y [n][Ho][Wo][Cout], guard, unwritten, amax_y)."""
    n, H, W, Cin = np.shape(x)
    y, shapes, guard, unwritten, amax = _conv_step(ctx, name, gemm, n, H, W, Cin, x, w, bias, ks, stride, res, relu, tile, pad)
    return y.reshape((n,) + shapes[0]), guard, unwritten, amax


def resnet_conv(ctx: 'Context', x, w, bias, ks, stride, res=None, relu=False, tile=None, pad=RN_PAD):
    """One convolution of the network (vbx_resnet_conv): x [n][H][W][Cin], w [ks ks Cin][Cout], bias [Cout], res
    [n][Ho][Wo][Cout] or None; tile None (the dispatcher's) or (BN, BM).  -> (y [n][Ho][Wo][Cout], guard-band words the
    kernel changed, output words it left unwritten)."""
    return _conv_stacked(ctx, 'vbx_resnet_conv', None, x, w, bias, ks, stride, res, relu, tile, pad)[:3]


def resnet_conv_gemm(ctx: 'Context', gemm, x, w, bias, ks, stride, res=None, relu=False, tile=None, pad=RN_PAD):
    """resnet_conv in either mode (vbx_resnet_conv_gemm; gemm 'exact' or 'split').  -> (y, guard, unwritten, amax_y [n]: max |y|
    over the finite outputs of every image as the split kernel records it for its consumer; zeros in the exact mode)."""
    return _conv_stacked(ctx, 'vbx_resnet_conv_gemm', gemm, x, w, bias, ks, stride, res, relu, tile, pad)


def resnet_conv_ragged(ctx: 'Context', gemm, xs, w, bias, ks, stride, res=None, relu=False, tile=None, pad=RN_PAD):
    """One convolution over a ragged batch (vbx_resnet_conv_ragged; gemm 'exact' or 'split'): xs a list of [H][W_b][Cin]
    windows, res a list of [Ho][Wo_b][Cout] or None.  -> (ys: the list of [Ho][Wo_b][Cout] outputs, guard, unwritten, amax_y [n])."""
    xs = [_f32(x) for x in xs]
    H, _, Cin = xs[0].shape
    assert all(x.ndim == 3 and x.shape[0] == H and x.shape[2] == Cin for x in xs)
    y, shapes, guard, unwritten, amax = _conv_step(ctx, 'vbx_resnet_conv_ragged', gemm, len(xs), H, [x.shape[1] for x in xs], Cin,
                                                   _pack(xs), w, bias, ks, stride, _pack(res), relu, tile, pad)
    return _split(y, shapes), guard, unwritten, amax


def _stem_step(ctx, name, n, T, x, w, bias, pad):
    """The stem through the C entry `name`: n windows [64][T_b], x flat, T as _widths takes it.  -> (y flat, the lengths [n],
    guard, unwritten)."""
    x, w, bias = _f32(x), _f32(w), _f32(bias)
    assert w.shape == (9, 32) and bias.shape == (32,)
    T, Targ = _widths(n, T)
    count = 64 * 32 * int(T.sum(dtype=np.int64))
    return (T,) + _step(ctx, name, lambda buf, pad: (n, Targ, _ptr(x), _ptr(w), _ptr(bias), buf, pad), count, pad)


def resnet_stem(ctx: 'Context', x, w, bias, pad=RN_PAD):
    """The stem (vbx_resnet_stem): x [n][64][T], w [9][32], bias [32] -> (y [n][64][T][32], guard, unwritten)."""
    n, mel, T = np.shape(x)
    assert mel == 64
    _, y, guard, unwritten = _stem_step(ctx, 'vbx_resnet_stem', n, T, x, w, bias, pad)
    return y.reshape(n, 64, T, 32), guard, unwritten


def resnet_stem_ragged(ctx: 'Context', xs, w, bias, pad=RN_PAD):
    """The stem over a ragged batch (vbx_resnet_stem_ragged): xs a list of [64][T_b] -> (list of [64][T_b][32], guard, unwritten)."""
    xs = [_f32(x) for x in xs]
    assert all(x.ndim == 2 and x.shape[0] == 64 for x in xs)
    T, y, guard, unwritten = _stem_step(ctx, 'vbx_resnet_stem_ragged', len(xs), [x.shape[1] for x in xs], _pack(xs), w, bias, pad)
    return _split(y, [(64, int(t), 32) for t in T]), guard, unwritten


def _pool_step(ctx, name, n, W4, x, pad):
    """Statistics pooling through the C entry `name`: n windows [8][W4_b][1024], x flat, W4 as _widths takes it.  -> (out
    [n][16384], guard, unwritten)."""
    x = _f32(x)
    W4, W4arg = _widths(n, W4)                                # (W4: kept while W4arg points into it)
    out, guard, unwritten = _step(ctx, name, lambda buf, pad: (n, W4arg, _ptr(x), buf, pad), n * 16384, pad)
    return out.reshape(n, 16384), guard, unwritten


def resnet_pool(ctx: 'Context', x, pad=RN_PAD):
    """Statistics pooling (vbx_resnet_pool): x [n][8][W4][1024] -> (out [n][16384], guard, unwritten)."""
    n, h, W4, c = np.shape(x)
    assert h == 8 and c == 1024
    return _pool_step(ctx, 'vbx_resnet_pool', n, W4, x, pad)


def resnet_pool_ragged(ctx: 'Context', xs, pad=RN_PAD):
    """Statistics pooling over a ragged batch (vbx_resnet_pool_ragged): xs a list of [8][W4_b][1024] -> (out [n][16384],
    guard, unwritten)."""
    xs = [_f32(x) for x in xs]
    assert all(x.ndim == 3 and x.shape[0] == 8 and x.shape[2] == 1024 for x in xs)
    return _pool_step(ctx, 'vbx_resnet_pool_ragged', len(xs), [x.shape[1] for x in xs], _pack(xs), pad)


def resnet_split_weights(w):
    """The library's own split of a weight matrix w [K][Cout] (vbx_resnet_split_weights, host code): -> (frag uint16
    [K / 16][Cout / 32][2][64][8], e int32 [Cout])."""
    w = _f32(w)
    K, Cout = w.shape
    frag = np.zeros((max(K // 16, 1), max(Cout // 32, 1), 2, 64, 8), dtype=np.uint16)
    e = np.zeros(Cout, dtype=np.int32)
    rc = load().vbx_resnet_split_weights(K, Cout, _ptr(w), _ptr(frag), _ptr(e))
    if rc != 0:
        raise VbxError(f'vbx_resnet_split_weights(K={K}, Cout={Cout}) failed ({rc})')
    return frag, e


class Scores:
    """A vector of float64 scores resident in HBM (vbx_scores): the T x T cosine similarities of the AHC
    initialisation, or any scores handed to the two-Gaussian calibration."""

    def __init__(self, ctx: Context, handle):
        self.ctx, self._lib, self._h = ctx, ctx._lib, handle

    @classmethod
    def cos_similarity(cls, ctx: Context, x):
        x = _f64(x)
        h = C.c_void_p()
        ctx.check(ctx._lib.vbx_cos_similarity(ctx._h, x.shape[0], x.shape[1], _ptr(x), C.byref(h)), 'vbx_cos_similarity')
        return cls(ctx, h)

    @classmethod
    def cos_similarity_resident(cls, ctx: Context, xv: 'XVectors', row0, T):
        """cos_similarity of rows [row0, row0 + T) of the projected x-vectors already in HBM."""
        h = C.c_void_p()
        ctx.check(ctx._lib.vbx_cos_similarity_resident(ctx._h, xv._h, int(row0), int(T), C.byref(h)),
                  'vbx_cos_similarity_resident')
        return cls(ctx, h)

    @classmethod
    def plda(cls, ctx: Context, x, mu, proj, acvar):
        """Dense PLDA scores (kaldi_ivector_plda_scoring_dense after its host part) of the rows ``x`` [T][D]: ``proj``
        [D][d] is the reference's ``PCA . wccn``, ``acvar`` [d] the across-class variances.  The matrix is symmetric to the
        last bit."""
        x, mu, proj, acvar = _f64(x), _f64(mu), _f64(proj), _f64(acvar)
        assert x.ndim == 2 and proj.shape == (x.shape[1], acvar.size) and mu.shape == (x.shape[1],)
        h = C.c_void_p()
        ctx.check(ctx._lib.vbx_plda_scores(ctx._h, x.shape[0], x.shape[1], _ptr(x), acvar.size, _ptr(mu), _ptr(proj),
                                           _ptr(acvar), C.byref(h)), 'vbx_plda_scores')
        return cls(ctx, h)

    @classmethod
    def plda_resident(cls, ctx: Context, xv: 'XVectors', row0, T, mu, proj, acvar):
        """Dense PLDA scores of rows [row0, row0 + T) of the projected x-vectors already in HBM."""
        mu, proj, acvar = _f64(mu), _f64(proj), _f64(acvar)
        assert proj.shape == (xv.dl, acvar.size) and mu.shape == (xv.dl,)
        h = C.c_void_p()
        ctx.check(ctx._lib.vbx_plda_scores_resident(ctx._h, xv._h, int(row0), int(T), acvar.size, _ptr(mu), _ptr(proj),
                                                    _ptr(acvar), C.byref(h)), 'vbx_plda_scores_resident')
        return cls(ctx, h)

    @classmethod
    def upload(cls, ctx: Context, s):
        s = _f64(s).reshape(-1)
        h = C.c_void_p()
        ctx.check(ctx._lib.vbx_scores_upload(ctx._h, s.size, _ptr(s), C.byref(h)), 'vbx_scores_upload')
        return cls(ctx, h)

    def __len__(self):
        return int(self._lib.vbx_scores_count(self._h))

    def get(self, offset=0, count=None, out=None):
        count = len(self) - offset if count is None else count
        if out is None:
            out = np.empty(count)
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.size == count
        self.ctx.check(self._lib.vbx_scores_get(self._h, int(offset), int(count), _ptr(out)), 'vbx_scores_get')
        return out

    def get_condensed(self, T, scale=1.0):
        """Strict upper triangle of ``scale * S`` (S = these scores as a T x T matrix), row by row: the vector form
        of ``scipy.spatial.distance.squareform``."""
        out = np.empty(int(T) * (int(T) - 1) // 2)
        self.ctx.check(self._lib.vbx_scores_get_condensed(self._h, int(T), float(scale), _ptr(out)),
                       'vbx_scores_get_condensed')
        return out

    def linkage_average(self, T):
        """``linkage(squareform(-S), 'average')`` for the T x T similarities held here, computed on the device (the scores
        are consumed); the linkage matrix [T - 1][4].  Below 256 clusters, and in the chain form
        (``VBX_AMD_LINKAGE_DEVICE=chain``), bit for bit what ``linkage_average`` gives on the host.  The default from 256
        clusters on merges in rounds of reciprocal pairs: the same tree (columns 0, 1, 3) wherever the heights are
        distinct, every height within ``max(16 ulp, 1e-15 max|S|)`` of the host's and within ``4 * 2**-53 * depth * max|S|``
        of the exact mean pairwise distance (``depth``: the node's height in the tree); with tied heights a valid
        average-linkage dendrogram."""
        Z = np.empty((max(int(T) - 1, 0), 4))
        self.ctx.check(self._lib.vbx_scores_linkage_average(self._h, int(T), _ptr(Z)), 'vbx_scores_linkage_average')
        return Z

    def two_gmm_calib(self, niters=20, want_llr=True):
        thr = C.c_double()
        llr = np.empty(len(self)) if want_llr else None
        self.ctx.check(self._lib.vbx_scores_two_gmm_calib(self._h, int(niters), C.byref(thr), _ptr(llr)),
                       'vbx_scores_two_gmm_calib')
        return thr.value, llr

    def close(self):
        if getattr(self, '_h', None):
            self._lib.vbx_scores_destroy(self._h)
            self._h = None

    def __del__(self):
        if sys.is_finalizing():          # the HIP runtime may already be gone: leave the device memory to the process exit
            return
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """A set of recordings resident in HBM (vbx_batch)."""

    def __init__(self, ctx: Context, T, S, D: int, precision='fp32', max_iters: int = 40, streams: int = 0):
        """``streams``: HIP streams (sub-batches) of the batch, 0 = the library's choice (vbx_batch_create_streams); a sweep
        over one long recording -- few recordings, many chunks -- asks for its streams here."""
        self.ctx = ctx
        self._lib = ctx._lib
        self.T = [int(t) for t in T]
        self.S = [int(s) for s in S]
        self.D = int(D)
        self.n = len(self.T)
        self.precision = precision_code(precision)
        self.max_iters = int(max_iters)
        h = C.c_void_p()
        Ta = (C.c_int64 * self.n)(*self.T)
        Sa = (C.c_int32 * self.n)(*self.S)
        ctx.check(self._lib.vbx_batch_create_streams(ctx._h, self.n, Ta, Sa, self.D, self.precision, self.max_iters,
                                                     int(streams or 0), C.byref(h)), 'vbx_batch_create_streams')
        self._h = h
        self._held = []                                    # arrays an asynchronous upload still reads (set_async_upload)
        self._n_ref = {}                                   # recording -> label count it is scored against (set_reference)
        self._async = False
        def choice(var, value, table):
            if value not in table:
                raise ValueError(f'{var}={value!r}: expected one of {", ".join(map(repr, table))}')
            return table[value]
        algo = experiment_env('VBX_AMD_FB_ALGO')          # 'sequential' | 'chunked' (default: auto)
        if algo:
            self.set_option(OPT_FB_ALGO, choice('VBX_AMD_FB_ALGO', algo, {'auto': FB_AUTO, 'sequential': FB_SEQUENTIAL,
                                                                          'chunked': FB_CHUNKED}))
        # VBX_OPT_GEMM: the precision argument decides where it names a mode ('fp32-split'); VBX_AMD_GEMM = exact | split
        # decides for a plain 'fp32' -- an explicit argument is never overridden by the environment, in either direction
        gemm = os.environ.get('VBX_AMD_GEMM')
        if gemm:
            choice('VBX_AMD_GEMM', gemm, {'exact': GEMM_EXACT, 'split': GEMM_SPLIT})
        if isinstance(precision, str) and precision in SPLIT_NAMES:
            gemm = 'split'
        if gemm:
            self.set_option(OPT_GEMM, {'exact': GEMM_EXACT, 'split': GEMM_SPLIT}[gemm])
        fuse = experiment_env('VBX_AMD_FUSE')             # '0' keeps every stage in its own kernel
        if fuse is not None:
            self.set_option(OPT_FUSE, int(fuse))

    def profile_kernels(self, names=None):
        """HIP events around every launch (names=None), around the given kernel classes only, or off ([])."""
        if names is None:
            self.set_option(OPT_PROFILE, 1)
        else:
            self.set_option(OPT_PROFILE, 2 * sum(1 << K_NAMES.index(n) for n in names))

    def set_option(self, option: int, value: int):
        self.ctx.check(self._lib.vbx_batch_set_option(self._h, int(option), int(value)), 'vbx_batch_set_option')

    def set_async_upload(self, on=True):
        """Uploads without a synchronize per recording (VBX_OPT_ASYNC_UPLOAD): set_recording only enqueues; the arrays it was
        given are kept alive here until the next run() / sync_uploads()."""
        self.set_option(OPT_ASYNC_UPLOAD, 1 if on else 0)
        self._async = bool(on)
        if not on:
            self._held.clear()

    def stream_of(self, b) -> int:
        """The stream (sub-batch) recording b was dealt to: recordings of different streams may be set from different threads."""
        return int(self._lib.vbx_batch_stream_of(self._h, int(b)))

    def sync_uploads(self):
        self.ctx.check(self._lib.vbx_batch_sync_uploads(self._h), 'vbx_batch_sync_uploads')
        self._held.clear()

    def set_recording(self, b, X, Phi, pi0, gamma0, loopProb, Fa, Fb, alpha0=None, invL0=None):
        X = np.ascontiguousarray(X)
        if X.dtype != np.float32:
            X = np.ascontiguousarray(X, dtype=np.float64)
        gamma0 = np.ascontiguousarray(gamma0)
        if gamma0.dtype != np.float32:
            gamma0 = np.ascontiguousarray(gamma0, dtype=np.float64)
        assert X.shape == (self.T[b], self.D) and gamma0.shape == (self.T[b], self.S[b])
        Phi, pi0, alpha0, invL0 = _f64(Phi), _f64(pi0), _f64(alpha0), _f64(invL0)
        assert Phi.shape == (self.D,) and pi0.shape == (self.S[b],)
        self.ctx.check(self._lib.vbx_batch_set_recording(
            self._h, int(b), _ptr(X), VBX_F32 if X.dtype == np.float32 else VBX_F64, _ptr(Phi), _ptr(pi0),
            _ptr(gamma0), VBX_F32 if gamma0.dtype == np.float32 else VBX_F64, _ptr(alpha0), _ptr(invL0),
            float(loopProb), float(Fa), float(Fb)), 'vbx_batch_set_recording')
        if self._async:
            self._held.append((X, gamma0))

    def set_recording_shared(self, b, src, pi0, gamma0, loopProb, Fa, Fb, alpha0=None, invL0=None):
        """Recording b on the x-vectors (rho, Phi) of recording ``src`` of this batch, set before: one point of an
        Fa / Fb / loopProb sweep over one recording (vbx_batch_set_recording_shared)."""
        gamma0 = np.ascontiguousarray(gamma0)
        if gamma0.dtype != np.float32:
            gamma0 = np.ascontiguousarray(gamma0, dtype=np.float64)
        assert gamma0.shape == (self.T[b], self.S[b]) and self.T[b] == self.T[src]
        pi0, alpha0, invL0 = _f64(pi0), _f64(alpha0), _f64(invL0)
        assert pi0.shape == (self.S[b],)
        self.ctx.check(self._lib.vbx_batch_set_recording_shared(
            self._h, int(b), int(src), _ptr(pi0), _ptr(gamma0), VBX_F32 if gamma0.dtype == np.float32 else VBX_F64,
            _ptr(alpha0), _ptr(invL0), float(loopProb), float(Fa), float(Fb)), 'vbx_batch_set_recording_shared')
        if self._async:
            self._held.append((gamma0,))

    def set_recording_resident(self, b, xv: 'XVectors', row0, labels, init_smoothing, Phi, loopProb, Fa, Fb):
        """Recording b from resident rows of ``xv.fea`` and the AHC labels: initial responsibilities
        softmax(init_smoothing * onehot(labels)) built on the device, uniform priors (vbhmm.py:150-158)."""
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        Phi = _f64(Phi)
        assert labels.shape == (self.T[b],) and Phi.shape == (self.D,)
        self.ctx.check(self._lib.vbx_batch_set_recording_resident(
            self._h, int(b), xv._h, int(row0), _ptr(labels), float(init_smoothing), _ptr(Phi), float(loopProb),
            float(Fa), float(Fb)), 'vbx_batch_set_recording_resident')

    def set_recording_random(self, b, xv, row0, src, seed, name_hash, restart, init_smoothing, Phi, loopProb, Fa, Fb):
        """Recording b from random labels in [0, S[b]) drawn on the device (``random_labels`` with N = S[b]) and smoothed
        into the initial responsibilities there, uniform priors (vbx_batch_set_recording_random).  ``src`` < 0: b owns a rho
        built from the resident rows of ``xv.fea`` from ``row0`` on; ``src`` >= 0: b runs on the rho of recording ``src`` of
        this batch, set before (``xv``, ``row0`` and ``Phi`` are not read then and may be None)."""
        src = -1 if src is None or int(src) < 0 else int(src)
        Phi = _f64(Phi)
        if src < 0:
            assert xv is not None and Phi is not None and Phi.shape == (self.D,)
        self.ctx.check(self._lib.vbx_batch_set_recording_random(
            self._h, int(b), xv._h if src < 0 else None, int(row0 or 0), src, _u64(seed), _u64(name_hash), int(restart),
            float(init_smoothing), _ptr(Phi) if src < 0 else None, float(loopProb), float(Fa), float(Fb)),
            'vbx_batch_set_recording_random')

    def set_recording_turns(self, b, xv: 'XVectors', row0, seg_a, seg_b, turn_u, turn_v, turn_spk, init_smoothing, Phi, loopProb,
                            Fa, Fb):
        """Recording b from the speaker turns of a diarization that exists (``--init RTTM+VB``): windows ``[seg_a, seg_b)``
        and turns ``[turn_u, turn_v)`` of the speakers ``turn_spk`` in [0, S[b]), all in integer microseconds, the turns
        sorted by (speaker, start).  The responsibilities of ``turn_weights`` are built on the device straight into the
        batch, uniform priors, rho from the resident rows of ``xv.fea`` from ``row0`` on (vbx_batch_set_recording_turns)."""
        seg_a, seg_b, turn_u, turn_v, turn_spk = _turn_arrays(seg_a, seg_b, turn_u, turn_v, turn_spk)
        Phi = _f64(Phi)
        if seg_a.shape != (self.T[b],):
            raise ValueError(f'set_recording_turns: {seg_a.shape[0]} windows, recording {b} has {self.T[b]} x-vectors')
        assert Phi.shape == (self.D,)
        self.ctx.check(self._lib.vbx_batch_set_recording_turns(
            self._h, int(b), xv._h, int(row0), _ptr(seg_a), _ptr(seg_b), turn_u.shape[0], _ptr(turn_u), _ptr(turn_v),
            _ptr(turn_spk), float(init_smoothing), _ptr(Phi), float(loopProb), float(Fa), float(Fb)),
            'vbx_batch_set_recording_turns')

    def final_elbos(self, recs=None):
        """The last ELBO of every recording of ``recs`` (default: all) after a run, nan for one that has not iterated: the
        small arrays only, one synchronize per stream (vbx_batch_get_results without responsibilities or models)."""
        res = self.results(recs, want_gamma=False, want_model=False, pinned=False)
        return [float(r['Li'][-1]) if len(r['Li']) else float('nan') for r in res]

    def labels(self, b):
        """(first, second) speaker of every frame of recording b: np.argsort(-gamma, axis=1)[:, 0 / 1] computed on the
        device (vbhmm.py:160-162); second is None for a single speaker."""
        first = np.empty(self.T[b], dtype=np.int32)
        second = np.empty(self.T[b], dtype=np.int32)
        self.ctx.check(self._lib.vbx_batch_get_labels(self._h, int(b), _ptr(first), _ptr(second)), 'vbx_batch_get_labels')
        return first.astype(np.int64), (second.astype(np.int64) if self.S[b] > 1 else None)

    def path(self, b):
        """(first, second) of recording b after a run: first is the most probable state sequence under the model of the
        last forward-backward pass, second the best other speaker of every frame by responsibility (None for a single
        speaker) -- vbx_batch_get_path."""
        first = np.empty(self.T[b], dtype=np.int32)
        second = np.empty(self.T[b], dtype=np.int32)
        self.ctx.check(self._lib.vbx_batch_get_path(self._h, int(b), _ptr(first), _ptr(second)), 'vbx_batch_get_path')
        return first.astype(np.int64), (second.astype(np.int64) if self.S[b] > 1 else None)

    def set_reference(self, b, ref, n_ref=None):
        """Reference labels of recording b (after it has been set, before a run): every iteration of run() then leaves the
        confusion block of its responsibilities in the recording's history (scores()).  ``ref=None`` clears them; ``n_ref``
        defaults to max(ref) + 1 (at most MAX_REF_LABELS)."""
        if ref is None:
            self.ctx.check(self._lib.vbx_batch_set_reference(self._h, int(b), None, 0), 'vbx_batch_set_reference')
            self._n_ref.pop(int(b), None)
            return
        ref = np.ascontiguousarray(ref, dtype=np.int32)
        assert ref.shape == (self.T[b],)
        n_ref = int(ref.max()) + 1 if n_ref is None else int(n_ref)
        self.ctx.check(self._lib.vbx_batch_set_reference(self._h, int(b), _ptr(ref), n_ref), 'vbx_batch_set_reference')
        self._n_ref[int(b)] = n_ref

    def scores(self, b):
        """The confusion blocks of recording b, one per iteration it has run: [n_iters][2][n_ref][S] (vbx_batch_get_scores)."""
        n_ref = self._n_ref.get(int(b), 1)                 # (no labels: the library says so)
        conf = np.zeros((max(self.max_iters, 1), 2, n_ref, self.S[b]))
        n = C.c_int()
        self.ctx.check(self._lib.vbx_batch_get_scores(self._h, int(b), _ptr(conf), len(conf), C.byref(n)), 'vbx_batch_get_scores')
        return conf[:min(n.value, len(conf))].copy()

    def n_iters(self, b):
        n, w = C.c_int(), C.c_int()
        self.ctx.check(self._lib.vbx_batch_get_result(self._h, int(b), None, None, None, 0, C.byref(n), C.byref(w), None, None),
                       'vbx_batch_get_result')
        return n.value

    def run(self, iters: int, epsilon: float = -np.inf):
        eps = float(epsilon)
        if not np.isfinite(eps):
            eps = -1e300 if eps < 0 else 1e300
        try:
            self.ctx.check(self._lib.vbx_batch_run(self._h, int(iters), eps), 'vbx_batch_run')
        finally:
            self._held.clear()                             # (the run begins by waiting for the uploads)

    def last_run_ms(self):
        ms, it = C.c_double(), C.c_int()
        self.ctx.check(self._lib.vbx_batch_last_run_ms(self._h, C.byref(ms), C.byref(it)), 'vbx_batch_last_run_ms')
        return ms.value, it.value

    @property
    def streams(self) -> int:
        """HIP streams (sub-batches) this batch runs on (VBX_OPT_STREAMS in effect)."""
        return int(self._lib.vbx_batch_streams(self._h))

    @property
    def gemm(self) -> str:
        """'split' when the iterations of the last run multiplied with f16 operand pairs (VBX_OPT_GEMM in effect), else
        'exact'."""
        return 'split' if int(self._lib.vbx_batch_gemm_in_effect(self._h)) == GEMM_SPLIT else 'exact'

    def set_stream_loads(self, mode: str):
        """'auto' | 'on' | 'off': non-temporal loads of rho in the per-chunk kernels (VBX_OPT_STREAM_LOADS)."""
        if mode not in STREAM_LOADS_NAMES:
            raise ValueError(f'stream_loads={mode!r}: expected one of {", ".join(map(repr, STREAM_LOADS_NAMES))}')
        self.set_option(OPT_STREAM_LOADS, STREAM_LOADS_NAMES[mode])

    @property
    def stream_loads(self) -> bool:
        """True when the per-chunk kernels of the last run fetched rho with non-temporal loads (VBX_OPT_STREAM_LOADS in effect)."""
        return bool(self._lib.vbx_batch_stream_loads_in_effect(self._h))

    @property
    def plan(self) -> dict:
        """The launch plan of the last run (vbx_batch_plan): which kernel instances its iterations launched -- flags as bool,
        ``walk_levels``, ``fin_threads``, ``Sp``, ``sgroup``, ``sgroup2`` as int.  Several streams: the first sub-batch's."""
        out = np.zeros(len(PLAN_FIELDS), dtype=np.int32)
        n = int(self._lib.vbx_batch_plan(self._h, _ptr(out), len(out)))
        self.ctx.check(min(n, 0), 'vbx_batch_plan')
        assert n >= len(PLAN_FIELDS), n
        return {k: bool(v) if k in PLAN_FLAGS else int(v) for k, v in zip(PLAN_FIELDS, out)}

    def kernel_times(self):
        ms = np.zeros(len(K_NAMES))
        n = np.zeros(len(K_NAMES), dtype=np.int64)
        self.ctx.check(self._lib.vbx_batch_kernel_times(self._h, _ptr(ms), _ptr(n)), 'vbx_batch_kernel_times')
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(K_NAMES)}

    def result(self, b, want_gamma=True, want_model=True):
        T, S, D = self.T[b], self.S[b], self.D
        gamma = np.empty((T, S)) if want_gamma else None
        pi = np.empty(S)
        Li = np.zeros(max(self.max_iters, 1))
        alpha = np.empty((S, D)) if want_model else None
        invL = np.empty((S, D)) if want_model else None
        n_iters, warned = C.c_int(), C.c_int()
        self.ctx.check(self._lib.vbx_batch_get_result(self._h, int(b), _ptr(gamma), _ptr(pi), _ptr(Li), len(Li),
                                                      C.byref(n_iters), C.byref(warned), _ptr(alpha), _ptr(invL)),
                       'vbx_batch_get_result')
        n = min(n_iters.value, self.max_iters)
        return {'gamma': gamma, 'pi': pi, 'Li': Li[:n].copy(), 'n_iters': n_iters.value,
                'warned': bool(warned.value), 'alpha': alpha, 'invL': invL}

    def results(self, recs=None, want_gamma=True, want_model=True, pinned=True):
        """``[result(b) for b in recs]`` (default: every recording) with ONE synchronize per stream (vbx_batch_get_results) and,
        with ``pinned``, the arrays of all recordings on one block of pinned host memory: the responsibilities leave HBM as
        plain DMA instead of through the runtime's staging buffers (64 recordings of T = 10 000: 25-37 ms -> a few)."""
        recs = list(range(self.n)) if recs is None else [int(b) for b in recs]
        # gamma on a pinned block of its own per recording (a caller that keeps one recording's responsibilities keeps that block,
        # not the batch's); the small arrays of all recordings share one block and are handed out as ordinary copies
        small, per = [], 4 if want_model else 2
        for b in recs:
            S, D = self.S[b], self.D
            small += [(S,), (max(self.max_iters, 1),)] + ([(S, D), (S, D)] if want_model else [])
        small = pinned_arrays(small) if pinned else [np.empty(s) for s in small]
        arrays = []
        for k, b in enumerate(recs):
            T, S = self.T[b], self.S[b]
            g = (pinned_arrays([(T, S)])[0] if pinned else np.empty((T, S))) if want_gamma else None
            arrays.append([g] + small[per * k: per * k + per])
        items = (Fetch * len(recs))()
        for k, b in enumerate(recs):
            g, p, L = arrays[k][:3]
            L[:] = 0.0
            items[k].rec = b
            items[k].gamma = g.ctypes.data if want_gamma else None
            items[k].pi = p.ctypes.data
            items[k].Li = L.ctypes.data
            items[k].li_cap = len(L)
            items[k].alpha = arrays[k][3].ctypes.data if want_model else None
            items[k].invL = arrays[k][4].ctypes.data if want_model else None
        self.ctx.check(self._lib.vbx_batch_get_results(self._h, len(recs), items), 'vbx_batch_get_results')
        out = []
        for k, b in enumerate(recs):
            g, p, L = arrays[k][:3]
            n = min(items[k].n_iters, self.max_iters)
            out.append({'gamma': g, 'pi': p.copy(), 'Li': L[:n].copy(), 'n_iters': int(items[k].n_iters),
                        'warned': bool(items[k].warned), 'alpha': arrays[k][3].copy() if want_model else None,
                        'invL': arrays[k][4].copy() if want_model else None})
        return out

    def close(self):
        if getattr(self, '_h', None):
            self._lib.vbx_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        if sys.is_finalizing():          # the HIP runtime may already be gone: leave the device memory to the process exit
            return
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def _u64(v) -> int:
    v = int(v)
    if not 0 <= v < 1 << 64:
        raise ValueError(f'{v} is not an unsigned 64-bit integer')
    return v


def random_labels(ctx: Context, seed, name_hash, restart, T, N, out=None) -> np.ndarray:
    """int32 [T]: the labels --init random_N starts restart ``restart`` of a recording from, drawn on the device
    (vbx_random_labels): ``(np.random.Philox(key=[seed, name_hash], counter=[0, restart, 0, 0]).random_raw(T) * N) >> 64``.
    ``out``: a contiguous int32 array of T elements to fill (default: a new one)."""
    T, N, seed, name_hash = int(T), int(N), _u64(seed), _u64(name_hash)
    if T < 1 or N < 1 or int(restart) < 0:
        raise ValueError(f'random_labels: T={T}, N={N}, restart={restart}: T and N must be >= 1, restart >= 0')
    if out is None:
        out = np.empty(T, dtype=np.int32)
    if out.dtype != np.int32 or out.shape != (T,) or not out.flags.c_contiguous:
        raise ValueError('random_labels: out must be a contiguous int32 array of T elements')
    ctx.check(ctx._lib.vbx_random_labels(ctx._h, _u64(seed), _u64(name_hash), int(restart), T, N, _ptr(out)), 'vbx_random_labels')
    return out


def _turn_arrays(seg_a, seg_b, turn_u, turn_v, turn_spk):
    """The five arrays of the turn entry points, contiguous in the C types; ValueError where their lengths disagree."""
    seg_a, seg_b, turn_u, turn_v = (np.ascontiguousarray(x, dtype=np.int64).reshape(-1) for x in (seg_a, seg_b, turn_u, turn_v))
    turn_spk = np.ascontiguousarray(turn_spk, dtype=np.int32).reshape(-1)
    if seg_a.shape != seg_b.shape or not turn_u.shape == turn_v.shape == turn_spk.shape:
        raise ValueError(f'windows: {seg_a.shape[0]} starts and {seg_b.shape[0]} ends; turns: {turn_u.shape[0]} starts, '
                         f'{turn_v.shape[0]} ends and {turn_spk.shape[0]} speakers')
    return seg_a, seg_b, turn_u, turn_v, turn_spk


def turn_weights(ctx, seg_a, seg_b, turn_u, turn_v, turn_spk, S, init_smoothing, want=('labels', 'w', 'q')):
    """(labels int32 [T], w f64 [T][S], q f64 [T][S]) of ``--init RTTM+VB`` (vbx_turn_weights), None for
    what ``want`` leaves out: the speaker turns ``[turn_u, turn_v)`` of ``turn_spk`` in [0, S), sorted by (speaker, start),
    resampled on the device onto the windows ``[seg_a, seg_b)`` -- all times in integer microseconds.  ``w`` shares a window
    among the speakers by overlap (the one-hot row of the nearest turn's speaker where nothing overlaps), ``labels`` is its
    arg-max and ``q = softmax(init_smoothing * w)``.  Bad input is a ``VbxError`` that says what is wrong, raised before
    the device is touched (``ctx`` None: only that check runs)."""
    seg_a, seg_b, turn_u, turn_v, turn_spk = _turn_arrays(seg_a, seg_b, turn_u, turn_v, turn_spk)
    T, S = seg_a.shape[0], int(S)
    sized = T >= 1 and S >= 1
    labels = np.empty(T, dtype=np.int32) if 'labels' in want and sized else None
    w = np.empty((T, S)) if 'w' in want and sized else None
    q = np.empty((T, S)) if 'q' in want and sized else None
    lib, handle = (load(), None) if ctx is None else (ctx._lib, ctx._h)
    rc = lib.vbx_turn_weights(handle, T, _ptr(seg_a), _ptr(seg_b), turn_u.shape[0], _ptr(turn_u), _ptr(turn_v), _ptr(turn_spk), S,
                              float(init_smoothing), _ptr(labels), _ptr(w), _ptr(q))
    if rc != 0:
        raise VbxError(f'vbx_turn_weights failed ({rc}): {lib.vbx_last_error(handle).decode()}')
    return labels, w, q


def nan_rows(ctx: Context, x_ptr, n, D) -> np.ndarray:
    """bool [n]: which rows of the f32 array [n][D] at the device address ``x_ptr`` hold a NaN (vbx_rows_nan_flags) --
    ``np.isnan(x).any(1)`` with only the n flags coming back."""
    n = int(n)
    if n == 0:
        return np.zeros(0, dtype=bool)
    flags = np.empty(max(n, 0), dtype=np.int32)
    ctx.check(ctx._lib.vbx_rows_nan_flags(ctx._h, C.c_void_p(x_ptr), n, int(D), _ptr(flags)), 'vbx_rows_nan_flags')
    return flags != 0


def plda_covariance(ctx: Context, x):
    """(mean [D], np.cov(x.T, bias=True) [D][D]) of the rows ``x`` [T][D], summed on the device in a fixed order."""
    x = _f64(x)
    assert x.ndim == 2
    mean, cov = np.empty(x.shape[1]), np.empty((x.shape[1], x.shape[1]))
    ctx.check(ctx._lib.vbx_plda_covariance(ctx._h, x.shape[0], x.shape[1], _ptr(x), _ptr(mean), _ptr(cov)), 'vbx_plda_covariance')
    return mean, cov


def plda_covariance_resident(ctx: Context, xv: 'XVectors', row0, T):
    """plda_covariance of rows [row0, row0 + T) of the projected x-vectors already in HBM: the same bits."""
    mean, cov = np.empty(xv.dl), np.empty((xv.dl, xv.dl))
    ctx.check(ctx._lib.vbx_plda_covariance_resident(ctx._h, xv._h, int(row0), int(T), _ptr(mean), _ptr(cov)),
              'vbx_plda_covariance_resident')
    return mean, cov


BACKEND_MAX_DIM = 1024       # dimensions of a segmented second moment (vbx_backend.hpp: kBackendMaxDim)


def _rows_f32_or_f64(x):
    x = np.asarray(x)
    x = np.ascontiguousarray(x, dtype=np.float32 if x.dtype == np.float32 else np.float64)
    assert x.ndim == 2
    return x, (VBX_F32 if x.dtype == np.float32 else VBX_F64)


def backend_class_sums(ctx: Context, x, class_of_row, K):
    """(sums [K][D] f64, counts [K]) of the rows ``x`` [N][D] (f32 or f64) by class, the rows of a class added in archive
    order over fixed chunks (vbx_backend_class_sums)."""
    x, dt = _rows_f32_or_f64(x)
    cls = np.ascontiguousarray(class_of_row, dtype=np.int32)
    assert cls.shape == (x.shape[0],)
    sums, counts = np.empty((max(int(K), 0), x.shape[1])), np.empty(max(int(K), 0), dtype=np.int64)
    ctx.check(ctx._lib.vbx_backend_class_sums(ctx._h, x.shape[0], x.shape[1], _ptr(x), dt, int(K), _ptr(cls), _ptr(sums), _ptr(counts)),
              'vbx_backend_class_sums')
    return sums, counts


def backend_second_moments(ctx: Context, rows, offsets):
    """out [G][D][D], out[g] = sum of r r^T over the rows [offsets[g], offsets[g + 1]) of ``rows`` [R][D]
    (vbx_backend_second_moments): float64 on the matrix cores, fixed summation order, symmetric to the last bit."""
    rows = _f64(rows)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    assert rows.ndim == 2 and off.ndim == 1 and off.size >= 1
    G, D = off.size - 1, rows.shape[1]
    out = np.empty((max(G, 0), D, D))
    ctx.check(ctx._lib.vbx_backend_second_moments(ctx._h, rows.shape[0], D, _ptr(rows), G, _ptr(off), _ptr(out)),
              'vbx_backend_second_moments')
    return out


class BackendStats:
    """Labelled x-vectors resident in HBM across the two statistics stages of backend training (vbx_backend)."""

    def __init__(self, ctx: Context, x, class_of_row, K):
        x, dt = _rows_f32_or_f64(x)
        cls = np.ascontiguousarray(class_of_row, dtype=np.int32)
        assert cls.shape == (x.shape[0],)
        self._ctx, self._lib = ctx, ctx._lib
        self.n, self.din, self.k = x.shape[0], x.shape[1], int(K)
        self.kernel_ms = [None, None]
        h = C.c_void_p()
        ctx.check(self._lib.vbx_backend_create(ctx._h, self.n, self.din, _ptr(x), dt, self.k, _ptr(cls), C.byref(h)), 'vbx_backend_create')
        self._h = h

    def stage1(self):
        """(mean1 [Din], class sums [K][Din] and second moment [Din][Din] of y = l2norm(x - mean1))."""
        mean1, cs, m2, ms = np.empty(self.din), np.empty((self.k, self.din)), np.empty((self.din, self.din)), C.c_double()
        self._ctx.check(self._lib.vbx_backend_stage1(self._h, _ptr(mean1), _ptr(cs), _ptr(m2), C.byref(ms)), 'vbx_backend_stage1')
        self.kernel_ms[0] = ms.value
        return mean1, cs, m2

    def stage2(self, lda, mean2):
        """(class sums [K][dl], second moment [dl][dl]) of u = l2norm(y lda - mean2)."""
        lda, mean2 = _f64(lda), _f64(mean2)
        assert lda.ndim == 2 and lda.shape[0] == self.din and mean2.shape == (lda.shape[1],)
        dl = lda.shape[1]
        cs, m2, ms = np.empty((self.k, dl)), np.empty((dl, dl)), C.c_double()
        self._ctx.check(self._lib.vbx_backend_stage2(self._h, dl, _ptr(lda), _ptr(mean2), _ptr(cs), _ptr(m2), C.byref(ms)), 'vbx_backend_stage2')
        self.kernel_ms[1] = ms.value
        return cs, m2

    def close(self):
        if getattr(self, '_h', None):
            self._lib.vbx_backend_destroy(self._h)
            self._h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


def plda_score_lda(ctx: Context, Fe, Ft, diagAC):
    """PLDA_scoring_in_LDA_space(Fe, Ft, diagAC) -> [N][M] (diarization_lib.py:34-56)."""
    Fe, Ft, diagAC = _f64(Fe), _f64(Ft), _f64(diagAC)
    assert Fe.ndim == 2 and Ft.ndim == 2 and Fe.shape[1] == Ft.shape[1] == diagAC.size
    out = np.empty((Fe.shape[0], Ft.shape[0]))
    ctx.check(ctx._lib.vbx_plda_score_lda(ctx._h, Fe.shape[0], Ft.shape[0], Fe.shape[1], _ptr(Fe), _ptr(Ft), _ptr(diagAC),
                                          _ptr(out)), 'vbx_plda_score_lda')
    return out


def rttm_score(ctx: Context, counts, edges, turns, spk, collar, ignore_overlaps):
    """vbx_rttm_score for the packed pairs: ``counts`` int32 [n][5] = (edges, reference turns, system turns, reference
    speakers, system speakers) of every pair, ``edges`` f64, ``turns`` f64 [.][2], ``spk`` int32, pair after pair.  -> f64,
    per pair 4 + n_ref n_sys numbers: scored reference time, miss, false alarm, sum of w min(|R|, |S|), then C."""
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1, 5)
    edges, turns = _f64(edges).reshape(-1), _f64(turns).reshape(-1, 2)
    spk = np.ascontiguousarray(spk, dtype=np.int32).reshape(-1)
    n_cnt = counts.astype(np.int64)
    assert edges.size == n_cnt[:, 0].sum() and turns.shape[0] == spk.size == n_cnt[:, 1:3].sum()
    out = np.empty(int((4 + n_cnt[:, 3] * n_cnt[:, 4]).sum()))
    if counts.shape[0]:
        ctx.check(ctx._lib.vbx_rttm_score(ctx._h, counts.shape[0], _ptr(counts), _ptr(edges), _ptr(turns), _ptr(spk), float(collar),
                                          int(bool(ignore_overlaps)), _ptr(out)), 'vbx_rttm_score')
    return out


def vad_energy(ctx: Context, samples, rec, winlen, shift, energy_threshold, mean_scale, context, proportion, min_silence,
               min_speech, pad, details=False, times=False):
    """vbx_vad_energy: ``samples`` int16 (the recordings end to end), ``rec`` int64 [n][2] = (first sample, samples).
    -> (counts int32 [n], segs int32 [sum counts][2] in frames, details, ms): details is None or (N int64, e f64, theta f64
    [n], raw uint8) over the frames of all recordings end to end, ms None or the device milliseconds (upload, kernels)."""
    samples = np.ascontiguousarray(samples, dtype=np.int16).reshape(-1)
    rec = np.ascontiguousarray(rec, dtype=np.int64).reshape(-1, 2)
    T = np.where(rec[:, 1] >= winlen, (rec[:, 1] - winlen) // shift + 1, 0)
    counts = np.zeros(rec.shape[0], dtype=np.int32)
    segs = np.empty((int(((T + 1) // 2).sum()), 2), dtype=np.int32)
    frames = int(T.sum())
    det = (np.empty(frames, dtype=np.int64), np.empty(frames), np.empty(rec.shape[0]), np.empty(frames, dtype=np.uint8)) if details else None
    ms = np.zeros(2, dtype=np.float32) if times else None
    N, e, theta, raw = det if details else (None, None, None, None)
    ctx.check(ctx._lib.vbx_vad_energy(ctx._h, samples.size, _ptr(samples), rec.shape[0], _ptr(rec), int(winlen), int(shift),
                                      float(energy_threshold), float(mean_scale), int(context), float(proportion), int(min_silence),
                                      int(min_speech), int(pad), _ptr(counts), _ptr(segs), _ptr(N), _ptr(e), _ptr(theta), _ptr(raw),
                                      _ptr(ms)), 'vbx_vad_energy')
    return counts, segs[:int(counts.sum())], det, ms


def resample_pcm(ctx: Context, data, rec, fmt, channels, L, M, table, times=False):
    """vbx_resample_pcm: ``data`` uint8 (the raw interleaved frames of the recordings end to end), ``rec`` int64 [n][2] =
    (first byte, frames), ``fmt`` 0 .. 4 = u8, s16, s24, s32, f32, ``table`` int32 [L][taps] (audio.phase_table).
    -> (int16 samples of all recordings end to end, ms): ms is None or the device milliseconds (upload, kernel)."""
    data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    rec = np.ascontiguousarray(rec, dtype=np.int64).reshape(-1, 2)
    table = np.ascontiguousarray(table, dtype=np.int32)
    assert table.ndim == 2 and table.shape[0] == L
    n_out = -((-np.maximum(rec[:, 1], 0) * int(L)) // int(M))
    out = np.empty(int(n_out.sum()), dtype=np.int16)
    ms = np.zeros(2, dtype=np.float32) if times else None
    ctx.check(ctx._lib.vbx_resample_pcm(ctx._h, data.size, _ptr(data), rec.shape[0], _ptr(rec), int(fmt), int(channels), int(L), int(M),
                                        table.shape[1], _ptr(table), _ptr(out), _ptr(ms)), 'vbx_resample_pcm')
    return out, ms


def frame_counts(ctx: Context, counts, extent, turns, spk, step):
    """vbx_frame_counts for the packed pairs: ``counts`` int32 [n][4] = (reference turns, system turns, reference speakers,
    system speakers) of every pair, ``extent`` f64 [n][2] = (lo, hi), ``turns`` f64 [.][2], ``spk`` int32, pair after pair.
    -> (info int32 [n][4] = cells, reference classes, system classes, 0; classes uint64 [n][2][256]: the speaker masks of the
    classes in order of first appearance; out int64, per pair ref_durs, sys_durs, inter [n_ref][n_sys] and -- unless a side
    has more than 256 classes -- cm [reference classes][system classes])."""
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1, 4)
    extent, turns = _f64(extent).reshape(-1, 2), _f64(turns).reshape(-1, 2)
    spk = np.ascontiguousarray(spk, dtype=np.int32).reshape(-1)
    n = counts.astype(np.int64)
    assert extent.shape[0] == n.shape[0] and turns.shape[0] == spk.size == n[:, :2].sum()
    # classes on a side: at most one per cell, at most 2 (turns of the pair) + 1 cells
    cls = np.minimum(2 * n[:, :2].sum(axis=1) + 1, FRAME_MAX_CLASSES)
    out = np.empty(int((n[:, 2] + n[:, 3] + n[:, 2] * n[:, 3] + cls * cls).sum()), dtype=np.int64)
    info = np.zeros((n.shape[0], 4), dtype=np.int32)
    classes = np.zeros((n.shape[0], 2, FRAME_MAX_CLASSES), dtype=np.uint64)
    if n.shape[0]:
        ctx.check(ctx._lib.vbx_frame_counts(ctx._h, n.shape[0], _ptr(counts), _ptr(extent), _ptr(turns), _ptr(spk), float(step),
                                            _ptr(info), _ptr(classes), _ptr(out), out.size), 'vbx_frame_counts')
    return info, classes, out


def labels_frame_counts(ctx: Context, rec_counts, seg_times, ref_turns, ref_spk, hyp, labels, step):
    """vbx_labels_frame_counts: ``rec_counts`` int32 [n_rec][3] = (T, reference turns, reference speakers) of every recording,
    ``seg_times`` f64 (starts[T] then ends[T] per recording), ``ref_turns`` f64 [.][2], ``ref_spk`` int32, ``hyp`` int32
    [n_hyp][2] = (recording, system speakers), ``labels`` int32, hypothesis after hypothesis.
    -> (info, classes, out) per hypothesis as ``frame_counts`` gives them per pair, and uint64 [n_hyp]: the mask of the labels
    with a turn of positive duration."""
    rec_counts = np.ascontiguousarray(rec_counts, dtype=np.int32).reshape(-1, 3)
    hyp = np.ascontiguousarray(hyp, dtype=np.int32).reshape(-1, 2)
    seg_times, ref_turns = _f64(seg_times).reshape(-1), _f64(ref_turns).reshape(-1, 2)
    ref_spk = np.ascontiguousarray(ref_spk, dtype=np.int32).reshape(-1)
    labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
    n_rec, n_hyp = rec_counts.astype(np.int64), hyp.astype(np.int64)
    assert ((n_hyp[:, 0] >= 0) & (n_hyp[:, 0] < len(n_rec))).all(), 'a hypothesis names a recording that is not there'
    assert seg_times.size == 2 * n_rec[:, 0].sum() and ref_turns.shape[0] == ref_spk.size == n_rec[:, 1].sum()
    assert labels.size == n_rec[n_hyp[:, 0], 0].sum()
    of = n_rec[n_hyp[:, 0]]                                             # the recording of every hypothesis
    # classes on a side: at most one per cell, at most 2 (reference turns + T) + 1 cells
    cls = np.minimum(2 * (of[:, 1] + of[:, 0]) + 1, FRAME_MAX_CLASSES)
    n_sys = np.maximum(n_hyp[:, 1], 0)
    out = np.empty(int((of[:, 2] + n_sys + of[:, 2] * n_sys + cls * cls).sum()), dtype=np.int64)
    info = np.zeros((hyp.shape[0], 4), dtype=np.int32)
    classes = np.zeros((hyp.shape[0], 2, FRAME_MAX_CLASSES), dtype=np.uint64)
    masks = np.zeros(hyp.shape[0], dtype=np.uint64)
    if hyp.shape[0]:
        ctx.check(ctx._lib.vbx_labels_frame_counts(ctx._h, rec_counts.shape[0], _ptr(rec_counts), _ptr(seg_times), _ptr(ref_turns),
                                                   _ptr(ref_spk), hyp.shape[0], _ptr(hyp), _ptr(labels), float(step), _ptr(info),
                                                   _ptr(classes), _ptr(out), out.size, _ptr(masks)), 'vbx_labels_frame_counts')
    return info, classes, out, masks


def labels_score(ctx: Context, rec_counts, seg_times, ref_turns, ref_spk, ref_edges, hyp, labels, collar, ignore_overlaps):
    """vbx_labels_score: ``rec_counts`` int32 [n_rec][4] = (T, reference turns, reference speakers, reference edges) of every
    recording, ``seg_times`` f64 (starts[T] then ends[T] per recording), ``ref_turns`` f64 [.][2], ``ref_spk`` int32,
    ``ref_edges`` f64, ``hyp`` int32 [n_hyp][2] = (recording, system speakers), ``labels`` int32, hypothesis after hypothesis.
    -> (f64: per hypothesis 4 + n_ref n_sys numbers as ``rttm_score`` gives them, int32 [n_hyp][4]: system turns, cell edges,
    low and high word of the mask of labels with a turn of positive duration)."""
    rec_counts = np.ascontiguousarray(rec_counts, dtype=np.int32).reshape(-1, 4)
    hyp = np.ascontiguousarray(hyp, dtype=np.int32).reshape(-1, 2)
    seg_times, ref_turns, ref_edges = _f64(seg_times).reshape(-1), _f64(ref_turns).reshape(-1, 2), _f64(ref_edges).reshape(-1)
    ref_spk = np.ascontiguousarray(ref_spk, dtype=np.int32).reshape(-1)
    labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
    n_rec, n_hyp = rec_counts.astype(np.int64), hyp.astype(np.int64)
    assert ((n_hyp[:, 0] >= 0) & (n_hyp[:, 0] < len(n_rec))).all(), 'a hypothesis names a recording that is not there'
    assert seg_times.size == 2 * n_rec[:, 0].sum() and ref_turns.shape[0] == ref_spk.size == n_rec[:, 1].sum()
    assert ref_edges.size == n_rec[:, 3].sum() and labels.size == n_rec[n_hyp[:, 0], 0].sum()
    out = np.empty(int((4 + n_rec[n_hyp[:, 0], 2] * np.maximum(n_hyp[:, 1], 0)).sum()))
    info = np.zeros((hyp.shape[0], 4), dtype=np.int32)
    if hyp.shape[0]:
        ctx.check(ctx._lib.vbx_labels_score(ctx._h, rec_counts.shape[0], _ptr(rec_counts), _ptr(seg_times), _ptr(ref_turns), _ptr(ref_spk),
                                            _ptr(ref_edges), hyp.shape[0], _ptr(hyp), _ptr(labels), float(collar),
                                            int(bool(ignore_overlaps)), _ptr(out), _ptr(info)), 'vbx_labels_score')
    return out, info


def linkage_variant():
    """'scipy' (default) or 'fastcluster' ($VBX_AMD_LINKAGE): which package's arithmetic the average linkage follows."""
    v = os.environ.get('VBX_AMD_LINKAGE', 'scipy').lower()
    if v not in ('scipy', 'fastcluster'):
        raise ValueError(f"VBX_AMD_LINKAGE={v!r}: expected 'scipy' or 'fastcluster'")
    return v


def linkage_average(condensed, variant=None):
    """``linkage(condensed, method='average')`` as native host code: the (n - 1) x 4 linkage matrix.  ``variant='scipy'``
    (default, or $VBX_AMD_LINKAGE): bit for bit ``scipy.cluster.hierarchy.linkage``; ``'fastcluster'``: the form
    ``fastcluster.linkage`` computes (vbhmm.py:140-141) -- weights divided before the update, its own chain bookkeeping --
    restated from the package's published source.  Same tree, distances equal to rounding, wherever no two candidate
    distances tie.  The call releases the GIL: one recording per thread."""
    variant = variant or linkage_variant()
    if variant not in ('scipy', 'fastcluster'):
        raise ValueError(f"linkage_average: variant {variant!r}: expected 'scipy' or 'fastcluster'")
    y = np.ascontiguousarray(condensed, dtype=np.float64)
    if y.ndim != 1:
        raise ValueError('linkage_average expects a condensed distance vector')
    n = int(round((1.0 + np.sqrt(1.0 + 8.0 * y.size)) / 2.0))
    if n * (n - 1) // 2 != y.size or n < 2:
        raise ValueError(f'{y.size} is not the length n (n - 1) / 2 of a condensed distance vector')
    Z = np.empty((n - 1, 4))
    fn = load().vbx_linkage_average_fastcluster if variant == 'fastcluster' else load().vbx_linkage_average
    rc = fn(n, _ptr(y), _ptr(Z))
    if rc != 0:
        raise VbxError(f'vbx_linkage_average failed ({rc})')
    return Z


def ark_index(buf):
    """Entries of a binary Kaldi vector archive held in ``buf`` (bytes-like): arrays (key offset, key length, data
    offset, dimension, element size), or ``None`` when the archive is not of that form (text archives)."""
    raw = np.frombuffer(buf, dtype=np.uint8)
    cap = max(16, raw.size // 64)
    while True:
        ko, kl = np.empty(cap, np.int64), np.empty(cap, np.int32)
        do, dm, es = np.empty(cap, np.int64), np.empty(cap, np.int32), np.empty(cap, np.int32)
        n = load().vbx_ark_index(_ptr(raw), raw.size, cap, _ptr(ko), _ptr(kl), _ptr(do), _ptr(dm), _ptr(es))
        if n == -2:
            cap *= 4
            continue
        if n < 0:
            return None
        return ko[:n], kl[:n], do[:n], dm[:n], es[:n]


def gather_rows(raw, offsets, row_bytes, dtype):
    """``len(offsets)`` rows of ``row_bytes`` bytes of the uint8 array ``raw`` packed into a new 2-D array of ``dtype``."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    out = np.empty((offsets.size, row_bytes // np.dtype(dtype).itemsize), dtype=dtype)
    rc = load().vbx_gather_rows(_ptr(raw), raw.size, _ptr(offsets), offsets.size, int(row_bytes), _ptr(out))
    if rc != 0:
        raise VbxError(f'vbx_gather_rows failed ({rc}): offsets outside the buffer')
    return out


def fcluster_distance(Z, t):
    """``scipy.cluster.hierarchy.fcluster(Z, t, criterion='distance')`` as native host code (labels from 1, int32)."""
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    if Z.ndim != 2 or Z.shape[1] != 4:
        raise ValueError('fcluster_distance expects an (n - 1) x 4 linkage matrix')
    n = Z.shape[0] + 1
    labels = np.empty(n, dtype=np.int32)
    rc = load().vbx_fcluster_distance(n, _ptr(Z), float(t), _ptr(labels))
    if rc != 0:
        raise VbxError(f'vbx_fcluster_distance failed ({rc}): not a linkage matrix')
    return labels


def default_context(device: int | None = None, slot: int = 0) -> Context:
    """The process-wide context of a device; ``slot`` > 0: a further one of the same device (its own streams and device
    arena: vbx_amd.batch pipelines a large batch call over two of them)."""
    if device is None:
        device = int(os.environ.get('VBX_AMD_DEVICE', os.environ.get('LOCAL_RANK', '0')))
    key = device if slot == 0 else (device, slot)
    if key not in _default_ctx:
        _default_ctx[key] = Context(device)
    return _default_ctx[key]
