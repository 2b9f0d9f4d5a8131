"""Host-side Python binding of the C ABI in include/cmix_amd.h (ctypes).

This mirrors, for test and bench drivers, what the C++ shim in INTEGRATION.md
does for the reference's `class Predictor` (reference src/predictor.h:17-22):
it only forwards to libcmixamd.so.  There is no Python or CPU implementation of
the per-bit path behind it -- if the HIP library is missing or no gfx950 device
is visible, construction raises.

torch is used purely as the device-memory allocator for chunk operands
(`tensor.data_ptr()` is what crosses the ABI).
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libcmixamd.so")

N_INPUTS, N_MIXERS = 2078, 47
PIPELINE_SLOTS = 8   # CMX_PIPELINE_SLOTS (include/cmix_amd.h): chunks in flight per stream


class CmxError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CmxError(f"{LIB_PATH} is missing: run `python -m cmix_amd.build` "
                           "(there is no non-HIP fallback)")
        # Load the HIP runtime that PyTorch-ROCm bundles first, so that libcmixamd.so binds to the
        # same libamdhip64 instance (two HIP runtimes in one process cannot both own the GPU).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.cmx_last_error.restype = C.c_char_p
        L.cmx_version.restype = C.c_char_p
        L.cmx_p8stage_create.restype = C.c_void_p
        L.cmx_p8stage_create.argtypes = [C.c_int]
        L.cmx_p8stage_destroy.argtypes = [C.c_void_p]
        L.cmx_p8stage_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        L.cmx_p8stage_sync.argtypes = [C.c_void_p]
        L.cmx_p8stage_set_generator_counter.argtypes = [C.c_void_p, C.c_uint32]
        L.cmx_fxcm_create.restype = C.c_void_p
        L.cmx_fxcm_create.argtypes = [C.c_char_p, C.c_int]
        L.cmx_fxcm_destroy.argtypes = [C.c_void_p]
        L.cmx_fxcm_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.cmx_fxcm_sync.argtypes = [C.c_void_p]
        L.cmx_fxcm_failed.argtypes = [C.c_void_p]
        L.cmx_fxcm_debug_set_blpos.argtypes = [C.c_void_p, C.c_int]
        L.cmx_fxcm_debug_jitter_counts.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_fxcm_debug_ring_waits.argtypes = [C.c_void_p]
        L.cmx_fxcm_debug_slot_parallel.argtypes = [C.c_void_p]
        L.cmx_fxcm_create_shadow.restype = C.c_void_p
        L.cmx_fxcm_create_shadow.argtypes = [C.c_int]
        L.cmx_fxcm_run_shared.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.cmx_fxcm_state_diff.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_fxcm_debug_state_xor.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint32]
        L.cmx_fxcm_debug_layout.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_fxcm_debug_state_read.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
        L.cmx_fxcmvote_create.restype = C.c_void_p
        L.cmx_fxcmvote_create.argtypes = [C.c_int, C.c_int]
        L.cmx_fxcmvote_destroy.argtypes = [C.c_void_p]
        L.cmx_fxcmvote_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_void_p]
        L.cmx_fxcmvote_report.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_fxcmvote_record.restype = C.c_void_p
        L.cmx_fxcmvote_record.argtypes = [C.c_void_p]
        L.cmx_fxcmvote_values.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_fxcmvote_last.argtypes = [C.c_void_p, C.c_void_p]
        for stem, kind in _SHADOW.items():   # the pipeline's and the engine's entry points of the four kinds of shadow stages
            for name, args in (("pipeline_set_" + stem, [C.c_int]), ("pipeline_" + stem + "_report", [C.c_void_p]),
                               ("pipeline_" + stem + "_values", [C.c_void_p] * kind["values_args"]),
                               ("pipeline_" + stem + "_state_diff", [C.c_int, C.c_int, C.c_void_p]),
                               ("pipeline_debug_" + stem + "_xor", [C.c_int, C.c_int] + [C.c_uint64] * kind["xor_words"] + [C.c_uint32]),
                               ("set_" + stem, [C.c_int]), (stem + "_report", [C.c_void_p])):
                getattr(L, "cmx_" + name).argtypes = [C.c_void_p] + args
        L.cmx_mixnet_create.restype = C.c_void_p
        L.cmx_mixnet_create.argtypes = [C.c_int]
        L.cmx_mixnet_destroy.argtypes = [C.c_void_p]
        L.cmx_mixnet_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_mixnet_predict.restype = C.c_float
        L.cmx_mixnet_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_mixnet_perceive.argtypes = [C.c_void_p, C.c_int]
        L.cmx_mixnet_sync.argtypes = [C.c_void_p]
        L.cmx_mixnet_bits_done.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_mixnet_profile.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.cmx_mixnet_last_kernel_ms.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_mixnet_spec_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_lstm_create.restype = C.c_void_p
        L.cmx_lstm_create.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.cmx_lstm_destroy.argtypes = [C.c_void_p]
        L.cmx_lstm_vocab_size.argtypes = [C.c_void_p]
        L.cmx_lstm_set_tolerance.argtypes = [C.c_void_p, C.c_int]
        L.cmx_lstm_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                   C.c_size_t, C.c_void_p, C.c_void_p]
        L.cmx_bytemodel_bits_run.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.cmx_lstm_get_gate_weights.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.cmx_lstm_gate_rowlen.argtypes = [C.c_void_p, C.c_int]
        L.cmx_lstm_failed.argtypes = [C.c_void_p]
        L.cmx_glibc_rand_selftest.argtypes = [C.c_uint32, C.c_int, C.c_void_p]
        L.cmx_ctxmodels_create.restype = C.c_void_p
        L.cmx_ctxmodels_create.argtypes = [C.c_void_p, C.c_int]
        L.cmx_ctxmodels_destroy.argtypes = [C.c_void_p]
        L.cmx_ctxmodels_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_void_p]
        L.cmx_ctxmodels_pretrain.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.cmx_ctxmodels_sync.argtypes = [C.c_void_p]
        L.cmx_ctxmodels_get_manager.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_ppmd_create.restype = C.c_void_p
        L.cmx_ppmd_create.argtypes = [C.c_void_p]
        L.cmx_ppmd_create_ex.restype = C.c_void_p
        L.cmx_ppmd_create_ex.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.cmx_ppmd_destroy.argtypes = [C.c_void_p]
        L.cmx_ppmd_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.cmx_pipeline_create.restype = C.c_void_p
        L.cmx_pipeline_create.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        L.cmx_pipeline_destroy.argtypes = [C.c_void_p]
        L.cmx_pipeline_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.cmx_create.restype = C.c_void_p
        L.cmx_create.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.cmx_destroy.argtypes = [C.c_void_p]
        L.cmx_predict.restype = C.c_float
        L.cmx_predict.argtypes = [C.c_void_p]
        L.cmx_perceive.argtypes = [C.c_void_p, C.c_int]
        L.cmx_pretrain.argtypes = [C.c_void_p, C.c_int]
        L.cmx_set_model_outputs.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_get_lstm_hint.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_stage_input.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.cmx_mode.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_debug_last_row.restype = C.c_void_p
        L.cmx_debug_last_row.argtypes = [C.c_void_p]
        L.cmx_ctxmodels_debug_slow_bytes.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_ctxmodels_peek.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.cmx_encoder_create.restype = C.c_void_p
        L.cmx_encoder_destroy.argtypes = [C.c_void_p]
        L.cmx_encoder_encode_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.cmx_encoder_encode_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.cmx_encoder_flush.argtypes = [C.c_void_p]
        L.cmx_encoder_size.restype = C.c_size_t
        L.cmx_encoder_size.argtypes = [C.c_void_p]
        L.cmx_encoder_data.restype = C.c_void_p
        L.cmx_encoder_data.argtypes = [C.c_void_p]
        L.cmx_decoder_create.restype = C.c_void_p
        L.cmx_decoder_create.argtypes = [C.c_void_p, C.c_size_t]
        L.cmx_decoder_destroy.argtypes = [C.c_void_p]
        L.cmx_decoder_decode.argtypes = [C.c_void_p, C.c_float]
        L.cmx_decoder_decode_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.cmx_header_write.restype = C.c_size_t
        L.cmx_header_write.argtypes = [C.c_uint64, C.c_void_p, C.c_int, C.c_void_p]
        L.cmx_header_read.restype = C.c_size_t
        L.cmx_header_read.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_pipeline_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.cmx_pipeline_hints.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_pipeline_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_pipeline_stage_totals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.cmx_pipeline_pretrain.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.cmx_pipeline_sync.argtypes = [C.c_void_p]
        L.cmx_pipeline_enable_fxcm.argtypes = [C.c_void_p, C.c_char_p]
        L.cmx_pipeline_fxcm_enabled.argtypes = [C.c_void_p]
        L.cmx_pipeline_finish_cols.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.cmx_pipeline_fxcm_total_ms.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_pipeline_enable_paq8.argtypes = [C.c_void_p]
        L.cmx_pipeline_wait.argtypes = [C.c_void_p, C.c_uint64]
        L.cmx_pipeline_debug_mix_out.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.cmx_pipeline_paq8_total_ms.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_pipeline_host_ms.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_pipeline_paq8_role_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_pipeline_last_stage_ms.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_probe_libm.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        L.cmx_probe_lds_fill.argtypes = [C.c_int, C.c_uint32, C.c_void_p]
        L.cmx_pipeline_set_tolerance.argtypes = [C.c_void_p, C.c_int]
        L.cmx_pipeline_mixnet_mode.argtypes = [C.c_void_p]
        L.cmx_pipeline_stage_overlap.argtypes = [C.c_void_p]
        L.cmx_hw_queues.argtypes = [C.c_int]
        L.cmx_mixnet_set_tolerance.argtypes = [C.c_void_p, C.c_int]
        L.cmx_mixnet_mode.argtypes = [C.c_void_p]
        L.cmx_mixnet_set_verify.argtypes = [C.c_void_p, C.c_int]
        L.cmx_mixnet_verify_report.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_mixnet_debug_verify_perturb.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32]
        L.cmx_pipeline_set_verify.argtypes = [C.c_void_p, C.c_int]
        L.cmx_pipeline_verify_report.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_set_verify.argtypes = [C.c_void_p, C.c_int]
        L.cmx_verify_report.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_vote_create.restype = C.c_void_p
        L.cmx_vote_create.argtypes = [C.c_int, C.c_int]
        L.cmx_vote_destroy.argtypes = [C.c_void_p]
        L.cmx_vote_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_vote_report.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_vote_record.restype = C.c_void_p
        L.cmx_vote_record.argtypes = [C.c_void_p]
        L.cmx_vote_values.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_mixnet_state_diff.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_mixnet_debug_state_xor.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32]
        L.cmx_vote_last.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_mixnet_state_repair.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_pipeline_set_shadow_repair.argtypes = [C.c_void_p, C.c_int]
        L.cmx_pipeline_shadow_repairs.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.cmx_set_shadow_repair.argtypes = [C.c_void_p, C.c_int]
        L.cmx_shadow_repairs.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.cmx_repair_text.restype = C.c_char_p
        L.cmx_repair_text.argtypes = [C.c_void_p]
        L.cmx_debug_shadow_xor.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32]
        L.cmx_ctxmodels_create_compact.restype = C.c_void_p
        L.cmx_ctxmodels_create_compact.argtypes = [C.c_void_p, C.c_int]
        L.cmx_ctxmodels_state_diff.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_ctxmodels_debug_state_xor.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32]
        L.cmx_ctxmodels_debug_layout.argtypes = [C.c_void_p]
        L.cmx_ctxvote_create.restype = C.c_void_p
        L.cmx_ctxvote_create.argtypes = [C.c_int, C.c_int]
        L.cmx_ctxvote_destroy.argtypes = [C.c_void_p]
        L.cmx_ctxvote_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_void_p]
        L.cmx_ctxvote_report.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_ctxvote_record.restype = C.c_void_p
        L.cmx_ctxvote_record.argtypes = [C.c_void_p]
        L.cmx_ctxvote_values.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_ctxvote_last.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_lstmvote_create.restype = C.c_void_p
        L.cmx_lstmvote_create.argtypes = [C.c_int, C.c_int]
        L.cmx_lstmvote_destroy.argtypes = [C.c_void_p]
        L.cmx_lstmvote_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_void_p]
        L.cmx_lstmvote_report.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_lstmvote_record.restype = C.c_void_p
        L.cmx_lstmvote_record.argtypes = [C.c_void_p]
        L.cmx_lstmvote_values.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_lstmvote_last.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_lstm_state_diff.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_lstm_debug_state_xor.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint32]
        L.cmx_lstm_debug_layout.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_debug_ctx_shadow_xor.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32]
        L.cmx_pipeline_late_start.argtypes = [C.c_void_p, C.c_int]
        L.cmx_pipeline_late_predict.restype = C.c_float
        L.cmx_pipeline_late_predict.argtypes = [C.c_void_p]
        L.cmx_pipeline_late_perceive.argtypes = [C.c_void_p, C.c_int]
        L.cmx_pipeline_late_stop.argtypes = [C.c_void_p]
        L.cmx_pipeline_late_host_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_pipeline_late_debug_row.restype = C.c_void_p
        L.cmx_pipeline_late_debug_row.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_journal_create.restype = C.c_void_p
        L.cmx_journal_create.argtypes = [C.c_int, C.c_int]
        L.cmx_journal_destroy.argtypes = [C.c_void_p]
        L.cmx_journal_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p]
        L.cmx_journal_blocks.argtypes = [C.c_void_p, C.c_void_p]
        L.cmx_journal_read.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.cmx_journal_host_digest.restype = C.c_size_t
        L.cmx_journal_host_digest.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_int, C.c_void_p]
        L.cmx_pipeline_set_journal.argtypes = [C.c_void_p, C.c_int]
        L.cmx_pipeline_journal_read.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
        L.cmx_pipeline_journal_write_files.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.cmx_set_journal.argtypes = [C.c_void_p, C.c_int]
        L.cmx_set_journal_check.argtypes = [C.c_void_p, C.c_char_p]
        L.cmx_journal_write_files.argtypes = [C.c_void_p, C.c_char_p]
        L.cmx_journal_close_files.argtypes = [C.c_void_p]
        L.cmx_state_digest_host.restype = C.c_uint64
        L.cmx_state_digest_host.argtypes = [C.c_void_p, C.c_uint64]
        L.cmx_state_digest_arrays.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        for st in ("mixnet", "ctxmodels", "lstm", "fxcm"):
            getattr(L, "cmx_%s_state_digest" % st).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
            getattr(L, "cmx_%s_state_digest_layout" % st).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.cmx_p8stage_state_digest.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.cmx_p8stage_debug_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.cmx_p8stage_debug_state_words.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.cmx_pipeline_state_digest.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.cmx_pipeline_state_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.cmx_pipeline_set_state_journal.argtypes = [C.c_void_p, C.c_int]
        L.cmx_pipeline_state_journal_read.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cmx_pipeline_state_journal_write_file.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.cmx_set_state_journal.argtypes = [C.c_void_p, C.c_int]
        L.cmx_state_journal_write_file.argtypes = [C.c_void_p, C.c_char_p]
        L.cmx_state_journal_close.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def last_error():
    return lib().cmx_last_error().decode()


def hw_queues(device=0):
    """dedicated hardware queues (HIP streams, one queue each) the library holds on the device now"""
    return lib().cmx_hw_queues(device)


def device_count():
    return lib().cmx_device_count()


# verify mode (include/cmix_amd.h, cmx_mixnet_set_verify): the report's classes
VERIFY_CLASSES = {1: "layer-0 row", 2: "coded bit", 3: "selectors", 4: "decay (gather wave)", 5: "decay (tail-a wave)", 6: "decay (tail-b wave)",
                  7: "ring written", 8: "ring read", 9: "layer-0 row segment"}
VERIFY_CLASS = {"row": 1, "bit": 2, "sel": 3, "decay": 4, "decay_tail_a": 5, "decay_tail_b": 6, "ring_written": 7, "ring_read": 8, "segment": 9}


def _verify_report(fn, h):
    out = (C.c_uint64 * 8)()
    if fn(h, out):
        raise CmxError(last_error())
    v = [int(x) for x in out]
    none = (1 << 64) - 1
    return {"chunks": v[0], "bits": v[1], "mismatches": v[2], "cls": v[3] if v[2] else None, "first_bit": v[4] if v[2] else None,
            "mixer": None if v[5] == none or not v[2] else v[5], "row": None if v[6] == none or not v[2] else v[6],
            "segment": None if v[7] == none or not v[2] else v[7]}


# the redundant vote (include/cmix_amd.h, cmx_vote_*; the rule's specification is cmix_amd.vote.vote_reference)
STATE_REGIONS = ("rows0", "rows1", "rows2", "row_steps", "map_keys", "map_vals", "s6", "s7", "x1", "x2", "scalars")
_NONE64 = (1 << 64) - 1


def _opt(v):
    return None if v == _NONE64 else v


def _vote_report(fn, h):
    out = (C.c_uint64 * 8)()
    if fn(h, out):
        raise CmxError(last_error())
    v = [int(x) for x in out]
    ev = v[3] != 0
    return {"chunks": v[0], "bits": v[1], "n": v[2], "events": v[3], "first_bit": v[4] if ev else None, "column": v[5] if ev else None,
            "odd": _opt(v[6]) if ev else None, "elements": v[7] if ev else None, "raw": v}


def _values(fn, h, n, cols, scalars, sel=False):
    """a vote's cmx_*_values as a dict: words [n, cols] u32 (the capture of the first event), sel [47] u32 where the vote has selectors, then its scalars"""
    words, sel, out = np.zeros(3 * cols, np.uint32), [np.zeros(47, np.uint32)] if sel else [], [C.c_uint32(0) for _ in scalars]
    if fn(h, words.ctypes.data, *[a.ctypes.data for a in sel], *[C.byref(x) for x in out]):
        raise CmxError(last_error())
    return {"words": words[:cols * n].reshape(n, cols).copy(), **({"sel": sel[0]} if sel else {}), **{k: int(x.value) for k, x in zip(scalars, out)}}


def _vote_values(fn, h, n):
    return _values(fn, h, n, 48, ("bit",), sel=True)


def _state_diff(out):
    v = [int(x) for x in out]
    first = None
    if v[0]:
        first = {"region": v[1], "mixer": _opt(v[2]), "row": _opt(v[3]), "index": _opt(v[4]), "a": v[5], "b": v[6]}
    return {"words": v[0], "first": first, "per_region": dict(zip(STATE_REGIONS, v[7:18])), "layer0_mask": v[18], "layer12_mask": v[19], "raw": v}


def _u64(v):
    return _NONE64 if v is None else int(v)


REPAIR_LOG, REPAIR_WORDS = 8, 16   # CMX_REPAIR_LOG, CMX_REPAIR_WORDS (include/cmix_amd.h)


def _shadow_repairs(fn, h):
    """cmx_pipeline_shadow_repairs / cmx_shadow_repairs as a dict: total, and log = the newest (at most 8) repairs, oldest first"""
    out = (C.c_uint64 * (2 + REPAIR_LOG * REPAIR_WORDS))()
    if fn(h, out, len(out)):
        raise CmxError(last_error())
    v = [int(x) for x in out]
    log = []
    for i in range(v[1]):
        e = v[2 + i * REPAIR_WORDS:2 + (i + 1) * REPAIR_WORDS]
        first = {"region": e[6], "mixer": _opt(e[7]), "row": _opt(e[8]), "index": _opt(e[9]), "a": e[10], "b": e[11]} if e[5] else None
        text = lib().cmx_repair_text((C.c_uint64 * REPAIR_WORDS)(*e)).decode()
        log.append({"text": text, "chunk": e[0], "bit": e[1], "column": e[2], "odd": e[3], "elements": e[4], "words": e[5], "first": first,
                    "layer0_mask": e[12], "layer12_mask": e[13], "chunks": e[14], "raw": e})
    return {"total": v[0], "log": log}


def _region(r, names=STATE_REGIONS):
    return names.index(r) if isinstance(r, str) else int(r)


class _VoteBase:
    """What the four vote wrappers share: the handle of cmx_<PREFIX>_create, report(), last(), close(). The record is sticky across run() calls."""
    PREFIX = None

    def __init__(self, n, device=0):
        self.n = int(n)
        self.h = self._c("create")(device, self.n)
        if not self.h:
            raise CmxError(last_error())

    def _c(self, name):
        return getattr(lib(), "cmx_%s_%s" % (self.PREFIX, name))

    def report(self):
        """dict: chunks, bits, n, events (chunks with a non-agreeing element), and of the first event: first_bit, column, odd (instance, None = no
        majority), elements; raw = the eight words. What bits and column count is the stage's (see the class). Synchronises the device."""
        return _vote_report(self._c("report"), self.h)

    def last(self):
        """the chunk voted last alone (cmx_*vote_last): dict elements (0 = the instances agreed), bit, column, odd (None = no majority; bit, column
        and odd are None without an event), raw = the four words. Synchronises the device."""
        out = (C.c_uint64 * 4)()
        if self._c("last")(self.h, out):
            raise CmxError(last_error())
        v = [int(x) for x in out]
        ev = v[0] != 0
        return {"elements": v[0], "bit": v[1] if ev else None, "column": v[2] if ev else None, "odd": _opt(v[3]) if ev else None, "raw": v}

    def close(self):
        if getattr(self, "h", None):
            self._c("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Vote(_VoteBase):
    """The vote kernel over n = 2 or 3 instances' p [T] and mixer outputs [T, 47] (CUDA float32 / int32 / uint8 tensors of 4-byte words are all
    taken as words). In report() and last(), column = 0..46 the mixer, 47 the final p."""
    PREFIX = "vote"

    def run(self, ps, mixes, stream_bit0=0, sel=None, bits=None, stream=None):
        import torch
        assert len(ps) == self.n and len(mixes) == self.n
        T = int(ps[0].numel())
        for p, m in zip(ps, mixes):
            assert p.is_cuda and m.is_cuda and p.is_contiguous() and m.is_contiguous() and p.element_size() == 4 and m.element_size() == 4
            assert p.numel() == T and m.numel() == T * N_MIXERS
        if stream is None:
            stream = torch.cuda.current_stream(ps[0].device).cuda_stream
        ap = (C.c_void_p * 3)(*[p.data_ptr() for p in ps])
        am = (C.c_void_p * 3)(*[m.data_ptr() for m in mixes])
        if lib().cmx_vote_run(self.h, ap, am, T, int(stream_bit0), sel.data_ptr() if sel is not None else None,
                              bits.data_ptr() if bits is not None else None, C.c_void_p(stream)):
            raise CmxError(last_error())

    def values(self):
        """the captured bit of the first event: words [n, 48] u32, sel [47] u32, bit"""
        return _vote_values(lib().cmx_vote_values, self.h, self.n)


# the redundant context-stage vote (include/cmix_amd.h, cmx_ctxvote_*; the rule's specification is cmix_amd.ctxvote.ctx_vote_reference)
CTX_STATE_REGIONS = ("persist", "history", "shared_map", "bstack", "pred", "cnt", "chk", "match_map", "ihash")
CTXVOTE_COLS = 101   # CMX_CTXVOTE_COLS: 54 model outputs in lane order (layer-0 columns SMALL_COLS), then the 47 selectors
CTX_COMPACT_STRIDE = 64


def _ctx_vote_values(fn, h, n):
    return _values(fn, h, n, CTXVOTE_COLS, ("bit",))


def _ctx_state_diff(out):
    v = [int(x) for x in out]
    first = {"region": v[1], "lane": _opt(v[2]), "index": v[3], "a": v[4], "b": v[5]} if v[0] else None
    return {"words": v[0], "first": first, "per_region": dict(zip(CTX_STATE_REGIONS, v[6:15])), "lane_mask": v[15], "raw": v}


def ctx_layout():
    """word offsets inside state region 0 (CtxPersist) of regs, br_probs, ipred, mpred, and the region's words (cmx_ctxmodels_debug_layout)"""
    out = (C.c_uint64 * 5)()
    if lib().cmx_ctxmodels_debug_layout(out):
        raise CmxError(last_error())
    return dict(zip(("regs", "br_probs", "ipred", "mpred", "words"), [int(x) for x in out]))


class CtxVote(_VoteBase):
    """The context-stage vote kernel over n = 2 or 3 instances' model outputs (a CUDA [T, stride] matrix of 4-byte words: stride >= 2078 the full
    layer-0 form, compact=True the [T, >= 64] form) and selectors [T, 47]; the record is sticky across run() calls. In report() and
    last(), column = the element's c (0..53 model output in lane order, 54..100 selector c - 54)."""
    PREFIX = "ctxvote"

    def run(self, probs, compact, sels, stream_bit0=0, bits=None, stream=None):
        import torch
        assert len(probs) == self.n and len(sels) == self.n and len(compact) == self.n
        T = int(sels[0].numel()) // N_MIXERS
        for p, s in zip(probs, sels):
            assert p.is_cuda and s.is_cuda and p.is_contiguous() and s.is_contiguous() and p.element_size() == 4 and s.element_size() == 4
            assert p.dim() == 2 and p.shape[0] == T and s.numel() == T * N_MIXERS
        if stream is None:
            stream = torch.cuda.current_stream(probs[0].device).cuda_stream
        ap = (C.c_void_p * 3)(*[p.data_ptr() for p in probs])
        ast = (C.c_size_t * 3)(*[p.shape[1] for p in probs])
        ac = (C.c_int * 3)(*[int(bool(c)) for c in compact])
        asel = (C.c_void_p * 3)(*[s.data_ptr() for s in sels])
        if lib().cmx_ctxvote_run(self.h, ap, ast, ac, asel, T, int(stream_bit0), bits.data_ptr() if bits is not None else None, C.c_void_p(stream)):
            raise CmxError(last_error())

    def values(self):
        """the captured bit of the first event: words [n, 101] u32, bit"""
        return _ctx_vote_values(lib().cmx_ctxvote_values, self.h, self.n)


# the redundant LSTM-stage vote (include/cmix_amd.h, cmx_lstmvote_*; the rule's specification is cmix_amd.lstmvote.lstm_vote_reference)
LSTM_STATE_REGIONS = ("W", "WT", "M", "Vv", "gb", "caches", "recurrent", "layer_input", "output_layer", "indices", "probs_rings")
LSTMVOTE_COLS = 272   # CMX_LSTMVOTE_COLS: the 256 distribution words of a byte, its 8 bit predictions, its 8 ex words
# the arrays of cmx_lstm_state_diff in their fixed order (l = layer outside, g = gate inside)
LSTM_STATE_ARRAYS = tuple(["%s[%d][%d]" % (a, l, g) for a in ("W", "WT", "M", "Vv", "gb") for l in range(2) for g in range(3)] + ["adam_tab"] +
                          ["%s[%d][%d]" % (a, l, g) for a in ("norm", "gstate", "ivar", "E") for l in range(2) for g in range(3)] +
                          ["%s[%d]" % (a, l) for a in ("last_state", "tanh_state", "in_gate_state") for l in range(2)] +
                          ["stateb[0][0]", "stateb[0][1]", "stateb[1][0]", "stateb[1][1]", "hid[0]", "hid[1]", "layer_input[0]", "layer_input[1]", "OL", "output",
                           "input_history", "bp_symbol", "dyn", "byte_probs", "d_prev_probs", "raw_ring", "h_ring", "logit_ring", "bp_pub"])


def _lstm_vote_values(fn, h, n):
    return _values(fn, h, n, LSTMVOTE_COLS, ("byte",))


def _lstm_state_diff(out, regions=LSTM_STATE_REGIONS):
    """cmx_lstm_state_diff's words, and cmx_fxcm_state_diff's with its regions"""
    v = [int(x) for x in out]
    first = {"region": v[1], "index": v[2], "a": v[3], "b": v[4]} if v[0] else None
    return {"words": v[0], "first": first, "per_region": dict(zip(regions, v[5:5 + len(regions)])), "raw": v}


def lstm_layout(lstm):
    """the state arrays of an Lstm handle in cmx_lstm_state_diff's order (cmx_lstm_debug_layout): list of dicts name, region (its name), offset (words
    inside the region), words -- for the handle's vocabulary size"""
    out = (C.c_uint64 * (3 * len(LSTM_STATE_ARRAYS)))()
    n = lib().cmx_lstm_debug_layout(lstm.h, out)
    if n != len(LSTM_STATE_ARRAYS):
        raise CmxError(last_error() if n < 0 else "cmx_lstm_debug_layout: %d arrays, expected %d" % (n, len(LSTM_STATE_ARRAYS)))
    return [{"name": LSTM_STATE_ARRAYS[i], "region": LSTM_STATE_REGIONS[int(out[3 * i])], "offset": int(out[3 * i + 1]), "words": int(out[3 * i + 2])} for i in range(n)]


class LstmVote(_VoteBase):
    """The LSTM-stage vote kernel over n = 2 or 3 instances' distributions [N, 256], bit predictions and ex [N, 8] (CUDA tensors of 4-byte words); an
    instance's bit predictions may instead be a [8N, 2078] layer-0 matrix, read in place from its column 2077. In report() and last(), bytes stand
    for bits: bits = bytes voted, first_bit / bit = the stream byte, column = the element's c (0..255 distribution entry, 256..263 bit prediction,
    264..271 ex)."""
    PREFIX = "lstmvote"

    def run(self, dists, bit_ps, exs, stream_byte0=0, data=None, stream=None):
        import torch
        assert len(dists) == self.n and len(bit_ps) == self.n and len(exs) == self.n
        N = int(exs[0].numel()) // 8
        ptr, stride = [], []
        for d, p, x in zip(dists, bit_ps, exs):
            assert d.is_cuda and p.is_cuda and x.is_cuda and d.is_contiguous() and p.is_contiguous() and x.is_contiguous()
            assert d.element_size() == 4 and p.element_size() == 4 and x.element_size() == 4 and d.numel() == N * 256 and x.numel() == N * 8
            if p.dim() == 2 and p.shape == (8 * N, N_INPUTS):   # layer-0 rows: column 2077 in place
                ptr.append(p.data_ptr() + 4 * (N_INPUTS - 1))
                stride.append(N_INPUTS)
            else:
                assert p.numel() == N * 8
                ptr.append(p.data_ptr())
                stride.append(1)
        if stream is None:
            stream = torch.cuda.current_stream(dists[0].device).cuda_stream
        ad = (C.c_void_p * 3)(*[d.data_ptr() for d in dists])
        ap = (C.c_void_p * 3)(*ptr)
        ast = (C.c_size_t * 3)(*stride)
        ax = (C.c_void_p * 3)(*[x.data_ptr() for x in exs])
        if lib().cmx_lstmvote_run(self.h, ad, ap, ast, ax, N, int(stream_byte0), data.data_ptr() if data is not None else None, C.c_void_p(stream)):
            raise CmxError(last_error())

    def values(self):
        """the captured row of the first event: words [n, 272] u32, byte"""
        return _lstm_vote_values(lib().cmx_lstmvote_values, self.h, self.n)


# the redundant fxcm-stage vote (include/cmix_amd.h, cmx_fxcmvote_*; the rule's specification is cmix_amd.fxcmvote.fxcm_vote_reference)
FXCM_STATE_REGIONS = ("const_tables", "map_buckets", "map_statemaps", "sscm", "sm1_t", "rcm_t", "mhash", "sp_table", "buffer", "wx", "apm", "fxdev")
FXCMVOTE_COLS = 431   # CMX_FXCMVOTE_COLS: FXCM::Predict()'s values of one bit = layer-0 columns 3..433
# the arrays of cmx_fxcm_state_diff in their fixed order (src/fxcm_build.h's blocks, region by region)
FXCM_STATE_ARRAYS = tuple(["squash", "stretch", "wrt"] + ["sta[%d]" % i for i in range(6)] + ["maps[%d].tab" % k for k in range(31)] + ["apm_pattern[%d]" % j for j in range(6)] +
                          ["maps[%d].t" % k for k in range(31)] + ["maps[%d].sm" % k for k in range(31)] + ["sscm_data[%d]" % j for j in range(7)] +
                          ["sm1_t[%d]" % j for j in range(3)] + ["rcm_t", "mhash", "sp_table", "buffer"] + ["wx[%d]" % k for k in range(12)] +
                          ["apm_t[%d]" % j for j in range(6)] + ["FxDev"])


def _fxcm_vote_values(fn, h, n):
    return _values(fn, h, n, FXCMVOTE_COLS, ("bit", "byte"))


def _fxcm_state_diff(out):
    return _lstm_state_diff(out, FXCM_STATE_REGIONS)


def fxcm_layout(fx):
    """the state arrays of an Fxcm handle in cmx_fxcm_state_diff's order (cmx_fxcm_debug_layout): list of dicts name, region (its name), offset (words
    inside the region), words; the last one is FxDev itself"""
    out = (C.c_uint64 * (3 * len(FXCM_STATE_ARRAYS)))()
    n = lib().cmx_fxcm_debug_layout(fx.h, out)
    if n != len(FXCM_STATE_ARRAYS):
        raise CmxError(last_error() if n < 0 else "cmx_fxcm_debug_layout: %d arrays, expected %d" % (n, len(FXCM_STATE_ARRAYS)))
    return [{"name": FXCM_STATE_ARRAYS[i], "region": FXCM_STATE_REGIONS[int(out[3 * i])], "offset": int(out[3 * i + 1]), "words": int(out[3 * i + 2])} for i in range(n)]


class FxcmVote(_VoteBase):
    """The fxcm-stage vote kernel over n = 2 or 3 instances' rows (CUDA float32 / 4-byte-word tensors [T, stride]): a [T, 2078] layer-0 matrix is read in
    place from its columns 3..433, a [T, 434] matrix (what Fxcm.run_shared writes) from columns 3..433 as well, a [T, 431] matrix as it is. The record is
    sticky across run(). In report() and last(), column = the fxcm column c (layer-0 column 3 + c)."""
    PREFIX = "fxcmvote"

    def run(self, rows, stream_bit0=0, data=None, stream=None):
        import torch
        assert len(rows) == self.n
        T = int(rows[0].shape[0])
        ptr, stride = [], []
        for r in rows:
            assert r.is_cuda and r.is_contiguous() and r.element_size() == 4 and r.dim() == 2 and r.shape[0] == T and r.shape[1] >= FXCMVOTE_COLS
            ptr.append(r.data_ptr() + (0 if r.shape[1] == FXCMVOTE_COLS else 12))
            stride.append(int(r.shape[1]))
        if stream is None:
            stream = torch.cuda.current_stream(rows[0].device).cuda_stream
        ap = (C.c_void_p * 3)(*ptr)
        ast = (C.c_size_t * 3)(*stride)
        if lib().cmx_fxcmvote_run(self.h, ap, ast, T, int(stream_bit0), data.data_ptr() if data is not None else None, C.c_void_p(stream)):
            raise CmxError(last_error())

    def values(self):
        """the captured row of the first event: words [n, 431] u32, the bit coded there and its byte"""
        return _fxcm_vote_values(lib().cmx_fxcmvote_values, self.h, self.n)


def probe_libm(which, x, device=0):
    """which: 0 expf, 1 tanhf, 2 logistic; x: float32 ndarray -> float32 ndarray (device-evaluated)."""
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    if lib().cmx_probe_libm(device, which, x.ctypes.data, y.ctypes.data, x.size):
        raise CmxError(last_error())
    return y


def lds_fill(pattern, device=0):
    """Test probe: write the 32-bit `pattern` over the LDS of every compute unit (device synchronise, fill on the null stream, synchronise).
    -> dict(resident, workgroups, bytes_per_workgroup, launches, compute_units, bytes_per_cu, uncovered_bytes_per_cu, full); `full` means
    every workgroup saw all others resident at once and no byte of a compute unit's LDS was out of the grid's reach.
    Never between late_start and late_stop: the decoder's kernels are resident there and the synchronise would wait for them."""
    out = (C.c_uint32 * 8)()
    if lib().cmx_probe_lds_fill(device, int(pattern) & 0xFFFFFFFF, out):
        raise CmxError(last_error())
    keys = ("resident", "workgroups", "bytes_per_workgroup", "launches", "compute_units", "bytes_per_cu", "uncovered_bytes_per_cu")
    d = {k: int(out[i]) for i, k in enumerate(keys)}
    d["full"] = d["workgroups"] > 0 and d["resident"] == d["workgroups"] and d["uncovered_bytes_per_cu"] == 0
    return d


JOURNAL_RECORD = 180   # CMX_JOURNAL_RECORD: a block's end byte position, then its 179 words (cmix_amd/journal.py)


def _journal_records(rec):
    """(ends [n] u64, words [n, 179] u64) of n records as the library hands them out"""
    rec = rec.reshape(-1, JOURNAL_RECORD)
    return rec[:, 0].copy(), rec[:, 1:].copy()


def journal_host_digest(p, bits, stream_bit0=0, log2=19):
    """cmx_journal_host_digest: the p and bits words of HOST values (either may be None), no device: (ends [n], p words [n], bits words [n])."""
    p = None if p is None else np.ascontiguousarray(p, np.float32)
    bits = None if bits is None else np.ascontiguousarray(bits, np.uint8)
    n = len(p) if p is not None else len(bits)
    if n == 0 or not 6 <= log2 <= 19:
        raise CmxError("journal_host_digest: no bits, or log2 not 6..19")
    span = ((stream_bit0 + n - 1) >> log2) - (stream_bit0 >> log2) + 1
    out = np.zeros((span, 3), np.uint64)
    got = lib().cmx_journal_host_digest(p.ctypes.data if p is not None else None, bits.ctypes.data if bits is not None else None, n, stream_bit0, log2, out.ctypes.data)
    if got != span:
        raise CmxError("cmx_journal_host_digest: %d blocks, expected %d" % (got, span))
    return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy()


def state_digest_host(words):
    """cmx_state_digest_host: the state digest (include/cmix_amd.h, "State digest") of HOST 32-bit words, in plain C++ (no device)."""
    w = np.ascontiguousarray(words).view(np.uint32).ravel()
    return int(lib().cmx_state_digest_host(w.ctypes.data if len(w) else None, len(w)))


def state_digest_arrays(tensors, device=0):
    """cmx_state_digest_arrays: the digests of a list of cuda tensors (4-byte elements, contiguous, each an allocation of its own) in ONE launch."""
    n = len(tensors)
    ptrs = (C.c_void_p * max(n, 1))(*[t.data_ptr() if t.numel() else None for t in tensors])
    words = np.array([t.numel() for t in tensors], np.uint64)
    assert all(t.is_cuda and t.element_size() == 4 and t.is_contiguous() for t in tensors)
    out = np.zeros(max(n, 1), np.uint64)
    if lib().cmx_state_digest_arrays(device, ptrs, words.ctypes.data, n, out.ctypes.data):
        raise CmxError(last_error())
    return out[:n]


def _state_digest(fn, h, per=1):
    """one of the cmx_*_state_digest / _layout calls: `per` words per column"""
    n = fn(h, None, 0)
    if n < 0:
        raise CmxError(last_error())
    out = np.zeros(max(n, 1) * per, np.uint64)
    if fn(h, out.ctypes.data, len(out)) != n:
        raise CmxError(last_error())
    return out[:n * per].reshape(n, per) if per > 1 else out[:n]


class _StateDigest:
    """state_digest() / state_digest_layout() of a stage handle (include/cmix_amd.h, "State digest"): one 64-bit digest per state array and a last one
    over the words the stage's state_diff compares on the host; the layout gives (region, word offset inside the region, words) per column."""
    _sd = None   # the stage's name in the C ABI

    def state_digest(self):
        return _state_digest(getattr(lib(), "cmx_%s_state_digest" % self._sd), self.h)

    def state_digest_layout(self):
        return _state_digest(getattr(lib(), "cmx_%s_debug_layout" % self._sd if self._sd == "p8stage" else "cmx_%s_state_digest_layout" % self._sd), self.h, 3)


class Journal:
    """The stand-alone stream journal (include/cmix_amd.h, cmx_journal_*): per-block digests of rows, selectors, bits and p on the device."""

    def __init__(self, device=0, log2=19):
        self.h = lib().cmx_journal_create(device, log2)
        if not self.h:
            raise CmxError(last_error())

    def run(self, rows, sel, bits, p, stream_bit0=0, stream=None):
        """rows: f32 cuda [T, >= 2078] (its row stride is the ld; a column slice of a wider matrix is fine), sel int32 cuda [T, 47], bits u8 cuda [T],
        p f32 cuda [T]; any may be None. Consecutive calls continue the stream and accumulate."""
        T = next(len(x) for x in (rows, sel, bits, p) if x is not None)
        ld = 0
        if rows is not None:
            assert rows.is_cuda and rows.dim() == 2 and rows.shape[0] == T and rows.stride(1) == 1 and rows.element_size() == 4
            ld = rows.stride(0)
        for x in (sel, bits, p):
            assert x is None or (x.is_cuda and x.is_contiguous() and x.shape[0] == T)
        assert sel is None or (sel.element_size() == 4 and sel.shape[1] == 47)
        assert bits is None or bits.element_size() == 1
        assert p is None or p.element_size() == 4
        ptr = lambda x: None if x is None else x.data_ptr()   # noqa: E731
        if lib().cmx_journal_run(self.h, ptr(rows), ld, ptr(sel), ptr(bits), ptr(p), T, stream_bit0, C.c_void_p(stream)):
            raise CmxError(last_error())

    def blocks(self):
        n = C.c_uint64(0)
        if lib().cmx_journal_blocks(self.h, C.byref(n)):
            raise CmxError(last_error())
        return n.value

    def read(self):
        """(ends, words [nblocks, 179]) of every block so far"""
        n = self.blocks()
        rec = np.zeros((n, JOURNAL_RECORD), np.uint64)
        if n and lib().cmx_journal_read(self.h, 0, n, rec.ctypes.data):
            raise CmxError(last_error())
        return _journal_records(rec)

    def close(self):
        if getattr(self, "h", None):
            lib().cmx_journal_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MixNet(_StateDigest):
    """Final mixing network stage (layers 0-2 + SSE) of one stream on one GPU."""

    _sd = "mixnet"

    def __init__(self, device=0):
        self.h = lib().cmx_mixnet_create(device)
        if not self.h:
            raise CmxError(last_error())
        self.device = device

    def set_tolerance(self, on=True):
        """Tolerance mode (NOT bit-exact: layer-0 dot products as f64 tree sums): explicit, before the handle's first bit."""
        if lib().cmx_mixnet_set_tolerance(self.h, int(bool(on))):
            raise CmxError(last_error())

    def set_verify(self, on=True):
        """Verify mode (include/cmix_amd.h): every word the network consumes checked against its source; explicit, before the handle's first bit."""
        if lib().cmx_mixnet_set_verify(self.h, int(bool(on))):
            raise CmxError(last_error())

    def verify_report(self):
        """dict: chunks, bits verified, mismatches, and of the first mismatch: cls (VERIFY_CLASSES), first_bit (its block's first stream bit), mixer, row,
        segment (None where they do not apply). Synchronises the device."""
        return _verify_report(lib().cmx_mixnet_verify_report, self.h)

    def debug_verify_perturb(self, cls, bit, index, xor_mask):
        """Test hook: one perturbation of class `cls` (number or VERIFY_CLASS key) for the next run (include/cmix_amd.h)."""
        cls = VERIFY_CLASS.get(cls, cls)
        if lib().cmx_mixnet_debug_verify_perturb(self.h, int(cls), int(bit), int(index), int(xor_mask)):
            raise CmxError(last_error())

    def state_diff(self, other):
        """Every word of this handle's and `other`'s state in HBM compared (include/cmix_amd.h, cmx_mixnet_state_diff): dict words, first
        (region, mixer, row, index, a, b -- None where a field does not apply), per_region, layer0_mask, layer12_mask, raw. Synchronises the device."""
        out = (C.c_uint64 * 20)()
        if lib().cmx_mixnet_state_diff(self.h, other.h, out):
            raise CmxError(last_error())
        return _state_diff(out)

    def state_repair(self, src):
        """Every state word of this handle that differs from `src`'s overwritten with src's (include/cmix_amd.h, cmx_mixnet_state_repair); returns
        what state_diff(src) would have returned just before. Between chunks; synchronises the device."""
        out = (C.c_uint64 * 20)()
        if lib().cmx_mixnet_state_repair(self.h, src.h, out):
            raise CmxError(last_error())
        return _state_diff(out)

    def debug_state_xor(self, region, mixer, row, index, xor_mask):
        """Test hook: XOR one state word (region: number or STATE_REGIONS name), between chunks."""
        if lib().cmx_mixnet_debug_state_xor(self.h, _region(region), _u64(mixer), _u64(row), _u64(index), int(xor_mask)):
            raise CmxError(last_error())

    def close(self):
        if getattr(self, "h", None):
            lib().cmx_mixnet_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, probs, sel, bits, p_out=None, mix_out=None, stream=None):
        """Chunk mode on HBM-resident torch tensors.
        probs [T,2078] f32, sel [T,47] int32 (u32 keys), bits [T] u8 -> p_out [T] f32."""
        import torch
        T = int(bits.numel())
        assert probs.is_cuda and sel.is_cuda and bits.is_cuda
        assert probs.dtype == torch.float32 and probs.is_contiguous() and probs.numel() == T * N_INPUTS
        assert sel.dtype == torch.int32 and sel.is_contiguous() and sel.numel() == T * N_MIXERS
        assert bits.dtype == torch.uint8 and bits.is_contiguous()
        if p_out is None:
            p_out = torch.empty(T, dtype=torch.float32, device=probs.device)
        if stream is None:
            stream = torch.cuda.current_stream(probs.device).cuda_stream
        rc = lib().cmx_mixnet_run(self.h, probs.data_ptr(), sel.data_ptr(), bits.data_ptr(), T,
                                  p_out.data_ptr(), mix_out.data_ptr() if mix_out is not None else None,
                                  C.c_void_p(stream))
        if rc:
            raise CmxError(last_error())
        return p_out

    def predict(self, probs, sel):
        """Bit-synchronous Predict(): host arrays in, float out."""
        probs = np.ascontiguousarray(probs, np.float32)
        sel = np.ascontiguousarray(sel, np.uint32)
        assert probs.size == N_INPUTS and sel.size == N_MIXERS
        p = lib().cmx_mixnet_predict(self.h, probs.ctypes.data, sel.ctypes.data)
        if p < 0:
            raise CmxError(last_error())
        return np.float32(p)

    def perceive(self, bit):
        if lib().cmx_mixnet_perceive(self.h, int(bit)):
            raise CmxError(last_error())

    def sync(self):
        if lib().cmx_mixnet_sync(self.h):
            raise CmxError(last_error())

    def bits_done(self):
        v = C.c_uint64(0)
        if lib().cmx_mixnet_bits_done(self.h, C.byref(v)):
            raise CmxError(last_error())
        return v.value

    def profile(self, enable=True):
        out = (C.c_uint64 * 16)()
        if lib().cmx_mixnet_profile(self.h, int(enable), out):
            raise CmxError(last_error())
        return list(out)

    def last_kernel_ms(self):
        v = C.c_float(0)
        if lib().cmx_mixnet_last_kernel_ms(self.h, C.byref(v)):
            raise CmxError(last_error())
        return v.value

    def debug_set_steps(self, steps):
        """Test hook (state injection): the network as after `steps` bits -- Mixer::steps_ of all 47 mixers."""
        lib().cmx_mixnet_debug_set_steps.argtypes = [C.c_void_p, C.c_uint64]
        if lib().cmx_mixnet_debug_set_steps(self.h, int(steps)):
            raise CmxError(last_error())

    def spec_stats(self):
        """Speculative segment-parallel chain (cmx_mixnet_spec_kernel): segments run, resolved from a candidate, re-runs of segment 1..3."""
        out = (C.c_uint64 * 5)()
        if lib().cmx_mixnet_spec_stats(self.h, out):
            raise CmxError(last_error())
        v = list(out)
        return {"segments": v[0], "hits": v[1], "reruns": v[2:5], "hit_rate": (v[1] / v[0]) if v[0] else None}

    def spec_rerun_stats(self):
        """How the re-runs of spec_stats() were executed (the split re-run): resolved from a mid-point candidate lane / second half run
        serially from the true mid-point. mid_hits + serial_halves == sum(spec_stats()["reruns"])."""
        out = (C.c_uint64 * 2)()
        lib().cmx_mixnet_spec_rerun_stats.argtypes = [C.c_void_p, C.c_void_p]
        if lib().cmx_mixnet_spec_rerun_stats(self.h, out):
            raise CmxError(last_error())
        return {"mid_hits": int(out[0]), "serial_halves": int(out[1])}


class Lstm(_StateDigest):
    """Byte-level LSTM byte mixer stage of one stream on one GPU (chunk mode)."""
    SKIP_RAND = 31

    _sd = "lstm"

    def __init__(self, vocab, device=0, skip_rand=SKIP_RAND):
        vocab = np.ascontiguousarray(vocab, np.uint8)
        assert vocab.size == 256
        self.h = lib().cmx_lstm_create(vocab.ctypes.data, skip_rand, device)
        if not self.h:
            raise CmxError(last_error())
        self.V = lib().cmx_lstm_vocab_size(self.h)

    def set_tolerance(self, on=True):
        """TOLERANCE mode (NOT bit-exact): the BPTT round's weight-update contraction as v_mfma_f32_16x16x4_f32 tiles"""
        if lib().cmx_lstm_set_tolerance(self.h, 1 if on else 0):
            raise CmxError(last_error())

    def close(self):
        if getattr(self, "h", None):
            lib().cmx_lstm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, in_probs, data, want_bits=True, stream=None, layer0=None, out=None):
        """in_probs [N,256] f32 cuda, data [N] u8 cuda -> (out_probs [N,256], bit_p [N,8], bit_ex [N,8]).
        With layer0 = the [8N,2078] layer-0 matrix, the bit predictions are written in place into its
        column 2077 (and bit_p is None)."""
        import torch
        N = int(data.numel())
        assert in_probs.is_cuda and in_probs.dtype == torch.float32 and in_probs.is_contiguous()
        assert in_probs.numel() == N * 256 and data.dtype == torch.uint8 and data.is_contiguous()
        if out is None:
            out = torch.empty((N, 256), dtype=torch.float32, device=in_probs.device)
        bp, bp_ptr, stride = None, None, 1
        if layer0 is not None:
            assert layer0.dtype == torch.float32 and layer0.is_contiguous() and layer0.shape == (8 * N, N_INPUTS)
            bp_ptr, stride = layer0.data_ptr() + 4 * (N_INPUTS - 1), N_INPUTS
        elif want_bits:
            bp = torch.empty((N, 8), dtype=torch.float32, device=in_probs.device)
            bp_ptr = bp.data_ptr()
        bx = torch.empty((N, 8), dtype=torch.int32, device=in_probs.device) if bp_ptr else None
        if stream is None:
            stream = torch.cuda.current_stream(in_probs.device).cuda_stream
        rc = lib().cmx_lstm_run(self.h, in_probs.data_ptr(), data.data_ptr(), N, out.data_ptr(),
                                bp_ptr, stride, bx.data_ptr() if bx is not None else None, C.c_void_p(stream))
        if rc:
            raise CmxError(last_error())
        return out, bp, bx

    def state_diff(self, other):
        """Every word of this handle's and `other`'s state in HBM compared (include/cmix_amd.h, cmx_lstm_state_diff): dict words, first (region, index,
        a, b), per_region, raw. Raises when a host-side counter differs. Synchronises the device."""
        out = (C.c_uint64 * 16)()
        if lib().cmx_lstm_state_diff(self.h, other.h, out):
            raise CmxError(last_error())
        return _lstm_state_diff(out)

    def debug_state_xor(self, region, index, xor_mask):
        """Test hook: XOR one state word (region: number or LSTM_STATE_REGIONS name) between runs; the index region is refused."""
        if lib().cmx_lstm_debug_state_xor(self.h, _region(region, LSTM_STATE_REGIONS), int(index), int(xor_mask)):
            raise CmxError(last_error())

    def gate_weights(self, layer, gate):
        n = lib().cmx_lstm_gate_rowlen(self.h, layer)
        out = np.empty((200, n), np.float32)
        if lib().cmx_lstm_get_gate_weights(self.h, layer, gate, out.ctypes.data):
            raise CmxError("cmx_lstm_get_gate_weights failed")
        return out


SMALL_COLS = [0, 1, 2] + list(range(2025, 2076))  # layer-0 columns the ctx/small-model stage writes


class CtxModels(_StateDigest):
    """Context plumbing + the 54 small native models of one stream on one GPU (chunk mode)."""

    _sd = "ctxmodels"

    def __init__(self, vocab, device=0, compact=False):
        """compact=True: model l writes column l of a [8N, >= 64] matrix (include/cmix_amd.h, cmx_ctxmodels_create_compact); the state is the same"""
        vocab = np.ascontiguousarray(vocab, np.uint8)
        assert vocab.size == 256
        self.compact = bool(compact)
        self.h = (lib().cmx_ctxmodels_create_compact if self.compact else lib().cmx_ctxmodels_create)(vocab.ctypes.data, device)
        if not self.h:
            raise CmxError(last_error())

    def state_diff(self, other):
        """Every word of this handle's and `other`'s state in HBM compared (include/cmix_amd.h, cmx_ctxmodels_state_diff): dict words, first (region,
        lane -- None in the regions without lanes --, index, a, b), per_region, lane_mask, raw. Synchronises the device."""
        out = (C.c_uint64 * 16)()
        if lib().cmx_ctxmodels_state_diff(self.h, other.h, out):
            raise CmxError(last_error())
        return _ctx_state_diff(out)

    def debug_state_xor(self, region, lane, index, xor_mask):
        """Test hook: XOR one state word (region: number or CTX_STATE_REGIONS name; lane None in regions 0..3), between chunks."""
        if lib().cmx_ctxmodels_debug_state_xor(self.h, _region(region, CTX_STATE_REGIONS), _u64(lane), int(index), int(xor_mask)):
            raise CmxError(last_error())

    def close(self):
        if getattr(self, "h", None):
            lib().cmx_ctxmodels_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, data, probs=None, sel=None, stream=None):
        """data [N] u8 cuda -> writes columns SMALL_COLS of probs [8N,2078] f32 and sel [8N,47] i32 (u32 keys)."""
        import torch
        N = int(data.numel())
        assert data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous()
        if probs is None:
            probs = torch.full((8 * N, CTX_COMPACT_STRIDE if self.compact else N_INPUTS), 0.5, dtype=torch.float32, device=data.device)
        if sel is None:
            sel = torch.zeros((8 * N, N_MIXERS), dtype=torch.int32, device=data.device)
        assert probs.dtype == torch.float32 and probs.is_contiguous() and probs.shape[0] == 8 * N
        assert sel.dtype == torch.int32 and sel.is_contiguous() and sel.numel() == 8 * N * N_MIXERS
        if stream is None:
            stream = torch.cuda.current_stream(data.device).cuda_stream
        rc = lib().cmx_ctxmodels_run(self.h, data.data_ptr(), N, probs.data_ptr(), probs.shape[1], sel.data_ptr(),
                                     C.c_void_p(stream))
        if rc:
            raise CmxError(last_error())
        return probs, sel

    def pretrain(self, data, stream=None):
        """Predictor::Pretrain over data [N] u8 cuda (dictionary warm-up): state only, no outputs."""
        import torch
        assert data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous()
        if stream is None:
            stream = torch.cuda.current_stream(data.device).cuda_stream
        if lib().cmx_ctxmodels_pretrain(self.h, data.data_ptr(), int(data.numel()), C.c_void_p(stream)):
            raise CmxError(last_error())

    def peek(self, byte, probs8, sel8, stream=None):
        """Bit-synchronous mode: the 8 rows the stage would write if the next byte were byte[0] (u8 cuda), leaving
        all state untouched; row j is exact when the top j bits of byte[0] are the coded ones."""
        import torch
        assert byte.is_cuda and byte.dtype == torch.uint8 and probs8.shape == (8, N_INPUTS) and sel8.numel() == 8 * N_MIXERS
        if stream is None:
            stream = torch.cuda.current_stream(byte.device).cuda_stream
        if lib().cmx_ctxmodels_peek(self.h, byte.data_ptr(), -1, probs8.data_ptr(), N_INPUTS, sel8.data_ptr(),
                                    C.c_void_p(stream)):
            raise CmxError(last_error())

    def debug_set_history(self, pos, tail):
        """Test hook (state injection): the stage as after `pos` bytes of a stream that ended in `tail` -- history ring position, Match counters."""
        tail = np.ascontiguousarray(np.frombuffer(bytes(tail), np.uint8))
        lib().cmx_ctxmodels_debug_set_history.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
        if lib().cmx_ctxmodels_debug_set_history(self.h, int(pos), tail.ctypes.data, len(tail)):
            raise CmxError(last_error())

    def slow_bytes(self):
        out = np.zeros(2, np.uint64)
        if lib().cmx_ctxmodels_debug_slow_bytes(self.h, out.ctypes.data):
            raise CmxError(last_error())
        return int(out[0]), int(out[1])

    def sync(self):
        if lib().cmx_ctxmodels_sync(self.h):
            raise CmxError(last_error())

    def manager(self):
        regs = np.empty(25, np.uint64)
        ctx = np.empty(54, np.uint64)
        bctx = np.empty(8, np.uint64)
        if lib().cmx_ctxmodels_get_manager(self.h, regs.ctypes.data, ctx.ctypes.data, bctx.ctypes.data):
            raise CmxError(last_error())
        return regs, ctx, bctx


def bytemodel_bits(dist0, dist_rest, data, layer0, col, device=0, stream=None):
    """ByteModel::Predict/Perceive along known bytes for any byte model (PPMd: col 2076): dist0 [256] is the
    distribution going into byte 0, dist_rest [N-1.., 256] the one after each byte; writes layer0[:, col]."""
    import torch
    N = int(data.numel())
    assert layer0.dtype == torch.float32 and layer0.is_contiguous() and layer0.shape == (8 * N, N_INPUTS)
    assert dist0.is_contiguous() and dist_rest.is_contiguous() and dist_rest.numel() >= (N - 1) * 256
    if stream is None:
        stream = torch.cuda.current_stream(data.device).cuda_stream
    rc = lib().cmx_bytemodel_bits_run(device, dist0.data_ptr(), dist_rest.data_ptr(), data.data_ptr(), N,
                                      layer0.data_ptr() + 4 * col, N_INPUTS, None, C.c_void_p(stream))
    if rc:
        raise CmxError(last_error())


# The four kinds of shadow stages (include/cmix_amd.h, cmx_pipeline_set_shadow and its three kin) by the stem of their C symbols: how a vote's captured
# values decode and how many pointers the call takes, how a state_diff decodes and its words, the state regions' names, and the u64 words that
# debug_*_xor takes between the region and the mask
_SHADOW = {
    "shadow": {"values": _vote_values, "values_args": 3, "diff": _state_diff, "diff_len": 20, "regions": STATE_REGIONS, "xor_words": 3},
    "ctx_shadow": {"values": _ctx_vote_values, "values_args": 2, "diff": _ctx_state_diff, "diff_len": 16, "regions": CTX_STATE_REGIONS, "xor_words": 2},
    "lstm_shadow": {"values": _lstm_vote_values, "values_args": 2, "diff": _lstm_state_diff, "diff_len": 16, "regions": LSTM_STATE_REGIONS, "xor_words": 1},
    "fxcm_shadow": {"values": _fxcm_vote_values, "values_args": 3, "diff": _fxcm_state_diff, "diff_len": 17, "regions": FXCM_STATE_REGIONS, "xor_words": 1},
}


class _Shadows:
    """The calls behind Pipeline's and Predictor's shadow methods, by kind (a key of _SHADOW); _C is the front of the class's C symbols."""

    def _shadow_c(self, name):
        return getattr(lib(), self._C + name)

    def _shadow_set(self, stem, k):
        if self._shadow_c("set_" + stem)(self.h, int(k)):
            raise CmxError(last_error())
        setattr(self, "_" + stem, int(k))

    def _shadow_report(self, stem):
        return _vote_report(self._shadow_c(stem + "_report"), self.h)

    def _shadow_values(self, stem):
        return _SHADOW[stem]["values"](self._shadow_c(stem + "_values"), self.h, 1 + getattr(self, "_" + stem, 0))

    def _shadow_state_diff(self, stem, a, b):
        out = (C.c_uint64 * _SHADOW[stem]["diff_len"])()
        if self._shadow_c(stem + "_state_diff")(self.h, int(a), int(b), out):
            raise CmxError(last_error())
        return _SHADOW[stem]["diff"](out)

    def _shadow_xor(self, stem, head, region, where, xor_mask):
        """head: (instance,), or a Predictor's (after_chunk, instance); where: the kind's words between region and mask"""
        if self._shadow_c("debug_" + stem + "_xor")(self.h, *[int(x) for x in head], _region(region, _SHADOW[stem]["regions"]), *where, int(xor_mask)):
            raise CmxError(last_error())


class Pipeline(_Shadows):
    """One stream through every stage built so far (native orchestration in libcmixamd.so)."""
    _C = "cmx_pipeline_"

    def __init__(self, vocab, device=0, max_chunk_bytes=4096):
        vocab = np.ascontiguousarray(vocab, np.uint8)
        assert vocab.size == 256
        self.h = lib().cmx_pipeline_create(vocab.ctypes.data, device, max_chunk_bytes)
        if not self.h:
            raise CmxError(last_error())

    def submit(self, data, layer0, p_out):
        """data: bytes / u8 array (host); layer0 [8n,2078] f32 cuda with columns 3..2024 filled and synchronised;
        p_out [8n] f32 cuda. Asynchronous."""
        import torch
        data = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8))
        n = len(data)
        assert layer0.is_cuda and layer0.dtype == torch.float32 and layer0.is_contiguous() and layer0.shape == (8 * n, N_INPUTS)
        assert p_out.is_cuda and p_out.dtype == torch.float32 and p_out.is_contiguous() and p_out.numel() == 8 * n
        if lib().cmx_pipeline_submit(self.h, data.ctypes.data, n, layer0.data_ptr(), p_out.data_ptr()):
            raise CmxError(last_error())

    def enable_fxcm(self, dictionary_path=None):
        """Run the fxcm family as a device stage (columns 3..433) instead of taking its columns from the caller; before the first chunk."""
        if lib().cmx_pipeline_enable_fxcm(self.h, dictionary_path.encode() if isinstance(dictionary_path, str) else dictionary_path):
            raise CmxError(last_error())

    def wait(self, index):
        if lib().cmx_pipeline_wait(self.h, index):
            raise CmxError(last_error())

    def debug_mix_out(self, d_mix):
        """Diagnosis: d_mix = a CUDA float32 tensor [bits][47] that receives all 47 mixer outputs of every bit from now on (None: off)."""
        if lib().cmx_pipeline_debug_mix_out(self.h, d_mix.data_ptr() if d_mix is not None else None, d_mix.shape[0] if d_mix is not None else 0):
            raise CmxError(last_error())

    def enable_paq8(self):
        """Run the paq8 family as a device stage (columns 434..2024); before the first chunk."""
        if lib().cmx_pipeline_enable_paq8(self.h):
            raise CmxError(last_error())

    def paq8_total_ms(self):
        ms = C.c_double(0)
        lib().cmx_pipeline_paq8_total_ms(self.h, C.byref(ms))
        return ms.value

    def paq8_role_ms(self):
        """(dict of the paq8 role kernels' summed HIP-event ms, chunks collected) since the last totals reset."""
        v, c = (C.c_double * 7)(), C.c_uint64(0)
        lib().cmx_pipeline_paq8_role_ms(self.h, v, C.byref(c))
        return dict(zip(("family", "mixer", "cm2_order_n", "cm2_text", "cm2_exe", "lanes", "dmc"), [float(x) for x in v])), int(c.value)

    def host_ms(self):
        """Calling-thread wall time inside begin / finish since the last totals reset: dict of ms."""
        v = (C.c_double * 6)()
        lib().cmx_pipeline_host_ms(self.h, v)
        return dict(zip(("slot_wait", "ppmd", "ctx_lstm_enqueue", "fxcm_parser_enqueue", "paq8_front_enqueue", "mixnet_enqueue"), [float(x) for x in v]))

    def finish_cols(self, cols, first_col, p_out):
        """finish() with host rows covering layer-0 columns first_col .. first_col + cols.shape[1] - 1 only."""
        cols = np.ascontiguousarray(cols, np.float32)
        if lib().cmx_pipeline_finish_cols(self.h, cols.ctypes.data, first_col, cols.shape[1], p_out.data_ptr()):
            raise CmxError(last_error())

    def fxcm_total_ms(self):
        ms = C.c_double(0)
        lib().cmx_pipeline_fxcm_total_ms(self.h, C.byref(ms))
        return ms.value

    def pretrain(self, data):
        data = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8))
        if lib().cmx_pipeline_pretrain(self.h, data.ctypes.data, len(data)):
            raise CmxError(last_error())

    def sync(self):
        if lib().cmx_pipeline_sync(self.h):
            raise CmxError(last_error())

    def last_stage_ms(self):
        ms = (C.c_float * 3)()
        lib().cmx_pipeline_last_stage_ms(self.h, ms)
        return {"ctxmodels": ms[0], "lstm": ms[1], "mixnet": ms[2]}

    def begin(self, data, layer0):
        """First step of a chunk (PPMd, contexts, LSTM); up to PIPELINE_SLOTS chunks may be begun and not finished."""
        data = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8))
        self._n_begun = getattr(self, "_n_begun", [])
        self._n_begun.append(len(data))
        if lib().cmx_pipeline_begin(self.h, data.ctypes.data, len(data), layer0.data_ptr()):
            raise CmxError(last_error())

    def hints(self, nbytes):
        """The LSTM byte mixer's per-bit ByteModel::Predict value and `ex` for the oldest begun chunk (8n+1 entries)."""
        p = np.empty(8 * nbytes + 1, np.float32)
        ex = np.empty(8 * nbytes + 1, np.int32)
        if lib().cmx_pipeline_hints(self.h, p.ctypes.data, ex.ctypes.data):
            raise CmxError(last_error())
        return p, ex

    def finish(self, cols, p_out):
        """Last step of the oldest begun chunk: host rows cols [8n, 2022] (or None) + the mixing network."""
        if cols is not None:
            cols = np.ascontiguousarray(cols, np.float32)
            assert cols.shape[1] == 2022
        if lib().cmx_pipeline_finish(self.h, cols.ctypes.data if cols is not None else None, p_out.data_ptr()):
            raise CmxError(last_error())

    def stage_totals(self, reset=False):
        """Mean HIP-event ms per chunk of each stage over the chunks finished since the last reset (call after sync)."""
        ms = (C.c_double * 3)()
        n = C.c_uint64(0)
        lib().cmx_pipeline_stage_totals(self.h, ms, C.byref(n), int(reset))
        k = max(n.value, 1)
        return {"ctxmodels": ms[0] / k, "lstm": ms[1] / k, "mixnet": ms[2] / k, "chunks": n.value}

    def set_tolerance(self, on=True):
        """The mixing network's tolerance mode (NOT bit-exact): an explicit switch, before the first chunk."""
        if lib().cmx_pipeline_set_tolerance(self.h, int(bool(on))):
            raise CmxError(last_error())

    def set_verify(self, on=True):
        """The mixing network's verify mode (include/cmix_amd.h): before the first chunk; wait / fetch / sync then fail on a mismatch."""
        if lib().cmx_pipeline_set_verify(self.h, int(bool(on))):
            raise CmxError(last_error())

    def verify_report(self):
        """as MixNet.verify_report"""
        return _verify_report(lib().cmx_pipeline_verify_report, self.h)

    def set_shadow(self, k):
        """k = 0 / 1 / 2 shadow mixing networks voting on every chunk (include/cmix_amd.h): before the first chunk; wait / fetch / sync then fail
        the chunk in which the instances disagree."""
        self._shadow_set("shadow", k)

    def set_journal(self, log2=19):
        """The stream journal (include/cmix_amd.h, cmx_pipeline_set_journal): blocks of 2^log2 bits, 0 = off; before the first chunk."""
        if lib().cmx_pipeline_set_journal(self.h, int(log2)):
            raise CmxError(last_error())

    def journal(self):
        """(ends, words [nblocks, 179]) of the blocks folded so far (all of them after sync()); cmix_amd.journal reads, writes and compares them."""
        n = C.c_uint64(0)
        if lib().cmx_pipeline_journal_read(self.h, 0, 0, None, C.byref(n)):
            raise CmxError(last_error())
        rec = np.zeros((n.value, JOURNAL_RECORD), np.uint64)
        if n.value and lib().cmx_pipeline_journal_read(self.h, 0, n.value, rec.ctypes.data, None):
            raise CmxError(last_error())
        return _journal_records(rec)

    def journal_write_files(self, path, final=False):
        """Append the blocks completed since the last call to `path` and `path.inputs` (final: the partial last block too, after sync())."""
        if lib().cmx_pipeline_journal_write_files(self.h, os.fsencode(path), int(bool(final))):
            raise CmxError(last_error())

    def state_digest(self):
        """cmx_pipeline_state_digest: between chunks; sync, then every enabled stage's digests in the order mixnet, context, LSTM, fxcm, paq8."""
        return _state_digest(lib().cmx_pipeline_state_digest, self.h)

    def state_layout(self):
        """cmx_pipeline_state_layout: per column (stage, region, word offset inside the region, words)."""
        return _state_digest(lib().cmx_pipeline_state_layout, self.h, 4)

    def set_state_journal(self, every_chunks=1):
        """The state journal (include/cmix_amd.h, cmx_pipeline_set_state_journal): a record after every every_chunks-th chunk, 0 = off; before the first chunk."""
        if lib().cmx_pipeline_set_state_journal(self.h, int(every_chunks)):
            raise CmxError(last_error())

    def state_journal(self):
        """(layout [ncols, 4], byte positions [nrecords], words [nrecords, ncols]) of the records taken so far; cmix_amd.journal writes and compares them."""
        n, c = C.c_uint64(0), C.c_uint64(0)
        if lib().cmx_pipeline_state_journal_read(self.h, 0, 0, None, C.byref(n), C.byref(c)):
            raise CmxError(last_error())
        lay = self.state_layout()
        rec = np.zeros((n.value, 1 + len(lay)), np.uint64)
        if n.value and (c.value != len(lay) or lib().cmx_pipeline_state_journal_read(self.h, 0, n.value, rec.ctypes.data, None, None)):
            raise CmxError(last_error())
        return lay, rec[:, 0].copy(), rec[:, 1:].copy()

    def state_journal_write_file(self, path, final=False):
        """From now on every record goes to `path` as it is taken (final: the record after the last chunk first, if the period has not taken it)."""
        if lib().cmx_pipeline_state_journal_write_file(self.h, os.fsencode(path), int(bool(final))):
            raise CmxError(last_error())

    def set_shadow_repair(self, max_repairs):
        """Repair on the majority (include/cmix_amd.h, cmx_pipeline_set_shadow_repair): after set_shadow(2), before the first chunk; wait / fetch
        then repair the outvoted instance from the majority, up to max_repairs times, instead of failing the chunk. 0 = off."""
        if lib().cmx_pipeline_set_shadow_repair(self.h, int(max_repairs)):
            raise CmxError(last_error())

    def shadow_repairs(self):
        """dict total, log (the newest repairs, oldest first: chunk, bit, column, odd, elements, words, first, layer0_mask, layer12_mask, chunks)"""
        return _shadow_repairs(lib().cmx_pipeline_shadow_repairs, self.h)

    def shadow_report(self):
        """as Vote.report (all zero while nothing was voted)"""
        return self._shadow_report("shadow")

    def shadow_values(self):
        """as Vote.values"""
        return self._shadow_values("shadow")

    def shadow_state_diff(self, a, b):
        """MixNet.state_diff of instances a and b (0 = the stream's own network, 1.. = the shadows)"""
        return self._shadow_state_diff("shadow", a, b)

    def debug_shadow_xor(self, instance, region, mixer, row, index, xor_mask):
        """Test hook: MixNet.debug_state_xor on one instance, between chunks."""
        self._shadow_xor("shadow", (instance,), region, (_u64(mixer), _u64(row), _u64(index)), xor_mask)

    def set_ctx_shadow(self, k):
        """k = 0 / 1 / 2 shadow context stages voting on every chunk's 54 columns and 47 selectors (include/cmix_amd.h): before the first chunk and
        before pretrain; wait / fetch / sync then fail the chunk in which the instances disagree."""
        self._shadow_set("ctx_shadow", k)

    def ctx_shadow_report(self):
        """as CtxVote.report (all zero while nothing was voted)"""
        return self._shadow_report("ctx_shadow")

    def ctx_shadow_values(self):
        """as CtxVote.values"""
        return self._shadow_values("ctx_shadow")

    def ctx_shadow_state_diff(self, a, b):
        """CtxModels.state_diff of instances a and b (0 = the stream's own stage, 1.. = the shadows)"""
        return self._shadow_state_diff("ctx_shadow", a, b)

    def debug_ctx_shadow_xor(self, instance, region, lane, index, xor_mask):
        """Test hook: CtxModels.debug_state_xor on one instance, between chunks."""
        self._shadow_xor("ctx_shadow", (instance,), region, (_u64(lane), int(index)), xor_mask)

    def set_lstm_shadow(self, k):
        """k = 0 / 1 / 2 shadow LSTM stages voting on every chunk's distributions, bit predictions and ex (include/cmix_amd.h): before the first
        chunk (pretrain may have run: the LSTM is not pretrained); wait / fetch / sync then fail the chunk in which the instances disagree."""
        self._shadow_set("lstm_shadow", k)

    def lstm_shadow_report(self):
        """as LstmVote.report (all zero while nothing was voted)"""
        return self._shadow_report("lstm_shadow")

    def lstm_shadow_values(self):
        """as LstmVote.values"""
        return self._shadow_values("lstm_shadow")

    def lstm_shadow_state_diff(self, a, b):
        """Lstm.state_diff of instances a and b (0 = the stream's own stage, 1.. = the shadows)"""
        return self._shadow_state_diff("lstm_shadow", a, b)

    def debug_lstm_shadow_xor(self, instance, region, index, xor_mask):
        """Test hook: Lstm.debug_state_xor on one instance, between chunks."""
        self._shadow_xor("lstm_shadow", (instance,), region, (int(index),), xor_mask)

    def set_fxcm_shadow(self, k):
        """k = 0 / 1 / 2 shadow fxcm stages voting on every chunk's 431 columns (include/cmix_amd.h): after enable_fxcm, before the first chunk and
        before pretrain (fxcm learns the dictionary); wait / fetch / sync then fail the chunk in which the instances disagree."""
        self._shadow_set("fxcm_shadow", k)

    def fxcm_shadow_report(self):
        """as FxcmVote.report (all zero while nothing was voted)"""
        return self._shadow_report("fxcm_shadow")

    def fxcm_shadow_values(self):
        """as FxcmVote.values"""
        return self._shadow_values("fxcm_shadow")

    def fxcm_shadow_state_diff(self, a, b):
        """Fxcm.state_diff of instances a and b (0 = the stream's own stage, 1.. = the shadows), between chunks"""
        return self._shadow_state_diff("fxcm_shadow", a, b)

    def debug_fxcm_shadow_xor(self, instance, region, index, xor_mask):
        """Test hook: Fxcm.debug_state_xor on one instance, between chunks."""
        self._shadow_xor("fxcm_shadow", (instance,), region, (int(index),), xor_mask)

    def mixnet_mode(self):
        """0 strict (bit-exact, the default), 1 tolerance -- as the library reports it"""
        return lib().cmx_pipeline_mixnet_mode(self.h)

    def stage_overlap(self):
        """The last overlap probe (creation, enable_fxcm / enable_paq8, late_start): True when every stage stream of the handle ran beside all
        the others, False when some share a hardware queue (the coded bytes are the same either way; a decoder refuses to start)."""
        r = lib().cmx_pipeline_stage_overlap(self.h)
        if r < 0:
            raise CmxError("stage_overlap: the probe has not run or failed")
        return r == 1

    # ---- the decoder's form (late-bit protocol, include/cmix_amd.h section 4): fxcm and paq8 must be enabled ----
    def late_start(self, last_bit=0):
        if lib().cmx_pipeline_late_start(self.h, int(last_bit)):
            raise CmxError(last_error())

    def late_predict(self):
        p = lib().cmx_pipeline_late_predict(self.h)
        if p < 0:
            raise CmxError(last_error())
        return p

    def late_perceive(self, bit):
        if lib().cmx_pipeline_late_perceive(self.h, int(bit)):
            raise CmxError(last_error())

    def late_replay(self, bits):
        """predict / perceive over known bits in one native call -> p before each bit"""
        bits = np.ascontiguousarray(bits, np.uint8)
        p = np.empty(len(bits), np.float32)
        lib().cmx_pipeline_late_replay.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        if lib().cmx_pipeline_late_replay(self.h, bits.ctypes.data, len(bits), p.ctypes.data):
            raise CmxError(last_error())
        return p

    def late_stop(self):
        if lib().cmx_pipeline_late_stop(self.h):
            raise CmxError(last_error())

    def late_row(self):
        """(layer-0 row [2078] f32, selectors [47] u32) of the bit predicted last, copied out of the host-coherent chunk buffers."""
        sel = C.c_void_p(0)
        r = lib().cmx_pipeline_late_debug_row(self.h, C.byref(sel))
        if not r:
            raise CmxError("no pending late predict")
        row = np.ctypeslib.as_array(C.cast(r, C.POINTER(C.c_float)), (N_INPUTS,)).copy()
        s = np.ctypeslib.as_array(C.cast(sel.value, C.POINTER(C.c_uint32)), (47,)).copy()
        return row, s

    def late_mix(self):
        """the 47 Mixer::Mix values of the bit BEFORE the one predicted last (CMX_LATE_DEBUG=1 when the handle was built), or None"""
        out = np.zeros(47, np.float32)
        lib().cmx_pipeline_late_debug_mix.argtypes = [C.c_void_p, C.c_void_p]
        return None if lib().cmx_pipeline_late_debug_mix(self.h, out.ctypes.data) else out

    def late_host_ms(self):
        v, n = (C.c_double * 6)(), C.c_uint64(0)
        lib().cmx_pipeline_late_host_ms(self.h, v, C.byref(n))
        return dict(zip(("wait_p", "ppmd", "paq8_front", "fxcm_parser", "lstm_launch", "chunk_launch"), [float(x) for x in v])), int(n.value)

    def close(self):
        if getattr(self, "h", None):
            lib().cmx_pipeline_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Ppmd:
    """HOST stage: PPMd order-25 byte model (runs on a host core ahead of the device pipeline)."""

    def __init__(self, vocab, order=25, memory_mb=14000):
        vocab = np.ascontiguousarray(vocab, np.uint8)
        assert vocab.size == 256
        self.h = lib().cmx_ppmd_create_ex(vocab.ctypes.data, order, memory_mb)
        if not self.h:
            raise CmxError(last_error())

    def run(self, data):
        """data: bytes / u8 array -> [N,256] f32: the byte distribution after each byte."""
        data = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8))
        out = np.empty((len(data), 256), np.float32)
        if lib().cmx_ppmd_run(self.h, data.ctypes.data, len(data), out.ctypes.data):
            raise CmxError(last_error())
        return out

    def close(self):
        if getattr(self, "h", None):
            lib().cmx_ppmd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def glibc_rand(seed, n):
    out = np.empty(n, np.int32)
    lib().cmx_glibc_rand_selftest(seed, n, out.ctypes.data)
    return out


class Encoder:
    """Encoder::Encode / Flush (src/coder/encoder.cpp) over probabilities a pipeline chunk produced (host arrays)."""

    def __init__(self):
        self.h = lib().cmx_encoder_create()

    def encode_bits(self, p, bits):
        p = np.ascontiguousarray(p, np.float32)
        bits = np.ascontiguousarray(bits, np.uint8)
        if p.shape != bits.shape:
            raise CmxError("Encoder.encode_bits: p and bits differ in length")
        if lib().cmx_encoder_encode_bits(self.h, p.ctypes.data, bits.ctypes.data, len(p)):
            raise CmxError(last_error())

    def encode_bytes(self, p, data):
        p = np.ascontiguousarray(p, np.float32)
        data = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8))
        if len(p) != 8 * len(data):
            raise CmxError("Encoder.encode_bytes: need 8 probabilities per byte")
        if lib().cmx_encoder_encode_bytes(self.h, p.ctypes.data, data.ctypes.data, len(data)):
            raise CmxError(last_error())

    def flush(self):
        if lib().cmx_encoder_flush(self.h):
            raise CmxError(last_error())

    def data(self):
        n = lib().cmx_encoder_size(self.h)
        return C.string_at(lib().cmx_encoder_data(self.h), n) if n else b""

    def close(self):
        if self.h:
            lib().cmx_encoder_destroy(self.h)
            self.h = None

    __del__ = close


class Decoder:
    """Decoder::Decode (src/coder/decoder.cpp)."""

    def __init__(self, code):
        self._code = np.ascontiguousarray(np.frombuffer(bytes(code), np.uint8))  # kept alive: the decoder reads it
        self.h = lib().cmx_decoder_create(self._code.ctypes.data if len(self._code) else None, len(self._code))
        if not self.h:
            raise CmxError(last_error())

    def decode(self, p):
        b = lib().cmx_decoder_decode(self.h, float(p))
        if b < 0:
            raise CmxError(last_error())
        return b

    def decode_bits(self, p):
        p = np.ascontiguousarray(p, np.float32)
        bits = np.empty(len(p), np.uint8)
        if lib().cmx_decoder_decode_bits(self.h, p.ctypes.data, len(p), bits.ctypes.data):
            raise CmxError(last_error())
        return bits

    def close(self):
        if self.h:
            lib().cmx_decoder_destroy(self.h)
            self.h = None

    __del__ = close


def header_write(length, vocab, dictionary_used=False):
    """WriteHeader (src/runner.cpp:34-52)."""
    out = np.zeros(37, np.uint8)
    vocab = np.ascontiguousarray(vocab, np.uint8)
    n = lib().cmx_header_write(int(length), vocab.ctypes.data, int(bool(dictionary_used)), out.ctypes.data)
    if n == 0:
        raise CmxError(last_error())
    return out[:n].tobytes()


def header_read(buf):
    """ReadHeader (src/runner.cpp:62-84) -> (length, dictionary_used, vocab[256], header bytes consumed)."""
    b = np.ascontiguousarray(np.frombuffer(bytes(buf[:37]), np.uint8))
    length, dic, vocab = C.c_uint64(0), C.c_int(0), np.zeros(256, np.uint8)
    n = lib().cmx_header_read(b.ctypes.data if len(b) else None, len(b), C.byref(length), C.byref(dic), vocab.ctypes.data)
    if n == 0:
        raise CmxError(last_error())
    return length.value, bool(dic.value), vocab, n


class Predictor(_Shadows):
    """`class Predictor` (src/predictor.h:17-22) over cmx_create .. cmx_destroy: Predict / Perceive / Pretrain in the
    reference's strict per-bit protocol. Two modes, decided by the first call that needs device state: after
    `stage_input` (a compressor knows its bytes) the handle runs the chunk pipeline with every model family on the device and
    Predict / Perceive pop and check; without it the per-bit stages are built (what a Decoder needs) and the fxcm / paq8
    columns of each bit come from the caller (`set_model_outputs`)."""
    _C = "cmx_"

    def __init__(self, vocab, device=0, dict_path=None):
        vocab = np.ascontiguousarray(vocab, np.uint8)
        assert vocab.size == 256
        self.h = lib().cmx_create(vocab.ctypes.data, dict_path.encode() if dict_path else None, device)
        if not self.h:
            raise CmxError(last_error())

    def set_model_outputs(self, cols):
        cols = np.ascontiguousarray(cols, np.float32)
        if cols.shape != (2022,):
            raise CmxError("Predictor.set_model_outputs: need the 2022 layer-0 columns 3..2024")
        if lib().cmx_set_model_outputs(self.h, cols.ctypes.data):
            raise CmxError(last_error())

    def Predict(self):
        p = lib().cmx_predict(self.h)
        if p < 0:
            raise CmxError(last_error())
        return np.float32(p)

    def Perceive(self, bit):
        if lib().cmx_perceive(self.h, int(bit)):
            raise CmxError(last_error())

    def Pretrain(self, bit):
        if lib().cmx_pretrain(self.h, int(bit)):
            raise CmxError(last_error())

    def stage_input(self, data, end=True):
        """Look-ahead: the bytes about to be coded (appended to what is already staged); end=True marks the end of the input."""
        b = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8))
        if len(b) and lib().cmx_stage_input(self.h, b.ctypes.data, len(b)):
            raise CmxError(last_error())
        if end and lib().cmx_stage_input(self.h, None, 0):
            raise CmxError(last_error())

    def mode(self):
        n = C.c_int(0)
        return lib().cmx_mode(self.h, C.byref(n)), n.value

    def set_verify(self, on=True):
        """Verify mode of the look-ahead pipeline's mixing network: before the first stage_input; Predict then raises on a mismatch."""
        if lib().cmx_set_verify(self.h, int(bool(on))):
            raise CmxError(last_error())

    def verify_report(self):
        """as MixNet.verify_report (all zero unless the handle compresses)"""
        return _verify_report(lib().cmx_verify_report, self.h)

    def set_shadow(self, k):
        """Shadow mixing networks of the look-ahead pipeline (include/cmix_amd.h, cmx_set_shadow): before the first stage_input / Predict."""
        self._shadow_set("shadow", k)

    def set_shadow_repair(self, max_repairs):
        """Repair on the majority (include/cmix_amd.h, cmx_set_shadow_repair): after set_shadow(2), before the first stage_input / Predict."""
        if lib().cmx_set_shadow_repair(self.h, int(max_repairs)):
            raise CmxError(last_error())

    def shadow_repairs(self):
        """as Pipeline.shadow_repairs (empty unless the handle compresses)"""
        return _shadow_repairs(lib().cmx_shadow_repairs, self.h)

    def debug_shadow_xor(self, after_chunk, instance, region, mixer, row, index, xor_mask):
        """Test hook: one Pipeline.debug_shadow_xor between look-ahead chunk `after_chunk` and the next (include/cmix_amd.h)."""
        self._shadow_xor("shadow", (after_chunk, instance), region, (_u64(mixer), _u64(row), _u64(index)), xor_mask)

    def set_ctx_shadow(self, k):
        """Shadow context stages of the look-ahead pipeline (include/cmix_amd.h, cmx_set_ctx_shadow): before the first stage_input / Predict."""
        self._shadow_set("ctx_shadow", k)

    def ctx_shadow_report(self):
        """as CtxVote.report (all zero unless the handle compresses)"""
        return self._shadow_report("ctx_shadow")

    def set_lstm_shadow(self, k):
        """Shadow LSTM stages of the look-ahead pipeline (include/cmix_amd.h, cmx_set_lstm_shadow): before the first stage_input / Predict."""
        self._shadow_set("lstm_shadow", k)

    def lstm_shadow_report(self):
        """as LstmVote.report (all zero unless the handle compresses)"""
        return self._shadow_report("lstm_shadow")

    def set_fxcm_shadow(self, k):
        """Shadow fxcm stages of the look-ahead pipeline (include/cmix_amd.h, cmx_set_fxcm_shadow): before the first stage_input / Predict."""
        self._shadow_set("fxcm_shadow", k)

    def fxcm_shadow_report(self):
        """as FxcmVote.report (all zero unless the handle compresses)"""
        return self._shadow_report("fxcm_shadow")

    def debug_ctx_shadow_xor(self, after_chunk, instance, region, lane, index, xor_mask):
        """Test hook: one Pipeline.debug_ctx_shadow_xor between look-ahead chunk `after_chunk` and the next (include/cmix_amd.h)."""
        self._shadow_xor("ctx_shadow", (after_chunk, instance), region, (_u64(lane), int(index)), xor_mask)

    def set_journal(self, log2=19):
        """The stream journal (include/cmix_amd.h, cmx_set_journal): a compressor's handle journals every chunk on the device, a decoder's folds the p
        and bits words on the host; before the first stage_input / Predict."""
        if lib().cmx_set_journal(self.h, int(log2)):
            raise CmxError(last_error())

    def set_state_journal(self, every_chunks=1, path=None):
        """The state journal of a look-ahead compressor (include/cmix_amd.h, cmx_set_state_journal): a record after every every_chunks-th chunk to `path`."""
        if lib().cmx_set_state_journal(self.h, int(every_chunks)) or (path is not None and lib().cmx_state_journal_write_file(self.h, os.fsencode(path))):
            raise CmxError(last_error())

    def state_journal_close(self):
        if lib().cmx_state_journal_close(self.h):
            raise CmxError(last_error())

    def set_journal_check(self, path):
        """A decoder only: hold the decode to a compressor's journal (`path`, `path.inputs`); Perceive raises at the first block that differs."""
        if lib().cmx_set_journal_check(self.h, os.fsencode(path)):
            raise CmxError(last_error())

    def journal_write_files(self, path):
        if lib().cmx_journal_write_files(self.h, os.fsencode(path)):
            raise CmxError(last_error())

    def journal_close_files(self):
        if lib().cmx_journal_close_files(self.h):
            raise CmxError(last_error())

    def shadow_report(self):
        """as Vote.report (all zero unless the handle compresses)"""
        return self._shadow_report("shadow")

    def decode_stream(self, code, nbytes):
        """Decoder::Decode over a whole stream inside the library (cmx_decode_stream): the arithmetic code behind the container header -> the nbytes
        bytes the predictor saw. On a fresh handle."""
        code = np.ascontiguousarray(np.frombuffer(bytes(code), np.uint8))
        out = np.zeros(nbytes, np.uint8)
        lib().cmx_decode_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        if lib().cmx_decode_stream(self.h, code.ctypes.data if len(code) else None, len(code), out.ctypes.data if nbytes else None, nbytes):
            raise CmxError(last_error())
        return out.tobytes()

    def lstm_hint(self):
        a, b = C.c_int(0), C.c_int(0)
        if lib().cmx_get_lstm_hint(self.h, C.byref(a), C.byref(b)):
            raise CmxError(last_error())
        return a.value, b.value

    def close(self):
        if self.h:
            lib().cmx_destroy(self.h)
            self.h = None

    __del__ = close



class Fxcm(_StateDigest):
    """The fxcm stage of one stream on one GPU (chunk mode): layer-0 columns 3..433. The text parser half runs on the
    calling thread inside run(); the learned tables live on the device (include/cmix_amd.h section 2f)."""

    _sd = "fxcm"

    def __init__(self, dictionary_path=None, device=0, shadow=False):
        """shadow=True: a shadow instance (cmx_fxcm_create_shadow) -- the same device state, no parser and no dictionary; run_shared() only"""
        self.shadow = bool(shadow)
        if self.shadow:
            self.h = lib().cmx_fxcm_create_shadow(device)
        else:
            self.h = lib().cmx_fxcm_create(dictionary_path.encode() if isinstance(dictionary_path, str) else dictionary_path, device)
        if not self.h:
            raise CmxError(last_error())
        self._keep = []
        self._last = None   # (d_bytes, lstmpr, lstmex) of the most recent run(): what a shadow's run_shared reads beside the records

    def run_shared(self, owner, probs=None, stream=None):
        """A shadow's launch on the records, bytes and hints of owner's most recent run() (cmx_fxcm_run_shared): writes columns 3..433 of
        probs [8N, >=434] f32 (default: a dense [8N, 434] buffer of 0.5)."""
        import torch
        if owner._last is None:
            raise CmxError("Fxcm.run_shared: the owner has not run a chunk")
        d_bytes, lstmpr, lstmex = owner._last
        N = int(d_bytes.numel())
        dev = lstmpr.device
        if probs is None:
            probs = torch.full((8 * N, 434), 0.5, dtype=torch.float32, device=dev)
        assert probs.dtype == torch.float32 and probs.is_contiguous() and probs.shape[0] == 8 * N and probs.shape[1] >= 434
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        if lib().cmx_fxcm_run_shared(self.h, owner.h, d_bytes.data_ptr(), N, lstmpr.data_ptr(), lstmex.data_ptr(), probs.data_ptr(), probs.shape[1], C.c_void_p(stream)):
            raise CmxError(last_error())
        self._keep.append((d_bytes, lstmpr, lstmex))
        return probs

    def state_diff(self, other):
        """Every word of this handle's and `other`'s state in HBM compared (include/cmix_amd.h, cmx_fxcm_state_diff): dict words, first (region, index,
        a, b), per_region, raw. Raises when the byte counts differ. Synchronises the device."""
        out = (C.c_uint64 * 17)()
        if lib().cmx_fxcm_state_diff(self.h, other.h, out):
            raise CmxError(last_error())
        return _fxcm_state_diff(out)

    def debug_state_read(self, region, index, count):
        """Test readout: `count` words of a region from `index` on, as uint32 (cmx_fxcm_debug_state_read). Synchronises."""
        out = np.zeros(int(count), np.uint32)
        if lib().cmx_fxcm_debug_state_read(self.h, _region(region, FXCM_STATE_REGIONS), int(index), int(count), out.ctypes.data):
            raise CmxError(last_error())
        return out

    def debug_state_xor(self, region, index, xor_mask):
        """Test hook: XOR one state word (region: number or FXCM_STATE_REGIONS name) between launches; regions whose words address memory are refused."""
        if lib().cmx_fxcm_debug_state_xor(self.h, _region(region, FXCM_STATE_REGIONS), int(index), int(xor_mask)):
            raise CmxError(last_error())

    def close(self):
        if getattr(self, "h", None):
            lib().cmx_fxcm_destroy(self.h)   # (waits for the device)
            self.h = None
            self._keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def debug_set_blpos(self, blpos):
        """Test hook, before the first byte: continue as if blpos bytes of the block had been coded (device model and host parser)."""
        if lib().cmx_fxcm_debug_set_blpos(self.h, int(blpos)):
            raise CmxError(last_error())

    def failed(self):
        """True if a bounded in-launch wait of the roles kernel ran out (syncs)."""
        return bool(lib().cmx_fxcm_failed(self.h))

    def debug_jitter_counts(self):
        """Test hook (CMX_FXCM_JITTER): stalls taken since creation by role M's 16 wavefronts, role U and role X (syncs)."""
        out = (C.c_uint * 18)()
        if lib().cmx_fxcm_debug_jitter_counts(self.h, out):
            raise CmxError(last_error())
        return [int(v) for v in out]

    def debug_ring_waits(self):
        """Test hook: launches so far that waited for their staging slot's previous launch, which was still in flight."""
        return int(lib().cmx_fxcm_debug_ring_waits(self.h))

    def debug_slot_parallel(self):
        """Test hook: the model's slot_parallel word in device memory (0: one lane per map, CMX_FXCM_SERIAL_MAPS=1); syncs."""
        return int(lib().cmx_fxcm_debug_slot_parallel(self.h))

    def run(self, data_host, lstmpr, lstmex, probs=None, stream=None):
        """data_host [N] u8 numpy; lstmpr [8N] i16 cuda, lstmex [8N] u8 cuda -> writes columns 3..433 of probs [8N, >=434] f32."""
        import torch
        data_host = np.ascontiguousarray(data_host, np.uint8)
        N = int(data_host.size)
        dev = lstmpr.device
        assert lstmpr.is_cuda and lstmpr.dtype == torch.int16 and lstmpr.is_contiguous() and lstmpr.numel() == 8 * N
        assert lstmex.is_cuda and lstmex.dtype == torch.uint8 and lstmex.is_contiguous() and lstmex.numel() == 8 * N
        d_bytes = torch.from_numpy(data_host.copy()).to(dev)
        if probs is None:
            probs = torch.full((8 * N, N_INPUTS), 0.5, dtype=torch.float32, device=dev)
        assert probs.dtype == torch.float32 and probs.is_contiguous() and probs.shape[0] == 8 * N and probs.shape[1] >= 434
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib().cmx_fxcm_run(self.h, data_host.ctypes.data, d_bytes.data_ptr(), N, lstmpr.data_ptr(), lstmex.data_ptr(), probs.data_ptr(),
                                probs.shape[1], C.c_void_p(stream))
        if rc:
            raise CmxError(last_error())
        self._keep.append(d_bytes)   # the kernel reads it asynchronously: every launch's copy lives until sync() / close()
        self._last = (d_bytes, lstmpr, lstmex)
        return probs

    def sync(self):
        if lib().cmx_fxcm_sync(self.h):
            raise CmxError(last_error())
        self._keep = []


class P8Stage(_StateDigest):
    """The paq8 stage of one stream on one GPU (include/cmix_amd.h section 2f): bytes in (host), per bit the 1591 values
    PAQ8::Predict() returns out (device)."""

    _sd = "p8stage"

    def __init__(self, device=0):
        self.device = device
        self.h = lib().cmx_p8stage_create(device)
        if not self.h:
            raise CmxError(last_error())

    def run(self, data, out=None, col0=0, stream=None):
        """data: bytes-like (host). out: cuda f32 [8 n, >= col0 + 1591] (default: a fresh [8 n, 1591]); the values go to
        columns col0 .. col0 + 1590 of row t."""
        import torch
        data = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8))
        n = len(data)
        if out is None:
            out = torch.empty((8 * n, 1591), dtype=torch.float32, device="cuda:%d" % self.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] == 8 * n and out.shape[1] >= col0 + 1591
        if stream is None:
            stream = torch.cuda.current_stream(out.device).cuda_stream
        if lib().cmx_p8stage_run(self.h, data.ctypes.data, n, out.data_ptr() + 4 * col0, out.shape[1], C.c_void_p(stream)):
            raise CmxError(last_error())
        return out

    def sync(self):
        if lib().cmx_p8stage_sync(self.h):
            raise CmxError(last_error())

    def debug_state_words(self):
        """The scalar words of the role structs, device addresses zeroed: what the digest's last column covers (cmx_p8stage_debug_state_words)."""
        n = lib().cmx_p8stage_debug_state_words(self.h, None, 0)
        if n < 0:
            raise CmxError(last_error())
        out = np.zeros(max(n, 1), np.uint32)
        if lib().cmx_p8stage_debug_state_words(self.h, out.ctypes.data, len(out)) != n:
            raise CmxError(last_error())
        return out[:n]

    def debug_set_pos(self, pos):
        """Test hook (before the first byte): the front end's byte position (the index into paq8's 2^30-byte history ring)."""
        lib().cmx_p8stage_debug_set_pos.argtypes = [C.c_void_p, C.c_int]
        if lib().cmx_p8stage_debug_set_pos(self.h, int(pos)):
            raise CmxError(last_error())

    def set_generator_counter(self, counter):
        """Test hook (before the first byte): the counter of the ContextMap family's shared generator, a multiple of 64."""
        if lib().cmx_p8stage_set_generator_counter(self.h, int(counter) & 0xFFFFFFFF):
            raise CmxError(last_error())

    def close(self):
        if getattr(self, "h", None):
            lib().cmx_p8stage_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass




