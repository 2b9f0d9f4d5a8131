/* cmix_amd.h -- C ABI of libcmixamd.so, the MI355X (gfx950) per-bit prediction
 * engine for cmix v21.
 *
 * Drop-in boundary: the reference's `class Predictor`
 *   Predictor(const std::vector<bool>& vocab); float Predict();
 *   void Perceive(int bit); void Pretrain(int bit);
 * (reference src/predictor.h:17-22), whose only callers are Encoder::Encode
 * (src/coder/encoder.cpp:14-30), Decoder::Decode (src/coder/decoder.cpp:20-39),
 * preprocessor::Pretrain (src/preprocess/preprocessor.cpp:37-69) and the two
 * construction sites src/runner.cpp:205,246.  INTEGRATION.md shows the C++ shim
 * a cmix maintainer adds to bind these entry points.
 *
 * Two granularities are exported:
 *   1. the whole-predictor surface (cmx_create .. cmx_destroy), one handle per
 *      input stream, any number of handles per process (one per GPU);
 *   2. stage-level entry points (cmx_mixnet_*, cmx_lstm_*, ...) -- the device
 *      pipeline stages the predictor is assembled from.  A stage consumes and
 *      produces plain arrays, either one bit at a time (bit-synchronous: what a
 *      decoder needs, and what a hybrid build uses while some model families
 *      still run on the host) or a whole chunk of already-known bits at once
 *      (compression look-ahead: every input bit is known in advance, SURVEY.md
 *      7.1) with all operands resident in HBM.
 *
 * All functions return 0 / non-NULL on success; on failure they return
 * nonzero / NULL and cmx_last_error() describes why.  Nothing here falls back
 * to a CPU implementation: without a gfx950 device every create call fails.
 *
 * Plain C: no C++ or torch types cross this boundary.
 */
#ifndef CMIX_AMD_H
#define CMIX_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMX_N_INPUTS 2078 /* layer-0 width, SURVEY.md Appendix A.1 */
#define CMX_N_MIXERS 47   /* 26 + 20 + 1, predictor.cpp:193-356 */
#define CMX_N_MIX0 26
#define CMX_N_MIX1 20
#define CMX_AUX_MIXER 12 /* layer-0 mixer keyed by auxiliary_context_ */

const char* cmx_last_error(void);
/* Library / device identification: fills name (<=256 bytes) and returns the
 * number of visible HIP devices (0 if none; never fails). */
int cmx_device_count(void);
const char* cmx_version(void);
/* Memory helpers, so that a host program written against this header needs no HIP headers: device memory,
 * page-locked host memory, and a synchronous device-to-host copy ordered after all prior work of the device. */
void* cmx_device_alloc(int device, size_t bytes);
void cmx_device_free(int device, void* p);
void* cmx_host_alloc(size_t bytes);
void cmx_host_free(void* p);
int cmx_copy_to_host(int device, void* dst, const void* d_src, size_t bytes);

/* ------------------------------------------------------------------------
 * 1. Whole-predictor surface (replaces class Predictor, predictor.h:17-22)
 * ------------------------------------------------------------------------ */
typedef struct cmx_engine cmx_t;
/* vocab[i] != 0 iff byte value i occurs in the (preprocessed) input
 * (runner.cpp:196-202). dict_path replaces the global `dictionary_path`
 * (runner.cpp:17) read by fxcm; may be NULL. */
cmx_t* cmx_create(const uint8_t vocab[256], const char* dict_path, int device);   /* checks the device; stages are built on first use */
float cmx_predict(cmx_t*);             /* Predictor::Predict,  predictor.cpp:361; < 0 on error */
int cmx_perceive(cmx_t*, int bit);     /* Predictor::Perceive, predictor.cpp:421 */
int cmx_pretrain(cmx_t*, int bit);     /* Predictor::Pretrain, predictor.cpp:471 */
/* Decoder::Decode (coder/decoder.cpp:20-39) + the Decompress loop (runner.cpp:214-246) over a whole stream inside the library: `code` = the arithmetic code behind
 * the container header, nbytes = the stream's length from that header, out[nbytes] = the bytes the predictor saw (the preprocessed stream; the caller runs the
 * reference's preprocessor::Decode over them). Call on a fresh handle (after cmx_pretrain, if there is a dictionary). Equivalent to nbytes x 8 rounds of
 * cmx_predict / cmx_decoder_decode / cmx_perceive; the reference's own decoder.cpp over the ABI remains the parity path (integration/predictor_dropin.h). */
int cmx_decode_stream(cmx_t*, const uint8_t* code, size_t code_len, uint8_t* out, size_t nbytes);
/* TEST HOOK (the third mode of a handle; rounds 1-3 decoded this way): fxcm and paq8 have been device stages since round 2 -- a compressor (cmx_stage_input)
 * and a decoder (cmx_predict without staged input) take no column from the caller. A handle that is given columns BEFORE its first cmx_predict() runs the
 * per-bit stages instead and takes the two families' outputs of every bit from the caller -- layer-0 columns 3..2024 in the reference's order (431 fxcm values,
 * then 1591 paq8 values; predictor.cpp:363-369) -- which is how tests/test_gpu_predictor.py isolates the other stages. cmx_predict() fails loudly when the
 * columns of a bit are missing: nothing is computed on the CPU in their place. */
int cmx_set_model_outputs(cmx_t*, const float cols_3_to_2024[2022]);
/* The hidden globals `lstmpr`, `lstmex` (predictor.cpp:359,462-465) as they stand after the last cmx_perceive():
 * what the caller's fxcm reads in its own Perceive. cmx_perceive() only enqueues the device work; this call (or the
 * next cmx_predict()) waits for it, so host work placed between the two overlaps the device. */
int cmx_get_lstm_hint(cmx_t*, int* lstmpr, int* lstmex);
/* Introspection used by the parity tests: the 2078 layer-0 inputs of the last cmx_predict() (valid until the next). */
const float* cmx_debug_last_row(cmx_t*);
/* Look-ahead for compression: the next n bytes the caller is going to code, in order; may be called
 * repeatedly (bytes are appended); n == 0 marks the end of the input (the ragged last chunk is then submitted at once).
 * The first call must precede the first cmx_predict() and puts the handle in LOOK-AHEAD MODE: it builds the chunk
 * pipeline (cmx_pipeline_*: every model family a device stage, fxcm and paq8 included -- no cmx_set_model_outputs),
 * trains it on the bytes cmx_pretrain() has collected, and keeps CMX_PIPELINE_SLOTS chunks of 4 KB in flight.
 * cmx_predict() then pops the next probability of the chunk that has left the mixing network (same float the per-bit
 * surface would return) and cmx_perceive(bit) checks the bit against the staged one -- a mismatch is an error, the
 * device has already learnt the staged bit. With it the reference's unmodified Encoder (encoder.cpp:14-30) and
 * Compress loop (runner.cpp:101-119) run at the pipeline's speed: integration/predictor_dropin.h.
 * Without it the handle builds the per-bit stages on first use (what a Decoder needs). */
int cmx_stage_input(cmx_t*, const uint8_t* bytes, size_t n);
/* 0 = undecided (nothing built yet), 1 = per-bit stages, 2 = look-ahead pipeline; *chunks_in_flight (may be NULL). */
int cmx_mode(cmx_t*, int* chunks_in_flight);
/* Verify mode of the look-ahead pipeline's mixing network (cmx_pipeline_set_verify): before the first cmx_stage_input. cmx_predict then
 * returns < 0 (cmx_last_error names the chunk, the stream bit and the kind of input) instead of a probability of a chunk in which a consumed word
 * differs from its source; a compression either ends with every word the final network consumed checked or stops. A handle that decodes is
 * not covered (the decoder's form of the network has no verify instantiation): its report stays at zero chunks. The programs in integration/
 * switch it on with CMIX_VERIFY=1; the library reads no environment variable for it. cmx_verify_report: as cmx_mixnet_verify_report. */
int cmx_set_verify(cmx_t*, int on);
int cmx_verify_report(cmx_t*, uint64_t out[8]);
/* Shadow mixing networks of the look-ahead pipeline (cmx_pipeline_set_shadow, k = 0 / 1 / 2): before the first cmx_stage_input or cmx_predict.
 * cmx_predict then returns < 0 instead of a probability of a chunk in which the instances disagreed. A handle that decodes is not covered: its
 * report stays at zero chunks. The programs in integration/ read CMIX_SHADOW=1|2; the library reads no environment variable for it.
 * cmx_shadow_report: as cmx_vote_report.
 * cmx_set_shadow_repair(max_repairs): repair on the majority (cmx_pipeline_set_shadow_repair, which states what a repaired stream guarantees);
 * 0 = off, the default; > 0 after cmx_set_shadow(h, 2) only. cmx_shadow_repairs: as cmx_pipeline_shadow_repairs (two zero words before the
 * pipeline exists). The programs in integration/ read CMIX_SHADOW_REPAIR=N (with CMIX_SHADOW=2 only) and print one line per repair at the end.
 * TEST HOOK cmx_debug_shadow_xor: arms ONE cmx_pipeline_debug_shadow_xor(instance, region, mixer, row, index, xor_mask), made between chunk
 * `after_chunk` and the next one of the look-ahead stream (chunks of 4096 bytes, 0 = the first). */
int cmx_set_shadow(cmx_t*, int k);
int cmx_shadow_report(cmx_t*, uint64_t out[8]);
int cmx_set_shadow_repair(cmx_t*, int max_repairs);
int cmx_shadow_repairs(cmx_t*, uint64_t out[], size_t cap);
int cmx_debug_shadow_xor(cmx_t*, uint64_t after_chunk, int instance, int region, uint64_t mixer, uint64_t row, uint64_t index, uint32_t xor_mask);
/* Shadow context stages of the look-ahead pipeline (cmx_pipeline_set_ctx_shadow, k = 0 / 1 / 2): before the first cmx_stage_input or cmx_predict.
 * cmx_predict then returns < 0 instead of a probability of a chunk in which the context-stage instances disagreed. A handle that decodes is not
 * covered. The programs in integration/ read CMIX_CTX_SHADOW=1|2; the library reads no environment variable for it. cmx_ctx_shadow_report: as
 * cmx_ctxvote_report. TEST HOOK cmx_debug_ctx_shadow_xor: arms ONE cmx_pipeline_debug_ctx_shadow_xor(instance, region, lane, index, xor_mask), made
 * between chunk `after_chunk` and the next one of the look-ahead stream. */
int cmx_set_ctx_shadow(cmx_t*, int k);
int cmx_ctx_shadow_report(cmx_t*, uint64_t out[8]);
int cmx_debug_ctx_shadow_xor(cmx_t*, uint64_t after_chunk, int instance, int region, uint64_t lane, uint64_t index, uint32_t xor_mask);
/* Shadow LSTM stages of the look-ahead pipeline (cmx_pipeline_set_lstm_shadow, k = 0 / 1 / 2): before the first cmx_stage_input or cmx_predict.
 * cmx_predict then returns < 0 instead of a probability of a chunk in which the LSTM instances disagreed. A handle that decodes is not covered. The
 * programs in integration/ read CMIX_LSTM_SHADOW=1|2; the library reads no environment variable for it. cmx_lstm_shadow_report: as
 * cmx_lstmvote_report. */
int cmx_set_lstm_shadow(cmx_t*, int k);
int cmx_lstm_shadow_report(cmx_t*, uint64_t out[8]);
/* Shadow fxcm stages of the look-ahead pipeline (cmx_pipeline_set_fxcm_shadow, k = 0 / 1 / 2): before the first cmx_stage_input or cmx_predict; they
 * are set before the dictionary is pretrained, so every instance learns it. A disagreement fails the call that waits for that chunk. The programs in
 * integration/ read CMIX_FXCM_SHADOW=1|2; the library reads no environment variable for it. cmx_fxcm_shadow_report: as cmx_fxcmvote_report. */
int cmx_set_fxcm_shadow(cmx_t*, int k);
int cmx_fxcm_shadow_report(cmx_t*, uint64_t out[8]);
/* The stream journal of a cmx_t (section "Stream journal" below has the digest; log2_block_bits 0 = off, else 6..19, 19 = the reference trace's 64 KB;
 * before the first cmx_stage_input / cmx_predict). A COMPRESSOR's handle (look-ahead mode) journals every chunk on the device
 * (cmx_pipeline_set_journal: all 179 words per block; coexists with verify, the shadows and repair). A DECODER's handle (late-bit mode)
 * folds the p and bits words on the calling thread, in cmx_perceive, from the p it returned and the bit it was given: no decoder kernel is involved, and
 * its records hold zeros for the column groups and the selectors. COVERS what the final mixing network read and wrote per chunk (rows, selectors, bits,
 * p) as they lay in device memory behind its kernel; DOES NOT COVER the network's own state, the stages' tables, pretraining, or the container's bytes.
 * cmx_journal_write_files appends every block completed since the last call to `path` ("<end byte> <131 hex words>": 130 column groups, p -- the form
 * oracle/ref_long_trace.cpp writes and takes as its fourth argument) and `path.inputs` ("<end byte> <48 hex words>": 47 selectors, bits), and flushes
 * them; the first call creates or empties the files; call it as often as wanted (the programs in integration/ do every MiB), a killed run leaves the
 * blocks written so far. cmx_journal_close_files writes the rest, the partial last block included, and -- with a journal to check against -- compares
 * that last block and the number of blocks.
 * cmx_set_journal_check (a decoder only): reads a compressor's `path` and `path.inputs`; the block size comes from the file's positions. cmx_perceive
 * then compares the p and bits words at the end of every block and FAILS on the first difference -- cmx_last_error names the block, its byte range and
 * which of the two words differs -- before the block's last byte has been handed to the caller; the handle is void from there.
 * cmx_journal_close_files without a journal does nothing and succeeds.
 * ENVIRONMENT: cmx_create itself reads CMIX_JOURNAL=path, CMIX_JOURNAL_LOG2=k (default 19) and CMIX_JOURNAL_CHECK=path (a decoder) -- the one switch the
 * library takes from the environment, so that a journal can be had from any program over a cmx_t as it is deployed, whichever shim it was compiled
 * against. It makes the cmx_set_journal / cmx_set_journal_check call (a file that cannot be read fails cmx_create), cmx_perceive then writes the
 * completed blocks to `path` every MiB, and cmx_destroy closes the files if the program did not (a difference found only there -- a checked decode's
 * partial last block, the block count -- can only be printed to stderr, so a program that wants it as an error calls cmx_journal_close_files first,
 * as integration/predictor_dropin.h does). With none of the three set nothing changes. */
int cmx_set_journal(cmx_t*, int log2_block_bits);
/* The STATE JOURNAL of a cmx_t (section "State digest" below; cmx_pipeline_set_state_journal has the record and the file's form): a compressor's handle
 * in look-ahead mode (cmx_stage_input) takes one record of every device stage's state digests after every every_chunks-th chunk of 4096 bytes and after
 * the last (0 = off, the default; before the first cmx_stage_input / cmx_predict). _write_file names the file the records go to as they are taken;
 * _close (cmx_destroy makes the call if the program has not) writes the record after the last chunk. A handle that takes its columns from the caller
 * has no pipeline and takes no records. A DECODER is not covered: cmx_predict fails with a message if the switch was set by cmx_set_state_journal.
 * ENVIRONMENT: cmx_create reads CMIX_STATE_JOURNAL=path [CMIX_STATE_JOURNAL_EVERY=n, default CMX_STATE_JOURNAL_EVERY] where it reads CMIX_JOURNAL; it
 * is a file of its own (`path` and `path.inputs` of the stream journal keep their form). A decoder created under it says on stderr that it is not
 * covered and decodes as before. */
#define CMX_STATE_JOURNAL_EVERY 256   /* chunks of 4096 bytes: a record per MiB, the smallest measured period with no cost resolved per stream (profiles/r21_state_journal.txt) */
int cmx_set_state_journal(cmx_t*, int every_chunks);
int cmx_state_journal_write_file(cmx_t*, const char* path);
int cmx_state_journal_close(cmx_t*);
int cmx_set_journal_check(cmx_t*, const char* path);
int cmx_journal_write_files(cmx_t*, const char* path);
int cmx_journal_close_files(cmx_t*);
void cmx_destroy(cmx_t*);

/* ------------------------------------------------------------------------
 * 2a. Stage: final mixing network = MixerInput stretch -> 26+20+1 gated
 *     logistic mixers -> squash -> SSE  (predictor.cpp:388-418,432-437;
 *     src/mixer/{mixer,mixer-input,sigmoid,sse}.cpp)
 * ------------------------------------------------------------------------ */
typedef struct cmx_mixnet cmx_mixnet_t;
cmx_mixnet_t* cmx_mixnet_create(int device);
void cmx_mixnet_destroy(cmx_mixnet_t*);

/* The stream the handle's host-to-device copies (the decay schedule of a chunk) go on; NULL-less default: a stream the handle
 * creates. A copy must never sit behind a long kernel in stream order: on this hardware it then holds up later copies of the
 * whole process. cmx_pipeline_* hands ONE upload stream to all its stages. Same for cmx_fxcm_* (records) and cmx_p8stage_*. */
/* Tolerance mode of the 27-workgroup kernel (NOT bit-exact: layer-0 dot products as f64 tree sums rounded once). An explicit
 * switch of the handle, before its first bit -- never an environment variable: a stream coded with it is not the reference's
 * and cannot be decoded by this library's (strict) decoder. cmx_mixnet_mode: 0 strict (default), 1 tolerance. */
int cmx_mixnet_set_tolerance(cmx_mixnet_t*, int on);
const int* cmx_mixnet_error_flag(cmx_mixnet_t*);   /* DEVICE address of the sticky "an in-launch wait ran out" word (see cmx_lstm_fail_flag) */
int cmx_mixnet_mode(cmx_mixnet_t*);
int cmx_mixnet_set_upload_stream(cmx_mixnet_t*, void* stream);
/* Chunk mode. All pointers are DEVICE pointers (HBM-resident operands):
 *   d_probs [nbits][2078] f32  raw model outputs (Model::Predict values)
 *   d_sel   [nbits][47]   u32  each mixer's selector key (its 64-bit context
 *                              truncated to 32 bits exactly as the reference's
 *                              unordered_map<unsigned int,...> key does,
 *                              mixer.h:33); entry 12 is ignored (derived on
 *                              device from the inputs, predictor.cpp:388-393)
 *   d_bits  [nbits]       u8   the coded bits
 *   d_p_out [nbits]       f32  OUT: value Predictor::Predict() returns
 *   d_mix_out [nbits][47] f32  OUT (may be NULL): every Mixer::p_
 * Processes the bits strictly in order inside one persistent kernel launch on
 * `stream` (a hipStream_t passed as void*, NULL = default stream) and returns
 * without synchronising. Every chunk of a handle must be enqueued on the SAME stream (the chunks train one state in order
 * and share one staging buffer); a call with a different stream is refused. */
int cmx_mixnet_run(cmx_mixnet_t*, const float* d_probs, const uint32_t* d_sel,
                   const uint8_t* d_bits, size_t nbits, float* d_p_out, float* d_mix_out,
                   void* stream);

/* Bit-synchronous mode. HOST pointers; synchronous. predict() may be followed
 * only by perceive() (same protocol as the reference). */
float cmx_mixnet_predict(cmx_mixnet_t*, const float* probs2078, const uint32_t* sel47);
int cmx_mixnet_perceive(cmx_mixnet_t*, int bit);

/* Bit-synchronous mode with DEVICE operands, asynchronous on `stream`: the same kernel and protocol without the
 * host round trips. The operands must stay untouched until the matching perceive has run; *d_p receives the
 * probability. */
int cmx_mixnet_predict_async(cmx_mixnet_t*, const float* d_probs2078, const uint32_t* d_sel47, float* d_p, void* stream);
int cmx_mixnet_perceive_async(cmx_mixnet_t*, int bit, void* stream);

/* Waits for all work of this handle and reports device-side failures (a bounded
 * in-kernel wait that timed out). */
int cmx_mixnet_sync(cmx_mixnet_t*);

/* Introspection used by the parity tests. */
int cmx_mixnet_bits_done(const cmx_mixnet_t*, uint64_t* out);
/* Phase timers: enable != 0 turns on in-kernel shader-clock accumulation for the
 * following chunks; out16 (may be NULL) receives the 16 accumulators gathered
 * since the previous call, which are then cleared. Synchronises the device. */
int cmx_mixnet_profile(cmx_mixnet_t*, int enable, uint64_t* out16);
/* Elapsed device time (ms, HIP events on the launch stream) of the last
 * cmx_mixnet_run kernel; synchronises with it. */
int cmx_mixnet_last_kernel_ms(cmx_mixnet_t*, float* ms);
/* Chunk mode runs cmx_mixnet_spec_kernel: 26 helper workgroups cut each layer-0 mixer's ordered 2078-term sum into four segments
 * that run at once, segments 1..3 speculatively from 64 candidate start values (exact: the lane whose candidate equals the true
 * start holds the reference's result, otherwise the segment is re-run). Statistics since creation: out[0] speculative segments,
 * [1] resolved from a candidate, [2..4] re-runs of segment 1 / 2 / 3. Synchronises the device. */
int cmx_mixnet_spec_stats(cmx_mixnet_t*, uint64_t out[5]);
/* How the re-runs were executed. A re-run is itself split in two halves inside its wave: lane 0 runs the segment's first 256 terms from
 * the true start, lanes 1..63 the rest from 63 candidate mid-points. out[0] re-runs resolved from a mid-point candidate, [1] re-runs
 * whose second half ran serially from the true mid-point; out[0] + out[1] == the three re-run counts of cmx_mixnet_spec_stats.
 * Synchronises the device. */
int cmx_mixnet_spec_rerun_stats(cmx_mixnet_t*, uint64_t out[2]);
/* Test hook (state injection): the network as after `steps` bits of a stream -- Mixer::steps_ (mixer.cpp:58,61) of all 47 mixers. The wrap / threshold
 * fixtures of tests/golden/make_wrap_traces.py place the reference's counters the same way (oracle/ref_harness.cpp). Between chunks only. */
int cmx_mixnet_debug_set_steps(cmx_mixnet_t*, uint64_t steps);
/* VERIFY MODE (opt-in; off by default, and then nothing of it is allocated or launched). Before the first bit, like cmx_mixnet_set_tolerance;
 * refused together with tolerance mode and on a handle that runs the decoder's (late) kernel, and chunks only (the bit-synchronous calls are
 * refused). Every chunk then runs cmx_mixnet_spec_verify_kernel -- the same roles and results as cmx_mixnet_spec_kernel, each also folding the
 * words it loaded into 64-bit block sums (src/cmx_verify.h: a splitmix64-style mix of (class, bit, index, word), summed mod 2^64 over blocks of
 * 64 bits) -- and, behind it on the same stream, cmx_mixnet_verify_kernel, which recomputes every block sum from the buffers in HBM: the raw
 * inputs, the coded bits, the selectors, the decay schedule (as the gather and both tail waves loaded it) and the stretched inputs the in-launch
 * ring carried (as the stretch waves stored them and as each helper loaded its slice). The helpers also store a digest with every layer-0 row
 * segment they write back (words 0..2077; a ~8 MB table of the handle) and check it when they load the segment again. A mismatch changes no
 * result and no control flow: it is counted in a sticky record, cmx_mixnet_sync fails naming it, cmx_pipeline_wait fails the chunk.
 * cmx_mixnet_verify_report: out[0] chunks verified, [1] bits verified, [2] mismatches (blocks x class, x helper for the ring read, or row
 * segments), then of the first one: [3] class (1 layer-0 row, 2 coded bit, 3 selectors, 4/5/6 decay as the gather / tail-a / tail-b wave
 * loaded it, 7 ring written, 8 ring read, 9 row segment), [4] its block's first stream bit, [5] mixer (ring read, row segment), [6] row,
 * [7] segment (row segment); UINT64_MAX where a field does not apply. Synchronises the device. */
int cmx_mixnet_set_verify(cmx_mixnet_t*, int on);
int cmx_mixnet_verify_on(cmx_mixnet_t*);
int cmx_mixnet_verify_report(cmx_mixnet_t*, uint64_t out[8]);
const unsigned long long* cmx_mixnet_verify_record(cmx_mixnet_t*);   /* DEVICE address of the 8 report words (NULL before verify mode was first on) */
/* TEST HOOK of verify mode: one perturbation for the next chunk, a data mismatch reported as an error return (no kernel stops early, no wait
 * times out). cls 1 / 2 / 3 / 4..6 (layer-0 row, coded bit, selectors, decay): word `index` of chunk bit `bit` of the caller's buffer (of the
 * handle's decay schedule) is XORed with xor_mask between the network kernel and the verify kernel, and back after it; cls 7 / 8 (ring): the
 * stretch wave stores stretched input `index` of chunk bit `bit` XOR xor_mask and folds the value it computed; cls 9 (row segment): `bit` =
 * mixer * 10001 + row, weight `index` (< 2078) of that layer-0 row is XORed before the next kernel. */
int cmx_mixnet_debug_verify_perturb(cmx_mixnet_t*, int cls, uint64_t bit, uint64_t index, uint32_t xor_mask);

/* THE REDUNDANT VOTE (opt-in; src/mixnet_vote.hip). Verify mode checks what the network LOADS from HBM; what it computes with it -- the main
 * workgroup's LDS, the layer-1 / layer-2 rows, the extras, row_steps, the SSE cells -- is covered by running the unchanged kernel on n = 2 or 3
 * handles over the same inputs and comparing what they produce. A vote handle compares, per chunk, the n instances' final p ([nbits] f32) and mixer
 * outputs ([nbits][47] f32) as 32-bit WORDS, never as floats: -0.0 differs from 0.0, equal NaN patterns are equal. Instance 0 is the stream's own
 * network. Elements are ordered by e = t * 48 + c, c = 0..46 the mixer, c = 47 the final p (the causal order within a bit). n = 3: all equal agree;
 * exactly two equal make the third the ODD instance; all different is NO MAJORITY. n = 2: different is no majority.
 * cmx_vote_run is asynchronous on `stream` (a hipStream_t as void*): one grid-stride kernel (16-byte loads where all arrays are 16-byte aligned) and
 * a one-wave kernel behind it that folds the chunk into the sticky DEVICE record and, for the first event, captures the bit. d_sel ([nbits][47]) and
 * d_bits ([nbits]) are the chunk's selectors and coded bits (either may be NULL: captured as 0).
 * The record (cmx_vote_report synchronises; cmx_vote_record is its DEVICE address, as cmx_mixnet_verify_record): [0] chunks voted, [1] bits voted,
 * [2] n, [3] chunks with at least one non-agreeing element, then of the FIRST such chunk: [4] stream bit (stream_bit0 + t) of its smallest
 * non-agreeing e, [5] the column c there, [6] the odd instance there or UINT64_MAX for no majority, [7] non-agreeing elements in that chunk.
 * cmx_vote_values: the capture of that bit -- words[i * 48 + c] of instance i (n x 48 used), its 47 selectors, the coded bit. Synchronises.
 * cmx_vote_last: the result of the chunk voted LAST alone (synchronises; on the device it lies right behind the record: cmx_vote_record + 8):
 * [0] its non-agreeing elements (0: the instances agreed, [1..3] are 0), [1] the stream bit and [2] the column of the first of them, [3] the
 * chunk's odd instance -- the one instance that was odd at every non-agreeing element -- or UINT64_MAX for no majority (an element at which all
 * differ, n = 2, or elements with different odd instances).
 * Continuing on the majority after an event is cmx_pipeline_set_shadow_repair's; out of scope: the decoder's form of the network. */
typedef struct cmx_vote cmx_vote_t;
cmx_vote_t* cmx_vote_create(int device, int n);
void cmx_vote_destroy(cmx_vote_t*);
int cmx_vote_run(cmx_vote_t*, const float* const* d_p, const float* const* d_mix, size_t nbits, uint64_t stream_bit0, const uint32_t* d_sel,
                 const uint8_t* d_bits, void* stream);
int cmx_vote_report(cmx_vote_t*, uint64_t out[8]);
const unsigned long long* cmx_vote_record(cmx_vote_t*);
int cmx_vote_values(cmx_vote_t*, uint32_t words[144], uint32_t sel[47], uint32_t* bit);
int cmx_vote_last(cmx_vote_t*, uint64_t out[4]);
/* Every 32-bit word of two handles' state in HBM, compared (both handles on one device; synchronises it; reads ~5.6 GB: after an event and in
 * tests, never per chunk). Regions in order: 0 rows0 [26][10001][2112], 1 rows1 [20][10001][64], 2 rows2 [10001][64], 3 row_steps [47][10001] (two
 * words each), 4 map_keys [47][32768], 5 map_vals, 6 s6, 7 s7, 8 x1, 9 x2, 10 the scalars n_rows[48], max_steps[48], steps, sse_j, sse_pc, sse_ffl.
 * out[0] differing words; [1..6] the first difference in region-then-address order: region, mixer, row, word index within the row (or table),
 * the word of a, the word of b (UINT64_MAX where a field does not apply); [7..17] the count per region; [18] bit m set: layer-0 mixer m has a
 * differing row word; [19] the same for the layer-1 and layer-2 mixers, bit m - 26. A mixer reads its layer's inputs and the outputs of the
 * mixers BEFORE it in its layer (predictor.cpp:395-412), and its update depends on its own output alone: an origin in mixer m leaves every mixer
 * before m in its layer identical, and an origin in layer 1 or 2 leaves all of layer 0 identical. The lowest set bit of the two masks names
 * the origin even a chunk after the event. */
int cmx_mixnet_state_diff(cmx_mixnet_t* a, cmx_mixnet_t* b, uint64_t out[20]);
/* The same walk that REPAIRS: wherever a state word of dst differs from src's, src's word is stored over it (only those words are stored: the pass
 * stays read-bound, and src is never written); the differing scalars of region 10 likewise, inside dst's device block. out[20] has exactly
 * cmx_mixnet_state_diff(dst, src)'s layout and describes the state BEFORE the repair -- one pass diagnoses and repairs; afterwards
 * cmx_mixnet_state_diff(dst, src) reports zero. If dst is in verify mode, the stored digests of the layer-0 row segments that received a word are
 * recomputed from the repaired rows (they are no state region; a stale one would raise a false alarm at the row's next reload). Between chunks
 * only; synchronises the device. Refuses dst == src and handles on different devices. */
int cmx_mixnet_state_repair(cmx_mixnet_t* dst, cmx_mixnet_t* src, uint64_t out[20]);
/* TEST HOOK: XOR one state word (addressed as cmx_mixnet_state_diff reports it) between chunks. Synchronises the device. A data change only: no
 * kernel stops and no wait times out. */
int cmx_mixnet_debug_state_xor(cmx_mixnet_t*, int region, uint64_t mixer, uint64_t row, uint64_t index, uint32_t xor_mask);

/* ------------------------------------------------------------------------
 * 2b. Stage: byte-level LSTM byte mixer = ByteMixer + Lstm + LstmLayer + its ByteModel bit
 *     interface (src/mixer/{byte-mixer,lstm,lstm-layer}.cpp, src/models/byte-model.cpp;
 *     wired at predictor.cpp:189-191,378-387,450-467)
 * ------------------------------------------------------------------------ */
typedef struct cmx_lstm cmx_lstm_t;
/* vocab as for cmx_create. skip_rand = number of rand() values the reference consumes after
 * srand(0xDEADBEEF) before it constructs the LSTM (31 in Predictor::Predictor: one per Indirect
 * model, indirect.cpp:10); the weights are then drawn exactly as lstm-layer.cpp:52-59 does. */
cmx_lstm_t* cmx_lstm_create(const uint8_t vocab[256], int skip_rand, int device);
void cmx_lstm_destroy(cmx_lstm_t*);
int cmx_lstm_vocab_size(const cmx_lstm_t*);
/* Chunk mode over nbytes already-known bytes. DEVICE pointers:
 *   d_in_probs  [nbytes][256] f32  the byte model's (PPMd) distribution after each byte
 *                                  (ByteModel::BytePredict, predictor.cpp:450-457)
 *   d_bytes     [nbytes]      u8   the bytes coded
 *   d_out_probs [nbytes][256] f32  OUT: the LSTM's distribution after each byte (ByteMixer::probs_)
 *   d_bit_p     [nbytes][8]   f32  OUT (may be NULL): ByteModel::Predict value for each bit of byte n,
 *                                  i.e. layer-0 input 2077 (for n = 0: from the state before this call);
 *                                  bit k of byte n goes to d_bit_p[(8n+k)*bit_p_stride] -- stride 1 for a
 *                                  dense array, 2078 to write column 2077 of the layer-0 matrix in place
 *   d_bit_ex    [nbytes][8]   i32  OUT (may be NULL): ByteModel::ex per bit (-> lstmex, predictor.cpp:465)
 * Asynchronous on `stream`. Truncated BPTT + Adam run every 100 bytes as in lstm.cpp:93-110. */
int cmx_lstm_run(cmx_lstm_t*, const float* d_in_probs, const uint8_t* d_bytes, size_t nbytes,
                 float* d_out_probs, float* d_bit_p, size_t bit_p_stride, int* d_bit_ex, void* stream);
/* ByteModel::Predict/Perceive for any byte model (PPMd, Bracket, LSTM): per-bit predictions along
 * the known bytes. dist for byte 0 = d_dist0[256]; for byte n >= 1 = d_dist_rest[(n-1)*256 ...]. */
int cmx_bytemodel_bits_run(int device, const float* d_dist0, const float* d_dist_rest,
                           const uint8_t* d_bytes, size_t nbytes, float* d_bit_p, size_t bit_p_stride,
                           int* d_bit_ex, void* stream);
/* Bit-synchronous mode: ByteModel::Predict for bit k (0..7) of the byte whose top k bits (in *d_byte) are the coded
 * ones: d_bit_p[k * stride] and *d_p_copy (may be NULL) receive the value, d_bit_ex[k] (may be NULL) `ex`. */
int cmx_bytemodel_bit_run(int device, const float* d_dist, const uint8_t* d_byte, int k, float* d_bit_p,
                          size_t bit_p_stride, int* d_bit_ex, float* d_p_copy, void* stream);
/* Test hooks. */
int cmx_lstm_get_gate_weights(cmx_lstm_t*, int layer, int gate, float* out_host);
int cmx_lstm_gate_rowlen(const cmx_lstm_t*, int layer);
/* 1 if a bounded in-launch wait of the multi-workgroup kernels (lstm_block.hip) ran out -- the stream's LSTM output
 * is void from that point --, 0 otherwise. Synchronises the device. */
int cmx_lstm_failed(cmx_lstm_t*);
/* TOLERANCE mode (NOT bit-exact, measurement only): the BPTT round's weight-update contraction (200 x rowlen x 100 per gate,
 * reference src/mixer/lstm-layer.cpp:182-186) as v_mfma_f32_16x16x4_f32 tiles instead of the ordered, separately rounded chain */
int cmx_lstm_set_tolerance(cmx_lstm_t*, int on);
/* DEVICE address of the sticky flag cmx_lstm_failed reads (4 bytes): copy it back in stream order behind the stage's
 * kernels to learn of a timed-out hand-off without synchronising the device. */
const unsigned* cmx_lstm_fail_flag(cmx_lstm_t*);
int cmx_glibc_rand_selftest(uint32_t seed, int n, int* out);
/* THE REDUNDANT LSTM-STAGE VOTE (opt-in; src/lstm_vote.hip). This stage writes layer-0 column 2077 and, through lstmpr / lstmex, steers fxcm's mixer
 * selection and APMs; its state learns online, and its block kernels hand values between 52 workgroups inside a launch. Verify mode, the network's vote
 * and the context vote take its column as given. The complementary guard runs the unchanged cmx_lstm_run on n = 2 or 3 handles over the same bytes and
 * the same PPMd distributions and compares what they wrote. A chunk of nbytes has nbytes rows; per row (byte b) and instance 272 values are compared as
 * 32-bit WORDS, never as floats (-0.0 differs from 0.0, equal NaN patterns are equal). Elements are ordered by e = b * 272 + c: c = 0..255 the
 * distribution after byte b (d_out_probs[b][c]; entries outside the vocabulary are written as 0 and compared too), c = 256..263 the ByteModel::Predict
 * value of the byte's bit c - 256 (layer-0 column 2077 of row 8 b + c - 256), c = 264..271 `ex` of the byte's bit c - 264. The rule is cmx_vote_run's:
 * n = 3: all equal agree, exactly two equal make the third the ODD instance, all different is NO MAJORITY; n = 2: different is no majority.
 * cmx_lstmvote_run is asynchronous on `stream`: per instance i the DEVICE arrays d_dist[i] [nbytes][256], d_bit_p[i] with bit k of byte b at
 * [(8 b + k) * pstride[i]] (pstride 1 = a dense [nbytes][8] array; 2078 with d_bit_p = layer0 + 2077 = read in place from the slot's layer-0 rows:
 * instance 0 is the stream's own stage) and d_bit_ex[i] [nbytes][8]. 4-byte loads only: nothing is assumed about alignment. d_bytes ([nbytes], may be
 * NULL: captured as 0) are the chunk's bytes. One kernel with one wavefront per row (grid-stride) and a one-wave kernel behind it that folds the chunk
 * into the sticky DEVICE record.
 * _report / _record / _last: exactly the eight / four words of cmx_vote_report / _record / _last with BYTES where those have bits: [1] bytes voted,
 * [4] (of _last: [1]) the stream byte of the first event, [5] (of _last: [2]) the element's c; "first" = lowest byte, then lowest element.
 * cmx_lstmvote_values: the capture of the first event's row -- words[i * 272 + c] of instance i (n x 272 used) and the byte coded. Synchronises.
 * NO REPAIR: by the time the host sees a vote, fxcm and the final network have consumed what the LSTM wrote on the device; correcting it would mean
 * running those stages again. An event stops the stream. Out of scope as well: the slot's other producers (fxcm, paq8, PPMd), PPMd's distributions
 * and the bytes (every instance reads the same), the decoder's form of the stage. */
#define CMX_LSTMVOTE_COLS 272
typedef struct cmx_lstmvote cmx_lstmvote_t;
cmx_lstmvote_t* cmx_lstmvote_create(int device, int n);
void cmx_lstmvote_destroy(cmx_lstmvote_t*);
int cmx_lstmvote_run(cmx_lstmvote_t*, const float* const* d_dist, const float* const* d_bit_p, const size_t* pstride, const int* const* d_bit_ex, size_t nbytes,
                     uint64_t stream_byte0, const uint8_t* d_bytes, void* stream);
int cmx_lstmvote_report(cmx_lstmvote_t*, uint64_t out[8]);
const unsigned long long* cmx_lstmvote_record(cmx_lstmvote_t*);
int cmx_lstmvote_values(cmx_lstmvote_t*, uint32_t words[3 * CMX_LSTMVOTE_COLS], uint32_t* byte);
int cmx_lstmvote_last(cmx_lstmvote_t*, uint64_t out[4]);
/* Every 32-bit word of two handles' state in HBM, compared (both on one device, same vocabulary size; a == b is refused; synchronises; tens of MB per
 * handle: after an event and in tests, between chunks only). Regions and, inside a region, the arrays in this order (l = layer 0, 1 outside, g = gate
 * 0 forget, 1 input node, 2 output inside; an index is a word offset into the region's arrays laid end to end):
 *   0 W           W[l][g]           [200][rowlen_l]
 *   1 WT          WT[l][g]          the transposed copies (their tail layout depends on insz_l % 4)
 *   2 M           M[l][g]           Adam's first moments
 *   3 Vv          Vv[l][g]          Adam's second moments
 *   4 gb          gb[l][g]          [8][200]: gamma, beta and their moments and updates (index 0 = gamma of layer 0's forget gate, cell 0); then adam_tab
 *   5 caches      norm[l][g], gstate[l][g], ivar[l][g], E[l][g], then last_state[l], tanh_state[l], in_gate_state[l]: the per-step caches of the horizon
 *   6 recurrent   stateb[0][l] (= state[l]), stateb[1][l], hid[0], hid[1]
 *   7 layer_input layer_input[l]    [100][insz_l]
 *   8 output_layer OL [100][V][401], output [100][256]
 *   9 indices     input_history [100], bp_symbol [100], dyn [4]
 *  10 probs_rings byte_probs [256], the handle's d_prev_probs [256], then the in-launch rings raw_ring, h_ring, logit_ring, bp_pub
 * NOT compared: `sync` (hand-off counters, zeroed ahead of every launch), `blk` (device addresses), `raw` and `logits` (allocated, but no kernel has
 * read or written them since the block kernels replaced the per-byte ones), `OLT` (null). Every other array -- the rings included: each entry has one
 * writer and a fixed summation order -- is a function of the bytes, PPMd's distributions and the chunk boundaries alone; no array was found whose
 * content depends on timing or placement. The host-side counters bytes_done, hc and bptt_rounds are compared first: a difference there is an ERROR
 * return whose message names the counter. out[0] differing words; [1..4] the first difference in region-then-array-then-address order: region, index,
 * the word of a, the word of b (UINT64_MAX without a difference); [5..15] the count per region. */
#define CMX_LSTM_STATE_REGIONS 11
#define CMX_LSTM_STATE_ARRAYS 80
int cmx_lstm_state_diff(cmx_lstm_t* a, cmx_lstm_t* b, uint64_t out[16]);
/* TEST HOOK: XOR one state word (addressed as cmx_lstm_state_diff reports it) between runs. Synchronises the device. REFUSES region 9: its words are
 * indices and counters the kernels address memory with; everywhere else a changed word is a float the kernels use as a value, never as an address. A
 * data change only: no kernel stops and no wait times out. */
int cmx_lstm_debug_state_xor(cmx_lstm_t*, int region, uint64_t index, uint32_t xor_mask);
/* TEST READOUT: per array, in the order above, [3 i] its region, [3 i + 1] its word offset inside the region, [3 i + 2] its words, for the handle's
 * vocabulary size; returns the number of arrays (CMX_LSTM_STATE_ARRAYS) or -1. */
int cmx_lstm_debug_layout(cmx_lstm_t*, uint64_t out[3 * CMX_LSTM_STATE_ARRAYS]);

/* ------------------------------------------------------------------------
 * 2c. Stage: context plumbing + the 54 small native models = ContextManager, the 54 byte / 8 bit
 *     contexts, Direct / DirectHash / Indirect / Match / Bracket (src/context-manager.cpp,
 *     src/contexts/ *.cpp, src/states/ *.cpp, src/models/{direct,direct-hash,indirect,match,bracket,
 *     byte-model}.cpp; wired at predictor.cpp:90-178,199-356,361-369,421-446)
 * ------------------------------------------------------------------------ */
typedef struct cmx_ctxmodels cmx_ctxmodels_t;
cmx_ctxmodels_t* cmx_ctxmodels_create(const uint8_t vocab[256], int device);
void cmx_ctxmodels_destroy(cmx_ctxmodels_t*);
/* Chunk mode over nbytes already-known bytes. DEVICE pointers:
 *   d_bytes [nbytes]            u8   the bytes coded
 *   d_probs [8*nbytes][pstride] f32  the layer-0 matrix the mixing network reads (pstride >= 2078; a compact handle, below: >= 64);
 *                                    OUT: columns 0,1,2 and 2025..2075 of every row (Model::Predict of
 *                                    the 54 models); other columns untouched
 *   d_sel   [8*nbytes][47]      u32  OUT: every mixer's selector at each Predict() (entry 12 = 0: the
 *                                    mixing-network stage derives auxiliary_context_ itself)
 * Asynchronous on `stream`. */
int cmx_ctxmodels_run(cmx_ctxmodels_t*, const uint8_t* d_bytes, size_t nbytes, float* d_probs, size_t pstride,
                      uint32_t* d_sel, void* stream);
/* Predictor::Pretrain (predictor.cpp:471-487) over nbytes dictionary bytes for the models of this
 * stage: same state transitions as cmx_ctxmodels_run, no outputs (mixers/SSE/LSTM/PPMd are not
 * trained during pretraining). */
/* Bit-synchronous mode: the 8 rows (outputs + selectors) the stage would produce if the next byte were *d_byte,
 * without changing any state. Row j depends only on the top j bits of *d_byte: with j bits of the byte coded, row j
 * is what Predict() uses for the next bit. */
int cmx_ctxmodels_peek(cmx_ctxmodels_t*, const uint8_t* d_byte, int bit_index /* 0..7: the row needed; -1: all */,
                       float* d_probs8, size_t probs_stride, uint32_t* d_sel8, void* stream);
int cmx_ctxmodels_pretrain(cmx_ctxmodels_t*, const uint8_t* d_bytes, size_t nbytes, void* stream);
/* Test introspection: bytes that went through the serial path taken when two Indirect models' 256-byte windows of
 * the shared map overlap (indirect.cpp:16-31) -- [0] committed, [1] in dry (peek) passes. Synchronises. */
int cmx_ctxmodels_debug_slow_bytes(cmx_ctxmodels_t*, uint64_t out2[2]);
/* Test hook (state injection): the stage as after `pos` bytes of a stream whose last n bytes were `tail` (HOST) -- ContextManager::history_pos_ (modulo the
 * 100 000 000-byte ring, context-manager.cpp:24-27), every Match model's own byte counter (match.cpp:43-46), the ring's bytes in front of the position. */
int cmx_ctxmodels_debug_set_history(cmx_ctxmodels_t*, uint64_t pos, const uint8_t* tail, uint64_t n);
/* Waits for the handle's work; reports device-side failures. */
int cmx_ctxmodels_sync(cmx_ctxmodels_t*);
/* Test hook: ContextManager registers (25), byte contexts (54), bit contexts (8) between bytes. */
int cmx_ctxmodels_get_manager(cmx_ctxmodels_t*, uint64_t* regs25, uint64_t* ctx54, uint64_t* bitctx8);
/* THE COMPACT FORM of a handle (for redundant instances, below): model l = 0..53 (lane order: layer-0 columns 0, 1, 2, 2025..2075) writes column l
 * of d_probs, and cmx_ctxmodels_run accepts pstride >= CMX_CTX_COMPACT_STRIDE. The Bracket model's column is 0 either way. Only the lane table's
 * `col` differs: the kernel, the state, the tables and the rand() draws are those of cmx_ctxmodels_create -- a compact and a full handle over the same
 * bytes differ in configuration, never in state. */
#define CMX_CTX_COMPACT_STRIDE 64
cmx_ctxmodels_t* cmx_ctxmodels_create_compact(const uint8_t vocab[256], int device);
/* THE REDUNDANT CONTEXT-STAGE VOTE (opt-in; src/ctxmodels_vote.hip). This stage is the only producer of the 47 selectors and writes 54 layer-0
 * columns. Verify mode compares the network's copy of a slot with the slot, and the network's vote runs every instance on the same slot: a word this
 * stage got WRONG passes both. The complementary guard runs the unchanged stage kernel on n = 2 or 3 handles over the same bytes and compares what they
 * wrote. A chunk of nbytes has T = nbits = 8 nbytes rows; per row and instance 101 values are compared as 32-bit WORDS, never as floats (-0.0 differs from
 * 0.0, equal NaN patterns are equal). Elements are ordered by e = t * 101 + c: c = 0..53 the model outputs in lane order (layer-0 columns 0, 1, 2,
 * 2025..2075), c = 54..100 selectors 0..46. Column 2076 (PPMd's bits) is not this stage's output and is not compared. The rule is cmx_vote_run's:
 * n = 3: all equal agree, exactly two equal make the third the ODD instance, all different is NO MAJORITY; n = 2: different is no majority.
 * cmx_ctxvote_run is asynchronous on `stream`: per instance i the DEVICE matrix d_probs[i] with row stride pstride[i] (floats), compact[i] != 0 where
 * it has the compact form (pstride >= 64), else the full layer-0 form (pstride >= 2078, read in place: instance 0 is the stream's own stage), and its
 * selectors d_sel[i] [T][47]. Nothing is assumed about alignment. d_bits ([T], may be NULL: captured as 0) are the coded bits. One kernel with one
 * wavefront per row (grid-stride) and a one-wave kernel behind it that folds the chunk into the sticky DEVICE record.
 * _report / _record / _last: exactly the eight / four words of cmx_vote_report / _record / _last, [5] (of _last: [2]) being the element's c.
 * cmx_ctxvote_values: the capture of the first event's bit -- words[i * 101 + c] of instance i (n x 101 used) and the coded bit. Synchronises.
 * Out of scope: REPAIR on the majority (an event stops the stream), the slot's other producers (fxcm, paq8, LSTM, PPMd), the bit and decay words,
 * the decoder's form of the stage. */
#define CMX_CTXVOTE_COLS 101
typedef struct cmx_ctxvote cmx_ctxvote_t;
cmx_ctxvote_t* cmx_ctxvote_create(int device, int n);
void cmx_ctxvote_destroy(cmx_ctxvote_t*);
int cmx_ctxvote_run(cmx_ctxvote_t*, const float* const* d_probs, const size_t* pstride, const int* compact, const uint32_t* const* d_sel, size_t nbits,
                    uint64_t stream_bit0, const uint8_t* d_bits, void* stream);
int cmx_ctxvote_report(cmx_ctxvote_t*, uint64_t out[8]);
const unsigned long long* cmx_ctxvote_record(cmx_ctxvote_t*);
int cmx_ctxvote_values(cmx_ctxvote_t*, uint32_t words[3 * CMX_CTXVOTE_COLS], uint32_t* bit);
int cmx_ctxvote_last(cmx_ctxvote_t*, uint64_t out[4]);
/* Every 32-bit word of two handles' state in HBM, compared (both on one device; a == b is refused; synchronises; reads several GB per handle: after
 * an event and in tests, between chunks only). Regions in order: 0 CtxPersist (the registers, the Bracket model, the Indirect / Match prediction
 * tables, the per-lane positions), 1 the history ring, 2 the shared map, 3 the bracket stack, then the per-lane tables: 4 pred, 5 cnt, 6 chk
 * (Direct / DirectHash), 7 the Match models' map, 8 ihash (IndirectHash contexts). out[0] differing words; [1..5] the first difference in
 * region-then-lane-then-address order: region, lane (UINT64_MAX in regions 0..3), word index within the array, the word of a, the word of b
 * (UINT64_MAX without a difference); [6..14] the count per region; [15] bit l set: lane l has a differing table word (regions 4..8). */
int cmx_ctxmodels_state_diff(cmx_ctxmodels_t* a, cmx_ctxmodels_t* b, uint64_t out[16]);
/* TEST HOOK: XOR one state word (addressed as cmx_ctxmodels_state_diff reports it; lane = UINT64_MAX in regions 0..3) between chunks. Synchronises
 * the device. A data change only: no kernel stops and no wait times out. */
int cmx_ctxmodels_debug_state_xor(cmx_ctxmodels_t*, int region, uint64_t lane, uint64_t index, uint32_t xor_mask);
/* TEST READOUT: word offsets inside region 0 of [0] regs (u64 each), [1] br_probs[256], [2] ipred[31][256], [3] mpred[16][256]; [4] the region's words */
int cmx_ctxmodels_debug_layout(uint64_t out[5]);

/* ------------------------------------------------------------------------
 * 2f. Stage: the vendored fxcm model = FXCM::Predict / FXCM::Perceive (src/models/fxcm.cpp:14-33) around
 *     fxcmv1::Predictor::update1 + modelPrediction (src/models/fxcmv1.cpp:4758-4833, :3798-4757); cmix wires it at
 *     predictor.cpp:98-99 (construction, dictionary path), :462-468 (lstmpr / lstmex set, then Perceive last).
 *     431 values per bit = layer-0 columns 3..433. The text parser half (everything the model computes at a byte
 *     boundary from the bytes alone) runs on the calling host thread, the learned tables on the device.
 * ------------------------------------------------------------------------ */
typedef struct cmx_fxcm cmx_fxcm_t;
/* dictionary_path: cmix's WRT dictionary (the reference's global `dictionary_path`, runner.cpp:17; fxcmv1.cpp:412-428),
 * NULL or "" without one. */
cmx_fxcm_t* cmx_fxcm_create(const char* dictionary_path, int device);
void cmx_fxcm_destroy(cmx_fxcm_t*);
/* Chunk mode over nbytes already-known bytes (whole bytes; chunks of one stream in order).
 *   bytes    [nbytes]            u8  HOST   the bytes coded (parsed on the calling thread before the call returns)
 *   d_bytes  [nbytes]            u8  DEVICE the same bytes
 *   d_lstmpr [8*nbytes]          i16 DEVICE lstmpr as cmix sets it before FXCM::Perceive of each bit (1 + 4094 * p, predictor.cpp:463)
 *   d_lstmex [8*nbytes]          u8  DEVICE lstmex, same (the LSTM's likeliest byte, predictor.cpp:464)
 *   d_probs  [8*nbytes][pstride] f32 DEVICE OUT columns 3..433 of every row: row q = FXCM::Predict() before bit q of the
 *                                    chunk is coded (row 0 of a stream's first chunk = the constructor's 0.5); other
 *                                    columns untouched; pstride >= 434
 * Asynchronous on `stream`. */
int cmx_fxcm_run(cmx_fxcm_t*, const uint8_t* bytes, const uint8_t* d_bytes, size_t nbytes, const int16_t* d_lstmpr, const uint8_t* d_lstmex,
                 float* d_probs, size_t pstride, void* stream);
int cmx_fxcm_sync(cmx_fxcm_t*);
/* 1 if a bounded in-launch wait of the roles kernel (context maps on two workgroups, units, mixers: four workgroups) ran out (the stream's
 * fxcm columns are void from there); syncs. */
int cmx_fxcm_failed(cmx_fxcm_t*);
const unsigned* cmx_fxcm_fail_flag(cmx_fxcm_t*);   /* as cmx_lstm_fail_flag */
int cmx_fxcm_set_upload_stream(cmx_fxcm_t*, void* stream);   /* see cmx_mixnet_set_upload_stream */
/* diagnostics (CMX_FXCM_PROFILE=1 at create time): thread 0's clocks per phase of each role since creation, out[16 role + k] (role 0 = the
 * context maps' first wavefront, 1 = units, 2 = mixers; scripts/gpu_fxcm_time.py names the phases) */
int cmx_fxcm_profile(cmx_fxcm_t*, unsigned long long out128[128]);   /* [64 + 8 bpos + k]: role M by bit position */
/* TEST HOOK (as cmx_p8stage_debug_set_pos): before the first byte, continue as if blpos bytes of the block had been coded -- the device model's
 * position (SSCM / APM rates, update1 :4772-4774) and the host parser's (the rules 448, 451 and 463 MB into a block). Waits for the device first;
 * refused once the stream has begun. */
int cmx_fxcm_debug_set_blpos(cmx_fxcm_t*, int blpos);
/* TEST HOOK (CMX_FXCM_JITTER=seed at create time): how often each of the roles kernel's 18 stall sites has stalled since creation -- [0..15] role M's
 * wavefronts, [16] role U, [17] role X; all zero without the switch. Syncs. */
int cmx_fxcm_debug_jitter_counts(cmx_fxcm_t*, unsigned out18[18]);
/* TEST HOOKS: the launches so far that found the previous launch of their record-staging slot (CMX_PIPELINE_SLOTS slots, taken in turn) still in
 * flight and waited for it; the model's slot_parallel word as the kernels read it from device memory (0 under CMX_FXCM_SERIAL_MAPS=1; syncs). -1: error. */
int cmx_fxcm_debug_ring_waits(cmx_fxcm_t*);
int cmx_fxcm_debug_slot_parallel(cmx_fxcm_t*);
/* SHADOW INSTANCES (for the vote below). ONE PARSER, SHARED RECORDS: the host text parser runs once per chunk, in the stream's own handle (the OWNER,
 * cmx_fxcm_create). cmx_fxcm_create_shadow makes a handle with the same device state (the same fxb::build, which reads no dictionary) and NO parser;
 * cmx_fxcm_run and the decoder's calls refuse it. cmx_fxcm_run_shared(shadow, owner, ...) launches the unchanged roles kernel on the shadow's own
 * FxDev, row buffer, hand-off block and fail flag, reading the records the owner's MOST RECENT cmx_fxcm_run uploaded: `stream` waits for that staging
 * slot's upload event, nbytes must be that chunk's size, and a shadow must have run exactly the chunks its owner ran before this one (refused with the
 * two byte counts otherwise). d_bytes, d_lstmpr, d_lstmex: as cmx_fxcm_run, normally the owner's own arrays; d_probs: the shadow's rows (columns
 * 3..433 of pstride >= 434). An owner takes at most two shadows. The parser's records, the chunk's bytes and the LSTM hints exist once and are read by
 * every instance: they are NOT covered by the vote. STAGING RING: the owner refills a staging slot only when its own launch on it AND every shadow
 * launch that read it have completed (a per-reader event in the owner's slot, waited for where the owner's own is); cmx_fxcm_debug_ring_waits counts a
 * launch that met any of them in flight, once. Destroy in any order. Under CMX_FXCM_JITTER a shadow stalls with a seed of its own. */
cmx_fxcm_t* cmx_fxcm_create_shadow(int device);
int cmx_fxcm_run_shared(cmx_fxcm_t* shadow, cmx_fxcm_t* owner, const uint8_t* d_bytes, size_t nbytes, const int16_t* d_lstmpr, const uint8_t* d_lstmex,
                        float* d_probs, size_t pstride, void* stream);
/* THE REDUNDANT FXCM-STAGE VOTE (opt-in; src/fxcm_vote.hip). n = 2 or 3 instances of the unchanged roles kernel (above) and a word-for-word
 * comparison of what they wrote. A chunk of nbits bits (whole bytes) has nbits rows; a row is one BIT: the 431 values FXCM::Predict() returns before
 * that bit is coded, compared as 32-bit WORDS, never as floats. Row t of instance i is at d_rows[i] + t * pstride[i]: instance 0 is the stream's own
 * stage, read IN PLACE from the slot's layer-0 rows (d_rows[0] = layer0 + 3, pstride 2078; such a row's base is only 4-byte aligned, differently from
 * row to row, so the kernel uses 4-byte loads and nothing wider); a shadow's dense buffer is d_probs + 3 with pstride 434. Elements are ordered by
 * e = t * 431 + c, c = 0..430 = layer-0 column 3 + c. The rule is cmx_vote_run's: n = 3: all equal agree, exactly two equal make the third the ODD
 * instance, all different is NO MAJORITY; n = 2: different is no majority. Asynchronous on `stream`: one kernel with one wavefront per row (grid-stride;
 * a per-lane minimum key (e << 2 | odd), count and odd mask, one reduction and one atomic each of the three per wave that saw a difference; no LDS, no scratch) and a
 * one-wave kernel behind it that folds the chunk into the sticky DEVICE record. d_bytes ([nbits / 8], may be NULL: captured as 0): the chunk's bytes.
 * _report / _record / _last: the eight / four words of cmx_lstmvote_report / _record / _last with BITS where those have bytes: [0] chunks voted,
 * [1] bits voted, [2] n, [3] chunks with an event, then of the FIRST event [4] (of _last: [1]) its stream bit, [5] (of _last: [2]) its column c,
 * [6] (of _last: [3]) the odd instance or UINT64_MAX = no majority, [7] (of _last: [0]) the chunk's differing elements; "first" = lowest bit, then
 * lowest column. _values: the capture of the first event's row -- words[i * 431 + c] of instance i (n x 431 used), the bit coded at that row and its
 * byte. Synchronises. NO REPAIR: the mixing network has consumed the columns when the host sees a vote; an event stops the stream. */
#define CMX_FXCMVOTE_COLS 431
typedef struct cmx_fxcmvote cmx_fxcmvote_t;
cmx_fxcmvote_t* cmx_fxcmvote_create(int device, int n);
void cmx_fxcmvote_destroy(cmx_fxcmvote_t*);
int cmx_fxcmvote_run(cmx_fxcmvote_t*, const float* const* d_rows, const size_t* pstride, size_t nbits, uint64_t stream_bit0, const uint8_t* d_bytes, void* stream);
int cmx_fxcmvote_report(cmx_fxcmvote_t*, uint64_t out[8]);
const unsigned long long* cmx_fxcmvote_record(cmx_fxcmvote_t*);
int cmx_fxcmvote_values(cmx_fxcmvote_t*, uint32_t words[3 * CMX_FXCMVOTE_COLS], uint32_t* bit, uint32_t* byte);
int cmx_fxcmvote_last(cmx_fxcmvote_t*, uint64_t out[4]);
/* Every 32-bit word of two handles' state in HBM, compared (both on one device; a == b is refused; synchronises; 4.4 GB per handle: after an event
 * and in tests, between chunks only). The arrays are the blocks fxb::build (src/fxcm_build.h) asks for, which two handles allocate in the same order
 * and size; an index is a word offset into the region's arrays laid end to end, each array rounded up to whole words:
 *    0 constant tables  squash, stretch, wrt, the six state tables, the 31 maps' lookup tables `tab` (map order), the six 33-entry APM fill patterns
 *    1 map buckets      maps[k].t, k = 0..30
 *    2 map StateMaps    maps[k].sm, k = 0..30 ([C_k][256])
 *    3 SSCM tables      sscm_data[0..6]
 *    4 sm1_t            sm1_t[0..2]
 *    5 rcm_t            6 mhash            7 sp_table            8 buffer (the byte history)
 *    9 wx               wx[0..11]: the ten first-layer mixers' rows of 512 weights, the two final mixers' rows of 16
 *   10 APM tables       apm_t[0..5]
 *   11 FxDev            the stream's FxDev itself (src/fxcm_dev.h) as sizeof(FxDev) / 4 words with every device pointer (and the padding of the four
 *                       match candidates) read as 0: the per-map cp / cp0 / runp / cxt / sm_cxt, the SSCM, sm1, run-map, match and sparse-match
 *                       scalars, pos, and everything from mx_elim to rec; an index is the word's offset in FxDev
 * NOT compared: the device pointers inside FxDev (they differ by construction), the per-launch hand-off block and row buffer (rewritten by every
 * launch before they are read), the staged records (the owner's only). The host-side counter bytes_done is compared first: a difference there is an
 * ERROR return whose message says so. out[0] differing words; [1..4] the first difference in region-then-array-then-address order: region, index, the
 * word of a, the word of b (UINT64_MAX without a difference); [5..16] the count per region. */
#define CMX_FXCM_STATE_REGIONS 12
#define CMX_FXCM_STATE_ARRAYS 141
#define CMX_FXCM_STATE_OUT 17
int cmx_fxcm_state_diff(cmx_fxcm_t* a, cmx_fxcm_t* b, uint64_t out[CMX_FXCM_STATE_OUT]);
/* TEST HOOK: XOR one state word (addressed as cmx_fxcm_state_diff reports it) between launches. Synchronises the device. A data change only: no kernel
 * stops, addresses memory with the changed word, or times out. OPEN: regions 2 (map StateMaps), 3 (SSCM), 4 (sm1_t), 5 (rcm_t), 9 (wx), 10 (APM):
 * every use of such a word is arithmetic or an index shifted into the range of the table it meets. REFUSED with a message: 0 (table values index other
 * tables), 1 (map buckets: the probe and replacement walks were not followed to the end), 6, 7, 8 (history positions and bytes the match models follow
 * in loops), 11 (offsets and indices). The reasoning per region stands next to the hook in src/fxcm_vote.hip. */
int cmx_fxcm_debug_state_xor(cmx_fxcm_t*, int region, uint64_t index, uint32_t xor_mask);
/* TEST READOUT: per array, in the order above, [3 i] its region, [3 i + 1] its word offset inside the region, [3 i + 2] its words; the last entry is
 * FxDev. Returns the number of arrays (CMX_FXCM_STATE_ARRAYS) or -1. Synchronises. */
int cmx_fxcm_debug_layout(cmx_fxcm_t*, uint64_t out[3 * CMX_FXCM_STATE_ARRAYS]);
/* TEST READOUT: `count` words of a region from `index` on (addressed as above; every region, 11 with its pointers read as 0) into out. Synchronises. A
 * test takes two readouts around a launch to learn which words the launch trained, i.e. which words the next one will read. */
int cmx_fxcm_debug_state_read(cmx_fxcm_t*, int region, uint64_t index, uint64_t count, uint32_t* out);

/* ---- callers of the path: arithmetic coder + container header (HOST code) -------------------------------------
 * Replaces Encoder::Encode/Flush (src/coder/encoder.cpp:10-39), Decoder::Decoder/Decode (src/coder/decoder.cpp:3-39)
 * and WriteHeader/ReadHeader (src/runner.cpp:34-84). The probabilities are the p[] a pipeline chunk produced
 * (copied to the host by the caller); p[t] = P(bit t = 1). Bytes are coded MSB first (runner.cpp:106-108). */
typedef struct cmx_encoder cmx_encoder_t;
typedef struct cmx_decoder cmx_decoder_t;
cmx_encoder_t* cmx_encoder_create(void);
void cmx_encoder_destroy(cmx_encoder_t*);
int cmx_encoder_encode_bits(cmx_encoder_t*, const float* p, const uint8_t* bits, size_t nbits);
int cmx_encoder_encode_bytes(cmx_encoder_t*, const float* p /* [8*nbytes] */, const uint8_t* bytes, size_t nbytes);
int cmx_encoder_flush(cmx_encoder_t*);                 /* Encoder::Flush; further encode calls fail */
size_t cmx_encoder_size(const cmx_encoder_t*);          /* code bytes produced so far */
const uint8_t* cmx_encoder_data(const cmx_encoder_t*);  /* valid until the next encode/flush/destroy */
/* `code` must stay valid for the decoder's lifetime; reads past its end return zeros like the reference. */
cmx_decoder_t* cmx_decoder_create(const uint8_t* code, size_t len);
void cmx_decoder_destroy(cmx_decoder_t*);
int cmx_decoder_decode(cmx_decoder_t*, float p);        /* the next bit (0/1), -1 on a bad argument */
int cmx_decoder_decode_bits(cmx_decoder_t*, const float* p, size_t nbits, uint8_t* bits_out); /* replay of known p[] */
#define CMX_HEADER_MAX 37
#define CMX_MIN_VOCAB_FILE_SIZE 10000                   /* runner.cpp:14 */
/* 5 bytes of length (bit 39 = dictionary flag) + the 32-byte vocabulary bitmap when length >= 10000. Return the
 * number of header bytes written / consumed, 0 on error. */
size_t cmx_header_write(uint64_t length, const uint8_t vocab[256], int dictionary_used, uint8_t out[CMX_HEADER_MAX]);
size_t cmx_header_read(const uint8_t* in, size_t len, uint64_t* length, int* dictionary_used, uint8_t vocab[256]);

/* ------------------------------------------------------------------------
 * 2d. HOST stage: PPMd order-25 byte model = PPMD::PPMD / PPMD::ByteUpdate (src/models/ppmd.cpp:
 *     1322-1338 and everything below it; constructed with (25, 14000 MB) at predictor.cpp:101).
 *     A pure function of the byte stream, 0.4 % of the reference's CPU time: it runs ahead of the device
 *     pipeline on one host core (SURVEY.md 8 note 2). HOST pointers.
 * ------------------------------------------------------------------------ */
typedef struct cmx_ppmd cmx_ppmd_t;
cmx_ppmd_t* cmx_ppmd_create(const uint8_t vocab[256]);
cmx_ppmd_t* cmx_ppmd_create_ex(const uint8_t vocab[256], int order, int memory_mb); /* test hook: other (order, MB) */
void cmx_ppmd_destroy(cmx_ppmd_t*);
/* Feeds nbytes bytes; out_probs [nbytes][256] f32 receives ByteModel::probs_ after each byte (what
 * predictor.cpp:450-457 hands to the byte mixer and what column 2076 is formed from). Fails (nonzero) if the
 * model would need the reference's memory-exhaustion path (ppmd.cpp:686-727), which is not implemented. */
int cmx_ppmd_run(cmx_ppmd_t*, const uint8_t* bytes, size_t nbytes, float* out_probs);

/* ------------------------------------------------------------------------
 * 3. One stream through every stage built so far: the native orchestration behind the Predictor
 *    surface, a chunk of already-known bytes at a time (Predictor::Predict/Perceive, predictor.cpp:
 *    361-469, in compression look-ahead form). PPMd runs on the calling host thread; the context /
 *    small-model stage, the LSTM and the mixing network run on three internal HIP streams; up to
 *    CMX_PIPELINE_SLOTS chunks may be in flight (a submit blocks while the chunk that many submits back is still running:
 *    a chunk's latency through the stages is several chunk periods, the depth keeps every stage busy).
 * ------------------------------------------------------------------------ */
/* Environment read by the engine (all optional):
 *   GPU_MAX_HW_QUEUES      (HIP's own) not read, not set and not needed: every HIP stream of the library is created with a compute-unit
 *                          mask (the device's full one), which HIP never pools onto its shared queues, so each stage stream has a
 *                          hardware queue of its own whatever the variable says. An engine holds 13 (5 stages, upload, 7 paq8 roles),
 *                          14 when it decodes (the byte model); at most CMX_MAX_HW_QUEUES per device and process (cmx_hw_queues()).
 *   CMX_PIPELINE_STREAMS   2 or 1: throughput mode for several streams per GPU -- fewer hardware queues per engine (8 or 6;
 *                          roles take turns on shared streams, the per-stream period grows)
 *   CMX_MIXNET_XCD=k       the mixing network's 27 workgroups on XCD k, hand-off words through that XCD's L2 (bit-exact either way)
 *   CMX_MIXNET_JITTER=1..15  test hook: pseudo-random stalls in the mixing network's roles (bit-exact by construction; tests/test_gpu_mixnet.py)
 *   CMX_FXCM_JITTER=1..15  test hook: the same for the fxcm stage's three roles (compressor's form; tests/test_zgpu_stage_fxcm.py)
 *   (tolerance mode is NOT an environment switch: cmx_mixnet_set_tolerance / cmx_lstm_set_tolerance / cmx_pipeline_set_tolerance --
 *    no program that writes files turns it on)
 *   CMX_P8CM_SERIAL        1: paq8's table families walk every instance serially (A/B timing); 2: the ContextMap family's narrowed walk takes
 *                          its whole-instance fall-back at every second visit (test switch)
 * Co-residency: a stream's stage kernels run for a whole chunk and wait for each other inside the launch, so their workgroups -- 94 per
 * stream, most of them a compute unit each -- must all be resident. cmx_pipeline_create / _enable_fxcm /
 * _enable_paq8 keep count per device and refuse (cmx_last_error says why) an engine that would exceed the device's compute units.
 *   CMX_FXCM_PROFILE, CMX_P8FAM_PROFILE, CMX_MIXNET_DBG     in-kernel phase timers / timing experiments (scripts/gpu_*prof*) */
#define CMX_PIPELINE_SLOTS 8   /* chunks in flight per stream (layer-0 matrices the caller cycles through) */
#define CMX_MAX_HW_QUEUES 32   /* dedicated hardware queues the library holds per device and process; a stage that would go past it is refused */
int cmx_hw_queues(int device);   /* the dedicated hardware queues (HIP streams) the library holds on the device now */
/* Construction ahead of time: start building the vocabulary-independent stages of an engine for `device` -- mixing
 * network, paq8 stage and (with_fxcm != 0; dictionary_path as for cmx_pipeline_enable_fxcm) the fxcm stage, ~16 GB of tables -- on a
 * thread of the library, and return at once. The caller goes on with what has to precede the predictor (runner.cpp:166-202:
 * preprocessing into the temp file, the vocabulary scan); the next cmx_pipeline_create / _enable_fxcm / _enable_paq8 on that device
 * (also behind cmx_stage_input) adopts whatever is ready and waits for what is not. Once per process; purely an optimisation: every
 * stage that was not prewarmed (or failed to) is built by the normal path. */
int cmx_prewarm(int device, const char* dictionary_path, int with_fxcm);

typedef struct cmx_pipeline cmx_pipeline_t;
cmx_pipeline_t* cmx_pipeline_create(const uint8_t vocab[256], int device, size_t max_chunk_bytes);
void cmx_pipeline_destroy(cmx_pipeline_t*);
/* The overlap probe (run by cmx_pipeline_create, _enable_fxcm, _enable_paq8 and cmx_pipeline_late_start): one tiny kernel on each of the
 * handle's streams, each waiting (at most ~50 ms) for all the others to run beside it. 1: every stage stream ran concurrently with all the
 * others at the last probe; 0: some did not (they share hardware queues: the stages of a chunk then run one after another -- the coded
 * bytes are right either way, only the period grows; a decoder refuses to start); -1: bad handle. */
int cmx_pipeline_stage_overlap(cmx_pipeline_t*);
/* Code the next n <= max_chunk_bytes bytes of the stream.
 *   bytes    HOST   [n]
 *   d_layer0 DEVICE [8n][2078] f32: columns 3..2024 (fxcm, paq8 -- no stage yet) must already hold the
 *                   Model::Predict values of every bit and be complete on the device; all other columns
 *                   are written by the engine
 *   d_p_out  DEVICE [8n] f32 OUT: the value Predictor::Predict() returns for each bit
 * Returns after enqueueing (it only waits for the chunk before the previous one); d_layer0 / d_p_out must
 * stay valid until cmx_pipeline_sync() or until two further submits have returned. */
int cmx_pipeline_submit(cmx_pipeline_t*, const uint8_t* bytes, size_t n, float* d_layer0, float* d_p_out);
/* The same chunk in steps, for look-ahead coding while some model families still run on the host:
 *   _begin   PPMd (this thread), upload, context stage and LSTM are enqueued; up to CMX_PIPELINE_SLOTS chunks may be begun and not
 *            finished;
 *   _hints   (optional) for the oldest begun chunk that has not handed them out: lstm_p[t], lstm_ex[t], t = 0 .. 8n,
 *            = the LSTM byte mixer's ByteModel::Predict value and `ex` for bit t of the chunk (t = 8n: the first bit
 *            after it). After coding bit t the reference's globals hold lstmpr = 1 + 4094 * lstm_p[t+1] (float
 *            arithmetic, truncated) and lstmex = lstm_ex[t+1] (predictor.cpp:180-182,462-465): what a host fxcm
 *            needs to run ahead. HOST arrays of 8n+1 entries; waits for that chunk's LSTM stage;
 *   _finish  the oldest begun chunk: its layer-0 columns 3..2024 from HOST rows cols[8n][2022] (NULL = already in
 *            d_layer0), then the mixing network -> d_p_out[8n]. Asynchronous.
 * cmx_pipeline_submit = _begin + _finish(NULL). */
int cmx_pipeline_begin(cmx_pipeline_t*, const uint8_t* bytes, size_t nbytes, float* d_layer0);
int cmx_pipeline_hints(cmx_pipeline_t*, float* lstm_p, int* lstm_ex);
int cmx_pipeline_finish(cmx_pipeline_t*, const float* cols, float* d_p_out);
/* The fxcm stage on the device (section 2f), opt-in, before the first chunk: cmx_pipeline_begin then also derives the
 * per-bit lstmpr / lstmex from the LSTM stage's output on the device and runs the fxcm stage (text parser on the calling
 * thread, kernel on a fourth HIP stream) into columns 3..433; cmx_pipeline_pretrain covers it; the caller hands in only
 * the remaining columns with cmx_pipeline_finish_cols (HOST rows of ncols floats = layer-0 columns first_col ..
 * first_col + ncols - 1; with the fxcm stage enabled first_col >= 434) -- cmx_pipeline_finish with rows then fails.
 * dictionary_path: as cmx_fxcm_create. */
int cmx_pipeline_enable_fxcm(cmx_pipeline_t*, const char* dictionary_path);
/* The paq8 stage on the device (section 2f at the end of this file), opt-in, before the first chunk: cmx_pipeline_begin then
 * also runs it (front end on the calling thread, kernels on the stage's own streams) into columns 434..2024 of d_layer0;
 * cmx_pipeline_pretrain feeds it the dictionary. With both vendored families on the device cmx_pipeline_finish takes no
 * columns (cmx_pipeline_submit does everything) and the Predictor shim needs no cmx_set_model_outputs. */
int cmx_pipeline_enable_paq8(cmx_pipeline_t*);
/* Wait until chunk number `index` (0 = the first submitted) has left the mixing network; only the last CMX_PIPELINE_SLOTS can be waited for. */
int cmx_pipeline_wait(cmx_pipeline_t*, uint64_t index);
/* cmx_pipeline_wait(index), then that chunk's probabilities (8 x its byte count floats, from the d_p_out it was submitted with) into
 * the HOST buffer p_host (page-locked for speed). Waits for this chunk only; the chunks behind it stay in flight. */
int cmx_pipeline_fetch(cmx_pipeline_t*, uint64_t index, float* p_host);
int cmx_pipeline_paq8_enabled(cmx_pipeline_t*);
int cmx_pipeline_paq8_total_ms(cmx_pipeline_t*, double* ms);
/* the paq8 stage's role-kernel times (cmx_p8stage_role_ms) since the last reset of the stage totals */
int cmx_pipeline_paq8_role_ms(cmx_pipeline_t*, double ms[7], uint64_t* chunks);
/* wall time of the calling thread inside begin / finish since the last reset of the stage totals, ms: [0] waiting for a
 * slot, [1] PPMd, [2] uploads + context stage + LSTM enqueue, [3] fxcm (parser + enqueue), [4] paq8 (front end + enqueue),
 * [5] mixing network enqueue */
int cmx_pipeline_host_ms(cmx_pipeline_t*, double ms[6]);
int cmx_pipeline_fxcm_enabled(cmx_pipeline_t*);
int cmx_pipeline_finish_cols(cmx_pipeline_t*, const float* cols, int first_col, int ncols, float* d_p_out);
int cmx_pipeline_fxcm_total_ms(cmx_pipeline_t*, double* ms);
/* the mixing network's tolerance mode for this stream (cmx_mixnet_set_tolerance), before the first chunk; _mixnet_mode: 0 strict, 1 tolerance */
/* diagnostics of a long run (all synchronise the device): rows allocated by each of the 47 final mixers (cap 10 000 + the shared
 * overflow row, mixer.cpp:16-36); speculation statistics of the mixing network (cmx_mixnet_spec_stats); the paq8 family kernel's
 * phase / path counters (CMX_P8FAM_PROFILE=1 at create time; cmx_p8stage_profile); PPMd's arena: {bytes reserved, untouched, in use} */
int cmx_mixnet_rows(cmx_mixnet_t*, uint32_t rows[47]);
int cmx_ppmd_arena(cmx_ppmd_t*, uint64_t out3[3]);
int cmx_pipeline_mixnet_rows(cmx_pipeline_t*, uint32_t rows[47]);
/* diagnosis: from now on every mixer's output (Mixer::Mix, mixer.cpp:38-55, all 47) of every bit of the stream's look-ahead chunks goes to
 * the DEVICE area d_mix[cap_bits][47] in stream order (bits past cap_bits are not recorded); NULL switches it off */
int cmx_pipeline_debug_mix_out(cmx_pipeline_t*, float* d_mix, uint64_t cap_bits);
/* diagnosis: the DEVICE selectors [8 n][47] and coded bits [8 n] of chunk number `index` (one of the last CMX_PIPELINE_SLOTS submitted), valid until its slot is reused */
int cmx_pipeline_debug_slot(cmx_pipeline_t*, uint64_t index, const uint32_t** d_sel, const uint8_t** d_bits, size_t* nbytes);
int cmx_pipeline_spec_stats(cmx_pipeline_t*, uint64_t out[5]);
int cmx_pipeline_paq8_profile(cmx_pipeline_t*, unsigned long long out128[128]);
int cmx_pipeline_ppmd_arena(cmx_pipeline_t*, uint64_t out3[3]);
int cmx_pipeline_set_tolerance(cmx_pipeline_t*, int on);
/* the mixing network's verify mode for this stream (cmx_mixnet_set_verify), before the first chunk: the record is copied back behind every chunk's
 * network, and cmx_pipeline_wait (and _fetch) fail the chunk in which a mismatch showed, with the record in the message, and void the handle;
 * _verify_report as cmx_mixnet_verify_report */
int cmx_pipeline_set_verify(cmx_pipeline_t*, int on);
int cmx_pipeline_verify_report(cmx_pipeline_t*, uint64_t out[8]);
/* SHADOW MIXING NETWORKS (opt-in, k = 0 off / 1 / 2; before the first chunk): k more cmx_mixnet_t run every chunk on the slot's own layer-0 rows,
 * selectors and bits (nothing is copied), each on a stream of its own, and a vote (cmx_vote_*; instance 0 = the stream's network) follows every
 * chunk. Refused, with the reason, together with tolerance mode, when the device's hardware-queue budget (CMX_MAX_HW_QUEUES) does not allow k more
 * streams, and when its compute units do not allow 27 more resident workgroups per shadow. The k handles (~2.8 GB each) and the per-slot p / mixer
 * output buffers are created at the first cmx_pipeline_finish; with k = 0 nothing is allocated or launched. cmx_pipeline_wait / _fetch / _sync
 * fail the chunk in which instances first disagreed -- the message names the chunk, the stream bit, the column ("mixer 31" or "final p") and the odd
 * instance or "no majority between 2 instances" -- and void the handle (unless repair is armed, below), which can still be diagnosed and destroyed. May be
 * combined with verify mode (which covers instance 0). A handle that decodes (cmx_pipeline_late_start) drops the reservation: its report stays at
 * zero chunks. _shadow_report / _shadow_values: as cmx_vote_report / cmx_vote_values (all zero while nothing was voted). _shadow_state_diff:
 * cmx_mixnet_state_diff of instances a and b (0 = the stream's own network). _debug_shadow_xor: the test hook cmx_mixnet_debug_state_xor on one
 * instance, between chunks. */
int cmx_pipeline_set_shadow(cmx_pipeline_t*, int k);
int cmx_pipeline_shadow_report(cmx_pipeline_t*, uint64_t out[8]);
int cmx_pipeline_shadow_values(cmx_pipeline_t*, uint32_t words[144], uint32_t sel[47], uint32_t* bit);
int cmx_pipeline_shadow_state_diff(cmx_pipeline_t*, int a, int b, uint64_t out[20]);
int cmx_pipeline_debug_shadow_xor(cmx_pipeline_t*, int instance, int region, uint64_t mixer, uint64_t row, uint64_t index, uint32_t xor_mask);
/* REPAIR ON THE MAJORITY (opt-in; max_repairs = 0 off, the default: everything above holds word for word, nothing more is allocated or launched).
 * > 0 needs k = 2 shadows (a vote of two has no majority) and, like _set_shadow, comes before the first chunk. cmx_pipeline_wait / _fetch that find
 * an event beyond those already repaired then (1) drain every finished chunk from the three instances and the vote -- look-ahead has let them run up
 * to CMX_PIPELINE_SLOTS chunks past the event --; (2) look at every drained chunk's own result (cmx_vote_last): each must agree or name the SAME odd
 * instance o; (3) STOP exactly as without repair -- the same message, with the repairs made so far appended -- on no majority in any of them, a second
 * odd instance, a shadow's time-out flag, an event whose chunk has already left its slot unseen, or max_repairs used up; otherwise (4) run
 * cmx_mixnet_state_repair(instance o, a member of the majority); (5) if o == 0, overwrite the caller's p[] of every drained chunk that did not agree
 * (and its part of a cmx_pipeline_debug_mix_out area) device-to-device with shadow 1's, before the call returns -- nothing else on the device
 * consumes the final p: the stages' hints come from the LSTM's column of the layer-0 rows --; (6) log the repair and return 0: the handle stays
 * usable. A caller that wants repair waits for (or fetches) every chunk before its slot is reused. The sticky record (_shadow_report) goes on
 * counting events; cmx_pipeline_sync fails on events beyond those repaired.
 * WHAT A REPAIRED STREAM GUARANTEES: its probabilities are the majority's -- two instances with independent state (rows, tables, LDS, registers)
 * agreed on every one of the 48 words of every bit of every chunk, and after a repair all three states are equal word for word. Nothing is claimed
 * about inputs all three share (the layer-0 rows, selectors, bits): that is verify mode's ground, and the two combine.
 * _shadow_repairs: out[0] repairs made, out[1] the n entries that follow (the newest, at most CMX_REPAIR_LOG and what cap words hold), oldest first,
 * CMX_REPAIR_WORDS each: [0] chunk of the event, [1] its stream bit, [2] column, [3] odd instance, [4] non-agreeing values in that chunk, [5] state
 * words repaired (the repair's out[0]), [6..11] its out[1..6] (the first differing word), [12] out[18], [13] out[19] (the layer masks, whose lowest
 * bit names the origin mixer), [14] drained chunks that did not agree, [15] 0. */
#define CMX_REPAIR_LOG 8
#define CMX_REPAIR_WORDS 16
int cmx_pipeline_set_shadow_repair(cmx_pipeline_t*, int max_repairs);
int cmx_pipeline_shadow_repairs(cmx_pipeline_t*, uint64_t out[], size_t cap);
/* one entry of that log in words ("chunk 3, stream bit 6144, mixer 26, instance 0 odd, 812 state word(s) repaired, origin mixer 26"): a
 * thread-local string, valid until the thread's next call */
const char* cmx_repair_text(const uint64_t entry[CMX_REPAIR_WORDS]);
/* SHADOW CONTEXT STAGES (opt-in, k = 0 off / 1 / 2; before the first chunk AND before cmx_pipeline_pretrain, which must train every instance): k
 * compact cmx_ctxmodels_t run every chunk's bytes again, each on a stream of its own (also in the reduced-stream modes of CMX_PIPELINE_STREAMS) into
 * [T][64] / [T][47] buffers of their own, and a vote (cmx_ctxvote_*; instance 0 = the stream's own stage, read in place from the slot's layer-0
 * rows) follows every chunk on the last shadow's stream. Reserved at the set call, refused with the reason: k streams of the queue budget
 * (CMX_MAX_HW_QUEUES) and one resident workgroup per shadow. The handles (every table of the stage again, per shadow), the vote and the per-slot
 * buffers are created at the first cmx_pipeline_begin (or _pretrain); k = 0 gives everything back, and with k = 0 nothing is allocated, launched or
 * waited for. cmx_pipeline_wait / _fetch / _sync fail the chunk in which the instances first disagreed -- the message names the chunk, the stream bit,
 * "layer-0 column C" or "selector M", and the odd instance or "no majority between 2 instances" -- and void the handle, which can still be diagnosed
 * (_ctx_shadow_report / _values: as cmx_ctxvote_report / _values, all zero while nothing was voted; _ctx_shadow_state_diff: cmx_ctxmodels_state_diff of
 * instances a and b, 0 = the stream's own stage) and destroyed. NO REPAIR on the majority: an event stops the stream. Coexists with _set_shadow,
 * _set_shadow_repair and _set_verify. A handle that decodes (cmx_pipeline_late_start) drops the shadows: a decoder is not covered.
 * _debug_ctx_shadow_xor: the test hook cmx_ctxmodels_debug_state_xor on one instance, between chunks. */
int cmx_pipeline_set_ctx_shadow(cmx_pipeline_t*, int k);
int cmx_pipeline_ctx_shadow_report(cmx_pipeline_t*, uint64_t out[8]);
int cmx_pipeline_ctx_shadow_values(cmx_pipeline_t*, uint32_t words[3 * CMX_CTXVOTE_COLS], uint32_t* bit);
int cmx_pipeline_ctx_shadow_state_diff(cmx_pipeline_t*, int a, int b, uint64_t out[16]);
int cmx_pipeline_debug_ctx_shadow_xor(cmx_pipeline_t*, int instance, int region, uint64_t lane, uint64_t index, uint32_t xor_mask);
/* SHADOW LSTM STAGES (opt-in, k = 0 off / 1 / 2; strict mode only; before the first chunk -- and, unlike the shadow context stages, also AFTER
 * cmx_pipeline_pretrain: the LSTM is not pretrained, predictor.cpp:471-487, so a shadow misses nothing): k cmx_lstm_t made as the stream's own
 * (cmx_lstm_create(vocab, 31, device), same avoid_xcd setting and environment) run every chunk again on the slot's bytes and PPMd distributions, each
 * on a stream of its own (also in the reduced-stream modes of CMX_PIPELINE_STREAMS), behind the upload event that covers both, into buffers of their
 * own ([max][256] distributions, [8 max] bit predictions, [8 max] ex per slot and shadow), and a vote (cmx_lstmvote_*; instance 0 = the stream's own
 * stage, its bit predictions read in place from column 2077 of the slot's layer-0 rows) follows every chunk on the last shadow's stream. Nothing
 * downstream of the stream's own LSTM -- fxcm's hints, the final network -- waits for a shadow or for the vote; a slot is not reused before its vote
 * has read it. Reserved at the set call, refused with the reason: k streams of the queue budget (CMX_MAX_HW_QUEUES) and 52 resident workgroups per
 * shadow; refused together with the tolerance switch, and cmx_pipeline_set_tolerance is refused while shadows are set. The handles, the vote and the
 * per-slot buffers are created at the first cmx_pipeline_begin; k = 0 gives everything back, and with k = 0 nothing is allocated, launched or waited
 * for. cmx_pipeline_wait / _fetch / _sync fail the chunk in which the instances first disagreed -- the message names the chunk, the stream byte,
 * "distribution entry v", "bit k's prediction (layer-0 column 2077)" or "bit k's ex", and the odd instance or "no majority between 2 instances" -- and
 * void the handle, which can still be diagnosed (_lstm_shadow_report / _values: as cmx_lstmvote_report / _values, all zero while nothing was voted;
 * _lstm_shadow_state_diff: cmx_lstm_state_diff of instances a and b, 0 = the stream's own stage) and destroyed. A shadow's sticky time-out flag is
 * copied back in stream order and names that instance in the "in-launch hand-off of the LSTM" message. NO REPAIR: when the host sees a vote, fxcm and
 * the network have already consumed what the LSTM wrote on the device; an event stops the stream. Coexists with _set_verify, _set_shadow,
 * _set_shadow_repair, _set_ctx_shadow and _set_journal. A handle that decodes (cmx_pipeline_late_start) drops the shadows: a decoder is not covered.
 * _debug_lstm_shadow_xor: the test hook cmx_lstm_debug_state_xor on one instance, between chunks. */
int cmx_pipeline_set_lstm_shadow(cmx_pipeline_t*, int k);
int cmx_pipeline_lstm_shadow_report(cmx_pipeline_t*, uint64_t out[8]);
int cmx_pipeline_lstm_shadow_values(cmx_pipeline_t*, uint32_t words[3 * CMX_LSTMVOTE_COLS], uint32_t* byte);
int cmx_pipeline_lstm_shadow_state_diff(cmx_pipeline_t*, int a, int b, uint64_t out[16]);
int cmx_pipeline_debug_lstm_shadow_xor(cmx_pipeline_t*, int instance, int region, uint64_t index, uint32_t xor_mask);
/* SHADOW FXCM STAGES (opt-in, k = 0 off / 1 / 2; needs cmx_pipeline_enable_fxcm; before the first chunk AND before cmx_pipeline_pretrain: unlike the
 * LSTM, fxcm is pretrained, predictor.cpp:471-476, and a shadow set afterwards would have missed the dictionary -- refused): k shadow handles
 * (cmx_fxcm_create_shadow: 4.4 GB of tables each, no parser) run the unchanged roles kernel again on every chunk, each on a stream of its own, on the
 * records the stream's own parser produced for that chunk (cmx_fxcm_run_shared), the slot's bytes and the slot's LSTM hints, behind the hints' event and
 * the records' upload, into rows of its own (8 max_chunk x 434 floats per slot and shadow). A vote (cmx_fxcmvote_*; instance 0 = the stream's own
 * stage, read in place from columns 3..433 of the slot's layer-0 rows) follows every chunk on the last shadow's stream. The records, the bytes and the
 * hints are shared by all instances and NOT covered. Nothing downstream -- the mixing network -- waits for a shadow or for the vote; a slot is not
 * reused, and cmx_pipeline_wait does not return, before the slot's vote has read the in-place rows. cmx_pipeline_pretrain runs every dictionary chunk
 * on every shadow as well (shared records, the zero hints, a scratch and stream of its own; rows discarded, no vote). Reserved at the set call, refused
 * with the reason: k streams of the queue budget (CMX_MAX_HW_QUEUES) and 4 resident workgroups per shadow. The handles, the vote and the buffers are
 * created at the first cmx_pipeline_begin or at cmx_pipeline_pretrain, whichever comes first; k = 0 gives everything back, and with k = 0 nothing is
 * allocated, launched or waited for. fxcm has no tolerance form, so the switch does not matter here. cmx_pipeline_wait / _fetch / _sync fail the chunk
 * in which the instances first disagreed -- the message names the chunk, the stream bit (and byte + bit in byte), "fxcm column c (layer-0 column
 * 3 + c)", and the odd instance ("the stream's own stage" for 0) or "no majority between 2 instances" -- and void the handle, which can still be
 * diagnosed (_fxcm_shadow_report / _values: as cmx_fxcmvote_report / _values, all zero while nothing was voted; _fxcm_shadow_state_diff:
 * cmx_fxcm_state_diff of instances a and b, 0 = the stream's own stage; between chunks) and destroyed. A shadow's sticky time-out flag is copied back
 * in stream order and names that instance in the "in-launch hand-off of the fxcm" message. NO REPAIR: the network has consumed the columns. Coexists
 * with _set_verify, _set_shadow, _set_shadow_repair, _set_ctx_shadow, _set_lstm_shadow, _set_journal and _set_tolerance. A handle that decodes
 * (cmx_pipeline_late_start) drops the shadows: a decoder is not covered. _debug_fxcm_shadow_xor: the test hook cmx_fxcm_debug_state_xor on one
 * instance, between chunks. */
int cmx_pipeline_set_fxcm_shadow(cmx_pipeline_t*, int k);
int cmx_pipeline_fxcm_shadow_report(cmx_pipeline_t*, uint64_t out[8]);
int cmx_pipeline_fxcm_shadow_values(cmx_pipeline_t*, uint32_t words[3 * CMX_FXCMVOTE_COLS], uint32_t* bit, uint32_t* byte);
int cmx_pipeline_fxcm_shadow_state_diff(cmx_pipeline_t*, int a, int b, uint64_t out[CMX_FXCM_STATE_OUT]);
int cmx_pipeline_debug_fxcm_shadow_xor(cmx_pipeline_t*, int instance, int region, uint64_t index, uint32_t xor_mask);
int cmx_pipeline_mixnet_mode(cmx_pipeline_t*);
/* STREAM JOURNAL (opt-in; log2_block_bits = 0 off, the default: nothing is allocated, launched or waited for; else 6..19, 19 = the 64 KB block
 * of oracle/ref_long_trace.cpp; before the first chunk). Behind every chunk's mixing network, on the same stream, cmx_journal's kernel digests what
 * that network read and wrote -- the slot's layer-0 rows, selectors and bits and the caller's p[] -- into per-chunk partial records, which an
 * asynchronous copy brings to pinned memory; the slot is not reused before that copy has landed, and the host folds the records when the slot comes
 * round again, in cmx_pipeline_wait and in cmx_pipeline_sync. Stream bit 0 is the first submitted bit (pretraining is not journalled). Coexists
 * with _set_verify, _set_shadow, _set_ctx_shadow and _set_shadow_repair: a chunk's records are folded behind cmx_pipeline_wait's repair, and a
 * chunk whose p[] a repair replaced has its journal taken again from the replaced p first, so the journal describes the p that is coded (as repair
 * itself asks, every chunk is then waited for before its slot is reused). Not available to a handle that decodes.
 * _journal_read: *nblocks = blocks folded so far (a partial last one included; call after _sync for all of them); out (may be NULL) receives
 * records first .. first + n - 1 as cmx_journal_read does. _journal_write_files: appends the blocks folded and complete since its last call to `path`
 * and `path.inputs` (the two text files of cmx_journal_write_files, created or emptied by the first call) and flushes them; final != 0 (after
 * cmx_pipeline_sync) writes the partial last block too. */
int cmx_pipeline_set_journal(cmx_pipeline_t*, int log2_block_bits);
int cmx_pipeline_journal_read(cmx_pipeline_t*, uint64_t first, uint64_t n, uint64_t* out, uint64_t* nblocks);
int cmx_pipeline_journal_write_files(cmx_pipeline_t*, const char* path, int final);
/* STATE DIGEST and STATE JOURNAL (section "State digest" below; opt-in). _state_digest: between chunks only (a begun chunk must have been finished);
 * cmx_pipeline_sync first -- after a sync that follows the submit of chunk c every stage's state is the state after chunk c -- then every enabled
 * stage's digest in the fixed order mixnet, context, LSTM, fxcm, paq8 into out[cap]; returns the number of columns (out == NULL: only that), -1 on
 * error. The shadows' state is not digested, only the stream's own. _state_layout: per column four words -- stage (0 mixnet, 1 context, 2 LSTM,
 * 3 fxcm, 4 paq8), region, word offset inside the region, words -- into out[cap] (cap >= 4 * columns); returns the number of columns.
 * _set_state_journal (every_chunks = 0 off, the default: the handle queues exactly the launches it queues without it; before the first chunk):
 * after every every_chunks-th finished chunk one record -- the stream's byte position, then one digest per column -- is taken (a sync and a read of
 * the whole state: the chunks in flight drain first). Coexists with verify, the shadow votes, repair, the stream journal and tolerance mode.
 * _state_journal_read: *nrecords / *ncols (either may be NULL) = records taken so far / columns; out receives records first .. first + n - 1 of
 * 1 + columns words. _state_journal_write_file: from this call on every record is appended to `path` (created or emptied by the first call,
 * which also writes the header lines that carry the layout) and flushed as it is taken, so that a run killed at a time limit leaves its records;
 * final != 0 (after the last chunk) first takes the record after the last chunk if the period has not. The file: lines "# cmix_amd state journal 1",
 * "# columns N", N lines "# col k stage region offset words", then per record "<byte position> <N words of 16 hex digits>" (cmix_amd/journal.py reads
 * and compares them: python -m cmix_amd.journal state-diff a b). A handle that decodes is refused by all of them, and cmx_pipeline_late_start
 * refuses a handle whose state journal is on: the decoder's kernels are resident and its stream has no rest point. */
int cmx_pipeline_state_digest(cmx_pipeline_t*, uint64_t* out, size_t cap);
int cmx_pipeline_state_layout(cmx_pipeline_t*, uint64_t* out, size_t cap);
int cmx_pipeline_set_state_journal(cmx_pipeline_t*, int every_chunks);
int cmx_pipeline_state_journal_read(cmx_pipeline_t*, uint64_t first, uint64_t n, uint64_t* out, uint64_t* nrecords, uint64_t* ncols);
int cmx_pipeline_state_journal_write_file(cmx_pipeline_t*, const char* path, int final);
/* Predictor::Pretrain over n dictionary bytes (HOST pointer), before the first submit: only the stages holding
 * `models_` learn (today: contexts + small models); mixers, SSE, LSTM and PPMd are not trained (predictor.cpp:471-487). */
int cmx_pipeline_pretrain(cmx_pipeline_t*, const uint8_t* bytes, size_t n);
int cmx_pipeline_sync(cmx_pipeline_t*);
/* HIP-event time (ms) the last submitted chunk spent in [0] contexts+small models, [1] LSTM, [2] mixing network. */
int cmx_pipeline_last_stage_ms(cmx_pipeline_t*, float ms[3]);
/* HIP-event time of each stage (contexts, LSTM, mixing network; ms) summed over every chunk that has finished since
 * the last reset, and the number of those chunks: call after cmx_pipeline_sync(). */
int cmx_pipeline_stage_totals(cmx_pipeline_t*, double ms[3], uint64_t* chunks, int reset);

/* ------------------------------------------------------------------------
 * Stream journal: per-block digests of what the final mixing network reads and writes, in the form of the reference-side trace tools
 * (oracle/ref_long_trace.cpp, oracle/ref_ctx_trace.cpp; cmix_amd/journal.py is the numpy model):
 *   A[c] = splitmix64(c) | 1, B[i] = splitmix64(0x1000000 + i) | 1, u32(x) = the word's bit pattern; sums mod 2^64 over the bits t of a block
 *   of 2^log2_block_bits stream bits, i = t mod 2^19:
 *     words   0..129  column group g : sum_t sum_{c in [16 g, min(16 g + 16, 2078))} (u32(row[t][c]) + 1) * A[c] * B[i]
 *     word    130     final p        : sum_t (u32(p[t]) + 1) * B[i]
 *     words 131..177  selector m     : sum_t (sel[t][m] + 1) * B[i]
 *     word    178     coded bits     : sum_t (bit[t] + 1) * B[i]
 * B's index does not depend on the block size, so the records of the sub-blocks of a 64 KB block add up to the reference's line.
 * _run digests nbits rows (DEVICE pointers: d_rows [nbits][ld] f32, ld even and >= 2078, 8-byte aligned; d_sel [nbits][47]; d_bits [nbits];
 * d_p [nbits]; any of them NULL: its words are not counted) whose first is stream bit stream_bit0; consecutive calls must continue where the
 * last one ended and accumulate. One kernel behind `stream` writes the chunk's partial records, the call waits for them and folds them on the host
 * (wrapping adds). _blocks: blocks seen so far, a partial last one included. _read: n records from `first`, CMX_JOURNAL_RECORD words each: the
 * block's end byte position so far, then the 179 words.
 * cmx_journal_host_digest: the p and bits words of nbits HOST values, in plain C++ (no device): out receives, per block the range touches,
 * {end byte position, p word, bits word}; returns the number of blocks, which is (stream_bit0 + nbits - 1 >> log2) - (stream_bit0 >> log2) + 1,
 * or 0 for nbits = 0 / a bad log2.
 * ------------------------------------------------------------------------ */
#define CMX_JOURNAL_WORDS 179
#define CMX_JOURNAL_RECORD 180
typedef struct cmx_journal cmx_journal_t;
cmx_journal_t* cmx_journal_create(int device, int log2_block_bits);
int cmx_journal_run(cmx_journal_t*, const float* d_rows, size_t ld, const uint32_t* d_sel, const uint8_t* d_bits, const float* d_p, size_t nbits,
                    uint64_t stream_bit0, void* stream);
int cmx_journal_blocks(cmx_journal_t*, uint64_t* nblocks);
int cmx_journal_read(cmx_journal_t*, uint64_t first, uint64_t n, uint64_t* out);
void cmx_journal_destroy(cmx_journal_t*);
size_t cmx_journal_host_digest(const float* p, const uint8_t* bits, size_t nbits, uint64_t stream_bit0, int log2_block_bits, uint64_t* out);

/* ------------------------------------------------------------------------
 * State digest: one 64-bit word per state array of a device stage (cmix_amd/csrc/cmx_state_digest.h, state_digest.hip; cmix_amd/journal.py has the
 * numpy model). For an array of n 32-bit words w[0..n), n < 2^32:
 *     D = sum over i of splitmix64((uint64(i) << 32) | w[i])   (mod 2^64), splitmix64 as in the stream journal above
 * The sum is order-independent (a parallel kernel is deterministic); splitmix64 is a bijection, so a change of one word w -> w' always changes D, by
 * splitmix64(i, w') - splitmix64(i, w). An array of 2^32 words or more is refused (none exists today). What it is for: two runs' state, written down
 * as they go (the state journal of a pipeline / a cmx_t), compared later -- "the first thing that differs is fxcm's wx after byte N".
 * cmx_state_digest_host: the function on the CPU (HOST words). cmx_state_digest_arrays: the kernel on n DEVICE arrays (each 16-byte aligned, as every
 * hipMalloc is; words[r] 32-bit words) in ONE launch; synchronises the device before and after; out[n]. 0, or 1 on error.
 * cmx_<stage>_state_digest(handle, out, cap): synchronises, then one digest per state array of the handle, in the order of the stage's state list
 * (mixnet: regions 0..9 of cmx_mixnet_state_diff; context: the arrays cmx_ctxmodels_state_diff walks, region-then-lane; LSTM and fxcm: the arrays of
 * their _debug_layout; paq8: cmx_p8stage_debug_layout), then -- so that nothing the stage's _state_diff sees is invisible -- one last column over the
 * words it compares on the host, digested with the same function: mixnet's scalar words (region 10), the LSTM's counters bytes_done, hc, bptt_rounds
 * as six words (listed as region 11), fxcm's FxDev with its device pointers zeroed followed by bytes_done as two words (region 11); the context stage
 * has none. Returns the number of columns (out == NULL: only that; 11, the context stage's arrays, 81, 141 and paq8's count), -1 on error.
 * cmx_<stage>_state_digest_layout: per column (region, word offset inside the region's arrays laid end to end, words), three words each.
 * paq8 (it has no _state_diff; this is its state list): every table p8b::build_stage allocates, by region 0 the ContextMap family with P8FamHome,
 * 1 the three ContextMap2, 2 the lanes' learners, 3 the DMC forest, 4 the 1552 x 28 mixer, 5 tail / APM tables, 6 the image models' families, 7 the
 * image models' lanes, 8 the image models' mixer maps; then region 9: the scalar words of the role structs (P8CmDev, P8Cm2Dev x 3, P8LanesDev,
 * P8DmcDev, P8MixDev, P8TailDev, the image models' P8CmDev / P8XLanesDev / P8JpgDev) with every device address in them zeroed, digested on the host
 * (cmx_p8stage_debug_state_words reads them: out == NULL returns their number). Left out, no model state: d_x, d_order, d_prx, staging, h_mixfail,
 * d_prof, the Late slots. No table was found whose words depend on timing: two handles fed equal bytes, in one launch or in ragged ones, and a
 * handle run under poisoned LDS agree in every column (tests/test_gpu_state_digest.py).
 * NOT COVERED: the host stages' state (PPMd's arena, paq8's front end, fxcm's parser); pretraining as it runs (the first record after it covers its
 * result); the decoder.
 * ------------------------------------------------------------------------ */
uint64_t cmx_state_digest_host(const uint32_t* words, uint64_t n);
int cmx_state_digest_arrays(int device, const void* const* d_arrays, const uint64_t* words, int n, uint64_t* out);
int cmx_mixnet_state_digest(cmx_mixnet_t*, uint64_t* out, size_t cap);
int cmx_mixnet_state_digest_layout(cmx_mixnet_t*, uint64_t* out, size_t cap);
int cmx_ctxmodels_state_digest(cmx_ctxmodels_t*, uint64_t* out, size_t cap);
int cmx_ctxmodels_state_digest_layout(cmx_ctxmodels_t*, uint64_t* out, size_t cap);
int cmx_lstm_state_digest(cmx_lstm_t*, uint64_t* out, size_t cap);
int cmx_lstm_state_digest_layout(cmx_lstm_t*, uint64_t* out, size_t cap);
int cmx_fxcm_state_digest(cmx_fxcm_t*, uint64_t* out, size_t cap);
int cmx_fxcm_state_digest_layout(cmx_fxcm_t*, uint64_t* out, size_t cap);

/* ------------------------------------------------------------------------
 * Device libm probes (parity tests): evaluate the engine's expf / tanhf /
 * logistic on the device for n host floats. which: 0 expf, 1 tanhf, 2 logistic
 * ------------------------------------------------------------------------ */
int cmx_probe_libm(int device, int which, const float* x, float* y, size_t n);

/* ------------------------------------------------------------------------
 * LDS fill probe (tests only, no product path calls it): writes `pattern` over the LDS of every compute
 * unit of the device, so that the next kernel launched finds that pattern, not what its own previous launch left, in every
 * LDS word it has not written itself. Synchronises the device first, runs on the null stream and synchronises again:
 * the fill runs while no kernel of this process is resident and is complete when the call returns.
 * One workgroup of 256 threads per compute unit (floor(per-CU LDS / per-workgroup maximum) of them where a workgroup may hold
 * at most half a compute unit's LDS), each with the device's largest per-workgroup LDS; a launch counts as complete when every
 * workgroup saw all the others resident at once (two do not fit one compute unit, so they sit on all of them). Up to 8
 * launches per call, the best one is reported.
 * out: [0] workgroups that saw all others resident, [1] workgroups launched, [2] LDS bytes written per workgroup,
 *      [3] launches used, [4] compute units, [5] LDS bytes per compute unit, [6] bytes per compute unit the grid cannot reach
 *      (0 on the MI355X), [7] 0. Full coverage: out[0] == out[1] and out[6] == 0.
 * Returns 0, or -1 on a HIP error (cmx_last_error).
 * NEVER call it between cmx_pipeline_late_start and _late_stop (or any stage's late start / stop): the decoder's kernels
 * stay resident waiting for the host, and the device synchronise here would wait for them until their 30 s timeout.
 * ------------------------------------------------------------------------ */
int cmx_probe_lds_fill(int device, uint32_t pattern, uint32_t out[8]);

/* ---- 2f. The paq8 stage: layer-0 columns 434..2024 = the 1591 values PAQ8::Predict() returns per bit (replaces
 *        src/models/paq8.{h,cpp} as wired at src/predictor.cpp:85-97: PAQ8::Predict / Perceive around
 *        paq8::Predictor::update, reference src/models/paq8.cpp:8248-8362, and contextModel2 :8101-8207).
 *        One handle per stream. cmx_p8stage_run takes the NEXT nbytes bytes of the stream in HOST memory: the front end
 *        (word / text / record / XML / x86 / match parsers, cmix_amd/csrc/p8front/) runs on the calling thread, the
 *        tables, the 1552 x 28 mixer and the APM chains run as kernels ordered behind `stream`.
 *        d_out: device matrix of f32, row t (ld floats apart, ld >= 1591) receives the 1591 values valid BEFORE bit t of
 *        this chunk is coded (pass layer0 + 434 with ld = 2078 to fill the predictor's columns in place).
 *        Scope: general data and text blocks; a stream that would switch on paq8's image / audio / JPEG sub-models makes
 *        the call fail (cmx_last_error names the detector) -- never a silently different number. ~9 GB of HBM. ---- */
typedef struct cmx_p8stage cmx_p8stage_t;
cmx_p8stage_t* cmx_p8stage_create(int device);
void cmx_p8stage_destroy(cmx_p8stage_t*);
int cmx_p8stage_run(cmx_p8stage_t*, const uint8_t* bytes_host, size_t nbytes, float* d_out, size_t ld, void* stream);
int cmx_p8stage_sync(cmx_p8stage_t*);
/* HIP-event time of the role kernels summed over the chunks collected so far (a chunk is collected when its staging
 * buffer comes round again, or by _sync): ms[0] family, [1] mixer + APM chains, [2..4] ContextMap2 x 3, [5] small learners (lanes), [6] DMC forest. */
int cmx_p8stage_role_ms(cmx_p8stage_t*, double ms[7], uint64_t* chunks, int reset);
int cmx_p8stage_set_upload_stream(cmx_p8stage_t*, void* stream);   /* see cmx_mixnet_set_upload_stream */
/* diagnostics (CMX_P8FAM_PROFILE=1 at create time): the family kernel's clocks by bit position and phase, and how often it left the
 * common path: out[8 bp + k] (k = 0 per-step values, 1 phase 1, 2 barrier, 3 run / rounds, 4 rest), out[64 + bp] steps in rounds,
 * out[72 + bp] instances walked, out[80 + bp] steps */
int cmx_p8stage_profile(cmx_p8stage_t*, unsigned long long out128[128]);
/* the stage's state digest, its layout and the scalar words of its last column (section "State digest" above) */
int cmx_p8stage_state_digest(cmx_p8stage_t*, uint64_t* out, size_t cap);
int cmx_p8stage_debug_layout(cmx_p8stage_t*, uint64_t* out, size_t cap);
int cmx_p8stage_debug_state_words(cmx_p8stage_t*, uint32_t* out, size_t cap);


/* ------------------------------------------------------------------------
 * 4. The DECODER's form of the stages: the late-bit protocol (cmix_amd/csrc/cmx_late.h)
 *
 * Decoder::Decode (src/coder/decoder.cpp:20-39) learns bit t only after Predictor::Predict() has returned p(t): nothing can be
 * looked ahead. The stage kernels are the chunk kernels of section 3, but each waits where it reads a coded bit, a host record or
 * another stage's row: they are launched for a chunk of bytes that do not exist yet, and a BOX in host-coherent memory carries the
 * bits in (with each bit: the host records of the step after it) and p out. cmx_pipeline_late_* below drive one stream this way --
 * every model family on the device, no column from the caller, no reference object; cmx_predict()/cmx_perceive() of section 1 sit
 * on top of them when no input was staged. The per-stage entry points are what the pipeline (and the stage-level tests) call.
 * ------------------------------------------------------------------------ */
void* cmx_late_alloc(size_t bytes);   /* zeroed host-coherent pinned memory: boxes, rows, records */
void cmx_late_free(void* p);
void* cmx_late_alloc_dev(int device, size_t bytes);   /* zeroed UNCACHED device memory: rows / row counters kernels hand to each other while they run */
void cmx_late_free_dev(void* p);
size_t cmx_late_box_bytes(size_t nbits);   /* allocation size of a box for a chunk of nbits */
/* `box` of the per-stage entry points below: a `const CmxLate*` (cmx_late.h) = the host box, the chunk's row counters and their base */
int cmx_ctxmodels_run_late(cmx_ctxmodels_t*, void* box, size_t nbytes, float* probs, size_t pstride, uint32_t* sel, float* brk_dist,
                           const float** brk_dist0_out, void* stream);
int cmx_bytemodel_late_run(int device, void* box, size_t nbytes, const float* brk0, const float* brk, const float* ppmd, const float* lstm0, const float* lstm,
                           const uint32_t* c0_brk, uint32_t c0_brk_want, const uint32_t* c0_lstm, uint32_t c0_lstm_want, float* layer0, size_t pstride,
                           int16_t* hint_pr, uint8_t* hint_ex, uint8_t* dbit0, const void* relay_dev, int nrelay, void* stream);
/* what a stage's records need from the stream's relay wave (an array of cmx_late_relay_t, cmx_late.h); returns the number of entries, -1 on error */
int cmx_p8stage_late_relay(cmx_p8stage_t*, int slot, void* out, int max);
int cmx_fxcm_late_relay(cmx_fxcm_t*, int slot, void* out, int max);
const float* cmx_lstm_byte_probs(cmx_lstm_t*);
/* _late_prepare: everything a stage allocates for chunks of that size, BEFORE the stream's first kernels are launched (an allocation
 * that maps memory into the device can wait for running kernels -- which, here, wait for the host) */
int cmx_fxcm_late_prepare(cmx_fxcm_t*, size_t nbytes);
int cmx_p8stage_late_prepare(cmx_p8stage_t*, size_t nbytes);
int cmx_mixnet_late_prepare(cmx_mixnet_t*, size_t nbits);
int cmx_fxcm_run_late(cmx_fxcm_t*, void* box, size_t nbytes, const int16_t* hint_pr, const uint8_t* hint_ex, float* probs, size_t pstride, int slot, void* stream);
int cmx_fxcm_late_byte(cmx_fxcm_t*, int slot, size_t b, uint8_t byte);
int cmx_p8stage_run_late(cmx_p8stage_t*, void* box, size_t nbytes, float* out, size_t ld, int slot);
int cmx_p8stage_late_emit(cmx_p8stage_t*, int slot, size_t step);
int cmx_p8stage_late_bit(cmx_p8stage_t*, int bit);
int cmx_p8stage_mixfail(cmx_p8stage_t*);
/* test hook: the counter of the ContextMap family's shared generator (paq8.cpp:152-165: `int i`, only i mod 64 matters), a multiple of 64, before the
 * first byte -- so that a test passes 2^31 / 2^32 draws (4 / 8 MB into a stream) within a few KB */
int cmx_p8stage_set_generator_counter(cmx_p8stage_t*, uint32_t counter);
/* test hook (state injection): the front end's byte position `pos` (paq8.cpp:167: the index into the 2^30-byte history ring at level 11), before the first
 * byte -- a test passes the ring's end, which a stream reaches after 1 GB, within a few KB */
int cmx_p8stage_debug_set_pos(cmx_p8stage_t*, int pos);
int cmx_mixnet_run_late(cmx_mixnet_t*, void* box, const float* probs, const uint32_t* sel, size_t nbits, void* stream);
/* the LSTM byte mixer in a decoder's chunk (round 6): one forward launch for the bytes b0 .. up to the end of the truncated-BPTT block or of the chunk -- its steps
 * wait for their bytes inside the launch and count the distributions they write (LC_LSTM); returns the number of bytes covered, -1 on error */
int cmx_lstm_run_late(cmx_lstm_t*, const void* late_box, const float* d_ppmd, const float* h_ppmd, const uint8_t* h_bytes, float* d_out, size_t b0, size_t nchunk, void* stream);
/* One stream, bit by bit. The handle is a pipeline of section 3 with the fxcm and paq8 stages enabled (and, if there is a
 * dictionary, pretrained): cmx_pipeline_late_start() launches the first chunks' kernels (last_bit: the bit coded before the first
 * one -- the last Pretrain bit, else 0); then strictly alternating cmx_pipeline_late_predict() -> p, cmx_pipeline_late_perceive(bit).
 * cmx_pipeline_late_stop() (also called by cmx_pipeline_destroy) unwinds the kernels of the chunk in progress. */
int cmx_pipeline_late_start(cmx_pipeline_t*, int last_bit);
float cmx_pipeline_late_predict(cmx_pipeline_t*);
int cmx_pipeline_late_perceive(cmx_pipeline_t*, int bit);
int cmx_pipeline_late_stop(cmx_pipeline_t*);
/* predict / perceive for n known bits in one call (a decoder minus the arithmetic decoder): p_out[i] = p before bits[i] */
int cmx_pipeline_late_replay(cmx_pipeline_t*, const uint8_t* bits, size_t n, float* p_out);
/* diagnostics: the calling thread's wall time since start, in ms: [0] waiting for p, [1] PPMd, [2] paq8 front end, [3] fxcm parser, [4] LSTM launches, [5] chunk launches */
int cmx_pipeline_late_host_ms(cmx_pipeline_t*, double ms[6], uint64_t* bits);
/* diagnostics: every row counter of the chunk being decoded and the device time (100 MHz) it was last moved at: out[2 i], out[2 i + 1] for
 * counter i of cmx_late.h (14 = the relay's); out[30..39] the mixing network's stamps of the current bit. Call between predict() and perceive(). */
int cmx_pipeline_late_debug_times(cmx_pipeline_t*, uint32_t out[48]);
/* test hook: the layer-0 row (2078 f32, host memory) and 47 selectors of the bit predicted last; valid until the matching perceive */
const float* cmx_pipeline_late_debug_row(cmx_pipeline_t*, const uint32_t** sel);
/* test hooks (CMX_LATE_DEBUG=1 in the environment when the handle is built): the 47 Mixer::Mix values of the bit BEFORE the one predicted last */
int cmx_pipeline_late_debug_mix(cmx_pipeline_t*, float out47[47]);
const float* cmx_mixnet_late_debug_mix(cmx_mixnet_t*, uint64_t chunk, size_t bit);
uint64_t cmx_mixnet_runs(cmx_mixnet_t*);

#ifdef __cplusplus
}
#endif
#endif /* CMIX_AMD_H */
