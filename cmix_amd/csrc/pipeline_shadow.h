// pipeline_shadow.h -- the pipeline's shadow stages (include/cmix_amd.h, cmx_pipeline_set_shadow and its three kin): one or two redundant copies of a
// stage run every chunk again on streams of their own, and a vote compares what all instances wrote. The four kinds -- mixing network, context stage,
// LSTM stage, fxcm -- are one mechanism (pipeline_api.hip: shadow_set, shadow_build, shadow_chunk, shadow_drop, ...) driven by the table below.
// Host only.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cmx_shadow_text.h"

struct cmx_pipeline;

// What differs between the kinds. Handles travel as void*: every kind has a stage type and a vote type of its own.
struct ShadowKind {
  ShadowId id;
  int wgs;                 // workgroups one shadow keeps resident (wg_claim)
  int stream_flag;         // cmx_make_stream's: the mixing network's streams are made like s_mix
  int probe_cap;           // the overlap probe lists this kind's streams while it holds fewer than this many
  bool strict;             // the vote compares strict kernels: refused beside the tolerance switch
  bool needs_fxcm;         // only with the fxcm stage on the device
  const char* pretrained;  // why it is refused after cmx_pipeline_pretrain (NULL: the stage is not pretrained) ...
  bool pretrained_first;   // ... said before the device is touched (fxcm) or behind the "k is what it was" return (context stage)
  bool diff_idle;          // _state_diff between chunks only (fxcm's state is only at rest there)
  int rec_words;           // the slot's pinned record: 12 words (the vote's record, the chunk's own result), 14 with the shadows' two sticky hand-off flags behind
  const char* alloc_fail;  // what a failed buffer allocation says
  void* (*own)(cmx_pipeline*);        // instance 0: the stream's own stage
  void* (*create)(cmx_pipeline*);     // a shadow's handle (NULL: it has said why)
  void (*destroy)(void*);
  const void* (*fail_flag)(void*);    // DEVICE address of a handle's sticky hand-off word (NULL: the context stage is one workgroup)
  int (*check)(void*);                // cmx_pipeline_sync's look at a shadow: 0 fine, 1 failed and said why, 2 a hand-off timed out
  int (*state_diff)(void*, void*, uint64_t*);
  void* (*vote_create)(int device, int n);
  void (*vote_destroy)(void*);
  int (*report)(void*, uint64_t out[8]);
  const unsigned long long* (*record)(void*);
  void (*sizes)(size_t max_chunk, size_t per_shadow[3], size_t* own);   // bytes of a slot's device buffers: up to three per shadow, one for instance 0
};

// A handle's shadows of one kind (k = 0: off, nothing below exists)
struct ShadowSet {
  int k = 0;
  hipStream_t q[2] = {nullptr, nullptr};      // their streams (from the factory, at the set call: the queue budget refuses there)
  void* inst[2] = {nullptr, nullptr};         // their handles, created at the first chunk (or pretrain)
  void* vote = nullptr;
  uint64_t units = 0;                         // stream bits (LSTM: bytes) handed to the vote so far
  float* d_scratch[2] = {nullptr, nullptr};   // fxcm: pretraining writes each shadow's (discarded) rows here
};

// ... and what one slot holds for them
struct ShadowSlot {
  void* d[2][3] = {};          // device buffers of shadow i + 1 (ShadowKind::sizes)
  void* d_own = nullptr;       // instance 0's buffer in the same form (mixing network: its 47 mixer outputs per bit, unless cmx_pipeline_debug_mix_out supplies the area)
  uint64_t* rec = nullptr;     // pinned: [8] the vote's record as it stood behind this chunk, [4] the chunk's own result, then the hand-off flags
  hipEvent_t ev[2] = {nullptr, nullptr}, ev_vote = nullptr;
  bool voted = false;          // this slot's chunk has a vote behind it: slot_done waits for ev_vote too
};
