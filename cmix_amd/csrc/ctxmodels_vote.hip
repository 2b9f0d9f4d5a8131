// ctxmodels_vote.hip -- the redundant context-stage vote (C ABI: cmx_ctxvote_*, cmx_ctxmodels_state_diff, cmx_ctxmodels_debug_state_xor,
// cmx_ctxmodels_debug_layout in include/cmix_amd.h).
//
// The context stage (ctxmodels_kernels.hip) is the only producer of the 47 mixer selectors and writes 54 of the layer-0 columns. Verify mode compares
// the mixing network's copy of those words with the slot they came from, and the network's own vote (mixnet_vote.hip) runs every instance on the same
// slot: a word the PRODUCER got wrong passes both. The guard here is the one the network has: the unchanged cmx_ctxmodels_kernel runs on two or three
// handles over the same bytes, and two kernels compare what they produced. The rule, the record and the handle's plumbing: cmx_vote_core.h.
//
//   cmx_rowvote_kernel<CtxRow> every chunk: the 54 model outputs and 47 selectors of every bit of n = 2 or 3 instances, word for word; one wavefront
//                             per row (a full-stride row's columns 2025..2075 and a row's selectors are consecutive words: coalesced, no LDS)
//   cmx_ctxvote_fold_kernel   behind it: folds the chunk's result into a sticky record and captures the first differing bit
//   cmx_state_diff_kernel     after an event (and in tests): every word of two handles' state arrays in HBM
//
// Out of scope: repairing an outvoted instance from the majority (the pipeline stops at the first event), the other producers of a slot (fxcm, paq8,
// LSTM, PPMd), the bit and decay words, and the decoder's form of the stage.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string>

#include "../../include/cmix_amd.h"
#include "cmx_vote_core.h"
#include "cmx_state_digest.h"
#include "ctxmodels_state.h"

extern "C" int cmx_ctxmodels_state_view(cmx_ctxmodels_t* h, const CtxRegion** regions, int* n, int* device);   // ctxmodels_api.hip

namespace {
constexpr unsigned long long kNone = ~0ull;
constexpr int kCols = CMX_CTXVOTE_COLS;   // 54 model outputs in lane order, then the 47 selectors
static_assert(kCols == CTX_NM + CTX_NSEL, "the vote's row is the stage's 54 model outputs and 47 selectors");

struct CtxVoteArgs {
  const uint32_t* probs[3];
  const uint32_t* sel[3];
  unsigned long long pstride[3];
  int compact[3];
};
// device block of a vote handle
struct CtxVoteDev {
  VoteHead head;
  uint32_t words[3 * kCols];     // capture of the first event's bit: instance i, element c at [i * 101 + c]
  uint32_t bit;
};
// A row is two passes of the wave: elements 0..63 and 64..100 (a full-stride row's columns 2025..2075 and a row's selectors are consecutive words).
struct CtxRow {
  typedef CtxVoteArgs Args;
  static constexpr int kCols = ::kCols;
  // element c (< 101) of row t of instance i
  static __device__ __forceinline__ uint32_t word(const CtxVoteArgs& a, int i, unsigned long long t, unsigned c) {
    if (c >= CTX_NM) return a.sel[i][t * CTX_NSEL + (c - CTX_NM)];
    const unsigned col = a.compact[i] || c < 3 ? c : 2022 + c;   // lane order: layer-0 columns 0, 1, 2, 2025..2075
    return a.probs[i][t * a.pstride[i] + col];
  }
};

// behind the vote kernel: the core's fold, and the first event's bit is captured
__global__ void cmx_ctxvote_fold_kernel(CtxVoteArgs a, unsigned long long nrows, unsigned long long bit0, int n, const uint8_t* bits, CtxVoteDev* d) {
  const VoteEvent ev = cmx_vote_fold(&d->head, nrows, bit0, n, kCols);
  if (!ev.capture) return;
  cmx_vote_capture<CtxRow>(a, n, ev.row, d->words);
  if (threadIdx.x == 0) d->bit = bits ? bits[ev.row] : 0u;
}

// the handle's state arrays as the core's
int ctx_arrays(cmx_ctxmodels_t* h, std::vector<StateArray>& a, int* device) {
  const CtxRegion* rg = nullptr; int n = 0;
  if (cmx_ctxmodels_state_view(h, &rg, &n, device)) return 1;
  a = state_arrays(rg, n);
  for (int r = 0; r < n; ++r) a[r].lane = rg[r].lane;
  return 0;
}
}  // namespace

struct cmx_ctxvote : VoteHandle {};

extern "C" {

cmx_ctxvote_t* cmx_ctxvote_create(int device, int n) { return vote_create<cmx_ctxvote>("cmx_ctxvote_create", device, n, sizeof(CtxVoteDev)); }
void cmx_ctxvote_destroy(cmx_ctxvote_t* v) { vote_destroy(v); }

int cmx_ctxvote_run(cmx_ctxvote_t* v, const float* const* d_probs, const size_t* pstride, const int* compact, const uint32_t* const* d_sel, size_t nbits,
                    uint64_t stream_bit0, const uint8_t* d_bits, void* stream) {
  if (!v || !d_probs || !pstride || !compact || !d_sel) { cmx_set_err("cmx_ctxvote_run: bad argument"); return 1; }
  if (nbits == 0) return 0;
  if (nbits > 0x7fffffff) { cmx_set_err("cmx_ctxvote_run: chunk too large"); return 1; }
  CtxVoteArgs a;
  memset(&a, 0, sizeof a);
  for (int i = 0; i < v->n; ++i) {
    if (!d_probs[i] || !d_sel[i]) { cmx_set_err("cmx_ctxvote_run: null array of instance " + std::to_string(i)); return 1; }
    if (pstride[i] < (compact[i] ? (size_t)CMX_CTX_COMPACT_STRIDE : (size_t)CMX_N_INPUTS)) {
      cmx_set_err("cmx_ctxvote_run: pstride of instance " + std::to_string(i) + " is below " + (compact[i] ? "64 (compact)" : "2078 (full)")); return 1;
    }
    a.probs[i] = (const uint32_t*)d_probs[i]; a.sel[i] = d_sel[i]; a.pstride[i] = pstride[i]; a.compact[i] = compact[i] != 0;
  }
  if (hipSetDevice(v->device) != hipSuccess) { cmx_set_err("hipSetDevice failed"); return 1; }
  hipStream_t st = (hipStream_t)stream;
  const unsigned long long nrows = nbits;
  if (v->n == 3) hipLaunchKernelGGL((cmx_rowvote_kernel<3, CtxRow>), dim3(vote_row_grid(nrows)), dim3(256), 0, st, a, nrows, v->d);
  else hipLaunchKernelGGL((cmx_rowvote_kernel<2, CtxRow>), dim3(vote_row_grid(nrows)), dim3(256), 0, st, a, nrows, v->d);
  hipLaunchKernelGGL(cmx_ctxvote_fold_kernel, dim3(1), dim3(64), 0, st, a, nrows, (unsigned long long)stream_bit0, v->n, d_bits, (CtxVoteDev*)v->d);
  if (hipGetLastError() != hipSuccess) { cmx_set_err("cmx_ctxvote_run: kernel launch failed"); return 1; }
  return 0;
}

const unsigned long long* cmx_ctxvote_record(cmx_ctxvote_t* v) { return v && v->d ? v->d->rec : nullptr; }

int cmx_ctxvote_report(cmx_ctxvote_t* v, uint64_t out[8]) { return vote_report("cmx_ctxvote_report", v, out); }
int cmx_ctxvote_last(cmx_ctxvote_t* v, uint64_t out[4]) { return vote_last("cmx_ctxvote_last", v, out); }

int cmx_ctxvote_values(cmx_ctxvote_t* v, uint32_t words[3 * CMX_CTXVOTE_COLS], uint32_t* bit) {
  CtxVoteDev h;
  if (vote_values("cmx_ctxvote_values", v, words, &h)) return 1;
  memcpy(words, h.words, sizeof h.words);
  if (bit) *bit = h.bit;
  return 0;
}

int cmx_ctxmodels_state_diff(cmx_ctxmodels_t* a, cmx_ctxmodels_t* b, uint64_t out[16]) {
  if (!a || !b || !out) { cmx_set_err("cmx_ctxmodels_state_diff: bad argument"); return 1; }
  if (a == b) { cmx_set_err("cmx_ctxmodels_state_diff: a and b are the same handle"); return 1; }
  std::vector<StateArray> ra, rb; int deva = 0, devb = 0;
  if (ctx_arrays(a, ra, &deva) || ctx_arrays(b, rb, &devb)) return 1;
  const int na = (int)ra.size();
  if (deva != devb) { cmx_set_err("cmx_ctxmodels_state_diff: the two handles live on different devices"); return 1; }
  if (ra.size() != rb.size()) { cmx_set_err("cmx_ctxmodels_state_diff: internal layout error"); return 1; }
  if (hipSetDevice(deva) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { cmx_set_err("cmx_ctxmodels_state_diff: device error"); return 1; }
  std::vector<DiffDev> h(ra.size());
  bool ok = state_diff_arrays(ra.data(), rb.data(), na, 4096, h.data());
  for (int i = 0; i < 16; ++i) out[i] = 0;
  for (int i = 1; i <= 5; ++i) out[i] = kNone;
  for (int r = 0; ok && r < na; ++r) {   // (region-then-lane order)
    if (!h[r].cnt) continue;
    out[0] += h[r].cnt; out[6 + ra[r].region] += h[r].cnt;
    if (ra[r].lane >= 0) out[15] |= 1ull << ra[r].lane;
    if (out[1] == kNone) {
      uint32_t x = 0, y = 0;
      ok = state_fetch_pair(ra[r], rb[r], h[r].first, &x, &y);
      out[1] = (uint64_t)ra[r].region; out[2] = ra[r].lane >= 0 ? (uint64_t)ra[r].lane : kNone; out[3] = h[r].first; out[4] = x; out[5] = y;
    }
  }
  if (!ok) { (void)hipGetLastError(); cmx_set_err("cmx_ctxmodels_state_diff: device error"); return 1; }
  return 0;
}

// one column per array of the state view (region-then-lane order); the stage compares nothing on the host
static int ctx_digest(const char* who, cmx_ctxmodels_t* h, uint64_t* out, size_t cap, int layout) {
  if (!h) { cmx_set_err(std::string(who) + ": null handle"); return -1; }
  std::vector<StateArray> rg; int dev = 0;
  if (ctx_arrays(h, rg, &dev)) return -1;
  return cmx_state_digest_stage(who, dev, rg.data(), (int)rg.size(), nullptr, 0, out, cap, layout);
}
int cmx_ctxmodels_state_digest(cmx_ctxmodels_t* h, uint64_t* out, size_t cap) { return ctx_digest("cmx_ctxmodels_state_digest", h, out, cap, 0); }
int cmx_ctxmodels_state_digest_layout(cmx_ctxmodels_t* h, uint64_t* out, size_t cap) { return ctx_digest("cmx_ctxmodels_state_digest_layout", h, out, cap, 1); }

int cmx_ctxmodels_debug_state_xor(cmx_ctxmodels_t* h, int region, uint64_t lane, uint64_t index, uint32_t xor_mask) {
  if (!h) { cmx_set_err("cmx_ctxmodels_debug_state_xor: null handle"); return 1; }
  if (!xor_mask) { cmx_set_err("cmx_ctxmodels_debug_state_xor: a zero mask changes nothing"); return 1; }
  std::vector<StateArray> rg; int dev = 0;
  if (ctx_arrays(h, rg, &dev)) return 1;
  uint32_t* p = nullptr;
  for (size_t r = 0; r < rg.size() && !p; ++r)
    if (rg[r].region == region && (rg[r].lane < 0 ? lane == kNone : lane == (uint64_t)rg[r].lane) && index < rg[r].words) p = rg[r].p + index;
  if (!p) { cmx_set_err("cmx_ctxmodels_debug_state_xor: no such word (region, lane, index out of range)"); return 1; }
  return state_xor("cmx_ctxmodels_debug_state_xor", dev, p, xor_mask);
}

int cmx_ctxmodels_debug_layout(uint64_t out[5]) {
  if (!out) { cmx_set_err("cmx_ctxmodels_debug_layout: bad argument"); return 1; }
  out[0] = offsetof(CtxPersist, regs) / 4; out[1] = offsetof(CtxPersist, br_probs) / 4; out[2] = offsetof(CtxPersist, ipred) / 4;
  out[3] = offsetof(CtxPersist, mpred) / 4; out[4] = sizeof(CtxPersist) / 4;
  return 0;
}

}  // extern "C"
