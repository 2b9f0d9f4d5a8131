// lstm_vote.hip -- the redundant LSTM-stage vote (C ABI: cmx_lstmvote_*, cmx_lstm_state_diff, cmx_lstm_debug_state_xor, cmx_lstm_debug_layout in
// include/cmix_amd.h).
//
// The LSTM byte mixer (lstm_block.hip) writes layer-0 column 2077 and, through lstmpr / lstmex, steers fxcm's mixer selection and APMs; its state
// learns online, so one wrong word in a gate matrix changes every later distribution. Its block kernels hand values between 52 workgroups inside a
// launch behind counters and have no host form. Verify mode, the network's vote and the context vote all take the column as given. The guard here is
// the one those stages have: the unchanged cmx_lstm_run runs on two or three handles over the same bytes and the same PPMd distributions, and two
// kernels compare what they produced. The rule, the record and the handle's plumbing: cmx_vote_core.h.
//
//   cmx_rowvote_kernel<LstmRow> every chunk: the distribution after every byte (256 words), the byte's eight bit predictions and eight `ex` words of
//                              n = 2 or 3 instances, word for word; one wavefront per byte (a row's 256 distribution words are consecutive:
//                              coalesced; the eight strided words of an instance read in place from layer-0 rows go to eight lanes; no LDS)
//   cmx_lstmvote_fold_kernel   behind it: folds the chunk's result into a sticky record and captures the first differing byte's row
//   cmx_state_diff_kernel      after an event (and in tests): every word of two handles' state arrays in HBM
//
// Out of scope: REPAIR (what the LSTM wrote has been consumed on the device by fxcm and the network before the host sees the vote: the pipeline stops
// at the first event), the other producers of a slot (fxcm, paq8, PPMd), PPMd's distributions and the bytes (shared by all instances), the decoder's
// form of the stage.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string>

#include "../../include/cmix_amd.h"
#include "cmx_vote_core.h"
#include "cmx_state_digest.h"
#include "lstm_state.h"

extern "C" int cmx_lstm_state_view(cmx_lstm_t* h, LstmRegion* out, int* n, int* device, uint64_t counters[3]);   // lstm_api.hip

namespace {
constexpr unsigned long long kNone = ~0ull;
constexpr int kCols = CMX_LSTMVOTE_COLS;   // 256 distribution words, 8 bit predictions, 8 `ex`
static_assert(kCols == LSTM_VP + 16, "the vote's row is a byte's distribution, its eight bit predictions and its eight ex words");
static_assert(CMX_LSTM_STATE_REGIONS == LSTM_REGIONS && CMX_LSTM_STATE_ARRAYS == LSTM_STATE_ARRAYS, "region and array counts of the header and of lstm_state.h");

struct LstmVoteArgs {
  const uint32_t* dist[3];       // [N][256]
  const uint32_t* bitp[3];       // bit k of byte b at [(8 b + k) * pstride]
  const uint32_t* ex[3];         // [N][8]
  unsigned long long pstride[3];
};
// device block of a vote handle
struct LstmVoteDev {
  VoteHead head;
  uint32_t words[3 * kCols];     // capture of the first event's byte: instance i, element c at [i * 272 + c]
  uint32_t byte;
};
// A row is five passes of the wave: four over the distribution, one in which lanes 0..7 take the bit predictions and lanes 8..15 the ex words.
struct LstmRow {
  typedef LstmVoteArgs Args;
  static constexpr int kCols = ::kCols;
  // element c (< 272) of byte b of instance i
  static __device__ __forceinline__ uint32_t word(const LstmVoteArgs& a, int i, unsigned long long b, unsigned c) {
    if (c < LSTM_VP) return a.dist[i][b * LSTM_VP + c];
    if (c < LSTM_VP + 8) return a.bitp[i][(b * 8 + (c - LSTM_VP)) * a.pstride[i]];
    return a.ex[i][b * 8 + (c - LSTM_VP - 8)];
  }
};

// behind the vote kernel: the core's fold, and the first event's byte's row is captured
__global__ void cmx_lstmvote_fold_kernel(LstmVoteArgs a, unsigned long long nrows, unsigned long long byte0, int n, const uint8_t* bytes, LstmVoteDev* d) {
  const VoteEvent ev = cmx_vote_fold(&d->head, nrows, byte0, n, kCols);
  if (!ev.capture) return;
  cmx_vote_capture<LstmRow>(a, n, ev.row, d->words);
  if (threadIdx.x == 0) d->byte = bytes ? bytes[ev.row] : 0u;
}

constexpr int kIndexRegion = 9;   // input_history, bp_symbol, dyn: words the kernels use as indices

// the handle's state arrays as the core's
int lstm_arrays(cmx_lstm_t* h, std::vector<StateArray>& a, int* device, uint64_t counters[3]) {
  LstmRegion rg[LSTM_STATE_ARRAYS]; int n = 0;
  if (cmx_lstm_state_view(h, rg, &n, device, counters)) return 1;
  a = state_arrays(rg, n);
  return 0;
}
}  // namespace

struct cmx_lstmvote : VoteHandle {};

extern "C" {

cmx_lstmvote_t* cmx_lstmvote_create(int device, int n) { return vote_create<cmx_lstmvote>("cmx_lstmvote_create", device, n, sizeof(LstmVoteDev)); }
void cmx_lstmvote_destroy(cmx_lstmvote_t* v) { vote_destroy(v); }

int cmx_lstmvote_run(cmx_lstmvote_t* v, const float* const* d_dist, const float* const* d_bit_p, const size_t* pstride, const int* const* d_bit_ex, size_t nbytes,
                     uint64_t stream_byte0, const uint8_t* d_bytes, void* stream) {
  if (!v || !d_dist || !d_bit_p || !pstride || !d_bit_ex) { cmx_set_err("cmx_lstmvote_run: bad argument"); return 1; }
  if (nbytes == 0) return 0;
  if (nbytes > 0x0fffffff) { cmx_set_err("cmx_lstmvote_run: chunk too large"); return 1; }
  LstmVoteArgs a;
  memset(&a, 0, sizeof a);
  for (int i = 0; i < v->n; ++i) {
    if (!d_dist[i] || !d_bit_p[i] || !d_bit_ex[i]) { cmx_set_err("cmx_lstmvote_run: null array of instance " + std::to_string(i)); return 1; }
    if (pstride[i] < 1) { cmx_set_err("cmx_lstmvote_run: pstride of instance " + std::to_string(i) + " is 0 (1 = a dense array, 2078 = column 2077 of layer-0 rows in place)"); return 1; }
    a.dist[i] = (const uint32_t*)d_dist[i]; a.bitp[i] = (const uint32_t*)d_bit_p[i]; a.ex[i] = (const uint32_t*)d_bit_ex[i]; a.pstride[i] = pstride[i];
  }
  if (hipSetDevice(v->device) != hipSuccess) { cmx_set_err("hipSetDevice failed"); return 1; }
  hipStream_t st = (hipStream_t)stream;
  const unsigned long long nrows = nbytes;
  if (v->n == 3) hipLaunchKernelGGL((cmx_rowvote_kernel<3, LstmRow>), dim3(vote_row_grid(nrows)), dim3(256), 0, st, a, nrows, v->d);
  else hipLaunchKernelGGL((cmx_rowvote_kernel<2, LstmRow>), dim3(vote_row_grid(nrows)), dim3(256), 0, st, a, nrows, v->d);
  hipLaunchKernelGGL(cmx_lstmvote_fold_kernel, dim3(1), dim3(64), 0, st, a, nrows, (unsigned long long)stream_byte0, v->n, d_bytes, (LstmVoteDev*)v->d);
  if (hipGetLastError() != hipSuccess) { cmx_set_err("cmx_lstmvote_run: kernel launch failed"); return 1; }
  return 0;
}

const unsigned long long* cmx_lstmvote_record(cmx_lstmvote_t* v) { return v && v->d ? v->d->rec : nullptr; }

int cmx_lstmvote_report(cmx_lstmvote_t* v, uint64_t out[8]) { return vote_report("cmx_lstmvote_report", v, out); }
int cmx_lstmvote_last(cmx_lstmvote_t* v, uint64_t out[4]) { return vote_last("cmx_lstmvote_last", v, out); }

int cmx_lstmvote_values(cmx_lstmvote_t* v, uint32_t words[3 * CMX_LSTMVOTE_COLS], uint32_t* byte) {
  LstmVoteDev h;
  if (vote_values("cmx_lstmvote_values", v, words, &h)) return 1;
  memcpy(words, h.words, sizeof h.words);
  if (byte) *byte = h.byte;
  return 0;
}

int cmx_lstm_state_diff(cmx_lstm_t* a, cmx_lstm_t* b, uint64_t out[16]) {
  if (!a || !b || !out) { cmx_set_err("cmx_lstm_state_diff: bad argument"); return 1; }
  if (a == b) { cmx_set_err("cmx_lstm_state_diff: a and b are the same handle"); return 1; }
  std::vector<StateArray> ra, rb; int deva = 0, devb = 0;
  uint64_t ca[3], cb[3];
  if (lstm_arrays(a, ra, &deva, ca) || lstm_arrays(b, rb, &devb, cb)) return 1;
  const int na = (int)ra.size();
  if (deva != devb) { cmx_set_err("cmx_lstm_state_diff: the two handles live on different devices"); return 1; }
  if (cmx_lstm_vocab_size(a) != cmx_lstm_vocab_size(b)) { cmx_set_err("cmx_lstm_state_diff: the two handles have different vocabulary sizes"); return 1; }
  static const char* const kCounter[3] = {"bytes_done", "hc", "bptt_rounds"};
  for (int i = 0; i < 3; ++i)
    if (ca[i] != cb[i]) {
      cmx_set_err(std::string("cmx_lstm_state_diff: the host-side counter ") + kCounter[i] + " differs: " + std::to_string(ca[i]) + " and " + std::to_string(cb[i]));
      return 1;
    }
  if (hipSetDevice(deva) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { cmx_set_err("cmx_lstm_state_diff: device error"); return 1; }
  std::vector<DiffDev> h(ra.size());
  bool ok = ra.size() == rb.size() && state_diff_arrays(ra.data(), rb.data(), na, 1024, h.data());
  for (int i = 0; i < 16; ++i) out[i] = 0;
  for (int i = 1; i <= 4; ++i) out[i] = kNone;
  for (int r = 0; ok && r < na; ++r) {   // (region-then-array order)
    if (!h[r].cnt) continue;
    out[0] += h[r].cnt; out[5 + ra[r].region] += h[r].cnt;
    if (out[1] == kNone) {
      uint32_t x = 0, y = 0;
      ok = state_fetch_pair(ra[r], rb[r], h[r].first, &x, &y);
      out[1] = (uint64_t)ra[r].region; out[2] = state_offset(ra.data(), r) + h[r].first; out[3] = x; out[4] = y;
    }
  }
  if (!ok) { (void)hipGetLastError(); cmx_set_err("cmx_lstm_state_diff: device error"); return 1; }
  return 0;
}

// one column per array of the state view, then the three host-side counters (bytes_done, hc, bptt_rounds; two words each) as region 11
static int lstm_digest(const char* who, cmx_lstm_t* h, uint64_t* out, size_t cap, int layout) {
  if (!h) { cmx_set_err(std::string(who) + ": null handle"); return -1; }
  std::vector<StateArray> rg; int dev = 0;
  uint64_t c[3] = {0, 0, 0};
  if (lstm_arrays(h, rg, &dev, c)) return -1;
  std::vector<uint32_t> w(6);
  memcpy(w.data(), c, sizeof c);
  return cmx_state_digest_stage(who, dev, rg.data(), (int)rg.size(), &w, CMX_LSTM_STATE_REGIONS, out, cap, layout);
}
int cmx_lstm_state_digest(cmx_lstm_t* h, uint64_t* out, size_t cap) { return lstm_digest("cmx_lstm_state_digest", h, out, cap, 0); }
int cmx_lstm_state_digest_layout(cmx_lstm_t* h, uint64_t* out, size_t cap) { return lstm_digest("cmx_lstm_state_digest_layout", h, out, cap, 1); }

int cmx_lstm_debug_state_xor(cmx_lstm_t* h, int region, uint64_t index, uint32_t xor_mask) {
  if (!h) { cmx_set_err("cmx_lstm_debug_state_xor: null handle"); return 1; }
  if (!xor_mask) { cmx_set_err("cmx_lstm_debug_state_xor: a zero mask changes nothing"); return 1; }
  if (region == kIndexRegion) {
    cmx_set_err("cmx_lstm_debug_state_xor: region 9 (input_history, bp_symbol, dyn) holds indices the kernels address memory with: refused (the hook changes values only)");
    return 1;
  }
  std::vector<StateArray> rg; int dev = 0;
  if (lstm_arrays(h, rg, &dev, nullptr)) return 1;
  uint32_t* p = state_word(rg.data(), (int)rg.size(), region, index);
  if (!p) { cmx_set_err("cmx_lstm_debug_state_xor: no such word (region, index out of range)"); return 1; }
  return state_xor("cmx_lstm_debug_state_xor", dev, p, xor_mask);
}

int cmx_lstm_debug_layout(cmx_lstm_t* h, uint64_t out[3 * CMX_LSTM_STATE_ARRAYS]) {
  if (!h || !out) { cmx_set_err("cmx_lstm_debug_layout: bad argument"); return -1; }
  std::vector<StateArray> rg; int dev = 0;
  if (lstm_arrays(h, rg, &dev, nullptr)) return -1;
  state_layout(rg.data(), (int)rg.size(), out);
  return (int)rg.size();
}

}  // extern "C"
