// fxcm_vote.hip -- the redundant fxcm-stage vote (C ABI: cmx_fxcmvote_*, cmx_fxcm_state_diff, cmx_fxcm_debug_state_xor, cmx_fxcm_debug_layout in
// include/cmix_amd.h).
//
// The fxcm stage (fxcm_stage.hip) writes 431 of the 2078 layer-0 columns (3..433) from 4.4 GB of tables that learn online -- one wrong word stays for
// good -- and its roles kernel hands rows between role M's sixteen free-running wavefronts, role U and role X behind counters inside every launch.
// Verify mode and the other votes take its columns as given. The guard here is the one the mixing network, the context stage and the LSTM have: the
// unchanged cmx_fxcm_roles_kernel runs on two or three FxDev (cmx_fxcm_run / cmx_fxcm_run_shared) and two kernels compare what they wrote.
// The rule, the record and the handle's plumbing: cmx_vote_core.h.
//
//   cmx_fxcmvote_kernel         every chunk: the 431 exported values of every bit of n = 2 or 3 instances, word for word; one wavefront per row
//                               (a row's words are consecutive: seven coalesced 4-byte loads per lane and instance, all issued before the first
//                               compare; no LDS). Instance 0 is read in place from the slot's layer-0 rows, whose base (layer0 + 3 + 2078 t) is only
//                               4-byte aligned, differently from row to row: nothing wider than a 4-byte load is used.
//   cmx_fxcmvote_fold_kernel    behind it: folds the chunk's result into a sticky record and captures the first differing bit's row
//   cmx_state_diff_kernel       after an event (and in tests): every word of two handles' tables in HBM
//
// Out of scope: REPAIR (the mixing network has consumed the columns before the host sees the vote: the pipeline stops at the first event), the host
// parser's records, the chunk's bytes and the LSTM hints (one copy of each, read by every instance: NOT covered by the vote), paq8 and PPMd, the
// decoder's form of the stage.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/cmix_amd.h"
#include "cmx_vote_core.h"
#include "cmx_state_digest.h"
#include "fxcm_rec.h"
#include "fxcm_state.h"

namespace {
constexpr unsigned long long kNone = ~0ull;
constexpr int kCols = CMX_FXCMVOTE_COLS;
constexpr int kPasses = (kCols + 63) / 64;   // 7: six full passes of the wave and one of 47 lanes
static_assert(kCols == FX_OUTPUTS, "the vote's row is FXCM::Predict()'s 431 values of one bit");
static_assert(CMX_FXCM_STATE_REGIONS == FX_STATE_REGIONS && CMX_FXCM_STATE_ARRAYS == FX_STATE_ARRAYS, "region and array counts of the header and of fxcm_state.h");

struct FxVoteArgs {
  const uint32_t* rows[3];       // row t of instance i at rows[i] + t * pstride[i]
  unsigned long long pstride[3];
};
// device block of a vote handle
struct FxVoteDev {
  VoteHead head;
  uint32_t words[3 * kCols];     // capture of the first event's bit: instance i, column c at [i * 431 + c]
  uint32_t bit, byte;            // the bit coded at that row and the byte it belongs to
};
struct FxRow {   // (the fold's capture; the vote kernel loads its rows itself)
  typedef FxVoteArgs Args;
  static constexpr int kCols = ::kCols;
  static __device__ __forceinline__ uint32_t word(const FxVoteArgs& a, int i, unsigned long long t, unsigned c) { return a.rows[i][t * a.pstride[i] + c]; }
};

// One wavefront per row (bit), grid-stride over the rows. Every lane keeps its own minimum key, count and odd mask; one reduction and one atomic per
// wave at the end, and only in waves that saw a difference. Registers only.
template <int N>
__global__ void __launch_bounds__(256) cmx_fxcmvote_kernel(FxVoteArgs a, unsigned long long nrows, VoteHead* d) {
  const unsigned lane = threadIdx.x & 63;
  const unsigned long long waves = (unsigned long long)gridDim.x * (blockDim.x >> 6);
  VoteAcc acc;
  for (unsigned long long t = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < nrows; t += waves) {
    const uint32_t* r0 = a.rows[0] + t * a.pstride[0];
    const uint32_t* r1 = a.rows[1] + t * a.pstride[1];
    const uint32_t* r2 = N == 3 ? a.rows[2] + t * a.pstride[2] : r1;
    uint32_t w0[kPasses], w1[kPasses], w2[kPasses];
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {   // (the last pass: lanes past column 430 load nothing and compare equal zeros)
      const unsigned c = lane + 64u * p;
      const bool in = c < (unsigned)kCols;
      w0[p] = in ? r0[c] : 0u; w1[p] = in ? r1[c] : 0u; w2[p] = N == 3 ? (in ? r2[c] : 0u) : w1[p];
    }
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
      const unsigned r = cmx_vote_one<N>(w0[p], w1[p], w2[p]);
      if (r) acc.note(t * kCols + (lane + 64u * p), r);
    }
  }
  acc.flush(d);
}

// behind the vote kernel: the core's fold, and the first event's row is captured with the bit coded there and its byte
__global__ void cmx_fxcmvote_fold_kernel(FxVoteArgs a, unsigned long long nrows, unsigned long long bit0, int n, const uint8_t* bytes, FxVoteDev* d) {
  const VoteEvent ev = cmx_vote_fold(&d->head, nrows, bit0, n, kCols);
  if (!ev.capture) return;
  cmx_vote_capture<FxRow>(a, n, ev.row, d->words);
  if (threadIdx.x == 0) {
    const uint32_t by = bytes ? bytes[ev.row >> 3] : 0u;
    d->byte = by; d->bit = (by >> (7 - (unsigned)(ev.row & 7))) & 1u;
  }
}

// the handle's state arrays as the core's
int fx_arrays(cmx_fxcm_t* h, std::vector<StateArray>& a, int* device, uint64_t* bytes_done) {
  std::vector<FxRegion> rg(FX_STATE_ARRAYS); int n = 0;
  if (cmx_fxcm_state_view(h, rg.data(), &n, device, bytes_done)) return 1;
  a = state_arrays(rg.data(), n);
  return 0;
}

// cmx_fxcm_debug_state_xor, region by region: may a word with ANY value be handed to the unchanged kernels? Decided by reading every use of the
// region's words in fxcm_dev.h and fxcm_stage.hip; "open" = the word is only ever a value (added, compared, shifted into a range that fits what it then
// indexes), "refused" = some value of it addresses memory not sized for it, bounds a loop, or its uses were not all followed.
//    0 constant tables  REFUSED  squash / stretch values index the APM rows (stretch[pr] -> row offset), the state tables' next-state bytes and `tab`
//                                feed StateMap and table indices, FX_WRT classes build mixer selectors: wrong values address past a table
//    1 map buckets      REFUSED  state bytes index nn[4 s + ..], sm[256 ctx + s] and tab[..+ s] (all sized for 256 states), and run bytes index
//                                tab[RC1 + ..] (sized for 512), which would allow it; but the buckets' check bytes steer the probe / replacement walk
//                                of fxd_map_touch and its serial fallback, whose uses were not all followed. Not needed by any test.
//    2 map StateMaps    open     a cell is read as (cell >> 20) = 0..4095 into tab[ST1 + ..] and tab[ST2 + ..] (4096 entries each) and updated by
//                                cell += (y << 19) - (cell >> 13): every 32-bit value stays a value
//    3 SSCM tables      open     a 16-bit cell is read as (cell >> 4) = 0..4095 into stretch[4096] and moved towards y << 16 by a shift
//    4 sm1_t            open     (cell >> 20) = 0..4095 into stretch[4096]; the low 10 bits are a count that enters fxd_dt() arithmetically
//    5 rcm_t            open     elements are (count, byte, 16-bit check): the count indexes rcm_rc[256 b + count] with b <= 1 (512 entries), the
//                                check is compared, the slot is chosen by the parser's hash and masked with rcm_n
//    6 mhash            REFUSED  history positions the match model follows and verifies byte by byte: they drive the recovery loops' lengths
//    7 sp_table         REFUSED  the same for the sparse match model
//    8 buffer           REFUSED  the byte history: expected bytes and match lengths are recovered from it in loops bounded by its content
//    9 wx               open     16-bit weights enter dot products whose results are clipped to +-2047 (fxd_clp) before they index squash[4095];
//                                the rows' numbers come from the selectors (parser fields, the maps' return values), never from a weight
//   10 APM tables       open     two 16-bit cells are interpolated, (t0 (128 - w) + t1 w) >> 11 <= 4095, the range of stretch[4096]; the row's
//                                number comes from the contexts (hashes masked to the table), the cell's from stretch[pr] of a pr <= 4095
//   11 FxDev scalars    REFUSED  cp / cp0 / runp are offsets into the buckets, sm_cxt / mx_cxt / apm_index / sscm_cp / rcm_cp / sm1_cxt / pos / the
//                                match candidates' indices address tables directly
constexpr bool kOpen[FX_STATE_REGIONS] = {false, false, true, true, true, true, false, false, false, true, true, false};
const char* const kRegionName[FX_STATE_REGIONS] = {"constant tables", "map buckets", "map StateMaps", "SSCM tables", "sm1_t", "rcm_t", "mhash", "sp_table", "buffer", "wx",
                                                   "APM tables", "FxDev scalars"};
}  // namespace

struct cmx_fxcmvote : VoteHandle {};

extern "C" {

cmx_fxcmvote_t* cmx_fxcmvote_create(int device, int n) { return vote_create<cmx_fxcmvote>("cmx_fxcmvote_create", device, n, sizeof(FxVoteDev)); }
void cmx_fxcmvote_destroy(cmx_fxcmvote_t* v) { vote_destroy(v); }

int cmx_fxcmvote_run(cmx_fxcmvote_t* v, const float* const* d_rows, const size_t* pstride, size_t nbits, uint64_t stream_bit0, const uint8_t* d_bytes, void* stream) {
  if (!v || !d_rows || !pstride) { cmx_set_err("cmx_fxcmvote_run: bad argument"); return 1; }
  if (nbits == 0) return 0;
  if (nbits > (1ull << 27)) { cmx_set_err("cmx_fxcmvote_run: chunk too large (2^27 bits at the most)"); return 1; }
  FxVoteArgs a;
  memset(&a, 0, sizeof a);
  for (int i = 0; i < v->n; ++i) {
    if (!d_rows[i]) { cmx_set_err("cmx_fxcmvote_run: null rows of instance " + std::to_string(i)); return 1; }
    if (pstride[i] < (size_t)kCols) { cmx_set_err("cmx_fxcmvote_run: pstride of instance " + std::to_string(i) + " is below 431 (434 = a shadow's dense rows, 2078 = layer-0 rows in place)"); return 1; }
    if ((uintptr_t)d_rows[i] & 3) { cmx_set_err("cmx_fxcmvote_run: rows of instance " + std::to_string(i) + " are not 4-byte aligned"); return 1; }
    a.rows[i] = (const uint32_t*)d_rows[i]; a.pstride[i] = pstride[i];
  }
  if (hipSetDevice(v->device) != hipSuccess) { cmx_set_err("hipSetDevice failed"); return 1; }
  hipStream_t st = (hipStream_t)stream;
  const unsigned long long nrows = nbits;
  if (v->n == 3) hipLaunchKernelGGL(cmx_fxcmvote_kernel<3>, dim3(vote_row_grid(nrows)), dim3(256), 0, st, a, nrows, v->d);
  else hipLaunchKernelGGL(cmx_fxcmvote_kernel<2>, dim3(vote_row_grid(nrows)), dim3(256), 0, st, a, nrows, v->d);
  hipLaunchKernelGGL(cmx_fxcmvote_fold_kernel, dim3(1), dim3(64), 0, st, a, nrows, (unsigned long long)stream_bit0, v->n, d_bytes, (FxVoteDev*)v->d);
  if (hipGetLastError() != hipSuccess) { cmx_set_err("cmx_fxcmvote_run: kernel launch failed"); return 1; }
  return 0;
}

const unsigned long long* cmx_fxcmvote_record(cmx_fxcmvote_t* v) { return v && v->d ? v->d->rec : nullptr; }

int cmx_fxcmvote_report(cmx_fxcmvote_t* v, uint64_t out[8]) { return vote_report("cmx_fxcmvote_report", v, out); }
int cmx_fxcmvote_last(cmx_fxcmvote_t* v, uint64_t out[4]) { return vote_last("cmx_fxcmvote_last", v, out); }

int cmx_fxcmvote_values(cmx_fxcmvote_t* v, uint32_t words[3 * CMX_FXCMVOTE_COLS], uint32_t* bit, uint32_t* byte) {
  FxVoteDev h;
  if (vote_values("cmx_fxcmvote_values", v, words, &h)) return 1;
  memcpy(words, h.words, sizeof h.words);
  if (bit) *bit = h.bit;
  if (byte) *byte = h.byte;
  return 0;
}

int cmx_fxcm_state_diff(cmx_fxcm_t* a, cmx_fxcm_t* b, uint64_t out[CMX_FXCM_STATE_OUT]) {
  if (!a || !b || !out) { cmx_set_err("cmx_fxcm_state_diff: bad argument"); return 1; }
  if (a == b) { cmx_set_err("cmx_fxcm_state_diff: a and b are the same handle"); return 1; }
  std::vector<StateArray> ra, rb; int deva = 0, devb = 0;
  uint64_t ca = 0, cb = 0;
  if (fx_arrays(a, ra, &deva, &ca) || fx_arrays(b, rb, &devb, &cb)) return 1;
  const int na = (int)ra.size();
  if (deva != devb) { cmx_set_err("cmx_fxcm_state_diff: the two handles live on different devices"); return 1; }
  if (ca != cb) { cmx_set_err("cmx_fxcm_state_diff: the host-side counter bytes_done differs: " + std::to_string(ca) + " and " + std::to_string(cb)); return 1; }
  if (hipSetDevice(deva) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { cmx_set_err("cmx_fxcm_state_diff: device error"); return 1; }
  std::vector<DiffDev> h(ra.size());
  bool ok = ra.size() == rb.size() && state_diff_arrays(ra.data(), rb.data(), na, 2048, h.data());
  for (int i = 0; i < CMX_FXCM_STATE_OUT; ++i) out[i] = 0;
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
  if (!ok) { (void)hipGetLastError(); cmx_set_err("cmx_fxcm_state_diff: device error"); return 1; }
  // region 11: FxDev itself, device pointers zeroed (they differ between two handles by construction)
  std::vector<uint32_t> wa, wb;
  if (cmx_fxcm_dev_words(a, wa) || cmx_fxcm_dev_words(b, wb)) return 1;
  for (size_t i = 0; i < wa.size(); ++i)
    if (wa[i] != wb[i]) {
      out[0] += 1; out[5 + FX_REGION_DEV] += 1;
      if (out[1] == kNone) { out[1] = FX_REGION_DEV; out[2] = i; out[3] = wa[i]; out[4] = wb[i]; }
    }
  return 0;
}

// one column per array of the state view, then region 11: FxDev with its device pointers zeroed, and behind it the host-side counter bytes_done
static int fx_digest(const char* who, cmx_fxcm_t* h, uint64_t* out, size_t cap, int layout) {
  if (!h) { cmx_set_err(std::string(who) + ": null handle"); return -1; }
  std::vector<StateArray> rg; int dev = 0;
  uint64_t done = 0;
  if (fx_arrays(h, rg, &dev, &done)) return -1;
  std::vector<uint32_t> w;
  if (cmx_fxcm_dev_words(h, w)) return -1;
  w.push_back((uint32_t)done); w.push_back((uint32_t)(done >> 32));
  return cmx_state_digest_stage(who, dev, rg.data(), (int)rg.size(), &w, FX_REGION_DEV, out, cap, layout);
}
int cmx_fxcm_state_digest(cmx_fxcm_t* h, uint64_t* out, size_t cap) { return fx_digest("cmx_fxcm_state_digest", h, out, cap, 0); }
int cmx_fxcm_state_digest_layout(cmx_fxcm_t* h, uint64_t* out, size_t cap) { return fx_digest("cmx_fxcm_state_digest_layout", h, out, cap, 1); }

int cmx_fxcm_debug_state_xor(cmx_fxcm_t* h, int region, uint64_t index, uint32_t xor_mask) {
  if (!h) { cmx_set_err("cmx_fxcm_debug_state_xor: null handle"); return 1; }
  if (!xor_mask) { cmx_set_err("cmx_fxcm_debug_state_xor: a zero mask changes nothing"); return 1; }
  if (region < 0 || region >= FX_STATE_REGIONS) { cmx_set_err("cmx_fxcm_debug_state_xor: no such region (0..11)"); return 1; }
  if (!kOpen[region]) {
    cmx_set_err("cmx_fxcm_debug_state_xor: region " + std::to_string(region) + " (" + kRegionName[region] +
                ") holds words the kernels address memory or bound loops with: refused (the hook changes values only)");
    return 1;
  }
  std::vector<StateArray> rg; int dev = 0;
  if (fx_arrays(h, rg, &dev, nullptr)) return 1;
  const int n = (int)rg.size();
  uint32_t* p = state_word(rg.data(), n, region, index);
  if (!p) { cmx_set_err("cmx_fxcm_debug_state_xor: no such word (region, index out of range)"); return 1; }
  return state_xor("cmx_fxcm_debug_state_xor", dev, p, xor_mask);
}

int cmx_fxcm_debug_state_read(cmx_fxcm_t* h, int region, uint64_t index, uint64_t count, uint32_t* out) {
  if (!h || !out || !count) { cmx_set_err("cmx_fxcm_debug_state_read: bad argument"); return 1; }
  if (region < 0 || region >= FX_STATE_REGIONS) { cmx_set_err("cmx_fxcm_debug_state_read: no such region (0..11)"); return 1; }
  if (region == FX_REGION_DEV) {
    std::vector<uint32_t> w;
    if (cmx_fxcm_dev_words(h, w)) return 1;
    if (index >= w.size() || count > w.size() - index) { cmx_set_err("cmx_fxcm_debug_state_read: no such words (region, index out of range)"); return 1; }
    memcpy(out, w.data() + index, count * 4);
    return 0;
  }
  std::vector<StateArray> rg; int dev = 0;
  if (fx_arrays(h, rg, &dev, nullptr)) return 1;
  const int n = (int)rg.size();
  if (hipSetDevice(dev) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { cmx_set_err("cmx_fxcm_debug_state_read: device error"); return 1; }
  unsigned long long done = 0;
  for (int r = 0; r < n && done < count; ++r) {   // (the words may run from one array of the region into the next)
    const unsigned long long off = state_offset(rg.data(), r);
    if (rg[r].region == region && index + done >= off && index + done - off < rg[r].words) {
      const unsigned long long at = index + done - off, m = count - done < rg[r].words - at ? count - done : rg[r].words - at;
      if (hipMemcpy(out + done, rg[r].p + at, m * 4, hipMemcpyDeviceToHost) != hipSuccess) { cmx_set_err("cmx_fxcm_debug_state_read: device error"); return 1; }
      done += m;
    }
  }
  if (done != count) { cmx_set_err("cmx_fxcm_debug_state_read: no such words (region, index out of range)"); return 1; }
  return 0;
}

int cmx_fxcm_debug_layout(cmx_fxcm_t* h, uint64_t out[3 * CMX_FXCM_STATE_ARRAYS]) {
  if (!h || !out) { cmx_set_err("cmx_fxcm_debug_layout: bad argument"); return -1; }
  std::vector<StateArray> rg; int dev = 0;
  if (fx_arrays(h, rg, &dev, nullptr)) return -1;
  const int n = (int)rg.size();
  state_layout(rg.data(), n, out);
  std::vector<uint32_t> w;
  if (cmx_fxcm_dev_words(h, w)) return -1;
  out[3 * n] = FX_REGION_DEV; out[3 * n + 1] = 0; out[3 * n + 2] = w.size();
  return n + 1;
}

}  // extern "C"
