// lstm_vote.hip -- the redundant LSTM-stage vote (C ABI: cmx_lstmvote_*, cmx_lstm_state_diff, cmx_lstm_debug_state_xor, cmx_lstm_debug_layout in
// include/cmix_amd.h).
//
// The LSTM byte mixer (lstm_block.hip) writes layer-0 column 2077 and, through lstmpr / lstmex, steers fxcm's mixer selection and APMs; its state
// learns online, so one wrong word in a gate matrix changes every later distribution. Its block kernels hand values between 52 workgroups inside a
// launch behind counters and have no host form. Verify mode, the network's vote and the context vote all take the column as given. The guard here is
// the one those stages have: the unchanged cmx_lstm_run runs on two or three handles over the same bytes and the same PPMd distributions, and two new
// kernels compare what they produced.
//
//   cmx_lstmvote_kernel        every chunk: the distribution after every byte (256 words), the byte's eight bit predictions and eight `ex` words of
//                              n = 2 or 3 instances, word for word; one wavefront per byte (a row's 256 distribution words are consecutive:
//                              coalesced; the eight strided words of an instance read in place from layer-0 rows go to eight lanes; no LDS)
//   cmx_lstmvote_fold_kernel   behind it: folds the chunk's result into a sticky record and captures the first differing byte's row
//   cmx_lstm_state_diff_kernel after an event (and in tests): every word of two handles' state arrays in HBM
//
// Out of scope: REPAIR (what the LSTM wrote has been consumed on the device by fxcm and the network before the host sees the vote: the pipeline stops
// at the first event), the other producers of a slot (fxcm, paq8, PPMd), PPMd's distributions and the bytes (shared by all instances), the decoder's
// form of the stage.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/cmix_amd.h"
#include "lstm_state.h"

void cmx_set_err(const std::string& s);  // cmx_api.hip
extern "C" int cmx_lstm_state_view(cmx_lstm_t* h, LstmRegion* out, int* n, int* device, uint64_t counters[3]);   // lstm_api.hip

namespace {
constexpr unsigned long long kNone = ~0ull;
constexpr int kCols = CMX_LSTMVOTE_COLS;   // 256 distribution words, 8 bit predictions, 8 `ex`
static_assert(kCols == LSTM_VP + 16, "the vote's row is a byte's distribution, its eight bit predictions and its eight ex words");
static_assert(CMX_LSTM_STATE_REGIONS == LSTM_REGIONS && CMX_LSTM_STATE_ARRAYS == LSTM_STATE_ARRAYS, "region and array counts of the header and of lstm_state.h");

// device block of a vote handle
struct LstmVoteDev {
  unsigned long long rec[8];     // the sticky record (cmx_lstmvote_report)
  unsigned long long last[4];    // the chunk folded last (cmx_lstmvote_last), right behind the record: one copy fetches both
  unsigned long long key;        // this chunk: min over non-agreeing elements of (e << 2 | odd instance, 3 = no majority); ~0 = none
  unsigned long long cnt;        // this chunk: non-agreeing elements
  unsigned long long odd;        // this chunk: bit i = instance i was the odd one of some element, bit 3 = some element had no majority
  unsigned long long pad;
  uint32_t words[3 * kCols];     // capture of the first event's byte: instance i, element c at [i * 272 + c]
  uint32_t byte;
};
struct LstmVoteArgs {
  const uint32_t* dist[3];       // [N][256]
  const uint32_t* bitp[3];       // bit k of byte b at [(8 b + k) * pstride]
  const uint32_t* ex[3];         // [N][8]
  unsigned long long pstride[3];
};

// one element of n instances: 0 agree, else 1 + (odd instance, 3 = no majority)
template <int N>
__device__ __forceinline__ unsigned vote_one(uint32_t a, uint32_t b, uint32_t c) {
  if (N == 2) return a == b ? 0u : 4u;
  if (a == b && b == c) return 0u;
  if (b == c) return 1u;
  if (a == c) return 2u;
  if (a == b) return 3u;
  return 4u;
}
// element c (< 272) of byte b of instance i
__device__ __forceinline__ uint32_t lstm_word(const LstmVoteArgs& a, int i, unsigned long long b, unsigned c) {
  if (c < LSTM_VP) return a.dist[i][b * LSTM_VP + c];
  if (c < LSTM_VP + 8) return a.bitp[i][(b * 8 + (c - LSTM_VP)) * a.pstride[i]];
  return a.ex[i][b * 8 + (c - LSTM_VP - 8)];
}

// One wavefront per byte, grid-stride over the bytes; a row is five passes of the wave: four over the distribution, one in which lanes 0..7 take the
// bit predictions and lanes 8..15 the ex words. 4-byte loads only: nothing is assumed about the arrays' alignment. Every lane keeps its own minimum
// key and count; one reduction per wave at the end.
template <int N>
__global__ void __launch_bounds__(256) cmx_lstmvote_kernel(LstmVoteArgs a, unsigned long long nrows, LstmVoteDev* d) {
  const unsigned lane = threadIdx.x & 63;
  const unsigned long long waves = (unsigned long long)gridDim.x * (blockDim.x >> 6);
  unsigned long long key = kNone, cnt = 0;
  unsigned odd = 0;
  for (unsigned long long b = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); b < nrows; b += waves) {
    for (unsigned c = lane; c < (unsigned)kCols; c += 64) {
      const uint32_t w0 = lstm_word(a, 0, b, c), w1 = lstm_word(a, 1, b, c), w2 = N == 3 ? lstm_word(a, 2, b, c) : w1;
      const unsigned r = vote_one<N>(w0, w1, w2);
      if (r) {
        const unsigned long long k = ((b * kCols + c) << 2) | (r - 1);
        key = k < key ? k : key; ++cnt; odd |= 1u << (r - 1);
      }
    }
  }
  if (__ballot(cnt != 0) == 0) return;   // (wave-uniform) nothing differed in this wave
  for (int o = 32; o; o >>= 1) {
    const unsigned long long k2 = __shfl_xor(key, o), c2 = __shfl_xor(cnt, o);
    key = k2 < key ? k2 : key; cnt += c2; odd |= __shfl_xor(odd, o);
  }
  if (lane == 0) { atomicMin(&d->key, key); atomicAdd(&d->cnt, cnt); atomicOr(&d->odd, (unsigned long long)odd); }
}

// one wave, behind the vote kernel on the same stream: the chunk's key and count into the sticky record; the first event's byte is captured.
// The chunk's OWN result goes into last[] exactly as cmx_vote_fold_kernel (mixnet_vote.hip) leaves it.
__global__ void cmx_lstmvote_fold_kernel(LstmVoteArgs a, unsigned long long nrows, unsigned long long byte0, int n, const uint8_t* bytes, LstmVoteDev* d) {
  const unsigned long long key = d->key, cnt = d->cnt, odd = d->odd;
  const bool first = cnt != 0 && d->rec[3] == 0;   // (read by every lane before lane 0 writes: one wave, the barrier below orders it)
  __syncthreads();
  const unsigned long long e = key >> 2, b = e / kCols, c = e - b * kCols;
  if (first && b < nrows)
    for (int i = threadIdx.x; i < n * kCols; i += blockDim.x) {
      const int inst = i / kCols;
      d->words[i] = lstm_word(a, inst, b, (unsigned)(i - inst * kCols));
    }
  if (threadIdx.x == 0) {
    d->rec[0] += 1; d->rec[1] += nrows; d->rec[2] = (unsigned long long)n;
    if (cnt) d->rec[3] += 1;
    if (first) {
      d->rec[4] = byte0 + b; d->rec[5] = c; d->rec[6] = (key & 3) == 3 ? kNone : (key & 3); d->rec[7] = cnt;
      d->byte = bytes && b < nrows ? bytes[b] : 0u;
    }
    d->last[0] = cnt; d->last[1] = cnt ? byte0 + b : 0; d->last[2] = cnt ? c : 0;
    d->last[3] = !cnt ? 0 : odd == 1 ? 0 : odd == 2 ? 1 : odd == 4 ? 2 : kNone;
    d->key = kNone; d->cnt = 0; d->odd = 0;   // the next chunk starts clean
  }
}

// ---- state diff: the words of two arrays; one launch per array ----
struct LstmDiffDev { unsigned long long cnt, first; };
__global__ void __launch_bounds__(256) cmx_lstm_state_diff_kernel(const uint32_t* x, const uint32_t* y, unsigned long long n, LstmDiffDev* d) {
  const unsigned long long nq = n / 4, items = nq + (n - 4 * nq);   // (every array is a hipMalloc of its own: 16-byte aligned)
  unsigned long long first = kNone, cnt = 0;
  auto word = [&](unsigned long long i) { ++cnt; first = i < first ? i : first; };
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (unsigned long long)gridDim.x * blockDim.x) {
    if (i < nq) {
      const uint4 u = reinterpret_cast<const uint4*>(x)[i], v = reinterpret_cast<const uint4*>(y)[i];
      if (u.x != v.x) word(4 * i);
      if (u.y != v.y) word(4 * i + 1);
      if (u.z != v.z) word(4 * i + 2);
      if (u.w != v.w) word(4 * i + 3);
    } else {
      const unsigned long long j = 4 * nq + (i - nq);
      if (x[j] != y[j]) word(j);
    }
  }
  if (__ballot(cnt != 0) == 0) return;
  for (int o = 32; o; o >>= 1) {
    const unsigned long long f2 = __shfl_xor(first, o), c2 = __shfl_xor(cnt, o);
    first = f2 < first ? f2 : first; cnt += c2;
  }
  if ((threadIdx.x & 63) == 0) { atomicMin(&d->first, first); atomicAdd(&d->cnt, cnt); }
}

constexpr int kIndexRegion = 9;   // input_history, bp_symbol, dyn: words the kernels use as indices
}  // namespace

struct cmx_lstmvote {
  int device = 0, n = 0;
  LstmVoteDev* d = nullptr;
};

extern "C" {

cmx_lstmvote_t* cmx_lstmvote_create(int device, int n) {
  if (n != 2 && n != 3) { cmx_set_err("cmx_lstmvote_create: n must be 2 or 3 instances"); return nullptr; }
  if (cmx_device_count() <= 0) { cmx_set_err("cmx_lstmvote_create: no HIP device visible (a gfx950 GPU is required)"); return nullptr; }
  if (device < 0 || device >= cmx_device_count() || hipSetDevice(device) != hipSuccess) { cmx_set_err("cmx_lstmvote_create: bad device index"); return nullptr; }
  cmx_lstmvote_t* v = new cmx_lstmvote();
  v->device = device; v->n = n;
  LstmVoteDev init;
  memset(&init, 0, sizeof init);
  init.key = kNone;
  if (hipMalloc((void**)&v->d, sizeof(LstmVoteDev)) != hipSuccess || hipMemcpy(v->d, &init, sizeof init, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    if (v->d) (void)hipFree(v->d);
    delete v;
    cmx_set_err("cmx_lstmvote_create: hipMalloc failed");
    return nullptr;
  }
  return v;
}

void cmx_lstmvote_destroy(cmx_lstmvote_t* v) {
  if (!v) return;
  (void)hipSetDevice(v->device);
  (void)hipDeviceSynchronize();
  if (v->d) (void)hipFree(v->d);
  delete v;
}

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
  const unsigned grid = (unsigned)((nrows + 3) / 4 < 512 ? (nrows + 3) / 4 : 512);   // four rows (waves) per workgroup
  if (v->n == 3) hipLaunchKernelGGL(cmx_lstmvote_kernel<3>, dim3(grid), dim3(256), 0, st, a, nrows, v->d);
  else hipLaunchKernelGGL(cmx_lstmvote_kernel<2>, dim3(grid), dim3(256), 0, st, a, nrows, v->d);
  hipLaunchKernelGGL(cmx_lstmvote_fold_kernel, dim3(1), dim3(64), 0, st, a, nrows, (unsigned long long)stream_byte0, v->n, d_bytes, v->d);
  if (hipGetLastError() != hipSuccess) { cmx_set_err("cmx_lstmvote_run: kernel launch failed"); return 1; }
  return 0;
}

const unsigned long long* cmx_lstmvote_record(cmx_lstmvote_t* v) { return v && v->d ? v->d->rec : nullptr; }

int cmx_lstmvote_report(cmx_lstmvote_t* v, uint64_t out[8]) {
  if (!v || !out) { cmx_set_err("cmx_lstmvote_report: bad argument"); return 1; }
  unsigned long long r[8];
  if (hipSetDevice(v->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(r, v->d->rec, sizeof r, hipMemcpyDeviceToHost) != hipSuccess) {
    cmx_set_err("cmx_lstmvote_report: device error"); return 1;
  }
  for (int i = 0; i < 8; ++i) out[i] = r[i];
  return 0;
}

int cmx_lstmvote_last(cmx_lstmvote_t* v, uint64_t out[4]) {
  if (!v || !out) { cmx_set_err("cmx_lstmvote_last: bad argument"); return 1; }
  unsigned long long r[4];
  if (hipSetDevice(v->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(r, v->d->last, sizeof r, hipMemcpyDeviceToHost) != hipSuccess) {
    cmx_set_err("cmx_lstmvote_last: device error"); return 1;
  }
  for (int i = 0; i < 4; ++i) out[i] = r[i];
  return 0;
}

int cmx_lstmvote_values(cmx_lstmvote_t* v, uint32_t words[3 * CMX_LSTMVOTE_COLS], uint32_t* byte) {
  if (!v || !words) { cmx_set_err("cmx_lstmvote_values: bad argument"); return 1; }
  LstmVoteDev h;
  if (hipSetDevice(v->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(&h, v->d, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) {
    cmx_set_err("cmx_lstmvote_values: device error"); return 1;
  }
  memcpy(words, h.words, sizeof h.words);
  if (byte) *byte = h.byte;
  return 0;
}

int cmx_lstm_state_diff(cmx_lstm_t* a, cmx_lstm_t* b, uint64_t out[16]) {
  if (!a || !b || !out) { cmx_set_err("cmx_lstm_state_diff: bad argument"); return 1; }
  if (a == b) { cmx_set_err("cmx_lstm_state_diff: a and b are the same handle"); return 1; }
  LstmRegion ra[LSTM_STATE_ARRAYS], rb[LSTM_STATE_ARRAYS]; int na = 0, nb = 0, deva = 0, devb = 0;
  uint64_t ca[3], cb[3];
  if (cmx_lstm_state_view(a, ra, &na, &deva, ca) || cmx_lstm_state_view(b, rb, &nb, &devb, cb)) return 1;
  if (deva != devb) { cmx_set_err("cmx_lstm_state_diff: the two handles live on different devices"); return 1; }
  if (cmx_lstm_vocab_size(a) != cmx_lstm_vocab_size(b)) { cmx_set_err("cmx_lstm_state_diff: the two handles have different vocabulary sizes"); return 1; }
  static const char* const kCounter[3] = {"bytes_done", "hc", "bptt_rounds"};
  for (int i = 0; i < 3; ++i)
    if (ca[i] != cb[i]) {
      cmx_set_err(std::string("cmx_lstm_state_diff: the host-side counter ") + kCounter[i] + " differs: " + std::to_string(ca[i]) + " and " + std::to_string(cb[i]));
      return 1;
    }
  if (hipSetDevice(deva) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { cmx_set_err("cmx_lstm_state_diff: device error"); return 1; }
  std::vector<LstmDiffDev> h((size_t)na, LstmDiffDev{0, kNone});
  LstmDiffDev* d = nullptr;
  bool ok = hipMalloc((void**)&d, h.size() * sizeof(LstmDiffDev)) == hipSuccess && hipMemcpy(d, h.data(), h.size() * sizeof(LstmDiffDev), hipMemcpyHostToDevice) == hipSuccess;
  for (int r = 0; ok && r < na; ++r) {
    if (ra[r].region != rb[r].region || ra[r].words != rb[r].words) { ok = false; break; }
    const unsigned long long items = ra[r].words / 4 + 4;
    const unsigned grid = (unsigned)(items / 256 + 1 < 1024 ? items / 256 + 1 : 1024);
    hipLaunchKernelGGL(cmx_lstm_state_diff_kernel, dim3(grid), dim3(256), 0, 0, ra[r].p, rb[r].p, ra[r].words, d + r);
    ok = hipGetLastError() == hipSuccess;
  }
  ok = ok && hipDeviceSynchronize() == hipSuccess && hipMemcpy(h.data(), d, h.size() * sizeof(LstmDiffDev), hipMemcpyDeviceToHost) == hipSuccess;
  for (int i = 0; i < 16; ++i) out[i] = 0;
  for (int i = 1; i <= 4; ++i) out[i] = kNone;
  unsigned long long off = 0;   // of array r inside its region
  for (int r = 0; ok && r < na; ++r) {   // (region-then-array order)
    if (r && ra[r].region != ra[r - 1].region) off = 0;
    if (h[r].cnt) {
      out[0] += h[r].cnt; out[5 + ra[r].region] += h[r].cnt;
      if (out[1] == kNone) {
        uint32_t x = 0, y = 0;
        ok = hipMemcpy(&x, ra[r].p + h[r].first, 4, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(&y, rb[r].p + h[r].first, 4, hipMemcpyDeviceToHost) == hipSuccess;
        out[1] = (uint64_t)ra[r].region; out[2] = off + h[r].first; out[3] = x; out[4] = y;
      }
    }
    off += ra[r].words;
  }
  if (d) (void)hipFree(d);
  if (!ok) { (void)hipGetLastError(); cmx_set_err("cmx_lstm_state_diff: device error"); return 1; }
  return 0;
}

int cmx_lstm_debug_state_xor(cmx_lstm_t* h, int region, uint64_t index, uint32_t xor_mask) {
  if (!h) { cmx_set_err("cmx_lstm_debug_state_xor: null handle"); return 1; }
  if (!xor_mask) { cmx_set_err("cmx_lstm_debug_state_xor: a zero mask changes nothing"); return 1; }
  if (region == kIndexRegion) {
    cmx_set_err("cmx_lstm_debug_state_xor: region 9 (input_history, bp_symbol, dyn) holds indices the kernels address memory with: refused (the hook changes values only)");
    return 1;
  }
  LstmRegion rg[LSTM_STATE_ARRAYS]; int n = 0, dev = 0;
  if (cmx_lstm_state_view(h, rg, &n, &dev, nullptr)) return 1;
  uint32_t* p = nullptr;
  unsigned long long off = 0;
  for (int r = 0; r < n && !p; ++r) {
    if (r && rg[r].region != rg[r - 1].region) off = 0;
    if (rg[r].region == region && index >= off && index - off < rg[r].words) p = rg[r].p + (index - off);
    off += rg[r].words;
  }
  if (!p) { cmx_set_err("cmx_lstm_debug_state_xor: no such word (region, index out of range)"); return 1; }
  uint32_t x = 0;
  if (hipSetDevice(dev) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(&x, p, 4, hipMemcpyDeviceToHost) != hipSuccess) {
    cmx_set_err("cmx_lstm_debug_state_xor: device error"); return 1;
  }
  x ^= xor_mask;
  if (hipMemcpy(p, &x, 4, hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { cmx_set_err("cmx_lstm_debug_state_xor: device error"); return 1; }
  return 0;
}

int cmx_lstm_debug_layout(cmx_lstm_t* h, uint64_t out[3 * CMX_LSTM_STATE_ARRAYS]) {
  if (!h || !out) { cmx_set_err("cmx_lstm_debug_layout: bad argument"); return -1; }
  LstmRegion rg[LSTM_STATE_ARRAYS]; int n = 0, dev = 0;
  if (cmx_lstm_state_view(h, rg, &n, &dev, nullptr)) return -1;
  unsigned long long off = 0;
  for (int r = 0; r < n; ++r) {
    if (r && rg[r].region != rg[r - 1].region) off = 0;
    out[3 * r] = (uint64_t)rg[r].region; out[3 * r + 1] = off; out[3 * r + 2] = rg[r].words;
    off += rg[r].words;
  }
  return n;
}

}  // extern "C"
