// ctxmodels_vote.hip -- the redundant context-stage vote (C ABI: cmx_ctxvote_*, cmx_ctxmodels_state_diff, cmx_ctxmodels_debug_state_xor,
// cmx_ctxmodels_debug_layout in include/cmix_amd.h).
//
// The context stage (ctxmodels_kernels.hip) is the only producer of the 47 mixer selectors and writes 54 of the layer-0 columns. Verify mode compares
// the mixing network's copy of those words with the slot they came from, and the network's own vote (mixnet_vote.hip) runs every instance on the same
// slot: a word the PRODUCER got wrong passes both. The guard here is the one the network has: the unchanged cmx_ctxmodels_kernel runs on two or three
// handles over the same bytes, and two new kernels compare what they produced.
//
//   cmx_ctxvote_kernel        every chunk: the 54 model outputs and 47 selectors of every bit of n = 2 or 3 instances, word for word; one wavefront
//                             per row (a full-stride row's columns 2025..2075 and a row's selectors are consecutive words: coalesced, no LDS)
//   cmx_ctxvote_fold_kernel   behind it: folds the chunk's result into a sticky record and captures the first differing bit
//   cmx_ctx_state_diff_kernel after an event (and in tests): every word of two handles' state arrays in HBM
//
// Out of scope: repairing an outvoted instance from the majority (the pipeline stops at the first event), the other producers of a slot (fxcm, paq8,
// LSTM, PPMd), the bit and decay words, and the decoder's form of the stage.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/cmix_amd.h"
#include "ctxmodels_state.h"

void cmx_set_err(const std::string& s);  // cmx_api.hip
extern "C" int cmx_ctxmodels_state_view(cmx_ctxmodels_t* h, const CtxRegion** regions, int* n, int* device);   // ctxmodels_api.hip

namespace {
constexpr unsigned long long kNone = ~0ull;
constexpr int kCols = CMX_CTXVOTE_COLS;   // 54 model outputs in lane order, then the 47 selectors
static_assert(kCols == CTX_NM + CTX_NSEL, "the vote's row is the stage's 54 model outputs and 47 selectors");

// device block of a vote handle
struct CtxVoteDev {
  unsigned long long rec[8];     // the sticky record (cmx_ctxvote_report)
  unsigned long long last[4];    // the chunk folded last (cmx_ctxvote_last), right behind the record: one copy fetches both
  unsigned long long key;        // this chunk: min over non-agreeing elements of (e << 2 | odd instance, 3 = no majority); ~0 = none
  unsigned long long cnt;        // this chunk: non-agreeing elements
  unsigned long long odd;        // this chunk: bit i = instance i was the odd one of some element, bit 3 = some element had no majority
  unsigned long long pad;
  uint32_t words[3 * kCols];     // capture of the first event's bit: instance i, element c at [i * 101 + c]
  uint32_t bit;
};
struct CtxVoteArgs {
  const uint32_t* probs[3];
  const uint32_t* sel[3];
  unsigned long long pstride[3];
  int compact[3];
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
// element c (< 101) of row t of instance i
__device__ __forceinline__ uint32_t ctx_word(const CtxVoteArgs& a, int i, unsigned long long t, unsigned c) {
  if (c >= CTX_NM) return a.sel[i][t * CTX_NSEL + (c - CTX_NM)];
  const unsigned col = a.compact[i] || c < 3 ? c : 2022 + c;   // lane order: layer-0 columns 0, 1, 2, 2025..2075
  return a.probs[i][t * a.pstride[i] + col];
}

// One wavefront per row, grid-stride over the rows; a row is two passes of the wave: elements 0..63 and 64..100. 4-byte loads only: nothing is
// assumed about the arrays' alignment. Every lane keeps its own minimum key and count; one reduction per wave at the end.
template <int N>
__global__ void __launch_bounds__(256) cmx_ctxvote_kernel(CtxVoteArgs a, unsigned long long nrows, CtxVoteDev* d) {
  const unsigned lane = threadIdx.x & 63;
  const unsigned long long waves = (unsigned long long)gridDim.x * (blockDim.x >> 6);
  unsigned long long key = kNone, cnt = 0;
  unsigned odd = 0;
  for (unsigned long long t = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < nrows; t += waves) {
    for (unsigned c = lane; c < (unsigned)kCols; c += 64) {
      const uint32_t w0 = ctx_word(a, 0, t, c), w1 = ctx_word(a, 1, t, c), w2 = N == 3 ? ctx_word(a, 2, t, c) : w1;
      const unsigned r = vote_one<N>(w0, w1, w2);
      if (r) {
        const unsigned long long k = ((t * kCols + c) << 2) | (r - 1);
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

// one wave, behind the vote kernel on the same stream: the chunk's key and count into the sticky record; the first event's bit is captured.
// The chunk's OWN result goes into last[] exactly as cmx_vote_fold_kernel (mixnet_vote.hip) leaves it.
__global__ void cmx_ctxvote_fold_kernel(CtxVoteArgs a, unsigned long long nrows, unsigned long long bit0, int n, const uint8_t* bits, CtxVoteDev* d) {
  const unsigned long long key = d->key, cnt = d->cnt, odd = d->odd;
  const bool first = cnt != 0 && d->rec[3] == 0;   // (read by every lane before lane 0 writes: one wave, the barrier below orders it)
  __syncthreads();
  const unsigned long long e = key >> 2, t = e / kCols, c = e - t * kCols;
  if (first && t < nrows)
    for (int i = threadIdx.x; i < n * kCols; i += blockDim.x) {
      const int inst = i / kCols;
      d->words[i] = ctx_word(a, inst, t, (unsigned)(i - inst * kCols));
    }
  if (threadIdx.x == 0) {
    d->rec[0] += 1; d->rec[1] += nrows; d->rec[2] = (unsigned long long)n;
    if (cnt) d->rec[3] += 1;
    if (first) {
      d->rec[4] = bit0 + t; d->rec[5] = c; d->rec[6] = (key & 3) == 3 ? kNone : (key & 3); d->rec[7] = cnt;
      d->bit = bits && t < nrows ? bits[t] : 0u;
    }
    d->last[0] = cnt; d->last[1] = cnt ? bit0 + t : 0; d->last[2] = cnt ? c : 0;
    d->last[3] = !cnt ? 0 : odd == 1 ? 0 : odd == 2 ? 1 : odd == 4 ? 2 : kNone;
    d->key = kNone; d->cnt = 0; d->odd = 0;   // the next chunk starts clean
  }
}

// ---- state diff: the words of two arrays; one launch per array ----
struct CtxDiffDev { unsigned long long cnt, first; };
__global__ void __launch_bounds__(256) cmx_ctx_state_diff_kernel(const uint32_t* x, const uint32_t* y, unsigned long long n, CtxDiffDev* d) {
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
}  // namespace

struct cmx_ctxvote {
  int device = 0, n = 0;
  CtxVoteDev* d = nullptr;
};

extern "C" {

cmx_ctxvote_t* cmx_ctxvote_create(int device, int n) {
  if (n != 2 && n != 3) { cmx_set_err("cmx_ctxvote_create: n must be 2 or 3 instances"); return nullptr; }
  if (cmx_device_count() <= 0) { cmx_set_err("cmx_ctxvote_create: no HIP device visible (a gfx950 GPU is required)"); return nullptr; }
  if (device < 0 || device >= cmx_device_count() || hipSetDevice(device) != hipSuccess) { cmx_set_err("cmx_ctxvote_create: bad device index"); return nullptr; }
  cmx_ctxvote_t* v = new cmx_ctxvote();
  v->device = device; v->n = n;
  CtxVoteDev init;
  memset(&init, 0, sizeof init);
  init.key = kNone;
  if (hipMalloc((void**)&v->d, sizeof(CtxVoteDev)) != hipSuccess || hipMemcpy(v->d, &init, sizeof init, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    if (v->d) (void)hipFree(v->d);
    delete v;
    cmx_set_err("cmx_ctxvote_create: hipMalloc failed");
    return nullptr;
  }
  return v;
}

void cmx_ctxvote_destroy(cmx_ctxvote_t* v) {
  if (!v) return;
  (void)hipSetDevice(v->device);
  (void)hipDeviceSynchronize();
  if (v->d) (void)hipFree(v->d);
  delete v;
}

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
  const unsigned grid = (unsigned)((nrows + 3) / 4 < 512 ? (nrows + 3) / 4 : 512);   // four rows (waves) per workgroup
  if (v->n == 3) hipLaunchKernelGGL(cmx_ctxvote_kernel<3>, dim3(grid), dim3(256), 0, st, a, nrows, v->d);
  else hipLaunchKernelGGL(cmx_ctxvote_kernel<2>, dim3(grid), dim3(256), 0, st, a, nrows, v->d);
  hipLaunchKernelGGL(cmx_ctxvote_fold_kernel, dim3(1), dim3(64), 0, st, a, nrows, (unsigned long long)stream_bit0, v->n, d_bits, v->d);
  if (hipGetLastError() != hipSuccess) { cmx_set_err("cmx_ctxvote_run: kernel launch failed"); return 1; }
  return 0;
}

const unsigned long long* cmx_ctxvote_record(cmx_ctxvote_t* v) { return v && v->d ? v->d->rec : nullptr; }

int cmx_ctxvote_report(cmx_ctxvote_t* v, uint64_t out[8]) {
  if (!v || !out) { cmx_set_err("cmx_ctxvote_report: bad argument"); return 1; }
  unsigned long long r[8];
  if (hipSetDevice(v->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(r, v->d->rec, sizeof r, hipMemcpyDeviceToHost) != hipSuccess) {
    cmx_set_err("cmx_ctxvote_report: device error"); return 1;
  }
  for (int i = 0; i < 8; ++i) out[i] = r[i];
  return 0;
}

int cmx_ctxvote_last(cmx_ctxvote_t* v, uint64_t out[4]) {
  if (!v || !out) { cmx_set_err("cmx_ctxvote_last: bad argument"); return 1; }
  unsigned long long r[4];
  if (hipSetDevice(v->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(r, v->d->last, sizeof r, hipMemcpyDeviceToHost) != hipSuccess) {
    cmx_set_err("cmx_ctxvote_last: device error"); return 1;
  }
  for (int i = 0; i < 4; ++i) out[i] = r[i];
  return 0;
}

int cmx_ctxvote_values(cmx_ctxvote_t* v, uint32_t words[3 * CMX_CTXVOTE_COLS], uint32_t* bit) {
  if (!v || !words) { cmx_set_err("cmx_ctxvote_values: bad argument"); return 1; }
  CtxVoteDev h;
  if (hipSetDevice(v->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(&h, v->d, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) {
    cmx_set_err("cmx_ctxvote_values: device error"); return 1;
  }
  memcpy(words, h.words, sizeof h.words);
  if (bit) *bit = h.bit;
  return 0;
}

int cmx_ctxmodels_state_diff(cmx_ctxmodels_t* a, cmx_ctxmodels_t* b, uint64_t out[16]) {
  if (!a || !b || !out) { cmx_set_err("cmx_ctxmodels_state_diff: bad argument"); return 1; }
  if (a == b) { cmx_set_err("cmx_ctxmodels_state_diff: a and b are the same handle"); return 1; }
  const CtxRegion *ra = nullptr, *rb = nullptr; int na = 0, nb = 0, deva = 0, devb = 0;
  if (cmx_ctxmodels_state_view(a, &ra, &na, &deva) || cmx_ctxmodels_state_view(b, &rb, &nb, &devb)) return 1;
  if (deva != devb) { cmx_set_err("cmx_ctxmodels_state_diff: the two handles live on different devices"); return 1; }
  if (na != nb) { cmx_set_err("cmx_ctxmodels_state_diff: internal layout error"); return 1; }
  if (hipSetDevice(deva) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { cmx_set_err("cmx_ctxmodels_state_diff: device error"); return 1; }
  std::vector<CtxDiffDev> h((size_t)na, CtxDiffDev{0, kNone});
  CtxDiffDev* d = nullptr;
  bool ok = hipMalloc((void**)&d, h.size() * sizeof(CtxDiffDev)) == hipSuccess && hipMemcpy(d, h.data(), h.size() * sizeof(CtxDiffDev), hipMemcpyHostToDevice) == hipSuccess;
  for (int r = 0; ok && r < na; ++r) {
    if (ra[r].region != rb[r].region || ra[r].lane != rb[r].lane || ra[r].words != rb[r].words) { ok = false; break; }
    const unsigned long long items = ra[r].words / 4 + 4;
    const unsigned grid = (unsigned)(items / 256 + 1 < 4096 ? items / 256 + 1 : 4096);
    hipLaunchKernelGGL(cmx_ctx_state_diff_kernel, dim3(grid), dim3(256), 0, 0, ra[r].p, rb[r].p, ra[r].words, d + r);
    ok = hipGetLastError() == hipSuccess;
  }
  ok = ok && hipDeviceSynchronize() == hipSuccess && hipMemcpy(h.data(), d, h.size() * sizeof(CtxDiffDev), hipMemcpyDeviceToHost) == hipSuccess;
  for (int i = 0; i < 16; ++i) out[i] = 0;
  for (int i = 1; i <= 5; ++i) out[i] = kNone;
  for (int r = 0; ok && r < na; ++r) {   // (region-then-lane order)
    if (!h[r].cnt) continue;
    out[0] += h[r].cnt; out[6 + ra[r].region] += h[r].cnt;
    if (ra[r].lane >= 0) out[15] |= 1ull << ra[r].lane;
    if (out[1] == kNone) {
      uint32_t x = 0, y = 0;
      ok = hipMemcpy(&x, ra[r].p + h[r].first, 4, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(&y, rb[r].p + h[r].first, 4, hipMemcpyDeviceToHost) == hipSuccess;
      out[1] = (uint64_t)ra[r].region; out[2] = ra[r].lane >= 0 ? (uint64_t)ra[r].lane : kNone; out[3] = h[r].first; out[4] = x; out[5] = y;
    }
  }
  if (d) (void)hipFree(d);
  if (!ok) { (void)hipGetLastError(); cmx_set_err("cmx_ctxmodels_state_diff: device error"); return 1; }
  return 0;
}

int cmx_ctxmodels_debug_state_xor(cmx_ctxmodels_t* h, int region, uint64_t lane, uint64_t index, uint32_t xor_mask) {
  if (!h) { cmx_set_err("cmx_ctxmodels_debug_state_xor: null handle"); return 1; }
  if (!xor_mask) { cmx_set_err("cmx_ctxmodels_debug_state_xor: a zero mask changes nothing"); return 1; }
  const CtxRegion* rg = nullptr; int n = 0, dev = 0;
  if (cmx_ctxmodels_state_view(h, &rg, &n, &dev)) return 1;
  uint32_t* p = nullptr;
  for (int r = 0; r < n && !p; ++r)
    if (rg[r].region == region && (rg[r].lane < 0 ? lane == kNone : lane == (uint64_t)rg[r].lane) && index < rg[r].words) p = rg[r].p + index;
  if (!p) { cmx_set_err("cmx_ctxmodels_debug_state_xor: no such word (region, lane, index out of range)"); return 1; }
  uint32_t x = 0;
  if (hipSetDevice(dev) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(&x, p, 4, hipMemcpyDeviceToHost) != hipSuccess) {
    cmx_set_err("cmx_ctxmodels_debug_state_xor: device error"); return 1;
  }
  x ^= xor_mask;
  if (hipMemcpy(p, &x, 4, hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { cmx_set_err("cmx_ctxmodels_debug_state_xor: device error"); return 1; }
  return 0;
}

int cmx_ctxmodels_debug_layout(uint64_t out[5]) {
  if (!out) { cmx_set_err("cmx_ctxmodels_debug_layout: bad argument"); return 1; }
  out[0] = offsetof(CtxPersist, regs) / 4; out[1] = offsetof(CtxPersist, br_probs) / 4; out[2] = offsetof(CtxPersist, ipred) / 4;
  out[3] = offsetof(CtxPersist, mpred) / 4; out[4] = sizeof(CtxPersist) / 4;
  return 0;
}

}  // extern "C"
