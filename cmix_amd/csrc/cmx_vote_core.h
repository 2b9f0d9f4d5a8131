// cmx_vote_core.h -- what the four redundant votes share (mixnet_vote.hip, ctxmodels_vote.hip, lstm_vote.hip, fxcm_vote.hip): the rule, the head of a
// vote handle's device block, the per-lane accumulator and its reduction, the fold step's bookkeeping, the state-diff walk, and the host plumbing of
// the handles and of the state hooks. Each stage's file keeps what only it knows: which words make up a row and how they are loaded, the capture's
// extras, its state arrays and the layout of its public out[].
//
// THE RULE. n = 2 or 3 instances produce rows of kCols 32-bit words; element e = row * kCols + column. n = 3: all equal agree, exactly two equal make
// the third the odd instance, all different is no majority; n = 2: different is no majority. A chunk's vote kernel leaves in the head the smallest
// non-agreeing element with its odd instance (key), the number of non-agreeing elements (cnt) and the set of odd instances seen (odd); the fold
// kernel behind it turns them into the sticky record rec[] and the chunk's own result last[] (cmx_vote_fold) and resets them.
#ifndef CMX_VOTE_CORE_H
#define CMX_VOTE_CORE_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/cmix_amd.h"

void cmx_set_err(const std::string& s);  // cmx_api.hip

constexpr unsigned long long kVoteNone = ~0ull;

// ---- device: the rule, the accumulator, the fold ----

// the first member of every stage's device block
struct VoteHead {
  unsigned long long rec[8];     // the sticky record (cmx_*vote_report)
  unsigned long long last[4];    // the chunk folded last (cmx_*vote_last), right behind the record: one copy fetches both
  unsigned long long key;        // this chunk: min over non-agreeing elements of (e << 2 | odd instance, 3 = no majority); ~0 = none
  unsigned long long cnt;        // this chunk: non-agreeing elements
  unsigned long long odd;        // this chunk: bit i = instance i was the odd one of some element, bit 3 = some element had no majority
  unsigned long long pad;
};

// one element of n instances: 0 agree, else 1 + (odd instance, 3 = no majority)
template <int N>
__device__ __forceinline__ unsigned cmx_vote_one(uint32_t a, uint32_t b, uint32_t c) {
  if (N == 2) return a == b ? 0u : 4u;
  if (a == b && b == c) return 0u;
  if (b == c) return 1u;
  if (a == c) return 2u;
  if (a == b) return 3u;
  return 4u;
}

// Every lane of a vote kernel keeps its own minimum key, count and odd mask; one reduction per wave at the end, and atomics only from waves that saw
// a difference.
struct VoteAcc {
  unsigned long long key = kVoteNone, cnt = 0;
  unsigned odd = 0;
  // element e does not agree: r = cmx_vote_one's answer (1..4)
  __device__ __forceinline__ void note(unsigned long long e, unsigned r) {
    const unsigned long long k = (e << 2) | (r - 1);
    key = k < key ? k : key; ++cnt; odd |= 1u << (r - 1);
  }
  __device__ __forceinline__ void flush(VoteHead* d) {
    if (__ballot(cnt != 0) == 0) return;   // (wave-uniform) nothing differed in this wave
    for (int o = 32; o; o >>= 1) {
      const unsigned long long k2 = __shfl_xor(key, o), c2 = __shfl_xor(cnt, o);
      key = k2 < key ? k2 : key; cnt += c2; odd |= __shfl_xor(odd, o);
    }
    if ((threadIdx.x & 63) == 0) { atomicMin(&d->key, key); atomicAdd(&d->cnt, cnt); atomicOr(&d->odd, (unsigned long long)odd); }
  }
};

// The vote kernel of a stage whose row is kCols words behind an accessor S::word(args, instance, row, c): one wavefront per row, grid-stride over the
// rows, a row in passes of 64 elements. 4-byte loads only: nothing is assumed about the arrays' alignment.
template <int N, class S>
__global__ void __launch_bounds__(256) cmx_rowvote_kernel(typename S::Args a, unsigned long long nrows, VoteHead* d) {
  const unsigned lane = threadIdx.x & 63;
  const unsigned long long waves = (unsigned long long)gridDim.x * (blockDim.x >> 6);
  VoteAcc acc;
  for (unsigned long long t = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < nrows; t += waves) {
    for (unsigned c = lane; c < (unsigned)S::kCols; c += 64) {
      const uint32_t w0 = S::word(a, 0, t, c), w1 = S::word(a, 1, t, c), w2 = N == 3 ? S::word(a, 2, t, c) : w1;
      const unsigned r = cmx_vote_one<N>(w0, w1, w2);
      if (r) acc.note(t * S::kCols + c, r);
    }
  }
  acc.flush(d);
}

// The fold kernel's bookkeeping (one wave, behind the vote kernel on the same stream): the chunk's key and count go into the sticky record, and the
// chunk's OWN result into last[]: [0] its non-agreeing elements (0: the instances agree, the rest is 0), [1] the stream position and [2] the column
// of the first of them, [3] the odd instance -- the one instance that was odd wherever the chunk's elements did not agree -- or ~0 for no majority:
// an element at which all differ (or n = 2), or two elements with different odd instances. pos0 = the stream position of the chunk's first row.
// Returns whether the caller is to capture the row of the handle's first event, and which.
struct VoteEvent { bool capture; unsigned long long row, col; };
__device__ __forceinline__ VoteEvent cmx_vote_fold(VoteHead* d, unsigned long long nrows, unsigned long long pos0, int n, int cols) {
  const unsigned long long key = d->key, cnt = d->cnt, odd = d->odd;
  const bool first = cnt != 0 && d->rec[3] == 0;   // (read by every lane before lane 0 writes: one wave, the barrier below orders it)
  __syncthreads();
  const unsigned long long e = key >> 2, t = e / cols, c = e - t * cols;
  if (threadIdx.x == 0) {
    d->rec[0] += 1; d->rec[1] += nrows; d->rec[2] = (unsigned long long)n;
    if (cnt) d->rec[3] += 1;
    if (first) { d->rec[4] = pos0 + t; d->rec[5] = c; d->rec[6] = (key & 3) == 3 ? kVoteNone : (key & 3); d->rec[7] = cnt; }
    d->last[0] = cnt; d->last[1] = cnt ? pos0 + t : 0; d->last[2] = cnt ? c : 0;
    d->last[3] = !cnt ? 0 : odd == 1 ? 0 : odd == 2 ? 1 : odd == 4 ? 2 : kVoteNone;
    d->key = kVoteNone; d->cnt = 0; d->odd = 0;   // the next chunk starts clean
  }
  return {first && t < nrows, t, c};
}
// the capture of row t: instance i, column c at words[i * kCols + c]
template <class S>
__device__ __forceinline__ void cmx_vote_capture(const typename S::Args& a, int n, unsigned long long t, uint32_t* words) {
  for (int i = threadIdx.x; i < n * S::kCols; i += blockDim.x) {
    const int inst = i / S::kCols;
    words[i] = S::word(a, inst, t, (unsigned)(i - inst * S::kCols));
  }
}

// The rest has internal linkage: every file that uses it carries its own copy (a kernel in its own code object), and the library exports nothing of it.
namespace {
// ---- device: the state walk (every word of two arrays; one launch per array) ----
struct DiffDev {
  unsigned long long cnt, first, mask;
  unsigned long long was;   // repair only: min over the repaired words of (word number << 32 | the word dst held), so the first one's old value survives
};
struct DiffAcc {
  unsigned long long first = kVoteNone, cnt = 0, mask = 0, was = kVoteNone;
  // word i differs; per_mixer: words per mixer of the array (0: it has no mixer mask)
  __device__ __forceinline__ void note(unsigned long long i, unsigned long long per_mixer) {
    ++cnt; first = i < first ? i : first;
    if (per_mixer) mask |= 1ull << (i / per_mixer);
  }
  template <bool kWas>
  __device__ __forceinline__ void flush(DiffDev* d) {
    if (__ballot(cnt != 0) == 0) return;
    for (int o = 32; o; o >>= 1) {
      const unsigned long long f2 = __shfl_xor(first, o), c2 = __shfl_xor(cnt, o), m2 = __shfl_xor(mask, o);
      first = f2 < first ? f2 : first; cnt += c2; mask |= m2;
      if (kWas) { const unsigned long long w2 = __shfl_xor(was, o); was = w2 < was ? w2 : was; }
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMin(&d->first, first); atomicAdd(&d->cnt, cnt);
      if (mask) atomicOr(&d->mask, mask);
      if (kWas) atomicMin(&d->was, was);
    }
  }
};
// differ(i, x's word, y's word) for every word i at which the arrays differ: 16-byte loads, then the single words left over (every array is a
// hipMalloc of its own: 16-byte aligned)
template <class F>
__device__ __forceinline__ void cmx_state_walk(const uint32_t* x, const uint32_t* y, unsigned long long n, F differ) {
  const unsigned long long nq = n / 4, items = nq + (n - 4 * nq);
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (unsigned long long)gridDim.x * blockDim.x) {
    if (i < nq) {
      const uint4 u = reinterpret_cast<const uint4*>(x)[i], v = reinterpret_cast<const uint4*>(y)[i];
      if (u.x != v.x) differ(4 * i, u.x, v.x);
      if (u.y != v.y) differ(4 * i + 1, u.y, v.y);
      if (u.z != v.z) differ(4 * i + 2, u.z, v.z);
      if (u.w != v.w) differ(4 * i + 3, u.w, v.w);
    } else {
      const unsigned long long j = 4 * nq + (i - nq);
      const uint32_t u = x[j], v = y[j];
      if (u != v) differ(j, u, v);
    }
  }
}
__global__ void __launch_bounds__(256) cmx_state_diff_kernel(const uint32_t* x, const uint32_t* y, unsigned long long n, unsigned long long per_mixer, DiffDev* d) {
  DiffAcc acc;
  cmx_state_walk(x, y, n, [&](unsigned long long i, uint32_t, uint32_t) { acc.note(i, per_mixer); });
  acc.flush<false>(d);
}

// ---- host: the handle ----
struct VoteHandle {   // what a cmx_*vote_t is
  int device = 0, n = 0;
  VoteHead* d = nullptr;   // the stage's device block
  size_t bytes = 0;        // of that block
};

template <class H>
H* vote_create(const std::string& who, int device, int n, size_t bytes) {
  if (n != 2 && n != 3) { cmx_set_err(who + ": n must be 2 or 3 instances"); return nullptr; }
  if (cmx_device_count() <= 0) { cmx_set_err(who + ": no HIP device visible (a gfx950 GPU is required)"); return nullptr; }
  if (device < 0 || device >= cmx_device_count() || hipSetDevice(device) != hipSuccess) { cmx_set_err(who + ": bad device index"); return nullptr; }
  H* v = new H();
  v->device = device; v->n = n; v->bytes = bytes;
  std::vector<unsigned char> init(bytes, 0);
  memcpy(init.data() + offsetof(VoteHead, key), &kVoteNone, sizeof kVoteNone);
  if (hipMalloc((void**)&v->d, bytes) != hipSuccess || hipMemcpy(v->d, init.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    if (v->d) (void)hipFree(v->d);
    delete v;
    cmx_set_err(who + ": hipMalloc failed");
    return nullptr;
  }
  return v;
}
template <class H>
void vote_destroy(H* v) {
  if (!v) return;
  (void)hipSetDevice(v->device);
  (void)hipDeviceSynchronize();
  if (v->d) (void)hipFree(v->d);
  delete v;
}
// the first `bytes` of the block, after everything queued on the device
int vote_fetch(const std::string& who, const VoteHandle* v, void* out, size_t bytes) {
  if (hipSetDevice(v->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, v->d, bytes, hipMemcpyDeviceToHost) != hipSuccess) {
    cmx_set_err(who + ": device error"); return 1;
  }
  return 0;
}
int vote_report(const std::string& who, const VoteHandle* v, uint64_t out[8]) {
  if (!v || !out) { cmx_set_err(who + ": bad argument"); return 1; }
  VoteHead h;
  if (vote_fetch(who, v, &h, sizeof h.rec)) return 1;
  for (int i = 0; i < 8; ++i) out[i] = h.rec[i];
  return 0;
}
int vote_last(const std::string& who, const VoteHandle* v, uint64_t out[4]) {
  if (!v || !out) { cmx_set_err(who + ": bad argument"); return 1; }
  VoteHead h;
  if (vote_fetch(who, v, &h, sizeof h.rec + sizeof h.last)) return 1;
  for (int i = 0; i < 4; ++i) out[i] = h.last[i];
  return 0;
}
// the capture: the whole block
template <class Dev>
int vote_values(const std::string& who, const VoteHandle* v, const void* words, Dev* h) {
  if (!v || !words) { cmx_set_err(who + ": bad argument"); return 1; }
  return vote_fetch(who, v, h, sizeof *h);
}
// four rows (waves) per workgroup; 2048 waves stride over the rest
unsigned vote_row_grid(unsigned long long nrows) { return (unsigned)((nrows + 3) / 4 < 512 ? (nrows + 3) / 4 : 512); }

// ---- host: state arrays (cmx_*_state_diff, cmx_*_debug_state_xor, cmx_*_debug_layout) ----
struct StateArray {   // one array of a handle's state in HBM; lane: -1 where the stage's regions have none
  uint32_t* p; unsigned long long words; int region; int lane;
};
// a stage's own list (its p, words, region) as StateArrays
template <class R>
std::vector<StateArray> state_arrays(const R* rg, int n) {
  std::vector<StateArray> a((size_t)n);
  for (int r = 0; r < n; ++r) a[r] = {rg[r].p, rg[r].words, rg[r].region, -1};
  return a;
}
// Per-array results h[n] of one walk: h[r] starts as (0, ~0, 0, ~0), launch(r, device address of h[r]) queues array r's kernel; synchronises.
// false: a device error.
template <class Launch>
bool state_each_array(int n, DiffDev* h, Launch launch) {
  for (int r = 0; r < n; ++r) h[r] = {0, kVoteNone, 0, kVoteNone};
  DiffDev* d = nullptr;
  bool ok = hipMalloc((void**)&d, n * sizeof(DiffDev)) == hipSuccess && hipMemcpy(d, h, n * sizeof(DiffDev), hipMemcpyHostToDevice) == hipSuccess;
  for (int r = 0; ok && r < n; ++r) { launch(r, d + r); ok = hipGetLastError() == hipSuccess; }
  ok = ok && hipDeviceSynchronize() == hipSuccess && hipMemcpy(h, d, n * sizeof(DiffDev), hipMemcpyDeviceToHost) == hipSuccess;
  if (d) (void)hipFree(d);
  return ok;
}
unsigned state_grid(unsigned long long words, unsigned cap) {
  const unsigned long long items = words / 4 + 4;
  return (unsigned)(items / 256 + 1 < cap ? items / 256 + 1 : cap);
}
// two equal-shaped lists of arrays, word for word: h[r] = array r's (cnt, first). false: the shapes differ or a device error.
bool state_diff_arrays(const StateArray* a, const StateArray* b, int n, unsigned grid_cap, DiffDev* h) {
  for (int r = 0; r < n; ++r)
    if (a[r].region != b[r].region || a[r].lane != b[r].lane || a[r].words != b[r].words) return false;
  return state_each_array(n, h, [&](int r, DiffDev* d) {
    hipLaunchKernelGGL(cmx_state_diff_kernel, dim3(state_grid(a[r].words, grid_cap)), dim3(256), 0, 0, a[r].p, b[r].p, a[r].words, 0ull, d);
  });
}
// word i of a and of b
bool state_fetch_pair(const StateArray& a, const StateArray& b, unsigned long long i, uint32_t* x, uint32_t* y) {
  return hipMemcpy(x, a.p + i, 4, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(y, b.p + i, 4, hipMemcpyDeviceToHost) == hipSuccess;
}
// offset of array r inside its region (a region's arrays stand together)
unsigned long long state_offset(const StateArray* a, int r) {
  unsigned long long off = 0;
  for (int i = r - 1; i >= 0 && a[i].region == a[r].region; --i) off += a[i].words;
  return off;
}
// word `index` of `region`, or NULL
uint32_t* state_word(const StateArray* a, int n, int region, unsigned long long index) {
  for (int r = 0; r < n; ++r) {
    const unsigned long long off = state_offset(a, r);
    if (a[r].region == region && index >= off && index - off < a[r].words) return a[r].p + (index - off);
  }
  return nullptr;
}
// the xor hooks' tail: *p ^= xor_mask on the device, behind everything queued
int state_xor(const std::string& who, int device, uint32_t* p, uint32_t xor_mask) {
  uint32_t x = 0;
  if (hipSetDevice(device) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(&x, p, 4, hipMemcpyDeviceToHost) != hipSuccess) {
    cmx_set_err(who + ": device error"); return 1;
  }
  x ^= xor_mask;
  if (hipMemcpy(p, &x, 4, hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { cmx_set_err(who + ": device error"); return 1; }
  return 0;
}
// the (region, offset, words) triples of cmx_*_debug_layout
void state_layout(const StateArray* a, int n, uint64_t* out) {
  for (int r = 0; r < n; ++r) { out[3 * r] = (uint64_t)a[r].region; out[3 * r + 1] = state_offset(a, r); out[3 * r + 2] = a[r].words; }
}
}  // namespace
#endif
