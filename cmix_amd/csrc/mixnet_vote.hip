// mixnet_vote.hip -- the redundant mixing-network vote (C ABI: cmx_vote_*, cmx_mixnet_state_diff, cmx_mixnet_state_repair, cmx_mixnet_debug_state_xor in
// include/cmix_amd.h).
//
// Verify mode (cmx_verify.h) checks every word the network LOADS from HBM against its source. What it cannot see is what the network computes with
// those words: the main workgroup's LDS, the layer-1 / layer-2 rows, the extras, row_steps, the SSE cells. The complementary guard is redundancy:
// the unchanged cmx_mixnet_spec_kernel runs on two or three handles over the same inputs, and two new kernels compare what they produced.
//
//   cmx_vote_kernel        every chunk: the final p and the 47 mixer outputs of every bit of n = 2 or 3 instances, word for word
//   cmx_vote_fold_kernel   behind it: folds the chunk's result into a sticky record and captures the first differing bit
//   cmx_state_diff_kernel  after an event (and in tests): every word of two handles' MixState arrays in HBM
//   cmx_state_repair_kernel  the same walk that also stores the second handle's word over every differing word of the first: an outvoted instance
//                          is made equal to a member of the majority (cmx_mixnet_state_repair), and cmx_verify_reseg_kernel re-digests the layer-0
//                          row segments of a verifying handle that received such a word
//
// Continuing a stream on the majority after an event is the pipeline's business (cmx_pipeline_set_shadow_repair, pipeline_api.hip): the fold
// kernel publishes every chunk's own result for it (cmx_vote_last) beside the sticky record. Out of scope here: the decoder's form of the
// network (a decoder's bits arrive one at a time from the host; its pipeline allocates nothing of this).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/cmix_amd.h"
#include "cmx_vote_core.h"
#include "cmx_state_digest.h"
#include "mixnet_state.h"
#include "cmx_verify.h"

extern "C" int cmx_mixnet_state_view(cmx_mixnet_t* h, const MixState** host, MixState** dev, int* device);   // cmx_api.hip
extern "C" unsigned long long* cmx_mixnet_verify_segments(cmx_mixnet_t* h);   // cmx_api.hip: a verifying handle's stored row-segment digests, else NULL
extern "C" int cmx_mixnet_state_refresh(cmx_mixnet_t* h);                     // cmx_api.hip: the host copy of the block's scalars, from the device

namespace {
constexpr unsigned long long kNone = ~0ull;
constexpr int kCols = CMX_MIXERS + 1;   // 47 mixer outputs, then the final p: the causal order within a bit

struct VoteArgs {
  const uint32_t* p[3];
  const uint32_t* mix[3];
};
// device block of a vote handle
struct VoteDev {
  VoteHead head;
  uint32_t words[3 * kCols];     // capture of the first event's bit: instance i, column c at [i * 48 + c]
  uint32_t sel[CMX_MIXERS];
  uint32_t bit;
};
struct MixRow {   // (the fold's capture; the vote kernel walks the flat arrays itself)
  typedef VoteArgs Args;
  static constexpr int kCols = ::kCols;
  static __device__ __forceinline__ uint32_t word(const VoteArgs& a, int i, unsigned long long t, unsigned c) {
    return c < CMX_MIXERS ? a.mix[i][t * CMX_MIXERS + c] : a.p[i][t];
  }
};

// Items: [0, nq) quads of the flat mix arrays, [nq, nq + pq) quads of p, then the single words either array has left over (all of them when an
// array is not 16-byte aligned: vec == 0). Every lane keeps its own minimum key and count; one reduction per wave at the end.
template <int N>
__global__ void __launch_bounds__(256) cmx_vote_kernel(VoteArgs a, unsigned long long nbits, int vec, VoteHead* d) {
  const unsigned long long nmix = nbits * CMX_MIXERS;
  const unsigned long long nq = vec ? nmix / 4 : 0, pq = vec ? nbits / 4 : 0;
  const unsigned long long mt = nmix - 4 * nq, pt = nbits - 4 * pq;
  const unsigned long long items = nq + pq + mt + pt;
  VoteAcc acc;
  auto mixword = [&](unsigned long long f, uint32_t w0, uint32_t w1, uint32_t w2) {
    const unsigned r = cmx_vote_one<N>(w0, w1, w2);
    if (r) {
      const unsigned long long t = f / CMX_MIXERS, c = f - t * CMX_MIXERS;
      acc.note(t * kCols + c, r);
    }
  };
  auto pword = [&](unsigned long long t, uint32_t w0, uint32_t w1, uint32_t w2) {
    const unsigned r = cmx_vote_one<N>(w0, w1, w2);
    if (r) acc.note(t * kCols + CMX_MIXERS, r);
  };
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (unsigned long long)gridDim.x * blockDim.x) {
    if (i < nq + pq) {
      const bool ism = i < nq;
      const unsigned long long q = ism ? i : i - nq;
      const uint4 v0 = reinterpret_cast<const uint4*>(ism ? a.mix[0] : a.p[0])[q];
      const uint4 v1 = reinterpret_cast<const uint4*>(ism ? a.mix[1] : a.p[1])[q];
      const uint4 v2 = N == 3 ? reinterpret_cast<const uint4*>(ism ? a.mix[2] : a.p[2])[q] : v1;
      if (v0.x != v1.x || v0.y != v1.y || v0.z != v1.z || v0.w != v1.w || v0.x != v2.x || v0.y != v2.y || v0.z != v2.z || v0.w != v2.w) {
        if (ism) { mixword(4 * q, v0.x, v1.x, v2.x); mixword(4 * q + 1, v0.y, v1.y, v2.y); mixword(4 * q + 2, v0.z, v1.z, v2.z); mixword(4 * q + 3, v0.w, v1.w, v2.w); }
        else { pword(4 * q, v0.x, v1.x, v2.x); pword(4 * q + 1, v0.y, v1.y, v2.y); pword(4 * q + 2, v0.z, v1.z, v2.z); pword(4 * q + 3, v0.w, v1.w, v2.w); }
      }
    } else if (i < nq + pq + mt) {
      const unsigned long long f = 4 * nq + (i - nq - pq);
      mixword(f, a.mix[0][f], a.mix[1][f], N == 3 ? a.mix[2][f] : a.mix[1][f]);
    } else {
      const unsigned long long t = 4 * pq + (i - nq - pq - mt);
      pword(t, a.p[0][t], a.p[1][t], N == 3 ? a.p[2][t] : a.p[1][t]);
    }
  }
  acc.flush(d);
}

// behind the vote kernel: the core's fold, and the first event's bit is captured with its selectors
__global__ void cmx_vote_fold_kernel(VoteArgs a, unsigned long long nbits, unsigned long long bit0, int n, const uint32_t* sel, const uint8_t* bits, VoteDev* d) {
  const VoteEvent ev = cmx_vote_fold(&d->head, nbits, bit0, n, kCols);
  if (!ev.capture) return;
  cmx_vote_capture<MixRow>(a, n, ev.row, d->words);
  for (int i = threadIdx.x; i < CMX_MIXERS; i += blockDim.x) d->sel[i] = sel ? sel[ev.row * CMX_MIXERS + i] : 0u;
  if (threadIdx.x == 0) d->bit = bits ? bits[ev.row] : 0u;
}

// ---- state repair: the diff's walk (cmx_vote_core.h), storing y's word over every differing word of x (y is only read) ----
// touched (region 0 of a verifying handle, else NULL): one flag per stored row segment of cmx_verify.h, [row number][CMX_VERIFY_SEGS], set where a word
// the segment's digest covers was repaired. Only differing words are stored, with ordinary 4-byte vector stores: a clean pass writes nothing.
__global__ void __launch_bounds__(256) cmx_state_repair_kernel(uint32_t* x, const uint32_t* y, unsigned long long n, unsigned long long per_mixer, DiffDev* d,
                                                               unsigned* touched) {
  DiffAcc acc;
  cmx_state_walk(x, y, n, [&](unsigned long long i, uint32_t old, uint32_t w) {
    x[i] = w;
    acc.note(i, per_mixer);
    const unsigned long long k = (i << 32) | old;   // (every region has fewer than 2^32 words)
    acc.was = k < acc.was ? k : acc.was;
    if (touched) {
      const unsigned long long row = i / CMX_ROW0_STRIDE;
      const unsigned idx = (unsigned)(i - row * CMX_ROW0_STRIDE);
      if (idx < CMX_IN0) touched[row * CMX_VERIFY_SEGS + (idx < 2048 ? idx >> 9 : CMX_VERIFY_SEGS - 1)] = 1u;   // (the same value from every writer)
    }
  });
  acc.flush<true>(d);
}

// Verify mode's stored digests of the touched layer-0 row segments, recomputed from the repaired rows: one wave per segment, the words and the sum of
// the network kernel's own seg_digest (mixnet_chunk.hip: helper wave w owns words [512 w, 512 w + 512), the last one also 2048..2077). A digest of 0
// (never stored by a verified launch, not checked) stays 0.
__global__ void __launch_bounds__(256) cmx_verify_reseg_kernel(const uint32_t* rows0, const unsigned* touched, unsigned long long* seg, unsigned nseg) {
  const unsigned lane = threadIdx.x & 63;
  const unsigned waves = gridDim.x * (blockDim.x >> 6);
  for (unsigned s = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); s < nseg; s += waves) {
    if (!touched[s] || seg[s] == 0) continue;   // (wave-uniform)
    const unsigned row = s / CMX_VERIFY_SEGS, w = s % CMX_VERIFY_SEGS;
    const uint32_t* r = rows0 + (unsigned long long)row * CMX_ROW0_STRIDE;
    unsigned long long dg = 0;
    for (unsigned k = 0; k < 8; ++k) { const unsigned i = 512 * w + 64 * k + lane; dg += cmx_vmix(CMX_VC_SEGMENT, row, i, r[i]); }
    if (w == CMX_VERIFY_SEGS - 1 && lane < CMX_IN0 - 2048) dg += cmx_vmix(CMX_VC_SEGMENT, row, 2048 + lane, r[2048 + lane]);
    for (int o = 32; o; o >>= 1) dg += __shfl_xor(dg, o);
    if (lane == 0) seg[s] = dg;
  }
}

constexpr unsigned long long kR = CMX_ROWS_PER_MIXER;
constexpr int kRegions = 11;
constexpr unsigned long long kScalarWords = (CMX_MIXERS + 1) + 2 * (CMX_MIXERS + 1) + 2 + 3;   // n_rows, max_steps, steps, sse_j / pc / ffl
struct Region { const uint32_t* p; unsigned long long words, per_mixer; };
void regions_of(const MixState& S, Region r[10]) {
  r[0] = {(const uint32_t*)S.rows0, (unsigned long long)CMX_MIX0 * kR * CMX_ROW0_STRIDE, kR * CMX_ROW0_STRIDE};
  r[1] = {(const uint32_t*)S.rows1, (unsigned long long)CMX_MIX1 * kR * CMX_ROW1_STRIDE, kR * CMX_ROW1_STRIDE};
  r[2] = {(const uint32_t*)S.rows2, kR * CMX_ROW2_STRIDE, kR * CMX_ROW2_STRIDE};
  r[3] = {(const uint32_t*)S.row_steps, (unsigned long long)CMX_MIXERS * kR * 2, 0};
  r[4] = {(const uint32_t*)S.map_keys, (unsigned long long)CMX_MIXERS * CMX_MAP_SLOTS, 0};
  r[5] = {(const uint32_t*)S.map_vals, (unsigned long long)CMX_MIXERS * CMX_MAP_SLOTS, 0};
  r[6] = {(const uint32_t*)S.s6, (unsigned long long)CMX_SM6_VOL * 4, 0};
  r[7] = {(const uint32_t*)S.s7, (unsigned long long)CMX_SM7_VOL * 4, 0};
  r[8] = {(const uint32_t*)S.x1, (unsigned long long)CMX_MIX1_VOL, 0};
  r[9] = {(const uint32_t*)S.x2, (unsigned long long)CMX_MIX2_VOL, 0};
}
// region 10: the scalars of a MixState block (host copy of the DEVICE block) as words, in the order n_rows, max_steps, steps, sse_j, sse_pc, sse_ffl
void scalar_words(const MixState& S, uint32_t w[kScalarWords]) {
  size_t k = 0;
  memcpy(w + k, S.n_rows, sizeof S.n_rows); k += CMX_MIXERS + 1;
  memcpy(w + k, S.max_steps, sizeof S.max_steps); k += 2 * (CMX_MIXERS + 1);
  memcpy(w + k, &S.steps, 8); k += 2;
  w[k++] = S.sse_j; w[k++] = S.sse_pc; w[k++] = S.sse_ffl;
}
// byte offset of scalar word `index` inside MixState
size_t scalar_offset(unsigned long long index) {
  if (index < CMX_MIXERS + 1) return offsetof(MixState, n_rows) + 4 * index;
  index -= CMX_MIXERS + 1;
  if (index < 2 * (CMX_MIXERS + 1)) return offsetof(MixState, max_steps) + 4 * index;
  index -= 2 * (CMX_MIXERS + 1);
  if (index < 2) return offsetof(MixState, steps) + 4 * index;
  index -= 2;
  return index == 0 ? offsetof(MixState, sse_j) : index == 1 ? offsetof(MixState, sse_pc) : offsetof(MixState, sse_ffl);
}
// (mixer, row, index) of word i of a region; kNone where a field does not apply
void locate(int region, unsigned long long i, unsigned long long out[3]) {
  out[0] = out[1] = kNone; out[2] = i;
  switch (region) {
    case 0: out[0] = i / (kR * CMX_ROW0_STRIDE); out[1] = i / CMX_ROW0_STRIDE % kR; out[2] = i % CMX_ROW0_STRIDE; break;
    case 1: out[0] = CMX_MIX0 + i / (kR * CMX_ROW1_STRIDE); out[1] = i / CMX_ROW1_STRIDE % kR; out[2] = i % CMX_ROW1_STRIDE; break;
    case 2: out[0] = CMX_MIXERS - 1; out[1] = i / CMX_ROW2_STRIDE; out[2] = i % CMX_ROW2_STRIDE; break;
    case 3: out[0] = i / 2 / kR; out[1] = i / 2 % kR; out[2] = i % 2; break;
    case 4: case 5: out[0] = i / CMX_MAP_SLOTS; out[2] = i % CMX_MAP_SLOTS; break;
    default: break;
  }
}
// the inverse, with bounds: word number inside the region, or kNone
unsigned long long word_of(int region, unsigned long long mixer, unsigned long long row, unsigned long long index, const Region r[10]) {
  switch (region) {
    case 0: return mixer < CMX_MIX0 && row < kR && index < CMX_ROW0_STRIDE ? (mixer * kR + row) * CMX_ROW0_STRIDE + index : kNone;
    case 1: return mixer >= CMX_MIX0 && mixer < CMX_MIX0 + CMX_MIX1 && row < kR && index < CMX_ROW1_STRIDE ? ((mixer - CMX_MIX0) * kR + row) * CMX_ROW1_STRIDE + index : kNone;
    case 2: return (mixer == CMX_MIXERS - 1 || mixer == kNone) && row < kR && index < CMX_ROW2_STRIDE ? row * CMX_ROW2_STRIDE + index : kNone;
    case 3: return mixer < CMX_MIXERS && row < kR && index < 2 ? (mixer * kR + row) * 2 + index : kNone;
    case 4: case 5: return mixer < CMX_MIXERS && index < CMX_MAP_SLOTS ? mixer * CMX_MAP_SLOTS + index : kNone;
    case 6: case 7: case 8: case 9: return index < r[region].words ? index : kNone;
    case 10: return index < kScalarWords ? index : kNone;
    default: return kNone;
  }
}
}  // namespace

struct cmx_vote : VoteHandle {};

extern "C" {

cmx_vote_t* cmx_vote_create(int device, int n) { return vote_create<cmx_vote>("cmx_vote_create", device, n, sizeof(VoteDev)); }
void cmx_vote_destroy(cmx_vote_t* v) { vote_destroy(v); }

int cmx_vote_run(cmx_vote_t* v, const float* const* d_p, const float* const* d_mix, size_t nbits, uint64_t stream_bit0, const uint32_t* d_sel, const uint8_t* d_bits,
                 void* stream) {
  if (!v || !d_p || !d_mix) { cmx_set_err("cmx_vote_run: bad argument"); return 1; }
  if (nbits == 0) return 0;
  if (nbits > 0x7fffffff) { cmx_set_err("cmx_vote_run: chunk too large"); return 1; }
  VoteArgs a;
  memset(&a, 0, sizeof a);
  int vec = 1;
  for (int i = 0; i < v->n; ++i) {
    if (!d_p[i] || !d_mix[i]) { cmx_set_err("cmx_vote_run: null array of instance " + std::to_string(i)); return 1; }
    a.p[i] = (const uint32_t*)d_p[i]; a.mix[i] = (const uint32_t*)d_mix[i];
    if (((uintptr_t)d_p[i] | (uintptr_t)d_mix[i]) & 15) vec = 0;   // 16-byte loads need every array aligned
  }
  if (hipSetDevice(v->device) != hipSuccess) { cmx_set_err("hipSetDevice failed"); return 1; }
  hipStream_t st = (hipStream_t)stream;
  const unsigned long long words = (unsigned long long)nbits * kCols;
  const unsigned long long items = vec ? words / 4 + 8 : words;
  const unsigned grid = (unsigned)(items / 256 + 1 < 1024 ? items / 256 + 1 : 1024);
  if (v->n == 3) hipLaunchKernelGGL(cmx_vote_kernel<3>, dim3(grid), dim3(256), 0, st, a, (unsigned long long)nbits, vec, v->d);
  else hipLaunchKernelGGL(cmx_vote_kernel<2>, dim3(grid), dim3(256), 0, st, a, (unsigned long long)nbits, vec, v->d);
  hipLaunchKernelGGL(cmx_vote_fold_kernel, dim3(1), dim3(64), 0, st, a, (unsigned long long)nbits, (unsigned long long)stream_bit0, v->n, d_sel, d_bits, (VoteDev*)v->d);
  if (hipGetLastError() != hipSuccess) { cmx_set_err("cmx_vote_run: kernel launch failed"); return 1; }
  return 0;
}

const unsigned long long* cmx_vote_record(cmx_vote_t* v) { return v && v->d ? v->d->rec : nullptr; }

int cmx_vote_report(cmx_vote_t* v, uint64_t out[8]) { return vote_report("cmx_vote_report", v, out); }
int cmx_vote_last(cmx_vote_t* v, uint64_t out[4]) { return vote_last("cmx_vote_last", v, out); }

int cmx_vote_values(cmx_vote_t* v, uint32_t words[144], uint32_t sel[47], uint32_t* bit) {
  VoteDev h;
  if (vote_values("cmx_vote_values", v, words, &h)) return 1;
  memcpy(words, h.words, sizeof h.words);
  if (sel) memcpy(sel, h.sel, sizeof h.sel);
  if (bit) *bit = h.bit;
  return 0;
}

// cmx_mixnet_state_diff (repair == false) and cmx_mixnet_state_repair (true: b's word goes over every differing word of a) are one walk
static int state_walk(cmx_mixnet_t* a, cmx_mixnet_t* b, uint64_t out[20], bool repair) {
  const std::string who = repair ? "cmx_mixnet_state_repair" : "cmx_mixnet_state_diff";
  if (!a || !b || !out) { cmx_set_err(who + ": bad argument"); return 1; }
  if (repair && a == b) { cmx_set_err(who + ": dst and src are the same handle"); return 1; }
  const MixState *ha = nullptr, *hb = nullptr; MixState *da = nullptr, *db = nullptr; int deva = 0, devb = 0;
  if (cmx_mixnet_state_view(a, &ha, &da, &deva) || cmx_mixnet_state_view(b, &hb, &db, &devb)) return 1;
  if (deva != devb) { cmx_set_err(who + ": the two handles live on different devices"); return 1; }
  if (hipSetDevice(deva) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { cmx_set_err(who + ": device error"); return 1; }
  Region ra[10], rb[10];
  regions_of(*ha, ra); regions_of(*hb, rb);
  // a verifying dst: its stored row-segment digests must follow the repaired layer-0 rows (the next reload would raise a false alarm otherwise)
  unsigned long long* vseg = repair ? cmx_mixnet_verify_segments(a) : nullptr;
  unsigned* touched = nullptr;
  const unsigned nseg = CMX_MIX0 * CMX_ROWS_PER_MIXER * CMX_VERIFY_SEGS;
  bool ok = !vseg || (hipMalloc((void**)&touched, (size_t)nseg * 4) == hipSuccess && hipMemset(touched, 0, (size_t)nseg * 4) == hipSuccess);
  DiffDev h[kRegions];
  for (DiffDev& x : h) x = {0, kNone, 0, kNone};   // (region 10, the scalars, is compared on the host, below)
  ok = ok && state_each_array(10, h, [&](int r, DiffDev* d) {
    const unsigned grid = state_grid(ra[r].words, 4096);
    if (repair) hipLaunchKernelGGL(cmx_state_repair_kernel, dim3(grid), dim3(256), 0, 0, (uint32_t*)ra[r].p, rb[r].p, ra[r].words, ra[r].per_mixer, d, r == 0 ? touched : nullptr);
    else hipLaunchKernelGGL(cmx_state_diff_kernel, dim3(grid), dim3(256), 0, 0, ra[r].p, rb[r].p, ra[r].words, ra[r].per_mixer, d);
  });
  MixState sa, sb;
  if (ok && touched && h[0].cnt) {   // (behind the repair kernel on the same stream)
    hipLaunchKernelGGL(cmx_verify_reseg_kernel, dim3(2048), dim3(256), 0, 0, ra[0].p, touched, vseg, nseg);
    ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  }
  ok = ok && hipMemcpy(&sa, da, sizeof sa, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(&sb, db, sizeof sb, hipMemcpyDeviceToHost) == hipSuccess;
  uint32_t wa[kScalarWords], wb[kScalarWords];
  if (ok) {
    scalar_words(sa, wa); scalar_words(sb, wb);
    for (unsigned long long i = 0; ok && i < kScalarWords; ++i)
      if (wa[i] != wb[i]) {
        if (!h[10].cnt) h[10].first = i;
        h[10].cnt++;
        if (repair) ok = hipMemcpy((char*)da + scalar_offset(i), &wb[i], 4, hipMemcpyHostToDevice) == hipSuccess;
      }
    if (repair && h[10].cnt) ok = ok && cmx_mixnet_state_refresh(a) == 0;
  }
  for (int i = 0; i < 20; ++i) out[i] = 0;
  for (int i = 1; i <= 6; ++i) out[i] = kNone;
  for (int r = 0; ok && r < kRegions; ++r) {
    out[0] += h[r].cnt; out[7 + r] = h[r].cnt;
    if (h[r].cnt && out[1] == kNone) {
      unsigned long long loc[3];
      locate(r, h[r].first, loc);
      uint32_t x = 0, y = 0;
      if (r < 10) {
        ok = hipMemcpy(&y, rb[r].p + h[r].first, 4, hipMemcpyDeviceToHost) == hipSuccess;
        if (repair) x = (uint32_t)h[r].was;   // (dst holds src's word by now)
        else ok = ok && hipMemcpy(&x, ra[r].p + h[r].first, 4, hipMemcpyDeviceToHost) == hipSuccess;
      } else { x = wa[h[r].first]; y = wb[h[r].first]; }
      out[1] = (uint64_t)r; out[2] = loc[0]; out[3] = loc[1]; out[4] = loc[2]; out[5] = x; out[6] = y;
    }
  }
  out[18] = h[0].mask;
  out[19] = h[1].mask | (h[2].mask ? 1ull << CMX_MIX1 : 0);
  if (touched) (void)hipFree(touched);
  if (!ok) { (void)hipGetLastError(); cmx_set_err(who + ": device error"); return 1; }
  return 0;
}
int cmx_mixnet_state_diff(cmx_mixnet_t* a, cmx_mixnet_t* b, uint64_t out[20]) { return state_walk(a, b, out, false); }
int cmx_mixnet_state_repair(cmx_mixnet_t* dst, cmx_mixnet_t* src, uint64_t out[20]) { return state_walk(dst, src, out, true); }

// the ten arrays of regions_of, then region 10: the scalar words
static int mix_digest(const char* who, cmx_mixnet_t* net, uint64_t* out, size_t cap, int layout) {
  if (!net) { cmx_set_err(std::string(who) + ": null handle"); return -1; }
  const MixState* hs = nullptr; MixState* ds = nullptr; int dev = 0;
  if (cmx_mixnet_state_view(net, &hs, &ds, &dev)) return -1;
  Region r[10];
  regions_of(*hs, r);
  StateArray a[10];
  for (int i = 0; i < 10; ++i) a[i] = {(uint32_t*)r[i].p, r[i].words, i, -1};
  std::vector<uint32_t> w(kScalarWords);
  if (out && !layout) {
    MixState s;
    if (hipSetDevice(dev) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(&s, ds, sizeof s, hipMemcpyDeviceToHost) != hipSuccess) {
      (void)hipGetLastError(); cmx_set_err(std::string(who) + ": device error"); return -1;
    }
    scalar_words(s, w.data());
  }
  return cmx_state_digest_stage(who, dev, a, 10, &w, 10, out, cap, layout);
}
int cmx_mixnet_state_digest(cmx_mixnet_t* net, uint64_t* out, size_t cap) { return mix_digest("cmx_mixnet_state_digest", net, out, cap, 0); }
int cmx_mixnet_state_digest_layout(cmx_mixnet_t* net, uint64_t* out, size_t cap) { return mix_digest("cmx_mixnet_state_digest_layout", net, out, cap, 1); }

int cmx_mixnet_debug_state_xor(cmx_mixnet_t* net, int region, uint64_t mixer, uint64_t row, uint64_t index, uint32_t xor_mask) {
  if (!net) { cmx_set_err("cmx_mixnet_debug_state_xor: null handle"); return 1; }
  if (!xor_mask) { cmx_set_err("cmx_mixnet_debug_state_xor: a zero mask changes nothing"); return 1; }
  const MixState* hs = nullptr; MixState* ds = nullptr; int dev = 0;
  if (cmx_mixnet_state_view(net, &hs, &ds, &dev)) return 1;
  Region r[10];
  regions_of(*hs, r);
  const unsigned long long w = word_of(region, mixer, row, index, r);
  if (w == kNone) { cmx_set_err("cmx_mixnet_debug_state_xor: no such word (region, mixer, row, index out of range)"); return 1; }
  uint32_t* p = region < 10 ? (uint32_t*)r[region].p + w : (uint32_t*)((char*)ds + scalar_offset(w));
  return state_xor("cmx_mixnet_debug_state_xor", dev, p, xor_mask);
}

}  // extern "C"
