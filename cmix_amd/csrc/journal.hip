// journal.hip -- the stream journal (C ABI: cmx_journal_* in include/cmix_amd.h; numpy model: cmix_amd/journal.py).
//
// Per block of 2^k stream bits, 179 order-independent 64-bit digests of what the final mixing network read and wrote: 130 groups of sixteen layer-0
// columns, the final p, the 47 selectors and the coded bits -- the digest of the reference-side trace tools, so that a run can be compared with the
// unmodified reference, with another run, or (p and bits, journal_host.cpp) with its own decode, block by block and stage by stage.
//
//   cmx_journal_kernel   one launch per chunk: streams the chunk's rows once. A workgroup of four waves takes 64 consecutive rows, a wave one row at a
//                        time: 1039 8-byte loads (a row of 2078 floats is 8-byte aligned only), lane l of load i holding columns 128 i + 2 l and the next.
//                        A[c] of a lane's 34 columns stays in registers; B of the wave's rows is computed once, a row per lane, and read by lane index.
//                        Sums stay in registers over the workgroup's rows of one block, are reduced across the eight lanes of a column group, across the
//                        waves through LDS, and leave as one 64-bit integer atomic add per (workgroup, word, block): exact and independent of order.
//
// The device holds a chunk's PARTIAL records only (one per block the chunk touches); the list of blocks lives on the host, which folds the partial
// records with wrapping adds (cmx_journal_fold). Nothing here touches another kernel, and nothing runs unless a journal was asked for.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <array>
#include <string>
#include <vector>

#include "cmx_journal.h"

void cmx_set_err(const std::string& s);  // cmx_api.hip

namespace {
constexpr int kCols = CMX_N_INPUTS;          // 2078
constexpr int kPairs = kCols / 2;            // 1039 8-byte loads per row
constexpr int kIter = (kPairs + 63) / 64;    // 17 per lane
constexpr int kWords = CMX_JOURNAL_WORDS;    // 179
constexpr int kSel = CMX_N_MIXERS;           // 47
constexpr int kWaves = 4;
constexpr int kWgRows = 64;                  // rows per workgroup: at most 16 per wave and run, so one lane per row holds B
static_assert(kCols == 2078 && kSel == 47 && kWords == 130 + 1 + kSel + 1, "the record's layout is the reference trace's");
static_assert(kWgRows / kWaves <= 64, "a wave keeps B of its rows one per lane");

__device__ inline unsigned long long wave_read(unsigned long long v, int lane) {   // v of lane `lane` (wave-uniform index)
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(256) void cmx_journal_kernel(const uint2* __restrict__ rows, unsigned long long ld2, const uint32_t* __restrict__ sel,
                                                          const uint8_t* __restrict__ bits, const uint32_t* __restrict__ p, unsigned nbits,
                                                          unsigned long long bit0, int k, unsigned long long* __restrict__ part) {
  __shared__ unsigned long long red[kWaves][kWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long a0[kIter], a1[kIter];
#pragma unroll
  for (int i = 0; i < kIter; ++i) {
    const int c = 2 * (i * 64 + lane);
    a0[i] = c < kCols ? (cmx_journal_splitmix64((unsigned long long)c) | 1ull) : 0ull;
    a1[i] = c + 1 < kCols ? (cmx_journal_splitmix64((unsigned long long)c + 1) | 1ull) : 0ull;
  }
  const unsigned r0 = blockIdx.x * kWgRows;
  const unsigned r1 = r0 + kWgRows < nbits ? r0 + kWgRows : nbits;
  const unsigned long long blk0 = bit0 >> k;
  unsigned r = r0;
  while (r < r1) {   // one run = the workgroup's rows of one block (workgroup-uniform: every wave takes every barrier)
    const unsigned long long t = bit0 + r, blk = t >> k;
    const unsigned long long left = ((blk + 1) << k) - t;
    const unsigned run_end = (unsigned long long)(r1 - r) < left ? r1 : r + (unsigned)left;
    unsigned long long acc[kIter], accx = 0;
#pragma unroll
    for (int i = 0; i < kIter; ++i) acc[i] = 0;
    const unsigned long long bv = cmx_journal_B(t + (unsigned)wave + (unsigned)(kWaves * lane));   // B of this wave's lane-th row of the run
    int q = 0;
    for (unsigned row = r + wave; row < run_end; row += kWaves, ++q) {
      const unsigned long long b = wave_read(bv, q);
      if (rows) {
        const uint2* rp = rows + (unsigned long long)row * ld2 + lane;
        uint2 v[kIter];
#pragma unroll
        for (int i = 0; i < kIter - 1; ++i) v[i] = rp[i * 64];
        v[kIter - 1] = (kIter - 1) * 64 + lane < kPairs ? rp[(kIter - 1) * 64] : make_uint2(0u, 0u);   // (its A's are zero past the row's end)
#pragma unroll
        for (int i = 0; i < kIter; ++i) acc[i] += (((unsigned long long)v[i].x + 1ull) * a0[i] + ((unsigned long long)v[i].y + 1ull) * a1[i]) * b;
      }
      if (lane < kSel) { if (sel) accx += ((unsigned long long)sel[(unsigned long long)row * kSel + lane] + 1ull) * b; }
      else if (lane == kSel) { if (p) accx += ((unsigned long long)p[row] + 1ull) * b; }
      else if (lane == kSel + 1) { if (bits) accx += ((unsigned long long)bits[row] + 1ull) * b; }
    }
#pragma unroll
    for (int i = 0; i < kIter; ++i) {   // a column group is eight neighbouring lanes of one load
      unsigned long long s = acc[i];
      s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4);
      const int g = i * 8 + (lane >> 3);
      if ((lane & 7) == 0 && g < 130) red[wave][g] = s;
    }
    if (lane < kSel) red[wave][131 + lane] = accx;
    else if (lane == kSel) red[wave][130] = accx;
    else if (lane == kSel + 1) red[wave][178] = accx;
    __syncthreads();
    if (threadIdx.x < kWords) {
      unsigned long long s = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) s += red[w][threadIdx.x];
      if (s) atomicAdd(&part[(blk - blk0) * kWords + threadIdx.x], s);
    }
    __syncthreads();
    r = run_end;
  }
}
}  // namespace

struct cmx_journal {
  int device = 0;
  int k = CMX_JOURNAL_MAX_LOG2;
  unsigned long long* d_part = nullptr;   // cmx_journal_run's own partial records (the pipeline brings a pair per slot)
  uint64_t* h_part = nullptr;             // pinned
  size_t cap_blocks = 0;
  bool started = false;
  uint64_t base_blk = 0;                  // the block of the first bit ever folded
  uint64_t next_bit = 0;                  // one past the last bit folded
  std::vector<std::array<uint64_t, CMX_JOURNAL_RECORD>> blocks;
};

extern "C" {

cmx_journal_t* cmx_journal_create(int device, int log2_block_bits) {
  if (log2_block_bits < CMX_JOURNAL_MIN_LOG2 || log2_block_bits > CMX_JOURNAL_MAX_LOG2) { cmx_set_err("cmx_journal_create: log2_block_bits must be 6..19"); return nullptr; }
  if (cmx_device_count() <= 0) { cmx_set_err("cmx_journal_create: no HIP device visible (a gfx950 GPU is required)"); return nullptr; }
  if (device < 0 || device >= cmx_device_count() || hipSetDevice(device) != hipSuccess) { cmx_set_err("cmx_journal_create: bad device index"); return nullptr; }
  cmx_journal_t* j = new cmx_journal();
  j->device = device; j->k = log2_block_bits;
  return j;
}

void cmx_journal_destroy(cmx_journal_t* j) {
  if (!j) return;
  (void)hipSetDevice(j->device);
  (void)hipDeviceSynchronize();
  if (j->d_part) (void)hipFree(j->d_part);
  if (j->h_part) (void)hipHostFree(j->h_part);
  delete j;
}

int cmx_journal_log2(cmx_journal_t* j) { return j ? j->k : 0; }

int cmx_journal_enqueue(cmx_journal_t* j, const float* d_rows, size_t ld, const uint32_t* d_sel, const uint8_t* d_bits, const float* d_p, size_t nbits,
                        uint64_t stream_bit0, unsigned long long* d_part, uint64_t* h_part, size_t cap_blocks, hipStream_t stream) {
  if (!j || !d_part || !h_part) { cmx_set_err("cmx_journal_run: bad argument"); return 1; }
  if (nbits == 0) return 0;
  if (nbits > 0x7fffffff) { cmx_set_err("cmx_journal_run: chunk too large"); return 1; }
  if (d_rows && (ld < (size_t)kCols || (ld & 1) || ((uintptr_t)d_rows & 7))) {
    cmx_set_err("cmx_journal_run: rows are read with 8-byte loads: ld must be even and >= 2078, d_rows 8-byte aligned");
    return 1;
  }
  if (d_p && ((uintptr_t)d_p & 3)) { cmx_set_err("cmx_journal_run: d_p is not 4-byte aligned"); return 1; }
  if (d_sel && ((uintptr_t)d_sel & 3)) { cmx_set_err("cmx_journal_run: d_sel is not 4-byte aligned"); return 1; }
  const size_t span = cmx_journal_span(j->k, nbits, stream_bit0);
  if (span > cap_blocks) { cmx_set_err("cmx_journal_run: the chunk touches more blocks than the partial-record buffer holds"); return 1; }
  if (hipSetDevice(j->device) != hipSuccess) { cmx_set_err("hipSetDevice failed"); return 1; }
  const size_t bytes = span * kWords * sizeof(unsigned long long);
  if (hipMemsetAsync(d_part, 0, bytes, stream) != hipSuccess) { cmx_set_err("cmx_journal_run: hipMemsetAsync failed"); return 1; }
  const unsigned grid = (unsigned)((nbits + kWgRows - 1) / kWgRows);
  hipLaunchKernelGGL(cmx_journal_kernel, dim3(grid), dim3(64 * kWaves), 0, stream, (const uint2*)d_rows, (unsigned long long)(ld / 2), d_sel, d_bits,
                     (const uint32_t*)d_p, (unsigned)nbits, (unsigned long long)stream_bit0, j->k, d_part);
  if (hipGetLastError() != hipSuccess) { cmx_set_err("cmx_journal_run: kernel launch failed"); return 1; }
  if (hipMemcpyAsync(h_part, d_part, bytes, hipMemcpyDeviceToHost, stream) != hipSuccess) { cmx_set_err("cmx_journal_run: hipMemcpyAsync failed"); return 1; }
  return 0;
}

int cmx_journal_fold(cmx_journal_t* j, const uint64_t* h_part, size_t nbits, uint64_t stream_bit0) {
  if (!j || !h_part) { cmx_set_err("cmx_journal_fold: bad argument"); return 1; }
  if (nbits == 0) return 0;
  if (j->started && stream_bit0 != j->next_bit) {
    cmx_set_err("cmx_journal_run: stream bit " + std::to_string(stream_bit0) + " does not continue the journal, which ends at bit " + std::to_string(j->next_bit));
    return 1;
  }
  if (!j->started) { j->started = true; j->base_blk = stream_bit0 >> j->k; }
  const uint64_t end = stream_bit0 + nbits;
  const size_t span = cmx_journal_span(j->k, nbits, stream_bit0);
  for (size_t i = 0; i < span; ++i) {
    const uint64_t blk = (stream_bit0 >> j->k) + i;
    const size_t at = (size_t)(blk - j->base_blk);
    if (at >= j->blocks.size()) { j->blocks.emplace_back(); j->blocks.back().fill(0); }
    std::array<uint64_t, CMX_JOURNAL_RECORD>& rec = j->blocks[at];
    const uint64_t blk_end = (blk + 1) << j->k;
    rec[0] = (blk_end < end ? blk_end : end) >> 3;
    for (int w = 0; w < kWords; ++w) rec[1 + w] += h_part[i * kWords + w];
  }
  j->next_bit = end;
  return 0;
}

int cmx_journal_run(cmx_journal_t* j, const float* d_rows, size_t ld, const uint32_t* d_sel, const uint8_t* d_bits, const float* d_p, size_t nbits,
                    uint64_t stream_bit0, void* stream) {
  if (!j) { cmx_set_err("cmx_journal_run: null handle"); return 1; }
  if (nbits == 0) return 0;
  if (j->started && stream_bit0 != j->next_bit) {
    cmx_set_err("cmx_journal_run: stream bit " + std::to_string(stream_bit0) + " does not continue the journal, which ends at bit " + std::to_string(j->next_bit));
    return 1;
  }
  if (hipSetDevice(j->device) != hipSuccess) { cmx_set_err("hipSetDevice failed"); return 1; }
  const size_t span = cmx_journal_span(j->k, nbits, stream_bit0);
  if (span > j->cap_blocks) {   // the stand-alone handle grows its pair of buffers to the largest chunk it has seen
    if (j->d_part) (void)hipFree(j->d_part);
    if (j->h_part) (void)hipHostFree(j->h_part);
    j->d_part = nullptr; j->h_part = nullptr; j->cap_blocks = 0;
    const size_t bytes = span * kWords * sizeof(unsigned long long);
    if (hipMalloc((void**)&j->d_part, bytes) != hipSuccess || hipHostMalloc((void**)&j->h_part, bytes, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      cmx_set_err("cmx_journal_run: allocating the partial records failed");
      return 1;
    }
    j->cap_blocks = span;
  }
  hipStream_t st = (hipStream_t)stream;
  if (cmx_journal_enqueue(j, d_rows, ld, d_sel, d_bits, d_p, nbits, stream_bit0, j->d_part, j->h_part, j->cap_blocks, st)) return 1;
  if (hipStreamSynchronize(st) != hipSuccess) { cmx_set_err("cmx_journal_run: device error"); return 1; }
  return cmx_journal_fold(j, j->h_part, nbits, stream_bit0);
}

int cmx_journal_blocks(cmx_journal_t* j, uint64_t* nblocks) {
  if (!j || !nblocks) { cmx_set_err("cmx_journal_blocks: bad argument"); return 1; }
  *nblocks = j->blocks.size();
  return 0;
}

int cmx_journal_read(cmx_journal_t* j, uint64_t first, uint64_t n, uint64_t* out) {
  if (!j || (n && !out)) { cmx_set_err("cmx_journal_read: bad argument"); return 1; }
  if (first > j->blocks.size() || n > j->blocks.size() - first) { cmx_set_err("cmx_journal_read: the journal holds " + std::to_string(j->blocks.size()) + " block(s)"); return 1; }
  for (uint64_t i = 0; i < n; ++i) memcpy(out + i * CMX_JOURNAL_RECORD, j->blocks[first + i].data(), CMX_JOURNAL_RECORD * sizeof(uint64_t));
  return 0;
}

}  // extern "C"
