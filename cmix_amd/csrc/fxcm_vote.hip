// fxcm_vote.hip -- the redundant fxcm-stage vote (C ABI: cmx_fxcmvote_*, cmx_fxcm_state_diff, cmx_fxcm_debug_state_xor, cmx_fxcm_debug_layout in
// include/cmix_amd.h).
//
// The fxcm stage (fxcm_stage.hip) writes 431 of the 2078 layer-0 columns (3..433) from 4.4 GB of tables that learn online -- one wrong word stays for
// good -- and its roles kernel hands rows between role M's sixteen free-running wavefronts, role U and role X behind counters inside every launch.
// Verify mode and the other votes take its columns as given. The guard here is the one the mixing network, the context stage and the LSTM have: the
// unchanged cmx_fxcm_roles_kernel runs on two or three FxDev (cmx_fxcm_run / cmx_fxcm_run_shared) and two new kernels compare what they wrote.
//
//   cmx_fxcmvote_kernel         every chunk: the 431 exported values of every bit of n = 2 or 3 instances, word for word; one wavefront per row
//                               (a row's words are consecutive: seven coalesced 4-byte loads per lane and instance, all issued before the first
//                               compare; no LDS). Instance 0 is read in place from the slot's layer-0 rows, whose base (layer0 + 3 + 2078 t) is only
//                               4-byte aligned, differently from row to row: nothing wider than a 4-byte load is used.
//   cmx_fxcmvote_fold_kernel    behind it: folds the chunk's result into a sticky record and captures the first differing bit's row
//   cmx_fxcm_state_diff_kernel  after an event (and in tests): every word of two handles' tables in HBM
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
#include "fxcm_rec.h"
#include "fxcm_state.h"

void cmx_set_err(const std::string& s);  // cmx_api.hip

namespace {
constexpr unsigned long long kNone = ~0ull;
constexpr int kCols = CMX_FXCMVOTE_COLS;
constexpr int kPasses = (kCols + 63) / 64;   // 7: six full passes of the wave and one of 47 lanes
static_assert(kCols == FX_OUTPUTS, "the vote's row is FXCM::Predict()'s 431 values of one bit");
static_assert(CMX_FXCM_STATE_REGIONS == FX_STATE_REGIONS && CMX_FXCM_STATE_ARRAYS == FX_STATE_ARRAYS, "region and array counts of the header and of fxcm_state.h");

// device block of a vote handle
struct FxVoteDev {
  unsigned long long rec[8];     // the sticky record (cmx_fxcmvote_report)
  unsigned long long last[4];    // the chunk folded last (cmx_fxcmvote_last), right behind the record: one copy fetches both
  unsigned long long key;        // this chunk: min over non-agreeing elements of (e << 2 | odd instance, 3 = no majority); ~0 = none
  unsigned long long cnt;        // this chunk: non-agreeing elements
  unsigned long long odd;        // this chunk: bit i = instance i was the odd one of some element, bit 3 = some element had no majority
  unsigned long long pad;
  uint32_t words[3 * kCols];     // capture of the first event's bit: instance i, column c at [i * 431 + c]
  uint32_t bit, byte;            // the bit coded at that row and the byte it belongs to
};
struct FxVoteArgs {
  const uint32_t* rows[3];       // row t of instance i at rows[i] + t * pstride[i]
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

// One wavefront per row (bit), grid-stride over the rows. Every lane keeps its own minimum key, count and odd mask; one reduction and one atomic per
// wave at the end, and only in waves that saw a difference. Registers only.
template <int N>
__global__ void __launch_bounds__(256) cmx_fxcmvote_kernel(FxVoteArgs a, unsigned long long nrows, FxVoteDev* d) {
  const unsigned lane = threadIdx.x & 63;
  const unsigned long long waves = (unsigned long long)gridDim.x * (blockDim.x >> 6);
  unsigned long long key = kNone, cnt = 0;
  unsigned odd = 0;
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
      const unsigned r = vote_one<N>(w0[p], w1[p], w2[p]);
      if (r) {
        const unsigned long long k = ((t * kCols + (lane + 64u * p)) << 2) | (r - 1);
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

// one wave, behind the vote kernel on the same stream: the chunk's key and count into the sticky record; the first event's row is captured.
// The chunk's OWN result goes into last[] exactly as cmx_vote_fold_kernel (mixnet_vote.hip) leaves it.
__global__ void cmx_fxcmvote_fold_kernel(FxVoteArgs a, unsigned long long nrows, unsigned long long bit0, int n, const uint8_t* bytes, FxVoteDev* d) {
  const unsigned long long key = d->key, cnt = d->cnt, odd = d->odd;
  const bool first = cnt != 0 && d->rec[3] == 0;   // (read by every lane before lane 0 writes: one wave, the barrier below orders it)
  __syncthreads();
  const unsigned long long e = key >> 2, t = e / kCols, c = e - t * kCols;
  if (first && t < nrows)
    for (int i = threadIdx.x; i < n * kCols; i += blockDim.x) {
      const int inst = i / kCols;
      d->words[i] = a.rows[inst][t * a.pstride[inst] + (unsigned)(i - inst * kCols)];
    }
  if (threadIdx.x == 0) {
    d->rec[0] += 1; d->rec[1] += nrows; d->rec[2] = (unsigned long long)n;
    if (cnt) d->rec[3] += 1;
    if (first) {
      d->rec[4] = bit0 + t; d->rec[5] = c; d->rec[6] = (key & 3) == 3 ? kNone : (key & 3); d->rec[7] = cnt;
      const uint32_t by = bytes && t < nrows ? bytes[t >> 3] : 0u;
      d->byte = by; d->bit = (by >> (7 - (unsigned)(t & 7))) & 1u;
    }
    d->last[0] = cnt; d->last[1] = cnt ? bit0 + t : 0; d->last[2] = cnt ? c : 0;
    d->last[3] = !cnt ? 0 : odd == 1 ? 0 : odd == 2 ? 1 : odd == 4 ? 2 : kNone;
    d->key = kNone; d->cnt = 0; d->odd = 0;   // the next chunk starts clean
  }
}

// ---- state diff: the words of two arrays; one launch per array ----
struct FxDiffDev { unsigned long long cnt, first; };
__global__ void __launch_bounds__(256) cmx_fxcm_state_diff_kernel(const uint32_t* x, const uint32_t* y, unsigned long long n, FxDiffDev* d) {
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

struct cmx_fxcmvote {
  int device = 0, n = 0;
  FxVoteDev* d = nullptr;
};

extern "C" {

cmx_fxcmvote_t* cmx_fxcmvote_create(int device, int n) {
  if (n != 2 && n != 3) { cmx_set_err("cmx_fxcmvote_create: n must be 2 or 3 instances"); return nullptr; }
  if (cmx_device_count() <= 0) { cmx_set_err("cmx_fxcmvote_create: no HIP device visible (a gfx950 GPU is required)"); return nullptr; }
  if (device < 0 || device >= cmx_device_count() || hipSetDevice(device) != hipSuccess) { cmx_set_err("cmx_fxcmvote_create: bad device index"); return nullptr; }
  cmx_fxcmvote_t* v = new cmx_fxcmvote();
  v->device = device; v->n = n;
  FxVoteDev init;
  memset(&init, 0, sizeof init);
  init.key = kNone;
  if (hipMalloc((void**)&v->d, sizeof(FxVoteDev)) != hipSuccess || hipMemcpy(v->d, &init, sizeof init, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    if (v->d) (void)hipFree(v->d);
    delete v;
    cmx_set_err("cmx_fxcmvote_create: hipMalloc failed");
    return nullptr;
  }
  return v;
}

void cmx_fxcmvote_destroy(cmx_fxcmvote_t* v) {
  if (!v) return;
  (void)hipSetDevice(v->device);
  (void)hipDeviceSynchronize();
  if (v->d) (void)hipFree(v->d);
  delete v;
}

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
  const unsigned grid = (unsigned)((nrows + 3) / 4 < 512 ? (nrows + 3) / 4 : 512);   // four rows (waves) per workgroup; 2048 waves stride over the rest
  if (v->n == 3) hipLaunchKernelGGL(cmx_fxcmvote_kernel<3>, dim3(grid), dim3(256), 0, st, a, nrows, v->d);
  else hipLaunchKernelGGL(cmx_fxcmvote_kernel<2>, dim3(grid), dim3(256), 0, st, a, nrows, v->d);
  hipLaunchKernelGGL(cmx_fxcmvote_fold_kernel, dim3(1), dim3(64), 0, st, a, nrows, (unsigned long long)stream_bit0, v->n, d_bytes, v->d);
  if (hipGetLastError() != hipSuccess) { cmx_set_err("cmx_fxcmvote_run: kernel launch failed"); return 1; }
  return 0;
}

const unsigned long long* cmx_fxcmvote_record(cmx_fxcmvote_t* v) { return v && v->d ? v->d->rec : nullptr; }

int cmx_fxcmvote_report(cmx_fxcmvote_t* v, uint64_t out[8]) {
  if (!v || !out) { cmx_set_err("cmx_fxcmvote_report: bad argument"); return 1; }
  unsigned long long r[8];
  if (hipSetDevice(v->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(r, v->d->rec, sizeof r, hipMemcpyDeviceToHost) != hipSuccess) {
    cmx_set_err("cmx_fxcmvote_report: device error"); return 1;
  }
  for (int i = 0; i < 8; ++i) out[i] = r[i];
  return 0;
}

int cmx_fxcmvote_last(cmx_fxcmvote_t* v, uint64_t out[4]) {
  if (!v || !out) { cmx_set_err("cmx_fxcmvote_last: bad argument"); return 1; }
  unsigned long long r[4];
  if (hipSetDevice(v->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(r, v->d->last, sizeof r, hipMemcpyDeviceToHost) != hipSuccess) {
    cmx_set_err("cmx_fxcmvote_last: device error"); return 1;
  }
  for (int i = 0; i < 4; ++i) out[i] = r[i];
  return 0;
}

int cmx_fxcmvote_values(cmx_fxcmvote_t* v, uint32_t words[3 * CMX_FXCMVOTE_COLS], uint32_t* bit, uint32_t* byte) {
  if (!v || !words) { cmx_set_err("cmx_fxcmvote_values: bad argument"); return 1; }
  std::vector<FxVoteDev> h(1);
  if (hipSetDevice(v->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(h.data(), v->d, sizeof(FxVoteDev), hipMemcpyDeviceToHost) != hipSuccess) {
    cmx_set_err("cmx_fxcmvote_values: device error"); return 1;
  }
  memcpy(words, h[0].words, sizeof h[0].words);
  if (bit) *bit = h[0].bit;
  if (byte) *byte = h[0].byte;
  return 0;
}

int cmx_fxcm_state_diff(cmx_fxcm_t* a, cmx_fxcm_t* b, uint64_t out[CMX_FXCM_STATE_OUT]) {
  if (!a || !b || !out) { cmx_set_err("cmx_fxcm_state_diff: bad argument"); return 1; }
  if (a == b) { cmx_set_err("cmx_fxcm_state_diff: a and b are the same handle"); return 1; }
  std::vector<FxRegion> ra(FX_STATE_ARRAYS), rb(FX_STATE_ARRAYS);
  int na = 0, nb = 0, deva = 0, devb = 0;
  uint64_t ca = 0, cb = 0;
  if (cmx_fxcm_state_view(a, ra.data(), &na, &deva, &ca) || cmx_fxcm_state_view(b, rb.data(), &nb, &devb, &cb)) return 1;
  if (deva != devb) { cmx_set_err("cmx_fxcm_state_diff: the two handles live on different devices"); return 1; }
  if (ca != cb) { cmx_set_err("cmx_fxcm_state_diff: the host-side counter bytes_done differs: " + std::to_string(ca) + " and " + std::to_string(cb)); return 1; }
  if (hipSetDevice(deva) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { cmx_set_err("cmx_fxcm_state_diff: device error"); return 1; }
  std::vector<FxDiffDev> h((size_t)na, FxDiffDev{0, kNone});
  FxDiffDev* d = nullptr;
  bool ok = na == nb && hipMalloc((void**)&d, h.size() * sizeof(FxDiffDev)) == hipSuccess && hipMemcpy(d, h.data(), h.size() * sizeof(FxDiffDev), hipMemcpyHostToDevice) == hipSuccess;
  for (int r = 0; ok && r < na; ++r) {
    if (ra[r].region != rb[r].region || ra[r].words != rb[r].words) { ok = false; break; }
    const unsigned long long items = ra[r].words / 4 + 4;
    const unsigned grid = (unsigned)(items / 256 + 1 < 2048 ? items / 256 + 1 : 2048);
    hipLaunchKernelGGL(cmx_fxcm_state_diff_kernel, dim3(grid), dim3(256), 0, 0, ra[r].p, rb[r].p, ra[r].words, d + r);
    ok = hipGetLastError() == hipSuccess;
  }
  ok = ok && hipDeviceSynchronize() == hipSuccess && hipMemcpy(h.data(), d, h.size() * sizeof(FxDiffDev), hipMemcpyDeviceToHost) == hipSuccess;
  for (int i = 0; i < CMX_FXCM_STATE_OUT; ++i) out[i] = 0;
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

int cmx_fxcm_debug_state_xor(cmx_fxcm_t* h, int region, uint64_t index, uint32_t xor_mask) {
  if (!h) { cmx_set_err("cmx_fxcm_debug_state_xor: null handle"); return 1; }
  if (!xor_mask) { cmx_set_err("cmx_fxcm_debug_state_xor: a zero mask changes nothing"); return 1; }
  if (region < 0 || region >= FX_STATE_REGIONS) { cmx_set_err("cmx_fxcm_debug_state_xor: no such region (0..11)"); return 1; }
  if (!kOpen[region]) {
    cmx_set_err("cmx_fxcm_debug_state_xor: region " + std::to_string(region) + " (" + kRegionName[region] +
                ") holds words the kernels address memory or bound loops with: refused (the hook changes values only)");
    return 1;
  }
  std::vector<FxRegion> rg(FX_STATE_ARRAYS);
  int n = 0, dev = 0;
  if (cmx_fxcm_state_view(h, rg.data(), &n, &dev, nullptr)) return 1;
  uint32_t* p = nullptr;
  unsigned long long off = 0;
  for (int r = 0; r < n && !p; ++r) {
    if (r && rg[r].region != rg[r - 1].region) off = 0;
    if (rg[r].region == region && index >= off && index - off < rg[r].words) p = rg[r].p + (index - off);
    off += rg[r].words;
  }
  if (!p) { cmx_set_err("cmx_fxcm_debug_state_xor: no such word (region, index out of range)"); return 1; }
  uint32_t x = 0;
  if (hipSetDevice(dev) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(&x, p, 4, hipMemcpyDeviceToHost) != hipSuccess) {
    cmx_set_err("cmx_fxcm_debug_state_xor: device error"); return 1;
  }
  x ^= xor_mask;
  if (hipMemcpy(p, &x, 4, hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { cmx_set_err("cmx_fxcm_debug_state_xor: device error"); return 1; }
  return 0;
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
  std::vector<FxRegion> rg(FX_STATE_ARRAYS);
  int n = 0, dev = 0;
  if (cmx_fxcm_state_view(h, rg.data(), &n, &dev, nullptr)) return 1;
  if (hipSetDevice(dev) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { cmx_set_err("cmx_fxcm_debug_state_read: device error"); return 1; }
  unsigned long long off = 0, done = 0;
  for (int r = 0; r < n && done < count; ++r) {   // (the words may run from one array of the region into the next)
    if (r && rg[r].region != rg[r - 1].region) off = 0;
    if (rg[r].region == region && index + done >= off && index + done - off < rg[r].words) {
      const unsigned long long at = index + done - off, m = count - done < rg[r].words - at ? count - done : rg[r].words - at;
      if (hipMemcpy(out + done, rg[r].p + at, m * 4, hipMemcpyDeviceToHost) != hipSuccess) { cmx_set_err("cmx_fxcm_debug_state_read: device error"); return 1; }
      done += m;
    }
    off += rg[r].words;
  }
  if (done != count) { cmx_set_err("cmx_fxcm_debug_state_read: no such words (region, index out of range)"); return 1; }
  return 0;
}

int cmx_fxcm_debug_layout(cmx_fxcm_t* h, uint64_t out[3 * CMX_FXCM_STATE_ARRAYS]) {
  if (!h || !out) { cmx_set_err("cmx_fxcm_debug_layout: bad argument"); return -1; }
  std::vector<FxRegion> rg(FX_STATE_ARRAYS);
  int n = 0, dev = 0;
  if (cmx_fxcm_state_view(h, rg.data(), &n, &dev, nullptr)) return -1;
  unsigned long long off = 0;
  for (int r = 0; r < n; ++r) {
    if (r && rg[r].region != rg[r - 1].region) off = 0;
    out[3 * r] = (uint64_t)rg[r].region; out[3 * r + 1] = off; out[3 * r + 2] = rg[r].words;
    off += rg[r].words;
  }
  std::vector<uint32_t> w;
  if (cmx_fxcm_dev_words(h, w)) return -1;
  out[3 * n] = FX_REGION_DEV; out[3 * n + 1] = 0; out[3 * n + 2] = w.size();
  return n + 1;
}

}  // extern "C"
