// state_digest.hip -- the state digest's kernel and its host form (cmx_state_digest.h has the formula; C ABI: cmx_state_digest_host,
// cmx_state_digest_arrays in include/cmix_amd.h).
//
//   cmx_state_digest_kernel   ONE launch for a whole list of arrays (fxcm has 140, paq8 461, most of them tiny): a device table holds (pointer, words, first
//                             workgroup, workgroups) per array and a second one the array of every workgroup. Workgroups are dealt to the arrays by
//                             size, at least one to every array that has a word. Inside an array: cmx_state_walk's pattern (cmx_vote_core.h) -- 16-byte
//                             loads, then the single words left over -- in a grid-stride loop over the array's own workgroups, one 64-bit
//                             accumulator per lane, one __shfl_xor reduction per wave and one 64-bit atomicAdd per wave into the array's word.
//                             Registers only: no LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/cmix_amd.h"
#include "cmx_state_digest.h"

namespace {
constexpr unsigned kThreads = 256;
constexpr unsigned kGrid = 2048;   // workgroups dealt among a list's arrays: eight per compute unit

struct DigestJob {
  const uint32_t* p; unsigned long long words;
  unsigned wg0, nwg;   // the array's workgroups: [wg0, wg0 + nwg)
};

__global__ void __launch_bounds__(kThreads) cmx_state_digest_kernel(const DigestJob* jobs, const unsigned* wg_job, unsigned long long* out) {
  const unsigned j = wg_job[blockIdx.x];
  const DigestJob job = jobs[j];
  const unsigned long long n = job.words, nq = n / 4, items = nq + (n - 4 * nq);
  const unsigned long long stride = (unsigned long long)job.nwg * kThreads;
  unsigned long long acc = 0;
  for (unsigned long long i = (unsigned long long)(blockIdx.x - job.wg0) * kThreads + threadIdx.x; i < items; i += stride) {
    if (i < nq) {
      const uint4 u = reinterpret_cast<const uint4*>(job.p)[i];
      acc += cmx_state_digest_term(4 * i, u.x) + cmx_state_digest_term(4 * i + 1, u.y) + cmx_state_digest_term(4 * i + 2, u.z) + cmx_state_digest_term(4 * i + 3, u.w);
    } else {
      const unsigned long long k = 4 * nq + (i - nq);
      acc += cmx_state_digest_term(k, job.p[k]);
    }
  }
  for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0 && acc) atomicAdd(&out[j], acc);
}
}  // namespace

int cmx_state_digest_spans(const char* who_, int device, const CmxDigestSpan* a, int n, uint64_t* out) {
  const std::string who(who_);
  if (n < 0 || (n && (!a || !out))) { cmx_set_err(who + ": bad argument"); return 1; }
  unsigned long long total = 0;
  for (int r = 0; r < n; ++r) {
    if (a[r].words >> 32) { cmx_set_err(who + ": state array " + std::to_string(r) + " has 2^32 words or more: its word numbers do not fit the digest's key"); return 1; }
    if (a[r].words && (!a[r].p || ((uintptr_t)a[r].p & 15))) { cmx_set_err(who + ": state array " + std::to_string(r) + " is null or not 16-byte aligned"); return 1; }
    total += a[r].words;
  }
  for (int r = 0; r < n; ++r) out[r] = 0;
  if (hipSetDevice(device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { cmx_set_err(who + ": device error"); return 1; }
  if (!total) return 0;
  // the deal: an array's share of kGrid by its words, at least one workgroup, never more than it has items for
  std::vector<DigestJob> jobs((size_t)n);
  std::vector<unsigned> wg_job;
  for (int r = 0; r < n; ++r) {
    const unsigned long long w = a[r].words, items = w / 4 + (w & 3), most = (items + kThreads - 1) / kThreads;
    unsigned long long g = (unsigned long long)((long double)w / (long double)total * kGrid);
    g = g < 1 ? 1 : g;
    g = g > most ? most : g;   // (most == 0 only where w == 0: no workgroup, the digest stays 0)
    jobs[r] = {a[r].p, w, (unsigned)wg_job.size(), (unsigned)g};
    wg_job.insert(wg_job.end(), (size_t)g, (unsigned)r);
  }
  const size_t jb = (jobs.size() * sizeof(DigestJob) + 15) / 16 * 16, mb = (wg_job.size() * sizeof(unsigned) + 15) / 16 * 16, ob = (size_t)n * 8;
  char* d = nullptr;
  bool ok = hipMalloc((void**)&d, jb + mb + ob) == hipSuccess && hipMemcpy(d, jobs.data(), jobs.size() * sizeof(DigestJob), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(d + jb, wg_job.data(), wg_job.size() * sizeof(unsigned), hipMemcpyHostToDevice) == hipSuccess && hipMemset(d + jb + mb, 0, ob) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(cmx_state_digest_kernel, dim3((unsigned)wg_job.size()), dim3(kThreads), 0, 0, (const DigestJob*)d, (const unsigned*)(d + jb), (unsigned long long*)(d + jb + mb));
    ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, d + jb + mb, ob, hipMemcpyDeviceToHost) == hipSuccess;
  }
  if (d) (void)hipFree(d);
  if (!ok) { (void)hipGetLastError(); cmx_set_err(who + ": device error"); return 1; }
  return 0;
}

extern "C" {

uint64_t cmx_state_digest_host(const uint32_t* words, uint64_t n) {
  uint64_t d = 0;
  for (uint64_t i = 0; i < n; ++i) d += cmx_state_digest_term(i, words[i]);
  return d;
}

int cmx_state_digest_arrays(int device, const void* const* d_arrays, const uint64_t* words, int n, uint64_t* out) {
  if (n < 0 || (n && (!d_arrays || !words || !out))) { cmx_set_err("cmx_state_digest_arrays: bad argument"); return 1; }
  if (cmx_device_count() <= 0) { cmx_set_err("cmx_state_digest_arrays: no HIP device visible (a gfx950 GPU is required)"); return 1; }
  std::vector<CmxDigestSpan> s((size_t)n);
  for (int r = 0; r < n; ++r) s[r] = {(const uint32_t*)d_arrays[r], words[r]};
  return cmx_state_digest_spans("cmx_state_digest_arrays", device, s.data(), n, out);
}

}  // extern "C"
