// cmx_state_digest.h -- the state digest (state_digest.hip; C ABI: cmx_*_state_digest in include/cmix_amd.h, "State digest"): one 64-bit word per
// state array of a device stage, small enough to be written down as a run goes, so that two runs -- on different machines and days -- can be compared in
// state as the stream journal compares them in columns.
//
// THE DIGEST of an array of n 32-bit words w[0..n), n < 2^32:
//     D = sum over i of splitmix64((uint64(i) << 32) | w[i])   (mod 2^64),   splitmix64 = cmx_journal_splitmix64 (cmx_journal.h)
// The sum does not depend on the order of its terms: the kernel is parallel and still deterministic. splitmix64 is a bijection: a change of one word
// w -> w' always changes D, by exactly splitmix64(i, w') - splitmix64(i, w). An array of 2^32 words or more is refused (its index would not fit the
// key); none exists today.
//
// COLUMNS of a stage: one per state array, in the order of the stage's state view (what its _debug_layout lists), then -- where the stage's
// _state_diff compares words on the host -- one last column over those words with the same function: mixnet's scalar words, fxcm's FxDev with its
// device pointers zeroed and bytes_done, the LSTM's three counters. paq8's last column covers the scalar words of its role structs (p8stage.hip).
//
// NOT COVERED: the host stages' state (PPMd's arena, paq8's front end, fxcm's parser), pretraining as it runs (the first record after it covers its
// result), and the decoder (its patient kernels are resident and a stream has no rest point).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "cmx_journal.h"

void cmx_set_err(const std::string& s);  // cmx_api.hip

static __host__ __device__ inline unsigned long long cmx_state_digest_term(unsigned long long i, uint32_t w) { return cmx_journal_splitmix64((i << 32) | w); }

struct CmxStateRegion { uint32_t* p; unsigned long long words; int region; };   // a stage's state array where it has no list type of its own (paq8)
struct CmxDigestSpan { const uint32_t* p; unsigned long long words; };   // one array in HBM (a hipMalloc of its own: 16-byte aligned)

// state_digest.hip. _spans: the digests of n arrays of `device` in one launch; synchronises the device before and after. 0, or 1 and cmx_last_error.
int cmx_state_digest_spans(const char* who, int device, const CmxDigestSpan* a, int n, uint64_t* out);
extern "C" uint64_t cmx_state_digest_host(const uint32_t* words, uint64_t n);

// What the stages' entry points share. a[n]: the stage's state arrays (anything with .p, .words and .region), host: the words its _state_diff compares
// on the host (NULL: the stage has none), host_region: the region number they are listed under. out == NULL: only the count. layout != 0: out
// receives (region, offset within the region, words) per column, nothing is digested. Returns the number of columns, or -1.
template <class A>
int cmx_state_digest_stage(const char* who, int device, const A* a, int n, const std::vector<uint32_t>* host, int host_region, uint64_t* out, size_t cap, int layout) {
  const int cols = n + (host ? 1 : 0);
  if (!out) return cols;
  if (cap < (size_t)cols * (layout ? 3 : 1)) { cmx_set_err(std::string(who) + ": out[] is too small (" + std::to_string(cols) + " columns)"); return -1; }
  if (layout) {
    for (int r = 0; r < n; ++r) {
      unsigned long long off = 0;
      for (int i = r - 1; i >= 0 && a[i].region == a[r].region; --i) off += a[i].words;
      out[3 * r] = (uint64_t)a[r].region; out[3 * r + 1] = off; out[3 * r + 2] = a[r].words;
    }
    if (host) { out[3 * n] = (uint64_t)host_region; out[3 * n + 1] = 0; out[3 * n + 2] = host->size(); }
    return cols;
  }
  std::vector<CmxDigestSpan> s((size_t)n);
  for (int r = 0; r < n; ++r) s[r] = {(const uint32_t*)a[r].p, a[r].words};
  if (cmx_state_digest_spans(who, device, s.data(), n, out)) return -1;
  if (host) out[n] = cmx_state_digest_host(host->data(), host->size());
  return cols;
}
