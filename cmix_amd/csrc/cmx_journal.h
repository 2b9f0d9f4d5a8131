// cmx_journal.h -- what journal.hip, journal_host.cpp and the pipeline share of the stream journal (include/cmix_amd.h, "Stream journal").
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <array>
#include <string>
#include <vector>

#include "../../include/cmix_amd.h"

#define CMX_JOURNAL_MIN_LOG2 6
#define CMX_JOURNAL_MAX_LOG2 19   // B's period: the reference trace's 64 KB block

// A[c] and B[i] of the digest are splitmix64 values with the lowest bit set (ref_long_trace)
static __host__ __device__ inline unsigned long long cmx_journal_splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
static __host__ __device__ inline unsigned long long cmx_journal_B(unsigned long long t) {
  return cmx_journal_splitmix64(0x1000000ull + (t & ((1ull << CMX_JOURNAL_MAX_LOG2) - 1))) | 1ull;
}
// blocks of 2^k bits that the nbits bits from stream bit bit0 on touch
static inline size_t cmx_journal_span(int k, size_t nbits, uint64_t bit0) {
  return nbits ? (size_t)(((bit0 + nbits - 1) >> k) - (bit0 >> k)) + 1 : 0;
}

// journal.hip: the two halves of cmx_journal_run, for a caller that keeps chunks in flight (the pipeline). _enqueue clears d_part (cap_blocks records of
// CMX_JOURNAL_WORDS words), runs the kernel behind `stream` and copies the chunk's partial records to the pinned h_part behind it; nothing is waited for.
// _fold adds those records to the handle's blocks once the copy has landed; chunks are folded in stream order.
extern "C" int cmx_journal_enqueue(cmx_journal_t* j, const float* d_rows, size_t ld, const uint32_t* d_sel, const uint8_t* d_bits, const float* d_p, size_t nbits,
                                   uint64_t stream_bit0, unsigned long long* d_part, uint64_t* h_part, size_t cap_blocks, hipStream_t stream);
extern "C" int cmx_journal_fold(cmx_journal_t* j, const uint64_t* h_part, size_t nbits, uint64_t stream_bit0);
extern "C" int cmx_journal_log2(cmx_journal_t* j);

// journal_host.cpp: what a host thread that holds p(t) and bit t one at a time folds (a decoder: cmx_predict / cmx_perceive in late-bit mode), the
// journal files, and a compressor's journal to check a decode against. A record here is {end byte position, p word, bits word}.
struct CmxHostJournal {
  int k = CMX_JOURNAL_MAX_LOG2;
  uint64_t t = 0;                                   // bits folded: stream bit 0 is the first coded bit
  std::vector<std::array<uint64_t, 3>> blocks;      // a partial last one included
  bool check = false;                               // compare every block, as it completes, with want[]
  std::vector<std::array<uint64_t, 3>> want;
};
// folds bit t; at the end of a block of a checking journal compares it: 1 and *err on the first difference (the block, its byte range, which word)
int cmx_hostjournal_add(CmxHostJournal* j, float p, int bit, std::string* err);
// the (partial) block in progress against the compressor's, at the end of a decode
int cmx_hostjournal_check_tail(CmxHostJournal* j, std::string* err);
// `path` ("<end byte> <131 hex words>") and `path.inputs` ("<end byte> <48 hex words>") of a compressor's journal: the p and bits words per block and the
// block size its positions imply
int cmx_journal_load_check(const char* path, std::vector<std::array<uint64_t, 3>>* want, int* log2_block_bits, std::string* err);
// appends n records of CMX_JOURNAL_RECORD words to `path` and `path.inputs` (created, or emptied first, where truncate is set) and flushes
int cmx_journal_append_files(const char* path, const uint64_t* records, size_t n, bool truncate, std::string* err);
