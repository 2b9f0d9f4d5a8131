// journal_host.cpp -- the stream journal's host side (include/cmix_amd.h, "Stream journal"): the p and bits words of a block from values the HOST
// holds, in plain C++. A decoder's thread has p(t) and bit t in hand one at a time and no rows to read back; these two words are what it can
// compare with a compressor's journal. HOST code, no device call: usable (and tested) without a GPU.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "cmx_journal.h"

namespace {
std::string block_text(const CmxHostJournal* j, size_t blk, uint64_t end_byte) {
  return "block " + std::to_string(blk) + " (bytes " + std::to_string((uint64_t)blk << (j->k - 3)) + ".." + std::to_string(end_byte ? end_byte - 1 : 0) + ")";
}
int compare_block(const CmxHostJournal* j, size_t blk, std::string* err) {
  const std::array<uint64_t, 3>& got = j->blocks[blk];
  if (blk >= j->want.size()) { if (err) *err = "journal check: " + block_text(j, blk, got[0]) + " lies beyond the compressor's journal, which holds " + std::to_string(j->want.size()) + " block(s)"; return 1; }
  const std::array<uint64_t, 3>& want = j->want[blk];
  const bool bad_p = got[1] != want[1], bad_b = got[2] != want[2];
  if (!bad_p && !bad_b && got[0] == want[0]) return 0;
  if (err) {
    char hex[96];
    if (bad_b) snprintf(hex, sizeof hex, "%016llx, the compressor's journal has %016llx", (unsigned long long)got[2], (unsigned long long)want[2]);
    else snprintf(hex, sizeof hex, "%016llx, the compressor's journal has %016llx", (unsigned long long)got[1], (unsigned long long)want[1]);
    *err = "journal check: " + block_text(j, blk, got[0]) + ": " +
           (bad_b ? (bad_p ? std::string("the bits word and the p word differ; bits ") : std::string("the bits word differs: ")) : bad_p ? std::string("the p word differs: ") :
            "ends at byte " + std::to_string(got[0]) + ", the compressor's at " + std::to_string(want[0]) + "; p ") + hex + " (the decoded bytes are wrong from this block on)";
  }
  return 1;
}
int read_lines(const std::string& path, int nwords, std::vector<std::vector<uint64_t>>* out, std::string* err) {
  FILE* f = fopen(path.c_str(), "r");
  if (!f) { if (err) *err = "journal check: cannot read " + path; return 1; }
  unsigned long long pos;
  while (fscanf(f, "%llu", &pos) == 1) {
    std::vector<uint64_t> row(1 + nwords);
    row[0] = pos;
    for (int i = 0; i < nwords; ++i) {
      unsigned long long v;
      if (fscanf(f, "%llx", &v) != 1) { fclose(f); if (err) *err = "journal check: " + path + ": a line with fewer than " + std::to_string(nwords) + " words"; return 1; }
      row[1 + i] = v;
    }
    out->push_back(row);
  }
  fclose(f);
  return 0;
}
}  // namespace

int cmx_hostjournal_add(CmxHostJournal* j, float p, int bit, std::string* err) {
  const size_t blk = (size_t)(j->t >> j->k);
  if (blk >= j->blocks.size()) j->blocks.push_back({0, 0, 0});
  const uint64_t b = cmx_journal_B(j->t);
  uint32_t u;
  memcpy(&u, &p, 4);
  std::array<uint64_t, 3>& rec = j->blocks[blk];
  rec[1] += ((uint64_t)u + 1ull) * b;
  rec[2] += ((uint64_t)(bit ? 1 : 0) + 1ull) * b;
  j->t++;
  rec[0] = j->t >> 3;
  if (j->check && (j->t & ((1ull << j->k) - 1)) == 0) return compare_block(j, blk, err);
  return 0;
}

int cmx_hostjournal_check_tail(CmxHostJournal* j, std::string* err) {
  if (!j->check) return 0;
  if (j->t & ((1ull << j->k) - 1)) { if (compare_block(j, j->blocks.size() - 1, err)) return 1; }
  if (j->blocks.size() != j->want.size()) {
    if (err) *err = "journal check: the decode ended after " + std::to_string(j->blocks.size()) + " block(s), the compressor's journal holds " + std::to_string(j->want.size());
    return 1;
  }
  return 0;
}

int cmx_journal_load_check(const char* path, std::vector<std::array<uint64_t, 3>>* want, int* log2_block_bits, std::string* err) {
  std::vector<std::vector<uint64_t>> a, b;
  if (read_lines(path, 131, &a, err) || read_lines(std::string(path) + ".inputs", 48, &b, err)) return 1;
  if (a.empty() || a.size() != b.size()) { if (err) *err = std::string("journal check: ") + path + " and its .inputs file hold " + std::to_string(a.size()) + " and " + std::to_string(b.size()) + " block(s)"; return 1; }
  int k = 0;
  for (int q = CMX_JOURNAL_MIN_LOG2; q <= CMX_JOURNAL_MAX_LOG2 && !k; ++q)   // the block size the positions imply: the first block's end, or the smallest block that holds a lone partial one
    if (a.size() > 1 ? a[0][0] == (1ull << q) >> 3 : a[0][0] <= (1ull << q) >> 3) k = q;
  if (!k) { if (err) *err = std::string("journal check: ") + path + ": the first block ends at byte " + std::to_string(a[0][0]) + ", which no block size of 2^6..2^19 bits gives"; return 1; }
  want->clear();
  for (size_t i = 0; i < a.size(); ++i) {
    if (a[i][0] != b[i][0]) { if (err) *err = std::string("journal check: ") + path + " and its .inputs file list different blocks"; return 1; }
    want->push_back({a[i][0], a[i][1 + 130], b[i][1 + 47]});
  }
  *log2_block_bits = k;
  return 0;
}

int cmx_journal_append_files(const char* path, const uint64_t* records, size_t n, bool truncate, std::string* err) {
  const std::string pa = path, pb = pa + ".inputs";
  FILE* fa = fopen(pa.c_str(), truncate ? "w" : "a");
  FILE* fb = fopen(pb.c_str(), truncate ? "w" : "a");
  if (!fa || !fb) { if (fa) fclose(fa); if (fb) fclose(fb); if (err) *err = "stream journal: cannot write " + pa + " / " + pb; return 1; }
  for (size_t i = 0; i < n; ++i) {
    const uint64_t* r = records + i * CMX_JOURNAL_RECORD;
    fprintf(fa, "%llu", (unsigned long long)r[0]);
    fprintf(fb, "%llu", (unsigned long long)r[0]);
    for (int w = 0; w < 131; ++w) fprintf(fa, " %016llx", (unsigned long long)r[1 + w]);
    for (int w = 131; w < CMX_JOURNAL_WORDS; ++w) fprintf(fb, " %016llx", (unsigned long long)r[1 + w]);
    fprintf(fa, "\n");
    fprintf(fb, "\n");
  }
  const bool ok = fflush(fa) == 0 && fflush(fb) == 0;
  fclose(fa); fclose(fb);
  if (!ok && err) *err = "stream journal: writing " + pa + " failed";
  return ok ? 0 : 1;
}

extern "C" size_t cmx_journal_host_digest(const float* p, const uint8_t* bits, size_t nbits, uint64_t stream_bit0, int log2_block_bits, uint64_t* out) {
  if (!out || nbits == 0 || log2_block_bits < CMX_JOURNAL_MIN_LOG2 || log2_block_bits > CMX_JOURNAL_MAX_LOG2) return 0;
  const int k = log2_block_bits;
  const size_t span = cmx_journal_span(k, nbits, stream_bit0);
  const uint64_t end = stream_bit0 + nbits;
  for (size_t i = 0; i < span; ++i) {
    const uint64_t blk_end = ((stream_bit0 >> k) + i + 1) << k;
    out[3 * i] = (blk_end < end ? blk_end : end) >> 3;
    out[3 * i + 1] = out[3 * i + 2] = 0;
  }
  for (size_t r = 0; r < nbits; ++r) {
    const uint64_t t = stream_bit0 + r, b = cmx_journal_B(t);
    uint64_t* rec = out + 3 * (size_t)((t >> k) - (stream_bit0 >> k));
    if (p) { uint32_t u; memcpy(&u, &p[r], 4); rec[1] += ((uint64_t)u + 1ull) * b; }
    if (bits) rec[2] += ((uint64_t)bits[r] + 1ull) * b;
  }
  return span;
}
