// integration/predictor_dropin.h -- the drop-in `class Predictor` (src/predictor.h:17-22) for a build that links NO
// reference model object: the four members forward to the C ABI, and compression runs in the library's look-ahead mode
// (cmx_stage_input): every model family is a device stage and Predict() / Perceive() pop and check the probabilities of
// chunks that have already left the mixing network. src/coder/*, src/preprocess/* and src/runner.cpp compile against
// it unmodified; the one thing the reference does not have is the look-ahead itself, so a maintainer adds ONE line to
// RunCompression (runner.cpp:205-206), after the pretraining call and before Compress():
//
//       Predictor p(vocab);
//       if (enable_preprocess) preprocessor::Pretrain(&p, dictionary);
//   +   p.StageInput(&temp_in, temp_bytes);          // the bytes Compress() is about to code
//       Compress(temp_bytes, &temp_in, &data_out, output_bytes, &p);
//
// (oracle/Makefile target `dropin_engine` applies exactly that line to a scratch copy of runner.cpp at build time.)
// Decompression cannot look ahead: without StageInput the handle builds the per-bit stages, which take the fxcm / paq8
// columns from the caller -- integration/predictor.h is the shim for that direction.
#ifndef PREDICTOR_H
#define PREDICTOR_H

#include <cstdio>
#include <cstdlib>
#include <istream>
#include <vector>

#include "cmix_amd.h"

extern char* dictionary_path;  // runner.cpp:17

// SURVEY.md 8f-3 without touching main(): the vocabulary-independent stages the engine needs whatever the input is (mixing network,
// paq8 stage: ~12 GB of tables) start being built on a library thread when the program starts, i.e. while runner.cpp parses its
// arguments and preprocesses the input into the temp file; the Predictor constructed afterwards adopts them (cmx_prewarm). The fxcm
// stage waits for the dictionary path, which only main() knows. CMIX_NO_PREWARM=1 switches this off (decompression does not use
// the chunk pipeline's stages).
inline void cmx_dropin_prewarm_once() {
  static const int once = []() {
    if (!getenv("CMIX_NO_PREWARM")) { const char* dev = getenv("CMIX_DEVICE"); (void)cmx_prewarm(dev ? atoi(dev) : 0, NULL, 0); }
    return 0;
  }();
  (void)once;
}
namespace { struct CmxAtStart { CmxAtStart() { cmx_dropin_prewarm_once(); } } cmx_at_start; }

class Predictor {
 public:
  explicit Predictor(const std::vector<bool>& vocab) {
    unsigned char v[256];
    for (int i = 0; i < 256; ++i) v[i] = vocab[i] ? 1 : 0;
    const char* dev = getenv("CMIX_DEVICE");
    h_ = cmx_create(v, dictionary_path, dev ? atoi(dev) : 0);
    if (!h_) Die();
    // CMIX_VERIFY=1: the mixing network checks every word it consumes; a mismatch stops the program before a wrong file is finished (a decoder is not covered)
    const char* ver = getenv("CMIX_VERIFY");
    if (ver && ver[0] == '1' && cmx_set_verify(h_, 1)) Die();
    // CMIX_SHADOW=1|2: that many shadow mixing networks run beside the stream's own and vote on every chunk's probabilities (a decoder is not covered)
    const char* sha = getenv("CMIX_SHADOW");
    if (sha && (sha[0] == '1' || sha[0] == '2') && cmx_set_shadow(h_, sha[0] - '0')) Die();
    // CMIX_SHADOW_REPAIR=N (with CMIX_SHADOW=2 only): up to N times an outvoted instance is repaired from the majority and the stream carries on
    const char* rep = getenv("CMIX_SHADOW_REPAIR");
    if (rep && atoi(rep) > 0) {
      if (!sha || sha[0] != '2') { fprintf(stderr, "cmix_amd: CMIX_SHADOW_REPAIR needs CMIX_SHADOW=2 (a vote of two has no majority)\n"); exit(1); }
      if (cmx_set_shadow_repair(h_, atoi(rep))) Die();
    }
    // CMIX_CTX_SHADOW=1|2: that many shadow context stages run beside the stream's own and vote on every chunk's 54 columns and 47 selectors (a decoder is not covered)
    const char* csh = getenv("CMIX_CTX_SHADOW");
    if (csh && (csh[0] == '1' || csh[0] == '2') && cmx_set_ctx_shadow(h_, csh[0] - '0')) Die();
    // CMIX_LSTM_SHADOW=1|2: that many shadow LSTM stages run beside the stream's own and vote on every chunk's distributions, bit predictions and ex (a decoder is not covered)
    const char* lsh = getenv("CMIX_LSTM_SHADOW");
    if (lsh && (lsh[0] == '1' || lsh[0] == '2') && cmx_set_lstm_shadow(h_, lsh[0] - '0')) Die();
    // CMIX_FXCM_SHADOW=1|2: that many shadow fxcm stages run beside the stream's own and vote on every chunk's 431 columns (a decoder is not covered)
    const char* fsh = getenv("CMIX_FXCM_SHADOW");
    if (fsh && (fsh[0] == '1' || fsh[0] == '2') && cmx_set_fxcm_shadow(h_, fsh[0] - '0')) Die();
    // CMIX_JOURNAL=path [CMIX_JOURNAL_LOG2=k, default 19 = 64 KB]: per-block digests of what the mixing network read and wrote go to `path` and `path.inputs` as the
    // run goes (-c: all 179 words per block, from the device; -d: the p and bits words, folded on this thread). CMIX_JOURNAL_CHECK=path (-d): the decode is held to a
    // compressor's journal block by block and stops at the first block whose p or bits word differs (the block size comes from that file). cmx_create reads the three
    // itself (the one switch the library takes from the environment: a journal works in a program whichever shim it was compiled against); Perceive writes as it goes.
    // CMIX_STATE_JOURNAL=path [CMIX_STATE_JOURNAL_EVERY=n chunks]: cmx_create reads it at the same place. -c: one record of every device stage's state digests after every
    // n-th chunk of 4096 bytes and after the last goes to `path` (a file of its own); -d: the decoder is not covered, says so on stderr and decodes as before.
  }
  ~Predictor() {
    // the rest of the journal, the partial last block included; with CMIX_JOURNAL_CHECK the last block and the block count are compared here (nothing without a journal)
    if (cmx_journal_close_files(h_)) Die();
    if (cmx_state_journal_close(h_)) Die();   // the state journal's record after the last chunk (nothing without CMIX_STATE_JOURNAL)
    uint64_t rep[2 + CMX_REPAIR_LOG * CMX_REPAIR_WORDS];   // one line per repair on the majority: none without an event
    if (cmx_shadow_repairs(h_, rep, sizeof rep / sizeof rep[0]) == 0)
      for (uint64_t i = 0; i < rep[1]; ++i)
        fprintf(stderr, "cmix_amd: repair %llu of %llu: %s\n", (unsigned long long)(rep[0] - rep[1] + i + 1), (unsigned long long)rep[0], cmx_repair_text(rep + 2 + i * CMX_REPAIR_WORDS));
    cmx_destroy(h_);
  }
  Predictor(const Predictor&) = delete;
  Predictor& operator=(const Predictor&) = delete;

  // The next n bytes of *is, handed to the engine ahead of the coder; the stream is left where it was.
  void StageInput(std::istream* is, unsigned long long n) {
    const std::istream::pos_type at = is->tellg();
    std::vector<unsigned char> buf(1 << 20);
    while (n) {
      const size_t m = n < buf.size() ? (size_t)n : buf.size();
      is->read((char*)buf.data(), (std::streamsize)m);
      if ((size_t)is->gcount() != m) { fprintf(stderr, "cmix_amd shim: short read while staging the input\n"); abort(); }
      if (cmx_stage_input(h_, buf.data(), m)) Die();
      n -= m;
    }
    if (cmx_stage_input(h_, NULL, 0)) Die();   // end of input: the ragged last chunk goes now
    is->clear();
    is->seekg(at);
  }

  float Predict() {  // predictor.cpp:361-419
    const float p = cmx_predict(h_);
    if (p < 0) Die();
    return p;
  }
  void Perceive(int bit) {  // predictor.cpp:421-469
    if (cmx_perceive(h_, bit)) Die();
  }
  void Pretrain(int bit) {  // predictor.cpp:471-487
    if (cmx_pretrain(h_, bit)) Die();
  }

 private:
  static void Die() {  // the reference has no error path: report and stop
    fprintf(stderr, "cmix_amd: %s\n", cmx_last_error());
    abort();
  }
  cmx_t* h_;
};

#endif
