// cmx_shadow_text.h -- the words of the pipeline's four kinds of shadow stages and of their votes' error messages, in one table; and the
// mixing network's repair log in words. Host only, standard headers only: tests/host/shadow_text.cpp builds it with a plain C++ compiler.
#pragma once
#include <cstdint>
#include <string>

// The kinds, in the order in which a handle holds them (cmx_pipeline_destroy drops them in this order, the overlap probe lists their streams in it).
enum ShadowId { SH_MIX = 0, SH_CTX = 1, SH_LSTM = 2, SH_FXCM = 3, SH_KINDS = 4 };

struct ShadowWords {
  const char* stem;       // the public names: cmx_pipeline_set_<stem>, cmx_pipeline_<stem>_report, cmx_pipeline_debug_<stem>_xor, cmx_set_<stem>, ...
  const char* noun;       // one of them, in messages
  const char* vote;       // how a vote's message begins
  const char* instances;  // what a vote compares
  const char* unit;       // what a vote's positions count: bits, or the LSTM's bytes
  const char* odd0;       // instance 0 in a vote's message
  const char* own;        // instance 0 in "no such instance"
  const char* since;      // from when on the shadow handles exist
  const char* late_who;   // a timed-out hand-off: whose, in front of the instance's number (NULL: the context stage has none, one workgroup)
  const char* late_what;  // ... and what is void
  std::string (*where)(uint64_t pos, uint64_t c);   // the element of a vote's first event: behind the position, column c of the record's [5]
};

static inline std::string shadow_where_mix(uint64_t, uint64_t c) { return ", " + (c < 47 ? "mixer " + std::to_string(c) : std::string("final p")); }
static inline std::string shadow_where_ctx(uint64_t, uint64_t c) {   // lane order: layer-0 columns 0, 1, 2, 2025..2075, then the 47 selectors
  return ", " + (c < 54 ? "layer-0 column " + std::to_string(c < 3 ? c : 2025 - 3 + c) : "selector " + std::to_string(c - 54));
}
static inline std::string shadow_where_lstm(uint64_t, uint64_t c) {
  return ", " + (c < 256 ? "distribution entry " + std::to_string(c) : c < 264 ? "bit " + std::to_string(c - 256) + "'s prediction (layer-0 column 2077)" : "bit " + std::to_string(c - 264) + "'s ex");
}
static inline std::string shadow_where_fxcm(uint64_t pos, uint64_t c) {
  return " (byte " + std::to_string(pos >> 3) + ", bit " + std::to_string(pos & 7) + "), fxcm column " + std::to_string(c) + " (layer-0 column " + std::to_string(3 + c) + ")";
}

static inline const ShadowWords& shadow_words(int kind) {
  static const ShadowWords w[SH_KINDS] = {
      {"shadow", "shadow mixing network", "shadow vote", "mixing-network", "bit", "network", "the stream's network", "the first chunk", "shadow mixing network ", "the vote", shadow_where_mix},
      {"ctx_shadow", "shadow context stage", "context shadow vote", "context-stage", "bit", "stage", "the stream's own stage", "the first chunk", nullptr, nullptr, shadow_where_ctx},
      {"lstm_shadow", "shadow LSTM stage", "LSTM shadow vote", "LSTM-stage", "byte", "stage", "the stream's own stage", "the first chunk", "the LSTM kernels of shadow instance ", "the LSTM vote",
       shadow_where_lstm},
      {"fxcm_shadow", "shadow fxcm stage", "fxcm shadow vote", "fxcm-stage", "bit", "stage", "the stream's own stage", "the first chunk or pretrain", "the fxcm kernel of shadow instance ",
       "the fxcm vote", shadow_where_fxcm},
  };
  return w[kind];
}
// "cmx_pipeline_set_ctx_shadow" = shadow_fn(SH_CTX, "cmx_pipeline_set_", ""): a public function's name, for the front of its messages
static inline std::string shadow_fn(int kind, const char* before, const char* after) { return std::string(before) + shadow_words(kind).stem + after; }

// What a vote's record (the eight words of cmx_vote_report and its three kin) says, for an error message
static inline std::string shadow_vote_text(int kind, const uint64_t r[8]) {
  const ShadowWords& w = shadow_words(kind);
  std::string s = std::string(w.vote) + ": the " + std::to_string(r[2]) + " " + w.instances + " instances disagree in " + std::to_string(r[7]) + " value(s) of the chunk, first at stream " + w.unit +
                  " " + std::to_string(r[4]) + w.where(r[4], r[5]) + ": ";
  if (r[6] == ~0ull) s += "no majority between " + std::to_string(r[2]) + " instances";
  else s += "instance " + std::to_string(r[6]) + " is the odd one" + (r[6] == 0 ? std::string(" (the stream's own ") + w.odd0 + ")" : std::string());
  return s + " (the stream's output is void)";
}
// An in-launch hand-off of shadow `instance` (1 or 2) timed out: as cmx_pipeline_wait says it of a chunk, or (chunk < 0) cmx_pipeline_sync of the stream
static inline std::string shadow_timeout_text(int kind, int instance, int64_t chunk) {
  const ShadowWords& w = shadow_words(kind);
  return std::string(chunk < 0 ? "cmx_pipeline_sync" : "cmx_pipeline_wait") + ": an in-launch hand-off of " + w.late_who + std::to_string(instance) + " timed out (workgroups not co-resident?): " +
         w.late_what + " is void" + (chunk < 0 ? std::string() : " from chunk " + std::to_string(chunk) + " on");
}
static inline std::string shadow_no_instance_text(int kind, const std::string& fn) {
  const ShadowWords& w = shadow_words(kind);
  return fn + ": no such instance (0 = " + w.own + ", 1.. = the shadows, which exist from " + w.since + " on)";
}
static inline std::string shadow_queue_text(int kind, int held, int device, int k, int limit) {
  return shadow_fn(kind, "cmx_pipeline_set_", "") + ": this process holds " + std::to_string(held) + " dedicated hardware queues on device " + std::to_string(device) + " and " + std::to_string(k) + " " +
         shadow_words(kind).noun + "(s) need one each, the limit is " + std::to_string(limit);
}

// ---- the mixing network's repair on the majority (cmx_pipeline_shadow_repairs) ----
static inline std::string origin_text(uint64_t m0, uint64_t m12) {
  for (int i = 0; i < 26; ++i) if (m0 >> i & 1) return "mixer " + std::to_string(i);
  for (int i = 0; i < 21; ++i) if (m12 >> i & 1) return "mixer " + std::to_string(26 + i);
  return "no mixer row (tables / scalars only)";
}
// one entry of the repair log in words
static inline std::string repair_entry_text(const uint64_t* e) {
  return "chunk " + std::to_string(e[0]) + ", stream bit " + std::to_string(e[1]) + shadow_where_mix(0, e[2]) + ", instance " + std::to_string(e[3]) + " odd, " + std::to_string(e[5]) +
         " state word(s) repaired, origin " + origin_text(e[12], e[13]);
}
