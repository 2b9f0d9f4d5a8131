// The words of the pipeline's shadow stages (cmix_amd/csrc/cmx_shadow_text.h) behind a C ABI, for tests/test_shadow_text.py.
#include "../../cmix_amd/csrc/cmx_shadow_text.h"

static thread_local std::string g_text;
static const char* keep(const std::string& s) { g_text = s; return g_text.c_str(); }

extern "C" {
const char* st_vote(int kind, const uint64_t r[8]) { return keep(shadow_vote_text(kind, r)); }
const char* st_timeout(int kind, int instance, long long chunk) { return keep(shadow_timeout_text(kind, instance, chunk)); }
const char* st_no_instance(int kind, const char* before, const char* after) { return keep(shadow_no_instance_text(kind, shadow_fn(kind, before, after))); }
const char* st_queue(int kind, int held, int device, int k, int limit) { return keep(shadow_queue_text(kind, held, device, k, limit)); }
const char* st_origin(uint64_t m0, uint64_t m12) { return keep(origin_text(m0, m12)); }
const char* st_repair_entry(const uint64_t* e) { return keep(repair_entry_text(e)); }
}
