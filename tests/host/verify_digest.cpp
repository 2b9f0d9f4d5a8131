// Host build of cmix_amd/csrc/cmx_verify.h (the digest of the mixing network's verify mode) for tests/test_verify_digest.py.
#include <stddef.h>
#include <stdint.h>
#include "../../cmix_amd/csrc/cmx_verify.h"

extern "C" {
uint64_t vd_mix(uint32_t c, uint32_t t, uint32_t i, uint32_t w) { return cmx_vmix(c, t, i, w); }
uint64_t vd_key(uint32_t blk, uint32_t cls, uint32_t m, uint32_t row, uint32_t seg) { return cmx_vkey(blk, cls, m, row, seg); }
uint32_t vd_mix_class(uint32_t cls) { return cmx_vmix_class(cls); }
// block sums of class c over words[nbits][nwords] (bit t0 + k for row k), bits in order
void vd_block_sums(uint32_t c, uint32_t t0, const uint32_t* words, int nbits, int nwords, uint64_t* out) {
  for (int b = 0; b * CMX_VERIFY_BLOCK < nbits; ++b) out[b] = 0;
  for (int k = 0; k < nbits; ++k)
    for (int i = 0; i < nwords; ++i) out[k / CMX_VERIFY_BLOCK] += cmx_vmix(c, t0 + (uint32_t)k, (uint32_t)i, words[(size_t)k * nwords + i]);
}
int vd_block() { return CMX_VERIFY_BLOCK; }
}
