// cmx_verify.h -- the digest of the mixing network's verify mode (cmx_mixnet_set_verify), shared by the kernels and the host.
//
// Every word w the network consumes -- word i of bit t in class c -- maps through cmx_vmix(c, t, i, w): a splitmix64 finaliser over the
// key (c, t, i) XOR w. For a fixed key the map is a bijection in w (XOR with a constant, then the finaliser, a bijection of 64-bit words).
// The digest of a block of CMX_VERIFY_BLOCK bits is the sum mod 2^64 of the mixed words of its bits: any ONE changed word always changes
// its block's sum, and partial sums may be added in any order (each wave folds its own bits; the verify kernel recomputes with another split).
#ifndef CMX_VERIFY_H
#define CMX_VERIFY_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CMX_VHD __host__ __device__ __forceinline__
#else
#define CMX_VHD static inline
#endif

#define CMX_VERIFY_BLOCK 64   /* bits per digest block */

// Classes (the report's `class`): what was consumed, and by whom. The two decay classes of the tail and the two ring classes fold the same
// words as their first member (same mix class); they are compared separately.
#define CMX_VC_ROW 1          /* the 2078 raw probs words of a bit the stretch waves load */
#define CMX_VC_BIT 2          /* the coded bit (u8 as a word) the stretch wave loads */
#define CMX_VC_SEL 3          /* the 47 selector words the select wave loads */
#define CMX_VC_DECAY_GATHER 4 /* the decay word of the bit, as the gather wave loaded it */
#define CMX_VC_DECAY_TAIL_A 5 /* ... the layer-1 tail wave */
#define CMX_VC_DECAY_TAIL_B 6 /* ... the layer-2 / SSE tail wave */
#define CMX_VC_RING_WRITTEN 7 /* the 2078 stretched inputs of a bit the stretch waves store into the in-launch ring */
#define CMX_VC_RING_READ 8    /* the ring slice a helper wave loads (the report names the helper's mixer) */
#define CMX_VC_SEGMENT 9      /* a layer-0 row segment a helper wave loads, against the digest it stored with it */
#define CMX_VC_N 10

// Per-block record of consumed sums (u64 words, CMX_VERIFY_REC per block; every word is written by one wave only -- no atomics):
#define CMX_VR_ROW 0          /* [0..3]   ROW, stretch wave sw */
#define CMX_VR_BIT 4          /* [4..7]   BIT, stretch wave sw */
#define CMX_VR_RINGW 8        /* [8..11]  RING_WRITTEN, stretch wave sw */
#define CMX_VR_SEL 12         /* [12]     SEL */
#define CMX_VR_DECAY 13       /* [13..15] decay of the gather, tail-a, tail-b waves */
#define CMX_VR_RINGR 16       /* [16 + 4 m + w] RING_READ, helper m's wave w */
#define CMX_VERIFY_REC 128

// Row-segment table: one digest per (layer-0 mixer, row, helper wave segment); 0 = never written (not checked). A segment's digest mixes with
// t = mixer * 10001 + row (the row's number in the network's table of layer-0 rows) and i = the word's index in the row.
#define CMX_VERIFY_SEGS 4

// Host-visible header of the verify area (device memory of the handle). launch_*: per launch, cleared before it; cum: the sticky record
// cmx_mixnet_verify_report returns.
struct CmxVerifyHdr {
  unsigned long long launch_count;   // mismatching blocks / row segments of the launch
  unsigned long long launch_first;   // ~key of the first of them (atomic max of ~key; 0 = none), see cmx_vkey
  unsigned long long pad[6];
  unsigned long long cum[8];         // chunks verified, bits verified, mismatches, first class, first stream bit, mixer, row, segment
};
#define CMX_VERIFY_CLEAR_BYTES 64    /* the launch_* part of the header */

// What the verify instantiation of the network kernel (cmx_mixnet_spec_verify_kernel) and cmx_mixnet_verify_kernel are launched with
struct CmxVerify {
  unsigned long long* rec;   // [blocks][CMX_VERIFY_REC] consumed sums of the launch (cleared before it)
  unsigned long long* seg;   // [26][10001][CMX_VERIFY_SEGS] digests of the stored row segments (0: never stored)
  CmxVerifyHdr* hdr;         // the launch's mismatch count and first key
  int pert_bit, pert_index;  // test hook (cmx_mixnet_debug_verify_perturb, ring): the stretch wave stores ring word pert_index of bit pert_bit XOR pert_mask and
  unsigned pert_mask;        //   folds the value it computed; pert_bit < 0: none
};

// The order in which "first" is decided: block, then class, then mixer, row, segment (all fields fit their widths: block < 2^24 bits / 64,
// mixer < 32, row < 2^14, segment < 4)
CMX_VHD unsigned long long cmx_vkey(uint32_t blk, uint32_t cls, uint32_t m, uint32_t row, uint32_t seg) {
  return ((unsigned long long)(blk & 0xffffffu) << 40) | ((unsigned long long)(cls & 15u) << 36) | ((unsigned long long)(m & 31u) << 31) |
         ((unsigned long long)(row & 0x3fffu) << 17) | ((unsigned long long)(seg & 3u) << 15);
}

CMX_VHD uint64_t cmx_fmix64(uint64_t x) {   // splitmix64's finaliser (a bijection of 64-bit words)
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}
CMX_VHD uint64_t cmx_vmix(uint32_t c, uint32_t t, uint32_t i, uint32_t w) {
  const uint64_t key = (((uint64_t)c << 60) ^ ((uint64_t)t << 24) ^ (uint64_t)i) * 0x9e3779b97f4a7c15ull;
  return cmx_fmix64(key ^ (uint64_t)w);
}
// the mix class of a report class: the tail's decay words and the helpers' ring words are the same words as the gather's / the stretch waves'
CMX_VHD uint32_t cmx_vmix_class(uint32_t cls) {
  return (cls == CMX_VC_DECAY_TAIL_A || cls == CMX_VC_DECAY_TAIL_B) ? CMX_VC_DECAY_GATHER : cls == CMX_VC_RING_READ ? CMX_VC_RING_WRITTEN : cls;
}

#endif
