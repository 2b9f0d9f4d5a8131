// fxcm_state.h -- a handle's state arrays as cmx_fxcm_state_diff / _debug_state_xor / _debug_layout walk them (fxcm_vote.hip; the view itself is
// built in fxcm_stage.hip from the blocks fxb::build asked for, in its order). Region numbers and the array order inside each: include/cmix_amd.h.
#ifndef CMX_FXCM_STATE_H
#define CMX_FXCM_STATE_H
#include <stdint.h>

#include <vector>

#define FX_STATE_REGIONS 12
#define FX_STATE_ARRAYS 141        // 140 blocks of fxb::build, then FxDev itself
#define FX_REGION_DEV 11           // the non-pointer fields of FxDev: compared on the host from masked copies
struct FxRegion { int region; uint32_t* p; unsigned long long words; };

struct cmx_fxcm;
// the 140 device arrays in region-then-build order; 0 = ok
int cmx_fxcm_state_view(cmx_fxcm* h, FxRegion* out, int* n, int* device, uint64_t* bytes_done);
// FxDev as 32-bit words with every device pointer and the padding of the match candidates zeroed; synchronises; 0 = ok
int cmx_fxcm_dev_words(cmx_fxcm* h, std::vector<uint32_t>& out);
#endif
