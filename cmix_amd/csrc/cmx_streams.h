// cmx_streams.h -- the library's one stream factory (cmx_api.hip): every HIP stream the stages create comes from cmx_make_stream and goes
// through cmx_destroy_stream. Each stream has a hardware queue of its own (a compute-unit mask: HIP does not pool such queues under
// GPU_MAX_HW_QUEUES), counted against CMX_MAX_HW_QUEUES per device.
#pragma once
#include <hip/hip_runtime.h>

// which: 0 = a stage's kernel stream, 1 = the mixing network's, 2 = an upload stream (copies only). 0 on success, else 1 with cmx_last_error set
// (the device's queue budget is spent, or the runtime refused the stream).
extern "C" int cmx_make_stream(hipStream_t* st, int which);
extern "C" void cmx_destroy_stream(hipStream_t st);
// one probe kernel on each distinct stream of st[0..n) (null entries skipped); returns how many saw all the others running beside them, -1 on
// a device error; *distinct = the number of distinct streams probed
extern "C" int cmx_overlap_probe(const hipStream_t* st, int n, int* distinct);
