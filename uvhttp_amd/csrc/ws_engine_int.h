// The engine bits a source outside ws_gpu.hip needs to add a device call to the engine
// (utf8_gpu.hip): the engine's device, the stream hand-over every call goes through, and
// last_error.  Defined in ws_gpu.hip; internal to the library (hidden symbols).
#ifndef UVHTTP_WS_ENGINE_INT_H
#define UVHTTP_WS_ENGINE_INT_H

#include <hip/hip_runtime.h>

#include "uvhttp_ws_amd.h"

#define UVWS_INTERNAL __attribute__((visibility("hidden")))

extern "C" {

// Start of a call: makes the engine's device current (returns the one that was), notes whether
// `s` is being captured and, when the call names another stream than the previous call, makes
// `s` wait for the work already queued on that one (call_begin in ws_gpu.hip).
UVWS_INTERNAL int uvws_call_enter(uvhttp_ws_gpu_engine_t* e, hipStream_t s);
// End of a call: leaves capture mode, restores the device, and turns a pending HIP launch error
// into UVHTTP_WS_GPU_ELAUNCH with last_error set ("<what>: <hip error>"); else OK.
UVWS_INTERNAL int uvws_call_leave(uvhttp_ws_gpu_engine_t* e, int prev_device, const char* what);
// Sets last_error and returns `code`.
UVWS_INTERNAL int uvws_set_err(uvhttp_ws_gpu_engine_t* e, int code, const char* what);
// The frame UTF-8 validator's engine-owned scratch of at least `bytes` (not zeroed), grown on
// the call's stream like every other scratch block; null when it cannot grow (a captured call
// that would allocate, or out of memory).  Call between uvws_call_enter and uvws_call_leave.
UVWS_INTERNAL void* uvws_utf8_scratch(uvhttp_ws_gpu_engine_t* e, uint64_t bytes, hipStream_t s);
// The control replies' scratch (ws_replies_gpu.hip), by the same rule.
UVWS_INTERNAL void* uvws_replies_scratch(uvhttp_ws_gpu_engine_t* e, uint64_t bytes, hipStream_t s);

}  // extern "C"

#endif
