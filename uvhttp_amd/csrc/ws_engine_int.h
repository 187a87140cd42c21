// The engine bits a source outside ws_gpu.hip needs to add a device call to the engine
// (utf8_gpu.hip): the engine's device, the stream hand-over every call goes through, and
// last_error.  Defined in ws_gpu.hip; internal to the library (hidden symbols).
#ifndef UVHTTP_WS_ENGINE_INT_H
#define UVHTTP_WS_ENGINE_INT_H

#include <hip/hip_runtime.h>

#include "device_guard.h"
#include "uvhttp_ws_amd.h"

#define UVWS_INTERNAL __attribute__((visibility("hidden")))

// The dispatch packet counts work-items in 32 bits, so a pass of `tiles` workgroups goes out in
// launches of at most `piece` (the engine's grid_piece: kMaxGrid = 2^24 in the product; the
// experiment build's UVHTTP_WS_GRID_PIECE makes it small, so that tests run every chunked pass in
// several pieces): launch(grid, tile_base) once per piece, none for an empty pass.  Returns the
// number of pieces launched.
constexpr uint64_t kMaxGrid = 1ull << 24;
template <class F>
static inline uint64_t for_grid_chunks(uint64_t piece, uint64_t tiles, F&& launch) {
    uint64_t pieces = 0;
    for (uint64_t tb = 0; tb < tiles; tb += piece, ++pieces)
        launch((uint32_t)(tiles - tb < piece ? tiles - tb : piece), tb);
    return pieces;
}

extern "C" {

// Start of a call (EngineCall in ws_gpu.hip, in two halves): makes the engine's device current
// (returns the one that was), then notes whether `s` is being captured and, when the call names
// another stream than the previous call, makes `s` wait for the work already queued on that one
// (call_begin).
UVWS_INTERNAL int uvws_call_enter(uvhttp_ws_gpu_engine_t* e, hipStream_t s);
// End of a call: turns a pending HIP launch error into UVHTTP_WS_GPU_ELAUNCH with last_error set
// ("<what>: <hip error>"), else OK; leaves capture mode and restores the device.
UVWS_INTERNAL int uvws_call_leave(uvhttp_ws_gpu_engine_t* e, int prev_device, const char* what);
// Sets last_error and returns `code`.
UVWS_INTERNAL int uvws_set_err(uvhttp_ws_gpu_engine_t* e, int code, const char* what);
// The engine's piece limit, for_grid_chunks' first argument (grid_piece).
UVWS_INTERNAL uint64_t uvws_grid_piece(const uvhttp_ws_gpu_engine_t* e);
// After a chunked pass: what for_grid_chunks covered and returned.  The experiment build counts
// them for the grid-piece tests (uvhttp_ws_gpu_test_grid_pieces); the product does nothing.
UVWS_INTERNAL void uvws_grid_note(uvhttp_ws_gpu_engine_t* e, uint64_t tiles, uint64_t pieces);
// The frame UTF-8 validator's engine-owned scratch of at least `bytes` (not zeroed), grown on
// the call's stream by the rule of every scratch block (scratch_fit in ws_gpu.hip); null when
// it cannot grow (a captured call that would allocate, or out of memory).  Call between
// uvws_call_enter and uvws_call_leave.
UVWS_INTERNAL void* uvws_utf8_scratch(uvhttp_ws_gpu_engine_t* e, uint64_t bytes, hipStream_t s);
// The control replies' scratch (ws_replies_gpu.hip), likewise.
UVWS_INTERNAL void* uvws_replies_scratch(uvhttp_ws_gpu_engine_t* e, uint64_t bytes, hipStream_t s);
// The echo of data messages' scratch (ws_echo_gpu.hip), likewise.
UVWS_INTERNAL void* uvws_echo_scratch(uvhttp_ws_gpu_engine_t* e, uint64_t bytes, hipStream_t s);
// The server's own CLOSE frames' scratch (ws_close_gpu.hip), likewise.
UVWS_INTERNAL void* uvws_close_scratch(uvhttp_ws_gpu_engine_t* e, uint64_t bytes, hipStream_t s);
// The fail points' scratch (ws_fail_gpu.hip), likewise.
UVWS_INTERNAL void* uvws_fail_scratch(uvhttp_ws_gpu_engine_t* e, uint64_t bytes, hipStream_t s);

}  // extern "C"

// A chunked pass of engine `e`: for_grid_chunks at the engine's piece limit, noted.
template <class F>
static inline void engine_grid_chunks(uvhttp_ws_gpu_engine_t* e, uint64_t tiles, F&& launch) {
    uvws_grid_note(e, tiles, for_grid_chunks(uvws_grid_piece(e), tiles, launch));
}

#endif
