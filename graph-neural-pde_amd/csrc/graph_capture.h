// Stream capture of a launch sequence into an executable hipGraph, and its release: the one statement every solver of the library uses
// (solver.hip, adjoint.hip, sharded.hip, dopri5.hip, adjoint_adaptive.hip).
#pragma once
#include "common.h"

namespace gnpde {

// Capture what enqueue(stream) launches -- on a non-blocking stream of the solver's own, created on first use, in thread-local capture
// mode -- into *graph and instantiate it as *exec.  A failing enqueue ends the capture, drops the graph and returns its code; `who`
// prefixes the message of a failing end of capture.
template <typename F>
int capture_into(hipStream_t* cap_stream, hipGraph_t* graph, hipGraphExec_t* exec, F&& enqueue, const char* who = "") {
  if (*cap_stream == nullptr) GNPDE_HIP(hipStreamCreateWithFlags(cap_stream, hipStreamNonBlocking));
  GNPDE_HIP(hipStreamBeginCapture(*cap_stream, hipStreamCaptureModeThreadLocal));
  const int rc = enqueue(*cap_stream);
  hipGraph_t gobj = nullptr;
  const hipError_t ec = hipStreamEndCapture(*cap_stream, &gobj);
  if (rc != 0) {
    if (gobj) (void)hipGraphDestroy(gobj);
    return rc;
  }
  if (ec != hipSuccess) {
    set_error("%shipStreamEndCapture failed: %s", who, hipGetErrorString(ec));
    return static_cast<int>(ec);
  }
  *graph = gobj;
  GNPDE_HIP(hipGraphInstantiate(exec, gobj, nullptr, nullptr, 0));
  return 0;
}

inline void drop_capture(hipGraph_t* graph, hipGraphExec_t* exec) {
  if (*exec) { (void)hipGraphExecDestroy(*exec); *exec = nullptr; }
  if (*graph) { (void)hipGraphDestroy(*graph); *graph = nullptr; }
}

}  // namespace gnpde
