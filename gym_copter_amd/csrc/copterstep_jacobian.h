// Internal declarations between the C-ABI layer (copterstep_api.hip: contexts, error reporting) and
// copterstep_jacobian.hip (cs_step_jacobian and its kernels).  Not installed; the public ABI is include/copterstep.h.
#pragma once

#include "copterstep_internal.h"

namespace cs {

// what an entry point launches on: the context's task, storage mode, constants and device state
struct ContextView {
  int task, mode;
  const DevConst* c;
  const DevState* s;
};
// (copterstep_api.hip) check the context as every entry point does (null, served session, draining) and describe it
int enter_context(cs_ctx* ctx, const char* who, void* stream, ContextView* out);
// (copterstep_api.hip) set cs_last_error() and return `code` / CS_ERR_HIP
int report_error(int code, const char* message);
int report_hip(hipError_t e, const char* what);

}  // namespace cs
