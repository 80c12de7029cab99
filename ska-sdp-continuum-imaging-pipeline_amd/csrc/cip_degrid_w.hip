// cip_degrid_w.hip - one kernel support per translation unit: compiled once
// per W in {4, 6, ..., 16} with -DCIP_DEGRID_W=W (Makefile), so the degrid
// instantiations build in parallel.
#include "cip_degrid.h"

#ifndef CIP_DEGRID_W
#error "compile with -DCIP_DEGRID_W=<support>"
#endif

namespace cip {
template hipError_t launch_degrid_w<CIP_DEGRID_W>(const DegridLaunch&, dim3, hipStream_t);
}  // namespace cip
