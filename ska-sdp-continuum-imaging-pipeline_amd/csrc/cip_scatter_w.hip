// cip_scatter_w.hip - one kernel support per translation unit: compiled once
// per W in {4, 6, ..., 16} with -DCIP_SCATTER_W=W (Makefile), so the scatter
// instantiations build in parallel.
#include "cip_scatter.h"

#ifndef CIP_SCATTER_W
#error "compile with -DCIP_SCATTER_W=<support>"
#endif

namespace cip {
template hipError_t launch_scatter_w<CIP_SCATTER_W>(const ScatterLaunch&, dim3, unsigned, hipStream_t);
}  // namespace cip
