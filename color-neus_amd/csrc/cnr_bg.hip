// N_OUTSIDE > 0, the NeRF++ background: one thread per ray / per point, the bodies of cnr_bg.h.  No shipped configuration takes this path.
#include <hip/hip_runtime.h>

#include "cnr_bg.h"
#include "cnr_hip_util.h"

namespace cnr {

CNR_BG_KERNELS(CNR_PW_KERNEL)

}  // namespace cnr
