// Learnable cameras: one thread per slot (forward) / per camera (backward), the bodies of cnr_cameras.h.
#include <hip/hip_runtime.h>

#include "cnr_cameras.h"
#include "cnr_hip_util.h"

namespace cnr {

CNR_CAMERA_KERNELS(CNR_PW_KERNEL)

}  // namespace cnr
