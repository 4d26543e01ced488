// The frozen experiment copies (r03 .. r05) keep the launch idiom they were written with: a
// hipLaunchKernelGGL followed by this check of the launch that was just enqueued (configuration errors
// only; no sync). The product launches through csrc/dispatch.h's launch() instead.
#pragma once

#include "../../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/common.h"

#define SFA_LAUNCH_CHECK()                                                                      \
  do {                                                                                          \
    hipError_t e_ = hipGetLastError();                                                          \
    if (e_ != hipSuccess) {                                                                     \
      ::sfa::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, \
                       __LINE__);                                                               \
      return SFA_E_HIP;                                                                         \
    }                                                                                           \
  } while (0)
