// ToTensor + Normalize of one grey level, shared by image_crop.hip and image_finish.hip so that the
// uint8 crop followed by normalize_erase gives the bits of the float crop. The fused multiply-add is
// spelled out: image_crop.hip is compiled with -ffp-contract=fast (where v * k - mean contracts to
// this) and image_finish.hip with =off (where it would not).
#pragma once
#include <hip/hip_runtime.h>

namespace tdp {

__device__ __forceinline__ float image_normalize(float v, float mean, float inv_std) {
  return __builtin_fmaf(v, 1.f / 255.f, -mean) * inv_std;
}

}  // namespace tdp
