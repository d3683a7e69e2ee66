// cv2.borderInterpolate on the device: shared by the sampler of the affine and field warps (warp_sample.h: warp.hip, warp_field.hip), the
// elastic-field filter (warp_field.hip) and the separable blur (pixel_aug.hip)
#pragma once

#include <hip/hip_runtime.h>

namespace unet {

constexpr int B_CONSTANT = 0, B_REPLICATE = 1, B_REFLECT = 2, B_REFLECT101 = 4;      // cv2 border codes

// cv2.borderInterpolate for |i| <= 2^24 + 1 and N >= 1: an index in [0, N), or -1 (constant border: take the fill value)
template <int BORDER>
__device__ __forceinline__ int border_index(int i, int N) {
    if (i >= 0 && i < N) return i;
    if (BORDER == B_CONSTANT) return -1;
    if (BORDER == B_REPLICATE) return i < 0 ? 0 : N - 1;
    if (BORDER == B_REFLECT) {                         // fedcba|abcdef|fedcba: period 2N
        const int P = 2 * N;
        const int r = ((i % P) + P) % P;               // [0, 2N)
        return r < N ? r : P - 1 - r;                  // [0, N)
    }
    // B_REFLECT101, gfedcb|abcdefg|fedcba: period 2N - 2
    if (N == 1) return 0;
    const int P = 2 * N - 2;
    const int r = ((i % P) + P) % P;                   // [0, 2N - 2)
    return r < N ? r : P - r;                          // [0, N)
}

}  // namespace unet
