// Philox4x32-10 on the device (the definition in include/unet_hip.h; augment.philox4x32_10 on the host): shared by the Gaussian noise of
// pixel_aug.hip and the elastic field of warp_field.hip
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace unet {

// the four words of counter (c0, c1, 0, 0) under the key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t w[4]) {
    uint32_t c2 = 0, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

}  // namespace unet
