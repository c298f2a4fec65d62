// The code value of a probability on the device, once, for every kernel that needs it (csrc/ac_codes.hip: ac_codes_k;
// csrc/ac_device_dec.hip: rc_decode_k):
//   c1 = (rint((1 - p) * 65534) + 1) & 0xFFFF                     (binary_c1 of csrc/ac.cpp; torchac's cdf row [0, c1, 2^16])
// as two separately rounded fp32 operations, the way the host computes them: a contracted fma(-p, 65534, 65534) rounds once.
// p is finite and in [0, 1]; outside that the host's lrintf and this conversion differ.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint32_t linr_c1_from_p(float p) {
    return ((uint32_t)__float2int_rn(__fmul_rn(__fsub_rn(1.0f, p), 65534.0f)) + 1u) & 0xFFFFu;
}
