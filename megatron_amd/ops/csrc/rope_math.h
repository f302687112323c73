// The rotate-half RoPE arithmetic, shared by rope.hip and qkv_rope.hip so that
// both kernels give the same bits.
//
//   o1 = x1*c - x2*s        o2 = x2*c + x1*s        (backward: s -> -s)
//
// Each output has one product rounded to fp32 and one fused into the add.
// Which one is fused changes the last bit, and left to the compiler's
// contraction it depends on the code around the expression (scalar here,
// packed two-wide there).  So it is pinned: the sine product is rounded, the
// cosine product is fused, which is what rope_kernel has always computed.
#pragma once

#include "common.h"

template <bool BWD>
__device__ __forceinline__ void rope_rotate(float x1, float x2, float c, float sn,
                                            float& o1, float& o2) {
  float sv = BWD ? -sn : sn;
  o1 = fma_rn(x1, c, -mul_rn(x2, sv));
  o2 = fma_rn(x2, c, mul_rn(x1, sv));
}
