// bf16_common.h -- the vector types and the fp32 -> bf16 conversion shared by the bf16 matrix-core sources (linear_bf16.hip,
// linear_bf16_train.hip).
#pragma once
#include <stdint.h>

#include "hf_common.h"

namespace hf {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// two floats -> two bf16 (round to nearest even) in one register, `lo` in the low half: v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi)
{
    const f32x2 v = { lo, hi };
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

static inline bool bf_aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace hf
