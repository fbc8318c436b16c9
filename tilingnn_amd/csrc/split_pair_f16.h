// fp32 values -> fp16 pairs (hi + lo) for the matrix cores: the split the NNConv edge-group kernels run on gathered rows and on
// their messages (nnconv_eg.hip, nnconv64_eg.hip)
#pragma once
#include <hip/hip_runtime.h>

namespace tgnn {

// a = x . s (s a power of two: exact) -> fp16 pair hi = RN16(a), lo = RN16(a - hi); 5 instructions per two values, none of them
// a multiply of its own: v_fma_mixlo_f16 / v_fma_mixhi_f16 (hi = RN16(x s)), 2 x v_fma_mix_f32 (x s - hi, hi read as fp16),
// v_cvt_pk_f16_f32
__device__ __forceinline__ void split_pair_f16(float x0, float x1, float s, unsigned &hi, unsigned &lo) {
    unsigned h;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h) : "v"(x0), "v"(s));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h) : "v"(x1), "v"(s));
    float l0, l1;
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(l0) : "v"(x0), "v"(s), "v"(h));
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(l1) : "v"(x1), "v"(s), "v"(h));
    using h2 = __attribute__((ext_vector_type(2))) _Float16;
    h2 lv;
    lv[0] = (_Float16)l0;
    lv[1] = (_Float16)l1;
    hi = h;
    lo = __builtin_bit_cast(unsigned, lv);
}
// the same without a scale (the messages: in range by construction); 4 instructions per two values
__device__ __forceinline__ void split_pair_f16(float a0, float a1, unsigned &hi, unsigned &lo) {
    using h2 = __attribute__((ext_vector_type(2))) _Float16;
    h2 hv;
    hv[0] = (_Float16)a0;
    hv[1] = (_Float16)a1;
    hi = __builtin_bit_cast(unsigned, hv);
    float l0, l1;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l0) : "v"(hi), "v"(a0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(l1) : "v"(hi), "v"(a1));
    h2 lv;
    lv[0] = (_Float16)l0;
    lv[1] = (_Float16)l1;
    lo = __builtin_bit_cast(unsigned, lv);
}

}  // namespace tgnn
