// sdm_align_tensor_kernel.h -- what the crop-tensor kernels share around the per-pixel arithmetic (csrc/sdm_align_tensor.hip and
// csrc/sdm_align_area.hip): the workgroup size, the element types and the stores.  Device code only.
#pragma once
#include "sdm_kernels.h"
#include "sdm_align_tensor_device.h"

#include <limits.h>

#pragma clang fp contract(off)

#define ALIGN_T_BLOCK 256

template <int DT> struct AlignElem;
template <> struct AlignElem<SDM_ALIGN_U8> { typedef uint8_t T; };
template <> struct AlignElem<SDM_ALIGN_F16> { typedef _Float16 T; };
template <> struct AlignElem<SDM_ALIGN_F32> { typedef float T; };

template <int DT>
__device__ __forceinline__ typename AlignElem<DT>::T make_elem(uint32_t v, float scale, float bias)
{
    if constexpr (DT == SDM_ALIGN_U8) return (uint8_t)v;
    else if constexpr (DT == SDM_ALIGN_F32) return align_element(v, scale, bias);
    else return (_Float16)align_element(v, scale, bias);          // round to nearest even
}

// cnt <= CNT consecutive elements from element index e of out (16-byte aligned): whole groups of 4 as one vector store when e is a
// multiple of 4, the rest element by element
template <class T, int CNT>
__device__ __forceinline__ void store_run(void* out, long long e, const T (&vals)[CNT], int cnt)
{
    struct alignas(4 * sizeof(T)) Vec { T v[4]; };
    T* o = (T*)out + e;
    const bool aligned = (e & 3) == 0;
#pragma unroll
    for (int g = 0; g < CNT / 4; ++g) {
        if (aligned && cnt >= 4 * g + 4) {
            Vec v;
#pragma unroll
            for (int b = 0; b < 4; ++b) v.v[b] = vals[4 * g + b];
            *(Vec*)(o + 4 * g) = v;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * g + b < cnt) o[4 * g + b] = vals[4 * g + b];
        }
    }
}
