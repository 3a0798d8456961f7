// sdm_ied.h -- the inter-eye distance of one landmark row on the device, shared by the kernels that normalise by it
// (sdm_apply.hip: the update step and the landmark errors) and the tracker's lost rule (sdm_track.hip).
#pragma once
#include "sdm_kernels.h"

__device__ inline double device_ied_rows(const float* __restrict__ xr, int L, const EyeIdxDev& e)
{
    // get_ied, include/rcr/helpers.hpp:136-160 (same arithmetic as sdm_hog.hip::device_ied)
    // (all coordinates requested at once -- clamped index, selected add -- instead of one memory round trip per eye landmark; same sums in the same order)
    float rx = 0.0f, ry = 0.0f, lx = 0.0f, ly = 0.0f;
    float vrx[SDM_MAX_EYE], vry[SDM_MAX_EYE], vlx[SDM_MAX_EYE], vly[SDM_MAX_EYE];
#pragma unroll
    for (int i = 0; i < SDM_MAX_EYE; ++i) {
        const int ir = e.re[i < e.nre ? i : 0], il = e.le[i < e.nle ? i : 0];
        vrx[i] = xr[ir]; vry[i] = xr[ir + L]; vlx[i] = xr[il]; vly[i] = xr[il + L];
    }
#pragma unroll
    for (int i = 0; i < SDM_MAX_EYE; ++i) {
        if (i < e.nre) { rx += vrx[i]; ry += vry[i]; }
        if (i < e.nle) { lx += vlx[i]; ly += vly[i]; }
    }
    rx /= (float)e.nre; ry /= (float)e.nre;
    lx /= (float)e.nle; ly /= (float)e.nle;
    float dxf = rx - lx, dyf = ry - ly;
    double dx = dxf, dy = dyf;
    return sqrt(dx * dx + dy * dy);
}
