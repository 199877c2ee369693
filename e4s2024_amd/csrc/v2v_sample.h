// The trilinear sampling arithmetic every face-vid2vid kernel shares (csrc/vid2vid.hip: e4s_v2v_motion_input, e4s_v2v_deform; tools/probes/deform_forms_probe.hip).
#pragma once
#include <hip/hip_runtime.h>

// floor of an unnormalised grid_sample coordinate as an int, held to [-2, size]: at -2 and at size both taps are outside, as they are beyond
__device__ __forceinline__ int v2v_floor_clamped(float v, int size) {
    const float f = fminf(fmaxf(floorf(v), -2.f), (float)size);
    return (int)f;
}

// F.grid_sample's defaults on a 5-D input at the normalised point (mx, my, mz): trilinear, zero padding, align_corners = False (grid_sampler_unnormalize:
// ((coord + 1) size - 1) / 2).  ATen's eight weights in its order, tnw tne tsw tse bnw bne bsw bse (n / s: y0 / y0 + 1, w / e: x0 / x0 + 1, t / b: z0 / z0 + 1), the
// taps' element offsets in a [D][H][W] volume (0 where a tap is outside) and, returned, bit t set where tap t is inside.  The one function every sampling kernel
// calls: the same bits on the same coordinates.
__device__ __forceinline__ unsigned v2v_trilinear_taps(float (&wgt)[8], int (&off)[8], float mx, float my, float mz, int D, int H, int W) {
#pragma clang fp contract(off)
    const float ix = ((mx + 1.f) * (float)W - 1.f) / 2.f, iy = ((my + 1.f) * (float)H - 1.f) / 2.f, iz = ((mz + 1.f) * (float)D - 1.f) / 2.f;
    const int x0 = v2v_floor_clamped(ix, W), y0 = v2v_floor_clamped(iy, H), z0 = v2v_floor_clamped(iz, D);
    const float fx0 = (float)x0, fy0 = (float)y0, fz0 = (float)z0;
    const float fx1 = fx0 + 1.f, fy1 = fy0 + 1.f, fz1 = fz0 + 1.f;
    wgt[0] = (fx1 - ix) * (fy1 - iy) * (fz1 - iz);
    wgt[1] = (ix - fx0) * (fy1 - iy) * (fz1 - iz);
    wgt[2] = (fx1 - ix) * (iy - fy0) * (fz1 - iz);
    wgt[3] = (ix - fx0) * (iy - fy0) * (fz1 - iz);
    wgt[4] = (fx1 - ix) * (fy1 - iy) * (iz - fz0);
    wgt[5] = (ix - fx0) * (fy1 - iy) * (iz - fz0);
    wgt[6] = (fx1 - ix) * (iy - fy0) * (iz - fz0);
    wgt[7] = (ix - fx0) * (iy - fy0) * (iz - fz0);
    unsigned okm = 0u;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int xx = x0 + (t & 1), yy = y0 + ((t >> 1) & 1), zz = z0 + (t >> 2);
        const bool ok = xx >= 0 && xx < W && yy >= 0 && yy < H && zz >= 0 && zz < D;
        okm |= ok ? (1u << t) : 0u;
        off[t] = ok ? (zz * H + yy) * W + xx : 0;
    }
    return okm;
}
