// Row f16: GPEN face enhancement, stage 5 — the input of the RealESRNet pass (swap_face_fine/gpen/sr_model/real_esrnet.py:26-60 RealESRNet.process around
// rrdbnet_arch.py:64-116 RRDBNet) and the resize of the frame to the super-resolved size (face_enhancement.py:66).  The network's convolutions run on conv.hip
// (e4s_conv2d_sb3); its glue and the tail of process (e4s_gsr_tail) are on rrdb.hip, shared with row f11.  No atomics, no host synchronisation, grids from the
// shapes alone: the same inputs give the same bits, and the calls can be captured in a graph.
//   input  : the head of process and pixel_unshuffle (arch_util.py:109-125) in one pass: uint8 [bs][H][W][3] -> v / 255 (a correctly rounded float32 division, as
//            numpy divides; this build has no fast-math flag), the optional channel flip, the reflect pad of ph = (-H) mod r rows and pw = (-W) mod r columns at
//            the bottom / right (index n + i is n - 2 - i, F.pad(..., 'reflect'): no edge repeat) and the unshuffle by r to [bs][3 r r][(H + ph) / r][(W + pw) / r],
//            channel c r r + dy r + dx.  r = 1 (scale 4): no pad, no unshuffle.  It moves 16 bytes per lane along a row where the pointer and the row length
//            allow and single elements otherwise, with the same expressions per element in both forms.
//   resize : cv2.resize(uint8 [H][W][3], (Wo, Ho)) at its default INTER_LINEAR in OpenCV's portable fixed-point arithmetic: per axis scale = src / dst in double,
//            f = float((d + 0.5) scale - 0.5), s = floor(f), f -= s; s < 0: s = 0, f = 0; s >= src - 1: s = src - 1, f = 0; coefficients short(rint((1 - f) 2048))
//            and short(rint(f 2048)) with 1 - f in float32; rows first in int32, S[s] a0 + S[s + 1] a1, then
//            (((b0 (r0 >> 4)) >> 16) + ((b1 (r1 >> 4)) >> 16) + 2) >> 2.  The exact 2 : 1 downscale, which OpenCV routes to INTER_AREA, is refused.
//            cv2 is installed nowhere this project is built or tested, so nobody has run this against OpenCV: the numpy restatement in tests/gpen_sr_model.py,
//            written from OpenCV's algorithm, is the pin (as row f15's warpAffine is pinned by tests/gpen_paste_model.py).  A gather of bytes, one output pixel
//            per lane.
#include "common.h"

namespace e4s {

// A group is V consecutive elements of one output row (V = 4: ow % 4 == 0, out 16-byte aligned).  n: groups in all.
template <int V>
__global__ __launch_bounds__(256) void gsr_input_kernel(float* __restrict__ out, const uint8_t* __restrict__ img, int64_t n, int H, int W, int r, int oh, int ow,
                                                        int bgr) {
    const int gpr = ow / V;
    const int rr = r * r;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int64_t row = g / gpr;                                            // (b * 3 r r + ch) * oh + y
        const int x0 = (int)(g - row * gpr) * V;
        const int64_t plane = row / oh;
        const int y = (int)(row - plane * oh);
        const int64_t b = plane / (3 * rr);
        const int ch = (int)(plane - b * 3 * rr);
        const int c = ch / rr, d = ch - c * rr;
        const int dy = d / r, dx = d - dy * r;
        int sy = y * r + dy;
        if (sy >= H) sy = 2 * H - 2 - sy;                                       // reflect: H > ph, so 0 <= sy
        const uint8_t* rp = img + ((b * H + sy) * W) * 3 + (bgr ? 2 - c : c);
        float v[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            int sx = (x0 + j) * r + dx;
            if (sx >= W) sx = 2 * W - 2 - sx;
            v[j] = (float)rp[(int64_t)sx * 3] / 255.f;
        }
        float* op = out + row * ow + x0;
        if constexpr (V == 4) *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
        else op[0] = v[0];
    }
}

// cv2.resize's coordinate along one axis: the source index and the two 11-bit coefficients
__device__ __forceinline__ void cvr_coord(int d, double scale, int src, int& s, int& a0, int& a1) {
#pragma clang fp contract(off)
    const double t = ((double)d + 0.5) * scale;
    float f = (float)(t - 0.5);
    s = (int)floorf(f);
    f = f - (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= src - 1) { s = src - 1; f = 0.f; }
    const float g = 1.f - f;
    a0 = (int)rintf(g * 2048.f);
    a1 = (int)rintf(f * 2048.f);
}

// one lane per output pixel (three bytes); n = bs * Ho * Wo
__global__ __launch_bounds__(256) void cv_resize_linear_u8_kernel(uint8_t* __restrict__ out, const uint8_t* __restrict__ img, int64_t n, int H, int W, int Ho,
                                                                  int Wo, double sy, double sx) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t row = e / Wo;                                             // b * Ho + y
        const int x = (int)(e - row * Wo);
        const int64_t b = row / Ho;
        const int y = (int)(row - b * Ho);
        int y0, b0, b1, x0, a0, a1;
        cvr_coord(y, sy, H, y0, b0, b1);
        cvr_coord(x, sx, W, x0, a0, a1);
        const int y1 = y0 + 1 < H ? y0 + 1 : H - 1, x1 = x0 + 1 < W ? x0 + 1 : W - 1;       // (their coefficient is 0 where they are clamped)
        const uint8_t* r0 = img + (b * H + y0) * (int64_t)W * 3;
        const uint8_t* r1 = img + (b * H + y1) * (int64_t)W * 3;
        uint8_t* op = out + e * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int h0 = (int)r0[x0 * 3 + c] * a0 + (int)r0[x1 * 3 + c] * a1;
            const int h1 = (int)r1[x0 * 3 + c] * a0 + (int)r1[x1 * 3 + c] * a1;
            op[c] = (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
        }
    }
}

}  // namespace e4s

using namespace e4s;

extern "C" int e4s_gsr_input(float* out, const uint8_t* img, int bs, int H, int W, int r, int bgr, void* stream) {
    E4S_REQUIRE(bs >= 0 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "gsr_input: bad size");
    E4S_REQUIRE(r == 1 || r == 2 || r == 4, "gsr_input: r is 1, 2 or 4, got %d", r);
    const int ph = (r - H % r) % r, pw = (r - W % r) % r;
    E4S_REQUIRE(H > ph && W > pw, "gsr_input: a %d x %d image cannot be reflect-padded by %d x %d", H, W, ph, pw);
    if (bs == 0) return 0;
    E4S_REQUIRE(out && img, "gsr_input: null tensor");
    const int oh = (H + ph) / r, ow = (W + pw) / r;
    const int64_t n = (int64_t)bs * 3 * r * r * oh * ow;
    if (ow % 4 == 0 && (((uintptr_t)out) & 15) == 0)
        hipLaunchKernelGGL(gsr_input_kernel<4>, dim3(grid_1d(n / 4)), dim3(256), 0, (hipStream_t)stream, out, img, n / 4, H, W, r, oh, ow, bgr ? 1 : 0);
    else
        hipLaunchKernelGGL(gsr_input_kernel<1>, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, out, img, n, H, W, r, oh, ow, bgr ? 1 : 0);
    return check_launch("gsr_input");
}

extern "C" int e4s_cv_resize_linear_u8(uint8_t* out, const uint8_t* img, int bs, int H, int W, int Ho, int Wo, void* stream) {
    E4S_REQUIRE(bs >= 0 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1 && H <= 16384 && W <= 16384 && Ho <= 16384 && Wo <= 16384, "cv_resize_linear_u8: bad size");
    E4S_REQUIRE(!(H == 2 * Ho && W == 2 * Wo), "cv_resize_linear_u8: the exact 2 : 1 downscale is cv2's INTER_AREA, which is not offered");
    if (bs == 0) return 0;
    E4S_REQUIRE(out && img, "cv_resize_linear_u8: null tensor");
    const int64_t n = (int64_t)bs * Ho * Wo;
    hipLaunchKernelGGL(cv_resize_linear_u8_kernel, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, out, img, n, H, W, Ho, Wo, (double)H / (double)Ho,
                       (double)W / (double)Wo);
    return check_launch("cv_resize_linear_u8");
}
