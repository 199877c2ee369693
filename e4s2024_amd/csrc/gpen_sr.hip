// Row f16: GPEN face enhancement, stage 5 — the ends of the RealESRNet pass (swap_face_fine/gpen/sr_model/real_esrnet.py:26-60 RealESRNet.process around
// rrdbnet_arch.py:64-116 RRDBNet) and the resize of the frame to the super-resolved size (face_enhancement.py:66).  The network's convolutions run on conv.hip
// (e4s_conv2d_sb3), its glue on rrdb.hip (e4s_esr_scale_add, e4s_esr_up2).  No atomics, no host synchronisation, grids from the shapes alone: the same inputs
// give the same bits, and the calls can be captured in a graph.
//   input  : the head of process and pixel_unshuffle (arch_util.py:109-125) in one pass: uint8 [bs][H][W][3] -> v / 255 (a correctly rounded float32 division, as
//            numpy divides; this build has no fast-math flag), the optional channel flip, the reflect pad of ph = (-H) mod r rows and pw = (-W) mod r columns at
//            the bottom / right (index n + i is n - 2 - i, F.pad(..., 'reflect'): no edge repeat) and the unshuffle by r to [bs][3 r r][(H + ph) / r][(W + pw) / r],
//            channel c r r + dy r + dx.  r = 1 (scale 4): no pad, no unshuffle.
//   tail   : conv_last (C -> 3, 3x3, zero pad 1) in exact float32 as e4s_esr_tail does it (a 64 x 16 tile per workgroup, chunks of 8 input channels with their
//            halo in LDS, a lane owns four neighbouring pixels; each sum is bias, then C * 9 fused multiply-adds in (input channel, row, column) order), with C a
//            parameter.  Then the tail of process: clamp(r, 0, 1), * 255.0f rounded on its own, round half to even (numpy's .round()), the crop to the first
//            Ho x Wo pixels, the optional flip back, uint8 [bs][Ho][Wo][3]; r itself, uncropped, as float32 [bs][3][H][W] when the caller asks for it.
//   resize : cv2.resize(uint8 [H][W][3], (Wo, Ho)) at its default INTER_LINEAR in OpenCV's portable fixed-point arithmetic: per axis scale = src / dst in double,
//            f = float((d + 0.5) scale - 0.5), s = floor(f), f -= s; s < 0: s = 0, f = 0; s >= src - 1: s = src - 1, f = 0; coefficients short(rint((1 - f) 2048))
//            and short(rint(f 2048)) with 1 - f in float32; rows first in int32, S[s] a0 + S[s + 1] a1, then
//            (((b0 (r0 >> 4)) >> 16) + ((b1 (r1 >> 4)) >> 16) + 2) >> 2.  The exact 2 : 1 downscale, which OpenCV routes to INTER_AREA, is refused.
//            cv2 is installed nowhere this project is built or tested, so nobody has run this against OpenCV: the numpy restatement in tests/gpen_sr_model.py,
//            written from OpenCV's algorithm, is the pin (as row f15's warpAffine is pinned by tests/gpen_paste_model.py).
// input and tail move 16 bytes per lane along a row (12 bytes of uint8 pixels) where the pointers and the row length allow and single elements otherwise, with
// the same expressions per element in both forms; the resize is a gather of bytes, one output pixel per lane.
#include "common.h"

namespace e4s {

static inline int gsr_grid(int64_t n) {
    const int64_t b = cdiv64(n, 256);
    return (int)(b < 1 ? 1 : (b < 16384 ? b : 16384));
}

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

constexpr int GSR_CMAX = 64;                     // conv_last's input channels: a multiple of GSR_CH up to this
constexpr int GSR_TW = 64, GSR_TH = 16;          // the tile of a workgroup: 16 lanes x 4 pixels across, 16 rows
constexpr int GSR_CH = 8;                        // input channels per LDS chunk
constexpr int GSR_LW = 72;                       // LDS row: the left halo at column 3, the tile at 4 .. 67 (16-byte aligned), the right halo at 68
constexpr int GSR_LH = GSR_TH + 2;
constexpr int GSR_WROW = 28;                     // 27 weights of an input channel, [row][column][output], padded to seven 16-byte reads

// the output chain of RealESRNet.process behind the network, every rounding written out
__device__ __forceinline__ uint8_t gsr_to_u8(float r) {
#pragma clang fp contract(off)
    float a = fminf(fmaxf(r, 0.f), 1.f);
    a = a * 255.f;
    return (uint8_t)rintf(a);                                                   // round half to even
}

// grid (ceil(W / 64), ceil(H / 16), bs).  VEC: W % 4 == 0, x and out_f 16-byte aligned.  pack8: VEC, Wo % 4 == 0 and out_u8 4-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void gsr_tail_kernel(uint8_t* __restrict__ out_u8, float* __restrict__ out_f, const float* __restrict__ x,
                                                       const float* __restrict__ wgt, const float* __restrict__ bias, int C, int H, int W, int Ho, int Wo, int bgr,
                                                       int pack8) {
    __shared__ __attribute__((aligned(16))) float tile[GSR_CH * GSR_LH * GSR_LW];
    __shared__ __attribute__((aligned(16))) float wl[GSR_CMAX * GSR_WROW];
    const int tid = threadIdx.x;
    const int lx = tid & 15, ly = tid >> 4;
    const int tx0 = blockIdx.x * GSR_TW, ty0 = blockIdx.y * GSR_TH;
    const int64_t b = blockIdx.z;
    const int64_t hw = (int64_t)H * W;
    const float* xb = x + b * C * hw;

    for (int i = tid; i < C * 27; i += 256) {
        const int ci = i / 27, r = i - ci * 27;
        const int tap = r / 3, o = r - tap * 3;
        wl[ci * GSR_WROW + r] = wgt[(o * C + ci) * 9 + tap];
    }
    for (int i = tid; i < C; i += 256) wl[i * GSR_WROW + 27] = 0.f;

    float acc[3][4];
#pragma unroll
    for (int o = 0; o < 3; ++o)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[o][j] = bias[o];

    for (int c0 = 0; c0 < C; c0 += GSR_CH) {
        __syncthreads();                                                        // the previous chunk has been read (first pass: nothing yet)
        if constexpr (VEC) {
            for (int i = tid; i < GSR_CH * GSR_LH * (GSR_TW / 4); i += 256) {
                const int rr = i / (GSR_TW / 4), q = i - rr * (GSR_TW / 4);     // rr = c * LH + r
                const int c = rr / GSR_LH, r = rr - c * GSR_LH;
                const int gy = ty0 - 1 + r, gx = tx0 + 4 * q;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gy >= 0 && gy < H && gx < W) v = *reinterpret_cast<const float4*>(xb + (c0 + c) * hw + (int64_t)gy * W + gx);
                *reinterpret_cast<float4*>(tile + rr * GSR_LW + 4 + 4 * q) = v;
            }
            for (int i = tid; i < GSR_CH * GSR_LH * 2; i += 256) {
                const int rr = i >> 1, side = i & 1;
                const int c = rr / GSR_LH, r = rr - c * GSR_LH;
                const int gy = ty0 - 1 + r, gx = side ? tx0 + GSR_TW : tx0 - 1;
                float v = 0.f;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xb[(c0 + c) * hw + (int64_t)gy * W + gx];
                tile[rr * GSR_LW + (side ? 4 + GSR_TW : 3)] = v;
            }
        } else {
            for (int i = tid; i < GSR_CH * GSR_LH * (GSR_TW + 2); i += 256) {
                const int rr = i / (GSR_TW + 2), cx = i - rr * (GSR_TW + 2);
                const int c = rr / GSR_LH, r = rr - c * GSR_LH;
                const int gy = ty0 - 1 + r, gx = tx0 - 1 + cx;
                float v = 0.f;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xb[(c0 + c) * hw + (int64_t)gy * W + gx];
                tile[rr * GSR_LW + 3 + cx] = v;
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int c = 0; c < GSR_CH; ++c) {
            float wv[GSR_WROW];
            const float4* wp = reinterpret_cast<const float4*>(wl + (c0 + c) * GSR_WROW);      // the same address in every lane
#pragma unroll
            for (int k = 0; k < GSR_WROW / 4; ++k) {
                const float4 q = wp[k];
                wv[4 * k] = q.x; wv[4 * k + 1] = q.y; wv[4 * k + 2] = q.z; wv[4 * k + 3] = q.w;
            }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const float* rp = tile + (c * GSR_LH + ly + ky) * GSR_LW + 4 * lx + 3;
                const float4 mid = *reinterpret_cast<const float4*>(rp + 1);
                const float v[6] = {rp[0], mid.x, mid.y, mid.z, mid.w, rp[5]};
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int o = 0; o < 3; ++o)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[o][j] = fmaf(wv[(ky * 3 + kx) * 3 + o], v[j + kx], acc[o][j]);
            }
        }
    }

    const int y = ty0 + ly, x0 = tx0 + 4 * lx;
    if (y >= H || x0 >= W) return;
    const int64_t pix = (int64_t)y * W + x0;
    if (out_f) {
        if constexpr (VEC) {
#pragma unroll
            for (int o = 0; o < 3; ++o) *reinterpret_cast<float4*>(out_f + (b * 3 + o) * hw + pix) = make_float4(acc[o][0], acc[o][1], acc[o][2], acc[o][3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (x0 + j >= W) break;
#pragma unroll
                for (int o = 0; o < 3; ++o) out_f[(b * 3 + o) * hw + pix + j] = acc[o][j];
            }
        }
    }
    if (y >= Ho || x0 >= Wo) return;                                            // the crop
    uint8_t u[12];                                                              // [pixel][byte of the output order]
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int o = 0; o < 3; ++o) u[j * 3 + o] = gsr_to_u8(bgr ? acc[2 - o][j] : acc[o][j]);
    uint8_t* up8 = out_u8 + ((b * Ho + y) * (int64_t)Wo + x0) * 3;
    if (pack8) {                                                                // Wo % 4 == 0: the four pixels lie inside the crop together
        uint32_t* up = reinterpret_cast<uint32_t*>(up8);
#pragma unroll
        for (int k = 0; k < 3; ++k) up[k] = (uint32_t)u[4 * k] | ((uint32_t)u[4 * k + 1] << 8) | ((uint32_t)u[4 * k + 2] << 16) | ((uint32_t)u[4 * k + 3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x0 + j >= Wo) break;
#pragma unroll
            for (int o = 0; o < 3; ++o) up8[j * 3 + o] = u[j * 3 + o];
        }
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
        hipLaunchKernelGGL(gsr_input_kernel<4>, dim3(gsr_grid(n / 4)), dim3(256), 0, (hipStream_t)stream, out, img, n / 4, H, W, r, oh, ow, bgr ? 1 : 0);
    else
        hipLaunchKernelGGL(gsr_input_kernel<1>, dim3(gsr_grid(n)), dim3(256), 0, (hipStream_t)stream, out, img, n, H, W, r, oh, ow, bgr ? 1 : 0);
    return check_launch("gsr_input");
}

extern "C" int e4s_gsr_tail(uint8_t* out_u8, float* out_f, const float* x, const float* weight, const float* bias, int bs, int C, int H, int W, int Ho, int Wo,
                            int bgr, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "gsr_tail: bad size");
    E4S_REQUIRE(C >= GSR_CH && C <= GSR_CMAX && C % GSR_CH == 0, "gsr_tail: C is a multiple of %d up to %d, got %d", GSR_CH, GSR_CMAX, C);
    E4S_REQUIRE(Ho >= 1 && Ho <= H && Wo >= 1 && Wo <= W, "gsr_tail: the crop %d x %d does not lie in %d x %d", Ho, Wo, H, W);
    if (bs == 0) return 0;
    E4S_REQUIRE(out_u8 && x && weight && bias, "gsr_tail: null tensor");
    const dim3 grid(cdiv(W, GSR_TW), cdiv(H, GSR_TH), bs);
    const bool vec = W % 4 == 0 && ((((uintptr_t)x) | ((uintptr_t)out_f)) & 15) == 0;
    const int pack8 = vec && Wo % 4 == 0 && (((uintptr_t)out_u8) & 3) == 0;
    if (vec)
        hipLaunchKernelGGL(gsr_tail_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, out_u8, out_f, x, weight, bias, C, H, W, Ho, Wo, bgr ? 1 : 0, pack8);
    else
        hipLaunchKernelGGL(gsr_tail_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, out_u8, out_f, x, weight, bias, C, H, W, Ho, Wo, bgr ? 1 : 0, 0);
    return check_launch("gsr_tail");
}

extern "C" int e4s_cv_resize_linear_u8(uint8_t* out, const uint8_t* img, int bs, int H, int W, int Ho, int Wo, void* stream) {
    E4S_REQUIRE(bs >= 0 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1 && H <= 16384 && W <= 16384 && Ho <= 16384 && Wo <= 16384, "cv_resize_linear_u8: bad size");
    E4S_REQUIRE(!(H == 2 * Ho && W == 2 * Wo), "cv_resize_linear_u8: the exact 2 : 1 downscale is cv2's INTER_AREA, which is not offered");
    if (bs == 0) return 0;
    E4S_REQUIRE(out && img, "cv_resize_linear_u8: null tensor");
    const int64_t n = (int64_t)bs * Ho * Wo;
    hipLaunchKernelGGL(cv_resize_linear_u8_kernel, dim3(gsr_grid(n)), dim3(256), 0, (hipStream_t)stream, out, img, n, H, W, Ho, Wo, (double)H / (double)Ho,
                       (double)W / (double)Wo);
    return check_launch("cv_resize_linear_u8");
}
