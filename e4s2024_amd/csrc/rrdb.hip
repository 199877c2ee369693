// Rows f11 and f16: the glue of the RRDB network the two rows share (e4s2024_amd/ops_rrdb.py) between its convolutions, which run on conv.hip (e4s_conv2d_sb3),
// and the two ends of row f11, the Real-ESRGAN step (swap_face_fine/realesr/image_infer.py: RealESRBatchInfer around RRDBNet(3, 3, 64, 23, 32, scale=4)).  Row
// f16's input and resize are on gpen_sr.hip.  fp32 NCHW, no atomics, no host synchronisation, grids from the shapes alone: the same inputs give the same bits,
// and the calls can be captured in a graph.
//   input     : the head of infer_image and infer_batch in one pass: uint8 [bs][H][W][3] -> clamp((v / 127.5 - 1) * 0.5 + 0.5, 0, 1) -> bilinear (align_corners) to
//               [bs][3][oh][ow].  Every operation is rounded on its own; "/ 127.5" is the device's division by a host scalar, which PyTorch compiles to a
//               product with the float32 reciprocal.  Coordinates and blend are e4s_bilinear_resize's (bilinear_coord, bilinear_blend of common.h).
//   scale_add : y = t * 0.2 + x, the product rounded, then the sum: the residual of an RRDB (an RDB's own goes into conv5's weights and the convolution's
//               residual pointer).  y may be x or t itself: every element is read before it is written, by the same lane.
//   up2       : nearest x2 (F.interpolate(scale_factor=2, mode='nearest'): source index dst >> 1).
//   tail      : conv_last (C -> 3, 3x3, zero pad 1; C a multiple of 8 up to 64) with what follows the network: three output channels would waste nine tenths of
//               conv.hip's 32-output MFMA tile, so this is an exact-float32 VALU kernel.  A workgroup owns a 64 x 16 tile of the image and walks the input
//               channels in chunks of 8; a chunk's tile with its one-pixel halo (zero outside the image) and all C x 9 x 3 weights sit in LDS; a lane owns four
//               neighbouring pixels of a row and their 3 x 4 sums.  Each sum is bias, then C * 9 fused multiply-adds in (input channel, row, column) order; it
//               is written as float32 [bs][3][H][W] when the caller asks for it.  Then the uint8 image, each step rounded on its own:
//                 e4s_esr_tail (infer_batch / infer_image, C = 64): r * 2, - 1, clamp(-1, 1), * 127.5, + 127.5, clamp(0, 255), truncation, [bs][H][W][3];
//                 e4s_gsr_tail (row f16, real_esrnet.py:26-60 RealESRNet.process): clamp(r, 0, 1), * 255.0f, round half to even (numpy's .round()), the crop to
//                 the first Ho x Wo pixels, the optional channel flip back, [bs][Ho][Wo][3].
// Every kernel moves 16 bytes per lane along a row (the tail: 12 bytes of uint8 pixels) where the pointers and the row length allow and single elements
// otherwise, with the same expressions per element in both forms.
#include "common.h"

namespace e4s {

static inline bool esr_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15) == 0;
}

// one colour value of the network's input, every rounding written out
__device__ __forceinline__ float esr_unit(uint8_t v, float inv) {
#pragma clang fp contract(off)
    float a = (float)v * inv;
    a = a - 1.f;
    a = a * 0.5f;
    a = a + 0.5f;
    return fminf(fmaxf(a, 0.f), 1.f);
}

// A group is V consecutive elements of one output row (V = 4: ow % 4 == 0).  n: groups in all.
template <int V>
__global__ __launch_bounds__(256) void esr_input_kernel(float* __restrict__ out, const uint8_t* __restrict__ img, int64_t n, int H, int W, int oh, int ow,
                                                        float sy, float sx, float inv) {
    const int gpr = ow / V;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int64_t row = g / gpr;                                            // (b * 3 + c) * oh + y
        const int x0 = (int)(g - row * gpr) * V;
        const int64_t plane = row / oh;
        const int y = (int)(row - plane * oh);
        const int64_t b = plane / 3;
        const int c = (int)(plane - b * 3);
        int y0, y1;
        float ly;
        bilinear_coord(y, sy, 1, H, y0, y1, ly);
        const uint8_t* r0 = img + ((b * H + y0) * W) * 3 + c;
        const uint8_t* r1 = img + ((b * H + y1) * W) * 3 + c;
        float v[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            int xa, xb;
            float lx;
            bilinear_coord(x0 + j, sx, 1, W, xa, xb, lx);
            v[j] = bilinear_blend(esr_unit(r0[xa * 3], inv), esr_unit(r0[xb * 3], inv), esr_unit(r1[xa * 3], inv), esr_unit(r1[xb * 3], inv), ly, lx);
        }
        float* op = out + row * ow + x0;
        if constexpr (V == 4) *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
        else op[0] = v[0];
    }
}

__device__ __forceinline__ float esr_scale_add(float t, float x) {
#pragma clang fp contract(off)
    const float s = t * 0.2f;
    return s + x;
}

// n: elements (V = 1) or groups of four (V = 4).  No __restrict__: y may alias x or t.
template <int V>
__global__ __launch_bounds__(256) void esr_scale_add_kernel(float* y, const float* t, const float* x, int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        if constexpr (V == 4) {
            const float4 a = reinterpret_cast<const float4*>(t)[e], b = reinterpret_cast<const float4*>(x)[e];
            reinterpret_cast<float4*>(y)[e] = make_float4(esr_scale_add(a.x, b.x), esr_scale_add(a.y, b.y), esr_scale_add(a.z, b.z), esr_scale_add(a.w, b.w));
        } else {
            y[e] = esr_scale_add(t[e], x[e]);
        }
    }
}

// A group is V consecutive INPUT elements of one row (V = 4: w % 4 == 0); it writes 2V elements of two output rows.  n: groups in all.
template <int V>
__global__ __launch_bounds__(256) void esr_up2_kernel(float* __restrict__ out, const float* __restrict__ in, int64_t n, int w) {
    const int gpr = w / V;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int64_t row = g / gpr;                                            // plane * h + y
        const int x0 = (int)(g - row * gpr) * V;
        float* o0 = out + row * 4 * w + 2 * x0;                                 // output row 2y of the same plane: (plane * 2h + 2y) * 2w
        float* o1 = o0 + 2 * w;
        if constexpr (V == 4) {
            const float4 q = *reinterpret_cast<const float4*>(in + row * w + x0);
            const float4 lo = make_float4(q.x, q.x, q.y, q.y), hi = make_float4(q.z, q.z, q.w, q.w);
            reinterpret_cast<float4*>(o0)[0] = lo;
            reinterpret_cast<float4*>(o0)[1] = hi;
            reinterpret_cast<float4*>(o1)[0] = lo;
            reinterpret_cast<float4*>(o1)[1] = hi;
        } else {
            const float q = in[row * w + x0];
            o0[0] = q; o0[1] = q; o1[0] = q; o1[1] = q;
        }
    }
}

constexpr int TAIL_CMAX = 64;                    // conv_last's input channels: a multiple of TAIL_CH up to this
constexpr int TAIL_TW = 64, TAIL_TH = 16;        // the tile of a workgroup: 16 lanes x 4 pixels across, 16 rows
constexpr int TAIL_CH = 8;                       // input channels per LDS chunk
constexpr int TAIL_LW = 72;                      // LDS row: the left halo at column 3, the tile at 4 .. 67 (16-byte aligned), the right halo at 68
constexpr int TAIL_LH = TAIL_TH + 2;
constexpr int TAIL_WROW = 28;                    // 27 weights of an input channel, [row][column][output], padded to seven 16-byte reads

// the output chain of infer_batch and infer_image behind the network, every rounding written out
struct EsrEnd {
    static __device__ __forceinline__ uint8_t to_u8(float r) {
#pragma clang fp contract(off)
        float a = r * 2.f;
        a = a - 1.f;
        a = fminf(fmaxf(a, -1.f), 1.f);
        a = a * 127.5f;
        a = a + 127.5f;
        a = fminf(fmaxf(a, 0.f), 255.f);
        return (uint8_t)a;
    }
};

// the output chain of RealESRNet.process behind the network, every rounding written out
struct GsrEnd {
    static __device__ __forceinline__ uint8_t to_u8(float r) {
#pragma clang fp contract(off)
        float a = fminf(fmaxf(r, 0.f), 1.f);
        a = a * 255.f;
        return (uint8_t)rintf(a);                                               // round half to even
    }
};

// grid (ceil(W / 64), ceil(H / 16), bs).  VEC: W % 4 == 0, x and out_f 16-byte aligned.  pack8: VEC, Wo % 4 == 0 and out_u8 4-byte aligned.
template <bool VEC, class End>
__global__ __launch_bounds__(256) void rrdb_tail_kernel(uint8_t* __restrict__ out_u8, float* __restrict__ out_f, const float* __restrict__ x,
                                                        const float* __restrict__ wgt, const float* __restrict__ bias, int C, int H, int W, int Ho, int Wo,
                                                        int bgr, int pack8) {
    __shared__ __attribute__((aligned(16))) float tile[TAIL_CH * TAIL_LH * TAIL_LW];
    __shared__ __attribute__((aligned(16))) float wl[TAIL_CMAX * TAIL_WROW];
    const int tid = threadIdx.x;
    const int lx = tid & 15, ly = tid >> 4;
    const int tx0 = blockIdx.x * TAIL_TW, ty0 = blockIdx.y * TAIL_TH;
    const int64_t b = blockIdx.z;
    const int64_t hw = (int64_t)H * W;
    const float* xb = x + b * C * hw;

    for (int i = tid; i < C * 27; i += 256) {
        const int ci = i / 27, r = i - ci * 27;
        const int tap = r / 3, o = r - tap * 3;
        wl[ci * TAIL_WROW + r] = wgt[(o * C + ci) * 9 + tap];
    }
    for (int i = tid; i < C; i += 256) wl[i * TAIL_WROW + 27] = 0.f;

    float acc[3][4];
#pragma unroll
    for (int o = 0; o < 3; ++o)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[o][j] = bias[o];

    for (int c0 = 0; c0 < C; c0 += TAIL_CH) {
        __syncthreads();                                                        // the previous chunk has been read (first pass: nothing yet)
        if constexpr (VEC) {
            for (int i = tid; i < TAIL_CH * TAIL_LH * (TAIL_TW / 4); i += 256) {
                const int rr = i / (TAIL_TW / 4), q = i - rr * (TAIL_TW / 4);   // rr = c * LH + r
                const int c = rr / TAIL_LH, r = rr - c * TAIL_LH;
                const int gy = ty0 - 1 + r, gx = tx0 + 4 * q;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gy >= 0 && gy < H && gx < W) v = *reinterpret_cast<const float4*>(xb + (c0 + c) * hw + (int64_t)gy * W + gx);
                *reinterpret_cast<float4*>(tile + rr * TAIL_LW + 4 + 4 * q) = v;
            }
            for (int i = tid; i < TAIL_CH * TAIL_LH * 2; i += 256) {
                const int rr = i >> 1, side = i & 1;
                const int c = rr / TAIL_LH, r = rr - c * TAIL_LH;
                const int gy = ty0 - 1 + r, gx = side ? tx0 + TAIL_TW : tx0 - 1;
                float v = 0.f;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xb[(c0 + c) * hw + (int64_t)gy * W + gx];
                tile[rr * TAIL_LW + (side ? 4 + TAIL_TW : 3)] = v;
            }
        } else {
            for (int i = tid; i < TAIL_CH * TAIL_LH * (TAIL_TW + 2); i += 256) {
                const int rr = i / (TAIL_TW + 2), cx = i - rr * (TAIL_TW + 2);
                const int c = rr / TAIL_LH, r = rr - c * TAIL_LH;
                const int gy = ty0 - 1 + r, gx = tx0 - 1 + cx;
                float v = 0.f;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xb[(c0 + c) * hw + (int64_t)gy * W + gx];
                tile[rr * TAIL_LW + 3 + cx] = v;
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int c = 0; c < TAIL_CH; ++c) {
            float wv[TAIL_WROW];
            const float4* wp = reinterpret_cast<const float4*>(wl + (c0 + c) * TAIL_WROW);     // the same address in every lane
#pragma unroll
            for (int k = 0; k < TAIL_WROW / 4; ++k) {
                const float4 q = wp[k];
                wv[4 * k] = q.x; wv[4 * k + 1] = q.y; wv[4 * k + 2] = q.z; wv[4 * k + 3] = q.w;
            }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const float* rp = tile + (c * TAIL_LH + ly + ky) * TAIL_LW + 4 * lx + 3;
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
        for (int o = 0; o < 3; ++o) u[j * 3 + o] = End::to_u8(bgr ? acc[2 - o][j] : acc[o][j]);
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

// both tails behind their argument checks: the vector form where the row length and the pointers allow, packed uint8 stores where the crop allows too
template <class End>
static int rrdb_tail_launch(const char* what, uint8_t* out_u8, float* out_f, const float* x, const float* weight, const float* bias, int bs, int C, int H, int W,
                            int Ho, int Wo, int bgr, void* stream) {
    const dim3 grid(cdiv(W, TAIL_TW), cdiv(H, TAIL_TH), bs);
    const bool vec = W % 4 == 0 && esr_aligned16(x, out_f);
    const int pack8 = vec && Wo % 4 == 0 && (((uintptr_t)out_u8) & 3) == 0;
    if (vec)
        hipLaunchKernelGGL((rrdb_tail_kernel<true, End>), grid, dim3(256), 0, (hipStream_t)stream, out_u8, out_f, x, weight, bias, C, H, W, Ho, Wo, bgr, pack8);
    else
        hipLaunchKernelGGL((rrdb_tail_kernel<false, End>), grid, dim3(256), 0, (hipStream_t)stream, out_u8, out_f, x, weight, bias, C, H, W, Ho, Wo, bgr, 0);
    return check_launch(what);
}

}  // namespace e4s

using namespace e4s;

extern "C" int e4s_esr_input(float* out, const uint8_t* img, int bs, int H, int W, int oh, int ow, void* stream) {
    E4S_REQUIRE(bs >= 0 && H >= 1 && W >= 1 && oh >= 1 && ow >= 1 && H <= 16384 && W <= 16384 && oh <= 16384 && ow <= 16384, "esr_input: bad size");
    if (bs == 0) return 0;
    E4S_REQUIRE(out && img, "esr_input: null tensor");
    // align_corners=True: (in - 1) / (out - 1) as e4s_bilinear_resize forms it, 0 for a single output
    const float sy = oh > 1 ? (float)(H - 1) / (float)(oh - 1) : 0.f, sx = ow > 1 ? (float)(W - 1) / (float)(ow - 1) : 0.f;
    const float inv = 1.f / 127.5f;
    const int64_t n = (int64_t)bs * 3 * oh * ow;
    if (ow % 4 == 0 && esr_aligned16(out))
        hipLaunchKernelGGL(esr_input_kernel<4>, dim3(grid_1d(n / 4)), dim3(256), 0, (hipStream_t)stream, out, img, n / 4, H, W, oh, ow, sy, sx, inv);
    else
        hipLaunchKernelGGL(esr_input_kernel<1>, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, out, img, n, H, W, oh, ow, sy, sx, inv);
    return check_launch("esr_input");
}

extern "C" int e4s_esr_scale_add(float* y, const float* t, const float* x, int planes, int hw, void* stream) {
    E4S_REQUIRE(planes >= 0 && hw >= 1, "esr_scale_add: bad size");
    if (planes == 0) return 0;
    E4S_REQUIRE(y && t && x, "esr_scale_add: null tensor");
    const int64_t n = (int64_t)planes * hw;
    if (n % 4 == 0 && esr_aligned16(y, t, x))
        hipLaunchKernelGGL(esr_scale_add_kernel<4>, dim3(grid_1d(n / 4)), dim3(256), 0, (hipStream_t)stream, y, t, x, n / 4);
    else
        hipLaunchKernelGGL(esr_scale_add_kernel<1>, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, y, t, x, n);
    return check_launch("esr_scale_add");
}

extern "C" int e4s_esr_up2(float* out, const float* in, int planes, int h, int w, void* stream) {
    E4S_REQUIRE(planes >= 0 && h >= 1 && w >= 1 && h <= 16384 && w <= 16384, "esr_up2: bad size");
    if (planes == 0) return 0;
    E4S_REQUIRE(out && in, "esr_up2: null tensor");
    const int64_t n = (int64_t)planes * h * w;
    if (w % 4 == 0 && esr_aligned16(out, in))
        hipLaunchKernelGGL(esr_up2_kernel<4>, dim3(grid_1d(n / 4)), dim3(256), 0, (hipStream_t)stream, out, in, n / 4, w);
    else
        hipLaunchKernelGGL(esr_up2_kernel<1>, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, out, in, n, w);
    return check_launch("esr_up2");
}

extern "C" int e4s_esr_tail(uint8_t* out_u8, float* out_f, const float* x, const float* weight, const float* bias, int bs, int H, int W, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "esr_tail: bad size");
    if (bs == 0) return 0;
    E4S_REQUIRE(out_u8 && x && weight && bias, "esr_tail: null tensor");
    return rrdb_tail_launch<EsrEnd>("esr_tail", out_u8, out_f, x, weight, bias, bs, TAIL_CMAX, H, W, H, W, 0, stream);
}

extern "C" int e4s_gsr_tail(uint8_t* out_u8, float* out_f, const float* x, const float* weight, const float* bias, int bs, int C, int H, int W, int Ho, int Wo,
                            int bgr, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "gsr_tail: bad size");
    E4S_REQUIRE(C >= TAIL_CH && C <= TAIL_CMAX && C % TAIL_CH == 0, "gsr_tail: C is a multiple of %d up to %d, got %d", TAIL_CH, TAIL_CMAX, C);
    E4S_REQUIRE(Ho >= 1 && Ho <= H && Wo >= 1 && Wo <= W, "gsr_tail: the crop %d x %d does not lie in %d x %d", Ho, Wo, H, W);
    if (bs == 0) return 0;
    E4S_REQUIRE(out_u8 && x && weight && bias, "gsr_tail: null tensor");
    return rrdb_tail_launch<GsrEnd>("gsr_tail", out_u8, out_f, x, weight, bias, bs, C, H, W, Ho, Wo, bgr ? 1 : 0, stream);
}
