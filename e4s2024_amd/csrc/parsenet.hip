// Row f13: what GPEN's ParseNet (swap_face_fine/gpen/face_parse/parse_model.py: ParseNet; blocks.py: ConvLayer, ResidualBlock; face_parsing.py: FaceParse.img2tensor)
// needs around its 3 x 3 convolutions, which run on conv.hip (e4s_conv2d_sb3).  conv.hip pads with zeros only; every ConvLayer pads by reflection and the decoder's
// put a nearest x 2 in front, so the convolutions read planes that the pad kernel here wrote, with pad = 0.  fp32 NCHW, no atomics, no host synchronisation, grids
// from the shapes alone: the same inputs give the same bits.
//   stem : encoder.0 = ConvLayer(3, C0, 3): reflection pad 1, 3 x 3, bias, no norm, no activation.  Three input channels would leave 29/32 of an MFMA tile on
//          zeros, so this is an exact-float32 VALU kernel: each output is bias[co], then 27 fused multiply-adds in (input channel, row, column) order.  The
//          reflection is index arithmetic (index -1 is 1, index n is n - 2).  A lane owns V consecutive pixels of a row, keeps their 3 x 3 x (V + 2) inputs in
//          registers and walks 16 output channels whose weights are the same in every lane.  The input is float [bs][3][H][W], or uint8 [bs][H][W][3] taken
//          through FaceParse.img2tensor first: the channel flip when the image is BGR, and v / 255. * 2 - 1 in float64 rounded once to float32, which the host
//          hands over as a 256-entry table.
//   pad  : out [planes][u h + 2][u w + 2] = reflection pad 1 of the nearest x u (u = 1, 2) of v = x + add (one rounding; add may be NULL).  A lane owns output
//          cells, not inputs: every cell is the sum of the one source element its index arithmetic names, so a border cell holds the bits of the interior cell
//          it mirrors.  The padded rows start two floats further on each row, so no row of out is 16-byte aligned as a rule; the 16-byte stores therefore run
//          over the flat output, four consecutive cells per lane (a group may continue on the next row), and the last cells of an output that is no multiple
//          of four, or every cell when out is not aligned, go one at a time: the same expression per cell.
#include "common.h"

namespace e4s {

constexpr int PN_CPB = 16;                       // output channels of the stem per workgroup row (blockIdx.y)

static inline bool pn_aligned16(const void* a, const void* b = nullptr) { return ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0; }

// ReflectionPad2d(1): index -1 is 1, index n is n - 2 (n >= 2; with n == 2 the two sides read 1 and 0)
__device__ __forceinline__ int pn_reflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// A group is V consecutive pixels of one row (V = 4: W % 4 == 0).  n: groups in all.  blockIdx.y picks PN_CPB output channels.  weight [C0][3][3][3].
template <int V, bool U8>
__global__ __launch_bounds__(256) void parsenet_stem_kernel(float* __restrict__ out, const float* __restrict__ xf, const uint8_t* __restrict__ xu,
                                                            const float* __restrict__ lut, int bgr, const float* __restrict__ weight,
                                                            const float* __restrict__ bias, int64_t n, int H, int W, int C0) {
    const int c_lo = blockIdx.y * PN_CPB;
    const int c_hi = c_lo + PN_CPB < C0 ? c_lo + PN_CPB : C0;
    const int gpr = W / V;                                                      // groups per row
    const int64_t hw = (int64_t)H * W;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int64_t row = g / gpr;                                            // b * H + y
        const int x0 = (int)(g - row * gpr) * V;
        const int64_t b = row / H;
        const int y = (int)(row - b * H);
        const int xl = pn_reflect1(x0 - 1, W), xr = pn_reflect1(x0 + V, W);
        float in[3][3][V + 2];                                                  // [channel][row][column x0 - 1 .. x0 + V]
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int r = pn_reflect1(y + ky - 1, H);
            if constexpr (U8) {
                const uint8_t* src = xu + (b * H + r) * (int64_t)W * 3;
                uint8_t px[V + 2][3];
#pragma unroll
                for (int c = 0; c < 3; ++c) { px[0][c] = src[xl * 3 + c]; px[V + 1][c] = src[xr * 3 + c]; }
                if constexpr (V == 4) {
                    const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src + x0 * 3);      // 12 bytes: the host checked the alignment
                    const uint32_t q[3] = {s32[0], s32[1], s32[2]};
#pragma unroll
                    for (int e = 0; e < 12; ++e) px[1 + e / 3][e % 3] = (uint8_t)(q[e >> 2] >> (8 * (e & 3)));
                } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c) px[1][c] = src[x0 * 3 + c];
                }
#pragma unroll
                for (int j = 0; j < V + 2; ++j)
#pragma unroll
                    for (int c = 0; c < 3; ++c) in[c][ky][j] = lut[px[j][bgr ? 2 - c : c]];
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float* src = xf + (b * 3 + c) * hw + (int64_t)r * W;
                    in[c][ky][0] = src[xl];
                    in[c][ky][V + 1] = src[xr];
                    if constexpr (V == 4) {
                        const float4 q = *reinterpret_cast<const float4*>(src + x0);
                        in[c][ky][1] = q.x; in[c][ky][2] = q.y; in[c][ky][3] = q.z; in[c][ky][4] = q.w;
                    } else {
                        in[c][ky][1] = src[x0];
                    }
                }
            }
        }
        for (int co = c_lo; co < c_hi; ++co) {
            const float* wr = weight + (size_t)co * 27;                         // the same address in every lane
            float acc[V];
            const float bi = bias[co];
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = bi;
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {                            // input channel, then row, then column: one definite order
                        const float wv = wr[(c * 3 + ky) * 3 + kx];
#pragma unroll
                        for (int j = 0; j < V; ++j) acc[j] = __builtin_fmaf(wv, in[c][ky][j + kx], acc[j]);
                    }
            float* op = out + (b * C0 + co) * hw + (int64_t)y * W + x0;
            if constexpr (V == 4) *reinterpret_cast<float4*>(op) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            else op[0] = acc[0];
        }
    }
}

// A group is V consecutive cells of the flat output [planes][hp][wp].  n: groups in all; total: cells in all.  sh = 0 (u = 1) or 1 (u = 2); H = u h, W = u w.
template <int V>
__global__ __launch_bounds__(256) void parsenet_pad_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ add, int64_t n,
                                                           int64_t total, int h, int w, int sh) {
    const int H = h << sh, W = w << sh, hp = H + 2, wp = W + 2;
    const int pp = hp * wp;
    const int64_t hw = (int64_t)h * w;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int64_t i0 = g * V;
        int64_t plane = i0 / pp;
        const int rem = (int)(i0 - plane * pp);
        int Y = rem / wp, X = rem - Y * wp;
        float v[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            v[j] = 0.f;
            if (i0 + j < total) {
                const int sy = pn_reflect1(Y - 1, H) >> sh, sx = pn_reflect1(X - 1, W) >> sh;
                const int64_t idx = plane * hw + (int64_t)sy * w + sx;
                v[j] = add ? x[idx] + add[idx] : x[idx];
            }
            if (++X == wp) {
                X = 0;
                if (++Y == hp) { Y = 0; ++plane; }
            }
        }
        if constexpr (V == 4) {
            if (i0 + 4 <= total) {
                *reinterpret_cast<float4*>(out + i0) = make_float4(v[0], v[1], v[2], v[3]);
                continue;
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (i0 + j < total) out[i0 + j] = v[j];
    }
}

}  // namespace e4s

using namespace e4s;

extern "C" int e4s_parsenet_stem(float* out, const float* x, const uint8_t* x_u8, const float* lut, int bgr, const float* weight, const float* bias, int bs,
                                 int C0, int H, int W, void* stream) {
    E4S_REQUIRE(bs >= 0 && C0 >= 1 && C0 <= 65535 * PN_CPB, "parsenet_stem: bad batch or channel count");
    E4S_REQUIRE(H >= 2 && W >= 2 && H <= 16384 && W <= 16384, "parsenet_stem: a %d x %d image: reflection padding needs at least 2 x 2 (at most 16384 x 16384)", H, W);
    E4S_REQUIRE(bgr == 0 || bgr == 1, "parsenet_stem: bgr is 0 or 1");
    if (bs == 0) return 0;
    E4S_REQUIRE(out && weight && bias && ((x != nullptr) != (x_u8 != nullptr)), "parsenet_stem: null tensor, or not exactly one of the float and the uint8 input");
    E4S_REQUIRE(x || lut, "parsenet_stem: the uint8 input needs the 256-entry table");
    const int64_t n = (int64_t)bs * H * W;
    const int gy = cdiv(C0, PN_CPB);
    hipStream_t st = (hipStream_t)stream;
    if (x) {
        if (W % 4 == 0 && pn_aligned16(out, x))
            hipLaunchKernelGGL((parsenet_stem_kernel<4, false>), dim3(grid_1d(n / 4), gy), dim3(256), 0, st, out, x, x_u8, lut, bgr, weight, bias, n / 4, H, W, C0);
        else
            hipLaunchKernelGGL((parsenet_stem_kernel<1, false>), dim3(grid_1d(n), gy), dim3(256), 0, st, out, x, x_u8, lut, bgr, weight, bias, n, H, W, C0);
    } else {
        if (W % 4 == 0 && pn_aligned16(out) && (((uintptr_t)x_u8) & 3) == 0)
            hipLaunchKernelGGL((parsenet_stem_kernel<4, true>), dim3(grid_1d(n / 4), gy), dim3(256), 0, st, out, x, x_u8, lut, bgr, weight, bias, n / 4, H, W, C0);
        else
            hipLaunchKernelGGL((parsenet_stem_kernel<1, true>), dim3(grid_1d(n), gy), dim3(256), 0, st, out, x, x_u8, lut, bgr, weight, bias, n, H, W, C0);
    }
    return check_launch("parsenet_stem");
}

extern "C" int e4s_parsenet_pad(float* out, const float* x, const float* add, int planes, int h, int w, int u, void* stream) {
    E4S_REQUIRE(planes >= 0 && (u == 1 || u == 2), "parsenet_pad: planes >= 0 and u is 1 or 2");
    E4S_REQUIRE(h >= 1 && w >= 1 && h <= 8192 && w <= 8192 && u * h >= 2 && u * w >= 2,
                "parsenet_pad: a %d x %d map at u = %d: reflection padding needs at least 2 x 2 after the upsampling (at most 8192 x 8192 before)", h, w, u);
    if (planes == 0) return 0;
    E4S_REQUIRE(out && x, "parsenet_pad: null tensor");
    const int64_t total = (int64_t)planes * (u * h + 2) * (u * w + 2);
    hipStream_t st = (hipStream_t)stream;
    if (pn_aligned16(out)) {
        const int64_t n = cdiv64(total, 4);
        hipLaunchKernelGGL(parsenet_pad_kernel<4>, dim3(grid_1d(n)), dim3(256), 0, st, out, x, add, n, total, h, w, u - 1);
    } else {
        hipLaunchKernelGGL(parsenet_pad_kernel<1>, dim3(grid_1d(total)), dim3(256), 0, st, out, x, add, total, total, h, w, u - 1);
    }
    return check_launch("parsenet_pad");
}
