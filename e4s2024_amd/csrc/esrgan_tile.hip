// Row f23: CodeFormer face restoration, stage 3 — the tile ends of RealESRGANer.enhance (swap_face_fine/realesrgan_utils.py:69-172 pre_process, tile_process,
// post_process around RRDBNet x4plus, half=False) and its cv2.resize(..., INTER_LANCZOS4) on uint8 (:243-248).  The network's convolutions run on conv.hip
// (e4s_conv2d_sb3) and its glue on rrdb.hip, as rows f11 and f16 run them.  No atomics, no host synchronisation, grids from the shapes alone: the same inputs give
// the same bits, and the calls can be captured in a graph.
//   input  : one tile window of a uint8 image as the network's float32 input: v / 255 (a correctly rounded float32 division, as numpy divides; this build has no
//            fast-math flag).  The window is in coordinates of the pre-padded image, which is never formed: a row or column at or beyond H / W reads the source
//            by F.pad(..., 'reflect') (index n + i is n - 2 - i).  HWC or planar source, channel order kept.
//   tail   : conv_last on the kept window of a tile's x4 output alone, in the arithmetic of rrdb.hip's tail (bias, then C * 9 fused multiply-adds in (input channel,
//            row, column) order; a workgroup owns 64 x 16 pixels of the WINDOW, a lane four neighbours of a row), then clamp(0, 1), * 255.0f, round half to even, and
//            the bytes stored at the window's place in the whole x4 canvas.  A lane whose four pixels lie in the window and whose place is 4-byte aligned stores
//            three dwords, any other lane single bytes; nothing outside the window is written.
//   resize : cv2.resize at INTER_LANCZOS4 on uint8 in OpenCV's portable fixed-point arithmetic: eight taps per axis at clamp(s - 3 + k, 0, src - 1) with 11-bit
//            coefficients (tables made on the host: the device's double sin / cos is not libm's), h = sum S a in int32, v = sum h b in int32,
//            saturate_u8((v + 2^21) >> 22).  A workgroup owns 16 x 64 output pixels.  LDS plan (the 2 : 1 shrink of the 2048^2 image, any enlargement): the source
//            window of the tile, at most 40 rows x 136 pixels, is staged with aligned dword loads (a row keeps its address's low two bits as its offset in LDS);
//            every staged row is filtered horizontally ONCE, a lane forming the three channels of one (row, column) from 24 consecutive bytes (seven aligned
//            LDS dwords, v_alignbyte), into int32 [row][64][3]; the vertical pass reads that.  A tile whose window does not fit (a shrink beyond 2 : 1) is
//            formed directly from global memory, 64 taps a pixel.  Integer sums: both forms give the same bits.  cv2 is installed nowhere this project is built or
//            tested: the numpy restatement in tests/esrgan_tile_model.py, written from OpenCV's algorithm, is the pin.
#include "common.h"

namespace e4s {

__global__ __launch_bounds__(256) void esrt_input_kernel(float* __restrict__ out, const uint8_t* __restrict__ img, int64_t n, int H, int W, int chw, int y0,
                                                         int x0, int th, int tw) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t row = e / tw;                                             // (b * 3 + c) * th + y
        const int x = (int)(e - row * tw);
        const int64_t plane = row / th;
        const int y = (int)(row - plane * th);
        const int64_t b = plane / 3;
        const int c = (int)(plane - b * 3);
        int sy = y0 + y, sx = x0 + x;
        if (sy >= H) sy = 2 * H - 2 - sy;                                       // reflect: Hp - H < H, so 0 <= sy
        if (sx >= W) sx = 2 * W - 2 - sx;
        const int64_t src = chw ? ((b * 3 + c) * H + sy) * (int64_t)W + sx : ((b * H + sy) * (int64_t)W + sx) * 3 + c;
        out[e] = (float)img[src] / 255.f;
    }
}

constexpr int ET_CMAX = 64;                      // conv_last's input channels: a multiple of ET_CH up to this
constexpr int ET_TW = 64, ET_TH = 16;            // the tile of a workgroup: 16 lanes x 4 pixels across, 16 rows
constexpr int ET_CH = 8;                         // input channels per LDS chunk
constexpr int ET_LW = 72;                        // LDS row: the left halo at column 3, the tile at 4 .. 67, the right halo at 68
constexpr int ET_LH = ET_TH + 2;
constexpr int ET_WROW = 28;                      // 27 weights of an input channel, [row][column][output], padded to seven 16-byte reads

// the output chain of RealESRGANer.enhance behind the network, every rounding written out
__device__ __forceinline__ uint8_t esrt_u8(float r) {
#pragma clang fp contract(off)
    float a = fminf(fmaxf(r, 0.f), 1.f);
    a = a * 255.f;
    return (uint8_t)rintf(a);                                                   // round half to even
}

// grid (ceil((ox1 - ox0) / 64), ceil((oy1 - oy0) / 16), bs)
__global__ __launch_bounds__(256) void esrt_tail_kernel(uint8_t* __restrict__ canvas, const float* __restrict__ x, const float* __restrict__ wgt,
                                                        const float* __restrict__ bias, int C, int H, int W, int oy0, int oy1, int ox0, int ox1, int Y0, int X0,
                                                        int CH, int64_t pitch, int pack) {
    __shared__ __attribute__((aligned(16))) float tile[ET_CH * ET_LH * ET_LW];
    __shared__ __attribute__((aligned(16))) float wl[ET_CMAX * ET_WROW];
    const int tid = threadIdx.x;
    const int lx = tid & 15, ly = tid >> 4;
    const int tx0 = ox0 + blockIdx.x * ET_TW, ty0 = oy0 + blockIdx.y * ET_TH;   // in the tile's output
    const int64_t b = blockIdx.z;
    const int64_t hw = (int64_t)H * W;
    const float* xb = x + b * C * hw;

    for (int i = tid; i < C * 27; i += 256) {
        const int ci = i / 27, r = i - ci * 27;
        const int tap = r / 3, o = r - tap * 3;
        wl[ci * ET_WROW + r] = wgt[(o * C + ci) * 9 + tap];
    }
    for (int i = tid; i < C; i += 256) wl[i * ET_WROW + 27] = 0.f;

    float acc[3][4];
#pragma unroll
    for (int o = 0; o < 3; ++o)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[o][j] = bias[o];

    for (int c0 = 0; c0 < C; c0 += ET_CH) {
        __syncthreads();                                                        // the previous chunk has been read (first pass: nothing yet)
        for (int i = tid; i < ET_CH * ET_LH * (ET_TW + 2); i += 256) {
            const int rr = i / (ET_TW + 2), cx = i - rr * (ET_TW + 2);          // rr = c * LH + r
            const int c = rr / ET_LH, r = rr - c * ET_LH;
            const int gy = ty0 - 1 + r, gx = tx0 - 1 + cx;
            float v = 0.f;                                                      // zero outside the TILE's output: conv_last's own padding
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xb[(c0 + c) * hw + (int64_t)gy * W + gx];
            tile[rr * ET_LW + 3 + cx] = v;
        }
        __syncthreads();
#pragma unroll 2
        for (int c = 0; c < ET_CH; ++c) {
            float wv[ET_WROW];
            const float4* wp = reinterpret_cast<const float4*>(wl + (c0 + c) * ET_WROW);       // the same address in every lane
#pragma unroll
            for (int k = 0; k < ET_WROW / 4; ++k) {
                const float4 q = wp[k];
                wv[4 * k] = q.x; wv[4 * k + 1] = q.y; wv[4 * k + 2] = q.z; wv[4 * k + 3] = q.w;
            }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const float* rp = tile + (c * ET_LH + ly + ky) * ET_LW + 4 * lx + 3;
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

    const int y = ty0 + ly, xq = tx0 + 4 * lx;
    if (y >= oy1 || xq >= ox1) return;                                          // outside the kept window: nothing is written
    uint8_t u[12];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int o = 0; o < 3; ++o) u[j * 3 + o] = esrt_u8(acc[o][j]);
    uint8_t* up8 = canvas + (b * CH + (Y0 + y - oy0)) * pitch + (int64_t)(X0 + xq - ox0) * 3;
    if (pack && xq + 4 <= ox1) {                                                // pitch, the canvas and X0 * 3 are multiples of 4; so is (xq - ox0) * 3
        uint32_t* up = reinterpret_cast<uint32_t*>(up8);
#pragma unroll
        for (int k = 0; k < 3; ++k) up[k] = (uint32_t)u[4 * k] | ((uint32_t)u[4 * k + 1] << 8) | ((uint32_t)u[4 * k + 2] << 16) | ((uint32_t)u[4 * k + 3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (xq + j >= ox1) break;
#pragma unroll
            for (int o = 0; o < 3; ++o) up8[j * 3 + o] = u[j * 3 + o];
        }
    }
}

constexpr int LZ_TH = 16, LZ_TW = 64;            // output pixels of a workgroup
constexpr int LZ_SR = 40, LZ_SC = 136;           // the staged source window at the most: 2 * 15 + 8 rows, 2 * 63 + 8 pixels, the 2 : 1 shrink
constexpr int LZ_PITCH = 416;                    // bytes of a staged row: 136 * 3 + 3 of alignment offset, to a multiple of 16
constexpr int LZ_ROWDW = LZ_PITCH / 4;

__device__ __forceinline__ int lz_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ uint8_t lz_u8(int v) {
    const int r = (v + (1 << 21)) >> 22;
    return (uint8_t)lz_clamp(r, 0, 255);
}

// eight int16 coefficients of one destination index (16-byte aligned)
__device__ __forceinline__ void lz_coef(const void* table, int d, int (&a)[8]) {
    const int4 q = reinterpret_cast<const int4*>(table)[d];
    const int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a[2 * k] = (int)(short)(w[k] & 0xffff);
        a[2 * k + 1] = w[k] >> 16;
    }
}

// one output pixel straight from global memory
__device__ void lz_direct(uint8_t* __restrict__ op, const uint8_t* __restrict__ src, int H, int W, int yo, const int (&bc)[8], int xo, const int (&ac)[8]) {
    int v[3] = {0, 0, 0};
    int xs[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) xs[k] = lz_clamp(xo + k, 0, W - 1) * 3;
    for (int ky = 0; ky < 8; ++ky) {
        const uint8_t* rp = src + (int64_t)lz_clamp(yo + ky, 0, H - 1) * W * 3;
        int h[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) h[c] += (int)rp[xs[k] + c] * ac[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] += h[c] * bc[ky];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) op[c] = lz_u8(v[c]);
}

// grid (ceil(Wo / 64), ceil(Ho / 16), bs)
__global__ __launch_bounds__(256) void cv_resize_lanczos4_u8_kernel(uint8_t* __restrict__ out, const uint8_t* __restrict__ img, const int* __restrict__ yofs,
                                                                    const void* __restrict__ ycoef, const int* __restrict__ xofs,
                                                                    const void* __restrict__ xcoef, int bs, int H, int W, int Ho, int Wo) {
    __shared__ __attribute__((aligned(16))) uint8_t sbuf[LZ_SR * LZ_PITCH + 32];               // (+ 32: the seven-dword read of the last pixel of the last row)
    __shared__ int hbuf[LZ_SR * LZ_TW * 3];
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * LZ_TW, ty0 = blockIdx.y * LZ_TH;
    const int b = blockIdx.z;
    const int ny = min(LZ_TH, Ho - ty0), nx = min(LZ_TW, Wo - tx0);
    const uint8_t* src = img + (int64_t)b * H * W * 3;
    // the tile's source window [rmin, rmax) x [cmin, cmax), cut to the image (the taps clamp their index, so what lies outside is never read)
    const int rmin = lz_clamp(yofs[ty0], 0, H - 1), rmax = lz_clamp(yofs[ty0 + ny - 1] + 8, rmin + 1, H);
    const int cmin = lz_clamp(xofs[tx0], 0, W - 1), cmax = lz_clamp(xofs[tx0 + nx - 1] + 8, cmin + 1, W);
    const int nr = rmax - rmin, nc = cmax - cmin;

    if (nr > LZ_SR || nc > LZ_SC) {                                             // the window does not fit: every pixel on its own (uniform over the workgroup)
        for (int i = tid; i < LZ_TH * LZ_TW; i += 256) {
            const int y = i >> 6, x = i & 63;
            if (y >= ny || x >= nx) continue;
            int ac[8], bc[8];
            lz_coef(xcoef, tx0 + x, ac);
            lz_coef(ycoef, ty0 + y, bc);
            lz_direct(out + (((int64_t)b * Ho + ty0 + y) * Wo + tx0 + x) * 3, src, H, W, yofs[ty0 + y], bc, xofs[tx0 + x], ac);
        }
        return;
    }

    // stage: row i of LDS holds bytes cmin * 3 .. cmax * 3 of source row rmin + i behind an offset of (address & 3) bytes, moved as aligned dwords.  A dword that
    // reaches outside the image tensor is put together from the bytes inside it.
    const uint8_t* lo = img;
    const uint8_t* hi = img + (int64_t)bs * H * W * 3;
    for (int i = tid; i < nr * LZ_ROWDW; i += 256) {
        const int r = i / LZ_ROWDW, d = i - r * LZ_ROWDW;
        const uint8_t* g = src + ((int64_t)(rmin + r) * W + cmin) * 3;
        const int a = (int)((uintptr_t)g & 3);
        if (4 * d >= a + nc * 3) continue;
        const uint8_t* p = g - a + 4 * d;
        uint32_t v;
        if (p >= lo && p + 4 <= hi) {
            v = *reinterpret_cast<const uint32_t*>(p);
        } else {
            v = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (p + k >= lo && p + k < hi) v |= (uint32_t)p[k] << (8 * k);
        }
        reinterpret_cast<uint32_t*>(sbuf)[r * LZ_ROWDW + d] = v;
    }
    __syncthreads();

    // horizontal: hbuf[r][x][c] = sum_k S[r][clamp(xofs + k)][c] * a_k.  A lane keeps its column (256 is a multiple of 64): offset and coefficients are read once.
    const int x = tid & 63;
    if (x < nx) {
        const int xo = xofs[tx0 + x];
        int ac[8];
        lz_coef(xcoef, tx0 + x, ac);
        const bool whole = xo >= cmin && xo + 8 <= cmax;                        // no tap clamps: 24 consecutive bytes
        for (int r = tid >> 6; r < nr; r += 4) {
            const int a = (int)((uintptr_t)(src + ((int64_t)(rmin + r) * W + cmin) * 3) & 3);
            int h[3] = {0, 0, 0};
            if (whole) {
                const int off = r * LZ_PITCH + a + (xo - cmin) * 3;
                const uint32_t* wp = reinterpret_cast<const uint32_t*>(sbuf) + (off >> 2);
                const int sh = off & 3;
                uint32_t w[7], u[6];
#pragma unroll
                for (int k = 0; k < 7; ++k) w[k] = wp[k];
#pragma unroll
                for (int k = 0; k < 6; ++k) u[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);
#pragma unroll
                for (int k = 0; k < 8; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int byte = k * 3 + c;
                        h[c] += (int)((u[byte >> 2] >> (8 * (byte & 3))) & 0xffu) * ac[k];
                    }
            } else {
                const uint8_t* rowp = sbuf + r * LZ_PITCH + a;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int col = lz_clamp(lz_clamp(xo + k, 0, W - 1), cmin, cmax - 1) - cmin;   // (the second clamp holds for the tables of the rule)
#pragma unroll
                    for (int c = 0; c < 3; ++c) h[c] += (int)rowp[col * 3 + c] * ac[k];
                }
            }
            int* hp = hbuf + (r * LZ_TW + x) * 3;
            hp[0] = h[0]; hp[1] = h[1]; hp[2] = h[2];
        }
    }
    __syncthreads();

    // vertical: a lane owns column x of rows y, y + 4, y + 8, y + 12
    if (x >= nx) return;
    for (int y = tid >> 6; y < ny; y += 4) {
        const int yo = yofs[ty0 + y];
        int bc[8];
        lz_coef(ycoef, ty0 + y, bc);
        int v[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int r = lz_clamp(lz_clamp(yo + k, 0, H - 1), rmin, rmax - 1) - rmin;
            const int* hp = hbuf + (r * LZ_TW + x) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] += hp[c] * bc[k];
        }
        uint8_t* op = out + (((int64_t)b * Ho + ty0 + y) * Wo + tx0 + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) op[c] = lz_u8(v[c]);
    }
}

}  // namespace e4s

using namespace e4s;

extern "C" int e4s_esrt_input(float* out, const uint8_t* img, int bs, int H, int W, int Hp, int Wp, int chw, int y0, int x0, int th, int tw, void* stream) {
    E4S_REQUIRE(bs >= 0 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "esrt_input: bad size");
    E4S_REQUIRE(Hp >= H && Wp >= W && Hp - H < H && Wp - W < W, "esrt_input: a %d x %d image cannot be reflect-padded to %d x %d", H, W, Hp, Wp);
    E4S_REQUIRE(th >= 1 && tw >= 1 && y0 >= 0 && x0 >= 0 && y0 <= Hp - th && x0 <= Wp - tw, "esrt_input: the window [%d:%d+%d, %d:%d+%d] does not lie in %d x %d",
                y0, y0, th, x0, x0, tw, Hp, Wp);
    if (bs == 0) return 0;
    E4S_REQUIRE(out && img, "esrt_input: null tensor");
    const int64_t n = (int64_t)bs * 3 * th * tw;
    hipLaunchKernelGGL(esrt_input_kernel, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, out, img, n, H, W, chw ? 1 : 0, y0, x0, th, tw);
    return check_launch("esrt_input");
}

extern "C" int e4s_esrt_tail(uint8_t* canvas, float* out_f, const float* x, const float* weight, const float* bias, int bs, int C, int H, int W, int oy0, int oy1,
                             int ox0, int ox1, int Y0, int X0, int CH, int CW, int64_t pitch, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "esrt_tail: bad size");
    E4S_REQUIRE(C >= ET_CH && C <= ET_CMAX && C % ET_CH == 0, "esrt_tail: C is a multiple of %d up to %d, got %d", ET_CH, ET_CMAX, C);
    E4S_REQUIRE(oy0 >= 0 && oy0 < oy1 && oy1 <= H && ox0 >= 0 && ox0 < ox1 && ox1 <= W, "esrt_tail: the window [%d:%d, %d:%d] does not lie in %d x %d", oy0, oy1, ox0,
                ox1, H, W);
    E4S_REQUIRE(CH >= 1 && CW >= 1 && CH <= 16384 && CW <= 16384 && pitch >= (int64_t)CW * 3, "esrt_tail: bad canvas %d x %d, pitch %lld", CH, CW, (long long)pitch);
    E4S_REQUIRE(Y0 >= 0 && X0 >= 0 && Y0 <= CH - (oy1 - oy0) && X0 <= CW - (ox1 - ox0), "esrt_tail: the window placed at (%d, %d) leaves the %d x %d canvas", Y0, X0, CH,
                CW);
    E4S_REQUIRE(out_f == nullptr, "esrt_tail: no float output is offered");
    if (bs == 0) return 0;
    E4S_REQUIRE(canvas && x && weight && bias, "esrt_tail: null tensor");
    const int pack = pitch % 4 == 0 && (((uintptr_t)canvas) & 3) == 0 && X0 % 4 == 0;
    const dim3 grid(cdiv(ox1 - ox0, ET_TW), cdiv(oy1 - oy0, ET_TH), bs);
    hipLaunchKernelGGL(esrt_tail_kernel, grid, dim3(256), 0, (hipStream_t)stream, canvas, x, weight, bias, C, H, W, oy0, oy1, ox0, ox1, Y0, X0, CH, pitch, pack);
    return check_launch("esrt_tail");
}

extern "C" int e4s_cv_resize_lanczos4_u8(uint8_t* out, const uint8_t* img, const int* yofs, const void* ycoef, const int* xofs, const void* xcoef, int bs, int H,
                                         int W, int Ho, int Wo, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1 && H <= 16384 && W <= 16384 && Ho <= 16384 && Wo <= 16384,
                "cv_resize_lanczos4_u8: bad size");
    if (bs == 0) return 0;
    E4S_REQUIRE(out && img && yofs && ycoef && xofs && xcoef, "cv_resize_lanczos4_u8: null tensor");
    E4S_REQUIRE(((((uintptr_t)ycoef) | ((uintptr_t)xcoef)) & 15) == 0 && ((((uintptr_t)yofs) | ((uintptr_t)xofs)) & 3) == 0, "cv_resize_lanczos4_u8: unaligned table");
    const dim3 grid(cdiv(Wo, LZ_TW), cdiv(Ho, LZ_TH), bs);
    hipLaunchKernelGGL(cv_resize_lanczos4_u8_kernel, grid, dim3(256), 0, (hipStream_t)stream, out, img, yofs, ycoef, xofs, xcoef, bs, H, W, Ho, Wo);
    return check_launch("cv_resize_lanczos4_u8");
}
