// f17: the 3 x 3 x 3, stride 1, zero-pad 1 convolution on [bs, Cin, D, H, W] float32 (face-vid2vid: UpBlock3d, the kp / jacobian heads, later ResBlock3d) as an
// implicit GEMM on the three-way bf16 split of conv.hip's e4s_conv2d_sb3 (a = a0 + a1 + a2, six v_mfma_f32_32x32x16_bf16 per 16-deep step, fp32 accumulation).
//
//   D[co][pos] = sum_{k = (ci, kd, kh, kw)} W[co][k] * X'[k][pos],   X' = x read at (d, y / up_hw, x / up_hw): UpBlock3d's nearest (1, 2, 2) upsampling is in the gather
//
// A workgroup owns one depth slice d of the output, a TH x TW pixel tile of it and TN output channels.  Its K loop runs over (16-channel chunk, kd) steps: a step
// stages ONE input depth slice d + kd - 1 of the chunk (patch (TH + 2) x (TW + 2), split once into three bf16 planes) and the 9 (kh, kw) taps of that kd from the
// slabs, so a step is exactly a 3 x 3 step of the 2-D kernel; steps whose slice lies in the depth padding are skipped as a whole (workgroup-uniform).  The next
// step's global loads are issued before the current step's MFMAs.  The order of accumulation depends on the shapes alone: the same inputs give the same bits, a batch
// of two equals two batches of one, and up_hw = 2 equals up_hw = 1 on the upsampled volume (the same values reach LDS).
// f18: x, out and residual carry element batch strides (e4s_conv3d_sb3_strided); the unstrided entry point passes the dense ones.
#include <stdlib.h>

#include "common.h"

using namespace e4s;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
constexpr int C3_CK = 16;      // channels per K chunk
constexpr int C3_TAPS = 27;

__device__ __forceinline__ unsigned c3_pack_bf16(float a, float b) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, bf16x2));
}

extern "C" int e4s_conv3d_prep_weights_sb3(uint16_t* w0, uint16_t* w1, uint16_t* w2, float* bias_out, const float* weight, const float* bn_gamma,
                                           const float* bn_beta, const float* bn_mean, const float* bn_var, float bn_eps, const float* conv_bias, int cout,
                                           int cin, void* stream) {
    E4S_REQUIRE(w0 && w1 && w2 && weight, "conv3d_prep_weights_sb3: null tensor");
    E4S_REQUIRE(cout >= 1 && cin >= 1, "conv3d_prep_weights_sb3: bad size");
    // [cout][cin][27] is the 2-D preparation's [cout][cin][kh * kw] with 27 taps: the same chunk layout, the same three-way split
    return e4s_conv_prep_weights_sb3(w0, w1, w2, bias_out, weight, bn_gamma, bn_beta, bn_mean, bn_var, bn_eps, conv_bias, cout, cin, C3_TAPS, 1, stream);
}

struct Conv3dParams {
    float* out;
    const float* x;
    const uint4* wsl[3];
    const float* bias;
    const float* residual;
    int act, up;
    int bs, cin, cout, D, H, W;      // output extents
    int hin, win;                    // input plane: H / up, W / up
    int tiles_x, tiles_y;
    size_t x_bs, out_bs, res_bs;     // element strides between samples (f18: a channel slice of a wider buffer is read or written in place)
};

template <int CB, int PB, int WC, int WP, int LOG_TW>
struct C3Cfg {
    static constexpr int TN = WC * CB * 32;
    static constexpr int NPB = WP * PB;
    static constexpr int TW = 1 << LOG_TW;
    static constexpr int RPB = 32 >> LOG_TW;
    static constexpr int TH = NPB * RPB;
    static constexpr int PW = TW + 2, PH = TH + 2;
    static constexpr int PATCH = PH * PW;
    static constexpr int NT = 64 * WC * WP;
    static constexpr int EPT = (PATCH + NT - 1) / NT;
    static constexpr int W4 = 3 * 9 * 2 * TN;        // uint4: [term][tap of one kd][half][TN]
    static constexpr int WPT = (W4 + NT - 1) / NT;
    static constexpr int LDS_BYTES = W4 * 16 + PATCH * 32 * 3;
    static_assert(WC * WP == 4, "256-thread workgroups");
    static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU");
};

template <int CB, int PB, int WC, int WP, int LOG_TW>
__global__ __launch_bounds__(256, 2) void conv3d_sb3_kernel(const Conv3dParams p) {
    using C = C3Cfg<CB, PB, WC, WP, LOG_TW>;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    uint4* wsm = reinterpret_cast<uint4*>(lds_raw);                 // [3][9][2][TN]
    uint4* xpl = reinterpret_cast<uint4*>(lds_raw + C::W4 * 16);    // 3 planes of [PATCH][2]: 16 bf16 per patch pixel, halves swizzled

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l5 = lane & 31, khalf = lane >> 5;
    const int wc = wave / WP, wp = wave % WP;
    const int ntile = p.tiles_x * p.tiles_y;
    const int d = blockIdx.x / ntile, tile = blockIdx.x - d * ntile;
    const int oy0 = (tile / p.tiles_x) * C::TH, ox0 = (tile % p.tiles_x) * C::TW;
    const int co0 = blockIdx.y * C::TN;
    const int b = blockIdx.z;
    const int nchunk = (p.cin + C3_CK - 1) / C3_CK;
    const size_t plane = (size_t)p.hin * p.win;        // one input depth slice
    const size_t cstride = plane * p.D;                // one input channel

    // patch element -> offset inside an input slice (the upsampling is here), or out of the image
    int goffs[C::EPT];
    bool ginb[C::EPT];
#pragma unroll
    for (int j = 0; j < C::EPT; ++j) {
        const int e = tid + j * C::NT;
        const int py = e / C::PW, px = e - py * C::PW;
        const int gy = oy0 - 1 + py, gx = ox0 - 1 + px;
        ginb[j] = (e < C::PATCH) && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
        goffs[j] = ginb[j] ? (p.up == 2 ? (gy >> 1) * p.win + (gx >> 1) : gy * p.win + gx) : 0;
    }
    const float* xb = p.x + (size_t)b * p.x_bs;

    int xoff[PB];
#pragma unroll
    for (int q = 0; q < PB; ++q) {
        const int pbk = wp * PB + q;
        const int ty = pbk * C::RPB + (l5 >> LOG_TW), tx = l5 & (C::TW - 1);
        xoff[q] = ty * C::PW + tx;
    }

    f32x16 acc[CB][PB];
#pragma unroll
    for (int i = 0; i < CB; ++i)
#pragma unroll
        for (int q = 0; q < PB; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][q][r] = 0.f;

    // the kd taps whose input slice exists: a contiguous range, the same for every lane of the workgroup
    const int kd_lo = d == 0 ? 1 : 0, kd_hi = d == p.D - 1 ? 1 : 2;
    const int nkd = kd_hi - kd_lo + 1;
    const int nstep = nchunk * nkd;

    float xr[C3_CK][C::EPT];
    unsigned wr[C::WPT][4];

    // Unconditional loads: out-of-image elements read a valid clamped address and are zeroed at conversion time; channels >= cin read the last channel and meet
    // zero-padded weights; output-channel rows >= cout read the last row and are never stored.
    auto load_step = [&](int step) __attribute__((always_inline)) {
        const int chunk = step / nkd, kd = kd_lo + (step - chunk * nkd);
        const int ci0 = chunk * C3_CK;
        const float* xs = xb + (size_t)ci0 * cstride + (size_t)(d + kd - 1) * plane;
        const int cmax = p.cin - 1 - ci0;
#pragma unroll
        for (int c = 0; c < C3_CK; ++c) {
            const float* xc = xs + (size_t)(c < cmax ? c : cmax) * cstride;
#pragma unroll
            for (int j = 0; j < C::EPT; ++j) xr[c][j] = xc[goffs[j]];
        }
        const size_t wbase = ((size_t)chunk * C3_TAPS + kd * 9) * 2 * p.cout;
#pragma unroll
        for (int v = 0; v < C::WPT; ++v) {
            int idx = tid + v * C::NT;
            idx = idx < C::W4 ? idx : C::W4 - 1;
            const int hl = idx / (9 * 2 * C::TN);
            const int rem = idx - hl * 9 * 2 * C::TN;
            const int th = rem / C::TN, n = rem - th * C::TN;
            const int co = (co0 + n < p.cout) ? co0 + n : p.cout - 1;
            const uint4* slab = hl == 0 ? p.wsl[0] : (hl == 1 ? p.wsl[1] : p.wsl[2]);
            const uint4 t4 = slab[wbase + (size_t)th * p.cout + co];
            wr[v][0] = t4.x; wr[v][1] = t4.y; wr[v][2] = t4.z; wr[v][3] = t4.w;
        }
    };
    auto store_step = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < C::EPT; ++j) {
            const int e = tid + j * C::NT;
            if (e < C::PATCH) {
                unsigned h[8], l[8], l2[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float t0 = ginb[j] ? xr[2 * c][j] : 0.f;
                    const float t1 = ginb[j] ? xr[2 * c + 1][j] : 0.f;
                    h[c] = c3_pack_bf16(t0, t1);
                    const float r0 = t0 - __builtin_bit_cast(float, h[c] << 16), r1 = t1 - __builtin_bit_cast(float, h[c] & 0xffff0000u);
                    l[c] = c3_pack_bf16(r0, r1);
                    l2[c] = c3_pack_bf16(r0 - __builtin_bit_cast(float, l[c] << 16), r1 - __builtin_bit_cast(float, l[c] & 0xffff0000u));
                }
                const int sw = (e >> 3) & 1;
                uint4 *x0p = xpl, *x1p = xpl + 2 * C::PATCH, *x2p = xpl + 4 * C::PATCH;
                x0p[e * 2 + (0 ^ sw)] = make_uint4(h[0], h[1], h[2], h[3]);
                x0p[e * 2 + (1 ^ sw)] = make_uint4(h[4], h[5], h[6], h[7]);
                x1p[e * 2 + (0 ^ sw)] = make_uint4(l[0], l[1], l[2], l[3]);
                x1p[e * 2 + (1 ^ sw)] = make_uint4(l[4], l[5], l[6], l[7]);
                x2p[e * 2 + (0 ^ sw)] = make_uint4(l2[0], l2[1], l2[2], l2[3]);
                x2p[e * 2 + (1 ^ sw)] = make_uint4(l2[4], l2[5], l2[6], l2[7]);
            }
        }
#pragma unroll
        for (int v = 0; v < C::WPT; ++v) {
            const int idx = tid + v * C::NT;
            if (idx < C::W4) wsm[idx] = make_uint4(wr[v][0], wr[v][1], wr[v][2], wr[v][3]);
        }
    };
    auto compute_step = [&]() __attribute__((always_inline)) {
        const uint4* whalf = wsm + khalf * C::TN + wc * CB * 32 + l5;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int toff = (tap / 3) * C::PW + (tap % 3);
            uint4 bt[3][PB];
#pragma unroll
            for (int q = 0; q < PB; ++q) {
                const int e = xoff[q] + toff;
                const int slot = e * 2 + (khalf ^ ((e >> 3) & 1));
#pragma unroll
                for (int t = 0; t < 3; ++t) bt[t][q] = xpl[t * 2 * C::PATCH + slot];
            }
            uint4 at[3][CB];
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int i = 0; i < CB; ++i) at[t][i] = whalf[t * 9 * 2 * C::TN + tap * 2 * C::TN + i * 32];
            // products in order of magnitude: (0,0) (0,1) (1,0) (0,2) (2,0) (1,1)
            constexpr int TA[6] = {0, 0, 1, 0, 2, 1};
            constexpr int TB[6] = {0, 1, 0, 2, 0, 1};
#pragma unroll
            for (int pr = 0; pr < 6; ++pr)
#pragma unroll
                for (int i = 0; i < CB; ++i)
#pragma unroll
                    for (int q = 0; q < PB; ++q)
                        acc[i][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, at[TA[pr]][i]), __builtin_bit_cast(bf16x8, bt[TB[pr]][q]),
                                                                            acc[i][q], 0, 0, 0);
        }
    };

    load_step(0);
    for (int step = 0; step < nstep; ++step) {
        __syncthreads();
        store_step();
        __syncthreads();
        if (step + 1 < nstep) load_step(step + 1);
        compute_step();
    }

    // Epilogue in two passes (conv.hip): every global load first, then the stores.
    const size_t ohw = (size_t)p.H * p.W;
    const size_t odhw = ohw * p.D;
#pragma unroll
    for (int q = 0; q < PB; ++q) {
        const int pbk = wp * PB + q;
        const int oy = oy0 + pbk * C::RPB + (l5 >> LOG_TW), ox = ox0 + (l5 & (C::TW - 1));
        const bool pix_ok = oy < p.H && ox < p.W;
        const size_t opix = (size_t)d * ohw + (size_t)oy * p.W + ox;
#pragma unroll
        for (int i = 0; i < CB; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + (wc * CB + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
                if (pix_ok && co < p.cout) {
                    float v = acc[i][q][r];
                    if (p.bias) v += p.bias[co];
                    if (p.residual) v += p.residual[(size_t)b * p.res_bs + (size_t)co * odhw + opix];
                    if (p.act == 1) v = fmaxf(v, 0.f);
                    acc[i][q][r] = v;
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < PB; ++q) {
        const int pbk = wp * PB + q;
        const int oy = oy0 + pbk * C::RPB + (l5 >> LOG_TW), ox = ox0 + (l5 & (C::TW - 1));
        if (oy >= p.H || ox >= p.W) continue;
        const size_t opix = (size_t)d * ohw + (size_t)oy * p.W + ox;
#pragma unroll
        for (int i = 0; i < CB; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + (wc * CB + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
                if (co < p.cout) p.out[(size_t)b * p.out_bs + (size_t)co * odhw + opix] = acc[i][q][r];
            }
        }
    }
}

template <int CB, int PB, int WC, int WP, int LOG_TW>
static int launch3d(Conv3dParams& p, hipStream_t st) {
    using C = C3Cfg<CB, PB, WC, WP, LOG_TW>;
    p.tiles_x = cdiv(p.W, C::TW);
    p.tiles_y = cdiv(p.H, C::TH);
    const int64_t gx = (int64_t)p.tiles_x * p.tiles_y * p.D;
    E4S_REQUIRE(gx <= 0x7fffffff, "conv3d_sb3: volume too large");
    dim3 grid((unsigned)gx, cdiv(p.cout, C::TN), p.bs);
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3d_sb3_kernel<CB, PB, WC, WP, LOG_TW>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES);
    if (attr != hipSuccess) return fail((int)attr, "conv3d_sb3: cannot raise the dynamic LDS limit: %s", hipGetErrorString(attr));
    hipLaunchKernelGGL((conv3d_sb3_kernel<CB, PB, WC, WP, LOG_TW>), grid, dim3(C::NT), C::LDS_BYTES, st, p);
    return check_launch("conv3d_sb3");
}

extern "C" int e4s_conv3d_sb3_strided(float* out, const float* x, const uint16_t* w0, const uint16_t* w1, const uint16_t* w2, const float* bias,
                                      const float* residual, int act, int up_hw, int bs, int cin, int cout, int D, int H, int W, int64_t x_bstride,
                                      int64_t out_bstride, int64_t res_bstride, void* stream) {
    E4S_REQUIRE(w0 && w1 && w2 && (bs == 0 || (out && x)), "conv3d_sb3: null tensor");
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && cin >= 1 && cout >= 1 && D >= 1 && H >= 1 && W >= 1, "conv3d_sb3: bad size");
    E4S_REQUIRE(act == 0 || act == 1, "conv3d_sb3: bad activation (0 none, 1 ReLU)");
    E4S_REQUIRE(up_hw == 1 || up_hw == 2, "conv3d_sb3: up_hw %d not supported (1 or 2)", up_hw);
    E4S_REQUIRE(H % up_hw == 0 && W % up_hw == 0, "conv3d_sb3: H and W are the output extents: multiples of up_hw");
    E4S_REQUIRE((int64_t)(H / up_hw) * (W / up_hw) <= 0x7fffffff && cdiv(cout, 32) <= 65535, "conv3d_sb3: volume too large");
    E4S_REQUIRE((((uintptr_t)w0 | (uintptr_t)w1 | (uintptr_t)w2) & 15) == 0, "conv3d_sb3: weight slabs must be 16-byte aligned");
    E4S_REQUIRE(x_bstride >= (int64_t)cin * D * (H / up_hw) * (W / up_hw) && out_bstride >= (int64_t)cout * D * H * W &&
                    (!residual || res_bstride >= (int64_t)cout * D * H * W),
                "conv3d_sb3: a batch stride is smaller than its sample");
    if (bs == 0) return 0;
    Conv3dParams p;
    p.x_bs = (size_t)x_bstride; p.out_bs = (size_t)out_bstride; p.res_bs = (size_t)res_bstride;
    p.out = out; p.x = x; p.bias = bias; p.residual = residual; p.act = act; p.up = up_hw;
    p.wsl[0] = reinterpret_cast<const uint4*>(w0); p.wsl[1] = reinterpret_cast<const uint4*>(w1); p.wsl[2] = reinterpret_cast<const uint4*>(w2);
    p.bs = bs; p.cin = cin; p.cout = cout; p.D = D; p.H = H; p.W = W; p.hin = H / up_hw; p.win = W / up_hw;
    hipStream_t st = (hipStream_t)stream;
    if (cout <= 32) {      // the kp / jacobian heads (15, 45 channels would idle half of a 64-row tile): 32 co x 128 px
        if (W > 16) return launch3d<1, 1, 1, 4, 5>(p, st);      // 32 x 4 pixels
        return launch3d<1, 1, 1, 4, 4>(p, st);                  // 16 x 8 pixels
    }
    if (W > 16) return launch3d<2, 1, 1, 4, 5>(p, st);          // 64 co x 128 px (32 x 4)
    return launch3d<1, 1, 2, 2, 4>(p, st);                      // 64 co x  64 px (16 x 4)
}

extern "C" int e4s_conv3d_sb3(float* out, const float* x, const uint16_t* w0, const uint16_t* w1, const uint16_t* w2, const float* bias, const float* residual,
                              int act, int up_hw, int bs, int cin, int cout, int D, int H, int W, void* stream) {
    E4S_REQUIRE(up_hw == 1 || up_hw == 2, "conv3d_sb3: up_hw %d not supported (1 or 2)", up_hw);
    const int64_t o = (int64_t)cout * D * H * W;
    return e4s_conv3d_sb3_strided(out, x, w0, w1, w2, bias, residual, act, up_hw, bs, cin, cout, D, H, W, (int64_t)cin * D * (H / up_hw) * (W / up_hw), o, o, stream);
}
