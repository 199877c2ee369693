// f18: the kd x 7 x 7 (kd 7 or 1), stride 1, zero-pad (kd / 2, 3, 3) convolution on [bs, Cin, D, H, W] float32 with at most 32 output channels (face-vid2vid's
// DenseMotionNetwork: the `mask` head, a 7 x 7 x 7 Conv3d 112 -> 16, and the `occlusion` head, a 7 x 7 Conv2d on prediction.view(bs, C D, H, W), which is kd 1
// with D 1) as an implicit GEMM on the three-way bf16 split of conv3d.hip (a = a0 + a1 + a2, six MFMAs per K step, fp32 accumulation).
//
//   D[co][pos] = sum_{k = (ci, kd, kh, kw)} W[co][k] * X[k][pos]
//
// The MFMA is v_mfma_f32_16x16x32_bf16: 16 output channels (A rows) x 16 pixels of one image row (B columns); its 32-deep K holds TWO (kh, kw) taps of a
// 16-channel chunk (k group l >> 4: tap 2 pair + (group >> 1), channel half group & 1), so 16 output channels fill the tile and 17 .. 32 take two of them.  The 7
// taps of a kh are four pairs; the eighth tap is a block of zero weights that stays in LDS (its pixels are read from tap 6: finite).
//
// A workgroup owns one depth slice d of the output, a 16 x 8 pixel tile of it and every output channel; wave w owns rows 2 w and 2 w + 1.  Its K loop runs over
// (16-channel chunk, kd) steps: a step stages ONE input depth slice d + kd - kd / 2 of the chunk (patch 22 x 14, split once into three bf16 planes) and reuses it
// for the 49 (kh, kw) taps of that kd; steps whose slice lies in the depth padding are skipped as a whole (workgroup-uniform).  The weights stream in sub-steps of one
// kh (7 taps, 10.5 KB per 16 output channels) through two LDS buffers; the next sub-step's weights and the next step's patch are loaded from global memory before the
// current MFMAs.  The leading products of a step are summed apart and join the total through an error-free two-sum (K reaches 38 416: one fp32 chain would
// cost a few 1e-6 of the result).  The order of accumulation depends on the shapes alone: the same inputs give the same bits and a batch of two equals two
// batches of one.
#include "common.h"

using namespace e4s;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int K7_CK = 16;                    // channels per K chunk
constexpr int K7_TW = 16, K7_TH = 8;         // output tile
constexpr int K7_PW = K7_TW + 6, K7_PH = K7_TH + 6;
constexpr int K7_PATCH = K7_PW * K7_PH;      // 308
constexpr int K7_NT = 256;
constexpr int K7_EPT = (K7_PATCH + K7_NT - 1) / K7_NT;

__device__ __forceinline__ unsigned k7_pack_bf16(float a, float b) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, bf16x2));
}

extern "C" int e4s_conv3d_k7_prep_weights_sb3(uint16_t* w0, uint16_t* w1, uint16_t* w2, const float* weight, int cout, int cin, int kd, void* stream) {
    E4S_REQUIRE(w0 && w1 && w2 && weight, "conv3d_k7_prep_weights_sb3: null tensor");
    E4S_REQUIRE(cout >= 1 && cin >= 1, "conv3d_k7_prep_weights_sb3: bad size");
    E4S_REQUIRE(kd == 7 || kd == 1, "conv3d_k7_prep_weights_sb3: kd %d not supported (7 or 1)", kd);
    // [cout][cin][49 kd] is the 2-D preparation's [cout][cin][kh * kw]: the same chunk layout, the same three-way split
    return e4s_conv_prep_weights_sb3(w0, w1, w2, nullptr, weight, nullptr, nullptr, nullptr, nullptr, 0.f, nullptr, cout, cin, 49 * kd, 1, stream);
}

struct Conv3dK7Params {
    float* out;
    const float* x;
    const uint4* wsl[3];
    const float* bias;
    int act, kdim;
    int bs, cin, cout, D, H, W;
    int tiles_x, tiles_y;
};

template <int CB>
struct K7Cfg {
    static constexpr int TN = 16 * CB;
    static constexpr int WB4 = 3 * 8 * 2 * TN;          // uint4 per weight buffer: [term][tap of one kh, the eighth zero][half][TN]
    static constexpr int WS4 = 3 * 7 * 2 * TN;          // uint4 loaded per sub-step
    static constexpr int WPT = (WS4 + K7_NT - 1) / K7_NT;
    static constexpr int LDS_BYTES = 2 * WB4 * 16 + K7_PATCH * 32 * 3;
    static_assert(LDS_BYTES <= 80 * 1024, "two workgroups per CU");
};

template <int CB>
__global__ __launch_bounds__(256, 2) void conv3d_k7_sb3_kernel(const Conv3dK7Params p) {
    using C = K7Cfg<CB>;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    uint4* wsm = reinterpret_cast<uint4*>(lds_raw);                     // [2][3][8][2][TN]
    uint4* xpl = reinterpret_cast<uint4*>(lds_raw + 2 * C::WB4 * 16);   // 3 planes of [PATCH][2]: 16 bf16 per patch pixel, halves swizzled

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l4 = lane & 15, grp = lane >> 4;
    const int ntile = p.tiles_x * p.tiles_y;
    const int d = blockIdx.x / ntile, tile = blockIdx.x - d * ntile;
    const int oy0 = (tile / p.tiles_x) * K7_TH, ox0 = (tile % p.tiles_x) * K7_TW;
    const int b = blockIdx.z;
    const int nchunk = (p.cin + K7_CK - 1) / K7_CK;
    const int ntap = 49 * p.kdim;
    const size_t plane = (size_t)p.H * p.W;
    const size_t cstride = plane * p.D;

    // the eighth tap of both buffers: zero weights, written once
    for (int i = tid; i < 2 * 3 * 2 * C::TN; i += K7_NT) {
        const int bt = i / (2 * C::TN), r = i - bt * 2 * C::TN;          // (buffer, term), (half, n)
        wsm[bt * 16 * C::TN + 14 * C::TN + r] = make_uint4(0u, 0u, 0u, 0u);
    }

    int goffs[K7_EPT];
    bool ginb[K7_EPT];
#pragma unroll
    for (int j = 0; j < K7_EPT; ++j) {
        const int e = tid + j * K7_NT;
        const int py = e / K7_PW, px = e - py * K7_PW;
        const int gy = oy0 - 3 + py, gx = ox0 - 3 + px;
        ginb[j] = (e < K7_PATCH) && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
        goffs[j] = ginb[j] ? gy * p.W + gx : 0;
    }
    const float* xb = p.x + (size_t)b * p.cin * cstride;

    // K is long (343 x 112 for the mask head): a single fp32 chain would lose a few 1e-6 of the result to its own roundings.  The leading products a0 b0 of a
    // step go to acc_hi, which is added to the total with an error-free two-sum after every step; the five small products go to acc_lo for the whole loop.
    f32x4 acc_hi[CB][2], acc_lo[CB][2], tot[CB][2], tot_err[CB][2];
#pragma unroll
    for (int i = 0; i < CB; ++i)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc_hi[i][q] = acc_lo[i][q] = tot[i][q] = tot_err[i][q] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // the kd taps whose input slice exists: a contiguous range, the same for every lane of the workgroup
    const int pd = p.kdim >> 1;
    const int kd_lo = pd - d > 0 ? pd - d : 0;
    const int kd_hi = p.D - 1 - d + pd < p.kdim - 1 ? p.D - 1 - d + pd : p.kdim - 1;
    const int nkd = kd_hi - kd_lo + 1;
    const int nstep = nchunk * nkd;

    float xr[K7_CK][K7_EPT];
    unsigned wr[C::WPT][4];

    // Unconditional loads: out-of-image elements read a valid clamped address and are zeroed at conversion time; channels >= cin read the last channel and meet
    // zero-padded weights; output-channel rows >= cout read the last row and are never stored.
    auto load_patch = [&](int step) __attribute__((always_inline)) {
        const int chunk = step / nkd, kd = kd_lo + (step - chunk * nkd);
        const int ci0 = chunk * K7_CK;
        const float* xs = xb + (size_t)ci0 * cstride + (size_t)(d + kd - pd) * plane;
        const int cmax = p.cin - 1 - ci0;
#pragma unroll
        for (int c = 0; c < K7_CK; ++c) {
            const float* xc = xs + (size_t)(c < cmax ? c : cmax) * cstride;
#pragma unroll
            for (int j = 0; j < K7_EPT; ++j) xr[c][j] = xc[goffs[j]];
        }
    };
    auto load_w = [&](int step, int kh) __attribute__((always_inline)) {
        const int chunk = step / nkd, kd = kd_lo + (step - chunk * nkd);
        const size_t wbase = ((size_t)chunk * ntap + kd * 49 + kh * 7) * 2 * p.cout;
#pragma unroll
        for (int v = 0; v < C::WPT; ++v) {
            int idx = tid + v * K7_NT;
            idx = idx < C::WS4 ? idx : C::WS4 - 1;
            const int hl = idx / (14 * C::TN);
            const int rem = idx - hl * 14 * C::TN;
            const int th = rem / C::TN, n = rem - th * C::TN;
            const int co = n < p.cout ? n : p.cout - 1;
            const uint4* slab = hl == 0 ? p.wsl[0] : (hl == 1 ? p.wsl[1] : p.wsl[2]);
            const uint4 t4 = slab[wbase + (size_t)th * p.cout + co];
            wr[v][0] = t4.x; wr[v][1] = t4.y; wr[v][2] = t4.z; wr[v][3] = t4.w;
        }
    };
    auto store_w = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int v = 0; v < C::WPT; ++v) {
            const int idx = tid + v * K7_NT;
            if (idx < C::WS4) {
                const int hl = idx / (14 * C::TN);
                const int rem = idx - hl * 14 * C::TN;
                wsm[buf * C::WB4 + hl * 16 * C::TN + rem] = make_uint4(wr[v][0], wr[v][1], wr[v][2], wr[v][3]);
            }
        }
    };
    auto store_patch = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < K7_EPT; ++j) {
            const int e = tid + j * K7_NT;
            if (e < K7_PATCH) {
                unsigned h[8], l[8], l2[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float t0 = ginb[j] ? xr[2 * c][j] : 0.f;
                    const float t1 = ginb[j] ? xr[2 * c + 1][j] : 0.f;
                    h[c] = k7_pack_bf16(t0, t1);
                    const float r0 = t0 - __builtin_bit_cast(float, h[c] << 16), r1 = t1 - __builtin_bit_cast(float, h[c] & 0xffff0000u);
                    l[c] = k7_pack_bf16(r0, r1);
                    l2[c] = k7_pack_bf16(r0 - __builtin_bit_cast(float, l[c] << 16), r1 - __builtin_bit_cast(float, l[c] & 0xffff0000u));
                }
                const int sw = (e >> 3) & 1;
                uint4 *x0p = xpl, *x1p = xpl + 2 * K7_PATCH, *x2p = xpl + 4 * K7_PATCH;
                x0p[e * 2 + (0 ^ sw)] = make_uint4(h[0], h[1], h[2], h[3]);
                x0p[e * 2 + (1 ^ sw)] = make_uint4(h[4], h[5], h[6], h[7]);
                x1p[e * 2 + (0 ^ sw)] = make_uint4(l[0], l[1], l[2], l[3]);
                x1p[e * 2 + (1 ^ sw)] = make_uint4(l[4], l[5], l[6], l[7]);
                x2p[e * 2 + (0 ^ sw)] = make_uint4(l2[0], l2[1], l2[2], l2[3]);
                x2p[e * 2 + (1 ^ sw)] = make_uint4(l2[4], l2[5], l2[6], l2[7]);
            }
        }
    };
    const int half = grp & 1, tsel = grp >> 1;
    auto compute = [&](int kh, int buf) __attribute__((always_inline)) {
        const uint4* wb = wsm + buf * C::WB4 + half * C::TN + l4;
#pragma unroll
        for (int pair = 0; pair < 4; ++pair) {
            const int tap = 2 * pair + tsel;                 // 7: the zero block
            const int tapx = tap < 6 ? tap : 6;
            uint4 bt[3][2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int e = (wave * 2 + q + kh) * K7_PW + l4 + tapx;
                const int slot = e * 2 + (half ^ ((e >> 3) & 1));
#pragma unroll
                for (int t = 0; t < 3; ++t) bt[t][q] = xpl[t * 2 * K7_PATCH + slot];
            }
            uint4 at[3][CB];
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int i = 0; i < CB; ++i) at[t][i] = wb[t * 16 * C::TN + tap * 2 * C::TN + i * 16];
            // products in order of magnitude: (0,0) (0,1) (1,0) (0,2) (2,0) (1,1)
            constexpr int TA[6] = {0, 0, 1, 0, 2, 1};
            constexpr int TB[6] = {0, 1, 0, 2, 0, 1};
#pragma unroll
            for (int i = 0; i < CB; ++i)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    acc_hi[i][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, at[0][i]), __builtin_bit_cast(bf16x8, bt[0][q]),
                                                                           acc_hi[i][q], 0, 0, 0);
#pragma unroll
                    for (int pr = 1; pr < 6; ++pr)
                        acc_lo[i][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, at[TA[pr]][i]), __builtin_bit_cast(bf16x8, bt[TB[pr]][q]),
                                                                               acc_lo[i][q], 0, 0, 0);
                }
        }
    };
    // tot + acc_hi as an exact sum (Knuth's two-sum): the rounded sum stays in tot, what the rounding dropped is collected in tot_err
    auto flush = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < CB; ++i)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float a = tot[i][q][r], b = acc_hi[i][q][r];
                    const float t = a + b;
                    if constexpr (CB == 1) {      // (the 32-channel form has no registers left for tot_err: its total takes one rounding per step)
                        const float bp = t - a;
                        tot_err[i][q][r] += (a - (t - bp)) + (b - bp);
                    }
                    tot[i][q][r] = t;
                    acc_hi[i][q][r] = 0.f;
                }
    };

    load_patch(0);
    load_w(0, 0);
    int cnt = 0;                                             // sub-steps done: the weights of sub-step cnt live in buffer cnt & 1
    for (int step = 0; step < nstep; ++step) {
        __syncthreads();                                     // the previous step's patch and the buffer cnt & 1 (read two sub-steps ago) are free
        store_patch();
        store_w(cnt & 1);
        __syncthreads();
        if (step + 1 < nstep) load_patch(step + 1);
        for (int kh = 0; kh < 7; ++kh) {
            if (kh < 6) load_w(step, kh + 1);
            else if (step + 1 < nstep) load_w(step + 1, 0);
            compute(kh, cnt & 1);
            if (kh < 6) {
                store_w((cnt + 1) & 1);                      // last read in sub-step cnt - 1, before the barrier that ended it
                __syncthreads();
            }
            ++cnt;
        }
        flush();
    }

    // Epilogue: D column = pixel l4 of the row, D row = output channel 4 grp + r
    const int ox = ox0 + l4;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int oy = oy0 + wave * 2 + q;
        if (oy >= p.H || ox >= p.W) continue;
        const size_t opix = (size_t)d * plane + (size_t)oy * p.W + ox;
#pragma unroll
        for (int i = 0; i < CB; ++i) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = i * 16 + grp * 4 + r;
                if (co < p.cout) {
                    float v = tot[i][q][r] + (tot_err[i][q][r] + acc_lo[i][q][r]);
                    if (p.bias) v += p.bias[co];
                    if (p.act == 3) v = 1.f / (1.f + expf(-v));
                    p.out[((size_t)b * p.cout + co) * cstride + opix] = v;
                }
            }
        }
    }
}

template <int CB>
static int launch_k7(Conv3dK7Params& p, hipStream_t st) {
    using C = K7Cfg<CB>;
    p.tiles_x = cdiv(p.W, K7_TW);
    p.tiles_y = cdiv(p.H, K7_TH);
    const int64_t gx = (int64_t)p.tiles_x * p.tiles_y * p.D;
    E4S_REQUIRE(gx <= 0x7fffffff, "conv3d_k7_sb3: volume too large");
    dim3 grid((unsigned)gx, 1, p.bs);
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3d_k7_sb3_kernel<CB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       C::LDS_BYTES);
    if (attr != hipSuccess) return fail((int)attr, "conv3d_k7_sb3: cannot raise the dynamic LDS limit: %s", hipGetErrorString(attr));
    hipLaunchKernelGGL((conv3d_k7_sb3_kernel<CB>), grid, dim3(K7_NT), C::LDS_BYTES, st, p);
    return check_launch("conv3d_k7_sb3");
}

extern "C" int e4s_conv3d_k7_sb3(float* out, const float* x, const uint16_t* w0, const uint16_t* w1, const uint16_t* w2, const float* bias, int act, int kd, int bs,
                                 int cin, int cout, int D, int H, int W, void* stream) {
    E4S_REQUIRE(w0 && w1 && w2 && (bs == 0 || (out && x)), "conv3d_k7_sb3: null tensor");
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && cin >= 1 && D >= 1 && H >= 1 && W >= 1, "conv3d_k7_sb3: bad size");
    E4S_REQUIRE(cout >= 1 && cout <= 32, "conv3d_k7_sb3: cout %d not supported (1 .. 32)", cout);
    E4S_REQUIRE(kd == 7 || kd == 1, "conv3d_k7_sb3: kd %d not supported (7 or 1)", kd);
    E4S_REQUIRE(act == 0 || act == 3, "conv3d_k7_sb3: bad activation (0 none, 3 sigmoid)");
    E4S_REQUIRE((int64_t)H * W <= 0x7fffffff, "conv3d_k7_sb3: volume too large");
    E4S_REQUIRE((((uintptr_t)w0 | (uintptr_t)w1 | (uintptr_t)w2) & 15) == 0, "conv3d_k7_sb3: weight slabs must be 16-byte aligned");
    if (bs == 0) return 0;
    Conv3dK7Params p;
    p.out = out; p.x = x; p.bias = bias; p.act = act; p.kdim = kd;
    p.wsl[0] = reinterpret_cast<const uint4*>(w0); p.wsl[1] = reinterpret_cast<const uint4*>(w1); p.wsl[2] = reinterpret_cast<const uint4*>(w2);
    p.bs = bs; p.cin = cin; p.cout = cout; p.D = D; p.H = H; p.W = W;
    hipStream_t st = (hipStream_t)stream;
    if (cout <= 16) return launch_k7<1>(p, st);
    return launch_k7<2>(p, st);
}
