// f8 (Blender recolouring, stage 1): the semantic colour reference of swap_face_fine/Blender/model_center/semantic_tools.py:50-167 on the device, a masked
// cross-attention per facial part: ref_p[:, a] = sum_t softmax_t(tau cos(x_a, y_t)) rgb_T[:, t] over the part's pixels a of A and t of T, and its inverse.
//   cr_lists   : one workgroup per (sample, part): the part's pixels of A and of T at the feature size (the nearest pick is index arithmetic), ascending,
//                with their counts; a T entry carries CR_ZERO when A's mask of the part is 0 there (the reference masks T's features with A's mask).
//   cr_rows    : per PIXEL, not per part: the 256 channels of a pixel with their mean subtracted, divided by max(norm, 1e-8), as one 1 KiB row.  Centring and
//                scaling a row do not depend on the part; only the zeroing of a key does, and that is the list's flag.  So the scratch is 2 hw rows per
//                sample whatever the masks are (overlapping ones too), where rows per part would need 18 hw.  Also rgb_T and the inverse's target.
//   cr_attend  : 32 queries per workgroup, the part's keys in tiles of 32 dealt to the 4 waves.  Scores on v_mfma_f32_32x32x2_f32 (exact float32) with the KEYS
//                as rows and the QUERIES as columns: a lane then owns one query and 16 of a tile's 32 scores, so the online softmax (running maximum, sum,
//                RGB sums) is private to the lane.  The 8 partial states of a query (4 waves x 2 lane halves) are merged in a fixed order, divided and
//                scattered to the [3, h, w] plane.  The query operand (128 floats per lane) stays in registers; key rows come straight from L2.
//                The inverse is the same kernel with the two lists swapped and ref_p as the values.
//   cr_sum_parts / cr_package : inv = sum_p inv_p; head_ref / inpaint_ref (zero below two present parts) resized bilinearly (align_corners) to H x W.
// Grids depend on shapes alone, a workgroup without work returns; no atomics, fixed summation orders: the same inputs give the same bits.
#include <math.h>

#include "common.h"

using namespace e4s;

namespace {

constexpr int CR_D = 256;                  // feature channels
constexpr int CR_PARTS = 9;                // skin hair eye nose lip tooth ear brow inpainting
constexpr int CR_MAXHW = 4096;
constexpr int CR_T = 32;                   // queries per workgroup = keys per tile = the MFMA's 32 x 32
constexpr int CR_ZERO = 1 << 16;           // list entry flag: this T pixel's feature row counts as zero
constexpr int CR_PIX = 0xFFFF;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct CrScratch {                         // byte offsets into the scratch buffer
    size_t counts, idx, rows, rgb, total;
};
CrScratch cr_layout(int bs, int hw) {
    CrScratch s;
    s.counts = 0;
    s.idx = ((size_t)bs * 2 * CR_PARTS * sizeof(int) + 255) & ~(size_t)255;
    s.rows = s.idx + (size_t)bs * 2 * CR_PARTS * hw * sizeof(int);
    s.rows = (s.rows + 255) & ~(size_t)255;
    s.rgb = s.rows + (size_t)bs * 2 * hw * CR_D * sizeof(float);
    s.total = s.rgb + (size_t)bs * 3 * hw * sizeof(float);
    return s;
}

// ------------------------------------------------------------------------------------------------ part lists
// parts_a / parts_t uint8 [bs][9][H][W]; counts int [bs][2][9]; idx int [bs][2][9][hw]; present uint8 [bs][9]
__global__ __launch_bounds__(256) void cr_lists_kernel(int* __restrict__ counts, int* __restrict__ idx, uint8_t* __restrict__ present,
                                                       const uint8_t* __restrict__ parts_a, const uint8_t* __restrict__ parts_t, int H, int W, int h, int w) {
    __shared__ int offs[257];
    const int p = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int hw = h * w, per = (hw + 255) >> 8;
    const float sy = (float)H / (float)h, sx = (float)W / (float)w;
    const uint8_t* __restrict__ ma = parts_a + ((size_t)b * CR_PARTS + p) * H * W;
    const uint8_t* __restrict__ mt = parts_t + ((size_t)b * CR_PARTS + p) * H * W;
    const int lo = t * per, hi = min(lo + per, hw);
    int total[2];
    for (int side = 0; side < 2; ++side) {
        const uint8_t* __restrict__ m = side ? mt : ma;
        int n = 0;
        for (int i = lo; i < hi; ++i) {
            const int y = i / w, x = i - y * w;
            n += m[(size_t)nearest_src(y, sy, H) * W + nearest_src(x, sx, W)] != 0;
        }
        offs[t + 1] = n;
        __syncthreads();
        if (t == 0) {
            offs[0] = 0;
            for (int k = 1; k <= 256; ++k) offs[k] += offs[k - 1];
        }
        __syncthreads();
        int o = offs[t];
        total[side] = offs[256];
        int* __restrict__ list = idx + (((size_t)b * 2 + side) * CR_PARTS + p) * hw;
        for (int i = lo; i < hi; ++i) {
            const int y = i / w, x = i - y * w;
            const size_t src = (size_t)nearest_src(y, sy, H) * W + nearest_src(x, sx, W);
            if (m[src] != 0) list[o++] = i | ((side && ma[src] == 0) ? CR_ZERO : 0);
        }
        __syncthreads();
    }
    if (t == 0) {
        counts[((size_t)b * 2 + 0) * CR_PARTS + p] = total[0];
        counts[((size_t)b * 2 + 1) * CR_PARTS + p] = total[1];
        present[(size_t)b * CR_PARTS + p] = (total[0] > 0 && total[1] > 0) ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ unit rows, rgb_T, the inverse's target
__device__ __forceinline__ float cr_denorm(float v, int c) {
#pragma clang fp contract(off)
    const float std_c = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
    const float mean_c = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f);
    const float r = v * std_c + mean_c;                                // a rounded product, then a rounded sum, as the tensor expression
    return fminf(fmaxf(r, 0.f), 1.f);
}

// grid (ceil(hw / 32), 2, bs): 32 pixels of side blockIdx.y (0 = A, 1 = T).  rows [bs][2][hw][256]; rgb [bs][3][hw]; inv_target [bs][3][hw] or NULL
__global__ __launch_bounds__(256) void cr_rows_kernel(float* __restrict__ rows, float* __restrict__ rgb, float* __restrict__ inv_target,
                                                      const float* __restrict__ feats_a, const float* __restrict__ feats_t, const float* __restrict__ img_t,
                                                      const uint8_t* __restrict__ parts_t, int H, int W, int h, int w) {
    __shared__ float tile[CR_T][CR_D + 1];
    const int side = blockIdx.y, b = blockIdx.z, hw = h * w;
    const int pix0 = blockIdx.x * CR_T;
    const float* __restrict__ f = (side ? feats_t : feats_a) + (size_t)b * CR_D * hw;
    for (int e = threadIdx.x; e < CR_T * CR_D; e += 256) {             // lanes run over pixels: consecutive addresses
        const int c = e >> 5, r = e & 31;
        tile[r][c] = pix0 + r < hw ? f[(size_t)c * hw + pix0 + r] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* __restrict__ dst = rows + ((size_t)b * 2 + side) * hw * CR_D;
    for (int k = 0; k < CR_T / 4; ++k) {
        const int r = wv * (CR_T / 4) + k;
        if (pix0 + r >= hw) break;                                     // wave-uniform
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = tile[r][lane + 64 * j];
        const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.f / CR_D);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] -= mean;
        const float nrm = sqrtf(wave_sum((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3])));
        const float den = fmaxf(nrm, 1e-8f);
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[(size_t)(pix0 + r) * CR_D + lane + 64 * j] = v[j] / den;
    }
    if (side == 1 && threadIdx.x < 3 * CR_T) {
        const int c = threadIdx.x >> 5, pix = pix0 + (threadIdx.x & 31);
        if (pix < hw) {
            const int y = pix / w, x = pix - y * w;
            const size_t src = (size_t)nearest_src(y, (float)H / (float)h, H) * W + nearest_src(x, (float)W / (float)w, W);
            const float v = cr_denorm(img_t[((size_t)b * 3 + c) * H * W + src], c);
            rgb[((size_t)b * 3 + c) * hw + pix] = v;
            if (inv_target) {
                int m = 0;                                             // head_T + inpainting_T = the sum of the nine masks
                for (int p = 0; p < CR_PARTS; ++p) m += parts_t[((size_t)b * CR_PARTS + p) * H * W + src];
                inv_target[((size_t)b * 3 + c) * hw + pix] = v * (float)m;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ the fused attention
struct CrState { float m, l, a0, a1, a2; };

// grid (ceil(hw / 32), 9, bs).  Queries: list `qside` of the part, keys: the other list.  values: [3][hw] planes at values + b vstride_b + p vstride_p,
// read at the keys' pixels; out [bs][9][3][hw], written at the queries' pixels (the rest stays as the caller zeroed it).
__global__ __launch_bounds__(256) void cr_attend_kernel(float* __restrict__ out, const float* __restrict__ values, size_t vstride_b, size_t vstride_p,
                                                        const int* __restrict__ counts, const int* __restrict__ idx, const float* __restrict__ rows,
                                                        float tau_host, const float* __restrict__ tau_dev, int hw, int qside) {
    __shared__ float4 kval[4][CR_T];                                   // per wave: the values of its tile's keys
    __shared__ CrState part[8][CR_T];
    const int p = blockIdx.y, b = blockIdx.z, kside = 1 - qside;
    const int nq = counts[((size_t)b * 2 + qside) * CR_PARTS + p], nk = counts[((size_t)b * 2 + kside) * CR_PARTS + p];
    const int q0 = blockIdx.x * CR_T;
    if (nq == 0 || nk == 0 || q0 >= nq) return;                        // workgroup-uniform, before any barrier
    const float tau = tau_dev ? *tau_dev : tau_host;
    const int* __restrict__ qlist = idx + (((size_t)b * 2 + qside) * CR_PARTS + p) * hw;
    const int* __restrict__ klist = idx + (((size_t)b * 2 + kside) * CR_PARTS + p) * hw;
    const float* __restrict__ qrows = rows + ((size_t)b * 2 + qside) * hw * CR_D;
    const float* __restrict__ krows = rows + ((size_t)b * 2 + kside) * hw * CR_D;
    const float* __restrict__ val = values + (size_t)b * vstride_b + (size_t)p * vstride_p;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, hf = lane >> 5, col = lane & 31;

    // the MFMA sums over k in pairs (k = lane half); which 256 -> 128 x 2 pairing is free as long as both operands use it: half hf takes channels 128 hf ..
    const int qe = qlist[min(q0 + col, nq - 1)];
    float q[CR_D / 2];
    {
        const float4* __restrict__ src = reinterpret_cast<const float4*>(qrows + (size_t)(qe & CR_PIX) * CR_D + hf * (CR_D / 2));
        const bool zero = (qe & CR_ZERO) != 0;
#pragma unroll
        for (int c = 0; c < CR_D / 8; ++c) {
            const float4 v = zero ? make_float4(0.f, 0.f, 0.f, 0.f) : src[c];
            q[4 * c] = v.x; q[4 * c + 1] = v.y; q[4 * c + 2] = v.z; q[4 * c + 3] = v.w;
        }
    }
    CrState st = {-INFINITY, 0.f, 0.f, 0.f, 0.f};
    const int nkt = (nk + CR_T - 1) / CR_T;
    for (int kt0 = 0; kt0 < nkt; kt0 += 4) {                           // every wave makes the same number of trips: the barriers are uniform
        const int kt = kt0 + wv;
        const bool active = kt < nkt;
        int ke = 0;
        if (active) {
            ke = klist[min(kt * CR_T + col, nk - 1)];
            if (hf == 0) {
                const int kp = ke & CR_PIX;
                kval[wv][col] = make_float4(val[kp], val[(size_t)hw + kp], val[(size_t)2 * hw + kp], 0.f);
            }
        }
        __syncthreads();
        if (active) {
            const float4* __restrict__ src = reinterpret_cast<const float4*>(krows + (size_t)(ke & CR_PIX) * CR_D + hf * (CR_D / 2));
            const bool zero = (ke & CR_ZERO) != 0;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int c = 0; c < CR_D / 8; ++c) {
                const float4 v = zero ? make_float4(0.f, 0.f, 0.f, 0.f) : src[c];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v.x, q[4 * c], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v.y, q[4 * c + 1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v.z, q[4 * c + 2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v.w, q[4 * c + 3], acc, 0, 0, 0);
            }
            // register r of this lane: key (r & 3) + 8 (r >> 2) + 4 hf of the tile, query col
            const int nvalid = nk - kt * CR_T;
            float s[16], mt = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[r] = tau * acc[r];
                if ((r & 3) + 8 * (r >> 2) + 4 * hf < nvalid) mt = fmaxf(mt, s[r]);
            }
            if (mt > -INFINITY) {
                const float mn = fmaxf(st.m, mt);
                const float sc = expf(st.m - mn);                      // 0 on the first tile (m = -inf)
                st.l *= sc; st.a0 *= sc; st.a1 *= sc; st.a2 *= sc;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = (r & 3) + 8 * (r >> 2) + 4 * hf;
                    if (i < nvalid) {
                        const float pr = expf(s[r] - mn);
                        const float4 v = kval[wv][i];
                        st.l += pr; st.a0 += pr * v.x; st.a1 += pr * v.y; st.a2 += pr * v.z;
                    }
                }
                st.m = mn;
            }
        }
        __syncthreads();
    }
    part[wv * 2 + hf][col] = st;
    __syncthreads();
    if (threadIdx.x < CR_T && q0 + threadIdx.x < nq) {
        float M = -INFINITY;
#pragma unroll
        for (int k = 0; k < 8; ++k) M = fmaxf(M, part[k][threadIdx.x].m);
        float l = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const CrState s = part[k][threadIdx.x];
            if (s.m > -INFINITY) {
                const float sc = expf(s.m - M);
                l += s.l * sc; a0 += s.a0 * sc; a1 += s.a1 * sc; a2 += s.a2 * sc;
            }
        }
        const int qp = qe & CR_PIX;                                    // threads 0 .. 31 are lanes 0 .. 31 of wave 0: col = threadIdx.x
        float* __restrict__ o = out + ((size_t)b * CR_PARTS + p) * 3 * hw;
        o[qp] = a0 / l;
        o[(size_t)hw + qp] = a1 / l;
        o[(size_t)2 * hw + qp] = a2 / l;
    }
}

// ------------------------------------------------------------------------------------------------ sums and the package's reference channels
// inv [bs][3][hw] = sum over p, ascending, of inv_parts [bs][9][3][hw]
__global__ __launch_bounds__(256) void cr_sum_parts_kernel(float* __restrict__ inv, const float* __restrict__ inv_parts, int n3hw) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= n3hw) return;
    const float* __restrict__ src = inv_parts + (size_t)b * CR_PARTS * n3hw + i;
    float s = src[0];
    for (int p = 1; p < CR_PARTS; ++p) s += src[(size_t)p * n3hw];
    inv[(size_t)b * n3hw + i] = s;
}

// out [bs][6][H][W]: channels 0-2 = head_ref (parts 0 .. 7 summed, ascending), 3-5 = inpaint_ref (part 8), bilinear with align_corners = True from h x w;
// all zero where fewer than two of the sample's nine parts are present
__global__ __launch_bounds__(256) void cr_package_kernel(float* __restrict__ out, const float* __restrict__ refs, const uint8_t* __restrict__ present,
                                                         int H, int W, int h, int w) {
    const int b = blockIdx.y, o = blockIdx.x * 256 + threadIdx.x;
    if (o >= H * W) return;
    int npresent = 0;
    for (int p = 0; p < CR_PARTS; ++p) npresent += present[(size_t)b * CR_PARTS + p];
    const int Y = o / W, X = o - Y * W, hw = h * w;
    float* __restrict__ dst = out + (size_t)b * 6 * H * W + o;
    if (npresent < 2) {
        for (int c = 0; c < 6; ++c) dst[(size_t)c * H * W] = 0.f;
        return;
    }
    const float sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    const float fy = sy * (float)Y, fx = sx * (float)X;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly1 = fy - (float)y0, lx1 = fx - (float)x0, ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    const int t00 = y0 * w + x0, t01 = y0 * w + x1, t10 = y1 * w + x0, t11 = y1 * w + x1;
    const float* __restrict__ rb = refs + (size_t)b * CR_PARTS * 3 * hw;
    for (int c = 0; c < 3; ++c) {
        float v00 = 0.f, v01 = 0.f, v10 = 0.f, v11 = 0.f;
        for (int p = 0; p < CR_PARTS - 1; ++p) {
            const float* __restrict__ pl = rb + ((size_t)p * 3 + c) * hw;
            v00 += pl[t00]; v01 += pl[t01]; v10 += pl[t10]; v11 += pl[t11];
        }
        dst[(size_t)c * H * W] = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
        const float* __restrict__ pl = rb + ((size_t)(CR_PARTS - 1) * 3 + c) * hw;
        dst[(size_t)(3 + c) * H * W] = ly0 * (lx0 * pl[t00] + lx1 * pl[t01]) + ly1 * (lx0 * pl[t10] + lx1 * pl[t11]);
    }
}

bool cr_aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

#define CR_SHAPES(name)                                                                                                                    \
    E4S_REQUIRE(bs >= 0 && bs <= 65535, name ": bs %d is not in 0..65535", bs);                                                            \
    E4S_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= CR_MAXHW, name ": feature size %d x %d: h * w must be in 1..%d", h, w, CR_MAXHW)
#define CR_MAPS(name) E4S_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 26), name ": map size %d x %d: H * W must be in 1..2^26", H, W)

}  // namespace

extern "C" int e4s_colorref_scratch_bytes(int bs, int h, int w, int64_t* bytes) {
    E4S_REQUIRE(bytes, "colorref_scratch_bytes: null result");
    CR_SHAPES("colorref_scratch_bytes");
    *bytes = (int64_t)cr_layout(bs, h * w).total;
    return 0;
}

extern "C" int e4s_colorref_lists(void* scratch, uint8_t* present, const uint8_t* parts_a, const uint8_t* parts_t, int bs, int H, int W, int h, int w,
                                  void* stream) {
    CR_SHAPES("colorref_lists");
    CR_MAPS("colorref_lists");
    if (bs == 0) return 0;
    E4S_REQUIRE(scratch && present && parts_a && parts_t && cr_aligned(scratch, 16), "colorref_lists: null or misaligned tensor");
    const CrScratch s = cr_layout(bs, h * w);
    char* base = (char*)scratch;
    hipLaunchKernelGGL(cr_lists_kernel, dim3(CR_PARTS, bs), dim3(256), 0, (hipStream_t)stream, (int*)(base + s.counts), (int*)(base + s.idx), present, parts_a,
                       parts_t, H, W, h, w);
    return check_launch("colorref_lists");
}

extern "C" int e4s_colorref_rows(void* scratch, float* inv_target, const float* feats_a, const float* feats_t, const float* img_t, const uint8_t* parts_t,
                                 int bs, int D, int H, int W, int h, int w, void* stream) {
    CR_SHAPES("colorref_rows");
    CR_MAPS("colorref_rows");
    E4S_REQUIRE(D == CR_D, "colorref_rows: %d feature channels, the kernel is built for %d", D, CR_D);
    if (bs == 0) return 0;
    E4S_REQUIRE(scratch && feats_a && feats_t && img_t && parts_t && cr_aligned(scratch, 16), "colorref_rows: null or misaligned tensor");
    const CrScratch s = cr_layout(bs, h * w);
    char* base = (char*)scratch;
    hipLaunchKernelGGL(cr_rows_kernel, dim3(cdiv(h * w, CR_T), 2, bs), dim3(256), 0, (hipStream_t)stream, (float*)(base + s.rows), (float*)(base + s.rgb),
                       inv_target, feats_a, feats_t, img_t, parts_t, H, W, h, w);
    return check_launch("colorref_rows");
}

extern "C" int e4s_colorref_attend(float* refs, float* inv_parts, const void* scratch, float tau, const float* tau_dev, int bs, int h, int w, void* stream) {
    CR_SHAPES("colorref_attend");
    if (bs == 0) return 0;
    E4S_REQUIRE(refs && scratch && cr_aligned(scratch, 16) && refs != inv_parts, "colorref_attend: null, misaligned or aliased tensor");
    const int hw = h * w;
    const CrScratch s = cr_layout(bs, hw);
    const char* base = (const char*)scratch;
    const int* counts = (const int*)(base + s.counts);
    const int* idx = (const int*)(base + s.idx);
    const float* rows = (const float*)(base + s.rows);
    const float* rgb = (const float*)(base + s.rgb);
    const dim3 grid(cdiv(hw, CR_T), CR_PARTS, bs);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cr_attend_kernel, grid, dim3(256), 0, st, refs, rgb, (size_t)3 * hw, (size_t)0, counts, idx, rows, tau, tau_dev, hw, 0);
    if (inv_parts)
        hipLaunchKernelGGL(cr_attend_kernel, grid, dim3(256), 0, st, inv_parts, (const float*)refs, (size_t)CR_PARTS * 3 * hw, (size_t)3 * hw, counts, idx, rows,
                           tau, tau_dev, hw, 1);
    return check_launch("colorref_attend");
}

extern "C" int e4s_colorref_sum_parts(float* inv, const float* inv_parts, int bs, int h, int w, void* stream) {
    CR_SHAPES("colorref_sum_parts");
    if (bs == 0) return 0;
    E4S_REQUIRE(inv && inv_parts && inv != inv_parts, "colorref_sum_parts: null or aliased tensor");
    const int n = 3 * h * w;
    hipLaunchKernelGGL(cr_sum_parts_kernel, dim3(cdiv(n, 256), bs), dim3(256), 0, (hipStream_t)stream, inv, inv_parts, n);
    return check_launch("colorref_sum_parts");
}

extern "C" int e4s_colorref_package(float* out, const float* refs, const uint8_t* present, int bs, int H, int W, int h, int w, void* stream) {
    CR_SHAPES("colorref_package");
    CR_MAPS("colorref_package");
    if (bs == 0) return 0;
    E4S_REQUIRE(out && refs && present, "colorref_package: null tensor");
    hipLaunchKernelGGL(cr_package_kernel, dim3(cdiv(H * W, 256), bs), dim3(256), 0, (hipStream_t)stream, out, refs, present, H, W, h, w);
    return check_launch("colorref_package");
}
