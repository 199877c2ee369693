// Row f14: what GPEN's face detector (swap_face_fine/gpen/face_detect: RetinaFaceDetection.detect, facemodels/retinaface.py, facemodels/net.py, PriorBox, decode,
// decode_landm, py_cpu_nms) needs around its convolutions, which run on conv.hip, and the whole detection tail behind the network.  fp32, no float atomics, no host
// synchronisation, grids from the shapes and capacities alone: the same inputs give the same bits.  Every kernel has a 16-byte form and a one-element form that
// evaluate the same expression per element.  Floating-point contraction is off in this file: the priors, the boxes and the IoU are sequences of single float32
// operations in the reference, and a product fused into the addition behind it would round once where the reference rounds twice.
//   input   : uint8 [bs][H][W][3] -> float [bs][3][H][W], pixel - (104, 117, 123) in BGR plane order (retinaface_detection.py:62-75); exact.
//   up_add  : out = a + nearest(b -> size of a), FPN.forward's F.interpolate(size=..., mode="nearest") + add (net.py:89-94), ATen's legacy index rule
//             min(floor(dst * (float)in / out), in - 1).
//   cat_relu: SSH.forward's relu(cat(conv3X3, conv5X5, conv7X7)) (net.py:64-65) for any batch, one pass.
//   decode  : per position of the three levels' 32-channel head maps (bbox 2 x 4, class 2 x 2, landmark 2 x 10; anchor index (y w + x) 2 + a, levels
//             concatenated): the dense loc / softmax conf / landms of RetinaFace.forward, the prior from index arithmetic, decode, decode_landm, the scale.
//   compact : every anchor with score > threshold, in anchor order, into [bs][cap] sort keys (score bits << 32 | ~index) with the counts; with more than cap of
//             them the cap highest scores survive (a radix select on the score bits; ties at the cut go to the lower index).  One workgroup per image.
//   nms     : py_cpu_nms on candidates sorted by score: gather, then greedy suppression by one workgroup per image with the flags in LDS.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace e4s {

constexpr int RF_HEAD = 32;                      // channels of a level's head map: 8 bbox, 4 class, 20 landmark
constexpr int RF_MAX_CAP = 16384;                // candidates per image the NMS holds flags for
constexpr int RF_CT = 1024;                      // threads of the one-workgroup-per-image kernels

static inline bool rf_al16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0;
}

// ------------------------------------------------------------------------------------------------ input
// A group is V consecutive pixels of one image (V = 4: H W % 4 == 0).  n: groups in all.
template <int V>
__global__ __launch_bounds__(256) void retina_input_kernel(float* __restrict__ out, const uint8_t* __restrict__ img, int bgr, int64_t n, int64_t hw) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int64_t p0 = g * V;
        const int64_t b = p0 / hw, r = p0 - b * hw;
        uint8_t px[V][3];
        if constexpr (V == 4) {
            const uint32_t* s32 = reinterpret_cast<const uint32_t*>(img + p0 * 3);
            const uint32_t q[3] = {s32[0], s32[1], s32[2]};
#pragma unroll
            for (int e = 0; e < 12; ++e) px[e / 3][e % 3] = (uint8_t)(q[e >> 2] >> (8 * (e & 3)));
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) px[0][c] = img[p0 * 3 + c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float mean = c == 0 ? 104.f : (c == 1 ? 117.f : 123.f);
            float v[V];
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = (float)px[j][bgr ? c : 2 - c] - mean;
            float* op = out + (b * 3 + c) * hw + r;
            if constexpr (V == 4) *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
            else op[0] = v[0];
        }
    }
}

// ------------------------------------------------------------------------------------------------ nearest upsampling + add
template <int V>
__global__ __launch_bounds__(256) void retina_up_add_kernel(float* __restrict__ out, const float* __restrict__ a, const float* __restrict__ b, int64_t n, int h,
                                                            int w, int hb, int wb, float sy, float sx) {
    const int gpr = w / V;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int64_t row = g / gpr;
        const int x0 = (int)(g - row * gpr) * V;
        const int64_t plane = row / h;
        const int y = (int)(row - plane * h);
        const float* br = b + (plane * hb + nearest_src(y, sy, hb)) * (int64_t)wb;
        const int64_t o = row * w + x0;
        if constexpr (V == 4) {
            const float4 q = *reinterpret_cast<const float4*>(a + o);
            *reinterpret_cast<float4*>(out + o) = make_float4(q.x + br[nearest_src(x0, sx, wb)], q.y + br[nearest_src(x0 + 1, sx, wb)],
                                                              q.z + br[nearest_src(x0 + 2, sx, wb)], q.w + br[nearest_src(x0 + 3, sx, wb)]);
        } else {
            out[o] = a[o] + br[nearest_src(x0, sx, wb)];
        }
    }
}

// ------------------------------------------------------------------------------------------------ cat + ReLU
template <int V>
__global__ __launch_bounds__(256) void retina_cat_relu_kernel(float* __restrict__ out, const float* __restrict__ a, const float* __restrict__ b,
                                                              const float* __restrict__ c, int64_t n, int ca, int cb, int cc, int hw) {
    const int ct = ca + cb + cc;
    const int gpp = hw / V;                                                      // groups per plane
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int64_t plane = g / gpp;                                           // s * ct + channel
        const int r = (int)(g - plane * gpp) * V;
        const int64_t s = plane / ct;
        const int ch = (int)(plane - s * ct);
        const float* src = ch < ca ? a + (s * ca + ch) * (int64_t)hw : (ch < ca + cb ? b + (s * cb + ch - ca) * (int64_t)hw : c + (s * cc + ch - ca - cb) * (int64_t)hw);
        if constexpr (V == 4) {
            const float4 q = *reinterpret_cast<const float4*>(src + r);
            *reinterpret_cast<float4*>(out + plane * hw + r) = make_float4(fmaxf(q.x, 0.f), fmaxf(q.y, 0.f), fmaxf(q.z, 0.f), fmaxf(q.w, 0.f));
        } else {
            out[plane * hw + r] = fmaxf(src[r], 0.f);
        }
    }
}

// ------------------------------------------------------------------------------------------------ decode
struct RetinaDecodeParams {
    const float* head[3];
    float *loc, *conf, *landms;                  // dense [bs][N][4], [bs][N][2], [bs][N][10], or all NULL
    float *score, *boxes, *lmk;                  // decoded [bs][N], [bs][N][4], [bs][N][10], or all NULL
    int bs, H, W, N;
    int lh[3], lw[3], pos0[3];                   // a level's map and its first position among all positions
};

template <bool VEC>
__device__ __forceinline__ void rf_store(float* dst, const float* v, int n4) {
    if constexpr (VEC) {
#pragma unroll
        for (int j = 0; j < 5; ++j)
            if (j < n4) reinterpret_cast<float4*>(dst)[j] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < 20; ++j)
            if (j < 4 * n4) dst[j] = v[j];
    }
}

// One lane owns a position: its two anchors are adjacent in every output, so the 16-byte form stores whole float4s (2 x 4 loc, 2 x 2 conf, 2 x 10 landms).
template <bool VEC>
__global__ __launch_bounds__(256) void retina_decode_kernel(RetinaDecodeParams p) {
    const int P = p.N / 2;
    const int64_t n = (int64_t)p.bs * P;
    const float fW = (float)p.W, fH = (float)p.H;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int64_t b = g / P;
        const int pos = (int)(g - b * P);
        const int l = pos >= p.pos0[2] ? 2 : (pos >= p.pos0[1] ? 1 : 0);
        const int q = pos - p.pos0[l];
        const int hwl = p.lh[l] * p.lw[l];
        const int y = q / p.lw[l], x = q - y * p.lw[l];
        const float* hp = p.head[l] + b * RF_HEAD * (int64_t)hwl + q;
        float v[RF_HEAD];
#pragma unroll
        for (int c = 0; c < RF_HEAD; ++c) v[c] = hp[(int64_t)c * hwl];
        // softmax over the two classes of each anchor, as F.softmax: exp(x - max) / sum
        float cf[4];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const float c0 = v[8 + 2 * a], c1 = v[9 + 2 * a];
            const float m = fmaxf(c0, c1);
            const float e0 = expf(c0 - m), e1 = expf(c1 - m);
            const float s = e0 + e1;
            cf[2 * a] = e0 / s;
            cf[2 * a + 1] = e1 / s;
        }
        const int64_t a0 = b * p.N + 2 * (int64_t)pos;                           // the first of the position's two anchors
        if (p.loc) {
            rf_store<VEC>(p.loc + a0 * 4, v, 2);
            rf_store<VEC>(p.conf + a0 * 2, cf, 1);
            rf_store<VEC>(p.landms + a0 * 10, v + 12, 5);
        }
        if (!p.score) continue;
        // PriorBox.forward: cx = (x + 0.5) * step / W, cy = (y + 0.5) * step / H, s_kx = min_size / W, s_ky = min_size / H; the numerators are exact
        const float step = (float)(8 << l);
        const float cx = ((float)x + 0.5f) * step / fW, cy = ((float)y + 0.5f) * step / fH;
        float bx[8], lm[20];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const float ms = (float)((16 << (2 * l)) << a);                      // 16, 32 / 64, 128 / 256, 512
            const float sw = ms / fW, sh = ms / fH;
            const float* lo = v + 4 * a;
            // decode: centre = prior + loc * 0.1 * size; size = prior size * exp(loc * 0.2); corners from the centre; then the scale (W, H, W, H)
            const float bcx = cx + lo[0] * 0.1f * sw, bcy = cy + lo[1] * 0.1f * sh;
            const float bw = sw * expf(lo[2] * 0.2f), bh = sh * expf(lo[3] * 0.2f);
            const float x1 = bcx - bw / 2.f, y1 = bcy - bh / 2.f;
            const float x2 = bw + x1, y2 = bh + y1;
            bx[4 * a] = x1 * fW; bx[4 * a + 1] = y1 * fH; bx[4 * a + 2] = x2 * fW; bx[4 * a + 3] = y2 * fH;
            const float* lp = v + 12 + 10 * a;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                lm[10 * a + 2 * k] = (cx + lp[2 * k] * 0.1f * sw) * fW;
                lm[10 * a + 2 * k + 1] = (cy + lp[2 * k + 1] * 0.1f * sh) * fH;
            }
        }
        p.score[a0] = cf[1];
        p.score[a0 + 1] = cf[3];
        rf_store<VEC>(p.boxes + a0 * 4, bx, 2);
        rf_store<VEC>(p.lmk + a0 * 10, lm, 5);
    }
}

// The priors alone, [N][4] = (cx, cy, s_kx, s_ky): what the decode kernel computes in registers, for the tests and for callers that want PriorBox.forward().
__global__ __launch_bounds__(256) void retina_priors_kernel(float* __restrict__ out, RetinaDecodeParams p) {
    const float fW = (float)p.W, fH = (float)p.H;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < p.N; i += gridDim.x * 256) {
        const int pos = i >> 1, a = i & 1;
        const int l = pos >= p.pos0[2] ? 2 : (pos >= p.pos0[1] ? 1 : 0);
        const int q = pos - p.pos0[l];
        const int y = q / p.lw[l], x = q - y * p.lw[l];
        const float step = (float)(8 << l), ms = (float)((16 << (2 * l)) << a);
        out[4 * (int64_t)i] = ((float)x + 0.5f) * step / fW;
        out[4 * (int64_t)i + 1] = ((float)y + 0.5f) * step / fH;
        out[4 * (int64_t)i + 2] = ms / fW;
        out[4 * (int64_t)i + 3] = ms / fH;
    }
}

// ------------------------------------------------------------------------------------------------ threshold + compaction
// Exclusive position of this thread's flag among the workgroup's, and the workgroup's total: a 64-bit ballot per wave, the wave totals through LDS.
__device__ __forceinline__ int rf_block_scan(bool flag, int* wave_tot, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                                                             // the previous round's readers are done with wave_tot
    if (lane == 0) wave_tot[wv] = __popcll(m);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < RF_CT / 64; ++k) {
        const int t = wave_tot[k];
        base += k < wv ? t : 0;
        total += t;
    }
    return base + before;
}

// keys [bs][cap] (int64): (score bits << 32) | (0xFFFFFFFF - anchor), -1 in the unused slots; counts [bs][2]: anchors above the threshold, candidates kept.
__global__ __launch_bounds__(RF_CT) void retina_compact_kernel(long long* __restrict__ keys, int* __restrict__ counts, const float* __restrict__ score, int N,
                                                               int cap, float thr) {
    __shared__ int wave_tot[RF_CT / 64];
    __shared__ int hist[256];
    __shared__ unsigned sel[2];                  // the radix select's prefix and how many of the cap are still to be found below it
    const float* sc = score + (int64_t)blockIdx.x * N;
    long long* kp = keys + (int64_t)blockIdx.x * cap;
    const int tid = threadIdx.x;
    // pass 1: count
    int mine = 0;
    for (int i = tid; i < N; i += RF_CT) mine += sc[i] > thr ? 1 : 0;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    atomicAdd(&hist[0], mine);                                                   // integer, in LDS: the sum does not depend on the order
    __syncthreads();
    const int count = hist[0];
    __syncthreads();
    // more than cap: find the cap-th largest score's bits, 8 bits at a time from the top (scores are positive floats: their bits order as they do)
    unsigned cut = 0u;                           // a candidate survives with bits > cut, or bits == cut and a place among the `ties` lowest indices
    int ties = 0;
    if (count > cap) {
        if (tid == 0) { sel[0] = 0u; sel[1] = (unsigned)cap; }
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const unsigned prefix = sel[0];
            const unsigned himask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
            for (int i = tid; i < N; i += RF_CT) {
                const float s = sc[i];
                const unsigned u = __float_as_uint(s);
                if (s > thr && (u & himask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned want = sel[1];
                int d = 255;
                for (; d > 0; --d) {
                    if ((unsigned)hist[d] >= want) break;
                    want -= (unsigned)hist[d];
                }
                sel[0] = prefix | ((unsigned)d << shift);
                sel[1] = want;
            }
            __syncthreads();
        }
        cut = sel[0];
        ties = (int)sel[1];
    }
    // pass 2: ordered compaction, 1024 anchors a round
    int base = 0, tie_base = 0;
    for (int i0 = 0; i0 < N; i0 += RF_CT) {
        const int i = i0 + tid;
        const float s = i < N ? sc[i] : 0.f;
        const unsigned u = __float_as_uint(s);
        const bool cand = i < N && s > thr;
        bool take = cand;
        if (count > cap) {
            const bool tie = cand && u == cut;
            int tie_total;
            const int tpos = rf_block_scan(tie, wave_tot, tie_total);
            take = cand && (u > cut || (tie && tie_base + tpos < ties));
            tie_base += tie_total;
        }
        int total;
        const int pos = rf_block_scan(take, wave_tot, total);
        if (take && base + pos < cap) kp[base + pos] = ((long long)u << 32) | (long long)(0xFFFFFFFFu - (unsigned)i);
        base += total;
    }
    const int kept = base < cap ? base : cap;
    for (int i = kept + tid; i < cap; i += RF_CT) kp[i] = -1ll;
    if (tid == 0) {
        counts[2 * blockIdx.x] = count;
        counts[2 * blockIdx.x + 1] = kept;
    }
}

// ------------------------------------------------------------------------------------------------ NMS
// cbox [bs][cap][4] = the boxes of the sorted candidates (rows past the count are not written and not read).
__global__ __launch_bounds__(256) void retina_gather_kernel(float* __restrict__ cbox, const long long* __restrict__ keys, const int* __restrict__ counts,
                                                            const float* __restrict__ boxes, int64_t n, int N, int cap) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int64_t b = g / cap;
        const int r = (int)(g - b * cap);
        if (r >= min(counts[2 * b + 1], cap)) continue;                         // counts come from the caller: never past the capacity
        const unsigned idx = 0xFFFFFFFFu - (unsigned)(keys[g] & 0xFFFFFFFFll);
        if (idx >= (unsigned)N) continue;                                        // never with keys the compaction wrote
        const float* s = boxes + (b * N + idx) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) cbox[g * 4 + j] = s[j];
    }
}

// Greedy suppression as py_cpu_nms walks it: the best candidate left is kept and removes every later one with ovr > thresh (ovr <= thresh stays), areas and
// overlaps with the + 1 pixel convention, each operation rounded to float32.  A candidate's fate is final once every kept one before it has been applied, so the
// walk stops at keep_top_k kept.
__global__ __launch_bounds__(RF_CT) void retina_nms_kernel(float* __restrict__ dets, float* __restrict__ lm_out, int* __restrict__ keep, int* __restrict__ nkeep,
                                                           const float* __restrict__ cbox, const long long* __restrict__ keys, const int* __restrict__ counts,
                                                           const float* __restrict__ lmk, int N, int cap, int keep_top_k, float thresh) {
    __shared__ uint8_t dead[RF_MAX_CAP];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(counts[2 * b + 1], cap);                                   // counts come from the caller: never past the capacity (dead[] holds RF_MAX_CAP)
    const float4* bx = reinterpret_cast<const float4*>(cbox) + (int64_t)b * cap;  // (cbox comes from the allocator: 16-byte aligned, checked on the host)
    const long long* kp = keys + (int64_t)b * cap;
    for (int i = tid; i < n; i += RF_CT) dead[i] = 0;
    __syncthreads();
    int kept = 0;
    for (int i = 0; i < n && kept < keep_top_k; ++i) {
        if (dead[i]) continue;                                                   // uniform: every thread reads the same flag behind the last barrier
        const float4 bi = bx[i];
        const float ai = (bi.z - bi.x + 1.f) * (bi.w - bi.y + 1.f);
        for (int j = i + 1 + tid; j < n; j += RF_CT) {
            if (dead[j]) continue;
            const float4 bj = bx[j];
            const float aj = (bj.z - bj.x + 1.f) * (bj.w - bj.y + 1.f);
            const float w = fmaxf(0.f, fminf(bi.z, bj.z) - fmaxf(bi.x, bj.x) + 1.f);
            const float h = fmaxf(0.f, fminf(bi.w, bj.w) - fmaxf(bi.y, bj.y) + 1.f);
            const float inter = w * h;
            const float ovr = inter / (ai + aj - inter);
            if (!(ovr <= thresh)) dead[j] = 1;
        }
        if (tid < 15) {                                                          // the kept row: box, score, and the landmarks as (x0..x4, y0..y4)
            const long long key = kp[i];
            const unsigned idx = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFll);
            const int64_t o = (int64_t)b * keep_top_k + kept;
            if (tid < 4) dets[o * 5 + tid] = tid == 0 ? bi.x : (tid == 1 ? bi.y : (tid == 2 ? bi.z : bi.w));
            else if (tid == 4) { dets[o * 5 + 4] = __uint_as_float((unsigned)((unsigned long long)key >> 32)); keep[o] = i; }
            else {
                const int k = tid - 5;                                           // output column: x of point k, or y of point k - 5
                lm_out[o * 10 + k] = idx < (unsigned)N ? lmk[((int64_t)b * N + idx) * 10 + (k < 5 ? 2 * k : 2 * (k - 5) + 1)] : 0.f;   // as the gather
            }
        }
        ++kept;
        __syncthreads();
    }
    if (tid == 0) nkeep[b] = kept;
}

static int rf_levels(RetinaDecodeParams& p, int bs, int H, int W) {
    p.bs = bs; p.H = H; p.W = W;
    int pos = 0;
    for (int l = 0; l < 3; ++l) {
        const int step = 8 << l;
        p.lh[l] = cdiv(H, step); p.lw[l] = cdiv(W, step); p.pos0[l] = pos;
        pos += p.lh[l] * p.lw[l];
    }
    p.N = 2 * pos;
    return p.N;
}

}  // namespace e4s

using namespace e4s;

extern "C" int e4s_retina_input(float* out, const uint8_t* img_u8, int bgr, int bs, int H, int W, void* stream) {
    E4S_REQUIRE(bs >= 0 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384 && (bgr == 0 || bgr == 1), "retina_input: bad size, or bgr is not 0 or 1");
    if (bs == 0) return 0;
    E4S_REQUIRE(out && img_u8, "retina_input: null tensor");
    const int64_t hw = (int64_t)H * W, n = bs * hw;
    hipStream_t st = (hipStream_t)stream;
    if (hw % 4 == 0 && rf_al16(out) && (((uintptr_t)img_u8) & 3) == 0)
        hipLaunchKernelGGL(retina_input_kernel<4>, dim3(grid_1d(n / 4)), dim3(256), 0, st, out, img_u8, bgr, n / 4, hw);
    else
        hipLaunchKernelGGL(retina_input_kernel<1>, dim3(grid_1d(n)), dim3(256), 0, st, out, img_u8, bgr, n, hw);
    return check_launch("retina_input");
}

extern "C" int e4s_retina_up_add(float* out, const float* a, const float* b, int planes, int h, int w, int hb, int wb, void* stream) {
    E4S_REQUIRE(planes >= 0 && h >= 1 && w >= 1 && hb >= 1 && wb >= 1 && h <= 16384 && w <= 16384 && hb <= 16384 && wb <= 16384, "retina_up_add: bad size");
    if (planes == 0) return 0;
    E4S_REQUIRE(out && a && b, "retina_up_add: null tensor");
    const float sy = (float)hb / (float)h, sx = (float)wb / (float)w;            // ATen's compute_scales_value without a scale factor: (float)in / out
    const int64_t n = (int64_t)planes * h * w;
    hipStream_t st = (hipStream_t)stream;
    if (w % 4 == 0 && rf_al16(out, a))
        hipLaunchKernelGGL(retina_up_add_kernel<4>, dim3(grid_1d(n / 4)), dim3(256), 0, st, out, a, b, n / 4, h, w, hb, wb, sy, sx);
    else
        hipLaunchKernelGGL(retina_up_add_kernel<1>, dim3(grid_1d(n)), dim3(256), 0, st, out, a, b, n, h, w, hb, wb, sy, sx);
    return check_launch("retina_up_add");
}

extern "C" int e4s_retina_cat_relu(float* out, const float* a, const float* b, const float* c, int bs, int ca, int cb, int cc, int hw, void* stream) {
    E4S_REQUIRE(bs >= 0 && ca >= 1 && cb >= 1 && cc >= 1 && hw >= 1 && ca + cb + cc <= 65536, "retina_cat_relu: bad size");
    if (bs == 0) return 0;
    E4S_REQUIRE(out && a && b && c, "retina_cat_relu: null tensor");
    const int64_t n = (int64_t)bs * (ca + cb + cc) * hw;
    hipStream_t st = (hipStream_t)stream;
    if (hw % 4 == 0 && rf_al16(out, a, b, c))
        hipLaunchKernelGGL(retina_cat_relu_kernel<4>, dim3(grid_1d(n / 4)), dim3(256), 0, st, out, a, b, c, n / 4, ca, cb, cc, hw);
    else
        hipLaunchKernelGGL(retina_cat_relu_kernel<1>, dim3(grid_1d(n)), dim3(256), 0, st, out, a, b, c, n, ca, cb, cc, hw);
    return check_launch("retina_cat_relu");
}

extern "C" int e4s_retina_priors(float* out, int H, int W, void* stream) {
    E4S_REQUIRE(out && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "retina_priors: null tensor or bad size");
    RetinaDecodeParams p;
    rf_levels(p, 1, H, W);
    hipLaunchKernelGGL(retina_priors_kernel, dim3(grid_1d(p.N)), dim3(256), 0, (hipStream_t)stream, out, p);
    return check_launch("retina_priors");
}

extern "C" int e4s_retina_decode(float* loc, float* conf, float* landms, float* score, float* boxes, float* lmk, const float* head0, const float* head1,
                                 const float* head2, int bs, int H, int W, void* stream) {
    E4S_REQUIRE(bs >= 0 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "retina_decode: bad size");
    if (bs == 0) return 0;
    E4S_REQUIRE(head0 && head1 && head2, "retina_decode: null head map");
    E4S_REQUIRE((loc != nullptr) == (conf != nullptr) && (loc != nullptr) == (landms != nullptr), "retina_decode: loc, conf and landms go together");
    E4S_REQUIRE((score != nullptr) == (boxes != nullptr) && (score != nullptr) == (lmk != nullptr), "retina_decode: score, boxes and lmk go together");
    E4S_REQUIRE(loc || score, "retina_decode: nothing to write");
    RetinaDecodeParams p;
    rf_levels(p, bs, H, W);
    p.head[0] = head0; p.head[1] = head1; p.head[2] = head2;
    p.loc = loc; p.conf = conf; p.landms = landms; p.score = score; p.boxes = boxes; p.lmk = lmk;
    const int64_t n = (int64_t)bs * (p.N / 2);
    hipStream_t st = (hipStream_t)stream;
    // a position's rows start at multiples of 32, 16 and 80 bytes: aligned whenever the tensors are
    if (rf_al16(loc, conf, landms) && rf_al16(boxes, lmk))
        hipLaunchKernelGGL(retina_decode_kernel<true>, dim3(grid_1d(n)), dim3(256), 0, st, p);
    else
        hipLaunchKernelGGL(retina_decode_kernel<false>, dim3(grid_1d(n)), dim3(256), 0, st, p);
    return check_launch("retina_decode");
}

extern "C" int e4s_retina_compact(int64_t* keys, int* counts, const float* score, int bs, int N, int cap, float threshold, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && N >= 1 && cap >= 1 && cap <= RF_MAX_CAP, "retina_compact: bad size (at most %d candidates an image)", RF_MAX_CAP);
    E4S_REQUIRE(threshold >= 0.f, "retina_compact: the threshold is a score, not below 0");
    if (bs == 0) return 0;
    E4S_REQUIRE(keys && counts && score, "retina_compact: null tensor");
    hipLaunchKernelGGL(retina_compact_kernel, dim3(bs), dim3(RF_CT), 0, (hipStream_t)stream, reinterpret_cast<long long*>(keys), counts, score, N, cap, threshold);
    return check_launch("retina_compact");
}

extern "C" int e4s_retina_nms(float* dets, float* landms_out, int* keep, int* nkeep, float* cbox, int64_t* sorted_keys, const int* counts,
                              const float* boxes, const float* lmk, int bs, int N, int cap, int keep_top_k, float nms_threshold, void* stream) {
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && N >= 1 && cap >= 1 && cap <= RF_MAX_CAP && keep_top_k >= 1, "retina_nms: bad size (at most %d candidates an image)",
                RF_MAX_CAP);
    if (bs == 0) return 0;
    E4S_REQUIRE(dets && landms_out && keep && nkeep && cbox && sorted_keys && counts && boxes && lmk, "retina_nms: null tensor");
    E4S_REQUIRE(rf_al16(cbox), "retina_nms: the candidate workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)bs * cap;
    const long long* kp = reinterpret_cast<const long long*>(sorted_keys);
    hipLaunchKernelGGL(retina_gather_kernel, dim3(grid_1d(n)), dim3(256), 0, st, cbox, kp, counts, boxes, n, N, cap);
    hipLaunchKernelGGL(retina_nms_kernel, dim3(bs), dim3(RF_CT), 0, st, dets, landms_out, keep, nkeep, cbox, kp, counts, lmk, N, cap, keep_top_k, nms_threshold);
    return check_launch("retina_nms");
}
