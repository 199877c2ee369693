// Row f15: GPEN face enhancement, stage 4 — everything FaceEnhancement.process(aligned=False) (swap_face_fine/gpen/face_enhancement.py:68-108, align_faces.py)
// does between its three networks: the 5-point similarity pair per face, cv2.warpAffine to the S x S crop, the 3 x 3 smoothing of small faces, mask_postprocess
// (border + two Gaussian blurs), and the paste — the two warpAffine back to the frame, the "largest mask wins" composition and the blend — in one pass over the frame.
// The arithmetic is OpenCV's, as tests/gpen_paste_model.py restates it: warpAffine's fixed-point map (10 fractional bits, sampled on a 1/32 grid), integer bilinear
// weights for uint8, float32 ones for the mask, float64 blurs.  No host synchronisation, no atomics, grids from shapes and counts alone.
#include <math.h>

#include "common.h"

// Every rounding of the model is one operation here: an FMA would round once where OpenCV and numpy round twice.
#pragma clang fp contract(off)

using namespace e4s;

namespace {

constexpr int kSkip = 1, kSmall = 2;           // the face flags (bits)
constexpr int kPx = 4;                         // pixels per lane: 12 bytes = three aligned dword stores
constexpr int kBlockX = 64, kBlockY = 4;
constexpr int kMaxTaps = 129;                  // the blur's column tile, (32 + k - 1) x 32 doubles, must fit 64 KB of LDS

// round half to even to int32, saturating; NaN goes to INT_MIN
__device__ __forceinline__ int rne_sat(double v) {
    v = rint(v);
    if (!(v > -2147483648.0)) return INT_MIN;
    if (v >= 2147483647.0) return INT_MAX;
    return (int)v;
}
__device__ __forceinline__ int add_wrap(int a, int b) { return (int)((unsigned)a + (unsigned)b); }

// cv2.warpAffine's inverted map in fixed point.  m: the 2 x 3 matrix as given (destination <- source is its inverse).
struct AffineMap {
    double m0, m1, m2, m3, m4, m5;
    __device__ __forceinline__ void invert_from(const double* __restrict__ M) {
        const double a0 = M[0], a1 = M[1], a2 = M[2], a3 = M[3], a4 = M[4], a5 = M[5];
        double D = a0 * a4 - a1 * a3;
        D = D != 0.0 ? 1.0 / D : 0.0;
        const double A11 = a4 * D, A22 = a0 * D;
        m0 = A11;
        m1 = a1 * -D;
        m3 = a3 * -D;
        m4 = A22;
        m2 = -m0 * a2 - m1 * a5;
        m5 = -m3 * a2 - m4 * a5;
    }
    // row y: X0, Y0 (with the + 16 rounding offset of the 1/32 grid)
    __device__ __forceinline__ void row(int y, int& X0, int& Y0) const {
        X0 = add_wrap(rne_sat((m1 * (double)y + m2) * 1024.0), 16);
        Y0 = add_wrap(rne_sat((m4 * (double)y + m5) * 1024.0), 16);
    }
    // column x of that row: the source pixel (sx, sy) and the 1/32 fractions (ax, ay)
    __device__ __forceinline__ void at(int X0, int Y0, int x, int& sx, int& sy, int& ax, int& ay) const {
        const int X = add_wrap(X0, rne_sat(m0 * (double)x * 1024.0)) >> 5;
        const int Y = add_wrap(Y0, rne_sat(m3 * (double)x * 1024.0)) >> 5;
        sx = X >> 5;
        sy = Y >> 5;
        ax = X & 31;
        ay = Y & 31;
    }
};

// true when at least one of the taps (sy, sx) .. (sy + 1, sx + 1) lies inside h x w
__device__ __forceinline__ bool touches(int sx, int sy, int w, int h) { return sx >= -1 && sx < w && sy >= -1 && sy < h; }

// the uint8 bilinear sample of an RGB image h x w at (sx, sy) + (ax, ay) / 32; the caller has checked touches()
__device__ __forceinline__ void sample_u8(const uint8_t* __restrict__ src, int w, int h, int sx, int sy, int ax, int ay, uint8_t* px) {
    const bool x0 = sx >= 0, x1 = sx + 1 < w, y0 = sy >= 0, y1 = sy + 1 < h;
    const int w00 = (32 - ax) * (32 - ay), w01 = ax * (32 - ay), w10 = (32 - ax) * ay, w11 = ax * ay;
    const uint8_t* r0 = src + ((size_t)(y0 ? sy : 0) * w + (x0 ? sx : 0)) * 3;       // clamped: never dereferenced where the tap is outside
    const uint8_t* r1 = src + ((size_t)(y1 ? sy + 1 : 0) * w + (x0 ? sx : 0)) * 3;
    const int dx = (x0 && x1) ? 3 : 0;                                                // x0 false: the pointer already stands on column sx + 1 = 0
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v00 = (y0 && x0) ? r0[c] : 0, v01 = (y0 && x1) ? r0[dx + c] : 0;
        const int v10 = (y1 && x0) ? r1[c] : 0, v11 = (y1 && x1) ? r1[dx + c] : 0;
        px[c] = (uint8_t)((v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11 + 512) >> 10);
    }
}

// the float32 bilinear sample of a plane h x w
__device__ __forceinline__ float sample_f32(const float* __restrict__ src, int w, int h, int sx, int sy, int ax, int ay) {
    const bool x0 = sx >= 0, x1 = sx + 1 < w, y0 = sy >= 0, y1 = sy + 1 < h;
    const float fx = (float)ax / 32.f, fy = (float)ay / 32.f;
    const float w0 = (1.f - fx) * (1.f - fy), w1 = fx * (1.f - fy), w2 = (1.f - fx) * fy, w3 = fx * fy;
    const float* r0 = src + (size_t)(y0 ? sy : 0) * w + (x0 ? sx : 0);
    const float* r1 = src + (size_t)(y1 ? sy + 1 : 0) * w + (x0 ? sx : 0);
    const int dx = (x0 && x1) ? 1 : 0;
    const float v00 = (y0 && x0) ? r0[0] : 0.f, v01 = (y0 && x1) ? r0[dx] : 0.f;
    const float v10 = (y1 && x0) ? r1[0] : 0.f, v11 = (y1 && x1) ? r1[dx] : 0.f;
    return ((v00 * w0 + v01 * w1) + v10 * w2) + v11 * w3;
}

// 12 bytes of 4 pixels: three dword stores when the address allows and all four are there, else byte stores of the first `count` pixels.
__device__ __forceinline__ void store_px4(uint8_t* dst, const uint8_t (&px)[12], int count) {
    if (count == kPx && ((uintptr_t)dst & 3u) == 0) {
        uint32_t* d = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            d[j] = (uint32_t)px[4 * j] | ((uint32_t)px[4 * j + 1] << 8) | ((uint32_t)px[4 * j + 2] << 16) | ((uint32_t)px[4 * j + 3] << 24);
        return;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k)
        if (k < 3 * count) dst[k] = px[k];
}
__device__ __forceinline__ void load_px4(const uint8_t* src, uint8_t (&px)[12], int count) {
    if (count == kPx && ((uintptr_t)src & 3u) == 0) {
        const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint32_t v = s[j];
            px[4 * j] = (uint8_t)v, px[4 * j + 1] = (uint8_t)(v >> 8), px[4 * j + 2] = (uint8_t)(v >> 16), px[4 * j + 3] = (uint8_t)(v >> 24);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) px[k] = k < 3 * count ? src[k] : 0;
}

// ------------------------------------------------------------------------------------------------ the transforms: one lane per face
__global__ __launch_bounds__(64) void face_transforms_kernel(double* __restrict__ T, int* __restrict__ flags, const float* __restrict__ dets,
                                                             const float* __restrict__ landms, const double* __restrict__ ref, float threshold, float small_face,
                                                             int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float* d = dets + (size_t)i * 5;
    int flag = 0;
    if (d[4] < threshold) flag |= kSkip;
    const float fh = d[3] - d[1], fw = d[2] - d[0];
    if ((fh < fw ? fh : fw) < small_face) flag |= kSmall;                     // numpy's min: fh unless fw is smaller
    const float* l = landms + (size_t)i * 10;
    double sx[5], sy[5], dx[5], dy[5];
    bool finite = true;
    double smx = 0, smy = 0, dmx = 0, dmy = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        sx[k] = (double)l[k];
        sy[k] = (double)l[5 + k];
        dx[k] = (double)(float)ref[2 * k];
        dy[k] = (double)(float)ref[2 * k + 1];
        finite = finite && isfinite(sx[k]) && isfinite(sy[k]);
        smx += sx[k], smy += sy[k], dmx += dx[k], dmy += dy[k];
    }
    smx /= 5, smy /= 5, dmx /= 5, dmy /= 5;
    double a = 0, b = 0, var = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double px = sx[k] - smx, py = sy[k] - smy, qx = dx[k] - dmx, qy = dy[k] - dmy;
        a += px * qx + py * qy;
        b += px * qy - py * qx;
        var += px * px + py * py;
    }
    double* t = T + (size_t)i * 12;
    if (!finite || var == 0.0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) t[k] = 0.0;
        flags[i] = flag | kSkip;
        return;
    }
    const double r00 = a / var, r01 = -b / var, r10 = b / var, r11 = a / var;
    t[0] = r00, t[1] = r01, t[2] = dmx - (r00 * smx + r01 * smy);
    t[3] = r10, t[4] = r11, t[5] = dmy - (r10 * smx + r11 * smy);
    const double h = hypot(a, b), den = h * (h / var);
    const double i00 = a / den, i01 = b / den, i10 = -b / den, i11 = a / den;
    t[6] = i00, t[7] = i01, t[8] = smx - (i00 * dmx + i01 * dmy);
    t[9] = i10, t[10] = i11, t[11] = smy - (i10 * dmx + i11 * dmy);
    flags[i] = flag;
}

// ------------------------------------------------------------------------------------------------ warpAffine of the frame to the S x S crop, per face
__global__ __launch_bounds__(kBlockX* kBlockY) void warp_crop_kernel(uint8_t* __restrict__ out, const uint8_t* __restrict__ frames,
                                                                     const int* __restrict__ frame_of_face, const double* __restrict__ T, int bs, int H, int W,
                                                                     int S) {
    const int f = blockIdx.z;
    const int y = blockIdx.y * kBlockY + threadIdx.y;
    const int x4 = (blockIdx.x * kBlockX + threadIdx.x) * kPx;
    if (y >= S || x4 >= S) return;
    const int b = frame_of_face[f];
    const bool has_frame = b >= 0 && b < bs;                                   // a bad index reads nothing: the crop is zero
    const uint8_t* src = frames + (size_t)(has_frame ? b : 0) * H * W * 3;
    AffineMap map;
    map.invert_from(T + (size_t)f * 12);
    int X0, Y0;
    map.row(y, X0, Y0);
    uint8_t px[12];
    const int count = S - x4 < kPx ? S - x4 : kPx;
#pragma unroll
    for (int k = 0; k < kPx; ++k) {
        int sx, sy, ax, ay;
        map.at(X0, Y0, x4 + k, sx, sy, ax, ay);
        if (k < count && has_frame && touches(sx, sy, W, H))
            sample_u8(src, W, H, sx, sy, ax, ay, px + 3 * k);
        else
            px[3 * k] = px[3 * k + 1] = px[3 * k + 2] = 0;
    }
    store_px4(out + (((size_t)f * S + y) * S + x4) * 3, px, count);
}

// ------------------------------------------------------------------------------------------------ the 3 x 3 binomial filter of the small faces
// BORDER_REFLECT_101 for an overhang below n; an axis of one pixel reflects onto itself (cv::borderInterpolate)
__device__ __forceinline__ int reflect101(int i, int n) { return n == 1 ? 0 : (i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i)); }

__global__ __launch_bounds__(kBlockX* kBlockY) void smooth3_kernel(uint8_t* __restrict__ out, const uint8_t* __restrict__ in, const int* __restrict__ flags,
                                                                   int S) {
    const int f = blockIdx.z;
    const int y = blockIdx.y * kBlockY + threadIdx.y;
    const int x4 = (blockIdx.x * kBlockX + threadIdx.x) * kPx;
    if (y >= S || x4 >= S) return;
    const int count = S - x4 < kPx ? S - x4 : kPx;
    const uint8_t* src = in + (size_t)f * S * S * 3;
    uint8_t px[12];
    if (!(flags[f] & kSmall)) {
        load_px4(src + ((size_t)y * S + x4) * 3, px, count);
    } else {
        const int ry[3] = {reflect101(y - 1, S), y, reflect101(y + 1, S)};
#pragma unroll
        for (int k = 0; k < kPx; ++k) {
            const int x = x4 + k < S ? x4 + k : S - 1;
            const int rx[3] = {reflect101(x - 1, S), x, reflect101(x + 1, S)};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                int s = 0;
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int i = 0; i < 3; ++i) s += (j == 1 ? 2 : 1) * (i == 1 ? 2 : 1) * (int)src[((size_t)ry[j] * S + rx[i]) * 3 + c];
                px[3 * k + c] = (uint8_t)((s + 7 + ((s >> 4) & 1)) >> 4);       // s / 16 rounded half to even
            }
        }
    }
    store_px4(out + (((size_t)f * S + y) * S + x4) * 3, px, count);
}

// ------------------------------------------------------------------------------------------------ mask_postprocess: border + two separable Gaussian blurs, float64
// One pass of a blur along x (VERT = false) or y (VERT = true): a TW x TH output tile with its k - 1 halo along the filtered axis lies in LDS as doubles; the taps
// are read with a uniform index (scalar loads).  FIRST reads the uint8 mask / 255 with the border of `thres` zeroed; LAST writes float32.
constexpr int kRowTW = 128, kRowTH = 4, kColTW = 32, kColTH = 32;

template <bool VERT, bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void blur_pass_kernel(void* __restrict__ out_v, const void* __restrict__ in_v, const double* __restrict__ taps, int S, int k,
                                                        int thres) {
    extern __shared__ double tile[];
    constexpr int TW = VERT ? kColTW : kRowTW, TH = VERT ? kColTH : kRowTH;
    const int r = k / 2;
    const int LW = VERT ? TW : TW + k - 1, LH = VERT ? TH + k - 1 : TH;
    const int f = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const size_t plane = (size_t)f * S * S;
    for (int e = threadIdx.x; e < LW * LH; e += 256) {
        const int ly = e / LW, lx = e - ly * LW;
        int gx = x0 + lx - (VERT ? 0 : r), gy = y0 + ly - (VERT ? r : 0);
        double v = 0.0;
        if ((VERT ? gx : gy) < S) {                                            // the unfiltered axis has no halo: past the plane nothing is needed
            gx = VERT ? gx : reflect101(gx, S);
            gy = VERT ? reflect101(gy, S) : gy;
            if (gx >= 0 && gx < S && gy >= 0 && gy < S) {                       // (a tile past the plane along the filtered axis reflects out of range)
                if (FIRST) {
                    const bool border = gx < thres || gx >= S - thres || gy < thres || gy >= S - thres;
                    v = border ? 0.0 : (double)static_cast<const uint8_t*>(in_v)[plane + (size_t)gy * S + gx] / 255.0;
                } else {
                    v = static_cast<const double*>(in_v)[plane + (size_t)gy * S + gx];
                }
            }
        }
        tile[e] = v;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < TW * TH; e += 256) {
        const int ty = e / TW, tx = e - ty * TW;
        const int gx = x0 + tx, gy = y0 + ty;
        if (gx >= S || gy >= S) continue;
        const double* p = tile + ty * LW + tx;
        const int step = VERT ? LW : 1;
        double acc = 0.0;
        for (int i = 0; i < k; ++i) acc += taps[i] * p[i * step];
        if (LAST)
            static_cast<float*>(out_v)[plane + (size_t)gy * S + gx] = (float)acc;
        else
            static_cast<double*>(out_v)[plane + (size_t)gy * S + gx] = acc;
    }
}

// ------------------------------------------------------------------------------------------------ the paste: one pass over the frame
// A lane owns 4 adjacent pixels of a frame row and walks its frame's faces in detector order.  Per face: the fixed-point source coordinate; nothing more when all
// four taps are outside (the warped mask is 0 there and 0 - full_mask > 0 never holds: full_mask starts at 0 and only grows); else the float32 mask sample, the
// comparison with the running maximum, and the uint8 face sample only where it wins.  The face's matrix, flag and planes are the same for the whole workgroup.
// A lane reads its own pixels of `base` before it writes them to `out`, and no other lane touches them: out may be base.
__global__ __launch_bounds__(kBlockX* kBlockY) void paste_kernel(uint8_t* out, float* __restrict__ full_mask, const uint8_t* base,
                                                                 const uint8_t* __restrict__ faces, const float* __restrict__ masks, const double* __restrict__ T,
                                                                 const int* __restrict__ flags, const int* __restrict__ face_begin, int n, int H, int W, int S) {
    const int b = blockIdx.z;
    const int y = blockIdx.y * kBlockY + threadIdx.y;
    const int x4 = (blockIdx.x * kBlockX + threadIdx.x) * kPx;
    if (y >= H || x4 >= W) return;
    const int count = W - x4 < kPx ? W - x4 : kPx;
    int first = face_begin[b], last = face_begin[b + 1];
    first = first < 0 ? 0 : first;                                             // a bad offset reads no face outside [0, n)
    last = last > n ? n : last;
    float fm[kPx] = {0.f, 0.f, 0.f, 0.f};
    uint8_t fi[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int f = first; f < last; ++f) {
        if (flags[f] & kSkip) continue;
        AffineMap map;
        map.invert_from(T + (size_t)f * 12 + 6);
        int X0, Y0;
        map.row(y, X0, Y0);
        const float* __restrict__ mp = masks + (size_t)f * S * S;
        const uint8_t* __restrict__ fp = faces + (size_t)f * S * S * 3;
#pragma unroll
        for (int k = 0; k < kPx; ++k) {
            int sx, sy, ax, ay;
            map.at(X0, Y0, x4 + k, sx, sy, ax, ay);
            if (!touches(sx, sy, S, S)) continue;
            const float m = sample_f32(mp, S, S, sx, sy, ax, ay);
            if (m - fm[k] > 0.f) {
                fm[k] = m;
                sample_u8(fp, S, S, sx, sy, ax, ay, fi + 3 * k);
            }
        }
    }
    const size_t o = ((size_t)b * H + y) * W + x4;
    uint8_t px[12];
    load_px4(base + o * 3, px, count);
#pragma unroll
    for (int k = 0; k < kPx; ++k) {
        const float m = fm[k], om = 1.f - m;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float lo = (float)px[3 * k + c] * om, hi = (float)fi[3 * k + c] * m;
            const float s = fabsf(lo + hi);
            px[3 * k + c] = (uint8_t)fminf(rintf(s), 255.f);                   // NaN: fminf returns 255
        }
        if (full_mask && k < count) full_mask[o + k] = m;
    }
    store_px4(out + o * 3, px, count);
}

int check_faces(const char* what, int n, int S) {
    E4S_REQUIRE(n >= 0 && n <= 65535, "%s: n = %d faces (0 .. 65535)", what, n);
    E4S_REQUIRE(S >= 1 && S <= 4096, "%s: face size %d (1 .. 4096)", what, S);
    return 0;
}
int check_frames(const char* what, int bs, int H, int W) {
    E4S_REQUIRE(bs >= 1 && bs <= 65535, "%s: bs = %d frames (1 .. 65535)", what, bs);
    E4S_REQUIRE(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "%s: bad frame size %d x %d (1 .. 32768)", what, H, W);
    return 0;
}
int check_blur(const char* what, int S, int k, int thres) {
    E4S_REQUIRE(k >= 1 && (k & 1) && k <= kMaxTaps, "%s: %d taps: an odd number in 1 .. %d", what, k, kMaxTaps);
    E4S_REQUIRE(k / 2 < S, "%s: %d taps reach %d pixels past a %d wide mask: reflection needs k / 2 < S", what, k, k / 2, S);
    E4S_REQUIRE(thres >= 1, "%s: thres = %d (must be >= 1)", what, thres);
    return 0;
}

}  // namespace

extern "C" int e4s_gpen_face_transforms(void* transforms, int* flags, const float* dets, const float* landms, const void* ref_points, float threshold,
                                        float small_face, int n, void* stream) {
    E4S_REQUIRE(n >= 0, "gpen_face_transforms: n = %d", n);
    if (n == 0) return 0;
    E4S_REQUIRE(transforms && flags && dets && landms && ref_points, "gpen_face_transforms: null pointer");
    hipLaunchKernelGGL(face_transforms_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, static_cast<double*>(transforms), flags, dets, landms,
                       static_cast<const double*>(ref_points), threshold, small_face, n);
    return check_launch("gpen_face_transforms");
}

extern "C" int e4s_gpen_warp_crop_u8(uint8_t* out, const uint8_t* frames, const int* frame_of_face, const void* transforms, int n, int bs, int H, int W, int S,
                                     void* stream) {
    if (int st = check_faces("gpen_warp_crop_u8", n, S)) return st;
    if (int st = check_frames("gpen_warp_crop_u8", bs, H, W)) return st;
    if (n == 0) return 0;
    E4S_REQUIRE(out && frames && frame_of_face && transforms, "gpen_warp_crop_u8: null pointer");
    hipLaunchKernelGGL(warp_crop_kernel, dim3(cdiv(S, kBlockX * kPx), cdiv(S, kBlockY), n), dim3(kBlockX, kBlockY), 0, (hipStream_t)stream, out, frames,
                       frame_of_face, static_cast<const double*>(transforms), bs, H, W, S);
    return check_launch("gpen_warp_crop_u8");
}

extern "C" int e4s_gpen_smooth3_u8(uint8_t* out, const uint8_t* faces, const int* flags, int n, int S, void* stream) {
    if (int st = check_faces("gpen_smooth3_u8", n, S)) return st;
    if (n == 0) return 0;
    E4S_REQUIRE(out && faces && flags, "gpen_smooth3_u8: null pointer");
    E4S_REQUIRE(out != faces, "gpen_smooth3_u8: out must not be faces (a 3 x 3 filter reads its neighbours)");
    hipLaunchKernelGGL(smooth3_kernel, dim3(cdiv(S, kBlockX * kPx), cdiv(S, kBlockY), n), dim3(kBlockX, kBlockY), 0, (hipStream_t)stream, out, faces, flags, S);
    return check_launch("gpen_smooth3_u8");
}

extern "C" int e4s_gpen_mask_feather_scratch_bytes(int n, int S, int64_t* bytes) {
    E4S_REQUIRE(bytes, "gpen_mask_feather_scratch_bytes: null result");
    if (int st = check_faces("gpen_mask_feather_scratch_bytes", n, S)) return st;
    *bytes = 2 * (int64_t)n * S * S * 8;
    return 0;
}

extern "C" int e4s_gpen_mask_feather(float* out, const uint8_t* masks, const void* taps, void* scratch, int n, int S, int k, int thres, void* stream) {
    if (int st = check_faces("gpen_mask_feather", n, S)) return st;
    if (int st = check_blur("gpen_mask_feather", S, k, thres)) return st;
    if (n == 0) return 0;
    E4S_REQUIRE(out && masks && taps && scratch, "gpen_mask_feather: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const double* t = static_cast<const double*>(taps);
    double* a = static_cast<double*>(scratch);
    double* b = a + (size_t)n * S * S;
    const dim3 grow(cdiv(S, kRowTW), cdiv(S, kRowTH), n), gcol(cdiv(S, kColTW), cdiv(S, kColTH), n);
    const size_t lrow = (size_t)(kRowTW + k - 1) * kRowTH * 8, lcol = (size_t)(kColTH + k - 1) * kColTW * 8;
    hipLaunchKernelGGL((blur_pass_kernel<false, true, false>), grow, dim3(256), lrow, st, a, masks, t, S, k, thres);
    hipLaunchKernelGGL((blur_pass_kernel<true, false, false>), gcol, dim3(256), lcol, st, b, a, t, S, k, thres);
    hipLaunchKernelGGL((blur_pass_kernel<false, false, false>), grow, dim3(256), lrow, st, a, b, t, S, k, thres);
    hipLaunchKernelGGL((blur_pass_kernel<true, false, true>), gcol, dim3(256), lcol, st, out, a, t, S, k, thres);
    return check_launch("gpen_mask_feather");
}

extern "C" int e4s_gpen_paste_u8(uint8_t* out, float* full_mask, const uint8_t* base, const uint8_t* faces, const float* masks, const void* transforms,
                                 const int* flags, const int* face_begin, int n, int bs, int H, int W, int S, void* stream) {
    if (int st = check_faces("gpen_paste_u8", n, S)) return st;
    if (int st = check_frames("gpen_paste_u8", bs, H, W)) return st;
    E4S_REQUIRE(out && base, "gpen_paste_u8: null pointer");
    if (n == 0) {                                                              // no face anywhere: the frames come back as they are, without a kernel
        const size_t px = (size_t)bs * H * W;
        if (out != base && hipMemcpyAsync(out, base, px * 3, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return check_launch("gpen_paste_u8");
        if (full_mask && hipMemsetAsync(full_mask, 0, px * 4, (hipStream_t)stream) != hipSuccess) return check_launch("gpen_paste_u8");
        return 0;
    }
    E4S_REQUIRE(faces && masks && transforms && flags && face_begin, "gpen_paste_u8: null pointer");
    hipLaunchKernelGGL(paste_kernel, dim3(cdiv(W, kBlockX * kPx), cdiv(H, kBlockY), bs), dim3(kBlockX, kBlockY), 0, (hipStream_t)stream, out, full_mask, base,
                       faces, masks, static_cast<const double*>(transforms), flags, face_begin, n, H, W, S);
    return check_launch("gpen_paste_u8");
}
