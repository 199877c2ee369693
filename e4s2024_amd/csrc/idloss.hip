// ArcFace IR-SE50 identity loss (criteria/id_loss.py + models/encoders/model_irse.py::Backbone(112, 50, 'ir_se') + helpers.py::bottleneck_IR_SE) —
// the parts of its forward pass and of its gradient with respect to the input image that the existing kernels do not cover:
//   resample   the pool -> crop -> pool pre-processing of IDLoss.extract_feats as a separable banded operator out = A_y X A_x^T (A built on the host
//              from PyTorch's adaptive-pool windows), and its adjoint (the gradient lands on the full input, zero outside the crop)
//   affine     y = x * scale[c] + shift[c], optionally followed by PReLU: a residual branch's input BatchNorm in scale / shift form (exact for gamma = 0)
//              and the PReLU after its first convolution (whose pre-activation is kept for the backward)
//   prelu bwd  g * (pre > 0 ? 1 : slope[c]) from the kept pre-activation, optionally reading a cropped window of a larger source (the
//              [2h+1]^2 output of the stride-2 transposed convolution, offset 1 = the forward's padding)
//   SE bwd     s[b,c] = sum_hw g r in a fixed order; v = (1/HW) fc1^T (relu' . fc2^T (sigmoid' . s)) in one launch per batch; dr = g gate + v
//   scatter    gx[2y, 2x] += src[y, x]: the backward of MaxPool2d(1, 2) and of the 1x1 stride-2 shortcut convolution (after its stride-1 data gradient)
//   linear     the output layer (BN2d, Linear, BN1d folded on the host) and its transpose for the gradient; HBM-bound GEMVs, fixed-order sums
//   heads      per tap: |x|^2, |y|^2, x.y as per-block partials, summed by one workgroup into the loss, the similarity improvement and the per-sample
//              (|x|, |y|, cos) the backward needs; gx = -gout / bs (y/|y| - cos x/|x|) / |x|
// No float atomics anywhere: the same inputs give the same bits.  Convolutions run on conv.hip (e4s_conv2d_sb3 forward, e4s_conv2d_sb data gradients
// of the stride-1 3x3 / 1x1 convolutions on flipped, transposed weights) and the stride-2 3x3 data gradient on modconv_sb.hip's transposed convolution
// (e4s_modconv_tconv_sb: split-bf16 at 1x the MACs, no zero insertion).
#include "common.h"
#include "targets.h"

using namespace e4s;

namespace {

int grid_for(int64_t n) { return (int)(cdiv64(n, 256) < 65536 ? cdiv64(n, 256) : 65536); }

// block sum of 256 values in a fixed order (LDS tree)
__device__ __forceinline__ float bsum256(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// out[p, i, j] = sum_y ay[i, y] sum_x ax[j, x] x[p, y, x] over the nonzero bands rng_y[i] = [lo, hi), rng_x[j]
__global__ __launch_bounds__(256) void id_resample_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ ay,
                                                          const float* __restrict__ ax, const int* __restrict__ ry, const int* __restrict__ rx,
                                                          int64_t n, int h, int w, int no) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int j = (int)(e % no), i = (int)((e / no) % no);
        const int64_t p = e / ((int64_t)no * no);
        const float* xp = x + (size_t)p * h * w;
        const int y0 = ry[2 * i], y1 = ry[2 * i + 1], x0 = rx[2 * j], x1 = rx[2 * j + 1];
        float s = 0.f;
        for (int y = y0; y < y1; ++y) {
            float t = 0.f;
            for (int xx = x0; xx < x1; ++xx) t = fmaf(ax[(size_t)j * w + xx], xp[(size_t)y * w + xx], t);
            s = fmaf(ay[(size_t)i * h + y], t, s);
        }
        out[e] = s;
    }
}

// gx[p, y, x] (+)= sum_i ay[i, y] sum_j ax[j, x] g[p, i, j] over the column bands cy[y] = [lo, hi), cx[x] (empty outside the crop)
__global__ __launch_bounds__(256) void id_resample_adj_kernel(float* __restrict__ gx, const float* __restrict__ g, const float* __restrict__ ay,
                                                              const float* __restrict__ ax, const int* __restrict__ cy, const int* __restrict__ cx,
                                                              int64_t n, int h, int w, int no, int accumulate) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int xx = (int)(e % w), y = (int)((e / w) % h);
        const int64_t p = e / ((int64_t)h * w);
        const float* gp = g + (size_t)p * no * no;
        const int i0 = cy[2 * y], i1 = cy[2 * y + 1], j0 = cx[2 * xx], j1 = cx[2 * xx + 1];
        float s = 0.f;
        for (int i = i0; i < i1; ++i) {
            float t = 0.f;
            for (int j = j0; j < j1; ++j) t = fmaf(ax[(size_t)j * w + xx], gp[(size_t)i * no + j], t);
            s = fmaf(ay[(size_t)i * h + y], t, s);
        }
        gx[e] = accumulate ? gx[e] + s : s;
    }
}

__global__ __launch_bounds__(256) void id_affine_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, const float* __restrict__ slope, int64_t n, int C, int hw) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int c = (int)((e / hw) % C);
        float v = x[e];
        if (scale) v = fmaf(v, scale[c], shift[c]);
        if (slope) v = v > 0.f ? v : v * slope[c];
        out[e] = v;
    }
}

// g[p, y, x] = src[p, y + off, x + off] * (pre[p, y, x] > 0 ? 1 : slope[c]); src planes are sh x sw
__global__ __launch_bounds__(256) void id_prelu_bwd_kernel(float* __restrict__ g, const float* __restrict__ src, const float* __restrict__ pre,
                                                           const float* __restrict__ slope, int64_t n, int C, int h, int w, int sh, int sw, int off) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int xx = (int)(e % w), y = (int)((e / w) % h);
        const int64_t p = e / ((int64_t)h * w);
        const int c = (int)(p % C);
        const float v = src[((size_t)p * sh + y + off) * sw + xx + off];
        g[e] = pre[e] > 0.f ? v : v * slope[c];
    }
}

// s[p] = sum_hw g[p] r[p], one workgroup per plane, fixed order
__global__ __launch_bounds__(256) void id_se_dot_kernel(float* __restrict__ s, const float* __restrict__ g, const float* __restrict__ r, int hw) {
    __shared__ float red[256];
    const size_t base = (size_t)blockIdx.x * hw;
    float a = 0.f;
    for (int i = threadIdx.x; i < hw; i += 256) a = fmaf(g[base + i], r[base + i], a);
    a = bsum256(a, red);
    if (threadIdx.x == 0) s[blockIdx.x] = a;
}

// one workgroup per sample: a = s * gate (1 - gate); z = fc1 . pooled (recomputed); dz = (z > 0) fc2^T a; v = fc1^T dz / hw
// fc1 [H][C], fc2 [C][H]; C <= 1024, H <= 64
__global__ __launch_bounds__(256) void id_se_bwd_kernel(float* __restrict__ v, const float* __restrict__ s, const float* __restrict__ pooled,
                                                        const float* __restrict__ gate, const float* __restrict__ fc1, const float* __restrict__ fc2, int C,
                                                        int H, float inv_hw) {
    __shared__ float a[1024], pl[1024], dz[64];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int c = tid; c < C; c += 256) {
        const float gt = gate[(size_t)b * C + c];
        a[c] = s[(size_t)b * C + c] * (gt * (1.f - gt));
        pl[c] = pooled[(size_t)b * C + c];
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int hh = wave; hh < H; hh += 4) {       // one wave per hidden unit: z and fc2^T a, lane-strided then a fixed butterfly
        float z = 0.f, d = 0.f;
        for (int c = lane; c < C; c += 64) {
            z = fmaf(fc1[(size_t)hh * C + c], pl[c], z);
            d = fmaf(fc2[(size_t)c * H + hh], a[c], d);
        }
        z = wave_sum(z);
        d = wave_sum(d);
        if (lane == 0) dz[hh] = z > 0.f ? d : 0.f;
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        float t = 0.f;
        for (int hh = 0; hh < H; ++hh) t = fmaf(fc1[(size_t)hh * C + c], dz[hh], t);
        v[(size_t)b * C + c] = t * inv_hw;
    }
}

__global__ __launch_bounds__(256) void id_se_dr_kernel(float* __restrict__ dr, const float* __restrict__ g, const float* __restrict__ gate,
                                                       const float* __restrict__ v, int64_t n, int hw) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t p = e / hw;
        dr[e] = fmaf(g[e], gate[p], v[p]);
    }
}

// gx[p, 2y, 2x] += src[p, y, x]; src planes ho x wo, gx planes h x w
__global__ __launch_bounds__(256) void id_scatter_add_kernel(float* __restrict__ gx, const float* __restrict__ src, int64_t n, int h, int w, int ho, int wo) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int xx = (int)(e % wo), y = (int)((e / wo) % ho);
        const int64_t p = e / ((int64_t)ho * wo);
        gx[((size_t)p * h + 2 * y) * w + 2 * xx] += src[e];
    }
}

constexpr int LB = 4;          // samples per pass of the GEMVs

// y[b, n] = sum_k W[n, k] x[b, k] + bias[n]: one workgroup per output n, samples in passes of LB
__global__ __launch_bounds__(256) void id_linear_kernel(float* __restrict__ y, const float* __restrict__ x, const float* __restrict__ W,
                                                        const float* __restrict__ bias, int bs, int K, int N) {
    __shared__ float red[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* wr = W + (size_t)n * K;
    for (int b0 = 0; b0 < bs; b0 += LB) {
        float acc[LB];
#pragma unroll
        for (int q = 0; q < LB; ++q) acc[q] = 0.f;
        for (int k = tid; k < K; k += 256) {
            const float wv = wr[k];
#pragma unroll
            for (int q = 0; q < LB; ++q)
                if (b0 + q < bs) acc[q] = fmaf(wv, x[(size_t)(b0 + q) * K + k], acc[q]);
        }
#pragma unroll
        for (int q = 0; q < LB; ++q) {
            const float s = bsum256(acc[q], red);
            if (tid == 0 && b0 + q < bs) y[(size_t)(b0 + q) * N + n] = s + (bias ? bias[n] : 0.f);
        }
    }
}

// gx[b, k] = sum_n W[n, k] g[b, n]: a workgroup owns 64 consecutive k; its four waves take a quarter of the n each, summed in LDS in wave order
__global__ __launch_bounds__(256) void id_linear_t_kernel(float* __restrict__ gx, const float* __restrict__ g, const float* __restrict__ W, int bs, int K,
                                                          int N) {
    __shared__ float part[4][LB][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int k = blockIdx.x * 64 + lane;
    const int nq = (N + 3) / 4, n0 = wave * nq, n1 = min(N, n0 + nq);
    for (int b0 = 0; b0 < bs; b0 += LB) {
        float acc[LB];
#pragma unroll
        for (int q = 0; q < LB; ++q) acc[q] = 0.f;
        if (k < K) {
            for (int n = n0; n < n1; ++n) {
                const float wv = W[(size_t)n * K + k];
#pragma unroll
                for (int q = 0; q < LB; ++q)
                    if (b0 + q < bs) acc[q] = fmaf(wv, g[(size_t)(b0 + q) * N + n], acc[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < LB; ++q) part[wave][q][lane] = acc[q];
        __syncthreads();
        if (wave == 0 && k < K) {
#pragma unroll
            for (int q = 0; q < LB; ++q)
                if (b0 + q < bs) gx[(size_t)(b0 + q) * K + k] = ((part[0][q][lane] + part[1][q][lane]) + part[2][q][lane]) + part[3][q][lane];
        }
        __syncthreads();
    }
}

constexpr int HB = 8192;       // elements of one sample's feature per head workgroup

// part[(b * nblk + blk) * 3 + {0, 1, 2}] = sum |x|^2, |y|^2, x.y over the block's elements
__global__ __launch_bounds__(256) void id_head_partial_kernel(float* __restrict__ part, const float* __restrict__ fx, const float* __restrict__ fy, int64_t D) {
    __shared__ float red[256];
    const int blk = blockIdx.x, b = blockIdx.y, nblk = gridDim.x;
    const float* xp = fx + (size_t)b * D;
    const float* yp = fy + (size_t)b * D;
    const int64_t e0 = (int64_t)blk * HB, e1 = min<int64_t>(D, e0 + HB);
    float sxx = 0.f, syy = 0.f, sxy = 0.f;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
        const float u = xp[e], v = yp[e];
        sxx = fmaf(u, u, sxx);
        syy = fmaf(v, v, syy);
        sxy = fmaf(u, v, sxy);
    }
    sxx = bsum256(sxx, red);
    syy = bsum256(syy, red);
    sxy = bsum256(sxy, red);
    if (threadIdx.x == 0) {
        float* o = part + ((size_t)b * nblk + blk) * 3;
        o[0] = sxx; o[1] = syy; o[2] = sxy;
    }
}

// one workgroup: for each tap t < ntap and sample b, the partials in block order -> |x|, |y|, cos = x.y / (|x| |y|); stats[(t * bs + b) * 3] = (|x|, |y|, cos);
// loss_out[0] = sum_t mean_b (1 - cos), sim_out[0] = sum_t mean_b (cos - y.y / |y|^2) (IDLoss.forward's loss and sim_improvement)
__global__ __launch_bounds__(256) void id_head_sum_kernel(float* __restrict__ loss_out, float* __restrict__ sim_out, float* __restrict__ stats,
                                                          const float* __restrict__ part, int bs, int ntap,
                                                          int nb0, int nb1, int nb2, int nb3, int nb4) {
    __shared__ float red[256];
    const int nbs[5] = {nb0, nb1, nb2, nb3, nb4};
    float loss = 0.f, sim = 0.f;
    size_t off = 0;
    for (int t = 0; t < ntap; ++t) {
        const int nb = nbs[t];
        float lt = 0.f, st = 0.f;
        for (int b = 0; b < bs; ++b) {
            const float* pp = part + off + (size_t)b * nb * 3;
            float sxx = 0.f, syy = 0.f, sxy = 0.f;
            for (int i = threadIdx.x; i < nb; i += 256) {
                sxx += pp[3 * i];
                syy += pp[3 * i + 1];
                sxy += pp[3 * i + 2];
            }
            sxx = bsum256(sxx, red);
            syy = bsum256(syy, red);
            sxy = bsum256(sxy, red);
            const float nx = sqrtf(sxx), ny = sqrtf(syy);
            const float c = sxy / (nx * ny);
            if (threadIdx.x == 0) {
                stats[((size_t)t * bs + b) * 3] = nx;
                stats[((size_t)t * bs + b) * 3 + 1] = ny;
                stats[((size_t)t * bs + b) * 3 + 2] = c;
            }
            lt += 1.f - c;
            st += c - syy / (ny * ny);
        }
        loss += lt / (float)bs;
        sim += st / (float)bs;
        off += (size_t)bs * nb * 3;
    }
    if (threadIdx.x == 0) {
        loss_out[0] = loss;
        sim_out[0] = sim;
    }
}

// gx[b, k] (+)= -gout[0] scale (fy_k / |y| - cos fx_k / |x|) / |x| from the stats (|x|, |y|, cos) of the tap
__global__ __launch_bounds__(256) void id_head_bwd_kernel(float* __restrict__ gx, const float* __restrict__ fx, const float* __restrict__ fy,
                                                          const float* __restrict__ stats, const float* __restrict__ gout, int64_t D, float scale,
                                                          int accumulate) {
    const int b = blockIdx.y;
    const float nx = stats[(size_t)b * 3], ny = stats[(size_t)b * 3 + 1], c = stats[(size_t)b * 3 + 2];
    const float k = -gout[0] * scale / nx;
    const float ix = c / nx, iy = 1.f / ny;
    const size_t base = (size_t)b * D;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < D; e += (int64_t)gridDim.x * 256) {
        const float v = k * (fy[base + e] * iy - fx[base + e] * ix);
        gx[base + e] = accumulate ? gx[base + e] + v : v;
    }
}

// The multi-target heads (targets.h): one read of fx against k targets, target j weighted by w_j in the loss and the gradient.  Partials and stats carry
// MS floats per entry: |x|^2 (|x|), then (|y_j|^2, x.y_j) ((|y_j|, cos_j)) per target; unused targets are 0.
constexpr int MS = 1 + 2 * MAX_TARGETS;

// part[(b * nblk + blk) * MS + ...] = block sums of x^2, then y_j^2, x.y_j per target
__global__ __launch_bounds__(256) void id_head_partial_multi_kernel(float* __restrict__ part, const float* __restrict__ fx, const Targets tg, int64_t D) {
    __shared__ float red[256];
    const int blk = blockIdx.x, b = blockIdx.y, nblk = gridDim.x;
    const float* xp = fx + (size_t)b * D;
    const int64_t e0 = (int64_t)blk * HB, e1 = min<int64_t>(D, e0 + HB);
    float* o = part + ((size_t)b * nblk + blk) * MS;
    float sxx = 0.f;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
        const float u = xp[e];
        sxx = fmaf(u, u, sxx);
    }
    sxx = bsum256(sxx, red);
    if (threadIdx.x == 0) o[0] = sxx;
    for (int j = 0; j < MAX_TARGETS; ++j) {
        float syy = 0.f, sxy = 0.f;
        if (j < tg.k) {
            const float* yp = target_base(tg, j) + (size_t)b * D;
            for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
                const float u = xp[e], v = yp[e];
                syy = fmaf(v, v, syy);
                sxy = fmaf(u, v, sxy);
            }
            syy = bsum256(syy, red);
            sxy = bsum256(sxy, red);
        }
        if (threadIdx.x == 0) {
            o[1 + 2 * j] = syy;
            o[2 + 2 * j] = sxy;
        }
    }
}

// one workgroup: stats[(t * bs + b) * MS + ...] = |x|, then (|y_j|, cos_j) per target; loss_out[0] = sum_t sum_j w_j mean_b (1 - cos_j)
__global__ __launch_bounds__(256) void id_head_sum_multi_kernel(float* __restrict__ loss_out, float* __restrict__ stats, const float* __restrict__ part,
                                                                const Targets tg, int bs, int ntap, int nb0, int nb1, int nb2, int nb3, int nb4) {
    __shared__ float red[256];
    const int nbs[5] = {nb0, nb1, nb2, nb3, nb4};
    float loss = 0.f;
    size_t off = 0;
    for (int t = 0; t < ntap; ++t) {
        const int nb = nbs[t];
        float lt[MAX_TARGETS] = {0.f, 0.f, 0.f, 0.f};
        for (int b = 0; b < bs; ++b) {
            const float* pp = part + off + (size_t)b * nb * MS;
            float* st = stats + ((size_t)t * bs + b) * MS;
            float sxx = 0.f;
            for (int i = threadIdx.x; i < nb; i += 256) sxx += pp[MS * i];
            sxx = bsum256(sxx, red);
            const float nx = sqrtf(sxx);
            if (threadIdx.x == 0) st[0] = nx;
#pragma unroll
            for (int j = 0; j < MAX_TARGETS; ++j) {
                float syy = 0.f, sxy = 0.f;
                for (int i = threadIdx.x; i < nb; i += 256) {
                    syy += pp[MS * i + 1 + 2 * j];
                    sxy += pp[MS * i + 2 + 2 * j];
                }
                syy = bsum256(syy, red);
                sxy = bsum256(sxy, red);
                const float ny = sqrtf(syy);
                const float c = j < tg.k ? sxy / (nx * ny) : 0.f;
                if (threadIdx.x == 0) {
                    st[1 + 2 * j] = ny;
                    st[2 + 2 * j] = c;
                }
                lt[j] += 1.f - c;
            }
        }
        for (int j = 0; j < tg.k; ++j) loss += tg.w[j] * (lt[j] / (float)bs);
        off += (size_t)bs * nb * MS;
    }
    if (threadIdx.x == 0) loss_out[0] = loss;
}

// gx[b, e] (+)= -gout[0] scale sum_j w_j (fy_j / |y_j| - cos_j fx / |x|) / |x| from the multi-target stats of the tap
__global__ __launch_bounds__(256) void id_head_bwd_multi_kernel(float* __restrict__ gx, const float* __restrict__ fx, const Targets tg,
                                                                const float* __restrict__ stats, const float* __restrict__ gout, int64_t D, float scale,
                                                                int accumulate) {
    const int b = blockIdx.y;
    const float* st = stats + (size_t)b * MS;
    const float nx = st[0];
    const float* yp[MAX_TARGETS];
    float kk[MAX_TARGETS], ix[MAX_TARGETS], iy[MAX_TARGETS];
#pragma unroll
    for (int j = 0; j < MAX_TARGETS; ++j) {
        const bool on = j < tg.k;
        yp[j] = on ? target_base(tg, j) + (size_t)b * D : fx + (size_t)b * D;
        kk[j] = on ? -gout[0] * scale * tg.w[j] / nx : 0.f;
        ix[j] = on ? st[2 + 2 * j] / nx : 0.f;
        iy[j] = on ? 1.f / st[1 + 2 * j] : 0.f;
    }
    const int nt = tg.k;
    const size_t base = (size_t)b * D;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < D; e += (int64_t)gridDim.x * 256) {
        const float x = fx[base + e];
        float v = kk[0] * (yp[0][e] * iy[0] - x * ix[0]);
#pragma unroll
        for (int j = 1; j < MAX_TARGETS; ++j)
            if (j < nt) v += kk[j] * (yp[j][e] * iy[j] - x * ix[j]);
        gx[base + e] = accumulate ? gx[base + e] + v : v;
    }
}

}  // namespace

extern "C" int e4s_id_head_partial_multi(float* part, const float* fx, const float* const* ys, const float* tw, int k, const int* frame, int64_t fstride, int nframes,
                                         int bs, int64_t D, void* stream) {
    E4S_REQUIRE(part && fx, "id_head_partial_multi: null tensor");
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && D >= 1 && cdiv64(D, HB) <= (1 << 20), "id_head_partial_multi: bad size");
    Targets tg;
    if (const int st = make_targets(tg, ys, tw, k, frame, fstride, nframes, "id_head_partial_multi")) return st;
    if (bs == 0) return 0;
    hipLaunchKernelGGL(id_head_partial_multi_kernel, dim3((unsigned)cdiv64(D, HB), bs), dim3(256), 0, (hipStream_t)stream, part, fx, tg, D);
    return check_launch("id_head_partial_multi");
}

extern "C" int e4s_id_head_sum_multi(float* loss, float* stats, const float* part, const float* tw, int k, int bs, int ntap, int nb0, int nb1, int nb2,
                                     int nb3, int nb4, void* stream) {
    E4S_REQUIRE(loss && stats && part, "id_head_sum_multi: null tensor");
    E4S_REQUIRE(bs >= 1 && bs <= 65535 && ntap >= 1 && ntap <= 5, "id_head_sum_multi: bad size");
    const int nbs[5] = {nb0, nb1, nb2, nb3, nb4};
    for (int t = 0; t < ntap; ++t) E4S_REQUIRE(nbs[t] >= 1, "id_head_sum_multi: tap %d has no partials", t);
    const float* dummy[MAX_TARGETS] = {part, part, part, part};       // only the weights and the count are read here
    Targets tg;
    if (const int st = make_targets(tg, dummy, tw, k, nullptr, 0, 1, "id_head_sum_multi")) return st;
    hipLaunchKernelGGL(id_head_sum_multi_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, loss, stats, part, tg, bs, ntap, nb0, nb1, nb2, nb3, nb4);
    return check_launch("id_head_sum_multi");
}

extern "C" int e4s_id_head_bwd_multi(float* gx, const float* fx, const float* const* ys, const float* tw, int k, const int* frame, int64_t fstride, int nframes,
                                     const float* stats, const float* gout, int bs, int64_t D, float scale, int accumulate, void* stream) {
    E4S_REQUIRE(gx && fx && stats && gout, "id_head_bwd_multi: null tensor");
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && D >= 1, "id_head_bwd_multi: bad size");
    Targets tg;
    if (const int st = make_targets(tg, ys, tw, k, frame, fstride, nframes, "id_head_bwd_multi")) return st;
    if (bs == 0) return 0;
    const int gxs = (int)(cdiv64(D, 256) < 1024 ? cdiv64(D, 256) : 1024);
    hipLaunchKernelGGL(id_head_bwd_multi_kernel, dim3(gxs, bs), dim3(256), 0, (hipStream_t)stream, gx, fx, tg, stats, gout, D, scale, accumulate);
    return check_launch("id_head_bwd_multi");
}

extern "C" int e4s_id_resample(float* out, const float* x, const float* ay, const float* ax, const int* ry, const int* rx, int planes, int h, int w, int no,
                               void* stream) {
    E4S_REQUIRE(out && x && ay && ax && ry && rx, "id_resample: null tensor");
    E4S_REQUIRE(planes >= 0 && h >= 1 && w >= 1 && no >= 1, "id_resample: bad size");
    const int64_t n = (int64_t)planes * no * no;
    if (n == 0) return 0;
    hipLaunchKernelGGL(id_resample_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, out, x, ay, ax, ry, rx, n, h, w, no);
    return check_launch("id_resample");
}

extern "C" int e4s_id_resample_adjoint(float* gx, const float* g, const float* ay, const float* ax, const int* cy, const int* cx, int planes, int h, int w,
                                       int no, int accumulate, void* stream) {
    E4S_REQUIRE(gx && g && ay && ax && cy && cx, "id_resample_adjoint: null tensor");
    E4S_REQUIRE(planes >= 0 && h >= 1 && w >= 1 && no >= 1, "id_resample_adjoint: bad size");
    const int64_t n = (int64_t)planes * h * w;
    if (n == 0) return 0;
    hipLaunchKernelGGL(id_resample_adj_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, gx, g, ay, ax, cy, cx, n, h, w, no, accumulate);
    return check_launch("id_resample_adjoint");
}

extern "C" int e4s_id_affine(float* out, const float* x, const float* scale, const float* shift, const float* slope, int bs, int C, int hw, void* stream) {
    E4S_REQUIRE(out && x, "id_affine: null tensor");
    E4S_REQUIRE((scale == nullptr) == (shift == nullptr), "id_affine: scale and shift go together");
    E4S_REQUIRE(bs >= 0 && C >= 1 && hw >= 1, "id_affine: bad size");
    const int64_t n = (int64_t)bs * C * hw;
    if (n == 0) return 0;
    hipLaunchKernelGGL(id_affine_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, out, x, scale, shift, slope, n, C, hw);
    return check_launch("id_affine");
}

extern "C" int e4s_id_prelu_bwd(float* g, const float* src, const float* pre, const float* slope, int bs, int C, int h, int w, int sh, int sw, int off,
                                void* stream) {
    E4S_REQUIRE(g && src && pre && slope, "id_prelu_bwd: null tensor");
    E4S_REQUIRE(bs >= 0 && C >= 1 && h >= 1 && w >= 1 && off >= 0 && sh >= h + off && sw >= w + off, "id_prelu_bwd: bad size");
    const int64_t n = (int64_t)bs * C * h * w;
    if (n == 0) return 0;
    hipLaunchKernelGGL(id_prelu_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, g, src, pre, slope, n, C, h, w, sh, sw, off);
    return check_launch("id_prelu_bwd");
}

extern "C" int e4s_id_se_bwd(float* dr, float* s, float* v, const float* g, const float* r, const float* pooled, const float* gate, const float* fc1,
                             const float* fc2, int bs, int C, int H, int hw, void* stream) {
    E4S_REQUIRE(dr && s && v && g && r && pooled && gate && fc1 && fc2, "id_se_bwd: null tensor");
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && C >= 1 && C <= 1024 && H >= 1 && H <= 64 && hw >= 1, "id_se_bwd: bad size (C <= 1024, H <= 64)");
    if (bs == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(id_se_dot_kernel, dim3(bs * C), dim3(256), 0, st, s, g, r, hw);
    hipLaunchKernelGGL(id_se_bwd_kernel, dim3(bs), dim3(256), 0, st, v, s, pooled, gate, fc1, fc2, C, H, 1.f / (float)hw);
    const int64_t n = (int64_t)bs * C * hw;
    hipLaunchKernelGGL(id_se_dr_kernel, dim3(grid_for(n)), dim3(256), 0, st, dr, g, gate, v, n, hw);
    return check_launch("id_se_bwd");
}

extern "C" int e4s_id_scatter_add(float* gx, const float* src, int planes, int h, int w, void* stream) {
    E4S_REQUIRE(gx && src, "id_scatter_add: null tensor");
    E4S_REQUIRE(planes >= 0 && h >= 1 && w >= 1, "id_scatter_add: bad size");
    const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
    const int64_t n = (int64_t)planes * ho * wo;
    if (n == 0) return 0;
    hipLaunchKernelGGL(id_scatter_add_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, gx, src, n, h, w, ho, wo);
    return check_launch("id_scatter_add");
}

extern "C" int e4s_id_linear(float* y, const float* x, const float* W, const float* bias, int bs, int K, int N, void* stream) {
    E4S_REQUIRE(y && x && W, "id_linear: null tensor");
    E4S_REQUIRE(bs >= 0 && K >= 1 && N >= 1 && N <= 65535 * 64, "id_linear: bad size");
    if (bs == 0) return 0;
    hipLaunchKernelGGL(id_linear_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, y, x, W, bias, bs, K, N);
    return check_launch("id_linear");
}

extern "C" int e4s_id_linear_t(float* gx, const float* g, const float* W, int bs, int K, int N, void* stream) {
    E4S_REQUIRE(gx && g && W, "id_linear_t: null tensor");
    E4S_REQUIRE(bs >= 0 && K >= 1 && N >= 1, "id_linear_t: bad size");
    if (bs == 0) return 0;
    hipLaunchKernelGGL(id_linear_t_kernel, dim3(cdiv(K, 64)), dim3(256), 0, (hipStream_t)stream, gx, g, W, bs, K, N);
    return check_launch("id_linear_t");
}

extern "C" int e4s_id_head_partial(float* part, const float* fx, const float* fy, int bs, int64_t D, void* stream) {
    E4S_REQUIRE(part && fx && fy, "id_head_partial: null tensor");
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && D >= 1 && cdiv64(D, HB) <= (1 << 20), "id_head_partial: bad size");
    if (bs == 0) return 0;
    hipLaunchKernelGGL(id_head_partial_kernel, dim3((unsigned)cdiv64(D, HB), bs), dim3(256), 0, (hipStream_t)stream, part, fx, fy, D);
    return check_launch("id_head_partial");
}

extern "C" int e4s_id_head_sum(float* loss, float* sim, float* stats, const float* part, int bs, int ntap, int nb0, int nb1, int nb2, int nb3, int nb4,
                               void* stream) {
    E4S_REQUIRE(loss && sim && stats && part, "id_head_sum: null tensor");
    E4S_REQUIRE(bs >= 1 && bs <= 65535 && ntap >= 1 && ntap <= 5, "id_head_sum: bad size");
    const int nbs[5] = {nb0, nb1, nb2, nb3, nb4};
    for (int t = 0; t < ntap; ++t) E4S_REQUIRE(nbs[t] >= 1, "id_head_sum: tap %d has no partials", t);
    hipLaunchKernelGGL(id_head_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, loss, sim, stats, part, bs, ntap, nb0, nb1, nb2, nb3, nb4);
    return check_launch("id_head_sum");
}

extern "C" int e4s_id_head_bwd(float* gx, const float* fx, const float* fy, const float* stats, const float* gout, int bs, int64_t D, float scale,
                               int accumulate, void* stream) {
    E4S_REQUIRE(gx && fx && fy && stats && gout, "id_head_bwd: null tensor");
    E4S_REQUIRE(bs >= 0 && bs <= 65535 && D >= 1, "id_head_bwd: bad size");
    if (bs == 0) return 0;
    const int gxs = (int)(cdiv64(D, 256) < 1024 ? cdiv64(D, 256) : 1024);
    hipLaunchKernelGGL(id_head_bwd_kernel, dim3(gxs, bs), dim3(256), 0, (hipStream_t)stream, gx, fx, fy, stats, gout, D, scale, accumulate);
    return check_launch("id_head_bwd");
}
