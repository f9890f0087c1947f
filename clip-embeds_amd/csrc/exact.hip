// fp32 precision mode (CE_PREC_F32): the towers' GEMMs, attention and patchify with f32 operands on
// the f32-input MFMA of gfx950 (v_mfma_f32_32x32x2_f32), whose result is bit for bit a k-ordered
// f32 fmaf chain.  Each output element is one accumulator chain over all of K (no split-K), the
// activations are the device library's erff / expf, and the softmax keeps the true running row
// maximum.  The mode exists for decision parity with an f32 reference at batch 1-2 (the eval
// drivers), so the kernels are plain LDS-tiled designs with none of the bf16 kernels' DMA schedules.
//
// Reference semantics:
//   nn.Linear / nn.GELU / QuickGELU   open_clip/src/open_clip/transformer.py:32-35,235-239
//   attention                         transformer.py:242-255 (softmax(q k^T / sqrt(64) [+ causal]) v)
//   conv1 patchify                    transformer.py:549-555,702-704
#include "ce_device.h"
#include "ce_kernels.h"

namespace ce {
namespace {

__device__ __forceinline__ int map_row_x(int r, int grp, int gs, int go) {
    if (grp == 0) return r;
    const int g = r / grp;
    return g * gs + go + (r - g * grp);
}

template <int ACT>
__device__ __forceinline__ float act_exact(float x) {
    if constexpr (ACT == ACT_GELU) return 0.5f * x * (1.0f + erff(x * 0.70710678f));
    else if constexpr (ACT == ACT_QGELU) return x / (1.0f + expf(-1.702f * x));
    else return x;
}

// ---- GEMM -------------------------------------------------------------------------------
// 128 x 128 x 32 block, 256 threads: wave (wm, wn) of the 2 x 2 owns a 64 x 64 quadrant as 2 x 2
// MFMA tiles of 32 x 32.  A and W tiles sit in LDS as [row][k] with rows of 33 floats: the MFMA
// operand read (lane l: row l & 31, k = 2 step + (l >> 5)) then touches 64 different banks.
constexpr int kGT = 128, kGK = 32, kGLd = kGK + 1;

template <int ACT>
__global__ __launch_bounds__(256) void gemm_f32_k(GemmF32Params p) {
    __shared__ float As[kGT * kGLd];
    __shared__ float Ws[kGT * kGLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * kGT, n0 = blockIdx.x * kGT;
    const int lr = lane & 31, lh = lane >> 5;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // staging: thread t moves the float4 at (row t / 8 + 32 i, k 4 (t % 8)) of both tiles, i = 0..3;
    // rows past M (A) or N (W) are zero
    const int sr = tid >> 3, sk = (tid & 7) * 4;
    for (int k0 = 0; k0 < p.K; k0 += kGK) {
        float4 ra[4], rw[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + sr + 32 * i, n = n0 + sr + 32 * i;
            ra[i] = m < p.M ? *reinterpret_cast<const float4*>(p.A + (size_t)m * p.lda + k0 + sk)
                            : make_float4(0.f, 0.f, 0.f, 0.f);
            rw[i] = n < p.N ? *reinterpret_cast<const float4*>(p.W + (size_t)n * p.K + k0 + sk)
                            : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();      // the previous tile's MFMA reads are done
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float* a = As + (sr + 32 * i) * kGLd + sk;
            a[0] = ra[i].x; a[1] = ra[i].y; a[2] = ra[i].z; a[3] = ra[i].w;
            float* w = Ws + (sr + 32 * i) * kGLd + sk;
            w[0] = rw[i].x; w[1] = rw[i].y; w[2] = rw[i].z; w[3] = rw[i].w;
        }
        __syncthreads();
        const float* ab = As + (wm * 64 + lr) * kGLd + lh;
        const float* wb = Ws + (wn * 64 + lr) * kGLd + lh;
#pragma unroll
        for (int s = 0; s < kGK / 2; ++s) {
            const float a0 = ab[2 * s], a1 = ab[32 * kGLd + 2 * s];
            const float b0 = wb[2 * s], b1 = wb[32 * kGLd + 2 * s];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // C/D map of the 32 x 32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn * 64 + j * 32 + lr;
        if (n >= p.N) continue;
        const float bias = p.bias ? p.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m >= p.M) continue;
                float v = act_exact<ACT>(acc[i][j][r] + bias);
                if (p.resid) v += p.resid[(size_t)map_row_x(m, p.grp, p.r_gs, p.r_go) * p.ldr + n];
                p.out[(size_t)map_row_x(m, p.grp, p.o_gs, p.o_go) * p.ldo + n] = v;
            }
    }
}

// ---- attention --------------------------------------------------------------------------
// One wave per 32 query rows of one (b, h); key tiles of 32 staged in LDS.  Both products run
// transposed so that a lane owns one query: S^T = K (Q / 8)^T puts query l & 31 on the lane and 16
// of the tile's 32 keys in its registers (key (r & 3) + 8 (r >> 2) + 4 (l >> 5) in register r), so
// the row maximum and sum are in-lane reductions plus one exchange with lane l ^ 32; O^T = V^T P^T
// takes P^T straight from those registers as the B operand, MFMA step r summing the two keys the
// lane halves hold in register r (V^T, the A operand, is read from LDS in that same key order).
constexpr int kKLd = 66;    // K rows: lane reads [key l & 31][2 s + (l >> 5)]: bank 2 key + half
constexpr int kVLd = 72;    // V rows: the halves read rows 4 apart: 4 * 72 = 32 banks apart

template <bool CAUSAL>
__global__ __launch_bounds__(64) void attention_f32_k(const float* __restrict__ qkv, float* __restrict__ out,
                                                      int L, int H) {
    __shared__ float Ks[32 * kKLd];
    __shared__ __attribute__((aligned(16))) float Vs[32 * kVLd];
    const int lane = threadIdx.x, lr = lane & 31, lh = lane >> 5;
    const int q0 = blockIdx.x * 32, h = blockIdx.y, b = blockIdx.z;
    const long ld = 3L * H * 64;
    const float* base = qkv + (size_t)b * L * ld + h * 64;
    const int qi = q0 + lr;
    // B operand of S^T: lane holds (Q / 8)[query l & 31][d = 2 s + (l >> 5)]
    float qf[32];
    if (qi < L) {
        const float* qrow = base + (size_t)qi * ld + lh;
#pragma unroll
        for (int s = 0; s < 32; ++s) qf[s] = qrow[2 * s] * 0.125f;
    } else {
#pragma unroll
        for (int s = 0; s < 32; ++s) qf[s] = 0.f;
    }
    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) o0[r] = o1[r] = 0.f;
    float mrun = -INFINITY, lsum = 0.f;      // lsum: this lane half's share of the row sum
    const int nkt = (L + 31) / 32;
    const int nt = CAUSAL ? min(nkt, blockIdx.x + 1) : nkt;
    for (int kt = 0; kt < nt; ++kt) {
        __syncthreads();
        // stage keys kt * 32 .. + 31 (rows past L as zeros): lane moves float4 (key i * 4 + l / 16, d 4 (l % 16))
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int key = i * 4 + (lane >> 4), d4 = (lane & 15) * 4;
            const int kj = kt * 32 + key;
            float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
            if (kj < L) {
                const float* row = base + (size_t)kj * ld + d4;
                kv = *reinterpret_cast<const float4*>(row + H * 64);
                vv = *reinterpret_cast<const float4*>(row + 2 * H * 64);
            }
            float* kd = Ks + key * kKLd + d4;
            kd[0] = kv.x; kd[1] = kv.y; kd[2] = kv.z; kd[3] = kv.w;
            *reinterpret_cast<float4*>(Vs + key * kVLd + d4) = vv;
        }
        __syncthreads();
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
        const float* kb = Ks + lr * kKLd + lh;
#pragma unroll
        for (int s = 0; s < 32; ++s) st = __builtin_amdgcn_mfma_f32_32x32x2f32(kb[2 * s], qf[s], st, 0, 0, 0);
        // masked and out-of-range keys: -inf, so their weight is exactly 0
        float mt = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kj = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (kj >= L || (CAUSAL && kj > qi)) st[r] = -INFINITY;
            mt = fmaxf(mt, st[r]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        // (key 0 is live for every query, so the maximum is finite from the first tile on)
        const float mnew = fmaxf(mrun, mt);
        const float alpha = expf(mrun - mnew);
        mrun = mnew;
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            st[r] = expf(st[r] - mnew);
            ps += st[r];
        }
        lsum = lsum * alpha + ps;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            o0[r] *= alpha;
            o1[r] *= alpha;
        }
        // O^T[d][q] += V^T[d][key] P^T[key][q]: step r sums keys (r & 3) + 8 (r >> 2) + 4 half
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* vr = Vs + ((r & 3) + 8 * (r >> 2) + 4 * lh) * kVLd + lr;
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[0], st[r], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[32], st[r], o1, 0, 0, 0);
        }
    }
    lsum += __shfl_xor(lsum, 32, 64);
    if (qi >= L) return;
    const float inv = 1.0f / lsum;
    float* orow = out + ((size_t)b * L + qi) * ((size_t)H * 64) + h * 64;
    // lane holds d = 32 t + 8 g + 4 half + (0..3) of its query in registers 4 g .. 4 g + 3 of o_t
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int d = 8 * g + 4 * lh;
        *reinterpret_cast<float4*>(orow + d) =
            make_float4(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
        *reinterpret_cast<float4*>(orow + 32 + d) =
            make_float4(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
    }
}

// ---- patchify ---------------------------------------------------------------------------
template <bool PIX_BF16>
__global__ __launch_bounds__(256) void im2col_f32_k(const void* __restrict__ pix, float* __restrict__ cols, int B,
                                                    int S, int patch, int Kp) {
    const int G = S / patch;
    const long total = (long)B * G * G * Kp;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int col = (int)(idx % Kp);
    const long row = idx / Kp;
    const int pp2 = patch * patch;
    float val = 0.f;
    if (col < 3 * pp2) {
        const int b = (int)(row / (G * G));
        const int pidx = (int)(row % (G * G));
        const int py = pidx / G, px = pidx % G;
        const int c = col / pp2, rem = col % pp2;
        const int ky = rem / patch, kx = rem % patch;
        const size_t off = (((size_t)b * 3 + c) * S + (size_t)(py * patch + ky)) * S + px * patch + kx;
        if constexpr (PIX_BF16) val = bf2f(static_cast<const bf16_t*>(pix)[off]);
        else val = static_cast<const float*>(pix)[off];
    }
    cols[idx] = val;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

hipError_t launch_gemm_f32(const GemmF32Params& p, int act, hipStream_t s) {
    if (!p.A || !p.W || !p.out || p.M <= 0 || p.N <= 0 || p.K <= 0 || p.N % 64 || p.K % 32) return hipErrorInvalidValue;
    if (p.lda < p.K || p.lda % 4 || p.ldo < p.N || (p.resid && p.ldr < p.N) || !aligned16(p.A) || !aligned16(p.W))
        return hipErrorInvalidValue;
    if (p.grp < 0 || act < ACT_NONE_ || act > ACT_QGELU_) return hipErrorInvalidValue;
    const dim3 grid((p.N + kGT - 1) / kGT, (p.M + kGT - 1) / kGT);
    if (act == ACT_GELU_) hipLaunchKernelGGL(gemm_f32_k<ACT_GELU>, grid, dim3(256), 0, s, p);
    else if (act == ACT_QGELU_) hipLaunchKernelGGL(gemm_f32_k<ACT_QGELU>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(gemm_f32_k<ACT_NONE>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_attention_f32(const float* qkv, float* out, int B, int L, int H, bool causal, hipStream_t s) {
    if (!qkv || !out || B <= 0 || L <= 0 || H <= 0 || H > 65535 || B > 65535 || !aligned16(qkv) || !aligned16(out))
        return hipErrorInvalidValue;
    const dim3 grid((L + 31) / 32, H, B);
    if (causal) hipLaunchKernelGGL(attention_f32_k<true>, grid, dim3(64), 0, s, qkv, out, L, H);
    else hipLaunchKernelGGL(attention_f32_k<false>, grid, dim3(64), 0, s, qkv, out, L, H);
    return hipGetLastError();
}

hipError_t launch_im2col_f32(const void* pix, bool pix_bf16, float* cols, int B, int S, int patch, int Kp,
                             hipStream_t s) {
    if (!pix || !cols || B <= 0 || S <= 0 || patch <= 0 || S % patch || Kp < 3 * patch * patch) return hipErrorInvalidValue;
    const int G = S / patch;
    const long total = (long)B * G * G * Kp;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (pix_bf16) hipLaunchKernelGGL(im2col_f32_k<true>, grid, dim3(256), 0, s, pix, cols, B, S, patch, Kp);
    else hipLaunchKernelGGL(im2col_f32_k<false>, grid, dim3(256), 0, s, pix, cols, B, S, patch, Kp);
    return hipGetLastError();
}

}  // namespace ce
