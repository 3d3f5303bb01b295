// Packed forward of the BERT / XLM-R block (BGE-small / base / large, bge-m3, e5: the reference's CLS-pooling branch,
// modeling.py:231-232) for rankpo_amd/encoder.py `BertEncoder.pooled_cls`.  Four entry points, bf16 or fp16 storage, f32
// arithmetic inside:
//   rpo_bidir_attn_fwd     non-causal variable-length attention over packed tokens (HF BertSelfAttention's softmax(QK^T s) V,
//                          which the padded path runs as F.scaled_dot_product_attention with a boolean key mask)
//   rpo_add_layernorm_fwd  LayerNorm(a + b) (HF BertSelfOutput / BertOutput: `LayerNorm(dropout(dense(h)) + input)`)
//   rpo_gelu_fwd           exact erf GELU in place (HF BertIntermediate with hidden_act "gelu")
//   rpo_bert_embed_ln_fwd  word + token type + position embedding gather, then LayerNorm (HF BertEmbeddings.forward)
// the same four on f32 storage, as entries of their own (header section 9b; the four above answer RPO_DT_F32 with UNSUPPORTED):
//   rpo_bidir_attn_fwd_f32       the attention on the f32-input MFMA (v_mfma_f32_16x16x4_f32), P never rounded
//   rpo_add_layernorm_fwd_f32 / rpo_gelu_fwd_f32 / rpo_bert_embed_ln_fwd_f32   the row kernels instantiated for float
// and the TRAINING step on the same packed layout (`BertEncoder.pooled_cls_train`):
//   rpo_bidir_attn_train_fwd     the forward with attention-probability dropout (a template arm of the same kernel)
//   rpo_bidir_attn_bwd           dQ kernel + dK/dV kernel in the forward's wave layout, P recomputed from lse, dropout replayed
//   rpo_bidir_attn_dropout_mask  the keep mask of a block from the kernels' own device function (tests, diagnostics)
//   rpo_add_layernorm_train_fwd / rpo_bert_embed_ln_train_fwd   the forwards, also storing the rounded sum s
//   rpo_layernorm_bwd            ds and per-block dgamma / dbeta partials from s, gamma and dy
//   rpo_gelu_out_fwd / rpo_gelu_bwd   out-of-place GELU and its derivative
// and, opt-in, the hidden-state dropout inside the row kernels (what gradient checkpointing on the packed step recomputes):
//   rpo_add_layernorm_drop_fwd / rpo_bert_embed_ln_drop_fwd / rpo_layernorm_drop_bwd   the three row kernels with a stateless keep
//   rpo_hidden_dropout_mask / rpo_hidden_dropout_scale                                 that keep function and its scale (tests)
// Plain HIP with MFMA builtins; no inline asm, no counted waits.  No atomics: every entry is deterministic.
#include "common.hpp"

#include <initializer_list>
#include <type_traits>

namespace {

// ---- storage-type helpers -------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ unsigned short to_bits(float f);
template <> __device__ __forceinline__ unsigned short to_bits<bf16_t>(float f) { return f32_to_bf16(f); }
template <> __device__ __forceinline__ unsigned short to_bits<f16_t>(float f) {
    return __builtin_bit_cast(unsigned short, (f16_t)f);
}
template <typename T> __device__ __forceinline__ unsigned pack2(float a, float b) {
    return (unsigned)to_bits<T>(a) | ((unsigned)to_bits<T>(b) << 16);
}
__device__ __forceinline__ int64_t clamp_index(int64_t i, int64_t n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// v_mfma_f32_16x16x32_{bf16,f16}: lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15], j = 0..7;
// C[row 4 (l >> 4) + i][col l & 15], i = 0..3.
template <typename T> struct AttnMma;
template <> struct AttnMma<bf16_t> {
    __device__ static __forceinline__ void mma(uint4_t a, uint4_t b, float4_t& c) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(short8_t, a), __builtin_bit_cast(short8_t, b), c, 0, 0, 0);
    }
};
template <> struct AttnMma<f16_t> {
    __device__ static __forceinline__ void mma(uint4_t a, uint4_t b, float4_t& c) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, a), __builtin_bit_cast(half8_t, b), c, 0, 0, 0);
    }
};

// ---- (1) bidirectional variable-length attention ---------------------------------------------------
// One wave per (work-list entry, head); an entry = 32 queries (two 16-query MFMA tiles) of one sequence.  The wave computes
// S^T = K Q^T per 32-key step (A = 16 key rows straight from global memory, B = Q^T from registers), so that every lane owns ONE
// query (column l & 15) in the accumulator layout: the softmax statistics stay per lane and reduce over the 4 lane groups with two
// shuffles.  P^T is rounded to the storage type and used as the B operand of O^T = V^T P^T as it lies in the registers: lane
// group g holds keys 4g..4g+3 of each 16-key half of the step, which fixes the key order of the k slots; V is staged row-major in
// LDS and read column-wise in that order.  O^T accumulates in f32 (lane: query l & 15, head dims 4g..4g+3 of each 16-block).
constexpr int kAttnQBlock = 32;     // queries per work-list entry
constexpr int kAttnKeys = 32;       // keys per step
constexpr float kLn2 = 0.6931471805599453f;

// ---- attention-probability dropout ---------------------------------------------------------------
// keep(seed, head, packed query row, packed key row): ONE stateless counter-based function shared by the training forward, both
// backward kernels and the mask dump.  Philox2x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) with
// counter = (packed query row, packed key row >> 2) and a 32-bit key mixed (murmur3 finaliser) from the 64-bit seed and the head;
// the 64 output bits are four 16-bit fields, one per key of the group of 4, and a key is KEPT when its field >= thr =
// round(p_drop * 65536) (p_drop is quantised to 1 / 65536).  dropout_keep is that function; dropout_keep4 and the dK/dV kernel
// evaluate the same pieces (dropout_key, dropout_bits, dropout_field_keep) with the shared parts hoisted.
__device__ __forceinline__ unsigned fmix32(unsigned x) {
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    return x ^ (x >> 16);
}
struct DropBits { unsigned c0, c1; };
__device__ __forceinline__ unsigned dropout_key(uint64_t seed, int head) {
    return fmix32((unsigned)seed ^ fmix32((unsigned)(seed >> 32) ^ fmix32((unsigned)head + 0x9e3779b9u)));
}
__device__ __forceinline__ DropBits dropout_bits(unsigned key, int qrow, int kgroup) {
    unsigned c0 = (unsigned)qrow, c1 = (unsigned)kgroup;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned hi = __umulhi(0xd256d193u, c0), lo = 0xd256d193u * c0;
        c0 = hi ^ key ^ c1;
        c1 = lo;
        key += 0x9e3779b9u;
    }
    return DropBits{c0, c1};
}
__device__ __forceinline__ bool dropout_field_keep(DropBits b, int krow, unsigned thr) {
    return ((((krow & 2) ? b.c1 : b.c0) >> (16 * (krow & 1))) & 0xffffu) >= thr;
}
__device__ __forceinline__ bool dropout_keep(uint64_t seed, int head, int qrow, int krow, unsigned thr) {
    return dropout_field_keep(dropout_bits(dropout_key(seed, head), qrow, krow >> 2), krow, thr);
}
// dropout_keep for the four consecutive key rows krow0 .. krow0 + 3 of one query row (what a lane of the forward and of the dQ
// kernel owns): they lie in one group of 4 when krow0 is a multiple of 4 (wave-uniform: the sequence's first packed row decides
// it), else in two, so one or two Philox evaluations serve four elements.  key = dropout_key(seed, head).
__device__ __forceinline__ void dropout_keep4(unsigned key, int qrow, int krow0, unsigned thr, bool (&keep)[4]) {
    const DropBits lo = dropout_bits(key, qrow, krow0 >> 2);
    if ((krow0 & 3) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) keep[i] = dropout_field_keep(lo, krow0 + i, thr);
    } else {
        const DropBits hi = dropout_bits(key, qrow, (krow0 >> 2) + 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) keep[i] = dropout_field_keep(((krow0 + i) >> 2) == (krow0 >> 2) ? lo : hi, krow0 + i, thr);
    }
}

// DROP: the training arm (rpo_bidir_attn_train_fwd).  The row sum and lse come from the undropped probabilities; dropped ones
// enter the PV product as zeros and O is scaled by inv_keep = 1 / (1 - p_drop) at the end.  DROP = false is the forward as before.
template <typename T, int HD, bool DROP>
__global__ __launch_bounds__(64) void bidir_attn_fwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, int64_t q_stride, int64_t k_stride,
    int64_t v_stride, const int* __restrict__ cu_q, const int* __restrict__ cu_k, const int* __restrict__ tiles,
    float scale_log2, T* __restrict__ out, int64_t out_stride, float* __restrict__ lse, int64_t total_q, unsigned thr,
    float inv_keep, uint64_t seed) {
    constexpr int QS = kAttnQBlock / 16;   // query tiles per wave
    constexpr int KS = HD / 32;            // k-steps of the score product
    constexpr int OB = HD / 16;            // 16-row blocks of O^T
    constexpr int VLD = HD + 8;            // LDS row stride (elements): rows stay 16-byte aligned
    constexpr int VCH = kAttnKeys * HD / 8 / 64;   // 16-byte V chunks per lane per step
    __shared__ __attribute__((aligned(16))) unsigned short vs[kAttnKeys * VLD];

    const int entry = blockIdx.x, h = blockIdx.y;
    const int seq = tiles[2 * entry], q0 = tiles[2 * entry + 1];
    const int tq0 = cu_q[seq], lq = cu_q[seq + 1] - tq0;
    const int tk0 = cu_k[seq], lk = cu_k[seq + 1] - tk0;
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const int64_t hcol = (int64_t)h * HD;
    if (lq <= 0) return;

    uint4_t qf[QS][KS];
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        const int qi = min(q0 + s * 16 + r, lq - 1);     // rows past the end: loaded (in bounds), never stored
        const T* qp = q + (int64_t)(tq0 + qi) * q_stride + hcol + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[s][ks] = *reinterpret_cast<const uint4_t*>(qp + 32 * ks);
    }
    float m[QS], l[QS];
    float4_t o[QS][OB];
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        m[s] = -INFINITY;
        l[s] = 0.f;
#pragma unroll
        for (int b = 0; b < OB; ++b) o[s][b] = float4_t{0.f, 0.f, 0.f, 0.f};
    }

    for (int kt = 0; kt < lk; kt += kAttnKeys) {
        // V rows of this step -> registers (clamped to the sequence: in bounds; masked keys get p = 0)
        uint4_t vr[VCH];
#pragma unroll
        for (int c = 0; c < VCH; ++c) {
            const int idx = lane + 64 * c, key = idx / (HD / 8), c8 = idx - key * (HD / 8);
            const int kk = min(kt + key, lk - 1);
            vr[c] = *reinterpret_cast<const uint4_t*>(v + (int64_t)(tk0 + kk) * v_stride + hcol + 8 * c8);
        }
        float4_t sc[2][QS];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int kk = min(kt + b * 16 + r, lk - 1);
            const T* kp = k + (int64_t)(tk0 + kk) * k_stride + hcol + 8 * g;
            uint4_t kf[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) kf[ks] = *reinterpret_cast<const uint4_t*>(kp + 32 * ks);
#pragma unroll
            for (int s = 0; s < QS; ++s) {
                sc[b][s] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) AttnMma<T>::mma(kf[ks], qf[s][ks], sc[b][s]);
            }
        }
        __syncthreads();                                   // the previous step's V reads are done
#pragma unroll
        for (int c = 0; c < VCH; ++c) {
            const int idx = lane + 64 * c, key = idx / (HD / 8), c8 = idx - key * (HD / 8);
            *reinterpret_cast<uint4_t*>(&vs[key * VLD + 8 * c8]) = vr[c];
        }
        // online softmax (log2 domain, scale folded in); sc[b][s][i] = score of key kt + 16 b + 4 g + i, query q0 + 16 s + r
        uint4_t pf[QS];
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            float mx = -INFINITY;
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float x = (kt + b * 16 + 4 * g + i < lk) ? sc[b][s][i] * scale_log2 : -INFINITY;
                    sc[b][s][i] = x;
                    mx = fmaxf(mx, x);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mn = fmaxf(m[s], mx);              // finite: key kt is always valid
            const float alpha = __builtin_amdgcn_exp2f(m[s] - mn);
            m[s] = mn;
            float ps = 0.f;
            unsigned w[4];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                float p[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    p[i] = __builtin_amdgcn_exp2f(sc[b][s][i] - mn);
                    ps += p[i];
                }
                if constexpr (DROP) {
                    bool keep[4];
                    dropout_keep4(dropout_key(seed, h), tq0 + q0 + s * 16 + r, tk0 + kt + b * 16 + 4 * g, thr, keep);
#pragma unroll
                    for (int i = 0; i < 4; ++i) p[i] = keep[i] ? p[i] : 0.f;
                }
                w[2 * b] = pack2<T>(p[0], p[1]);
                w[2 * b + 1] = pack2<T>(p[2], p[3]);
            }
            pf[s] = uint4_t{w[0], w[1], w[2], w[3]};
            l[s] = fmaf(l[s], alpha, ps);                  // per-lane partial sum: alpha is the same on the 4 lanes of a query
#pragma unroll
            for (int b = 0; b < OB; ++b) o[s][b] *= alpha;
        }
        __syncthreads();                                   // V tile visible
        // A = V^T (row = head dim 16 b + r, k slot j = key 4 g + j for j < 4, 16 + 4 g + j - 4 else), B = P^T
#pragma unroll
        for (int b = 0; b < OB; ++b) {
            unsigned e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = (j < 4) ? 4 * g + j : 16 + 4 * g + (j - 4);
                e[j] = vs[key * VLD + 16 * b + r];
            }
            const uint4_t va{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
#pragma unroll
            for (int s = 0; s < QS; ++s) AttnMma<T>::mma(va, pf[s], o[s][b]);
        }
    }

#pragma unroll
    for (int s = 0; s < QS; ++s) {
        float L = l[s];
        L += __shfl_xor(L, 16, 64);
        L += __shfl_xor(L, 32, 64);
        const int qi = q0 + s * 16 + r;
        if (qi >= lq) continue;
        float inv = L > 0.f ? 1.0f / L : 0.f;
        if constexpr (DROP) inv *= inv_keep;
        T* op = out + (int64_t)(tq0 + qi) * out_stride + hcol + 4 * g;
#pragma unroll
        for (int b = 0; b < OB; ++b) {
            const uint2_t pk{pack2<T>(o[s][b][0] * inv, o[s][b][1] * inv), pack2<T>(o[s][b][2] * inv, o[s][b][3] * inv)};
            *reinterpret_cast<uint2_t*>(op + 16 * b) = pk;
        }
        if (lse && g == 0) lse[(int64_t)h * total_q + tq0 + qi] = L > 0.f ? (m[s] + log2f(L)) * kLn2 : -INFINITY;
    }
}

// ---- (1a) the same attention on f32 storage (rpo_bidir_attn_fwd_f32) ---------------------------------
// The wave layout, the work list and the accumulator map of the kernel above, on v_mfma_f32_16x16x4_f32 (f32 operands, exact f32
// products, f32 accumulation: nothing is rounded to 16 bits anywhere).  Operands are ONE f32 per lane: A[row l & 15][k = l >> 4],
// B[k = l >> 4][col l & 15].
//   S^T = K Q^T: a lane keeps the HD / 4 consecutive head dims HD / 4 g .. of its key row (A) and of its query row (B), loaded as
//   16-byte vectors; MFMA t of the HD / 4 takes element t of both, so its k slot g is head dim HD / 4 g + t (any one-to-one map
//   of k slots to head dims gives the same dot product, as long as A and B use the same one).
//   O^T = V^T P^T: MFMA t of a 16-key half takes p[t] as B as it lies in the accumulator (k slot g = key 4 g + t) and
//   A = V[key 4 g + t][16 b + r] from the LDS tile.  Row stride HD + 4 words: the two lane groups of a ds_read_b32 half
//   (g, g + 1: 4 rows apart) then read banks 16 apart, and rows stay 16-byte aligned for the staging stores.
// One 16x16x4 MFMA issues in 32 cycles and its result is ready after 40: consecutive MFMAs go round four accumulators (scores:
// two query tiles x two chains) or the two query tiles and the HD / 16 output blocks (PV), never the same one back to back.
// The exponent is exp2(((s - m) |scale|) log2 e) with m the running maximum of the RAW scores (sign-adjusted by negating Q when
// scale < 0) and log2 e carried as hi + lo: the roundings are relative to the DISTANCE from the maximum, none is taken at the
// magnitude of a large score.
constexpr float kLog2eHi = 1.44269502162933349609375f;        // (float)log2(e)
constexpr float kLog2eLo = 1.92596299112661746e-8f;           // log2(e) - kLog2eHi
template <int HD>
__global__ __launch_bounds__(64) void bidir_attn_fwd_f32_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t q_stride, int64_t k_stride,
    int64_t v_stride, const int* __restrict__ cu_q, const int* __restrict__ cu_k, const int* __restrict__ tiles,
    float scale_abs, float sgn, float* __restrict__ out, int64_t out_stride, float* __restrict__ lse, int64_t total_q) {
    constexpr int QS = kAttnQBlock / 16;   // query tiles per wave
    constexpr int DK = HD / 4;             // MFMAs of a 16x16 score block = head dims per lane
    constexpr int OB = HD / 16;            // 16-row blocks of O^T
    constexpr int VLD = HD + 4;            // LDS row stride (words)
    constexpr int VCH = kAttnKeys * HD / 4 / 64;   // 16-byte V chunks per lane per step
    __shared__ __attribute__((aligned(16))) float vs[kAttnKeys * VLD];

    const int entry = blockIdx.x, h = blockIdx.y;
    const int seq = tiles[2 * entry], q0 = tiles[2 * entry + 1];
    const int tq0 = cu_q[seq], lq = cu_q[seq + 1] - tq0;
    const int tk0 = cu_k[seq], lk = cu_k[seq + 1] - tk0;
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const int64_t hcol = (int64_t)h * HD;
    if (lq <= 0) return;

    float qf[QS][DK];
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        const int qi = min(q0 + s * 16 + r, lq - 1);     // rows past the end: loaded (in bounds), never stored
        const float* qp = q + (int64_t)(tq0 + qi) * q_stride + hcol + DK * g;
#pragma unroll
        for (int j = 0; j < DK / 4; ++j) {
            const float4_t t = *reinterpret_cast<const float4_t*>(qp + 4 * j);
#pragma unroll
            for (int e = 0; e < 4; ++e) qf[s][4 * j + e] = t[e] * sgn;
        }
    }
    float m[QS], l[QS];
    float4_t o[QS][OB];
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        m[s] = -INFINITY;
        l[s] = 0.f;
#pragma unroll
        for (int b = 0; b < OB; ++b) o[s][b] = float4_t{0.f, 0.f, 0.f, 0.f};
    }

    for (int kt = 0; kt < lk; kt += kAttnKeys) {
        // V rows of this step -> registers (clamped to the sequence: in bounds; masked keys get p = 0)
        float4_t vr[VCH];
#pragma unroll
        for (int c = 0; c < VCH; ++c) {
            const int idx = lane + 64 * c, key = idx / (HD / 4), c4 = idx - key * (HD / 4);
            const int kk = min(kt + key, lk - 1);
            vr[c] = *reinterpret_cast<const float4_t*>(v + (int64_t)(tk0 + kk) * v_stride + hcol + 4 * c4);
        }
        float4_t sc[2][QS];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int kk = min(kt + b * 16 + r, lk - 1);
            const float* kp = k + (int64_t)(tk0 + kk) * k_stride + hcol + DK * g;
            float4_t kf[DK / 4];
#pragma unroll
            for (int j = 0; j < DK / 4; ++j) kf[j] = *reinterpret_cast<const float4_t*>(kp + 4 * j);
            // two chains per score block (even / odd t), added at the end: half the length of each rounding chain, and four
            // independent accumulators in flight
            float4_t odd[QS];
#pragma unroll
            for (int s = 0; s < QS; ++s) sc[b][s] = odd[s] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < DK; t += 2)
#pragma unroll
                for (int s = 0; s < QS; ++s) {
                    sc[b][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[t / 4][t % 4], qf[s][t], sc[b][s], 0, 0, 0);
                    odd[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[t / 4][t % 4 + 1], qf[s][t + 1], odd[s], 0, 0, 0);
                }
#pragma unroll
            for (int s = 0; s < QS; ++s) sc[b][s] += odd[s];
        }
        __syncthreads();                                   // the previous step's V reads are done
#pragma unroll
        for (int c = 0; c < VCH; ++c) {
            const int idx = lane + 64 * c, key = idx / (HD / 4), c4 = idx - key * (HD / 4);
            *reinterpret_cast<float4_t*>(&vs[key * VLD + 4 * c4]) = vr[c];
        }
        // online softmax; sc[b][s][i] = raw score of key kt + 16 b + 4 g + i, query q0 + 16 s + r; afterwards the probability
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            float mx = -INFINITY;
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (kt + b * 16 + 4 * g + i < lk) mx = fmaxf(mx, sc[b][s][i]);
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mn = fmaxf(m[s], mx);              // finite: key kt is always valid
            const float da = (m[s] - mn) * scale_abs;
            const float alpha = m[s] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(fmaf(da, kLog2eHi, da * kLog2eLo));
            m[s] = mn;
            float ps = 0.f;
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float dx = (sc[b][s][i] - mn) * scale_abs;
                    const float p = (kt + b * 16 + 4 * g + i < lk) ? __builtin_amdgcn_exp2f(fmaf(dx, kLog2eHi, dx * kLog2eLo)) : 0.f;
                    sc[b][s][i] = p;
                    ps += p;
                }
            l[s] = fmaf(l[s], alpha, ps);                  // per-lane partial sum: alpha is the same on the 4 lanes of a query
#pragma unroll
            for (int b = 0; b < OB; ++b) o[s][b] *= alpha;
        }
        __syncthreads();                                   // V tile visible
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int ob = 0; ob < OB; ++ob) {
                    const float va = vs[(16 * b + 4 * g + t) * VLD + 16 * ob + r];
#pragma unroll
                    for (int s = 0; s < QS; ++s) o[s][ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(va, sc[b][s][t], o[s][ob], 0, 0, 0);
                }
    }

#pragma unroll
    for (int s = 0; s < QS; ++s) {
        float L = l[s];
        L += __shfl_xor(L, 16, 64);
        L += __shfl_xor(L, 32, 64);
        const int qi = q0 + s * 16 + r;
        if (qi >= lq) continue;
        const float inv = L > 0.f ? 1.0f / L : 0.f;
        float* op = out + (int64_t)(tq0 + qi) * out_stride + hcol + 4 * g;
#pragma unroll
        for (int b = 0; b < OB; ++b) *reinterpret_cast<float4_t*>(op + 16 * b) = o[s][b] * inv;
        if (lse && g == 0) lse[(int64_t)h * total_q + tq0 + qi] = L > 0.f ? fmaf(m[s], scale_abs, logf(L)) : -INFINITY;
    }
}

// ---- (1b) backward of the bidirectional attention -------------------------------------------------
// Two launches in the forward's wave layout.  P is recomputed from lse, delta = rowsum(dO o O) is computed in f32 in both kernels,
// P and dS are rounded to the storage type before they enter an MFMA (as the forward rounds P).  With dropout, dP <- keep o dP /
// (1 - p), dS = P o (dP - delta), and dV uses the dropped P.
//
// dQ: one wave per (32-query entry, head), loop over the sequence's keys.  S^T = K Q^T and dP^T = V dO^T land in the forward's
// accumulator layout (lane: query l & 15, keys 4 g + i of each 16-key half), dS^T is the B operand of dQ^T = K^T dS^T as it lies in
// the registers, K is staged row-major in LDS and read column-wise (the forward's V path).
template <typename T, int HD, bool DROP>
__global__ __launch_bounds__(64) void bidir_attn_bwd_dq_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, int64_t q_stride, int64_t k_stride,
    int64_t v_stride, const T* __restrict__ out, int64_t out_stride, const T* __restrict__ dout, int64_t dout_stride,
    const float* __restrict__ lse, const int* __restrict__ cu_q, const int* __restrict__ cu_k, const int* __restrict__ tiles,
    float scale, float scale_log2, T* __restrict__ dq, int64_t dq_stride, int64_t total_q, unsigned thr, float inv_keep,
    uint64_t seed) {
    constexpr int QS = kAttnQBlock / 16;
    constexpr int KS = HD / 32;
    constexpr int OB = HD / 16;
    constexpr int VLD = HD + 8;
    constexpr int VCH = kAttnKeys * HD / 8 / 64;
    __shared__ __attribute__((aligned(16))) unsigned short ksm[kAttnKeys * VLD];

    const int entry = blockIdx.x, h = blockIdx.y;
    const int seq = tiles[2 * entry], q0 = tiles[2 * entry + 1];
    const int tq0 = cu_q[seq], lq = cu_q[seq + 1] - tq0;
    const int tk0 = cu_k[seq], lk = cu_k[seq + 1] - tk0;
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const int64_t hcol = (int64_t)h * HD;
    if (lq <= 0) return;

    uint4_t qf[QS][KS], dof[QS][KS];
    float nl[QS], delta[QS];
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        const int qi = min(q0 + s * 16 + r, lq - 1);     // rows past the end: loaded (in bounds), never stored
        const T* qp = q + (int64_t)(tq0 + qi) * q_stride + hcol + 8 * g;
        const T* dop = dout + (int64_t)(tq0 + qi) * dout_stride + hcol + 8 * g;
        const T* op = out + (int64_t)(tq0 + qi) * out_stride + hcol + 8 * g;
        float dl = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qf[s][ks] = *reinterpret_cast<const uint4_t*>(qp + 32 * ks);
            dof[s][ks] = *reinterpret_cast<const uint4_t*>(dop + 32 * ks);
            Vec16<T> a, b;
            a.load(dop + 32 * ks);
            b.load(op + 32 * ks);
#pragma unroll
            for (int e = 0; e < 8; ++e) dl = fmaf(a.v[e], b.v[e], dl);
        }
        dl += __shfl_xor(dl, 16, 64);
        dl += __shfl_xor(dl, 32, 64);
        delta[s] = dl;
        nl[s] = -lse[(int64_t)h * total_q + tq0 + qi] * 1.4426950408889634f;
    }
    float4_t acc[QS][OB];
#pragma unroll
    for (int s = 0; s < QS; ++s)
#pragma unroll
        for (int b = 0; b < OB; ++b) acc[s][b] = float4_t{0.f, 0.f, 0.f, 0.f};

    for (int kt = 0; kt < lk; kt += kAttnKeys) {
        uint4_t kr[VCH];
#pragma unroll
        for (int c = 0; c < VCH; ++c) {
            const int idx = lane + 64 * c, key = idx / (HD / 8), c8 = idx - key * (HD / 8);
            const int kk = min(kt + key, lk - 1);
            kr[c] = *reinterpret_cast<const uint4_t*>(k + (int64_t)(tk0 + kk) * k_stride + hcol + 8 * c8);
        }
        float4_t sc[2][QS], dp[2][QS];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int kk = min(kt + b * 16 + r, lk - 1);
            const T* kp = k + (int64_t)(tk0 + kk) * k_stride + hcol + 8 * g;
            const T* vp = v + (int64_t)(tk0 + kk) * v_stride + hcol + 8 * g;
            uint4_t kf[KS], vf[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                kf[ks] = *reinterpret_cast<const uint4_t*>(kp + 32 * ks);
                vf[ks] = *reinterpret_cast<const uint4_t*>(vp + 32 * ks);
            }
#pragma unroll
            for (int s = 0; s < QS; ++s) {
                sc[b][s] = float4_t{0.f, 0.f, 0.f, 0.f};
                dp[b][s] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    AttnMma<T>::mma(kf[ks], qf[s][ks], sc[b][s]);
                    AttnMma<T>::mma(vf[ks], dof[s][ks], dp[b][s]);
                }
            }
        }
        __syncthreads();                                   // the previous step's K reads are done
#pragma unroll
        for (int c = 0; c < VCH; ++c) {
            const int idx = lane + 64 * c, key = idx / (HD / 8), c8 = idx - key * (HD / 8);
            *reinterpret_cast<uint4_t*>(&ksm[key * VLD + 8 * c8]) = kr[c];
        }
        // dS^T[key kt + 16 b + 4 g + i][query q0 + 16 s + r] = P (dP - delta); masked keys: P = 0
        uint4_t dsf[QS];
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            unsigned w[4];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                float ds[4];
                bool keep[4] = {true, true, true, true};
                if constexpr (DROP) dropout_keep4(dropout_key(seed, h), tq0 + q0 + s * 16 + r, tk0 + kt + b * 16 + 4 * g, thr, keep);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int key = kt + b * 16 + 4 * g + i;
                    const float p = key < lk ? __builtin_amdgcn_exp2f(fmaf(sc[b][s][i], scale_log2, nl[s])) : 0.f;
                    float d = dp[b][s][i];
                    if constexpr (DROP) d = keep[i] ? d * inv_keep : 0.f;
                    ds[i] = p * (d - delta[s]);
                }
                w[2 * b] = pack2<T>(ds[0], ds[1]);
                w[2 * b + 1] = pack2<T>(ds[2], ds[3]);
            }
            dsf[s] = uint4_t{w[0], w[1], w[2], w[3]};
        }
        __syncthreads();                                   // K tile visible
        // A = K^T (row = head dim 16 b + r, k slot j = key 4 g + j for j < 4, 16 + 4 g + j - 4 else), B = dS^T
#pragma unroll
        for (int b = 0; b < OB; ++b) {
            unsigned e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = (j < 4) ? 4 * g + j : 16 + 4 * g + (j - 4);
                e[j] = ksm[key * VLD + 16 * b + r];
            }
            const uint4_t ka{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
#pragma unroll
            for (int s = 0; s < QS; ++s) AttnMma<T>::mma(ka, dsf[s], acc[s][b]);
        }
    }

#pragma unroll
    for (int s = 0; s < QS; ++s) {
        const int qi = q0 + s * 16 + r;
        if (qi >= lq) continue;
        T* op = dq + (int64_t)(tq0 + qi) * dq_stride + hcol + 4 * g;
#pragma unroll
        for (int b = 0; b < OB; ++b) {
            const uint2_t pk{pack2<T>(acc[s][b][0] * scale, acc[s][b][1] * scale), pack2<T>(acc[s][b][2] * scale, acc[s][b][3] * scale)};
            *reinterpret_cast<uint2_t*>(op + 16 * b) = pk;
        }
    }
}

// dK / dV: one wave per (32-key entry, head), loop over the sequence's queries in steps of 32.  The roles of the forward swap: the
// wave keeps its keys' K and V as B operands, S = Q K^T and dP = dO V^T take 16 query rows straight from global memory as A, so
// every lane owns ONE key (column l & 15) and queries 4 g + i of each 16-query half.  The dropped P and dS are the B operands of
// dV^T = dO^T P and dK^T = Q^T dS as they lie in the registers; Q and dO are staged row-major in LDS and read column-wise.
// The step's delta values are computed by lane pairs (query lane >> 1, half of the head dim each) and passed through LDS.
template <typename T, int HD, bool DROP>
__global__ __launch_bounds__(64) void bidir_attn_bwd_dkv_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, int64_t q_stride, int64_t k_stride,
    int64_t v_stride, const T* __restrict__ out, int64_t out_stride, const T* __restrict__ dout, int64_t dout_stride,
    const float* __restrict__ lse, const int* __restrict__ cu_q, const int* __restrict__ cu_k, const int* __restrict__ tiles,
    float scale, float scale_log2, T* __restrict__ dk, int64_t dk_stride, T* __restrict__ dv, int64_t dv_stride, int64_t total_q,
    unsigned thr, float inv_keep, uint64_t seed) {
    constexpr int KT = kAttnQBlock / 16;   // key tiles per wave
    constexpr int KS = HD / 32;
    constexpr int OB = HD / 16;
    constexpr int VLD = HD + 8;
    constexpr int VCH = kAttnKeys * HD / 8 / 64;
    __shared__ __attribute__((aligned(16))) unsigned short qsm[kAttnKeys * VLD];
    __shared__ __attribute__((aligned(16))) unsigned short dosm[kAttnKeys * VLD];
    __shared__ float dlsm[kAttnKeys];

    const int entry = blockIdx.x, h = blockIdx.y;
    const int seq = tiles[2 * entry], k0 = tiles[2 * entry + 1];
    const int tq0 = cu_q[seq], lq = cu_q[seq + 1] - tq0;
    const int tk0 = cu_k[seq], lk = cu_k[seq + 1] - tk0;
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const int64_t hcol = (int64_t)h * HD;
    if (lk <= 0) return;

    uint4_t kf[KT][KS], vf[KT][KS];
#pragma unroll
    for (int s = 0; s < KT; ++s) {
        const int ki = min(k0 + s * 16 + r, lk - 1);     // rows past the end: loaded (in bounds), never stored
        const T* kp = k + (int64_t)(tk0 + ki) * k_stride + hcol + 8 * g;
        const T* vp = v + (int64_t)(tk0 + ki) * v_stride + hcol + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            kf[s][ks] = *reinterpret_cast<const uint4_t*>(kp + 32 * ks);
            vf[s][ks] = *reinterpret_cast<const uint4_t*>(vp + 32 * ks);
        }
    }
    float4_t dka[KT][OB], dva[KT][OB];
#pragma unroll
    for (int s = 0; s < KT; ++s)
#pragma unroll
        for (int b = 0; b < OB; ++b) {
            dka[s][b] = float4_t{0.f, 0.f, 0.f, 0.f};
            dva[s][b] = float4_t{0.f, 0.f, 0.f, 0.f};
        }

    for (int qt = 0; qt < lq; qt += kAttnKeys) {
        uint4_t qr[VCH], dor[VCH];
#pragma unroll
        for (int c = 0; c < VCH; ++c) {
            const int idx = lane + 64 * c, row = idx / (HD / 8), c8 = idx - row * (HD / 8);
            const int qq = min(qt + row, lq - 1);
            qr[c] = *reinterpret_cast<const uint4_t*>(q + (int64_t)(tq0 + qq) * q_stride + hcol + 8 * c8);
            dor[c] = *reinterpret_cast<const uint4_t*>(dout + (int64_t)(tq0 + qq) * dout_stride + hcol + 8 * c8);
        }
        float dl = 0.f;
        {
            const int qq = min(qt + (lane >> 1), lq - 1);
            const T* dop = dout + (int64_t)(tq0 + qq) * dout_stride + hcol + (lane & 1) * (HD / 2);
            const T* op = out + (int64_t)(tq0 + qq) * out_stride + hcol + (lane & 1) * (HD / 2);
#pragma unroll
            for (int c = 0; c < HD / 16; ++c) {
                Vec16<T> a, b;
                a.load(dop + 8 * c);
                b.load(op + 8 * c);
#pragma unroll
                for (int e = 0; e < 8; ++e) dl = fmaf(a.v[e], b.v[e], dl);
            }
            dl += __shfl_xor(dl, 1, 64);
        }
        float4_t sc[2][KT], dp[2][KT];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int qq = min(qt + b * 16 + r, lq - 1);
            const T* qp = q + (int64_t)(tq0 + qq) * q_stride + hcol + 8 * g;
            const T* dop = dout + (int64_t)(tq0 + qq) * dout_stride + hcol + 8 * g;
            uint4_t qa[KS], da[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                qa[ks] = *reinterpret_cast<const uint4_t*>(qp + 32 * ks);
                da[ks] = *reinterpret_cast<const uint4_t*>(dop + 32 * ks);
            }
#pragma unroll
            for (int s = 0; s < KT; ++s) {
                sc[b][s] = float4_t{0.f, 0.f, 0.f, 0.f};
                dp[b][s] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    AttnMma<T>::mma(qa[ks], kf[s][ks], sc[b][s]);
                    AttnMma<T>::mma(da[ks], vf[s][ks], dp[b][s]);
                }
            }
        }
        __syncthreads();                                   // the previous step's LDS reads are done
#pragma unroll
        for (int c = 0; c < VCH; ++c) {
            const int idx = lane + 64 * c, row = idx / (HD / 8), c8 = idx - row * (HD / 8);
            *reinterpret_cast<uint4_t*>(&qsm[row * VLD + 8 * c8]) = qr[c];
            *reinterpret_cast<uint4_t*>(&dosm[row * VLD + 8 * c8]) = dor[c];
        }
        if ((lane & 1) == 0) dlsm[lane >> 1] = dl;
        __syncthreads();                                   // Q, dO tiles and delta visible
        // element [query qt + 16 b + 4 g + i][key k0 + 16 s + r]; queries past the end: P = 0
        float nl[2][4], de[2][4];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int qq = min(qt + b * 16 + 4 * g + i, lq - 1);
                nl[b][i] = -lse[(int64_t)h * total_q + tq0 + qq] * 1.4426950408889634f;
                de[b][i] = dlsm[b * 16 + 4 * g + i];
            }
        uint4_t pf[KT], dsf[KT];
#pragma unroll
        for (int s = 0; s < KT; ++s) {
            unsigned wp[4], wd[4];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                float p[4], ds[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int qq = qt + b * 16 + 4 * g + i;
                    const float pu = qq < lq ? __builtin_amdgcn_exp2f(fmaf(sc[b][s][i], scale_log2, nl[b][i])) : 0.f;
                    float d = dp[b][s][i];
                    p[i] = pu;
                    if constexpr (DROP) {
                        const int krow = tk0 + k0 + s * 16 + r;     // one key, four queries per lane: one evaluation per element
                        const bool keep = dropout_field_keep(dropout_bits(dropout_key(seed, h), tq0 + qq, krow >> 2), krow, thr);
                        d = keep ? d * inv_keep : 0.f;
                        p[i] = keep ? pu : 0.f;
                    }
                    ds[i] = pu * (d - de[b][i]);
                }
                wp[2 * b] = pack2<T>(p[0], p[1]);
                wp[2 * b + 1] = pack2<T>(p[2], p[3]);
                wd[2 * b] = pack2<T>(ds[0], ds[1]);
                wd[2 * b + 1] = pack2<T>(ds[2], ds[3]);
            }
            pf[s] = uint4_t{wp[0], wp[1], wp[2], wp[3]};
            dsf[s] = uint4_t{wd[0], wd[1], wd[2], wd[3]};
        }
        // A = dO^T / Q^T (row = head dim 16 b + r, k slot j = query 4 g + j for j < 4, 16 + 4 g + j - 4 else), B = P / dS
#pragma unroll
        for (int b = 0; b < OB; ++b) {
            unsigned e[8], f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int row = (j < 4) ? 4 * g + j : 16 + 4 * g + (j - 4);
                e[j] = dosm[row * VLD + 16 * b + r];
                f[j] = qsm[row * VLD + 16 * b + r];
            }
            const uint4_t da{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
            const uint4_t qa{f[0] | (f[1] << 16), f[2] | (f[3] << 16), f[4] | (f[5] << 16), f[6] | (f[7] << 16)};
#pragma unroll
            for (int s = 0; s < KT; ++s) {
                AttnMma<T>::mma(da, pf[s], dva[s][b]);
                AttnMma<T>::mma(qa, dsf[s], dka[s][b]);
            }
        }
    }

    const float vscale = DROP ? inv_keep : 1.0f;
#pragma unroll
    for (int s = 0; s < KT; ++s) {
        const int ki = k0 + s * 16 + r;
        if (ki >= lk) continue;
        T* kp = dk + (int64_t)(tk0 + ki) * dk_stride + hcol + 4 * g;
        T* vp = dv + (int64_t)(tk0 + ki) * dv_stride + hcol + 4 * g;
#pragma unroll
        for (int b = 0; b < OB; ++b) {
            const uint2_t pk{pack2<T>(dka[s][b][0] * scale, dka[s][b][1] * scale), pack2<T>(dka[s][b][2] * scale, dka[s][b][3] * scale)};
            const uint2_t pv{pack2<T>(dva[s][b][0] * vscale, dva[s][b][1] * vscale), pack2<T>(dva[s][b][2] * vscale, dva[s][b][3] * vscale)};
            *reinterpret_cast<uint2_t*>(kp + 16 * b) = pk;
            *reinterpret_cast<uint2_t*>(vp + 16 * b) = pv;
        }
    }
}

// the keep mask of one sequence's block, heads head0 .. head0 + nh - 1: mask[head][query][key] (tests and diagnostics)
__global__ __launch_bounds__(256) void dropout_mask_kernel(int q_row0, int k_row0, int lq, int lk, int head0, int nh, unsigned thr,
                                                           uint64_t seed, unsigned char* __restrict__ mask) {
    const int64_t n = (int64_t)nh * lq * lk;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int key = (int)(i % lk), qi = (int)((i / lk) % lq), hh = (int)(i / ((int64_t)lk * lq));
        mask[i] = dropout_keep(seed, head0 + hh, q_row0 + qi, k_row0 + key, thr) ? 1 : 0;
    }
}

// ---- hidden-state dropout inside the row kernels (their DROP = true instances) -------------------------
// keep(seed, site, packed row, column): the attention dropout's stateless function with (site, row, column) in the places of
// (head, query row, key row): key = dropout_key(seed, site), bits = dropout_bits(key, row, column >> 2), one 16-bit field per
// column of the group of 4, KEPT when field >= thr = round(p_drop * 65536).  A lane's 16-byte vector (8 columns) takes two Philox
// evaluations.  site 0 = the embedding output, 1 + 2 i / 2 + 2 i = the two `dropout(dense(..))` of block i; the seed is
// ops.bert_hidden_seed(call seed), which no block's attention seed equals.  A recomputed forward (gradient checkpointing) and the
// backward evaluate the function again: no mask is stored and no generator state is kept.
// Rounding points are those of the unfused path, x -> round(f32(x) * inv_keep) * keep on stored values: the dense output before
// the add (add + LayerNorm), the ROUNDED LayerNorm output (embedding), the rounded ds (backward, towards the dense output).
__device__ __forceinline__ bool hidden_keep(uint64_t seed, int site, int row, int col, unsigned thr) {
    return dropout_field_keep(dropout_bits(dropout_key(seed, site), row, col >> 2), col, thr);
}
// t <- round(t * inv_keep) * keep for the 8 columns c0 .. c0 + 7 (c0 % 8 == 0) of one row; key = dropout_key(seed, site)
template <typename T>
__device__ __forceinline__ void hidden_drop8(Vec16<T>& t, unsigned key, int row, int c0, unsigned thr, float inv_keep) {
    static_assert(Elem<T>::kVec == 8, "the DROP = true instances are the 16-bit ones");
    const DropBits lo = dropout_bits(key, row, c0 >> 2), hi = dropout_bits(key, row, (c0 >> 2) + 1);
#pragma unroll
    for (int e = 0; e < 8; ++e)
        t.v[e] = Elem<T>::round(t.v[e] * inv_keep) * (dropout_field_keep(e < 4 ? lo : hi, c0 + e, thr) ? 1.f : 0.f);
}
// what a DROP = true instance reads (a DROP = false one reads none of it): site = the forwards' site and the backward's site_out,
// site_in = the backward's only
struct RowDrop {
    unsigned thr = 0;
    float inv_keep = 1.0f;
    uint64_t seed = 0;
    int site = 0, site_in = -1;
};

// ---- (2)-(4) row kernels: one wave per row, NV 16-byte vectors per lane ------------------------------
// A row lies in registers as Vec16<T> x[NV]: columns V (lane + 64 j) .. + V - 1, V = Elem<T>::kVec = elements per 16 bytes (8, or
// 4 for f32 storage).
constexpr int kRowThreads = 256;

// mean and rstd of the row in f32, in ONE fixed order (forward and backward take the same two numbers from the same s).
// sum = the lane's part of the row sum, its vectors added in the order j, then e: lane_sum, or vec_sum beside the loads.
template <typename T>
__device__ __forceinline__ void vec_sum(const Vec16<T>& v, float& sum) {
#pragma unroll
    for (int e = 0; e < Elem<T>::kVec; ++e) sum += v.v[e];
}
template <typename T, int NV>
__device__ __forceinline__ float lane_sum(const Vec16<T> (&x)[NV], int d, int lane) {
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
        if (Elem<T>::kVec * (lane + 64 * j) < d) vec_sum<T>(x[j], sum);
    return sum;
}
template <typename T, int NV>
__device__ __forceinline__ void row_stats(const Vec16<T> (&x)[NV], float sum, float eps, int d, int lane, float& mean, float& rstd) {
    constexpr int V = Elem<T>::kVec;
    mean = wave_sum(sum) / (float)d;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
        if (V * (lane + 64 * j) < d)
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float c = x[j].v[e] - mean;
                sq = fmaf(c, c, sq);
            }
    rstd = rsqrtf(wave_sum(sq) / (float)d + eps);
}
// y = (x - mean) rstd gamma + beta, rounded once as it is stored.  A DROP = false instance stores each vector as it is normalised.
// A DROP = true instance leaves the f32 results in x and stores in a pass of its own (which keeps the NV = 8 add + LayerNorm at
// 96 VGPRs = 5 waves per SIMD); DROP_Y (the embedding) drops in that pass: the value as it would be stored, rounded, then
// y = round(that * inv_keep) * keep(site) of row `row`.
template <typename T, int NV, bool DROP, bool DROP_Y>
__device__ __forceinline__ void layernorm_store(Vec16<T> (&x)[NV], const T* __restrict__ gamma, const T* __restrict__ beta,
                                                float eps, T* __restrict__ y, int d, int lane, int row, const RowDrop& drop) {
    constexpr int V = Elem<T>::kVec;
    float mean, rstd;
    row_stats<T, NV>(x, lane_sum<T, NV>(x, d, lane), eps, d, lane, mean, rstd);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c0 = V * (lane + 64 * j);
        if (c0 < d) {
            Vec16<T> gw, bw;
            gw.load(gamma + c0);
            bw.load(beta + c0);
#pragma unroll
            for (int e = 0; e < V; ++e) x[j].v[e] = fmaf((x[j].v[e] - mean) * rstd, gw.v[e], bw.v[e]);
            if constexpr (!DROP) x[j].store(y + c0);
        }
    }
    if constexpr (DROP) {
        const unsigned key = dropout_key(drop.seed, drop.site);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c0 = V * (lane + 64 * j);
            if (c0 < d) {
                if constexpr (DROP_Y) {
#pragma unroll
                    for (int e = 0; e < V; ++e) x[j].v[e] = Elem<T>::round(x[j].v[e]);
                    hidden_drop8<T>(x[j], key, row, c0, drop.thr, drop.inv_keep);
                }
                x[j].store(y + c0);
            }
        }
    }
}

// s = round(a + b), y = LayerNorm(s).  DROP = false: b may be null (s = a) and s is stored where s_out is given (training: the
// backward recomputes the statistics from it).  DROP = true: s = round(a + round(b * inv_keep) * keep(site)); b and s_out required.
template <typename T, int NV, bool DROP>
__global__ __launch_bounds__(kRowThreads) void add_layernorm_kernel(const T* __restrict__ a, int64_t lda, const T* __restrict__ b,
                                                                     int64_t ldb, const T* __restrict__ gamma,
                                                                     const T* __restrict__ beta, float eps, T* __restrict__ y,
                                                                     int64_t ldy, T* __restrict__ s_out, int64_t lds,
                                                                     int64_t rows, int d, RowDrop drop) {
    const int64_t row = (int64_t)blockIdx.x * (kRowThreads / 64) + (threadIdx.x >> 6);
    constexpr int V = Elem<T>::kVec;
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const unsigned key = DROP ? dropout_key(drop.seed, drop.site) : 0u;
    Vec16<T> x[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c0 = V * (lane + 64 * j);
        if (c0 < d) {
            x[j].load(a + row * lda + c0);
            if (DROP || b) {
                Vec16<T> t;
                t.load(b + row * ldb + c0);
                if constexpr (DROP) hidden_drop8<T>(t, key, (int)row, c0, drop.thr, drop.inv_keep);
#pragma unroll
                for (int e = 0; e < V; ++e) x[j].v[e] = Elem<T>::round(x[j].v[e] + t.v[e]);   // the reference's rounded sum
            }
            if (DROP || s_out) x[j].store(s_out + row * lds + c0);
        }
    }
    layernorm_store<T, NV, DROP, false>(x, gamma, beta, eps, y + row * ldy, d, lane, (int)row, drop);
}

// s = round(round(word + type) + position), y = LayerNorm(s); s stored where s_out is given.  DROP = true (s_out required):
// y = round(round(LayerNorm(s)) * inv_keep) * keep(site), the dropout of the LayerNorm output as it would be stored.
template <typename T, int NV, bool DROP>
__global__ __launch_bounds__(kRowThreads) void bert_embed_ln_kernel(
    const int* __restrict__ ids, const int* __restrict__ tts, const int* __restrict__ pos, int64_t tokens,
    const T* __restrict__ word, int64_t vocab, const T* __restrict__ temb, int64_t ntypes, const T* __restrict__ pemb,
    int64_t npos, const T* __restrict__ gamma, const T* __restrict__ beta, float eps, T* __restrict__ y, int64_t ldy, T* __restrict__ s_out,
    int64_t lds, int d, RowDrop drop) {
    const int64_t row = (int64_t)blockIdx.x * (kRowThreads / 64) + (threadIdx.x >> 6);
    constexpr int V = Elem<T>::kVec;
    const int lane = threadIdx.x & 63;
    if (row >= tokens) return;
    // indices are clamped into their tables: an id out of range reads a valid row, never foreign memory (the Python wrapper
    // checks the ranges on the host, where torch's embedding would raise)
    const int64_t wi = clamp_index(ids[row], vocab);
    const int64_t ti = tts ? clamp_index(tts[row], ntypes) : 0;
    const int64_t pi = clamp_index(pos[row], npos);
    Vec16<T> x[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c0 = V * (lane + 64 * j);
        if (c0 < d) {
            Vec16<T> t, p;
            x[j].load(word + wi * d + c0);
            t.load(temb + ti * d + c0);
            p.load(pemb + pi * d + c0);
#pragma unroll
            for (int e = 0; e < V; ++e) x[j].v[e] = Elem<T>::round(Elem<T>::round(x[j].v[e] + t.v[e]) + p.v[e]);   // (w + t) + p
            if (DROP || s_out) x[j].store(s_out + row * lds + c0);
        }
    }
    layernorm_store<T, NV, DROP, DROP>(x, gamma, beta, eps, y + row * ldy, d, lane, (int)row, drop);
}

// exact erf GELU (HF's "gelu"), shared by the in-place and the out-of-place kernel
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }

template <typename T>
__global__ __launch_bounds__(256) void gelu_kernel(T* __restrict__ x, int64_t rows, int64_t cols, int64_t ld) {
    constexpr int V = Elem<T>::kVec;
    const int64_t vpr = cols / V, n = rows * vpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t rr = i / vpr, c = (i - rr * vpr) * V;
        T* p = x + rr * ld + c;
        Vec16<T> t;
        t.load(p);
#pragma unroll
        for (int e = 0; e < V; ++e) t.v[e] = gelu_erf(t.v[e]);
        t.store(p);
    }
}

// backward of LayerNorm(s) gamma + beta from the stored rounded sum s: mean / rstd recomputed per row in f32 exactly as the forward
// takes them, ds = rstd (g - mean(g) - xhat mean(g xhat)) with g = dy gamma, xhat = (s - mean) rstd.  One wave per row, four waves
// per block; wave w of block b walks rows 4 b + w, + 4 gridDim.x, .. with the row in registers and adds dy xhat / dy into per-lane
// f32 sums in that fixed order; the block's four waves then add their sums through LDS in wave order 0, 1, 2, 3 and the last one
// writes dgamma_partial / dbeta_partial [gridDim.x, d], summed by the caller (the dw_partial pattern of rpo_add_rmsnorm_bwd).
// DROP = true adds the dropout of the fused forwards, each a run-time condition: site_in >= 0: dy <- round(dy * inv_keep) *
// keep(site_in) as it is loaded (the embedding: dropout AFTER the LayerNorm); db_out != nullptr: db = round(round(ds) * inv_keep) *
// keep(site) beside ds (add + LayerNorm: ds to a, db to the dense output b).  DROP = false reads neither db_out nor drop.
constexpr int kLnBwdMaxBlocks = 1024;
constexpr int kLnBwdWaves = 4;

template <typename T, int NV, bool DROP>
__global__ __launch_bounds__(64 * kLnBwdWaves) void layernorm_bwd_kernel(
    const T* __restrict__ s, int64_t lds, const T* __restrict__ gamma, const T* __restrict__ dy, int64_t lddy, float eps,
    T* __restrict__ ds, int64_t ldds, float* __restrict__ dgp, float* __restrict__ dbp, int64_t rows, int d,
    T* __restrict__ db_out, int64_t lddb, RowDrop drop) {
    extern __shared__ float ln_red[];       // [2][d]: the block's dgamma | dbeta sums
    constexpr int V = Elem<T>::kVec;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned key_in = DROP ? dropout_key(drop.seed, drop.site_in) : 0u, key_out = DROP ? dropout_key(drop.seed, drop.site) : 0u;
    float dg[NV][V], db[NV][V];
    Vec16<T> gw[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
#pragma unroll
        for (int e = 0; e < V; ++e) dg[j][e] = db[j][e] = 0.f;
        if (V * (lane + 64 * j) < d) gw[j].load(gamma + V * (lane + 64 * j));
    }
    for (int64_t row = (int64_t)blockIdx.x * kLnBwdWaves + wave; row < rows; row += (int64_t)gridDim.x * kLnBwdWaves) {
        Vec16<T> x[NV], g[NV];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c0 = V * (lane + 64 * j);
            if (c0 < d) {
                x[j].load(s + row * lds + c0);
                g[j].load(dy + row * lddy + c0);
                if constexpr (DROP)
                    if (drop.site_in >= 0) hidden_drop8<T>(g[j], key_in, (int)row, c0, drop.thr, drop.inv_keep);
                vec_sum<T>(x[j], sum);
            }
        }
        float mean, rstd;
        row_stats<T, NV>(x, sum, eps, d, lane, mean, rstd);
        float c1 = 0.f, c2 = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j)
            if (V * (lane + 64 * j) < d)
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float xh = (x[j].v[e] - mean) * rstd, dyv = g[j].v[e], gg = dyv * gw[j].v[e];
                    dg[j][e] = fmaf(dyv, xh, dg[j][e]);
                    db[j][e] += dyv;
                    x[j].v[e] = xh;
                    g[j].v[e] = gg;
                    c1 += gg;
                    c2 = fmaf(gg, xh, c2);
                }
        c1 = wave_sum(c1) / (float)d;
        c2 = wave_sum(c2) / (float)d;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c0 = V * (lane + 64 * j);
            if (c0 < d) {
#pragma unroll
                for (int e = 0; e < V; ++e) g[j].v[e] = rstd * (g[j].v[e] - c1 - x[j].v[e] * c2);
                g[j].store(ds + row * ldds + c0);
                if constexpr (DROP)
                    if (db_out) {
#pragma unroll
                        for (int e = 0; e < V; ++e) g[j].v[e] = Elem<T>::round(g[j].v[e]);      // ds as stored
                        hidden_drop8<T>(g[j], key_out, (int)row, c0, drop.thr, drop.inv_keep);
                        g[j].store(db_out + row * lddb + c0);
                    }
            }
        }
    }
    for (int w = 0; w < kLnBwdWaves; ++w) {
        if (wave == w) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int c0 = V * (lane + 64 * j);
                if (c0 < d) {
                    float* gl = ln_red + c0;
                    float* bl = ln_red + d + c0;
                    float* gp = dgp + (int64_t)blockIdx.x * d + c0;
                    float* bp = dbp + (int64_t)blockIdx.x * d + c0;
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        const float a = w == 0 ? dg[j][e] : gl[e] + dg[j][e];
                        const float b = w == 0 ? db[j][e] : bl[e] + db[j][e];
                        if (w == kLnBwdWaves - 1) {
                            gp[e] = a;
                            bp[e] = b;
                        } else {
                            gl[e] = a;
                            bl[e] = b;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

// h = gelu(u) out of place: the pre-activation survives for the backward
template <typename T>
__global__ __launch_bounds__(256) void gelu_out_kernel(const T* __restrict__ u, int64_t ldu, T* __restrict__ hh, int64_t ldh,
                                                       int64_t rows, int64_t cols) {
    const int64_t vpr = cols / 8, n = rows * vpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t rr = i / vpr, c = (i - rr * vpr) * 8;
        Vec16<T> t;
        t.load(u + rr * ldu + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) t.v[e] = gelu_erf(t.v[e]);
        t.store(hh + rr * ldh + c);
    }
}

// du = dh (Phi(u) + u phi(u)): Phi = erfc(-u / sqrt 2) / 2 (no cancellation in the left tail), phi = exp(-u^2 / 2) / sqrt(2 pi).
// phi is taken as (c e) e with e = exp2(-u^2 log2(e) / 4) = sqrt(exp(-u^2 / 2)): the hardware exp2 returns 0 where its result would
// be a subnormal f32, which exp(-u^2 / 2) is for |u| > 13.2, where u phi is nearly all of du and bf16 (f32's exponent range) still
// holds it; e stays normal up to |u| = 18.7, beyond which phi is below the smallest subnormal, and the last multiply rounds into the
// subnormals.  The same number of operations as c * __expf(-0.5 u u): the two constants of the exponent are folded into one.
template <typename T>
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const T* __restrict__ u, int64_t ldu, const T* __restrict__ dh, int64_t lddh,
                                                       T* __restrict__ du, int64_t lddu, int64_t rows, int64_t cols) {
    const int64_t vpr = cols / 8, n = rows * vpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t rr = i / vpr, c = (i - rr * vpr) * 8;
        Vec16<T> t, gvec;
        t.load(u + rr * ldu + c);
        gvec.load(dh + rr * lddh + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float x = t.v[e];
            const float cdf = 0.5f * erfcf(-x * 0.70710678118654752f);
            const float h = __builtin_amdgcn_exp2f(x * x * -0.36067376022224085f);       // -log2(e) / 4
            const float pdf = 0.3989422804014327f * h * h;
            t.v[e] = gvec.v[e] * fmaf(x, pdf, cdf);
        }
        t.store(du + rr * lddu + c);
    }
}

// the keep mask of rows row0 .. row0 + rows - 1, columns 0 .. d - 1 of one site: mask[row][column] (tests and diagnostics)
__global__ __launch_bounds__(256) void hidden_dropout_mask_kernel(int row0, int rows, int d, int site, unsigned thr, uint64_t seed,
                                                                  unsigned char* __restrict__ mask) {
    const int64_t n = (int64_t)rows * d;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        mask[i] = hidden_keep(seed, site, row0 + (int)(i / d), (int)(i % d), thr) ? 1 : 0;
}

// ---- host side: the argument checks and the dispatch that the entries share -----------------------------
// An entry answers INVALID_ARG before UNSUPPORTED.  Each helper returns the status of ONE group of arguments; first_error keeps
// that order over the groups of an entry.
int first_error(std::initializer_list<int> groups) {
    int rc = RPO_OK;
    for (const int s : groups) {
        if (s == RPO_ERR_INVALID_ARG) return s;
        if (s != RPO_OK) rc = s;
    }
    return rc;
}
// NV of the row kernels: 1, 2, 4 or 8 vectors of 8 elements, up to 16 of 4 on f32 storage (d <= 4096); 0 = too wide
int row_vectors(int64_t d, bool f32) {
    const int64_t nv = rpo_cdiv(d, f32 ? 256 : 512);
    return nv <= 1 ? 1 : nv <= 2 ? 2 : nv <= 4 ? 4 : nv <= 8 ? 8 : (f32 && nv <= 16) ? 16 : 0;
}
// rows x d of a row entry; nv = 0: too wide.  dtype is the entry's argument, or RPO_DT_F32 from an _f32 entry (f32_entry): the
// 16-bit entries answer RPO_DT_F32 with UNSUPPORTED.
int row_shape(int64_t rows, int64_t d, int dtype, bool f32_entry, int nv) {
    if (rows < 0 || d <= 0 || !rpo_dtype_ok(dtype)) return RPO_ERR_INVALID_ARG;
    return ((dtype == RPO_DT_F32) != f32_entry || d % 8 || nv == 0) ? RPO_ERR_UNSUPPORTED : RPO_OK;
}
// a [rows, d] operand with row stride ld; vec = elements per 16 bytes
int row_operand(const void* p, int64_t ld, int64_t d, int vec) {
    if (!p || ld < d) return RPO_ERR_INVALID_ARG;
    return (!rpo_aligned16(p) || ld % vec) ? RPO_ERR_UNSUPPORTED : RPO_OK;
}
// gamma, beta, an embedding table
int vec_operand(const void* p) { return !p ? RPO_ERR_INVALID_ARG : !rpo_aligned16(p) ? RPO_ERR_UNSUPPORTED : RPO_OK; }
int embed_tables(const int* ids, const int* pos, const void* word, int64_t vocab, const void* type_emb, int64_t n_types,
                 const void* pos_emb, int64_t n_pos) {
    if (!ids || !pos || vocab <= 0 || n_types <= 0 || n_pos <= 0) return RPO_ERR_INVALID_ARG;
    return first_error({vec_operand(word), vec_operand(type_emb), vec_operand(pos_emb)});
}

bool attn_common_ok(int64_t num_heads, int64_t num_kv_heads, int64_t head_dim, int dtype, int64_t tile_cols, int64_t block,
                    int64_t ntiles) {
    return !(dtype == RPO_DT_F32 || (head_dim != 32 && head_dim != 64) || num_heads != num_kv_heads || tile_cols != 2 ||
             block != kAttnQBlock || ntiles > 0x7fffffff || num_heads > 65535);
}
bool dropout_args(float p_drop, unsigned* thr, float* inv_keep) {      // false: p_drop outside [0, 1)
    if (!(p_drop >= 0.f) || !(p_drop < 1.f)) return false;
    *thr = (unsigned)lrintf(p_drop * 65536.f);
    *inv_keep = 1.0f / (1.0f - p_drop);
    return true;
}
// thr / inv_keep of the row kernels: p_drop below 2^-17 quantises to thr = 0 = no dropout, and then nothing is scaled either
bool hidden_dropout_args(float p_drop, unsigned* thr, float* inv_keep) {
    if (!dropout_args(p_drop, thr, inv_keep)) return false;
    if (*thr == 0) *inv_keep = 1.0f;
    return true;
}
constexpr int64_t kHiddenMaxSite = 1 << 20;     // a site is a small layer index; the bound only keeps it an int
// dropout and site of a drop entry -> *drop.  Only these entries bound rows: the keep function takes the row as an int.
int drop_args(int64_t rows, float p_drop, uint64_t seed, int64_t site, RowDrop* drop) {
    if (rows > 0x7fffffff || site < 0 || site > kHiddenMaxSite || !hidden_dropout_args(p_drop, &drop->thr, &drop->inv_keep))
        return RPO_ERR_INVALID_ARG;
    drop->seed = seed;
    drop->site = (int)site;
    return RPO_OK;
}

// f(TypeTag<T>) with T from dtype; F32 = false leaves float out of the instances (the 16-bit entries never reach it)
template <typename T> struct TypeTag { using type = T; };
template <bool F32, typename F> void dtype_dispatch(int dtype, F f) {
    if (dtype == RPO_DT_BF16) f(TypeTag<bf16_t>{});
    else if (dtype == RPO_DT_F16) f(TypeTag<f16_t>{});
    else if constexpr (F32) f(TypeTag<float>{});
}
// f(integral_constant<NV>) with NV = nv from row_vectors; 16 exists on f32 storage only
template <typename T, typename F> void nv_dispatch(int nv, F f) {
    if (nv == 1) f(std::integral_constant<int, 1>{});
    else if (nv == 2) f(std::integral_constant<int, 2>{});
    else if (nv == 4) f(std::integral_constant<int, 4>{});
    else if (sizeof(T) != 4 || nv == 8) f(std::integral_constant<int, 8>{});
    else if constexpr (sizeof(T) == 4) f(std::integral_constant<int, 16>{});
}

}  // namespace

// launch KERNEL<T> resp. KERNEL<T, NV, DROP>: T from DTYPE (F32: float included), NV from row_vectors; the arguments may name T
#define RPO_TYPE_DISPATCH(F32, DTYPE, KERNEL, GRID, BLOCK, LDS, ST, ...)               \
    dtype_dispatch<F32>(DTYPE, [&](auto tag_) {                                        \
        using T = typename decltype(tag_)::type;                                       \
        RPO_LAUNCH(KERNEL<T>, GRID, BLOCK, LDS, ST, __VA_ARGS__);                      \
    })
#define RPO_ROW_DISPATCH(F32, DTYPE, NV, KERNEL, DROP, GRID, BLOCK, LDS, ST, ...)                                     \
    dtype_dispatch<F32>(DTYPE, [&](auto tag_) {                                                                       \
        using T = typename decltype(tag_)::type;                                                                      \
        nv_dispatch<T>(NV, [&](auto nv_) {                                                                            \
            RPO_LAUNCH((KERNEL<T, decltype(nv_)::value, DROP>), GRID, BLOCK, LDS, ST, __VA_ARGS__);                   \
        });                                                                                                           \
    })
#define RPO_ATTN_DISPATCH(LAUNCH)                           \
    do {                                                    \
        if (dtype == RPO_DT_BF16) {                         \
            if (head_dim == 32) LAUNCH(bf16_t, 32);         \
            else LAUNCH(bf16_t, 64);                        \
        } else {                                            \
            if (head_dim == 32) LAUNCH(f16_t, 32);          \
            else LAUNCH(f16_t, 64);                         \
        }                                                   \
    } while (0)

namespace {

// rpo_bidir_attn_fwd (thr = 0, lse may be null) and rpo_bidir_attn_train_fwd: thr > 0 takes the DROP = true instance
int bidir_attn_fwd_launch(const void* q, const void* k, const void* v, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                          const int* cu_seqlens_q, const int* cu_seqlens_k, const int* tiles, int64_t ntiles, int64_t tile_cols,
                          int64_t q_block, int64_t total_q, int64_t num_heads, int64_t num_kv_heads, int64_t head_dim, int dtype,
                          float scale, void* out, int64_t out_stride, float* lse, unsigned thr, float inv_keep, uint64_t seed,
                          rpo_stream_t stream) {
    if (!q || !k || !v || !cu_seqlens_q || !cu_seqlens_k || !tiles || !out || ntiles < 0 || total_q <= 0 || num_heads <= 0 ||
        num_kv_heads <= 0 || head_dim <= 0 || !rpo_dtype_ok(dtype) || q_stride <= 0 || k_stride <= 0 || v_stride <= 0 ||
        out_stride <= 0)
        return RPO_ERR_INVALID_ARG;
    if (!attn_common_ok(num_heads, num_kv_heads, head_dim, dtype, tile_cols, q_block, ntiles)) return RPO_ERR_UNSUPPORTED;
    if (!rpo_aligned16(q) || !rpo_aligned16(k) || !rpo_aligned16(v) || (reinterpret_cast<uintptr_t>(out) & 7) || q_stride % 8 ||
        k_stride % 8 || v_stride % 8 || out_stride % 4)
        return RPO_ERR_UNSUPPORTED;
    if (ntiles == 0) return RPO_OK;
    const dim3 grid((unsigned)ntiles, (unsigned)num_heads), block(64);
    hipStream_t st = (hipStream_t)stream;
    const float sl = scale * 1.4426950408889634f;
#define RPO_BIDIR_ARGS(T)                                                                                                    \
    grid, block, 0, st, (const T*)q, (const T*)k, (const T*)v, q_stride, k_stride, v_stride, cu_seqlens_q, cu_seqlens_k, tiles, \
        sl, (T*)out, out_stride, lse, total_q
#define RPO_BIDIR(T, HD)                                                                                           \
    do {                                                                                                           \
        if (thr > 0) RPO_LAUNCH((bidir_attn_fwd_kernel<T, HD, true>), RPO_BIDIR_ARGS(T), thr, inv_keep, seed);     \
        else RPO_LAUNCH((bidir_attn_fwd_kernel<T, HD, false>), RPO_BIDIR_ARGS(T), 0u, 1.0f, (uint64_t)0);          \
    } while (0)
    RPO_ATTN_DISPATCH(RPO_BIDIR);
#undef RPO_BIDIR
#undef RPO_BIDIR_ARGS
    return rpo_launch_status();
}

// the add + LayerNorm entries.  train: s is stored (required); DROP: b is required and drop / drop_rc come from drop_args
template <bool F32, bool DROP>
int add_layernorm(const void* a, int64_t lda, const void* b, int64_t ldb, const void* gamma, const void* beta, float eps, void* y,
                  int64_t ldy, void* s, int64_t lds, bool train, int64_t rows, int64_t d, int dtype, int drop_rc, RowDrop drop,
                  rpo_stream_t stream) {
    const int vec = F32 ? 4 : 8, nv = row_vectors(d, F32);
    const int rc = first_error({row_shape(rows, d, dtype, F32, nv), row_operand(a, lda, d, vec),
                                (DROP || b) ? row_operand(b, ldb, d, vec) : RPO_OK, vec_operand(gamma), vec_operand(beta),
                                row_operand(y, ldy, d, vec), train ? row_operand(s, lds, d, vec) : RPO_OK, drop_rc});
    if (rc != RPO_OK || rows == 0) return rc;
    RPO_ROW_DISPATCH(F32, dtype, nv, add_layernorm_kernel, DROP, dim3((unsigned)rpo_cdiv(rows, kRowThreads / 64)), dim3(kRowThreads),
                     0, (hipStream_t)stream, (const T*)a, lda, (const T*)b, ldb, (const T*)gamma, (const T*)beta, eps, (T*)y, ldy,
                     (T*)s, lds, rows, (int)d, drop);
    return rpo_launch_status();
}

// the embedding + LayerNorm entries, as add_layernorm
template <bool F32, bool DROP>
int bert_embed_ln(const int* ids, const int* token_types, const int* pos, int64_t tokens, const void* word, int64_t vocab,
                  const void* type_emb, int64_t n_types, const void* pos_emb, int64_t n_pos, const void* gamma, const void* beta,
                  float eps, void* y, int64_t ldy, void* s, int64_t lds, bool train, int64_t d, int dtype, int drop_rc, RowDrop drop,
                  rpo_stream_t stream) {
    const int vec = F32 ? 4 : 8, nv = row_vectors(d, F32);
    const int rc = first_error({row_shape(tokens, d, dtype, F32, nv),
                                embed_tables(ids, pos, word, vocab, type_emb, n_types, pos_emb, n_pos), vec_operand(gamma),
                                vec_operand(beta), row_operand(y, ldy, d, vec), train ? row_operand(s, lds, d, vec) : RPO_OK, drop_rc});
    if (rc != RPO_OK || tokens == 0) return rc;
    RPO_ROW_DISPATCH(F32, dtype, nv, bert_embed_ln_kernel, DROP, dim3((unsigned)rpo_cdiv(tokens, kRowThreads / 64)),
                     dim3(kRowThreads), 0, (hipStream_t)stream, ids, token_types, pos, tokens, (const T*)word, vocab,
                     (const T*)type_emb, n_types, (const T*)pos_emb, n_pos, (const T*)gamma, (const T*)beta, eps, (T*)y, ldy, (T*)s,
                     lds, (int)d, drop);
    return rpo_launch_status();
}

// grid of the GELU kernels: a grid-stride loop over the 16-byte vectors of rows x cols, 256 threads per block
dim3 gelu_grid(int64_t rows, int64_t cols, int vec) {
    const int64_t nb = rpo_cdiv(rows * (cols / vec), 256);
    return dim3((unsigned)(nb < 8192 ? nb : 8192));
}

}  // namespace

extern "C" int rpo_bidir_attn_fwd(const void* q, const void* k, const void* v, int64_t q_stride, int64_t k_stride,
                                  int64_t v_stride, const int* cu_seqlens_q, const int* cu_seqlens_k, const int* tiles,
                                  int64_t ntiles, int64_t tile_cols, int64_t q_block, int64_t total_q, int64_t num_heads,
                                  int64_t num_kv_heads, int64_t head_dim, int dtype, float scale, void* out,
                                  int64_t out_stride, float* lse, rpo_stream_t stream) {
    return bidir_attn_fwd_launch(q, k, v, q_stride, k_stride, v_stride, cu_seqlens_q, cu_seqlens_k, tiles, ntiles, tile_cols, q_block,
                                 total_q, num_heads, num_kv_heads, head_dim, dtype, scale, out, out_stride, lse, 0u, 1.0f, 0, stream);
}

extern "C" int rpo_add_layernorm_fwd(const void* a, int64_t lda, const void* b, int64_t ldb, const void* gamma, const void* beta,
                                     float eps, void* y, int64_t ldy, int64_t rows, int64_t d, int dtype, rpo_stream_t stream) {
    return add_layernorm<false, false>(a, lda, b, ldb, gamma, beta, eps, y, ldy, nullptr, 0, false, rows, d, dtype, RPO_OK, RowDrop{},
                                       stream);
}

extern "C" int rpo_gelu_fwd(void* x, int64_t rows, int64_t cols, int64_t ld, int dtype, rpo_stream_t stream) {
    const int rc = first_error({row_shape(rows, cols, dtype, false, 1), row_operand(x, ld, cols, 8)});
    if (rc != RPO_OK || rows == 0) return rc;
    RPO_TYPE_DISPATCH(false, dtype, gelu_kernel, gelu_grid(rows, cols, 8), dim3(256), 0, (hipStream_t)stream, (T*)x, rows, cols, ld);
    return rpo_launch_status();
}

extern "C" int rpo_bert_embed_ln_fwd(const int* ids, const int* token_types, const int* pos, int64_t tokens, const void* word,
                                     int64_t vocab, const void* type_emb, int64_t n_types, const void* pos_emb, int64_t n_pos,
                                     const void* gamma, const void* beta, float eps, void* y, int64_t ldy, int64_t d, int dtype,
                                     rpo_stream_t stream) {
    return bert_embed_ln<false, false>(ids, token_types, pos, tokens, word, vocab, type_emb, n_types, pos_emb, n_pos, gamma, beta, eps,
                                       y, ldy, nullptr, 0, false, d, dtype, RPO_OK, RowDrop{}, stream);
}

// ---- f32 storage (header section 9b): entries of their own; the ones above keep answering RPO_DT_F32 with UNSUPPORTED --------

extern "C" int rpo_bidir_attn_fwd_f32(const void* q, const void* k, const void* v, int64_t q_stride, int64_t k_stride,
                                      int64_t v_stride, const int* cu_seqlens_q, const int* cu_seqlens_k, const int* tiles,
                                      int64_t ntiles, int64_t tile_cols, int64_t q_block, int64_t total_q, int64_t num_heads,
                                      int64_t num_kv_heads, int64_t head_dim, float scale, void* out, int64_t out_stride,
                                      float* lse, rpo_stream_t stream) {
    if (!q || !k || !v || !cu_seqlens_q || !cu_seqlens_k || !tiles || !out || ntiles < 0 || total_q <= 0 || num_heads <= 0 ||
        num_kv_heads <= 0 || head_dim <= 0 || q_stride <= 0 || k_stride <= 0 || v_stride <= 0 || out_stride <= 0 ||
        !(fabsf(scale) <= 3.0e38f))
        return RPO_ERR_INVALID_ARG;
    if ((head_dim != 32 && head_dim != 64) || num_heads != num_kv_heads || tile_cols != 2 || q_block != kAttnQBlock ||
        ntiles > 0x7fffffff || num_heads > 65535)
        return RPO_ERR_UNSUPPORTED;
    if (!rpo_aligned16(q) || !rpo_aligned16(k) || !rpo_aligned16(v) || !rpo_aligned16(out) || q_stride % 4 || k_stride % 4 ||
        v_stride % 4 || out_stride % 4)
        return RPO_ERR_UNSUPPORTED;
    if (ntiles == 0) return RPO_OK;
    const dim3 grid((unsigned)ntiles, (unsigned)num_heads), block(64);
    hipStream_t st = (hipStream_t)stream;
    const float sa = fabsf(scale), sgn = scale < 0.f ? -1.0f : 1.0f;
    if (head_dim == 32)
        RPO_LAUNCH(bidir_attn_fwd_f32_kernel<32>, grid, block, 0, st, (const float*)q, (const float*)k, (const float*)v, q_stride,
                   k_stride, v_stride, cu_seqlens_q, cu_seqlens_k, tiles, sa, sgn, (float*)out, out_stride, lse, total_q);
    else
        RPO_LAUNCH(bidir_attn_fwd_f32_kernel<64>, grid, block, 0, st, (const float*)q, (const float*)k, (const float*)v, q_stride,
                   k_stride, v_stride, cu_seqlens_q, cu_seqlens_k, tiles, sa, sgn, (float*)out, out_stride, lse, total_q);
    return rpo_launch_status();
}

extern "C" int rpo_add_layernorm_fwd_f32(const void* a, int64_t lda, const void* b, int64_t ldb, const void* gamma,
                                         const void* beta, float eps, void* y, int64_t ldy, int64_t rows, int64_t d,
                                         rpo_stream_t stream) {
    return add_layernorm<true, false>(a, lda, b, ldb, gamma, beta, eps, y, ldy, nullptr, 0, false, rows, d, RPO_DT_F32, RPO_OK,
                                      RowDrop{}, stream);
}

extern "C" int rpo_gelu_fwd_f32(void* x, int64_t rows, int64_t cols, int64_t ld, rpo_stream_t stream) {
    const int rc = first_error({row_shape(rows, cols, RPO_DT_F32, true, 1), row_operand(x, ld, cols, 4)});
    if (rc != RPO_OK || rows == 0) return rc;
    RPO_LAUNCH(gelu_kernel<float>, gelu_grid(rows, cols, 4), dim3(256), 0, (hipStream_t)stream, (float*)x, rows, cols, ld);
    return rpo_launch_status();
}

extern "C" int rpo_bert_embed_ln_fwd_f32(const int* ids, const int* token_types, const int* pos, int64_t tokens, const void* word,
                                         int64_t vocab, const void* type_emb, int64_t n_types, const void* pos_emb, int64_t n_pos,
                                         const void* gamma, const void* beta, float eps, void* y, int64_t ldy, int64_t d,
                                         rpo_stream_t stream) {
    return bert_embed_ln<true, false>(ids, token_types, pos, tokens, word, vocab, type_emb, n_types, pos_emb, n_pos, gamma, beta, eps,
                                      y, ldy, nullptr, 0, false, d, RPO_DT_F32, RPO_OK, RowDrop{}, stream);
}

// ---- training entries ---------------------------------------------------------------------------------
extern "C" int rpo_bidir_attn_train_fwd(const void* q, const void* k, const void* v, int64_t q_stride, int64_t k_stride,
                                        int64_t v_stride, const int* cu_seqlens_q, const int* cu_seqlens_k, const int* tiles,
                                        int64_t ntiles, int64_t tile_cols, int64_t q_block, int64_t total_q, int64_t num_heads,
                                        int64_t num_kv_heads, int64_t head_dim, int dtype, float scale, float p_drop,
                                        uint64_t seed, void* out, int64_t out_stride, float* lse, rpo_stream_t stream) {
    unsigned thr;
    float inv_keep;
    if (!lse || !dropout_args(p_drop, &thr, &inv_keep)) return RPO_ERR_INVALID_ARG;
    return bidir_attn_fwd_launch(q, k, v, q_stride, k_stride, v_stride, cu_seqlens_q, cu_seqlens_k, tiles, ntiles, tile_cols, q_block,
                                 total_q, num_heads, num_kv_heads, head_dim, dtype, scale, out, out_stride, lse, thr, inv_keep, seed,
                                 stream);
}

extern "C" int rpo_bidir_attn_bwd(const void* q, const void* k, const void* v, int64_t q_stride, int64_t k_stride,
                                  int64_t v_stride, const void* out, int64_t out_stride, const void* dout, int64_t dout_stride,
                                  const float* lse, const int* cu_seqlens_q, const int* cu_seqlens_k, const int* q_tiles,
                                  int64_t n_q_tiles, const int* k_tiles, int64_t n_k_tiles, int64_t tile_cols, int64_t block_rows,
                                  int64_t total_q, int64_t num_heads, int64_t num_kv_heads, int64_t head_dim, int dtype,
                                  float scale, float p_drop, uint64_t seed, void* dq, int64_t dq_stride, void* dk,
                                  int64_t dk_stride, void* dv, int64_t dv_stride, rpo_stream_t stream) {
    unsigned thr;
    float inv_keep;
    if (!q || !k || !v || !out || !dout || !lse || !cu_seqlens_q || !cu_seqlens_k || !q_tiles || !k_tiles || !dq || !dk || !dv ||
        n_q_tiles < 0 || n_k_tiles < 0 || total_q <= 0 || num_heads <= 0 || num_kv_heads <= 0 || head_dim <= 0 ||
        !rpo_dtype_ok(dtype) || q_stride <= 0 || k_stride <= 0 || v_stride <= 0 || out_stride <= 0 || dout_stride <= 0 ||
        dq_stride <= 0 || dk_stride <= 0 || dv_stride <= 0 || !dropout_args(p_drop, &thr, &inv_keep))
        return RPO_ERR_INVALID_ARG;
    if (!attn_common_ok(num_heads, num_kv_heads, head_dim, dtype, tile_cols, block_rows, n_q_tiles) || n_k_tiles > 0x7fffffff)
        return RPO_ERR_UNSUPPORTED;
    if (!rpo_aligned16(q) || !rpo_aligned16(k) || !rpo_aligned16(v) || !rpo_aligned16(out) || !rpo_aligned16(dout) ||
        (reinterpret_cast<uintptr_t>(dq) & 7) || (reinterpret_cast<uintptr_t>(dk) & 7) || (reinterpret_cast<uintptr_t>(dv) & 7) ||
        q_stride % 8 || k_stride % 8 || v_stride % 8 || out_stride % 8 || dout_stride % 8 || dq_stride % 4 || dk_stride % 4 ||
        dv_stride % 4)
        return RPO_ERR_UNSUPPORTED;
    const dim3 block(64);
    hipStream_t st = (hipStream_t)stream;
    const float sl = scale * 1.4426950408889634f;
    const bool drop = thr > 0;
#define RPO_BIDIR_DQ(T, HD)                                                                                                      \
    do {                                                                                                                         \
        if (drop)                                                                                                                \
            RPO_LAUNCH((bidir_attn_bwd_dq_kernel<T, HD, true>), grid, block, 0, st, (const T*)q, (const T*)k, (const T*)v,       \
                       q_stride, k_stride, v_stride, (const T*)out, out_stride, (const T*)dout, dout_stride, lse, cu_seqlens_q,  \
                       cu_seqlens_k, q_tiles, scale, sl, (T*)dq, dq_stride, total_q, thr, inv_keep, seed);                       \
        else                                                                                                                     \
            RPO_LAUNCH((bidir_attn_bwd_dq_kernel<T, HD, false>), grid, block, 0, st, (const T*)q, (const T*)k, (const T*)v,      \
                       q_stride, k_stride, v_stride, (const T*)out, out_stride, (const T*)dout, dout_stride, lse, cu_seqlens_q,  \
                       cu_seqlens_k, q_tiles, scale, sl, (T*)dq, dq_stride, total_q, 0u, 1.0f, (uint64_t)0);                     \
    } while (0)
#define RPO_BIDIR_DKV(T, HD)                                                                                                     \
    do {                                                                                                                         \
        if (drop)                                                                                                                \
            RPO_LAUNCH((bidir_attn_bwd_dkv_kernel<T, HD, true>), grid, block, 0, st, (const T*)q, (const T*)k, (const T*)v,      \
                       q_stride, k_stride, v_stride, (const T*)out, out_stride, (const T*)dout, dout_stride, lse, cu_seqlens_q,  \
                       cu_seqlens_k, k_tiles, scale, sl, (T*)dk, dk_stride, (T*)dv, dv_stride, total_q, thr, inv_keep, seed);    \
        else                                                                                                                     \
            RPO_LAUNCH((bidir_attn_bwd_dkv_kernel<T, HD, false>), grid, block, 0, st, (const T*)q, (const T*)k, (const T*)v,     \
                       q_stride, k_stride, v_stride, (const T*)out, out_stride, (const T*)dout, dout_stride, lse, cu_seqlens_q,  \
                       cu_seqlens_k, k_tiles, scale, sl, (T*)dk, dk_stride, (T*)dv, dv_stride, total_q, 0u, 1.0f, (uint64_t)0);  \
    } while (0)
    if (n_q_tiles > 0) {
        const dim3 grid((unsigned)n_q_tiles, (unsigned)num_heads);
        RPO_ATTN_DISPATCH(RPO_BIDIR_DQ);
        const int rc = rpo_launch_status();
        if (rc != RPO_OK) return rc;
    }
    if (n_k_tiles > 0) {
        const dim3 grid((unsigned)n_k_tiles, (unsigned)num_heads);
        RPO_ATTN_DISPATCH(RPO_BIDIR_DKV);
        return rpo_launch_status();
    }
#undef RPO_BIDIR_DQ
#undef RPO_BIDIR_DKV
    return RPO_OK;
}

extern "C" int rpo_bidir_attn_dropout_mask(int64_t q_row0, int64_t k_row0, int64_t len_q, int64_t len_k, int64_t head0,
                                           int64_t num_heads, float p_drop, uint64_t seed, unsigned char* mask,
                                           rpo_stream_t stream) {
    unsigned thr;
    float inv_keep;
    if (!mask || q_row0 < 0 || k_row0 < 0 || len_q < 0 || len_k < 0 || head0 < 0 || num_heads < 0 ||
        q_row0 + len_q > 0x7fffffff || k_row0 + len_k > 0x7fffffff || head0 + num_heads > 65535 ||
        !dropout_args(p_drop, &thr, &inv_keep))
        return RPO_ERR_INVALID_ARG;
    const int64_t n = num_heads * len_q * len_k;
    if (n == 0) return RPO_OK;
    const int64_t nb = rpo_cdiv(n, 256);
    RPO_LAUNCH(dropout_mask_kernel, dim3((unsigned)(nb < 65536 ? nb : 65536)), dim3(256), 0, (hipStream_t)stream, (int)q_row0,
               (int)k_row0, (int)len_q, (int)len_k, (int)head0, (int)num_heads, thr, seed, mask);
    return rpo_launch_status();
}

extern "C" int rpo_add_layernorm_train_fwd(const void* a, int64_t lda, const void* b, int64_t ldb, const void* gamma,
                                           const void* beta, float eps, void* y, int64_t ldy, void* s, int64_t lds, int64_t rows,
                                           int64_t d, int dtype, rpo_stream_t stream) {
    return add_layernorm<false, false>(a, lda, b, ldb, gamma, beta, eps, y, ldy, s, lds, true, rows, d, dtype, RPO_OK, RowDrop{},
                                       stream);
}

extern "C" int rpo_bert_embed_ln_train_fwd(const int* ids, const int* token_types, const int* pos, int64_t tokens,
                                           const void* word, int64_t vocab, const void* type_emb, int64_t n_types,
                                           const void* pos_emb, int64_t n_pos, const void* gamma, const void* beta, float eps,
                                           void* y, int64_t ldy, void* s, int64_t lds, int64_t d, int dtype, rpo_stream_t stream) {
    return bert_embed_ln<false, false>(ids, token_types, pos, tokens, word, vocab, type_emb, n_types, pos_emb, n_pos, gamma, beta, eps,
                                       y, ldy, s, lds, true, d, dtype, RPO_OK, RowDrop{}, stream);
}

extern "C" int rpo_layernorm_bwd_blocks(int64_t rows) {
    const int64_t nb = rpo_cdiv(rows < 1 ? 1 : rows, kLnBwdWaves);
    return (int)(nb < kLnBwdMaxBlocks ? nb : kLnBwdMaxBlocks);
}

namespace {
// rpo_layernorm_bwd (db = nullptr) and rpo_layernorm_drop_bwd; entry_rc = what only the one entry checks
template <bool DROP>
int layernorm_bwd(const void* s, int64_t lds, const void* gamma, const void* dy, int64_t lddy, float eps, void* ds, int64_t ldds,
                  void* db, int64_t lddb, float* dgamma_partial, float* dbeta_partial, int64_t rows, int64_t d, int dtype,
                  int entry_rc, RowDrop drop, rpo_stream_t stream) {
    const int nv = row_vectors(d, false);
    const int rc = first_error({row_shape(rows, d, dtype, false, nv), row_operand(s, lds, d, 8), vec_operand(gamma),
                                row_operand(dy, lddy, d, 8), row_operand(ds, ldds, d, 8), db ? row_operand(db, lddb, d, 8) : RPO_OK,
                                (!dgamma_partial || !dbeta_partial) ? RPO_ERR_INVALID_ARG : RPO_OK, entry_rc});
    if (rc != RPO_OK || rows == 0) return rc;
    const size_t red_bytes = 2 * (size_t)d * sizeof(float);     // <= 32 KiB (d <= 4096)
    RPO_ROW_DISPATCH(false, dtype, nv, layernorm_bwd_kernel, DROP, dim3((unsigned)rpo_layernorm_bwd_blocks(rows)),
                     dim3(64 * kLnBwdWaves), red_bytes, (hipStream_t)stream, (const T*)s, lds, (const T*)gamma, (const T*)dy, lddy, eps,
                     (T*)ds, ldds, dgamma_partial, dbeta_partial, rows, (int)d, (T*)db, lddb, drop);
    return rpo_launch_status();
}
}  // namespace

extern "C" int rpo_layernorm_bwd(const void* s, int64_t lds, const void* gamma, const void* dy, int64_t lddy, float eps, void* ds,
                                 int64_t ldds, float* dgamma_partial, float* dbeta_partial, int64_t rows, int64_t d, int dtype,
                                 rpo_stream_t stream) {
    return layernorm_bwd<false>(s, lds, gamma, dy, lddy, eps, ds, ldds, nullptr, 0, dgamma_partial, dbeta_partial, rows, d, dtype,
                                rows == 0 ? RPO_ERR_INVALID_ARG : RPO_OK, RowDrop{}, stream);
}

extern "C" int rpo_gelu_out_fwd(const void* u, int64_t ldu, void* h, int64_t ldh, int64_t rows, int64_t cols, int dtype,
                                rpo_stream_t stream) {
    const int rc = first_error({row_shape(rows, cols, dtype, false, 1), row_operand(u, ldu, cols, 8), row_operand(h, ldh, cols, 8)});
    if (rc != RPO_OK || rows == 0) return rc;
    RPO_TYPE_DISPATCH(false, dtype, gelu_out_kernel, gelu_grid(rows, cols, 8), dim3(256), 0, (hipStream_t)stream, (const T*)u, ldu,
                      (T*)h, ldh, rows, cols);
    return rpo_launch_status();
}

extern "C" int rpo_gelu_bwd(const void* u, int64_t ldu, const void* dh, int64_t lddh, void* du, int64_t lddu, int64_t rows,
                            int64_t cols, int dtype, rpo_stream_t stream) {
    const int rc = first_error({row_shape(rows, cols, dtype, false, 1), row_operand(u, ldu, cols, 8), row_operand(dh, lddh, cols, 8),
                                row_operand(du, lddu, cols, 8)});
    if (rc != RPO_OK || rows == 0) return rc;
    RPO_TYPE_DISPATCH(false, dtype, gelu_bwd_kernel, gelu_grid(rows, cols, 8), dim3(256), 0, (hipStream_t)stream, (const T*)u, ldu,
                      (const T*)dh, lddh, (T*)du, lddu, rows, cols);
    return rpo_launch_status();
}

// ---- hidden-state dropout inside the row kernels: the entries of the DROP = true instances ----------------
// p_drop that quantises to thr = 0 still takes the DROP = true instance, with inv_keep = 1: every element is kept and unscaled.
extern "C" float rpo_hidden_dropout_scale(float p_drop) {
    unsigned thr;
    float inv_keep;
    return hidden_dropout_args(p_drop, &thr, &inv_keep) ? inv_keep : 0.0f;
}

extern "C" int rpo_add_layernorm_drop_fwd(const void* a, int64_t lda, const void* b, int64_t ldb, const void* gamma,
                                          const void* beta, float eps, void* y, int64_t ldy, void* s, int64_t lds, int64_t rows,
                                          int64_t d, int dtype, float p_drop, uint64_t seed, int64_t site, rpo_stream_t stream) {
    RowDrop drop;
    const int drop_rc = drop_args(rows, p_drop, seed, site, &drop);
    return add_layernorm<false, true>(a, lda, b, ldb, gamma, beta, eps, y, ldy, s, lds, true, rows, d, dtype, drop_rc, drop, stream);
}

extern "C" int rpo_bert_embed_ln_drop_fwd(const int* ids, const int* token_types, const int* pos, int64_t tokens,
                                          const void* word, int64_t vocab, const void* type_emb, int64_t n_types,
                                          const void* pos_emb, int64_t n_pos, const void* gamma, const void* beta, float eps,
                                          void* y, int64_t ldy, void* s, int64_t lds, int64_t d, int dtype, float p_drop,
                                          uint64_t seed, int64_t site, rpo_stream_t stream) {
    RowDrop drop;
    const int drop_rc = drop_args(tokens, p_drop, seed, site, &drop);
    return bert_embed_ln<false, true>(ids, token_types, pos, tokens, word, vocab, type_emb, n_types, pos_emb, n_pos, gamma, beta, eps,
                                      y, ldy, s, lds, true, d, dtype, drop_rc, drop, stream);
}

extern "C" int rpo_layernorm_drop_bwd(const void* s, int64_t lds, const void* gamma, const void* dy, int64_t lddy, float eps,
                                      void* ds, int64_t ldds, void* db, int64_t lddb, float* dgamma_partial, float* dbeta_partial,
                                      int64_t rows, int64_t d, int dtype, float p_drop, uint64_t seed, int64_t site_in,
                                      int64_t site_out, rpo_stream_t stream) {
    RowDrop drop;       // site = site_out (0 where there is none: unused without db), site_in < 0: dy is not dropped
    const int drop_rc = first_error({drop_args(rows, p_drop, seed, site_out < 0 ? 0 : site_out, &drop),
                                     (site_in > kHiddenMaxSite || (db && site_out < 0)) ? RPO_ERR_INVALID_ARG : RPO_OK});
    drop.site_in = site_in < 0 ? -1 : (int)site_in;
    return layernorm_bwd<true>(s, lds, gamma, dy, lddy, eps, ds, ldds, db, lddb, dgamma_partial, dbeta_partial, rows, d, dtype,
                               drop_rc, drop, stream);      // rows == 0: nothing is written, the caller's partials stay as they are
}

extern "C" int rpo_hidden_dropout_mask(int64_t row0, int64_t rows, int64_t d, float p_drop, uint64_t seed, int64_t site,
                                       unsigned char* mask, rpo_stream_t stream) {
    unsigned thr;
    float inv_keep;
    if (!mask || row0 < 0 || rows < 0 || d < 0 || row0 + rows > 0x7fffffff || d > 0x7fffffff || site < 0 ||
        site > kHiddenMaxSite || !hidden_dropout_args(p_drop, &thr, &inv_keep))
        return RPO_ERR_INVALID_ARG;
    const int64_t n = rows * d;
    if (n == 0) return RPO_OK;
    const int64_t nb = rpo_cdiv(n, 256);
    RPO_LAUNCH(hidden_dropout_mask_kernel, dim3((unsigned)(nb < 65536 ? nb : 65536)), dim3(256), 0, (hipStream_t)stream,
               (int)row0, (int)rows, (int)d, (int)site, thr, seed, mask);
    return rpo_launch_status();
}
