// Packed forward of the BERT / XLM-R block (BGE-small / base / large, bge-m3, e5: the reference's CLS-pooling branch,
// modeling.py:231-232) for rankpo_amd/encoder.py `BertEncoder.pooled_cls`.  Four entry points, bf16 or fp16 storage, f32
// arithmetic inside:
//   rpo_bidir_attn_fwd     non-causal variable-length attention over packed tokens (HF BertSelfAttention's softmax(QK^T s) V,
//                          which the padded path runs as F.scaled_dot_product_attention with a boolean key mask)
//   rpo_add_layernorm_fwd  LayerNorm(a + b) (HF BertSelfOutput / BertOutput: `LayerNorm(dropout(dense(h)) + input)`)
//   rpo_gelu_fwd           exact erf GELU in place (HF BertIntermediate with hidden_act "gelu")
//   rpo_bert_embed_ln_fwd  word + token type + position embedding gather, then LayerNorm (HF BertEmbeddings.forward)
// Plain HIP with MFMA builtins; no inline asm, no counted waits.
#include "common.hpp"

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

template <typename T, int HD>
__global__ __launch_bounds__(64) void bidir_attn_fwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, int64_t q_stride, int64_t k_stride,
    int64_t v_stride, const int* __restrict__ cu_q, const int* __restrict__ cu_k, const int* __restrict__ tiles,
    float scale_log2, T* __restrict__ out, int64_t out_stride, float* __restrict__ lse, int64_t total_q) {
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
        const float inv = L > 0.f ? 1.0f / L : 0.f;
        T* op = out + (int64_t)(tq0 + qi) * out_stride + hcol + 4 * g;
#pragma unroll
        for (int b = 0; b < OB; ++b) {
            const uint2_t pk{pack2<T>(o[s][b][0] * inv, o[s][b][1] * inv), pack2<T>(o[s][b][2] * inv, o[s][b][3] * inv)};
            *reinterpret_cast<uint2_t*>(op + 16 * b) = pk;
        }
        if (lse && g == 0) lse[(int64_t)h * total_q + tq0 + qi] = L > 0.f ? (m[s] + log2f(L)) * kLn2 : -INFINITY;
    }
}

// ---- (2)-(4) row kernels: one wave per row, NV 16-byte vectors per lane ------------------------------
constexpr int kRowThreads = 256;

// y = (x - mean) rstd gamma + beta over a row held in registers (columns 8 (lane + 64 j) .. + 7), statistics in f32, rounded once
template <typename T, int NV>
__device__ __forceinline__ void layernorm_store(Vec16<T> (&x)[NV], const T* __restrict__ gamma, const T* __restrict__ beta,
                                                float eps, T* __restrict__ y, int d, int lane) {
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
        if (8 * (lane + 64 * j) < d)
#pragma unroll
            for (int e = 0; e < 8; ++e) sum += x[j].v[e];
    const float mean = wave_sum(sum) / (float)d;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
        if (8 * (lane + 64 * j) < d)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float c = x[j].v[e] - mean;
                sq = fmaf(c, c, sq);
            }
    const float rstd = rsqrtf(wave_sum(sq) / (float)d + eps);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c0 = 8 * (lane + 64 * j);
        if (c0 < d) {
            Vec16<T> gw, bw;
            gw.load(gamma + c0);
            bw.load(beta + c0);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[j].v[e] = fmaf((x[j].v[e] - mean) * rstd, gw.v[e], bw.v[e]);
            x[j].store(y + c0);
        }
    }
}

template <typename T, int NV>
__global__ __launch_bounds__(kRowThreads) void add_layernorm_kernel(const T* __restrict__ a, int64_t lda, const T* __restrict__ b,
                                                                     int64_t ldb, const T* __restrict__ gamma,
                                                                     const T* __restrict__ beta, float eps, T* __restrict__ y,
                                                                     int64_t ldy, int64_t rows, int d) {
    const int64_t row = (int64_t)blockIdx.x * (kRowThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    Vec16<T> x[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c0 = 8 * (lane + 64 * j);
        if (c0 < d) {
            x[j].load(a + row * lda + c0);
            if (b) {
                Vec16<T> t;
                t.load(b + row * ldb + c0);
#pragma unroll
                for (int e = 0; e < 8; ++e) x[j].v[e] = Elem<T>::round(x[j].v[e] + t.v[e]);   // the reference's rounded sum
            }
        }
    }
    layernorm_store<T, NV>(x, gamma, beta, eps, y + row * ldy, d, lane);
}

template <typename T, int NV>
__global__ __launch_bounds__(kRowThreads) void bert_embed_ln_kernel(
    const int* __restrict__ ids, const int* __restrict__ tts, const int* __restrict__ pos, int64_t tokens,
    const T* __restrict__ word, int64_t vocab, const T* __restrict__ temb, int64_t ntypes, const T* __restrict__ pemb,
    int64_t npos, const T* __restrict__ gamma, const T* __restrict__ beta, float eps, T* __restrict__ y, int64_t ldy, int d) {
    const int64_t row = (int64_t)blockIdx.x * (kRowThreads / 64) + (threadIdx.x >> 6);
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
        const int c0 = 8 * (lane + 64 * j);
        if (c0 < d) {
            Vec16<T> t, p;
            x[j].load(word + wi * d + c0);
            t.load(temb + ti * d + c0);
            p.load(pemb + pi * d + c0);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[j].v[e] = Elem<T>::round(Elem<T>::round(x[j].v[e] + t.v[e]) + p.v[e]);   // (w + t) + p
        }
    }
    layernorm_store<T, NV>(x, gamma, beta, eps, y + row * ldy, d, lane);
}

template <typename T>
__global__ __launch_bounds__(256) void gelu_kernel(T* __restrict__ x, int64_t rows, int64_t cols, int64_t ld) {
    const int64_t vpr = cols / 8, n = rows * vpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t rr = i / vpr, c = (i - rr * vpr) * 8;
        T* p = x + rr * ld + c;
        Vec16<T> t;
        t.load(p);
#pragma unroll
        for (int e = 0; e < 8; ++e) t.v[e] = 0.5f * t.v[e] * (1.0f + erff(t.v[e] * 0.70710678118654752f));
        t.store(p);
    }
}

int row_vectors(int64_t d) {                // NV of the row kernels: 1, 2, 4 or 8 (d <= 4096); 0 = too wide
    const int64_t nv = rpo_cdiv(d, 512);
    return nv <= 1 ? 1 : nv <= 2 ? 2 : nv <= 4 ? 4 : nv <= 8 ? 8 : 0;
}

}  // namespace

#define RPO_ROW_DISPATCH(KERNEL, T, NV, GRID, ST, ...)                                                          \
    do {                                                                                                        \
        if (NV == 1) RPO_LAUNCH((KERNEL<T, 1>), GRID, dim3(kRowThreads), 0, ST, __VA_ARGS__);                   \
        else if (NV == 2) RPO_LAUNCH((KERNEL<T, 2>), GRID, dim3(kRowThreads), 0, ST, __VA_ARGS__);              \
        else if (NV == 4) RPO_LAUNCH((KERNEL<T, 4>), GRID, dim3(kRowThreads), 0, ST, __VA_ARGS__);              \
        else RPO_LAUNCH((KERNEL<T, 8>), GRID, dim3(kRowThreads), 0, ST, __VA_ARGS__);                           \
    } while (0)

extern "C" int rpo_bidir_attn_fwd(const void* q, const void* k, const void* v, int64_t q_stride, int64_t k_stride,
                                  int64_t v_stride, const int* cu_seqlens_q, const int* cu_seqlens_k, const int* tiles,
                                  int64_t ntiles, int64_t tile_cols, int64_t q_block, int64_t total_q, int64_t num_heads,
                                  int64_t num_kv_heads, int64_t head_dim, int dtype, float scale, void* out,
                                  int64_t out_stride, float* lse, rpo_stream_t stream) {
    if (!q || !k || !v || !cu_seqlens_q || !cu_seqlens_k || !tiles || !out || ntiles < 0 || total_q <= 0 || num_heads <= 0 ||
        num_kv_heads <= 0 || head_dim <= 0 || !rpo_dtype_ok(dtype) || q_stride <= 0 || k_stride <= 0 || v_stride <= 0 ||
        out_stride <= 0)
        return RPO_ERR_INVALID_ARG;
    if (dtype == RPO_DT_F32 || (head_dim != 32 && head_dim != 64) || num_heads != num_kv_heads || tile_cols != 2 ||
        q_block != kAttnQBlock || ntiles > 0x7fffffff || num_heads > 65535)
        return RPO_ERR_UNSUPPORTED;
    if (!rpo_aligned16(q) || !rpo_aligned16(k) || !rpo_aligned16(v) || (reinterpret_cast<uintptr_t>(out) & 7) || q_stride % 8 ||
        k_stride % 8 || v_stride % 8 || out_stride % 4)
        return RPO_ERR_UNSUPPORTED;
    if (ntiles == 0) return RPO_OK;
    const dim3 grid((unsigned)ntiles, (unsigned)num_heads), block(64);
    hipStream_t st = (hipStream_t)stream;
    const float sl = scale * 1.4426950408889634f;
#define RPO_BIDIR(T, HD)                                                                                                         \
    RPO_LAUNCH((bidir_attn_fwd_kernel<T, HD>), grid, block, 0, st, (const T*)q, (const T*)k, (const T*)v, q_stride, k_stride, \
               v_stride, cu_seqlens_q, cu_seqlens_k, tiles, sl, (T*)out, out_stride, lse, total_q)
    if (dtype == RPO_DT_BF16) {
        if (head_dim == 32) RPO_BIDIR(bf16_t, 32);
        else RPO_BIDIR(bf16_t, 64);
    } else {
        if (head_dim == 32) RPO_BIDIR(f16_t, 32);
        else RPO_BIDIR(f16_t, 64);
    }
#undef RPO_BIDIR
    return rpo_launch_status();
}

extern "C" int rpo_add_layernorm_fwd(const void* a, int64_t lda, const void* b, int64_t ldb, const void* gamma, const void* beta,
                                     float eps, void* y, int64_t ldy, int64_t rows, int64_t d, int dtype, rpo_stream_t stream) {
    if (!a || !gamma || !beta || !y || rows < 0 || d <= 0 || !rpo_dtype_ok(dtype) || lda < d || ldy < d || (b && ldb < d))
        return RPO_ERR_INVALID_ARG;
    const int nv = row_vectors(d);
    if (dtype == RPO_DT_F32 || d % 8 || nv == 0) return RPO_ERR_UNSUPPORTED;
    if (!rpo_aligned16(a) || (b && !rpo_aligned16(b)) || !rpo_aligned16(gamma) || !rpo_aligned16(beta) || !rpo_aligned16(y) ||
        lda % 8 || (b && ldb % 8) || ldy % 8)
        return RPO_ERR_UNSUPPORTED;
    if (rows == 0) return RPO_OK;
    const dim3 grid((unsigned)rpo_cdiv(rows, kRowThreads / 64));
    hipStream_t st = (hipStream_t)stream;
    if (dtype == RPO_DT_BF16)
        RPO_ROW_DISPATCH(add_layernorm_kernel, bf16_t, nv, grid, st, (const bf16_t*)a, lda, (const bf16_t*)b, ldb,
                         (const bf16_t*)gamma, (const bf16_t*)beta, eps, (bf16_t*)y, ldy, rows, (int)d);
    else
        RPO_ROW_DISPATCH(add_layernorm_kernel, f16_t, nv, grid, st, (const f16_t*)a, lda, (const f16_t*)b, ldb,
                         (const f16_t*)gamma, (const f16_t*)beta, eps, (f16_t*)y, ldy, rows, (int)d);
    return rpo_launch_status();
}

extern "C" int rpo_gelu_fwd(void* x, int64_t rows, int64_t cols, int64_t ld, int dtype, rpo_stream_t stream) {
    if (!x || rows < 0 || cols <= 0 || ld < cols || !rpo_dtype_ok(dtype)) return RPO_ERR_INVALID_ARG;
    if (dtype == RPO_DT_F32 || cols % 8 || ld % 8 || !rpo_aligned16(x)) return RPO_ERR_UNSUPPORTED;
    if (rows == 0) return RPO_OK;
    const int64_t n = rows * (cols / 8), nb = rpo_cdiv(n, 256);
    const dim3 grid((unsigned)(nb < 8192 ? nb : 8192)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == RPO_DT_BF16) RPO_LAUNCH(gelu_kernel<bf16_t>, grid, block, 0, st, (bf16_t*)x, rows, cols, ld);
    else RPO_LAUNCH(gelu_kernel<f16_t>, grid, block, 0, st, (f16_t*)x, rows, cols, ld);
    return rpo_launch_status();
}

extern "C" int rpo_bert_embed_ln_fwd(const int* ids, const int* token_types, const int* pos, int64_t tokens, const void* word,
                                     int64_t vocab, const void* type_emb, int64_t n_types, const void* pos_emb, int64_t n_pos,
                                     const void* gamma, const void* beta, float eps, void* y, int64_t ldy, int64_t d, int dtype,
                                     rpo_stream_t stream) {
    if (!ids || !pos || !word || !type_emb || !pos_emb || !gamma || !beta || !y || tokens < 0 || vocab <= 0 || n_types <= 0 ||
        n_pos <= 0 || d <= 0 || ldy < d || !rpo_dtype_ok(dtype))
        return RPO_ERR_INVALID_ARG;
    const int nv = row_vectors(d);
    if (dtype == RPO_DT_F32 || d % 8 || nv == 0 || ldy % 8) return RPO_ERR_UNSUPPORTED;
    if (!rpo_aligned16(word) || !rpo_aligned16(type_emb) || !rpo_aligned16(pos_emb) || !rpo_aligned16(gamma) ||
        !rpo_aligned16(beta) || !rpo_aligned16(y))
        return RPO_ERR_UNSUPPORTED;
    if (tokens == 0) return RPO_OK;
    const dim3 grid((unsigned)rpo_cdiv(tokens, kRowThreads / 64));
    hipStream_t st = (hipStream_t)stream;
    if (dtype == RPO_DT_BF16)
        RPO_ROW_DISPATCH(bert_embed_ln_kernel, bf16_t, nv, grid, st, ids, token_types, pos, tokens, (const bf16_t*)word, vocab,
                         (const bf16_t*)type_emb, n_types, (const bf16_t*)pos_emb, n_pos, (const bf16_t*)gamma,
                         (const bf16_t*)beta, eps, (bf16_t*)y, ldy, (int)d);
    else
        RPO_ROW_DISPATCH(bert_embed_ln_kernel, f16_t, nv, grid, st, ids, token_types, pos, tokens, (const f16_t*)word, vocab,
                         (const f16_t*)type_emb, n_types, (const f16_t*)pos_emb, n_pos, (const f16_t*)gamma,
                         (const f16_t*)beta, eps, (f16_t*)y, ldy, (int)d);
    return rpo_launch_status();
}
