// Causal, grouped-query, variable-length attention forward on f32 storage (header section 9c: rpo_causal_attn_fwd_f32) for the
// packed Llama pass of `LlamaEncoder.pooled_last_token_multi` under no-grad (encoder.LLAMA_F32_ATTENTION /
// LlamaEncoder.f32_attention, ModelForInference(f32_attention=True)).  The numerics of bidir_attn_fwd_f32_kernel (bert_ops.hip) on
// v_mfma_f32_16x16x4_f32: f32 operands, exact f32 products, f32 accumulation, P never rounded to 16 bits.
//
// Block shape.  One block per (work-list entry = 32 queries of one sequence, kv head); G = num_heads / num_kv_heads waves, wave w
// owns query head kvh * G + w.  Per 32-key step the block stages the K rows and the V rows of the kv head ONCE in LDS and every wave
// reads them from there, so K / V global traffic is 1 / G of a wave-per-head layout.  The rows of step i + 1 are loaded from global
// memory into registers while step i computes, and stored to LDS between the two barriers of the next step.
//   S^T = K Q^T per 16-key half (A = 16 key rows, B = Q^T), so a lane owns ONE query (column l & 15) of each of the two 16-query
//   tiles in the accumulator layout: the softmax statistics stay per lane and reduce over the 4 lane groups with two shuffles.
//   MFMA (m, e) of the HD / 4 takes head dim 8 m + 2 g + e in k slot g = l >> 4 of both operands (any one-to-one map of k slots to
//   head dims gives the same dot product): a lane reads its K operands as 8-byte LDS words, and with a row stride of HD + 4 words
//   (4 mod 64) the 32 lanes of a ds_read_b64 half (16 rows x 2 lane groups) hit 64 different banks.  Two alternating chains
//   (e = 0 / 1) per score block, added at the end.
//   O^T = V^T P^T: MFMA t of a 16-key half takes p[t] as B as it lies in the accumulator (k slot g = key 4 g + t) and
//   A = V[key 4 g + t][16 b + r] by ds_read_b32 (lane groups g, g + 1 read rows 4 apart = banks 16 apart: conflict-free).
// The work-list decode with its guard, the causal rule (bottom-right aligned: query i sees key j iff j <= i + (lk - lq); where a
// block's key loop ends) and the running-maximum step live in causal_attn_common.hpp, with the entry's checks and dispatch.  Inside
// a step masked keys get p = 0 and do not enter the running maximum (no visible key in a step: the maximum stays, alpha = 1).  Key 0 is visible to every query (lq <= lk, the
// caller's precondition), so the maximum is finite from the first step on; with lq > lk the rows that see no key come out as zeros
// with lse = -inf, and no access leaves the sequence.
// Budget (hipcc -Rpass-analysis=kernel-resource-usage, no scratch in any instantiation):
//   registers per lane, head_dim 64: Q 2 x 16, O 2 x 4 x 4, scores 2 x 2 x 4 + 8, K operands 16, staging 2 x 8 / G float4;
//   head_dim 128: Q 2 x 32, O 2 x 8 x 4, scores 16 + 8, K operands 32, staging 2 x 16 / G float4 (G = 4: 32 registers).
//   Allocated, G = 1 / 2 / 4 / 8: 262 / 206 / 162 / 146 at head_dim 64 (1 / 2 / 3 / 3 waves per SIMD) and 502 / 389 / 256 / 226 at
//   head_dim 128 (1 / 1 / 2 / 2); see waves_per_simd below.
//   LDS: 2 x 32 x (HD + 4) x 4 bytes = 17 408 (head_dim 64) / 33 792 (head_dim 128) per block.
// Plain HIP with MFMA builtins; no asm statements, no counted waits, no atomics: deterministic.
#include "causal_attn_common.hpp"

using namespace causal_attn;

namespace {

typedef __attribute__((ext_vector_type(2))) float float2_t;

// waves per SIMD the register allocation aims at: with 4 or 8 waves per block the staging registers are few and the kernel fits
// 3 (head_dim 64) / 2 (head_dim 128) waves per SIMD without scratch, which hides one wave's softmax and barriers behind another's
// MFMAs; groups of 1 and 2 keep up to 2 x 16 staging float4 per lane and take what they need (1 wave per SIMD at head_dim 128)
constexpr int waves_per_simd(int hd, int g) { return g >= 4 ? (hd == 64 ? 3 : 2) : 1; }

template <int HD, int G>
__global__ __launch_bounds__(64 * G) __attribute__((amdgpu_waves_per_eu(waves_per_simd(HD, G)))) void causal_attn_fwd_f32_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t q_stride, int64_t k_stride,
    int64_t v_stride, const int* __restrict__ cu_q, const int* __restrict__ cu_k, const int* __restrict__ tiles, int num_seqs,
    float scale_abs, float sgn, float* __restrict__ out, int64_t out_stride, float* __restrict__ lse) {
    constexpr int QS = kQBlock / 16;    // query tiles per wave
    constexpr int DK = HD / 4;          // MFMAs of a 16x16 score block = head dims per lane
    constexpr int OB = HD / 16;         // 16-row blocks of O^T
    constexpr int LD = HD + 4;          // LDS row stride (words)
    constexpr int NT = 64 * G;          // threads of the block
    constexpr int CH = kKeys * HD / 4 / NT;   // 16-byte chunks of a K (or V) step per thread
    static_assert(CH >= 1 && CH * NT * 4 == kKeys * HD, "a step must split evenly over the block");
    __shared__ __attribute__((aligned(16))) float ks[kKeys * LD];
    __shared__ __attribute__((aligned(16))) float vs[kKeys * LD];

    Entry ent;
    if (!entry_listed(tiles, num_seqs, ent) || !query_entry_has_work(cu_q, cu_k, ent)) return;   // block-uniform
    const int kvh = blockIdx.y, q0 = ent.row0, tq0 = ent.tq0, lq = ent.lq, tk0 = ent.tk0, lk = ent.lk;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int h = kvh * G + w;
    const int kend = key_loop_end(ent, q0, kQBlock);   // one past the last key any query of the entry sees
    const int64_t qcol = (int64_t)h * HD, kvcol = (int64_t)kvh * HD;

    float qf[QS][DK];
    int lim[QS];                                     // last visible key of this lane's query
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        const int qi = min(q0 + s * 16 + r, lq - 1); // rows past the end: loaded (in bounds), never stored
        lim[s] = last_visible_key(ent, qi);
        const float* qp = q + (int64_t)(tq0 + qi) * q_stride + qcol + 2 * g;
#pragma unroll
        for (int m = 0; m < DK / 2; ++m) {
            const float2_t t = *reinterpret_cast<const float2_t*>(qp + 8 * m);
            qf[s][2 * m] = t[0] * sgn;
            qf[s][2 * m + 1] = t[1] * sgn;
        }
    }
    float mrun[QS], l[QS];
    float4_t o[QS][OB];
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        mrun[s] = -INFINITY;
        l[s] = 0.f;
#pragma unroll
        for (int b = 0; b < OB; ++b) o[s][b] = float4_t{0.f, 0.f, 0.f, 0.f};
    }

    // the K and V rows of a step -> registers (rows clamped to the sequence: in bounds; keys past the end are masked)
    float4_t kr[CH], vr[CH];
    auto load_step = [&](int kt) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int idx = tid + NT * c, key = idx / (HD / 4), c4 = idx - key * (HD / 4);
            const int64_t row = tk0 + min(kt + key, lk - 1);
            kr[c] = *reinterpret_cast<const float4_t*>(k + row * k_stride + kvcol + 4 * c4);
            vr[c] = *reinterpret_cast<const float4_t*>(v + row * v_stride + kvcol + 4 * c4);
        }
    };
    load_step(0);

    for (int kt = 0; kt < kend; kt += kKeys) {
        __syncthreads();                                   // the previous step's LDS reads are done
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int idx = tid + NT * c, key = idx / (HD / 4), c4 = idx - key * (HD / 4);
            *reinterpret_cast<float4_t*>(&ks[key * LD + 4 * c4]) = kr[c];
            *reinterpret_cast<float4_t*>(&vs[key * LD + 4 * c4]) = vr[c];
        }
        __syncthreads();                                   // K and V of this step visible
        if (kt + kKeys < kend) load_step(kt + kKeys);      // in flight while this step computes

        float4_t sc[2][QS];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            float kf[DK];
#pragma unroll
            for (int m = 0; m < DK / 2; ++m) {
                const float2_t t = *reinterpret_cast<const float2_t*>(&ks[(16 * b + r) * LD + 8 * m + 2 * g]);
                kf[2 * m] = t[0];
                kf[2 * m + 1] = t[1];
            }
            // two chains per score block (even / odd head dims of a pair), added at the end: half the length of each rounding
            // chain, and four independent accumulators in flight
            float4_t odd[QS];
#pragma unroll
            for (int s = 0; s < QS; ++s) sc[b][s] = odd[s] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < DK; t += 2)
#pragma unroll
                for (int s = 0; s < QS; ++s) {
                    sc[b][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[t], qf[s][t], sc[b][s], 0, 0, 0);
                    odd[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[t + 1], qf[s][t + 1], odd[s], 0, 0, 0);
                }
#pragma unroll
            for (int s = 0; s < QS; ++s) sc[b][s] += odd[s];
        }
        // online softmax; sc[b][s][i] = raw score of key kt + 16 b + 4 g + i, query q0 + 16 s + r; afterwards the probability
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            const int vis = step_visibility(lim[s], kt, g);
            const float alpha = running_max_step(sc[0][s], sc[1][s], vis, scale_abs, mrun[s]);
            const float mn = mrun[s];
            float ps = 0.f;
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float p = key_visible(b, i, vis) ? exp_hilo((sc[b][s][i] - mn) * scale_abs) : 0.f;
                    sc[b][s][i] = p;
                    ps += p;
                }
            l[s] = fmaf(l[s], alpha, ps);                  // per-lane partial sum: alpha is the same on the 4 lanes of a query
#pragma unroll
            for (int b = 0; b < OB; ++b) o[s][b] *= alpha;
        }
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int ob = 0; ob < OB; ++ob) {
                    const float va = vs[(16 * b + 4 * g + t) * LD + 16 * ob + r];
#pragma unroll
                    for (int s = 0; s < QS; ++s) o[s][ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(va, sc[b][s][t], o[s][ob], 0, 0, 0);
                }
    }

    const int64_t total_q = lse ? cu_q[num_seqs] : 0;
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        float L = l[s];
        L += __shfl_xor(L, 16, 64);
        L += __shfl_xor(L, 32, 64);
        const int qi = q0 + s * 16 + r;
        if (qi >= lq) continue;
        const float inv = L > 0.f ? 1.0f / L : 0.f;
        float* op = out + (int64_t)(tq0 + qi) * out_stride + qcol + 4 * g;
#pragma unroll
        for (int b = 0; b < OB; ++b) *reinterpret_cast<float4_t*>(op + 16 * b) = o[s][b] * inv;
        if (lse && g == 0) lse[(int64_t)h * total_q + tq0 + qi] = L > 0.f ? fmaf(mrun[s], scale_abs, logf(L)) : -INFINITY;
    }
}

template <int HD, int G>
void launch(const HostArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)a.ntiles, (unsigned)a.num_kv_heads), block(64 * G);
    RPO_LAUNCH((causal_attn_fwd_f32_kernel<HD, G>), grid, block, 0, st, (const float*)a.q, (const float*)a.k, (const float*)a.v,
               a.q_stride, a.k_stride, a.v_stride, a.cu_q, a.cu_k, a.tiles, (int)a.num_seqs, fabsf(a.scale),
               a.scale < 0.f ? -1.0f : 1.0f, (float*)a.out, a.out_stride, a.lse);
}

}  // namespace

extern "C" int rpo_causal_attn_fwd_f32(const void* q, const void* k, const void* v, int64_t q_stride, int64_t k_stride,
                                       int64_t v_stride, const int* cu_seqlens_q, const int* cu_seqlens_k, const int* tiles,
                                       int64_t ntiles, int64_t tile_cols, int64_t q_block, int64_t num_seqs, int64_t num_heads,
                                       int64_t num_kv_heads, int64_t head_dim, float scale, void* out, int64_t out_stride,
                                       float* lse, rpo_stream_t stream) {
    HostArgs a{};
    a.q = q, a.k = k, a.v = v, a.q_stride = q_stride, a.k_stride = k_stride, a.v_stride = v_stride;
    a.cu_q = cu_seqlens_q, a.cu_k = cu_seqlens_k, a.tiles = tiles, a.ntiles = ntiles, a.tile_cols = tile_cols, a.q_block = q_block;
    a.num_seqs = num_seqs, a.num_heads = num_heads, a.num_kv_heads = num_kv_heads, a.head_dim = head_dim, a.scale = scale;
    a.out = out, a.out_stride = out_stride, a.lse = lse;
    if (const int rc = check_forward(a, 4)) return rc;       // 16-byte vectors of 4 floats
    if (ntiles == 0) return RPO_OK;
    RPO_CAUSAL_ATTN_DISPATCH(launch, a, (hipStream_t)stream)
    return rpo_launch_status();
}
