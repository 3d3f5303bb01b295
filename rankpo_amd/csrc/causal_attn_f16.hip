// Causal, grouped-query, variable-length attention forward on fp16 storage (header section 9e: rpo_causal_attn_fwd_f16) for the
// packed Llama pass of `LlamaEncoder.pooled_last_token_multi` under no-grad (encoder.LLAMA_FP16_NATIVE / LlamaEncoder.native_fp16,
// ModelForInference(native_fp16=True)).  The contract and the masking rule of rpo_causal_attn_fwd_f32 (causal_attn_f32.hip), the
// arithmetic of bidir_attn_fwd_kernel<f16_t> (bert_ops.hip) on v_mfma_f32_16x16x32_f16: fp16 operands, f32 accumulation.
//
// Block shape: the one of causal_attn_f32.hip, not the one-wave-per-entry layout of bidir_attn_fwd_kernel.  One block per
// (work-list entry = 32 queries of one sequence, kv head); G = num_heads / num_kv_heads waves, wave w owns query head kvh * G + w.
// Per 32-key step the block stages the K rows and the V rows of the kv head ONCE in LDS and every wave reads them from there: with
// grouped queries (Llama-3.2-1B: G = 4, Llama-3-8B: G = 4) K / V global traffic is 1 / G of a wave-per-head layout, and the
// transposition of V (below) is paid once per kv head instead of once per query head.  The rows of step i + 1 are loaded from
// global memory into registers while step i computes, and stored to LDS between the two barriers of the next step.
//   S^T = K Q^T per 16-key half (A = 16 key rows from LDS, B = Q^T from registers; k slot 8 g + j of MFMA ks = head dim
//   32 ks + 8 g + j, one 16-byte read per operand), so a lane owns ONE query (column l & 15) of each of the two 16-query tiles in
//   the accumulator layout: the softmax statistics stay per lane and reduce over the 4 lane groups with two shuffles.
//   O^T = V^T P^T: P is rounded to fp16 ONCE and goes into the MFMA as the B operand as it lies in the accumulators: lane group g
//   holds keys 4 g .. 4 g + 3 of each 16-key half, so k slot 8 g + j is key 4 g + j (j < 4) / 16 + 4 g + j - 4 (j >= 4) of the
//   step.  V is therefore staged TRANSPOSED, vt[head dim][slot] with slot(key) = 8 ((key & 15) >> 2) + 4 (key >> 4) + (key & 3):
//   the A operand of a 16-row output block (row = head dim 16 b + r) is ONE 16-byte LDS read per lane.  The staging writes 2-byte
//   elements (8 per 16-byte chunk loaded), once per block and step.
// Arithmetic.  Raw scores stay f32; the scale is applied in f32 to the distance from the running maximum m of the RAW scores
// (sign-adjusted by negating Q, exact in fp16, when scale < 0): p = exp2(((s - m) |scale|) log2 e) with log2 e carried as hi + lo,
// as in the f32 kernel.  Q is never pre-scaled.  The row sum adds the ROUNDED p that multiplies V (the bf16 kernels' convention);
// O is divided in f32 and rounded to fp16 once (overflow -> inf, as torch's .half()).
// The work-list decode with its guard, the causal rule (bottom-right aligned: query i sees key j iff j <= i + (lk - lq); where a
// block's key loop ends) and the running-maximum step live in causal_attn_common.hpp, with the entry's checks and dispatch.  Inside
// a step masked keys get p = 0 and do not enter the running maximum (no visible key in a step: the maximum stays, alpha = 1).  Key 0 is visible to every query (lq <= lk, the
// caller's precondition), so the maximum is finite from the first step on; with lq > lk the rows that see no key come out as zeros
// with lse = -inf.  Rows are clamped to the sequence on every load: no access leaves it.
// Budget (the .vgpr_count of `make isa-llama-f16`, no scratch in any instantiation):
//   registers per lane, head_dim 64: Q 2 x 2 x 4, O 2 x 4 x 4, scores 2 x 2 x 4, P 2 x 4, K operands 2 x 4, staging 2 x CH x 4
//   (CH = 4 / G chunks, at least 1); head_dim 128: twice the Q, O, K-operand and staging registers.
//   Allocated, G = 1 / 2 / 4 / 8: 184 / 156 / 140 / 112 at head_dim 64 (2 / 3 / 3 / 4 waves per SIMD) and 325 / 276 / 244 / 159 at
//   head_dim 128 (1 / 1 / 2 / 3): what hipcc takes unasked, no waves-per-SIMD attribute.
//   LDS: 32 x (HD + 8) x 2 (K rows) + HD x 40 x 2 (V^T) = 9 728 bytes (head_dim 64) / 18 944 (head_dim 128) per block.
// Plain HIP with MFMA builtins; no assembly statements, no counted waits, no atomics: deterministic.
#include "causal_attn_common.hpp"

using namespace causal_attn;

namespace {

constexpr int kVtLd = kKeys + 8;    // row stride of the transposed V tile (elements): rows stay 16-byte aligned, 20 words apart

__device__ __forceinline__ void mma_f16(uint4_t a, uint4_t b, float4_t& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, a), __builtin_bit_cast(half8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ unsigned short f16_bits(float f) { return __builtin_bit_cast(unsigned short, (f16_t)f); }

template <int HD, int G>
__global__ __launch_bounds__(64 * G) void causal_attn_fwd_f16_kernel(
    const f16_t* __restrict__ q, const f16_t* __restrict__ k, const f16_t* __restrict__ v, int64_t q_stride, int64_t k_stride,
    int64_t v_stride, const int* __restrict__ cu_q, const int* __restrict__ cu_k, const int* __restrict__ tiles, int num_seqs,
    float scale_abs, unsigned sgn_mask, f16_t* __restrict__ out, int64_t out_stride, float* __restrict__ lse) {
    constexpr int QS = kQBlock / 16;    // query tiles per wave
    constexpr int KS = HD / 32;         // MFMAs of a 16x16 score block
    constexpr int OB = HD / 16;         // 16-row blocks of O^T
    constexpr int KLD = HD + 8;         // LDS row stride of the K tile (elements)
    constexpr int NT = 64 * G;          // threads of the block
    constexpr int NCH = kKeys * HD / 8; // 16-byte chunks of a K (or V) step
    constexpr int CH = (NCH + NT - 1) / NT;   // chunks per thread (head_dim 64 with 8 waves: half the threads stage one chunk)
    static_assert(CH * NT == NCH || (CH == 1 && NCH < NT), "a step splits evenly over the block, or over its first threads");
    __shared__ __attribute__((aligned(16))) unsigned short ks[kKeys * KLD];
    __shared__ __attribute__((aligned(16))) unsigned short vt[HD * kVtLd];

    Entry ent;
    if (!entry_listed(tiles, num_seqs, ent) || !query_entry_has_work(cu_q, cu_k, ent)) return;   // block-uniform
    const int kvh = blockIdx.y, q0 = ent.row0, tq0 = ent.tq0, lq = ent.lq, tk0 = ent.tk0, lk = ent.lk;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int h = kvh * G + w;
    const int kend = key_loop_end(ent, q0, kQBlock);       // one past the last key any query of the entry sees
    const int64_t qcol = (int64_t)h * HD, kvcol = (int64_t)kvh * HD;

    uint4_t qf[QS][KS];
    int lim[QS];                                         // last visible key of this lane's query
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        const int qi = min(q0 + s * 16 + r, lq - 1);     // rows past the end: loaded (in bounds), never stored
        lim[s] = last_visible_key(ent, qi);
        const f16_t* qp = q + (int64_t)(tq0 + qi) * q_stride + qcol + 8 * g;
#pragma unroll
        for (int c = 0; c < KS; ++c) {
            qf[s][c] = *reinterpret_cast<const uint4_t*>(qp + 32 * c);
#pragma unroll
            for (int e = 0; e < 4; ++e) qf[s][c][e] ^= sgn_mask;     // scale < 0: -Q, exact
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
    uint4_t kr[CH], vr[CH];
    auto load_step = [&](int kt) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int idx = tid + NT * c;
            if (CH * NT == NCH || idx < NCH) {
                const int key = idx / (HD / 8), c8 = idx - key * (HD / 8);
                const int64_t row = tk0 + min(kt + key, lk - 1);
                kr[c] = *reinterpret_cast<const uint4_t*>(k + row * k_stride + kvcol + 8 * c8);
                vr[c] = *reinterpret_cast<const uint4_t*>(v + row * v_stride + kvcol + 8 * c8);
            }
        }
    };
    load_step(0);

    for (int kt = 0; kt < kend; kt += kKeys) {
        __syncthreads();                                   // the previous step's LDS reads are done
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int idx = tid + NT * c;
            if (CH * NT == NCH || idx < NCH) {
                const int key = idx / (HD / 8), c8 = idx - key * (HD / 8);
                *reinterpret_cast<uint4_t*>(&ks[key * KLD + 8 * c8]) = kr[c];
                const int slot = 8 * ((key & 15) >> 2) + 4 * (key >> 4) + (key & 3);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    vt[(8 * c8 + 2 * e) * kVtLd + slot] = (unsigned short)(vr[c][e] & 0xffffu);
                    vt[(8 * c8 + 2 * e + 1) * kVtLd + slot] = (unsigned short)(vr[c][e] >> 16);
                }
            }
        }
        __syncthreads();                                   // K and V of this step visible
        if (kt + kKeys < kend) load_step(kt + kKeys);      // in flight while this step computes

        float4_t sc[2][QS];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            uint4_t kf[KS];
#pragma unroll
            for (int c = 0; c < KS; ++c) kf[c] = *reinterpret_cast<const uint4_t*>(&ks[(16 * b + r) * KLD + 32 * c + 8 * g]);
#pragma unroll
            for (int s = 0; s < QS; ++s) {
                sc[b][s] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < KS; ++c) mma_f16(kf[c], qf[s][c], sc[b][s]);
            }
        }
        // online softmax; sc[b][s][i] = raw score of key kt + 16 b + 4 g + i, query q0 + 16 s + r
        uint4_t pf[QS];
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            const int vis = step_visibility(lim[s], kt, g);
            const float alpha = running_max_step(sc[0][s], sc[1][s], vis, scale_abs, mrun[s]);
            const float mn = mrun[s];
            float ps = 0.f;
            unsigned wd[4];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                unsigned short pb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float p = key_visible(b, i, vis) ? exp_hilo((sc[b][s][i] - mn) * scale_abs) : 0.f;
                    const f16_t ph = (f16_t)p;             // the ONE rounding of P: the PV operand, and what the row sum adds
                    pb[i] = __builtin_bit_cast(unsigned short, ph);
                    ps += (float)ph;
                }
                wd[2 * b] = (unsigned)pb[0] | ((unsigned)pb[1] << 16);
                wd[2 * b + 1] = (unsigned)pb[2] | ((unsigned)pb[3] << 16);
            }
            pf[s] = uint4_t{wd[0], wd[1], wd[2], wd[3]};
            l[s] = fmaf(l[s], alpha, ps);                  // per-lane partial sum: alpha is the same on the 4 lanes of a query
#pragma unroll
            for (int b = 0; b < OB; ++b) o[s][b] *= alpha;
        }
        // A = V^T (row = head dim 16 b + r, k slot 8 g + j as P has it), B = P^T
#pragma unroll
        for (int b = 0; b < OB; ++b) {
            const uint4_t va = *reinterpret_cast<const uint4_t*>(&vt[(16 * b + r) * kVtLd + 8 * g]);
#pragma unroll
            for (int s = 0; s < QS; ++s) mma_f16(va, pf[s], o[s][b]);
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
        f16_t* op = out + (int64_t)(tq0 + qi) * out_stride + qcol + 4 * g;
#pragma unroll
        for (int b = 0; b < OB; ++b) {
            const uint2_t pk{(unsigned)f16_bits(o[s][b][0] * inv) | ((unsigned)f16_bits(o[s][b][1] * inv) << 16),
                             (unsigned)f16_bits(o[s][b][2] * inv) | ((unsigned)f16_bits(o[s][b][3] * inv) << 16)};
            *reinterpret_cast<uint2_t*>(op + 16 * b) = pk;
        }
        if (lse && g == 0) lse[(int64_t)h * total_q + tq0 + qi] = L > 0.f ? fmaf(mrun[s], scale_abs, logf(L)) : -INFINITY;
    }
}

template <int HD, int G>
void launch(const HostArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)a.ntiles, (unsigned)a.num_kv_heads), block(64 * G);
    RPO_LAUNCH((causal_attn_fwd_f16_kernel<HD, G>), grid, block, 0, st, (const f16_t*)a.q, (const f16_t*)a.k, (const f16_t*)a.v,
               a.q_stride, a.k_stride, a.v_stride, a.cu_q, a.cu_k, a.tiles, (int)a.num_seqs, fabsf(a.scale),
               a.scale < 0.f ? 0x80008000u : 0u, (f16_t*)a.out, a.out_stride, a.lse);
}

}  // namespace

extern "C" int rpo_causal_attn_fwd_f16(const void* q, const void* k, const void* v, int64_t q_stride, int64_t k_stride,
                                       int64_t v_stride, const int* cu_seqlens_q, const int* cu_seqlens_k, const int* tiles,
                                       int64_t ntiles, int64_t tile_cols, int64_t q_block, int64_t num_seqs, int64_t num_heads,
                                       int64_t num_kv_heads, int64_t head_dim, float scale, void* out, int64_t out_stride,
                                       float* lse, rpo_stream_t stream) {
    HostArgs a{};
    a.q = q, a.k = k, a.v = v, a.q_stride = q_stride, a.k_stride = k_stride, a.v_stride = v_stride;
    a.cu_q = cu_seqlens_q, a.cu_k = cu_seqlens_k, a.tiles = tiles, a.ntiles = ntiles, a.tile_cols = tile_cols, a.q_block = q_block;
    a.num_seqs = num_seqs, a.num_heads = num_heads, a.num_kv_heads = num_kv_heads, a.head_dim = head_dim, a.scale = scale;
    a.out = out, a.out_stride = out_stride, a.lse = lse;
    // 16-byte vector loads of q / k / v rows, 8-byte stores of out: 8-element (16-byte) token strides
    if (const int rc = check_forward(a, 8)) return rc;
    if (ntiles == 0) return RPO_OK;
    RPO_CAUSAL_ATTN_DISPATCH(launch, a, (hipStream_t)stream)
    return rpo_launch_status();
}
