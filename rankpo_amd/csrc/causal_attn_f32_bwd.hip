// Backward of the causal, grouped-query, variable-length f32 attention of causal_attn_f32.hip (header section 9d:
// rpo_causal_attn_bwd_f32) for the packed f32 Llama TRAINING pass (encoder.LLAMA_F32_ATTENTION_TRAIN /
// LlamaEncoder.f32_attention_train, ModelForTraining(f32_attention=True)).  Two kernels on v_mfma_f32_16x16x4_f32, launched in this
// order on one stream: f32 operands, exact f32 products, f32 accumulation, P and dS never rounded to 16 bits, no atomics.
//
// Maths, per query head h (kv head h / G), query i, key j of one sequence, j <= i + (lk - lq) visible:
//   s = q_i . k_j, p' = exp(s scale - lse_i), L'_i = sum_j p', p = p' / L'_i, dP = dO_i . v_j, delta_i = dO_i . O_i,
//   dS = p (dP - delta_i), dQ_i = scale sum_j dS k_j, dK_j = scale sum_h sum_i dS q_i, dV_j = sum_h sum_i p dO_i.
// The statistic.  lse is ONE f32: at |lse| ~ 60 (saturated softmax) its rounding (~2e-6) would enter every p relatively.  The
// dQ kernel walks every visible key of a query anyway, so it sums p' (L', 1 up to that rounding) beside dQ, scales its dQ row
// by 1 / L' and hands 1 / L' to the dK/dV kernel: p = p' / L' is normalised by its own sum, as the f32 softmax of stock torch
// is, and any per-query error of lse cancels.  The forward entry and its lse stay as they are.
//
// dQ kernel: the forward's block shape.  One block per (work-list entry = 32 queries of one sequence, kv head), wave w owns query
//   head kvh * G + w; K and V steps of 32 keys staged ONCE in LDS for the group's waves, the next step's rows in flight in
//   registers.  The wave keeps Q^T and dO^T of its queries as B operands; S^T = K Q^T and dP^T = V dO^T per 16-key half (A = 16
//   rows of the LDS tile by ds_read_b64, row stride HD + 4 words: 64 different banks per half), two alternating chains each, so
//   a lane owns ONE query (column l & 15) per 16-query tile and lse / delta / L' stay per lane.  dS^T is formed in place and
//   dQ^T = K^T dS^T takes it as B as it lies in the accumulator (k slot g = key 4 g + t), A = K[key 4 g + t][16 b + r] by
//   ds_read_b32: the forward's O^T = V^T P^T with K for V.  delta = dO . O is formed here (DK products per lane, two shuffles).
//   The key loop ends with the step that holds the last visible key of the entry's last query.  It writes the workspace
//   ws[h][t] = (delta, 1 / L') for the second kernel.  head_dim 128 with 8 waves (2 per SIMD: 256 registers) or 1 wave (all of
//   the staging registers) takes its 32 queries as two passes of 16 over the keys.
// dK/dV kernel: one block of 2 waves per (key work-list entry = 32 keys of one sequence, kv head); wave w OWNS keys 16 w .. 16 w +
//   15 of the entry (K and V rows as B operands in registers, dK^T and dV^T accumulators) outright.  It walks the query steps of
//   32 from the first query that sees the entry's first key to the sequence's end and, inside a step, the G query heads of the
//   group in ascending order, each (step, head) summed from zero and added to the running total: ONE order per output
//   element, which the indices alone fix -- no combination across waves or
//   blocks, so the result depends neither on scheduling nor on what else is packed in the batch.  Q and dO rows of a (step,
//   head) are staged in LDS for both waves, the next pair in flight in registers.  S = Q K^T and dP = dO V^T (A = LDS rows, a
//   lane owns ONE key); dV^T = dO^T P and dK^T = Q^T dS take P and dS as B as they lie in the accumulator (k slot g = query
//   4 g + t), A = dO / Q[query 4 g + t][16 b + r] by ds_read_b32.  S is recomputed in both kernels: executed work is 7 products
//   per pair (3 + 4), useful work 5.
// Every dq row of a listed entry and every dk / dv row of a listed key entry is written; keys no query sees get exact zeros; a
// query whose lse is -inf (no visible key) contributes exact zeros.  Rows past a sequence's end are loaded clamped to its last
// row (in bounds) and masked; no access leaves the sequence.
// Budget (hipcc -Rpass-analysis=kernel-resource-usage; no scratch in any instantiation), allocated registers per lane (VGPR +
// AGPR) / waves per SIMD the allocation allows / LDS bytes per block, G = 1 / 2 / 4 / 8:
//   dQ    head_dim 64:  337 / 286 / 206 / 212 registers, 1 / 1 / 2 / 2 waves per SIMD, 17 408 bytes
//   dQ    head_dim 128: 462 / 420 / 392 / 201 registers, 1 / 1 / 1 / 2 waves per SIMD, 33 792 bytes
//   dK/dV head_dim 64:  218 / 212 / 212 / 212 registers, 2 waves per SIMD, 17 408 bytes
//   dK/dV head_dim 128: 370 / 350 / 350 / 350 registers, 1 wave per SIMD, 33 792 bytes
// The decode of both work lists with its guard, the causal rule, exp through exp2 and the entry's checks and dispatch:
// causal_attn_common.hpp.
// Plain HIP with MFMA builtins; no asm statements, no counted waits, no atomics: deterministic.
#include "causal_attn_common.hpp"

using namespace causal_attn;

namespace {

typedef __attribute__((ext_vector_type(2))) float float2_t;

// 16-query tiles a wave of the dQ kernel carries at once.  head_dim 128 takes one tile (Q^T, dO^T, dQ^T: 96 registers), not two,
// where two would spill: with 8 waves per block (2 per SIMD: 256 registers each), and with 1 wave per block, which stages a
// whole K and V step by itself (2 x 16 float4 = 128 registers in flight)
constexpr int dq_tiles(int hd, int g) { return hd == 128 && (g == 8 || g == 1) ? 1 : 2; }

template <int HD, int G>
__global__ __launch_bounds__(64 * G) void causal_attn_bwd_dq_f32_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const float* __restrict__ out,
    const float* __restrict__ dout, int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t out_stride, int64_t dout_stride,
    const float* __restrict__ lse, const int* __restrict__ cu_q, const int* __restrict__ cu_k, const int* __restrict__ tiles,
    int num_seqs, float scale_abs, float sgn, float scale, float* __restrict__ dq, int64_t dq_stride, float* __restrict__ ws) {
    constexpr int QS = dq_tiles(HD, G); // query tiles per wave and pass
    constexpr int PASSES = kQBlock / (16 * QS);
    constexpr int DK = HD / 4;          // MFMAs of a 16x16 score block = head dims per lane
    constexpr int OB = HD / 16;         // 16-row blocks of dQ^T
    constexpr int LD = HD + 4;          // LDS row stride (words)
    constexpr int NT = 64 * G;          // threads of the block
    constexpr int CH = kKeys * HD / 4 / NT;   // 16-byte chunks of a K (or V) step per thread
    static_assert(CH >= 1 && CH * NT * 4 == kKeys * HD, "a step must split evenly over the block");
    __shared__ __attribute__((aligned(16))) float ks[kKeys * LD];
    __shared__ __attribute__((aligned(16))) float vs[kKeys * LD];

    Entry ent;
    if (!entry_listed(tiles, num_seqs, ent) || !query_entry_has_work(cu_q, cu_k, ent)) return;   // block-uniform
    const int kvh = blockIdx.y, q0e = ent.row0, tq0 = ent.tq0, lq = ent.lq, tk0 = ent.tk0, lk = ent.lk;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int h = kvh * G + w;
    const int64_t qcol = (int64_t)h * HD, kvcol = (int64_t)kvh * HD;
    const int64_t total_q = cu_q[num_seqs];

    for (int pass = 0; pass < PASSES; ++pass) {
        const int q0 = q0e + 16 * QS * pass;
        if (q0 >= lq) break;                         // block-uniform
        const int kend = key_loop_end(ent, q0, 16 * QS);   // one past the last key any query of the pass sees

        float qf[QS][DK], dof[QS][DK], lsev[QS], delta[QS], lsum[QS];
        int lim[QS];                                 // last visible key of this lane's query
        float4_t acc[QS][OB];
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            const int qi = min(q0 + s * 16 + r, lq - 1);   // rows past the end: loaded (in bounds), never stored
            lim[s] = last_visible_key(ent, qi);
            const float* qp = q + (int64_t)(tq0 + qi) * q_stride + qcol + 2 * g;
            const float* dp = dout + (int64_t)(tq0 + qi) * dout_stride + qcol + 2 * g;
            const float* op = out + (int64_t)(tq0 + qi) * out_stride + qcol + 2 * g;
            float d0 = 0.f, d1 = 0.f;
#pragma unroll
            for (int m = 0; m < DK / 2; ++m) {
                const float2_t t = *reinterpret_cast<const float2_t*>(qp + 8 * m);
                const float2_t u = *reinterpret_cast<const float2_t*>(dp + 8 * m);
                const float2_t o = *reinterpret_cast<const float2_t*>(op + 8 * m);
                qf[s][2 * m] = t[0] * sgn;
                qf[s][2 * m + 1] = t[1] * sgn;
                dof[s][2 * m] = u[0];
                dof[s][2 * m + 1] = u[1];
                d0 = fmaf(u[0], o[0], d0);
                d1 = fmaf(u[1], o[1], d1);
            }
            float d = d0 + d1;
            d += __shfl_xor(d, 16, 64);
            d += __shfl_xor(d, 32, 64);
            delta[s] = d;
            lsev[s] = lse[(int64_t)h * total_q + tq0 + qi];
            lsum[s] = 0.f;
#pragma unroll
            for (int b = 0; b < OB; ++b) acc[s][b] = float4_t{0.f, 0.f, 0.f, 0.f};
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
            __syncthreads();                                   // the previous step's (and pass's) LDS reads are done
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int idx = tid + NT * c, key = idx / (HD / 4), c4 = idx - key * (HD / 4);
                *reinterpret_cast<float4_t*>(&ks[key * LD + 4 * c4]) = kr[c];
                *reinterpret_cast<float4_t*>(&vs[key * LD + 4 * c4]) = vr[c];
            }
            __syncthreads();                                   // K and V of this step visible
            if (kt + kKeys < kend) load_step(kt + kKeys);      // in flight while this step computes

            // sc[b][s][i]: raw score, dp[b][s][i]: dO . v, of key kt + 16 b + 4 g + i and query q0 + 16 s + r
            float4_t sc[2][QS], dp[2][QS];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                float af[DK];
                float4_t odd[QS];
#pragma unroll
                for (int m = 0; m < DK / 2; ++m) {
                    const float2_t t = *reinterpret_cast<const float2_t*>(&ks[(16 * b + r) * LD + 8 * m + 2 * g]);
                    af[2 * m] = t[0];
                    af[2 * m + 1] = t[1];
                }
                // two chains per block (even / odd head dims of a pair), added at the end, as in the forward
#pragma unroll
                for (int s = 0; s < QS; ++s) sc[b][s] = odd[s] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < DK; t += 2)
#pragma unroll
                    for (int s = 0; s < QS; ++s) {
                        sc[b][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[t], qf[s][t], sc[b][s], 0, 0, 0);
                        odd[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[t + 1], qf[s][t + 1], odd[s], 0, 0, 0);
                    }
#pragma unroll
                for (int s = 0; s < QS; ++s) sc[b][s] += odd[s];
#pragma unroll
                for (int m = 0; m < DK / 2; ++m) {
                    const float2_t t = *reinterpret_cast<const float2_t*>(&vs[(16 * b + r) * LD + 8 * m + 2 * g]);
                    af[2 * m] = t[0];
                    af[2 * m + 1] = t[1];
                }
#pragma unroll
                for (int s = 0; s < QS; ++s) dp[b][s] = odd[s] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < DK; t += 2)
#pragma unroll
                    for (int s = 0; s < QS; ++s) {
                        dp[b][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[t], dof[s][t], dp[b][s], 0, 0, 0);
                        odd[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[t + 1], dof[s][t + 1], odd[s], 0, 0, 0);
                    }
#pragma unroll
                for (int s = 0; s < QS; ++s) dp[b][s] += odd[s];
            }
            // p' and dS' = p' (dP - delta) in place of the scores; masked keys and rows without a finite lse: exact zeros
#pragma unroll
            for (int s = 0; s < QS; ++s) {
                const int vis = step_visibility(lim[s], kt, g);
                const bool ok = lsev[s] > -INFINITY;
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float p = (ok && key_visible(b, i, vis)) ? exp_hilo(fmaf(sc[b][s][i], scale_abs, -lsev[s])) : 0.f;
                        lsum[s] += p;
                        sc[b][s][i] = p * (dp[b][s][i] - delta[s]);
                    }
            }
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int ob = 0; ob < OB; ++ob) {
                        const float ka = ks[(16 * b + 4 * g + t) * LD + 16 * ob + r];
#pragma unroll
                        for (int s = 0; s < QS; ++s)
                            acc[s][ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka, sc[b][s][t], acc[s][ob], 0, 0, 0);
                    }
        }

#pragma unroll
        for (int s = 0; s < QS; ++s) {
            float L = lsum[s];
            L += __shfl_xor(L, 16, 64);
            L += __shfl_xor(L, 32, 64);
            const int qi = q0 + s * 16 + r;
            if (qi >= lq) continue;
            const float inv = L > 0.f ? 1.0f / L : 0.f;
            const float f = inv * scale;
            float* op = dq + (int64_t)(tq0 + qi) * dq_stride + qcol + 4 * g;
#pragma unroll
            for (int b = 0; b < OB; ++b) *reinterpret_cast<float4_t*>(op + 16 * b) = acc[s][b] * f;
            if (g == 0) *reinterpret_cast<float2_t*>(ws + 2 * ((int64_t)h * total_q + tq0 + qi)) = float2_t{delta[s], inv};
        }
    }
}

template <int HD, int G>
__global__ __launch_bounds__(128) void causal_attn_bwd_dkdv_f32_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const float* __restrict__ dout,
    int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t dout_stride, const float* __restrict__ lse,
    const float* __restrict__ ws, const int* __restrict__ cu_q, const int* __restrict__ cu_k, const int* __restrict__ ktiles,
    int num_seqs, float scale_abs, float sgn, float scale, float* __restrict__ dk, int64_t dk_stride, float* __restrict__ dv,
    int64_t dv_stride) {
    constexpr int QS = kQBlock / 16;    // query tiles per step
    constexpr int DK = HD / 4;          // MFMAs of a 16x16 score block = head dims per lane
    constexpr int OB = HD / 16;         // 16-row blocks of dK^T / dV^T
    constexpr int LD = HD + 4;          // LDS row stride (words)
    constexpr int NT = 128;             // threads of the block: 2 waves of 16 keys
    constexpr int CH = kQBlock * HD / 4 / NT;   // 16-byte chunks of a Q (or dO) step per thread
    static_assert(CH * NT * 4 == kQBlock * HD && kKeys == 32, "a step must split evenly over the block");
    __shared__ __attribute__((aligned(16))) float qsm[kQBlock * LD];
    __shared__ __attribute__((aligned(16))) float dsm[kQBlock * LD];

    Entry ent;
    if (!entry_listed(ktiles, num_seqs, ent) || !key_entry_has_work(cu_q, cu_k, ent)) return;   // block-uniform
    const int kvh = blockIdx.y, k0 = ent.row0, tq0 = ent.tq0, lq = ent.lq, tk0 = ent.tk0, lk = ent.lk;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int kj = k0 + 16 * w + r;                  // this lane's key
    const int64_t kvcol = (int64_t)kvh * HD;
    const int64_t total_q = cu_q[num_seqs];

    float kf[DK], vf[DK];
    {
        const int64_t row = tk0 + min(kj, lk - 1);   // keys past the end: loaded (in bounds), masked, never stored
        const float* kp = k + row * k_stride + kvcol + 2 * g;
        const float* vp = v + row * v_stride + kvcol + 2 * g;
#pragma unroll
        for (int m = 0; m < DK / 2; ++m) {
            const float2_t t = *reinterpret_cast<const float2_t*>(kp + 8 * m);
            const float2_t u = *reinterpret_cast<const float2_t*>(vp + 8 * m);
            kf[2 * m] = t[0] * sgn;
            kf[2 * m + 1] = t[1] * sgn;
            vf[2 * m] = u[0];
            vf[2 * m + 1] = u[1];
        }
    }
    float4_t dka[OB], dva[OB];
#pragma unroll
    for (int b = 0; b < OB; ++b) dka[b] = dva[b] = float4_t{0.f, 0.f, 0.f, 0.f};

    // query steps of 32 from the first query that sees key k0 to the sequence's end; inside a step the G heads in ascending order
    const int qbeg = first_query_seeing(ent, k0);
    const int niter = lq > qbeg ? ((lq - qbeg + kQBlock - 1) / kQBlock) * G : 0;

    // the Q and dO rows of a (step, head) -> registers (rows clamped to the sequence: in bounds; queries past the end are masked)
    float4_t qr[CH], dr[CH];
    auto load_iter = [&](int it) {
        const int qstep = qbeg + kQBlock * (it / G);
        const int64_t col = (int64_t)(kvh * G + it % G) * HD;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int idx = tid + NT * c, row = idx / (HD / 4), c4 = idx - row * (HD / 4);
            const int64_t t = tq0 + min(qstep + row, lq - 1);
            qr[c] = *reinterpret_cast<const float4_t*>(q + t * q_stride + col + 4 * c4);
            dr[c] = *reinterpret_cast<const float4_t*>(dout + t * dout_stride + col + 4 * c4);
        }
    };
    if (niter > 0) load_iter(0);

    for (int it = 0; it < niter; ++it) {
        __syncthreads();                                   // the previous iteration's LDS reads are done
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int idx = tid + NT * c, row = idx / (HD / 4), c4 = idx - row * (HD / 4);
            *reinterpret_cast<float4_t*>(&qsm[row * LD + 4 * c4]) = qr[c];
            *reinterpret_cast<float4_t*>(&dsm[row * LD + 4 * c4]) = dr[c];
        }
        __syncthreads();                                   // Q and dO of this iteration visible
        if (it + 1 < niter) load_iter(it + 1);             // in flight while this iteration computes

        const int qstep = qbeg + kQBlock * (it / G);
        const int64_t hrow = (int64_t)(kvh * G + it % G) * total_q + tq0;
        // the statistics of this lane's queries 16 s + 4 g + i: lse, (delta, 1 / L')
        float lsev[QS][4];
        float2_t st[QS][4];
#pragma unroll
        for (int s = 0; s < QS; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t t = hrow + min(qstep + 16 * s + 4 * g + i, lq - 1);
                lsev[s][i] = lse[t];
                st[s][i] = *reinterpret_cast<const float2_t*>(ws + 2 * t);
            }

        // sc[s][i]: raw score, dp[s][i]: dO . v, of query qstep + 16 s + 4 g + i and key kj
        float4_t sc[QS], dp[QS];
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            float af[DK];
            float4_t odd;
#pragma unroll
            for (int m = 0; m < DK / 2; ++m) {
                const float2_t t = *reinterpret_cast<const float2_t*>(&qsm[(16 * s + r) * LD + 8 * m + 2 * g]);
                af[2 * m] = t[0];
                af[2 * m + 1] = t[1];
            }
            sc[s] = odd = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < DK; t += 2) {
                sc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[t], kf[t], sc[s], 0, 0, 0);
                odd = __builtin_amdgcn_mfma_f32_16x16x4f32(af[t + 1], kf[t + 1], odd, 0, 0, 0);
            }
            sc[s] += odd;
#pragma unroll
            for (int m = 0; m < DK / 2; ++m) {
                const float2_t t = *reinterpret_cast<const float2_t*>(&dsm[(16 * s + r) * LD + 8 * m + 2 * g]);
                af[2 * m] = t[0];
                af[2 * m + 1] = t[1];
            }
            dp[s] = odd = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < DK; t += 2) {
                dp[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[t], vf[t], dp[s], 0, 0, 0);
                odd = __builtin_amdgcn_mfma_f32_16x16x4f32(af[t + 1], vf[t + 1], odd, 0, 0, 0);
            }
            dp[s] += odd;
        }
        // p in place of the scores, dS in place of dP; masked pairs and rows without a finite lse: exact zeros
#pragma unroll
        for (int s = 0; s < QS; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int qi = qstep + 16 * s + 4 * g + i;
                const bool on = qi < lq && kj <= last_visible_key(ent, qi) && lsev[s][i] > -INFINITY;
                const float p = on ? exp_hilo(fmaf(sc[s][i], scale_abs, -lsev[s][i])) * st[s][i][1] : 0.f;
                sc[s][i] = p;
                dp[s][i] = p * (dp[s][i] - st[s][i][0]);
            }
        // the 32 queries of this (step, head) are summed from zero and the sum is added to the running total: the long chain
        // over steps and heads takes one rounding per 32 queries, not one per query
        float4_t pv[OB], pk[OB];
#pragma unroll
        for (int ob = 0; ob < OB; ++ob) pv[ob] = pk[ob] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < QS; ++s)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int ob = 0; ob < OB; ++ob) {
                    const float da = dsm[(16 * s + 4 * g + t) * LD + 16 * ob + r];
                    const float qa = qsm[(16 * s + 4 * g + t) * LD + 16 * ob + r];
                    pv[ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(da, sc[s][t], pv[ob], 0, 0, 0);
                    pk[ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa, dp[s][t], pk[ob], 0, 0, 0);
                }
#pragma unroll
        for (int ob = 0; ob < OB; ++ob) {
            dva[ob] += pv[ob];
            dka[ob] += pk[ob];
        }
    }

    if (kj < lk) {
        float* kp = dk + (int64_t)(tk0 + kj) * dk_stride + kvcol + 4 * g;
        float* vp = dv + (int64_t)(tk0 + kj) * dv_stride + kvcol + 4 * g;
#pragma unroll
        for (int b = 0; b < OB; ++b) {
            *reinterpret_cast<float4_t*>(kp + 16 * b) = dka[b] * scale;
            *reinterpret_cast<float4_t*>(vp + 16 * b) = dva[b];
        }
    }
}

template <int HD, int G>
void launch(const HostArgs& a, hipStream_t st) {
    const float sa = fabsf(a.scale), sgn = a.scale < 0.f ? -1.0f : 1.0f;
    if (a.ntiles > 0) {
        const dim3 grid((unsigned)a.ntiles, (unsigned)a.num_kv_heads), block(64 * G);
        RPO_LAUNCH((causal_attn_bwd_dq_f32_kernel<HD, G>), grid, block, 0, st, (const float*)a.q, (const float*)a.k, (const float*)a.v, (const float*)a.out, (const float*)a.dout, a.q_stride, a.k_stride,
                   a.v_stride, a.out_stride, a.dout_stride, (const float*)a.lse, a.cu_q, a.cu_k, a.tiles, (int)a.num_seqs, sa, sgn, a.scale,
                   (float*)a.dq, a.dq_stride, a.ws);
        if (hipPeekAtLastError() != hipSuccess) return;
    }
    if (a.nktiles > 0) {
        const dim3 grid((unsigned)a.nktiles, (unsigned)a.num_kv_heads), block(128);
        RPO_LAUNCH((causal_attn_bwd_dkdv_f32_kernel<HD, G>), grid, block, 0, st, (const float*)a.q, (const float*)a.k, (const float*)a.v, (const float*)a.dout, a.q_stride, a.k_stride,
                   a.v_stride, a.dout_stride, (const float*)a.lse, (const float*)a.ws, a.cu_q, a.cu_k, a.k_tiles, (int)a.num_seqs, sa, sgn,
                   a.scale, (float*)a.dk, a.dk_stride, (float*)a.dv, a.dv_stride);
    }
}

}  // namespace

extern "C" int rpo_causal_attn_bwd_f32(const void* q, const void* k, const void* v, const void* out, const void* dout,
                                       int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t out_stride,
                                       int64_t dout_stride, const float* lse, const int* cu_seqlens_q, const int* cu_seqlens_k,
                                       const int* tiles, int64_t ntiles, const int* k_tiles, int64_t nktiles, int64_t tile_cols,
                                       int64_t q_block, int64_t num_seqs, int64_t num_heads, int64_t num_kv_heads, int64_t head_dim,
                                       float scale, void* dq, int64_t dq_stride, void* dk, int64_t dk_stride, void* dv,
                                       int64_t dv_stride, float* ws, rpo_stream_t stream) {
    HostArgs a{};
    a.q = q, a.k = k, a.v = v, a.q_stride = q_stride, a.k_stride = k_stride, a.v_stride = v_stride;
    a.cu_q = cu_seqlens_q, a.cu_k = cu_seqlens_k, a.tiles = tiles, a.ntiles = ntiles, a.tile_cols = tile_cols, a.q_block = q_block;
    a.num_seqs = num_seqs, a.num_heads = num_heads, a.num_kv_heads = num_kv_heads, a.head_dim = head_dim, a.scale = scale;
    a.out = const_cast<void*>(out), a.out_stride = out_stride, a.lse = const_cast<float*>(lse);
    a.dout = dout, a.dout_stride = dout_stride, a.k_tiles = k_tiles, a.nktiles = nktiles;
    a.dq = dq, a.dk = dk, a.dv = dv, a.dq_stride = dq_stride, a.dk_stride = dk_stride, a.dv_stride = dv_stride, a.ws = ws;
    // 16-byte vectors of 4 floats; ws: 8-byte (delta, 1 / L') pairs, 16-byte aligned
    if (const int rc = check_backward(a, 4, 16)) return rc;
    if (ntiles == 0 && nktiles == 0) return RPO_OK;
    RPO_CAUSAL_ATTN_DISPATCH(launch, a, (hipStream_t)stream)
    return rpo_launch_status();
}
