// Backward of the causal, grouped-query, variable-length fp16 attention of causal_attn_f16.hip (header section 9f:
// rpo_causal_attn_bwd_f16) for the packed fp16 Llama TRAINING pass (encoder.LLAMA_FP16_NATIVE_TRAIN /
// LlamaEncoder.native_fp16_train, ModelForTraining(native_fp16=True)).  Two kernels on v_mfma_f32_16x16x32_f16, launched in this
// order on one stream: fp16 operands, f32 accumulation, the contract and the work lists of rpo_causal_attn_bwd_f32
// (causal_attn_f32_bwd.hip), the operand layouts of causal_attn_f16.hip.  No atomics.
//
// Maths, per query head h (kv head h / G), query i, key j of one sequence, j <= i + (lk - lq) visible:
//   s = q_i . k_j, p = exp(s scale - lse_i), dP = dO_i . v_j, delta_i = dO_i . O_i,
//   dS = p (dP - delta_i), dQ_i = scale sum_j dS k_j, dK_j = scale sum_h sum_i dS q_i, dV_j = sum_h sum_i p dO_i.
// Arithmetic.  dP stays f32 and a raw score an f32 pair (chunk_add below); p = exp2((s |scale| - lse) log2 e) with log2 e
// carried as hi + lo and Q (dQ kernel) or
// K (dK/dV kernel) negated, exact in fp16, when scale < 0.  No renormalisation by the sum of p as in the f32 backward: one f32 lse
// at |lse| ~ 60 carries ~4e-6 relative into p, two orders below fp16's 2^-11, which the operand rounding costs anyway.  P is
// rounded to fp16 ONCE (the operand of dV); dS is formed in f32 and rounded to fp16 ONCE (the operand of dQ and of dK); the
// scale is applied in f32 to the f32 sums; dq / dk / dv are rounded to fp16 once (overflow -> inf, never saturated).  Masked
// pairs and queries whose lse is -inf get p = dS = 0 exactly; a non-finite dout element makes dP and delta of its query
// non-finite, hence dS of its visible keys and its dq row.
//
// dQ kernel: the forward's block.  One block per (work-list entry = 32 queries of one sequence, kv head), wave w owns query head
//   kvh * G + w; K and V steps of 32 keys staged ONCE in LDS for the group's waves, the next step's rows in flight in registers.
//   The wave keeps Q^T and dO^T of its queries as B operands (k slot 8 g + j = head dim 32 c + 8 g + j); S^T = K Q^T and
//   dP^T = V dO^T per 16-key half (A = 16 rows of the LDS tile, one 16-byte read per operand), so a lane owns ONE query (column
//   l & 15) per 16-query tile and lse / delta stay per lane.  dS^T goes into dQ^T = K^T dS^T as the B operand as it lies in the
//   accumulators (k slot 8 g + j = key 4 g + j (j < 4) / 16 + 4 g + j - 4 (j >= 4) of the step), so K is staged a second time
//   TRANSPOSED, kt[head dim][slot] with slot(key) = 8 ((key & 15) >> 2) + 4 (key >> 4) + (key & 3): the forward's V^T with K for V,
//   one 16-byte read per A operand.  delta = dO . O is formed here, as the diagonal of O dO^T on the MFMA (KS instructions per
//   16-query tile, one shuffle: the summation order of dP, so that a fully cancelling dP - delta is an exact zero), and written to
//   ws[h][t] for the second kernel.  The key loop ends with the step that holds the last visible key of the entry's last query;
//   dq sums the keys ascending in 32-key steps.
// dK/dV kernel: one block of 2 waves per (key work-list entry = 32 keys of one sequence, kv head); wave w OWNS keys 16 w .. 16 w +
//   15 (K and V rows as B operands in registers, dK^T and dV^T accumulators).  It walks the query steps of 32 from the first
//   query that sees the entry's first key to the sequence's end and, inside a step, the G query heads ascending; each (step,
//   head) is summed from zero (the 32 queries are exactly ONE MFMA k) and added to the running total: one order per output
//   element, fixed by the indices alone.  Q and dO of a (step, head) are staged in LDS as rows (A of S = Q K^T, dP = dO V^T: a
//   lane owns ONE key) and transposed, [head dim][slot(query)] (A of dV^T = dO^T P and dK^T = Q^T dS, with P / dS as B as they
//   lie in the accumulators); the next pair's rows are in flight in registers.  S is recomputed in both kernels.
// Every dq row of a listed entry and every dk / dv row of a listed key entry is written; keys no query sees get exact zeros.
// Rows past a sequence's end are loaded clamped to its last row (in bounds) and masked; no access leaves the sequence.
// Budget (the .vgpr_count of `make isa-llama-f16-bwd` under the waves-per-SIMD floors below; no scratch in any of the 16
// instantiations):
// allocated registers per lane / waves per SIMD the allocation allows / LDS bytes per block, G = 1 / 2 / 4 / 8:
//   dQ    head_dim 64:  195 / 163 / 147 / 147 registers, 2 / 3 / 3 / 3 waves per SIMD, 14 336 bytes
//   dQ    head_dim 128: 348 / 284 / 247 / 231 registers, 1 / 1 / 2 / 2 waves per SIMD, 27 648 bytes
//   dK/dV head_dim 64:  162 / 160 / 160 / 160 registers, 3 waves per SIMD, 19 456 bytes
//   dK/dV head_dim 128: 254 / 254 / 254 / 254 registers, 2 waves per SIMD, 37 888 bytes
// The decode of both work lists with its guard, the causal rule, exp through exp2 and the entry's checks and dispatch:
// causal_attn_common.hpp.
// Plain HIP with MFMA builtins; no assembly statements, no counted waits, no atomics: deterministic.
#include "causal_attn_common.hpp"

using namespace causal_attn;

namespace {

constexpr int kTLd = 32 + 8;        // row stride of a transposed tile (elements): rows stay 16-byte aligned, 20 words apart

__device__ __forceinline__ void mma_f16(uint4_t a, uint4_t b, float4_t& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, a), __builtin_bit_cast(half8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ unsigned f16_bits(float f) { return __builtin_bit_cast(unsigned short, (f16_t)f); }
__device__ __forceinline__ unsigned pack2(float a, float b) { return f16_bits(a) | (f16_bits(b) << 16); }
// a + b = s + e exactly (Knuth), per element
__device__ __forceinline__ void two_sum(float4_t a, float4_t b, float4_t& s, float4_t& e) {
    s = a + b;
    const float4_t bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
// A raw score as an f32 PAIR hi + lo.  Each 32-wide chunk of the head dim is ONE MFMA summed from zero, and the chunks' f32 sums
// are added without a rounding (two_sum; the errors, far below hi, by plain adds into lo): what is left of the f32 accumulation
// is one rounding per chunk, at a chunk's
// magnitude, instead of one per chained MFMA at the magnitude of the growing sum -- at raw scores of 3e5 (ulp 2^-5, times the
// scale ~1e-3 in the exponent of p) that is the difference between the fp16 roundoff and three times it.
__device__ __forceinline__ void chunk_add(float4_t part, float4_t& hi, float4_t& lo) {
    float4_t e;
    two_sum(hi, part, hi, e);
    lo += e;
}
// (hi + lo) scale - lse: the product hi x scale enters the fma unrounded, lo x scale is a correction far below it
__device__ __forceinline__ float exponent_of(float hi, float lo, float scale_abs, float lse) {
    return fmaf(lo, scale_abs, fmaf(hi, scale_abs, -lse));
}
// the k slot of row `i` (a key of a dQ step, a query of a dK/dV step) in a transposed tile: where the accumulator layout puts it
__device__ __forceinline__ int slot_of(int i) { return 8 * ((i & 15) >> 2) + 4 * (i >> 4) + (i & 3); }

// one 16-byte chunk of 8 fp16 (columns c0 .. c0 + 7 of row `slot`) -> 8 two-byte stores into the transposed tile t[column][slot]
__device__ __forceinline__ void store_transposed(unsigned short* t, int c0, int slot, uint4_t x) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        t[(c0 + 2 * e) * kTLd + slot] = (unsigned short)(x[e] & 0xffffu);
        t[(c0 + 2 * e + 1) * kTLd + slot] = (unsigned short)(x[e] >> 16);
    }
}

// waves per SIMD asked of the register allocator: what the kernels took unasked before the scores became f32 pairs (the chunk
// accumulators would otherwise cost the dQ kernel of the Llama shapes and the dK/dV kernel one wave per SIMD each)
constexpr int dq_waves(int hd, int g) { return hd == 64 ? (g >= 4 ? 3 : 2) : (g >= 4 ? 2 : 1); }
constexpr int dkdv_waves(int hd) { return hd == 64 ? 3 : 2; }

template <int HD, int G>
__global__ __launch_bounds__(64 * G) __attribute__((amdgpu_waves_per_eu(dq_waves(HD, G))))
void causal_attn_bwd_dq_f16_kernel(
    const f16_t* __restrict__ q, const f16_t* __restrict__ k, const f16_t* __restrict__ v, const f16_t* __restrict__ out,
    const f16_t* __restrict__ dout, int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t out_stride, int64_t dout_stride,
    const float* __restrict__ lse, const int* __restrict__ cu_q, const int* __restrict__ cu_k, const int* __restrict__ tiles,
    int num_seqs, float scale_abs, unsigned sgn_mask, float scale, f16_t* __restrict__ dq, int64_t dq_stride,
    float* __restrict__ ws) {
    constexpr int QS = kQBlock / 16;    // query tiles per wave
    constexpr int KS = HD / 32;         // MFMAs of a 16x16 score block
    constexpr int OB = HD / 16;         // 16-row blocks of dQ^T
    constexpr int KLD = HD + 8;         // LDS row stride of the K and V tiles (elements)
    constexpr int NT = 64 * G;          // threads of the block
    constexpr int NCH = kKeys * HD / 8; // 16-byte chunks of a K (or V) step
    constexpr int CH = (NCH + NT - 1) / NT;   // chunks per thread (head_dim 64 with 8 waves: half the threads stage one chunk)
    static_assert(CH * NT == NCH || (CH == 1 && NCH < NT), "a step splits evenly over the block, or over its first threads");
    __shared__ __attribute__((aligned(16))) unsigned short ks[kKeys * KLD];
    __shared__ __attribute__((aligned(16))) unsigned short vs[kKeys * KLD];
    __shared__ __attribute__((aligned(16))) unsigned short kt_[HD * kTLd];

    Entry ent;
    if (!entry_listed(tiles, num_seqs, ent) || !query_entry_has_work(cu_q, cu_k, ent)) return;   // block-uniform
    const int kvh = blockIdx.y, q0 = ent.row0, tq0 = ent.tq0, lq = ent.lq, tk0 = ent.tk0, lk = ent.lk;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int h = kvh * G + w;
    const int kend = key_loop_end(ent, q0, kQBlock);     // one past the last key any query of the entry sees
    const int64_t qcol = (int64_t)h * HD, kvcol = (int64_t)kvh * HD;
    const int64_t total_q = cu_q[num_seqs];

    uint4_t qf[QS][KS], dof[QS][KS];
    float lsev[QS], delta[QS];
    int lim[QS];                                         // last visible key of this lane's query
    float4_t acc[QS][OB];
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        const int qi = min(q0 + s * 16 + r, lq - 1);     // rows past the end: loaded (in bounds), never stored
        lim[s] = last_visible_key(ent, qi);
        const f16_t* qp = q + (int64_t)(tq0 + qi) * q_stride + qcol + 8 * g;
        const f16_t* dp = dout + (int64_t)(tq0 + qi) * dout_stride + qcol + 8 * g;
        const f16_t* op = out + (int64_t)(tq0 + qi) * out_stride + qcol + 8 * g;
        // delta = dO . O as the DIAGONAL of O dO^T on the MFMA, A = the O rows in the layout of the V rows of a step: where a
        // query's out row IS a V row (the first query of a sequence: p = 1) delta is dP of that key bit for bit, the sum taken
        // in the same order, and dS cancels to an exact zero instead of to f32 summation noise
        float4_t dd{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < KS; ++c) {
            qf[s][c] = *reinterpret_cast<const uint4_t*>(qp + 32 * c);
            dof[s][c] = *reinterpret_cast<const uint4_t*>(dp + 32 * c);
            mma_f16(*reinterpret_cast<const uint4_t*>(op + 32 * c), dof[s][c], dd);
#pragma unroll
            for (int e = 0; e < 4; ++e) qf[s][c][e] ^= sgn_mask;     // scale < 0: -Q, exact
        }
        // dd[i] = O[16 s + 4 g + i] . dO[16 s + r]: the diagonal element of column r lies in lane group r >> 2, register r & 3
        const int di = r & 3;
        const float dsel = di == 0 ? dd[0] : di == 1 ? dd[1] : di == 2 ? dd[2] : dd[3];
        delta[s] = __shfl(dsel, 16 * (r >> 2) + r, 64);
        lsev[s] = lse[(int64_t)h * total_q + tq0 + qi];
#pragma unroll
        for (int b = 0; b < OB; ++b) acc[s][b] = float4_t{0.f, 0.f, 0.f, 0.f};
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
                *reinterpret_cast<uint4_t*>(&vs[key * KLD + 8 * c8]) = vr[c];
                store_transposed(kt_, 8 * c8, slot_of(key), kr[c]);
            }
        }
        __syncthreads();                                   // K, V and K^T of this step visible
        if (kt + kKeys < kend) load_step(kt + kKeys);      // in flight while this step computes

        // per 16-key half b and 16-query tile s: x[i] = s |scale| - lse (from the raw score as an f32 pair) and dpv[i] = dO . v of
        // key kt + 16 b + 4 g + i and query q0 + 16 s + r, then dS = p (dP - delta) in f32, rounded to fp16 ONCE; masked keys and
        // rows without a finite lse: exact zeros.  A half's dS words are packed before the next half's products start.
        unsigned wd[QS][4];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            uint4_t kf[KS], vf[KS];
#pragma unroll
            for (int c = 0; c < KS; ++c) {
                kf[c] = *reinterpret_cast<const uint4_t*>(&ks[(16 * b + r) * KLD + 32 * c + 8 * g]);
                vf[c] = *reinterpret_cast<const uint4_t*>(&vs[(16 * b + r) * KLD + 32 * c + 8 * g]);
            }
#pragma unroll
            for (int s = 0; s < QS; ++s) {
                float4_t hi{0.f, 0.f, 0.f, 0.f}, lo{0.f, 0.f, 0.f, 0.f}, dpv{0.f, 0.f, 0.f, 0.f};
                mma_f16(kf[0], qf[s][0], hi);
                mma_f16(vf[0], dof[s][0], dpv);
#pragma unroll
                for (int c = 1; c < KS; ++c) {
                    float4_t part{0.f, 0.f, 0.f, 0.f};
                    mma_f16(kf[c], qf[s][c], part);
                    mma_f16(vf[c], dof[s][c], dpv);
                    chunk_add(part, hi, lo);
                }
                const int vis = step_visibility(lim[s], kt, g);
                const bool ok = lsev[s] > -INFINITY;
                float ds[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool on = ok && key_visible(b, i, vis);
                    const float p = exp_hilo(exponent_of(hi[i], lo[i], scale_abs, lsev[s]));
                    ds[i] = on ? p * (dpv[i] - delta[s]) : 0.f;
                }
                wd[s][2 * b] = pack2(ds[0], ds[1]);
                wd[s][2 * b + 1] = pack2(ds[2], ds[3]);
            }
        }
        uint4_t sf[QS];
#pragma unroll
        for (int s = 0; s < QS; ++s) sf[s] = uint4_t{wd[s][0], wd[s][1], wd[s][2], wd[s][3]};
        // A = K^T (row = head dim 16 b + r, k slot 8 g + j as dS has it), B = dS^T
#pragma unroll
        for (int b = 0; b < OB; ++b) {
            const uint4_t ka = *reinterpret_cast<const uint4_t*>(&kt_[(16 * b + r) * kTLd + 8 * g]);
#pragma unroll
            for (int s = 0; s < QS; ++s) mma_f16(ka, sf[s], acc[s][b]);
        }
    }

#pragma unroll
    for (int s = 0; s < QS; ++s) {
        const int qi = q0 + s * 16 + r;
        if (qi >= lq) continue;
        f16_t* op = dq + (int64_t)(tq0 + qi) * dq_stride + qcol + 4 * g;
#pragma unroll
        for (int b = 0; b < OB; ++b)
            *reinterpret_cast<uint2_t*>(op + 16 * b) =
                uint2_t{pack2(acc[s][b][0] * scale, acc[s][b][1] * scale), pack2(acc[s][b][2] * scale, acc[s][b][3] * scale)};
        if (g == 0) ws[(int64_t)h * total_q + tq0 + qi] = delta[s];
    }
}

template <int HD, int G>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(dkdv_waves(HD))))
void causal_attn_bwd_dkdv_f16_kernel(
    const f16_t* __restrict__ q, const f16_t* __restrict__ k, const f16_t* __restrict__ v, const f16_t* __restrict__ dout,
    int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t dout_stride, const float* __restrict__ lse,
    const float* __restrict__ ws, const int* __restrict__ cu_q, const int* __restrict__ cu_k, const int* __restrict__ ktiles,
    int num_seqs, float scale_abs, unsigned sgn_mask, float scale, f16_t* __restrict__ dk, int64_t dk_stride,
    f16_t* __restrict__ dv, int64_t dv_stride) {
    constexpr int QS = kQBlock / 16;    // query tiles per step
    constexpr int KS = HD / 32;         // MFMAs of a 16x16 score block
    constexpr int OB = HD / 16;         // 16-row blocks of dK^T / dV^T
    constexpr int LD = HD + 8;          // LDS row stride of the Q and dO tiles (elements)
    constexpr int NT = 128;             // threads of the block: 2 waves of 16 keys
    constexpr int CH = kQBlock * HD / 8 / NT;   // 16-byte chunks of a Q (or dO) step per thread
    static_assert(CH * NT * 8 == kQBlock * HD && kKeys == 32 && QS == 2, "a step must split evenly over the block");
    __shared__ __attribute__((aligned(16))) unsigned short qsm[kQBlock * LD];
    __shared__ __attribute__((aligned(16))) unsigned short dsm[kQBlock * LD];
    __shared__ __attribute__((aligned(16))) unsigned short qtm[HD * kTLd];
    __shared__ __attribute__((aligned(16))) unsigned short dtm[HD * kTLd];

    Entry ent;
    if (!entry_listed(ktiles, num_seqs, ent) || !key_entry_has_work(cu_q, cu_k, ent)) return;   // block-uniform
    const int kvh = blockIdx.y, k0 = ent.row0, tq0 = ent.tq0, lq = ent.lq, tk0 = ent.tk0, lk = ent.lk;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const int kj = k0 + 16 * w + r;                      // this lane's key
    const int64_t kvcol = (int64_t)kvh * HD;
    const int64_t total_q = cu_q[num_seqs];

    uint4_t kf[KS], vf[KS];
    {
        const int64_t row = tk0 + min(kj, lk - 1);       // keys past the end: loaded (in bounds), masked, never stored
        const f16_t* kp = k + row * k_stride + kvcol + 8 * g;
        const f16_t* vp = v + row * v_stride + kvcol + 8 * g;
#pragma unroll
        for (int c = 0; c < KS; ++c) {
            kf[c] = *reinterpret_cast<const uint4_t*>(kp + 32 * c);
            vf[c] = *reinterpret_cast<const uint4_t*>(vp + 32 * c);
#pragma unroll
            for (int e = 0; e < 4; ++e) kf[c][e] ^= sgn_mask;        // scale < 0: -K, exact
        }
    }
    float4_t dka[OB], dva[OB];
#pragma unroll
    for (int b = 0; b < OB; ++b) dka[b] = dva[b] = float4_t{0.f, 0.f, 0.f, 0.f};

    // query steps of 32 from the first query that sees key k0 to the sequence's end; inside a step the G heads in ascending order
    const int qbeg = first_query_seeing(ent, k0);
    const int niter = lq > qbeg ? ((lq - qbeg + kQBlock - 1) / kQBlock) * G : 0;

    // the Q and dO rows of a (step, head) -> registers (rows clamped to the sequence: in bounds; queries past the end are masked)
    uint4_t qr[CH], dr[CH];
    auto load_iter = [&](int it) {
        const int qstep = qbeg + kQBlock * (it / G);
        const int64_t col = (int64_t)(kvh * G + it % G) * HD;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int idx = tid + NT * c, row = idx / (HD / 8), c8 = idx - row * (HD / 8);
            const int64_t t = tq0 + min(qstep + row, lq - 1);
            qr[c] = *reinterpret_cast<const uint4_t*>(q + t * q_stride + col + 8 * c8);
            dr[c] = *reinterpret_cast<const uint4_t*>(dout + t * dout_stride + col + 8 * c8);
        }
    };
    if (niter > 0) load_iter(0);

    for (int it = 0; it < niter; ++it) {
        __syncthreads();                                   // the previous iteration's LDS reads are done
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int idx = tid + NT * c, row = idx / (HD / 8), c8 = idx - row * (HD / 8);
            *reinterpret_cast<uint4_t*>(&qsm[row * LD + 8 * c8]) = qr[c];
            *reinterpret_cast<uint4_t*>(&dsm[row * LD + 8 * c8]) = dr[c];
            store_transposed(qtm, 8 * c8, slot_of(row), qr[c]);
            store_transposed(dtm, 8 * c8, slot_of(row), dr[c]);
        }
        __syncthreads();                                   // Q, dO and their transposes of this iteration visible
        if (it + 1 < niter) load_iter(it + 1);             // in flight while this iteration computes

        const int qstep = qbeg + kQBlock * (it / G);
        const int64_t hrow = (int64_t)(kvh * G + it % G) * total_q + tq0;
        // the statistics of this lane's queries 16 s + 4 g + i
        float lsev[QS][4], dlt[QS][4];
#pragma unroll
        for (int s = 0; s < QS; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t t = hrow + min(qstep + 16 * s + 4 * g + i, lq - 1);
                lsev[s][i] = lse[t];
                dlt[s][i] = ws[t];
            }

        // sc[s][i]: s |scale| - lse (from the raw score as an f32 pair), dp[s][i]: dO . v, of query qstep + 16 s + 4 g + i and
        // key kj
        float4_t sc[QS], dp[QS];
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            float4_t hi{0.f, 0.f, 0.f, 0.f}, lo{0.f, 0.f, 0.f, 0.f};
            dp[s] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < KS; ++c) {
                const uint4_t qa = *reinterpret_cast<const uint4_t*>(&qsm[(16 * s + r) * LD + 32 * c + 8 * g]);
                const uint4_t da = *reinterpret_cast<const uint4_t*>(&dsm[(16 * s + r) * LD + 32 * c + 8 * g]);
                float4_t part{0.f, 0.f, 0.f, 0.f};
                mma_f16(qa, kf[c], part);
                mma_f16(da, vf[c], dp[s]);
                if (c == 0) hi = part; else chunk_add(part, hi, lo);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) sc[s][i] = exponent_of(hi[i], lo[i], scale_abs, lsev[s][i]);
        }
        // P and dS, each rounded to fp16 ONCE, as B operands: k slot 8 g + j = query 4 g + j (j < 4) / 16 + 4 g + j - 4 (j >= 4);
        // masked pairs and rows without a finite lse: exact zeros
        unsigned pw[4], sw[4];
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            float p[4], ds[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int qi = qstep + 16 * s + 4 * g + i;
                const bool on = qi < lq && kj <= last_visible_key(ent, qi) && lsev[s][i] > -INFINITY;
                const float e = exp_hilo(sc[s][i]);
                p[i] = on ? e : 0.f;
                ds[i] = on ? e * (dp[s][i] - dlt[s][i]) : 0.f;
            }
            pw[2 * s] = pack2(p[0], p[1]);
            pw[2 * s + 1] = pack2(p[2], p[3]);
            sw[2 * s] = pack2(ds[0], ds[1]);
            sw[2 * s + 1] = pack2(ds[2], ds[3]);
        }
        const uint4_t pf{pw[0], pw[1], pw[2], pw[3]}, sf{sw[0], sw[1], sw[2], sw[3]};
        // the 32 queries of this (step, head) are ONE MFMA k: summed from zero, and the sum is added to the running total
#pragma unroll
        for (int b = 0; b < OB; ++b) {
            const uint4_t da = *reinterpret_cast<const uint4_t*>(&dtm[(16 * b + r) * kTLd + 8 * g]);
            const uint4_t qa = *reinterpret_cast<const uint4_t*>(&qtm[(16 * b + r) * kTLd + 8 * g]);
            float4_t pv{0.f, 0.f, 0.f, 0.f}, pk{0.f, 0.f, 0.f, 0.f};
            mma_f16(da, pf, pv);
            mma_f16(qa, sf, pk);
            dva[b] += pv;
            dka[b] += pk;
        }
    }

    if (kj < lk) {
        f16_t* kp = dk + (int64_t)(tk0 + kj) * dk_stride + kvcol + 4 * g;
        f16_t* vp = dv + (int64_t)(tk0 + kj) * dv_stride + kvcol + 4 * g;
#pragma unroll
        for (int b = 0; b < OB; ++b) {
            *reinterpret_cast<uint2_t*>(kp + 16 * b) =
                uint2_t{pack2(dka[b][0] * scale, dka[b][1] * scale), pack2(dka[b][2] * scale, dka[b][3] * scale)};
            *reinterpret_cast<uint2_t*>(vp + 16 * b) = uint2_t{pack2(dva[b][0], dva[b][1]), pack2(dva[b][2], dva[b][3])};
        }
    }
}

template <int HD, int G>
void launch(const HostArgs& a, hipStream_t st) {
    const float sa = fabsf(a.scale);
    const unsigned sgn = a.scale < 0.f ? 0x80008000u : 0u;
    if (a.ntiles > 0) {
        const dim3 grid((unsigned)a.ntiles, (unsigned)a.num_kv_heads), block(64 * G);
        RPO_LAUNCH((causal_attn_bwd_dq_f16_kernel<HD, G>), grid, block, 0, st, (const f16_t*)a.q, (const f16_t*)a.k, (const f16_t*)a.v, (const f16_t*)a.out, (const f16_t*)a.dout, a.q_stride, a.k_stride,
                   a.v_stride, a.out_stride, a.dout_stride, (const float*)a.lse, a.cu_q, a.cu_k, a.tiles, (int)a.num_seqs, sa, sgn, a.scale,
                   (f16_t*)a.dq, a.dq_stride, a.ws);
        if (hipPeekAtLastError() != hipSuccess) return;
    }
    if (a.nktiles > 0) {
        const dim3 grid((unsigned)a.nktiles, (unsigned)a.num_kv_heads), block(128);
        RPO_LAUNCH((causal_attn_bwd_dkdv_f16_kernel<HD, G>), grid, block, 0, st, (const f16_t*)a.q, (const f16_t*)a.k, (const f16_t*)a.v, (const f16_t*)a.dout, a.q_stride, a.k_stride,
                   a.v_stride, a.dout_stride, (const float*)a.lse, (const float*)a.ws, a.cu_q, a.cu_k, a.k_tiles, (int)a.num_seqs, sa, sgn,
                   a.scale, (f16_t*)a.dk, a.dk_stride, (f16_t*)a.dv, a.dv_stride);
    }
}

}  // namespace

extern "C" int rpo_causal_attn_bwd_f16(const void* q, const void* k, const void* v, const void* out, const void* dout,
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
    // 16-byte vector loads of q / k / v / out / dout rows, 8-byte stores of dq / dk / dv: 8-element (16-byte) token strides;
    // ws: one float per query
    if (const int rc = check_backward(a, 8, 4)) return rc;
    if (ntiles == 0 && nktiles == 0) return RPO_OK;
    RPO_CAUSAL_ATTN_DISPATCH(launch, a, (hipStream_t)stream)
    return rpo_launch_status();
}
