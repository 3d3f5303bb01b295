// What the four causal, grouped-query, variable-length attention units share (causal_attn_f32.hip, causal_attn_f32_bwd.hip,
// causal_attn_f16.hip, causal_attn_f16_bwd.hip; header sections 9c-9f): the block constants, the decode of a work-list entry with
// its validity guard, the causal rule, the running-maximum step of the online softmax, and on the host the argument checks of the
// four entries and their (head_dim, group) dispatch.  The MFMA bodies stay in the units: their operand layouts differ.
// Plain HIP; no assembly statements, no counted waits, no read-modify-write memory operations.
#pragma once
#include "common.hpp"

namespace causal_attn {

constexpr int kQBlock = 32;         // queries per query work-list entry = queries per step of the dK/dV kernels
constexpr int kKeys = 32;           // keys per step of the forward and dQ kernels = keys per key work-list entry
constexpr float kLog2eHi = 1.44269502162933349609375f;        // (float)log2(e)
constexpr float kLog2eLo = 1.92596299112661746e-8f;           // log2(e) - kLog2eHi

// exp(x) through exp2 with log2(e) as hi + lo
__device__ __forceinline__ float exp_hilo(float x) { return __builtin_amdgcn_exp2f(fmaf(x, kLog2eHi, x * kLog2eLo)); }

// ---- work-list entries ---------------------------------------------------------------------------
// One entry (sequence id, first row) of a query or key work list, decoded against cu_q / cu_k.
struct Entry {
    int seq, row0;      // sequence, first query (query list) or first key (key list) of the block
    int tq0, lq;        // first packed query token of the sequence, its queries
    int tk0, lk;        // first packed key token of the sequence, its keys
    int shift;          // lk - lq: query i sees keys j <= i + shift (bottom-right aligned)
};

// The decode, in two steps that a kernel joins in ONE block-uniform test,
//     Entry ent;
//     if (!entry_listed(list, num_seqs, ent) || !query_entry_has_work(cu_q, cu_k, ent)) return;
// (two plain predicates joined by the kernel's own ||: the form whose generated code is the hand-written prologue's; one function
// with early returns moved the register allocation of every instantiation).
// Step 1: entry blockIdx.x of `list`.  False for an entry that names no sequence or a negative row: cu_q / cu_k are not read for it.
__device__ __forceinline__ bool entry_listed(const int* __restrict__ list, int num_seqs, Entry& e) {
    const int entry = blockIdx.x;
    e.seq = list[2 * entry];
    e.row0 = list[2 * entry + 1];
    return !(e.seq < 0 || e.seq >= num_seqs || e.row0 < 0);
}
__device__ __forceinline__ void entry_lengths(const int* __restrict__ cu_q, const int* __restrict__ cu_k, Entry& e) {
    e.tq0 = cu_q[e.seq];
    e.lq = cu_q[e.seq + 1] - e.tq0;
    e.tk0 = cu_k[e.seq];
    e.lk = cu_k[e.seq + 1] - e.tk0;
    e.shift = e.lk - e.lq;
}
// Step 2, query list: false for a sequence without queries or keys and for a first query past the end.
__device__ __forceinline__ bool query_entry_has_work(const int* __restrict__ cu_q, const int* __restrict__ cu_k, Entry& e) {
    entry_lengths(cu_q, cu_k, e);
    return !(e.lq <= 0 || e.lk <= 0 || e.row0 >= e.lq);
}
// Step 2, key list: false for a sequence without keys and for a first key past the end (a sequence without queries still
// zero-fills its dk / dv rows).
__device__ __forceinline__ bool key_entry_has_work(const int* __restrict__ cu_q, const int* __restrict__ cu_k, Entry& e) {
    entry_lengths(cu_q, cu_k, e);
    return !(e.lk <= 0 || e.row0 >= e.lk);
}

// ---- the causal rule -----------------------------------------------------------------------------
// The last key query qi sees (`lim`), and one past the last key any of the queries q0 .. q0 + nq - 1 sees: where a key loop ends.
__device__ __forceinline__ int last_visible_key(const Entry& e, int qi) { return qi + e.shift; }
__device__ __forceinline__ int key_loop_end(const Entry& e, int q0, int nq) { return min(e.lk, min(q0 + nq, e.lq) + e.shift); }
// the first query that sees key kj: where the query walk of a key block starts
__device__ __forceinline__ int first_query_seeing(const Entry& e, int kj) { return max(0, kj - e.shift); }
// In the step that starts at key kt, lane group g holds keys kt + 16 b + 4 g + i (b < 2, i < 4) of a query whose last visible key
// is lim: with vis = step_visibility(lim, kt, g), key (b, i) is visible iff key_visible(b, i, vis).
__device__ __forceinline__ int step_visibility(int lim, int kt, int g) { return lim - kt - 4 * g; }
__device__ __forceinline__ bool key_visible(int b, int i, int vis) { return 16 * b + i <= vis; }

// The running-maximum step of the forward's online softmax for one query: s0 / s1 = the raw scores of this lane's keys in the two
// 16-key halves.  Masked keys do not enter the maximum; it is reduced over the 4 lane groups of the query.  mrun becomes the new
// maximum; returns alpha = exp((old - new) |scale|), 0 on the first step.
__device__ __forceinline__ float running_max_step(const float4_t& s0, const float4_t& s1, int vis, float scale_abs, float& mrun) {
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (key_visible(0, i, vis)) mx = fmaxf(mx, s0[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (key_visible(1, i, vis)) mx = fmaxf(mx, s1[i]);
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(mrun, mx);               // finite from the first step on: key 0 is visible to every query
    const float alpha = mrun == -INFINITY ? 0.f : exp_hilo((mrun - mn) * scale_abs);
    mrun = mn;
    return alpha;
}

// ---- host side -----------------------------------------------------------------------------------
// The arguments of the four entries as the header names them; a forward entry leaves the backward's fields zero.
struct HostArgs {
    const void *q, *k, *v;
    int64_t q_stride, k_stride, v_stride;
    const int *cu_q, *cu_k, *tiles;
    int64_t ntiles, tile_cols, q_block, num_seqs, num_heads, num_kv_heads, head_dim;
    float scale;
    void* out;              // forward: written; backward: the forward's result, read
    int64_t out_stride;
    float* lse;             // forward: written where not null; backward: read
    const void* dout;
    int64_t dout_stride;
    const int* k_tiles;
    int64_t nktiles;
    void *dq, *dk, *dv;
    int64_t dq_stride, dk_stride, dv_stride;
    float* ws;
};

static inline bool misaligned(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0; }
// a [tokens, heads * head_dim] operand read or written with 16-byte (f32 out: 16, fp16 out: 8) vectors
static inline bool bad_rows(const void* p, int64_t stride, int mult) { return misaligned(p, 16) || stride % mult != 0; }

static inline bool forward_args_invalid(const HostArgs& a) {
    return !a.q || !a.k || !a.v || !a.cu_q || !a.cu_k || !a.tiles || !a.out || a.ntiles < 0 || a.num_seqs <= 0 ||
           a.num_seqs >= 0x7fffffff || a.num_heads <= 0 || a.num_kv_heads <= 0 || a.head_dim <= 0 || a.q_stride <= 0 ||
           a.k_stride <= 0 || a.v_stride <= 0 || a.out_stride <= 0 || !(fabsf(a.scale) <= 3.0e38f);
}
static inline bool shape_unsupported(const HostArgs& a) {
    if ((a.head_dim != 64 && a.head_dim != 128) || a.num_heads % a.num_kv_heads != 0 || a.tile_cols != 2 || a.q_block != kQBlock ||
        a.ntiles > 0x7fffffff || a.nktiles > 0x7fffffff || a.num_kv_heads > 65535)
        return true;
    const int64_t group = a.num_heads / a.num_kv_heads;
    return group != 1 && group != 2 && group != 4 && group != 8;
}

// The refusals of rpo_causal_attn_fwd_f32 / _f16, in the header's order.  stride_mult: elements per 16 bytes (4 / 8).
static inline int check_forward(const HostArgs& a, int stride_mult) {
    if (forward_args_invalid(a)) return RPO_ERR_INVALID_ARG;
    if (shape_unsupported(a)) return RPO_ERR_UNSUPPORTED;
    if (bad_rows(a.q, a.q_stride, stride_mult) || bad_rows(a.k, a.k_stride, stride_mult) || bad_rows(a.v, a.v_stride, stride_mult) ||
        bad_rows(a.out, a.out_stride, stride_mult) || (a.lse && misaligned(a.lse, 4)))
        return RPO_ERR_UNSUPPORTED;
    return RPO_OK;
}

// The refusals of rpo_causal_attn_bwd_f32 / _f16.  ws_align: bytes (16: the f32 kernels' 8-byte pairs; 4: one float per query).
static inline int check_backward(const HostArgs& a, int stride_mult, unsigned ws_align) {
    if (forward_args_invalid(a) || !a.dout || !a.lse || !a.k_tiles || !a.dq || !a.dk || !a.dv || !a.ws || a.nktiles < 0 ||
        a.dout_stride <= 0 || a.dq_stride <= 0 || a.dk_stride <= 0 || a.dv_stride <= 0)
        return RPO_ERR_INVALID_ARG;
    if (shape_unsupported(a)) return RPO_ERR_UNSUPPORTED;
    if (bad_rows(a.q, a.q_stride, stride_mult) || bad_rows(a.k, a.k_stride, stride_mult) || bad_rows(a.v, a.v_stride, stride_mult) ||
        bad_rows(a.out, a.out_stride, stride_mult) || bad_rows(a.dout, a.dout_stride, stride_mult) ||
        bad_rows(a.dq, a.dq_stride, stride_mult) || bad_rows(a.dk, a.dk_stride, stride_mult) ||
        bad_rows(a.dv, a.dv_stride, stride_mult) || misaligned(a.lse, 4) || misaligned(a.ws, ws_align))
        return RPO_ERR_UNSUPPORTED;
    return RPO_OK;
}

}  // namespace causal_attn

// LAUNCH<HD, G>(a, st) for the head_dim 64 / 128 and the 1 / 2 / 4 / 8 query heads per kv head of a checked HostArgs
#define RPO_CAUSAL_ATTN_CASE(LAUNCH, HD, G, a, st) \
    if ((a).head_dim == HD && (a).num_heads == G * (a).num_kv_heads) LAUNCH<HD, G>(a, st);
#define RPO_CAUSAL_ATTN_DISPATCH(LAUNCH, a, st)  \
    RPO_CAUSAL_ATTN_CASE(LAUNCH, 64, 1, a, st)   \
    RPO_CAUSAL_ATTN_CASE(LAUNCH, 64, 2, a, st)   \
    RPO_CAUSAL_ATTN_CASE(LAUNCH, 64, 4, a, st)   \
    RPO_CAUSAL_ATTN_CASE(LAUNCH, 64, 8, a, st)   \
    RPO_CAUSAL_ATTN_CASE(LAUNCH, 128, 1, a, st)  \
    RPO_CAUSAL_ATTN_CASE(LAUNCH, 128, 2, a, st)  \
    RPO_CAUSAL_ATTN_CASE(LAUNCH, 128, 4, a, st)  \
    RPO_CAUSAL_ATTN_CASE(LAUNCH, 128, 8, a, st)
