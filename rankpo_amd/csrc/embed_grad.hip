// Embedding-table gradient of the packed BERT / XLM-R training step without atomics (`ops.embed_grad_sorted`, header section 10c;
// opt-in: encoder.BERT_DETERMINISTIC_EMBED_GRAD).  The rows of ds [T, d] that share a table row are summed in an order fixed by the
// ids alone, in f32, and every touched table row is written once in the storage dtype.  The grouping is host work
// (`ops.embed_grad_plan`: stable ascending sort of the ids, one segment per distinct id, every segment cut into chunks of at most
// EMBED_GRAD_CHUNK rows); the kernels only walk it:
//   embed_grad_chunk_kernel   one wave per (chunk, 512-column slice = blockIdx.y): the chunk's rows, in ascending packed-token
//                             order, added one after the other into f32 registers.  The only chunk of its segment: rounded and
//                             stored to the table row.  Otherwise: stored as an f32 partial to workspace row `slot`.
//   embed_grad_finish_kernel  one wave per (segment of several chunks, slice): its partials added in ascending chunk order, rounded
//                             once, stored.
// A token that occurs thousands of times (a pad-like id, one of two token types) is therefore spread over T / chunk waves.
// Plain HIP; no atomics, nothing depends on how blocks are scheduled.  A file of its own: bert_ops.hip's code stays what it is.
#include "common.hpp"

namespace {

constexpr int kEgWaves = 4;          // waves per block, one work item each
constexpr int kEgSliceCols = 512;    // 64 lanes x 16 bytes of a 16-bit row

template <typename T> __device__ __forceinline__ void add_row(float (&acc)[8], const Vec16<T>& x) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += x.v[j];
}

template <typename T> __device__ __forceinline__ void store_rounded(T* p, const float (&acc)[8]) {
    Vec16<T> r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r.v[j] = acc[j];
    r.store(p);
}

// The plan is host-built and trusted for WHAT it sums; the range checks below only keep a damaged one from reaching memory outside
// the caller's buffers (such an item is skipped, a token index is clamped as the forward kernels clamp theirs).
template <typename T>
__global__ __launch_bounds__(64 * kEgWaves) void embed_grad_chunk_kernel(
    const T* __restrict__ ds, int64_t ldds, int tokens, int d, const int* __restrict__ order, const int* __restrict__ chunks,
    int64_t n_chunks, int64_t n_partials, T* __restrict__ out, int64_t ldout, int64_t table_rows, int64_t padding_idx,
    float* __restrict__ ws) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t c = (int64_t)blockIdx.x * kEgWaves + wave;
    if (c >= n_chunks) return;
    const int slice = (int)blockIdx.y;
    const int* ch = chunks + 4 * c;
    const int row = ch[0], start = ch[1], n = ch[2], slot = ch[3];
    if (row < 0 || row >= table_rows || row == padding_idx || start < 0 || n < 1 || (int64_t)start + n > tokens ||
        slot >= n_partials)
        return;
    const int col = slice * kEgSliceCols + (int)(threadIdx.x & 63) * 8;
    if (col >= d) return;                                           // d % 8 == 0: a lane has a whole vector or nothing
    const int* ord = order + start;
    const T* src = ds + col;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    int i = 0;
    for (; i + 4 <= n; i += 4) {                                    // four loads in flight, added in row order
        Vec16<T> x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int t = ord[i + u];
            t = t < 0 ? 0 : (t >= tokens ? tokens - 1 : t);
            x[u].load(src + (int64_t)t * ldds);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) add_row<T>(acc, x[u]);
    }
    for (; i < n; ++i) {
        int t = ord[i];
        t = t < 0 ? 0 : (t >= tokens ? tokens - 1 : t);
        Vec16<T> x;
        x.load(src + (int64_t)t * ldds);
        add_row<T>(acc, x);
    }
    if (slot < 0) {
        store_rounded<T>(out + (int64_t)row * ldout + col, acc);
    } else {
        float* p = ws + (int64_t)slot * d + col;
        *reinterpret_cast<float4*>(p) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        *reinterpret_cast<float4*>(p + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
}

template <typename T>
__global__ __launch_bounds__(64 * kEgWaves) void embed_grad_finish_kernel(
    const int* __restrict__ multi, int64_t n_multi, int d, int64_t n_partials, const float* __restrict__ ws,
    T* __restrict__ out, int64_t ldout, int64_t table_rows, int64_t padding_idx) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t m = (int64_t)blockIdx.x * kEgWaves + wave;
    if (m >= n_multi) return;
    const int slice = (int)blockIdx.y;
    const int* mu = multi + 3 * m;
    const int row = mu[0], slot0 = mu[1], k = mu[2];
    if (row < 0 || row >= table_rows || row == padding_idx || slot0 < 0 || k < 1 || (int64_t)slot0 + k > n_partials) return;
    const int col = slice * kEgSliceCols + (int)(threadIdx.x & 63) * 8;
    if (col >= d) return;
    const float* p = ws + (int64_t)slot0 * d + col;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int i = 0; i < k; ++i, p += d) {
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
        acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w;
        acc[4] += b.x; acc[5] += b.y; acc[6] += b.z; acc[7] += b.w;
    }
    store_rounded<T>(out + (int64_t)row * ldout + col, acc);
}

}  // namespace

extern "C" int64_t rpo_embed_grad_workspace_elems(int64_t n_partials, int64_t d) {
    return n_partials <= 0 || d <= 0 ? 0 : n_partials * d;
}

extern "C" int rpo_embed_grad_sorted(const void* ds, int64_t ldds, int64_t tokens, int64_t d, int dtype, const int* order,
                                     const int* chunks, int64_t n_chunks, const int* multi, int64_t n_multi, int64_t n_partials,
                                     void* out, int64_t ldout, int64_t table_rows, int64_t padding_idx, float* workspace,
                                     int64_t workspace_elems, rpo_stream_t stream) {
    if (!ds || !out || tokens < 0 || tokens > INT32_MAX || d <= 0 || table_rows <= 0 || table_rows > INT32_MAX || ldds < d ||
        ldout < d || !rpo_dtype_ok(dtype) || n_chunks < 0 || n_multi < 0 || n_partials < 0 || padding_idx < -1 ||
        padding_idx >= table_rows || (n_chunks > 0 && (!order || !chunks)) || (n_multi > 0 && !multi) ||
        (n_partials > 0 && !workspace) || (n_multi > 0) != (n_partials > 0))
        return RPO_ERR_INVALID_ARG;
    if (dtype == RPO_DT_F32 || d % 8 || d > 65535 * (int64_t)kEgSliceCols) return RPO_ERR_UNSUPPORTED;    // slices = grid.y
    if (!rpo_aligned16(ds) || !rpo_aligned16(out) || ldds % 8 || ldout % 8 || (n_partials > 0 && !rpo_aligned16(workspace)))
        return RPO_ERR_UNSUPPORTED;
    if (workspace_elems < rpo_embed_grad_workspace_elems(n_partials, d)) return RPO_ERR_WORKSPACE;
    if (tokens == 0 || n_chunks == 0) return RPO_OK;
    const unsigned nslices = (unsigned)rpo_cdiv(d, kEgSliceCols);
    if (n_chunks > INT32_MAX || n_multi > INT32_MAX) return RPO_ERR_UNSUPPORTED;       // a real plan has at most `tokens` of each
    const dim3 block(64 * kEgWaves), grid1((unsigned)rpo_cdiv(n_chunks, kEgWaves), nslices),
        grid2((unsigned)rpo_cdiv(n_multi, kEgWaves), nslices);
    hipStream_t st = (hipStream_t)stream;
#define RPO_EG(T)                                                                                                              \
    do {                                                                                                                       \
        RPO_LAUNCH(embed_grad_chunk_kernel<T>, grid1, block, 0, st, (const T*)ds, ldds, (int)tokens, (int)d, order, chunks,    \
                   n_chunks, n_partials, (T*)out, ldout, table_rows, padding_idx, workspace);                         \
        if (n_multi > 0) {                                                                                                     \
            const int rc = rpo_launch_status();                                                                                \
            if (rc != RPO_OK) return rc;                                                                                       \
            RPO_LAUNCH(embed_grad_finish_kernel<T>, grid2, block, 0, st, multi, n_multi, (int)d, n_partials,                   \
                       (const float*)workspace, (T*)out, ldout, table_rows, padding_idx);                                      \
        }                                                                                                                      \
    } while (0)
    if (dtype == RPO_DT_BF16) RPO_EG(bf16_t);
    else RPO_EG(f16_t);
#undef RPO_EG
    return rpo_launch_status();
}
