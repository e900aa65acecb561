// ag_dense.hip — the reference's dense one-hot relation matrices to the engine's CSR adjacency and back, with no host sync.
//
// edges_from_dense replaces the reading side of DynamicsPredictor.forward's input contract (src/dynamics/model.py:129-160: Rr, Rs (B, E, N) one-hot,
// zero rows = padding), edges_to_dense the writing side of construct_edges_from_states_batch (src/dynamics/dataset/graph.py:146-155).
//
// Contract of edges_from_dense (the statement it is tested against is adaptigraph_amd.graph.csr_from_dense, bit for bit):
//   row (b, e) is an edge  <=>  Rr[b, e, :] and Rs[b, e, :] both hold a non-zero entry (a NaN counts as non-zero)
//   receiver / sender      =    the LOWEST index of a non-zero entry of the row (== argmax for 0/1 rows, multi-hot ones included)
//   order                  :    by global receiver b*N + r, and within one receiver by ascending e (stable): the segment reduce adds in this order
// Indices come from POSITIONS in the row, never from values, so any input content stays in range.
//
// Launches: zero the B*N counters | row scan (one wave per row pair: keys + counts) | two-pass scan of the counts -> row_ptr | stable placement
// (one wave per sample walks its E keys in order).  Integer atomics only.
#include "ag_block_dev.h"
#include "ag_common.h"

namespace {

constexpr int kDenseLdsN = 8192;      // placement: a sample's N write cursors live in LDS up to this N, beyond it in the workspace (same results)

// A row of N floats starts wherever row * N falls, so rows are read and written through the 16-byte "quads" of the tensor's allocation: with `m` =
// the base pointer's misalignment in elements, element i of the tensor is element m + i of the ALIGNED base.  Quads that lie wholly inside the tensor
// move as one 16-byte access (they may overlap the neighbouring rows — in bounds, and masked by the caller); the at most two that stick out of it
// move element by element.
__device__ __forceinline__ int misalign(const float *p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }

// elements [4q, 4q + 4) of the aligned base `a`; those outside the tensor [vlo, vhi) read as 0
__device__ __forceinline__ float4 load_quad(const float *a, long long q, long long vlo, long long vhi)
{
    const long long e0 = q * 4;
    if (e0 >= vlo && e0 + 4 <= vhi) return ag_ld_nt(reinterpret_cast<const float4 *>(a) + q);      // read-once stream
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e0 >= vlo && e0 < vhi) v.x = a[e0];
    if (e0 + 1 >= vlo && e0 + 1 < vhi) v.y = a[e0 + 1];
    if (e0 + 2 >= vlo && e0 + 2 < vhi) v.z = a[e0 + 2];
    if (e0 + 3 >= vlo && e0 + 3 < vhi) v.w = a[e0 + 3];
    return v;
}

// The lanes of a wave hold consecutive quads (lane l: elements e0 = 4 (q0 + l) ..): index within the row [lo, hi) of its first non-zero element, or -1.
// Wave-uniform result: the first set lane of the ballot holds the lowest index.
__device__ __forceinline__ int first_nonzero(const float4 &v, long long e0, long long lo, long long hi, int lane)
{
    int c = 4;
    if (e0 + 3 >= lo && e0 + 3 < hi && v.w != 0.0f) c = 3;      // (NaN != 0: non-zero)
    if (e0 + 2 >= lo && e0 + 2 < hi && v.z != 0.0f) c = 2;
    if (e0 + 1 >= lo && e0 + 1 < hi && v.y != 0.0f) c = 1;
    if (e0 >= lo && e0 < hi && v.x != 0.0f) c = 0;
    const unsigned long long bal = __ballot(c < 4);
    if (!bal) return -1;
    const int src = __ffsll((long long)bal) - 1;
    return (int)(e0 - lo) + 4 * (src - lane) + __shfl(c, src);
}

// One wave per row pair.  Rows of up to ~250 slots are one 16-byte load per lane and tensor, both in flight together; longer rows loop, and stop at
// the first hit.  key_recv[row] = receiver slot or -1 (no edge), key_send[row] = sender slot (written for edges only), cnt[b N + r] += 1.
__global__ __launch_bounds__(256) void dense_rows_kernel(const float *Rr, const float *Rs, int B, int E, int N, int32_t *key_recv,
                                                         int32_t *key_send, int32_t *cnt)
{
    const int lane = threadIdx.x & 63;
    const long long rows = (long long)B * E;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;      // wave-uniform
    const int mr = misalign(Rr), ms = misalign(Rs);
    const float *ar = Rr - mr, *as = Rs - ms;
    const long long lo_r = mr + row * N, hi_r = lo_r + N, lo_s = ms + row * N, hi_s = lo_s + N;
    const long long end_r = mr + rows * N, end_s = ms + rows * N;
    const long long q_r = lo_r >> 2, q_s = lo_s >> 2;
    const int nq_r = (int)(((hi_r + 3) >> 2) - q_r), nq_s = (int)(((hi_s + 3) >> 2) - q_s);
    int fr = -1, fs = -1;
    for (int it = 0;; it += 64) {
        const bool need_r = fr < 0 && it < nq_r, need_s = fs < 0 && it < nq_s;      // wave-uniform
        if (!need_r && !need_s) break;
        if (fr < 0 && !need_r) break;      // the receiver row is all zero: no edge, whatever the sender row holds
        if (fs < 0 && !need_s) break;
        float4 vr = make_float4(0.f, 0.f, 0.f, 0.f), vs = vr;
        if (need_r && it + lane < nq_r) vr = load_quad(ar, q_r + it + lane, mr, end_r);
        if (need_s && it + lane < nq_s) vs = load_quad(as, q_s + it + lane, ms, end_s);
        if (need_r) fr = first_nonzero(vr, (q_r + it + lane) * 4, lo_r, hi_r, lane);
        if (need_s) fs = first_nonzero(vs, (q_s + it + lane) * 4, lo_s, hi_s, lane);
    }
    if (lane == 0) {
        const bool edge = fr >= 0 && fs >= 0;
        key_recv[row] = edge ? fr : -1;
        if (edge) {
            key_send[row] = fs;
            atomicAdd(&cnt[(row / E) * N + fr], 1);
        }
    }
}

// ---- counts -> row_ptr: the two-pass scan of ag_block_dev.h, kScanRows rows per workgroup
__global__ __launch_bounds__(256) void dense_count_partial_kernel(const int32_t *cnt, int rows, int32_t *blk_sum)
{
    const long long r = (long long)blockIdx.x * kScanRows + threadIdx.x;      // (64 bits: B N may sit right under 2^31)
    int total;
    block_exclusive_scan(r < rows ? cnt[r] : 0, &total);
    if (threadIdx.x == 0) blk_sum[blockIdx.x] = total;
}

// every block adds up the partial sums in front of it itself; `cnt` goes from a row's count to its first output position (the placement's cursor)
__global__ __launch_bounds__(256) void dense_rowptr_kernel(int32_t *cnt, int rows, const int32_t *blk_sum, int32_t *row_ptr)
{
    const int base = block_offset(blk_sum);
    const long long r = (long long)blockIdx.x * kScanRows + threadIdx.x;
    int total;
    const int off = base + block_exclusive_scan(r < rows ? cnt[r] : 0, &total);
    if (r < rows) { row_ptr[r] = off; cnt[r] = off; }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) row_ptr[rows] = base + total;
}

// Stable placement, one wave per sample: the sample's keys in ascending e, 64 at a time.  Within a chunk the lanes of one receiver are found by
// ballot (one trip per DISTINCT receiver of the chunk: a handful for inputs in the reference's receiver-sorted order, at most 64), take consecutive
// positions from the receiver's cursor in lane order, and the cursor moves on — so every receiver's edges land in ascending e.
template <bool LDS>
__global__ __launch_bounds__(64) void dense_place_kernel(const int32_t *key_recv, const int32_t *key_send, int32_t *cursor, int E, int N,
                                                         long long cap, int32_t *edge_recv, int32_t *edge_send)
{
    __shared__ int s_cur[LDS ? kDenseLdsN : 1];
    const int b = blockIdx.x, lane = threadIdx.x;
    int *g_cur = cursor + (size_t)b * N;
    if (LDS) {
        for (int i = lane; i < N; i += 64) s_cur[i] = g_cur[i];
        __syncthreads();
    }
    const int32_t *kr = key_recv + (size_t)b * E, *ks = key_send + (size_t)b * E;
    const int g0 = b * N;
    int k = lane < E ? kr[lane] : -1;
    int sd = k >= 0 ? ks[lane] : 0;
    for (long long e0 = 0; e0 < E; e0 += 64) {      // (64 bits: E may sit right under 2^31)
        const long long en = e0 + 64 + lane;                       // the next chunk's keys are on their way while this one is placed
        const int kn = en < E ? kr[en] : -1;
        const int sn = kn >= 0 ? ks[en] : 0;
        unsigned long long rem = __ballot(k >= 0);
        while (rem) {
            const int leader = __ffsll((long long)rem) - 1;
            const int kk = __shfl(k, leader);
            const unsigned long long m = __ballot(k == kk);
            int first = 0;
            if (lane == leader)      // (an atomic for its return value and its ordering; one wave, no contention)
                first = LDS ? atomicAdd(&s_cur[kk], __popcll(m)) : atomicAdd(&g_cur[kk], __popcll(m));
            first = __shfl(first, leader);
            const long long pos = (long long)first + ballot_rank(m, lane);
            if (k == kk && pos >= 0 && pos < cap) {
                edge_recv[pos] = g0 + kk;
                edge_send[pos] = g0 + sd;
            }
            rem &= ~m;
        }
        k = kn;
        sd = sn;
    }
}

// ---- CSR -> dense: one wave per output row (b, j) writes the row's N floats of both tensors, zeros included.
__device__ __forceinline__ void write_onehot_row(float *P, long long row, int N, int one, int lane)
{
    const int m = misalign(P);
    float *a = P - m;
    const long long lo = m + row * N, hi = lo + N, hot = one >= 0 ? lo + one : -1;
    for (long long q = (lo >> 2) + lane; q * 4 < hi; q += 64) {
        const long long e0 = q * 4;
        if (e0 >= lo && e0 + 4 <= hi)
            reinterpret_cast<float4 *>(a)[q] = make_float4(e0 == hot ? 1.f : 0.f, e0 + 1 == hot ? 1.f : 0.f, e0 + 2 == hot ? 1.f : 0.f, e0 + 3 == hot ? 1.f : 0.f);
        else
            for (int c = 0; c < 4; ++c)      // a quad shared with a neighbouring row: this row's elements only
                if (e0 + c >= lo && e0 + c < hi) a[e0 + c] = e0 + c == hot ? 1.f : 0.f;
    }
}

__global__ __launch_bounds__(256) void dense_fill_kernel(const int32_t *row_ptr, const int32_t *edge_recv, const int32_t *edge_send, int B, int N,
                                                         int E_out, float *Rr, float *Rs, int32_t *overflow)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == 0 && wave == 0) {      // the overflow word is written exactly once per call, 0 or 1
        bool over = false;
        for (int b = lane; b < B; b += 64) over = over || (long long)row_ptr[(size_t)(b + 1) * N] - row_ptr[(size_t)b * N] > E_out;
        const bool any = __ballot(over) != 0;
        if (lane == 0) *overflow = any ? 1 : 0;
    }
    const long long rows = (long long)B * E_out;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const int b = (int)(row / E_out), j = (int)(row - (long long)b * E_out);
    const int start = row_ptr[(size_t)b * N], end = row_ptr[(size_t)(b + 1) * N];
    int r = -1, s = -1;
    if (start >= 0 && j < (long long)end - start) {      // edges behind the first E_out of a sample are dropped; the indices are checked, not trusted
        r = edge_recv[start + j] - b * N;
        s = edge_send[start + j] - b * N;
        if ((unsigned)r >= (unsigned)N) r = -1;
        if ((unsigned)s >= (unsigned)N) s = -1;
    }
    write_onehot_row(Rr, row, N, r, lane);
    write_onehot_row(Rs, row, N, s, lane);
}

}  // namespace

void ag_launch_edges_from_dense(const AgDenseArgs &a, hipStream_t s)
{
    const int rows = a.B * a.N;
    const long long pairs = (long long)a.B * a.E;
    ag_launch_zero_words(a.cnt, rows, s);
    hipLaunchKernelGGL(dense_rows_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, s, a.Rr, a.Rs, a.B, a.E, a.N, a.key_recv, a.key_send, a.cnt);
    const int nblk = (rows + kScanRows - 1) / kScanRows;
    hipLaunchKernelGGL(dense_count_partial_kernel, dim3(nblk), dim3(256), 0, s, a.cnt, rows, a.blk_sum);
    hipLaunchKernelGGL(dense_rowptr_kernel, dim3(nblk), dim3(256), 0, s, a.cnt, rows, a.blk_sum, a.row_ptr);
    if (a.N <= kDenseLdsN)
        hipLaunchKernelGGL(dense_place_kernel<true>, dim3(a.B), dim3(64), 0, s, a.key_recv, a.key_send, a.cnt, a.E, a.N, pairs, a.edge_recv, a.edge_send);
    else
        hipLaunchKernelGGL(dense_place_kernel<false>, dim3(a.B), dim3(64), 0, s, a.key_recv, a.key_send, a.cnt, a.E, a.N, pairs, a.edge_recv, a.edge_send);
}

void ag_launch_edges_to_dense(const int32_t *row_ptr, const int32_t *edge_recv, const int32_t *edge_send, int B, int N, int E_out, float *Rr,
                              float *Rs, int32_t *overflow, hipStream_t s)
{
    const long long rows = (long long)B * E_out;
    hipLaunchKernelGGL(dense_fill_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, row_ptr, edge_recv, edge_send, B, N, E_out, Rr, Rs, overflow);
}
