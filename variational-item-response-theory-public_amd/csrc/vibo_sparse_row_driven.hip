// vibo_sparse_row_driven.hip -- the gathered ELBO call on sparse response rows with a row-driven item pass
// (include/vibo_hip_sparse_row_driven.h: THE KEY, THE LAUNCHES), with its extern "C" tail.  The map, the person pass and its finish are
// the column-driven gathered call's (vibo_sparse.hip: sparse_elbo_call); this unit holds what replaces that call's item pass:
//
//   row offsets    a thread per row for the cells it emits, then one workgroup: every thread a contiguous share of the call's rows, an
//                  integer scan of the shares in LDS
//   emit           one wave per row: the row's cells as keys item | person | right at row_off[r] + k; the pad key elsewhere
//   sort           rocPRIM's device radix sort between the two key buffers
//   segment heads  a thread per sorted position; the first position of every item appends itself to the segment list
//   segment sums   one wave per segment: the column-driven item kernel's statements over the batch's own cells of one item
// No float atomics, no LDS outside the scan, no index is trusted: every position is held against n and cap, every person against the map.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include "vibo_sparse_device.hpp"

namespace vibo {

constexpr int kScanThreads = 1024;              // the row-offset scan's one workgroup
constexpr int kEmitMaxBlocks = 4096;            // emit: workgroups of 4 waves until the grid is full
constexpr size_t kSortTempPerKey = 4;           // the bound on the sort's temporary storage that needs no device: bytes per key ...
constexpr size_t kSortTempFixed = 256 * 1024;   // ... and fixed (with both key buffers the caller's, rocPRIM keeps histograms and per-block states only)

struct RowDrivenParams {
    SparseParams p;
    long long max_row_cells;
    int cap;                         // B * max_row_cells < 2^31
    int seg_cap;                     // min(cap, I)
    int shift;                       // bP + 1: the item's place in a key
    int* row_off;                    // [B + 1]
    int* counters;                   // [0]: segments found
    int* seg;                        // [seg_cap]: the sorted position of a segment's first key
    unsigned long long* keys;        // [cap]: emit's target; for the heads and the sums the sorted buffer
};

// Row r of the call: its person q, the first of its cells k0, the clamped cell count `total` and -> the cells it emits: 0 for a row
// that is not live (as row_person: q outside the image, or a person another row owns), else min(total, max_row_cells).
__device__ __forceinline__ int emitted_cells(const RowDrivenParams& rp, const long long r, long long& q, long long& k0, long long& total) {
    const SparseParams& p = rp.p;
    total = 0; k0 = 0;
    q = p.person_index[r];
    if (q < 0 || q >= p.P) return 0;
    if (p.person_slot[q] != (int32_t)r) return 0;
    k0 = clamp_ll(p.row_ptr[q], 0, p.nnz);
    total = clamp_ll(p.row_ptr[q + 1], k0, p.nnz) - k0;
    return (int)(total < rp.max_row_cells ? total : rp.max_row_cells);
}

// len[r] = the cells row r emits, left in row_off[r]: a thread per row (the three dependent loads of a row run B wide, not in the scan)
__global__ __launch_bounds__(256) void sparse_row_lengths_kernel(const RowDrivenParams rp) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rp.p.B) return;
    long long q, k0, total;
    rp.row_off[r] = emitted_cells(rp, r, q, k0, total);
}

// row_off[r]: len[r] -> the emitted cells of the rows before r, in place; row_off[B] = n.  One workgroup: thread t the rows
// [t * share, (t + 1) * share), an integer scan of the shares' sums in LDS between two walks over the share.
__global__ __launch_bounds__(kScanThreads) void sparse_row_offsets_kernel(const RowDrivenParams rp) {
    __shared__ int part[kScanThreads];
    const int t = threadIdx.x;
    const long long B = rp.p.B;
    const long long share = (B + kScanThreads - 1) / kScanThreads;
    const long long r0 = (long long)t * share < B ? (long long)t * share : B;
    const long long r1 = r0 + share < B ? r0 + share : B;
    int sum = 0;
    for (long long r = r0; r < r1; ++r) sum += rp.row_off[r];
    part[t] = sum;
    __syncthreads();
    for (int step = 1; step < kScanThreads; step <<= 1) {      // inclusive scan of the shares (integers: any order gives the same)
        const int add = t >= step ? part[t - step] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int off = part[t] - sum;
    for (long long r = r0; r < r1; ++r) {
        const int len = rp.row_off[r];
        rp.row_off[r] = off;
        off += len;
    }
    if (t == kScanThreads - 1) rp.row_off[B] = part[t];
}

__global__ __launch_bounds__(256) void sparse_emit_kernel(const RowDrivenParams rp) {
    const SparseParams& p = rp.p;
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * 4;
    const unsigned long long pad = (unsigned long long)p.I << rp.shift;
    unsigned long long cut = 0;
    for (long long r = w; r < p.B; r += n_waves) {
        long long q, k0, total;
        const int len = emitted_cells(rp, r, q, k0, total);
        if (lane == 0 && total > len) cut += (unsigned long long)(total - len);      // (a row that is not live has total 0)
        const long long off = rp.row_off[r];
        for (int k = lane; k < len; k += 64) {
            const uint32_t c = p.row_cell[k0 + k];
            const uint32_t i = c >> 1;
            const unsigned long long key = i >= (uint32_t)p.I ? pad      // (counted by the person pass's row_counts)
                                                             : ((unsigned long long)i << rp.shift) | ((unsigned long long)q << 1) | (c & 1u);
            if (off + k < rp.cap) rp.keys[off + k] = key;
        }
    }
    if (lane == 0 && cut > 0 && p.bad) atomicAdd(p.bad, cut);
    // the positions no cell takes
    const long long n = clamp_ll(rp.row_off[p.B], 0, rp.cap);
    const long long threads = (long long)gridDim.x * 256;
    for (long long pos = n + (long long)blockIdx.x * 256 + threadIdx.x; pos < rp.cap; pos += threads) rp.keys[pos] = pad;
}

__global__ __launch_bounds__(256) void sparse_segment_heads_kernel(const RowDrivenParams rp) {
    const long long pos = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n = clamp_ll(rp.row_off[rp.p.B], 0, rp.cap);
    if (pos >= n) return;
    const unsigned long long item = rp.keys[pos] >> rp.shift;
    if (item >= (unsigned long long)rp.p.I) return;                                   // a pad key: the cell of no item
    if (pos > 0 && (rp.keys[pos - 1] >> rp.shift) == item) return;
    const int at = atomicAdd(&rp.counters[0], 1);
    if (at < rp.seg_cap) rp.seg[at] = (int)pos;                                       // (at most one segment per item: at < min(cap, I))
}

template <int MA>
__global__ __launch_bounds__(256) void sparse_segment_kernel(const RowDrivenParams rp) {
    const SparseParams& p = rp.p;
    const int lane = threadIdx.x & 63;
    constexpr int A = MA;      // (one instantiation per ability_dim: every `a < A` below is decided at compile time)
    const int D = p.D, irt = p.irt;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * 4;
    const long long n = clamp_ll(rp.row_off[p.B], 0, rp.cap);
    const int found = rp.counters[0];
    const int n_seg = found < rp.seg_cap ? found : rp.seg_cap;
    const unsigned long long person_mask = (1ull << (rp.shift - 1)) - 1;

    for (long long sg = w; sg < n_seg; sg += n_waves) {
        const long long start = rp.seg[sg];
        if (start < 0 || start >= n) continue;                 // (wave-uniform)
        const unsigned long long i64 = rp.keys[start] >> rp.shift;
        if (i64 >= (unsigned long long)p.I) continue;
        const int i = __builtin_amdgcn_readfirstlane((int)i64);

        const float* it = p.item + (size_t)i * D;
        float disc[MA], diff, glogit = 0.f;
        item_row<MA>(it, irt, disc, diff, glogit);

        float gd[MA], gb = 0.f, gg = 0.f;
#pragma unroll
        for (int a = 0; a < MA; ++a) gd[a] = 0.f;
        for (long long k = start + lane; k < n; k += 64) {
            const unsigned long long key = rp.keys[k];
            if ((key >> rp.shift) != i64) break;               // sorted: the segment ends here for this lane and for every later trip
            const long long q = (long long)((key >> 1) & person_mask);
            if (q >= p.P) continue;
            const long long r = p.person_slot[q];
            if (r == VIBO_SPARSE_NO_SLOT) continue;            // not a person of this call
            if (r < 0 || r >= p.B) continue;                   // (a map entry that is no row: the person is not this call's)
            float th[MA];
#pragma unroll
            for (int a = 0; a < MA; ++a) th[a] = (a < A) ? p.ability[r * A + a] : 0.f;
            float ll, gl, gguess;
            cell_terms<MA>(irt, A, disc, diff, glogit, th, (key & 1ull) ? 1.f : 0.f, ll, gl, gguess);
            gb += gl;
            gg += gguess;
#pragma unroll
            for (int a = 0; a < MA; ++a)
                if (a < A) gd[a] = fmaf(-gl, th[a], gd[a]);
        }

        // column j of the item's row: 1PL [difficulty]; 2PL / 3PL [discrimination 0..A-1 | difficulty | guess logit]
        float out = 0.f;
        if (irt == 1) {
            out = wave_total(gb);
        } else {
#pragma unroll
            for (int a = 0; a < MA; ++a)
                if (a < A) {
                    const float t = wave_total(gd[a]);
                    if (lane == a) out = t;
                }
            const float tb = wave_total(gb);
            if (lane == A) out = tb;
            if (irt == 3) {
                const float tg = wave_total(gg);
                if (lane == A + 1) out = tg;
            }
        }
        if (lane < D) p.grad_item[(size_t)i * D + lane] = out;
    }
}

// ---- host ----
static int bit_length(unsigned long long v) {
    int n = 0;
    for (; v; v >>= 1) ++n;
    return n;
}
// THE KEY of the header for an image of P persons and I items
static int key_shift(long long P) { const int bp = bit_length((unsigned long long)(P - 1)); return (bp < 1 ? 1 : bp) + 1; }
static int key_end_bit(long long P, long long I) { return key_shift(P) + bit_length((unsigned long long)I); }

// cap = B * max_row_cells, or 0 where it is outside [1, 2^31)
static long long row_driven_cap(long long B, long long max_row_cells) {
    if (B < 1 || max_row_cells < 1 || max_row_cells >= (1ll << 31)) return 0;
    const long long cap = B * max_row_cells;      // (both below 2^31: no overflow)
    return cap < (1ll << 31) ? cap : 0;
}

// the workspace behind the person pass's records: byte offsets, each part 256-byte rounded
struct RowDrivenLayout { size_t row_off, counters, seg, keys_a, keys_b, temp, temp_bytes, end; };
static RowDrivenLayout row_driven_layout(long long B, long long I, long long cap) {
    RowDrivenLayout l = {};
    size_t at = 0;
    l.row_off = at;  at += up256((size_t)(B + 1) * sizeof(int));
    l.counters = at; at += 256;
    l.seg = at;      at += up256((size_t)(cap < I ? cap : I) * sizeof(int));
    l.keys_a = at;   at += up256((size_t)cap * sizeof(unsigned long long));
    l.keys_b = at;   at += up256((size_t)cap * sizeof(unsigned long long));
    l.temp = at;     l.temp_bytes = up256((size_t)cap * kSortTempPerKey + kSortTempFixed); at += l.temp_bytes;
    l.end = at;
    return l;
}

#define VIBO_SEGMENT_LAUNCH(W, grid, stream, rp) hipLaunchKernelGGL((sparse_segment_kernel<W>), dim3((unsigned)(grid)), dim3(256), 0, stream, rp)

int sparse_row_driven_item_pass(const SparseParams& p, long long max_row_cells, char* ws, hipStream_t s) {
    int rc = 0;
    const long long cap = row_driven_cap(p.B, max_row_cells);
    if (cap == 0) return fail(-8, "sparse rows: the row-driven item pass takes 1 <= num_person * max_row_cells < 2^31");
    const RowDrivenLayout l = row_driven_layout(p.B, p.I, cap);
    RowDrivenParams rp = {};
    rp.p = p;
    rp.max_row_cells = max_row_cells;
    rp.cap = (int)cap;
    rp.seg_cap = (int)(cap < p.I ? cap : p.I);
    rp.shift = key_shift(p.P);
    rp.row_off = reinterpret_cast<int*>(ws + l.row_off);
    rp.counters = reinterpret_cast<int*>(ws + l.counters);
    rp.seg = reinterpret_cast<int*>(ws + l.seg);
    unsigned long long* keys_a = reinterpret_cast<unsigned long long*>(ws + l.keys_a);
    unsigned long long* keys_b = reinterpret_cast<unsigned long long*>(ws + l.keys_b);
    rp.keys = keys_a;

    if ((rc = hip_rc(hipMemsetAsync(rp.counters, 0, 256, s), "sparse rows row-driven: counter reset")) != 0) return rc;
    hipLaunchKernelGGL(sparse_row_lengths_kernel, dim3((unsigned)(((long long)p.B + 255) / 256)), dim3(256), 0, s, rp);
    if ((rc = launch_rc("sparse rows row lengths launch")) != 0) return rc;
    hipLaunchKernelGGL(sparse_row_offsets_kernel, dim3(1), dim3(kScanThreads), 0, s, rp);
    if ((rc = launch_rc("sparse rows row offsets launch")) != 0) return rc;
    const long long emit_blocks = ((long long)p.B + 3) / 4;
    hipLaunchKernelGGL(sparse_emit_kernel, dim3((unsigned)(emit_blocks > kEmitMaxBlocks ? kEmitMaxBlocks : emit_blocks)), dim3(256), 0, s, rp);
    if ((rc = launch_rc("sparse rows emit launch")) != 0) return rc;

    // the sort: both key buffers are the workspace's, the temporary storage is asked for with a null pointer and held against the bound
    rocprim::double_buffer<unsigned long long> keys(keys_a, keys_b);
    const unsigned end_bit = (unsigned)key_end_bit(p.P, p.I);
    size_t temp_bytes = 0;
    if ((rc = hip_rc(rocprim::radix_sort_keys(nullptr, temp_bytes, keys, (unsigned)cap, 0u, end_bit, s), "sparse rows sort (size query)")) != 0) return rc;
    if (temp_bytes > l.temp_bytes)
        return fail(-8, "sparse rows: the sort asks for %zu bytes of temporary storage, the workspace holds %zu", temp_bytes, l.temp_bytes);
    temp_bytes = l.temp_bytes;
    if ((rc = hip_rc(rocprim::radix_sort_keys(ws + l.temp, temp_bytes, keys, (unsigned)cap, 0u, end_bit, s), "sparse rows sort")) != 0) return rc;
    rp.keys = keys.current();

    hipLaunchKernelGGL(sparse_segment_heads_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, s, rp);
    if ((rc = launch_rc("sparse rows segment heads launch")) != 0) return rc;
    if ((rc = hip_rc(hipMemsetAsync(p.grad_item, 0, (size_t)p.I * p.D * sizeof(float), s), "sparse rows row-driven: grad_item reset")) != 0) return rc;
    long long seg_blocks = ((long long)rp.seg_cap + 3) / 4;
    if (seg_blocks > VIBO_SPARSE_MAX_BLOCKS) seg_blocks = VIBO_SPARSE_MAX_BLOCKS;
    switch (p.A) {
        case 1: VIBO_SEGMENT_LAUNCH(1, seg_blocks, s, rp); break;
        case 2: VIBO_SEGMENT_LAUNCH(2, seg_blocks, s, rp); break;
        case 3: VIBO_SEGMENT_LAUNCH(3, seg_blocks, s, rp); break;
        case 4: VIBO_SEGMENT_LAUNCH(4, seg_blocks, s, rp); break;
        case 5: VIBO_SEGMENT_LAUNCH(5, seg_blocks, s, rp); break;
        case 6: VIBO_SEGMENT_LAUNCH(6, seg_blocks, s, rp); break;
        case 7: VIBO_SEGMENT_LAUNCH(7, seg_blocks, s, rp); break;
        default: VIBO_SEGMENT_LAUNCH(8, seg_blocks, s, rp); break;
    }
    return launch_rc("sparse rows segment sums launch");
}

}  // namespace vibo

using namespace vibo;

extern "C" {

size_t vibo_sparse_row_driven_workspace_bytes(const vibo_desc* d, int64_t num_item, int64_t num_person_image, int64_t max_row_cells) {
    if (sparse_desc_rc(d) != 0) return 0;
    if (num_item != d->num_item || num_item >= (1ll << 31) || num_person_image < 1 || num_person_image >= (1ll << 31)) return 0;
    if (!d->want_grad) return vibo_sparse_workspace_bytes(d, 0);
    const long long cap = row_driven_cap(d->num_person, max_row_cells);
    if (cap == 0) return 0;
    return sparse_record_bytes(d) + row_driven_layout(d->num_person, num_item, cap).end;
}

int vibo_sparse_elbo_fwd_bwd_gather_rows(const vibo_desc* d, const vibo_sparse_image* im, const int64_t* person_index, int32_t* person_slot,
                                         int64_t max_row_cells, const float* table, const float* item, const float* eps,
                                         float* out_scalars, float* ability_mu, float* ability_logvar, float* ability, float* grad_table,
                                         float* grad_item, int64_t* bad_cells, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = sparse_desc_rc(d);
    if (rc) return rc;
    if (!d->want_grad)      // forward only: no item pass at all -- the column-driven call's path, no map, the same bits
        return vibo_sparse_elbo_fwd_bwd_gather(d, im, person_index, person_slot, table, item, eps, out_scalars, ability_mu, ability_logvar,
                                               ability, grad_table, grad_item, bad_cells, workspace, workspace_bytes, stream);
    if (row_driven_cap(d->num_person, max_row_cells) == 0)
        return fail(-8, "sparse rows: the row-driven item pass takes 1 <= num_person * max_row_cells < 2^31 (%d x %lld): use the "
                        "column-driven call, vibo_sparse_elbo_fwd_bwd_gather", d->num_person, (long long)max_row_cells);
    if ((rc = sparse_image_rc(d, im, 0, false, false)) != 0) return rc;
    if (!person_index) return fail(-5, "sparse rows: null person_index");
    if (!person_slot) return fail(-5, "sparse rows: gradients of a gathered call need the person_slot map");
    return sparse_elbo_call(d, im, true, 0, person_index, person_slot, table, item, eps, out_scalars, ability_mu, ability_logvar, ability,
                            grad_table, grad_item, bad_cells, workspace, workspace_bytes, stream, max_row_cells);
}

}  // extern "C"
