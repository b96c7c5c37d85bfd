// Item exposure of ranked lists (include/pda_hip_exposure.h): per item and column bucket, how often the lists show it and how often that is a hit.
#include "pda_common.h"
#include "pda_hip_exposure.h"

namespace {

constexpr int EXPO_THREADS = 256;
constexpr int EXPO_MIN_ROWS = 128;            // rows of a workgroup's slab, at least (fewer rows: fewer workgroups)
constexpr int EXPO_MAX_WGS = 512;             // two per CU: a slab of the evaluation's 262 144 x 50 block is 512 rows, 25 600 entries
constexpr int EXPO_MAX_SLAB_ROWS = 1 << 20;   // x 1 024 columns = 2^30 entries: a slab's entry index fits 32 bits
constexpr int EXPO_LDS_BYTES = 48 << 10;      // key + counters of every slot
constexpr int EXPO_MAX_LOG2_SLOTS = 12;
constexpr int EXPO_PROBES = 8;                // linear probes before an entry goes to the global buffers

// COMBINE: the slab's entries are counted in an LDS table with open addressing -- s_key[slot] claimed with atomicCAS (-1 = free), the counters of
// plane p at s_cnt[p * slots + slot] (planes: n_ks of `shown`, then n_ks of `hit`) -- and every occupied slot is added to the buffers once at the
// end.  An entry that finds neither its key nor a free slot within EXPO_PROBES probes is added to the buffers directly, so the result does not
// depend on what fits.  !COMBINE: every entry is added directly.
template <bool HITS, bool COMBINE>
__global__ void __launch_bounds__(EXPO_THREADS) exposure_kernel(const int32_t* __restrict__ topk, int n_rows, int k_cols, int n_items,
                                                                const int64_t* __restrict__ tgt_indptr, const int32_t* __restrict__ tgt_indices,
                                                                const int32_t* __restrict__ Ks, int n_ks, int32_t* shown, int32_t* hit,
                                                                int rows_per_wg, int log2_slots) {
    extern __shared__ int32_t s_mem[];
    __shared__ int32_t s_ks[PDA_EXPOSURE_MAX_KS];
    const int tid = threadIdx.x;
    const int slots = COMBINE ? (1 << log2_slots) : 0, planes = HITS ? 2 * n_ks : n_ks;
    int32_t* s_key = s_mem;
    int32_t* s_cnt = s_mem + slots;
    if constexpr (COMBINE) {
        for (int i = tid; i < slots; i += EXPO_THREADS) s_key[i] = -1;
        for (int i = tid; i < slots * planes; i += EXPO_THREADS) s_cnt[i] = 0;
    }
    if (tid < n_ks) s_ks[tid] = Ks[tid];
    __syncthreads();

    const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
    const int64_t r1 = r0 + rows_per_wg < n_rows ? r0 + rows_per_wg : n_rows;
    const uint32_t n_local = r1 > r0 ? (uint32_t)(r1 - r0) * (uint32_t)k_cols : 0u;
    const int32_t* base = topk + (size_t)r0 * k_cols;
    // entry e of the slab = (row lr, column j); a thread's next entry is EXPO_THREADS further
    uint32_t lr = (uint32_t)tid / (uint32_t)k_cols, j = (uint32_t)tid % (uint32_t)k_cols;
    const uint32_t step_r = EXPO_THREADS / (uint32_t)k_cols, step_j = EXPO_THREADS % (uint32_t)k_cols;
    for (uint32_t e = tid; e < n_local; e += EXPO_THREADS) {
        const int32_t id = base[e];
        int b = n_ks;
        for (int q = n_ks - 1; q >= 0; --q)
            if ((int64_t)j < (int64_t)s_ks[q]) b = q;
        if (b < n_ks && (uint32_t)id < (uint32_t)n_items) {
            bool h = false;
            if constexpr (HITS) {
                const int64_t p0 = tgt_indptr[r0 + lr], p1 = tgt_indptr[r0 + lr + 1];
                for (int64_t p = p0; p < p1; ++p) h |= (tgt_indices[p] == id);
            }
            int slot = -1;
            if constexpr (COMBINE) {
                uint32_t s = ((uint32_t)id * 2654435761u) >> (32 - log2_slots);
                for (int probe = 0; probe < EXPO_PROBES; ++probe) {
                    const int32_t old = atomicCAS(&s_key[s], -1, id);
                    if (old == -1 || old == id) {
                        slot = (int)s;
                        break;
                    }
                    s = (s + 1u) & (uint32_t)(slots - 1);
                }
            }
            if (slot >= 0) {
                atomicAdd(&s_cnt[b * slots + slot], 1);
                if (HITS && h) atomicAdd(&s_cnt[(n_ks + b) * slots + slot], 1);
            } else {
                atomicAdd(shown + (size_t)b * n_items + id, 1);
                if (HITS && h) atomicAdd(hit + (size_t)b * n_items + id, 1);
            }
        }
        lr += step_r;
        j += step_j;
        if (j >= (uint32_t)k_cols) {
            j -= (uint32_t)k_cols;
            ++lr;
        }
    }
    if constexpr (COMBINE) {
        __syncthreads();
        for (int s = tid; s < slots; s += EXPO_THREADS) {
            const int32_t id = s_key[s];
            if (id < 0) continue;
            for (int b = 0; b < n_ks; ++b) {
                const int32_t c = s_cnt[b * slots + s];
                if (c) atomicAdd(shown + (size_t)b * n_items + id, c);
                if constexpr (HITS) {
                    const int32_t ch = s_cnt[(n_ks + b) * slots + s];
                    if (ch) atomicAdd(hit + (size_t)b * n_items + id, ch);
                }
            }
        }
    }
}

template <bool COMBINE>
int exposure_call(const int32_t* topk, int n_rows, int k_cols, int n_items, const int64_t* tgt_indptr, const int32_t* tgt_indices, const int32_t* Ks,
                  int n_ks, int32_t* shown, int32_t* hit, void* stream) {
    if (!topk || !Ks || !shown) return PDA_ERR_ARG;
    const int n_tgt = (tgt_indptr != nullptr) + (tgt_indices != nullptr) + (hit != nullptr);
    if (n_tgt != 0 && n_tgt != 3) return PDA_ERR_ARG;
    if (n_rows < 1 || n_items < 1 || k_cols < 1 || k_cols > 1024 || n_ks < 1 || n_ks > PDA_EXPOSURE_MAX_KS) return PDA_ERR_ARG;
    const bool hits = n_tgt == 3;
    int64_t wgs = ((int64_t)n_rows + EXPO_MIN_ROWS - 1) / EXPO_MIN_ROWS;
    if (wgs > EXPO_MAX_WGS) wgs = EXPO_MAX_WGS;
    const int64_t wgs_min = ((int64_t)n_rows + EXPO_MAX_SLAB_ROWS - 1) / EXPO_MAX_SLAB_ROWS;
    if (wgs < wgs_min) wgs = wgs_min;
    const int rows_per_wg = (int)(((int64_t)n_rows + wgs - 1) / wgs);
    const unsigned grid = (unsigned)(((int64_t)n_rows + rows_per_wg - 1) / rows_per_wg);
    int log2_slots = 0;
    size_t lds = 0;
    if (COMBINE) {
        const size_t per_slot = sizeof(int32_t) * (size_t)(1 + (hits ? 2 : 1) * n_ks);
        log2_slots = EXPO_MAX_LOG2_SLOTS;
        while (((size_t)1 << log2_slots) * per_slot > (size_t)EXPO_LDS_BYTES) --log2_slots;   // (>= 9: 68 bytes per slot at most)
        lds = ((size_t)1 << log2_slots) * per_slot;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hits)
        hipLaunchKernelGGL((exposure_kernel<true, COMBINE>), dim3(grid), dim3(EXPO_THREADS), lds, s, topk, n_rows, k_cols, n_items, tgt_indptr,
                           tgt_indices, Ks, n_ks, shown, hit, rows_per_wg, log2_slots);
    else
        hipLaunchKernelGGL((exposure_kernel<false, COMBINE>), dim3(grid), dim3(EXPO_THREADS), lds, s, topk, n_rows, k_cols, n_items, tgt_indptr,
                           tgt_indices, Ks, n_ks, shown, hit, rows_per_wg, log2_slots);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

}  // namespace

extern "C" int pda_list_exposure(const int32_t* topk, int n_rows, int k_cols, int n_items, const int64_t* tgt_indptr, const int32_t* tgt_indices,
                                 const int32_t* Ks, int n_ks, int32_t* shown, int32_t* hit, void* stream) {
    return exposure_call<true>(topk, n_rows, k_cols, n_items, tgt_indptr, tgt_indices, Ks, n_ks, shown, hit, stream);
}

extern "C" int pda_list_exposure_plain(const int32_t* topk, int n_rows, int k_cols, int n_items, const int64_t* tgt_indptr, const int32_t* tgt_indices,
                                       const int32_t* Ks, int n_ks, int32_t* shown, int32_t* hit, void* stream) {
    return exposure_call<false>(topk, n_rows, k_cols, n_items, tgt_indptr, tgt_indices, Ks, n_ks, shown, hit, stream);
}
