// Popularity-weighted negative sampling (include/pda_hip_negpop.h) on MI355X (gfx950): the uniform samplers' kernels with the
// negative of a row drawn through an alias table.  Every piece of a row -- step, user, positive, time slot, membership test, the alias try
// itself -- is pda_sample.h's; here are only the kernels around them and the entry points' checks.
//
// Layout: that of the uniform twins.  A thread is a chain of dependent loads (user -> train row bounds -> table slot -> binary search), so one
// wave per workgroup spreads the chains over the CUs (pda_aux.hip measured 13 -> 9 us for that choice).  The rejection loop diverges: a wave
// runs as long as its unluckiest lane, and a try costs two hashes (independent, issued together), one 8-byte gather and one search.
#include "pda_common.h"
#include "pda_sample.h"
#include "pda_hip_negpop.h"

namespace {

__device__ __forceinline__ int triplet_negative(const SampleArgs& a, const uint64_t* alias, int r, int64_t b, int64_t e) {
    return sample_negative_alias(a.seed, a.step, r, kNegDraw, (uint32_t)(a.neg_hi - a.neg_lo), a.neg_lo, alias, a.indices, b, e);
}

__global__ void __launch_bounds__(64) negpop_sample_kernel(SampleArgs a, const uint64_t* alias) {
    sample_row<false>(a, (int)(blockIdx.x * blockDim.x + threadIdx.x),
                      [alias](const SampleArgs& a, int r, int64_t b, int64_t e) { return triplet_negative(a, alias, r, b, e); });
}

// blockIdx.y = batch j, drawn with step + j into row j of the [n][B] buffers: the slicing of sample_batches_kernel (pda_aux.hip)
__global__ void __launch_bounds__(64) negpop_sample_batches_kernel(SampleArgs a, const uint64_t* alias, int n_batches) {
    const int j = (int)blockIdx.y, r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const uint64_t cur = a.step_dev ? *a.step_dev : 0ull;
    if (a.step_next && j == 0 && r == 0) *a.step_next = cur + (uint64_t)n_batches;
    a.step += cur + (uint64_t)j;
    a.step_dev = nullptr;
    a.step_next = nullptr;
    const size_t off = (size_t)j * a.B;
    a.users += off;
    a.pos += off;
    a.neg += off;
    if (a.pos_pop) { a.pos_pop += off; a.neg_pop += off; }
    sample_row<false>(a, r, [alias](const SampleArgs& a, int r, int64_t b, int64_t e) { return triplet_negative(a, alias, r, b, e); });
}

__global__ void __launch_bounds__(64) negpop_ssm_sample_kernel(SsmSampleArgs a, const uint64_t* alias) {
    sample_block_entry(a, (size_t)blockIdx.x * 64 + threadIdx.x, [alias](const SsmSampleArgs& a, int r, uint32_t first_draw, int64_t b, int64_t e) {
        return sample_negative_alias(a.seed, a.step, r, first_draw, (uint32_t)(a.neg_hi - a.neg_lo), a.neg_lo, alias, a.indices, b, e);
    });
}

// The three triplet entry points.  counter: the _dev variants; n_batches 0: one batch, else [n_batches][B] buffers.
int negpop_triplets(bool counter, const SampleArgs& a, const uint64_t* alias, int n_batches, void* stream) {
    if (!alias || !triplet_sample_ok(a, counter)) return PDA_ERR_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned blocks = (unsigned)((a.B + 63) / 64);
    if (n_batches) hipLaunchKernelGGL(negpop_sample_batches_kernel, dim3(blocks, (unsigned)n_batches), dim3(64), 0, s, a, alias, n_batches);
    else hipLaunchKernelGGL(negpop_sample_kernel, dim3(blocks), dim3(64), 0, s, a, alias);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

int negpop_block(bool counter, const SsmSampleArgs& a, const uint64_t* alias, void* stream) {
    if (!alias || !block_sample_ok(a, counter, PDA_SSM_MAX_NEGS)) return PDA_ERR_ARG;
    const size_t n = (size_t)a.B * (size_t)a.N;             // <= 2^30: B <= 2^22, N <= 256
    hipLaunchKernelGGL(negpop_ssm_sample_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), a, alias);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

}  // namespace

extern "C" int pda_negpop_sample_triplets(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, const int64_t* train_indptr,
                                          const int32_t* train_indices, const int32_t* train_slots, int neg_lo, int neg_hi, const uint64_t* alias,
                                          const float* pop_matrix, int n_slots, uint64_t seed, uint64_t step, int32_t* pos, int32_t* neg,
                                          float* pos_pop, float* neg_pop, void* stream) {
    return negpop_triplets(false, SampleArgs{users, user_pool, train_indptr, train_indices, train_slots, pop_matrix, pos, neg, pos_pop, neg_pop, seed,
                                             step, B, n_pool, gen_users, neg_lo, neg_hi, n_slots, nullptr, nullptr}, alias, 0, stream);
}

extern "C" int pda_negpop_sample_triplets_dev(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B,
                                              const int64_t* train_indptr, const int32_t* train_indices, const int32_t* train_slots, int neg_lo,
                                              int neg_hi, const uint64_t* alias, const float* pop_matrix, int n_slots, uint64_t seed,
                                              const uint64_t* step_dev, uint64_t* step_next, int32_t* pos, int32_t* neg, float* pos_pop,
                                              float* neg_pop, void* stream) {
    return negpop_triplets(true, SampleArgs{users, user_pool, train_indptr, train_indices, train_slots, pop_matrix, pos, neg, pos_pop, neg_pop, seed,
                                            0, B, n_pool, gen_users, neg_lo, neg_hi, n_slots, step_dev, step_next}, alias, 0, stream);
}

extern "C" int pda_negpop_sample_batches_dev(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, int n_batches,
                                             const int64_t* train_indptr, const int32_t* train_indices, const int32_t* train_slots, int neg_lo,
                                             int neg_hi, const uint64_t* alias, const float* pop_matrix, int n_slots, uint64_t seed,
                                             const uint64_t* step_dev, uint64_t* step_next, int32_t* pos, int32_t* neg, float* pos_pop,
                                             float* neg_pop, void* stream) {
    if (n_batches <= 0 || n_batches > 65535) return PDA_ERR_ARG;
    return negpop_triplets(true, SampleArgs{users, user_pool, train_indptr, train_indices, train_slots, pop_matrix, pos, neg, pos_pop, neg_pop, seed,
                                            0, B, n_pool, gen_users, neg_lo, neg_hi, n_slots, step_dev, step_next}, alias, n_batches, stream);
}

extern "C" int pda_negpop_ssm_sample(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, int N,
                                     const int64_t* train_indptr, const int32_t* train_indices, int neg_lo, int neg_hi, const uint64_t* alias,
                                     uint64_t seed, uint64_t step, int32_t* pos, int32_t* negs, void* stream) {
    return negpop_block(false, SsmSampleArgs{users, user_pool, train_indptr, train_indices, pos, negs, seed, step, B, N, n_pool, gen_users, neg_lo,
                                             neg_hi, nullptr, nullptr}, alias, stream);
}

extern "C" int pda_negpop_ssm_sample_dev(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, int N,
                                         const int64_t* train_indptr, const int32_t* train_indices, int neg_lo, int neg_hi, const uint64_t* alias,
                                         uint64_t seed, const uint64_t* step_dev, uint64_t* step_next, int32_t* pos, int32_t* negs, void* stream) {
    return negpop_block(true, SsmSampleArgs{users, user_pool, train_indptr, train_indices, pos, negs, seed, 0, B, N, n_pool, gen_users, neg_lo,
                                            neg_hi, step_dev, step_next}, alias, stream);
}
