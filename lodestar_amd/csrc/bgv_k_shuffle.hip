// Epoch shuffling on the device (gfx950, bgv_shuffling_put): the swap-or-not digests of every
// round, one walk per output position into the committee index pool, and the directory entries
// of the epoch's committees.  The arithmetic is bgv_shuffle.h's (shared with the CPU simulator).
#include "bgv_layout.h"
#include "bgv_shuffle.h"
#include "bgv_launch.h"

extern "C" {

// One thread per digest (round, block of 256 positions) and, after those, one per round's pivot:
// rounds * (ceil(n / 256) + 1) single-block SHA-256 compressions, each thread storing its 32
// bytes (consecutive threads write consecutive 32-byte records).
__global__ void __launch_bounds__(256) k_shuffle_table(shuf_seed seed, uint32_t n, uint32_t rounds,
                                                       uint32_t* __restrict__ table, uint32_t* __restrict__ pivots) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  shuf_table_item(t, seed, n, rounds, table, pivots);
}

// One thread per output position i: p = compute_shuffled_index(i) over the rounds in order (the
// pivots in LDS, per round one dependent 4-byte gather from the round's digests, which L2 holds:
// 128 KB per round at 2^20 positions), then one gather active[p], written to the pool.  No
// atomics, no cross-lane traffic; consecutive lanes write consecutive words.
__global__ void __launch_bounds__(256) k_shuffle_walk(const uint32_t* __restrict__ table,
                                                      const uint32_t* __restrict__ pivots, uint32_t n, uint32_t rounds,
                                                      const uint32_t* __restrict__ active, uint32_t* __restrict__ out) {
  __shared__ uint32_t piv[BGV_SHUFFLE_MAX_ROUNDS + 1];
  if (threadIdx.x < rounds) piv[threadIdx.x] = pivots[threadIdx.x];  // rounds <= 255 < blockDim.x
  __syncthreads();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = active[shuf_walk(i, n, rounds, table, piv)];
}

// {off, n} of the nh non-empty committees of the shuffling at pool[base ..), the j-th one into the
// directory entry handles[j]; k_committee_total then sums them.
__global__ void __launch_bounds__(256) k_shuffle_dir(bgv_dcommittee* __restrict__ dir,
                                                     const uint32_t* __restrict__ handles, uint32_t nh, uint32_t base,
                                                     uint32_t n, uint32_t count) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nh) return;
  uint32_t lo, hi;
  shuf_nonempty_k(n, count, j, &lo, &hi);
  bgv_dcommittee* cm = dir + handles[j];
  cm->off = base + lo;
  cm->n = hi - lo;
}

}  // extern "C"

size_t bgv_shuffle_scratch_words(uint32_t n, uint32_t rounds) {
  return (size_t)n + (size_t)shuf_table_words(n, rounds) + rounds;
}

// scratch: n words of active indices (already there), then the table, then the pivots
hipError_t bgv_launch_shuffle(const uint8_t seed[32], uint32_t n, uint32_t rounds, uint32_t* scratch, uint32_t* out,
                              hipStream_t st) {
  const uint32_t* active = scratch;
  uint32_t* table = scratch + n;
  uint32_t* pivots = table + shuf_table_words(n, rounds);
  if (n < 2) rounds = 0;  // a list of one stays as it is (and has no pivot: mod 1)
  if (rounds) {
    const uint32_t items = rounds * (shuf_nblk(n) + 1u);
    hipLaunchKernelGGL(k_shuffle_table, dim3((items + 255u) / 256u), dim3(256), 0, st, shuf_seed_load(seed), n, rounds,
                       table, pivots);
  }
  hipLaunchKernelGGL(k_shuffle_walk, dim3((n + 255u) / 256u), dim3(256), 0, st, table, pivots, n, rounds, active, out);
  return hipGetLastError();
}

hipError_t bgv_launch_shuffle_dir(bgv_dcommittee* dir, const uint32_t* handles, uint32_t nh, uint32_t base, uint32_t n,
                                  uint32_t count, hipStream_t st) {
  if (nh == 0) return hipSuccess;
  hipLaunchKernelGGL(k_shuffle_dir, dim3((nh + 255u) / 256u), dim3(256), 0, st, dir, handles, nh, base, n, count);
  return hipGetLastError();
}
