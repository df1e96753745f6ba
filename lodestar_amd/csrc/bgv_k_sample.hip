// Balance-weighted sampling on the device (gfx950; bgv_proposers, bgv_sync_committee_put): the
// candidates of a window evaluated one per thread, then compacted in order into each seed's
// picks.  The arithmetic is bgv_sample.h's (shared with the CPU simulator).
#include "bgv_sample.h"
#include "bgv_launch.h"

// One thread per (seed, candidate) of a window: block (x, y) takes candidates next + 256 x ..
// + 255 of seed todo[y].  The block first fills LDS with the seed's pivots (one digest per thread
// t < rounds) and the digests its 256 draws come from (the last threads: 8 digests of 32 random
// bytes under the byte rule, 16 digests of 16 two-byte values under the 16-bit rule).  Each thread
// then walks the rounds with NO digest table: per round it hashes the one block digest its
// position needs and tests one bit.  k_shuffle_table's table costs rounds * n / 256 digests per
// seed -- 369 k at 2^20 indices, and an epoch's proposers would need 32 of them -- where the
// direct walk costs `rounds` digests per candidate, and a seed needs about `want` candidates
// over its acceptance rate: about 1 for a proposer, about 520 for a mainnet sync committee under
// the byte rule, about 32,768 under the 16-bit rule with every balance at 32 of 2048.  Every lane
// runs the same number of rounds, so there is no divergence.  Writes v_i and the accept flag of
// each candidate (consecutive lanes, consecutive words / bytes).
template <class R>
__device__ __forceinline__ void sample_eval(const shuf_seed* __restrict__ seeds, const uint32_t* __restrict__ todo,
                                            const samp_state* __restrict__ state, const uint32_t* __restrict__ active,
                                            uint32_t n, const typename R::eff_t* __restrict__ eff, uint32_t max_incr,
                                            uint32_t rounds, uint32_t limit, uint32_t window,
                                            uint32_t* __restrict__ vals, uint8_t* __restrict__ flags) {
  __shared__ uint32_t piv[BGV_SAMPLE_BLOCK];
  __shared__ uint32_t rnd[samp_rand_digests<R>() * 8u];
  const uint32_t t = threadIdx.x, s = todo[blockIdx.y];
  const shuf_seed seed = seeds[s];
  const uint32_t base = state[s].next + blockIdx.x * BGV_SAMPLE_BLOCK;
  samp_setup_item_r<R>(t, seed, n, rounds, base, piv, rnd);
  __syncthreads();
  uint32_t v;
  const bool ok = samp_eval_item_r<R>(t, seed, n, rounds, base, limit, piv, rnd, active, eff, max_incr, &v);
  const size_t at = (size_t)blockIdx.y * window + blockIdx.x * BGV_SAMPLE_BLOCK + t;
  vals[at] = v;
  flags[at] = ok ? 1 : 0;
}

extern "C" {

__global__ void __launch_bounds__(BGV_SAMPLE_BLOCK)
    k_sample_eval(const shuf_seed* __restrict__ seeds, const uint32_t* __restrict__ todo,
                  const samp_state* __restrict__ state, const uint32_t* __restrict__ active, uint32_t n,
                  const uint8_t* __restrict__ eff, uint32_t max_incr, uint32_t rounds, uint32_t limit, uint32_t window,
                  uint32_t* __restrict__ vals, uint8_t* __restrict__ flags) {
  sample_eval<samp_rule8>(seeds, todo, state, active, n, eff, max_incr, rounds, limit, window, vals, flags);
}

// The same grid under the 16-bit rule: uint16_t balances, 16 digests of draws per block.
__global__ void __launch_bounds__(BGV_SAMPLE_BLOCK)
    k_sample_eval16(const shuf_seed* __restrict__ seeds, const uint32_t* __restrict__ todo,
                    const samp_state* __restrict__ state, const uint32_t* __restrict__ active, uint32_t n,
                    const uint16_t* __restrict__ eff, uint32_t max_incr, uint32_t rounds, uint32_t limit,
                    uint32_t window, uint32_t* __restrict__ vals, uint8_t* __restrict__ flags) {
  sample_eval<samp_rule16>(seeds, todo, state, active, n, eff, max_incr, rounds, limit, window, vals, flags);
}

// One block per seed of the pass, over the window just evaluated: ordered compaction of the
// accepted candidates behind the seed's picks, 256 candidates at a time -- a ballot (64 bits) and
// a popcount of the lower lanes inside a wave, the waves' counts through LDS across waves, no
// atomics.  Picks past `want` are dropped.  window / 256 steps whatever the flags say; then the
// seed's count and next candidate number are stored for a further pass.
__global__ void __launch_bounds__(BGV_SAMPLE_BLOCK)
    k_sample_pick(const uint32_t* __restrict__ todo, samp_state* __restrict__ state, const uint32_t* __restrict__ vals,
                  const uint8_t* __restrict__ flags, uint32_t window, uint32_t count, uint32_t* __restrict__ picks,
                  uint32_t want) {
  constexpr uint32_t NW = BGV_SAMPLE_BLOCK / BGV_SAMPLE_WAVE;
  __shared__ uint32_t wcnt[2][NW];  // two sets: one barrier per step
  const uint32_t t = threadIdx.x, lane = t % BGV_SAMPLE_WAVE, wave = t / BGV_SAMPLE_WAVE, s = todo[blockIdx.x];
  const size_t row = (size_t)blockIdx.x * window;
  uint32_t have = state[s].have;
  for (uint32_t c = 0; c < window / BGV_SAMPLE_BLOCK; ++c) {
    const uint32_t j = c * BGV_SAMPLE_BLOCK + t;
    const bool f = j < count && flags[row + j];
    const uint64_t ballot = __ballot(f);
    if (lane == 0) wcnt[c & 1u][wave] = (uint32_t)__builtin_popcountll(ballot);
    __syncthreads();
    uint32_t before = have, total = 0;
    for (uint32_t w = 0; w < NW; ++w) {
      const uint32_t k = wcnt[c & 1u][w];
      before += w < wave ? k : 0u;
      total += k;
    }
    const uint32_t dst = samp_pick_dst(ballot, lane, before, want);
    if (dst < want) picks[(size_t)s * want + dst] = vals[row + j];
    have = have + total < want ? have + total : want;
  }
  if (t == 0) {
    state[s].have = have;
    state[s].next += count;
  }
}

}  // extern "C"

// One pass for the n_todo seeds of todo (device words): vals / flags hold n_todo * window results.
hipError_t bgv_launch_sample_pass(const bgv_sample_in& in, const uint32_t* todo, uint32_t n_todo, uint32_t window,
                                  uint32_t count, uint32_t* vals, uint8_t* flags, hipStream_t st) {
  if (n_todo == 0 || window == 0) return hipSuccess;
  const dim3 grid(window / BGV_SAMPLE_BLOCK, n_todo);
  if (in.rule == SAMP_RULE_U16)
    hipLaunchKernelGGL(k_sample_eval16, grid, dim3(BGV_SAMPLE_BLOCK), 0, st, in.seeds, todo, in.state, in.active, in.n,
                       (const uint16_t*)in.eff, in.max_incr, in.rounds, in.limit, window, vals, flags);
  else
    hipLaunchKernelGGL(k_sample_eval, grid, dim3(BGV_SAMPLE_BLOCK), 0, st, in.seeds, todo, in.state, in.active, in.n,
                       (const uint8_t*)in.eff, in.max_incr, in.rounds, in.limit, window, vals, flags);
  hipLaunchKernelGGL(k_sample_pick, dim3(n_todo), dim3(BGV_SAMPLE_BLOCK), 0, st, todo, in.state, vals, flags, window,
                     count, in.picks, in.want);
  return hipGetLastError();
}
