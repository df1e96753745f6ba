// bgv_verify_aggregate's aggregation step (gfx950): the signatures a verify call accepted,
// decompressed a second time and summed per aggregate.  task_sig has proved an accepted
// signature's membership of G2, so decoding here is the decompression alone (the Fp2 square
// root); there is no subgroup check.  Two decoding forms, chosen by the host plan
// (bgv_sigagg_plan.h):
//   k_sigagg_decode_wave  one signature per wavefront: every lane holds the same values and the
//                         square root's two exponentiations run one limb per lane (bgv_pow_wave,
//                         as k_prep_a_wave's signature plane; the few products around them stay
//                         on the lanes, this unit's fp_mul being the one-lane product the sum
//                         kernel needs) -- for calls on the latency path
//   k_sigagg_decode_lane  one signature per lane (bgv_pow_lane) -- for larger calls
// Both write g2_jac points in member order; k_sigagg_sum is k_sig_sum's scheme (bgv_k_util.hip:
// each unit compiles its own copy): one wavefront per aggregate, strided partial sums, an LDS
// tree, then the affine form with the inversion on the whole wave; lane 0 compresses.
#include "bgv_device.h"
#include "bgv_wfp.h"

// status BGV_OK with the point (infinity for the infinity encoding), or the decoding's code
template <class PW>
__device__ __forceinline__ int32_t sigagg_decode(const uint8_t* __restrict__ sig, g2_jac* out) {
  uint8_t b[96];
  for (int q = 0; q < 96; ++q) b[q] = sig[q];
  g2_aff a;
  bool inf;
  const int32_t st = g2_decompress_t<PW>(&a, &inf, b);
  *out = (st == BGV_OK && !inf) ? jac_from_aff(a) : jac_infinity<fp2_t>();
  return st;
}

extern "C" {

__global__ void __launch_bounds__(64) k_sigagg_decode_wave(const uint8_t* __restrict__ sigs96, uint32_t n,
                                                           g2_jac* __restrict__ pts, int32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x;  // grid.x = n; the whole wave takes the same path
  if (i >= n) return;
  g2_jac p;
  const int32_t st = sigagg_decode<bgv_pow_wave>(sigs96 + 96ull * i, &p);
  if (threadIdx.x == 0) {
    pts[i] = p;
    status[i] = st;
  }
}

__global__ void BGV_KATTR k_sigagg_decode_lane(const uint8_t* __restrict__ sigs96, uint32_t n,
                                               g2_jac* __restrict__ pts, int32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * BGV_WAVE + threadIdx.x;
  if (i >= n) return;
  g2_jac p;
  const int32_t st = sigagg_decode<bgv_pow_lane>(sigs96 + 96ull * i, &p);
  pts[i] = p;
  status[i] = st;
}

__global__ void BGV_KATTR k_sigagg_sum(const uint32_t* __restrict__ first, const uint32_t* __restrict__ count,
                                       const g2_jac* __restrict__ pts, uint8_t* __restrict__ out96) {
  extern __shared__ uint32_t lds[];
  g2_jac* ls = reinterpret_cast<g2_jac*>(lds);
  const uint32_t a = blockIdx.x, j = threadIdx.x, f = first[a], n = count[a];
  if (n == 0) return;  // the whole block: the host reports an empty aggregate and zero bytes
  g2_jac acc = jac_infinity<fp2_t>();
  for (uint32_t k = j; k < n; k += BGV_WAVE) acc = jac_add(acc, pts[f + k]);
  for (uint32_t d = 1; d < BGV_WAVE; d <<= 1) {
    ls[j] = acc;
    __syncthreads();
    if ((j & (2 * d - 1)) == 0) acc = jac_add(acc, ls[j + d]);
    __syncthreads();
  }
  // jac_to_aff on the whole wave: every lane takes lane 0's sum, and the inversion's
  // exponentiation runs one limb per lane (the same field values, so the same bytes)
  if (j == 0) ls[0] = acc;
  __syncthreads();
  acc = ls[0];
  const fp_t ni = wfp_pow_fixed<BGV_POW_INV>(fp_add(fp_sqr(acc.z.c0), fp_sqr(acc.z.c1)));
  const fp2_t zi = {fp_mul(acc.z.c0, ni), fp_neg(fp_mul(acc.z.c1, ni))};
  const fp2_t zi2 = fp2_sqr(zi);
  const g2_aff r = {fp2_mul(acc.x, zi2), fp2_mul(acc.y, fp2_mul(zi2, zi))};
  if (j == 0) {
    uint8_t b[96];
    g2_compress(b, r, jac_is_inf(acc));
    for (int q = 0; q < 96; ++q) out96[96ull * a + q] = b[q];
  }
}

}  // extern "C"

// the decoding alone (bgv_sigpool.cpp: the pool's accumulation step sums the points itself)
hipError_t bgv_launch_sigagg_decode(const uint8_t* sigs96, uint32_t n, bool wave, void* pts, int32_t* status,
                                    hipStream_t st) {
  g2_jac* p = reinterpret_cast<g2_jac*>(pts);
  if (n && wave)
    hipLaunchKernelGGL(k_sigagg_decode_wave, dim3(n), dim3(BGV_WAVE), 0, st, sigs96, n, p, status);
  else if (n)
    hipLaunchKernelGGL(k_sigagg_decode_lane, dim3(nblk(n, BGV_WAVE)), dim3(BGV_WAVE), 0, st, sigs96, n, p, status);
  return hipGetLastError();
}

hipError_t bgv_launch_sigagg(const uint8_t* sigs96, uint32_t n, bool wave, const uint32_t* first,
                             const uint32_t* count, uint32_t naggs, void* pts, int32_t* status, uint8_t* out96,
                             hipStream_t st) {
  g2_jac* p = reinterpret_cast<g2_jac*>(pts);
  if (n && wave)
    hipLaunchKernelGGL(k_sigagg_decode_wave, dim3(n), dim3(BGV_WAVE), 0, st, sigs96, n, p, status);
  else if (n)
    hipLaunchKernelGGL(k_sigagg_decode_lane, dim3(nblk(n, BGV_WAVE)), dim3(BGV_WAVE), 0, st, sigs96, n, p, status);
  if (naggs) hipLaunchKernelGGL(k_sigagg_sum, dim3(naggs), dim3(BGV_WAVE), BGV_WAVE * sizeof(g2_jac), st, first, count, p,
                       out96);
  return hipGetLastError();
}
