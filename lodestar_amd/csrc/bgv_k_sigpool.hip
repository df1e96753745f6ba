// Device-resident signature pools (gfx950): the running G2 aggregate per pool entry, kept in
// Jacobian form on the device.  The signatures a verify call accepted are decoded by
// bgv_k_sigagg.hip's kernels as they are (bgv_launch_sigagg_decode); here
//   k_sigpool_acc  one wavefront per touched entry adds the call's decoded members to the stored
//                  accumulator: strided partial sums and an LDS tree as in k_sigagg_sum, and no
//                  inversion or compression -- the sum stays Jacobian until somebody asks
//   k_sigpool_get  one wavefront per requested entry: k_sigagg_sum's tail (the affine form with
//                  the inversion on the whole wave, lane 0 compresses), the same field values as
//                  bgv_aggregate_signatures' and so the same bytes
//   k_sigpool_sum  one wavefront per group of up to 64 entries (bgv_sigpool_sum): lane j loads
//                  entry j's accumulator, then k_sigpool_acc's tree and k_sigpool_get's tail; no
//                  entry is written
#include "bgv_device.h"
#include "bgv_wfp.h"

extern "C" {

// ids/first/count/fresh: one per touched entry (ids below BGV_MAX_SIGPOOL, the host's check; the
// members within the n decoded points).  flag[e] receives 0, or the status of the entry's first
// member that did not decode; the slot is written only in the first case.
__global__ void __launch_bounds__(64) k_sigpool_acc(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ first,
                                                    const uint32_t* __restrict__ count,
                                                    const uint32_t* __restrict__ fresh, const g2_jac* __restrict__ pts,
                                                    const int32_t* __restrict__ status, g2_jac* __restrict__ acc,
                                                    int32_t* __restrict__ flag) {
  extern __shared__ uint32_t lds[];
  g2_jac* ls = reinterpret_cast<g2_jac*>(lds);
  const uint32_t e = blockIdx.x, j = threadIdx.x, f = first[e], n = count[e];
  // decided before the write: the first member (in member order) whose status is not 0.  Its
  // position goes through the first word of the tree's LDS (no static LDS: that would move the
  // dynamic region off its 16-byte alignment)
  if (j == 0) lds[0] = 0xFFFFFFFFu;
  __syncthreads();
  for (uint32_t k = j; k < n; k += BGV_WAVE)
    if (status[f + k] != BGV_OK) {
      atomicMin(&lds[0], k);
      break;
    }
  __syncthreads();
  const uint32_t bad = lds[0];  // the whole block takes the same path
  __syncthreads();              // read by every lane before the tree reuses the word
  if (bad != 0xFFFFFFFFu) {
    if (j == 0) flag[e] = status[f + bad];
    return;
  }
  g2_jac* slot = acc + ids[e];
  g2_jac sum = (j == 0 && !fresh[e]) ? *slot : jac_infinity<fp2_t>();
  for (uint32_t k = j; k < n; k += BGV_WAVE) sum = jac_add(sum, pts[f + k]);
  for (uint32_t d = 1; d < BGV_WAVE; d <<= 1) {
    ls[j] = sum;
    __syncthreads();
    if ((j & (2 * d - 1)) == 0) sum = jac_add(sum, ls[j + d]);
    __syncthreads();
  }
  if (j == 0) {
    *slot = sum;
    flag[e] = BGV_OK;
  }
}

// ids: n entries that have been written (the host answers for the others itself)
__global__ void __launch_bounds__(64) k_sigpool_get(const uint32_t* __restrict__ ids, uint32_t n,
                                                    const g2_jac* __restrict__ acc, uint8_t* __restrict__ out96) {
  const uint32_t a = blockIdx.x, j = threadIdx.x;
  if (a >= n) return;  // grid.x = n; the whole wave takes the same path
  // jac_to_aff on the whole wave: every lane takes the accumulator, and the inversion's
  // exponentiation runs one limb per lane (k_sigagg_sum's tail)
  const g2_jac p = acc[ids[a]];
  const fp_t ni = wfp_pow_fixed<BGV_POW_INV>(fp_add(fp_sqr(p.z.c0), fp_sqr(p.z.c1)));
  const fp2_t zi = {fp_mul(p.z.c0, ni), fp_neg(fp_mul(p.z.c1, ni))};
  const fp2_t zi2 = fp2_sqr(zi);
  const g2_aff r = {fp2_mul(p.x, zi2), fp2_mul(p.y, fp2_mul(zi2, zi))};
  if (j == 0) {
    uint8_t b[96];
    g2_compress(b, r, jac_is_inf(p));
    for (int q = 0; q < 96; ++q) out96[96ull * a + q] = b[q];
  }
}

// One wavefront per group g: the sum of acc[ids[first[g] + j]], j < count[g] (1 .. BGV_WAVE entries,
// every one written: the host's check).  Lane j takes entry j, the other lanes infinity; then
// k_sigpool_acc's tree and k_sigpool_get's tail.  288 B read per entry, 96 B written per group.
__global__ void __launch_bounds__(64) k_sigpool_sum(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ first,
                                                    const uint32_t* __restrict__ count, uint32_t ngroups,
                                                    const g2_jac* __restrict__ acc, uint8_t* __restrict__ out96) {
  extern __shared__ uint32_t lds[];
  g2_jac* ls = reinterpret_cast<g2_jac*>(lds);
  const uint32_t g = blockIdx.x, j = threadIdx.x;
  if (g >= ngroups) return;  // grid.x = ngroups; the whole wave takes the same path
  const uint32_t f = first[g], n = count[g];
  g2_jac sum = j < n ? acc[ids[f + j]] : jac_infinity<fp2_t>();
  for (uint32_t d = 1; d < BGV_WAVE; d <<= 1) {
    ls[j] = sum;
    __syncthreads();
    if ((j & (2 * d - 1)) == 0) sum = jac_add(sum, ls[j + d]);
    __syncthreads();
  }
  if (j == 0) ls[0] = sum;
  __syncthreads();
  sum = ls[0];
  const fp_t ni = wfp_pow_fixed<BGV_POW_INV>(fp_add(fp_sqr(sum.z.c0), fp_sqr(sum.z.c1)));
  const fp2_t zi = {fp_mul(sum.z.c0, ni), fp_neg(fp_mul(sum.z.c1, ni))};
  const fp2_t zi2 = fp2_sqr(zi);
  const g2_aff r = {fp2_mul(sum.x, zi2), fp2_mul(sum.y, fp2_mul(zi2, zi))};
  if (j == 0) {
    uint8_t b[96];
    g2_compress(b, r, jac_is_inf(sum));
    for (int q = 0; q < 96; ++q) out96[96ull * g + q] = b[q];
  }
}

}  // extern "C"

hipError_t bgv_launch_sigpool_sum(const uint32_t* ids, const uint32_t* first, const uint32_t* count, uint32_t ngroups,
                                  const void* acc, uint8_t* out96, hipStream_t st) {
  if (ngroups)
    hipLaunchKernelGGL(k_sigpool_sum, dim3(ngroups), dim3(BGV_WAVE), BGV_WAVE * sizeof(g2_jac), st, ids, first, count,
                       ngroups, reinterpret_cast<const g2_jac*>(acc), out96);
  return hipGetLastError();
}

hipError_t bgv_launch_sigpool_acc(const uint32_t* ids, const uint32_t* first, const uint32_t* count,
                                  const uint32_t* fresh, uint32_t nentries, const void* pts, const int32_t* status,
                                  void* acc, int32_t* flag, hipStream_t st) {
  if (nentries)
    hipLaunchKernelGGL(k_sigpool_acc, dim3(nentries), dim3(BGV_WAVE), BGV_WAVE * sizeof(g2_jac), st, ids, first, count,
                       fresh, reinterpret_cast<const g2_jac*>(pts), status, reinterpret_cast<g2_jac*>(acc), flag);
  return hipGetLastError();
}

hipError_t bgv_launch_sigpool_get(const uint32_t* ids, uint32_t n, const void* acc, uint8_t* out96, hipStream_t st) {
  if (n)
    hipLaunchKernelGGL(k_sigpool_get, dim3(n), dim3(BGV_WAVE), 0, st, ids, n, reinterpret_cast<const g2_jac*>(acc),
                       out96);
  return hipGetLastError();
}
