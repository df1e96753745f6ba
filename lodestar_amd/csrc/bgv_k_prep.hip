// Per-set preparation kernels (gfx950) other than the bulk k_prep (bgv_k_prep_bulk.hip);
// see bgv_sched.cpp for the launch order of a verify call and bgv_k_miller.hip /
// bgv_k_final.hip for the rest.
//
//   k_pk_agg16 / k_pk_agg  (only when a call holds a set with >= BGV_PK_TREE_MIN cached
//              keys) a team of 16 lanes per committee-sized set, a whole wavefront per set
//              above BGV_PK_TEAM_MAX keys, sums its keys with a ds_swizzle/ds_bpermute tree
//   k_pk_agg_bits  (only when a call holds committee-bitfield sets, BGV_SLOT_PK_COMMITTEE) the
//              selected members of a device-resident committee, or the unselected ones subtracted
//              from its total, on a 16-lane team or a whole wave per set (bgv_pk_bits.h)
//   k_pk_agg_span  (only when a call holds span sets, BGV_SLOT_PK_SPAN) the same for one bitfield
//              laid over several committees: every committee's shorter side and the totals of
//              the complement ones as ONE term list, walked by rank on a team or a wave per set
//   k_prep_a / k_prep_team   the latency path for small calls (bgv_latency_max): the same
//              work over two launches with more lanes per set, so the longest chain per
//              lane roughly halves: (a) one SSWU map + isogeny per lane for u0 and u1, the
//              signature's decompression, the pubkey task; (team) the cofactor clearing of
//              q0 + q1 and r_i * sig_i on 16-lane teams, the subgroup check on one lane
//   k_prep     (bgv_k_prep_bulk.hip) sig, hash and pk tasks side by side for larger calls
#include "bgv_k_lat.h"
#include "bgv_pk_bits.h"
#include "bgv_team_dev.h"
#include "bgv_tcurve.h"
#include "bgv_tg1.h"
#include "bgv_tround_dev.h"

static __constant__ uint8_t kTcProg[TCP_TABLE_BYTES] = TCP_TABLE_INIT;
static __constant__ uint8_t kTg1Prog[TG1_TABLE_BYTES] = TG1_TABLE_INIT;

// Device engine of the team G2 schedules (bgv_tcurve.h): programs over the team's LDS slots
// with a block barrier per round; every team of the block runs the same sequence.
struct tc_dev_engine {
  const uint8_t* prog;
  fp_t* S;
  int c;
  bool bad;
  __device__ void run(int off) {
    int pos = off;
    const int nr = prog[pos++];
    for (int r = 0; r < nr; ++r) {
      const int T = prog[pos], M = prog[pos + 1];
      pos += 2;
      const int rb = tmp_rec_bytes(T, M);
      int out;
      const fp_t v = tmp_lane_any(S, prog + pos + c * rb, T, M, &out);
      S[out] = v;  // no slot is read and written in one round (tools/gen_tcurve.py)
      __syncthreads();
      pos += BGV_TEAM * rb;
    }
  }
  __device__ void copy(int dst, int src) {  // src may differ per team (a digit's table entry)
    if (c < 6 && dst != src) S[TCP_BANK(dst) + c] = S[TCP_BANK(src) + c];
    __syncthreads();
  }
  __device__ void neg_y(int b) {
    if (c == 2 || c == 3) S[TCP_BANK(b) + c] = fp_neg(S[TCP_BANK(b) + c]);
    __syncthreads();
  }
  __device__ void check_add() {
    if (c == 0) {
      const auto z2 = [&](int s) { return fp_is_zero(S[s]) && fp_is_zero(S[s + 1]); };
      bad = bad || z2(TC_CHK_A) || z2(TC_CHK_B);
    }
  }
};

#ifndef BGV_WPE_AGG
#define BGV_WPE_AGG 2
#endif

// Committee-bitfield sets (bgv_pk_bits.h).  One team of T lanes (16: four slots per wave, 64: the
// wave) sums the chosen side of one slot: lane l gathers the selected members of rank l, l + T,
// ... (direct mode: bit set; complement mode: bit clear), found from the per-word popcount
// prefix, so every lane of a team does the same number of additions whatever the pattern.  Every
// lane reads the same bit word at a time (one broadcast fetch) and the member table through it;
// each key is gathered one addition ahead of its use.  words == nullptr selects every member
// (the committee's total, k_committee_total).  Then the butterfly inside the team; complement
// mode returns total + (-sum).  The additions are the complete ones (jac_add_aff with its
// doubling branch, jac_add), so members that cancel, an infinity total and an infinity result
// take no special case.  Every lane of the wave must reach the exchanges: an idle team (act
// false) carries infinity through them.
static_assert(sizeof(g1_jac) == sizeof(bgv_dcommittee::total), "bgv_dcommittee keeps a Jacobian G1 point");
template <int T>
__device__ __forceinline__ g1_jac pk_bits_sum(bool act, uint32_t l, const uint32_t* __restrict__ words,
                                              const uint32_t* __restrict__ members, uint32_t n, bool comp,
                                              const g1_aff* __restrict__ cache) {
  g1_jac acc = jac_infinity<fp_t>();
  if (act) {
    pkb_cursor c = pkb_begin(l);
    uint32_t pos;
    if (pkb_next(c, words, n, comp, T, &pos)) {
      acc = jac_from_aff(cache[members[pos]]);
      bool have = pkb_next(c, words, n, comp, T, &pos);
      g1_aff cur = cache[members[have ? pos : 0]];
      while (have) {
        uint32_t pn;
        const bool hn = pkb_next(c, words, n, comp, T, &pn);
        const g1_aff nxt = cache[members[hn ? pn : pos]];
        acc = jac_add_aff(acc, cur);
        cur = nxt;
        pos = hn ? pn : pos;
        have = hn;
      }
    }
  }
  if constexpr (T == 64) {
    acc = jac_add(acc, point_xor<32>(acc));
    acc = jac_add(acc, point_xor<16>(acc));
  }
  acc = jac_add(acc, point_xor<8>(acc));
  acc = jac_add(acc, point_xor<4>(acc));
  acc = jac_add(acc, point_xor<2>(acc));
  acc = jac_add(acc, point_xor<1>(acc));
  return acc;
}

// pk_agg[s] of committee slot s on a team of T lanes (lane l of it); act false: an idle team
template <int T>
__device__ __forceinline__ void pk_bits_slot(bool act, uint32_t s, uint32_t l, const bgv_dslot* __restrict__ slots,
                                             const uint32_t* __restrict__ pk_idx,
                                             const bgv_dcommittee* __restrict__ dir,
                                             const uint32_t* __restrict__ pool, const g1_aff* __restrict__ cache,
                                             g1_jac* __restrict__ pk_agg, bool writer) {
  const uint32_t* words = nullptr;
  const uint32_t* members = nullptr;
  const bgv_dcommittee* cm = nullptr;
  uint32_t n = 0;
  bool comp = false;
  if (act) {
    const bgv_dslot& d = slots[s];
    cm = dir + pk_idx[d.pk_off];
    words = pk_idx + d.pk_off + 1;
    members = pool + cm->off;
    n = cm->n;
    comp = (d.flags & BGV_SLOT_PK_COMPLEMENT) != 0;
  }
  g1_jac acc = pk_bits_sum<T>(act, l, words, members, n, comp, cache);
  if (act && writer) {
    if (comp) acc = jac_add(*reinterpret_cast<const g1_jac*>(cm->total), jac_neg(acc));
    pk_agg[s] = acc;
  }
}

// Span sets (BGV_SLOT_PK_SPAN; bgv_pk_bits.h): one bitfield over several committees.  The same
// walk over the span's whole term list: lane l of a team of T takes the terms of rank l, l + T,
// ..., so its number of additions is ceil((M - l) / T) however the bits fall across the
// committees.  The member terms come first, record by record -- every lane reads the same record
// at a time, the key through the record's committee, negated where that committee is on the
// complement side, and gathered one addition ahead of its use -- then the totals of the
// complement committees, which are Jacobian and take jac_add.  All additions are the complete
// ones, so cancelling members, an infinity total and an infinity result take no special case.
__device__ __forceinline__ g1_aff pk_span_key(uint32_t meta, uint32_t pos, const bgv_dcommittee* __restrict__ dir,
                                              const uint32_t* __restrict__ pool, const g1_aff* __restrict__ cache) {
  g1_aff a = cache[pool[dir[pkb_meta_handle(meta)].off + pos]];
  if (pkb_meta_complement(meta)) a.y = fp_neg(a.y);
  return a;
}
template <int T>
__device__ __forceinline__ g1_jac pk_span_sum(bool act, uint32_t l, const uint32_t* __restrict__ run,
                                              const bgv_dcommittee* __restrict__ dir,
                                              const uint32_t* __restrict__ pool, const g1_aff* __restrict__ cache) {
  g1_jac acc = jac_infinity<fp_t>();
  if (act) {
    const uint32_t nrec = run[0], ncomp = run[1];
    const uint32_t* tot = run + PKB_SPAN_HEAD;
    const uint32_t* recs = tot + ncomp;
    pkb_span_cursor c = pkb_span_begin(l);
    uint32_t meta, pos;
    if (pkb_span_next(c, recs, nrec, T, &meta, &pos)) {
      acc = jac_from_aff(pk_span_key(meta, pos, dir, pool, cache));
      bool have = pkb_span_next(c, recs, nrec, T, &meta, &pos);
      g1_aff cur = {acc.x, acc.y};  // never added unless replaced
      if (have) cur = pk_span_key(meta, pos, dir, pool, cache);
      while (have) {
        const bool hn = pkb_span_next(c, recs, nrec, T, &meta, &pos);
        g1_aff nxt = cur;
        if (hn) nxt = pk_span_key(meta, pos, dir, pool, cache);
        acc = jac_add_aff(acc, cur);
        cur = nxt;
        have = hn;
      }
    }
    // the walk ended at c.base = the number of member terms: the lane's totals
    uint32_t t = c.want - c.base;
    if (t < ncomp) {
      g1_jac cur = *reinterpret_cast<const g1_jac*>(dir[tot[t]].total);
      for (t += T; t < ncomp; t += T) {
        const g1_jac nxt = *reinterpret_cast<const g1_jac*>(dir[tot[t]].total);
        acc = jac_add(acc, cur);
        cur = nxt;
      }
      acc = jac_add(acc, cur);
    }
  }
  if constexpr (T == 64) {
    acc = jac_add(acc, point_xor<32>(acc));
    acc = jac_add(acc, point_xor<16>(acc));
  }
  acc = jac_add(acc, point_xor<8>(acc));
  acc = jac_add(acc, point_xor<4>(acc));
  acc = jac_add(acc, point_xor<2>(acc));
  acc = jac_add(acc, point_xor<1>(acc));
  return acc;
}

// pk_agg[s] of span slot s on a 16-lane team (team true: four slots per block, lane % 16 of
// team lane / 16) or on the whole wave; act false: an idle team.  Out of line: the kernels that
// call it keep the code and the registers of their own bodies.
__device__ __noinline__ void pk_span_slot(bool team, bool act, uint32_t s, const bgv_dslot* __restrict__ slots,
                                          const uint32_t* __restrict__ pk_idx, const bgv_dcommittee* __restrict__ dir,
                                          const uint32_t* __restrict__ pool, const g1_aff* __restrict__ cache,
                                          g1_jac* __restrict__ pk_agg, bool writer) {
  const uint32_t* run = act ? pk_idx + slots[s].pk_off : nullptr;
  const g1_jac acc = team ? pk_span_sum<16>(act, threadIdx.x % 16, run, dir, pool, cache)
                          : pk_span_sum<64>(act, threadIdx.x, run, dir, pool, cache);
  if (act && writer) pk_agg[s] = acc;
}

extern "C" {

// Pubkey aggregation of many-key sets as a wavefront tree (one wave per slot): lane l
// sums the set's cached keys l, l + 64, ... with mixed additions (coalesced gathers),
// then six butterfly levels of complete Jacobian additions with the partner lane's
// partial sum (lane ^ 32, 16, ..., 1) exchanged in registers.  Every lane ends with the
// total; the sum is the same group element as the serial one.  Waves of slots with fewer
// than BGV_PK_TREE_MIN cached keys exit at once (uniformly: every lane reads the same slot).
__device__ __forceinline__ void pk_aggw_body(const bgv_dslot* __restrict__ slots, uint32_t s,
                                             const uint32_t* __restrict__ pk_idx, const g1_aff* __restrict__ cache,
                                             g1_jac* __restrict__ pk_agg) {
  const bgv_dslot& d = slots[s];
  if ((d.flags & BGV_SLOT_PAD) || !(d.flags & BGV_SLOT_PK_CACHED) || d.n_pk <= BGV_PK_TEAM_MAX) return;
  const uint32_t l = threadIdx.x;
  g1_jac acc = jac_infinity<fp_t>();
  for (uint32_t k = l; k < d.n_pk; k += 64) acc = jac_add_aff(acc, cache[pk_idx[d.pk_off + k]]);
  acc = jac_add(acc, point_xor<32>(acc));
  acc = jac_add(acc, point_xor<16>(acc));
  acc = jac_add(acc, point_xor<8>(acc));
  acc = jac_add(acc, point_xor<4>(acc));
  acc = jac_add(acc, point_xor<2>(acc));
  acc = jac_add(acc, point_xor<1>(acc));
  if (l == 0) pk_agg[s] = acc;
}

__device__ __forceinline__ void pk_agg16_body(const bgv_dslot* __restrict__ slots, uint32_t nslots, uint32_t blk,
                                              const uint32_t* __restrict__ pk_idx, const g1_aff* __restrict__ cache,
                                              g1_jac* __restrict__ pk_agg) {
  const uint32_t s = blk * (64 / 16) + threadIdx.x / 16;
  const uint32_t l = threadIdx.x % 16;
  const bgv_dslot* d = s < nslots ? &slots[s] : nullptr;
  const bool act = d && !(d->flags & BGV_SLOT_PAD) && (d->flags & BGV_SLOT_PK_CACHED) &&
                   d->n_pk >= BGV_PK_TREE_MIN && d->n_pk <= BGV_PK_TEAM_MAX;
  g1_jac acc = jac_infinity<fp_t>();
  if (act) {  // n_pk >= 16: every lane has a first key
    const uint32_t* idx = pk_idx + d->pk_off;
    const uint32_t n = d->n_pk;
    acc = jac_from_aff(cache[idx[l]]);
    uint32_t k = l + 16;
    g1_aff cur = cache[idx[k < n ? k : l]];
    for (; k < n; k += 16) {
      const uint32_t kn = k + 16 < n ? k + 16 : k;
      const g1_aff nxt = cache[idx[kn]];
      acc = jac_add_aff(acc, cur);
      cur = nxt;
    }
  }
  // every lane of the wave reaches the exchanges
  acc = jac_add(acc, point_xor<8>(acc));
  acc = jac_add(acc, point_xor<4>(acc));
  acc = jac_add(acc, point_xor<2>(acc));
  acc = jac_add(acc, point_xor<1>(acc));
  if (act && l == 0) pk_agg[s] = acc;
}

// One set's tree sum on a whole 64-lane block with the bulk path's summation order (so the
// same Jacobian representative, hence the same Miller value f): k_pk_agg16's 16-lane team for
// BGV_PK_TREE_MIN..BGV_PK_TEAM_MAX cached keys (lanes 16..63 repeat lanes 0..15), k_pk_agg's
// wave tree above.
__device__ __forceinline__ void pk_agg_one(const bgv_dslot* __restrict__ slots, uint32_t s,
                                           const uint32_t* __restrict__ pk_idx, const g1_aff* __restrict__ cache,
                                           g1_jac* __restrict__ pk_agg) {
  const bgv_dslot& d = slots[s];
  if ((d.flags & BGV_SLOT_PAD) || !(d.flags & BGV_SLOT_PK_CACHED) || d.n_pk < BGV_PK_TREE_MIN) return;
  if (d.n_pk > BGV_PK_TEAM_MAX) {
    pk_aggw_body(slots, s, pk_idx, cache, pk_agg);
    return;
  }
  const uint32_t l = threadIdx.x % 16;
  const uint32_t* idx = pk_idx + d.pk_off;
  const uint32_t n = d.n_pk;
  g1_jac acc = jac_from_aff(cache[idx[l]]);
  for (uint32_t k = l + 16; k < n; k += 16) acc = jac_add_aff(acc, cache[idx[k]]);
  acc = jac_add(acc, point_xor<8>(acc));
  acc = jac_add(acc, point_xor<4>(acc));
  acc = jac_add(acc, point_xor<2>(acc));
  acc = jac_add(acc, point_xor<1>(acc));
  if (threadIdx.x == 0) pk_agg[s] = acc;
}

// com: the batch's committee slots, nteam of them on 16-lane teams (four per block), then nwave
// on a wave each.  One wave per SIMD: the cursor, the prefetched key and the sum fit the
// registers (at two waves per SIMD the compiler spills 354 VGPRs to scratch).
#ifndef BGV_WPE_BITS
#define BGV_WPE_BITS 1
#endif
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BGV_WPE_BITS, BGV_WPE_BITS)))
k_pk_agg_bits(const bgv_dslot* __restrict__ slots, const uint32_t* __restrict__ com, uint32_t nteam, uint32_t nwave,
              const uint32_t* __restrict__ pk_idx, const bgv_dcommittee* __restrict__ dir,
              const uint32_t* __restrict__ pool, const g1_aff* __restrict__ cache, g1_jac* __restrict__ pk_agg) {
  const uint32_t nb_team = (nteam + 3) / 4;
  if (blockIdx.x < nb_team) {
    const uint32_t q = blockIdx.x * 4 + threadIdx.x / 16, l = threadIdx.x % 16;
    const bool act = q < nteam;
    pk_bits_slot<16>(act, act ? com[q] : 0u, l, slots, pk_idx, dir, pool, cache, pk_agg, l == 0);
  } else {
    const uint32_t q = nteam + (blockIdx.x - nb_team);
    const bool act = q < nteam + nwave;
    pk_bits_slot<64>(act, act ? com[q] : 0u, threadIdx.x, slots, pk_idx, dir, pool, cache, pk_agg, threadIdx.x == 0);
  }
}

// One committee slot on a whole 64-lane block (k_prep_wide's pubkey plane), where the block has
// nothing else to do: the shorter chain of additions decides.  A 16-lane team (the four teams
// of the block repeat each other, as pk_agg_one's do) runs ceil(m / 16) + 4 additions per lane
// for m terms, the whole wave ceil(m / 64) + 6: the wave from BGV_PK_ONE_WAVE_MIN terms on
// (m = 49: 8 against 7).  The high-participation sets this path serves have a few terms.  Out of line: k_prep_wide's other planes and its index-set path keep the code they
// had without it.
#define BGV_PK_ONE_WAVE_MIN 49
__device__ __noinline__ void pk_bits_one(const bgv_dslot* __restrict__ slots, uint32_t s,
                                            const uint32_t* __restrict__ pk_idx,
                                            const bgv_dcommittee* __restrict__ dir,
                                            const uint32_t* __restrict__ pool, const g1_aff* __restrict__ cache,
                                            g1_jac* __restrict__ pk_agg) {
  const bgv_dslot& d = slots[s];
  // uniform over the block; a span slot's sum is in pk_agg already (k_pk_agg_span runs ahead of k_prep_wide)
  if ((d.flags & (BGV_SLOT_PAD | BGV_SLOT_PK_SPAN)) || !(d.flags & BGV_SLOT_PK_COMMITTEE)) return;
  const uint32_t n = dir[pk_idx[d.pk_off]].n;
  if (pkb_terms(n, d.n_pk, (d.flags & BGV_SLOT_PK_COMPLEMENT) != 0) < BGV_PK_ONE_WAVE_MIN)
    pk_bits_slot<16>(true, s, threadIdx.x % 16, slots, pk_idx, dir, pool, cache, pk_agg, threadIdx.x == 0);
  else
    pk_bits_slot<64>(true, s, threadIdx.x, slots, pk_idx, dir, pool, cache, pk_agg, threadIdx.x == 0);
}

// k_pk_agg_bits for the batch's span slots (span: nteam of them on 16-lane teams, four per
// block, then nwave on a wave each), with the multi-committee body.  A kernel of its own, so
// k_pk_agg_bits keeps its code and registers; launched only when a batch holds span slots.
// one != 0 (ahead of k_prep_wide, where nothing else waits for a SIMD): a block per slot of the
// list, and the shorter chain decides as in pk_bits_one -- a 16-lane team (the four teams of
// the block repeat each other) below BGV_PK_ONE_WAVE_MIN terms, the whole wave from there on.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BGV_WPE_BITS, BGV_WPE_BITS)))
k_pk_agg_span(const bgv_dslot* __restrict__ slots, const uint32_t* __restrict__ span, uint32_t nteam, uint32_t nwave,
              uint32_t one, const uint32_t* __restrict__ pk_idx, const bgv_dcommittee* __restrict__ dir,
              const uint32_t* __restrict__ pool, const g1_aff* __restrict__ cache, g1_jac* __restrict__ pk_agg) {
  if (one) {
    const bool act = blockIdx.x < nteam + nwave;
    const uint32_t s = act ? span[blockIdx.x] : 0u;
    const bool team = act && pk_idx[slots[s].pk_off + 2] < BGV_PK_ONE_WAVE_MIN;
    pk_span_slot(team, act, s, slots, pk_idx, dir, pool, cache, pk_agg, threadIdx.x == 0);
    return;
  }
  const uint32_t nb_team = (nteam + 3) / 4;
  const bool team = blockIdx.x < nb_team;
  const uint32_t q = team ? blockIdx.x * 4 + threadIdx.x / 16 : nteam + (blockIdx.x - nb_team);
  const bool act = q < (team ? nteam : nteam + nwave);
  pk_span_slot(team, act, act ? span[q] : 0u, slots, pk_idx, dir, pool, cache, pk_agg,
               (team ? threadIdx.x % 16 : threadIdx.x) == 0);
}

// The pubkey sums of the committees listed in handles (one wave each) into their directory
// entries: k_pk_agg_bits' body with every bit set, direct mode (bgv_committee_put, and after a
// bgv_pubkeys_put over members of live committees).
__global__ void __launch_bounds__(64) k_committee_total(bgv_dcommittee* __restrict__ dir,
                                                        const uint32_t* __restrict__ handles, uint32_t nh,
                                                        const uint32_t* __restrict__ pool,
                                                        const g1_aff* __restrict__ cache) {
  if (blockIdx.x >= nh) return;
  bgv_dcommittee* cm = dir + handles[blockIdx.x];
  const g1_jac acc = pk_bits_sum<64>(true, threadIdx.x, nullptr, pool + cm->off, cm->n, false, cache);
  if (threadIdx.x == 0) *reinterpret_cast<g1_jac*>(cm->total) = acc;
}

__global__ void __launch_bounds__(64) k_pk_agg(const bgv_dslot* __restrict__ slots, uint32_t nslots,
                                               const uint32_t* __restrict__ pk_idx,
                                               const g1_aff* __restrict__ cache, g1_jac* __restrict__ pk_agg) {
  if (blockIdx.x < nslots) pk_aggw_body(slots, blockIdx.x, pk_idx, cache, pk_agg);
}

// The latency path's first launch for calls above BGV_PREP_WIDE_MAX sets (the smallest calls
// run k_prep_a_wave, bgv_k_prep_wave.hip): planes 0..2 the maps of u0 / u1 and the signature's
// decoding, one lane per set, plane 3 the pubkey task.
__global__ void BGV_KATTR_PREP k_prep_a(const bgv_dslot* __restrict__ slots, uint32_t nslots, g2_jac* __restrict__ h,
                                        fp12_t* __restrict__ f, int32_t* __restrict__ sig_status,
                                        const uint32_t* __restrict__ pk_idx, const g1_aff* __restrict__ cache,
                                        const uint8_t* __restrict__ pk_bytes, g1_jac* __restrict__ rpk,
                                        int32_t* __restrict__ pk_status, g1_jac* __restrict__ pk_agg) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nslots) return;
  if (blockIdx.y == 0)
    task_map_t<bgv_pow_lane>(s, 0, slots, h + s, true);
  else if (blockIdx.y == 1)
    task_map_t<bgv_pow_lane>(s, 1, slots, split_q1(f, s), true);
  else if (blockIdx.y == 2)
    task_sig_decode_t<bgv_pow_lane>(s, slots, split_sig(f, s), sig_status, true);
  else
    task_pk(s, slots, pk_idx, cache, pk_bytes, rpk, pk_status, pk_agg);
}

// The latency path's second launch on teams (bgv_tcurve.h): blockIdx.y = 0 the cofactor
// clearing of q0 + q1 (one team per set), 1 r_i * sig_i (one team per set), 2 the
// signature's subgroup check (one lane per set).  A team whose cofactor clearing met an
// exceptional addition recomputes it on one lane with the complete formulas.
__global__ void __launch_bounds__(64) k_prep_team(const bgv_dslot* __restrict__ slots, uint32_t nslots,
                                                  g2_jac* __restrict__ h, fp12_t* __restrict__ f,
                                                  g2_jac* __restrict__ rsig, int32_t* __restrict__ sig_status) {
  if (blockIdx.y == 2) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslots || (slots[s].flags & BGV_SLOT_PAD) || sig_status[s] != BGV_ST_OK) return;
    if (!g2_in_subgroup(jac_from_aff(*split_sig(f, s)))) sig_status[s] = BGV_POINT_NOT_IN_GROUP;
    return;
  }
  __shared__ uint8_t prog[TCP_TABLE_BYTES];
  __shared__ fp_t Sall[BGV_FINAL_TEAMS][TCP_NSLOT];
  __shared__ int flags[BGV_FINAL_TEAMS];
  for (int i = threadIdx.x; i < TCP_TABLE_BYTES; i += 64) prog[i] = kTcProg[i];
  const int team = threadIdx.x / BGV_TEAM, c = threadIdx.x % BGV_TEAM;
  const uint32_t u = blockIdx.x * BGV_FINAL_TEAMS + team;
  const uint32_t uu = u < nslots ? u : nslots - 1;
  const bgv_dslot& d = slots[uu];
  const bool real = u < nslots && !(d.flags & BGV_SLOT_PAD);
  fp_t* S = Sall[team];
  if (c == 6) {
    S[TCP_S_ONE] = fp_one();
  } else if (c >= 7 && c < 11) {
    const fp2_t cx = BGV_PSI_CX, cy = BGV_PSI_CY;
    const fp2_t& v = c < 9 ? cx : cy;
    S[c < 9 ? TCP_S_PSI_CX + (c - 7) : TCP_S_PSI_CY + (c - 9)] = (c & 1) ? v.c0 : v.c1;
  } else if (c == 11) {
    S[TCP_S_PSI2_CX] = fp_t{BGV_PSI2_CX};
  } else if (c == 12) {
    S[TCP_S_PSI2_CY] = fp_t{BGV_PSI2_CY};
  }
  for (int i = c; i < TC_ISO_NCONST; i += BGV_TEAM) S[TCP_S_ISO + i] = tc_iso_const(i);
  tc_dev_engine e{prog, S, c, false};
  if (blockIdx.y == 0) {
    if (c < 6) {
      S[TCP_BANK(1) + c] = reinterpret_cast<const fp_t*>(h + uu)[c];
      S[TCP_BANK(2) + c] = reinterpret_cast<const fp_t*>(split_q1(f, uu))[c];
    }
    __syncthreads();
    tc_clear_cofactor(e);
    if (c == 0) flags[team] = e.bad ? 1 : 0;
    __syncthreads();
    if (real) {
      if (!flags[team]) {
        if (c < 6) reinterpret_cast<fp_t*>(h + uu)[c] = S[TCP_BANK(3) + c];
      } else if (c == 0) {
        h[uu] = g2_clear_cofactor(jac_add(iso_map_g2_jac(h[uu]), iso_map_g2_jac(*split_q1(f, uu))));
      }
    }
  } else {
    const bool ok = sig_status[uu] == BGV_ST_OK;  // the decode left it OK (the subgroup lanes may flip it)
    if (c < 4)
      S[TCP_BANK(1) + c] = reinterpret_cast<const fp_t*>(split_sig(f, uu))[c];
    else if (c < 6)
      S[TCP_BANK(1) + c] = c == 4 ? fp_one() : fp_zero();
    __syncthreads();
    tc_mul_glv(e, d.scalar);
    if (real && ok && c < 6) reinterpret_cast<fp_t*>(rsig + uu)[c] = S[TCP_BANK(4) + c];
  }
}

// The point-program engine of bgv_tcurve.h's schedules on a whole block (bgv_tround_dev.h:
// four-part round instructions): bank moves by the q = 0 lanes, one block per set.
struct tc_wide_engine : tr_wide_engine {
  __device__ void copy(int dst, int src) {
    if (q == 0 && c < 6 && dst != src) S[TCP_BANK(dst) + c] = S[TCP_BANK(src) + c];
    __syncthreads();
  }
  __device__ void neg_y(int b) {
    if (q == 0 && (c == 2 || c == 3)) S[TCP_BANK(b) + c] = fp_neg(S[TCP_BANK(b) + c]);
    __syncthreads();
  }
  __device__ void check_add() {
    if (q == 0 && c == 0) {
      const auto z2 = [&](int s) { return fp_is_zero(S[s]) && fp_is_zero(S[s + 1]); };
      bad = bad || z2(TC_CHK_A) || z2(TC_CHK_B);
    }
  }
};

// The G1 schedule (bgv_tg1.h) on the same four-part engine: three-slot banks.
struct tg1_wide_engine : tr_wide_engine {
  __device__ void copy(int dst, int src) {
    if (q == 0 && c < 3 && dst != src) S[TG1_BANK(dst) + c] = S[TG1_BANK(src) + c];
    __syncthreads();
  }
};

// k_prep_team for the smallest calls, one set per 64-lane block and task (blockIdx.y): 0 the
// cofactor clearing of q0 + q1, 1 r_i * sig_i, 2 the signature's subgroup check psi(P) ==
// [x]P with [|x|]P from the same point programs (a team-level exceptional addition falls
// back to the one-lane g2_in_subgroup).  Same schedules and formulas as k_prep_team.
__global__ void __launch_bounds__(64) k_prep_wide(const bgv_dslot* __restrict__ slots, uint32_t nslots,
                                                  g2_jac* __restrict__ h, fp12_t* __restrict__ f,
                                                  g2_jac* __restrict__ rsig, int32_t* __restrict__ sig_status,
                                                  const uint32_t* __restrict__ pk_idx,
                                                  const g1_aff* __restrict__ cache, const uint8_t* __restrict__ pk_bytes,
                                                  g1_jac* __restrict__ rpk, int32_t* __restrict__ pk_status,
                                                  g1_jac* __restrict__ pk_agg,
                                                  const bgv_dcommittee* __restrict__ com_dir,
                                                  const uint32_t* __restrict__ com_pool) {
  static_assert(TG1_TABLE_BYTES <= TCP_TABLE_BYTES && TG1_NSLOT <= TCP_NSLOT, "plane 3 reuses the G2 buffers");
  __shared__ uint8_t prog[TCP_TABLE_BYTES];
  __shared__ fp_t S[TCP_NSLOT];
  __shared__ fp_t RP[64];
  __shared__ int flag;
  if (blockIdx.y == 3) {  // the pubkey task, one set per block
    // a set of >= BGV_PK_TREE_MIN cached keys first sums them on the whole wave (k_pk_agg's
    // tree); lane 0 then takes the set's sum and status, and r * sum runs on the G1 point
    // programs (bgv_tg1.h) as rounds, concurrently with the other planes' G2 programs
    const uint32_t s = blockIdx.x;
    if (pk_agg) pk_agg_one(slots, s, pk_idx, cache, pk_agg);
    if (pk_agg) pk_bits_one(slots, s, pk_idx, com_dir, com_pool, cache, pk_agg);  // a committee-bitfield set
    if (threadIdx.x == 0) {
      g1_jac acc;
      const bool go = task_pk_sum(s, slots, pk_idx, cache, pk_bytes, pk_status, pk_agg, &acc);
      flag = go ? 1 : 0;
      if (go) {
        S[TG1_BANK(1)] = acc.x;
        S[TG1_BANK(1) + 1] = acc.y;
        S[TG1_BANK(1) + 2] = acc.z;
      }
      S[TG1_S_ONE] = fp_one();
      S[TG1_S_BETA] = fp_t{BGV_BETA_MX2};
    }
    for (int i = threadIdx.x; i < TG1_TABLE_BYTES; i += 64) prog[i] = kTg1Prog[i];
    __syncthreads();
    if (!flag) return;  // uniform over the block
    const int lane = threadIdx.x;
    tg1_wide_engine e{{prog, S, RP, tr_wide_lane_c(lane), tr_wide_lane_q(lane), false}};
    tg1_mul_glv(e, slots[s].scalar);
    // a sum outside G1 (a key taken on trust) whose schedule met an exceptional addition
    // (bgv_tg1.h tg1_exceptional): lane 0 repeats the task with the complete one-lane formulas
    if (tg1_exceptional(S[TG1_BANK(4) + 2])) {
      if (lane == 0) task_pk(s, slots, pk_idx, cache, pk_bytes, rpk, pk_status, pk_agg);
      return;
    }
    if (lane < 3) reinterpret_cast<fp_t*>(rpk + s)[lane] = S[TG1_BANK(4) + lane];
    if (lane == 0) pk_status[s] = BGV_ST_OK;
    return;
  }
  const uint32_t uu = blockIdx.x;  // grid = exactly nslots blocks per task
  const int lane = threadIdx.x, c = lane % BGV_TEAM, q = lane / BGV_TEAM;
  const bgv_dslot& d = slots[uu];
  const bool real = !(d.flags & BGV_SLOT_PAD);
  // the subgroup check only for signatures that decoded to a finite point (uniform per block)
  if (blockIdx.y == 2 && (!real || sig_status[uu] != BGV_ST_OK)) return;
  for (int i = lane; i < TCP_TABLE_BYTES; i += 64) prog[i] = kTcProg[i];
  if (q == 0) {
    if (c == 6) {
      S[TCP_S_ONE] = fp_one();
    } else if (c >= 7 && c < 11) {
      const fp2_t cx = BGV_PSI_CX, cy = BGV_PSI_CY;
      const fp2_t& v = c < 9 ? cx : cy;
      S[c < 9 ? TCP_S_PSI_CX + (c - 7) : TCP_S_PSI_CY + (c - 9)] = (c & 1) ? v.c0 : v.c1;
    } else if (c == 11) {
      S[TCP_S_PSI2_CX] = fp_t{BGV_PSI2_CX};
    } else if (c == 12) {
      S[TCP_S_PSI2_CY] = fp_t{BGV_PSI2_CY};
    }
  }
  for (int i = lane; i < TC_ISO_NCONST; i += 64) S[TCP_S_ISO + i] = tc_iso_const(i);
  tc_wide_engine e{{prog, S, RP, tr_wide_lane_c(lane), tr_wide_lane_q(lane), false}};
  if (blockIdx.y == 0) {
    if (q == 0 && c < 6) {
      S[TCP_BANK(1) + c] = reinterpret_cast<const fp_t*>(h + uu)[c];
      S[TCP_BANK(2) + c] = reinterpret_cast<const fp_t*>(split_q1(f, uu))[c];
    }
    __syncthreads();
    tc_clear_cofactor(e);
    if (lane == 0) flag = e.bad ? 1 : 0;
    __syncthreads();
    if (real) {
      if (!flag) {
        if (q == 0 && c < 6) reinterpret_cast<fp_t*>(h + uu)[c] = S[TCP_BANK(3) + c];
      } else if (lane == 0) {
        h[uu] = g2_clear_cofactor(jac_add(iso_map_g2_jac(h[uu]), iso_map_g2_jac(*split_q1(f, uu))));
      }
    }
  } else if (blockIdx.y == 1) {
    const bool ok = sig_status[uu] == BGV_ST_OK;  // read before the subgroup blocks may flip it
    if (q == 0) {
      if (c < 4)
        S[TCP_BANK(1) + c] = reinterpret_cast<const fp_t*>(split_sig(f, uu))[c];
      else if (c < 6)
        S[TCP_BANK(1) + c] = c == 4 ? fp_one() : fp_zero();
    }
    __syncthreads();
    tc_mul_glv(e, d.scalar);
    if (real && ok && q == 0 && c < 6) reinterpret_cast<fp_t*>(rsig + uu)[c] = S[TCP_BANK(4) + c];
  } else {
    // [|x|]P: base in bank 0, the accumulator (= P) in bank 4
    if (q == 0 && c < 6) {
      const fp_t v = c < 4 ? reinterpret_cast<const fp_t*>(split_sig(f, uu))[c] : (c == 4 ? fp_one() : fp_zero());
      S[TCP_BANK(0) + c] = v;
      S[TCP_BANK(4) + c] = v;
    }
    __syncthreads();
    const int a = tc_to_jac(e, tc_mul_x_abs(e));
    if (lane == 0) {
      const g2_jac p = jac_from_aff(*split_sig(f, uu));
      bool in;
      if (e.bad) {
        in = g2_in_subgroup(p);
      } else {
        const fp_t* B = S + TCP_BANK(a);
        const g2_jac xp = {{B[0], B[1]}, {B[2], B[3]}, {B[4], B[5]}};
        in = jac_eq(g2_psi(p), jac_neg(xp));  // psi(P) == [x]P = -[|x|]P
      }
      if (!in) sig_status[uu] = BGV_POINT_NOT_IN_GROUP;
    }
  }
}

// Committee-sized sets (BGV_PK_TREE_MIN..BGV_PK_TEAM_MAX cached keys, e.g. 128-key
// attestation aggregates) on a team of 16 lanes, four sets per wave: lane l sums keys
// l, l + 16, ... with mixed additions, then four ds_swizzle butterfly levels (xor 8..1, inside
// the team).  A whole wave per 128-key set spent ~4x the lane work on the tree levels.
// The lane's first key starts the sum (no addition to infinity), and each key is gathered
// one addition ahead of its use.  A gather-latency-bound kernel: BGV_WPE_AGG waves per SIMD.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BGV_WPE_AGG, BGV_WPE_AGG)))
k_pk_agg16(const bgv_dslot* __restrict__ slots, uint32_t nslots, const uint32_t* __restrict__ pk_idx,
           const g1_aff* __restrict__ cache, g1_jac* __restrict__ pk_agg) {
  pk_agg16_body(slots, nslots, blockIdx.x, pk_idx, cache, pk_agg);
}

// PublicKey.aggregate(...).toBytes(uncompressed) over cached keys through the verify
// path's own code: pk_sum of one slot (k_pk_agg's tree sum for >= BGV_PK_TREE_MIN keys,
// task_pk's serial sum below), then affine and the 96-byte ZCash encoding.
__global__ void k_pk_sum_out(const bgv_dslot* __restrict__ slot, const uint32_t* __restrict__ idx,
                             const g1_aff* __restrict__ cache, const g1_jac* __restrict__ pk_agg,
                             uint8_t* __restrict__ out96) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int32_t st = BGV_OK;
  const g1_jac acc = pk_sum(slot[0], idx, cache, nullptr, pk_agg, 0, &st);
  g1_aff a;
  const bool fin = jac_to_aff(&a, acc);
  uint8_t b[96];
  g1_serialize(b, a, !fin);
  for (int i = 0; i < 96; ++i) out96[i] = b[i];
}

}  // extern "C"

hipError_t bgv_launch_prep(const bgv_dev_batch& b, const bgv_streams& s) {
  const uint32_t n = b.nslots;
  if (n == 0) return hipSuccess;
  BGV_MARK(0);
  // k_pk_agg only when some set is large enough; otherwise k_prep sums serially (null pk_agg)
  const bool tree = b.max_npk >= BGV_PK_TREE_MIN;
  const uint32_t ncom = b.ncom_team + b.ncom_wave;  // committee-bitfield slots: their sums are in pk_agg too
  const uint32_t nspan = b.nspan_team + b.nspan_wave;  // span slots: the same, from k_pk_agg_span
  const bool agg = tree || ncom > 0 || nspan > 0;
  const bool wide = bgv_use_latency(b, n + b.ngroups) && n <= BGV_PREP_WIDE_MAX;
  if (wide) {
    const g1_aff* cache = reinterpret_cast<const g1_aff*>(b.cache_opaque);
    const hipError_t e = bgv_launch_prep_wave(b, s.main);
    if (e != hipSuccess) return e;
    // Span slots first, in a launch of their own: their body inside plane 3 (as pk_bits_one is)
    // grew k_prep_wide's scratch frame from 5,632 to 6,192 B per lane for every call.  A block per
    // set, as plane 3 has.
    if (nspan)
      hipLaunchKernelGGL(k_pk_agg_span, dim3(nspan), dim3(64), 0, s.main, b.slots, b.span, b.nspan_team, b.nspan_wave,
                         1u, b.pk_idx, b.com_dir, b.com_pool, cache, b.pk_agg);
    hipLaunchKernelGGL(k_prep_wide, dim3(n, 4), dim3(64), 0, s.main, b.slots, n, b.h, b.f, b.rsig, b.sig_status,
                       b.pk_idx, cache, b.pk_bytes, b.rpk, b.pk_status, agg ? b.pk_agg : nullptr, b.com_dir, b.com_pool);
    BGV_MARK(1);
    return hipGetLastError();
  }
  if (ncom)
    hipLaunchKernelGGL(k_pk_agg_bits, dim3(nblk(b.ncom_team, 4) + b.ncom_wave), dim3(64), 0, s.main, b.slots, b.com,
                       b.ncom_team, b.ncom_wave, b.pk_idx, b.com_dir, b.com_pool,
                       reinterpret_cast<const g1_aff*>(b.cache_opaque), b.pk_agg);
  if (nspan)
    hipLaunchKernelGGL(k_pk_agg_span, dim3(nblk(b.nspan_team, 4) + b.nspan_wave), dim3(64), 0, s.main, b.slots, b.span,
                       b.nspan_team, b.nspan_wave, 0u, b.pk_idx, b.com_dir, b.com_pool,
                       reinterpret_cast<const g1_aff*>(b.cache_opaque), b.pk_agg);
  if (tree)
    hipLaunchKernelGGL(k_pk_agg16, dim3(nblk(n, 4)), dim3(64), 0, s.main, b.slots, n, b.pk_idx,
                       reinterpret_cast<const g1_aff*>(b.cache_opaque), b.pk_agg);
  if (b.max_npk > BGV_PK_TEAM_MAX)
    hipLaunchKernelGGL(k_pk_agg, dim3(n), dim3(64), 0, s.main, b.slots, n, b.pk_idx,
                       reinterpret_cast<const g1_aff*>(b.cache_opaque), b.pk_agg);
  if (bgv_use_latency(b, n + b.ngroups)) {
    hipLaunchKernelGGL(k_prep_a, dim3(nblk(n, 64), 4), dim3(64), 0, s.main, b.slots, n, b.h, b.f, b.sig_status,
                       b.pk_idx, reinterpret_cast<const g1_aff*>(b.cache_opaque), b.pk_bytes, b.rpk, b.pk_status,
                       agg ? b.pk_agg : nullptr);
    hipLaunchKernelGGL(k_prep_team, dim3(nblk(n, BGV_FINAL_TEAMS), 3), dim3(64), 0, s.main, b.slots, n, b.h, b.f,
                       b.rsig, b.sig_status);
  } else {
    const hipError_t e = bgv_launch_prep_bulk(b, s, agg);
    if (e != hipSuccess) return e;
  }
  BGV_MARK(1);
  return hipGetLastError();
}

// slot: one device bgv_dslot {PK_CACHED, n_pk = n, pk_off = 0}; agg: one g1_jac of scratch
hipError_t bgv_launch_aggregate(const bgv_dslot* slot, const uint32_t* idx, uint32_t n, const bgv_cache_entry* cache,
                                void* agg, uint8_t* out96, hipStream_t st) {
  const g1_aff* c = reinterpret_cast<const g1_aff*>(cache);
  g1_jac* a = reinterpret_cast<g1_jac*>(agg);
  const bool tree = n >= BGV_PK_TREE_MIN;
  if (tree && n <= BGV_PK_TEAM_MAX) hipLaunchKernelGGL(k_pk_agg16, dim3(1), dim3(64), 0, st, slot, 1u, idx, c, a);
  if (tree && n > BGV_PK_TEAM_MAX) hipLaunchKernelGGL(k_pk_agg, dim3(1), dim3(64), 0, st, slot, 1u, idx, c, a);
  hipLaunchKernelGGL(k_pk_sum_out, dim3(1), dim3(64), 0, st, slot, idx, c, tree ? a : nullptr, out96);
  return hipGetLastError();
}

// The aggregate of one committee slot through k_pk_agg_bits.  slot: one device bgv_dslot
// {PK_COMMITTEE [| PK_COMPLEMENT], n_pk = bits set, pk_off = 0}; idx: the handle, then the bit
// words; list: one zero word (the slot's id); team: the chosen side has at most
// BGV_PK_TEAM_MAX terms; span: a span slot {PK_COMMITTEE | PK_SPAN}, idx its run (k_pk_agg_span);
// agg: one g1_jac of scratch
hipError_t bgv_launch_aggregate_bits(const bgv_dslot* slot, const uint32_t* idx, const uint32_t* list, bool team,
                                     bool span, const bgv_dcommittee* dir, const uint32_t* pool, const bgv_cache_entry* cache,
                                     void* agg, uint8_t* out96, hipStream_t st) {
  const g1_aff* c = reinterpret_cast<const g1_aff*>(cache);
  g1_jac* a = reinterpret_cast<g1_jac*>(agg);
  if (span)
    hipLaunchKernelGGL(k_pk_agg_span, dim3(1), dim3(64), 0, st, slot, list, team ? 1u : 0u, team ? 0u : 1u, 0u, idx,
                       dir, pool, c, a);
  else
    hipLaunchKernelGGL(k_pk_agg_bits, dim3(1), dim3(64), 0, st, slot, list, team ? 1u : 0u, team ? 0u : 1u, idx, dir,
                       pool, c, a);
  hipLaunchKernelGGL(k_pk_sum_out, dim3(1), dim3(64), 0, st, slot, idx, c, a, out96);
  return hipGetLastError();
}

hipError_t bgv_launch_committee_totals(bgv_dcommittee* dir, const uint32_t* handles, uint32_t nh, const uint32_t* pool,
                                       const bgv_cache_entry* cache, hipStream_t st) {
  if (nh == 0) return hipSuccess;
  hipLaunchKernelGGL(k_committee_total, dim3(nh), dim3(64), 0, st, dir, handles, nh, pool,
                     reinterpret_cast<const g1_aff*>(cache));
  return hipGetLastError();
}
