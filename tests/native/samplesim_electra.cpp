// CPU simulation of the device-side balance-weighted sampling under Electra's rule (16 random
// bits per candidate, uint16_t balances): bgv_sample.h's 16-bit item functions, ordered compaction
// and pass loop run as k_sample_eval16 / k_sample_pick of bgv_k_sample.hip run them, block by block
// and wave by wave, over buffers of the exact sizes the device call allocates.  The byte rule's
// simulator is samplesim.cpp.  Test infrastructure only; it reads a line protocol from stdin
// (tests/samplesim_electra.py writes it) and prints what it computed.
//
//   sample <n_seeds> <want> <proposers 0|1> <max_incr> <rounds> <n> <n_eff> <seedhex>.. <a_0>.. <effhex>
//     effhex: four hex digits per validator index, the uint16_t little-endian as it lies in memory
//     -> "pass <window> <count> <seeds in the pass>" per pass of samp_run, then per seed
//        "seed <have> <candidates examined> <pick>..", then "us <microseconds of the loop>"
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <sstream>
#include <string>
#include <vector>

#include "../../lodestar_amd/csrc/bgv_sample.h"

namespace {

[[noreturn]] void die(const std::string& why) {
  fprintf(stderr, "samplesim_electra: %s\n", why.c_str());
  exit(2);
}

// k_sample_eval16 + k_sample_pick of one pass, thread by thread
struct SimDev {
  std::vector<shuf_seed> seeds;
  std::vector<samp_state> state;  // the device's copy
  std::vector<uint32_t> active;
  std::vector<uint16_t> eff;
  uint32_t max_incr, rounds, limit, want;
  std::vector<uint32_t> picks;
  std::vector<samp_pass> passes;
  std::vector<uint32_t> pass_seeds;

  void eval_block(uint32_t bx, uint32_t by, const std::vector<uint32_t>& todo, uint32_t window, uint32_t* vals,
                  uint8_t* flags) {
    uint32_t piv[BGV_SAMPLE_BLOCK], rnd[BGV_SAMPLE_RAND_DIGESTS16 * 8u];
    const uint32_t s = todo[by], n = (uint32_t)active.size();
    const uint32_t base = state[s].next + bx * BGV_SAMPLE_BLOCK;
    if (base % BGV_SAMPLE_BLOCK) die("a block's first candidate is no multiple of the block");
    for (uint32_t t = 0; t < BGV_SAMPLE_BLOCK; ++t) samp_setup_item16(t, seeds[s], n, rounds, base, piv, rnd);
    for (uint32_t t = 0; t < BGV_SAMPLE_BLOCK; ++t) {
      uint32_t v;
      const bool ok =
          samp_eval_item16(t, seeds[s], n, rounds, base, limit, piv, rnd, active.data(), eff.data(), max_incr, &v);
      const size_t at = (size_t)by * window + bx * BGV_SAMPLE_BLOCK + t;
      vals[at] = v;
      flags[at] = ok ? 1 : 0;
    }
  }

  void pick_block(uint32_t bx, const std::vector<uint32_t>& todo, uint32_t window, uint32_t count, const uint32_t* vals,
                  const uint8_t* flags) {
    constexpr uint32_t NW = BGV_SAMPLE_BLOCK / BGV_SAMPLE_WAVE;
    const uint32_t s = todo[bx];
    const size_t row = (size_t)bx * window;
    uint32_t have = state[s].have;
    for (uint32_t c = 0; c < window / BGV_SAMPLE_BLOCK; ++c) {
      uint64_t ballot[NW] = {};
      uint32_t wcnt[NW], total = 0;
      for (uint32_t t = 0; t < BGV_SAMPLE_BLOCK; ++t) {
        const uint32_t j = c * BGV_SAMPLE_BLOCK + t;
        if (j < count && flags[row + j]) ballot[t / BGV_SAMPLE_WAVE] |= uint64_t(1) << (t % BGV_SAMPLE_WAVE);
      }
      for (uint32_t w = 0; w < NW; ++w) total += wcnt[w] = (uint32_t)__builtin_popcountll(ballot[w]);
      for (uint32_t t = 0; t < BGV_SAMPLE_BLOCK; ++t) {
        const uint32_t wave = t / BGV_SAMPLE_WAVE;
        uint32_t before = have;
        for (uint32_t w = 0; w < wave; ++w) before += wcnt[w];
        const uint32_t dst = samp_pick_dst(ballot[wave], t % BGV_SAMPLE_WAVE, before, want);
        if (dst < want) {
          if ((size_t)s * want + dst >= picks.size()) die("pick past the seed's picks");
          picks[(size_t)s * want + dst] = vals[row + c * BGV_SAMPLE_BLOCK + t];
        }
      }
      have = have + total < want ? have + total : want;
    }
    state[s].have = have;
    state[s].next += count;
  }

  int pass(const std::vector<uint32_t>& todo, const samp_pass& p, std::vector<samp_state>& st) {
    if (p.window % BGV_SAMPLE_BLOCK || p.count > p.window || !p.count) die("bad pass");
    passes.push_back(p);
    pass_seeds.push_back((uint32_t)todo.size());
    std::vector<uint32_t> vals(todo.size() * (size_t)p.window);
    std::vector<uint8_t> flags(vals.size());
    for (uint32_t by = 0; by < todo.size(); ++by)
      for (uint32_t bx = 0; bx < p.window / BGV_SAMPLE_BLOCK; ++bx)
        eval_block(bx, by, todo, p.window, vals.data(), flags.data());
    for (uint32_t bx = 0; bx < todo.size(); ++bx) pick_block(bx, todo, p.window, p.count, vals.data(), flags.data());
    st = state;
    return 0;
  }
};

void run_sample(std::istringstream& in) {
  uint32_t n_seeds, want, prop, max_incr, rounds, n, n_eff;
  in >> n_seeds >> want >> prop >> max_incr >> rounds >> n >> n_eff;
  if (!in || n_seeds < 1 || n_seeds > BGV_SAMPLE_MAX_SEEDS || want < 1 || want > BGV_SAMPLE_MAX_WANT || n < 1 ||
      n > BGV_SHUFFLE_MAX_N || rounds > BGV_SHUFFLE_MAX_ROUNDS || max_incr < 1 || max_incr > samp_rule16::MAX_INCR ||
      n_eff < 1)
    die("bad sample line");
  SimDev dev;
  dev.max_incr = max_incr;
  dev.rounds = rounds;
  dev.want = want;
  dev.limit = samp_limit(n, prop != 0);
  for (uint32_t s = 0; s < n_seeds; ++s) {
    std::string sh;
    in >> sh;
    if (!in || sh.size() != 64) die("bad seed");
    uint8_t seed[32];
    for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)std::stoul(sh.substr(2 * i, 2), nullptr, 16);
    dev.seeds.push_back(shuf_seed_load(seed));
  }
  dev.active.resize(n);
  for (uint32_t& a : dev.active) in >> a;
  std::string eh;
  in >> eh;
  if (!in || eh.size() != 4 * (size_t)n_eff) die("short lists");
  dev.eff.resize(n_eff);
  for (uint32_t i = 0; i < n_eff; ++i) {
    const unsigned long lo = std::stoul(eh.substr(4 * (size_t)i, 2), nullptr, 16);
    const unsigned long hi = std::stoul(eh.substr(4 * (size_t)i + 2, 2), nullptr, 16);
    dev.eff[i] = (uint16_t)(lo | hi << 8);
  }
  for (uint32_t a : dev.active)
    if (a >= n_eff) die("active index past the balances");
  dev.state.assign(n_seeds, samp_state{0, 0});
  dev.picks.assign((size_t)n_seeds * want, 0);
  std::vector<samp_state> st;
  const auto t0 = std::chrono::steady_clock::now();
  if (samp_run(dev, n_seeds, want, dev.limit, st)) die("pass failed");
  const auto us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
  for (size_t k = 0; k < dev.passes.size(); ++k)
    printf("pass %u %u %u\n", dev.passes[k].window, dev.passes[k].count, dev.pass_seeds[k]);
  for (uint32_t s = 0; s < n_seeds; ++s) {
    if (st[s].have > want || st[s].next > dev.limit) die("state out of range");
    printf("seed %u %u", st[s].have, st[s].next);
    for (uint32_t k = 0; k < st[s].have; ++k) printf(" %u", dev.picks[(size_t)s * want + k]);
    printf("\n");
  }
  printf("us %lld\n", (long long)us);
}

}  // namespace

int main() {
  std::vector<char> buf(size_t(1) << 26);
  while (fgets(buf.data(), (int)buf.size(), stdin)) {
    std::istringstream in(buf.data());
    std::string op;
    if (!(in >> op)) continue;
    if (op == "sample")
      run_sample(in);
    else
      die("unknown line: " + op);
  }
  return 0;
}
