// CPU simulation of the device-side epoch shuffling: bgv_shuffle.h's table, walk and committee
// bounds run as the kernels of bgv_k_shuffle.hip run them, thread by thread, over buffers of the
// exact sizes the device call allocates.  Test infrastructure only; it reads a line protocol
// from stdin (tests/test_shuffling_cpu.py writes it) and prints what it computed.
//
//   shuffle <seedhex> <rounds> <n> <a_0> ... <a_{n-1}>
//     -> one line: the n shuffled indices, out[i] = a[compute_shuffled_index(i, n, seed)]
//        (k_shuffle_table's items in thread order, then k_shuffle_walk's positions)
//   bounds <n> <slots> <committees_per_slot>
//     -> "com <k> <lo> <hi>" per committee (shuf_bound), then "dir <j> <k> <lo> <hi>" per
//        non-empty committee as k_shuffle_dir's thread j derives it, then
//        "longest <len> nonempty <m>"
#include <stdio.h>
#include <stdlib.h>

#include <sstream>
#include <string>
#include <vector>

#include "../../lodestar_amd/csrc/bgv_shuffle.h"

namespace {

[[noreturn]] void die(const std::string& why) {
  fprintf(stderr, "shufflesim: %s\n", why.c_str());
  exit(2);
}

void run_shuffle(std::istringstream& in) {
  std::string sh;
  uint32_t rounds, n;
  in >> sh >> rounds >> n;
  if (!in || sh.size() != 64 || n < 1 || n > BGV_SHUFFLE_MAX_N || rounds > BGV_SHUFFLE_MAX_ROUNDS) die("bad shuffle line");
  uint8_t seed[32];
  for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)std::stoul(sh.substr(2 * i, 2), nullptr, 16);
  std::vector<uint32_t> active(n);
  for (uint32_t& a : active) in >> a;
  if (!in) die("short index list");
  if (n < 2) rounds = 0;  // bgv_launch_shuffle
  std::vector<uint32_t> table(shuf_table_words(n, rounds)), pivots(rounds), out(n);
  const shuf_seed s = shuf_seed_load(seed);
  const uint32_t items = rounds * (shuf_nblk(n) + 1u);
  // the grid is rounded up to whole blocks of 256 threads: the threads past the items write nothing
  for (uint32_t t = 0; t < (items + 255u) / 256u * 256u; ++t) shuf_table_item(t, s, n, rounds, table.data(), pivots.data());
  for (uint32_t p : pivots)
    if (p >= n) die("pivot past the list");
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t p = shuf_walk(i, n, rounds, table.data(), pivots.data());
    if (p >= n) die("walk left the list");
    out[i] = active[p];
  }
  for (uint32_t i = 0; i < n; ++i) printf(i ? " %u" : "%u", out[i]);
  printf("\n");
}

void run_bounds(std::istringstream& in) {
  uint32_t n, slots, cps;
  in >> n >> slots >> cps;
  if (!in || !slots || !cps) die("bad bounds line");
  const uint32_t count = slots * cps;
  for (uint32_t k = 0; k < count; ++k) printf("com %u %u %u\n", k, shuf_bound(n, k, count), shuf_bound(n, k + 1, count));
  const uint32_t m = shuf_nonempty(n, count);
  for (uint32_t j = 0; j < m; ++j) {
    uint32_t lo, hi;
    const uint32_t k = shuf_nonempty_k(n, count, j, &lo, &hi);
    printf("dir %u %u %u %u\n", j, k, lo, hi);
  }
  printf("longest %u nonempty %u\n", shuf_longest(n, count), m);
}

}  // namespace

int main() {
  std::string line;
  std::vector<char> buf(size_t(1) << 26);
  while (fgets(buf.data(), (int)buf.size(), stdin)) {
    std::istringstream in(buf.data());
    std::string op;
    if (!(in >> op)) continue;
    if (op == "shuffle")
      run_shuffle(in);
    else if (op == "bounds")
      run_bounds(in);
    else
      die("unknown line: " + op);
  }
  return 0;
}
