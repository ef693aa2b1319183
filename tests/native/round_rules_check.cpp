// Host-side check of the two round rules the kernels share with host code (csrc/sgn_internal.h):
// sgn::wg_groups (the groups of a persistent grid's workgroup) and sgn::window_end (the next
// window's end). Prints one "groups P G w: g ..." line per PERIODIC workgroup, for the test that
// reads the real mapping, then "N checks, M bad".
#include <cstdio>
#include <random>
#include <vector>

#include "sgn_internal.h"

static long n_checks = 0, n_bad = 0;
static void check(bool ok, const char* what, uint64_t a, uint64_t b, uint64_t c) {
  n_checks++;
  if (!ok && n_bad++ < 10)
    printf("bad: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
}

template <uint32_t kApp>
static void groups(uint32_t P, uint32_t G) {
  std::vector<uint32_t> seen(G, 0), lo(8, G), hi(8, 0), cnt(8, 0);
  for (uint32_t w = 0; w < P; w++) {
    uint32_t gq0, gq1, gqs;
    sgn::wg_groups<kApp>(G, w, P, gq0, gq1, gqs);
    check(gqs > 0, "a zero stride", P, G, w);
    if (kApp == SGN_TRAFFIC_PERIODIC) printf("groups %u %u %u:", P, G, w);
    for (uint32_t g = gq0; g < gq1 && gqs; g += gqs) {
      check(g < G, "a group past G", P, G, w);
      if (g >= G) break;
      seen[g]++;
      const uint32_t x = w & 7u;
      lo[x] = g < lo[x] ? g : lo[x];
      hi[x] = g > hi[x] ? g : hi[x];
      cnt[x]++;
      if (kApp == SGN_TRAFFIC_PERIODIC) printf(" %u", g);
    }
    if (kApp == SGN_TRAFFIC_PERIODIC) printf("\n");
  }
  for (uint32_t g = 0; g < G; g++) check(seen[g] == 1, "a group not exactly once per round", P, G, g);
  if (kApp == SGN_TRAFFIC_PERIODIC)  // each w % 8 class covers one contiguous range
    for (uint32_t x = 0; x < 8; x++) check(cnt[x] == 0 || hi[x] - lo[x] + 1 == cnt[x], "a class with holes", P, G, x);
}

// the rule restated without the wrap test: the sum in 128 bits
static uint64_t window_end_ref(uint64_t min_next, uint64_t used, bool dynamic, uint64_t min_possible, uint64_t cfg,
                               uint64_t end_time) {
  const uint64_t lat = dynamic && used != sgn::INVALID ? used : min_possible;
  const unsigned __int128 sum = (unsigned __int128)min_next + (lat > cfg ? lat : cfg);
  const uint64_t ne = sum > sgn::EMU_MAX ? sgn::EMU_MAX : (uint64_t)sum;
  return ne < end_time ? ne : end_time;
}

static void window(uint64_t min_next, uint64_t used, bool dynamic, uint64_t min_possible, uint64_t cfg,
                   uint64_t end_time) {
  const uint64_t got = sgn::window_end(min_next, used, dynamic, min_possible, cfg, end_time);
  check(got == window_end_ref(min_next, used, dynamic, min_possible, cfg, end_time), "window_end", min_next, used, cfg);
  check(got <= end_time && got <= sgn::EMU_MAX, "window_end past its clamps", min_next, got, end_time);
  if (end_time < min_next) check(!(min_next < got), "an active window past the end", min_next, got, end_time);
}

int main() {
  const uint32_t pg[][2] = {{1, 1}, {2, 5}, {7, 7}, {9, 100}, {625, 625}, {2048, 15625}, {1792, 15625},
                            {2040, 15625}, {300, 200}};
  for (const auto& c : pg) {
    groups<SGN_TRAFFIC_PERIODIC>(c[0], c[1]);
    groups<SGN_TRAFFIC_TGEN>(c[0], c[1]);
    groups<SGN_TRAFFIC_EXTERNAL>(c[0], c[1]);
  }
  const uint64_t T0 = sgn::SIM_START, MS = 1000000, MAXT = sgn::EMU_MAX, NONE = sgn::INVALID;
  // min_next + ra wrapping past 2^64, and landing above EMU_MAX
  window(MAXT - 5, NONE, false, 10, 0, MAXT);
  window(MAXT - 5, 20, true, 10, 0, NONE);
  window(MAXT, NONE, false, 1, 0, MAXT);
  window(MAXT - 1, NONE, false, 2, 0, NONE);  // (lands on INVALID: above EMU_MAX)
  window(MAXT - 1, NONE, false, 1, 0, NONE);  // (lands on EMU_MAX itself)
  window(1ull << 63, NONE, false, 1ull << 63, 0, NONE);
  window(T0, NONE, false, NONE, NONE, MAXT);
  // end_time below min_next: an inactive window
  window(T0 + 5 * MS, NONE, false, MS, 0, T0 + MS);
  window(T0 + 5 * MS, NONE, false, MS, 0, T0 + 5 * MS);
  window(MAXT, 7, true, MS, 0, T0);
  // dynamic with and without a used latency; runahead_cfg above and below the latency
  for (int dynamic = 0; dynamic < 2; dynamic++)
    for (uint64_t used : {NONE, 3 * MS, MS / 2})
      for (uint64_t cfg : {(uint64_t)0, MS / 4, MS, 2 * MS, 10 * MS})
        for (uint64_t end : {T0 + MS / 8, T0 + 20 * MS, MAXT}) window(T0 + MS / 4, used, dynamic != 0, MS, cfg, end);
  std::mt19937_64 rng(20240611);
  auto some = [&]() -> uint64_t {  // every magnitude, and the values next to the special ones
    switch (rng() % 6) {
      case 0: return rng();
      case 1: return rng() >> (rng() % 64);
      case 2: return MAXT - (rng() % 1000);
      case 3: return NONE;
      case 4: return T0 + (rng() >> (24 + rng() % 40));
      default: return rng() % 1000;
    }
  };
  for (int i = 0; i < 6000; i++) window(some(), some(), (rng() & 1) != 0, some(), some(), some());
  printf("%ld checks, %ld bad\n", n_checks, n_bad);
  return n_bad != 0;
}
