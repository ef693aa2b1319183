// Host-side check of the event path's division-free arithmetic (csrc/sgn_internal.h: umod64,
// tb_refills, tb_quot, tb_conforming) against the plain / and % operators, and of the batched
// token-bucket removal against n removals one after another.
#include <cstdio>
#include <random>
#include <vector>

#include "sgn_internal.h"

using u64 = uint64_t;
static long bad = 0, n_checks = 0;

#define CHECK(cond, ...)                \
  do {                                  \
    n_checks++;                         \
    if (!(cond) && bad++ < 10) {        \
      printf("mismatch: " __VA_ARGS__); \
      printf("\n");                     \
    }                                   \
  } while (0)

static void check_mod(u64 d, u64 x) {
  sgn::UDiv64 u;
  u.init(d);
  CHECK(sgn::umod64(u, x, d) == x % d, "umod64 d=%llu x=%llu", (unsigned long long)d, (unsigned long long)x);
}

// ceil(req / inc) for the removals a bucket can refuse: 0 < req < 2^32
static void check_refills(u64 req, u64 inc) {
  if (req == 0 || (req >> 32)) return;
  CHECK(sgn::tb_refills(req, inc) == req / inc + ((req % inc) ? 1 : 0), "tb_refills req=%llu inc=%llu",
        (unsigned long long)req, (unsigned long long)inc);
}

// bal / dec for a balance up to 2^53 and a wire length below 2^32
static void check_quot(u64 bal, u64 dec) {
  if (bal > (1ULL << 53) || dec == 0 || (dec >> 32)) return;
  CHECK(sgn::tb_quot(bal, dec) == bal / dec, "tb_quot bal=%llu dec=%llu", (unsigned long long)bal,
        (unsigned long long)dec);
  for (uint32_t n : {1u, 2u, 3u, 65535u, 0xFFFFFFFFu}) {
    const u64 q = bal / dec;
    CHECK(sgn::tb_conforming(bal, dec, n) == (q < n ? q : n), "tb_conforming bal=%llu dec=%llu n=%u",
          (unsigned long long)bal, (unsigned long long)dec, n);
  }
}

// n TokenBucket::comforming_remove(dec) calls at one instant after the refill, one by one with
// plain division (token_bucket.rs:65-117), against the batched form the round kernels use
static void check_batch(u64 bal, u64 dec, uint32_t n, u64 inc) {
  if (dec == 0 || dec > sgn::TB_WIRE_MAX || bal > (1ULL << 53)) return;
  u64 b = bal, refills = 0;
  uint32_t ok = 0;
  for (uint32_t k = 0; k < n; k++) {
    if (dec > b) {
      const u64 req = dec - b;
      refills = req / inc + ((req % inc) ? 1 : 0);
      break;
    }
    b -= dec;
    ok++;
  }
  const uint32_t m = sgn::tb_conforming(bal, dec, n);
  const u64 b2 = bal - (u64)m * dec;
  const u64 r2 = m < n ? sgn::tb_refills(dec - b2, inc) : 0;
  CHECK(m == ok && b2 == b && r2 == refills, "batch bal=%llu dec=%llu n=%u inc=%llu", (unsigned long long)bal,
        (unsigned long long)dec, n, (unsigned long long)inc);
}

static std::vector<u64> dividends(u64 d) {
  std::vector<u64> x = {0, d - 1, d, d + 1, (1ULL << 32) - 1, 1ULL << 32, (1ULL << 32) + 1, 1ULL << 53,
                        ~0ULL, ~0ULL - 1};
  for (u64 k : {2ULL, 3ULL, 7ULL, 1000ULL, 65536ULL, 1ULL << 20, (1ULL << 32) + 5}) {
    const unsigned __int128 p = (unsigned __int128)k * d;
    if (p + 1 <= (unsigned __int128)~0ULL) {
      x.push_back((u64)p - 1);
      x.push_back((u64)p);
      x.push_back((u64)p + 1);
    }
  }
  return x;
}

int main() {
  std::mt19937_64 rng(20240607);
  // the free ring's modulus: cq_pages
  const u64 pages[] = {1, 2, 3, 16, 160, 65535, 65537, 1ULL << 31, (1ULL << 32) - 1};
  for (u64 d : pages) {
    for (u64 x : dividends(d)) check_mod(d, x);
    for (int i = 0; i < 100000; i++) {
      check_mod(d, rng());
      check_mod(d, rng() >> (rng() % 64));
    }
  }
  // every refill increment from 8 kbit/s to 2^63 bit/s (sgn_sim_init: max(1, bw / 8 / 1000)),
  // by powers of two and their neighbours, plus the common decimal rates
  std::vector<u64> incs;
  auto add_bw = [&](u64 bw) { incs.push_back(std::max<u64>(1, bw / 8 / 1000)); };
  for (int s = 13; s <= 63; s++)
    for (long o = -1; o <= 1; o++) add_bw((1ULL << s) + (u64)o);
  for (u64 bw : {8000ULL, 64000ULL, 1000000ULL, 10000000ULL, 100000000ULL, 1000000000ULL, 10000000000ULL,
                 100000000000ULL, 34359738368000ULL, 34359738376000ULL, 1ULL << 46})
    add_bw(bw);
  const u64 wires[] = {28, 29, 40, 44, 128, 1028, 1488, 1500, 65535 + 28, sgn::TB_WIRE_MAX};
  for (u64 inc : incs) {
    for (u64 x : dividends(inc)) {
      check_refills(x, inc);
      for (u64 w : wires) check_quot(x, w);
    }
    for (u64 w : wires) {
      for (u64 x : dividends(w)) {
        check_refills(x, inc);
        check_quot(x, w);
        check_quot(x + inc, w);
        if (x / w < 4096)  // (the one-by-one reference walks the conforming packets)
          for (uint32_t n : {1u, 2u, 5u, 64u, 65535u, 0xFFFFFFFFu}) check_batch(x, w, n, inc);
      }
      for (uint32_t n : {1u, 2u, 5u, 64u, 4000u})  // a full bucket
        check_batch(std::min<u64>(inc + 1500, 1ULL << 53), w, n, inc);
    }
  }
  // seeded random pairs
  for (int i = 0; i < 3000000; i++) {
    const u64 inc = incs[rng() % incs.size()];
    const u64 dec = 28 + rng() % (sgn::TB_WIRE_MAX - 27);
    const u64 cap = std::min<u64>(inc + 1500, 1ULL << 53);
    const u64 bal = (rng() >> (rng() % 64)) % (cap + 1);
    check_refills(1 + rng() % dec, inc);
    check_refills((rng() >> (32 + rng() % 32)) | 1, inc);
    check_quot(bal, dec);
    check_quot(rng() >> (11 + rng() % 53), 1 + (rng() >> (32 + rng() % 32)));
    if ((i & 7) == 0) check_batch(bal, dec, 1 + (uint32_t)(rng() % 3000), inc);
  }
  printf("%ld checks, %ld bad\n", n_checks, bad);
  return bad != 0;
}
