// Stand-alone check of the arithmetic and the chunking of a sum of ciphertext
// products (orion_amd/csrc/tensor_sum.h), which is all it includes.  The
// header's lazy accumulation -- 128-bit sums of unreduced products, a Barrett
// reduction every tsum::interval pairs -- is compared with unsigned __int128
// arithmetic that reduces after every product, on moduli of every Barrett
// class: 40, 46, 50 and 52 bits (x < 256 q^2), 55 and 60 bits (x < 8 q^2) and
// 61 bits (x < 4 q^2, the size of the special primes).  Per size two primes:
// the largest below 2^k and the smallest above 2^(k-1), the two ends of what
// bitlen(q) = k allows.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "tensor_sum.h"

typedef unsigned __int128 u128;
using tsum::u64;

static int g_fail = 0;
#define EXPECT(c)                                         \
  do {                                                    \
    if (!(c)) {                                           \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      if (++g_fail > 20) exit(1);                         \
    }                                                     \
  } while (0)

// the fields of common.h ModConst that tsum::mod_of reads, formed as the
// library's table forms them: floor(2^(2k+s) / q) where it fits 64 bits
struct ModConst {
  u64 q;
  int bar_k;
  u64 bar_mu2, bar_mu3, bar_mu8;
};
static ModConst mod_const(u64 q) {
  ModConst m{q, 0, 0, 0, 0};
  while ((q >> m.bar_k) != 0) ++m.bar_k;
  const int k = m.bar_k;
  m.bar_mu2 = (u64)(((u128)1 << (2 * k + 2)) / q);
  if (k <= 60) m.bar_mu3 = (u64)(((u128)1 << (2 * k + 3)) / q);
  if (k <= 52) m.bar_mu8 = (u64)(((u128)1 << (2 * k + 8)) / q);
  return m;
}

static u64 mulmod(u64 a, u64 b, u64 q) { return (u64)((u128)a * b % q); }
static u64 powmod(u64 a, u64 e, u64 q) {
  u64 r = 1;
  for (; e; e >>= 1, a = mulmod(a, a, q))
    if (e & 1) r = mulmod(r, a, q);
  return r;
}
// Miller-Rabin with the bases that decide every n < 2^64
static bool is_prime(u64 n) {
  if (n < 2) return false;
  for (u64 p : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull}) {
    if (n % p == 0) return n == p;
  }
  u64 d = n - 1;
  int r = 0;
  while (!(d & 1)) d >>= 1, ++r;
  for (u64 a : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull}) {
    u64 x = powmod(a, d, n);
    if (x == 1 || x == n - 1) continue;
    bool comp = true;
    for (int i = 1; i < r && comp; ++i) {
      x = mulmod(x, x, n);
      if (x == n - 1) comp = false;
    }
    if (comp) return false;
  }
  return true;
}

static u64 g_rng = 0x9e3779b97f4a7c15ull;
static u64 rnd() {  // xorshift64*
  g_rng ^= g_rng >> 12, g_rng ^= g_rng << 25, g_rng ^= g_rng >> 27;
  return g_rng * 0x2545f4914f6cdd1dull;
}
static u64 rnd_below(u64 q) { return (u64)(((u128)rnd() * q) >> 64); }

struct Tuple {
  std::vector<u64> a0, a1, b0, b1;
  std::vector<unsigned char> sq;
};
// D0, D1, D2 reduced after every product
static void reference(const Tuple& t, int n, u64 q, u64* d) {
  d[0] = d[1] = d[2] = 0;
  for (int i = 0; i < n; ++i) {
    const u64 b0 = t.sq[i] ? t.a0[i] : t.b0[i], b1 = t.sq[i] ? t.a1[i] : t.b1[i];
    d[0] = (d[0] + mulmod(t.a0[i], b0, q)) % q;
    d[1] = (u64)(((u128)d[1] + mulmod(t.a0[i], b1, q) + mulmod(t.a1[i], b0, q)) % q);
    d[2] = (d[2] + mulmod(t.a1[i], b1, q)) % q;
  }
}
// the header's routine, pair by pair
static void lazy(const Tuple& t, int n, const tsum::Mod& m, u64* d) {
  tsum::accumulate(t.a0.data(), t.a1.data(), t.b0.data(), t.b1.data(), t.sq.data(), n, m, d[0], d[1], d[2]);
}
// the same pairs in the kernel's order (tensor_sum_kernel): the squares first,
// two pairs at a time and an odd one last, each kind; d starts from d_in (a
// launch that adds to an earlier one's result).  `over` counts the steps that
// held more pairs than the interval allows
static void kernel_order(const Tuple& t, int n, const tsum::Mod& m, const u64* d_in, u64* d, int* over) {
  tsum::Acc3 s;
  tsum::zero(s);
  d[0] = d_in[0], d[1] = d_in[1], d[2] = d_in[2];
  int held = 0;
  for (int sq = 1; sq >= 0; --sq) {
    std::vector<int> idx;
    for (int i = 0; i < n; ++i)
      if ((int)t.sq[i] == sq) idx.push_back(i);
    size_t j = 0;
    for (; j < idx.size(); j += 2) {
      const int step = j + 1 < idx.size() ? 2 : 1;
      if (tsum::due(held, step, m)) tsum::flush(s, m, d[0], d[1], d[2]), held = 0;
      for (int u = 0; u < step; ++u) {
        const int i = idx[j + u];
        if (sq)
          tsum::mac_square(s, t.a0[i], t.a1[i]);
        else
          tsum::mac_pair(s, t.a0[i], t.a1[i], t.b0[i], t.b1[i]);
      }
      held += step;
      if (held > m.iv) ++*over;
    }
  }
  tsum::flush(s, m, d[0], d[1], d[2]);
}

static long g_cases = 0;
static void check_tuple(const Tuple& t, int n, const ModConst& mc, const u64* want) {
  const tsum::Mod m = tsum::mod_of(mc);
  u64 ref[3], got[3], ker[3];
  reference(t, n, mc.q, ref);
  lazy(t, n, m, got);
  EXPECT(got[0] == ref[0] && got[1] == ref[1] && got[2] == ref[2]);
  if (want) EXPECT(ref[0] == want[0] && ref[1] == want[1] && ref[2] == want[2]);
  int over = 0;
  const u64 d_in[3] = {mc.q - 1, mc.q - 1, rnd_below(mc.q)};
  kernel_order(t, n, m, d_in, ker, &over);
  EXPECT(over == 0);
  for (int c = 0; c < 3; ++c) EXPECT(ker[c] == (u64)(((u128)ref[c] + d_in[c]) % mc.q));
  ++g_cases;
}

static void check_modulus(u64 q, int bits) {
  EXPECT(is_prime(q));
  const ModConst mc = mod_const(q);
  EXPECT(mc.bar_k == bits);
  for (int n : {1, 2, 3, 4, 5, 8, 15, 16}) {
    Tuple t;
    t.a0.assign(n, q - 1), t.a1.assign(n, q - 1), t.b0.assign(n, q - 1), t.b1.assign(n, q - 1), t.sq.assign(n, 0);
    // the largest accumulators: (q-1)^2 = 1 mod q, so D0 = n, D1 = 2n, D2 = n
    const u64 top[3] = {(u64)n % q, (u64)(2 * n) % q, (u64)n % q};
    check_tuple(t, n, mc, top);
    t.sq.assign(n, 1);  // ... and as squares
    check_tuple(t, n, mc, top);
    t.a0.assign(n, 0), t.a1.assign(n, 0), t.b0.assign(n, 0), t.b1.assign(n, 0), t.sq.assign(n, 0);
    const u64 none[3] = {0, 0, 0};
    check_tuple(t, n, mc, none);
    for (int it = 0; it < 10000; ++it) {
      for (int i = 0; i < n; ++i) {
        // a quarter of the residues at the top of the range, a quarter of the pairs squares
        t.a0[i] = rnd() & 3 ? rnd_below(q) : q - 1 - (rnd() & 7);
        t.a1[i] = rnd() & 3 ? rnd_below(q) : q - 1 - (rnd() & 7);
        t.b0[i] = rnd() & 3 ? rnd_below(q) : q - 1 - (rnd() & 7);
        t.b1[i] = rnd() & 3 ? rnd_below(q) : q - 1 - (rnd() & 7);
        t.sq[i] = (rnd() & 3) == 0;
      }
      check_tuple(t, n, mc, nullptr);
    }
  }
}

int main() {
  // the documented bounds (tensor_sum.h): with s = 8, 3, 2 for k <= 52, 60, 61 a
  // reduction takes at most 2^s products, D1 takes two per pair, the Barrett
  // shift k + 1 + s fits 64 bits and the sum 2^s q^2 < 2^(2k+s) fits 128
  for (int k = 2; k <= 61; ++k) {
    const int s = k <= 52 ? 8 : k <= 60 ? 3 : 2;
    EXPECT(tsum::barrett_bits(k) == s);
    EXPECT(tsum::interval(k) >= 1 && 2 * tsum::interval(k) <= (1 << s));
    EXPECT(k + 1 + s <= 64 && 2 * k + s <= 128);
  }
  EXPECT(tsum::interval(52) >= ORION_MAXTSUM);  // one reduction per launch on the chain's 40-bit primes
  // the chunk planner
  const int M = ORION_MAXTSUM;
  EXPECT(M >= 2 && sizeof(tsum::Table) <= 1024 + 16);
  EXPECT(tsum::launches(1) == 1 && tsum::launches(M) == 1 && tsum::launches(M + 1) == 2 &&
         tsum::launches(2 * M + 1) == 3);
  EXPECT(tsum::launches(0) == 0 && tsum::launches(2 * M) == 2);
  for (int n : {1, M - 1, M, M + 1, 2 * M, 2 * M + 1, 5 * M + 3}) {
    int covered = 0;
    for (int c = 0; c < tsum::launches(n); ++c) {
      EXPECT(tsum::chunk_first(c) == covered);
      EXPECT(tsum::chunk_count(n, c) >= 1 && tsum::chunk_count(n, c) <= M);
      covered += tsum::chunk_count(n, c);
    }
    EXPECT(covered == n && tsum::chunk_count(n, tsum::launches(n)) == 0);
  }
  // the arithmetic
  for (int bits : {40, 46, 50, 52, 55, 60, 61}) {
    u64 hi = ((u64)1 << bits) - 1, lo = ((u64)1 << (bits - 1)) + 1;
    while (!is_prime(hi)) hi -= 2;
    while (!is_prime(lo)) lo += 2;
    check_modulus(hi, bits);
    check_modulus(lo, bits);
  }
  if (g_fail) {
    printf("%d checks failed\n", g_fail);
    return 1;
  }
  printf("tensor sums agree with 128-bit arithmetic on %ld tuples; the planner and the bounds hold\n", g_cases);
  return 0;
}
