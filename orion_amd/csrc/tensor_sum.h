// tensor_sum.h -- the arithmetic and the chunking of a sum of ciphertext
// products, sum_i a_i x b_i, accumulated before its one relinearisation
// (Context::mul_relin_sum, tensor_sum_kernel).  Host and device; it includes
// nothing of the library, so it also compiles host-only (tsum::mod_of takes
// the modulus' constants from any type shaped like common.h ModConst).
//
// Per coefficient and limb, over the pairs i:
//   D0 = sum a_i.c0 b_i.c0,  D1 = sum (a_i.c0 b_i.c1 + a_i.c1 b_i.c0),  D2 = sum a_i.c1 b_i.c1   (mod q)
// The products are summed unreduced in 128 bits and reduced rarely; every
// result is exact mod q and fully reduced, so neither the order of the pairs
// nor where the reductions fall changes a bit of it.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define TSUM_HD __host__ __device__ inline
#else
#define TSUM_HD inline
#endif

// pairs per tensor_sum_kernel launch: 16 pairs x 64 B of {2 pointers, 2 x
// (component, limb, batch) strides} are 1 KB of kernel arguments
#define ORION_MAXTSUM 16

namespace tsum {

typedef uint64_t u64;

struct Acc {
  u64 hi, lo;
};
struct Acc3 {
  Acc d0, d1, d2;
};

// (in the library, after hip_runtime.h: common.h mulhi64's device form)
TSUM_HD u64 mulhi(u64 a, u64 b) {
#if defined(__HIP_DEVICE_COMPILE__) && defined(HIP_INCLUDE_HIP_HIP_RUNTIME_H)
  return __umul64hi(a, b);
#else
  return (u64)(((unsigned __int128)a * b) >> 64);
#endif
}
// a += h:l
TSUM_HD void add128(Acc& a, u64 h, u64 l) {
  const u64 nl = a.lo + l;
  a.hi += h + (nl < l);
  a.lo = nl;
}
TSUM_HD void zero(Acc3& s) { s.d0.hi = s.d0.lo = s.d1.hi = s.d1.lo = s.d2.hi = s.d2.lo = 0; }

// The accumulation bounds.  Residues are below q < 2^k, k = bitlen(q) <= 61, so
// a product is below q^2 and a sum of m products below m q^2.  The Barrett
// reduction below takes x < 2^s q^2 with mu = floor(2^(2k+s) / q): its first
// shift t1 = x >> (k-1) is below 2^(k+1+s) and must fit 64 bits, so s <= 63 - k.
// The table of moduli carries mu for s = 8 (k <= 52), s = 3 (k <= 60) and s = 2
// (k <= 61): 256, 8 or 4 products per reduction.  (The 128-bit sum itself has
// room to spare: 2^s q^2 < 2^(2k+s) <= 2^124.)
TSUM_HD int barrett_bits(int k) { return k <= 52 ? 8 : k <= 60 ? 3 : 2; }
// Pairs between two reductions.  D1 takes two products per pair, D0 and D2 one;
// the three are reduced together, so D1's bound holds for all: 2 * interval <=
// 2^s, that is 128, 4 or 2 pairs.  (At 128 a launch of ORION_MAXTSUM pairs
// reduces once, at its end.)
TSUM_HD int interval(int k) { return (1 << barrett_bits(k)) / 2; }

// what the reduction needs of one modulus, chosen once per limb from the
// modulus' constants (common.h ModConst, or any type with its q, bar_k,
// bar_mu2, bar_mu3 and bar_mu8)
struct Mod {
  u64 q, mu;  // mu = floor(2^(2k+s) / q), s = barrett_bits(k)
  int k, sh;  // sh = k + 1 + s <= 64
  int iv;     // interval(k)
};
template <class MC>
TSUM_HD Mod mod_of(const MC& m) {
  const int k = m.bar_k, s = barrett_bits(k);
  return Mod{m.q, s == 8 ? m.bar_mu8 : s == 3 ? m.bar_mu3 : m.bar_mu2, k, k + 1 + s, interval(k)};
}
// x = a.hi:a.lo < 2^s q^2 to [0, q).  q_est = (t1 mu) >> sh is low by less than
// 1 (its own floor) + 1 (mu's: t1 < 2^sh) + 1 (t1's: mu <= 2^sh), so by at
// most 2: two conditional subtractions
TSUM_HD u64 reduce(const Acc& a, const Mod& m) {
  const u64 t1 = (a.lo >> (m.k - 1)) | (a.hi << (65 - m.k));
  const u64 ph = mulhi(t1, m.mu), pl = t1 * m.mu;
  const u64 t2 = m.sh < 64 ? (pl >> m.sh) | (ph << (64 - m.sh)) : ph;
  u64 r = a.lo - t2 * m.q;
  r = r >= m.q ? r - m.q : r;
  return r >= m.q ? r - m.q : r;
}

// one pair's four products
TSUM_HD void mac_pair(Acc3& s, u64 a0, u64 a1, u64 b0, u64 b1) {
  add128(s.d0, mulhi(a0, b0), a0 * b0);
  add128(s.d1, mulhi(a0, b1), a0 * b1);
  add128(s.d1, mulhi(a1, b0), a1 * b0);
  add128(s.d2, mulhi(a1, b1), a1 * b1);
}
// a square pair (b = a): three products, the middle one added twice
TSUM_HD void mac_square(Acc3& s, u64 a0, u64 a1) {
  add128(s.d0, mulhi(a0, a0), a0 * a0);
  const u64 h = mulhi(a0, a1), l = a0 * a1;
  add128(s.d1, h, l);
  add128(s.d1, h, l);
  add128(s.d2, mulhi(a1, a1), a1 * a1);
}
// true: `held` pairs are in the sums and `more` further ones would pass the bound
TSUM_HD bool due(int held, int more, const Mod& m) { return held + more > m.iv; }
// the sums reduced, added to (r0, r1, r2) mod q, and cleared
TSUM_HD void flush(Acc3& s, const Mod& m, u64& r0, u64& r1, u64& r2) {
  const u64 q = m.q;
  u64 t = r0 + reduce(s.d0, m);
  r0 = t >= q ? t - q : t;
  t = r1 + reduce(s.d1, m);
  r1 = t >= q ? t - q : t;
  t = r2 + reduce(s.d2, m);
  r2 = t >= q ? t - q : t;
  zero(s);
}

// One coefficient's D0, D1, D2 over the pairs [0, n): pair i is (a0[i], a1[i])
// x (b0[i], b1[i]), a square where sq[i] (sq may be null).  The results are in
// [0, q).  tensor_sum_kernel runs the same steps on two coefficients at once.
TSUM_HD void accumulate(const u64* a0, const u64* a1, const u64* b0, const u64* b1, const unsigned char* sq, int n,
                        const Mod& m, u64& d0, u64& d1, u64& d2) {
  Acc3 s;
  zero(s);
  d0 = d1 = d2 = 0;
  int held = 0;
  for (int i = 0; i < n; ++i) {
    if (due(held, 1, m)) flush(s, m, d0, d1, d2), held = 0;
    if (sq && sq[i])
      mac_square(s, a0[i], a1[i]);
    else
      mac_pair(s, a0[i], a1[i], b0[i], b1[i]);
    ++held;
  }
  flush(s, m, d0, d1, d2);
}

// The pairs of one launch, by value in the kernel arguments (a captured graph
// holds them in its node, no device buffer): component c, limb l, image b of
// operand a at a + c a_comp + l a_limb + b a_batch, a batch stride of 0 for a
// one-image operand broadcast over the batch.  The squares come first: pr[0,
// nsq) read a alone, pr[nsq, n) both operands.
struct Pair {
  const u64 *a, *b;
  long long a_comp, a_limb, a_batch, b_comp, b_limb, b_batch;
};
struct Table {
  Pair pr[ORION_MAXTSUM];
  int n, nsq;
};

// n pairs run as ceil(n / ORION_MAXTSUM) launches; launch c takes the pairs
// [chunk_first(c), chunk_first(c) + chunk_count(n, c)); the first writes d,
// every later one adds its sums to d
inline int launches(int n) { return n < 1 ? 0 : (n + ORION_MAXTSUM - 1) / ORION_MAXTSUM; }
inline int chunk_first(int c) { return c * ORION_MAXTSUM; }
inline int chunk_count(int n, int c) {
  const int left = n - c * ORION_MAXTSUM;
  return left < 0 ? 0 : left < ORION_MAXTSUM ? left : ORION_MAXTSUM;
}

}  // namespace tsum
