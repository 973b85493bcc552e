// kernels.hip -- coefficient-wise, rescale, basis-extension, key-switch MAC
// and automorphism kernels for the gfx950 RNS-CKKS backend.
//
// Every kernel here is HBM-bound integer work (no MFMA).  Grid shape: x covers
// the N coefficients of one limb (2 coefficients per thread, 16-B accesses),
// y covers the (comp, limb, image) rows.  Operands that are shared by the
// whole batch (plaintexts, LT diagonals, evaluation keys) are passed with
// batch_stride = 0 and are read once per row from L2.
#include <type_traits>

#include "common.h"
#include "launch.h"
#include "ntt2s_rows.h"
#include "tensor_sum.h"

namespace {

// the workgroup size of every kernel in this file (launch_bounds and launches:
// 256).  As a constant, not blockDim.x: HIP reads blockDim.x from the
// dispatch's implicit arguments (the remainder for a partial last block) with
// a 16-bit vector load and waits for it before any address is formed
constexpr int kBlk = 256;

// ks_mac: digits per load chunk (4 -> 2: 84 -> 62 VGPRs, 5 -> 8 waves per
// SIMD; ks_mac 104.3 -> 96.6 us per launch, profiles/r03z_ks_mac_chunk_ab.txt)
constexpr int KS_CH = 2;
// lt_bsgs_kernel8: minimum waves per SIMD (VGPR budget 512 / this); a macro: used inside an attribute
#define LT_WAVES8 4
// images per lt_bsgs workgroup that share one staged copy of the diagonals
constexpr int LT_IW = 4;
// images per lt_giant thread
constexpr int LT_GIANT_IB = 4;

// p[i] through a global-address-space pointer: for a pointer read from device
// memory (a plan's diagonal table) the compiler cannot infer the address
// space and emits a flat load, whose completion is only trackable with
// vmcnt(0) lgkmcnt(0) -- every product would wait for all loads in flight
__device__ __forceinline__ u64 gld(const u64* p, long long i) {
  return ((const __attribute__((address_space(1))) u64*)p)[i];
}

__device__ __forceinline__ long long row_off(const LimbSet& s, int c, int l, int b) {
  return c * s.comp_stride + arg_byte(s.pos, l) * s.limb_stride + b * s.batch_stride;
}

struct Scalars {
  u64 s[ORION_MAXLIMB];
  u64 ss[ORION_MAXLIMB];
};

template <int OP>
__global__ void __launch_bounds__(256) ew_kernel(LimbSet o, LimbSet a, LimbSet b, Scalars sc,
                                                 const DeviceTables* __restrict__ tb, int N) {
  const int row = blockIdx.y;
  const int bi = row % o.nbatch;
  const int r = row / o.nbatch;
  const int l = r % o.nlimb;
  const int c = r / o.nlimb;
  const int n = (blockIdx.x * kBlk + threadIdx.x) * 2;
  if (n >= N) return;
  const ModConst mc = tb->mc[arg_byte(o.mod, l)];
  const u64 q = mc.q;
  ulonglong2* po = (ulonglong2*)(o.p + row_off(o, c, l, bi) + n);
  const ulonglong2 x = *(const ulonglong2*)(a.p + row_off(a, c, l, bi) + n);
  ulonglong2 y = make_ulonglong2(0, 0), z;
  if (OP == EW_ADD || OP == EW_SUB || OP == EW_MUL || OP == EW_MULADD || OP == EW_SUBSCALE)
    y = *(const ulonglong2*)(b.p + row_off(b, c, l, bi) + n);
  switch (OP) {
    case EW_ADD: z.x = add_mod(x.x, y.x, q); z.y = add_mod(x.y, y.y, q); break;
    case EW_SUB: z.x = sub_mod(x.x, y.x, q); z.y = sub_mod(x.y, y.y, q); break;
    case EW_MUL: z.x = mul_mod(x.x, y.x, mc); z.y = mul_mod(x.y, y.y, mc); break;
    case EW_MULADD: {
      const ulonglong2 w = *po;
      z.x = add_mod(w.x, mul_mod(x.x, y.x, mc), q);
      z.y = add_mod(w.y, mul_mod(x.y, y.y, mc), q);
      break;
    }
    case EW_NEG: z.x = x.x ? q - x.x : 0; z.y = x.y ? q - x.y : 0; break;
    case EW_SCALE: z.x = shoup_mul(x.x, sc.s[l], sc.ss[l], q); z.y = shoup_mul(x.y, sc.s[l], sc.ss[l], q); break;
    case EW_ADDC: z.x = add_mod(x.x, sc.s[l], q); z.y = add_mod(x.y, sc.s[l], q); break;
    case EW_SUBSCALE:
      z.x = shoup_mul(sub_mod(x.x, y.x, q), sc.s[l], sc.ss[l], q);
      z.y = shoup_mul(sub_mod(x.y, y.y, q), sc.s[l], sc.ss[l], q);
      break;
    case EW_COPY: z = x; break;
    case EW_SPLIT24:
      z = mc.bar_k <= 48                 ? make_ulonglong2(split24(x.x), split24(x.y))
          : mc.bar_k <= 60 ? make_ulonglong2(split30(x.x), split30(x.y))
                                         : x;
      break;
    case EW_ADDSCALE: {
      const ulonglong2 w = *po;
      z.x = add_mod(w.x, shoup_mul(x.x, sc.s[l], sc.ss[l], q), q);
      z.y = add_mod(w.y, shoup_mul(x.y, sc.s[l], sc.ss[l], q), q);
      break;
    }
  }
  *po = z;
}

// Complex packing (OrionHipPackComplex / OrionHipUnpackComplex).  I = NTT of
// X^(N/2) is w4 = psi^(N/2) on the first half of a limb and -w4 on the second
// (the forward NTT's output order puts psi^((2 br(j) + 1) N/2) at j, and
// br(j) is odd exactly for j >= N/2), so it travels as one Shoup constant per
// limb in the kernel arguments (sc.s, sc.ss) and no table is read.  Grid as
// ew_kernel's: a thread's two coefficients lie in one half (N/2 is even).
//
// pack: o = a + I b on the images bi < npair; the images from npair on have
// no partner and are copied (OrionHipBootstrapPacked's lone image)
__global__ void __launch_bounds__(256) pack_complex_kernel(LimbSet o, LimbSet a, LimbSet b, Scalars sc, int npair,
                                                           const DeviceTables* __restrict__ tb, int N) {
  const int row = blockIdx.y;
  const int bi = row % o.nbatch;
  const int r = row / o.nbatch;
  const int l = r % o.nlimb;
  const int c = r / o.nlimb;
  const int n = (blockIdx.x * kBlk + threadIdx.x) * 2;
  if (n >= N) return;
  const u64 q = tb->mc[arg_byte(o.mod, l)].q;
  ulonglong2 z = *(const ulonglong2*)(a.p + row_off(a, c, l, bi) + n);
  if (bi < npair) {
    const ulonglong2 y = *(const ulonglong2*)(b.p + row_off(b, c, l, bi) + n);
    const u64 w = sc.s[l], ws = sc.ss[l];
    const u64 t0 = shoup_mul(y.x, w, ws, q), t1 = shoup_mul(y.y, w, ws, q);
    if (n < N / 2) {
      z.x = add_mod(z.x, t0, q);
      z.y = add_mod(z.y, t1, q);
    } else {
      z.x = sub_mod(z.x, t0, q);
      z.y = sub_mod(z.y, t1, q);
    }
  }
  *(ulonglong2*)(o.p + row_off(o, c, l, bi) + n) = z;
}

// unpack: with y = conj x, re = x + y and im = I (y - x) = -i (x - conj x);
// im is written for the images bi < nim only (the lone image has none).
// Rows over x's (comp, limb, image); re and im have their own geometry
__global__ void __launch_bounds__(256) unpack_complex_kernel(LimbSet re, LimbSet im, LimbSet x, LimbSet y, Scalars sc,
                                                             int nim, const DeviceTables* __restrict__ tb, int N) {
  const int row = blockIdx.y;
  const int bi = row % x.nbatch;
  const int r = row / x.nbatch;
  const int l = r % x.nlimb;
  const int c = r / x.nlimb;
  const int n = (blockIdx.x * kBlk + threadIdx.x) * 2;
  if (n >= N) return;
  const u64 q = tb->mc[arg_byte(x.mod, l)].q;
  const ulonglong2 u = *(const ulonglong2*)(x.p + row_off(x, c, l, bi) + n);
  const ulonglong2 v = *(const ulonglong2*)(y.p + row_off(y, c, l, bi) + n);
  *(ulonglong2*)(re.p + row_off(re, c, l, bi) + n) = make_ulonglong2(add_mod(u.x, v.x, q), add_mod(u.y, v.y, q));
  if (bi >= nim) return;
  const u64 w = sc.s[l], ws = sc.ss[l];
  // -w4 d = w4 (-d): the second half multiplies x - y
  const bool lo = n < N / 2;
  const u64 d0 = lo ? sub_mod(v.x, u.x, q) : sub_mod(u.x, v.x, q);
  const u64 d1 = lo ? sub_mod(v.y, u.y, q) : sub_mod(u.y, v.y, q);
  *(ulonglong2*)(im.p + row_off(im, c, l, bi) + n) = make_ulonglong2(shoup_mul(d0, w, ws, q), shoup_mul(d1, w, ws, q));
}

// Monomial packing (OrionHipPackMonomials / OrionHipUnpackMonomials).  M_i =
// NTT of X^i is the i-th power of M_1 coefficient by coefficient, so a thread
// carries the running product f_i = f_(i-1) m of its two coefficients of m =
// M_1 (pack) or M_-1 (unpack) and reads no table of powers.  Every product is
// fully reduced before it is added or stored, so g is bounded by nothing.
// Rows over (comp, limb, group k); group k holds the images k + i h, i < g,
// that exist (k + i h < B).  m: the factor's row per limb (one component, one
// image), on the limbs of o / x.
//
// pack: o_k = sum_i M_i a_(k + i h), h = o.nbatch, B = a.nbatch
__global__ void __launch_bounds__(256) mono_pack_kernel(LimbSet o, LimbSet a, LimbSet m, int g,
                                                        const DeviceTables* __restrict__ tb, int N) {
  const int row = blockIdx.y;
  const int h = o.nbatch, B = a.nbatch;
  const int k = row % h;
  const int r = row / h;
  const int l = r % o.nlimb;
  const int c = r / o.nlimb;
  const int n = (blockIdx.x * kBlk + threadIdx.x) * 2;
  if (n >= N) return;
  const ModConst mc = tb->mc[arg_byte(o.mod, l)];
  const u64 q = mc.q;
  ulonglong2 z = *(const ulonglong2*)(a.p + row_off(a, c, l, k) + n);
  if (k + h < B && g > 1) {
    const ulonglong2 w = *(const ulonglong2*)(m.p + row_off(m, 0, l, 0) + n);
    ulonglong2 f = w;
    for (int i = 1;;) {
      const ulonglong2 x = *(const ulonglong2*)(a.p + row_off(a, c, l, k + i * h) + n);
      z.x = add_mod(z.x, mul_mod(f.x, x.x, mc), q);
      z.y = add_mod(z.y, mul_mod(f.y, x.y, mc), q);
      if (++i >= g || k + i * h >= B) break;
      f.x = mul_mod(f.x, w.x, mc);
      f.y = mul_mod(f.y, w.y, mc);
    }
  }
  *(ulonglong2*)(o.p + row_off(o, c, l, k) + n) = z;
}

// unpack: o_(k + i h) = M_-i x_k, h = x.nbatch, B = o.nbatch: each source row
// is read once and its (at most g) images written
__global__ void __launch_bounds__(256) mono_unpack_kernel(LimbSet o, LimbSet x, LimbSet m, int g,
                                                          const DeviceTables* __restrict__ tb, int N) {
  const int row = blockIdx.y;
  const int h = x.nbatch, B = o.nbatch;
  const int k = row % h;
  const int r = row / h;
  const int l = r % x.nlimb;
  const int c = r / x.nlimb;
  const int n = (blockIdx.x * kBlk + threadIdx.x) * 2;
  if (n >= N) return;
  const ModConst mc = tb->mc[arg_byte(x.mod, l)];
  const ulonglong2 u = *(const ulonglong2*)(x.p + row_off(x, c, l, k) + n);
  *(ulonglong2*)(o.p + row_off(o, c, l, k) + n) = u;
  if (k + h < B && g > 1) {
    const ulonglong2 w = *(const ulonglong2*)(m.p + row_off(m, 0, l, 0) + n);
    ulonglong2 f = w;
    for (int i = 1;;) {
      *(ulonglong2*)(o.p + row_off(o, c, l, k + i * h) + n) =
          make_ulonglong2(mul_mod(f.x, u.x, mc), mul_mod(f.y, u.y, mc));
      if (++i >= g || k + i * h >= B) break;
      f.x = mul_mod(f.x, w.x, mc);
      f.y = mul_mod(f.y, w.y, mc);
    }
  }
}

// whole images gathered into a batch ciphertext: image i of the launch
// (i < ORION_MAXGATHER) is copied from T.src[i] to dst + i*N, limb planes
// (c, l), c < 2, l < nlimb, dst plane (c, l) at c*d_comp + l*d_limb.
// Grid: x covers the N coefficients (kGatherU 16-B accesses per thread, all
// loads issued before the first store; N is a multiple of a workgroup's
// share, so there is no tail), y = image (neighbouring workgroups write
// neighbouring memory), z = plane c*nlimb + l.
constexpr int kGatherU = 4;
__global__ void __launch_bounds__(256) gather_images_kernel(u64* __restrict__ dst, long long d_comp, long long d_limb,
                                                            int nlimb, GatherTable T, int N) {
  const int i = blockIdx.y;
  const int pl = blockIdx.z;
  const int c = pl >= nlimb ? 1 : 0;
  const int l = pl - c * nlimb;
  const GatherSrc s = T.src[i];  // wave-uniform: scalar loads from the kernel arguments
  // 16-byte accesses: every plane base is 16-byte aligned -- pool buffers are
  // hipMalloc allocations (256-byte aligned) and every offset (component,
  // limb and image strides) is a multiple of N words = 8 N bytes, N even
  const ulonglong2* ps = (const ulonglong2*)(s.p + c * s.comp_stride + l * s.limb_stride);
  ulonglong2* pd = (ulonglong2*)(dst + c * d_comp + l * d_limb + (long long)i * N);
  const int k0 = blockIdx.x * (kBlk * kGatherU) + threadIdx.x;
  ulonglong2 v[kGatherU];
#pragma unroll
  for (int u = 0; u < kGatherU; ++u) v[u] = ps[k0 + u * kBlk];
#pragma unroll
  for (int u = 0; u < kGatherU; ++u) pd[k0 + u * kBlk] = v[u];
}

// ct x ct tensor: d0 = a0 b0, d1 = a0 b1 + a1 b0, d2 = a1 b1  (a, b: 2 comps; d: 3 comps)
__global__ void __launch_bounds__(256) tensor_kernel(LimbSet d, LimbSet a, LimbSet b,
                                                     const DeviceTables* __restrict__ tb, int N) {
  const int row = blockIdx.y;
  const int bi = row % d.nbatch;
  const int l = row / d.nbatch;
  const int n = (blockIdx.x * kBlk + threadIdx.x) * 2;
  if (n >= N) return;
  const ModConst mc = tb->mc[arg_byte(d.mod, l)];
  const u64 q = mc.q;
  const ulonglong2 a0 = *(const ulonglong2*)(a.p + row_off(a, 0, l, bi) + n);
  const ulonglong2 a1 = *(const ulonglong2*)(a.p + row_off(a, 1, l, bi) + n);
  const ulonglong2 b0 = *(const ulonglong2*)(b.p + row_off(b, 0, l, bi) + n);
  const ulonglong2 b1 = *(const ulonglong2*)(b.p + row_off(b, 1, l, bi) + n);
  ulonglong2 d0, d1, d2;
  d0.x = mul_mod(a0.x, b0.x, mc); d0.y = mul_mod(a0.y, b0.y, mc);
  d1.x = add_mod(mul_mod(a0.x, b1.x, mc), mul_mod(a1.x, b0.x, mc), q);
  d1.y = add_mod(mul_mod(a0.y, b1.y, mc), mul_mod(a1.y, b0.y, mc), q);
  d2.x = mul_mod(a1.x, b1.x, mc); d2.y = mul_mod(a1.y, b1.y, mc);
  *(ulonglong2*)(d.p + row_off(d, 0, l, bi) + n) = d0;
  *(ulonglong2*)(d.p + row_off(d, 1, l, bi) + n) = d1;
  *(ulonglong2*)(d.p + row_off(d, 2, l, bi) + n) = d2;
}

// A sum of ct x ct tensors (tensor_sum.h): d0 = sum a0 b0, d1 = sum (a0 b1 +
// a1 b0), d2 = sum a1 b1 over the T.n pairs of the launch; ACC: added to the d
// an earlier launch wrote.  tensor_kernel's layout (two coefficients per
// thread, 16-B accesses, grid y = (limb, image)); the pair table is read from
// the kernel arguments with wave-uniform indices (scalar loads).  Memory-bound:
// per limb-image 8 N (4 n + 3) bytes, 8 N (2 n + 3) when every pair is a
// square.  The loads of two pairs are issued before the first product; the
// squares (two rows each, not four) have a loop of their own, so that no load
// sits under a per-pair branch.  The products are summed unreduced and reduced
// every tsum::interval pairs (once per launch on moduli of at most 52 bits).
struct TsumRows {
  ulonglong2 a0, a1, b0, b1;
};
template <bool SQ>
__device__ __forceinline__ TsumRows tsum_load(const tsum::Pair& p, int l, int bi, int n) {
  TsumRows r;
  const u64* pa = p.a + l * p.a_limb + bi * p.a_batch + n;
  r.a0 = *(const ulonglong2*)pa;
  r.a1 = *(const ulonglong2*)(pa + p.a_comp);
  if (!SQ) {
    const u64* pb = p.b + l * p.b_limb + bi * p.b_batch + n;
    r.b0 = *(const ulonglong2*)pb;
    r.b1 = *(const ulonglong2*)(pb + p.b_comp);
  }
  return r;
}
template <bool SQ>
__device__ __forceinline__ void tsum_mac(tsum::Acc3& sx, tsum::Acc3& sy, const TsumRows& r) {
  if (SQ) {
    tsum::mac_square(sx, r.a0.x, r.a1.x);
    tsum::mac_square(sy, r.a0.y, r.a1.y);
  } else {
    tsum::mac_pair(sx, r.a0.x, r.a1.x, r.b0.x, r.b1.x);
    tsum::mac_pair(sy, r.a0.y, r.a1.y, r.b0.y, r.b1.y);
  }
}
struct TsumState {
  tsum::Acc3 sx, sy;  // the unreduced sums of the thread's two coefficients
  u64 x0, x1, x2, y0, y1, y2;  // the reduced sums so far: (d0, d1, d2) of either coefficient
  int held;                    // pairs in sx, sy
};
__device__ __forceinline__ void tsum_flush(TsumState& s, const tsum::Mod& mc) {
  tsum::flush(s.sx, mc, s.x0, s.x1, s.x2);
  tsum::flush(s.sy, mc, s.y0, s.y1, s.y2);
  s.held = 0;
}
// the pairs [first, end) of the table, two at a time and an odd one last
template <bool SQ>
__device__ __forceinline__ void tsum_run(TsumState& s, const tsum::Table& T, int first, int end, int l, int bi, int n,
                                         const tsum::Mod& mc) {
  int i = first;
  for (; i + 1 < end; i += 2) {
    const TsumRows r0 = tsum_load<SQ>(T.pr[i], l, bi, n), r1 = tsum_load<SQ>(T.pr[i + 1], l, bi, n);
    if (tsum::due(s.held, 2, mc)) tsum_flush(s, mc);
    tsum_mac<SQ>(s.sx, s.sy, r0);
    tsum_mac<SQ>(s.sx, s.sy, r1);
    s.held += 2;
  }
  if (i < end) {
    const TsumRows r0 = tsum_load<SQ>(T.pr[i], l, bi, n);
    if (tsum::due(s.held, 1, mc)) tsum_flush(s, mc);
    tsum_mac<SQ>(s.sx, s.sy, r0);
    s.held += 1;
  }
}
template <bool ACC>
__global__ void __launch_bounds__(256) tensor_sum_kernel(LimbSet d, tsum::Table T,
                                                         const DeviceTables* __restrict__ tb, int N) {
  const int row = blockIdx.y;
  const int bi = row % d.nbatch;
  const int l = row / d.nbatch;
  const int n = (blockIdx.x * kBlk + threadIdx.x) * 2;
  if (n >= N) return;
  // (read through the pointer: a copy of the whole ModConst would live in scratch)
  const tsum::Mod mc = tsum::mod_of(tb->mc[arg_byte(d.mod, l)]);
  ulonglong2* p0 = (ulonglong2*)(d.p + row_off(d, 0, l, bi) + n);
  ulonglong2* p1 = (ulonglong2*)(d.p + row_off(d, 1, l, bi) + n);
  ulonglong2* p2 = (ulonglong2*)(d.p + row_off(d, 2, l, bi) + n);
  TsumState s;
  tsum::zero(s.sx);
  tsum::zero(s.sy);
  s.held = 0;
  s.x0 = s.x1 = s.x2 = s.y0 = s.y1 = s.y2 = 0;
  if (ACC) {
    const ulonglong2 e0 = *p0, e1 = *p1, e2 = *p2;
    s.x0 = e0.x, s.y0 = e0.y, s.x1 = e1.x, s.y1 = e1.y, s.x2 = e2.x, s.y2 = e2.y;
  }
  tsum_run<true>(s, T, 0, T.nsq, l, bi, n, mc);
  tsum_run<false>(s, T, T.nsq, T.n, l, bi, n, mc);
  tsum_flush(s, mc);
  *p0 = make_ulonglong2(s.x0, s.y0);
  *p1 = make_ulonglong2(s.x1, s.y1);
  *p2 = make_ulonglong2(s.x2, s.y2);
}

// Exact basis extension (Lattigo ModUpExact restated; the
// source-side math is bext_prep in common.h, the target side bext_target_sel).
// in: ns source limbs (coefficient domain), out: nt target limbs.  Two
// coefficients per thread (16-B accesses).
template <int MS>
__global__ void __launch_bounds__(256) basis_ext_kernel(LimbSet out, LimbSet in, const BasisExtTable* __restrict__ T,
                                                        int N, int tchunk) {
  const int row = blockIdx.y;  // (comp, image)
  const int bi = row % out.nbatch;
  const int c = row / out.nbatch;
  const int n = (blockIdx.x * kBlk + threadIdx.x) * 2;
  if (n >= N) return;
  const int ns = T->ns, nt = T->nt;
  u64 x0[MS], x1[MS], y0[MS], y1[MS];
#pragma unroll
  for (int i = 0; i < MS; ++i) {
    if (i >= ns) break;
    const ulonglong2 v = *(const ulonglong2*)(in.p + row_off(in, c, i, bi) + n);
    x0[i] = v.x;
    x1[i] = v.y;
  }
  const u64 v0 = bext_prep<MS>(T, x0, y0), v1 = bext_prep<MS>(T, x1, y1);
  const int tend = min(nt, (int)(blockIdx.z + 1) * tchunk);
  for (int t = blockIdx.z * tchunk; t < tend; ++t) {
    u64 o0, o1;
    bext_target2<MS>(T->tgt + t, ns, y0, v0, y1, v1, o0, o1);
    *(ulonglong2*)(out.p + row_off(out, c, t, bi) + n) = make_ulonglong2(o0, o1);
  }
}

// The ModDown's extension with the rescale that follows it folded in (common.h
// BextRescaleTable).  in: limb 0 = limb l of x, limbs 1..ns = its P limbs, all
// in the coefficient domain; out: the l limbs e_i + (P mod q_i) t_i.  y, v and
// every e_j are formed as basis_ext_kernel forms them; the pivot e_l stays in
// registers (each target chunk forms it again: one more target per chunk).
template <int MS>
__global__ void __launch_bounds__(256) basis_ext_rescale_kernel(LimbSet out, LimbSet in,
                                                                const BextRescaleTable* __restrict__ W, int N,
                                                                int tchunk) {
  const int row = blockIdx.y;  // (comp, image)
  const int bi = row % out.nbatch;
  const int c = row / out.nbatch;
  const int n = (blockIdx.x * kBlk + threadIdx.x) * 2;
  if (n >= N) return;
  const BasisExtTable* __restrict__ T = &W->bx;
  const int ns = T->ns, piv = W->piv;
  u64 x0[MS], x1[MS], y0[MS], y1[MS];
#pragma unroll
  for (int i = 0; i < MS; ++i) {
    if (i >= ns) break;
    const ulonglong2 v = *(const ulonglong2*)(in.p + row_off(in, c, 1 + i, bi) + n);
    x0[i] = v.x;
    x1[i] = v.y;
  }
  const u64 v0 = bext_prep<MS>(T, x0, y0), v1 = bext_prep<MS>(T, x1, y1);
  u64 r0, r1;
  {
    const ulonglong2 xl = *(const ulonglong2*)(in.p + row_off(in, c, 0, bi) + n);
    const u64 ql = T->tgt[piv].q, pinv = W->pinv, pinvs = W->pinvs, h = W->h;
    u64 e0, e1;
    bext_target2<MS>(T->tgt + piv, ns, y0, v0, y1, v1, e0, e1);
    r0 = add_mod(shoup_mul(sub_mod(xl.x, e0, ql), pinv, pinvs, ql), h, ql);
    r1 = add_mod(shoup_mul(sub_mod(xl.y, e1, ql), pinv, pinvs, ql), h, ql);
  }
  const int tend = min(piv, (int)(blockIdx.z + 1) * tchunk);
  for (int t = blockIdx.z * tchunk; t < tend; ++t) {
    u64 o0, o1;
    bext_target2<MS>(T->tgt + t, ns, y0, v0, y1, v1, o0, o1);
    const BextRescaleTarget* __restrict__ R = W->rt + t;
    const u64 q = T->tgt[t].q, pq = R->pq, pqs = R->pqs, hm = R->hm, ones = R->ones;
    const u64 t0 = sub_mod(shoup_mul(r0, 1, ones, q), hm, q), t1 = sub_mod(shoup_mul(r1, 1, ones, q), hm, q);
    o0 = add_mod(o0, shoup_mul(t0, pq, pqs, q), q);
    o1 = add_mod(o1, shoup_mul(t1, pq, pqs, q), q);
    *(ulonglong2*)(out.p + row_off(out, c, t, bi) + n) = make_ulonglong2(o0, o1);
  }
}

// ModUp of every digit of a decomposition in one launch (small launches:
// one image at N = 2^13..2^15 gives a per-digit basis_ext only 16..64
// workgroups).  Row = (comp c, digit i, image); blockIdx.z = a chunk of the
// nqp QP positions.  Digit i's own positions [iK, iK + ns) are not written
// (consumers read the own limbs from the NTT-domain input, and the NTT that
// follows covers only the target positions).
// D: comps c*beta + i, limb j at position j; Ts[i] = digit i's table.
template <int MS>
__global__ void __launch_bounds__(256) modup_all_kernel(LimbSet D, LimbSet in, const BasisExtTable* __restrict__ Ts,
                                                        int beta, int K, int nqp, int N, int tchunk) {
  const int row = blockIdx.y;
  const int bi = row % D.nbatch;
  const int r = row / D.nbatch;
  const int i = r % beta;
  const int c = r / beta;
  const int n = (blockIdx.x * kBlk + threadIdx.x) * 2;
  if (n >= N) return;
  const BasisExtTable* __restrict__ T = Ts + i;
  const int ns = T->ns, lo = i * K;
  u64 x0[MS], x1[MS], y0[MS], y1[MS];
#pragma unroll
  for (int s = 0; s < MS; ++s) {
    if (s >= ns) break;
    const ulonglong2 v = *(const ulonglong2*)(in.p + row_off(in, c, lo + s, bi) + n);
    x0[s] = v.x;
    x1[s] = v.y;
  }
  const u64 v0 = bext_prep<MS>(T, x0, y0), v1 = bext_prep<MS>(T, x1, y1);
  // D's positions are the identity (checked at launch): limb j of the row is
  // limb_stride past limb j - 1, so the loop carries one pointer and one
  // target record instead of re-deriving both from (j, pos[j], dst_mod[t])
  // own limbs [lo, lo + ns) are not written: every consumer reads them from
  // the NTT-domain input of the decomposition; positions below them are
  // targets 0.., positions above them targets lo..
  const int j0 = blockIdx.z * tchunk, jend = min(nqp, j0 + tchunk);
  u64* const dst = D.p + row_off(D, c * beta + i, 0, bi) + n;
  auto targets = [&](int ja, int jb, int toff) {
    u64* op = dst + (long long)ja * D.limb_stride;
    const BextTarget* __restrict__ R = T->tgt + (ja - toff);
    for (int j = ja; j < jb; ++j, ++R, op += D.limb_stride) {
      u64 o0, o1;
      bext_target2<MS>(R, ns, y0, v0, y1, v1, o0, o1);
      *(ulonglong2*)op = make_ulonglong2(o0, o1);
    }
  };
  targets(j0, min(jend, lo), 0);
  targets(max(j0, lo + ns), jend, ns);
}

// Gadget-product MAC over G groups (one evaluation key per group):
//   out_g,c[j] = add0_g[j]*(c == 0) + sum_i D_g,i[j] * key_g[i][c][mod_j]   (c = 0, 1)
// D: comps = digits, limbs = QP positions; group g's digits start at
// D.p + g*d_gstride (d_gstride = 0: one decomposition shared by every group,
// the hoisted baby steps of a BSGS transform).  If own.p is set, digit i's
// own Q limbs (l / K == i) are read from `own` (the NTT-domain input of the
// decomposition, group stride own_gstride) instead of D, so the decomposition
// never copies them.  out comps 0/1 of group g at out.p + g*out_gstride.
// key layout [digit][2][klvl+1+K][N] (common.h key_pos).
template <bool ROWS, bool FR = false, bool PRE = false>
__device__ __forceinline__ void ks_mac_body(LimbSet& out, LimbSet& D, LimbSet& own, MacGroups& G, int beta,
                                            const DeviceTables* __restrict__ tb, int N, u64* lds) {
  const int row = blockIdx.y;
  const int bi = row % out.nbatch;
  const int r = row / out.nbatch;
  const int l = r % out.nlimb;
  const int g = r / out.nlimb;
  const int n = (blockIdx.x * kBlk + threadIdx.x) * 2;
  if (n >= N) return;
  const int m = arg_byte(out.mod, l);
  const ModConst mc = tb->mc[m];
  const u64 q = mc.q;
  const u64* key = G.key[g];
  const u64* dp = D.p + g * G.d_gstride;
  const int owndigit = (own.p && l < own.nlimb) ? l / G.K : -1;
  u64* op = out.p + g * G.out_gstride;
  ulonglong2 r0 = make_ulonglong2(0, 0), r1 = make_ulonglong2(0, 0);
  if (G.add_nq > 0) {
    if (l < G.add_nq) {
      const long long ao = g * G.add_gstride + row_off(out, 0, l, bi) + n;
      const u64 s = G.add_s[l], ss = G.add_ss[l];
      const ulonglong2 a = *(const ulonglong2*)(G.add0 + ao);
      r0 = make_ulonglong2(shoup_mul(a.x, s, ss, q), shoup_mul(a.y, s, ss, q));
      if (G.add1) {
        const ulonglong2 b = *(const ulonglong2*)(G.add1 + ao);
        r1 = make_ulonglong2(shoup_mul(b.x, s, ss, q), shoup_mul(b.y, s, ss, q));
      }
    }
  } else if (G.add0) {
    r0 = *(const ulonglong2*)(G.add0 + g * G.add_gstride + row_off(out, 0, l, bi) + n);
  }
  const int kl = G.klvl[g];
  const long long kstride = (long long)(kl + 1 + G.K) * N;
  const u64* kp = key + (long long)key_pos(m, G.L, kl) * N + n;
  // FR: the decomposition's forward NTT stopped after its columns pass; rows
  // 2 bx and 2 bx + 1 of every non-own digit's row set go through the
  // forward rows pass here, 4 rows at a time (groups past the last row keep
  // the barriers on their own LDS row), into fr = [digit][2 rows][256]
  [[maybe_unused]] const u64* fr = nullptr;
  // FR with at most 4 digits (the batch-1 key switches): the key words and the
  // own digit's words are loaded before the rows pass, so their latency
  // overlaps it instead of following it
  // (PRE: an instantiation of its own, so the other launches keep their registers)
  constexpr bool pre = FR && PRE;
  [[maybe_unused]] ulonglong2 pkb[4], pka[4], pown = make_ulonglong2(0, 0);
  if constexpr (pre) {
    {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (u < beta) {
          pkb[u] = *(const ulonglong2*)(kp + (2 * u + 0) * kstride);
          pka[u] = *(const ulonglong2*)(kp + (2 * u + 1) * kstride);
        }
      }
      if (owndigit >= 0) pown = *(const ulonglong2*)(own.p + g * G.own_gstride + row_off(own, 0, l, bi) + n);
    }
  }
  // ... and a P limb's inverse-rows twiddles (the ROWS epilogue below), raw
  [[maybe_unused]] ulonglong2 itw[12];
  if constexpr (pre && ROWS) {
    if (l >= G.rows_from) {  // (block-uniform)
      const int t = threadIdx.x, rr = t >> 6, kk = t & 63, row = 2 * blockIdx.x + (rr & 1);
      auto tws = [&](const auto& ar, __amdgpu_buffer_rsrc_t tw) {
        using A = std::decay_t<decltype(ar)>;
        typename A::W wa[4], wb[4], wc[4];
        if (G.logN == 15)
          inv_rows4_tw<A, 15>(row, kk, ar, tw, wa, wb, wc);
        else
          inv_rows4_tw<A, 16>(row, kk, ar, tw, wa, wb, wc);
#pragma unroll
        for (int st = 0; st < 4; ++st) itw[st] = w_raw(wa[st]), itw[4 + st] = w_raw(wb[st]), itw[8 + st] = w_raw(wc[st]);
      };
      if (mc.f64)
        tws(F64Arith(mc), twr_s(tb->inv_d[m], 8 * N));
      else
        tws(IntArith(mc), twr_s(tb->inv[m], 16 * N));
    }
  }
  if constexpr (FR) {
    u64* const frw = lds + 4 * 256;
    const int t = threadIdx.x, rr = t >> 6, kk = t & 63;
    for (int q0 = 0; q0 < 2 * beta; q0 += 4) {  // (uniform)
      if (q0 > 0) __syncthreads();  // the previous round's exchange reads done
      const int q = q0 + rr, i = q >> 1, rw = 2 * blockIdx.x + (q & 1);
      const bool live = q < 2 * beta && i != owndigit;
      const u64* const src = dp + row_off(D, live ? i : 0, l, bi) + ((long long)rw << 8);
      auto rows = [&](const auto& ar, __amdgpu_buffer_rsrc_t tw) {
        using A = std::decay_t<decltype(ar)>;
        typename A::T x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = from_bits<typename A::T>(live ? src[kk + 64 * k] : 0);
        if (G.logN == 15)
          fwd_rows4_core<A, 15>(x, rw, kk, ar, tw, lds + rr * 256);
        else
          fwd_rows4_core<A, 16>(x, rw, kk, ar, tw, lds + rr * 256);
        if (live) {
#pragma unroll
          for (int k = 0; k < 4; ++k) frw[q * 256 + 4 * kk + k] = ar.final_fwd(x[k]);
        }
      };
      if (mc.f64)
        rows(F64Arith(mc), twr_s(tb->fwd_d[m], 8 * N));
      else
        rows(IntArith(mc), twr_s(tb->fwd[m], 16 * N));
    }
    __syncthreads();  // fr complete
    fr = frw;
  }
  // one reduction per chunk.  (Once per output on moduli below 2^52 keeps the
  // accumulators live across the digit loop: 84 -> 102 VGPRs, 5 -> 4 waves per
  // SIMD, ks_mac 1.31 -> 1.48 ms per LoLA step, profiles/r03n_ab.txt; LoLA's
  // decompositions have at most 3 digits, so there is one chunk anyway)
  MacAcc s0x, s0y, s1x, s1y;
  mac_zero(s0x), mac_zero(s0y), mac_zero(s1x), mac_zero(s1y);
  if constexpr (pre) {
    {  // the preloaded words, in chunks of 2 digits as below
      const int lt = 2 * (int)threadIdx.x;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (u < beta) {
          const ulonglong2 d = u == owndigit ? pown
                                             : make_ulonglong2(fr[(2 * u + (lt >> 8)) * 256 + (lt & 255)],
                                                               fr[(2 * u + (lt >> 8)) * 256 + (lt & 255) + 1]);
          mac_add(s0x, d.x, pkb[u].x);
          mac_add(s0y, d.y, pkb[u].y);
          mac_add(s1x, d.x, pka[u].x);
          mac_add(s1y, d.y, pka[u].y);
        }
        if ((u & 1) && u - 1 < beta) {
          r0.x = add_mod(r0.x, mac_reduce(s0x, mc), q);
          r0.y = add_mod(r0.y, mac_reduce(s0y, mc), q);
          r1.x = add_mod(r1.x, mac_reduce(s1x, mc), q);
          r1.y = add_mod(r1.y, mac_reduce(s1y, mc), q);
          mac_zero(s0x), mac_zero(s0y), mac_zero(s1x), mac_zero(s1y);
        }
      }
    }
  }
  for (int i0 = 0; i0 < (pre ? 0 : beta); i0 += KS_CH) {  // chunks of KS_CH digits: 3 KS_CH loads in flight
    ulonglong2 d[KS_CH], kb[KS_CH], ka[KS_CH];
#pragma unroll
    for (int u = 0; u < KS_CH; ++u) {
      const int i = i0 + u;
      if (i < beta) {
        if (i == owndigit) {
          d[u] = *(const ulonglong2*)(own.p + g * G.own_gstride + row_off(own, 0, l, bi) + n);
        } else if constexpr (FR) {  // this thread's 2 coefficients: local 2t, 2t + 1 of the block's 2 rows
          const int lt = 2 * (int)threadIdx.x;
          d[u] = make_ulonglong2(fr[(2 * i + (lt >> 8)) * 256 + (lt & 255)], fr[(2 * i + (lt >> 8)) * 256 + (lt & 255) + 1]);
        } else {
          d[u] = *(const ulonglong2*)(dp + row_off(D, i, l, bi) + n);
        }
        kb[u] = *(const ulonglong2*)(kp + (2 * i + 0) * kstride);
        ka[u] = *(const ulonglong2*)(kp + (2 * i + 1) * kstride);
      }
    }
#pragma unroll
    for (int u = 0; u < KS_CH; ++u) {
      if (i0 + u < beta) {
        mac_add(s0x, d[u].x, kb[u].x);
        mac_add(s0y, d[u].y, kb[u].y);
        mac_add(s1x, d[u].x, ka[u].x);
        mac_add(s1y, d[u].y, ka[u].y);
      }
    }
    r0.x = add_mod(r0.x, mac_reduce(s0x, mc), q);
    r0.y = add_mod(r0.y, mac_reduce(s0y, mc), q);
    r1.x = add_mod(r1.x, mac_reduce(s1x, mc), q);
    r1.y = add_mod(r1.y, mac_reduce(s1y, mc), q);
    mac_zero(s0x), mac_zero(s0y), mac_zero(s1x), mac_zero(s1y);
  }
  if constexpr (ROWS) {
    if (l >= G.rows_from) {  // (block-uniform) a P limb: the ModDown INTT's rows pass, here
      // the block's 512 coefficients are rows 2 bx and 2 bx + 1 of both
      // components: staged in LDS as 4 rows (comp-major), then thread
      // (rr, kk) runs the radix-4 inverse rows steps on elements 4 kk .. 4 kk + 3
      const int t = threadIdx.x, lrw = (2 * t) >> 8, col = (2 * t) & 255;
      lds[lrw * 256 + col] = r0.x, lds[lrw * 256 + col + 1] = r0.y;
      lds[(2 + lrw) * 256 + col] = r1.x, lds[(2 + lrw) * 256 + col + 1] = r1.y;
      __syncthreads();
      const int rr = t >> 6, kk = t & 63, row = 2 * blockIdx.x + (rr & 1);
      u64* const lr = lds + rr * 256;
      u64* const mid = op + row_off(out, rr >> 1, l, bi) + (row << 8);
      auto rows = [&](const auto& ar, __amdgpu_buffer_rsrc_t tw) {
        using A = std::decay_t<decltype(ar)>;
        typename A::T x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = ar.from_u64(lr[4 * kk + i]);
        if constexpr (pre) {  // the twiddles fetched at the start
          typename A::W wa[4], wb[4], wc[4];
#pragma unroll
          for (int st = 0; st < 4; ++st)
            wa[st] = w_of<A>(itw[st]), wb[st] = w_of<A>(itw[4 + st]), wc[st] = w_of<A>(itw[8 + st]);
          inv_rows4_run<A>(x, kk, ar, wa, wb, wc, lr, mid);
        } else if (G.logN == 15) {
          inv_rows4_core<A, 15>(x, row, kk, ar, tw, lr, mid);
        } else {
          inv_rows4_core<A, 16>(x, row, kk, ar, tw, lr, mid);
        }
      };
      if (mc.f64)
        rows(F64Arith(mc), twr_s(tb->inv_d[m], 8 * N));
      else
        rows(IntArith(mc), twr_s(tb->inv[m], 16 * N));
      return;
    }
  }
  *(ulonglong2*)(op + row_off(out, 0, l, bi) + n) = r0;
  *(ulonglong2*)(op + row_off(out, 1, l, bi) + n) = r1;
}
__global__ void __launch_bounds__(256) ks_mac_kernel(LimbSet out, LimbSet D, LimbSet own, MacGroups G, int beta,
                                                     const DeviceTables* __restrict__ tb, int N) {
  ks_mac_body<false>(out, D, own, G, beta, tb, N, nullptr);
}
// the same, the P limbs' results through the INTT's rows pass (MacGroups.rows_from)
__global__ void __launch_bounds__(256) ks_mac_rows_kernel(LimbSet out, LimbSet D, LimbSet own, MacGroups G, int beta,
                                                          const DeviceTables* __restrict__ tb, int N) {
  __shared__ u64 lds[4 * 256];
  ks_mac_body<true>(out, D, own, G, beta, tb, N, lds);
}
// the same, and before the products the decomposition's forward rows pass
// (MacGroups.fwd_rows; dynamic LDS: (4 + 2 beta) rows of 256 words)
template <bool PRE>
__global__ void __launch_bounds__(256) ks_mac_full_kernel(LimbSet out, LimbSet D, LimbSet own, MacGroups G, int beta,
                                                          const DeviceTables* __restrict__ tb, int N) {
  extern __shared__ u64 lds_dyn[];
  ks_mac_body<true, true, PRE>(out, D, own, G, beta, tb, N, lds_dyn);
}

// Gadget products of one decomposition with many keys (hoisted rotations,
// Context::rotate_hoisted):
//   out_g,c[j] = P*add[j]*(c == 0) + sum_i D_i[j] * key_g[i][c][mod_j]   (c = 0, 1)
// for every key g of H.keys.  A thread owns two adjacent coefficients of one
// (limb, image) row: it loads the beta digit words once (digit i's own Q limbs
// from `own`, as ks_mac_body) and forms P*add once, then loops over the keys:
// 2 beta key words, the split MAC in chunks of KS_CH digits, both components
// stored.  ks_mac_kernel with the keys as groups reads the beta rows of D once
// per key.  HB: the digit slots held in registers (beta <= HB).  The results
// are ks_mac_kernel's bit for bit: both are exact mod q and fully reduced.
template <int HB>
__global__ void __launch_bounds__(256) ks_mac_hoisted_kernel(LimbSet out, LimbSet D, LimbSet own, LimbSet add,
                                                             MacHoist H, const DeviceTables* __restrict__ tb, int N) {
  const int row = blockIdx.y;
  const int bi = row % out.nbatch;
  const int l = row / out.nbatch;
  const int n = (blockIdx.x * kBlk + threadIdx.x) * 2;
  if (n >= N) return;
  const int m = arg_byte(out.mod, l);
  const ModConst mc = tb->mc[m];
  const u64 q = mc.q;
  const int beta = H.beta;
  const int owndigit = l < own.nlimb ? l / H.K : -1;
  ulonglong2 d[HB];
#pragma unroll
  for (int u = 0; u < HB; ++u) {
    if (u < beta)
      d[u] = u == owndigit ? *(const ulonglong2*)(own.p + row_off(own, 0, l, bi) + n)
                           : *(const ulonglong2*)(D.p + row_off(D, u, l, bi) + n);
  }
  ulonglong2 a0 = make_ulonglong2(0, 0);
  if (l < add.nlimb) {  // a Q limb: P * add (the P limbs get 0)
    const ulonglong2 a = *(const ulonglong2*)(add.p + row_off(add, 0, l, bi) + n);
    const u64 s = H.add_s[l], ss = H.add_ss[l];
    a0 = make_ulonglong2(shoup_mul(a.x, s, ss, q), shoup_mul(a.y, s, ss, q));
  }
  const long long o0 = row_off(out, 0, l, bi) + n, o1 = row_off(out, 1, l, bi) + n;
  for (int g = 0; g < H.keys.n; ++g) {  // (uniform)
    const int kl = H.keys.klvl[g];
    const long long kstride = (long long)(kl + 1 + H.K) * N;
    const u64* kp = H.keys.key[g] + (long long)key_pos(m, H.L, kl) * N + n;
    ulonglong2 r0 = a0, r1 = make_ulonglong2(0, 0);
#pragma unroll
    for (int i0 = 0; i0 < HB; i0 += KS_CH) {
      if (i0 < beta) {
        ulonglong2 kb[KS_CH], ka[KS_CH];
#pragma unroll
        for (int u = 0; u < KS_CH; ++u) {
          if (i0 + u < beta) {
            kb[u] = *(const ulonglong2*)(kp + (2 * (i0 + u) + 0) * kstride);
            ka[u] = *(const ulonglong2*)(kp + (2 * (i0 + u) + 1) * kstride);
          }
        }
        MacAcc s0x, s0y, s1x, s1y;
        mac_zero(s0x), mac_zero(s0y), mac_zero(s1x), mac_zero(s1y);
#pragma unroll
        for (int u = 0; u < KS_CH; ++u) {
          if (i0 + u < beta) {
            mac_add(s0x, d[i0 + u].x, kb[u].x);
            mac_add(s0y, d[i0 + u].y, kb[u].y);
            mac_add(s1x, d[i0 + u].x, ka[u].x);
            mac_add(s1y, d[i0 + u].y, ka[u].y);
          }
        }
        r0.x = add_mod(r0.x, mac_reduce(s0x, mc), q);
        r0.y = add_mod(r0.y, mac_reduce(s0y, mc), q);
        r1.x = add_mod(r1.x, mac_reduce(s1x, mc), q);
        r1.y = add_mod(r1.y, mac_reduce(s1y, mc), q);
      }
    }
    u64* op = out.p + g * H.out_gstride;
    *(ulonglong2*)(op + o0) = r0;
    *(ulonglong2*)(op + o1) = r1;
  }
}

// NTT-domain automorphism: o[j] = a[idx[j]]  (optionally o += a[idx[j]])
__global__ void __launch_bounds__(256) automorph_kernel(LimbSet o, LimbSet a, const u32* __restrict__ idx,
                                                        const DeviceTables* __restrict__ tb, int N, int accumulate) {
  const int row = blockIdx.y;
  const int bi = row % o.nbatch;
  const int r = row / o.nbatch;
  const int l = r % o.nlimb;
  const int c = r / o.nlimb;
  const int n = (blockIdx.x * kBlk + threadIdx.x) * 2;
  if (n >= N) return;
  const u64 q = tb->mc[arg_byte(o.mod, l)].q;
  const u64* src = a.p + row_off(a, c, l, bi);
  u64* dst = o.p + row_off(o, c, l, bi) + n;
  const uint2 ix = *(const uint2*)(idx + n);
  ulonglong2 z = make_ulonglong2(src[ix.x], src[ix.y]);
  if (accumulate) {
    const ulonglong2 w = *(const ulonglong2*)dst;
    z.x = add_mod(z.x, w.x, q);
    z.y = add_mod(z.y, w.y, q);
  }
  *(ulonglong2*)dst = z;
}

// One gadget product of a hoisted key switch, read at the automorphism index j:
//   (sum_i D_i[j] * key[i][0][m][j],  sum_i D_i[j] * key[i][1][m][j])   mod q
// D_i rows at dp + i*dstride; digit `owndigit` comes from ownp instead.
// Digits go in chunks of 4: all 12 loads of a chunk are issued before the
// first product, so their latencies overlap.
// key: made for level klvl (limb of modulus m at key_pos(m, L, klvl), K P limbs)
__device__ __forceinline__ void gadget_at(const u64* __restrict__ dp, long long dstride, const u64* ownp,
                                          int owndigit, const u64* __restrict__ key, int beta, int L, int K, int klvl,
                                          int m, int N, int j, const ModConst& mc, u64& r0, u64& r1) {
  r0 = r1 = 0;
  const long long kstride = (long long)(klvl + 1 + K) * N;
  const u64* kp = key + (long long)key_pos(m, L, klvl) * N + j;
  for (int i0 = 0; i0 < beta; i0 += 4) {
    u64 d[4], k0[4], k1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u;
      if (i < beta) {
        d[u] = i == owndigit ? ownp[j] : dp[i * dstride + j];
        k0[u] = kp[(2 * i + 0) * kstride];
        k1[u] = kp[(2 * i + 1) * kstride];
      }
    }
    MacAcc a0, a1;
    mac_zero(a0), mac_zero(a1);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i0 + u < beta) {
        mac_add(a0, d[u], k0[u]);
        mac_add(a1, d[u], k1[u]);
      }
    }
    r0 = add_mod(r0, mac_reduce(a0, mc), mc.q);
    r1 = add_mod(r1, mac_reduce(a1, mc), mc.q);
  }
}

__device__ __forceinline__ void mac_add1(MacAcc& a, u64 x) {
  a.lo += x;
  a.c += (a.lo < x);
}

// XCD-aware block order for the grids (images, coefficient blocks, limbs) of
// lt_bsgs / lt_giant: workgroups go round-robin to the 8 XCDs by linear id,
// so with the image index fastest every XCD would see every coefficient block
// and fill its own L2 with all of the blocks' shared words (diagonals, keys).
// Here linear id L runs on XCD L % 8 over coefficient blocks = XCD (mod 8),
// images fastest: each block's shared words are read into one XCD's L2 only.
// (x, y, z) = (image, coefficient block, limb); needs gridDim.y % 8 == 0.
__device__ __forceinline__ void lt_xcd_decode(int& x, int& y, int& z) {
  const unsigned gx = gridDim.x, gy = gridDim.y;
  const unsigned lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
  const unsigned xcd = lin & 7, k = lin >> 3, cpx = gy >> 3;
  x = (int)(k % gx);
  const unsigned rest = k / gx;
  y = (int)((rest % cpx) * 8 + xcd);
  z = (int)(rest / cpx);
}

// Hoisted BSGS linear transform, baby steps and giant inner products fused
// (lintrans MultiplyByDiagMatrixBSGS):
//   rot_s  = sigma_s( gadget(D, key_s) + (P * ct0, 0) )   s != 0   (QP, hoisted key switch)
//   rot_0  = (P * ct0, P * ct1) on Q, 0 on P
//   t_g[c] = sum_{s in babies(g)} pt_{g,s} * rot_s[c]
// The NTT-domain automorphism maps every aligned block of 2^k coefficients
// onto an aligned block, so the gathers of one wave stay inside one 512-B
// segment of each source row.  Each thread builds all baby rotations of its
// coefficient in registers and loops over the giants: the rotations never
// touch HBM, and every diagonal (shared by the batch; the image index is the
// fastest grid dimension) is read from L2.
// The "giants" g0..g1 are the entries of one chunk of a column's plan
// (lt_blocks.h; one transform is the 1 x 1 block), each with an output
// component, an output row (images row * colB + bi; the grid spans the colB
// images of the column's input) and its own accumulate flag -- all read from
// the plan at a uniform index, so they stay in SGPRs.  t0 / t1: components 0
// and ng of the layer's inner-sum buffer (batch rows * colB).
// ONE: a chunk of a 1 x 1 layout, where the plan's comp, row and acc say
// nothing new and are not read: entry g goes to component g - g0 of t0 / t1
// (the components of the chunk's first entry), row 0, and no entry accumulates
// but through `accumulate` (measured: profiles/r09a_lt_unify_ab.txt).
// IW: images per workgroup.  1: a workgroup is 256 coefficients of one image
// (grid: colB images x N / 256 blocks x limbs).  4: a workgroup is 64
// coefficients of 4 images, wave w on image 4 bx + w (grid: ceil(colB / 4) x
// N / 64 x limbs, exact: N % 64 == 0).  A diagonal word depends on the
// coefficient and not on the image, so per giant the workgroup loads the MB
// diagonal rows of its 64 coefficients once -- wave w the rows s = w (mod 4),
// into `lds` (2 x MB x 64 words) -- and every wave reads its lane's MB words
// from there.  Two buffers: the rows of giant g + 1 are loaded before giant
// g's products and stored to LDS after them, so one barrier per giant orders
// both the stores to a buffer before its reads and the reads before the next
// stores.  That store waits for the two loads with vmcnt(0), so it stands
// before the giant's own two stores to t0 / t1: behind them it waited for
// their completion too, every giant (lt_bsgs 4.86 against 4.76 ms per step,
// profiles/r10a_lt_shared_diag_ab.txt).
// No thread leaves before the last barrier: a wave past the batch (colB % 4
// != 0) stages its rows like the others and skips its own loads, products and
// stores.  The arithmetic and its order are those of IW = 1.
template <int MB, bool ONE, int IW>
__device__ __forceinline__ void lt_bsgs_body(LimbSet& t0, LimbSet& t1, const LimbSet& D, const LimbSet& ct,
                                             const LtBabies& Bb, const LtPlan* __restrict__ P, int g0, int g1,
                                             int accumulate, const LimbSet& ptl, const DeviceTables* __restrict__ tb,
                                             int N, int z0, int colB, u64* lds) {
  static_assert(IW == 1 || (kBlk / IW == 64 && MB % IW == 0), "one wave per image, the rows dealt out evenly");
  // offset of entry g's output plane in t (t0 or t1), and whether the entry adds to it
  auto tgo = [&](const LimbSet& t, int g) -> long long {
    if constexpr (ONE)
      return (long long)(g - g0) * t.comp_stride;
    else
      return (long long)P->comp[g] * t.comp_stride + (long long)P->row[g] * colB * t.batch_stride;
  };
  auto adds = [&](int g) -> bool {
    if constexpr (ONE)
      return accumulate;
    else
      return accumulate || P->acc[g];
  };
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (Bb.xcd) lt_xcd_decode(bx, by, bz);
  constexpr int CW = kBlk / IW;  // coefficients per workgroup
  const int wv = IW > 1 ? __builtin_amdgcn_readfirstlane((int)threadIdx.x / CW) : 0;
  const int lane = IW > 1 ? (int)threadIdx.x % CW : (int)threadIdx.x;
  const int bi = IW > 1 ? bx * IW + wv : bx;
  const int n = by * CW + lane;
  const int l = z0 + bz;
  if constexpr (IW == 1) {
    if (n >= N) return;
  }
  const bool active = bi < colB;  // wave-uniform; IW = 1: the grid has colB images
  const int m = arg_byte(t0.mod, l);
  const ModConst mc = tb->mc[m];
  const bool isq = l <= Bb.level;
  const long long ro = row_off(t0, 0, l, bi) + n;
  const long long po = (long long)arg_byte(ptl.pos, l) * ptl.limb_stride + n;
  const u64* c0p = ct.p + row_off(ct, 0, isq ? l : 0, bi);
  const u64* c1p = ct.p + row_off(ct, 1, isq ? l : 0, bi);
  const u64* dp = D.p + row_off(D, 0, l, bi);
  const int owndigit = isq ? l / Bb.K : -1;
  const u64 pq = Bb.pq[l], pqs = Bb.pqs[l];
  u64 x0[MB], x1[MB];
  int jx[MB];
#pragma unroll
  for (int s = 0; s < MB; ++s) jx[s] = (s < Bb.nb && Bb.key[s]) ? (int)Bb.idx[s][n] : n;
#pragma unroll
  for (int s = 0; s < MB; ++s) {
    x0[s] = x1[s] = 0;
    if (s < Bb.nb && (IW == 1 || active)) {
      if (Bb.key[s]) {
        const int j = jx[s];
        u64 r0, r1;
        // (a split30 copy of the keys with carry-free MacW products measured
        // 1848 -> 1947 us per lt_bsgs_kernel8 launch just for being compiled in,
        // and no faster when used: profiles/r04h_lt_gadget_w_ab.txt)
        gadget_at(dp, D.comp_stride, c1p, owndigit, Bb.key[s], Bb.beta, Bb.L, Bb.K, Bb.klvl[s], m, N, j, mc, r0, r1);
        if (isq) r0 = add_mod(r0, shoup_mul(c0p[j], pq, pqs, mc.q), mc.q);
        x0[s] = r0;
        x1[s] = r1;
      } else if (isq) {
        x0[s] = shoup_mul(c0p[n], pq, pqs, mc.q);
        x1[s] = shoup_mul(c1p[n], pq, pqs, mc.q);
      }
    }
  }
  // IW > 1, the staged diagonals: diag_first before a giant loop, then per
  // giant diag (pv[s] = slot Bb.s0 + s at this thread's coefficient) before
  // its products and diag_next after them.  (IW = 1 loads pv in the loop.)
  constexpr int RW = IW > 1 ? MB / IW : 1;  // rows a wave stages per giant
  u64 stg[RW];
  int cur = 0;
  auto fetch = [&](int g) {
#pragma unroll
    for (int k = 0; k < RW; ++k) stg[k] = gld(P->pt[g][Bb.s0 + wv + IW * k], po);
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int k = 0; k < RW; ++k) lds[(buf * MB + wv + IW * k) * CW + lane] = stg[k];
  };
  auto diag_first = [&]() {
    if constexpr (IW > 1) {
      if (g0 < g1) {
        fetch(g0);
        put(0);
      }
    }
  };
  auto diag = [&](int g, u64(&pv)[MB]) {
    // (after the last giant: its own rows again, into the buffer nobody reads.
    // Without a branch round the loads and the stores to LDS the compiler
    // counts the loads in flight, and waits for these two only)
    fetch(g + 1 < g1 ? g + 1 : g);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < MB; ++s) pv[s] = lds[(cur * MB + s) * CW + lane];
  };
  auto diag_next = [&](int g) {
    if constexpr (IW > 1) {
      cur ^= 1;
      put(cur);
    }
  };
  const bool small = mc.bar_k <= 48;  // block-uniform
  if (small) {
    // < 2^48 moduli: float64 split products (MacD), one reduction per giant;
    // the baby rotations as 24-bit pieces in doubles
    double xb0[MB], xa0[MB], xb1[MB], xa1[MB];
#pragma unroll
    for (int s = 0; s < MB; ++s) {
      xb0[s] = (double)(u32)(x0[s] & 0xffffffull), xa0[s] = (double)(u32)(x0[s] >> 24);
      xb1[s] = (double)(u32)(x1[s] & 0xffffffull), xa1[s] = (double)(u32)(x1[s] >> 24);
    }
    // the giant loop instantiated with and without accumulation (uniform).
    // Every register slot of every giant runs without branches: the plan
    // points the slots a giant does not use at a zero diagonal, so their
    // products add zero
    auto giants = [&](auto acc_tag) {
      diag_first();
      for (int g = g0; g < g1; ++g) {
        const bool ACC = ONE ? decltype(acc_tag)::value : adds(g);  // (a layer's entries: per entry, uniform)
        const long long to0 = tgo(t0, g) + ro, to1 = tgo(t1, g) + ro;
        const u64* const* rows = P->pt[g];  // the giant's diagonals, by slot
        u64 r0 = 0, r1 = 0;
        if (ACC && (IW == 1 || active)) {
          r0 = t0.p[to0];
          r1 = t1.p[to1];
        }
        u64 pv[MB];
        if constexpr (IW == 1) {
#pragma unroll
          for (int s = 0; s < MB; ++s) pv[s] = gld(rows[Bb.s0 + s], po);
        } else {
          diag(g, pv);
          if (!active) {
            diag_next(g);
            continue;
          }
        }
        MacD a0, a1;
        macd_zero(a0), macd_zero(a1);
#pragma unroll
        for (int s = 0; s < MB; ++s) {
          // the plan's diagonal copies are stored split (EW_SPLIT24): pieces in the two dwords
          // (signed conversions of the dwords: converting (u32)(pv >> 32) went
          // through the u64 conversion and left an add of 0.0 * 2^32 behind)
          u32 w[2];
          __builtin_memcpy(w, &pv[s], 8);
          const double pb = (double)(int)w[0], pa = (double)(int)w[1];  // pieces < 2^24
          macd_add(a0, xb0[s], xa0[s], pb, pa);
          macd_add(a1, xb1[s], xa1[s], pb, pa);
        }
        const u64 v0 = macd_reduce(a0, mc), v1 = macd_reduce(a1, mc);
        r0 = ACC ? add_mod(r0, v0, mc.q) : v0;
        r1 = ACC ? add_mod(r1, v1, mc.q) : v1;
        diag_next(g);
        t0.p[to0] = r0;
        t1.p[to1] = r1;
      }
    };
    if (ONE && accumulate) giants(std::true_type{});
    else giants(std::false_type{});
    return;
  }
  if (mc.bar_k <= 60) {
    // 48..60-bit moduli: 30-bit piece products accumulated without carries
    // (MacW, one v_mad_u64_u32 each), one reduction per 8 babies; the plan's
    // diagonal copies are stored split30, and the baby rotations are cut into
    // their pieces once here (the split30 word takes the same two VGPRs), not
    // per giant
#pragma unroll
    for (int s = 0; s < MB; ++s) x0[s] = split30(x0[s]), x1[s] = split30(x1[s]);
    diag_first();
    for (int g = g0; g < g1; ++g) {
      const u64* const* rows = P->pt[g];  // the giant's diagonals, by slot
      u64 r0 = 0, r1 = 0;
      const long long to0 = tgo(t0, g) + ro, to1 = tgo(t1, g) + ro;
      if (adds(g) && (IW == 1 || active)) {
        r0 = t0.p[to0];
        r1 = t1.p[to1];
      }
      u64 pv[MB];
      if constexpr (IW == 1) {
#pragma unroll
        for (int s = 0; s < MB; ++s) pv[s] = gld(rows[Bb.s0 + s], po);
      } else {
        diag(g, pv);
        if (!active) {
          diag_next(g);
          continue;
        }
      }
      MacW a0, a1;
      macw_zero(a0), macw_zero(a1);
#pragma unroll
      for (int s = 0; s < MB; ++s) {
        const u32 yb = (u32)pv[s], ya = (u32)(pv[s] >> 32);
        macw_add(a0, (u32)x0[s], (u32)(x0[s] >> 32), yb, ya);
        macw_add(a1, (u32)x1[s], (u32)(x1[s] >> 32), yb, ya);
        if ((s & 7) == 7) {
          r0 = add_mod(r0, macw_reduce8(a0, mc), mc.q);
          r1 = add_mod(r1, macw_reduce8(a1, mc), mc.q);
          macw_zero(a0), macw_zero(a1);
        }
      }
      diag_next(g);
      t0.p[to0] = r0;
      t1.p[to1] = r1;
    }
    return;
  }
  // moduli of at most 60 bits: 8 products per reduction (mac_reduce8).  (Those
  // limbs took the 30-bit pieces above, so acc8 is false here; the compiler
  // does not see that, and without the arm all eight lt_bsgs kernels come out
  // differently, lt_bsgs_kernel8<false> with 36 B of scratch for 28: it stays
  // until a change that is timed)
  const bool acc8 = mc.bar_k <= 60;
  diag_first();
  for (int g = g0; g < g1; ++g) {
    const u64* const* rows = P->pt[g];  // the giant's diagonals, by slot
    u64 r0 = 0, r1 = 0;
    const long long to0 = tgo(t0, g) + ro, to1 = tgo(t1, g) + ro;
    if (adds(g) && (IW == 1 || active)) {
      r0 = t0.p[to0];
      r1 = t1.p[to1];
    }
    // issue every diagonal load of this giant before the first product so
    // their latencies overlap (the branches are wave-uniform)
    u64 pv[MB];
    if constexpr (IW == 1) {
#pragma unroll
      for (int s = 0; s < MB; ++s) pv[s] = gld(rows[Bb.s0 + s], po);
    } else {
      diag(g, pv);
      if (!active) {
        diag_next(g);
        continue;
      }
    }
    MacAcc a0, a1;
    mac_zero(a0), mac_zero(a1);
#pragma unroll
    for (int s = 0; s < MB; ++s) {
      mac_add(a0, pv[s], x0[s]);
      mac_add(a1, pv[s], x1[s]);
      if (acc8 ? (s & 7) == 7 : (s & 3) == 3) {  // (acc8 is block-uniform)
        r0 = add_mod(r0, acc8 ? mac_reduce8(a0, mc) : mac_reduce(a0, mc), mc.q);
        r1 = add_mod(r1, acc8 ? mac_reduce8(a1, mc) : mac_reduce(a1, mc), mc.q);
        mac_zero(a0), mac_zero(a1);
      }
    }
    diag_next(g);
    t0.p[to0] = r0;
    t1.p[to1] = r1;
  }
}

// Entries e0 .. e1 - 1 of one plan chunk.  MB = 8 at 4 waves per SIMD (<= 128
// VGPRs); MB = 16 holds twice the babies
template <bool ONE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LT_WAVES8)))
lt_bsgs_kernel8(LimbSet t0, LimbSet t1, LimbSet D, LimbSet ct, LtBabies Bb, const LtPlan* __restrict__ P, int e0,
                int e1, int accumulate, LimbSet ptl, const DeviceTables* __restrict__ tb, int N, int z0, int colB) {
  lt_bsgs_body<8, ONE, 1>(t0, t1, D, ct, Bb, P, e0, e1, accumulate, ptl, tb, N, z0, colB, nullptr);
}
template <bool ONE>
__global__ void __launch_bounds__(256)
lt_bsgs_kernel16(LimbSet t0, LimbSet t1, LimbSet D, LimbSet ct, LtBabies Bb, const LtPlan* __restrict__ P, int e0,
                 int e1, int accumulate, LimbSet ptl, const DeviceTables* __restrict__ tb, int N, int z0, int colB) {
  lt_bsgs_body<16, ONE, 1>(t0, t1, D, ct, Bb, P, e0, e1, accumulate, ptl, tb, N, z0, colB, nullptr);
}
// The same with LT_IW images per workgroup, the diagonals staged in LDS once
// for all of them (lt_bsgs_body, IW > 1)
template <bool ONE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LT_WAVES8)))
lt_bsgs_shared_kernel8(LimbSet t0, LimbSet t1, LimbSet D, LimbSet ct, LtBabies Bb, const LtPlan* __restrict__ P,
                       int e0, int e1, int accumulate, LimbSet ptl, const DeviceTables* __restrict__ tb, int N, int z0,
                       int colB) {
  __shared__ u64 lds[2 * 8 * (256 / LT_IW)];
  lt_bsgs_body<8, ONE, LT_IW>(t0, t1, D, ct, Bb, P, e0, e1, accumulate, ptl, tb, N, z0, colB, lds);
}
template <bool ONE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
lt_bsgs_shared_kernel16(LimbSet t0, LimbSet t1, LimbSet D, LimbSet ct, LtBabies Bb, const LtPlan* __restrict__ P,
                        int e0, int e1, int accumulate, LimbSet ptl, const DeviceTables* __restrict__ tb, int N,
                        int z0, int colB) {
  __shared__ u64 lds[2 * 16 * (256 / LT_IW)];
  lt_bsgs_body<16, ONE, LT_IW>(t0, t1, D, ct, Bb, P, e0, e1, accumulate, ptl, tb, N, z0, colB, lds);
}

// Giant steps of a hoisted BSGS transform, key switches and accumulation fused:
//   acc[c] = sum_g sigma_g( gadget(D_g, key_g)[c] + (c == 0) * t0_g ) + z[c]
// D_g: decomposition of ModDown(t1_g) (digit i of group g at D.p + g*d_gstride
// + i*D.comp_stride; its own Q limbs read from `own`, the ModDown output);
// z = the zero giant's (t0, t1), added without automorphism.
// Each thread takes one coefficient of IB images: the automorphism index, the
// key words and every pointer step are shared by the IB images, so the key
// reads from L2 and the scalar address work per product drop IB-fold.
template <int IB, bool ROWS>
__global__ void __launch_bounds__(256) lt_giant_kernel(LimbSet acc, LimbSet D, LimbSet own, LimbSet t0, LimbSet z,
                                                       LtGiants G, const DeviceTables* __restrict__ tb, int N) {
  constexpr int CH = IB >= 4 ? 2 : 4;  // digits per load chunk
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (G.xcd) lt_xcd_decode(bx, by, bz);
  const int b0 = bx * IB;
  const int n = by * kBlk + threadIdx.x;
  const int l = bz;
  if (n >= N) return;
  const int nb = acc.nbatch - b0 < IB ? acc.nbatch - b0 : IB;  // uniform
  const int m = arg_byte(acc.mod, l);
  const ModConst mc = tb->mc[m];
  const bool isq = l <= G.level;
  const int owndigit = isq ? l / G.K : -1;
  const long long dro = row_off(D, 0, l, b0), oro = row_off(own, 0, isq ? l : 0, b0), tro = row_off(t0, 0, l, b0);
  const long long dbs = D.batch_stride, obs = own.batch_stride, tbs = t0.batch_stride;
  u64 r0[IB], r1[IB];
#pragma unroll
  for (int b = 0; b < IB; ++b) r0[b] = r1[b] = 0;
  // the giant loop, instantiated for the two reduction schemes
  auto giants = [&](auto small_tag) {
    constexpr bool SMALL = decltype(small_tag)::value;
    MacAcc a0[IB], a1[IB];
    if (SMALL) {
#pragma unroll
      for (int b = 0; b < IB; ++b) mac_zero(a0[b]), mac_zero(a1[b]);
    }
    int cnt = 0;
    int jn = G.ng > 0 ? (int)G.idx[0][n] : 0;
    for (int g = 0; g < G.ng; ++g) {
      const int j = jn;
      if (g + 1 < G.ng) jn = G.idx[g + 1][n];  // prefetch the next giant's index
      const int klvl = G.klvl[g];
      const long long kstride = (long long)(klvl + 1 + G.K) * N;
      const u64* kp = G.key[g] + (long long)key_pos(m, G.L, klvl) * N + j;
      const u64* dp = D.p + g * G.d_gstride + dro + j;
      const u64* op = own.p + g * G.own_gstride + oro + j;
      for (int i0 = 0; i0 < G.beta; i0 += CH) {
        u64 d[CH][IB], k0[CH], k1[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
          const int i = i0 + u;
          if (i < G.beta) {
            k0[u] = kp[(2 * i + 0) * kstride];
            k1[u] = kp[(2 * i + 1) * kstride];
            const u64* src = i == owndigit ? op : dp + i * D.comp_stride;
            const long long bs = i == owndigit ? obs : dbs;
#pragma unroll
            for (int b = 0; b < IB; ++b)
              if (b < nb) d[u][b] = src[b * bs];
          }
        }
        if (SMALL) {
#pragma unroll
          for (int u = 0; u < CH; ++u)
            if (i0 + u < G.beta) {
#pragma unroll
              for (int b = 0; b < IB; ++b)
                if (b < nb) mac_add(a0[b], d[u][b], k0[u]), mac_add(a1[b], d[u][b], k1[u]);
            }
        } else {
#pragma unroll
          for (int b = 0; b < IB; ++b) {
            if (b >= nb) break;
            MacAcc c0, c1;
            mac_zero(c0), mac_zero(c1);
#pragma unroll
            for (int u = 0; u < CH; ++u)
              if (i0 + u < G.beta) mac_add(c0, d[u][b], k0[u]), mac_add(c1, d[u][b], k1[u]);
            r0[b] = add_mod(r0[b], mac_reduce(c0, mc), mc.q);
            r1[b] = add_mod(r1[b], mac_reduce(c1, mc), mc.q);
          }
        }
      }
      const u64* tp = t0.p + g * G.t0_gstride + tro + j;
#pragma unroll
      for (int b = 0; b < IB; ++b)
        if (b < nb) {
          const u64 t = tp[b * tbs];
          if (SMALL) mac_add1(a0[b], t);
          else r0[b] = add_mod(r0[b], t, mc.q);
        }
      if (SMALL) {
        cnt += G.beta + 1;
        if (cnt + G.beta + 1 > 120) {
#pragma unroll
          for (int b = 0; b < IB; ++b) {
            r0[b] = add_mod(r0[b], mac_reduce_small(a0[b], mc), mc.q);
            r1[b] = add_mod(r1[b], mac_reduce_small(a1[b], mc), mc.q);
            mac_zero(a0[b]), mac_zero(a1[b]);
          }
          cnt = 0;
        }
      }
    }
    if (SMALL) {
#pragma unroll
      for (int b = 0; b < IB; ++b) {
        r0[b] = add_mod(r0[b], mac_reduce_small(a0[b], mc), mc.q);
        r1[b] = add_mod(r1[b], mac_reduce_small(a1[b], mc), mc.q);
      }
    }
  };
  // moduli below 2^52: every giant's products and its t0 term go into one
  // unreduced accumulator per image, reduced once per <= 120 products instead
  // of once per giant (the Barrett reduction is ~40 VALU ops per component)
  if (mc.bar_k <= 52) giants(std::true_type{});  // block-uniform
  else giants(std::false_type{});
#pragma unroll
  for (int b = 0; b < IB; ++b) {
    if (b >= nb) break;
    u64 x0 = r0[b], x1 = r1[b];
    if (G.has_zero) {
      x0 = add_mod(x0, z.p[row_off(z, 0, l, b0 + b) + n], mc.q);
      x1 = add_mod(x1, z.p[row_off(z, 1, l, b0 + b) + n], mc.q);
    }
    r0[b] = x0, r1[b] = x1;
  }
  if constexpr (ROWS) {
    if (l >= G.rows_from) {  // (block-uniform) a P limb: the final ModDown INTT's rows pass, here
      // the block's 256 coefficients are row `by` of the limb, for 2 nb
      // (image, component) rows q = 2 b + c: staged in LDS, then 4 rows at a
      // time, thread (rr, kk) runs the radix-4 inverse rows steps on elements
      // 4 kk .. 4 kk + 3 of row q0 + rr and stores the INTT's intermediate in
      // place of the row.  A group past the last row works on a spare LDS row
      // of its own and stores nothing, so every thread keeps the barriers.
      constexpr int NR = 2 * IB > 4 ? 2 * IB : 4;
      __shared__ u64 lds[NR * 256];
      const int t = threadIdx.x;
#pragma unroll
      for (int b = 0; b < IB; ++b)
        if (b < nb) lds[(2 * b) * 256 + t] = r0[b], lds[(2 * b + 1) * 256 + t] = r1[b];
      __syncthreads();
      const int rr = t >> 6, kk = t & 63;
      for (int q0 = 0; q0 < 2 * nb; q0 += 4) {  // (uniform)
        const int q = q0 + rr;
        const bool live = q < 2 * nb;
        u64* const lr = lds + q * 256;
        u64* const mid = acc.p + row_off(acc, q & 1, l, b0 + (live ? q >> 1 : 0)) + (by << 8);
        auto rows = [&](const auto& ar, __amdgpu_buffer_rsrc_t tw) {
          using A = std::decay_t<decltype(ar)>;
          typename A::T x[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) x[i] = ar.from_u64(lr[4 * kk + i]);
          if (G.logN == 15)
            inv_rows4_core<A, 15>(x, by, kk, ar, tw, lr, mid, live);
          else
            inv_rows4_core<A, 16>(x, by, kk, ar, tw, lr, mid, live);
        };
        if (mc.f64)
          rows(F64Arith(mc), twr_s(tb->inv_d[m], 8 * N));
        else
          rows(IntArith(mc), twr_s(tb->inv[m], 16 * N));
      }
      return;
    }
  }
#pragma unroll
  for (int b = 0; b < IB; ++b) {
    if (b >= nb) break;
    acc.p[row_off(acc, 0, l, b0 + b) + n] = r0[b];
    acc.p[row_off(acc, 1, l, b0 + b) + n] = r1[b];
  }
}

inline dim3 ew_grid(int N, int rows) { return dim3((N / 2 + 255) / 256, rows); }
// split the targets of a small basis extension over blockIdx.z until the
// launch has ~2048 workgroups (8 per CU); the per-coefficient prologue is
// recomputed per chunk, which costs ns multiplies against nt/chunk targets
inline unsigned target_chunks(dim3 g, int nt) {
  const long long wg = (long long)g.x * g.y;
  long long z = (2048 + wg - 1) / wg;
  if (z > nt / 4) z = nt / 4;  // keep >= 4 targets per chunk
  return z < 1 ? 1u : (unsigned)z;
}

}  // namespace

// ------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------
int orion_launch_ew(int op, const LimbSet& o, const LimbSet& a, const LimbSet& b, const u64* s, const u64* ss,
                    const DeviceTables* tb, int N, hipStream_t st) {
  Scalars sc;
  for (int l = 0; l < o.nlimb; ++l) {
    sc.s[l] = s ? s[l] : 0;
    sc.ss[l] = ss ? ss[l] : 0;
  }
  const int rows = o.ncomp * o.nlimb * o.nbatch;
  if (rows == 0) return 0;
  dim3 g = ew_grid(N, rows), blk(256);
  switch (op) {
#define CASE(OPC) \
  case OPC: hipLaunchKernelGGL(ew_kernel<OPC>, g, blk, 0, st, o, a, b, sc, tb, N); break;
    CASE(EW_ADD) CASE(EW_SUB) CASE(EW_MUL) CASE(EW_MULADD) CASE(EW_NEG) CASE(EW_SCALE) CASE(EW_ADDC)
    CASE(EW_SUBSCALE) CASE(EW_COPY) CASE(EW_ADDSCALE) CASE(EW_SPLIT24)
#undef CASE
    default: return -1;
  }
  return 0;
}

// o = a + I b (images below npair; the rest a alone), w4/w4s: psi^(N/2) and
// its Shoup companion per limb of o
int orion_launch_pack_complex(const LimbSet& o, const LimbSet& a, const LimbSet& b, int npair, const u64* w4,
                              const u64* w4s, const DeviceTables* tb, int N, hipStream_t st) {
  const int rows = o.ncomp * o.nlimb * o.nbatch;
  if (rows < 1 || rows > 65535 || N < 4 || (N & 3) || npair < 0 || npair > o.nbatch || (npair && !b.p)) return -1;
  Scalars sc;
  for (int l = 0; l < o.nlimb; ++l) sc.s[l] = w4[l], sc.ss[l] = w4s[l];
  hipLaunchKernelGGL(pack_complex_kernel, ew_grid(N, rows), dim3(kBlk), 0, st, o, a, b, sc, npair, tb, N);
  return 0;
}

// re = x + y, im = I (y - x) on the images below nim
int orion_launch_unpack_complex(const LimbSet& re, const LimbSet& im, const LimbSet& x, const LimbSet& y, int nim,
                                const u64* w4, const u64* w4s, const DeviceTables* tb, int N, hipStream_t st) {
  const int rows = x.ncomp * x.nlimb * x.nbatch;
  if (rows < 1 || rows > 65535 || N < 4 || (N & 3) || nim < 0 || nim > x.nbatch || (nim && !im.p)) return -1;
  Scalars sc;
  for (int l = 0; l < x.nlimb; ++l) sc.s[l] = w4[l], sc.ss[l] = w4s[l];
  hipLaunchKernelGGL(unpack_complex_kernel, ew_grid(N, rows), dim3(kBlk), 0, st, re, im, x, y, sc, nim, tb, N);
  return 0;
}

// o_k = sum_i M_i a_(k + i h): o holds h = ceil(B / g) groups of a's B images; m1 = the row of M_1 per limb of o
int orion_launch_mono_pack(const LimbSet& o, const LimbSet& a, const LimbSet& m1, int g, const DeviceTables* tb,
                           int N, hipStream_t st) {
  const int h = o.nbatch, B = a.nbatch;
  const long long rows = (long long)o.ncomp * o.nlimb * h;
  if (rows < 1 || rows > 65535 || N < 4 || (N & 3) || g < 1 || g > N || B < 1 || h != (B + g - 1) / g ||
      a.ncomp != o.ncomp || a.nlimb != o.nlimb || m1.nlimb != o.nlimb || !o.p || !a.p || !m1.p)
    return -1;
  hipLaunchKernelGGL(mono_pack_kernel, ew_grid(N, (int)rows), dim3(kBlk), 0, st, o, a, m1, g, tb, N);
  return 0;
}

// o_(k + i h) = M_-i x_k: x holds h = ceil(B / g) groups, o B images; mi = the row of M_-1 per limb of x
int orion_launch_mono_unpack(const LimbSet& o, const LimbSet& x, const LimbSet& mi, int g, const DeviceTables* tb,
                             int N, hipStream_t st) {
  const int h = x.nbatch, B = o.nbatch;
  const long long rows = (long long)x.ncomp * x.nlimb * h;
  if (rows < 1 || rows > 65535 || N < 4 || (N & 3) || g < 1 || g > N || B < 1 || h != (B + g - 1) / g ||
      o.ncomp != x.ncomp || o.nlimb != x.nlimb || mi.nlimb != x.nlimb || !o.p || !x.p || !mi.p)
    return -1;
  hipLaunchKernelGGL(mono_unpack_kernel, ew_grid(N, (int)rows), dim3(kBlk), 0, st, o, x, mi, g, tb, N);
  return 0;
}

int orion_launch_gather(u64* dst, long long d_comp, long long d_limb, int nimg, int nlimb, const GatherTable& T,
                        int N, hipStream_t st) {
  constexpr int per = 2 * kBlk * kGatherU;  // coefficients per workgroup
  if (nimg < 1 || nimg > ORION_MAXGATHER || nlimb < 1 || 2 * nlimb > 65535 || N < per || N % per) return -1;
  hipLaunchKernelGGL(gather_images_kernel, dim3(N / per, nimg, 2 * nlimb), dim3(kBlk), 0, st, dst, d_comp, d_limb,
                     nlimb, T, N);
  return 0;
}

int orion_launch_tensor(const LimbSet& d, const LimbSet& a, const LimbSet& b, const DeviceTables* tb, int N,
                        hipStream_t st) {
  const int rows = d.nlimb * d.nbatch;
  hipLaunchKernelGGL(tensor_kernel, ew_grid(N, rows), dim3(256), 0, st, d, a, b, tb, N);
  return 0;
}

// d (3 components) = (acc ? d : 0) + the tensors of T's pairs
int orion_launch_tensor_sum(const LimbSet& d, const tsum::Table& T, bool acc, const DeviceTables* tb, int N,
                            hipStream_t st) {
  const int rows = d.nlimb * d.nbatch;
  if (T.n < 1 || T.n > ORION_MAXTSUM || T.nsq < 0 || T.nsq > T.n || d.ncomp != 3 || rows < 1 || rows > 65535 || N < 2 ||
      (N & 1))
    return -1;
  if (acc)
    hipLaunchKernelGGL(tensor_sum_kernel<true>, ew_grid(N, rows), dim3(256), 0, st, d, T, tb, N);
  else
    hipLaunchKernelGGL(tensor_sum_kernel<false>, ew_grid(N, rows), dim3(256), 0, st, d, T, tb, N);
  return 0;
}


int orion_launch_basis_ext(const LimbSet& out, const LimbSet& in, const BasisExtTable* T, const DeviceTables* tb,
                           int N, hipStream_t st) {
  const int rows = out.ncomp * out.nbatch;
  dim3 g = ew_grid(N, rows);
  const int nt = out.nlimb;
  g.z = target_chunks(g, nt);
  const int tc = (nt + g.z - 1) / g.z;
  // the kernel's source arrays sized for in.nlimb (= the table's ns)
  if (in.nlimb <= 2)
    hipLaunchKernelGGL(basis_ext_kernel<2>, g, dim3(256), 0, st, out, in, T, N, tc);
  else if (in.nlimb <= 4)
    hipLaunchKernelGGL(basis_ext_kernel<4>, g, dim3(256), 0, st, out, in, T, N, tc);
  else if (in.nlimb <= ORION_MAXSRC)
    hipLaunchKernelGGL(basis_ext_kernel<ORION_MAXSRC>, g, dim3(256), 0, st, out, in, T, N, tc);
  else
    return -1;
  return 0;
}

// in: limb l of x, then the table's ns P limbs; out: the l limbs below the pivot
int orion_launch_basis_ext_rescale(const LimbSet& out, const LimbSet& in, const BextRescaleTable* W, int N,
                                   hipStream_t st) {
  const int rows = out.ncomp * out.nbatch, ns = in.nlimb - 1;
  if (out.nlimb < 1 || ns < 1 || in.ncomp != out.ncomp || in.nbatch != out.nbatch) return -1;
  dim3 g = ew_grid(N, rows);
  const int nt = out.nlimb;
  g.z = target_chunks(g, nt);
  const int tc = (nt + g.z - 1) / g.z;
  if (ns <= 2)
    hipLaunchKernelGGL(basis_ext_rescale_kernel<2>, g, dim3(256), 0, st, out, in, W, N, tc);
  else if (ns <= 4)
    hipLaunchKernelGGL(basis_ext_rescale_kernel<4>, g, dim3(256), 0, st, out, in, W, N, tc);
  else if (ns <= ORION_MAXSRC)
    hipLaunchKernelGGL(basis_ext_rescale_kernel<ORION_MAXSRC>, g, dim3(256), 0, st, out, in, W, N, tc);
  else
    return -1;
  return 0;
}

int orion_launch_modup_all(const LimbSet& D, const LimbSet& in, const BasisExtTable* Ts, int beta, int K,
                           int nqp, const DeviceTables* tb, int N, hipStream_t st) {
  if (beta < 1 || nqp > ORION_MAXLIMB || D.ncomp != in.ncomp * beta) return -1;
  for (int j = 0; j < nqp; ++j)
    if (D.pos[j] != j) return -1;  // the kernel walks the limbs with one pointer
  const int rows = D.ncomp * D.nbatch;
  dim3 g = ew_grid(N, rows);
  g.z = target_chunks(g, nqp);
  const int tc = (nqp + g.z - 1) / g.z;
  if (K <= 2)  // every digit has at most K sources
    hipLaunchKernelGGL(modup_all_kernel<2>, g, dim3(256), 0, st, D, in, Ts, beta, K, nqp, N, tc);
  else if (K <= 4)
    hipLaunchKernelGGL(modup_all_kernel<4>, g, dim3(256), 0, st, D, in, Ts, beta, K, nqp, N, tc);
  else if (K <= ORION_MAXSRC)
    hipLaunchKernelGGL(modup_all_kernel<ORION_MAXSRC>, g, dim3(256), 0, st, D, in, Ts, beta, K, nqp, N, tc);
  else
    return -1;
  return 0;
}

int orion_launch_ks_mac(const LimbSet& out, const LimbSet& D, const LimbSet& own, const MacGroups& G, int ngroup,
                        int beta, const DeviceTables* tb, int N, hipStream_t st) {
  const int rows = ngroup * out.nlimb * out.nbatch;
  if (rows == 0) return 0;
  if (ngroup > ORION_MAXGROUP) return -1;
  if (G.rows_from > 0) {
    if ((G.logN != 15 && G.logN != 16) || N != (1 << G.logN) || ngroup != 1) return -1;
    if (G.fwd_rows) {
      if (beta > 16 || G.d_gstride) return -1;
      // (4 + 2 beta) x 2 KiB of LDS: up to 72 KiB at beta = 16, past the
      // 64 KiB a launch gets without the attribute (set once, for the largest)
      static const bool lds_attr = hipFuncSetAttribute((const void*)ks_mac_full_kernel<false>,
                                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       (4 + 2 * 16) * 256 * 8) == hipSuccess;
      if (!lds_attr) return -1;
      const size_t lds = (size_t)(4 + 2 * beta) * 256 * 8;
      if (beta <= 4)  // the key words loaded before the rows pass (12 KiB of LDS at most)
        hipLaunchKernelGGL(ks_mac_full_kernel<true>, ew_grid(N, rows), dim3(256), lds, st, out, D, own, G, beta, tb, N);
      else
        hipLaunchKernelGGL(ks_mac_full_kernel<false>, ew_grid(N, rows), dim3(256), lds, st, out, D, own, G, beta, tb, N);
      return 0;
    }
    hipLaunchKernelGGL(ks_mac_rows_kernel, ew_grid(N, rows), dim3(256), 0, st, out, D, own, G, beta, tb, N);
    return 0;
  }
  hipLaunchKernelGGL(ks_mac_kernel, ew_grid(N, rows), dim3(256), 0, st, out, D, own, G, beta, tb, N);
  return 0;
}

int orion_launch_ks_mac_hoisted(const LimbSet& out, const LimbSet& D, const LimbSet& own, const LimbSet& add,
                                const MacHoist& H, const DeviceTables* tb, int N, hipStream_t st) {
  if (H.keys.n < 1 || H.keys.n > ORION_MAXHOIST || !hoist::in_registers(H.beta)) return -1;
  if (D.ncomp < H.beta || D.nlimb != out.nlimb || D.nbatch != out.nbatch || own.nbatch != out.nbatch ||
      add.nbatch != out.nbatch || own.nlimb > out.nlimb || add.nlimb > out.nlimb || out.ncomp != 2 || (N & 1))
    return -1;
  const int rows = out.nlimb * out.nbatch;
  if (rows == 0) return 0;
  if (hoist::digit_slots(H.beta) == 4)
    hipLaunchKernelGGL(ks_mac_hoisted_kernel<4>, ew_grid(N, rows), dim3(256), 0, st, out, D, own, add, H, tb, N);
  else
    hipLaunchKernelGGL(ks_mac_hoisted_kernel<ORION_HOIST_MAXBETA>, ew_grid(N, rows), dim3(256), 0, st, out, D, own,
                       add, H, tb, N);
  return 0;
}

// The first ne entries of chunk `chunk` of a column's plan (plan: the column's
// first chunk).  t0 / t1: components 0 and ng of the inner-sum buffer, batch
// rows * colB, every entry's row below rows; ct and D: the column's colB
// images.  one: the layout is 1 x 1, so the chunk's entries are the components
// from chunk * LT_MAXG on, in order (the ONE instantiation)
int orion_launch_lt_bsgs(const LimbSet& t0, const LimbSet& t1, const LimbSet& D, const LimbSet& ct,
                         const LtBabies& Bb, const LtPlan* plan, int chunk, int ne, int accumulate, bool one,
                         const LimbSet& ptl, const DeviceTables* tb, int N, int colB, hipStream_t st) {
  if (Bb.nb < 1 || Bb.nb > LT_MAXB || chunk < 0 || ne < 1 || ne > LT_MAXG) return -1;
  if (colB < 1 || t0.nbatch % colB || ct.nbatch != colB || (one && t0.nbatch != colB)) return -1;
  const LtPlan* P = plan + chunk;
  LimbSet a0 = t0, a1 = t1;
  if (one) a0.p += (long long)chunk * LT_MAXG * a0.comp_stride, a1.p += (long long)chunk * LT_MAXG * a1.comp_stride;
  // LT_IW images and more: a workgroup is 64 coefficients of LT_IW images and
  // loads their diagonals once (its grid must be exact: the kernel has barriers
  // and no bounds check)
  const bool shared = colB >= LT_IW && N % (256 / LT_IW) == 0;
  auto launch = [&](int z0, int nz) {
    if (nz <= 0) return;
    const dim3 g = shared ? dim3((colB + LT_IW - 1) / LT_IW, N / (256 / LT_IW), nz) : dim3(colB, (N + 255) / 256, nz);
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, g, dim3(256), 0, st, a0, a1, D, ct, Bb, P, 0, ne, accumulate, ptl, tb, N, z0, colB);
    };
    if (shared) {
      if (Bb.nb <= 8)
        one ? go(lt_bsgs_shared_kernel8<true>) : go(lt_bsgs_shared_kernel8<false>);
      else
        one ? go(lt_bsgs_shared_kernel16<true>) : go(lt_bsgs_shared_kernel16<false>);
    } else if (Bb.nb <= 8)
      one ? go(lt_bsgs_kernel8<true>) : go(lt_bsgs_kernel8<false>);
    else
      one ? go(lt_bsgs_kernel16<true>) : go(lt_bsgs_kernel16<false>);
  };
  // ORION_LT_SPLIT=1 (timing diagnostics): three launches, limb 0, the middle
  // Q limbs and the last Bb.K (P) limbs, so a kernel trace times each class
  static const bool split = getenv("ORION_LT_SPLIT") && atoi(getenv("ORION_LT_SPLIT")) == 1;
  if (split && t0.nlimb > Bb.K + 1) {
    launch(0, 1);
    launch(1, t0.nlimb - 1 - Bb.K);
    launch(t0.nlimb - Bb.K, Bb.K);
  } else {
    launch(0, t0.nlimb);
  }
  return 0;
}

int orion_launch_lt_giant(const LimbSet& acc, const LimbSet& D, const LimbSet& own, const LimbSet& t0,
                          const LimbSet& z, const LtGiants& G, const DeviceTables* tb, int N, hipStream_t st) {
  if (G.ng > ORION_MAXGROUP) return -1;
  if (G.rows_from > 0 && ((G.logN != 15 && G.logN != 16) || N != (1 << G.logN))) return -1;
  // one image (batch 1): the one-image instantiation, whose registers are a
  // quarter of IB = 4's (more waves per SIMD, more loads in flight per CU)
  const bool one = acc.nbatch == 1;
  if (one) {
    const dim3 g(1, (N + 255) / 256, acc.nlimb);
    if (G.rows_from > 0)
      hipLaunchKernelGGL((lt_giant_kernel<1, true>), g, dim3(256), 0, st, acc, D, own, t0, z, G, tb, N);
    else
      hipLaunchKernelGGL((lt_giant_kernel<1, false>), g, dim3(256), 0, st, acc, D, own, t0, z, G, tb, N);
    return 0;
  }
  constexpr int IB = LT_GIANT_IB;
  dim3 g((acc.nbatch + IB - 1) / IB, (N + 255) / 256, acc.nlimb);
  if (G.rows_from > 0) {
    hipLaunchKernelGGL((lt_giant_kernel<IB, true>), g, dim3(256), 0, st, acc, D, own, t0, z, G, tb, N);
    return 0;
  }
  hipLaunchKernelGGL((lt_giant_kernel<IB, false>), g, dim3(256), 0, st, acc, D, own, t0, z, G, tb, N);
  return 0;
}

int orion_launch_automorph(const LimbSet& o, const LimbSet& a, const u32* idx, const DeviceTables* tb, int N,
                           int accumulate, hipStream_t st) {
  const int rows = o.ncomp * o.nlimb * o.nbatch;
  hipLaunchKernelGGL(automorph_kernel, ew_grid(N, rows), dim3(256), 0, st, o, a, idx, tb, N, accumulate);
  return 0;
}
