// ntt2s.hip -- latency-oriented two-pass NTT / INTT for launches of few
// limb-transforms (one image: the batch-1 forward pass, small decompositions)
// at N = 2^15 and 2^16.
//
// The same transform and the same pass split as ntt2.hip (Lattigo v6 ring
// convention, e = col + 256 * row; cols pass = the stages on the row bits,
// rows pass = the stages on bits 7..0), but each thread owns ONE butterfly of
// every stage instead of a 16-point sub-transform: the tile sits in LDS and
// every stage is one LDS read, one butterfly, one LDS write and one barrier.
// ntt2.hip's thread runs 32 butterflies back to back per pass, which a launch
// of a few limbs (under one wave per SIMD) cannot hide; here the per-thread
// chain is R or 8 butterflies and a launch has 16x the threads.  Large
// launches keep ntt2.hip / ntt.hip (more LDS traffic and barriers per
// butterfly here).  Outputs are fully reduced, so they are bit-identical to
// the other kernels'.
#include <type_traits>

#include "common.h"
#include "launch.h"
#include "ntt_arith.h"
#include "ntt2s_rows.h"

namespace {

// columns per cols-pass workgroup at N = 2^15, rows per rows-pass workgroup:
// a launch of J jobs runs J 256/CW (J 2^R/RW) workgroups, and with a few jobs
// (one image) the time is that of the CUs holding the most workgroups
constexpr int NTT2S_CW15 = 8;
constexpr int NTT2S_RW = 4;
template <int LOGN>
struct S2 {
  static constexpr int R = LOGN - 8;            // row bits: the cols pass transforms 2^R-point columns
  static constexpr int CW = LOGN == 15 ? NTT2S_CW15 : 4;  // columns per cols-pass workgroup
  static constexpr int CTILES = 256 / CW;        // cols-pass workgroups per limb
  static constexpr int RW = NTT2S_RW;           // rows per rows-pass workgroup
  static constexpr int RTILES = (1 << R) / RW;   // rows-pass workgroups per limb
  static constexpr int CT4 = CW << (R - 2);      // cols-pass threads (256)
  static constexpr int RT4 = RW * 64;            // rows-pass threads (256)
};

// forward prologue: element e of job (c, l, b)
template <class A, int PRO>
__device__ __forceinline__ typename A::T fwd_load(const NttIO& io, int c, int l, int b, int e, const ModConst& mc,
                                                  const A& ar, const DeviceTables* __restrict__ tb) {
  if constexpr (PRO == NTT_PRO_LOAD) {
    return ar.from_u64(row_ptr(io.src, c, l, b)[e]);
  } else if constexpr (PRO == NTT_PRO_BEXT) {
    const int k = arg_byte(io.bx_tab, l), ti = arg_byte(io.bx_t, l), s0 = arg_byte(io.bx_s0, k);
    const BasisExtTable* __restrict__ T = io.bx + k;
    const int ns = T->ns;
    u64 x[2] = {row_ptr(io.src, c, s0, b)[e], ns > 1 ? row_ptr(io.src, c, s0 + 1, b)[e] : 0}, y[2];
    const u64 v = bext_prep<2>(T, x, y);
    return ar.from_u64(bext_target_sel<2>(T->tgt + ti, ns, y, v));
  } else {  // NTT_PRO_RESCALE
    const u64 qL = tb->mc[io.modL].q, h = qL >> 1;
    const u64 hm = barrett128(0, h, mc);
    const u64 x = row_ptr(io.src, c, 0, b)[e];
    return ar.from_u64(sub_mod(barrett128(0, add_mod(x, h, qL), mc), hm, mc.q));
  }
}

// ---------------------------------------------------------------------------
// radix-4 form: a thread owns 4 elements and runs two stages per
// LDS exchange (two butterflies per stage), so a pass has half the barriers
// and exchanges of the one-butterfly form with half the threads.  Step on
// bits (b, b - 1) (forward) or (b, b + 1) (inverse) over elements
//   e0 = j with two zero bits inserted at those positions, e1 = e0 + 2^lo_bit,
//   e2 = e0 + 2^hi_bit, e3 = e2 + 2^lo_bit.
// An odd stage count ends (forward) or ends (inverse) with one radix-2 stage.
// A forward columns pass starts on, and an inverse columns pass ends on, the
// set {j, j + 2^(R-2), j + 2^(R-1), j + 3 2^(R-2)} -- so ntt2s_ifwd_cols_p needs
// no exchange between its inverse and forward halves.
// ---------------------------------------------------------------------------
// forward columns pass, radix 4: thread (cl, j), j < 2^(R-2)
// the twiddles of thread row j's forward columns stages (wa/wb/wc per radix-4
// step, wl for an odd last stage)
template <class A, int LOGN>
__device__ __forceinline__ void s_fwd_cols4_tw(const A& ar, __amdgpu_buffer_rsrc_t tw, int j,
                                               typename A::W (&wa)[S2<LOGN>::R / 2],
                                               typename A::W (&wb)[S2<LOGN>::R / 2],
                                               typename A::W (&wc)[S2<LOGN>::R / 2], typename A::W (&wl)[2]) {
  constexpr int N = 1 << LOGN, R = S2<LOGN>::R, NS = R / 2;
#pragma unroll
  for (int st = 0; st < NS; ++st) {
    const int hb = R - 1 - 2 * st, g = j >> (hb - 1);
    wa[st] = ar.tw(tw, g, N >> (hb + 9));
    wb[st] = ar.tw(tw, 2 * g, N >> (hb + 8));
    wc[st] = ar.tw(tw, 2 * g + 1, N >> (hb + 8));
  }
  if (R & 1) wl[0] = ar.tw(tw, 2 * j, N >> 9), wl[1] = ar.tw(tw, 2 * j + 1, N >> 9);
}
template <class A, int LOGN>
__device__ __forceinline__ void s_fwd_cols4_run(const NttIO& io, int c, int l, int b, int tile,
                                                typename A::T (&x)[4], const A& ar,
                                                const typename A::W (&wa)[S2<LOGN>::R / 2],
                                                const typename A::W (&wb)[S2<LOGN>::R / 2],
                                                const typename A::W (&wc)[S2<LOGN>::R / 2],
                                                const typename A::W (&wl)[2], u64* lds, int t) {
  constexpr int R = S2<LOGN>::R, CW = S2<LOGN>::CW, NS = R / 2;
  const int cl = t % CW, j = t / CW, col = tile * CW + cl;
  // (wave-uniform; formed ahead of the stages: formed at the store, the
  // N = 2^16 ntt2s_ifwd_cols_p kernels took 66 VGPRs, 7 waves instead of 8)
  u64* mid = row_ptr(io.mid, c, l, b);
#pragma unroll
  for (int st = 0; st < NS; ++st) {
    const int hb = R - 1 - 2 * st, lb = hb - 1;
    const int e0 = ins2(j, lb), e1 = e0 + (1 << lb), e2 = e0 + (1 << hb), e3 = e2 + (1 << lb);
    if (st > 0) {
      x[0] = from_bits<typename A::T>(lds[e0 * CW + cl]);
      x[1] = from_bits<typename A::T>(lds[e1 * CW + cl]);
      x[2] = from_bits<typename A::T>(lds[e2 * CW + cl]);
      x[3] = from_bits<typename A::T>(lds[e3 * CW + cl]);
    }
    ct4(ar, x, wa[st], wb[st], wc[st]);
    if (st == 1)  // after 4 stages (float64: |x| stays below 16q)
      for (int i = 0; i < 4; ++i) x[i] = ar.reduce_round(x[i]);
    if (st < NS - 1 || (R & 1)) {
      lds[e0 * CW + cl] = to_bits(x[0]);
      lds[e1 * CW + cl] = to_bits(x[1]);
      lds[e2 * CW + cl] = to_bits(x[2]);
      lds[e3 * CW + cl] = to_bits(x[3]);
      __syncthreads();
    }
  }
  if (R & 1) {  // the last stage (bit 0): pairs (4j, 4j + 1), (4j + 2, 4j + 3)
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = from_bits<typename A::T>(lds[(4 * j + i) * CW + cl]);
    ar.ct(x[0], x[1], wl[0]);
    ar.ct(x[2], x[3], wl[1]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) mid[col + ((4 * j + i) << 8)] = to_bits(ar.reduce_round(x[i]));
}
template <class A, int LOGN>
__device__ __forceinline__ void s_fwd_cols4_core(const NttIO& io, int c, int l, int b, int tile,
                                                 typename A::T (&x)[4], const A& ar, __amdgpu_buffer_rsrc_t tw,
                                                 u64* lds, int t) {
  constexpr int NS = S2<LOGN>::R / 2;
  typename A::W wa[NS], wb[NS], wc[NS], wl[2];
  s_fwd_cols4_tw<A, LOGN>(ar, tw, t / S2<LOGN>::CW, wa, wb, wc, wl);
  s_fwd_cols4_run<A, LOGN>(io, c, l, b, tile, x, ar, wa, wb, wc, wl, lds, t);
}
template <class A, int LOGN, int PRO>
__device__ __forceinline__ void s_fwd_cols4(const NttIO& io, int c, int l, int b, int tile,
                                            const ModConst& mc, const A& ar, __amdgpu_buffer_rsrc_t tw, u64* lds,
                                            const DeviceTables* __restrict__ tb) {
  constexpr int R = S2<LOGN>::R, CW = S2<LOGN>::CW, Q = 1 << (R - 2);
  const int t = threadIdx.x, cl = t % CW, j = t / CW, col = tile * CW + cl;
  typename A::T x[4];
  if constexpr (PRO == NTT_PRO_BEXT) {
    // the extension's constants once per thread, through the scalar cache (bext2_load)
    const int k = arg_byte(io.bx_tab, l), ti = arg_byte(io.bx_t, l), s0 = arg_byte(io.bx_s0, k);
    const Bext2 bc = bext2_load(io.bx + k, ti);
    const u64* p0 = row_ptr(io.src, c, s0, b);
    const u64* p1 = row_ptr(io.src, c, s0 + (bc.ns > 1 ? 1 : 0), b);
    u64 x0[4], x1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x0[i] = p0[col + ((j + i * Q) << 8)];
      x1[i] = bc.ns > 1 ? p1[col + ((j + i * Q) << 8)] : 0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = ar.from_u64(bext2_apply(bc, x0[i], x1[i]));
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = fwd_load<A, PRO>(io, c, l, b, col + ((j + i * Q) << 8), mc, ar, tb);
  }
  s_fwd_cols4_core<A, LOGN>(io, c, l, b, tile, x, ar, tw, lds, (int)threadIdx.x);
}

// forward rows pass, radix 4: thread (rr, kk), kk < 64
template <class A, int LOGN, int EPI>
__device__ __forceinline__ void s_fwd_rows4(const NttIO& io, int c, int l, int b, int tile, const ModConst& mc,
                                            const A& ar, __amdgpu_buffer_rsrc_t tw, u64* lds) {
  const int t = threadIdx.x, rr = t >> 6, kk = t & 63, row = tile * S2<LOGN>::RW + rr;
  const u64* mid = row_ptr(io.mid, c, l, b) + (row << 8);
  typename A::T x[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] = from_bits<typename A::T>(mid[kk + 64 * i]);
  typename A::W wa[4], wb[4], wc[4];
  fwd_rows4_tw<A, LOGN>(row, kk, ar, tw, wa, wb, wc);
  // the epilogue's operands are loaded before the steps, so their latency
  // overlaps them: ex, the scatter index and (_ACC) the words at aut[e] (aut
  // is a permutation: no other thread of the launch writes them)
  [[maybe_unused]] ulonglong2 e01, e23;
  [[maybe_unused]] uint4 ix;
  [[maybe_unused]] u64 dv[4];
  if constexpr (EPI != NTT_EPI_STORE) {
    const u64* ex = row_ptr(io.ex, c, l, b) + (row << 8) + 4 * kk;
    e01 = *(const ulonglong2*)ex, e23 = *(const ulonglong2*)(ex + 2);
  }
  u64* const d = row_ptr(io.dst, c, l, b);
  if constexpr (epi_aut(EPI)) {
    ix = *(const uint4*)(io.aut + (row << 8) + 4 * kk);
    if constexpr (EPI == NTT_EPI_SUBSCALE_AUT_ACC) dv[0] = d[ix.x], dv[1] = d[ix.y], dv[2] = d[ix.z], dv[3] = d[ix.w];
  }
  fwd_rows4_run<A>(x, kk, ar, wa, wb, wc, lds + rr * 256);
  // the last step's elements: columns 4kk .. 4kk + 3
  u64* dst = d + (row << 8) + 4 * kk;
  u64 o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = ar.final_fwd(x[i]);
  if constexpr (EPI != NTT_EPI_STORE) {  // dst = (ex - y) * s_l
    const u64 ev[4] = {e01.x, e01.y, e23.x, e23.y};
    const u64 s = io.s[l], ss = io.ss[l];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = shoup_mul(sub_mod(ev[i], o[i], mc.q), s, ss, mc.q);
  }
  if constexpr (epi_aut(EPI)) {  // element e to position aut[e] (added to the word there for _ACC)
    if constexpr (EPI == NTT_EPI_SUBSCALE_AUT_ACC) {
      o[0] = add_mod(o[0], dv[0], mc.q);
      o[1] = add_mod(o[1], dv[1], mc.q);
      o[2] = add_mod(o[2], dv[2], mc.q);
      o[3] = add_mod(o[3], dv[3], mc.q);
    }
    d[ix.x] = o[0];
    d[ix.y] = o[1];
    d[ix.z] = o[2];
    d[ix.w] = o[3];
    return;
  }
  *(ulonglong2*)dst = make_ulonglong2(o[0], o[1]);
  *(ulonglong2*)(dst + 2) = make_ulonglong2(o[2], o[3]);
}

// inverse rows pass, radix 4 (first): steps on bits (0, 1) .. (6, 7)
// (inv_rows4_core, ntt2s_rows.h)
template <class A, int LOGN>
__device__ __forceinline__ void s_inv_rows4(const NttIO& io, int c, int l, int b, int tile, const A& ar,
                                            __amdgpu_buffer_rsrc_t tw, u64* lds) {
  const int t = threadIdx.x, rr = t >> 6, kk = t & 63, row = tile * S2<LOGN>::RW + rr;
  const u64* src = row_ptr(io.src, c, l, b) + (row << 8) + 4 * kk;
  const ulonglong2 v01 = *(const ulonglong2*)src, v23 = *(const ulonglong2*)(src + 2);
  typename A::T x[4] = {ar.from_u64(v01.x), ar.from_u64(v01.y), ar.from_u64(v23.x), ar.from_u64(v23.y)};
  inv_rows4_core<A, LOGN>(x, row, kk, ar, tw, lds + rr * 256, row_ptr(io.mid, c, l, b) + (row << 8));
}

// inverse columns pass, radix 4 (second) of one limb's column tile, kept in
// registers; ends on the forward's first set
template <class A, int LOGN>
__device__ __forceinline__ void s_inv_cols4_src(const u64* m, const A& ar, __amdgpu_buffer_rsrc_t tw, u64* lds,
                                                typename A::T (&x)[4], int t, int tile) {
  constexpr int N = 1 << LOGN, R = S2<LOGN>::R, CW = S2<LOGN>::CW, NS = R / 2, Q = 1 << (R - 2);
  const int cl = t % CW, j = t / CW, col = tile * CW + cl;
  typename A::W wa[NS], wb[NS], wc[NS], wl;
#pragma unroll
  for (int st = 0; st < NS; ++st) {
    const int lb = 2 * st, g = j >> lb;
    wa[st] = ar.tw(tw, 2 * g, N >> (lb + 9));
    wb[st] = ar.tw(tw, 2 * g + 1, N >> (lb + 9));
    wc[st] = ar.tw(tw, g, N >> (lb + 10));
  }
  if (R & 1) wl = ar.tw(tw, 0, N >> (R + 8));  // the last stage (bit R - 1): one twiddle
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] = from_bits<typename A::T>(m[col + ((4 * j + i) << 8)]);
#pragma unroll
  for (int st = 0; st < NS; ++st) {
    const int lb = 2 * st, hb = lb + 1;
    const int e0 = ins2(j, lb), e1 = e0 + (1 << lb), e2 = e0 + (1 << hb), e3 = e2 + (1 << lb);
    const int e[4] = {e0, e1, e2, e3};
    if (st > 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = from_bits<typename A::T>(lds[e[i] * CW + cl]);
    }
    gs4(ar, x, wa[st], wb[st], wc[st], false, true);
    if (st < NS - 1 || (R & 1)) {
#pragma unroll
      for (int i = 0; i < 4; ++i) lds[e[i] * CW + cl] = to_bits(x[i]);
      __syncthreads();
    }
  }
  if (R & 1) {  // bit R - 1: pairs (j, j + 2Q), (j + Q, j + 3Q); the sum is not reduced (stage R - 1 even)
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = from_bits<typename A::T>(lds[(j + i * Q) * CW + cl]);
    ar.gs(x[0], x[2], wl, ((R - 1) & 1) == 1);
    ar.gs(x[1], x[3], wl, ((R - 1) & 1) == 1);
  }
}

// forward columns pass of a launch whose sources skipped the inverse's columns
// pass (NttIO.ifuse): the sources' INTT is finished on the workgroup's column
// tile, the prologue (the basis extension, or the rescale prep) is formed from
// registers, and the forward columns stages run -- the INTT output never goes
// to HBM and its second launch disappears.  The sources' INTT columns are
// shared by a segment of G targets (NttIO.tgroup = G; targets that read the
// same source limbs): a workgroup of G groups of 256 threads per (row, segment,
// column tile) runs the sources' INTT columns once -- source s on group s,
// concurrently -- then every group forms its own target's prologue from the
// shared values and runs that target's forward columns stages, on as many
// threads per workgroup as targets.  (G = 2 ships: four groups measured +8 %,
// r05r.)
template <int LOGN>
__device__ __forceinline__ void idle_inv_cols4_barriers() {  // the barriers of s_inv_cols4_src
  constexpr int R = S2<LOGN>::R, NS = R / 2;
#pragma unroll
  for (int k = 0; k < NS - 1 + (R & 1); ++k) __syncthreads();
}
template <int LOGN, int PRO, int G>
__global__ void __launch_bounds__(G * S2<LOGN>::CT4) ntt2s_ifwd_cols_p(NttIO io, const DeviceTables* __restrict__ tb) {
  constexpr int CT = S2<LOGN>::CT4, REG = S2<LOGN>::CW << S2<LOGN>::R;  // LDS words per group
  __shared__ u64 lds[G * REG + 2 * 4 * CT];
  u64* const sb = lds + G * REG;  // the sources' INTT values, [source][element][thread]
  // BEXT: the sources' y_i (in sb) and float-quotient terms, formed once per
  // source in phase 1 instead of once per target in phase 2
  [[maybe_unused]] __shared__ double sf[PRO == NTT_PRO_BEXT ? 2 * 4 * CT : 1];
  const int grp = threadIdx.x / CT, t = threadIdx.x % CT;  // (group-uniform, so wave-uniform)
  const int tile = blockIdx.x % S2<LOGN>::CTILES, q = blockIdx.x / S2<LOGN>::CTILES;
  const int seg = q % io.ntg, row = q / io.ntg;
  const int b = row % io.dst.nbatch, c = row / io.dst.nbatch;
  // surplus groups of a short segment redo its last target (identical stores)
  const int l = arg_byte(io.tg_l0, seg) + min(grp, arg_byte(io.tg_n, seg) - 1);
  int sl0 = 0, ns = 1, ti = 0;
  const BasisExtTable* __restrict__ T = nullptr;
  if constexpr (PRO == NTT_PRO_BEXT) {
    const int kt = arg_byte(io.bx_tab, l);
    ti = arg_byte(io.bx_t, l);
    sl0 = arg_byte(io.bx_s0, kt);
    T = io.bx + kt;
    ns = T->ns;
  }
  // the extension's constants, in SGPRs before the INTT half (bext2_load)
  [[maybe_unused]] Bext2 bc;
  if constexpr (PRO == NTT_PRO_BEXT) bc = bext2_load(T, ti);
  const int mod = arg_byte(io.dst.mod, l);
  const ModConst mc = tb->mc[mod];
  // phase 1: group s < ns finishes source s's INTT columns on this tile
  if (grp < ns) {
    const int ms = arg_byte(io.src.mod, sl0 + grp);
    const u64* p = row_ptr(io.imid, c, sl0 + grp, b);
    const ModConst& mcs = tb->mc[ms];
    auto inv = [&](const auto& ar, __amdgpu_buffer_rsrc_t tw) {
      using A = std::decay_t<decltype(ar)>;
      typename A::T x[4];
      s_inv_cols4_src<A, LOGN>(p, ar, tw, lds + grp * REG, x, t, tile);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        u64 xv = ar.final_inv(x[i]);
        if constexpr (PRO == NTT_PRO_BEXT) {
          if (!bc.centered) {  // (grp wave-uniform: constant table indices on each branch)
            double f;
            xv = __builtin_amdgcn_readfirstlane(grp) == 0 ? bext2_src(bc, 0, xv, f) : bext2_src(bc, 1, xv, f);
            sf[(grp * 4 + i) * CT + t] = f;
          }
        }
        sb[(grp * 4 + i) * CT + t] = xv;
      }
    };
    if (mcs.f64)
      inv(F64Arith(mcs), twr_s(tb->inv_d[ms], 8 << LOGN));
    else
      inv(IntArith(mcs), twr_s(tb->inv[ms], 16 << LOGN));
  } else {
    idle_inv_cols4_barriers<LOGN>();
  }
  __syncthreads();  // sb complete; the group regions are free for the forward stages
  u64 o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u64 v0 = sb[i * CT + t];
    if constexpr (PRO == NTT_PRO_BEXT) {
      const u64 y1 = ns > 1 ? sb[(4 + i) * CT + t] : 0;
      const double f0 = bc.centered ? 0.0 : sf[i * CT + t];
      const double f1 = (bc.centered || ns < 2) ? 0.0 : sf[(4 + i) * CT + t];
      o[i] = bext2_tgt(bc, v0, y1, bext2_v(bc, v0, f0, f1));
    } else {  // NTT_PRO_RESCALE
      const u64 qL = tb->mc[io.modL].q, h = qL >> 1;
      const u64 hm = barrett128(0, h, mc);
      o[i] = sub_mod(barrett128(0, add_mod(v0, h, qL), mc), hm, mc.q);
    }
  }
  auto fwd = [&](const auto& ar, __amdgpu_buffer_rsrc_t tw) {
    using A = std::decay_t<decltype(ar)>;
    typename A::T x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = ar.from_u64(o[i]);
    s_fwd_cols4_core<A, LOGN>(io, c, l, b, tile, x, ar, tw, lds + grp * REG, t);
  };
  if (mc.f64)
    fwd(F64Arith(mc), twr_s(tb->fwd_d[mod], 8 << LOGN));
  else
    fwd(IntArith(mc), twr_s(tb->fwd[mod], 16 << LOGN));
}

// ---------------------------------------------------------------------------
// kernels: blockIdx.x = job * tiles + tile
// ---------------------------------------------------------------------------
template <int LOGN, int PRO>
__global__ void __launch_bounds__(S2<LOGN>::CT4)
    ntt2s_fwd_cols(NttIO io, const DeviceTables* __restrict__ tb) {
  __shared__ u64 lds[S2<LOGN>::CW << S2<LOGN>::R];
  const int job = blockIdx.x / S2<LOGN>::CTILES, tile = blockIdx.x % S2<LOGN>::CTILES;
  int c, l, b;
  job_of(io, job, c, l, b);
  const int mod = arg_byte(io.dst.mod, l);
  const ModConst mc = tb->mc[mod];
  if (mc.f64)
    s_fwd_cols4<F64Arith, LOGN, PRO>(io, c, l, b, tile, mc, F64Arith(mc), twr_s(tb->fwd_d[mod], 8 << LOGN), lds, tb);
  else
    s_fwd_cols4<IntArith, LOGN, PRO>(io, c, l, b, tile, mc, IntArith(mc), twr_s(tb->fwd[mod], 16 << LOGN), lds, tb);
}

template <int LOGN, int EPI>
__global__ void __launch_bounds__(S2<LOGN>::RT4)
    ntt2s_fwd_rows(NttIO io, const DeviceTables* __restrict__ tb) {
  __shared__ u64 lds[S2<LOGN>::RW * 256];
  const int job = blockIdx.x / S2<LOGN>::RTILES, tile = blockIdx.x % S2<LOGN>::RTILES;
  int c, l, b;
  job_of(io, job, c, l, b);
  const int mod = arg_byte(io.dst.mod, l);
  const ModConst mc = tb->mc[mod];
  if (mc.f64)
    s_fwd_rows4<F64Arith, LOGN, EPI>(io, c, l, b, tile, mc, F64Arith(mc), twr_s(tb->fwd_d[mod], 8 << LOGN), lds);
  else
    s_fwd_rows4<IntArith, LOGN, EPI>(io, c, l, b, tile, mc, IntArith(mc), twr_s(tb->fwd[mod], 16 << LOGN), lds);
}

template <int LOGN>
__global__ void __launch_bounds__(S2<LOGN>::RT4)
    ntt2s_inv_rows(NttIO io, const DeviceTables* __restrict__ tb) {
  __shared__ u64 lds[S2<LOGN>::RW * 256];
  const int job = blockIdx.x / S2<LOGN>::RTILES, tile = blockIdx.x % S2<LOGN>::RTILES;
  int c, l, b;
  job_of(io, job, c, l, b);
  const int mod = arg_byte(io.dst.mod, l);
  const ModConst mc = tb->mc[mod];
  if (mc.f64)
    s_inv_rows4<F64Arith, LOGN>(io, c, l, b, tile, F64Arith(mc), twr_s(tb->inv_d[mod], 8 << LOGN), lds);
  else
    s_inv_rows4<IntArith, LOGN>(io, c, l, b, tile, IntArith(mc), twr_s(tb->inv[mod], 16 << LOGN), lds);
}

template <int LOGN>
__global__ void __launch_bounds__(S2<LOGN>::CT4)
    ntt2s_inv_cols(NttIO io, const DeviceTables* __restrict__ tb) {
  __shared__ u64 lds[S2<LOGN>::CW << S2<LOGN>::R];
  const int job = blockIdx.x / S2<LOGN>::CTILES, tile = blockIdx.x % S2<LOGN>::CTILES;
  int c, l, b;
  job_of(io, job, c, l, b);
  const int mod = arg_byte(io.dst.mod, l);
  const ModConst mc = tb->mc[mod];
  auto inv = [&](const auto& ar, __amdgpu_buffer_rsrc_t tw) {
    using A = std::decay_t<decltype(ar)>;
    constexpr int CW = S2<LOGN>::CW, Q = 1 << (S2<LOGN>::R - 2);
    const int t = threadIdx.x, cl = t % CW, j = t / CW, col = tile * CW + cl;
    typename A::T x[4];
    s_inv_cols4_src<A, LOGN>(row_ptr(io.mid, c, l, b), ar, tw, lds, x, t, tile);
    u64* dst = row_ptr(io.dst, c, l, b);
#pragma unroll
    for (int i = 0; i < 4; ++i) dst[col + ((j + i * Q) << 8)] = ar.final_inv(x[i]);
  };
  if (mc.f64)
    inv(F64Arith(mc), twr_s(tb->inv_d[mod], 8 << LOGN));
  else
    inv(IntArith(mc), twr_s(tb->inv[mod], 16 << LOGN));
}

template <int LOGN>
int launch2s(const NttIO& io, const DeviceTables* tb, bool inverse, bool rows_only, hipStream_t st) {
  const int total = io.dst.ncomp * io.dst.nlimb * io.dst.nbatch;
  if (total == 0) return 0;
  if (io.jobs != total || io.ci) return -1;
  const dim3 ga(total * S2<LOGN>::CTILES), ba(S2<LOGN>::CT4), gb(total * S2<LOGN>::RTILES), bb(S2<LOGN>::RT4);
  if (inverse) {
    if (io.pro != NTT_PRO_LOAD || io.epi != NTT_EPI_STORE) return -1;
    hipLaunchKernelGGL(ntt2s_inv_rows<LOGN>, gb, bb, 0, st, io, tb);
    // rows_only: the columns pass is left to the forward launch that consumes
    // this INTT (NttIO.ifuse; the intermediate stays in io.mid)
    if (!rows_only) hipLaunchKernelGGL(ntt2s_inv_cols<LOGN>, ga, ba, 0, st, io, tb);
    return 0;
  }
  if (io.ifuse) {  // the sources' INTT columns shared by pairs of targets
    if (io.tgroup != 2 || !io.imid.p || io.ntg < 1) return -1;
    const dim3 gg(io.dst.ncomp * io.dst.nbatch * io.ntg * S2<LOGN>::CTILES), bg(2 * S2<LOGN>::CT4);
    if (io.pro == NTT_PRO_BEXT)
      hipLaunchKernelGGL((ntt2s_ifwd_cols_p<LOGN, NTT_PRO_BEXT, 2>), gg, bg, 0, st, io, tb);
    else if (io.pro == NTT_PRO_RESCALE)
      hipLaunchKernelGGL((ntt2s_ifwd_cols_p<LOGN, NTT_PRO_RESCALE, 2>), gg, bg, 0, st, io, tb);
    else
      return -1;
  } else if (io.pro == NTT_PRO_LOAD)
    hipLaunchKernelGGL((ntt2s_fwd_cols<LOGN, NTT_PRO_LOAD>), ga, ba, 0, st, io, tb);
  else if (io.pro == NTT_PRO_BEXT)
    hipLaunchKernelGGL((ntt2s_fwd_cols<LOGN, NTT_PRO_BEXT>), ga, ba, 0, st, io, tb);
  else if (io.pro == NTT_PRO_RESCALE)
    hipLaunchKernelGGL((ntt2s_fwd_cols<LOGN, NTT_PRO_RESCALE>), ga, ba, 0, st, io, tb);
  else
    return -1;
  if (io.cols_only) {  // the rows pass runs in the consumer
    if (io.epi != NTT_EPI_STORE) return -1;
    return 0;
  }
  if (io.epi == NTT_EPI_STORE)
    hipLaunchKernelGGL((ntt2s_fwd_rows<LOGN, NTT_EPI_STORE>), gb, bb, 0, st, io, tb);
  else if (io.epi == NTT_EPI_SUBSCALE)
    hipLaunchKernelGGL((ntt2s_fwd_rows<LOGN, NTT_EPI_SUBSCALE>), gb, bb, 0, st, io, tb);
  else if (io.epi == NTT_EPI_SUBSCALE_AUT && io.aut)
    hipLaunchKernelGGL((ntt2s_fwd_rows<LOGN, NTT_EPI_SUBSCALE_AUT>), gb, bb, 0, st, io, tb);
  else if (io.epi == NTT_EPI_SUBSCALE_AUT_ACC && io.aut)
    hipLaunchKernelGGL((ntt2s_fwd_rows<LOGN, NTT_EPI_SUBSCALE_AUT_ACC>), gb, bb, 0, st, io, tb);
  else
    return -1;
  return 0;
}

}  // namespace

// host entry: two launches on stream st (same contract as orion_launch_ntt2);
// inverse with rows_only: the rows pass alone (its columns pass then runs
// inside the forward launch that reads this INTT, NttIO.ifuse)
int orion_launch_ntt2s(int logN, const NttIO& io, const DeviceTables* tb, bool inverse, hipStream_t st,
                       bool rows_only) {
  if (rows_only && !inverse) return -1;
  switch (logN) {
    case 15: return launch2s<15>(io, tb, inverse, rows_only, st);
    case 16: return launch2s<16>(io, tb, inverse, rows_only, st);
    default: return -1;
  }
}
