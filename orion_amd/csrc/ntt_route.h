// ntt_route.h -- where every NTT launch route is decided.  Host only: integers
// in, a route value out; no HIP types, no Context, no allocation.  An
// operation's entry point computes its route once (Context::ks_route, lt_route,
// moddown_route, rescale_route) and the stages below it build their NttIOs
// from that value; ntt_io alone asks ntt_family for a finished NttIO.
#pragma once
#include <algorithm>
#include <cstdlib>
#include "ntt_consts.h"

// the launch-path switches, read once per Context (every pipeline context
// reads the environment at its creation)
struct NttTuning {
  // 1: one limb per workgroup (ntt.hip); 2: two-pass N = 2^15 kernels (ntt2.hip)
  int ntt_impl = 1;
  // N = 2^15 launches with fewer limb-transforms than this use the two-pass
  // kernels: one limb per CU leaves most of the 256 CUs idle there (8 jobs:
  // 15 vs 37 us; 64 jobs: 32 vs 40 us, float64 path).  Batched launches
  // (>= 128 jobs at 64 images) keep the one-pass kernel.
  int ntt2_below = 128;
  // two-pass launches of at most this many limb-transforms use the
  // latency-oriented kernels of ntt2s.hip (one butterfly per thread per
  // stage, the tile in LDS) instead of ntt2.hip's 16-point threads
  int ntt2s_below = 128;
  // N = 2^15 inverse launches up to ntt2_tail_max limb-transforms whose last
  // round of one-limb workgroups would be partial (jobs / (rounds * CUs) below
  // ntt2_tail_eff) also take the two-pass kernels: a one-pass round costs one
  // limb's latency on every CU whether or not the CU has a job, while the
  // two-pass kernels scale with the job count (tools/ntt_bench.py, mixed
  // moduli, inverse: 192 jobs 61 vs 76 us, 384 jobs 98 vs 127 us).  Forward
  // launches keep the one-pass kernel: their fused epilogues cost the
  // two-pass kernels a scratch round trip, and the LoLA bench measured them
  // slower (profiles/r01z_ntt2_tailfwd_ab.txt)
  double ntt2_tail_eff = 0.9;
  int ntt2_tail_max = 1024;
  // 1: plain forward launches (load prologue, store epilogue) follow the same
  // rule; 2: every forward launch that needs no scratch (not an in-place tail)
  int ntt2_tail_fwd = 1;
  // 1: ModUp and ModDown form the extended limbs in the forward NTT's prologue
  // (NTT_PRO_BEXT) instead of a basis_ext / modup_all launch whose output the
  // NTT reads back (sources of at most 2 limbs, Standard ring), when the NTT
  // runs on the two-pass kernels (bext_in_prologue); 0: never
  int bext_fuse = 1;
  // (see bext_in_prologue)
  int bext_fuse_below = 64;
  // 1: an INTT whose output feeds only the prologue of the forward NTT that
  // follows (ModUp and ModDown sources, the rescale's last limb) runs its rows
  // pass alone when both launches take the latency kernels (ntt2s.hip); the
  // forward launch finishes the INTT's columns pass on its own column tile
  // (ntt2s_ifwd_cols_p), so the INTT output never goes to HBM and its second
  // launch disappears
  int ntt_ifuse = 1;
  // ... as long as the sources' columns pass is not redone too often: every
  // pair of targets redoes it for its own sources, (targets x sources per
  // target) / source limbs times the INTT's own columns work (ResNet's
  // N = 2^16 ModDowns onto 20-30 Q limbs measured slower fused)
  double ntt_ifuse_maxr = 8.0;
  // 1: a rotation's NTT-domain automorphism is applied in the ModDown's final
  // NTT store (NTT_EPI_SUBSCALE_AUT) where the kernel supports it
  int ntt_aut_fuse = 1;
  // decompositions with fewer limb-transforms per digit than this run every
  // digit's ModUp + NTT as one launch pair (0 = always per digit)
  int modup_merge = 256;
  // 1: keyswitch's gadget product stores the P limbs through the ModDown
  // INTT's rows pass when the ModDown takes the fused latency path
  int mac_rows = 1;
  // 1: ... and runs the decomposition NTT's forward rows pass itself
  int mac_fwd_rows = 1;
  // ORION_DEFER (0: off): the deferred rotate-and-add and RescaleNew's
  // aliasing (deferral.h, backend.hip alias), and here the ModDown left pending for a
  // rescale that may follow (KsEnd::KeepQP)
  bool defer = true;

  static NttTuning from_env() {
    NttTuning t;
    auto geti = [](const char* v, int& x) { if (v) x = atoi(v); };
    auto getd = [](const char* v, double& x) { if (v) x = atof(v); };
    geti(getenv("ORION_NTT_IMPL"), t.ntt_impl);
    geti(getenv("ORION_NTT2_BELOW"), t.ntt2_below);
    geti(getenv("ORION_NTT2S_BELOW"), t.ntt2s_below);
    getd(getenv("ORION_NTT2_TAIL_EFF"), t.ntt2_tail_eff);
    geti(getenv("ORION_NTT2_TAIL_MAX"), t.ntt2_tail_max);
    geti(getenv("ORION_NTT2_TAIL_FWD"), t.ntt2_tail_fwd);
    geti(getenv("ORION_BEXT_FUSE"), t.bext_fuse);
    geti(getenv("ORION_BEXT_FUSE_BELOW"), t.bext_fuse_below);
    geti(getenv("ORION_NTT_IFUSE"), t.ntt_ifuse);
    getd(getenv("ORION_NTT_IFUSE_MAXR"), t.ntt_ifuse_maxr);
    geti(getenv("ORION_NTT_AUT_FUSE"), t.ntt_aut_fuse);
    geti(getenv("ORION_MODUP_MERGE"), t.modup_merge);
    geti(getenv("ORION_MAC_ROWS"), t.mac_rows);
    geti(getenv("ORION_MAC_FWD_ROWS"), t.mac_fwd_rows);
    if (const char* v = getenv("ORION_DEFER")) t.defer = atoi(v) != 0;
    return t;
  }
};

// what the rules depend on besides the launch itself; filled once at
// init_moduli (n_cu from the device attribute query there)
struct NttEnv {
  int logN = 0;
  bool ci = false;   // ConjugateInvariant ring
  int K = 0;         // P primes
  int n_cu = 0;      // compute units
  int max_limb = 0, max_src = 0, max_group = 0;  // ORION_MAXLIMB, ORION_MAXSRC, ORION_MAXGROUP (common.h)
};

// the kernel family of one NTT launch; the numbers are ORION_NTT_LOG's family field
enum NttFamily { OnePass = 1, TwoPass = 2, Latency = 3 };

// N = 2^16 always leaves the one-pass kernel; N = 2^15 (Standard ring) for
// small launches and for partial last rounds of inverse and plain forward
// launches (NttTuning::ntt2_tail_*); then launches of at most ntt2s_below
// limb-transforms take the latency kernels.  inplace_sub: a subtract-and-scale
// epilogue whose operand is the destination (Context::inplace_sub)
inline NttFamily ntt_family(const NttEnv& e, const NttTuning& t, int jobs, bool inv, int pro, int epi,
                            bool inplace_sub) {
  bool two = e.logN == 16;
  if (!two && e.logN == 15 && !e.ci) {
    two = t.ntt_impl == 2 || jobs < t.ntt2_below;
    const bool plain = (pro == NTT_PRO_LOAD || pro == NTT_PRO_BEXT) && epi == NTT_EPI_STORE;
    if (!two && (inv || (t.ntt2_tail_fwd == 1 && plain) || (t.ntt2_tail_fwd == 2 && !inplace_sub)) &&
        jobs <= t.ntt2_tail_max && t.ntt2_tail_eff > 0) {
      const int rounds = (jobs + e.n_cu - 1) / e.n_cu;
      two = (double)jobs / ((double)rounds * e.n_cu) < t.ntt2_tail_eff;
    }
  }
  return !two ? OnePass : jobs <= t.ntt2s_below ? Latency : TwoPass;
}

// the fused basis extension (NTT_PRO_BEXT) pays on the two-pass kernels
// only: in the one-pass kernel, one CU per limb, every target re-forms the
// shared y_i and float quotient and loads ns source limbs in its memory
// phase, and the LoLA step took 36.8 instead of 30.6 ms
// (profiles/r04c_bext_fuse_ab.txt); on the two-pass kernels batch 1 went
// from 3.0 to 2.84 ms per image
// and at B = 64 LoLA its partial-round two-pass launches were neutral to
// -0.5% (2089 / 2091 vs 2105 / 2097 img/s, profiles/r04d_bext_fuse_ab.txt),
// so it is kept to small launches (bext_fuse_below limb-transforms).
// ns: the most source limbs of one target
inline bool bext_in_prologue(const NttEnv& e, const NttTuning& t, int jobs, int ns, int epi, bool inplace_sub) {
  return t.bext_fuse && ns <= 2 && !e.ci && jobs <= t.bext_fuse_below &&
         ntt_family(e, t, jobs, false, NTT_PRO_BEXT, epi, inplace_sub) != OnePass;
}

// whether the forward NTT of jobs limb-transforms with prologue pro runs on
// a kernel with the automorphism-scatter epilogue (NTT_EPI_SUBSCALE_AUT):
// the one-pass kernel with the load prologue, or the radix-4 latency kernels
// (the large two-pass kernels, ntt2.hip, have no scatter epilogue)
inline bool scatter_epilogue(const NttEnv& e, const NttTuning& t, int jobs, int pro) {
  if (e.ci) return false;
  const NttFamily f = ntt_family(e, t, jobs, false, pro, NTT_EPI_SUBSCALE_AUT, false);
  if (f == OnePass) return e.logN <= 15 && pro == NTT_PRO_LOAD;
  return jobs <= t.ntt2s_below;
}

// an INTT (load, store) followed by the forward NTT whose BEXT / RESCALE
// prologue reads only the INTT's output (Context::intt_then_fwd)
struct InvFwdRoute {
  bool ifuse = false;        // the INTT's rows pass alone, its columns pass inside the forward's latency kernels
  int tgroup = 0;            // ifuse: 2, the targets per workgroup sharing their sources' columns pass
  bool rows_stored = false;  // ifuse: the producer's kernel already stored the rows pass' intermediate
};
// src_limbs -> dst_limbs limbs over nimg = components x images; ns_max: the
// most source limbs one target reads
inline InvFwdRoute inv_fwd_route(const NttEnv& e, const NttTuning& t, int nimg, int src_limbs, int dst_limbs,
                                 int ns_max, int pro, int epi, bool inplace_sub) {
  InvFwdRoute r;
  const double redo = (double)dst_limbs * ns_max / std::max(1, src_limbs);
  r.ifuse = t.ntt_ifuse && !e.ci && redo <= t.ntt_ifuse_maxr && (pro == NTT_PRO_BEXT || pro == NTT_PRO_RESCALE) &&
            ntt_family(e, t, nimg * src_limbs, true, NTT_PRO_LOAD, NTT_EPI_STORE, false) == Latency &&
            ntt_family(e, t, nimg * dst_limbs, false, pro, epi, inplace_sub) == Latency;
  if (r.ifuse) r.tgroup = 2;
  return r;
}

// ModDown of nc components, B images at `level`.  aut: 0 none, 1 the result
// permuted by an automorphism, 2 and added to the output; aliased: the output
// is the input's Q limbs; producer_rows: the kernel before it can store the P
// limbs through the INTT's rows pass (ks_mac_rows, lt_giant)
struct ModDownRoute {
  bool bext_pro = false;  // the basis extension in the NTT's prologue (else its own launch)
  bool scatter = false;   // aut: in the NTT's store (else a separate automorph from a temporary)
  int epi = NTT_EPI_SUBSCALE;
  InvFwdRoute inv;        // bext_pro only
};
inline ModDownRoute moddown_route(const NttEnv& e, const NttTuning& t, int nc, int B, int level, int aut,
                                  bool aliased, bool producer_rows = false) {
  ModDownRoute r;
  const int jobs = nc * B * (level + 1);
  // (with aut the NTT never runs in place: it scatters out of place or stores to a temporary)
  const bool inplace_sub = !aut && aliased;
  r.bext_pro = bext_in_prologue(e, t, jobs, e.K, NTT_EPI_SUBSCALE, inplace_sub);
  r.scatter = aut && t.ntt_aut_fuse && scatter_epilogue(e, t, jobs, r.bext_pro ? NTT_PRO_BEXT : NTT_PRO_LOAD);
  r.epi = !r.scatter ? NTT_EPI_SUBSCALE : aut == 2 ? NTT_EPI_SUBSCALE_AUT_ACC : NTT_EPI_SUBSCALE_AUT;
  if (r.bext_pro) {
    r.inv = inv_fwd_route(e, t, nc * B, e.K, level + 1, e.K, NTT_PRO_BEXT, r.epi, inplace_sub);
    r.inv.rows_stored = producer_rows && t.mac_rows && r.inv.ifuse && !(aut && !r.scatter);
  }
  return r;
}

// gadget decomposition of nc components at `level`: merged (every digit's
// ModUp + NTT as one launch pair) or per digit.  want_cols_only: the consumer
// can run the forward's rows pass itself (ks_mac_full)
struct DecomposeRoute {
  bool merged = false;
  bool tset = false;       // merged: the NTT runs over the target limbs only
  bool bext_pro = false;   // merged: the extension in the NTT's prologue; per digit: for the full digits
  bool bext_pro_last = false;  // per digit: for the last digit (it may have fewer limbs)
  InvFwdRoute inv;         // merged with bext_pro only
  bool cols_only = false;  // the forward stops after its columns pass
};
inline DecomposeRoute decompose_route(const NttEnv& e, const NttTuning& t, int nc, int B, int level,
                                      bool want_cols_only = false) {
  DecomposeRoute r;
  const int K = e.K, beta = (level + K) / K, nqp = level + 1 + K;
  r.merged = nc * B * (level + 1) < t.modup_merge && nqp <= e.max_limb;
  if (r.merged) {
    const int ntgt = beta * nqp - (level + 1);  // every Q limb is its own digit's once
    r.tset = beta * nqp <= 256 && ntgt <= e.max_limb;
    r.bext_pro = r.tset && bext_in_prologue(e, t, nc * B * ntgt, K, NTT_EPI_STORE, false);
    if (r.bext_pro) {
      r.inv = inv_fwd_route(e, t, nc * B, level + 1, ntgt, K, NTT_PRO_BEXT, NTT_EPI_STORE, false);
      r.cols_only = want_cols_only && r.inv.ifuse;
    }
  } else {
    const int ns_last = level + 1 - (beta - 1) * K;
    r.bext_pro = bext_in_prologue(e, t, nc * B * (nqp - K), K, NTT_EPI_STORE, false);
    r.bext_pro_last = bext_in_prologue(e, t, nc * B * (nqp - ns_last), ns_last, NTT_EPI_STORE, false);
  }
  return r;
}

// whether a ModDown at `level` that is rescaled next runs as one division by
// P q_level (moddown_rescale): where the ModDown takes the separate basis_ext
// route (small launches keep the fused latency path and the sequential rescale)
inline bool merged_rescale(const NttEnv& e, const NttTuning& t, int nc, int B, int level) {
  return level >= 1 && e.K <= e.max_src &&
         !bext_in_prologue(e, t, nc * B * (level + 1), e.K, NTT_EPI_SUBSCALE, false);
}

// how a key switch ends: its ModDown, or the QP accumulator kept for the
// merged ModDown and rescale (KeepQP: Ciphertext::pend; the caller asked for
// it with want_keep and NttTuning::defer, and merged_rescale holds)
enum class KsEnd { ModDown, KeepQP };

// key switch of one component into two (keyswitch): decomposition, gadget
// product, ModDown into a separate output
struct KeySwitchRoute {
  DecomposeRoute dec;
  ModDownRoute md;
  bool mac_rows = false;      // the gadget product stores the P limbs through the ModDown INTT's rows pass
  bool mac_fwd_rows = false;  // ... and runs the decomposition NTT's forward rows pass (dec.cols_only)
  KsEnd end = KsEnd::ModDown;
};
inline KeySwitchRoute keyswitch_route(const NttEnv& e, const NttTuning& t, int B, int level, int aut,
                                      bool want_keep = false) {
  KeySwitchRoute r;
  if (want_keep && t.defer && merged_rescale(e, t, 2, B, level)) {
    r.end = KsEnd::KeepQP;
    r.dec = decompose_route(e, t, 1, B, level);
    return r;
  }
  r.md = moddown_route(e, t, 2, B, level, aut, false, true);
  r.mac_rows = r.md.inv.rows_stored;
  r.dec = decompose_route(e, t, 1, B, level, r.mac_rows && t.mac_fwd_rows);
  r.mac_fwd_rows = r.dec.cols_only;
  return r;
}

// BSGS linear transform (eval_lt) with nzg rotating giants: the hoisted
// decomposition, the giants' ModDown and decomposition, the final ModDown
struct LtRoute {
  DecomposeRoute hoist, giant_dec;
  ModDownRoute giant_md, fin;  // fin.inv.rows_stored: lt_giant stores through the rows pass
  KsEnd end = KsEnd::ModDown;
};
inline LtRoute lt_route(const NttEnv& e, const NttTuning& t, int B, int level, int nzg, bool want_keep) {
  LtRoute r;
  r.hoist = decompose_route(e, t, 1, B, level);
  if (nzg > 0) {
    r.giant_md = moddown_route(e, t, nzg, B, level, 0, false);
    r.giant_dec = decompose_route(e, t, nzg, B, level);
  }
  if (want_keep && t.defer && merged_rescale(e, t, 2, B, level))
    r.end = KsEnd::KeepQP;
  else
    r.fin = moddown_route(e, t, 2, B, level, 0, false, nzg > 0 && nzg <= e.max_group);
  return r;
}

// hoisted rotations of one ciphertext (rotate_hoisted, rotate_sum): the one
// decomposition of c1, each output's ModDown with its automorphism, and the
// sum's one ModDown.  sum_rows: the sum has a rotating term, so lt_giant
// produces the accumulator and may store through the rows pass
struct HoistRoute {
  DecomposeRoute dec;
  ModDownRoute out_md;  // rotate_hoisted: per output, the automorphism in its store where the kernel scatters
  ModDownRoute sum_md;  // rotate_sum; sum_md.inv.rows_stored: lt_giant stores through the rows pass
};
inline HoistRoute hoist_route(const NttEnv& e, const NttTuning& t, int B, int level, bool sum_rows) {
  HoistRoute r;
  r.dec = decompose_route(e, t, 1, B, level);
  r.out_md = moddown_route(e, t, 2, B, level, 1, false);
  r.sum_md = moddown_route(e, t, 2, B, level, 0, false, sum_rows);
  return r;
}

// rescale by the last limb (rescale_inplace): the INTT of limb `level`, then
// the prep + NTT + (c - .) q_level^-1 of the others, in place
inline InvFwdRoute rescale_route(const NttEnv& e, const NttTuning& t, int nc, int B, int level) {
  return inv_fwd_route(e, t, nc * B, 1, level, 1, NTT_PRO_RESCALE, NTT_EPI_SUBSCALE, true);
}
