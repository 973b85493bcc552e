// launch.h -- the kernel interface: the host launchers that kernels.hip,
// ntt.hip, ntt2.hip, ntt2s.hip and encoder.hip define and backend.hip calls,
// and the op codes of the coefficient-wise kernel.  Every one of those files
// includes it, so a signature or an op code that drifts is a compile error.
// A launcher returns 0, or nonzero for a launch it refuses.
#pragma once
#include "common.h"
#include "tensor_sum.h"

// orion_launch_ew's op
enum EwOp : int {
  EW_ADD = 0,      // o = a + b
  EW_SUB = 1,      // o = a - b
  EW_MUL = 2,      // o = a * b
  EW_MULADD = 3,   // o = o + a * b
  EW_NEG = 4,      // o = -a
  EW_SCALE = 5,    // o = a * s_l            (Shoup scalar per limb)
  EW_ADDC = 6,     // o = a + s_l            (constant per limb)
  EW_SUBSCALE = 7, // o = (a - b) * s_l
  EW_COPY = 8,     // o = a
  EW_ADDSCALE = 9, // o = o + a * s_l
  EW_SPLIT24 = 10, // o = split24(a) on limbs below 2^48, split30(a) on limbs up to 2^60, else a
                   // (lt_bsgs's split-MAC operand forms)
};

// ntt.hip, ntt2.hip, ntt2s.hip
int orion_launch_ntt(int logN, const LimbSet& s, const DeviceTables* tb, bool inverse, hipStream_t st);
int orion_launch_ntt_io(int logN, const NttIO& io, const DeviceTables* tb, bool inverse, hipStream_t st);
int orion_launch_ntt2(int logN, const NttIO& io, const DeviceTables* tb, bool inverse, hipStream_t st);
int orion_launch_ntt2s(int logN, const NttIO& io, const DeviceTables* tb, bool inverse, hipStream_t st,
                       bool rows_only = false);
int orion_ntt_init();

// kernels.hip
int orion_launch_ew(int op, const LimbSet& o, const LimbSet& a, const LimbSet& b, const u64* s, const u64* ss,
                    const DeviceTables* tb, int N, hipStream_t st);
int orion_launch_tensor(const LimbSet& d, const LimbSet& a, const LimbSet& b, const DeviceTables* tb, int N,
                        hipStream_t st);
int orion_launch_tensor_sum(const LimbSet& d, const tsum::Table& T, bool acc, const DeviceTables* tb, int N,
                            hipStream_t st);
int orion_launch_gather(u64* dst, long long d_comp, long long d_limb, int nimg, int nlimb, const GatherTable& T,
                        int N, hipStream_t st);
int orion_launch_pack_complex(const LimbSet& o, const LimbSet& a, const LimbSet& b, int npair, const u64* w4,
                              const u64* w4s, const DeviceTables* tb, int N, hipStream_t st);
int orion_launch_unpack_complex(const LimbSet& re, const LimbSet& im, const LimbSet& x, const LimbSet& y, int nim,
                                const u64* w4, const u64* w4s, const DeviceTables* tb, int N, hipStream_t st);
int orion_launch_mono_pack(const LimbSet& o, const LimbSet& a, const LimbSet& m1, int g, const DeviceTables* tb,
                           int N, hipStream_t st);
int orion_launch_mono_unpack(const LimbSet& o, const LimbSet& x, const LimbSet& mi, int g, const DeviceTables* tb,
                             int N, hipStream_t st);
int orion_launch_basis_ext(const LimbSet& out, const LimbSet& in, const BasisExtTable* T, const DeviceTables* tb,
                           int N, hipStream_t st);
int orion_launch_basis_ext_rescale(const LimbSet& out, const LimbSet& in, const BextRescaleTable* W, int N,
                                   hipStream_t st);
int orion_launch_modup_all(const LimbSet& D, const LimbSet& in, const BasisExtTable* Ts, int beta, int K,
                           int nqp, const DeviceTables* tb, int N, hipStream_t st);
int orion_launch_ks_mac(const LimbSet& out, const LimbSet& D, const LimbSet& own, const MacGroups& G, int ngroup,
                        int beta, const DeviceTables* tb, int N, hipStream_t st);
int orion_launch_ks_mac_hoisted(const LimbSet& out, const LimbSet& D, const LimbSet& own, const LimbSet& add,
                                const MacHoist& H, const DeviceTables* tb, int N, hipStream_t st);
int orion_launch_automorph(const LimbSet& o, const LimbSet& a, const u32* idx, const DeviceTables* tb, int N,
                           int accumulate, hipStream_t st);
int orion_launch_lt_bsgs(const LimbSet& t0, const LimbSet& t1, const LimbSet& D, const LimbSet& ct,
                         const LtBabies& Bb, const LtPlan* plan, int chunk, int ne, int accumulate, bool one,
                         const LimbSet& ptl, const DeviceTables* tb, int N, int colB, hipStream_t st);
int orion_launch_lt_giant(const LimbSet& acc, const LimbSet& D, const LimbSet& own, const LimbSet& t0,
                          const LimbSet& z, const LtGiants& G, const DeviceTables* tb, int N, hipStream_t st);

// encoder.hip
int orion_launch_encode(const float* vals, int nvals, int B, double2* v, const double2* tw_inv, int logn, bool ci,
                        const LimbSet& out, double scale, const DeviceTables* tb, hipStream_t st);
int orion_launch_decode(const LimbSet& x, const u64* garner, double scale, int logn, bool ci, double2* v,
                        const double2* tw_fwd, double* out, const DeviceTables* tb, hipStream_t st);
int orion_launch_enc_sample(const LimbSet& r, const EncSampler& sp, const DeviceTables* tb, int N, hipStream_t st);
int orion_launch_encode_c(double2* v, int B, const double2* tw_inv, int logn, bool ci, const LimbSet& out, double scale,
                          const DeviceTables* tb, hipStream_t st);
int orion_launch_modraise(const LimbSet& out, const LimbSet& in, const DeviceTables* tb, int N, hipStream_t st);
