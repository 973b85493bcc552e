// hoist.h -- the host-only decisions of the hoisted rotations: n rotations of
// one ciphertext, or their sum, from one gadget decomposition
// (Context::rotate_hoisted, Context::rotate_sum, ks_mac_hoisted_kernel).  It
// includes nothing of the library, so it also compiles host-only.
//
// rotate_hoisted runs the gadget products of up to ORION_MAXHOIST keys as one
// ks_mac_hoisted_kernel launch: a thread keeps the beta digit words of its two
// coefficients in registers and loops over the keys, so a row of the
// decomposition is read once per launch, not once per key.
#pragma once
#include <stdint.h>

// keys per ks_mac_hoisted_kernel launch: 16 x {key pointer, key level} beside
// the three LimbSets stay far below the 4 KB of kernel arguments
#define ORION_MAXHOIST 16
// the widest decomposition whose digits the kernel holds in registers (4 VGPRs
// per digit: two 64-bit coefficients); wider ones take the grouped ks_mac
// launch with the shared decomposition
#define ORION_HOIST_MAXBETA 8

namespace hoist {

// whether a decomposition of beta digits runs on ks_mac_hoisted_kernel
inline bool in_registers(int beta) { return beta >= 1 && beta <= ORION_HOIST_MAXBETA; }
// the digit slots of the instantiation that takes beta digits (4 or
// ORION_HOIST_MAXBETA): at most 4 digits need half the digit registers
inline int digit_slots(int beta) { return beta <= 4 ? 4 : ORION_HOIST_MAXBETA; }

// n keys run as ceil(n / ORION_MAXHOIST) launches; launch c takes the keys
// [chunk_first(c), chunk_first(c) + chunk_count(n, c)), in the caller's order
inline int launches(int n) { return n < 1 ? 0 : (n + ORION_MAXHOIST - 1) / ORION_MAXHOIST; }
inline int chunk_first(int c) { return c * ORION_MAXHOIST; }
inline int chunk_count(int n, int c) {
  const int left = n - c * ORION_MAXHOIST;
  return left < 0 ? 0 : left < ORION_MAXHOIST ? left : ORION_MAXHOIST;
}

// the keys of one launch, by value in the kernel arguments (a captured graph
// holds them in its node, no device buffer); key layout as MacGroups'
struct Keys {
  const uint64_t* key[ORION_MAXHOIST];
  int klvl[ORION_MAXHOIST];  // the level each key was made for
  int n;
};

}  // namespace hoist
