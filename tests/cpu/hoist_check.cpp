// Stand-alone check of the hoisted rotations' host-only decisions
// (orion_amd/csrc/hoist.h, and HoistRoute of ntt_route.h), which are all it
// includes: the keys-per-launch chunks, the register bound on the digit count,
// and the routes of the shapes tests/test_gpu_hoisted.py runs.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "hoist.h"
#include "ntt_route.h"

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
      ++fails;                                                    \
    }                                                             \
  } while (0)

static NttEnv env(int logN, int K) {
  NttEnv e;
  e.logN = logN, e.ci = false, e.K = K, e.n_cu = 256;
  e.max_limb = 64, e.max_src = 8, e.max_group = 64;
  return e;
}
static bool same(const InvFwdRoute& a, const InvFwdRoute& b) {
  return a.ifuse == b.ifuse && a.tgroup == b.tgroup && a.rows_stored == b.rows_stored;
}
static bool same(const ModDownRoute& a, const ModDownRoute& b) {
  return a.bext_pro == b.bext_pro && a.scatter == b.scatter && a.epi == b.epi && same(a.inv, b.inv);
}
static bool same(const DecomposeRoute& a, const DecomposeRoute& b) {
  return a.merged == b.merged && a.tset == b.tset && a.bext_pro == b.bext_pro && a.bext_pro_last == b.bext_pro_last &&
         same(a.inv, b.inv) && a.cols_only == b.cols_only;
}

int main() {
  // the chunks cover 0..n-1 exactly once, in order, none over ORION_MAXHOIST
  int chunks = 0;
  for (int n = 1; n <= 64; ++n) {
    int next = 0;
    const int nl = hoist::launches(n);
    CHECK(nl == (n + ORION_MAXHOIST - 1) / ORION_MAXHOIST);
    for (int c = 0; c < nl; ++c) {
      const int first = hoist::chunk_first(c), cnt = hoist::chunk_count(n, c);
      CHECK(first == next);
      CHECK(cnt >= 1 && cnt <= ORION_MAXHOIST);
      next = first + cnt;
      ++chunks;
    }
    CHECK(next == n);
    CHECK(hoist::chunk_count(n, nl) == 0);  // nothing past the last launch
  }
  CHECK(hoist::launches(0) == 0 && hoist::launches(-3) == 0);
  // the keys of one launch fit beside three LimbSets in 4 KB of arguments
  CHECK(sizeof(hoist::Keys) <= 16 * 12 + 8);

  // the register bound: monotone (once past it, always past it), ORION_HOIST_MAXBETA the last held
  CHECK(!hoist::in_registers(0));
  bool in = true;
  int last = 0;
  for (int beta = 1; beta <= 64; ++beta) {
    const bool now = hoist::in_registers(beta);
    CHECK(in || !now);
    if (now) {
      last = beta;
      CHECK(hoist::digit_slots(beta) >= beta && hoist::digit_slots(beta) <= ORION_HOIST_MAXBETA);
      CHECK(beta == 1 || hoist::digit_slots(beta) >= hoist::digit_slots(beta - 1));
    }
    in = now;
  }
  CHECK(last == ORION_HOIST_MAXBETA);

  // HoistRoute of the GPU tests' shapes {logN, K, level, B}: one decomposition
  // of one component, the outputs' ModDowns carry the automorphism (in the
  // store wherever the kernel scatters, never through a producer's rows pass),
  // the sum's ModDown carries none
  struct Shape { int logN, K, level, B; };
  std::vector<Shape> shapes;
  for (int level : {5, 4, 2, 1, 0})
    for (int B : {1, 2, 3, 5}) shapes.push_back({13, 2, level, B});
  shapes.push_back({13, 2, 1, 64});
  for (int level : {9, 8, 7})
    for (int B : {1, 2}) shapes.push_back({13, 1, level, B});
  for (int B : {1, 2}) shapes.push_back({15, 2, 5, B});
  for (int level : {5, 11})
    for (int B : {1, 64}) shapes.push_back({15, 2, level, B});  // tools/hoist_ab.py
  int routes = 0, scattered = 0;
  for (const Shape& s : shapes) {
    const NttEnv e = env(s.logN, s.K);
    const NttTuning t;
    for (int rows = 0; rows < 2; ++rows) {
      const HoistRoute r = hoist_route(e, t, s.B, s.level, rows != 0);
      CHECK(same(r.dec, decompose_route(e, t, 1, s.B, s.level)));
      CHECK(!r.dec.cols_only);  // no consumer here runs the forward rows pass
      CHECK(same(r.out_md, moddown_route(e, t, 2, s.B, s.level, 1, false, false)));
      CHECK(!r.out_md.inv.rows_stored);
      const int jobs = 2 * s.B * (s.level + 1);
      const bool sc = scatter_epilogue(e, t, jobs, r.out_md.bext_pro ? NTT_PRO_BEXT : NTT_PRO_LOAD);
      CHECK(r.out_md.scatter == sc);
      CHECK(r.out_md.epi == (sc ? NTT_EPI_SUBSCALE_AUT : NTT_EPI_SUBSCALE));
      scattered += sc;
      CHECK(same(r.sum_md, moddown_route(e, t, 2, s.B, s.level, 0, false, rows != 0)));
      CHECK(!r.sum_md.scatter && r.sum_md.epi == NTT_EPI_SUBSCALE);
      CHECK(rows || !r.sum_md.inv.rows_stored);
      ++routes;
    }
  }
  CHECK(scattered > 0);
  if (fails) return 1;
  printf("hoist plan holds: %d chunks, register bound %d, %d routes\n", chunks, last, routes);
  return 0;
}
