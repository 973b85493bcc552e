// Stand-alone check of the blocked linear transform's layout planner
// (orion_amd/csrc/lt_blocks.h), which is all it includes besides common.h's
// three limits, restated here.  Every expected value below was derived by hand
// from the rule in the header: bsgs_split of each diagonal by its block's N1,
// babies per column (nonzero amounts first-seen, rows in order, then 0), giants
// per layer (ascending nonzero amounts, then 0), entries by row then giant slot.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lt_blocks.h"

using namespace lt_blocks;

static int g_fail = 0;
#define EXPECT(c)                                              \
  do {                                                         \
    if (!(c)) {                                                \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);      \
      ++g_fail;                                                \
    }                                                          \
  } while (0)

enum { MAXB = 16, MAXG = 64, MAXSLOT = 64, SLOTS = 4096 };

static std::vector<Pair> block(const std::vector<int>& idx, int n1) {
  std::vector<Pair> v;
  for (int d : idx) {
    const int rot = d & (SLOTS - 1);
    v.push_back({((rot / n1) * n1) & (SLOTS - 1), rot & (n1 - 1)});
  }
  return v;
}
static bool entry_is(const Entry& e, int row, int gslot, unsigned long long mask, int acc) {
  return e.row == row && e.gslot == gslot && e.mask == mask && e.acc == acc;
}

// the 2 x 3 layer of tests/test_gpu_ltblocks.py: N1 = 32, 1, 128 / 2, 256, 32
static void check_2x3() {
  const std::vector<int> big = {0, 1, 2, 3, 17, 64, 65, 300, 4095};
  const std::vector<std::vector<Pair>> blocks = {block(big, 32),       block({0}, 1),
                                                 block({5, 64, 128, 192}, 128), block({1, 2, 3}, 2),
                                                 block({64, 128, 4000}, 256),   block(big, 32)};
  // (0,0): 300 = 288 + 12, 4095 = 4064 + 31; (1,1): 4000 = 3840 + 160; (0,2): 192 = 128 + 64
  EXPECT(blocks[0][7].giant == 288 && blocks[0][7].baby == 12 && blocks[0][8].giant == 4064 && blocks[0][8].baby == 31);
  EXPECT(blocks[4][2].giant == 3840 && blocks[4][2].baby == 160 && blocks[2][3].giant == 128 && blocks[2][3].baby == 64);
  const Plan P = plan(blocks, 2, 3, MAXB, MAXG, MAXSLOT);
  EXPECT(P.error.empty());
  EXPECT((P.giants == std::vector<int>{2, 64, 128, 288, 3840, 4064, 0}));
  EXPECT(P.nonzero_giants == 6);
  EXPECT((P.row_giants[0] == std::vector<int>{64, 128, 288, 4064, 0}));
  EXPECT((P.row_giants[1] == std::vector<int>{2, 64, 288, 3840, 4064, 0}));
  // a row lacking a giant that another row has (row 0: 2 and 3840, row 1: 128): nobody's
  // diagonals go there, so column 0 writes the zero (entries with an empty mask)
  // column 0
  const Column& c0 = P.columns[0];
  EXPECT((c0.babies == std::vector<int>{1, 2, 3, 17, 12, 31, 0}));
  EXPECT(c0.rotating == 6 && c0.passes == 1 && c0.chunks == 1 && c0.entries.size() == 9);
  EXPECT(entry_is(c0.entries[0], 0, 0, 0, 0));    // giant 2: row 0 has none
  EXPECT(entry_is(c0.entries[1], 0, 1, 65, 0));   // giant 64: babies 0 (slot 6), 1 (slot 0)
  EXPECT(entry_is(c0.entries[2], 0, 3, 16, 0));   // giant 288: baby 12 (slot 4)
  EXPECT(entry_is(c0.entries[3], 0, 4, 0, 0));    // giant 3840: row 0 has none
  EXPECT(entry_is(c0.entries[4], 0, 5, 32, 0));   // giant 4064: baby 31 (slot 5)
  EXPECT(entry_is(c0.entries[5], 0, 6, 79, 0));   // giant 0: babies 0, 1, 2, 3, 17
  EXPECT(entry_is(c0.entries[6], 1, 0, 65, 0));   // row 1, giant 2: diagonals 2 (baby 0), 3 (baby 1)
  EXPECT(entry_is(c0.entries[7], 1, 2, 0, 0));    // row 1, giant 128: none
  EXPECT(entry_is(c0.entries[8], 1, 6, 1, 0));    // row 1, giant 0: diagonal 1
  EXPECT(c0.entries[1].diag[6] == 5 && c0.entries[1].diag[0] == 6 && c0.entries[1].diag[1] == -1);
  EXPECT(c0.entries[6].diag[6] == 1 && c0.entries[6].diag[0] == 2);
  for (int s = 0; s < 7; ++s) EXPECT(c0.entries[0].diag[s] == -1);
  // column 1: a block with no rotation at all, and a block without the zero baby
  const Column& c1 = P.columns[1];
  EXPECT((c1.babies == std::vector<int>{64, 128, 160, 0}));
  EXPECT(c1.entries.size() == 3);
  EXPECT(entry_is(c1.entries[0], 0, 6, 8, 1));    // adds to column 0's (row 0, giant 0)
  EXPECT(entry_is(c1.entries[1], 1, 4, 4, 0));    // giant 3840: first writer
  EXPECT(entry_is(c1.entries[2], 1, 6, 3, 1));
  // column 2
  const Column& c2 = P.columns[2];
  EXPECT((c2.babies == std::vector<int>{5, 64, 1, 2, 3, 17, 12, 31, 0}));
  EXPECT(c2.rotating == 8 && c2.passes == 1 && c2.entries.size() == 6);
  EXPECT(entry_is(c2.entries[0], 0, 2, 258, 0));  // giant 128: babies 0 (slot 8), 64 (slot 1)
  EXPECT(entry_is(c2.entries[1], 0, 6, 3, 1));
  EXPECT(entry_is(c2.entries[2], 1, 1, 260, 0));
  EXPECT(entry_is(c2.entries[3], 1, 3, 64, 0));
  EXPECT(entry_is(c2.entries[4], 1, 5, 128, 0));
  EXPECT(entry_is(c2.entries[5], 1, 6, 316, 1));
  EXPECT(P.total_chunks == 3);
  // every (row, giant) plane is written first by exactly one entry; only column 0 writes zeros
  std::vector<int> first(2 * 7, 0);
  for (const Column& c : P.columns)
    for (const Entry& e : c.entries) {
      first[e.row * 7 + e.gslot] += e.acc ? 0 : 1;
      EXPECT(e.mask != 0 || &c == &P.columns[0]);
    }
  for (int v : first) EXPECT(v == 1);
}

// 3 x 1 of the dense band range(768) at N1 = 32: 32 babies (two passes of
// MAXB = 16 register slots), 3 * 24 = 72 entries (two chunks of MAXG = 64)
static void check_band() {
  std::vector<int> idx;
  for (int d = 0; d < 768; ++d) idx.push_back(d);
  const std::vector<std::vector<Pair>> blocks(3, block(idx, 32));
  const Plan P = plan(blocks, 3, 1, MAXB, MAXG, MAXSLOT);
  EXPECT(P.error.empty());
  EXPECT(P.giants.size() == 24 && P.giants.front() == 32 && P.giants[22] == 736 && P.giants.back() == 0);
  const Column& c = P.columns[0];
  EXPECT(c.babies.size() == 32 && c.babies.front() == 1 && c.babies[30] == 31 && c.babies.back() == 0);
  EXPECT(c.rotating == 31 && c.passes == 2);
  EXPECT(c.entries.size() == 72 && c.chunks == 2 && P.total_chunks == 2);
  EXPECT(Plan::chunk_first(1, MAXG) == 64 && Plan::chunk_count(c, 0, MAXG) == 64 && Plan::chunk_count(c, 1, MAXG) == 8);
  EXPECT(entry_is(c.entries[64], 2, 16, 0xffffffffull, 0));  // 64 = 2 * 24 + 16
  // giant slot 16 = amount 544; baby slot 31 = amount 0: diagonal 544; slot 0 = amount 1: diagonal 545
  EXPECT(c.entries[64].diag[31] == 544 && c.entries[64].diag[0] == 545);
}

// One transform is the 1 x 1 block: one entry per giant, in the order of the
// giant list, none accumulating.
static void check_single() {
  // range(65) + {2048} at N1 = 1: every diagonal its own giant, the one baby 0
  std::vector<int> idx;
  for (int d = 0; d <= 64; ++d) idx.push_back(d);
  idx.push_back(2048);
  const Plan P = plan({block(idx, 1)}, 1, 1, MAXB, MAXG, MAXSLOT);
  EXPECT(P.error.empty());
  EXPECT(P.giants.size() == 66 && P.giants.front() == 1 && P.giants[63] == 64 && P.giants[64] == 2048 && P.giants.back() == 0);
  EXPECT(P.nonzero_giants == 65);
  const Column& c = P.columns[0];
  EXPECT((c.babies == std::vector<int>{0}));
  EXPECT(c.entries.size() == 66 && c.chunks == 2 && c.passes == 1 && c.rotating == 0 && P.total_chunks == 2);
  EXPECT(Plan::chunk_count(c, 0, MAXG) == 64 && Plan::chunk_count(c, 1, MAXG) == 2);
  for (size_t k = 0; k < c.entries.size(); ++k) EXPECT(entry_is(c.entries[k], 0, (int)k, 1, 0));
  // giant 1 is diagonal 1, giant 2048 the last of the list, giant 0 the first
  EXPECT(c.entries[0].diag[0] == 1 && c.entries[64].diag[0] == 65 && c.entries[65].diag[0] == 0);

  // the dense band range(768) at N1 = 32 alone: 24 giants, 32 babies in two passes
  std::vector<int> band;
  for (int d = 0; d < 768; ++d) band.push_back(d);
  const Plan Q = plan({block(band, 32)}, 1, 1, MAXB, MAXG, MAXSLOT);
  EXPECT(Q.error.empty());
  const Column& q = Q.columns[0];
  EXPECT(q.entries.size() == 24 && q.chunks == 1 && q.passes == 2 && q.rotating == 31);
  for (size_t k = 0; k < q.entries.size(); ++k) EXPECT(entry_is(q.entries[k], 0, (int)k, 0xffffffffull, 0));

  // no zero giant: 33 = 32 + 1, 65 = 64 + 1, 66 = 64 + 2 at N1 = 32; babies 1 (slot 0), 2 (slot 1)
  const Plan S = plan({block({33, 65, 66}, 32)}, 1, 1, MAXB, MAXG, MAXSLOT);
  EXPECT(S.error.empty());
  EXPECT((S.giants == std::vector<int>{32, 64}) && S.nonzero_giants == 2);
  const Column& s = S.columns[0];
  EXPECT((s.babies == std::vector<int>{1, 2}) && s.rotating == 2 && s.entries.size() == 2);
  EXPECT(entry_is(s.entries[0], 0, 0, 1, 0) && entry_is(s.entries[1], 0, 1, 3, 0));
  EXPECT(s.entries[1].diag[0] == 1 && s.entries[1].diag[1] == 2 && s.entries[0].diag[1] == -1);
}

static void check_refusals() {
  std::vector<Pair> wide;
  for (int b = 0; b <= 64; ++b) wide.push_back({0, b});  // 65 distinct babies
  const Plan P = plan({wide}, 1, 1, MAXB, MAXG, MAXSLOT);
  EXPECT(!P.error.empty() && P.error.find("column 0") != std::string::npos && P.error.find("65") != std::string::npos);
  // ... spread over two rows of one column all the same; two columns of 33 are fine
  std::vector<Pair> lo, hi;
  for (int b = 0; b < 33; ++b) lo.push_back({0, b}), hi.push_back({0, 100 + b});
  EXPECT(!plan({lo, hi}, 2, 1, MAXB, MAXG, MAXSLOT).error.empty());
  const Plan Q = plan({lo, hi}, 1, 2, MAXB, MAXG, MAXSLOT);
  EXPECT(Q.error.empty() && Q.columns[0].passes == 3 && Q.columns[1].passes == 3);
  EXPECT(Q.columns[1].entries[0].acc == 1 && Q.columns[0].entries.size() == 1);
  EXPECT(!plan({}, 0, 1, MAXB, MAXG, MAXSLOT).error.empty());
  EXPECT(!plan({lo}, 1, 2, MAXB, MAXG, MAXSLOT).error.empty());
}

int main() {
  check_2x3();
  check_band();
  check_single();
  check_refusals();
  if (g_fail) {
    printf("%d checks failed\n", g_fail);
    return 1;
  }
  printf("lt_blocks: all anchor cases hold\n");
  return 0;
}
