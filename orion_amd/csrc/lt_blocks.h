// lt_blocks.h -- the layout of a blocked linear transform (an R x C matrix of
// BSGS transforms evaluated as one call).  A single transform is the 1 x 1
// case: every linear transform the library evaluates is laid out here.  Host
// only: rotation amounts in, slot and entry numbers out; no HIP, no device
// pointer, no Context.  backend.hip fills the device plan (common.h LtPlan)
// from this and decides nothing of the layout itself.
//
// The blocks of one layer have different N1, so everything is keyed by the
// rotation amount.  Per column j the baby rotations of ct[j] are shared by all
// rows: the column's baby list is the union over its blocks.  Per row i the
// inner sums of equal giant amount are added across the columns before the
// giant step runs: the layer has one giant list, the union over all blocks, so
// that the rows (which become images of one batch) share keys and indices.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

namespace lt_blocks {

// one diagonal of a block: its giant and baby amounts (bsgs_split of the
// diagonal index by the block's own N1), in the order of the block's index list
struct Pair {
  int giant, baby;
};
// an (output row, giant) pair some block of the column has diagonals for; or,
// in column 0 only and with an empty mask, a pair no block of the row has any
// for (a row without one of the layer's giants): the launch writes its zero
struct Entry {
  int row = 0;
  int gslot = 0;  // position of the giant in Plan::giants
  int acc = 0;    // 1: a column before this one has an entry for (row, gslot)
  unsigned long long mask = 0;  // bit s: baby slot s of the column takes part
  std::vector<int> diag;        // per baby slot: index into the block's Pair list, -1: none
};
struct Column {
  std::vector<int> babies;     // amount of each register slot: nonzero amounts first-seen, then 0
  std::vector<Entry> entries;  // by row, then by giant slot
  int passes = 0;              // lt_bsgs launches per chunk: ceil(babies / maxb), slots [p maxb, (p + 1) maxb)
  int chunks = 0;              // device plans: ceil(entries / maxg)
  int rotating = 0;            // babies that need a key (nonzero amounts)
};
struct Plan {
  std::string error;  // empty: the plan holds
  int rows = 0, cols = 0;
  std::vector<int> giants;                   // the layer's giant amounts: ascending nonzero, then 0
  std::vector<std::vector<int>> row_giants;  // per row: the amounts it has diagonals for, same order
  std::vector<Column> columns;
  int nonzero_giants = 0;  // giants.size() less the zero giant
  int total_chunks = 0;
  // entry range [first, first + count) of chunk k of a column
  static int chunk_first(int k, int maxg) { return k * maxg; }
  static int chunk_count(const Column& c, int k, int maxg) {
    return std::min(maxg, (int)c.entries.size() - k * maxg);
  }
};

// blocks: row-major, rows * cols lists
inline Plan plan(const std::vector<std::vector<Pair>>& blocks, int rows, int cols, int maxb, int maxg, int maxslot) {
  Plan P;
  P.rows = rows, P.cols = cols;
  if (rows < 1 || cols < 1 || (int)blocks.size() != rows * cols) {
    P.error = "a blocked transform needs rows >= 1, cols >= 1 and rows * cols blocks";
    return P;
  }
  // the layer's giants
  bool has_zero = false;
  for (const auto& b : blocks)
    for (const Pair& p : b)
      if (p.giant == 0)
        has_zero = true;
      else if (std::find(P.giants.begin(), P.giants.end(), p.giant) == P.giants.end())
        P.giants.push_back(p.giant);
  std::sort(P.giants.begin(), P.giants.end());
  P.nonzero_giants = (int)P.giants.size();
  if (has_zero) P.giants.push_back(0);
  const int ng = (int)P.giants.size();
  if (ng == 0) {
    P.error = "a blocked transform without diagonals";
    return P;
  }
  // which (row, giant) planes of the inner sums some block writes
  std::vector<char> any((size_t)rows * ng, 0), written((size_t)rows * ng, 0);
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < cols; ++j)
      for (const Pair& p : blocks[(size_t)i * cols + j])
        any[(size_t)i * ng + (std::find(P.giants.begin(), P.giants.end(), p.giant) - P.giants.begin())] = 1;
  P.row_giants.resize(rows);
  P.columns.resize(cols);
  for (int j = 0; j < cols; ++j) {
    Column& c = P.columns[j];
    bool zero = false;
    for (int i = 0; i < rows; ++i)
      for (const Pair& p : blocks[(size_t)i * cols + j])
        if (p.baby == 0)
          zero = true;
        else if (std::find(c.babies.begin(), c.babies.end(), p.baby) == c.babies.end())
          c.babies.push_back(p.baby);
    c.rotating = (int)c.babies.size();
    if (zero) c.babies.push_back(0);
    const int nb = (int)c.babies.size();
    if (nb > maxslot) {
      P.error = "column " + std::to_string(j) + " of a blocked transform needs " + std::to_string(nb) +
                " baby steps: more than " + std::to_string(maxslot);
      return P;
    }
    for (int i = 0; i < rows; ++i) {
      const std::vector<Pair>& blk = blocks[(size_t)i * cols + j];
      for (int gs = 0; gs < ng; ++gs) {
        Entry e;
        e.row = i, e.gslot = gs;
        e.diag.assign(nb, -1);
        for (size_t k = 0; k < blk.size(); ++k) {
          if (blk[k].giant != P.giants[gs]) continue;
          const int s = (int)(std::find(c.babies.begin(), c.babies.end(), blk[k].baby) - c.babies.begin());
          e.mask |= 1ull << s;
          e.diag[s] = (int)k;
        }
        if (!e.mask && (j > 0 || any[(size_t)i * ng + gs])) continue;
        char& w = written[(size_t)i * ng + gs];
        e.acc = w;
        w = 1;
        c.entries.push_back(e);
      }
    }
    c.passes = (nb + maxb - 1) / maxb;
    c.chunks = ((int)c.entries.size() + maxg - 1) / maxg;
    P.total_chunks += c.chunks;
  }
  for (int i = 0; i < rows; ++i)
    for (int gs = 0; gs < ng; ++gs)
      if (any[(size_t)i * ng + gs]) P.row_giants[i].push_back(P.giants[gs]);
  return P;
}

}  // namespace lt_blocks
