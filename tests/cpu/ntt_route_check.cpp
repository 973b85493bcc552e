// Stand-alone check of the launch planner (orion_amd/csrc/ntt_route.h), which
// is all it includes: anchor cases derived from the rules as written, and the
// recorded decisions of commit a9bb9bd (tests/golden/ntt_routes.json, expanded
// to text by tests/test_ntt_route.py).  usage: ntt_route_check TABLE.txt
//
// The table has one line per context, "<key>|<digits>", in the order of
// contexts(); emit() below defines the digits.  The fixture was recorded by
// compiling this file with NTT_ROUTE_CHECK_NO_MAIN next to a decider made of
// a9bb9bd's predicates (two_pass, fuse_bext, on_ntt2s, ifuse_ok, aut_epi_ok,
// moddown_rows_fusable, moddown_rescale_ok, ntt2_tail; n_cu a parameter) and
// printing emit() for every context.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include "ntt_route.h"

struct Ctx {
  int tuning, n_cu, logN, ci, K;  // K = 0: the single-launch section
};
static const char* const TUNINGS[] = {"default", "ORION_BEXT_FUSE_BELOW=1024", "ORION_NTT_IFUSE=0",
                                      "ORION_NTT_AUT_FUSE=0", "ORION_NTT_IFUSE_MAXR=1000", "ORION_BEXT_FUSE=0",
                                      "ORION_MODUP_MERGE=0", "ORION_DEFER=0", "ORION_NTT2_TAIL_FWD=2",
                                      "ORION_MAC_ROWS=0", "ORION_MAC_FWD_ROWS=0", "ORION_NTT_IMPL=2"};
static const int NTUNING = sizeof(TUNINGS) / sizeof(TUNINGS[0]);
static NttTuning tuning(int i) {
  NttTuning t;
  switch (i) {
    case 1: t.bext_fuse_below = 1024; break;
    case 2: t.ntt_ifuse = 0; break;
    case 3: t.ntt_aut_fuse = 0; break;
    case 4: t.ntt_ifuse_maxr = 1000; break;
    case 5: t.bext_fuse = 0; break;
    case 6: t.modup_merge = 0; break;
    case 7: t.defer = false; break;
    case 8: t.ntt2_tail_fwd = 2; break;
    case 9: t.mac_rows = 0; break;
    case 10: t.mac_fwd_rows = 0; break;
    case 11: t.ntt_impl = 2; break;
  }
  return t;
}
static NttEnv env(int logN, int ci, int K, int n_cu) {
  NttEnv e;
  e.logN = logN, e.ci = ci != 0, e.K = K, e.n_cu = n_cu;
  e.max_limb = 64, e.max_src = 8, e.max_group = 64;
  return e;
}
static std::vector<Ctx> contexts() {
  std::vector<Ctx> v;
  for (int t = 0; t < NTUNING; ++t)
    for (int n_cu : {256, 128})
      for (int logN : {13, 15, 16})
        for (int ci = 0; ci < 2; ++ci)
          for (int K : {0, 1, 2, 8}) v.push_back(Ctx{t, n_cu, logN, ci, K});
  return v;
}
static std::string key(const Ctx& c) {
  char b[128];
  snprintf(b, sizeof b, "%s cu=%d logN=%d ci=%d K=%d", TUNINGS[c.tuning], c.n_cu, c.logN, c.ci, c.K);
  return b;
}

// what a decider answers (the planner below; a9bb9bd's predicates when recording)
struct MdOut { bool bext_pro, scatter, ifuse, rows; int tgroup; };
struct DecOut { bool merged, tset, bext_pro, bext_pro_last, ifuse, cols_only; int tgroup; };
struct KsOut { bool mac_rows, mac_fwd_rows, keep; };

struct Planner {
  NttEnv e;
  NttTuning t;
  int family(int jobs, bool inv, int pro, int epi, bool ips) const { return ntt_family(e, t, jobs, inv, pro, epi, ips); }
  bool bext(int jobs, int ns, int epi, bool ips) const { return bext_in_prologue(e, t, jobs, ns, epi, ips); }
  bool scatter(int jobs, int pro) const { return scatter_epilogue(e, t, jobs, pro); }
  MdOut moddown(int nc, int B, int level, int aut, bool aliased, bool producer) const {
    const ModDownRoute r = moddown_route(e, t, nc, B, level, aut, aliased, producer);
    return MdOut{r.bext_pro, r.scatter, r.inv.ifuse, r.inv.rows_stored, r.inv.tgroup};
  }
  DecOut decompose(int nc, int B, int level, bool want) const {
    const DecomposeRoute r = decompose_route(e, t, nc, B, level, want);
    return DecOut{r.merged, r.tset, r.bext_pro, r.bext_pro_last, r.inv.ifuse, r.cols_only, r.inv.tgroup};
  }
  InvFwdRoute rescale(int nc, int B, int level) const { return rescale_route(e, t, nc, B, level); }
  bool merged(int nc, int B, int level) const { return merged_rescale(e, t, nc, B, level); }
  KsOut keyswitch(int B, int level, int aut, bool keep) const {
    const KeySwitchRoute r = keyswitch_route(e, t, B, level, aut, keep);
    return KsOut{r.mac_rows, r.mac_fwd_rows, r.end == KsEnd::KeepQP};
  }
  KsOut lt(int B, int level, int nzg, bool keep) const {
    const LtRoute r = lt_route(e, t, B, level, nzg, keep);
    return KsOut{r.fin.inv.rows_stored, false, r.end == KsEnd::KeepQP};
  }
};

static const int JOBS[] = {1, 2, 8, 63, 64, 65, 120, 127, 128, 129, 192, 255, 256, 257, 384, 600, 768, 1024, 1025, 2048};
static const int PROS[] = {NTT_PRO_LOAD, NTT_PRO_RESCALE, NTT_PRO_BEXT};
static const int LEVELS[] = {0, 1, 5, 15, 32};
static const int BATCHES[] = {1, 2, 5, 6, 12, 40, 64};

// one context's decisions as digits; lab (optional): what each digit is
template <class D>
static std::string emit(const D& d, const Ctx& c, std::vector<std::string>* lab = nullptr) {
  std::string s;
  char where[160];
  auto put = [&](int v, const char* what) {
    s.push_back("0123456789abcdef"[v & 15]);
    if (lab) lab->push_back(std::string(where) + " " + what);
  };
  if (c.K == 0) {  // single launches
    for (int jobs : JOBS) {
      for (int inv = 0; inv < 2; ++inv)
        for (int pro : PROS)
          for (int epi = 0; epi < 4; ++epi)
            for (int ips = 0; ips < 2; ++ips) {
              snprintf(where, sizeof where, "jobs=%d inv=%d pro=%d epi=%d inplace_sub=%d", jobs, inv, pro, epi, ips);
              put(d.family(jobs, inv, pro, epi, ips), "family");
            }
      for (int ns = 1; ns <= 3; ++ns)
        for (int epi = 0; epi < 2; ++epi)
          for (int ips = 0; ips < 2; ++ips) {
            snprintf(where, sizeof where, "jobs=%d ns=%d epi=%d inplace_sub=%d", jobs, ns, epi, ips);
            put(d.bext(jobs, ns, epi, ips), "basis extension in the prologue");
          }
      for (int pro : {NTT_PRO_LOAD, NTT_PRO_BEXT}) {
        snprintf(where, sizeof where, "jobs=%d pro=%d", jobs, pro);
        put(d.scatter(jobs, pro), "scatter epilogue");
      }
    }
    return s;
  }
  for (int level : LEVELS)
    for (int B : BATCHES) {
      for (int nc = 1; nc <= 3; ++nc) {
        for (int aut = 0; aut < 3; ++aut)
          for (int al = 0; al < 2; ++al) {
            for (int pr = 0; pr < 2; ++pr) {
              snprintf(where, sizeof where, "moddown level=%d B=%d nc=%d aut=%d aliased=%d producer=%d", level, B, nc, aut, al, pr);
              const MdOut m = d.moddown(nc, B, level, aut, al, pr);
              put(m.bext_pro | m.scatter << 1 | m.ifuse << 2 | m.rows << 3, "bext_pro|scatter<<1|ifuse<<2|rows<<3");
              put(m.tgroup, "tgroup");
            }
          }
        for (int want = 0; want < 2; ++want) {
          snprintf(where, sizeof where, "decompose level=%d B=%d nc=%d want_cols_only=%d", level, B, nc, want);
          const DecOut r = d.decompose(nc, B, level, want);
          const bool many = level + 1 > c.K;  // more than one digit
          put(r.merged | r.tset << 1 | (r.bext_pro && (r.merged || many)) << 2 | (r.bext_pro_last && !r.merged) << 3,
              "merged|tset<<1|bext_pro<<2|bext_pro_last<<3");
          put(r.ifuse | r.cols_only << 1, "ifuse|cols_only<<1");
          put(r.tgroup, "tgroup");
        }
        snprintf(where, sizeof where, "rescale level=%d B=%d nc=%d", level, B, nc);
        if (level >= 1) {
          const InvFwdRoute r = d.rescale(nc, B, level);
          put(r.ifuse, "ifuse");
          put(r.tgroup, "tgroup");
        }
        put(d.merged(nc, B, level), "merged ModDown->rescale");
      }
      for (int keep = 0; keep < 2; ++keep) {
        for (int aut = 0; aut < 3; ++aut) {
          snprintf(where, sizeof where, "keyswitch level=%d B=%d aut=%d want_keep=%d", level, B, aut, keep);
          const KsOut k = d.keyswitch(B, level, aut, keep);
          put(k.mac_rows | k.mac_fwd_rows << 1 | k.keep << 2, "mac_rows|mac_fwd_rows<<1|keep_qp<<2");
        }
        for (int nzg : {0, 1, 65}) {
          snprintf(where, sizeof where, "eval_lt level=%d B=%d nzg=%d want_keep=%d", level, B, nzg, keep);
          const KsOut k = d.lt(B, level, nzg, keep);
          put(k.mac_rows | k.keep << 2, "giant_rows|keep_qp<<2");
        }
      }
    }
  return s;
}

#ifndef NTT_ROUTE_CHECK_NO_MAIN
static int fails = 0;
#define EXPECT(cond)                                          \
  do {                                                        \
    if (!(cond)) {                                            \
      printf("anchor failed, line %d: %s\n", __LINE__, #cond); \
      ++fails;                                                \
    }                                                         \
  } while (0)

// N = 2^15, Standard ring, 256 CUs, default tuning unless stated
static void anchors() {
  const NttTuning t;
  const int LOAD = NTT_PRO_LOAD, BEXT = NTT_PRO_BEXT, STORE = NTT_EPI_STORE, SUB = NTT_EPI_SUBSCALE;
  const NttEnv e = env(15, 0, 2, 256), e16 = env(16, 0, 2, 256), eci = env(15, 1, 2, 256);
  EXPECT(ntt_family(e, t, 8, false, LOAD, STORE, false) == Latency);
  EXPECT(ntt_family(e, t, 128, true, LOAD, STORE, false) == Latency);  // 128/256 = 0.5 < 0.9
  EXPECT(ntt_family(e, t, 192, true, LOAD, STORE, false) == TwoPass);
  EXPECT(ntt_family(e, t, 256, true, LOAD, STORE, false) == OnePass);
  EXPECT(ntt_family(e, t, 600, true, LOAD, STORE, false) == TwoPass);  // 600/768
  EXPECT(ntt_family(e, t, 600, false, LOAD, SUB, false) == OnePass);
  EXPECT(ntt_family(e, t, 768, true, LOAD, STORE, false) == OnePass);
  EXPECT(ntt_family(e, t, 1025, true, LOAD, STORE, false) == OnePass);  // > tail_max
  EXPECT(ntt_family(e16, t, 128, true, LOAD, STORE, false) == Latency);
  EXPECT(ntt_family(e16, t, 129, true, LOAD, STORE, false) == TwoPass);
  for (int jobs : JOBS)
    for (int inv = 0; inv < 2; ++inv) {
      EXPECT(ntt_family(eci, t, jobs, inv, LOAD, STORE, false) == OnePass);
      EXPECT(ntt_family(env(13, 0, 2, 256), t, jobs, inv, LOAD, STORE, false) == OnePass);
      EXPECT(ntt_family(env(14, 0, 2, 256), t, jobs, inv, LOAD, STORE, false) == OnePass);
    }
  EXPECT(bext_in_prologue(e, t, 64, 2, STORE, false));
  EXPECT(!bext_in_prologue(e, t, 65, 2, STORE, false));
  EXPECT(!bext_in_prologue(e, t, 64, 3, STORE, false));
  EXPECT(!bext_in_prologue(eci, t, 64, 2, STORE, false));
  EXPECT(!bext_in_prologue(env(14, 0, 2, 256), t, 64, 2, STORE, false));
  // K = 2, level 5, 2 components: 12 B <= 64 keeps the latency path
  for (int B = 1; B <= 5; ++B) EXPECT(!merged_rescale(e, t, 2, B, 5));
  EXPECT(merged_rescale(e, t, 2, 6, 5));
  for (int B : BATCHES) EXPECT(!merged_rescale(e, t, 2, B, 0));
  EXPECT(ntt_family(e, t, 256, false, LOAD, NTT_EPI_SUBSCALE_AUT, false) == OnePass && scatter_epilogue(e, t, 256, LOAD));
  EXPECT(ntt_family(e, t, 64, false, BEXT, NTT_EPI_SUBSCALE_AUT, false) == Latency && scatter_epilogue(e, t, 64, BEXT));
  EXPECT(ntt_family(e16, t, 256, false, LOAD, NTT_EPI_SUBSCALE_AUT, false) == TwoPass && !scatter_epilogue(e16, t, 256, LOAD));
  EXPECT(!scatter_epilogue(eci, t, 256, LOAD) && !scatter_epilogue(eci, t, 64, LOAD));
}

int main(int argc, char** argv) {
  anchors();
  if (argc < 2) {
    printf("usage: ntt_route_check TABLE.txt\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  std::string line;
  size_t rows = 0;
  for (const Ctx& c : contexts()) {
    if (!std::getline(in, line)) {
      printf("table ends before context %s\n", key(c).c_str());
      return 1;
    }
    const Planner p{env(c.logN, c.ci, c.K, c.n_cu), tuning(c.tuning)};
    const std::string want = key(c) + "|", got = emit(p, c);
    if (line.compare(0, want.size(), want) != 0 || line.size() != want.size() + got.size()) {
      printf("table line does not match context %s\n", key(c).c_str());
      return 1;
    }
    for (size_t i = 0; i < got.size(); ++i)
      if (got[i] != line[want.size() + i]) {
        std::vector<std::string> lab;
        emit(p, c, &lab);
        printf("first difference: [%s] %s: recorded %c, planner %c\n", key(c).c_str(), lab[i].c_str(),
               line[want.size() + i], got[i]);
        return 1;
      }
    rows += got.size();
  }
  if (std::getline(in, line) && !line.empty()) {
    printf("table has more lines than contexts\n");
    return 1;
  }
  printf("%zu recorded decisions reproduced, anchors %s\n", rows, fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}
#endif
