// Stand-alone check of the C-ABI's deferral rule (orion_amd/csrc/deferral.h),
// which is all it includes.  usage: deferral_check [STREAMS.txt]
//
// 1. Observational equivalence, exhaustively.  Two symbolic interpreters over
//    expression strings such as add(c0,rot(c0)) and rescale(moddown(lt(c1))):
//    Ref runs every call op by op; Mach keeps a deferral::Pending, sends the
//    events the entry points of backend.hip send and carries out the actions
//    step() returns.  Over every call sequence of length <= 4 on three
//    ciphertext handles (and those the calls return), from the empty state and
//    from each pending state: the live handle sets are equal; every handle an
//    action reads is live and formed, and what a call reads holds Ref's
//    expression; after every call each handle that is not owed pending work holds Ref's
//    expression, and all do once what is pending has run (which is what any
//    call that reads one sees).
// 2. Failure.  The same at length <= 3 with each executed action made to
//    throw: the call that ran it reports the error, the handles owed the
//    pending work (and no others) are poisoned, DeleteCiphertext's handle is
//    gone all the same, no other handle changed, nothing is pending.
// 3. Streams.  Each "stream NAME" section of the file, one call per line as
//    "op arg0 arg1 ret" (-1: none), is run through the state machine; prints
//    how many rotations ran fused, were dropped or ran plain, and how many
//    ModDowns ran merged with their rescale, plain, or were dropped.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>
#include "deferral.h"

using namespace deferral;

// ---- expression strings, interned ------------------------------------------
static std::vector<std::string> g_expr;
static std::unordered_map<std::string, int> g_expr_id;
static std::unordered_map<unsigned long long, int> g_memo;
static int intern(const std::string& s) {
  auto it = g_expr_id.find(s);
  if (it != g_expr_id.end()) return it->second;
  g_expr.push_back(s);
  return g_expr_id[s] = (int)g_expr.size() - 1;
}
static const char* const FN[] = {"rot", "add", "rescale", "moddown", "lt"};
enum { ROT, ADD, RESCALE, MODDOWN, LT };
static int expr(int fn, int a, int b = -1) {
  const unsigned long long key = ((unsigned long long)fn << 48) | ((unsigned long long)(a + 1) << 24) | (b + 1);
  auto it = g_memo.find(key);
  if (it != g_memo.end()) return it->second;
  const std::string s = std::string(FN[fn]) + "(" + g_expr[a] + (b >= 0 ? "," + g_expr[b] : "") + ")";
  return g_memo[key] = intern(s);
}

// ---- the alphabet ----------------------------------------------------------
enum Op { ROTATE_NEW, ADD_CT, DELETE_CT, RESCALE_CT, RESCALE_NEW, LT_PENDING, LT_FINISHED, READ, KEEP, NOP };
// (LT_PENDING / LT_FINISHED: a transform or product whose result comes back
// holding its accumulator, or finished; READ: a flushing call that reads its
// argument; KEEP: a metadata read)
static const char* const OP_NAME[NOP] = {"RotateNew", "AddCiphertext", "DeleteCiphertext", "Rescale", "RescaleNew",
                                         "EvaluateLinearTransform", "MulRelinCiphertextNew", "Decrypt",
                                         "GetCiphertextLevel"};
static const int OP_ARGS[NOP] = {1, 2, 1, 1, 1, 1, 1, 1, 1};

constexpr int MAXH = 8;  // 3 handles, one from the starting state, one per call
enum { DEAD = -1, UNFORMED = -2 };

static long g_checks = 0;
struct Made {
  int op, a, b;
};
static Made g_trail[8];  // the calls so far, for a failure report
static int g_ntrail = 0;
static void fail(const char* what);
#define EXPECT(cond)           \
  do {                         \
    ++g_checks;                \
    if (!(cond)) fail(#cond);  \
  } while (0)

static void fail(const char* what) {
  printf("FAILED: %s\n  after:", what);
  for (int i = 0; i < g_ntrail; ++i)
    printf(" %s%s(%d,%d)", OP_NAME[g_trail[i].op], g_trail[i].op == LT_FINISHED ? "*" : "", g_trail[i].a, g_trail[i].b);
  printf("\n");
  exit(1);
}

// ---- op by op ---------------------------------------------------------------
struct Ref {
  int v[MAXH];
  int alloc() const {
    for (int i = 0; i < MAXH; ++i)
      if (v[i] == DEAD) return i;
    fail("out of handles");
    return -1;
  }
  void call(Op op, int a, int b) {
    switch (op) {
      case ROTATE_NEW: v[alloc()] = expr(ROT, v[a]); break;
      case ADD_CT: v[a] = expr(ADD, v[a], v[b]); break;
      case DELETE_CT: v[a] = DEAD; break;
      case RESCALE_CT: v[a] = expr(RESCALE, v[a]); break;
      case RESCALE_NEW: v[a] = expr(RESCALE, v[a]), v[alloc()] = v[a]; break;
      case LT_PENDING:
      case LT_FINISHED: v[alloc()] = expr(MODDOWN, expr(LT, v[a])); break;
      default: break;
    }
  }
};

// ---- the state machine and its executor -------------------------------------
struct Thrown {};
// the action made to throw (Act::None: none); after_rotation: RotateThenAdd
// throws in its addition
static Act g_throw = Act::None;
static bool g_throw_after_rotation = false;

struct Mach {
  int v[MAXH], acc[MAXH];  // acc: the accumulator of a pending ModDown (Ciphertext::pend)
  bool poison[MAXH];
  Pending st;
  const Ref* ref = nullptr;  // Ref before the running call: what a read must see

  // what an action reads: no action names a deleted handle, or an unformed one
  int have(int h) const {
    EXPECT(h >= 0 && h < MAXH && v[h] != DEAD);
    EXPECT(v[h] != UNFORMED);
    return v[h];
  }
  // what a call reads, once the gate has run: Ref's expression
  int read(int h) const {
    if (ref) EXPECT(have(h) == ref->v[h]);
    return have(h);
  }
  int alloc() const {
    Ref r;
    memcpy(r.v, v, sizeof v);
    return r.alloc();
  }
  // backend.hip defer_apply
  Act apply(const Event& e) {
    const Pending d = st;
    const Step s = step(d, e);
    st = s.next;
    try {
      if (s.act != Act::None && s.act == g_throw && !g_throw_after_rotation) throw Thrown();
      switch (s.act) {
        case Act::Rotate:
        case Act::RotateThenAdd:
          EXPECT(v[d.r] == UNFORMED);
          v[d.r] = expr(ROT, have(d.x));
          if (s.act == Act::RotateThenAdd) {
            if (g_throw == s.act && g_throw_after_rotation) throw Thrown();
            v[d.x] = expr(ADD, have(d.x), have(d.r));
          }
          break;
        case Act::FusedRotateAdd:
          EXPECT(v[d.r] == UNFORMED);
          v[d.x] = expr(ADD, have(d.x), expr(ROT, have(d.x)));
          break;
        case Act::ModDown:
        case Act::ModDownRescale:
          EXPECT(v[d.r] == UNFORMED && acc[d.r] >= 0);
          v[d.r] = expr(MODDOWN, acc[d.r]);
          if (s.act == Act::ModDownRescale) v[d.r] = expr(RESCALE, v[d.r]);
          acc[d.r] = -1;
          break;
        case Act::RecordAdd: EXPECT(v[d.x] != DEAD && v[d.r] == UNFORMED); break;
        case Act::DropRotation:
        case Act::DropModDown: EXPECT(v[d.r] == UNFORMED); break;
        case Act::None: break;
      }
    } catch (const Thrown&) {
      poison[d.r] = true;
      if (d.kind == Kind::RotationAdded) poison[d.x] = true;
      throw;
    }
    return s.act;
  }
  // the C-ABI entry points of backend.hip: the gate of API_BEGIN, then the body
  void call(Op op, int a, int b) {
    static const std::vector<bool> keeps = [] {  // (each entry point looks its row up once)
      std::vector<bool> k;
      for (const char* name : OP_NAME) k.push_back(deferral::call(name).keeps);
      return k;
    }();
    apply({keeps[op] ? Ev::Keeps : Ev::Flushes});
    int r;
    switch (op) {
      case ROTATE_NEW:
        read(a);
        v[r = alloc()] = UNFORMED;
        apply({Ev::OpenRotation, a, r, 1});
        break;
      case ADD_CT:
        if (apply({Ev::Add, a, b}) == Act::RecordAdd) break;
        v[a] = expr(ADD, read(a), read(b));
        break;
      case DELETE_CT:
        try {
          apply({Ev::Delete, a});
        } catch (const Thrown&) {
          v[a] = DEAD;
          throw;
        }
        v[a] = DEAD;
        break;
      case RESCALE_CT:
      case RESCALE_NEW:
        if (apply({Ev::Rescale, a}) != Act::ModDownRescale) v[a] = expr(RESCALE, read(a));
        if (op == RESCALE_NEW) v[alloc()] = v[a];  // (the copy of what the call itself wrote)
        break;
      case LT_PENDING:
        r = alloc();
        acc[r] = expr(LT, read(a));
        v[r] = UNFORMED;
        apply({Ev::OpenModDown, r});
        break;
      case LT_FINISHED: v[alloc()] = expr(MODDOWN, expr(LT, read(a))); break;
      case READ: read(a); break;
      default: break;
    }
  }
};

// after a call: the same live handles; every handle not owed pending work
// holds Ref's expression; all do once the pending work has run
static void check_equal(const Ref& R, Mach M) {
  for (int h = 0; h < MAXH; ++h) {
    EXPECT((R.v[h] == DEAD) == (M.v[h] == DEAD));
    const bool owed = M.st.kind != Kind::None && (h == M.st.r || (M.st.kind == Kind::RotationAdded && h == M.st.x));
    if (!owed) EXPECT(M.v[h] == R.v[h]);
  }
  if (M.st.kind == Kind::None) return;
  const Act keep = g_throw;
  g_throw = Act::None;
  M.ref = nullptr;
  M.apply({Ev::Flushes});
  g_throw = keep;
  EXPECT(M.st.kind == Kind::None);
  for (int h = 0; h < MAXH; ++h) EXPECT(M.v[h] == R.v[h]);
}
// after a call that threw (M0: the machine before it)
static void check_failure(const Ref& R, const Mach& M0, const Mach& M, Op op, int a) {
  EXPECT(M.st.kind == Kind::None);
  for (int h = 0; h < MAXH; ++h) {
    const bool gone = R.v[h] == DEAD || (op == DELETE_CT && h == a);
    EXPECT(gone == (M.v[h] == DEAD));
    if (gone) continue;
    const bool owed = M0.v[h] != R.v[h];  // reported as written, never written
    EXPECT(M.poison[h] == owed);
    if (!owed) EXPECT(M.v[h] == R.v[h]);
  }
}

static long g_sequences = 0, g_failures = 0;
static void enumerate(const Ref& R, const Mach& M, int left) {
  for (int op = 0; op < NOP; ++op)
    for (int a = 0; a < MAXH; ++a)
      for (int b = 0; b < (OP_ARGS[op] == 2 ? MAXH : 1); ++b) {
        if (R.v[a] == DEAD || (OP_ARGS[op] == 2 && R.v[b] == DEAD)) continue;
        g_trail[g_ntrail++] = Made{op, a, b};
        Ref R2 = R;
        Mach M2 = M;
        M2.ref = &R;
        bool threw = false;
        try {
          M2.call((Op)op, a, b);
        } catch (const Thrown&) {
          threw = true;
        }
        if (threw) {
          ++g_failures;
          check_failure(R, M, M2, (Op)op, a);
        } else {
          R2.call((Op)op, a, b);
          check_equal(R2, M2);
          ++g_sequences;
          if (left > 1) enumerate(R2, M2, left - 1);
        }
        --g_ntrail;
      }
}
static void enumerate_from_every_state(int length) {
  static const struct { Op op; int a, b; } START[4][2] = {{{NOP, 0, 0}, {NOP, 0, 0}},
                                                          {{ROTATE_NEW, 0, 0}, {NOP, 0, 0}},
                                                          {{ROTATE_NEW, 0, 0}, {ADD_CT, 0, 3}},
                                                          {{LT_PENDING, 0, 0}, {NOP, 0, 0}}};
  static const Kind KIND[4] = {Kind::None, Kind::Rotation, Kind::RotationAdded, Kind::ModDown};
  for (int s = 0; s < 4; ++s) {
    Ref R;
    Mach M;
    for (int h = 0; h < MAXH; ++h) {
      R.v[h] = M.v[h] = h < 3 ? intern("c" + std::to_string(h)) : DEAD;
      M.acc[h] = -1, M.poison[h] = false;
    }
    const Act keep = g_throw;
    g_throw = Act::None;
    g_ntrail = 0;
    for (const auto& c : START[s])
      if (c.op != NOP) M.call(c.op, c.a, c.b), R.call(c.op, c.a, c.b), g_trail[g_ntrail++] = Made{c.op, c.a, c.b};
    g_throw = keep;
    EXPECT(M.st.kind == KIND[s]);
    enumerate(R, M, length);
  }
}

// ---- recorded call streams ---------------------------------------------------
static void run_streams(const char* path) {
  std::ifstream in(path);
  if (!in) fail("cannot read the streams file");
  std::string line, name;
  Pending st;
  long n[9] = {0};
  auto send = [&](const Event& e) {
    const Step s = step(st, e);
    st = s.next, ++n[(int)s.act];
    return s.act;
  };
  auto finish = [&] {
    if (name.empty()) return;
    send({Ev::Flushes});  // what is pending at the end runs on its own
    printf("stream %s: rotations fused %ld dropped %ld plain %ld; moddowns merged %ld plain %ld dropped %ld\n",
           name.c_str(), n[(int)Act::FusedRotateAdd], n[(int)Act::DropRotation],
           n[(int)Act::Rotate] + n[(int)Act::RotateThenAdd], n[(int)Act::ModDownRescale], n[(int)Act::ModDown],
           n[(int)Act::DropModDown]);
    memset(n, 0, sizeof n);
  };
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string op;
    int a = -1, b = -1, ret = -1;
    ls >> op;
    if (op == "stream") {
      finish();
      ls >> name;
      continue;
    }
    ls >> a >> b >> ret;
    send({deferral::call(op.c_str()).keeps ? Ev::Keeps : Ev::Flushes});
    if (op == "RotateNew") send({Ev::OpenRotation, a, ret, b});
    if (op == "AddCiphertext") send({Ev::Add, a, b});
    if (op == "DeleteCiphertext") send({Ev::Delete, a});
    if (op == "Rescale" || op == "RescaleNew") send({Ev::Rescale, a});
    // (every transform and product counted as leaving its ModDown pending)
    if (op == "EvaluateLinearTransform" || op == "MulRelinCiphertextNew") send({Ev::OpenModDown, ret});
  }
  finish();
}

int main(int argc, char** argv) {
  // the table: every name once, in order; the four calls that send their own
  // event pass the gate
  for (size_t i = 1; i < sizeof(kCalls) / sizeof(kCalls[0]); ++i) EXPECT(strcmp(kCalls[i - 1].name, kCalls[i].name) < 0);
  for (const char* fn : {"AddCiphertext", "DeleteCiphertext", "Rescale", "RescaleNew", "GetCiphertextLevel"})
    EXPECT(call(fn).keeps);
  for (const char* fn : {"RotateNew", "EvaluateLinearTransform", "MulRelinCiphertextNew", "Decrypt", "NewScheme"})
    EXPECT(!call(fn).keeps);
  EXPECT(call("RotateNew").capture && !call("Decrypt").capture && !call("OrionHipPeerCount").capture);

  enumerate_from_every_state(4);
  printf("%ld call sequences of length <= 4 equivalent (%ld checks)\n", g_sequences, g_checks);
  const long before = g_sequences;
  static const struct { Act act; bool after_rotation; } THROWS[] = {{Act::Rotate, false}, {Act::RotateThenAdd, false},
                                                                    {Act::RotateThenAdd, true},
                                                                    {Act::FusedRotateAdd, false},
                                                                    {Act::ModDown, false},
                                                                    {Act::ModDownRescale, false}};
  for (const auto& t : THROWS) {
    g_throw = t.act, g_throw_after_rotation = t.after_rotation;
    const long f0 = g_failures;
    enumerate_from_every_state(3);
    EXPECT(g_failures > f0);
  }
  g_throw = Act::None;
  printf("%ld failed flushes poisoned what they owed (%ld sequences of length <= 3)\n", g_failures,
         g_sequences - before);
  if (argc > 1) run_streams(argv[1]);
  return 0;
}
