// backend.hip -- context, device memory, keys, CKKS operators and the
// Lattigo-compatible C-ABI of liborion_hip.so (include/orion_hip.h).
//
// Operator algorithms follow Lattigo v6 as reached from
// /root/reference/orion/backend/lattigo/*.go; the CPU
// restatement they are checked against lives in oracle/ (tests only).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <shared_mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>
#include <complex>

#include "../../include/orion_hip.h"
#include "common.h"
#include "deferral.h"
#include "hostmath.h"
#include "launch.h"
#include "lt_blocks.h"
#include "ntt_route.h"
#include "tensor_sum.h"
#include "wire.h"

namespace orion {
struct LinTrans;
}
static std::vector<int> lt_bsgs_index(orion::LinTrans& T, int slots, int logRatio);

namespace orion {

#define HIPCHK(x)                                                                                  \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e_) + \
                                                   " at " + #x);                                   \
  } while (0)

static thread_local std::string g_last_error;

// ---------------------------------------------------------------------------
// device memory: size-class cache (no hipMalloc/hipFree on the op path)
// ---------------------------------------------------------------------------
// A captured hipGraph replays into the buffers its capture used, so every
// buffer handed out while capturing is pinned for the graph's lifetime: a
// pinned buffer that is released is parked instead of returning to the free
// lists, and nothing allocated later can alias a graph's temporaries.
class DevicePool {
  // ORION_DEBUG_POISON=1: fill each allocation with 0xA5 bytes, so a kernel that
  // reads memory nothing wrote fails deterministically
  bool poison_ = getenv("ORION_DEBUG_POISON") && atoi(getenv("ORION_DEBUG_POISON")) != 0;

 public:
  // every pool of the process shares one lock: the pipelines' contexts run on
  // threads of their own, a forced trim empties every pool, and a buffer can be
  // released by another context's thread than the one that allocated it (keys
  // and compiled objects are shared with the pipelines)
  static std::recursive_mutex& mu() {
    static auto* m = new std::recursive_mutex();
    return *m;
  }
  // ORION_POOL_CAP_BYTES: the device bytes all pools together may hold; an
  // allocation past it takes the failed-hipMalloc path (trim every pool's
  // cache, retry once) -- the regression test of that path, and a way to run
  // a workload inside a memory budget
  static double& cap_ref() {
    static double c = getenv("ORION_POOL_CAP_BYTES") ? atof(getenv("ORION_POOL_CAP_BYTES")) : 0;
    return c;
  }
  static double cap_bytes() { return cap_ref(); }
  // A cached buffer is reused for a request of up to its size when the
  // request is at least 7/8 of it (best fit): the limb counts of a chain's
  // levels make many nearby sizes, and exact-size classes alone left memory
  // cached in sizes no request took (ResNet-20 N=2^16 at batch 8 thrashed).
  void* alloc(size_t bytes) {
    std::lock_guard<std::recursive_mutex> lk(mu());
    void* p = nullptr;
    auto it = free_.lower_bound(bytes);
    if (it != free_.end() && it->first - bytes <= it->first / 8) {
      p = it->second.back();
      it->second.pop_back();
      if (it->second.empty()) free_.erase(it);
    } else {
      const bool over = cap_bytes() > 0 && stats()[0] + (double)bytes > cap_bytes();
      hipError_t e = over ? hipErrorOutOfMemory : hipMalloc(&p, bytes);
      if (e != hipSuccess) {
        // release cached buffers of every pool on the device (the scheme's,
        // its pipelines' and the bootstrappers' contexts), the largest first,
        // until the request fits; then, if it still does not, every cache --
        // not while capturing: a trim synchronises.  The failed call's error
        // is cleared: HIP keeps it as the thread's last error, and a later
        // launch check (hipGetLastError) would report it
        (void)hipGetLastError();
        for (DevicePool* q : registry())
          if (q->tracking_) throw std::runtime_error("device memory exhausted during graph capture");
        stats()[3] += 1;  // one forced trim per failed allocation, whatever the number of pools
        // first, the smallest cached buffer of any pool that is large enough
        // is taken over as it is (no free, no allocation: under memory
        // pressure a larger buffer serves the request); the device is drained
        // first, since another context's stream may still use its cache
        hipDeviceSynchronize();
        p = adopt_cached(bytes);
        if (p) {
          if (tracking_) touched_[p] = bytes;
          return p;
        }
        for (int pass = 0; pass < 2; ++pass) {
          // pass 0: twice the request (at least 1 GiB) from the largest
          // cached buffers; pass 1: everything
          trim_largest(pass == 0 ? std::max<size_t>(2 * bytes, (size_t)1 << 30) : SIZE_MAX);
          if (cap_bytes() > 0 && stats()[0] + (double)bytes > cap_bytes()) {
            if (pass == 0) continue;
            throw std::runtime_error("device memory exhausted: " + std::to_string(bytes) +
                                     " more bytes exceed the pool cap (ORION_POOL_CAP_BYTES) with every cache released");
          }
          e = hipMalloc(&p, bytes);
          if (e == hipSuccess) break;
          (void)hipGetLastError();
          if (pass == 1)
            throw std::runtime_error("device memory exhausted: hipMalloc of " + std::to_string(bytes) +
                                     " bytes failed with every pool's cache released (" +
                                     std::to_string((long long)stats()[0]) + " bytes held by live objects)");
        }
      }
      stats()[2] += 1;
      held_ += bytes;
      real_[p] = bytes;
      add_held((double)bytes);
    }
    if (tracking_) touched_[p] = bytes;
    // debugging: every buffer handed out holds garbage, not stale or zero pages
    // (skipped inside a graph capture: a device sync there would invalidate it)
    if (poison_ && !tracking_) {
      (void)hipDeviceSynchronize();
      (void)hipMemset(p, 0xA5, bytes);
    }
    return p;
  }
  // a pointer's allocated size (>= the bytes its holder asked for)
  size_t real(void* p) const {
    auto it = real_.find(p);
    return it == real_.end() ? 0 : it->second;
  }
  void release(void* p, size_t bytes) {
    std::lock_guard<std::recursive_mutex> lk(mu());
    bytes = real(p);  // cached by its allocated size
    if (pins_.count(p)) {
      parked_[p] = bytes;
      return;
    }
    if (tracking_ && !touched_.count(p)) {
      // predates the open capture: the captured work may read it at every
      // replay, so nothing recorded later in the capture may reuse it; it is
      // parked now and pinned with the graph's buffers at the end
      touched_[p] = bytes;
      parked_[p] = bytes;
      return;
    }
    free_[bytes].push_back(p);
  }
  // a capture that failed: buffers parked for it that no graph pins go back
  void unpark_unpinned(const std::vector<std::pair<void*, size_t>>& v) {
    std::lock_guard<std::recursive_mutex> lk(mu());
    for (auto& pb : v) {
      if (pins_.count(pb.first)) continue;
      auto pk = parked_.find(pb.first);
      if (pk != parked_.end()) {
        free_[real(pk->first)].push_back(pk->first);
        parked_.erase(pk);
      }
    }
  }
  // free the cached (unused) buffers
  void trim() {
    std::lock_guard<std::recursive_mutex> lk(mu());
    hipDeviceSynchronize();
    for (auto& kv : free_)
      for (void* p : kv.second) free_one(p);
    free_.clear();
  }
  // the smallest cached buffer of at least `bytes` in any pool, moved into
  // this pool (nullptr: none); the caller has drained the device
  void* adopt_cached(size_t bytes) {
    DevicePool* best = nullptr;
    size_t bsz = SIZE_MAX;
    for (DevicePool* q : registry()) {
      auto it = q->free_.lower_bound(bytes);
      if (it != q->free_.end() && it->first < bsz) best = q, bsz = it->first;
    }
    if (!best) return nullptr;
    auto it = best->free_.find(bsz);
    void* p = it->second.back();
    it->second.pop_back();
    if (it->second.empty()) best->free_.erase(it);
    if (best != this) {
      best->real_.erase(p);
      best->held_ -= bsz;
      real_[p] = bsz;
      held_ += bsz;
    }
    return p;
  }
  // free cached buffers of every pool, the largest first, until `need` bytes
  // are freed (or every cache is empty)
  static void trim_largest(size_t need) {
    std::lock_guard<std::recursive_mutex> lk(mu());
    hipDeviceSynchronize();
    std::vector<std::pair<size_t, DevicePool*>> sizes;
    for (DevicePool* q : registry())
      for (auto& kv : q->free_)
        if (!kv.second.empty()) sizes.push_back({kv.first, q});
    std::sort(sizes.begin(), sizes.end(), [](const std::pair<size_t, DevicePool*>& x,
                                              const std::pair<size_t, DevicePool*>& y) { return x.first > y.first; });
    size_t freed = 0;
    for (auto& sq : sizes) {
      auto it = sq.second->free_.find(sq.first);
      while (freed < need && it != sq.second->free_.end() && !it->second.empty()) {
        sq.second->free_one(it->second.back());
        it->second.pop_back();
        freed += sq.first;
      }
      if (it != sq.second->free_.end() && it->second.empty()) sq.second->free_.erase(it);
      if (freed >= need) break;
    }
  }
  DevicePool() {
    std::lock_guard<std::recursive_mutex> lk(mu());
    registry().push_back(this);
  }
  DevicePool(const DevicePool&) = delete;
  DevicePool& operator=(const DevicePool&) = delete;
  // every pool of the process (one per context), and process-wide counters:
  // device bytes held by the pools (handed out + cached), their peak,
  // hipMalloc calls, failed allocations that forced a trim of every cache
  static std::vector<DevicePool*>& registry() {
    // never destroyed: contexts held in namespace-scope statics are torn down
    // at library unload, possibly after a function-local static would be
    static auto* r = new std::vector<DevicePool*>();
    return *r;
  }
  static double* stats() {
    static double st[4] = {0, 0, 0, 0};
    return st;
  }
  static void add_held(double d) {
    stats()[0] += d;
    if (stats()[0] > stats()[1]) stats()[1] = stats()[0];
  }
  size_t cached() const {
    std::lock_guard<std::recursive_mutex> lk(mu());
    size_t c = 0;
    for (auto& kv : free_) c += kv.first * kv.second.size();
    return c;
  }
  // graph capture: record every buffer handed out until end_track()
  void begin_track() {
    std::lock_guard<std::recursive_mutex> lk(mu());
    touched_.clear();
    tracking_ = true;
  }
  std::vector<std::pair<void*, size_t>> end_track() {
    std::lock_guard<std::recursive_mutex> lk(mu());
    tracking_ = false;
    std::vector<std::pair<void*, size_t>> v(touched_.begin(), touched_.end());
    touched_.clear();
    return v;
  }
  void pin(const std::vector<std::pair<void*, size_t>>& v) {
    std::lock_guard<std::recursive_mutex> lk(mu());
    for (auto& pb : v) {
      if (pins_[pb.first]++) continue;
      auto fit = free_.find(real(pb.first));  // released during the capture: park it
      if (fit == free_.end()) continue;
      auto& fl = fit->second;
      for (size_t i = 0; i < fl.size(); ++i)
        if (fl[i] == pb.first) {
          fl[i] = fl.back();
          fl.pop_back();
          parked_[pb.first] = real(pb.first);
          break;
        }
      if (fl.empty()) free_.erase(fit);
    }
  }
  void unpin(const std::vector<std::pair<void*, size_t>>& v) {
    std::lock_guard<std::recursive_mutex> lk(mu());
    for (auto& pb : v) {
      auto it = pins_.find(pb.first);
      if (it == pins_.end() || --it->second > 0) continue;
      pins_.erase(it);
      auto pk = parked_.find(pb.first);
      if (pk != parked_.end()) {
        free_[real(pk->first)].push_back(pk->first);
        parked_.erase(pk);
      }
    }
  }
  ~DevicePool() {
    std::lock_guard<std::recursive_mutex> lk(mu());
    for (auto& kv : parked_) free_[real(kv.first)].push_back(kv.first);
    parked_.clear();
    trim();
    stats()[0] -= (double)held_;  // (buffers still handed out are released with their owners)
    auto& r = registry();
    r.erase(std::remove(r.begin(), r.end(), this), r.end());
  }

 private:
  void free_one(void* p) {
    const size_t b = real(p);
    hipFree(p);
    held_ -= b;
    add_held(-(double)b);
    real_.erase(p);
  }
  size_t held_ = 0;
  std::map<size_t, std::vector<void*>> free_;  // allocated size -> cached buffers
  std::unordered_map<void*, size_t> real_;     // every buffer this pool allocated -> its size
  bool tracking_ = false;
  std::unordered_map<void*, size_t> touched_, parked_;
  std::unordered_map<void*, int> pins_;
};

struct Buffer {
  DevicePool* pool;
  u64* p;
  size_t bytes;
  Buffer(DevicePool* pl, size_t b) : pool(pl), p((u64*)pl->alloc(b)), bytes(b) {}
  ~Buffer() { pool->release(p, bytes); }
};

// [ncomp][nlimb][B][N]
struct Poly {
  std::shared_ptr<Buffer> buf;
  int ncomp = 0, nlimb = 0, B = 0, N = 0;
  u64* ptr() const { return buf ? buf->p : nullptr; }
  long long batch_stride() const { return N; }
  long long limb_stride() const { return (long long)B * N; }
  long long comp_stride() const { return (long long)nlimb * B * N; }
};

// an evaluation key made for `level` (common.h key_pos): [digit][2][level+1+K][N]
struct EvKey {
  Poly k;
  int level = 0;
};

struct Ciphertext {
  Poly poly;
  int level = 0;
  long double scale = 1;
  // set when a deferred op that should have written this ciphertext failed:
  // every later use of the handle reports it (deleting it stays possible)
  std::string poison;
  // copy-on-write: handles made by RescaleNew share the rescaled input's
  // buffer (Lattigo returns a copy, evaluator.go:92-99); the first in-place op
  // on either one, while both are alive, copies it first (Context::inplace_ct)
  std::shared_ptr<char> share;
  // "ModDown pending" (deferral.h): the QP accumulator [Q 0..level][P] whose
  // final ModDown has not run; poly has no buffer yet
  Poly pend;
};

struct Plaintext {
  Poly poly;
  int level = 0;
  long double scale = 1;
  bool qp = false;  // limbs: Q 0..level then P (LT diagonals)
};

// The layout of a blocked linear transform (lt_blocks.h) and its device plans:
// one LtPlan per column chunk, columns in order.  They point at the members'
// plan copies of their diagonals (Context::build_layout).  A single transform
// holds the layout of itself as the 1 x 1 block.
struct LtLayout {
  lt_blocks::Plan plan;
  std::vector<int> first_chunk;  // per column: index of its first device plan
  LtPlan* d_plan = nullptr;      // = dev.get()
  std::shared_ptr<void> dev;     // owns d_plan (hipFree); captured graphs hold a reference
};

struct LinTrans {
  int level = 0, N1 = 1;
  float ratio = 1;
  std::vector<int> idx;                 // diagonal indices, as given
  std::map<int, Plaintext> diags;       // keyed by idx & (slots-1)
  std::map<int, Poly> sdiags;           // plan copies for lt_bsgs: limbs below 2^48 stored split24
  std::vector<int> giants, babies;      // sorted giants; babies in first-seen order
  // the transform as a 1 x 1 block (built at first evaluation, rebuilt when diagonals change)
  LtLayout lay;
  bool plan_dirty = true;
  // what a blocked transform (LtBlocks) remembers of a member: uid tells this
  // transform from a later one that reuses its handle id; rev counts the device
  // plans built (each build makes new plan copies of the diagonals)
  unsigned long long uid = 0, rev = 0;
  LinTrans() = default;
  LinTrans(const LinTrans&) = delete;
  LinTrans& operator=(const LinTrans&) = delete;
  LinTrans(LinTrans&& o) noexcept { *this = std::move(o); }
  LinTrans& operator=(LinTrans&& o) noexcept {
    level = o.level, N1 = o.N1, ratio = o.ratio;
    idx = std::move(o.idx), diags = std::move(o.diags), giants = std::move(o.giants), babies = std::move(o.babies);
    sdiags = std::move(o.sdiags);
    std::swap(lay, o.lay);
    plan_dirty = o.plan_dirty;
    uid = o.uid, rev = o.rev;
    return *this;
  }
  ~LinTrans() = default;
};

// A blocked linear transform: rows x cols member transforms of one level,
// evaluated as one call (Context::eval_lt_blocks).  Its device plans are
// rebuilt whenever a member's plan is (LinTrans::rev).
struct LtBlocks {
  int rows = 0, cols = 0, level = 0;
  std::vector<int> tids;                  // member handles, row-major
  std::vector<unsigned long long> uids;   // ... and which transforms they named
  std::vector<unsigned long long> revs;   // member plan revisions the device plans were built from
  LtLayout lay;
  bool built = false;
};

// a handle's context: the scheme's context is 0, pipeline i holds the ids
// [i << 20, (i + 1) << 20)
enum { kCtxShift = 20, kMaxCtx = 64 };
// birth stamps of pooled objects (HandlePool): a pipeline reading another
// context's compiled object orders its stream after the object's producer only
// when the object is younger than what it has already waited for
static std::atomic<unsigned long long> g_birth{1};

template <class T>
class HandlePool {  // lowest-free-id reuse (minheap.go:46-64)
 public:
  // another context's pool, by context index (nullptr: none); and the hook a
  // foreign lookup runs: (owner index, the object's birth stamp, ciphertext?)
  using Resolver = HandlePool<T>* (*)(int owner);
  using Hook = void (*)(int owner, unsigned long long birth);
  static Resolver& resolver() {
    static Resolver r = nullptr;
    return r;
  }
  static Hook& hook() {
    static Hook h = nullptr;
    return h;
  }
  // run on every foreign object get() returns (a capture on the acting
  // context keeps that object's device buffers alive with its graph)
  using Hold = void (*)(const T&);
  static Hold& hold() {
    static Hold h = nullptr;
    return h;
  }
  // run on every object get() returns (a poisoned ciphertext throws)
  using Check = void (*)(const T&);
  static Check& check() {
    static Check c = nullptr;
    return c;
  }
  // run on every foreign object get() returns, after the hook has ordered the
  // streams (a ciphertext whose ModDown is pending on its own context)
  using Fix = void (*)(T&, int owner);
  static Fix& fix() {
    static Fix f = nullptr;
    return f;
  }
  int add(T&& v) {
    std::lock_guard<std::mutex> lk(mu_);
    int id;
    if (!free_.empty()) {
      id = *free_.begin();
      free_.erase(free_.begin());
    } else {
      id = next_++;
    }
    map_[id] = Entry{std::make_unique<T>(std::move(v)), g_birth.fetch_add(1), false};
    if (born) born->insert(id);
    return id;
  }
  std::set<int>* born = nullptr;  // while set: ids handed out (graph capture)
  // Handles are unique across the contexts of a scheme: an id of another
  // context (a compiled plaintext or transform of the scheme read by a
  // pipeline, a ciphertext handed from one thread to another) resolves to that
  // context's object, after the hook has ordered this thread's stream after
  // the object's producer
  T& get(int id) {
    const int own = id >> kCtxShift;
    if (id >= 0 && own != (base_ >> kCtxShift)) {
      HandlePool* o = resolver() ? resolver()(own) : nullptr;
      if (!o || o == this) throw std::runtime_error("handle not found: " + std::to_string(id));
      unsigned long long birth = 0;
      T& v = o->get_local(id, &birth, true);
      if (check()) check()(v);
      if (hook()) hook()(own, birth);
      if (fix()) fix()(v, own);
      if (hold()) hold()(v);
      return v;
    }
    T& v = get_local(id, nullptr);
    if (check()) check()(v);
    return v;
  }
  // a new stamp for an object changed in place (a transform's diagonals)
  void touch(int id) {
    const int own = id >> kCtxShift;
    HandlePool* o = this;
    if (id >= 0 && own != (base_ >> kCtxShift)) o = resolver() ? resolver()(own) : nullptr;
    if (!o) throw std::runtime_error("handle not found: " + std::to_string(id));
    std::lock_guard<std::mutex> lk(o->mu_);
    auto it = o->map_.find(id);
    if (it != o->map_.end()) it->second.birth = g_birth.fetch_add(1);
  }
  bool has(int id) const {
    std::lock_guard<std::mutex> lk(mu_);
    return map_.count(id) != 0;
  }
  // owner of id: this pool, or the pool of the context its id names
  HandlePool* owner_pool(int id) {
    const int own = id >> kCtxShift;
    if (id < 0 || own == (base_ >> kCtxShift)) return this;
    HandlePool* o = resolver() ? resolver()(own) : nullptr;
    return o ? o : this;
  }
  // an object another context has read goes only once the device has drained:
  // that context's kernels may still read its buffer, which the owner's pool
  // would otherwise hand out again in the owner's stream order only
  void del(int id) {
    HandlePool* o = owner_pool(id);
    std::unique_ptr<T> dead;
    {
      std::lock_guard<std::mutex> lk(o->mu_);
      auto it = o->map_.find(id);
      if (it == o->map_.end()) return;
      if (it->second.foreign) (void)hipDeviceSynchronize();
      dead = std::move(it->second.obj);
      o->map_.erase(it);
      o->free_.insert(id);
    }
  }
  void reset() {
    std::lock_guard<std::mutex> lk(mu_);
    map_.clear();
    free_.clear();
    next_ = base_;
  }
  // ids from base on (a pipeline's handles live in a range of their own)
  void set_base(int b) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      base_ = b;
    }
    reset();
  }
  std::vector<int> live() const {
    std::lock_guard<std::mutex> lk(mu_);
    std::vector<int> v;
    for (auto& kv : map_) v.push_back(kv.first);
    return v;
  }

 private:
  struct Entry {
    std::unique_ptr<T> obj;
    unsigned long long birth = 0;
    bool foreign = false;  // read by another context
  };
  T& get_local(int id, unsigned long long* birth, bool foreign = false) {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = map_.find(id);
    if (it == map_.end()) throw std::runtime_error("handle not found: " + std::to_string(id));
    if (birth) *birth = it->second.birth;
    if (foreign) it->second.foreign = true;
    return *it->second.obj;
  }
  mutable std::mutex mu_;
  std::map<int, Entry> map_;
  std::set<int> free_;
  int base_ = 0, next_ = 0;
};

struct ProfRec {
  int cat;
  hipEvent_t e0, e1;
  double bytes, strict;
};
static const char* kProfNames[] = {"ntt_fwd", "ntt_inv", "elementwise", "basis_ext", "ks_mac", "automorph",
                                   "tensor", "rescale_prep", "lt_bsgs", "lt_giant", "ntt_bext",
                                   "mono_pack", "mono_unpack"};
// ntt_bext: forward NTTs whose prologue forms the extended limb (NTT_PRO_BEXT),
// priced (ns + 1) 8 N per limb-transform (+ 8 N for a subtract-and-scale epilogue)
enum { P_NTT_FWD = 0, P_NTT_INV, P_EW, P_BEXT, P_MAC, P_AUT, P_TENSOR, P_RSPREP, P_LTMAC, P_LTGIANT, P_NTT_BEXT,
       P_MONOPACK, P_MONOUNPACK, P_NCAT };

// wall-clock intervals of the profiled launches of every context (peer
// pipelines run concurrently), relative to one reference event
// (OrionHipProfileClock): the union per category is the time the GPU spent
// with at least one such launch running (OrionHipProfileUnion)
struct ProfIv {
  int cat;
  float t0, t1;
};
static hipEvent_t g_prof_ref = nullptr;
static std::vector<ProfIv> g_prof_iv;
static std::mutex g_prof_mu;  // g_prof_iv: every context's launches
// ORION_NTT_LOG: one line per NTT call for tools/pmc_summary.py -- one
// line-buffered file for the whole process, so the lines of every context
// (peer pipelines) stay in call order, which is dispatch order
static FILE* ntt_log_file() {
  static FILE* const f = []() -> FILE* {
    const char* p = getenv("ORION_NTT_LOG");
    FILE* h = p && *p ? fopen(p, "a") : nullptr;
    if (h) setvbuf(h, nullptr, _IOLBF, 0);
    return h;
  }();
  return f;
}

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
struct Context;
static Context* scheme_ctx();  // the scheme's context (index 0), or nullptr

struct Context {
  // index in the scheme's registry (0: the scheme's context, > 0: a pipeline,
  // -1: a bootstrapping context owned by another context); its device; the
  // lock every C-ABI call acting on it holds
  int index = -1, dev = 0;
  std::recursive_mutex mu;
  // per owner context: the birth stamp below which that context's objects are
  // known complete on this context's stream (HandlePool::get's hook)
  unsigned long long synced[kMaxCtx] = {0};
  int logN = 0, N = 0, L = 0, K = 0, dnum = 0, logScale = 0, h = 0;
  // ring (scheme.go:49-52): Standard Z[X]/(X^N + 1), N/2 complex slots, NthRoot
  // 2N; or ConjugateInvariant Z[X + X^-1]/(X^2N + 1) of degree N, N real
  // slots, NthRoot 4N (primes = 1 mod 4N; the NTT folds/unfolds, ntt.hip)
  bool ci = false;
  int slots = 0;
  u64 nthroot = 0;
  std::vector<u64> mods;  // QP
  hipStream_t stream = nullptr;
  bool own_stream = false;
  DevicePool pool;
  DeviceTables host_tb;
  DeviceTables* d_tb = nullptr;
  std::vector<void*> static_bufs;
  double2 *tw_inv = nullptr, *tw_fwd = nullptr;  // special FFT twiddles (encoder.hip)
  std::map<int, u64*> garner;                     // decode CRT tables per level
  Prng prng{0x0123456789abcdefull};               // key generation
  EncSampler enc_sampler;                         // encryption: ChaCha20 key, index, Gaussian table

  Poly sk, pk, rlk;  // rlk: full chain (level L - 1)
  bool have_sk = false, have_pk = false, have_rlk = false;
  // Galois keys, each made for the highest level it has been asked for.  A
  // key covers only the limbs and digits of its level, so a model whose
  // linear transforms run low in the chain (ResNet-20 at N = 2^16: LTs at
  // levels 1-4 under a 48-prime bootstrapping chain) keeps its ~120 keys in
  // a few GB instead of ~150 GB of full-chain keys.
  std::map<u64, EvKey> gks;
  std::map<u64, int> key_hint;  // galEl -> highest level of a linear transform that uses it
  std::map<u64, u32*> autidx;
  std::map<std::pair<int, int>, BasisExtTable*> betab;
  std::map<std::pair<int, int>, std::vector<int>> betab_pos;  // target positions (QP order)
  std::map<int, BasisExtTable*> modup_arr;  // level -> the digits' ModUp tables, contiguous (one device array)
  std::map<int, BextRescaleTable*> mdrs_tab;  // level -> the "ModDown, then rescale" table

  HandlePool<Plaintext> pts;
  HandlePool<Ciphertext> cts;
  HandlePool<LinTrans> lts;
  HandlePool<LtBlocks> ltbs;

  // hipGraphs captured from the library stream (OrionHipGraphBegin/End)
  struct GraphRec {
    hipGraph_t g = nullptr;
    hipGraphExec_t x = nullptr;
    std::vector<std::pair<void*, size_t>> pins;
    // every buffer the context's handles, keys and transforms referenced when
    // the capture ended: none of them returns to the pool (and can be handed
    // out again) while the graph may replay, whatever is deleted or replaced
    // meanwhile (DeleteCiphertext, a Galois key made again for a higher level,
    // LoadRotationKey, new LT diagonals or plans, DeleteLinearTransform)
    std::vector<std::shared_ptr<void>> holds;
  };
  std::set<int> capture_born;  // ciphertext ids created inside the open capture
  // buffers of other contexts' objects read inside the open capture (a
  // pipeline's graph reads the scheme's transforms and plaintexts)
  std::vector<std::shared_ptr<void>> capture_holds;
  std::map<int, GraphRec> graphs;
  int next_graph = 0;
  bool capturing = false;
  unsigned prof_saved = 0;

  unsigned prof = 0;  // bit mask of profiled kernel categories
  std::vector<ProfRec> prof_recs;
  std::vector<hipEvent_t> ev_free;
  // prof_bytes: the kernel's algorithmic bytes (for the NTT: 16 N per
  // limb-transform + 8 N per epilogue operand or addend it reads, the
  // "fused" model); prof_strict: SURVEY §8d's 16 N per limb-transform alone
  double prof_launch[P_NCAT] = {0}, prof_ms[P_NCAT] = {0}, prof_bytes[P_NCAT] = {0}, prof_strict[P_NCAT] = {0};

  ~Context() {
    hipDeviceSynchronize();
    btps.clear();  // circuits first: their buffers belong to the bootstrapping contexts' pools
    btp_ctx.clear();
    if (capturing) {
      hipGraph_t gr = nullptr;
      hipStreamEndCapture(stream, &gr);
      if (gr) hipGraphDestroy(gr);
    }
    for (auto& kv : graphs) {
      hipGraphExecDestroy(kv.second.x);
      hipGraphDestroy(kv.second.g);
    }
    graphs.clear();
    gks.clear();
    sk = pk = rlk = Poly();
    pts.reset();
    cts.reset();
    lts.reset();
    ltbs.reset();
    for (auto& kv : autidx) hipFree(kv.second);
    for (auto& kv : betab) hipFree(kv.second);
    for (auto& kv : modup_arr) hipFree(kv.second);
    for (auto& kv : mdrs_tab) hipFree(kv.second);
    for (auto& kv : garner) hipFree(kv.second);
    for (void* p : static_bufs) hipFree(p);
    if (d_tb) hipFree(d_tb);
    for (auto& r : prof_recs) {
      hipEventDestroy(r.e0);
      hipEventDestroy(r.e1);
    }
    for (auto e : ev_free) hipEventDestroy(e);
    if (own_stream && stream) hipStreamDestroy(stream);
  }

  // -- profiling -----------------------------------------------------------
  hipEvent_t ev() {
    if (!ev_free.empty()) {
      hipEvent_t e = ev_free.back();
      ev_free.pop_back();
      return e;
    }
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    return e;
  }
  struct Scope {
    Context* c;
    int cat;
    double bytes, strict;
    hipEvent_t e0 = nullptr;
    Scope(Context* ctx, int k, double b, double st = -1) : c(ctx), cat(k), bytes(b), strict(st < 0 ? b : st) {
      if (c->prof & (1u << cat)) {
        e0 = c->ev();
        hipEventRecord(e0, c->stream);
      }
    }
    ~Scope() {
      if (e0) {
        hipEvent_t e1 = c->ev();
        hipEventRecord(e1, c->stream);
        c->prof_recs.push_back(ProfRec{cat, e0, e1, bytes, strict});
        if (c->prof_recs.size() > 20000) c->prof_flush();
      }
    }
  };
  void prof_flush() {
    if (prof_recs.empty()) return;
    hipStreamSynchronize(stream);
    for (auto& r : prof_recs) {
      float ms = 0;
      hipEventElapsedTime(&ms, r.e0, r.e1);
      if (g_prof_ref) {
        float a0 = 0, a1 = 0;
        hipEventElapsedTime(&a0, g_prof_ref, r.e0);
        hipEventElapsedTime(&a1, g_prof_ref, r.e1);
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_prof_iv.push_back(ProfIv{r.cat, a0, a1});
      }
      prof_launch[r.cat] += 1;
      prof_ms[r.cat] += ms;
      prof_bytes[r.cat] += r.bytes;
      prof_strict[r.cat] += r.strict;
      ev_free.push_back(r.e0);
      ev_free.push_back(r.e1);
    }
    prof_recs.clear();
  }

  // -- graph capture ---------------------------------------------------------------
  // Every op issued between graph_begin and graph_end is recorded (not run)
  // into one hipGraph; a replay re-runs all its kernels on the library stream
  // with one launch.  The captured ops must not synchronise (keys, tables and
  // LT plans are made by a warm-up pass first); profiling is off meanwhile.
  void graph_begin() {
    if (capturing) throw std::runtime_error("a graph capture is already open");
    HIPCHK(hipStreamSynchronize(stream));
    prof_flush();
    prof_saved = prof;
    prof = 0;
    pool.begin_track();
    capture_born.clear();
    capture_holds.clear();
    cts.born = &capture_born;
    HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed));
    capturing = true;
  }
  int graph_end() {
    if (!capturing) throw std::runtime_error("no graph capture is open");
    capturing = false;
    cts.born = nullptr;
    prof = prof_saved;
    hipGraph_t gr = nullptr;
    const hipError_t e = hipStreamEndCapture(stream, &gr);
    auto touched = pool.end_track();
    if (e != hipSuccess || !gr) {
      if (gr) hipGraphDestroy(gr);
      pool.unpark_unpinned(touched);
      // an invalidated capture leaves its stream unusable: end whatever is
      // still open and, for the library's own stream, start a fresh one
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
        hipGraph_t g2 = nullptr;
        hipStreamEndCapture(stream, &g2);
        if (g2) hipGraphDestroy(g2);
      }
      (void)hipGetLastError();
      if (own_stream) {
        hipStreamDestroy(stream);
        HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
      }
      throw std::runtime_error(std::string("graph capture failed (an op synchronised or left the stream?): ") +
                               hipGetErrorString(e));
    }
    GraphRec r;
    r.g = gr;
    const hipError_t ei = hipGraphInstantiate(&r.x, gr, nullptr, nullptr, 0);
    if (ei != hipSuccess) {
      hipGraphDestroy(gr);
      pool.unpark_unpinned(touched);
      throw std::runtime_error(std::string("graph instantiation failed: ") + hipGetErrorString(ei));
    }
    pool.pin(touched);
    r.pins = std::move(touched);
    r.holds = graph_holds();
    r.holds.insert(r.holds.end(), capture_holds.begin(), capture_holds.end());
    capture_holds.clear();
    const int id = next_graph++;
    graphs[id] = std::move(r);
    return id;
  }
  void graph_launch(int id) {
    auto it = graphs.find(id);
    if (it == graphs.end()) throw std::runtime_error("graph not found: " + std::to_string(id));
    if (capturing) throw std::runtime_error("graph launch while capturing");
    HIPCHK(hipGraphLaunch(it->second.x, stream));
  }
  void graph_destroy(int id) {
    auto it = graphs.find(id);
    if (it == graphs.end()) return;
    HIPCHK(hipStreamSynchronize(stream));
    hipGraphExecDestroy(it->second.x);
    hipGraphDestroy(it->second.g);
    pool.unpin(it->second.pins);
    graphs.erase(it);
  }

  std::vector<std::shared_ptr<void>> graph_holds() {
    std::vector<std::shared_ptr<void>> h;
    auto add = [&h](const Poly& p) {
      if (p.buf) h.push_back(p.buf);
    };
    add(sk), add(pk), add(rlk);
    for (auto& kv : gks) add(kv.second.k);
    for (int id : cts.live()) add(cts.get(id).poly);
    for (int id : pts.live()) add(pts.get(id).poly);
    for (int id : lts.live()) {
      LinTrans& t = lts.get(id);
      for (auto& kv : t.diags) add(kv.second.poly);
      for (auto& kv : t.sdiags) add(kv.second);
      if (t.lay.dev) h.push_back(t.lay.dev);
    }
    for (int id : ltbs.live())
      if (ltbs.get(id).lay.dev) h.push_back(ltbs.get(id).lay.dev);
    return h;
  }
  // in-place ops inside a capture only on ciphertexts made inside it: on an
  // older handle a replay would apply the op again to its own output, and the
  // handle's level and scale would advance once (at capture) while its data
  // changes at every launch
  // a ciphertext an op is about to modify in place; cow = false: the caller
  // replaces the whole buffer (no copy of a shared one is needed)
  Ciphertext& inplace_ct(int id, bool cow = true) {
    // a buffer replaced here goes back to its owner's pool, which hands out
    // buffers in its own stream's order only: another context's ciphertext is
    // read, never changed
    if (index >= 0 && id >= 0 && (id >> kCtxShift) != index)
      throw std::runtime_error("in-place op on ciphertext " + std::to_string(id) + " of pipeline " +
                               std::to_string(id >> kCtxShift) + " from pipeline " + std::to_string(index) +
                               ": a ciphertext is changed only by the context (thread) that made it");
    Ciphertext& a = cts.get(id);
    if (capturing && !capture_born.count(id))
      throw std::runtime_error("in-place op on ciphertext " + std::to_string(id) +
                               ", which predates the graph capture (a replay would reapply it): clone it inside the "
                               "capture first");
    if (cow && a.share) {
      if (a.share.use_count() > 1) a.poly = clone(a).poly;  // the other handle keeps the old buffer
      a.share.reset();
    }
    return a;
  }
  // RescaleNew's result: a second handle on a's (just rescaled) buffer, when
  // nothing else (a captured graph) holds that buffer
  Ciphertext alias(Ciphertext& a) {
    if (!tun.defer || !a.poly.buf || a.poly.buf.use_count() != 1) return clone(a);
    if (!a.share) a.share = std::make_shared<char>(0);
    Ciphertext y;
    y.poly = a.poly;
    y.level = a.level;
    y.scale = a.scale;
    y.share = a.share;
    return y;
  }

  // the rotation or ModDown a C-ABI call left pending (deferral.h; defer_apply)
  deferral::Pending dfr;

  // lazily built tables, keys and host transfers synchronise, which would
  // invalidate an open capture (and leave HIP's stream state unusable): refuse
  // them first
  void no_capture(const char* what) const {
    if (capturing)
      throw std::runtime_error(std::string(what) +
                               " needs a host synchronisation, not allowed while capturing a graph (run the op "
                               "stream once before capturing it)");
  }
  // tables and plans made on first use go to the device in the library
  // stream's order: a blocking hipMemcpy runs on the legacy NULL stream, which
  // the non-blocking library stream does not wait for (a device-to-device
  // hipMemcpy can even return before the copy lands), so a kernel queued next
  // could read a table the copy has not finished, and a rewritten plan could
  // change under a kernel still queued on the stream
  void h2d(void* d, const void* h, size_t n) {
    HIPCHK(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }

  // -- allocation --------------------------------------------------------------
  Poly alloc(int ncomp, int nlimb, int B) {
    Poly p;
    p.ncomp = ncomp;
    p.nlimb = nlimb;
    p.B = B;
    p.N = N;
    p.buf = std::make_shared<Buffer>(&pool, (size_t)ncomp * nlimb * B * N * sizeof(u64) + 16);
    return p;
  }

  int qp_mod(int level, int pos) const { return pos <= level ? pos : L + (pos - level - 1); }

  // LimbSet over components [c0, c0+nc) and limb positions/moduli
  LimbSet ls(const Poly& P, int c0, int nc, const std::vector<int>& pos, const std::vector<int>& md,
             int nbatch = -1) const {
    LimbSet s;
    memset(&s, 0, sizeof(s));
    s.p = P.ptr() + c0 * P.comp_stride();
    s.comp_stride = P.comp_stride();
    s.limb_stride = P.limb_stride();
    s.batch_stride = P.batch_stride();
    s.ncomp = nc;
    s.nlimb = (int)pos.size();
    s.nbatch = nbatch < 0 ? P.B : nbatch;
    if (P.B == 1 && s.nbatch > 1) s.batch_stride = 0;  // broadcast
    if (pos.size() > ORION_MAXLIMB) throw std::runtime_error("too many limbs in one launch");
    for (size_t i = 0; i < pos.size(); ++i) {
      s.pos[i] = (unsigned char)pos[i];
      s.mod[i] = (unsigned char)md[i];
    }
    return s;
  }
  static std::vector<int> iota(int a, int b) {
    std::vector<int> v;
    for (int i = a; i < b; ++i) v.push_back(i);
    return v;
  }
  LimbSet lsq(const Poly& P, int c0, int nc, int level, int nbatch = -1) const {
    auto v = iota(0, level + 1);
    return ls(P, c0, nc, v, v, nbatch);
  }
  // QP limbs of a poly laid out [Q 0..lvl_alloc][P], used at `level` <= lvl_alloc
  LimbSet lsqp(const Poly& P, int c0, int nc, int level, int lvl_alloc, int nbatch = -1) const {
    std::vector<int> pos, md;
    for (int j = 0; j <= level; ++j) pos.push_back(j), md.push_back(j);
    for (int k = 0; k < K; ++k) pos.push_back(lvl_alloc + 1 + k), md.push_back(L + k);
    return ls(P, c0, nc, pos, md, nbatch);
  }
  LimbSet lsp(const Poly& P, int c0, int nc, int lvl_alloc) const {
    std::vector<int> pos, md;
    for (int k = 0; k < K; ++k) pos.push_back(lvl_alloc + 1 + k), md.push_back(L + k);
    return ls(P, c0, nc, pos, md);
  }

  // -- kernel wrappers ------------------------------------------------------------
  // NTT / INTT with a fused prologue (load, basis extension, rescale prep) and
  // epilogue (store, subtract-and-scale); bytes: 16 N per limb-transform
  static NttIO nio(const LimbSet& dst, const LimbSet& src) {
    NttIO io;
    memset(&io, 0, sizeof(io));
    io.dst = dst;
    io.src = src;
    return io;
  }
  int ntt_order = getenv("ORION_NTT_ORDER") ? atoi(getenv("ORION_NTT_ORDER")) : 2;
  // launch routes (ntt_route.h): the switches, and what init_moduli knows
  const NttTuning tun = NttTuning::from_env();
  NttEnv env;
  KeySwitchRoute ks_route(int B, int level, int aut = 0, bool want_keep = false) const {
    return keyswitch_route(env, tun, B, level, aut, want_keep);
  }
  // ORION_NTT_LOG=path: one line per NTT call ("<dispatches> <jobs> <epi> <inv>
  // <pro> <intjobs> <family>": dispatches = kernel launches of the call (1 or
  // 2); epi = the epilogue (NTT_EPI_*); pro = the prologue; intjobs =
  // limb-transforms on integer-path (>= 2^46) moduli; family 1 = ntt.hip, 2 =
  // ntt2.hip, 3 = ntt2s.hip, 4 = an ntt2s.hip INTT's rows pass alone), so
  // tools/pmc_summary.py can price each dispatch of a rocprofv3 pass with its
  // limb-transform count (persistent launches have fewer workgroups than
  // jobs) and break the NTT time down by launch class
  void log_ntt(int family, const NttIO& io, bool inv) {
    FILE* const ntt_log = ntt_log_file();
    if (!ntt_log) return;
    int nint = 0;
    for (int l = 0; l < io.dst.nlimb; ++l) nint += host_tb.mc[io.dst.mod[l]].f64 ? 0 : 1;
    const int dispatches = family == 2 || family == 3 ? 2 : 1;
    fprintf(ntt_log, "%d %d %d %d %d %d %d\n", dispatches, io.jobs, io.epi, inv ? 1 : 0,
            io.pro, io.jobs / std::max(1, io.dst.nlimb) * nint, family);
  }
  void prep_io(NttIO& io) {
    io.order = ntt_order;
    io.ci = ci ? 1 : 0;
    io.jobs = io.dst.ncomp * io.dst.nlimb * io.dst.nbatch;
    if (io.order == 2) {  // integer-path (>= 2^46) limbs are ~1.4x slower per transform: dispatch them first
      int k = 0;
      for (int pass = 0; pass < 2; ++pass)
        for (int l = 0; l < io.dst.nlimb; ++l)
          if ((host_tb.mc[io.dst.mod[l]].f64 != 0) == (pass == 1)) io.lord[k++] = (unsigned char)l;
    }
  }
  // a subtract-and-scale epilogue whose operand is the destination (the
  // routes' inplace_sub; the two-pass kernels then need a scratch intermediate)
  static bool inplace_sub(const NttIO& io) { return io.epi != NTT_EPI_STORE && io.ex.p == io.dst.p; }
  // the INTT iio (load prologue, store epilogue) and then the forward fio whose
  // BEXT / RESCALE prologue reads only the INTT's output (fio.src = iio.dst),
  // as the route says: the two launches, or (r.ifuse) the INTT's rows pass
  // alone, unless the producer's kernel already stored its intermediate in
  // iio.dst (r.rows_stored), and its columns pass inside the forward's
  // latency kernels
  void intt_then_fwd(NttIO iio, NttIO fio, const InvFwdRoute& r, double src_per_job = 0) {
    if (!r.ifuse) {
      ntt_io(iio, true);
      ntt_io(fio, false, src_per_job);
      return;
    }
    // the route was computed from limb counts: the forward reads exactly what the INTT wrote
    bool same = iio.dst.p == fio.src.p && iio.dst.nlimb == fio.src.nlimb && iio.dst.ncomp == fio.src.ncomp &&
                iio.dst.nbatch == fio.src.nbatch && iio.dst.comp_stride == fio.src.comp_stride &&
                iio.dst.limb_stride == fio.src.limb_stride && iio.dst.batch_stride == fio.src.batch_stride;
    for (int l = 0; same && l < iio.dst.nlimb; ++l)
      same = iio.dst.pos[l] == fio.src.pos[l] && iio.dst.mod[l] == fio.src.mod[l];
    if (!same) throw std::runtime_error("NTT: the fused forward does not read the INTT's output");
    const int ij = iio.dst.ncomp * iio.dst.nlimb * iio.dst.nbatch;
    prep_io(iio);
    iio.mid = iio.dst;  // the rows pass leaves its intermediate in the INTT's own output rows
    if (!r.rows_stored) {
      Scope sc(this, P_NTT_INV, 16.0 * N * ij);
      if (orion_launch_ntt2s(logN, iio, d_tb, true, stream, true)) throw std::runtime_error("NTT launch failed");
      log_ntt(4, iio, true);
    }
    fio.ifuse = 1;
    fio.imid = iio.dst;
    // segments: runs of target limbs on the same basis-extension table (the
    // same source limbs; the rescale prep has one source), at most tgroup each
    int k = 0;
    for (int l = 0; l < fio.dst.nlimb;) {
      int e = l + 1;
      while (e < fio.dst.nlimb && e - l < r.tgroup &&
             (fio.pro != NTT_PRO_BEXT || fio.bx_tab[e] == fio.bx_tab[l]))
        ++e;
      fio.tg_l0[k] = (unsigned char)l;
      fio.tg_n[k] = (unsigned char)(e - l);
      ++k;
      l = e;
    }
    fio.ntg = k;
    fio.tgroup = r.tgroup;
    ntt_io(fio, false, src_per_job);
  }
  // src_per_job: NTT_PRO_BEXT launches, the mean source limbs read per
  // limb-transform (their algorithmic bytes are (src_per_job + 1) 8 N, + 8 N
  // for a subtract-and-scale epilogue, in the ntt_bext category)
  void ntt_io(NttIO io, bool inv, double src_per_job = 0) {
    prep_io(io);
    const bool bx = io.pro == NTT_PRO_BEXT;
    // fused model: + 8 N for the subtract-and-scale operand, + 8 N for the word
    // a rotate-and-add store adds to; an automorphism's scatter index is a
    // table shared by every limb and image of the Galois element, amortised
    // like the twiddles and not counted.  strict: 16 N per
    // limb-transform, whatever the prologue and epilogue read
    const double per = (bx ? (src_per_job + 1) * 8.0 * N : 16.0 * N) + (io.epi != NTT_EPI_STORE ? 8.0 * N : 0.0) +
                       (io.epi == NTT_EPI_SUBSCALE_AUT_ACC ? 8.0 * N : 0.0);
    const double strict = 16.0 * N;
    const int cat = bx ? P_NTT_BEXT : inv ? P_NTT_INV : P_NTT_FWD;
    const NttFamily fam = ntt_family(env, tun, io.jobs, inv, io.pro, io.epi, inplace_sub(io));
    // a route's fusions name their kernels: the INTT columns pass exists in
    // the latency kernels only, the basis-extension prologue not in ntt.hip
    if ((io.ifuse && fam != Latency) || (bx && fam == OnePass))
      throw std::runtime_error("NTT: the launch's fusions do not fit its kernel family");
    if (fam != OnePass) {
      Poly scratch;
      io.mid = io.dst;
      // in-place tail: keep ex intact for pass 2; automorphism epilogue: a rows
      // workgroup stores into other rows of dst (and, accumulating, reads
      // their old words), so the intermediate cannot live there
      if (inplace_sub(io) || epi_aut(io.epi)) {
        scratch = alloc(io.dst.ncomp, io.dst.nlimb, io.dst.nbatch);
        io.mid = ls(scratch, 0, io.dst.ncomp, iota(0, io.dst.nlimb), std::vector<int>(io.dst.mod, io.dst.mod + io.dst.nlimb));
      }
      Scope sc(this, cat, per * io.jobs, strict * io.jobs);
      if (fam == Latency ? orion_launch_ntt2s(logN, io, d_tb, inv, stream) : orion_launch_ntt2(logN, io, d_tb, inv, stream))
        throw std::runtime_error("NTT launch failed");
      log_ntt(fam, io, inv);
      return;
    }
    // algorithmic bytes per limb-transform: read + write the limb (16 N), + 8 N
    // for the epilogue's second operand (per, above)
    Scope sc(this, cat, per * io.jobs, strict * io.jobs);
    if (orion_launch_ntt_io(logN, io, d_tb, inv, stream)) throw std::runtime_error("NTT launch failed");
    log_ntt(fam, io, inv);
  }
  void ntt(const LimbSet& s, bool inv) { ntt_io(nio(s, s), inv); }
  void ew(int op, const LimbSet& o, const LimbSet& a, const LimbSet& b, const std::vector<u64>* sc = nullptr) {
    std::vector<u64> s, ss;
    if (sc) {
      s = *sc;
      for (int l = 0; l < o.nlimb; ++l) ss.push_back(hm_shoup(s[l], mods[o.mod[l]]));
    }
    int nin = (op == EW_NEG || op == EW_SCALE || op == EW_ADDC || op == EW_COPY || op == EW_SPLIT24)
                  ? 1
                  : 2;
    if (op == EW_MULADD || op == EW_ADDSCALE) nin += 1;
    Scope scp(this, P_EW, 8.0 * N * o.ncomp * o.nlimb * o.nbatch * (nin + 1));
    orion_launch_ew(op, o, a, b, sc ? s.data() : nullptr, sc ? ss.data() : nullptr, d_tb, N, stream);
  }
  void ew1(int op, const LimbSet& o, const LimbSet& a, const std::vector<u64>* sc = nullptr) { ew(op, o, a, a, sc); }
  void copy(const LimbSet& o, const LimbSet& a) { ew(EW_COPY, o, a, a); }

  // -- tables ---------------------------------------------------------------------
  void setup(int logN_, const std::vector<int>& logQ, const std::vector<int>& logP, int logScale_, int h_,
             bool ci_ = false) {
    if ((int)(logQ.size() + logP.size()) > ORION_MAXMOD) throw std::runtime_error("too many moduli");
    for (int b : logQ)
      if (b > 61) throw std::runtime_error("moduli must be <= 61 bits");
    for (int b : logP)
      if (b > 61) throw std::runtime_error("moduli must be <= 61 bits");
    if (logN_ < 13 || logN_ > 16) throw std::runtime_error("logN must be 13..16 in this build");
    init_moduli(logN_, gen_moduli(logN_ + (ci_ ? 1 : 0), logQ, logP), logQ, logP, logScale_, h_, ci_);  // q = 1 mod NthRoot
  }
  // tables for explicit moduli m = [Q..., P...] (|Q| = |logQ|, |P| = |logP|)
  void init_moduli(int logN_, const std::vector<u64>& m, const std::vector<int>& logQ, const std::vector<int>& logP,
                   int logScale_, int h_, bool ci_) {
    logN = logN_;
    N = 1 << logN;
    ci = ci_;
    slots = ci ? N : N / 2;
    nthroot = (2 * (u64)N) << (ci ? 1 : 0);
    L = (int)logQ.size();
    K = (int)logP.size();
    if (K < 1) throw std::runtime_error("at least one P prime is required (hybrid key switching)");
    dnum = (L + K - 1) / K;
    logScale = logScale_;
    h = h_;
    if (L + K > ORION_MAXMOD || L + K > ORION_MAXLIMB) throw std::runtime_error("too many moduli");
    // the lazy NTT ranges (the cut quotient keeps forward values in [0, 8q)) and
    // lt_bsgs's 8-product Barrett (barrett_8q2, bar_k <= 60 for x < 8 q^2)
    // hold only for moduli below 2^61 (ntt_arith.h)
    for (u64 q : m)
      if (q >= (1ull << 61) || q < 3 || !(q & 1)) throw std::runtime_error("moduli must be odd and below 2^61");
    mods = m;
    logQ_bits = logQ;
    logP_bits = logP;
    if (!stream) {
      HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
      own_stream = true;
    }
    orion_ntt_init();
    {
      int dev = 0;
      HIPCHK(hipGetDevice(&dev));
      HIPCHK(hipDeviceGetAttribute(&env.n_cu, hipDeviceAttributeMultiprocessorCount, dev));
      env.logN = logN, env.ci = ci, env.K = K;
      env.max_limb = ORION_MAXLIMB, env.max_src = ORION_MAXSRC, env.max_group = ORION_MAXGROUP;
    }
    memset(&host_tb, 0, sizeof(host_tb));
    for (int m = 0; m < L + K; ++m) build_mod_tables(m);
    HIPCHK(hipMalloc(&d_tb, sizeof(DeviceTables)));
    HIPCHK(hipMemcpy(d_tb, &host_tb, sizeof(DeviceTables), hipMemcpyHostToDevice));
    for (int inv = 0; inv < 2; ++inv) {
      const std::vector<Cplx> tw = special_fft_twiddles(logN + (ci ? 1 : 0), inv != 0);  // slots = 2^(that - 1)
      void* d;
      HIPCHK(hipMalloc(&d, tw.size() * sizeof(double2)));
      HIPCHK(hipMemcpy(d, tw.data(), tw.size() * sizeof(double2), hipMemcpyHostToDevice));
      static_bufs.push_back(d);
      (inv ? tw_inv : tw_fwd) = (double2*)d;
    }
    // the blocking table copies above ran on the legacy NULL stream, which the
    // library stream does not wait for: drain the device before any kernel
    // reads a twiddle or constant table
    HIPCHK(hipDeviceSynchronize());
    memset(&enc_sampler, 0, sizeof(enc_sampler));
    gauss_cdt(3.2, ORION_GAUSS_BOUND, enc_sampler.cdt);
  }
  std::vector<int> logQ_bits, logP_bits;
  // per-modulus constants and NTT twiddle tables of QP index m (host_tb; device copy by the caller)
  void build_mod_tables(int m) {
    std::vector<ulonglong2> fw(N), iv(N);
    {
      const u64 q = mods[m];
      ModConst& mc = host_tb.mc[m];
      mc.q = q;
      mc.bar_k = 64 - __builtin_clzll(q);
      mc.bar_mu = (u64)(((u128)1 << (2 * mc.bar_k)) / q);
      mc.bar_mu2 = (u64)(((u128)1 << (2 * mc.bar_k + 2)) / q);
      mc.bar_mu8 = mc.bar_k <= 52 ? (u64)(((u128)1 << (2 * mc.bar_k + 8)) / q) : 0;
      mc.bar_mu3 = mc.bar_k <= 60 ? (u64)(((u128)1 << (2 * mc.bar_k + 3)) / q) : 0;
      // CI: the unfold's 1/2 rides on the inverse's final scaling, (2N)^-1
      mc.ninv = hm_invmod((u64)N << (ci ? 1 : 0), q);
      mc.ninv_s = hm_shoup(mc.ninv, q);
      const u64 g = primitive_root(q);
      const u64 psi = hm_powmod(g, (q - 1) / nthroot, q);  // primitive NthRoot-th root
      const u64 psii = hm_invmod(psi, q);
      // twiddles of the degree-M negacyclic NTT, M = NthRoot / 2, bit-reversed
      const int logM = logN + (ci ? 1 : 0), M = 1 << logM;
      std::vector<u64> tf(M), ti(M);
      u64 a = 1, b = 1;
      for (int j = 0; j < M; ++j) {
        const u64 r = hm_bitrev(j, logM);
        tf[r] = a;
        ti[r] = b;
        a = hm_mulmod(a, psi, q);
        b = hm_mulmod(b, psii, q);
      }
      // CI: after the fold, the N-point stage with m groups is the degree-2N
      // NTT's stage with 2m groups on its first half: twiddle m + i -> 2m + i
      // (oracle_new_ring)
      for (int k = 0; k < N; ++k) {
        int mm = 1;
        while (2 * mm <= k) mm <<= 1;
        const int src = ci ? (k ? k + mm : 0) : k;
        fw[k] = make_ulonglong2(tf[src], hm_shoup(tf[src], q));
        iv[k] = make_ulonglong2(ti[src], hm_shoup(ti[src], q));
      }
      mc.wl = hm_mulmod(iv[1].x, mc.ninv, q);
      mc.wl_s = hm_shoup(mc.wl, q);
      mc.ciw = ci ? tf[1] : 0;  // psi^N
      mc.ciw_s = ci ? hm_shoup(tf[1], q) : 0;
      // float64-path constants and centered twiddles for small moduli
      mc.f64 = mc.bar_k <= ORION_F64_BITS ? 1 : 0;
      mc.qd = (double)q;
      mc.qinv_d = 1.0 / (double)q;
      mc.ninv_d = (double)(mc.ninv > q / 2 ? (long long)mc.ninv - (long long)q : (long long)mc.ninv);
      mc.wl_d = (double)(mc.wl > q / 2 ? (long long)mc.wl - (long long)q : (long long)mc.wl);
      if (mc.f64) {
        std::vector<double> fd(N), id(N);
        for (int j = 0; j < N; ++j) {
          const u64 a1 = fw[j].x, b1 = iv[j].x;
          fd[j] = (double)(a1 > q / 2 ? (long long)a1 - (long long)q : (long long)a1);
          id[j] = (double)(b1 > q / 2 ? (long long)b1 - (long long)q : (long long)b1);
        }
        void *dfd, *did;
        HIPCHK(hipMalloc(&dfd, N * sizeof(double)));
        HIPCHK(hipMalloc(&did, N * sizeof(double)));
        HIPCHK(hipMemcpy(dfd, fd.data(), N * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(did, id.data(), N * sizeof(double), hipMemcpyHostToDevice));
        static_bufs.push_back(dfd);
        static_bufs.push_back(did);
        host_tb.fwd_d[m] = (const double*)dfd;
        host_tb.inv_d[m] = (const double*)did;
      }
      void *dfw, *div;
      HIPCHK(hipMalloc(&dfw, N * sizeof(ulonglong2)));
      HIPCHK(hipMalloc(&div, N * sizeof(ulonglong2)));
      HIPCHK(hipMemcpy(dfw, fw.data(), N * sizeof(ulonglong2), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(div, iv.data(), N * sizeof(ulonglong2), hipMemcpyHostToDevice));
      static_bufs.push_back(dfw);
      static_bufs.push_back(div);
      host_tb.fwd[m] = (const ulonglong2*)dfw;
      host_tb.inv[m] = (const ulonglong2*)div;
    }
  }

  // secret key coefficients (ternary) from its first limb
  std::vector<int64_t> secret_coeffs() {
    Poly t = alloc(1, 1, 1);
    ntt_io(nio(ls(t, 0, 1, {0}, {0}), ls(sk, 0, 1, {0}, {0})), true);
    std::vector<u64> host;
    download(t, host);
    std::vector<int64_t> s(N);
    const u64 q0 = mods[0];
    for (int i = 0; i < N; ++i) s[i] = host[i] > q0 / 2 ? -(int64_t)(q0 - host[i]) : (int64_t)host[i];
    return s;
  }
  // encryption randomness: ChaCha20 key from the seed, encryption index 0
  void seed_encryption(u64 seed) {
    enc_key_from_seed(seed, enc_sampler.key);
    enc_sampler.enc = 0;
  }

  u64 prod_mod(const std::vector<int>& src, int skip, u64 t) const {
    u64 r = 1 % t;
    for (int i = 0; i < (int)src.size(); ++i)
      if (i != skip) r = hm_mulmod(r, mods[src[i]] % t, t);
    return r;
  }

  // how a target's sum is formed (common.h BextTarget): every bound is checked
  // with the actual moduli, so each column and the final value fit their words
  // (the terms: y_i < s_i times qh_i < t, and v <= ns times nS < t)
  // 0: BEXT_WT / BEXT_NT off (timing switch)
  int bext_modes = getenv("ORION_BEXT_MODES") ? atoi(getenv("ORION_BEXT_MODES")) : 1;
  int bext_mode(const std::vector<int>& src, int ns, u64 t) const {
    const u128 M30 = (1u << 30) - 1, T1 = t - 1;
    u128 ssum = ns;  // sum (s_i - 1) + ns
    bool src32 = true, src62 = true;
    for (int i = 0; i < ns; ++i) {
      const u64 si = mods[src[i]];
      ssum += si - 1;
      src32 = src32 && si < (1ull << 32);
      src62 = src62 && si < (1ull << 62);
    }
    const u128 two64 = (u128)1 << 64;
    if (src32 && t < (1ull << 32) && (ssum + 1) * t < ((u128)1 << 63)) return BEXT_NARROW;
    if (!bext_modes) return BEXT_LAZY;
    if (ns >= 3 && src32 && t >= (1ull << 32) && t < (1ull << 61) && ssum * M30 < two64 &&
        ssum * T1 < (u128)4 * t * t)
      return BEXT_WT;
    // (columns: ns + 1 terms of a 30-bit piece times t - 1; the whole sum below
    // 2^96, so the folded high word is below 2^32)
    if (ns >= 4 && src62 && t < (1ull << 31) && (u128)(ns + 1) * M30 * T1 < two64 && ssum * T1 < ((u128)1 << 96))
      return BEXT_NT;
    return BEXT_LAZY;
  }

  // centered: a gadget digit (Lattigo DecomposeAndSplit extends a one-prime
  // digit from its centered representative; ModDown's ModUpExact does not)
  BasisExtTable* make_betab(const std::vector<int>& src, const std::vector<int>& dst, bool centered = false) {
    no_capture("a basis extension table");
    BasisExtTable T;
    fill_betab(T, src, dst, centered);
    BasisExtTable* d;
    HIPCHK(hipMalloc(&d, sizeof(T)));
    h2d(d, &T, sizeof(T));
    return d;
  }
  void fill_betab(BasisExtTable& T, const std::vector<int>& src, const std::vector<int>& dst, bool centered) const {
    memset(&T, 0, sizeof(T));
    T.ns = (int)src.size();
    T.nt = (int)dst.size();
    T.centered = centered && T.ns == 1 ? 1 : 0;
    T.chalf = mods[src[0]] >> 1;
    if (T.ns > ORION_MAXSRC || T.nt > ORION_MAXLIMB) throw std::runtime_error("basis extension too large");
    for (int i = 0; i < T.ns; ++i) {
      const u64 si = mods[src[i]];
      T.src_mod[i] = src[i];
      T.sq[i] = si;
      T.qhatinv[i] = hm_invmod(prod_mod(src, i, si), si);
      T.qhatinv_s[i] = hm_shoup(T.qhatinv[i], si);
      T.qf[i] = (double)si;
      T.qinv_f[i] = 1.0 / T.qf[i];
    }
    for (int t = 0; t < T.nt; ++t) {
      const u64 tm = mods[dst[t]];
      BextTarget& R = T.tgt[t];
      T.dst_mod[t] = dst[t];
      R.q = tm;
      const u64 S = prod_mod(src, -1, tm);
      for (int i = 0; i < T.ns; ++i) {
        R.qh[i] = prod_mod(src, i, tm);
        R.qhs[i] = hm_shoup(R.qh[i], tm);
      }
      R.nS = S ? tm - S : 0;
      R.nSs = hm_shoup(R.nS, tm);
      for (int v = 0; v < 3; ++v) R.vS[v] = hm_mulmod((u64)v, R.nS, tm);
      R.qd = (double)tm;
      R.tinv = 1.0 / (double)tm;
      R.tinv32 = std::ldexp(R.tinv, 32);
      R.k = 64 - __builtin_clzll(tm);
      R.mu2 = R.k <= 61 ? (u64)(((u128)1 << (2 * R.k + 2)) / tm) : 0;
      R.c64 = (u64)(((u128)1 << 64) % tm);
      auto pieces = [](u64 x, u32& a, u32& b, u32& c) {
        a = (u32)(x & 0x3fffffffu), b = (u32)((x >> 30) & 0x3fffffffu), c = (u32)(x >> 60);
      };
      for (int i = 0; i < T.ns; ++i) pieces(R.qh[i], R.h0[i], R.h1[i], R.h2[i]);
      pieces(R.nS, R.n0, R.n1, R.n2);
      R.mode = T.centered ? BEXT_LAZY : bext_mode(src, T.ns, tm);
    }
  }
  // ModUp of digit i at level: sources Q[lo,hi), targets = rest of QP in QP-position order
  BasisExtTable* modup_tab(int level, int digit, std::vector<int>& tpos) {
    auto key = std::make_pair(level, digit);
    auto it = betab.find(key);
    if (it != betab.end()) {
      tpos = betab_pos[key];
      return it->second;
    }
    const int lo = digit * K, hi = std::min((digit + 1) * K, level + 1);
    std::vector<int> src = iota(lo, hi), dst;
    tpos.clear();
    for (int j = 0; j <= level + K; ++j) {
      if (j >= lo && j < hi) continue;
      tpos.push_back(j);
      dst.push_back(qp_mod(level, j));
    }
    BasisExtTable* d = make_betab(src, dst, true);
    betab[key] = d;
    betab_pos[key] = tpos;
    return d;
  }
  // copies of the digits' ModUp tables in one array, so that modup_all_kernel
  // indexes them off a kernel argument (noalias: wave-uniform table reads
  // become scalar loads; through an array of pointers they were vector loads)
  const BasisExtTable* modup_tabs(int level) {
    auto it = modup_arr.find(level);
    if (it != modup_arr.end()) return it->second;
    no_capture("the ModUp table array");
    const int beta = (level + 1 + K - 1) / K;
    BasisExtTable* d;
    HIPCHK(hipMalloc(&d, sizeof(BasisExtTable) * beta));
    std::vector<int> tpos;
    for (int i = 0; i < beta; ++i)
      HIPCHK(hipMemcpyAsync(d + i, modup_tab(level, i, tpos), sizeof(BasisExtTable), hipMemcpyDeviceToDevice,
                             stream));
    HIPCHK(hipStreamSynchronize(stream));
    modup_arr[level] = d;
    return d;
  }
  BasisExtTable* moddown_tab(int level) {
    auto key = std::make_pair(level, -1);
    auto it = betab.find(key);
    if (it != betab.end()) return it->second;
    std::vector<int> src;
    for (int k = 0; k < K; ++k) src.push_back(L + k);
    BasisExtTable* d = make_betab(src, iota(0, level + 1));
    betab[key] = d;
    return d;
  }
  // the ModDown table of `level` (>= 1) with the constants of the rescale by
  // q_level folded into it (common.h BextRescaleTable)
  BextRescaleTable* moddown_rescale_tab(int level) {
    auto it = mdrs_tab.find(level);
    if (it != mdrs_tab.end()) return it->second;
    no_capture("a basis extension table");
    if (level < 1 || level >= L) throw std::runtime_error("moddown_rescale: no such level");
    std::vector<int> src;
    for (int k = 0; k < K; ++k) src.push_back(L + k);
    std::vector<BextRescaleTable> W(1);
    memset(&W[0], 0, sizeof(BextRescaleTable));
    fill_betab(W[0].bx, src, iota(0, level + 1), false);
    const std::vector<u64> pq = p_mod_q(level);
    const u64 ql = mods[level], h = ql >> 1;
    W[0].piv = level;
    W[0].pinv = hm_invmod(pq[level], ql);
    W[0].pinvs = hm_shoup(W[0].pinv, ql);
    W[0].h = h;
    for (int i = 0; i < level; ++i) {
      BextRescaleTarget& R = W[0].rt[i];
      R.pq = pq[i];
      R.pqs = hm_shoup(pq[i], mods[i]);
      R.hm = h % mods[i];
      R.ones = hm_shoup(1, mods[i]);
    }
    BextRescaleTable* d;
    HIPCHK(hipMalloc(&d, sizeof(BextRescaleTable)));
    h2d(d, W.data(), sizeof(BextRescaleTable));
    mdrs_tab[level] = d;
    return d;
  }

  u64 galois_element(int k) const {
    return hm_powmod(5, (u64)(long long)k & (nthroot - 1), nthroot);
  }
  const u32* aut_index(u64 g) {
    auto it = autidx.find(g);
    if (it != autidx.end()) return it->second;
    no_capture("an automorphism index table");
    // CI: the index over the degree-2N NTT; the ring keeps its first half,
    // which every g = 5^k (= 1 mod 4) maps onto itself
    std::vector<u32> idx(N);
    const int logM = logN + (ci ? 1 : 0);
    const u64 mask = nthroot - 1;
    for (int j = 0; j < N; ++j) {
      const u64 t1 = 2 * hm_bitrev(j, logM) + 1;
      const u64 t2 = (((g * t1) & mask) - 1) >> 1;
      idx[j] = (u32)hm_bitrev(t2, logM);
      if (idx[j] >= (u32)N) throw std::runtime_error("Galois element does not act on the ring");
    }
    u32* d;
    HIPCHK(hipMalloc(&d, N * sizeof(u32)));
    h2d(d, idx.data(), N * sizeof(u32));
    autidx[g] = d;
    return d;
  }
  void automorph(const LimbSet& o, const LimbSet& a, u64 g, bool acc) {
    const u32* idx = aut_index(g);
    Scope sc(this, P_AUT, 8.0 * N * o.ncomp * o.nlimb * o.nbatch * (acc ? 3 : 2));
    orion_launch_automorph(o, a, idx, d_tb, N, acc ? 1 : 0, stream);
  }

  // -- upload of host residues (coefficient domain) + NTT -------------------------------
  void upload(const Poly& P, const std::vector<u64>& host) {
    no_capture("a host upload");
    HIPCHK(hipMemcpyAsync(P.ptr(), host.data(), host.size() * sizeof(u64), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }
  void download(const Poly& P, std::vector<u64>& host) {
    no_capture("a host download");
    host.resize((size_t)P.ncomp * P.nlimb * P.B * N);
    HIPCHK(hipMemcpyAsync(host.data(), P.ptr(), host.size() * sizeof(u64), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }
  // small signed coefficients -> residues for moduli md, into host[l*N + n] of a [nl][N] block
  void small_residues(const std::vector<int64_t>& v, const std::vector<int>& md, u64* out) const {
    for (size_t l = 0; l < md.size(); ++l) {
      const u64 q = mods[md[l]];
      for (int n = 0; n < N; ++n) {
        const int64_t x = v[n];
        out[l * N + n] = x >= 0 ? (u64)x % q : (q - ((u64)(-x) % q)) % q;
      }
    }
  }
  std::vector<int64_t> sample_gauss() {
    std::vector<int64_t> e(N);
    for (auto& x : e) x = prng.gaussian(3.2, 19.2);
    return e;
  }
  std::vector<int64_t> sample_ternary_h(int hw) {
    std::vector<int64_t> s(N, 0);
    std::vector<int> perm(N);
    for (int i = 0; i < N; ++i) perm[i] = i;
    hw = std::min(hw, N);
    for (int i = 0; i < hw; ++i) {
      const int j = i + (int)(prng.next() % (u64)(N - i));
      std::swap(perm[i], perm[j]);
      s[perm[i]] = (prng.next() & 1) ? 1 : -1;
    }
    return s;
  }
  std::vector<u64> qp_mod_list() const {
    std::vector<u64> v;
    for (int j = 0; j < L + K; ++j) v.push_back(mods[j]);
    return v;
  }

  // ---------------------------------------------------------------------------
  // keys
  // ---------------------------------------------------------------------------
  void gen_secret() { import_secret(sample_ternary_h(h)); }
  // a secret with these (ternary) coefficients, expanded over QP (NTT domain)
  Poly secret_poly(const std::vector<int64_t>& s) {
    Poly p = alloc(1, L + K, 1);
    std::vector<u64> host((size_t)(L + K) * N);
    small_residues(s, iota(0, L + K), host.data());
    upload(p, host);
    ntt(ls(p, 0, 1, iota(0, L + K), iota(0, L + K)), false);
    return p;
  }
  void import_secret(const std::vector<int64_t>& s) {
    sk = secret_poly(s);
    have_sk = true;
  }
  // another context's keys (same chain), shared: the key polys are the same
  // device buffers (read-only once made), the loaded keys' host copies the
  // same host arrays
  void adopt_keys(const Context& o) {
    if (o.mods != mods) throw std::runtime_error("pipeline context: another modulus chain");
    HIPCHK(hipStreamSynchronize(o.stream));
    if (o.have_sk) sk = o.sk, have_sk = true;
    if (o.have_pk) pk = o.pk, have_pk = true;
    if (o.have_rlk) rlk = o.rlk, have_rlk = true;
    gks = o.gks;
    key_hint = o.key_hint;
    gk_host = o.gk_host;
  }
  LimbSet full(const Poly& P, int c0, int nc) const { return ls(P, c0, nc, iota(0, L + K), iota(0, L + K)); }

  void gen_public() {
    if (!have_sk) throw std::runtime_error("secret key not generated");
    pk = alloc(2, L + K, 1);
    std::vector<u64> a((size_t)(L + K) * N), e((size_t)(L + K) * N);
    for (int m = 0; m < L + K; ++m)
      for (int n = 0; n < N; ++n) a[(size_t)m * N + n] = prng.uniform(mods[m]);
    small_residues(sample_gauss(), iota(0, L + K), e.data());
    Poly tmp = alloc(1, L + K, 1);
    HIPCHK(hipMemcpyAsync(pk.ptr() + pk.comp_stride(), a.data(), a.size() * 8, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(pk.ptr(), e.data(), e.size() * 8, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    ntt(full(pk, 0, 1), false);
    ew(EW_MUL, full(tmp, 0, 1), full(pk, 1, 1), full(sk, 0, 1));
    ew(EW_SUB, full(pk, 0, 1), full(pk, 0, 1), full(tmp, 0, 1));
    have_pk = true;
  }

  // QP moduli of a key made for `level`: q_0..q_level, then p_0..p_{K-1}
  std::vector<int> key_mods(int level) const {
    std::vector<int> v = iota(0, level + 1);
    for (int k = 0; k < K; ++k) v.push_back(L + k);
    return v;
  }
  // evaluation key switching s_in -> s_out for ciphertexts up to `level`,
  // layout [beta][2][level+1+K][N] (beta = ceil((level+1)/K) digits); a
  // full-chain key (level L - 1) is [dnum][2][L+K][N]
  Poly gen_evk(const Poly& s_in, const Poly& s_out, int level) {
    no_capture("evaluation key generation");
    const int beta = (level + 1 + K - 1) / K, nl = level + 1 + K;
    const std::vector<int> md = key_mods(level), kp = iota(0, nl);
    const std::vector<u64> pq = p_mod_q(level);
    Poly k = alloc(2 * beta, nl, 1);
    Poly tmp = alloc(1, nl, 1);
    std::vector<u64> a((size_t)nl * N), e((size_t)nl * N);
    for (int i = 0; i < beta; ++i) {
      for (int x = 0; x < nl; ++x)
        for (int n = 0; n < N; ++n) a[(size_t)x * N + n] = prng.uniform(mods[md[x]]);
      small_residues(sample_gauss(), md, e.data());
      HIPCHK(hipMemcpyAsync(k.ptr() + (2 * i + 1) * k.comp_stride(), a.data(), a.size() * 8,
                            hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(k.ptr() + (2 * i) * k.comp_stride(), e.data(), e.size() * 8, hipMemcpyHostToDevice,
                            stream));
      HIPCHK(hipStreamSynchronize(stream));
      const LimbSet kb = ls(k, 2 * i, 1, kp, md), ka = ls(k, 2 * i + 1, 1, kp, md), lt = ls(tmp, 0, 1, kp, md);
      ntt(kb, false);
      ew(EW_MUL, lt, ka, ls(s_out, 0, 1, md, md));
      ew(EW_SUB, kb, kb, lt);
      // + P * s_in on the Q limbs of digit i
      const int lo = i * K, hi = std::min((i + 1) * K, level + 1);
      std::vector<int> dl = iota(lo, hi);
      const std::vector<u64> pm(pq.begin() + lo, pq.begin() + hi);
      ew(EW_ADDSCALE, ls(k, 2 * i, 1, dl, dl), ls(s_in, 0, 1, dl, dl), ls(s_in, 0, 1, dl, dl), &pm);
    }
    return k;
  }
  void gen_relin() {
    if (!have_sk) throw std::runtime_error("secret key not generated");
    Poly s2 = alloc(1, L + K, 1);
    ew(EW_MUL, full(s2, 0, 1), full(sk, 0, 1), full(sk, 0, 1));
    rlk = gen_evk(s2, sk, L - 1);
    have_rlk = true;
  }
  // LoadRotationKey's whole keys, for the ones it cut on the device
  struct HostKey {
    int level = 0;
    std::shared_ptr<const std::vector<u64>> words;  // [digit][2][level+1+K][N] (shared with the pipelines)
  };
  std::map<u64, HostKey> gk_host;
  int hinted_level(u64 g) const {
    auto it = key_hint.find(g);
    return it == key_hint.end() ? L - 1 : it->second;
  }
  // the Galois key of g, made for at least `level` (a key made for a lower
  // level is replaced by one for this level)
  void gen_galois(u64 g, int level) {
    auto have = gks.find(g);
    if (have != gks.end() && have->second.level >= level) return;
    // a pipeline's keys are the scheme's: a key it lacks (made, loaded or
    // raised to a higher level after the pipeline was created) is made by the
    // scheme's context, with the scheme's randomness, and shared, so every
    // context switches with the same key and a pipeline's output equals the
    // scheme's bit for bit
    Context* s = scheme_ctx();
    if (index > 0 && s && s != this) {
      no_capture("taking a Galois key from the scheme");
      std::lock_guard<std::recursive_mutex> lk(s->mu);  // (a pipeline may wait on the scheme: index order)
      s->gen_galois(g, level);
      HIPCHK(hipStreamSynchronize(s->stream));
      // the replaced key's buffer may return to the scheme's pool once this
      // context lets go of it: this stream is done reading it first
      if (have != gks.end()) HIPCHK(hipStreamSynchronize(stream));
      gks[g] = s->gks.at(g);
      return;
    }
    auto hk = gk_host.find(g);
    if (hk != gk_host.end() && hk->second.level >= level) {  // a loaded key, cut at load: the whole key
      no_capture("uploading a loaded rotation key past its cut level");
      const int kl = hk->second.level, kb = (kl + 1 + K - 1) / K;
      Poly k = alloc(2 * kb, kl + 1 + K, 1);
      upload(k, *hk->second.words);
      gks[g] = EvKey{k, kl};
      gk_host.erase(hk);
      return;
    }
    if (!have_sk)
      throw std::runtime_error(have == gks.end() ? "secret key not generated"
                                                 : "galois key " + std::to_string(g) + " covers level " +
                                                       std::to_string(have->second.level) + " < " +
                                                       std::to_string(level) +
                                                       " and there is no secret key (LoadRotationKey keeps a key "
                                                       "over the highest level of the linear transforms that exist "
                                                       "when it is loaded: load keys after creating the transforms "
                                                       "and before any higher-level rotation)");
    const u64 ginv = galois_inverse(g);
    Poly s_out = alloc(1, L + K, 1);
    automorph(full(s_out, 0, 1), full(sk, 0, 1), ginv, false);
    gks[g] = EvKey{gen_evk(sk, s_out, level), level};
  }
  const EvKey& galois_key(u64 g, int level) {
    gen_galois(g, level);  // Lattigo AddRotationKey semantics: generate on first use
    return gks.at(g);
  }

  // ---------------------------------------------------------------------------
  // key switching building blocks
  // ---------------------------------------------------------------------------
  // sub-range [first, first+count) of a LimbSet's limbs
  static LimbSet limbs(const LimbSet& x, int first, int count) {
    LimbSet s = x;
    s.nlimb = count;
    for (int i = 0; i < count; ++i) {
      s.pos[i] = x.pos[first + i];
      s.mod[i] = x.mod[first + i];
    }
    return s;
  }
  // decompose c.ncomp Q polys (limbs 0..level of c) into beta digits each,
  // extended to QP and in the NTT domain.  D layout [comp][digit][QP][B], QP
  // positions at lvl_alloc = level.  Digit i's own Q limbs (l / K == i) equal
  // c's and are not written: every consumer (ks_mac, lt_bsgs, lt_giant) reads
  // them from c.
  // r.cols_only: the forward NTT stops after the columns pass (the caller's
  // gadget product runs the rows pass, ks_mac_full_kernel)
  Poly decompose(const LimbSet& c, int level, int B, const DecomposeRoute& r) {
    const int nc = c.ncomp;
    const int beta = (level + 1 + K - 1) / K;
    const int nqp = level + 1 + K;
    Poly cinv = alloc(nc, level + 1, B);
    const NttIO iio = nio(lsq(cinv, 0, nc, level), c);  // out-of-place INTT
    Poly D = alloc(nc * beta, nqp, B);
    if (r.merged) {
      // small decomposition: every digit's ModUp in one launch (own limbs not
      // written), then one NTT over every digit's target limbs: limb (digit i,
      // QP position j) of comp c sits at comp c, position i*nqp + j of a
      // LimbSet whose comp stride spans the beta digits
      std::vector<int> md;
      for (int j = 0; j < nqp; ++j) md.push_back(qp_mod(level, j));
      LimbSet Dl = ls(D, 0, nc * beta, iota(0, nqp), md);
      LimbSet in = ls(cinv, 0, nc, iota(0, level + 1), iota(0, level + 1));
      std::vector<int> tpos, tmod;
      for (int i = 0; i < beta; ++i)
        for (int j = 0; j < nqp; ++j)
          if (!(j >= i * K && j < std::min((i + 1) * K, level + 1))) tpos.push_back(i * nqp + j), tmod.push_back(md[j]);
      if (r.bext_pro) {
        // every digit's extension formed in the prologue of one NTT over the
        // target limbs (no modup_all launch, no round trip through HBM)
        LimbSet T = ls(D, 0, nc, tpos, tmod);
        T.comp_stride = (long long)beta * D.comp_stride();
        NttIO io = nio(T, in);
        io.pro = NTT_PRO_BEXT;
        io.bx = modup_tabs(level);
        for (int i = 0; i < beta; ++i) io.bx_s0[i] = (unsigned char)(i * K);
        double srcs = 0;
        for (size_t l = 0; l < tpos.size(); ++l) {
          const int i = tpos[l] / nqp, j = tpos[l] % nqp, lo = i * K, ns = std::min(K, level + 1 - lo);
          io.bx_tab[l] = (unsigned char)i;
          io.bx_t[l] = (unsigned char)(j < lo ? j : j - ns);
          srcs += ns;
        }
        io.cols_only = r.cols_only ? 1 : 0;
        intt_then_fwd(iio, io, r.inv, srcs / (double)tpos.size());
        return D;
      }
      ntt_io(iio, true);
      {
        Scope sc(this, P_BEXT, 8.0 * N * B * nc * (level + 1 + beta * nqp - (level + 1)));
        if (orion_launch_modup_all(Dl, in, modup_tabs(level), beta, K, nqp, d_tb, N, stream))
          throw std::runtime_error("modup_all: bad launch shape");
      }
      if (r.tset) {
        LimbSet T = ls(D, 0, nc, tpos, tmod);
        T.comp_stride = (long long)beta * D.comp_stride();
        ntt(T, false);
      } else {
        ntt(Dl, false);  // (own limbs transformed too; their contents are unused)
      }
      return D;
    }
    ntt_io(iio, true);
    const long long dstride = (long long)beta * D.comp_stride();
    for (int i = 0; i < beta; ++i) {
      const int lo = i * K, hi = std::min((i + 1) * K, level + 1);
      std::vector<int> tpos;
      BasisExtTable* T = modup_tab(level, i, tpos);
      std::vector<int> tmod;
      for (int p : tpos) tmod.push_back(qp_mod(level, p));
      LimbSet in = ls(cinv, 0, nc, iota(lo, hi), iota(lo, hi));
      LimbSet out = ls(D, i, nc, tpos, tmod);
      out.comp_stride = dstride;
      if (i == beta - 1 ? r.bext_pro_last : r.bext_pro) {  // the extension formed in the NTT's prologue
        NttIO io = nio(out, in);
        io.pro = NTT_PRO_BEXT;
        io.bx = T;
        for (int t = 0; t < out.nlimb; ++t) io.bx_tab[t] = 0, io.bx_t[t] = (unsigned char)t;
        io.bx_s0[0] = 0;
        ntt_io(io, false, hi - lo);
        continue;
      }
      // ModUp as its own kernel (the ORION_BEXT_FUSE=0 path, and digits of more
      // than 2 limbs): y_i and the float64 quotient are shared by every target
      {
        Scope sc(this, P_BEXT, 8.0 * N * B * nc * (in.nlimb + out.nlimb));
        if (orion_launch_basis_ext(out, in, T, d_tb, N, stream))
          throw std::runtime_error("basis_ext: unsupported source count");
      }
      ntt(out, false);
    }
    return D;  // the own Q limbs of each digit are left unset: consumers read them from c

  }
  // grouped gadget products: out_g (comps 0/1 at o.p + g*out_gstride) =
  //   [add0_g on comp 0] + sum_i D_g,i * keys[g]_i,   D_g at d.p + g*d_gstride,
  // own Q limbs of each digit read from own (group stride own_gstride)
  void mac_groups(const LimbSet& o, long long out_gstride, const LimbSet& d, long long d_gstride,
                  const LimbSet& own, long long own_gstride, const std::vector<const u64*>& keys,
                  const std::vector<int>& klvl, int beta, const u64* add0 = nullptr, long long add_gstride = 0,
                  int add_nq = 0, const u64* add1 = nullptr, int rows_from = 0, bool fwd_rows = false) {
    const int G = (int)keys.size();
    for (int g0 = 0; g0 < G; g0 += ORION_MAXGROUP) {
      const int ng = std::min(ORION_MAXGROUP, G - g0);
      MacGroups mg;
      memset(&mg, 0, sizeof(mg));
      for (int g = 0; g < ng; ++g) mg.key[g] = keys[g0 + g], mg.klvl[g] = klvl[g0 + g];
      mg.L = L;
      mg.out_gstride = out_gstride;
      mg.d_gstride = d_gstride;
      mg.add_gstride = add_gstride;
      mg.own_gstride = own_gstride;
      mg.K = K;
      mg.add0 = add0 ? add0 + g0 * add_gstride : nullptr;
      mg.add1 = add1 ? add1 + g0 * add_gstride : nullptr;
      mg.add_nq = add0 ? add_nq : 0;
      mg.rows_from = rows_from;
      mg.logN = logN;
      mg.fwd_rows = (fwd_rows && rows_from > 0) ? 1 : 0;
      if (fwd_rows && rows_from == 0) throw std::runtime_error("mac_groups: forward rows without the ModDown rows pass");
      for (int j = 0; j < mg.add_nq; ++j) {  // P mod q_j: ModDown(u + P*a) = ModDown(u) + a exactly
        u64 P = 1;
        for (int k = 0; k < K; ++k) P = hm_mulmod(P, mods[L + k] % mods[o.mod[j]], mods[o.mod[j]]);
        mg.add_s[j] = P;
        mg.add_ss[j] = hm_shoup(P, mods[o.mod[j]]);
      }
      LimbSet oo = o, dd = d, ow = own;
      oo.p += g0 * out_gstride;
      dd.p += g0 * d_gstride;
      ow.p += g0 * own_gstride;
      const double rows = (double)o.nlimb * o.nbatch;
      const double dreads = d_gstride ? rows * ng * beta : rows * beta;
      const double adds = add0 ? (add_nq ? (add1 ? 2.0 : 1.0) * add_nq / o.nlimb : 1.0) : 0.0;
      Scope sc(this, P_MAC, 8.0 * N * (dreads + rows * ng * (2 + adds) + 2.0 * beta * ng * o.nlimb));
      if (orion_launch_ks_mac(oo, dd, ow, mg, ng, beta, d_tb, N, stream))
        throw std::runtime_error("ks_mac launch failed");
    }
  }
  u64 galois_inverse(u64 g) const {
    const u64 M = nthroot;
    u64 ginv = hm_powmod(g, M / 2 - 1, M);  // g^-1 mod NthRoot (the group order divides M/2)
    if ((g * ginv) % M != 1) {
      for (ginv = 1; ginv < M; ginv += 2)
        if ((g * ginv) % M == 1) break;
    }
    return ginv;
  }
  // x: x.ncomp polys, QP limbs in the order [Q 0..level][P 0..K-1] (any strides);
  // out = (x_Q - ModUp(INTT(x_P))) * P^-1.  Clobbers x's P limbs.  aut_g != 0:
  // out = sigma_g of that (a rotation's NTT-domain automorphism), applied in
  // the final NTT's store when its kernel can scatter, else by automorph();
  // aut_acc: out += sigma_g(...) instead
  // 1: lt_bsgs / lt_giant take their workgroups in XCD-aware order (every
  // coefficient block's diagonals and keys read into one XCD's L2)
  int lt_xcd = getenv("ORION_LT_XCD") ? atoi(getenv("ORION_LT_XCD")) : 1;
  // a ModDown's route where no producer stores through its rows pass
  ModDownRoute md_route(const LimbSet& x, int level, const LimbSet& out) const {
    return moddown_route(env, tun, x.ncomp, x.nbatch, level, 0, out.p == x.p);
  }
  void moddown(const LimbSet& x, int level, const LimbSet& out, const ModDownRoute& r, u64 aut_g = 0,
               bool aut_acc = false) {
    const int nc = x.ncomp, B = x.nbatch;
    LimbSet xp = limbs(x, level + 1, K);
    const bool scatter = r.scatter;
    Poly tmp;
    LimbSet dst = out;
    if (aut_g && !scatter) {  // the automorphism as its own launch, from a temporary
      tmp = alloc(nc, level + 1, B);
      dst = lsq(tmp, 0, nc, level);
    }
    auto epilogue = [&](NttIO& io) {
      io.epi = r.epi;
      if (scatter) {  // a scatter in place would overwrite ex words other rows still read
        if (dst.p == x.p) throw std::runtime_error("moddown: the automorphism epilogue cannot run in place");
        io.aut = aut_index(galois_inverse(aut_g));
      }
      io.ex = limbs(x, 0, level + 1);
      const std::vector<u64> pq = p_mod_q(level);
      for (int j = 0; j <= level; ++j) {
        io.s[j] = hm_invmod(pq[j], mods[j]);
        io.ss[j] = hm_shoup(io.s[j], mods[j]);
      }
    };
    if (r.bext_pro) {
      // the extension of the P limbs formed in the prologue of the NTT whose
      // epilogue is (x_Q - .) * P^-1: no basis_ext launch, no extended limbs in HBM
      NttIO io = nio(dst, xp);
      io.pro = NTT_PRO_BEXT;
      io.bx = moddown_tab(level);
      for (int j = 0; j <= level; ++j) io.bx_tab[j] = 0, io.bx_t[j] = (unsigned char)j;
      io.bx_s0[0] = 0;
      epilogue(io);
      intt_then_fwd(nio(xp, xp), io, r.inv, K);
    } else {
      ntt(xp, true);
      Poly ext = alloc(nc, level + 1, B);
      LimbSet le = lsq(ext, 0, nc, level);
      {
        Scope sc(this, P_BEXT, 8.0 * N * B * nc * (K + level + 1));
        if (orion_launch_basis_ext(le, xp, moddown_tab(level), d_tb, N, stream))
          throw std::runtime_error("basis_ext: unsupported source count");
      }
      NttIO io = nio(dst, le);  // NTT of the extension and (x_Q - .) * P^-1, fused
      epilogue(io);
      ntt_io(io, false);
    }
    if (aut_g && !scatter) automorph(out, dst, aut_g, aut_acc);
  }
  // ModDown of x (as moddown's, at `level` >= 1) and the rescale of its result
  // by q_level as one division by P q_level; out: limbs 0..level-1.  Both
  // transforms are linear, so the two subtractions are made once, in the
  // coefficient domain (common.h BextRescaleTable):
  //   out_i = (x_i - NTT(e_i + (P mod q_i) t_i)) (P q_level)^-1
  // which is the sequential result limb for limb: the float quotient is the
  // ModDown's, everything else exact.  Clobbers x's limbs level..level+K.
  void moddown_rescale(const LimbSet& x, int level, const LimbSet& out) {
    const int nc = x.ncomp, B = x.nbatch, l = level;
    if (l < 1) throw std::runtime_error("cannot rescale a level-0 ciphertext");
    if (out.nlimb != l) throw std::runtime_error("moddown_rescale: the output has level - 1");
    BextRescaleTable* W = moddown_rescale_tab(l);
    LimbSet xs = limbs(x, l, K + 1);  // limb l and the P limbs: adjacent in [Q 0..l][P]
    ntt(xs, true);
    Poly ext = alloc(nc, l, B);
    LimbSet le = lsq(ext, 0, nc, l - 1);
    {
      Scope sc(this, P_BEXT, 8.0 * N * B * nc * (K + 1 + l));
      if (orion_launch_basis_ext_rescale(le, xs, W, N, stream))
        throw std::runtime_error("basis_ext: unsupported source count");
    }
    NttIO io = nio(out, le);
    io.epi = NTT_EPI_SUBSCALE;
    io.ex = limbs(x, 0, l);
    const std::vector<u64> pq = p_mod_q(l - 1);
    for (int j = 0; j < l; ++j) {
      io.s[j] = hm_invmod(hm_mulmod(pq[j], mods[l] % mods[j], mods[j]), mods[j]);
      io.ss[j] = hm_shoup(io.s[j], mods[j]);
    }
    ntt_io(io, false);
  }
  // full key switch of c (Q, level) -> (k0, k1) written to out comps 0/1 (Q, level);
  // add0/add1 (optional, Q limbs 0..level with out's batch geometry): added to
  // comps 0/1 of the result, folded into the gadget product as P * add; aut_g:
  // the result permuted by that Galois element's automorphism (moddown), and
  // added to out's comps 0/1 for aut_acc
  void keyswitch(const KeySwitchRoute& r, const LimbSet& c, int level, int B, const Poly& key, int klvl,
                 Poly& out, const u64* add0 = nullptr, const u64* add1 = nullptr, u64 aut_g = 0,
                 bool aut_acc = false) {
    if (klvl < level) throw std::runtime_error("evaluation key made for a lower level");
    Poly u = alloc(2, level + 1 + K, B);
    Poly D = decompose(c, level, B, r.dec);
    const int beta = (level + 1 + K - 1) / K;
    const LimbSet uq = lsqp(u, 0, 2, level, level);
    // the gadget product may store the P limbs through the ModDown INTT's rows
    // pass, and then run the decomposition NTT's forward rows pass too
    mac_groups(uq, 0, lsqp(D, 0, beta, level, level), 0, c, 0, {key.ptr()}, {klvl}, beta, add0, 0,
               add0 ? level + 1 : 0, add1, r.mac_rows ? level + 1 : 0, r.mac_fwd_rows);
    if (r.end == KsEnd::KeepQP)
      out = u;  // no ModDown: the accumulator (Ciphertext::pend)
    else
      moddown(uq, level, lsq(out, 0, 2, level), r.md, aut_g, aut_acc);
  }
  std::vector<u64> p_mod_q(int level) const {
    std::vector<u64> v;
    for (int j = 0; j <= level; ++j) {
      u64 P = 1;
      for (int k = 0; k < K; ++k) P = hm_mulmod(P, mods[L + k] % mods[j], mods[j]);
      v.push_back(P);
    }
    return v;
  }

  // ---------------------------------------------------------------------------
  // ciphertext operators
  // ---------------------------------------------------------------------------
  Ciphertext new_ct(int level, int B, long double scale) {
    Ciphertext c;
    c.poly = alloc(2, level + 1, B);
    c.level = level;
    c.scale = scale;
    return c;
  }
  // a result whose final ModDown is pending: metadata now, the buffer when it runs
  Ciphertext pending_ct(int level, int B, long double scale) {
    Ciphertext c;
    c.poly.B = B;
    c.level = level;
    c.scale = scale;
    return c;
  }
  // runs the pending ModDown of r as the op-by-op path would have
  void finish_moddown(Ciphertext& r) {
    if (!r.pend.buf) return;
    const int B = r.pend.B;
    Poly o = alloc(2, r.level + 1, B);
    const LimbSet x = lsqp(r.pend, 0, 2, r.level, r.level), lo = lsq(o, 0, 2, r.level);
    moddown(x, r.level, lo, md_route(x, r.level, lo));
    r.poly = o;
    r.pend = Poly();
  }
  // ... or, when a rescale is what comes next, both as one division
  void finish_moddown_rescale(Ciphertext& r) {
    const int l = r.level, B = r.pend.B;
    Poly o = alloc(2, l, B);
    moddown_rescale(lsqp(r.pend, 0, 2, l, l), l, lsq(o, 0, 2, l - 1));
    r.poly = o;
    r.pend = Poly();
    r.level = l - 1;
    r.scale /= (long double)mods[l];
  }
  Ciphertext clone(const Ciphertext& a) {
    Ciphertext c = new_ct(a.level, a.poly.B, a.scale);
    copy(lsq(c.poly, 0, 2, a.level), lsq(a.poly, 0, 2, a.level));
    return c;
  }
  // image i of dst (its limbs 0..level) = the image src[i] points at, one
  // launch per ORION_MAXGATHER images (StackCiphertexts / SliceCiphertext);
  // bytes: 16 N per limb-image, read + write
  void gather(Ciphertext& dst, const std::vector<GatherSrc>& src) {
    const int nl = dst.level + 1;
    const Poly& D = dst.poly;
    if ((int)src.size() != D.B || D.nlimb < nl) throw std::runtime_error("gather: destination shape mismatch");
    for (int b0 = 0; b0 < D.B; b0 += ORION_MAXGATHER) {
      const int n = std::min(ORION_MAXGATHER, D.B - b0);
      GatherTable T;
      memset(&T, 0, sizeof(T));
      for (int i = 0; i < n; ++i) T.src[i] = src[b0 + i];
      Scope sc(this, P_EW, 16.0 * N * 2 * nl * n);
      if (orion_launch_gather(D.ptr() + (long long)b0 * D.batch_stride(), D.comp_stride(), D.limb_stride(), n, nl, T,
                              N, stream))
        throw std::runtime_error("gather launch failed");
    }
  }
  // the images [first, first + count) of a, as gather sources
  static void gather_sources(const Ciphertext& a, int first, int count, std::vector<GatherSrc>& out) {
    const Poly& P = a.poly;
    if (!P.ptr() || P.ncomp < 2 || P.nlimb < a.level + 1 || first < 0 || count < 0 || first + count > P.B)
      throw std::runtime_error("gather: source shape mismatch");
    for (int b = first; b < first + count; ++b)
      out.push_back(GatherSrc{P.ptr() + (long long)b * P.batch_stride(), P.comp_stride(), P.limb_stride()});
  }

  void rescale_inplace(Ciphertext& ct) {
    const int l = ct.level;
    if (l < 1) throw std::runtime_error("cannot rescale a level-0 ciphertext");
    const int B = ct.poly.B;
    LimbSet last = ls(ct.poly, 0, 2, {l}, {l});
    // (DivRoundByLastModulusNTT) prep of every other limb, NTT and (c - .) * q_l^-1, fused
    LimbSet cq = lsq(ct.poly, 0, 2, l - 1);
    NttIO io = nio(cq, last);
    io.pro = NTT_PRO_RESCALE;
    io.modL = l;
    io.epi = NTT_EPI_SUBSCALE;
    io.ex = cq;
    for (int j = 0; j < l; ++j) {
      io.s[j] = hm_invmod(mods[l] % mods[j], mods[j]);
      io.ss[j] = hm_shoup(io.s[j], mods[j]);
    }
    // INTT of the last limb, then the prep + NTT + tail
    intt_then_fwd(nio(last, last), io, rescale_route(env, tun, 2, B, l));
    ct.level = l - 1;
    ct.scale /= (long double)mods[l];
  }

  int batch_of(int a, int b) const {
    if (a == b || b == 1) return a;
    if (a == 1) return b;
    throw std::runtime_error("batch size mismatch");
  }

  // the relinearisation of a tensor d = (d0, d1, d2): (d0, d1) + keyswitch(d2),
  // the addition folded into the gadget product.  keep_qp: as eval_lt's
  Ciphertext relin_tail(const Poly& d, int level, int B, long double scale, bool keep_qp) {
    const KeySwitchRoute r = ks_route(B, level, 0, keep_qp);
    const bool pend = r.end == KsEnd::KeepQP;
    Ciphertext out = pend ? pending_ct(level, B, scale) : new_ct(level, B, scale);
    keyswitch(r, lsq(d, 2, 1, level), level, B, rlk, L - 1, pend ? out.pend : out.poly, d.ptr(),
              d.ptr() + d.comp_stride());
    return out;
  }
  // (tensor_kernel stays beside the one-pair tensor_sum_kernel, which computes
  // the same d: MulRelinCiphertextNew was 1.4-1.5% slower through it in three
  // of four cells, profiles/r14a_mul_relin_one_pair_ab.txt)
  Ciphertext mul_relin(const Ciphertext& a, const Ciphertext& b, bool keep_qp = false) {
    if (!have_rlk) throw std::runtime_error("relinearization key not generated");
    const int level = std::min(a.level, b.level);
    const int B = batch_of(a.poly.B, b.poly.B);
    Poly d = alloc(3, level + 1, B);
    {
      // distinct bytes: both operands' 2 components and the 3 outputs; a
      // square (Quad's x * x, activation.py:55) reads one ciphertext
      const bool square = a.poly.ptr() == b.poly.ptr();
      Scope sc(this, P_TENSOR, 8.0 * N * (level + 1) * B * (square ? 5 : 7));
      orion_launch_tensor(lsq(d, 0, 3, level), lsq(a.poly, 0, 2, level, B), lsq(b.poly, 0, 2, level, B), d_tb, N,
                          stream);
    }
    return relin_tail(d, level, B, a.scale * b.scale, keep_qp);
  }

  // sum_i a[i] x b[i] with one relinearisation (tensor_sum.h): one tensor pass
  // accumulates (d0, d1, d2) over all pairs, ORION_MAXTSUM pairs per launch,
  // then relin_tail.  The operands' batches are B or 1 (checked by the
  // caller); level = the minimum over the operands.  keep_qp: as eval_lt's
  Ciphertext mul_relin_sum(const std::vector<const Ciphertext*>& a, const std::vector<const Ciphertext*>& b, int level,
                           int B, long double scale, bool keep_qp = false) {
    if (!have_rlk) throw std::runtime_error("relinearization key not generated");
    const int n = (int)a.size();
    if (n < 1 || b.size() != a.size()) throw std::runtime_error("a sum of products needs as many a as b operands");
    Poly d = alloc(3, level + 1, B);
    const LimbSet ld = lsq(d, 0, 3, level);
    for (int c = 0; c < tsum::launches(n); ++c) {
      const int first = tsum::chunk_first(c), cnt = tsum::chunk_count(n, c);
      tsum::Table T;
      memset(&T, 0, sizeof(T));
      // the squares first (a pair of one buffer: two rows to read, not four),
      // each kind in the caller's order
      for (int sq = 1; sq >= 0; --sq) {
        for (int i = first; i < first + cnt; ++i) {
          const Poly &pa = a[i]->poly, &pb = b[i]->poly;
          if ((pa.ptr() == pb.ptr()) != (bool)sq) continue;
          tsum::Pair& e = T.pr[T.n++];
          e.a = pa.ptr(), e.a_comp = pa.comp_stride(), e.a_limb = pa.limb_stride();
          e.a_batch = pa.B == 1 && B > 1 ? 0 : pa.batch_stride();
          e.b = pb.ptr(), e.b_comp = pb.comp_stride(), e.b_limb = pb.limb_stride();
          e.b_batch = pb.B == 1 && B > 1 ? 0 : pb.batch_stride();
        }
        if (sq) T.nsq = T.n;
      }
      // distinct bytes per limb-image: 4 rows per pair (2 for a square), the 3
      // outputs, and d read back by every launch after the first
      Scope sc(this, P_TENSOR, 8.0 * N * (level + 1) * B * (4 * (cnt - T.nsq) + 2 * T.nsq + 3 + (c ? 3 : 0)));
      if (orion_launch_tensor_sum(ld, T, c > 0, d_tb, N, stream)) throw std::runtime_error("tensor sum launch failed");
    }
    return relin_tail(d, level, B, scale, keep_qp);
  }

  Ciphertext rotate(const Ciphertext& a, int k) { return apply_galois(a, galois_element(k)); }
  // out (acc: +)= sigma_g(a) = sigma_g((c0, 0) + keyswitch(c1)) with the Galois
  // key of g: the c0 addition folded into the gadget product, the automorphism
  // (an NTT-domain permutation) and the accumulation into the ModDown's store
  void galois_switch(const Ciphertext& a, u64 g, Poly& out, bool acc) {
    const int level = a.level, B = a.poly.B;
    const EvKey& key = galois_key(g, level);
    keyswitch(ks_route(B, level, acc ? 2 : 1), lsq(a.poly, 1, 1, level), level, B, key.k, key.level, out,
              a.poly.ptr(), nullptr, g, acc);
  }
  // sigma_{5^k}(a) into out's buffer (allocated here when it has none)
  void rotate_into(const Ciphertext& a, int k, Ciphertext& out) {
    if (!out.poly.buf) out.poly = new_ct(a.level, a.poly.B, a.scale).poly;
    out.level = a.level;
    galois_switch(a, galois_element(k), out.poly, false);
  }
  // sigma_g(a) (g = 2N - 1 is the complex conjugation of the slots)
  Ciphertext apply_galois(const Ciphertext& a, u64 g) {
    Ciphertext out = new_ct(a.level, a.poly.B, a.scale);
    galois_switch(a, g, out.poly, false);
    return out;
  }
  // a += sigma_{5^k}(a), in place: RotateNew(a, k) followed by
  // AddCiphertext(a, that rotation) (c1 is decomposed and c0 folded into the
  // gadget product before the ModDown writes a)
  void rotate_add_inplace(Ciphertext& a, int k) { galois_switch(a, galois_element(k), a.poly, true); }

  // -- hoisted rotations (orion_hip.h Part 2; hoist.h) ------------------------
  // sigma_g(a) for every g of gs, from one decomposition of a.c1: per chunk of
  // ORION_MAXHOIST rotating elements one gadget-product launch over all its
  // keys (ks_mac_hoisted_kernel; past hoist::in_registers the grouped ks_mac
  // with the shared decomposition) into a QP scratch [chunk][2][QP][B], then
  // one ModDown per output whose store applies the automorphism.  The
  // arithmetic is galois_switch's, so every output has its bits.  g = 1: a
  // copy of a.  Every key is made or checked before anything is allocated.
  std::vector<Ciphertext> rotate_hoisted(const Ciphertext& a, const std::vector<u64>& gs) {
    const int level = a.level, B = a.poly.B, nqp = level + 1 + K, beta = (level + 1 + K - 1) / K;
    std::vector<int> rot;  // the outputs that rotate
    for (size_t i = 0; i < gs.size(); ++i)
      if (gs[i] != 1) galois_key(gs[i], level), rot.push_back((int)i);
    std::vector<Ciphertext> out(gs.size());
    for (size_t i = 0; i < gs.size(); ++i)
      if (gs[i] == 1) out[i] = clone(a);
    const int nr = (int)rot.size();
    if (nr == 0) return out;
    const HoistRoute r = hoist_route(env, tun, B, level, false);
    const LimbSet c0 = lsq(a.poly, 0, 1, level), c1 = lsq(a.poly, 1, 1, level);
    Poly D = decompose(c1, level, B, r.dec);
    const LimbSet dl = lsqp(D, 0, beta, level, level);
    Poly u = alloc(2 * std::min(nr, ORION_MAXHOIST), nqp, B);  // reused by every chunk (stream order)
    const LimbSet uq = lsqp(u, 0, 2, level, level);
    const long long gstride = 2 * u.comp_stride();
    const std::vector<u64> pq = p_mod_q(level);
    for (int c = 0; c < hoist::launches(nr); ++c) {
      const int first = hoist::chunk_first(c), cnt = hoist::chunk_count(nr, c);
      if (hoist::in_registers(beta)) {
        MacHoist H;
        memset(&H, 0, sizeof(H));
        for (int k = 0; k < cnt; ++k) {
          const EvKey& kk = gks.at(gs[rot[first + k]]);
          H.keys.key[k] = kk.k.ptr(), H.keys.klvl[k] = kk.level;
        }
        H.keys.n = cnt;
        H.L = L, H.K = K, H.beta = beta;
        H.out_gstride = gstride;
        for (int j = 0; j <= level; ++j) H.add_s[j] = pq[j], H.add_ss[j] = hm_shoup(pq[j], mods[j]);
        // per row: the decomposition (beta digits, once for all keys), the c0
        // addend on the Q limbs, every key's output pair; per QP limb: each
        // key (2 beta)
        const double rows = (double)nqp * B;
        Scope sc(this, P_MAC, 8.0 * N * (rows * (beta + 2.0 * cnt) + (double)(level + 1) * B +
                                         (double)nqp * 2.0 * beta * cnt));
        if (orion_launch_ks_mac_hoisted(uq, dl, c1, c0, H, d_tb, N, stream))
          throw std::runtime_error("ks_mac_hoisted launch failed");
      } else {
        std::vector<const u64*> keys;
        std::vector<int> klvl;
        for (int k = 0; k < cnt; ++k) {
          const EvKey& kk = gks.at(gs[rot[first + k]]);
          keys.push_back(kk.k.ptr()), klvl.push_back(kk.level);
        }
        mac_groups(uq, gstride, dl, 0, c1, 0, keys, klvl, beta, a.poly.ptr(), 0, level + 1);
      }
      for (int k = 0; k < cnt; ++k) {
        Ciphertext o = new_ct(level, B, a.scale);
        moddown(lsqp(u, 2 * k, 2, level, level), level, lsq(o.poly, 0, 2, level), r.out_md, gs[rot[first + k]]);
        out[rot[first + k]] = std::move(o);
      }
    }
    return out;
  }
  // ModDown( sum_i r_i ) over the elements g_i of gs (orion_hip.h
  // OrionHipRotateSum), r_i = sigma_{g_i}( gadget(D, key_{g_i}) + (P c0, 0) )
  // in QP, or P a on the Q limbs where g_i = 1: one decomposition, the gadget
  // products and automorphisms summed in QP by one lt_giant launch whose giants
  // share the decomposition (group strides 0), one ModDown.  Every key is made
  // or checked before anything is allocated.
  Ciphertext rotate_sum(const Ciphertext& a, const std::vector<u64>& gs) {
    const int level = a.level, B = a.poly.B, nqp = level + 1 + K, beta = (level + 1 + K - 1) / K;
    if (gs.size() > ORION_MAXGROUP) throw std::runtime_error("rotate_sum: too many Galois elements for one launch");
    std::vector<u64> rot;
    u64 nid = 0;  // how often the identity appears
    for (u64 g : gs) {
      if (g == 1)
        ++nid;
      else
        galois_key(g, level), rot.push_back(g);
    }
    const HoistRoute r = hoist_route(env, tun, B, level, !rot.empty());
    LtGiants G;
    memset(&G, 0, sizeof(G));
    for (size_t k = 0; k < rot.size(); ++k) {  // (every key exists: gen_galois may replace one)
      const EvKey& kk = gks.at(rot[k]);
      G.key[k] = kk.k.ptr(), G.klvl[k] = kk.level, G.idx[k] = aut_index(rot[k]);
    }
    Ciphertext out = new_ct(level, B, a.scale);
    const std::vector<u64> pq = p_mod_q(level);
    // nid P a on the Q limbs, zeros on the P limbs: the sum itself without a
    // rotating term, lt_giant's zero giant with one
    Poly zp;
    LimbSet z;
    if (nid) {
      zp = alloc(2, nqp, B);
      z = lsqp(zp, 0, 2, level, level);
      std::vector<u64> s;
      for (int j = 0; j <= level; ++j) s.push_back(hm_mulmod(pq[j], nid % mods[j], mods[j]));
      HIPCHK(hipMemsetAsync(zp.ptr(), 0, (size_t)2 * nqp * B * N * sizeof(u64), stream));
      ew1(EW_SCALE, lsq(zp, 0, 2, level), lsq(a.poly, 0, 2, level), &s);
    }
    if (rot.empty()) {
      moddown(z, level, lsq(out.poly, 0, 2, level), r.sum_md);
      return out;
    }
    Poly D = decompose(lsq(a.poly, 1, 1, level), level, B, r.dec);
    // P c0 on the Q limbs, zeros on the P limbs (lt_giant reads every QP limb of t0)
    Poly t0 = alloc(1, nqp, B);
    HIPCHK(hipMemsetAsync(t0.ptr(), 0, (size_t)nqp * B * N * sizeof(u64), stream));
    ew1(EW_SCALE, lsq(t0, 0, 1, level), lsq(a.poly, 0, 1, level), &pq);
    Poly acc = alloc(2, nqp, B);
    const LimbSet la = lsqp(acc, 0, 2, level, level);
    G.ng = (int)rot.size();
    G.beta = beta, G.K = K, G.level = level, G.L = L;
    G.has_zero = nid ? 1 : 0;
    G.xcd = lt_xcd && (N / 256) % 8 == 0;
    G.rows_from = r.sum_md.inv.rows_stored ? level + 1 : 0;
    G.logN = logN;
    G.d_gstride = G.own_gstride = G.t0_gstride = 0;
    {
      // per row: the decomposition (beta digits) and the t0 term once, the
      // output pair and the identity's pair; per QP limb: each key (2 beta)
      const double rows = (double)nqp * B;
      Scope sc(this, P_LTGIANT,
               8.0 * N * (rows * (beta + 1.0 + 2.0 + 2.0 * G.has_zero) + (double)nqp * 2.0 * beta * G.ng));
      if (orion_launch_lt_giant(la, lsqp(D, 0, 1, level, level), lsq(a.poly, 1, 1, level),
                                lsqp(t0, 0, 1, level, level), nid ? z : la, G, d_tb, N, stream))
        throw std::runtime_error("lt_giant launch failed");
    }
    moddown(la, level, lsq(out.poly, 0, 2, level), r.sum_md);
    return out;
  }

  // -- complex packing (orion_hip.h Part 2) ---------------------------------
  // Two real images share one ciphertext as a + i b: I = NTT(X^(N/2)) is i on
  // every slot (5^j = 1 mod 4), and in the NTT domain it is w4 = psi^(N/2) on
  // the first half of a limb, -w4 on the second (kernels.hip
  // pack_complex_kernel), so the kernels take w4 per limb and read no table.
  // w4 of every Q limb and its Shoup companion: made at first use, kept.
  std::vector<u64> w4, w4s;
  void need_complex() {
    if (ci)
      throw std::runtime_error("complex packing needs the Standard ring (a ConjugateInvariant slot holds a real number)");
    if (!w4.empty()) return;
    for (int j = 0; j < L; ++j) {
      const u64 q = mods[j];
      const u64 psi = hm_powmod(primitive_root(q), (q - 1) / nthroot, q);  // build_mod_tables' root
      w4.push_back(hm_powmod(psi, (u64)N / 2, q));
      w4s.push_back(hm_shoup(w4.back(), q));
    }
  }
  void w4_of(const LimbSet& s, std::vector<u64>& w, std::vector<u64>& ws) const {
    for (int l = 0; l < s.nlimb; ++l) {
      if (s.mod[l] >= L) throw std::logic_error("complex packing runs on Q limbs");
      w.push_back(w4[s.mod[l]]), ws.push_back(w4s[s.mod[l]]);
    }
  }
  // o = a + I b on the images below npair, a alone on the rest; one launch
  // (bytes: a and o per row, b on the paired rows)
  void pack_launch(const LimbSet& o, const LimbSet& a, const LimbSet& b, int npair) {
    std::vector<u64> w, ws;
    w4_of(o, w, ws);
    Scope sc(this, P_EW, 8.0 * N * o.ncomp * o.nlimb * (2 * o.nbatch + npair));
    if (orion_launch_pack_complex(o, a, b, npair, w.data(), ws.data(), d_tb, N, stream))
      throw std::runtime_error("pack_complex launch failed (batch or limb count out of range)");
  }
  // re = x + y, im = I (y - x) on the images below nim; one launch
  void unpack_launch(const LimbSet& re, const LimbSet& im, const LimbSet& x, const LimbSet& y, int nim) {
    std::vector<u64> w, ws;
    w4_of(x, w, ws);
    Scope sc(this, P_EW, 8.0 * N * x.ncomp * x.nlimb * (3 * x.nbatch + nim));
    if (orion_launch_unpack_complex(re, im, x, y, nim, w.data(), ws.data(), d_tb, N, stream))
      throw std::runtime_error("unpack_complex launch failed (batch or limb count out of range)");
  }
  // a + I b at the lower of the two levels (batches and scales equal: the caller checks)
  Ciphertext pack_complex(const Ciphertext& a, const Ciphertext& b) {
    need_complex();
    const int level = std::min(a.level, b.level), B = a.poly.B;
    Ciphertext o = new_ct(level, B, a.scale);
    pack_launch(lsq(o.poly, 0, 2, level), lsq(a.poly, 0, 2, level), lsq(b.poly, 0, 2, level), B);
    return o;
  }
  // (a + conj a, -i (a - conj a)) = twice the real and the imaginary image,
  // held as the images themselves at twice the scale (exact, no level): the
  // conjugation's key switch, then one launch
  std::pair<Ciphertext, Ciphertext> unpack_complex(const Ciphertext& a) {
    need_complex();
    const int level = a.level, B = a.poly.B;
    Ciphertext yc = apply_galois(a, 2 * (u64)N - 1);
    Ciphertext re = new_ct(level, B, 2 * a.scale), im = new_ct(level, B, 2 * a.scale);
    unpack_launch(lsq(re.poly, 0, 2, level), lsq(im.poly, 0, 2, level), lsq(a.poly, 0, 2, level),
                  lsq(yc.poly, 0, 2, level), B);
    return {std::move(re), std::move(im)};
  }

  // -- monomial packing and the slot trace (orion_hip.h Part 2) ---------------
  // An image with n slots, projected onto Z[X^g] (g = N / (2 n)), occupies the
  // coefficients at multiples of g only, so g of them share one ciphertext as
  // sum_i X^i image_i; multiplying by X^-i and summing over the automorphisms
  // that fix Z[X^g] (slot_trace) pulls image i out again.  M_1 and M_-1, the
  // NTTs of X and of X^-1 = -X^(N-1) on every Q limb ([2][L][N], made at first
  // use by the forward NTT of the unit vectors, kept): the kernels form M_(+-i)
  // as running products (kernels.hip mono_pack_kernel).
  Poly mono;
  void check_mono_ring() const {
    if (ci)
      throw std::runtime_error("monomial packing needs the Standard ring (a ConjugateInvariant ring has no X^i "
                               "that the slot trace separates)");
  }
  void need_mono() {
    check_mono_ring();
    if (mono.buf) return;
    no_capture("the monomial factor table");
    std::vector<u64> host((size_t)2 * L * N, 0);
    for (int j = 0; j < L; ++j) {
      host[(size_t)j * N + 1] = 1;
      host[((size_t)L + j) * N + (N - 1)] = mods[j] - 1;
    }
    Poly m = alloc(2, L, 1);
    upload(m, host);
    ntt(lsq(m, 0, 2, L - 1), false);
    mono = m;
  }
  // ceil(B / g) for any B, g >= 1 (no B + g - 1: B may be any int)
  static long long mono_groups(long long B, long long g) { return (B + g - 1) / g; }
  void check_mono_g(int g) const {
    check_mono_ring();
    if (g < 1 || g > N)
      throw std::runtime_error("monomial packing: g = " + std::to_string(g) + " is out of range [1, " +
                               std::to_string(N) + "]");
  }
  // o_k = sum_i M_i a_(k + i h) on the limbs 0..level; one launch.  Bytes per
  // (comp, limb, group) row: its images and the output; per limb the factor row
  void mono_pack_launch(const LimbSet& o, const LimbSet& a, int level, int g) {
    Scope sc(this, P_MONOPACK, 8.0 * N * (o.nlimb * (o.ncomp * (double)(a.nbatch + o.nbatch) + 1)));
    if (orion_launch_mono_pack(o, a, lsq(mono, 0, 1, level), g, d_tb, N, stream))
      throw std::runtime_error("mono_pack launch failed (batch or limb count out of range)");
  }
  void mono_unpack_launch(const LimbSet& o, const LimbSet& x, int level, int g) {
    Scope sc(this, P_MONOUNPACK, 8.0 * N * (x.nlimb * (x.ncomp * (double)(o.nbatch + x.nbatch) + 1)));
    if (orion_launch_mono_unpack(o, x, lsq(mono, 1, 1, level), g, d_tb, N, stream))
      throw std::runtime_error("mono_unpack launch failed (batch or limb count out of range)");
  }
  // the batch of B images as h = ceil(B / g) groups: image k + i h rides in
  // group k at X^i.  The arguments are checked before the factor rows are made
  Ciphertext pack_monomials(const Ciphertext& a, int g) {
    check_mono_g(g);
    need_mono();
    const int level = a.level, B = a.poly.B;
    Ciphertext o = new_ct(level, (int)mono_groups(B, g), a.scale);
    mono_pack_launch(lsq(o.poly, 0, 2, level), lsq(a.poly, 0, 2, level), level, g);
    return o;
  }
  // out_(k + i h) = M_-i a_k: B images out of h = ceil(B / g) groups
  Ciphertext unpack_monomials(const Ciphertext& a, int g, int B) {
    check_mono_g(g);
    const long long need = B < 1 ? 0 : mono_groups(B, g);
    if (B < 1 || a.poly.B != need)
      throw std::runtime_error("cannot unpack " + std::to_string(B) + " images at g = " + std::to_string(g) +
                               " from a batch of " + std::to_string(a.poly.B) + ": ceil(B / g) = " +
                               std::to_string(need) + " groups are needed");
    need_mono();
    const int level = a.level;
    Ciphertext o = new_ct(level, B, a.scale);
    mono_unpack_launch(lsq(o.poly, 0, 2, level), lsq(a.poly, 0, 2, level), level, g);
    return o;
  }
  // the rotation amounts ns 2^s of the trace over the g = N / (2 ns) slots at
  // distance ns (Bootstrapper::trace_gal's order); checks the ring and ns
  std::vector<int> slot_trace_amounts(int ns) const {
    check_mono_ring();
    if (ns < 2 || ns > N / 2 || (ns & (ns - 1)))
      throw std::runtime_error("slots must be a power of two in [2, " + std::to_string(N / 2) + "]");
    std::vector<int> ks;
    for (int s = ns; s < N / 2; s *= 2) ks.push_back(s);
    return ks;
  }
  // every Galois key of the amounts made or checked at the top level, before
  // the caller allocates anything
  void slot_trace_keys(const std::vector<int>& ks) {
    for (int k : ks) {
      const u64 gel = galois_element(k);
      try {
        galois_key(gel, L - 1);
      } catch (const std::runtime_error& e) {  // Rotate's message, with the element it lacks
        throw std::runtime_error("slot trace: galois key " + std::to_string(gel) + " (rotation by " +
                                 std::to_string(k) + ") at level " + std::to_string(L - 1) + ": " + e.what());
      }
    }
  }
  // t = src (mean: g^-1 src, scaled before the rotations: after them it would
  // multiply the key-switch noise), then t += Rotate(t, k) for k of ks (checked
  // amounts whose keys exist); src: the limbs 0..level of a ciphertext's pair
  Ciphertext slot_trace_run(const Poly& src, int level, long double scale, const std::vector<int>& ks, bool mean) {
    Ciphertext t = new_ct(level, src.B, scale);
    const LimbSet tl = lsq(t.poly, 0, 2, level), sl = lsq(src, 0, 2, level);
    if (mean && !ks.empty()) {
      const u64 g = (u64)1 << ks.size();
      std::vector<u64> gi(level + 1);
      for (int l = 0; l <= level; ++l) gi[l] = hm_invmod(g % mods[l], mods[l]);
      ew1(EW_SCALE, tl, sl, &gi);
    } else {
      copy(tl, sl);
    }
    for (int k : ks) rotate_add_inplace(t, k);
    return t;
  }
  Ciphertext slot_trace(const Poly& src, int level, long double scale, int ns, bool mean) {
    const std::vector<int> ks = slot_trace_amounts(ns);
    slot_trace_keys(ks);
    return slot_trace_run(src, level, scale, ks, mean);
  }

  // scale matching for additions (Lattigo evaluateInPlace: the lower-scale
  // operand is multiplied by the rounded integer ratio when it is > 1)
  void add_like(Ciphertext& out, const Ciphertext& a, const LimbSet& b, long double bscale, int op) {
    const int level = out.level;
    LimbSet o = lsq(out.poly, 0, 2, level);
    LimbSet la = lsq(a.poly, 0, 2, level, out.poly.B);
    long double ratio = a.scale > bscale ? a.scale / bscale : bscale / a.scale;
    long long r = llroundl(ratio);
    if (r > 1) {
      std::vector<u64> sc;
      for (int j = 0; j <= level; ++j) sc.push_back((u64)r % mods[j]);
      if (a.scale > bscale) {
        Poly tb = alloc(b.ncomp, level + 1, out.poly.B);
        LimbSet lt = lsq(tb, 0, b.ncomp, level);
        ew1(EW_SCALE, lt, b, &sc);
        ew(op, lsq(out.poly, 0, b.ncomp, level), lsq(a.poly, 0, b.ncomp, level, out.poly.B), lt);
        if (b.ncomp == 1 && &out != &a) copy(lsq(out.poly, 1, 1, level), lsq(a.poly, 1, 1, level, out.poly.B));
        out.scale = a.scale;
        return;
      }
      ew1(EW_SCALE, o, la, &sc);
      ew(op, lsq(out.poly, 0, b.ncomp, level), lsq(out.poly, 0, b.ncomp, level), b);
      out.scale = bscale;
      return;
    }
    ew(op, lsq(out.poly, 0, b.ncomp, level), lsq(a.poly, 0, b.ncomp, level, out.poly.B), b);
    if (b.ncomp == 1 && &out != &a) copy(lsq(out.poly, 1, 1, level), lsq(a.poly, 1, 1, level, out.poly.B));
    out.scale = a.scale;
  }

  // device plan of a BSGS transform.  What belongs to the transform itself is
  // made here: the plan copies of its diagonals and the zero diagonal; the plan
  // is that of its layout as the 1 x 1 block (build_layout)
  void build_plan(LinTrans& T) {
    no_capture("building a linear transform's BSGS plan");
    // operand copies of the diagonals in lt_bsgs's split-MAC form (the
    // diagonals themselves stay canonical for serialisation)
    T.sdiags.clear();
    for (auto& kv : T.diags) {
      const Poly& src = kv.second.poly;
      Poly dst = alloc(src.ncomp, src.nlimb, src.B);
      std::vector<int> md;
      for (int j = 0; j < src.nlimb; ++j) md.push_back(qp_mod(T.level, j));
      ew(EW_SPLIT24, ls(dst, 0, 1, iota(0, src.nlimb), md), ls(src, 0, 1, iota(0, src.nlimb), md),
         ls(src, 0, 1, iota(0, src.nlimb), md));
      T.sdiags.emplace(kv.first, dst);
    }
    // a zero diagonal in every plan slot an entry does not use, so lt_bsgs can
    // run its slots without per-slot branches (the products with it add zero)
    {
      if (T.sdiags.empty()) throw std::runtime_error("linear transform has no diagonals loaded");
      const Poly& any = T.sdiags.begin()->second;
      Poly z = alloc(any.ncomp, any.nlimb, any.B);
      HIPCHK(hipMemsetAsync(z.ptr(), 0, (size_t)any.ncomp * any.nlimb * any.B * N * sizeof(u64), stream));
      T.sdiags.emplace(-1, z);
    }
    T.lay.plan = lt_blocks::plan({lt_pairs(T)}, 1, 1, LT_MAXB, LT_MAXG, LT_MAXSLOT);
    if (!T.lay.plan.error.empty())  // (worded for one transform)
      throw std::runtime_error(T.idx.empty() ? "linear transform without diagonals"
                                             : "linear transform with more than 64 baby steps");
    build_layout(T.lay, {&T});
    T.plan_dirty = false;
    ++T.rev;
  }
  // the device plans of every transform whose diagonals are all loaded (a
  // pipeline reads the scheme's transforms and never builds their plans)
  void build_dirty_plans() {
    for (int id : lts.live()) {
      LinTrans& T = lts.get(id);
      if (!T.plan_dirty || T.giants.empty()) continue;
      bool all = true;
      for (int d : T.idx) all = all && T.diags.count(d & (slots - 1));
      if (all) build_plan(T);
    }
  }

  // a transform can be evaluated: it has diagonals, all of them loaded
  void lt_loaded(const LinTrans& T) const {
    if (T.giants.empty()) throw std::runtime_error("linear transform without diagonals");
    for (int d : T.idx)
      if (!T.diags.count(d & (slots - 1)))
        throw std::runtime_error("linear transform diagonal " + std::to_string(d) +
                                 " is not loaded (io_mode load: call LoadPlaintextDiagonal first)");
  }

  // BSGS linear transform (lintrans MultiplyByDiagMatrixBSGS restated; oracle_lt_bsgs):
  // the transform's own layout, the 1 x 1 block, through eval_layout.
  // keep_qp: where moddown_rescale would apply, the final ModDown is left out
  // and the result holds the accumulator instead (Ciphertext::pend)
  Ciphertext eval_lt(LinTrans& T, const Ciphertext& ct, bool keep_qp = false) {
    lt_loaded(T);
    if (T.plan_dirty) build_plan(T);
    return eval_layout(T.lay, T, {&ct}, keep_qp);
  }
  // Steps 4 and 5 of eval_layout on the inner sums Tt of batch B: comps [0, ng) =
  // c0 of giant slot gi, [ng, 2 ng) = its c1; gorder: the giants' amounts, the
  // nonzero ones first, then 0 when there is one.  (A blocked transform's rows
  // are images of Tt.)
  Ciphertext lt_giant_steps(const Poly& Tt, const std::vector<int>& gorder, int level, int B, const LtRoute& r,
                            long double scale) {
    const int nqp = level + 1 + K, beta = (level + 1 + K - 1) / K;
    const int ng = (int)gorder.size();
    const bool has_g0 = gorder.back() == 0;
    const int nzg = ng - (has_g0 ? 1 : 0);
    // 4. giant key switches and the automorphism-accumulation (lt_giant)
    Poly acc = alloc(2, nqp, B);
    LimbSet la = lsqp(acc, 0, 2, level, level);
    const bool pend = r.end == KsEnd::KeepQP;
    Ciphertext out = pend ? pending_ct(level, B, scale) : new_ct(level, B, scale);
    const LimbSet lo = pend ? la : lsq(out.poly, 0, 2, level);
    // one lt_giant launch: it may store the P limbs through the final
    // ModDown INTT's rows pass (as keyswitch's gadget product does)
    const bool rows = r.fin.inv.rows_stored;
    LimbSet z = lsqp(Tt, ng - 1, 2, level, level);  // the zero giant: (c0, c1) at comps ng-1, 2ng-1
    z.comp_stride = (long long)ng * Tt.comp_stride();
    if (nzg > 0) {
      Poly T1q = alloc(nzg, level + 1, B);
      moddown(lsqp(Tt, ng, nzg, level, level), level, lsq(T1q, 0, nzg, level), r.giant_md);
      Poly Dg = decompose(lsq(T1q, 0, nzg, level), level, B, r.giant_dec);
      for (int g0 = 0; g0 < nzg; g0 += ORION_MAXGROUP) {
        LtGiants G;
        memset(&G, 0, sizeof(G));
        G.ng = std::min(ORION_MAXGROUP, nzg - g0);
        G.beta = beta;
        G.K = K;
        G.level = level;
        G.L = L;
        G.has_zero = (has_g0 && g0 == 0) ? 1 : 0;
        G.xcd = lt_xcd && (N / 256) % 8 == 0;
        G.rows_from = rows ? level + 1 : 0;
        G.logN = logN;
        G.d_gstride = (long long)beta * Dg.comp_stride();
        G.own_gstride = T1q.comp_stride();
        G.t0_gstride = Tt.comp_stride();
        for (int k = 0; k < G.ng; ++k) {
          const u64 g = galois_element(gorder[g0 + k]);
          const EvKey& kk = galois_key(g, level);
          G.key[k] = kk.k.ptr();
          G.klvl[k] = kk.level;
          G.idx[k] = aut_index(g);
        }
        LimbSet dg = lsqp(Dg, g0 * beta, 1, level, level);
        LimbSet own = lsq(T1q, g0, 1, level);
        LimbSet t0 = lsqp(Tt, g0, 1, level, level);
        LimbSet a = la;
        Poly part;
        if (g0 > 0) {  // > 64 giants: accumulate partial sums
          part = alloc(2, nqp, B);
          a = lsqp(part, 0, 2, level, level);
        }
        // per row: each giant's decomposition (beta) and t0 term, the output
        // pair and the zero giant; per QP limb: each giant's key (2 beta)
        const double rows = (double)nqp * B;
        Scope sc(this, P_LTGIANT, 8.0 * N * (rows * (G.ng * (beta + 1.0) + 2.0 + 2.0 * G.has_zero) +
                                          (double)nqp * 2.0 * beta * G.ng));
        if (orion_launch_lt_giant(a, dg, own, t0, z, G, d_tb, N, stream))
          throw std::runtime_error("lt_giant launch failed");
        if (g0 > 0) ew(EW_ADD, la, la, a);
      }
    } else {
      copy(la, z);
    }
    // 5.
    if (pend)
      out.pend = acc;
    else
      moddown(la, level, lo, r.fin);
    return out;
  }

  // the (giant, baby) amounts of a transform's diagonals, in the order of its index list
  std::vector<lt_blocks::Pair> lt_pairs(const LinTrans& T) const {
    std::vector<lt_blocks::Pair> v;
    for (int d : T.idx) {
      const int rot = d & (slots - 1);
      v.push_back({((rot / T.N1) * T.N1) & (slots - 1), rot & (T.N1 - 1)});
    }
    return v;
  }
  // device plans of a layout (lt_blocks.h) from the members' plan copies of
  // their diagonals; Ts: the members, row-major, their copies made
  void build_layout(LtLayout& Ly, const std::vector<LinTrans*>& Ts) {
    const lt_blocks::Plan& P = Ly.plan;
    std::vector<LtPlan> plans(P.total_chunks);
    memset(plans.data(), 0, plans.size() * sizeof(LtPlan));
    const u64* zero = Ts[0]->sdiags.at(-1).ptr();
    for (auto& pl : plans)
      for (int e = 0; e < LT_MAXG; ++e)
        for (int sl = 0; sl < LT_MAXSLOT; ++sl) pl.pt[e][sl] = zero;
    Ly.first_chunk.clear();
    int chunk = 0;
    for (int j = 0; j < P.cols; ++j) {
      const lt_blocks::Column& col = P.columns[j];
      Ly.first_chunk.push_back(chunk);
      for (size_t k = 0; k < col.entries.size(); ++k) {
        const lt_blocks::Entry& en = col.entries[k];
        LtPlan& pl = plans[chunk + k / LT_MAXG];
        const int e = (int)(k % LT_MAXG);
        const LinTrans& T = *Ts[(size_t)en.row * P.cols + j];
        pl.mask[e] = en.mask;
        pl.comp[e] = en.gslot, pl.row[e] = en.row, pl.acc[e] = en.acc;
        for (size_t sl = 0; sl < en.diag.size(); ++sl)
          if (en.diag[sl] >= 0) pl.pt[e][sl] = T.sdiags.at(T.idx[en.diag[sl]] & (slots - 1)).ptr();
      }
      chunk += col.chunks;
    }
    // a plan that a captured graph still holds is never rewritten: the graph
    // keeps replaying the plan (and the diagonals) it was captured with
    if (!Ly.dev || Ly.dev.use_count() > 1) {
      void* d = nullptr;
      HIPCHK(hipMalloc(&d, plans.size() * sizeof(LtPlan)));
      Ly.dev = std::shared_ptr<void>(d, [](void* q) { hipFree(q); });
      Ly.d_plan = (LtPlan*)d;
    }
    h2d(Ly.d_plan, plans.data(), plans.size() * sizeof(LtPlan));
  }
  // ... of a blocked transform; Ts: the members, plans built
  void build_blocks_plan(LtBlocks& Bk, const std::vector<LinTrans*>& Ts) {
    no_capture("building a blocked linear transform's plan");
    build_layout(Bk.lay, Ts);
    Bk.revs.clear();
    for (const LinTrans* T : Ts) Bk.revs.push_back(T->rev);
    Bk.built = true;
  }

  // BSGS linear transform of a layout (lt_blocks.h): all rows' sum_j T[i][j](ct[j])
  // as one batch, image i * B + b = row i.  Every phase runs as one grouped
  // launch over all babies / all giants:
  //   1. per column one hoisted decomposition of ct1;
  //   2. all baby key switches (one MAC, decomposition shared) and their
  //      automorphisms with the + P*ct0 term (one launch);
  //   3. all giant inner products sum_s pt * rot_s (lt_bsgs: each baby read
  //      once and shared by every row), those of equal giant amount added
  //      across the columns in the QP basis;
  //   4. all giant key switches: ModDown of c1, decomposition, MAC with each
  //      giant's key (+ c0 folded in), then the automorphism-accumulate;
  //   5. ModDown of the accumulator.
  // T0: the first member (the level, and a diagonal for the limb layout); cs:
  // the cols inputs, one level, scale and batch.  keep_qp: where
  // moddown_rescale would apply, step 5 is left out and the result holds the
  // accumulator instead (Ciphertext::pend)
  Ciphertext eval_layout(const LtLayout& Ly, const LinTrans& T0, const std::vector<const Ciphertext*>& cs,
                         bool keep_qp) {
    const lt_blocks::Plan& P = Ly.plan;
    const int level = std::min(cs[0]->level, T0.level);
    const int B = cs[0]->poly.B, RB = P.rows * B, nqp = level + 1 + K;
    const int beta = (level + 1 + K - 1) / K;
    const int ng = (int)P.giants.size();
    const LtRoute r = lt_route(env, tun, RB, level, P.nonzero_giants, keep_qp);
    const DecomposeRoute hoist = decompose_route(env, tun, 1, B, level);
    const std::vector<u64> pq = p_mod_q(level);
    // every key is looked up before anything is queued (galois_key throws)
    for (int g : P.giants)
      if (g) galois_key(galois_element(g), level);
    for (const auto& col : P.columns)
      for (int b : col.babies)
        if (b) galois_key(galois_element(b), level);

    // inner sums: comps [0, ng) = c0 of giant slot gs, [ng, 2 ng) = its c1
    Poly Tt = alloc(2 * ng, nqp, RB);
    const LimbSet t0 = lsqp(Tt, 0, 1, level, level), t1 = lsqp(Tt, ng, 1, level, level);
    // (every plane of Tt is written: a row without diagonals for one of the
    // layer's giants has an entry with an empty mask in column 0's plan)
    const Poly& pt0 = T0.diags.begin()->second.poly;
    const LimbSet ptl = lsqp(pt0, 0, 1, level, T0.level, 1);
    for (int j = 0; j < P.cols; ++j) {
      const lt_blocks::Column& col = P.columns[j];
      const Ciphertext& ct = *cs[j];
      const int nb = (int)col.babies.size();
      // one hoisted decomposition of the column's ct1 (when some baby rotates)
      Poly D = col.rotating > 0 ? decompose(lsq(ct.poly, 1, 1, level), level, B, hoist) : alloc(1, 1, 1);
      LimbSet dl = lsqp(D, 0, 1, level, level);
      if (col.rotating == 0) dl.p = nullptr;
      const LimbSet ctl = lsq(ct.poly, 0, 2, level);
      for (int pass = 0; pass < col.passes; ++pass) {
        const int s0 = pass * LT_MAXB;
        LtBabies Bb;
        memset(&Bb, 0, sizeof(Bb));
        Bb.nb = std::min(LT_MAXB, nb - s0);
        Bb.s0 = s0;
        Bb.xcd = lt_xcd && (N / 256) % 8 == 0;
        Bb.beta = beta;
        Bb.K = K;
        Bb.level = level;
        Bb.L = L;
        for (int l = 0; l <= level; ++l) Bb.pq[l] = pq[l], Bb.pqs[l] = hm_shoup(pq[l], mods[l]);
        int nrot = 0;
        for (int s = 0; s < Bb.nb; ++s) {
          const int b = col.babies[s0 + s];
          if (b == 0) continue;
          const u64 g = galois_element(b);
          const EvKey& kk = galois_key(g, level);
          Bb.key[s] = kk.k.ptr();
          Bb.klvl[s] = kk.level;
          Bb.idx[s] = aut_index(g);
          ++nrot;
        }
        for (int k = 0; k < col.chunks; ++k) {
          const int e0 = lt_blocks::Plan::chunk_first(k, LT_MAXG), ne = lt_blocks::Plan::chunk_count(col, k, LT_MAXG);
          // distinct bytes: the column's decomposition (beta digits) and ct0/ct1
          // once per row of the launch, each entry's output pair (read back when
          // it accumulates), and per QP limb the baby keys (2 beta each) and the
          // entries' diagonals, both shared by the batch
          const double lrows = (double)nqp * B;
          int npair = 0, nacc = 0;
          for (int e = e0; e < e0 + ne; ++e) {
            const lt_blocks::Entry& en = col.entries[e];
            for (int s = 0; s < Bb.nb; ++s) npair += (int)((en.mask >> (s0 + s)) & 1ull);
            nacc += (s0 > 0 || en.acc) ? 1 : 0;
          }
          Scope sc(this, P_LTMAC, 8.0 * N * (lrows * ((col.rotating ? beta : 0) + 2.0 + 2.0 * (ne + nacc)) +
                                             (double)nqp * (2.0 * beta * nrot + npair)));
          if (orion_launch_lt_bsgs(t0, t1, dl, ctl, Bb, Ly.d_plan + Ly.first_chunk[j], k, ne, s0 > 0,
                                   P.rows * P.cols == 1, ptl, d_tb, N, B, stream))
            throw std::runtime_error("lt_bsgs launch failed");
        }
      }
    }
    return lt_giant_steps(Tt, P.giants, level, RB, r, cs[0]->scale * (long double)mods[T0.level]);
  }

  // Blocked BSGS linear transform: out[i] = sum_j T[i][j](ct[j]), hoisted across
  // rows and columns (eval_layout), then the rows cut from the batch.  Ts: the
  // members (plans built).  rescale: the ModDown and the rescale as one division
  // where moddown_rescale applies, the sequence elsewhere (the same bits).
  std::vector<Ciphertext> eval_lt_blocks(const LtBlocks& Bk, const std::vector<LinTrans*>& Ts,
                                         const std::vector<const Ciphertext*>& cs, bool rescale) {
    if (rescale && std::min(cs[0]->level, Bk.level) < 1) throw std::runtime_error("cannot rescale a level-0 ciphertext");
    const int B = cs[0]->poly.B;
    Ciphertext all = eval_layout(Bk.lay, *Ts[0], cs, rescale);
    if (all.pend.buf)
      finish_moddown_rescale(all);
    else if (rescale)
      rescale_inplace(all);
    std::vector<Ciphertext> out;
    for (int i = 0; i < Bk.rows; ++i) {
      std::vector<GatherSrc> src;
      gather_sources(all, i * B, B, src);
      Ciphertext o = new_ct(all.level, B, all.scale);
      gather(o, src);
      out.push_back(std::move(o));
    }
    return out;
  }

  // ---------------------------------------------------------------------------
  // encoder / encryptor
  // ---------------------------------------------------------------------------
  // values: B images x nvals float32 slots, device memory (encoder.hip);
  // limbs Q 0..level (+ P when qp)
  Plaintext encode_dev(const float* dvals, int nvals, int B, int level, long double scale, bool qp) {
    const int n = slots;
    if (nvals > n) throw std::runtime_error("too many values for the slot count");
    std::vector<int> md = iota(0, level + 1);
    if (qp)
      for (int k = 0; k < K; ++k) md.push_back(L + k);
    const int nl = (int)md.size();
    Plaintext pt;
    pt.level = level;
    pt.scale = scale;
    pt.qp = qp;
    pt.poly = alloc(1, nl, B);
    Buffer v(&pool, (size_t)B * n * sizeof(double2));
    const LimbSet out = ls(pt.poly, 0, 1, iota(0, nl), md);
    if (orion_launch_encode(dvals, nvals, B, (double2*)v.p, tw_inv, ci ? logN : logN - 1, ci, out, (double)scale,
                            d_tb, stream))
      throw std::runtime_error("encode launch failed");
    ntt(out, false);
    return pt;
  }
  Plaintext encode(const float* values, int nvals, int B, int level, long double scale, bool qp) {
    if (nvals > slots) throw std::runtime_error("too many values for the slot count");
    Buffer dv(&pool, (size_t)B * nvals * sizeof(float) + 16);
    HIPCHK(hipMemcpyAsync(dv.p, values, (size_t)B * nvals * sizeof(float), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return encode_dev((const float*)dv.p, nvals, B, level, scale, qp);
  }

  // Garner table of `level`: inv[j][k] = (q_k mod q_j)^-1 mod q_j, then the
  // mixed-radix digits of floor((Q - 1) / 2)
  const u64* garner_table(int level) {
    auto it = garner.find(level);
    if (it != garner.end()) return it->second;
    no_capture("a decode CRT table");
    const int nl = level + 1;
    std::vector<u64> t((size_t)nl * nl + nl, 0);
    for (int j = 0; j < nl; ++j)
      for (int k = 0; k < j; ++k) t[(size_t)j * nl + k] = hm_invmod(mods[k] % mods[j], mods[j]);
    u64 rem = 0;
    for (int j = nl - 1; j >= 0; --j) {
      const u128 cur = (u128)rem * mods[j] + (mods[j] - 1);
      t[(size_t)nl * nl + j] = (u64)(cur / 2);
      rem = (u64)(cur % 2);
    }
    u64* d;
    HIPCHK(hipMalloc(&d, t.size() * sizeof(u64)));
    h2d(d, t.data(), t.size() * sizeof(u64));
    garner[level] = d;
    return d;
  }
  // slots (real parts) of every image into device memory out[B][slots]
  void decode_dev(const Plaintext& pt, double* out) {
    const int level = pt.level, B = pt.poly.B, nl = level + 1;
    if (nl > ORION_MAXLIMB) throw std::runtime_error("decode: too many limbs");
    Poly t = alloc(1, nl, B);
    const LimbSet x = lsq(t, 0, 1, level);
    ntt_io(nio(x, lsq(pt.poly, 0, 1, level)), true);
    Buffer v(&pool, (size_t)B * slots * sizeof(double2));
    if (orion_launch_decode(x, garner_table(level), (double)pt.scale, ci ? logN : logN - 1, ci, (double2*)v.p, tw_fwd,
                            out, d_tb, stream))
      throw std::runtime_error("decode launch failed");
  }
  std::vector<double> decode(const Plaintext& pt) {
    const size_t cnt = (size_t)pt.poly.B * slots;
    Buffer d(&pool, cnt * sizeof(double));
    decode_dev(pt, (double*)d.p);
    std::vector<double> out(cnt);
    HIPCHK(hipMemcpyAsync(out.data(), d.p, cnt * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return out;
  }

  // public-key encryption (Lattigo rlwe Encryptor.EncryptZero + pt):
  // c0 = u pk0 + e0 + m, c1 = u pk1 + e1; u, e0, e1 sampled on the GPU
  Ciphertext encrypt(const Plaintext& pt) {
    if (!have_pk) throw std::runtime_error("public key not generated");
    const int level = pt.level, B = pt.poly.B;
    Poly r = alloc(3, level + 1, B);
    const LimbSet rs = lsq(r, 0, 3, level);
    if (orion_launch_enc_sample(rs, enc_sampler, d_tb, N, stream)) throw std::runtime_error("sampler launch failed");
    enc_sampler.enc += 1;
    ntt(rs, false);
    Ciphertext ct = new_ct(level, B, pt.scale);
    LimbSet c0 = lsq(ct.poly, 0, 1, level), c1 = lsq(ct.poly, 1, 1, level);
    ew(EW_MUL, c0, lsq(r, 0, 1, level), lsq(pk, 0, 1, level, B));
    ew(EW_ADD, c0, c0, lsq(r, 1, 1, level));
    ew(EW_ADD, c0, c0, lsq(pt.poly, 0, 1, level, B));
    ew(EW_MUL, c1, lsq(r, 0, 1, level), lsq(pk, 1, 1, level, B));
    ew(EW_ADD, c1, c1, lsq(r, 2, 1, level));
    return ct;
  }

  Plaintext decrypt(const Ciphertext& ct) {
    if (!have_sk) throw std::runtime_error("secret key not generated");
    const int level = ct.level, B = ct.poly.B;
    Plaintext pt;
    pt.level = level;
    pt.scale = ct.scale;
    pt.poly = alloc(1, level + 1, B);
    LimbSet p = lsq(pt.poly, 0, 1, level);
    ew(EW_MUL, p, lsq(ct.poly, 1, 1, level), lsq(sk, 0, 1, level, B));
    ew(EW_ADD, p, p, lsq(ct.poly, 0, 1, level));
    return pt;
  }

  // rounded integer constant c -> residues at `level`
  std::vector<u64> const_residues(long double c, int level) const {
    std::vector<u64> r;
    const bool neg = c < 0;
    long double a = neg ? -c : c;
    // a < 2^64 required
    if (a >= 18446744073709551615.0L) throw std::runtime_error("scalar constant too large");
    const u64 v = (u64)a;
    for (int j = 0; j <= level; ++j) {
      const u64 x = v % mods[j];
      r.push_back(neg ? (x ? mods[j] - x : 0) : x);
    }
    return r;
  }
  // round(c) (half away from zero) of any magnitude -> residues at `level`;
  // |c| >= 2^63 is an integer m 2^e (64-bit long double mantissa), reduced exactly
  std::vector<u64> big_const_residues(long double c, int level) const {
    const bool neg = c < 0;
    long double a = floorl((neg ? -c : c) + 0.5L);
    u64 m;
    int e = 0;
    if (a >= 9223372036854775808.0L) {
      int ex;
      const long double fr = frexpl(a, &ex);
      m = (u64)ldexpl(fr, 64);
      e = ex - 64;
    } else {
      m = (u64)a;
    }
    std::vector<u64> r;
    for (int j = 0; j <= level; ++j) {
      const u64 q = mods[j];
      const u64 x = hm_mulmod(m % q, hm_powmod(2 % q, (u64)e, q), q);
      r.push_back(neg ? (x ? q - x : 0) : x);
    }
    return r;
  }
  // round(v * s) (half away from zero), formed exactly, -> residues at `level`
  // (AddScalar's v * scale, MulScalarFloat's v * q_level; Lattigo forms both in
  // arbitrary precision).  v = mv 2^ev with mv < 2^24 and s = ms 2^es with
  // ms < 2^64 (a prime below 2^61 or a long double scale), so the product's
  // mantissa fits 128 bits: the rounding is an integer shift, and a product of
  // 2^64 or more is reduced per limb as mant 2^e
  std::vector<u64> scaled_const_residues(float v, long double s, int level) const {
    if (!std::isfinite(v) || !std::isfinite(s) || s <= 0) throw std::runtime_error("scalar constant is not finite");
    const bool neg = std::signbit(v);
    int ev, es;
    const u64 mv = (u64)ldexpf(frexpf(fabsf(v), &ev), 24);
    const u64 ms = (u64)ldexpl(frexpl(s, &es), 64);
    unsigned __int128 m = (unsigned __int128)mv * ms;
    int e = (ev - 24) + (es - 64);
    if (e < 0) {
      // m < 2^88: shifted by 89 or more it is below one half
      m = -e > 88 ? 0 : ((m >> (-e - 1)) + 1) >> 1;
      e = 0;
    }
    std::vector<u64> r;
    for (int j = 0; j <= level; ++j) {
      const u64 q = mods[j];
      const u64 x = hm_mulmod((u64)(m % q), hm_powmod(2 % q, (u64)e, q), q);
      r.push_back(neg && x ? q - x : x);
    }
    return r;
  }

  // ---------------------------------------------------------------------------
  // polynomial evaluation (polyeval.go:63-84 -> Lattigo v6 he.EvaluatePolynomial,
  // restated): p(x) in the monomial or Chebyshev basis, consuming exactly
  // bitlen(degree) levels (orion/nn/activation.py:22-23,106-107 plans for that)
  // and returning exactly the requested scale.
  //   * power basis (PowerBasis.GenPower): T_{2s} = T_s^2 (Chebyshev
  //     2 T_s^2 - 1); baby steps T_j from a = 2^k - 1, b = j + 1 - 2^k
  //     (Chebyshev 2 T_a T_b - T_|a-b|, T_c scaled by round(s_a s_b / s_c)
  //     before the rescale); every stored power is rescaled once.  Babies are
  //     made on first use (Lattigo makes all j < 2^logSplit up front; the
  //     values are the same);
  //   * Paterson-Stockmeyer tree (GetPatersonStockmeyerPolynomial /
  //     recursePS): logSplit = OptimalSplit(bitlen(deg)), top target level
  //     level(x) - bitlen(deg) + 1.  A node of degree < 2^logSplit is a leaf,
  //     except that a lead node (the chain of quotients from the top) whose
  //     MaxDeg > 2^bitlen(MaxDeg) - 2^(logSplit-1) is re-split with
  //     logSplit = OptimalSplit(bitlen(deg)), passed down to its subtree.
  //     Otherwise p = q X^m + r, m = the smallest power of two >= 2^logSplit
  //     and >= deg/2 + 1 (Chebyshev: T_{m+j} = 2 T_m T_j - T_{m-j});
  //   * scales (ckks simEvaluator.UpdateLevelAndScale{Baby,Giant}Step): the q
  //     branch runs one level up at scale S q_i / scale(X^m), q_i = q_level
  //     for a lead node and q_{level+1} otherwise; its result is rescaled and
  //     multiplied by X^m, and the r branch runs at that product's scale; a
  //     lead leaf is evaluated at S q_level.  The top result is rescaled once,
  //     landing on the target scale;
  //   * a leaf (EvaluatePolynomialVectorFromPowerBasis) is c_0 S + sum_j
  //     round(c_j S / scale(T_j)) T_j (MulThenAdd: half away from zero), at
  //     the lowest level among its target and the powers it uses, as
  //     MulThenAdd and Add take the lower level of their operands.
  // ---------------------------------------------------------------------------
  struct PolyFn {
    bool cheb = false;
    std::vector<long double> c;  // lowest degree first
  };
  struct PolyRun {
    const Ciphertext* x;
    bool cheb;
    std::map<int, Ciphertext> pw;    // T_{2^k}, k >= 1
    std::map<int, Ciphertext> baby;  // T_j, j not a power of two
  };
  static int ceil_log2(int j) {
    int k = 0;
    while ((1 << k) < j) ++k;
    return k;
  }
  static int optimal_split(int logd) {  // Lattigo bignum.OptimalSplit
    int ls = logd >> 1;
    const int a = (1 << ls) + (1 << (logd - ls)) + logd - ls - 3;
    const int b = (1 << (ls + 1)) + (1 << (logd - ls - 1)) + logd - ls - 4;
    if (a > b) ++ls;
    return ls;
  }
  // t <- 2 t + round(c): the Chebyshev doubling T_2j = 2 T_j^2 - 1 and
  // EvalMod's double angle, c at t's scale (added to component 0)
  void double_add_const(Ciphertext& t, long double c) {
    const LimbSet lt = lsq(t.poly, 0, 2, t.level), l0 = lsq(t.poly, 0, 1, t.level);
    ew(EW_ADD, lt, lt, lt);
    const std::vector<u64> k = big_const_residues(c, t.level);
    ew1(EW_ADDC, l0, l0, &k);
  }
  const Ciphertext& poly_T(PolyRun& R, int j) {
    if (j == 1) return *R.x;
    if ((j & (j - 1)) == 0) return R.pw.at(j);
    auto it = R.baby.find(j);
    if (it != R.baby.end()) return it->second;
    const int k = ceil_log2(j) - 1, a = (1 << k) - 1, b = j + 1 - (1 << k), c = a > b ? a - b : b - a;
    const Ciphertext& A = poly_T(R, a);
    const Ciphertext& Bc = poly_T(R, b);
    Ciphertext t = mul_relin(A, Bc);
    if (R.cheb && c == 0) {
      double_add_const(t, -t.scale);
    } else if (R.cheb) {
      const LimbSet lt = lsq(t.poly, 0, 2, t.level);
      ew(EW_ADD, lt, lt, lt);
      const Ciphertext& C = poly_T(R, c);
      std::vector<u64> k = big_const_residues(-(t.scale / C.scale), t.level);
      ew(EW_ADDSCALE, lt, lsq(C.poly, 0, 2, t.level), lt, &k);
    }
    rescale_inplace(t);
    return R.baby.emplace(j, std::move(t)).first->second;
  }
  static std::pair<std::vector<long double>, std::vector<long double>> poly_split(const std::vector<long double>& c,
                                                                                  int s, bool cheb) {
    const int deg = (int)c.size() - 1;
    std::vector<long double> q(c.begin() + s, c.end()), r(c.begin(), c.begin() + s);
    if (cheb) {
      for (int j = 1; j <= deg - s; ++j) {
        q[j] = 2 * c[s + j];
        r[s - j] -= c[s + j];
      }
    }
    return {q, r};
  }
  // leaf: c_0 S + sum_j round(c_j S / scale(T_j)) T_j at level min(lam, level(T_j))
  Ciphertext poly_leaf(PolyRun& R, const std::vector<long double>& c, int lam, long double S) {
    const int deg = (int)c.size() - 1, B = R.x->poly.B;
    int lv = lam;
    for (int j = 1; j <= deg; ++j)
      if (c[j] != 0) lv = std::min(lv, poly_T(R, j).level);
    Ciphertext o = new_ct(lv, B, S);
    const LimbSet lo = lsq(o.poly, 0, 2, lv);
    bool first = true;
    for (int j = 1; j <= deg; ++j) {
      if (c[j] == 0) continue;
      const Ciphertext& T = poly_T(R, j);
      std::vector<u64> k = big_const_residues(c[j] * S / T.scale, lv);
      ew1(first ? EW_SCALE : EW_ADDSCALE, lo, lsq(T.poly, 0, 2, lv), &k);
      first = false;
    }
    if (first) HIPCHK(hipMemsetAsync(o.poly.ptr(), 0, (size_t)2 * (lv + 1) * B * N * sizeof(u64), stream));
    if (c[0] != 0) {
      std::vector<u64> k = big_const_residues(c[0] * S, lv);
      ew1(EW_ADDC, lsq(o.poly, 0, 1, lv), lsq(o.poly, 0, 1, lv), &k);
    }
    return o;
  }
  static int bitlen(int v) {
    int k = 0;
    while (v >> k) ++k;
    return k;
  }
  // recursePS: node c (lead: on the quotient chain from the top; maxdeg as
  // splitCoeffs propagates it) evaluated for target level lam and scale S
  Ciphertext poly_ps(PolyRun& R, const std::vector<long double>& c, bool lead, int maxdeg, int logSplit, int lam,
                     long double S) {
    const int deg = (int)c.size() - 1;
    if (deg < (1 << logSplit)) {
      if (lead && logSplit > 1 && maxdeg > (1 << bitlen(maxdeg)) - (1 << (logSplit - 1)))
        return poly_ps(R, c, lead, maxdeg, optimal_split(bitlen(deg)), lam, S);
      return poly_leaf(R, c, lam, lead ? S * (long double)mods[lam] : S);
    }
    int m = 1 << logSplit;
    while (m < (deg >> 1) + 1) m <<= 1;
    auto qr = poly_split(c, m, R.cheb);
    const int rmax = maxdeg == deg ? m - 1 : maxdeg - (deg - m + 1);
    const Ciphertext& X = R.pw.at(m);
    if (lam + 1 > R.x->level) throw std::runtime_error("polynomial evaluation: level plan violated");
    const long double qi = (long double)mods[lead ? lam : lam + 1];
    Ciphertext qc = poly_ps(R, qr.first, lead, maxdeg, logSplit, lam + 1, S * qi / X.scale);
    rescale_inplace(qc);
    Ciphertext o = mul_relin(qc, X);
    Ciphertext rc = poly_ps(R, qr.second, false, rmax, logSplit, lam, o.scale);
    const int lv = std::min(o.level, rc.level);  // Add takes the lower level
    o.level = lv;
    const LimbSet lo = lsq(o.poly, 0, 2, lv);
    ew(EW_ADD, lo, lo, lsq(rc.poly, 0, 2, lv));
    return o;
  }
  Ciphertext eval_poly(const Ciphertext& x, const PolyFn& p, long double target) {
    const int deg = (int)p.c.size() - 1;
    if (deg < 0) throw std::runtime_error("empty polynomial");
    const int depth = bitlen(deg);  // bits.Len64(degree)
    if (x.level < depth)
      throw std::runtime_error(std::to_string(x.level) + " levels < " + std::to_string(depth) +
                               " log(d) -> cannot evaluate poly");
    PolyRun R;
    R.x = &x;
    R.cheb = p.cheb;
    for (int s = 1; 2 * s <= deg; s *= 2) {
      const Ciphertext& a = s == 1 ? x : R.pw.at(s);
      Ciphertext t = mul_relin(a, a);
      rescale_inplace(t);
      if (p.cheb) double_add_const(t, -t.scale);
      R.pw.emplace(2 * s, std::move(t));
    }
    if (deg == 0) return poly_leaf(R, p.c, x.level, target);
    Ciphertext out = poly_ps(R, p.c, true, deg, optimal_split(depth), x.level - depth + 1, target);
    rescale_inplace(out);
    out.scale = target;
    return out;
  }
  HandlePool<PolyFn> polys;

  // ---------------------------------------------------------------------------
  // bootstrapping (bootstrapper.go:15-87).  As in Lattigo, a
  // bootstrapper is made per slot count (NewBootstrapper(logPs, slots)), and
  // its circuit runs under bootstrapping parameters of its own.  Orion sets
  // only LogN, LogP, Xs and LogSlots (bootstrapper.go:33-38); every other
  // field is Lattigo v6's default bootstrapping.ParametersLiteral [U]
  // (DESIGN.md §6 lists each default beside what is done here):
  //   CoeffsToSlots 4 levels of 56-bit primes, SlotsToCoeffs 3 levels of
  //   39-bit primes, EvalMod 60-bit primes, K = 16, Mod1 degree 30, 3 double
  //   angles, no arcsine (Mod1InvDegree 0), LogMessageRatio 8, an ephemeral
  //   secret of Hamming weight 32.
  // The chain is the residual Q chain + 3 x 39 + (bitlen(30) + 3) x 60 + 4 x
  // 56 bits, with key-switching P primes of the bit sizes logPs.  Those
  // parameters live in a second Context -- the bootstrapping context, one per
  // distinct logPs, shared by the slot counts -- that holds the same secret
  // and its own relinearisation and Galois keys; the scheme's context, chain
  // and keys are not touched.  The circuit, for n slots (gap = N / 2n), with
  // every constant derived from the parameters (oracle_bootstrap derives
  // them again, independently):
  //   ScaleDown: the level-0 residues times F = round(q0 / (2^8 Delta)), so
  //      the message sits 2^LogMessageRatio below q0
  //   -> EvkDenseToSparse at level 0 (key switch s -> s_eph, h(s_eph) = 32)
  //   -> ModRaise (level 0 -> top of the bootstrapping chain, t = m + q0 I
  //      with |I| small because s_eph is sparse)
  //   -> EvkSparseToDense at the top level (s_eph -> s)
  //   -> Trace, n < N/2 only: multiply by gap^-1 mod Q, then add the
  //      log2(gap) rotations by n 2^i (SubSum): the exact projection on
  //      Z[X^gap], whose slots are the n-periodic average of the input's
  //   -> CoeffsToSlots: the n-point special inverse FFT's butterfly stages
  //      merged into 4 BSGS transforms with complex diagonals (n-periodic; the
  //      extra stages go to the first transforms); the final bit reversal is
  //      skipped because EvalMod is slot-wise and SlotsToCoeffs starts with
  //      the matching one.  The 1/n and EvalMod's 1/(2K) are spread over the
  //      transforms.  For n < N/2 the last transform also packs: real parts
  //      into slots [0, n) and imaginary parts into [n, 2n) of every
  //      2n-period, so that one EvalMod serves both
  //   -> EvalMod: the degree-30 Chebyshev interpolant of
  //      a cos(2 pi (K u - 1/4) / 2^r) on [-1, 1], a = (2 pi)^(-1/2^r), at a
  //      target scale chosen so that after the r double angles
  //      y <- 2 y^2 - a^(2^(i+1)) (constant added before the rescale, as
  //      Lattigo's mod1 evaluator does) the scale is 2^60; the result is
  //      sin(2 pi x) / (2 pi) = F m / q0 + O(m^3); once (n < N/2) or on the
  //      real and the imaginary part (n = N/2, recombined with x i = X^(N/2))
  //   -> SlotsToCoeffs: the forward stages, 3 transforms carrying
  //      q0 / (F s_y) (for n < N/2 the first one also unpacks real + i imag)
  //      -> the residual top level, copied back into the scheme's context at
  //      the input's scale.
  // Bootstrap then applies Orion's post-scale 2^(LogMaxSlots - LogSlots)
  // (bootstrapper.go:73-74): an input whose slots >= n are zero comes back with
  // its n slots replicated over all N/2 (Lattigo's sparse packing).
  // ---------------------------------------------------------------------------
  typedef std::complex<double> cplx;
  typedef std::map<int, std::vector<cplx>> DiagMap;  // rotation offset -> diagonal (n slots)

  Plaintext encode_complex(const std::vector<cplx>& v, int level, long double scale, bool qp) {
    const int n = N / 2;
    std::vector<int> md = iota(0, level + 1);
    if (qp)
      for (int k = 0; k < K; ++k) md.push_back(L + k);
    const int nl = (int)md.size();
    Plaintext pt;
    pt.level = level;
    pt.scale = scale;
    pt.qp = qp;
    pt.poly = alloc(1, nl, 1);
    std::vector<double2> host(n);
    for (int i = 0; i < n; ++i) host[i] = make_double2(v[i].real(), v[i].imag());
    Buffer dv(&pool, (size_t)n * sizeof(double2));
    HIPCHK(hipMemcpyAsync(dv.p, host.data(), host.size() * sizeof(double2), hipMemcpyHostToDevice, stream));
    const LimbSet out = ls(pt.poly, 0, 1, iota(0, nl), md);
    if (orion_launch_encode_c((double2*)dv.p, 1, tw_inv, logN - 1, false, out, (double)scale, d_tb, stream))
      throw std::runtime_error("encode launch failed");
    HIPCHK(hipStreamSynchronize(stream));
    ntt(out, false);
    return pt;
  }
  // BSGS transform y = sum_d diag_d * rot(x, d) with complex diagonals encoded
  // at scale q_level; the bootstrapping DFT matrices' LogBSGSRatio is 1 [U]
  LinTrans make_lt_complex(const DiagMap& dm, int level) {
    const int slots = N / 2;
    LinTrans T;
    T.level = level;
    T.ratio = 2;
    for (auto& kv : dm) T.idx.push_back(kv.first);
    const std::vector<int> giant_of = lt_bsgs_index(T, slots, 1);
    std::vector<cplx> vec(slots);
    size_t k = 0;
    for (auto& kv : dm) {
      const int gi = giant_of[k++];
      for (int s2 = 0; s2 < slots; ++s2) vec[s2] = kv.second[((s2 - gi) % slots + slots) % slots];
      T.diags[kv.first & (slots - 1)] = encode_complex(vec, level, (long double)mods[level], true);
    }
    return T;
  }
  // one butterfly stage of the special FFT as a diagonal map (offsets mod n)
  DiagMap fft_stage(int len, bool inverse, const std::vector<Cplx>& tw) const {
    const int n = N / 2, h = len / 2;
    DiagMap m;
    auto at = [&](int off) -> std::vector<cplx>& {
      auto it = m.find(off);
      if (it == m.end()) it = m.emplace(off, std::vector<cplx>(n, cplx(0, 0))).first;
      return it->second;
    };
    std::vector<cplx>&d0 = at(0), &dp = at(h), &dm = at(n - h);
    for (int p = 0; p < n; ++p) {
      const int j = p & (len - 1);
      if (j < h) {
        const cplx w = inverse ? cplx(1, 0) : cplx(tw[h + j].re, tw[h + j].im);
        d0[p] += 1.0;
        dp[p] += w;  // x_{p+h}
      } else {
        const cplx w(tw[h + j - h].re, tw[h + j - h].im);
        if (inverse) {  // (x_{p-h} - x_p) w
          dm[p] += w;
          d0[p] -= w;
        } else {  // x_{p-h} - w x_p
          dm[p] += 1.0;
          d0[p] -= w;
        }
      }
    }
    return m;
  }
  // (A o B): apply B, then A
  DiagMap diag_compose(const DiagMap& A, const DiagMap& Bm) const {
    const int n = N / 2;
    DiagMap C;
    for (auto& a : A)
      for (auto& b : Bm) {
        const int off = (a.first + b.first) % n;
        auto it = C.find(off);
        if (it == C.end()) it = C.emplace(off, std::vector<cplx>(n, cplx(0, 0))).first;
        for (int p = 0; p < n; ++p) it->second[p] += a.second[p] * b.second[(p + a.first) % n];
      }
    return C;
  }
  // one evaluation key of a bootstrapping circuit: the key a circuit needs
  // (level = the highest level it is used at) or a key held (level = the level
  // it was made for; k = its words)
  enum { BK_RELIN = 1, BK_D2S = 2, BK_S2D = 3, BK_GALOIS = 4 };
  struct KeyNeed {
    int kind = 0;
    u64 gel = 0;  // BK_GALOIS: the Galois element
    int level = 0;
    const Poly* k = nullptr;
  };
  static const char* key_kind_name(int kind) {
    return kind == BK_RELIN ? "relin" : kind == BK_D2S ? "d2s" : kind == BK_S2D ? "s2d" : "galois";
  }
  struct Bootstrapper {
    // Lattigo v6 bootstrapping.ParametersLiteral defaults [U]:
    // CoeffsToSlots / SlotsToCoeffs factorisation depths and prime sizes,
    // EvalMod prime size, Mod1 degree, double angles, K, LogMessageRatio and
    // the ephemeral secret's Hamming weight
    static constexpr int kCtS = 4, kCtSBits = 56, kStC = 3, kStCBits = 39, kModBits = 60;
    static constexpr int kDegree = 30, kR = 3, kK = 16, kLogMsgRatio = 8, kEphH = 32;
    static constexpr int kDepthPoly = 5;  // bits.Len64(kDegree)
    static constexpr int kLogBSGSRatio = 1;  // dft.MatrixLiteral LogBSGSRatio
    static_assert(kCtS == 4 && kStC == 3, "the constant spreading below takes 4th and cube roots");
    Context* bc = nullptr;  // the bootstrapping context (owned by the scheme's btp_ctx)
    int slots = 0, gap = 1, K = kK, r = kR, degree = kDegree;
    PolyFn cosp;
    long double t0 = 0;              // EvalMod polynomial target scale
    std::vector<long double> dac;    // double-angle constants a^(2^(i+1)), i < r
    std::vector<LinTrans> cts, stc;  // in application order
    std::vector<u64> trace_gal;      // Galois elements of the trace (rotations by slots * 2^i)
    int top = 0;
    long double s_y = 0;  // scale of the EvalMod output (2^60 up to rounding)
    u64 F = 1;            // ScaleDown: message times F = round(q0 / (2^8 Delta)) before ModRaise
    EvKey d2s, s2d;       // EvkDenseToSparse (level 0), EvkSparseToDense (full chain)
    std::vector<KeyNeed> need;  // key_needs(): every evaluation key the circuit uses (made with the circuit)
  };
  // declared in this order so that the circuits (whose buffers belong to a
  // bootstrapping context's pool) are destroyed before the contexts
  std::map<std::vector<int>, std::unique_ptr<Context>> btp_ctx;  // logPs -> bootstrapping context
  std::map<int, std::unique_ptr<Bootstrapper>> btps;             // slot count -> circuit

  // the butterfly stages of the n-point special FFT (lengths in application
  // order) split over ng transforms, the extra stages to the first ones
  static std::vector<std::vector<int>> fft_groups(int ns, bool inverse, int ng) {
    std::vector<int> lens;
    for (int len = inverse ? ns : 2; inverse ? len >= 2 : len <= ns; len = inverse ? len / 2 : len * 2)
      lens.push_back(len);
    std::vector<std::vector<int>> g(ng);
    const int tot = (int)lens.size();
    int at = 0;
    for (int k = 0; k < ng; ++k)
      for (int i = 0; i < tot / ng + (k < tot % ng ? 1 : 0); ++i) g[k].push_back(lens[at++]);
    return g;
  }

  // (on the bootstrapping context) the circuit for `ns` slots
  std::unique_ptr<Bootstrapper> make_circuit(int ns) {
    typedef Bootstrapper BT;
    const int n = N / 2;
    auto B = std::unique_ptr<Bootstrapper>(new Bootstrapper());
    B->bc = this;
    B->slots = ns;
    B->gap = n / ns;
    const long double PI = 3.14159265358979323846264338327950288L;
    // EvalMod: Lattigo's default Mod1Type CosDiscrete [U] -- a cos(2 pi (x -
    // 1/4) / 2^r), a = (2 pi)^(-1/2^r), interpolated at nodes on the integers
    // the ModRaise overflow takes (x = K u; hostmath.cpp cos_discrete_cheb,
    // nodes within 2^-LogMessageRatio of each integer); after the r double
    // angles y <- 2 y^2 - a^(2^(i+1)) it is sin(2 pi x) / (2 pi)
    const long double a = powl(2 * PI, -1.0L / (long double)(1 << B->r));
    B->cosp.cheb = true;
    B->cosp.c = cos_discrete_cheb(B->K, B->degree, B->r, ldexp(1.0, -BT::kLogMsgRatio));
    {
      long double v = a;
      for (int i = 0; i < B->r; ++i) B->dac.push_back(v = v * v);
    }
    B->top = L - 1;
    {  // ScaleDown (LogMessageRatio): round(q0 / (2^8 Delta)), Delta the default scale
      const long double f = roundl((long double)mods[0] / ldexpl(1.0L, BT::kLogMsgRatio + logScale));
      B->F = f < 1 ? 1 : (u64)f;
    }
    for (int s = ns; s < n; s *= 2) B->trace_gal.push_back(galois_element(s));
    int logns = 0;
    while ((1 << logns) < ns) ++logns;
    // the n-point special FFT (slots of Z[Y]/(Y^2n + 1), Y = X^gap); its
    // diagonals act n-periodically on the N/2 slots
    const std::vector<Cplx> twi = special_fft_twiddles(logns + 1, true), twf = special_fft_twiddles(logns + 1, false);
    const bool packed = ns < n;
    // CoeffsToSlots: slots of t / q0 -> bitrev((t_j + i t_{j+n}) / q0) / (2K).  The 1/n of the
    // inverse transform and EvalMod's 1 / (2K) are spread over the transforms (2^-s per
    // transform of s stages, the 4th root of 1 / (2K) each), so no diagonal is small against
    // the fixed-point grid of its encoding
    {
      const auto g = fft_groups(ns, true, BT::kCtS);
      int level = B->top;
      const double kf = sqrt(sqrt(1.0 / (2.0 * B->K)));
      for (int k = 0; k < BT::kCtS; ++k) {
        DiagMap M;
        M[0] = std::vector<cplx>(n, cplx(ldexp(kf, -(int)g[k].size()), 0));
        for (int len : g[k]) M = diag_compose(fft_stage(len, true, twi), M);
        if (packed && k == BT::kCtS - 1) {
          // w -> a w, a = 1 on [0, n) and -i on [n, 2n) of every 2n-period: then
          // a w + conj(a w) = 2 Re w on the first half, 2 Im w on the second
          DiagMap A;
          A[0] = std::vector<cplx>(n);
          for (int p = 0; p < n; ++p) A[0][p] = (p % (2 * ns)) < ns ? cplx(1, 0) : cplx(0, -1);
          M = diag_compose(A, M);
        }
        B->cts.push_back(make_lt_complex(M, level--));
      }
    }
    // EvalMod scales: the polynomial's target t0 is chosen so that the r
    // double angles (rescaled by the primes below its output level) end on
    // 2^60; s_y is the scale they actually reach (the same long double steps
    // as mul_relin and rescale_inplace)
    {
      const int lp = B->top - BT::kCtS - BT::kDepthPoly;  // level of the polynomial's output
      long double T = ldexpl(1.0L, BT::kModBits);
      for (int i = B->r - 1; i >= 0; --i) T = sqrtl(T * (long double)mods[lp - i]);
      B->t0 = T;
      long double sc = T;
      for (int i = 0; i < B->r; ++i) sc = sc * sc / (long double)mods[lp - i];
      B->s_y = sc;
      // SlotsToCoeffs: forward stages times c = q0 / (F s_y), so the output decodes at the
      // input scale
      const auto g = fft_groups(ns, false, BT::kStC);
      int level = lp - B->r;
      const double cf = cbrt((double)((long double)mods[0] / ((long double)B->F * sc)));
      for (int k = 0; k < BT::kStC; ++k) {
        DiagMap M;
        if (packed && k == 0) {
          // unpack: y_p + i y_{p+n} on the first half of a 2n-period, i y_p + y_{p-n}
          // (= y_{p+n}: y is 2n-periodic) on the second, so the result is n-periodic
          M[0] = std::vector<cplx>(n);
          M[ns] = std::vector<cplx>(n);
          for (int p = 0; p < n; ++p) {
            const bool lo = (p % (2 * ns)) < ns;
            M[0][p] = lo ? cplx(cf, 0) : cplx(0, cf);
            M[ns][p] = lo ? cplx(0, cf) : cplx(cf, 0);
          }
        } else {
          M[0] = std::vector<cplx>(n, cplx(cf, 0));
        }
        for (int len : g[k]) M = diag_compose(fft_stage(len, false, twf), M);
        B->stc.push_back(make_lt_complex(M, level--));
      }
    }
    // x i on every slot = multiplication by X^(N/2): the packing kernels' w4
    if (!packed) need_complex();
    B->need = key_needs(*B);
    // the keyed part; a context without the secret gets the circuit alone and
    // receives its keys record by record (import_key_record)
    if (have_sk) gen_circuit_keys(*B);
    return B;
  }
  // (on the bootstrapping context) the ephemeral secret and its keys
  // (genEncapsulationEvaluationKeysNew)
  void gen_circuit_keys(Bootstrapper& bt) {
    if (!have_sk) throw std::runtime_error("bootstrapping keys need the secret key");
    const Poly se = secret_poly(sample_ternary_h(Bootstrapper::kEphH));
    bt.d2s = EvKey{gen_evk(sk, se, 0), 0};
    bt.s2d = EvKey{gen_evk(se, sk, L - 1), L - 1};
  }

  // (on the bootstrapping context) every evaluation key run_circuit uses for
  // this circuit and the highest level it uses it at, derived from the built
  // circuit alone (host arithmetic: no secret, no device work), in record
  // order: the relinearisation key, d2s, s2d, then the Galois keys by
  // ascending element.  The levels follow run_circuit step by step: the trace
  // at the top, each transform at min(ciphertext level, its own level) -- the
  // level eval_lt runs it at -- the conjugation below CoeffsToSlots, EvalMod's
  // polynomial and double angles in between.
  std::vector<KeyNeed> key_needs(const Bootstrapper& bt) const {
    typedef Bootstrapper BT;
    std::map<u64, int> gal;
    auto use = [&](u64 g, int level) {
      auto it = gal.find(g);
      if (it == gal.end()) gal[g] = level;
      else it->second = std::max(it->second, level);
    };
    auto use_lt = [&](const LinTrans& T, int level) {
      for (int b : T.babies)
        if (b) use(galois_element(b), level);
      for (int j : T.giants)
        if (j) use(galois_element(j), level);
    };
    int level = L - 1;
    if (bt.gap > 1)
      for (u64 g : bt.trace_gal) use(g, level);
    for (const LinTrans& T : bt.cts) {
      level = std::min(level, T.level);
      use_lt(T, level);
      --level;  // lt_rescale
    }
    use(2 * (u64)N - 1, level);  // the conjugation
    level -= BT::kDepthPoly + bt.r;  // eval_mod
    for (const LinTrans& T : bt.stc) {
      level = std::min(level, T.level);
      use_lt(T, level);
      --level;
    }
    std::vector<KeyNeed> v;
    v.push_back(KeyNeed{BK_RELIN, 0, L - 1, nullptr});
    v.push_back(KeyNeed{BK_D2S, 0, 0, nullptr});
    v.push_back(KeyNeed{BK_S2D, 0, L - 1, nullptr});
    for (auto& kv : gal) v.push_back(KeyNeed{BK_GALOIS, kv.first, kv.second, nullptr});
    return v;
  }
  // the key records held for a circuit, in record order.  The Galois keys are
  // the bootstrapping context's, which circuits with the same logPs share, so
  // they may include a sibling circuit's
  std::vector<KeyNeed> key_records(const Bootstrapper& bt) const {
    std::vector<KeyNeed> v;
    if (have_rlk) v.push_back(KeyNeed{BK_RELIN, 0, L - 1, &rlk});
    if (bt.d2s.k.buf) v.push_back(KeyNeed{BK_D2S, 0, bt.d2s.level, &bt.d2s.k});
    if (bt.s2d.k.buf) v.push_back(KeyNeed{BK_S2D, 0, bt.s2d.level, &bt.s2d.k});
    for (auto& kv : gks) v.push_back(KeyNeed{BK_GALOIS, kv.first, kv.second.level, &kv.second.k});
    return v;
  }
  // the needed keys that are absent or held below their needed level
  std::vector<KeyNeed> missing_keys(const Bootstrapper& bt) const {
    std::vector<KeyNeed> miss;
    for (const KeyNeed& n : bt.need) {
      bool ok = false;
      if (n.kind == BK_RELIN) ok = have_rlk;
      else if (n.kind == BK_D2S) ok = bt.d2s.k.buf && bt.d2s.level >= n.level;
      else if (n.kind == BK_S2D) ok = bt.s2d.k.buf && bt.s2d.level >= n.level;
      else {
        auto it = gks.find(n.gel);
        ok = it != gks.end() && it->second.level >= n.level;
      }
      if (!ok) miss.push_back(n);
    }
    return miss;
  }
  // every missing key of the need-list, made at its needed level without
  // running the circuit (afterwards galois_key finds each key it asks for)
  void prepare_keys(Bootstrapper& bt) {
    no_capture("bootstrapping key generation");
    if (!have_sk)
      throw std::runtime_error("preparing bootstrapping keys needs the secret key (a scheme without it imports "
                               "them: OrionHipImportBootstrapKey)");
    if (!have_rlk) gen_relin();
    if (!bt.d2s.k.buf || !bt.s2d.k.buf) gen_circuit_keys(bt);
    for (const KeyNeed& n : bt.need)
      if (n.kind == BK_GALOIS) gen_galois(n.gel, n.level);
    HIPCHK(hipStreamSynchronize(stream));
  }

  Ciphertext lt_rescale(LinTrans& T, const Ciphertext& x) {
    // (the final ModDown and the rescale as one division where that applies)
    Ciphertext y = eval_lt(T, x, true);
    if (y.pend.buf)
      finish_moddown_rescale(y);
    else
      rescale_inplace(y);
    y.scale = x.scale;  // diagonals at scale q_level
    return y;
  }
  // mod1 evaluator: the cosine polynomial, then the double angles
  // y <- 2 y^2 - a^(2^(k+1)), the constant added at the product's scale
  // before its rescale
  Ciphertext eval_mod(const Bootstrapper& bt, const Ciphertext& u) {
    Ciphertext y = eval_poly(u, bt.cosp, bt.t0);
    for (int k = 0; k < bt.r; ++k) {
      Ciphertext t = mul_relin(y, y);
      double_add_const(t, -bt.dac[k] * t.scale);
      rescale_inplace(t);
      y = std::move(t);
    }
    return y;
  }
  // (on the bootstrapping context) x: the level-0 residues (NTT domain) of a
  // batch of B ciphertexts, already scaled down by F
  Ciphertext run_circuit(Bootstrapper& bt, const Poly& x, int B) {
    // EvkDenseToSparse at level 0: (x0, 0) + KS(x1), now under the ephemeral secret
    Poly e = alloc(2, 1, B);
    keyswitch(ks_route(B, 0), lsq(x, 1, 1, 0), 0, B, bt.d2s.k, bt.d2s.level, e, x.ptr());
    // ModRaise: the centred level-0 residues (coefficient domain) lifted to every Q limb
    Poly c0 = alloc(2, 1, B);
    ntt_io(nio(lsq(c0, 0, 2, 0), lsq(e, 0, 2, 0)), true);
    Ciphertext m = new_ct(L - 1, B, (long double)mods[0]);
    const LimbSet ml = lsq(m.poly, 0, 2, L - 1);
    if (orion_launch_modraise(ml, lsq(c0, 0, 2, 0), d_tb, N, stream)) throw std::runtime_error("modraise failed");
    ntt(ml, false);
    // EvkSparseToDense at the top level: (m0, 0) + KS(m1), back under the secret
    Ciphertext t = new_ct(L - 1, B, m.scale);
    keyswitch(ks_route(B, L - 1), lsq(m.poly, 1, 1, L - 1), L - 1, B, bt.s2d.k, bt.s2d.level, t.poly, m.poly.ptr());
    const LimbSet tl = lsq(t.poly, 0, 2, L - 1);
    if (bt.gap > 1) {  // Trace: (gap^-1 t) summed over the rotations by slots * 2^i
      std::vector<u64> gi(L);
      for (int l = 0; l < L; ++l) gi[l] = hm_invmod((u64)bt.gap % mods[l], mods[l]);
      ew1(EW_SCALE, tl, tl, &gi);
      for (u64 gel : bt.trace_gal) {
        Ciphertext r = apply_galois(t, gel);
        ew(EW_ADD, tl, tl, lsq(r.poly, 0, 2, L - 1));
      }
    }
    // CoeffsToSlots
    Ciphertext z = std::move(t);
    for (LinTrans& T : bt.cts) z = lt_rescale(T, z);
    Ciphertext zc = apply_galois(z, 2 * (u64)N - 1);
    Ciphertext y;
    if (bt.gap > 1) {
      // packed real | imaginary parts: z + conj z
      Ciphertext u = new_ct(z.level, B, z.scale);
      ew(EW_ADD, lsq(u.poly, 0, 2, z.level), lsq(z.poly, 0, 2, z.level), lsq(zc.poly, 0, 2, z.level));
      y = eval_mod(bt, u);
    } else {
      // real and imaginary parts: z + conj z, (conj z - z) i = -i (z - conj z)
      Ciphertext re = new_ct(z.level, B, z.scale), im = new_ct(z.level, B, z.scale);
      unpack_launch(lsq(re.poly, 0, 2, z.level), lsq(im.poly, 0, 2, z.level), lsq(z.poly, 0, 2, z.level),
                    lsq(zc.poly, 0, 2, z.level), B);
      Ciphertext yr = eval_mod(bt, re), yi = eval_mod(bt, im);
      y = new_ct(yi.level, B, yi.scale);  // yr + i yi
      pack_launch(lsq(y.poly, 0, 2, y.level), lsq(yr.poly, 0, 2, y.level), lsq(yi.poly, 0, 2, y.level), B);
    }
    // SlotsToCoeffs
    for (LinTrans& T : bt.stc) y = lt_rescale(T, y);
    return y;
  }

  // bootstrapper.go:19-58: one circuit per slot count (made once); logPs
  // empty = the scheme's own P bit sizes
  void new_bootstrapper(std::vector<int> logPs, int ns) {
    typedef Bootstrapper BT;
    if (ci) throw std::runtime_error("bootstrapping needs the Standard ring (Lattigo has no ConjugateInvariant bootstrapper)");
    if (ns < 2 || ns > N / 2 || (ns & (ns - 1)))
      throw std::runtime_error("slots must be a power of two in [2, " + std::to_string(N / 2) + "]");
    if (btps.count(ns)) return;
    if (logPs.empty()) logPs = logP_bits;
    for (int b : logPs)
      if (b < 20 || b > 61) throw std::runtime_error("bootstrapping P primes must be 20..61 bits");
    auto it = btp_ctx.find(logPs);
    if (it == btp_ctx.end()) {
      // the bootstrapping chain: the residual Q, then SlotsToCoeffs 3 x 39-bit, EvalMod
      // depth(poly) + r x 60-bit, CoeffsToSlots 4 x 56-bit (bottom to top), so the refreshed
      // ciphertext comes out at the residual chain's top level; P from logPs.  New primes skip
      // every prime of the scheme.
      std::vector<int> ext(BT::kStC, BT::kStCBits);
      ext.insert(ext.end(), BT::kDepthPoly + BT::kR, BT::kModBits);
      ext.insert(ext.end(), BT::kCtS, BT::kCtSBits);
      std::vector<int> bits = ext;
      bits.insert(bits.end(), logPs.begin(), logPs.end());
      const std::vector<u64> fresh = gen_moduli_excluding(logN, bits, mods);
      std::vector<u64> m(mods.begin(), mods.begin() + L);
      m.insert(m.end(), fresh.begin(), fresh.end());
      std::vector<int> qb = logQ_bits;
      qb.insert(qb.end(), ext.begin(), ext.end());
      if ((int)m.size() > ORION_MAXMOD || (int)m.size() > ORION_MAXLIMB)
        throw std::runtime_error("bootstrapping chain too long");
      HIPCHK(hipStreamSynchronize(stream));
      std::unique_ptr<Context> bc(new Context());
      bc->stream = stream;  // shared, not owned
      bc->prng = Prng(prng.next());
      bc->init_moduli(logN, m, qb, logPs, logScale, h, false);
      // a scheme without the secret key builds the chain and the circuit alone:
      // its keys arrive from the key owner (import_key_record)
      if (have_sk) {
        bc->import_secret(secret_coeffs());
        bc->gen_relin();
      }
      it = btp_ctx.emplace(logPs, std::move(bc)).first;
    }
    btps[ns] = it->second->make_circuit(ns);
  }
  // bootstrapper.go:61-80: a new ciphertext at the residual top level, at the
  // input's scale, times the post-scale N / (2 slots)
  Ciphertext bootstrap(const Ciphertext& in, int ns) {
    auto it = btps.find(ns);
    if (it == btps.end()) throw std::runtime_error("no bootstrapper found for slot count: " + std::to_string(ns));
    Bootstrapper& bt = *it->second;
    const int B = in.poly.B;
    // the key owner makes a missing key at its first use (gen_galois); a
    // context without the secret must hold every key before any work is queued
    if (!bt.bc->have_sk) {
      const std::vector<KeyNeed> miss = bt.bc->missing_keys(bt);
      if (!miss.empty())
        throw std::runtime_error("bootstrapper for " + std::to_string(ns) + " slots lacks " +
                                 std::to_string(miss.size()) + " of its " + std::to_string(bt.need.size()) +
                                 " evaluation keys, the first: " + key_kind_name(miss[0].kind) +
                                 " key, galois element " + std::to_string(miss[0].gel) + ", level " +
                                 std::to_string(miss[0].level) +
                                 " (there is no secret key: import them, OrionHipImportBootstrapKey)");
    }
    // ScaleDown (Lattigo ScaleDown [U]): F = round(q0 / (2^LogMessageRatio
    // scale)) times the level-0 residues (an integer: no level), F from the
    // input's own scale so the message sits 2^-8 below q0 whatever its scale;
    // SlotsToCoeffs carries the default scale's F (bt.F), so the output scale
    // is scale F / bt.F -- the input scale exactly when it is the default
    const long double fr = roundl((long double)mods[0] / ldexpl(in.scale, Bootstrapper::kLogMsgRatio));
    const u64 F = fr < 1 ? 1 : (u64)fr;
    Poly x = alloc(2, 1, B);
    std::vector<u64> f{F % mods[0]};
    ew1(EW_SCALE, lsq(x, 0, 2, 0), lsq(in.poly, 0, 2, 0), &f);
    Ciphertext o = bt.bc->run_circuit(bt, x, B);
    if (o.level != L - 1) throw std::logic_error("bootstrapping circuit did not end at the residual top level");
    Ciphertext out = new_ct(L - 1, B, in.scale * (long double)F / (long double)bt.F);
    // the residual limbs hold the same primes in both contexts
    const LimbSet ol = lsq(out.poly, 0, 2, L - 1);
    if (bt.gap > 1) {  // post-scale (an integer: no level)
      std::vector<u64> ps(L);
      for (int l = 0; l < L; ++l) ps[l] = (u64)bt.gap % mods[l];
      ew1(EW_SCALE, ol, lsq(o.poly, 0, 2, L - 1), &ps);
    } else {
      copy(ol, lsq(o.poly, 0, 2, L - 1));
    }
    return out;
  }
  // bootstrap of a batch of B images as h = ceil(B / 2) packed ones: image k <
  // B - h rides with image k + h (for odd B image h - 1 goes alone).  The pack
  // reads limb 0 only, as bootstrap does; the unpack at the residual top level
  // writes its two outputs straight into the images k and k + h of the result,
  // which holds the refreshed images at twice bootstrap's scale
  Ciphertext bootstrap_packed(const Ciphertext& in, int ns) {
    need_complex();
    if (!btps.count(ns)) throw std::runtime_error("no bootstrapper found for slot count: " + std::to_string(ns));
    const int B = in.poly.B, h = (B + 1) / 2, np = B - h;
    Ciphertext p;
    p.poly = alloc(2, 1, h);
    p.level = 0;
    p.scale = in.scale;
    {
      const LimbSet a = lsq(in.poly, 0, 2, 0, h);
      LimbSet b = lsq(in.poly, 0, 2, 0, np);
      b.p = np ? in.poly.ptr() + (long long)h * in.poly.batch_stride() : nullptr;
      pack_launch(lsq(p.poly, 0, 2, 0), a, b, np);
    }
    const Ciphertext r = bootstrap(p, ns);
    const Ciphertext yc = apply_galois(r, 2 * (u64)N - 1);
    Ciphertext out = new_ct(r.level, B, 2 * r.scale);
    const LimbSet re = lsq(out.poly, 0, 2, r.level, h);
    LimbSet im = lsq(out.poly, 0, 2, r.level, np);
    im.p = np ? out.poly.ptr() + (long long)h * out.poly.batch_stride() : nullptr;
    unpack_launch(re, im, lsq(r.poly, 0, 2, r.level), lsq(yc.poly, 0, 2, r.level), np);
    return out;
  }
  // bootstrap of a batch of B images with ns slots each as h = ceil(B / g)
  // full-slot ones, g = N / (2 ns): the mean trace of limb 0 projects every
  // image onto Z[X^g], image k + i h rides in group k at X^i through the
  // full-slot bootstrapper's ScaleDown and circuit, and the unpack and the sum
  // trace at the residual top level pull it out again.  The g^-1 of the input
  // trace cancels against the g of the output trace, which also stands for the
  // sparse bootstrapper's post-scale: no scaling here.  Every step is the
  // public call's, so the bits are those of CloneCiphertext, ModDropCiphertext
  // to level 0, OrionHipSlotTraceNew(mean), OrionHipPackMonomials, Bootstrap(N / 2),
  // OrionHipUnpackMonomials, OrionHipSlotTraceNew.  ns = N / 2 is bootstrap.
  Ciphertext bootstrap_many(const Ciphertext& in, int ns) {
    const std::vector<int> ks = slot_trace_amounts(ns);  // (the ring and ns checked)
    if (!btps.count(N / 2))
      throw std::runtime_error("OrionHipBootstrapMany runs the full-slot circuit: no bootstrapper found for slot "
                               "count N/2 = " + std::to_string(N / 2) + " (NewBootstrapper(logPs, " +
                               std::to_string(N / 2) + ") makes it; one for " + std::to_string(ns) +
                               " slots is not needed)");
    if (ks.empty()) return bootstrap(in, ns);
    const int g = 1 << ks.size(), B = in.poly.B;
    slot_trace_keys(ks);  // every key, before anything is allocated
    need_mono();
    const Ciphertext u = slot_trace_run(in.poly, 0, in.scale, ks, true);
    const Ciphertext p = pack_monomials(u, g);
    const Ciphertext r = bootstrap(p, N / 2);
    Ciphertext w = unpack_monomials(r, g, B);
    for (int k : ks) rotate_add_inplace(w, k);  // the sum trace, on the unpacked images themselves (no copy)
    return w;
  }
  void delete_bootstrappers() {
    if (stream) HIPCHK(hipStreamSynchronize(stream));
    btps.clear();
    btp_ctx.clear();
  }
};

// ---------------------------------------------------------------------------
// the scheme's contexts: [0] the scheme's own, [1..] its pipelines
// ---------------------------------------------------------------------------
// A pipeline is a context on the scheme's chain that shares the scheme's keys
// and reads the scheme's compiled objects (plaintexts, linear transforms,
// polynomials), with its own HIP stream, buffer pool and handle range.  Each
// thread acts on one context: the thread that made the scheme on the scheme's,
// and, once OrionHipThreadPipelines(n > 1) is set (or ORION_THREAD_PIPELINES=n
// is in the environment), every other thread on a pipeline of its own, made at
// its first call (up to n contexts; further threads share them round-robin).
// So several threads each running the unchanged frontend's `net(ct)` over their
// own ciphertexts run their kernels concurrently on the GPU, each call holding
// only its own context's lock.  Handles are unique across the contexts; calls
// that only name a handle (deletes, metadata) go to the handle's context.
//
// Locks: g_reg (shared by every call, exclusive for NewScheme/DeleteScheme);
// a context's mu for a call acting on it; a thread holding a pipeline's mu may
// take the scheme's (keys, bootstrapping), never the other way round; the
// handle pools' and device pools' locks are leaves.
static std::unique_ptr<Context> g_slot[kMaxCtx];
static std::atomic<int> g_nctx{0};
static std::shared_mutex g_reg;
static std::mutex g_create_mu;
static std::atomic<unsigned long long> g_scheme_gen{1};
static std::atomic<int> g_thread_pipes{getenv("ORION_THREAD_PIPELINES") ? atoi(getenv("ORION_THREAD_PIPELINES")) : 0};
static std::atomic<unsigned> g_rr{0};
static std::thread::id g_scheme_thread;
static unsigned long g_seed = 0x0123456789abcdefull;
struct ThreadBind {
  Context* c = nullptr;
  unsigned long long gen = 0;
};
static thread_local ThreadBind t_bind;
static thread_local Context* t_act = nullptr;  // the context the running call acts on
static thread_local int t_depth = 0;           // nesting of C-ABI calls (SubScalar -> AddScalar)
static thread_local int t_dev = -1;            // this thread's HIP device, as last set here

static Context* scheme_ctx() { return g_nctx.load() > 0 ? g_slot[0].get() : nullptr; }
static Context* slot_ctx(int i) { return i >= 0 && i < g_nctx.load() ? g_slot[i].get() : nullptr; }

static Context& ctx() {
  if (!t_act) throw std::runtime_error("scheme not initialised: call NewScheme first");
  return *t_act;
}

// the caller's stream waits for everything queued on context `owner`'s stream
static void wait_on(Context& me, Context& o) {
  if (&me == &o) return;
  hipEvent_t e;
  HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIPCHK(hipEventRecord(e, o.stream));
  HIPCHK(hipStreamWaitEvent(me.stream, e, 0));
  HIPCHK(hipEventDestroy(e));  // (released once the wait has completed)
}
// HandlePool hooks: a call reading another context's object orders its stream
// after that object's producer.  A ciphertext (changed by the ops of its
// context) always waits for its context's queued work; a compiled object
// waits only when it is younger than what this context already waited for
// (every object older than a pipeline was complete when it was made)
static void foreign_order(int owner, unsigned long long birth, bool always) {
  Context* me = t_act;
  Context* o = slot_ctx(owner);
  if (!me || !o || o == me) return;
  if (!always && birth < me->synced[owner]) return;
  if (me->capturing)
    throw std::runtime_error("a captured op reads context " + std::to_string(owner) +
                             "'s newer object: capture on the context that owns it, or run the stream once first");
  const unsigned long long stamp = g_birth.load();
  wait_on(*me, *o);
  if (!always) me->synced[owner] = stamp;
}
// a ciphertext of context `owner` whose ModDown is pending there
// (deferral.h), read by the acting context: the plain ModDown runs here, on this
// context's stream (which the hook has ordered after the owner's), into a
// buffer of the owner's pool.  That buffer may have been released by work the
// owner queued since, so this stream waits for the owner's once more; the
// owner's stream then waits for the ModDown before the accumulator goes back
// to its pool.  The owner's record stays: its flush finds nothing pending
static void foreign_finish(Ciphertext& v, int owner) {
  Context* me = t_act;
  Context* o = slot_ctx(owner);
  if (!v.pend.buf || !me || !o || o == me) return;
  const int level = v.level;
  Poly out = o->alloc(2, level + 1, v.pend.B);
  wait_on(*me, *o);
  const LimbSet x = me->lsqp(v.pend, 0, 2, level, level), lo = me->lsq(out, 0, 2, level);
  me->moddown(x, level, lo, me->md_route(x, level, lo));
  wait_on(*o, *me);
  v.poly = out;
  v.pend = Poly();
}
static HandlePool<Ciphertext>* res_cts(int i) { Context* c = slot_ctx(i); return c ? &c->cts : nullptr; }
static HandlePool<Plaintext>* res_pts(int i) { Context* c = slot_ctx(i); return c ? &c->pts : nullptr; }
static HandlePool<LinTrans>* res_lts(int i) { Context* c = slot_ctx(i); return c ? &c->lts : nullptr; }
static HandlePool<LtBlocks>* res_ltbs(int i) { Context* c = slot_ctx(i); return c ? &c->ltbs : nullptr; }
static HandlePool<Context::PolyFn>* res_polys(int i) { Context* c = slot_ctx(i); return c ? &c->polys : nullptr; }
static const bool g_hooks_set = [] {
  HandlePool<Ciphertext>::resolver() = res_cts;
  HandlePool<Plaintext>::resolver() = res_pts;
  HandlePool<LinTrans>::resolver() = res_lts;
  HandlePool<Context::PolyFn>::resolver() = res_polys;
  HandlePool<LtBlocks>::resolver() = res_ltbs;
  HandlePool<LtBlocks>::hook() = [](int o, unsigned long long b) { foreign_order(o, b, false); };
  HandlePool<LtBlocks>::hold() = [](const LtBlocks& b) {
    if (t_act && t_act->capturing && b.lay.dev) t_act->capture_holds.push_back(b.lay.dev);
  };
  HandlePool<Ciphertext>::hook() = [](int o, unsigned long long b) { foreign_order(o, b, true); };
  HandlePool<Plaintext>::hook() = [](int o, unsigned long long b) { foreign_order(o, b, false); };
  HandlePool<LinTrans>::hook() = [](int o, unsigned long long b) { foreign_order(o, b, false); };
  HandlePool<Context::PolyFn>::hook() = [](int o, unsigned long long b) { foreign_order(o, b, false); };
  HandlePool<Ciphertext>::check() = [](const Ciphertext& c) {
    if (!c.poison.empty()) throw std::runtime_error(c.poison);
  };
  HandlePool<Ciphertext>::fix() = foreign_finish;
  HandlePool<Ciphertext>::hold() = [](const Ciphertext& c) {
    if (t_act && t_act->capturing && c.poly.buf) t_act->capture_holds.push_back(c.poly.buf);
  };
  HandlePool<Plaintext>::hold() = [](const Plaintext& p) {
    if (t_act && t_act->capturing && p.poly.buf) t_act->capture_holds.push_back(p.poly.buf);
  };
  HandlePool<LinTrans>::hold() = [](const LinTrans& t) {
    if (!t_act || !t_act->capturing) return;
    for (auto& kv : t.diags)
      if (kv.second.poly.buf) t_act->capture_holds.push_back(kv.second.poly.buf);
    for (auto& kv : t.sdiags)
      if (kv.second.buf) t_act->capture_holds.push_back(kv.second.buf);
    if (t.lay.dev) t_act->capture_holds.push_back(t.lay.dev);
  };
  return true;
}();

// a new pipeline context (the caller holds no context lock)
static Context* create_pipeline() {
  std::lock_guard<std::mutex> lk(g_create_mu);
  Context* s = scheme_ctx();
  if (!s) throw std::runtime_error("scheme not initialised: call NewScheme first");
  const int idx = g_nctx.load();
  if (idx >= kMaxCtx) throw std::runtime_error("too many pipelines (" + std::to_string(kMaxCtx - 1) + " at most)");
  std::lock_guard<std::recursive_mutex> sl(s->mu);  // the scheme's keys and transforms are read
  if (t_dev != s->dev) {
    HIPCHK(hipSetDevice(s->dev));
    t_dev = s->dev;
  }
  // the scheme's transforms get their device plans now, so a pipeline only
  // reads them; then every object born so far is complete once the queued
  // work of every context has run
  s->build_dirty_plans();
  const unsigned long long stamp = g_birth.load();
  for (int i = 0; i < idx; ++i) HIPCHK(hipStreamSynchronize(g_slot[i]->stream));
  std::unique_ptr<Context> p(new Context());
  p->index = idx;
  p->dev = s->dev;
  p->prng = Prng(g_seed ^ (0x9e3779b97f4a7c15ull * (u64)idx));
  p->init_moduli(s->logN, s->mods, s->logQ_bits, s->logP_bits, s->logScale, s->h, s->ci);
  p->adopt_keys(*s);
  p->seed_encryption(g_seed + 0x9e3779b97f4a7c15ull * (u64)idx);
  const int base = idx << kCtxShift;
  p->pts.set_base(base), p->cts.set_base(base), p->lts.set_base(base), p->polys.set_base(base);
  p->ltbs.set_base(base);
  p->next_graph = base;
  for (int j = 0; j < kMaxCtx; ++j) p->synced[j] = stamp;
  Context* r = p.get();
  g_slot[idx] = std::move(p);
  g_nctx.store(idx + 1);
  return r;
}

// the context the calling thread acts on (create: a thread's first call may
// make its pipeline); nullptr without a scheme
static Context* thread_ctx(bool create) {
  Context* s = scheme_ctx();
  if (!s) return nullptr;
  const unsigned long long gen = g_scheme_gen.load();
  if (t_bind.c && t_bind.gen == gen) return t_bind.c;
  const int n = g_thread_pipes.load();
  if (n <= 1 || std::this_thread::get_id() == g_scheme_thread) return s;
  if (!create) return s;
  Context* c = nullptr;
  if (g_nctx.load() < n) {
    c = create_pipeline();
  } else {
    const int np = g_nctx.load() - 1;
    c = np > 0 ? g_slot[1 + (int)(g_rr.fetch_add(1) % (unsigned)np)].get() : s;
  }
  t_bind = ThreadBind{c, gen};
  return c;
}
// the context of a handle (deletes and metadata go to the handle's own
// context, whichever thread asks)
static Context* handle_ctx(int id) {
  Context* c = id >= 0 ? slot_ctx(id >> kCtxShift) : nullptr;
  return c ? c : thread_ctx(false);
}

// one C-ABI call: the registry lock (outermost call only), the lock of the
// context it acts on, and that context as the thread's acting one
struct CallScope {
  std::shared_lock<std::shared_mutex> rl;
  std::unique_lock<std::recursive_mutex> cl;
  Context* saved;
  CallScope(bool reg = true) : saved(t_act) {
    if (t_depth++ == 0 && reg) rl = std::shared_lock<std::shared_mutex>(g_reg);
  }
  void act(Context* c) {
    if (!c) return;
    cl = std::unique_lock<std::recursive_mutex>(c->mu);
    t_act = c;
    if (t_dev != c->dev) {
      HIPCHK(hipSetDevice(c->dev));
      t_dev = c->dev;
    }
  }
  ~CallScope() {
    t_act = saved;
    --t_depth;
  }
};

}  // namespace orion

using namespace orion;

// ---------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------
// debugging switch ORION_DEBUG_SYNC=1: drain the library stream at the start
// of every C-ABI call (separates an ordering race from an arithmetic fault)
static const bool g_debug_sync = getenv("ORION_DEBUG_SYNC") && atoi(getenv("ORION_DEBUG_SYNC")) != 0;
// (deferral.h kCalls says which calls may be recorded into a graph)
static void capture_guard(const deferral::Call& fn) {
  Context* c = t_act;
  if (c && c->capturing && !fn.capture)
    throw std::runtime_error(std::string(fn.name) + " is not allowed while capturing a graph");
  if (g_debug_sync && c && !c->capturing && c->stream) (void)hipStreamSynchronize(c->stream);
}
static int ct_ct_op(int i0, int i1, int op, bool inplace);
// What event e makes of the context's pending work (deferral::step), carried
// out: the one place that sets the state and runs the work.  Returns what ran.
// If it fails, the ciphertexts it should have written are poisoned: every
// later use of r, or of x (which the AddCiphertext already reported as done),
// fails loudly with this error instead of reading a buffer never written.
static deferral::Act defer_apply(Context& c, const deferral::Event& e) {
  using namespace deferral;
  const Pending d = c.dfr;
  const Step s = step(d, e);
  Act ran = s.act;
  if (ran == Act::RecordAdd) c.inplace_ct(d.x);
  // (another context that read r has run the ModDown: foreign_finish)
  if (ran == Act::ModDownRescale && !c.inplace_ct(d.r).pend.buf) ran = Act::None;
  c.dfr = s.next;
  try {
    if (ran == Act::Rotate || ran == Act::RotateThenAdd) c.rotate_into(c.cts.get(d.x), d.k, c.cts.get(d.r));
    if (ran == Act::RotateThenAdd) ct_ct_op(d.x, d.r, EW_ADD, true);
    if (ran == Act::FusedRotateAdd) c.rotate_add_inplace(c.cts.get(d.x), d.k);
    if (ran == Act::ModDown) c.finish_moddown(c.cts.get(d.r));
    if (ran == Act::ModDownRescale) c.finish_moddown_rescale(c.cts.get(d.r));
  } catch (const std::exception& err) {
    const std::string what = d.kind == Kind::ModDown ? "ModDown" : "rotation by " + std::to_string(d.k);
    for (int id : {d.r, d.kind == Kind::RotationAdded ? d.x : -1}) {
      try {
        if (id >= 0)
          c.cts.get(id).poison =
              "a deferred " + what + " failed (" + err.what() + "): this ciphertext was never written";
      } catch (const std::exception&) {
      }
    }
    throw;
  }
  return ran;
}
static void api_gate(const deferral::Call& fn) {
  capture_guard(fn);
  if (t_act) defer_apply(*t_act, {fn.keeps ? deferral::Ev::Keeps : deferral::Ev::Flushes});
}
// a call acting on the calling thread's context
#define API_BEGIN         \
  CallScope cs_;          \
  try {                   \
    cs_.act(thread_ctx(true)); \
    static const deferral::Call fn_ = deferral::call(__func__); \
    api_gate(fn_);
// a call acting on the context of handle `id`
#define API_BEGIN_HANDLE(id) \
  CallScope cs_;             \
  try {                      \
    cs_.act(handle_ctx(id)); \
    static const deferral::Call fn_ = deferral::call(__func__); \
    api_gate(fn_);
// a call acting on no context (or on several, one at a time)
#define API_BEGIN_NOCTX \
  CallScope cs_;        \
  try {
// NewScheme / DeleteScheme: every other call is kept out
#define API_BEGIN_EXCL                                \
  std::unique_lock<std::shared_mutex> xl_(g_reg);     \
  CallScope cs_(false);                               \
  try {
// (a failed call's HIP error is read off here, so that it is reported once,
// by this call, and not again by the next call's launch checks)
#define API_END(errval)          \
  }                              \
  catch (const std::exception& e) { \
    g_last_error = e.what();     \
    (void)hipGetLastError();     \
    return errval;               \
  }
#define API_END_VOID                \
  }                                 \
  catch (const std::exception& e) { \
    g_last_error = e.what();        \
    (void)hipGetLastError();        \
  }

template <class T, class U>
static U* to_c_array(const std::vector<T>& v, unsigned long* len) {
  *len = v.size();
  if (v.empty()) return nullptr;
  U* p = (U*)malloc(sizeof(U) * v.size());
  for (size_t i = 0; i < v.size(); ++i) p[i] = (U)v[i];
  return p;
}

extern "C" {

const char* OrionHipLastError(void) { return g_last_error.c_str(); }
void OrionHipClearError(void) { g_last_error.clear(); }

static hipStream_t g_user_stream = nullptr;

int OrionHipSetDevice(int device) {
  API_BEGIN_NOCTX
  HIPCHK(hipSetDevice(device));
  t_dev = device;
  return 0;
  API_END(-1)
}

void OrionHipSetSeed(unsigned long seed) {
  API_BEGIN
  g_seed = seed;
  if (t_act) {
    t_act->prng = Prng(seed);
    t_act->seed_encryption(seed);
  }
  API_END_VOID
}

void OrionHipSetStream(void* s) {
  API_BEGIN
  Context* c = t_act;
  if (!c || c->index == 0) g_user_stream = (hipStream_t)s;
  if (c) {
    // the buffer pool hands freed buffers out again with no stream tracking:
    // drain the old stream so no kernel still reading or writing a pooled
    // buffer overlaps the first launches on the new one
    if (c->stream) HIPCHK(hipStreamSynchronize(c->stream));
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    c->own_stream = false;
    c->stream = (hipStream_t)s;
    if (!s) {
      HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
      c->own_stream = true;
    }
    for (auto& kv : c->btp_ctx) kv.second->stream = c->stream;
  }
  API_END_VOID
}

// the calling thread's context's stream (a thread's first call binds it to
// its pipeline when thread pipelines are on)
void* OrionHipGetStream(void) {
  API_BEGIN
  return t_act ? (void*)t_act->stream : nullptr;
  API_END(nullptr)
}

int OrionHipSynchronize(void) {  // every context's stream (the pipelines' included)
  API_BEGIN_NOCTX
  if (!scheme_ctx()) throw std::runtime_error("scheme not initialised: call NewScheme first");
  for (int i = 0; i < g_nctx.load(); ++i) HIPCHK(hipStreamSynchronize(g_slot[i]->stream));
  return 0;
  API_END(-1)
}

// ---- hipGraph capture of op streams (see Context::graph_begin) ----
int OrionHipGraphBegin(void) {
  API_BEGIN
  ctx().graph_begin();
  return 0;
  API_END(-1)
}
int OrionHipGraphEnd(void) {
  API_BEGIN
  return ctx().graph_end();
  API_END(-1)
}
int OrionHipGraphLaunch(int graph) {  // on the stream of the context that captured it
  API_BEGIN_HANDLE(graph)
  ctx().graph_launch(graph);
  return 0;
  API_END(-1)
}
void OrionHipGraphDestroy(int graph) {
  API_BEGIN_HANDLE(graph)
  ctx().graph_destroy(graph);
  API_END_VOID
}

int OrionHipLogN(void) { return scheme_ctx() ? scheme_ctx()->logN : -1; }
int OrionHipNumQ(void) { return scheme_ctx() ? scheme_ctx()->L : -1; }
int OrionHipNumP(void) { return scheme_ctx() ? scheme_ctx()->K : -1; }
unsigned long OrionHipModulus(int i) {
  Context* s = scheme_ctx();
  return (s && i >= 0 && i < (int)s->mods.size()) ? s->mods[i] : 0;
}

void NewScheme(int logN, int* logQ, int lenQ, int* logP, int lenP, int logScale, int h, char* ringType,
               char* keysPath, char* ioMode) {
  API_BEGIN_EXCL
  (void)keysPath;
  (void)ioMode;
  std::string rt = ringType ? ringType : "standard";
  for (auto& ch : rt) ch = (char)tolower(ch);
  // scheme.go:50-51: any ring type other than "standard" selects Lattigo's
  // ConjugateInvariant ring Z[X + X^-1]/(X^2N + 1) of degree N (NthRoot 4N,
  // N real slots), held natively: N coefficients per limb, the NTT folds and
  // unfolds around the degree-N transform (ntt.hip, Context::setup).
  const bool ci = rt != "standard";
  if (ci && rt != "conjugateinvariant")
    throw std::runtime_error("unknown ring type '" + rt + "' (standard | conjugateinvariant)");
  // the CI NTT folds/unfolds inside the one-pass kernels (N <= 2^15 per CU)
  if (ci && (logN < 13 || logN > 15))
    throw std::runtime_error("ConjugateInvariant ring: logN must be 13..15 in this build");
  for (int i = g_nctx.load() - 1; i >= 0; --i) g_slot[i].reset();  // pipelines first
  g_nctx.store(0);
  g_scheme_gen.fetch_add(1);
  std::unique_ptr<Context> c(new Context());
  c->index = 0;
  HIPCHK(hipGetDevice(&c->dev));
  t_dev = c->dev;
  c->stream = g_user_stream;
  c->prng = Prng(g_seed);
  c->setup(logN, std::vector<int>(logQ, logQ + lenQ), std::vector<int>(logP, logP + lenP), logScale, h, ci);
  c->seed_encryption(g_seed);
  g_scheme_thread = std::this_thread::get_id();
  t_bind = ThreadBind{c.get(), g_scheme_gen.load()};
  g_slot[0] = std::move(c);
  g_nctx.store(1);
  API_END_VOID
}

void DeleteScheme(void) {
  API_BEGIN_EXCL
  for (int i = g_nctx.load() - 1; i >= 0; --i) g_slot[i].reset();  // pipelines first
  g_nctx.store(0);
  g_scheme_gen.fetch_add(1);
  API_END_VOID
}

// Pipelines (see the registry above).  OrionHipPeerCreate makes one and
// returns its index (the scheme's context is 0) without binding any thread;
// OrionHipPeerSelect binds the calling thread to a context; with
// OrionHipThreadPipelines(n > 1) threads are bound automatically.
int OrionHipPeerCreate(void) {
  API_BEGIN_NOCTX
  return create_pipeline()->index;
  API_END(-1)
}
int OrionHipPeerSelect(int id) {
  API_BEGIN_NOCTX
  Context* c = slot_ctx(id);
  if (!c) throw std::runtime_error("no such pipeline context: " + std::to_string(id));
  t_bind = ThreadBind{c, g_scheme_gen.load()};
  return 0;
  API_END(-1)
}
int OrionHipPeerCount(void) { return g_nctx.load(); }
// n > 1: every thread other than the scheme's gets a pipeline of its own at
// its first call, up to n contexts in all (then round-robin); n <= 1: off.
// Returns the previous setting.
int OrionHipThreadPipelines(int n) { return g_thread_pipes.exchange(n); }
// the index of the calling thread's context (binding it, as any call does)
int OrionHipCurrentPipeline(void) {
  API_BEGIN
  return ctx().index;
  API_END(-1)
}
// ORION_POOL_CAP_BYTES at run time (0: no cap; see DevicePool::alloc);
// returns the previous cap
double OrionHipPoolCap(double bytes) {
  std::lock_guard<std::recursive_mutex> lk(DevicePool::mu());
  const double prev = DevicePool::cap_bytes();
  DevicePool::cap_ref() = bytes;
  return prev;
}
int OrionHipPoolStats(double* out, int n) {
  std::lock_guard<std::recursive_mutex> lk(DevicePool::mu());
  double cached = 0;
  for (DevicePool* q : DevicePool::registry()) cached += (double)q->cached();
  const double v[5] = {DevicePool::stats()[0], DevicePool::stats()[1], DevicePool::stats()[2], DevicePool::stats()[3],
                       cached};
  for (int i = 0; i < n && i < 5; ++i) out[i] = v[i];
  return 5;
}
int OrionHipStreamWaitPeer(int peer) {
  API_BEGIN
  Context* p = slot_ctx(peer);
  if (!p) throw std::runtime_error("no such pipeline context: " + std::to_string(peer));
  wait_on(ctx(), *p);
  return 0;
  API_END(-1)
}

void FreeCArray(void* p) { free(p); }

void DeletePlaintext(int id) {
  API_BEGIN_HANDLE(id)
  ctx().pts.del(id);
  API_END_VOID
}
void DeleteCiphertext(int id) {
  API_BEGIN_HANDLE(id)
  Context& c = ctx();
  try {
    defer_apply(c, {deferral::Ev::Delete, id});
  } catch (const std::exception&) {
    c.cts.del(id);  // the handle goes away whatever happens
    throw;
  }
  c.cts.del(id);
  API_END_VOID
}

static unsigned long scale_u64(long double s) {
  if (s >= 18446744073709551615.0L) return ~0ul;
  return (unsigned long)s;
}
unsigned long GetPlaintextScale(int id) {
  API_BEGIN_HANDLE(id)
  return scale_u64(ctx().pts.get(id).scale);
  API_END(0)
}
unsigned long GetCiphertextScale(int id) {
  API_BEGIN_HANDLE(id)
  return scale_u64(ctx().cts.get(id).scale);
  API_END(0)
}
double GetCiphertextScaleF(int id) {
  API_BEGIN_HANDLE(id)
  return (double)ctx().cts.get(id).scale;
  API_END(0)
}
void SetPlaintextScale(int id, unsigned long s) {
  API_BEGIN_HANDLE(id)
  ctx().pts.get(id).scale = (long double)s;
  API_END_VOID
}
void SetCiphertextScale(int id, unsigned long s) {
  API_BEGIN_HANDLE(id)
  ctx().cts.get(id).scale = (long double)s;
  API_END_VOID
}
int GetPlaintextLevel(int id) {
  API_BEGIN_HANDLE(id)
  return ctx().pts.get(id).level;
  API_END(-1)
}
int GetCiphertextLevel(int id) {
  API_BEGIN_HANDLE(id)
  return ctx().cts.get(id).level;
  API_END(-1)
}
int GetPlaintextSlots(int id) {
  API_BEGIN_HANDLE(id)
  ctx().pts.get(id);
  return ctx().slots;
  API_END(-1)
}
int GetCiphertextSlots(int id) {
  API_BEGIN_HANDLE(id)
  ctx().cts.get(id);
  return ctx().slots;
  API_END(-1)
}
int GetCiphertextDegree(int id) {
  API_BEGIN_HANDLE(id)
  ctx().cts.get(id);
  return 1;
  API_END(-1)
}
int GetCiphertextBatch(int id) {
  API_BEGIN_HANDLE(id)
  return ctx().cts.get(id).poly.B;
  API_END(-1)
}
int GetPlaintextBatch(int id) {
  API_BEGIN_HANDLE(id)
  return ctx().pts.get(id).poly.B;
  API_END(-1)
}
ArrayResultUInt64 GetModuliChain(void) {
  ArrayResultUInt64 r{nullptr, 0};
  API_BEGIN
  std::vector<u64> q(ctx().mods.begin(), ctx().mods.begin() + ctx().L);
  r.Data = to_c_array<u64, unsigned long>(q, &r.Length);
  return r;
  API_END(r)
}
ArrayResultInt GetLivePlaintexts(void) {
  ArrayResultInt r{nullptr, 0};
  API_BEGIN
  r.Data = to_c_array<int, int>(ctx().pts.live(), &r.Length);
  return r;
  API_END(r)
}
ArrayResultInt GetLiveCiphertexts(void) {
  ArrayResultInt r{nullptr, 0};
  API_BEGIN
  r.Data = to_c_array<int, int>(ctx().cts.live(), &r.Length);
  return r;
  API_END(r)
}
int CloneCiphertext(int id) {
  API_BEGIN
  Context& c = ctx();
  return c.cts.add(c.clone(c.cts.get(id)));
  API_END(-1)
}
static std::string scale_str(long double s) {
  char b[64];
  snprintf(b, sizeof(b), "%.21Lg", s);
  return b;
}
int OrionHipStackCiphertexts(const int* ids, int n) {
  API_BEGIN
  Context& c = ctx();
  if (n < 1) throw std::runtime_error("cannot stack " + std::to_string(n) + " ciphertexts: at least one is needed");
  if (!ids) throw std::runtime_error("null handle list");
  // every source is looked up (and checked) before anything is allocated; a
  // source of another context orders this stream after its producer (cts.get)
  std::vector<GatherSrc> src;
  std::vector<std::shared_ptr<Buffer>> keep;  // the sources' buffers, until the launches are queued
  int level = 0;
  long double scale = 0;
  for (int i = 0; i < n; ++i) {
    const Ciphertext& a = c.cts.get(ids[i]);
    if (i == 0) {
      level = a.level, scale = a.scale;
    } else if (a.level != level) {
      throw std::runtime_error("cannot stack ciphertexts " + std::to_string(ids[0]) + " (level " +
                               std::to_string(level) + ") and " + std::to_string(ids[i]) + " (level " +
                               std::to_string(a.level) + "): the levels differ");
    } else if (a.scale != scale) {
      throw std::runtime_error("cannot stack ciphertexts " + std::to_string(ids[0]) + " (scale " + scale_str(scale) +
                               ") and " + std::to_string(ids[i]) + " (scale " + scale_str(a.scale) +
                               "): the scales differ");
    }
    if (src.size() + (size_t)a.poly.B > (size_t)0x7fffffff) throw std::runtime_error("stacked batch too large");
    Context::gather_sources(a, 0, a.poly.B, src);
    keep.push_back(a.poly.buf);
  }
  Ciphertext out = c.new_ct(level, (int)src.size(), scale);
  c.gather(out, src);
  return c.cts.add(std::move(out));
  API_END(-1)
}
int OrionHipSliceCiphertext(int id, int first, int count) {
  API_BEGIN
  Context& c = ctx();
  const Ciphertext& a = c.cts.get(id);
  const int B = a.poly.B;
  if (count < 1) throw std::runtime_error("slice of " + std::to_string(count) + " images: at least one is needed");
  if (first < 0) throw std::runtime_error("slice starts at image " + std::to_string(first) + ": must not be negative");
  if ((long long)first + count > B)
    throw std::runtime_error("slice of images " + std::to_string(first) + ".." +
                             std::to_string((long long)first + count - 1) + " of ciphertext " + std::to_string(id) +
                             ", whose batch is " + std::to_string(B));
  std::vector<GatherSrc> src;
  std::shared_ptr<Buffer> keep = a.poly.buf;
  Context::gather_sources(a, first, count, src);
  Ciphertext out = c.new_ct(a.level, count, a.scale);
  c.gather(out, src);
  return c.cts.add(std::move(out));
  API_END(-1)
}

// ---- keys ----
void NewKeyGenerator(void) {}
void GenerateSecretKey(void) {
  API_BEGIN
  ctx().gen_secret();
  API_END_VOID
}
void GeneratePublicKey(void) {
  API_BEGIN
  ctx().gen_public();
  API_END_VOID
}
void GenerateRelinearizationKey(void) {
  API_BEGIN
  ctx().gen_relin();
  API_END_VOID
}
void GenerateEvaluationKeys(void) {}

// ---- Lattigo v6 wire formats (wire.h): rlwe.SecretKey = ringqp.Poly ----
static std::vector<u64> mods_of(const Context& c, int nq, bool with_p) {
  std::vector<u64> m(c.mods.begin(), c.mods.begin() + nq);
  if (with_p) m.insert(m.end(), c.mods.begin() + c.L, c.mods.begin() + c.L + c.K);
  return m;
}
// ringqp.Poly of a [nq + K][N] host block: ring.Poly Q (nq limbs), ring.Poly P (K limbs)
static void put_qp(std::vector<char>& b, const Context& c, const u64* data, int nq) {
  wire::put_poly(b, data, mods_of(c, nq, false), c.N);
  std::vector<u64> pm(c.mods.begin() + c.L, c.mods.begin() + c.L + c.K);
  wire::put_poly(b, data + (size_t)nq * c.N, pm, c.N);
}
static void get_qp(wire::Reader& rd, const Context& c, u64* out, int nq, const char* what) {
  rd.get_poly(out, mods_of(c, nq, false), c.N, what);
  std::vector<u64> pm(c.mods.begin() + c.L, c.mods.begin() + c.L + c.K);
  rd.get_poly(out + (size_t)nq * c.N, pm, c.N, what);
}
static ArrayResultByte to_bytes(const std::vector<char>& v) {
  ArrayResultByte r{nullptr, 0};
  r.Data = to_c_array<char, char>(v, &r.Length);
  return r;
}
// rlwe.GaloisKey: GaloisElement, NthRoot, GadgetCiphertext{BaseTwoDecomposition 0,
// Value: beta x 1 VectorQP (k0, k1)} of a [beta][2][level+1+K][N] host key made
// for `level` (Lattigo's key at LevelQ = level: beta rows, level+1 Q limbs)
static std::vector<char> galois_key_bytes(const Context& c, u64 galEl, const std::vector<u64>& key, int level) {
  std::vector<char> b;
  const int beta = (level + 1 + c.K - 1) / c.K;
  const size_t qp = (size_t)(level + 1 + c.K) * c.N;
  b.reserve(40 + (size_t)beta * (16 + 2 * (wire::poly_bytes(level + 1, c.N) + wire::poly_bytes(c.K, c.N))));
  wire::put_u64(b, galEl);
  wire::put_u64(b, c.nthroot);  // NthRoot
  wire::put_u64(b, 0);             // BaseTwoDecomposition
  wire::put_u64(b, (u64)beta);     // Matrix rows
  for (int i = 0; i < beta; ++i) {
    wire::put_u64(b, 1);  // one column (no power-of-two decomposition)
    wire::put_u64(b, 2);  // VectorQP length
    for (int k = 0; k < 2; ++k) put_qp(b, c, key.data() + (2 * (size_t)i + k) * qp, level + 1);
  }
  return b;
}

ArrayResultByte SerializeSecretKey(void) {
  ArrayResultByte r{nullptr, 0};
  API_BEGIN
  Context& c = ctx();
  if (!c.have_sk) throw std::runtime_error("secret key not generated");
  std::vector<u64> host;
  c.download(c.sk, host);
  std::vector<char> bytes;
  put_qp(bytes, c, host.data(), c.L);
  return to_bytes(bytes);
  API_END(r)
}
void LoadSecretKey(char* data, unsigned long len) {
  API_BEGIN
  Context& c = ctx();
  if (!data) throw std::runtime_error("null secret key data");
  wire::Reader rd(data, len);
  std::vector<u64> host((size_t)(c.L + c.K) * c.N);
  get_qp(rd, c, host.data(), c.L, "secret key");
  if (rd.left()) throw std::runtime_error("secret key blob has trailing bytes");
  c.sk = c.alloc(1, c.L + c.K, 1);
  c.upload(c.sk, host);
  c.have_sk = true;
  API_END_VOID
}

// ---- encoder / encryptor ----
void NewEncoder(void) {}
// enc_crt_kernel converts |x| * scale + 0.5 to u64: defined only for a finite scale > 0
static void check_encode_scale(double scale) {
  if (!(scale > 0) || !std::isfinite(scale)) throw std::runtime_error("scale must be finite and positive");
}
int Encode(float* values, int n, int level, unsigned long scale) {
  API_BEGIN
  Context& c = ctx();
  if (level < 0 || level >= c.L) throw std::runtime_error("invalid level");
  check_encode_scale((double)scale);
  return c.pts.add(c.encode(values, n, 1, level, (long double)scale, false));
  API_END(-1)
}
int EncodeBatch(float* values, int n, int B, int level, unsigned long scale) {
  API_BEGIN
  Context& c = ctx();
  if (level < 0 || level >= c.L || B < 1) throw std::runtime_error("invalid level/batch");
  check_encode_scale((double)scale);
  return c.pts.add(c.encode(values, n, B, level, (long double)scale, false));
  API_END(-1)
}
int EncodeBatchDevice(const float* dvalues, int n, int B, int level, double scale) {
  API_BEGIN
  Context& c = ctx();
  if (level < 0 || level >= c.L || B < 1 || !dvalues) throw std::runtime_error("invalid level/batch/pointer");
  check_encode_scale(scale);
  return c.pts.add(c.encode_dev(dvalues, n, B, level, (long double)scale, false));
  API_END(-1)
}
int DecodeDevice(int pt, double* dout) {
  API_BEGIN
  Context& c = ctx();
  if (!dout) throw std::runtime_error("null output pointer");
  c.decode_dev(c.pts.get(pt), dout);
  return 0;
  API_END(-1)
}
int DecodeF64(int pt, double* out, unsigned long n) {
  API_BEGIN
  Context& c = ctx();
  const Plaintext& p = c.pts.get(pt);
  if (n < (unsigned long)p.poly.B * (c.slots)) throw std::runtime_error("output buffer too small");
  std::vector<double> v = c.decode(p);
  memcpy(out, v.data(), v.size() * sizeof(double));
  return 0;
  API_END(-1)
}
ArrayResultFloat Decode(int id) {
  ArrayResultFloat r{nullptr, 0};
  API_BEGIN
  Context& c = ctx();
  std::vector<double> v = c.decode(c.pts.get(id));
  r.Data = to_c_array<double, float>(v, &r.Length);
  return r;
  API_END(r)
}
void NewEncryptor(void) {}
void NewDecryptor(void) {}
int Encrypt(int pt) {
  API_BEGIN
  Context& c = ctx();
  return c.cts.add(c.encrypt(c.pts.get(pt)));
  API_END(-1)
}
int Decrypt(int ct) {
  API_BEGIN
  Context& c = ctx();
  return c.pts.add(c.decrypt(c.cts.get(ct)));
  API_END(-1)
}

// ---- evaluator ----
void NewEvaluator(void) {
  API_BEGIN
  Context& c = ctx();
  for (int i = 1; i < c.slots; i *= 2) c.gen_galois(c.galois_element(i), c.L - 1);  // evaluator.go:25-31
  API_END_VOID
}
void AddRotationKey(int k) {
  API_BEGIN
  Context& c = ctx();
  c.gen_galois(c.galois_element(k), c.L - 1);
  API_END_VOID
}
unsigned long GaloisElement(int k) {
  API_BEGIN
  return ctx().galois_element(k);
  API_END(0)
}

int Negate(int id) {
  API_BEGIN
  Context& c = ctx();
  Ciphertext& a = c.cts.get(id);
  Ciphertext o = c.new_ct(a.level, a.poly.B, a.scale);
  c.ew1(EW_NEG, c.lsq(o.poly, 0, 2, a.level), c.lsq(a.poly, 0, 2, a.level));
  return c.cts.add(std::move(o));
  API_END(-1)
}
int Rotate(int id, int k) {
  API_BEGIN
  Context& c = ctx();
  Ciphertext& a = c.inplace_ct(id, false);  // the rotation replaces a (buffer and copy-on-write share)
  a = c.rotate(a, k);
  return id;
  API_END(-1)
}
int RotateNew(int id, int k) {
  API_BEGIN
  Context& c = ctx();
  Ciphertext& a = c.cts.get(id);
  if (!c.tun.defer) return c.cts.add(c.rotate(a, k));
  // deferred (deferral.h): the key is made (or checked) now, so a
  // missing key fails here as in the op-by-op path; r gets no buffer yet
  c.galois_key(c.galois_element(k), a.level);
  Ciphertext r;
  r.level = a.level;
  r.scale = a.scale;
  r.poly.B = a.poly.B;
  const int rid = c.cts.add(std::move(r));
  defer_apply(c, {deferral::Ev::OpenRotation, id, rid, k});
  return rid;
  API_END(-1)
}
int OrionHipRotateAdd(int id, int k) {
  API_BEGIN
  Context& c = ctx();
  c.rotate_add_inplace(c.inplace_ct(id), k);
  return id;
  API_END(-1)
}
// ---- hoisted rotations (orion_hip.h; Context::rotate_hoisted, rotate_sum) ----
// the checks both calls share; the Galois elements of the amounts into gs
static const Ciphertext& hoist_source(Context& c, int ct, const int* amounts, int n, std::vector<u64>& gs) {
  if (!amounts) throw std::runtime_error("null amount list");
  if (n < 1 || n > ORION_MAXGROUP)
    throw std::runtime_error("cannot rotate by " + std::to_string(n) + " amounts in one call: 1 to " +
                             std::to_string(ORION_MAXGROUP) + " are accepted");
  const Ciphertext& a = c.cts.get(ct);
  if (!a.poly.ptr() || a.poly.ncomp < 2 || a.poly.nlimb < a.level + 1)
    throw std::runtime_error("ciphertext " + std::to_string(ct) + " holds no degree-1 polynomial pair");
  for (int i = 0; i < n; ++i) gs.push_back(c.galois_element(amounts[i]));
  return a;
}
int OrionHipRotateHoisted(int ct, const int* amounts, int n, int* out) {
  API_BEGIN
  Context& c = ctx();
  if (!out) throw std::runtime_error("null output list");
  std::vector<u64> gs;
  const Ciphertext& a = hoist_source(c, ct, amounts, n, gs);
  std::shared_ptr<Buffer> keep = a.poly.buf;  // the operand's buffer, until the launches are queued
  std::vector<Ciphertext> r = c.rotate_hoisted(a, gs);
  for (int i = 0; i < n; ++i) out[i] = c.cts.add(std::move(r[i]));
  return 0;
  API_END(-1)
}
int OrionHipRotateSum(int ct, const int* amounts, int n) {
  API_BEGIN
  Context& c = ctx();
  std::vector<u64> gs;
  const Ciphertext& a = hoist_source(c, ct, amounts, n, gs);
  std::shared_ptr<Buffer> keep = a.poly.buf;  // the operand's buffer, until the launches are queued
  return c.cts.add(c.rotate_sum(a, gs));
  API_END(-1)
}
// Rescale / RescaleNew of handle id: when its ModDown is what is pending,
// both run as one division by P q_l
static Ciphertext& rescale_handle(Context& c, int id) {
  const bool merged = defer_apply(c, {deferral::Ev::Rescale, id}) == deferral::Act::ModDownRescale;
  Ciphertext& a = c.inplace_ct(id);
  if (!merged) c.rescale_inplace(a);
  return a;
}
int Rescale(int id) {
  API_BEGIN
  Context& c = ctx();
  rescale_handle(c, id);
  return id;
  API_END(-1)
}
int RescaleNew(int id) {  // evaluator.go:92-99: rescales the input in place, returns a copy
  API_BEGIN
  Context& c = ctx();
  Ciphertext& a = rescale_handle(c, id);
  return c.cts.add(c.alias(a));  // copy-on-write: the copy is made only if both are later written
  API_END(-1)
}

// evaluator.py:30-41 (the fork's HEonGPU-only mod_drop): drop the top modulus
// in place, scale unchanged; returns the input id
int ModDropCiphertext(int id) {
  API_BEGIN
  Ciphertext& a = ctx().inplace_ct(id);
  if (a.level < 1) throw std::runtime_error("cannot drop the last modulus");
  a.level -= 1;
  return id;
  API_END(-1)
}

static Ciphertext add_scalar(Context& c, const Ciphertext& a, float v, Ciphertext* dst) {
  std::vector<u64> k = c.scaled_const_residues(v, a.scale, a.level);
  Ciphertext o = dst ? Ciphertext() : c.new_ct(a.level, a.poly.B, a.scale);
  Ciphertext& out = dst ? *dst : o;
  c.ew1(EW_ADDC, c.lsq(out.poly, 0, 1, a.level), c.lsq(a.poly, 0, 1, a.level), &k);
  if (!dst) c.copy(c.lsq(out.poly, 1, 1, a.level), c.lsq(a.poly, 1, 1, a.level));
  return o;
}
int AddScalar(int id, float v) {
  API_BEGIN
  Context& c = ctx();
  Ciphertext& a = c.inplace_ct(id);
  add_scalar(c, a, v, &a);
  return id;
  API_END(-1)
}
int AddScalarNew(int id, float v) {
  API_BEGIN
  Context& c = ctx();
  return c.cts.add(add_scalar(c, c.cts.get(id), v, nullptr));
  API_END(-1)
}
int SubScalar(int id, float v) { return AddScalar(id, -v); }
int SubScalarNew(int id, float v) { return AddScalarNew(id, -v); }

static void mul_const(Context& c, const Ciphertext& a, Ciphertext& out, const std::vector<u64>& k) {
  c.ew1(EW_SCALE, c.lsq(out.poly, 0, 2, a.level), c.lsq(a.poly, 0, 2, a.level), &k);
}
int MulScalarInt(int id, int v) {
  API_BEGIN
  Context& c = ctx();
  Ciphertext& a = c.inplace_ct(id);
  mul_const(c, a, a, c.const_residues((long double)v, a.level));
  return id;
  API_END(-1)
}
int MulScalarIntNew(int id, int v) {
  API_BEGIN
  Context& c = ctx();
  Ciphertext& a = c.cts.get(id);
  Ciphertext o = c.new_ct(a.level, a.poly.B, a.scale);
  mul_const(c, a, o, c.const_residues((long double)v, a.level));
  return c.cts.add(std::move(o));
  API_END(-1)
}
// non-integral constants are scaled by q_level (Lattigo getConstantAndScale)
static void mul_float(Context& c, const Ciphertext& a, Ciphertext& out, float v) {
  const double dv = (double)v;
  if (dv == floor(dv)) {
    mul_const(c, a, out, c.scaled_const_residues(v, 1.0L, a.level));
    out.scale = a.scale;
    return;
  }
  const long double ql = (long double)c.mods[a.level];
  mul_const(c, a, out, c.scaled_const_residues(v, ql, a.level));
  out.scale = a.scale * ql;
}
int MulScalarFloat(int id, float v) {
  API_BEGIN
  Context& c = ctx();
  Ciphertext& a = c.inplace_ct(id);
  mul_float(c, a, a, v);
  return id;
  API_END(-1)
}
int MulScalarFloatNew(int id, float v) {
  API_BEGIN
  Context& c = ctx();
  Ciphertext& a = c.cts.get(id);
  Ciphertext o = c.new_ct(a.level, a.poly.B, a.scale);
  mul_float(c, a, o, v);
  return c.cts.add(std::move(o));
  API_END(-1)
}

// The ciphertext side of a binary op, resolved against the other operand's
// level and batch: a (made writable when in place), the result's level and
// batch, and where the result goes -- a itself, or a new ciphertext that
// done() registers
struct BinaryOp {
  Context& c;
  const int id;
  const bool inplace;
  Ciphertext& a;
  const int level, B;
  Ciphertext o;
  BinaryOp(Context& c_, int id_, int other_level, int other_B, bool inplace_)
      : c(c_), id(id_), inplace(inplace_), a(inplace_ ? c_.inplace_ct(id_) : c_.cts.get(id_)),
        level(std::min(a.level, other_level)), B(c_.batch_of(a.poly.B, other_B)) {
    if (inplace && B != a.poly.B) throw std::runtime_error("in-place op cannot grow the batch");
    if (!inplace) o = c.new_ct(level, B, a.scale);
  }
  Ciphertext& out() { return inplace ? a : o; }
  int done() { return inplace ? id : c.cts.add(std::move(o)); }
};
// ct (+/-) pt
static int ct_pt_op(int id, int pid, int op, bool inplace) {
  Context& c = ctx();
  const Plaintext& p = c.pts.get(pid);
  BinaryOp r(c, id, p.level, p.poly.B, inplace);
  r.out().level = r.level;
  c.add_like(r.out(), r.a, c.lsq(p.poly, 0, 1, r.level, r.B), p.scale, op);
  return r.done();
}
int AddPlaintext(int id, int pt) {
  API_BEGIN
  return ct_pt_op(id, pt, EW_ADD, true);
  API_END(-1)
}
int AddPlaintextNew(int id, int pt) {
  API_BEGIN
  return ct_pt_op(id, pt, EW_ADD, false);
  API_END(-1)
}
int SubPlaintext(int id, int pt) {
  API_BEGIN
  return ct_pt_op(id, pt, EW_SUB, true);
  API_END(-1)
}
int SubPlaintextNew(int id, int pt) {
  API_BEGIN
  return ct_pt_op(id, pt, EW_SUB, false);
  API_END(-1)
}
static int ct_pt_mul(int id, int pid, bool inplace) {
  Context& c = ctx();
  const Plaintext& p = c.pts.get(pid);
  BinaryOp r(c, id, p.level, p.poly.B, inplace);
  LimbSet lp = c.lsq(p.poly, 0, 1, r.level, r.B);
  lp.ncomp = 2;
  lp.comp_stride = 0;
  c.ew(EW_MUL, c.lsq(r.out().poly, 0, 2, r.level), c.lsq(r.a.poly, 0, 2, r.level, r.B), lp);
  r.out().level = r.level;
  r.out().scale = r.a.scale * p.scale;
  return r.done();
}
int MulPlaintext(int id, int pt) {
  API_BEGIN
  return ct_pt_mul(id, pt, true);
  API_END(-1)
}
int MulPlaintextNew(int id, int pt) {
  API_BEGIN
  return ct_pt_mul(id, pt, false);
  API_END(-1)
}
static int ct_ct_op(int i0, int i1, int op, bool inplace) {
  Context& c = ctx();
  const Ciphertext& b = c.cts.get(i1);
  BinaryOp r(c, i0, b.level, b.poly.B, inplace);
  r.out().level = r.level;
  c.add_like(r.out(), r.a, c.lsq(b.poly, 0, 2, r.level, r.B), b.scale, op);
  return r.done();
}
int AddCiphertext(int a, int b) {
  API_BEGIN
  Context& c = ctx();
  // x += (pending) Rotate(x, k) is only recorded
  if (defer_apply(c, {deferral::Ev::Add, a, b}) == deferral::Act::RecordAdd) return a;
  return ct_ct_op(a, b, EW_ADD, true);
  API_END(-1)
}
int AddCiphertextNew(int a, int b) {
  API_BEGIN
  return ct_ct_op(a, b, EW_ADD, false);
  API_END(-1)
}
int SubCiphertext(int a, int b) {
  API_BEGIN
  return ct_ct_op(a, b, EW_SUB, true);
  API_END(-1)
}
int SubCiphertextNew(int a, int b) {
  API_BEGIN
  return ct_ct_op(a, b, EW_SUB, false);
  API_END(-1)
}
int MulRelinCiphertext(int a, int b) {
  API_BEGIN
  Context& c = ctx();
  c.inplace_ct(a, false);  // the product replaces a (buffer and copy-on-write share)
  Ciphertext r = c.mul_relin(c.cts.get(a), c.cts.get(b));
  if (r.poly.B != c.cts.get(a).poly.B) throw std::runtime_error("in-place op cannot grow the batch");
  c.cts.get(a) = std::move(r);
  return a;
  API_END(-1)
}
int MulRelinCiphertextNew(int a, int b) {
  API_BEGIN
  Context& c = ctx();
  Ciphertext r = c.mul_relin(c.cts.get(a), c.cts.get(b), true);
  const bool pend = (bool)r.pend.buf;
  const int rid = c.cts.add(std::move(r));
  if (pend) defer_apply(c, {deferral::Ev::OpenModDown, rid});
  return rid;
  API_END(-1)
}
// sum_i a[i] x b[i], relinearised once (orion_hip.h; Context::mul_relin_sum)
int OrionHipMulRelinSum(const int* a, const int* b, int n) {
  API_BEGIN
  Context& c = ctx();
  if (!a || !b) throw std::runtime_error("null handle list");
  if (n < 1)
    throw std::runtime_error("cannot sum " + std::to_string(n) + " ciphertext products: at least one pair is needed");
  if (!c.have_rlk) throw std::runtime_error("relinearization key not generated");
  // every operand is looked up (and checked) before anything is allocated; an
  // operand of another context orders this stream after its producer (cts.get)
  std::vector<const Ciphertext*> A(n), Bv(n);
  std::vector<std::shared_ptr<Buffer>> keep;  // the operands' buffers, until the launches are queued
  int level = 0, B = 1, bid = -1;
  long double scale = 0;
  for (int i = 0; i < n; ++i) {
    A[i] = &c.cts.get(a[i]);
    Bv[i] = &c.cts.get(b[i]);
    for (int side = 0; side < 2; ++side) {
      const Ciphertext& x = side ? *Bv[i] : *A[i];
      const int id = side ? b[i] : a[i];
      if (!x.poly.ptr() || x.poly.ncomp < 2 || x.poly.nlimb < x.level + 1)
        throw std::runtime_error("ciphertext " + std::to_string(id) + " holds no degree-1 polynomial pair");
      level = i == 0 && side == 0 ? x.level : std::min(level, x.level);
      if (x.poly.B != 1) {
        if (B != 1 && x.poly.B != B)
          throw std::runtime_error("cannot sum products of ciphertexts " + std::to_string(bid) + " (batch " +
                                   std::to_string(B) + ") and " + std::to_string(id) + " (batch " +
                                   std::to_string(x.poly.B) + "): the batches differ");
        if (B == 1) B = x.poly.B, bid = id;
      }
      keep.push_back(x.poly.buf);
    }
    const long double si = A[i]->scale * Bv[i]->scale;
    if (i == 0)
      scale = si;
    else if (si != scale)
      throw std::runtime_error("cannot sum ciphertext products: pair " + std::to_string(i) + " (" +
                               std::to_string(a[i]) + " x " + std::to_string(b[i]) + ") has scale " + scale_str(si) +
                               ", pair 0 (" + std::to_string(a[0]) + " x " + std::to_string(b[0]) + ") has scale " +
                               scale_str(scale) + ": the scales differ");
  }
  Ciphertext r = c.mul_relin_sum(A, Bv, level, B, scale, true);
  const bool pend = (bool)r.pend.buf;
  const int rid = c.cts.add(std::move(r));
  if (pend) defer_apply(c, {deferral::Ev::OpenModDown, rid});
  return rid;
  API_END(-1)
}

// ---- complex packing (orion_hip.h; Context::pack_complex) ----
static const Ciphertext& complex_operand(Context& c, int id) {
  const Ciphertext& x = c.cts.get(id);
  if (!x.poly.ptr() || x.poly.ncomp < 2 || x.poly.nlimb < x.level + 1)
    throw std::runtime_error("ciphertext " + std::to_string(id) + " holds no degree-1 polynomial pair");
  return x;
}
int OrionHipConjugateNew(int ct) {
  API_BEGIN
  Context& c = ctx();
  c.need_complex();
  const Ciphertext& a = complex_operand(c, ct);
  std::shared_ptr<Buffer> keep = a.poly.buf;  // the operand's buffer, until the launches are queued
  return c.cts.add(c.apply_galois(a, 2 * (u64)c.N - 1));
  API_END(-1)
}
int OrionHipPackComplex(int a, int b) {
  API_BEGIN
  Context& c = ctx();
  c.need_complex();
  const Ciphertext &x = complex_operand(c, a), &y = complex_operand(c, b);
  if (x.poly.B != y.poly.B)
    throw std::runtime_error("cannot pack ciphertexts " + std::to_string(a) + " (batch " + std::to_string(x.poly.B) +
                             ") and " + std::to_string(b) + " (batch " + std::to_string(y.poly.B) +
                             "): the batches differ");
  if (x.scale != y.scale)
    throw std::runtime_error("cannot pack ciphertexts " + std::to_string(a) + " (scale " + scale_str(x.scale) +
                             ") and " + std::to_string(b) + " (scale " + scale_str(y.scale) + "): the scales differ");
  std::shared_ptr<Buffer> keep[2] = {x.poly.buf, y.poly.buf};
  return c.cts.add(c.pack_complex(x, y));
  API_END(-1)
}
int OrionHipUnpackComplex(int ct, int* out2) {
  API_BEGIN
  Context& c = ctx();
  c.need_complex();
  if (!out2) throw std::runtime_error("null output handle pair");
  const Ciphertext& a = complex_operand(c, ct);
  std::shared_ptr<Buffer> keep = a.poly.buf;
  std::pair<Ciphertext, Ciphertext> r = c.unpack_complex(a);
  out2[0] = c.cts.add(std::move(r.first));
  out2[1] = c.cts.add(std::move(r.second));
  return 0;
  API_END(-1)
}

// ---- monomial packing and the slot trace (orion_hip.h; Context::pack_monomials, slot_trace) ----
int OrionHipPackMonomials(int ct, int g) {
  API_BEGIN
  Context& c = ctx();
  const Ciphertext& a = complex_operand(c, ct);
  std::shared_ptr<Buffer> keep = a.poly.buf;  // the operand's buffer, until the launches are queued
  return c.cts.add(c.pack_monomials(a, g));
  API_END(-1)
}
int OrionHipUnpackMonomials(int ct, int g, int B) {
  API_BEGIN
  Context& c = ctx();
  const Ciphertext& a = complex_operand(c, ct);
  std::shared_ptr<Buffer> keep = a.poly.buf;
  return c.cts.add(c.unpack_monomials(a, g, B));
  API_END(-1)
}
int OrionHipSlotTraceNew(int ct, int slots, int mean) {
  API_BEGIN
  Context& c = ctx();
  const Ciphertext& a = complex_operand(c, ct);
  std::shared_ptr<Buffer> keep = a.poly.buf;
  return c.cts.add(c.slot_trace(a.poly, a.level, a.scale, slots, mean != 0));
  API_END(-1)
}

// ---- linear transforms ----
void NewLinearTransformEvaluator(void) {}

static void bsgs_split(int rot, int slots, int N1, int* giant, int* baby) {
  rot &= (slots - 1);
  *giant = ((rot / N1) * N1) & (slots - 1);
  *baby = rot & (N1 - 1);
}
// Lattigo lintrans FindBestBSGSRatio
static int find_best_n1(const std::vector<int>& idx, int slots, int logMaxRatio) {
  const double maxRatio = (double)(1 << logMaxRatio);
  for (int N1 = 1; N1 < slots; N1 <<= 1) {
    std::set<int> gs, bs;
    for (int d : idx) {
      int gi, bi;
      bsgs_split(d, slots, N1, &gi, &bi);
      gs.insert(gi);
      bs.insert(bi);
    }
    const double r = (double)((int)bs.size() - 1) / (double)((int)gs.size() - 1);
    if (r == maxRatio) return N1;
    if (r > maxRatio) return N1 / 2;
  }
  return 1;
}
// the BSGS index of a new transform from its index list (T.idx) and log-ratio:
// N1, the sorted giants, the babies in first-seen order; returns each
// diagonal's giant amount
static std::vector<int> lt_bsgs_index(LinTrans& T, int slots, int logRatio) {
  T.N1 = find_best_n1(T.idx, slots, logRatio);
  std::vector<int> giant_of;
  std::set<int> gs, bs;
  for (int d : T.idx) {
    int gi, bi;
    bsgs_split(d, slots, T.N1, &gi, &bi);
    giant_of.push_back(gi);
    gs.insert(gi);
    if (bs.insert(bi).second) T.babies.push_back(bi);
  }
  T.giants.assign(gs.begin(), gs.end());
  return giant_of;
}

int GenerateLinearTransform(int* diagIdx, int nIdx, float* data, int nData, int level, float ratio,
                            char* ioMode) {
  API_BEGIN
  Context& c = ctx();
  // lineartransform.go:79-88: in "load" mode the diagonals were serialised
  // earlier and arrive through LoadPlaintextDiagonal, so none is encoded here
  const bool load = ioMode && std::string(ioMode) == "load";
  const int slots = c.slots;
  if (!load && (long)nIdx * slots != (long)nData) throw std::runtime_error("diagonal data length != nIdx * slots");
  if (level < 0 || level >= c.L) throw std::runtime_error("invalid level");
  LinTrans T;
  T.level = level;
  T.ratio = ratio;
  T.uid = g_birth.fetch_add(1);
  T.idx.assign(diagIdx, diagIdx + nIdx);
  const int logRatio = (int)log((double)ratio);  // lineartransform.go:67 (natural log)
  if (logRatio < 0) throw std::runtime_error("naive (non-BSGS) linear transforms are not supported");
  const std::vector<int> giant_of = lt_bsgs_index(T, slots, logRatio);
  for (int r : T.giants)
    if (r) c.key_hint[c.galois_element(r)] = std::max(c.key_hint[c.galois_element(r)], level);
  for (int r : T.babies)
    if (r) c.key_hint[c.galois_element(r)] = std::max(c.key_hint[c.galois_element(r)], level);
  std::vector<float> vec(slots);
  for (int i = 0; i < nIdx && !load; ++i) {
    const int gi = giant_of[i];
    const float* v = data + (size_t)i * slots;
    for (int s = 0; s < slots; ++s) vec[s] = v[((s - gi) % slots + slots) % slots];  // rotate right by giant
    T.diags[diagIdx[i] & (slots - 1)] = c.encode(vec.data(), slots, 1, level, (long double)c.mods[level], true);
  }
  return c.lts.add(std::move(T));
  API_END(-1)
}

int GetLinearTransformN1(int id) {
  API_BEGIN_HANDLE(id)
  return ctx().lts.get(id).N1;
  API_END(-1)
}

// A device plan that is not built (the diagonals changed after the pipelines
// were made) is built by the context that owns the handle, under its lock --
// only a lower-index context may be waited on (lock order).  what: the kind of
// handle, for the error
static void owner_builds(Context& c, int id, const char* what, const std::function<void(Context&)>& build) {
  Context* o = handle_ctx(id);
  if (!o || o == &c) return build(c);
  if (o->index > c.index)
    throw std::runtime_error(std::string(what) + " " + std::to_string(id) + " of pipeline " +
                             std::to_string(o->index) + " has no device plan yet: evaluate it there first");
  std::lock_guard<std::recursive_mutex> lk(o->mu);
  build(*o);
}
// a transform about to be evaluated: its diagonals loaded, its device plan built
static void lt_ready(Context& c, LinTrans& T, int tid) {
  c.lt_loaded(T);
  if (T.plan_dirty)
    owner_builds(c, tid, "linear transform", [&T](Context& o) {
      if (T.plan_dirty) o.build_plan(T);
    });
}
int EvaluateLinearTransform(int tid, int cid) {
  API_BEGIN
  Context& c = ctx();
  LinTrans& T = c.lts.get(tid);
  lt_ready(c, T, tid);
  Ciphertext r = c.eval_lt(T, c.cts.get(cid), true);
  const bool pend = (bool)r.pend.buf;
  const int rid = c.cts.add(std::move(r));
  if (pend) defer_apply(c, {deferral::Ev::OpenModDown, rid});
  return rid;
  API_END(-1)
}
void DeleteLinearTransform(int id) {
  API_BEGIN_HANDLE(id)
  ctx().lts.del(id);
  API_END_VOID
}

// ---- blocked linear transforms (lt_blocks.h, Context::eval_lt_blocks) ----
// the members of a blocked transform, each still the transform it was made of
// (handle ids are reused: LinTrans::uid), its diagonals loaded and its device
// plan built
static std::vector<LinTrans*> blocks_members(Context& c, const LtBlocks& Bk, int bid) {
  std::vector<LinTrans*> Ts;
  for (size_t k = 0; k < Bk.tids.size(); ++k) {
    const int tid = Bk.tids[k];
    LinTrans* T = c.lts.owner_pool(tid)->has(tid) ? &c.lts.get(tid) : nullptr;
    if (!T || T->uid != Bk.uids[k])
      throw std::runtime_error("blocked linear transform " + std::to_string(bid) + ": its member transform " +
                               std::to_string(tid) + " has been deleted");
    lt_ready(c, *T, tid);
    Ts.push_back(T);
  }
  return Ts;
}
int OrionHipNewLinearTransformBlocks(const int* tids, int rows, int cols) {
  API_BEGIN
  Context& c = ctx();
  if (!tids) throw std::runtime_error("null handle list");
  if (rows < 1 || cols < 1)
    throw std::runtime_error("a blocked linear transform of " + std::to_string(rows) + " x " + std::to_string(cols) +
                             " blocks: at least one row and one column are needed");
  LtBlocks Bk;
  Bk.rows = rows, Bk.cols = cols;
  std::vector<std::vector<lt_blocks::Pair>> pairs;
  for (int k = 0; k < rows * cols; ++k) {
    const LinTrans& T = c.lts.get(tids[k]);
    if (k == 0)
      Bk.level = T.level;
    else if (T.level != Bk.level)
      throw std::runtime_error("cannot block linear transforms " + std::to_string(tids[0]) + " (level " +
                               std::to_string(Bk.level) + ") and " + std::to_string(tids[k]) + " (level " +
                               std::to_string(T.level) + "): the levels differ");
    Bk.tids.push_back(tids[k]);
    Bk.uids.push_back(T.uid);
    pairs.push_back(c.lt_pairs(T));
  }
  Bk.lay.plan = lt_blocks::plan(pairs, rows, cols, LT_MAXB, LT_MAXG, LT_MAXSLOT);
  if (!Bk.lay.plan.error.empty()) throw std::runtime_error(Bk.lay.plan.error);
  c.build_blocks_plan(Bk, blocks_members(c, Bk, -1));
  return c.ltbs.add(std::move(Bk));
  API_END(-1)
}
int OrionHipEvaluateLinearTransformBlocks(int bid, const int* cids, int rescale, int* out) {
  API_BEGIN
  Context& c = ctx();
  if (!cids || !out) throw std::runtime_error("null handle list");
  LtBlocks& Bk = c.ltbs.get(bid);
  const std::vector<LinTrans*> Ts = blocks_members(c, Bk, bid);
  bool dirty = !Bk.built;
  for (size_t k = 0; k < Ts.size(); ++k) dirty = dirty || Ts[k]->rev != Bk.revs[k];
  if (dirty) owner_builds(c, bid, "blocked linear transform", [&](Context& o) { o.build_blocks_plan(Bk, Ts); });
  // every source is looked up (and checked) before anything is allocated
  std::vector<const Ciphertext*> cs;
  for (int j = 0; j < Bk.cols; ++j) {
    const Ciphertext& a = c.cts.get(cids[j]);
    const Ciphertext* f = j ? cs[0] : &a;
    const std::string both = "blocked linear transform " + std::to_string(bid) + ": ciphertexts " +
                             std::to_string(cids[0]) + " (";
    if (a.level != f->level)
      throw std::runtime_error(both + "level " + std::to_string(f->level) + ") and " + std::to_string(cids[j]) +
                               " (level " + std::to_string(a.level) + "): the levels differ");
    if (a.scale != f->scale)
      throw std::runtime_error(both + "scale " + scale_str(f->scale) + ") and " + std::to_string(cids[j]) +
                               " (scale " + scale_str(a.scale) + "): the scales differ");
    if (a.poly.B != f->poly.B)
      throw std::runtime_error(both + "batch " + std::to_string(f->poly.B) + ") and " + std::to_string(cids[j]) +
                               " (batch " + std::to_string(a.poly.B) + "): the batches differ");
    cs.push_back(&a);
  }
  std::vector<Ciphertext> rows = c.eval_lt_blocks(Bk, Ts, cs, rescale != 0);
  for (int i = 0; i < Bk.rows; ++i) out[i] = c.cts.add(std::move(rows[i]));
  return 0;
  API_END(-1)
}
void OrionHipDeleteLinearTransformBlocks(int id) {
  API_BEGIN_HANDLE(id)
  ctx().ltbs.del(id);
  API_END_VOID
}
ArrayResultInt GetLinearTransformRotationKeys(int id) {
  ArrayResultInt r{nullptr, 0};
  API_BEGIN
  Context& c = ctx();
  const LinTrans& T = c.lts.get(id);
  std::vector<int> rots(T.giants.begin(), T.giants.end());
  for (int b : T.babies)
    if (std::find(rots.begin(), rots.end(), b) == rots.end()) rots.push_back(b);
  std::vector<int> gels;
  for (int k : rots) gels.push_back((int)c.galois_element(k));
  r.Data = to_c_array<int, int>(gels, &r.Length);
  return r;
  API_END(r)
}
// keys asked for by a linear transform are made for the highest level of the
// transforms that use them (key_hint); any other element gets a full-chain key
void GenerateLinearTransformRotationKey(int galEl) {
  API_BEGIN
  Context& c = ctx();
  const u64 g = (u64)(unsigned)galEl;
  if (g != 1) c.gen_galois(g, c.hinted_level(g));  // 1 = the identity (zero rotation): no key needed
  API_END_VOID
}
void GenerateConsolidatedRotationKeys(int* galEls, int n) {
  API_BEGIN
  Context& c = ctx();
  for (int i = 0; i < n; ++i) {
    const u64 g = (u64)(unsigned)galEls[i];
    if (g != 1) c.gen_galois(g, c.hinted_level(g));
  }
  API_END_VOID
}
// lineartransform.go:131-142: a fresh key, serialised and NOT kept (the
// save path stores it to HDF5 and LoadRotationKey brings it back per layer).
// Like Lattigo's GenGaloisKeyNew the blob is a full-chain key (every digit over
// every Q limb); LoadRotationKey scopes it to the level its transforms need.
ArrayResultByte GenerateAndSerializeRotationKey(int galEl) {
  ArrayResultByte r{nullptr, 0};
  API_BEGIN
  Context& c = ctx();
  const u64 g = (u64)(unsigned)galEl;
  auto kept = c.gks.find(g);
  EvKey saved;
  if (kept != c.gks.end()) {
    saved = kept->second;
    c.gks.erase(kept);
  }
  const int level = c.L - 1;
  c.gen_galois(g, level);
  std::vector<u64> host;
  c.download(c.gks.at(g).k, host);
  c.gks.erase(g);
  if (saved.k.buf) c.gks[g] = saved;
  return to_bytes(galois_key_bytes(c, g, host, level));
  API_END(r)
}
// lineartransform.go:145-164: unmarshal an rlwe.GaloisKey into the key set under
// galEl.  A key asked for by a linear transform is kept only over the limbs and
// digits of the highest level that uses it (key_hint): the digits 0..beta-1 of
// a key made for a higher level, restricted to q_0..q_level and P, are exactly
// the key Lattigo's gadget product reads at that level.
void LoadRotationKey(char* data, unsigned long len, unsigned long galEl) {
  API_BEGIN
  Context& c = ctx();
  if (!data) throw std::runtime_error("null rotation key data");
  wire::Reader rd(data, len);
  const u64 ge = rd.get_u64(), nth = rd.get_u64(), b2 = rd.get_u64(), rows = rd.get_u64();
  if (nth != c.nthroot) throw std::runtime_error("rotation key: NthRoot does not match the ring");
  if (b2 != 0) throw std::runtime_error("rotation key: power-of-two decomposition is not supported");
  if (ge != galEl) throw std::runtime_error("rotation key: blob is for Galois element " + std::to_string(ge));
  if (rows < 1 || rows > (u64)c.dnum) throw std::runtime_error("rotation key: gadget rows outside 1..dnum");
  if (rd.get_u64() != 1 || rd.get_u64() != 2) throw std::runtime_error("rotation key: unexpected gadget shape");
  // the level the key was made for: its Q limb count (peeked from the first ring.Poly)
  const u64 nq = rd.get_u64();
  if (nq < 1 || nq > (u64)c.L) throw std::runtime_error("rotation key: Q limb count outside the chain");
  const int level = (int)nq - 1, beta = (level + 1 + c.K - 1) / c.K;
  if (rows != (u64)beta) throw std::runtime_error("rotation key: gadget rows do not match its level");
  wire::Reader body(data + 48, len - 48);  // past the 4-word header and row 0's column/vector lengths
  const size_t qp = (size_t)(level + 1 + c.K) * c.N;
  std::vector<u64> host(2 * (size_t)beta * qp);
  for (int i = 0; i < beta; ++i) {
    if (i && (body.get_u64() != 1 || body.get_u64() != 2))
      throw std::runtime_error("rotation key: unexpected gadget shape");
    for (int k = 0; k < 2; ++k) get_qp(body, c, host.data() + (2 * (size_t)i + k) * qp, level + 1, "rotation key");
  }
  if (body.left()) throw std::runtime_error("rotation key blob has trailing bytes");
  const int tl = std::min(level, c.hinted_level(galEl)), tbeta = (tl + 1 + c.K - 1) / c.K;
  if (tl < level) {  // keep digits < tbeta over limbs q_0..q_tl, p_0..p_{K-1}
    const size_t tqp = (size_t)(tl + 1 + c.K) * c.N;
    std::vector<u64> sc(2 * (size_t)tbeta * tqp);
    for (int r = 0; r < 2 * tbeta; ++r) {
      const u64* src = host.data() + (size_t)r * qp;
      u64* dst = sc.data() + (size_t)r * tqp;
      memcpy(dst, src, sizeof(u64) * (size_t)(tl + 1) * c.N);
      memcpy(dst + (size_t)(tl + 1) * c.N, src + (size_t)(level + 1) * c.N, sizeof(u64) * (size_t)c.K * c.N);
    }
    // the whole key stays in host memory (as Lattigo keeps it,
    // lineartransform.go:143-159): a later use above tl uploads it whole
    c.gk_host[galEl] = Context::HostKey{level, std::make_shared<const std::vector<u64>>(std::move(host))};
    host = std::move(sc);
  } else {
    c.gk_host.erase(galEl);
  }
  Poly k = c.alloc(2 * tbeta, tl + 1 + c.K, 1);
  c.upload(k, host);
  c.gks[galEl] = EvKey{k, tl};
  API_END_VOID
}
// lineartransform.go:167-183: the diagonal's ringqp.Poly (Q at the transform's
// level, P), after which the transform forgets it until LoadPlaintextDiagonal
ArrayResultByte SerializeDiagonal(int tid, int diagIdx) {
  ArrayResultByte r{nullptr, 0};
  API_BEGIN
  Context& c = ctx();
  LinTrans& T = c.lts.get(tid);
  const int key = diagIdx & (c.slots - 1);
  auto it = T.diags.find(key);
  if (it == T.diags.end()) throw std::runtime_error("diagonal " + std::to_string(diagIdx) + " is not loaded");
  std::vector<u64> host;
  c.download(it->second.poly, host);
  std::vector<char> bytes;
  put_qp(bytes, c, host.data(), T.level + 1);
  T.diags.erase(it);
  T.sdiags.erase(key);
  T.plan_dirty = true;
  c.lts.touch(tid);  // (a pipeline reading it waits for this context's work again)
  return to_bytes(bytes);
  API_END(r)
}
// lineartransform.go:186-200
void LoadPlaintextDiagonal(char* data, unsigned long len, int tid, unsigned long diagIdx) {
  API_BEGIN
  Context& c = ctx();
  if (!data) throw std::runtime_error("null diagonal data");
  LinTrans& T = c.lts.get(tid);
  Plaintext p;
  p.level = T.level;
  p.qp = true;
  p.scale = (long double)c.mods[T.level];
  p.poly = c.alloc(1, T.level + 1 + c.K, 1);
  wire::Reader rd(data, len);
  std::vector<u64> host((size_t)p.poly.nlimb * c.N);
  get_qp(rd, c, host.data(), T.level + 1, "diagonal");
  if (rd.left()) throw std::runtime_error("diagonal blob has trailing bytes");
  c.upload(p.poly, host);
  T.diags[(int)diagIdx & (c.slots - 1)] = p;
  T.plan_dirty = true;
  c.lts.touch(tid);
  API_END_VOID
}
void RemovePlaintextDiagonals(int tid) {
  API_BEGIN
  ctx().lts.get(tid).diags.clear();
  ctx().lts.get(tid).sdiags.clear();
  ctx().lts.get(tid).plan_dirty = true;
  ctx().lts.touch(tid);
  API_END_VOID
}
void RemoveRotationKeys(void) {
  API_BEGIN
  ctx().gks.clear();
  ctx().gk_host.clear();
  API_END_VOID
}

// ---- SURVEY §8f "next": polynomial evaluation, minimax, bootstrapping ----
void NewPolynomialEvaluator(void) {}
static int add_poly(float* coeffs, int n, bool cheb) {
  Context& c = ctx();
  if (!coeffs || n < 1) throw std::runtime_error("polynomial needs at least one coefficient");
  Context::PolyFn p;
  p.cheb = cheb;
  for (int i = 0; i < n; ++i) p.c.push_back((long double)coeffs[i]);
  return c.polys.add(std::move(p));
}
// polyeval.go:38-47: bignum.Monomial, coefficients lowest degree first
int GenerateMonomial(float* coeffs, int n) {
  API_BEGIN
  return add_poly(coeffs, n, false);
  API_END(-1)
}
// polyeval.go:50-60: bignum.Chebyshev on [-1, 1]
int GenerateChebyshev(float* coeffs, int n) {
  API_BEGIN
  return add_poly(coeffs, n, true);
  API_END(-1)
}
// poly_evaluator.py:58-59: levels an evaluation consumes, bits.Len64(degree)
int GetPolyDepth(int poly) {
  API_BEGIN
  const int deg = (int)ctx().polys.get(poly).c.size() - 1;
  int d = 0;
  while ((1 << d) <= deg) ++d;
  return d;
  API_END(-1)
}
// polyeval.go:63-84: a new ciphertext at level - bitlen(degree), scale outScale
int EvaluatePolynomial(int ct, int poly, unsigned long outScale) {
  API_BEGIN
  Context& c = ctx();
  return c.cts.add(c.eval_poly(c.cts.get(ct), c.polys.get(poly), (long double)outScale));
  API_END(-1)
}
// polyeval.go:91-167: composite minimax sign coefficients (compile-time, host),
// cached per (degrees, prec, logalpha, logerr) like minimaxSignMap; every fit
// absorbs the scheme error 2^-logerr, and the last polynomial is mapped from
// [-1, 1] to [0, 1] (halved, + 0.5, inside minimax_sign_composite).  The Remez
// restatement works in binary128 / double-binary128 whatever `prec` asks for:
// at prec >= 113 (orion's default is 128) the doubles are the prec-bit
// computation's (tests/golden/minimax_sign.json).
static std::map<std::string, std::vector<double>> g_minimax_cache;
ArrayResultDouble GenerateMinimaxSignCoeffs(int* degrees, int n, int prec, int logalpha, int logerr, int debug) {
  ArrayResultDouble r{nullptr, 0};
  API_BEGIN
  std::vector<int> deg;
  for (int i = 0; i < n; ++i) deg.push_back(degrees[i]);
  if (deg.empty()) throw std::runtime_error("at least one degree is required");
  std::string key;
  for (int d : deg) key += std::to_string(d) + ",";
  key += "|" + std::to_string(prec) + "|" + std::to_string(logalpha) + "|" + std::to_string(logerr);
  auto it = g_minimax_cache.find(key);
  if (it == g_minimax_cache.end()) {
    std::vector<std::vector<double>> polys = minimax_sign_composite(deg, logalpha, logerr, nullptr, debug != 0);
    std::vector<double> flat;
    for (auto& p : polys) flat.insert(flat.end(), p.begin(), p.end());
    it = g_minimax_cache.emplace(key, flat).first;
  }
  r.Data = to_c_array<double, double>(it->second, &r.Length);
  return r;
  API_END(r)
}
// bootstrapper.go:19-58: one bootstrapper per slot count, made once, under
// bootstrapping parameters with P primes of the bit sizes logPs
// (Context::new_bootstrapper)
void NewBootstrapper(int* logPs, int n, int slots) {
  API_BEGIN
  Context& c = ctx();
  std::vector<int> lp;
  if (logPs && n > 0) lp.assign(logPs, logPs + n);
  c.new_bootstrapper(lp, slots);
  API_END_VOID
}
// bootstrapper.go:61-80: a new ciphertext refreshed to the residual top level,
// at the input's scale, post-scaled by 2^(LogMaxSlots - LogSlots)
// (BTP_PACKED: Context::bootstrap_packed in its place, OrionHipBootstrapPacked;
// BTP_MANY: Context::bootstrap_many, on the full-slot bootstrapper, OrionHipBootstrapMany)
enum BtpKind { BTP_PLAIN, BTP_PACKED, BTP_MANY };
static int bootstrap_handle(int ct, int slots, BtpKind kind) {
  Context& c = ctx();
  Context* s = scheme_ctx();
  const bool packed = kind == BTP_PACKED;
  if (packed) c.need_complex();
  auto run = [&](Context& on, const Ciphertext& in) {
    if (kind == BTP_PLAIN) return on.bootstrap(in, slots);
    if (!in.poly.ptr() || in.poly.ncomp < 2)
      throw std::runtime_error("ciphertext " + std::to_string(ct) + " holds no degree-1 polynomial pair");
    return packed ? on.bootstrap_packed(in, slots) : on.bootstrap_many(in, slots);
  };
  if (c.btps.count(kind == BTP_MANY ? c.N / 2 : slots) || !s || s == &c) return c.cts.add(run(c, c.cts.get(ct)));
  // a pipeline bootstraps with the scheme's bootstrapper (one circuit and key
  // set per process), on the scheme's stream under the scheme's lock: the
  // scheme's stream waits for the input, the result is copied into a buffer
  // of this pipeline's pool there, and this stream waits for the copy
  const Ciphertext& in = c.cts.get(ct);
  std::lock_guard<std::recursive_mutex> lk(s->mu);  // (a pipeline may wait on the scheme: index order)
  wait_on(*s, c);
  Ciphertext out;
  {
    Context* saved = t_act;
    t_act = s;
    try {
      Ciphertext r = run(*s, in);
      out = c.new_ct(r.level, r.poly.B, r.scale);
      s->copy(s->lsq(out.poly, 0, 2, r.level), s->lsq(r.poly, 0, 2, r.level));
    } catch (...) {
      t_act = saved;
      throw;
    }
    t_act = saved;
  }
  wait_on(c, *s);
  return c.cts.add(std::move(out));
}
int Bootstrap(int ct, int slots) {
  API_BEGIN
  return bootstrap_handle(ct, slots, BTP_PLAIN);
  API_END(-1)
}
// the batch refreshed two images per circuit run (orion_hip.h; Context::bootstrap_packed)
int OrionHipBootstrapPacked(int ct, int slots) {
  API_BEGIN
  return bootstrap_handle(ct, slots, BTP_PACKED);
  API_END(-1)
}
// the batch refreshed N / (2 slots) sparse images per full-slot circuit run (orion_hip.h; Context::bootstrap_many)
int OrionHipBootstrapMany(int ct, int slots) {
  API_BEGIN
  return bootstrap_handle(ct, slots, BTP_MANY);
  API_END(-1)
}
void DeleteBootstrappers(void) {
  API_BEGIN
  if (t_act) t_act->delete_bootstrappers();
  API_END_VOID
}
// the bootstrapping chain of the circuit for `slots` (its Q primes, then its P primes)
static Context* btp_context(int slots) {
  Context* s = scheme_ctx();
  if (!s) return nullptr;
  auto it = s->btps.find(slots);
  return it == s->btps.end() ? nullptr : it->second->bc;
}
int OrionHipBootstrapNumQ(int slots) {
  Context* b = btp_context(slots);
  return b ? b->L : -1;
}
int OrionHipBootstrapNumP(int slots) {
  Context* b = btp_context(slots);
  return b ? b->K : -1;
}
unsigned long OrionHipBootstrapModulus(int slots, int i) {
  Context* b = btp_context(slots);
  return (b && i >= 0 && i < (int)b->mods.size()) ? b->mods[i] : 0;
}

// an evaluation key in the full-chain layout [dnum][2][L+K][N]: a key made for
// a lower level fills its digits and limbs, the rest is zero
static void export_evk_full(Context& c, const EvKey& k, unsigned long* out, unsigned long n) {
  if (n != (unsigned long)2 * c.dnum * (c.L + c.K) * c.N) throw std::runtime_error("export buffer size mismatch");
  std::vector<u64> host;
  c.download(k.k, host);
  memset(out, 0, n * 8);
  const int beta = k.k.ncomp / 2, nl = k.k.nlimb;
  for (int i = 0; i < 2 * beta; ++i)
    for (int x = 0; x < nl; ++x) {
      const int m = x <= k.level ? x : c.L + (x - k.level - 1);
      memcpy(out + ((size_t)i * (c.L + c.K) + m) * c.N, host.data() + ((size_t)i * nl + x) * c.N, (size_t)c.N * 8);
    }
}

// Parity access to a bootstrapper's shared inputs (tests/test_gpu_parity.py
// bootstrapping parity; the CPU oracle restates the circuit from them):
// returns the element count written (or needed, out = NULL), -1 on error.
long OrionHipBootstrapExport(int slots, int what, long arg, void* out, unsigned long n) {
  API_BEGIN
  Context& c = ctx();
  auto it = c.btps.find(slots);
  if (it == c.btps.end()) throw std::runtime_error("no bootstrapper found for slot count: " + std::to_string(slots));
  Context::Bootstrapper& bt = *it->second;
  Context& b = *bt.bc;
  auto lt_of = [&](long i) -> LinTrans& {
    if (i < 0 || i >= (long)(bt.cts.size() + bt.stc.size())) throw std::runtime_error("bootstrap LT index out of range");
    return i < (long)bt.cts.size() ? bt.cts[i] : bt.stc[i - bt.cts.size()];
  };
  switch (what) {
    case ORION_BTX_PARAMS: {  // long double: F, gap, K, r, degree, slots, s_y, top, L, K_P, ntrace, nlt, degree+1, t0
      const long double v[] = {(long double)bt.F, (long double)bt.gap, (long double)bt.K, (long double)bt.r,
                               (long double)bt.degree, (long double)bt.slots, bt.s_y, (long double)bt.top,
                               (long double)b.L, (long double)b.K, (long double)bt.trace_gal.size(),
                               (long double)(bt.cts.size() + bt.stc.size()), (long double)bt.cosp.c.size(), bt.t0};
      const long cnt = (long)(sizeof(v) / sizeof(v[0]));
      if (out) {
        if (n < (unsigned long)cnt) throw std::runtime_error("export buffer too small");
        memcpy(out, v, sizeof(v));
      }
      return cnt;
    }
    case ORION_BTX_COS: {
      const long cnt = (long)bt.cosp.c.size();
      if (out) {
        if (n < (unsigned long)cnt) throw std::runtime_error("export buffer too small");
        for (long i = 0; i < cnt; ++i) ((long double*)out)[i] = bt.cosp.c[i];
      }
      return cnt;
    }
    case ORION_BTX_TRACE: {
      const long cnt = (long)bt.trace_gal.size();
      if (out) {
        if (n < (unsigned long)cnt) throw std::runtime_error("export buffer too small");
        for (long i = 0; i < cnt; ++i) ((unsigned long*)out)[i] = bt.trace_gal[i];
      }
      return cnt;
    }
    case ORION_BTX_RLK: {
      const long cnt = 2L * b.dnum * (b.L + b.K) * b.N;
      if (!b.have_rlk) throw std::runtime_error("the bootstrapper holds no relinearisation key yet");
      if (out) export_evk_full(b, EvKey{b.rlk, b.L - 1}, (unsigned long*)out, n);
      return cnt;
    }
    case ORION_BTX_GALOIS_KEYS: {  // the Galois elements with a key in the bootstrapping context
      const long cnt = (long)b.gks.size();
      if (out) {
        if (n < (unsigned long)cnt) throw std::runtime_error("export buffer too small");
        long i = 0;
        for (auto& kv : b.gks) ((unsigned long*)out)[i++] = kv.first;
      }
      return cnt;
    }
    case ORION_BTX_GALOIS: {
      auto kt = b.gks.find((u64)arg);
      if (kt == b.gks.end()) throw std::runtime_error("no galois key for element " + std::to_string(arg));
      const long cnt = 2L * b.dnum * (b.L + b.K) * b.N;
      if (out) export_evk_full(b, kt->second, (unsigned long*)out, n);
      return cnt;
    }
    case ORION_BTX_LT_INFO: {  // long: level, N1, ndiag, then the diagonal indices
      LinTrans& T = lt_of(arg);
      const long cnt = 3 + (long)T.idx.size();
      if (out) {
        if (n < (unsigned long)cnt) throw std::runtime_error("export buffer too small");
        long* o = (long*)out;
        o[0] = T.level, o[1] = T.N1, o[2] = (long)T.idx.size();
        for (size_t k = 0; k < T.idx.size(); ++k) o[3 + k] = T.idx[k];
      }
      return cnt;
    }
    case ORION_BTX_LT_DIAG: {  // arg = lt * 2^32 + k: the k-th diagonal (QP plaintext [level+1+K][N])
      LinTrans& T = lt_of(arg >> 32);
      const long k = arg & 0xffffffffl;
      if (k < 0 || k >= (long)T.idx.size()) throw std::runtime_error("bootstrap LT diagonal index out of range");
      const Poly& p = T.diags.at(T.idx[k] & (b.N / 2 - 1)).poly;
      const long cnt = (long)p.nlimb * b.N;
      if (out) {
        if (n != (unsigned long)cnt) throw std::runtime_error("export buffer size mismatch");
        std::vector<u64> host;
        b.download(p, host);
        memcpy(out, host.data(), (size_t)cnt * 8);
      }
      return cnt;
    }
    case ORION_BTX_D2S:  // the ephemeral-secret keys (full-chain layout; EvkDenseToSparse fills level 0)
    case ORION_BTX_S2D: {
      const long cnt = 2L * b.dnum * (b.L + b.K) * b.N;
      if (!(what == ORION_BTX_D2S ? bt.d2s : bt.s2d).k.buf)
        throw std::runtime_error("the bootstrapper holds no ephemeral-secret keys yet");
      if (out) export_evk_full(b, what == ORION_BTX_D2S ? bt.d2s : bt.s2d, (unsigned long*)out, n);
      return cnt;
    }
    case ORION_BTX_MONO_I: {  // what the circuit multiplies by: w4 on the first half of a limb, -w4 on the second
      if (bt.gap > 1) throw std::runtime_error("sparse-slot circuit: no X^(N/2) plaintext");
      const long cnt = (long)b.L * b.N;
      if (out) {
        if (n != (unsigned long)cnt) throw std::runtime_error("export buffer size mismatch");
        u64* o = (u64*)out;
        for (int l = 0; l < b.L; ++l) {
          std::fill(o + (size_t)l * b.N, o + (size_t)l * b.N + b.N / 2, b.w4[l]);
          std::fill(o + (size_t)l * b.N + b.N / 2, o + (size_t)(l + 1) * b.N, b.mods[l] - b.w4[l]);
        }
      }
      return cnt;
    }
    default:
      throw std::runtime_error("unknown bootstrap export item " + std::to_string(what));
  }
  API_END(-1)
}

// ---- import / export ----
static void to_canonical(const std::vector<u64>& dev, int ncomp, int nl, int B, int N, unsigned long* out) {
  // device [c][l][b][n] -> host [b][c][l][n]
  for (int c = 0; c < ncomp; ++c)
    for (int l = 0; l < nl; ++l)
      for (int b = 0; b < B; ++b)
        memcpy(out + (((size_t)b * ncomp + c) * nl + l) * N, dev.data() + (((size_t)c * nl + l) * B + b) * N, N * 8);
}
static std::vector<u64> from_canonical(const unsigned long* in, int ncomp, int nl, int B, int N) {
  std::vector<u64> dev((size_t)ncomp * nl * B * N);
  for (int c = 0; c < ncomp; ++c)
    for (int l = 0; l < nl; ++l)
      for (int b = 0; b < B; ++b)
        memcpy(dev.data() + (((size_t)c * nl + l) * B + b) * N, in + (((size_t)b * ncomp + c) * nl + l) * N, N * 8);
  return dev;
}
static void check_import(const Context& c, const void* data, int B, int level) {
  if (!data) throw std::runtime_error("null data pointer");
  if (level < 0 || level >= c.L || B < 1) throw std::runtime_error("invalid level/batch");
}
int ImportCiphertext(const unsigned long* data, int B, int level, double scale) {
  API_BEGIN
  Context& c = ctx();
  check_import(c, data, B, level);
  Ciphertext ct = c.new_ct(level, B, (long double)scale);
  c.upload(ct.poly, from_canonical(data, 2, level + 1, B, c.N));
  return c.cts.add(std::move(ct));
  API_END(-1)
}
int ExportCiphertext(int id, unsigned long* out, unsigned long n) {
  API_BEGIN
  Context& c = ctx();
  const Ciphertext& ct = c.cts.get(id);
  const int nl = ct.level + 1, B = ct.poly.B;
  if (n != (unsigned long)B * 2 * nl * c.N) throw std::runtime_error("export buffer size mismatch");
  Poly t = c.alloc(2, nl, B);
  c.copy(c.lsq(t, 0, 2, ct.level), c.lsq(ct.poly, 0, 2, ct.level));
  std::vector<u64> host;
  c.download(t, host);
  to_canonical(host, 2, nl, B, c.N, out);
  return 0;
  API_END(-1)
}
// canonical [B][2][nl][N] device layout <-> the library's [2][nl][B][N]: one
// strided 2-D copy per (comp, limb) plane, no host round trip
static void copy_planes(Context& c, u64* dst, long long dpitch, const u64* src, long long spitch, int nplane, int B,
                        long long dplane, long long splane) {
  for (int p = 0; p < nplane; ++p)
    HIPCHK(hipMemcpy2DAsync(dst + p * dplane, dpitch * 8, src + p * splane, spitch * 8, (size_t)c.N * 8, B,
                            hipMemcpyDeviceToDevice, c.stream));
}
int ImportCiphertextDevice(const unsigned long* dptr, int B, int level, double scale) {
  API_BEGIN
  Context& c = ctx();
  check_import(c, dptr, B, level);
  const int nl = level + 1;
  Ciphertext ct = c.new_ct(level, B, (long double)scale);
  // plane (comp, limb) = p: library offset p*B*N, canonical offset p*N with row pitch 2*nl*N
  copy_planes(c, ct.poly.ptr(), c.N, (const u64*)dptr, (long long)2 * nl * c.N, 2 * nl, B, (long long)B * c.N, c.N);
  return c.cts.add(std::move(ct));
  API_END(-1)
}
int ExportCiphertextDevice(int id, unsigned long* dptr, unsigned long n) {
  API_BEGIN
  Context& c = ctx();
  if (!dptr) throw std::runtime_error("null output pointer");
  const Ciphertext& ct = c.cts.get(id);
  const int nl = ct.level + 1, B = ct.poly.B;
  if (n != (unsigned long)B * 2 * nl * c.N) throw std::runtime_error("export buffer size mismatch");
  // a ciphertext's limb planes may be allocated for a higher level: address them by its strides
  const Poly& P = ct.poly;
  for (int comp = 0; comp < 2; ++comp)
    for (int l = 0; l < nl; ++l)
      HIPCHK(hipMemcpy2DAsync((u64*)dptr + ((size_t)comp * nl + l) * c.N, (size_t)2 * nl * c.N * 8,
                              P.ptr() + comp * P.comp_stride() + l * P.limb_stride(), (size_t)c.N * 8,
                              (size_t)c.N * 8, B, hipMemcpyDeviceToDevice, c.stream));
  return 0;
  API_END(-1)
}
int ImportPlaintext(const unsigned long* data, int B, int level, double scale) {
  API_BEGIN
  Context& c = ctx();
  check_import(c, data, B, level);
  Plaintext p;
  p.level = level;
  p.scale = (long double)scale;
  p.poly = c.alloc(1, level + 1, B);
  c.upload(p.poly, from_canonical(data, 1, level + 1, B, c.N));
  return c.pts.add(std::move(p));
  API_END(-1)
}
int ExportPlaintext(int id, unsigned long* out, unsigned long n) {
  API_BEGIN
  Context& c = ctx();
  const Plaintext& p = c.pts.get(id);
  const int nl = p.poly.nlimb, B = p.poly.B;
  if (n != (unsigned long)B * nl * c.N) throw std::runtime_error("export buffer size mismatch");
  std::vector<u64> host;
  c.download(p.poly, host);
  to_canonical(host, 1, nl, B, c.N, out);
  return 0;
  API_END(-1)
}
static int export_poly(const Poly& p, unsigned long* out, unsigned long n) {
  Context& c = ctx();
  std::vector<u64> host;
  c.download(p, host);
  if (n != host.size()) throw std::runtime_error("export buffer size mismatch");
  memcpy(out, host.data(), n * 8);
  return 0;
}
int ExportSecretKey(unsigned long* out, unsigned long n) {
  API_BEGIN
  if (!ctx().have_sk) throw std::runtime_error("no secret key");
  return export_poly(ctx().sk, out, n);
  API_END(-1)
}
int ExportPublicKey(unsigned long* out, unsigned long n) {
  API_BEGIN
  if (!ctx().have_pk) throw std::runtime_error("no public key");
  return export_poly(ctx().pk, out, n);
  API_END(-1)
}
unsigned int OrionHipEncryptionIndex(void) {
  API_BEGIN
  return t_act ? t_act->enc_sampler.enc : 0;
  API_END(0)
}
int ExportRelinKey(unsigned long* out, unsigned long n) {
  API_BEGIN
  if (!ctx().have_rlk) throw std::runtime_error("no relinearization key");
  return export_poly(ctx().rlk, out, n);
  API_END(-1)
}
int ExportGaloisKey(unsigned long galEl, unsigned long* out, unsigned long n) {
  API_BEGIN
  Context& c = ctx();
  auto it = c.gks.find(galEl);
  if (it == c.gks.end()) throw std::runtime_error("no galois key for element " + std::to_string(galEl));
  export_evk_full(c, it->second, out, n);  // the full-chain layout [dnum][2][L+K][N]
  return 0;
  API_END(-1)
}
int GetGaloisKeyLevel(unsigned long galEl) {
  API_BEGIN
  Context& c = ctx();
  auto it = c.gks.find(galEl);
  if (it == c.gks.end()) throw std::runtime_error("no galois key for element " + std::to_string(galEl));
  return it->second.level;
  API_END(-1)
}
int ExportLinearTransformDiagonal(int tid, int diagIdx, unsigned long* out, unsigned long n) {
  API_BEGIN
  Context& c = ctx();
  return export_poly(c.lts.get(tid).diags.at(diagIdx & (c.slots - 1)).poly, out, n);
  API_END(-1)
}

// ---- key bundle for RCCL broadcast ----
// layout: header u64[KB_HDR] {magic, ngk, withSecret, haveRlk, logN, L, K,
// dnum, moduli digest}, galEls[ngk], then pk, rlk, gk_0..gk_{ngk-1}, [sk] as
// raw device polys.  The importer rejects a bundle made for another chain.
enum { KB_HDR = 9 };
static const u64 KB_MAGIC = 0x4f52494f4e4b4232ull;  // "ORIONKB2"
static u64 moduli_digest(const Context& c) {
  u64 h = 0xcbf29ce484222325ull;  // FNV-1a over the QP moduli
  for (u64 q : c.mods)
    for (int b = 0; b < 8; ++b) h = (h ^ ((q >> (8 * b)) & 0xff)) * 0x100000001b3ull;
  return h;
}
unsigned long KeyBundleBytes(int withSecret) {
  API_BEGIN
  Context& c = ctx();
  const size_t key = (size_t)2 * c.dnum * (c.L + c.K) * c.N * 8, pk = (size_t)2 * (c.L + c.K) * c.N * 8,
               sk = (size_t)(c.L + c.K) * c.N * 8;
  size_t hdr = (KB_HDR + 2 * c.gks.size()) * 8;
  hdr = (hdr + 255) & ~(size_t)255;
  size_t gk = 0;
  for (auto& kv : c.gks) gk += (size_t)kv.second.k.ncomp * kv.second.k.nlimb * c.N * 8;
  return hdr + pk + (c.have_rlk ? key : 0) + gk + (withSecret ? sk : 0);
  API_END(0)
}
int ExportKeyBundle(void* dptr, int withSecret) {
  API_BEGIN
  Context& c = ctx();
  if (!dptr) throw std::runtime_error("null bundle pointer");
  if (!c.have_pk) throw std::runtime_error("no public key");
  if (withSecret && !c.have_sk) throw std::runtime_error("no secret key");
  std::vector<u64> hdr = {KB_MAGIC, (u64)c.gks.size(), (u64)(withSecret ? 1 : 0), (u64)c.have_rlk,
                          (u64)c.logN, (u64)c.L, (u64)c.K, (u64)c.dnum, moduli_digest(c)};
  for (auto& kv : c.gks) hdr.push_back(kv.first), hdr.push_back((u64)kv.second.level);
  size_t off = ((hdr.size() * 8) + 255) & ~(size_t)255;
  char* d = (char*)dptr;
  HIPCHK(hipMemcpyAsync(d, hdr.data(), hdr.size() * 8, hipMemcpyHostToDevice, c.stream));
  auto put = [&](const Poly& p) {
    const size_t b = (size_t)p.ncomp * p.nlimb * p.B * c.N * 8;
    HIPCHK(hipMemcpyAsync(d + off, p.ptr(), b, hipMemcpyDeviceToDevice, c.stream));
    off += b;
  };
  put(c.pk);
  if (c.have_rlk) put(c.rlk);
  for (auto& kv : c.gks) put(kv.second.k);
  if (withSecret) put(c.sk);
  HIPCHK(hipStreamSynchronize(c.stream));
  return 0;
  API_END(-1)
}
int ImportKeyBundle(const void* dptr, unsigned long bytes) {
  API_BEGIN
  Context& c = ctx();
  if (!dptr) throw std::runtime_error("null bundle pointer");
  if (bytes < KB_HDR * 8) throw std::runtime_error("key bundle shorter than its header");
  u64 h4[KB_HDR];
  HIPCHK(hipMemcpy(h4, dptr, sizeof(h4), hipMemcpyDeviceToHost));
  if (h4[0] != KB_MAGIC) throw std::runtime_error("not a key bundle");
  if (h4[4] != (u64)c.logN || h4[5] != (u64)c.L || h4[6] != (u64)c.K || h4[7] != (u64)c.dnum ||
      h4[8] != moduli_digest(c))
    throw std::runtime_error("key bundle was made for another modulus chain (logN/L/K/dnum/moduli differ)");
  if (h4[1] > (bytes / 8 - KB_HDR) / 2) throw std::runtime_error("key bundle truncated (galois element list)");
  std::vector<u64> gels(2 * h4[1]);  // (element, level) pairs
  if (h4[1]) HIPCHK(hipMemcpy(gels.data(), (const char*)dptr + KB_HDR * 8, h4[1] * 16, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < h4[1]; ++i)
    if (gels[2 * i + 1] >= (u64)c.L) throw std::runtime_error("key bundle: galois key level outside the chain");
  size_t off = ((KB_HDR + 2 * h4[1]) * 8 + 255) & ~(size_t)255;
  const char* d = (const char*)dptr;
  auto get = [&](int ncomp, int nlimb) {
    Poly p = c.alloc(ncomp, nlimb, 1);
    const size_t b = (size_t)ncomp * nlimb * c.N * 8;
    if (off + b > bytes) throw std::runtime_error("key bundle truncated");
    HIPCHK(hipMemcpyAsync(p.ptr(), d + off, b, hipMemcpyDeviceToDevice, c.stream));
    off += b;
    return p;
  };
  c.pk = get(2, c.L + c.K);
  c.have_pk = true;
  if (h4[3]) {
    c.rlk = get(2 * c.dnum, c.L + c.K);
    c.have_rlk = true;
  }
  for (size_t i = 0; i < h4[1]; ++i) {
    const int lv = (int)gels[2 * i + 1];
    c.gks[gels[2 * i]] = EvKey{get(2 * ((lv + 1 + c.K - 1) / c.K), lv + 1 + c.K), lv};
  }
  if (h4[2]) {
    c.sk = get(1, c.L + c.K);
    c.have_sk = true;
  }
  HIPCHK(hipStreamSynchronize(c.stream));
  return 0;
  API_END(-1)
}

// ---- bootstrapping keys, record by record ----
// A scheme without the secret key builds its bootstrapping circuits
// (NewBootstrapper) and receives their evaluation keys from the key owner, one
// self-describing record at a time (a bundle of them all would double the
// device memory the keys take).  A record: a 256-byte header u64[32] {magic,
// kind, galois element, level, slot count (d2s / s2d: they belong to one
// circuit; else 0), logN, Q and P prime counts of the bootstrapping chain,
// dnum, digest of its moduli, payload bytes}, then the key's raw device words
// [digit][2][level+1+K][N] (EvKey).  Records come in the need-list's order:
// relin, d2s, s2d, the Galois keys by ascending element.
enum { BKR_HDR = 32, BKR_MAGIC_I = 0, BKR_KIND, BKR_GEL, BKR_LEVEL, BKR_SLOTS, BKR_LOGN, BKR_L, BKR_K, BKR_DNUM,
       BKR_DIGEST, BKR_PAYLOAD, BKR_NFIELD };
static const u64 BKR_MAGIC = 0x4f52494f4e424b31ull;  // "ORIONBK1"
static Context::Bootstrapper& btp_of(Context& c, int slots) {
  auto it = c.btps.find(slots);
  if (it == c.btps.end()) throw std::runtime_error("no bootstrapper found for slot count: " + std::to_string(slots));
  return *it->second;
}
static size_t evk_bytes(const Context& b, int level) {
  return (size_t)2 * ((level + 1 + b.K - 1) / b.K) * (level + 1 + b.K) * b.N * 8;
}
static Context::KeyNeed btp_record(Context& c, int slots, int i, Context::Bootstrapper** btp = nullptr) {
  Context::Bootstrapper& bt = btp_of(c, slots);
  const std::vector<Context::KeyNeed> recs = bt.bc->key_records(bt);
  if (i < 0 || i >= (int)recs.size())
    throw std::runtime_error("bootstrap key record " + std::to_string(i) + " out of range: " +
                             std::to_string(recs.size()) + " records held for " + std::to_string(slots) + " slots");
  if (btp) *btp = &bt;
  return recs[i];
}
int OrionHipBootstrapPrepareKeys(int slots) {
  API_BEGIN
  Context& c = ctx();
  Context::Bootstrapper& bt = btp_of(c, slots);
  bt.bc->prepare_keys(bt);
  return (int)bt.bc->key_records(bt).size();
  API_END(-1)
}
int OrionHipBootstrapMissingKeys(int slots) {
  API_BEGIN
  Context::Bootstrapper& bt = btp_of(ctx(), slots);
  return (int)bt.bc->missing_keys(bt).size();
  API_END(-1)
}
int OrionHipBootstrapKeyCount(int slots) {
  API_BEGIN
  Context::Bootstrapper& bt = btp_of(ctx(), slots);
  return (int)bt.bc->key_records(bt).size();
  API_END(-1)
}
unsigned long OrionHipBootstrapKeyBytes(int slots, int i) {
  API_BEGIN
  Context::Bootstrapper* bt = nullptr;
  const Context::KeyNeed r = btp_record(ctx(), slots, i, &bt);
  return (unsigned long)(BKR_HDR * 8 + evk_bytes(*bt->bc, r.level));
  API_END(0)
}
int OrionHipBootstrapKeyInfo(int slots, int i, unsigned long* out4) {
  API_BEGIN
  if (!out4) throw std::runtime_error("null output pointer");
  Context::Bootstrapper* bt = nullptr;
  const Context::KeyNeed r = btp_record(ctx(), slots, i, &bt);
  out4[0] = (unsigned long)r.kind, out4[1] = r.gel, out4[2] = (unsigned long)r.level;
  out4[3] = (unsigned long)evk_bytes(*bt->bc, r.level);
  return 0;
  API_END(-1)
}
int OrionHipExportBootstrapKey(int slots, int i, void* dptr) {
  API_BEGIN
  Context& c = ctx();
  c.no_capture("exporting a bootstrapping key");
  if (!dptr) throw std::runtime_error("null record pointer");
  Context::Bootstrapper* bt = nullptr;
  const Context::KeyNeed r = btp_record(c, slots, i, &bt);
  Context& b = *bt->bc;
  const size_t payload = evk_bytes(b, r.level);
  if ((size_t)r.k->ncomp * r.k->nlimb * r.k->B * b.N * 8 != payload)
    throw std::logic_error("bootstrap key record: key buffer does not match its level");
  u64 hdr[BKR_HDR] = {0};
  hdr[BKR_MAGIC_I] = BKR_MAGIC, hdr[BKR_KIND] = (u64)r.kind, hdr[BKR_GEL] = r.gel, hdr[BKR_LEVEL] = (u64)r.level;
  hdr[BKR_SLOTS] = (r.kind == Context::BK_D2S || r.kind == Context::BK_S2D) ? (u64)slots : 0;
  hdr[BKR_LOGN] = (u64)b.logN, hdr[BKR_L] = (u64)b.L, hdr[BKR_K] = (u64)b.K, hdr[BKR_DNUM] = (u64)b.dnum;
  hdr[BKR_DIGEST] = moduli_digest(b), hdr[BKR_PAYLOAD] = (u64)payload;
  HIPCHK(hipMemcpyAsync(dptr, hdr, sizeof(hdr), hipMemcpyHostToDevice, b.stream));
  HIPCHK(hipMemcpyAsync((char*)dptr + sizeof(hdr), r.k->ptr(), payload, hipMemcpyDeviceToDevice, b.stream));
  HIPCHK(hipStreamSynchronize(b.stream));
  return 0;
  API_END(-1)
}
int OrionHipImportBootstrapKey(int slots, const void* dptr, unsigned long bytes) {
  API_BEGIN
  Context& c = ctx();
  c.no_capture("importing a bootstrapping key");
  if (!dptr) throw std::runtime_error("null record pointer");
  Context::Bootstrapper& bt = btp_of(c, slots);
  Context& b = *bt.bc;
  // every check comes before the first change: a refused record leaves the
  // bootstrapper as it was
  if (bytes < BKR_HDR * 8) throw std::runtime_error("bootstrap key record shorter than its header");
  u64 h[BKR_HDR];
  HIPCHK(hipMemcpyAsync(h, dptr, sizeof(h), hipMemcpyDeviceToHost, b.stream));
  HIPCHK(hipStreamSynchronize(b.stream));
  if (h[BKR_MAGIC_I] != BKR_MAGIC) throw std::runtime_error("not a bootstrap key record (bad magic)");
  if (h[BKR_LOGN] != (u64)b.logN || h[BKR_L] != (u64)b.L || h[BKR_K] != (u64)b.K || h[BKR_DNUM] != (u64)b.dnum ||
      h[BKR_DIGEST] != moduli_digest(b))
    throw std::runtime_error("bootstrap key record was made for another bootstrapping chain "
                             "(logN/L/K/dnum/moduli differ)");
  const int kind = (int)h[BKR_KIND];
  if (h[BKR_KIND] < (u64)Context::BK_RELIN || h[BKR_KIND] > (u64)Context::BK_GALOIS)
    throw std::runtime_error("bootstrap key record: unknown key kind " + std::to_string(h[BKR_KIND]));
  if (h[BKR_LEVEL] >= (u64)b.L)
    throw std::runtime_error("bootstrap key record: level " + std::to_string(h[BKR_LEVEL]) +
                             " outside the bootstrapping chain (" + std::to_string(b.L) + " levels)");
  const int level = (int)h[BKR_LEVEL];
  if (kind == Context::BK_RELIN && level != b.L - 1)
    throw std::runtime_error("bootstrap key record: a relinearisation key below the chain's top level");
  if ((kind == Context::BK_D2S || kind == Context::BK_S2D) && h[BKR_SLOTS] != (u64)slots)
    throw std::runtime_error(std::string("bootstrap key record: this ") + Context::key_kind_name(kind) +
                             " key belongs to the circuit for " + std::to_string(h[BKR_SLOTS]) + " slots, not " +
                             std::to_string(slots));
  if (kind == Context::BK_GALOIS && (h[BKR_GEL] >= 2 * (u64)b.N || !(h[BKR_GEL] & 1)))
    throw std::runtime_error("bootstrap key record: " + std::to_string(h[BKR_GEL]) + " is no Galois element");
  const size_t payload = evk_bytes(b, level);
  if (h[BKR_PAYLOAD] != (u64)payload)
    throw std::runtime_error("bootstrap key record: payload size does not match its level");
  if ((size_t)bytes < BKR_HDR * 8 + payload)
    throw std::runtime_error("bootstrap key record truncated: " + std::to_string(bytes) + " bytes, header + payload " +
                             std::to_string(BKR_HDR * 8 + payload));
  // a key already held at this level or above stays (the Galois keys are
  // shared by the circuits of one bootstrapping context: a sibling's record may
  // carry a lower level)
  EvKey* held = kind == Context::BK_D2S ? &bt.d2s : kind == Context::BK_S2D ? &bt.s2d : nullptr;
  if (kind == Context::BK_GALOIS) {
    auto it = b.gks.find(h[BKR_GEL]);
    if (it != b.gks.end()) held = &it->second;
  }
  if (kind == Context::BK_RELIN ? b.have_rlk : (held && held->k.buf && held->level >= level)) return 0;
  const int beta = (level + 1 + b.K - 1) / b.K;
  Poly k = b.alloc(2 * beta, level + 1 + b.K, 1);
  HIPCHK(hipMemcpyAsync(k.ptr(), (const char*)dptr + BKR_HDR * 8, payload, hipMemcpyDeviceToDevice, b.stream));
  HIPCHK(hipStreamSynchronize(b.stream));
  if (kind == Context::BK_RELIN) b.rlk = k, b.have_rlk = true;
  else if (kind == Context::BK_GALOIS) b.gks[h[BKR_GEL]] = EvKey{k, level};
  else *held = EvKey{k, level};
  return 0;
  API_END(-1)
}

// ---- profiling ----
// Profiling switches and counters cover every context of the scheme (the
// pipelines' launches included); each context is locked on its own in turn.
}  // extern "C"
template <class F>
static void each_ctx(F f) {
  for (int i = 0; i < g_nctx.load(); ++i) {
    Context* c = g_slot[i].get();
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    f(*c);
    // the bootstrapping contexts the context owns (their launches run under its lock)
    for (auto& kv : c->btp_ctx) f(*kv.second);
  }
}
extern "C" {
void OrionHipProfile(int enable) {
  API_BEGIN_NOCTX
  each_ctx([&](Context& c) {
    if (!enable) c.prof_flush();
    c.prof = enable == 1 ? 0xffffffffu : (unsigned)enable;  // 1 = all categories, else a bit mask
  });
  API_END_VOID
}
// the reference of the union timing: recorded on the scheme's stream once
// every context is drained; the intervals collected so far are dropped
void OrionHipProfileClock(void) {
  API_BEGIN_NOCTX
  Context* s = scheme_ctx();
  if (!s) throw std::runtime_error("scheme not initialised: call NewScheme first");
  each_ctx([](Context& c) { c.prof_flush(); });
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_iv.clear();
  if (!g_prof_ref) HIPCHK(hipEventCreate(&g_prof_ref));
  HIPCHK(hipEventRecord(g_prof_ref, s->stream));
  HIPCHK(hipEventSynchronize(g_prof_ref));
  API_END_VOID
}
// the union of the wall-clock intervals of every context's profiled launches
// of the categories in `mask` since OrionHipProfileClock (ms): e.g. the time
// at least one NTT ran while pipelines overlap
double OrionHipProfileUnion(unsigned mask) {
  API_BEGIN_NOCTX
  each_ctx([](Context& c) { c.prof_flush(); });
  std::vector<std::pair<float, float>> iv;
  {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (const ProfIv& r : g_prof_iv)
      if (mask & (1u << r.cat)) iv.push_back({r.t0, r.t1});
  }
  std::sort(iv.begin(), iv.end());
  double tot = 0;
  float b = 0, e = 0;
  bool open = false;
  for (auto& x : iv) {
    if (!open || x.first > e) {
      if (open) tot += e - b;
      b = x.first, e = x.second, open = true;
    } else if (x.second > e) {
      e = x.second;
    }
  }
  if (open) tot += e - b;
  return tot;
  API_END(-1.0)
}
// a marker line ("# tag") in the NTT call log (bench.py brackets its timed
// region, so a kernel trace can be cut to it)
void OrionHipLogMark(const char* tag) {
  if (FILE* f = ntt_log_file()) fprintf(f, "# %s\n", tag ? tag : "");
}
void OrionHipProfileReset(void) {
  API_BEGIN_NOCTX
  each_ctx([](Context& c) {
    c.prof_flush();
    for (int i = 0; i < P_NCAT; ++i) c.prof_launch[i] = c.prof_ms[i] = c.prof_bytes[i] = c.prof_strict[i] = 0;
  });
  API_END_VOID
}
// counters summed over every context
int OrionHipProfileRead(char* names, long* launches, double* ms, double* bytes, int max) {
  API_BEGIN_NOCTX
  int n = std::min(max, (int)P_NCAT);
  for (int i = 0; i < n; ++i) {
    strncpy(names + 32 * i, kProfNames[i], 31);
    names[32 * i + 31] = 0;
    launches[i] = 0;
    ms[i] = bytes[i] = 0;
  }
  each_ctx([&](Context& c) {
    c.prof_flush();
    for (int i = 0; i < n; ++i) {
      launches[i] += (long)c.prof_launch[i];
      ms[i] += c.prof_ms[i];
      bytes[i] += c.prof_bytes[i];
    }
  });
  return n;
  API_END(-1)
}
int OrionHipProfileReadStrict(double* strict, int max) {
  API_BEGIN_NOCTX
  int n = std::min(max, (int)P_NCAT);
  for (int i = 0; i < n; ++i) strict[i] = 0;
  each_ctx([&](Context& c) {
    c.prof_flush();
    for (int i = 0; i < n; ++i) strict[i] += c.prof_strict[i];
  });
  return n;
  API_END(-1)
}

int OrionHipNTT(unsigned long* dptr, int nlimb, int batch, const int* mods, int inverse) {
  API_BEGIN
  Context& c = ctx();
  LimbSet s;
  memset(&s, 0, sizeof(s));
  s.p = (u64*)dptr;
  s.ncomp = 1;
  s.nlimb = nlimb;
  s.nbatch = batch;
  s.batch_stride = c.N;
  s.limb_stride = (long long)batch * c.N;
  if (nlimb > ORION_MAXLIMB) throw std::runtime_error("too many limbs");
  for (int l = 0; l < nlimb; ++l) {
    if (mods[l] < 0 || mods[l] >= c.L + c.K) throw std::runtime_error("bad modulus index");
    s.mod[l] = (unsigned char)mods[l];
    s.pos[l] = (unsigned char)l;
  }
  c.ntt(s, inverse != 0);
  return 0;
  API_END(-1)
}

}  // extern "C"
