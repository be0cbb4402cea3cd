// tools/sanitize/spec_queue_main.cpp -- stand-alone host check of the background compile queue (SpecQueue) and the waiter's
// handle (SpecWaiter) of pine_amd/csrc/pine_specialize.h: plain C++, no GPU, built with -fsanitize=address,undefined and with
// -fsanitize=thread and run as an ordinary program by tests/test_specialize.py.  usage: spec_queue_main <tree>/pine_amd
// The compiler is this program itself ($PINE_GPU_HIPCC): started with --genco it notes the run, waits (at most 20 s) for the
// gate file $PINE_FAKE_GATE, and writes a few bytes to the path after -o -- or exits 1 when $PINE_FAKE_FAIL is set.
#include <filesystem>

#include "../../pine_amd/csrc/pine_specialize.h"

pine_gpu::AbiFingerprint pine_gpu::abi_fingerprint() { return pine_gpu::AbiFingerprint{}; }
using namespace pine_gpu;

#define CHECK(x)                                                          \
  do {                                                                    \
    if (!(x)) {                                                           \
      fprintf(stderr, "spec_queue_main: line %d: %s\n", __LINE__, #x);    \
      _exit(1);                                                           \
    }                                                                     \
  } while (0)

template <class Cond>
static bool soon(Cond cond) {  // every wait of this program: at most 20 s
  for (int i = 0; i < 4000 && !cond(); i++) usleep(5000);
  return cond();
}
static int fake_compiler(int argc, char** argv) {
  write_file(std::string(getenv("PINE_FAKE_RUNS")) + "/" + std::to_string(int(getpid())), "run");
  soon([] { return access(getenv("PINE_FAKE_GATE"), F_OK) == 0; });
  if (getenv("PINE_FAKE_FAIL")) return 1;
  for (int i = 1; i + 1 < argc; i++)
    if (!strcmp(argv[i], "-o")) return write_file(argv[i + 1], "not a code object") ? 0 : 1;
  return 1;
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++)
    if (!strcmp(argv[i], "--genco")) return fake_compiler(argc, argv);
  CHECK(argc == 2);
  namespace fs = std::filesystem;
  char tmpl[] = "/tmp/pine_spec_queue_XXXXXX";
  CHECK(mkdtemp(tmpl));
  const std::string dir = tmpl, gate = dir + "/gate", cache = dir + "/cache";
  fs::create_directory(dir + "/runs");
  setenv("PINE_GPU_HIPCC", fs::read_symlink("/proc/self/exe").c_str(), 1);
  setenv("PINE_GPU_CACHE_DIR", cache.c_str(), 1);
  setenv("PINE_GPU_SOURCE_DIR", argv[1], 1);
  setenv("PINE_FAKE_GATE", gate.c_str(), 1);
  setenv("PINE_FAKE_RUNS", (dir + "/runs").c_str(), 1);
  SpecQueue& q = SpecQueue::get();
  auto request = [](unsigned n) {  // (one key per feature word: the content key covers it)
    KernelRequest r;
    r.features = n, r.ctx = 1024, r.arch = "gfx950";
    std::string err;
    CHECK(kernel_cache_lookup(r, err) == 0);
    return r;
  };
  auto locked = [&](auto f) {
    std::lock_guard<std::mutex> lock(q.mu);
    return f();
  };
  auto job_of = [&](const KernelRequest& r) { return locked([&] { return q.jobs.count(r.key) ? q.jobs[r.key] : nullptr; }); };
  auto idle = [&] { return locked([&] { return !q.busy[0] && !q.busy[1] && q.pending.empty(); }); };
  auto both_compiling = [&] { return q.children[0].load() > 0 && q.children[1].load() > 0; };
  auto runs = [&] { return std::distance(fs::directory_iterator(dir + "/runs"), fs::directory_iterator()); };
  auto done = [](const SpecWaiter& w) { return w->state.load() != kSpecBuilding; };
  auto open_gate = [&] { CHECK(write_file(gate, "open")); };

  {  // (a) two handles for one key: one job, one compiler run; gone from `jobs` once built
    const KernelRequest r = request(1);
    SpecWaiter a = q.submit(r, false), b = q.submit(r, false);
    CHECK(a && b && a.get() == b.get() && a->waiters.load() == 2);
    open_gate();
    CHECK(soon([&] { return done(a); }) && a->state.load() == kSpecBuilt && runs() == 1);
    a.reset(), b.reset();
    CHECK(soon([&] { return !job_of(r); }) && soon(idle));
  }
  {  // (b) a job nobody waits for any more is cancelled without a compiler run; the key then gets a fresh job
    fs::remove(gate);
    const KernelRequest r = request(4);
    SpecWaiter w2 = q.submit(request(2), false), w3 = q.submit(request(3), false);
    CHECK(soon(both_compiling));
    SpecWaiter w4 = q.submit(r, false);
    const std::shared_ptr<SpecJob> dropped = job_of(r);
    w4.reset();
    open_gate();
    CHECK(soon([&] { return dropped->state.load() == kSpecFailed; }) && dropped->error == "cancelled" && soon(idle) && runs() == 3 && !job_of(r));
    w4 = q.submit(r, false);
    CHECK(w4 && w4.get() != dropped.get() && soon([&] { return done(w4); }) && w4->state.load() == kSpecBuilt && runs() == 4 && soon(idle));
  }
  {  // (c) a full queue: an empty handle, no count changed
    fs::remove(gate);
    std::vector<SpecWaiter> held;
    for (unsigned n = 10; n < 12; n++) held.push_back(q.submit(request(n), false));
    CHECK(soon(both_compiling));
    for (unsigned n = 12; n < 12 + SpecQueue::kMaxPending; n++) held.push_back(q.submit(request(n), false));
    const size_t known = locked([&] { return q.jobs.size(); });
    CHECK(known == 2 + SpecQueue::kMaxPending && locked([&] { return int(q.pending.size()); }) == SpecQueue::kMaxPending);
    SpecWaiter none = q.submit(request(99), false);
    CHECK(!none && locked([&] { return q.jobs.size(); }) == known && locked([&] { return int(q.pending.size()); }) == SpecQueue::kMaxPending);
    for (const SpecWaiter& w : held) CHECK(w && w->waiters.load() == 1);
    open_gate();
    for (const SpecWaiter& w : held) CHECK(soon([&] { return done(w); }) && w->state.load() == kSpecBuilt);
    CHECK(soon(idle));
  }
  {  // (d) a failed build is remembered: handed out again as it is, or built again on request; (e) the handle's count
    setenv("PINE_FAKE_FAIL", "1", 1);  // (the queue is idle: no worker reads the environment now)
    const KernelRequest r = request(20);
    const long before = runs();
    SpecWaiter f1 = q.submit(r, false);
    CHECK(soon([&] { return done(f1); }) && f1->state.load() == kSpecFailed && f1->error.find("failed") != std::string::npos && job_of(r).get() == f1.get());
    SpecWaiter f2 = q.submit(r, false);
    CHECK(f2.get() == f1.get() && f1->waiters.load() == 2 && soon(idle) && runs() == before + 1);
    SpecWaiter f3 = q.submit(r, true);
    CHECK(f3 && f3.get() != f1.get() && soon([&] { return done(f3); }) && f3->state.load() == kSpecFailed && soon(idle) && runs() == before + 2);
    const std::shared_ptr<SpecJob> last = job_of(r);  // (the retry's job has taken the key)
    f2.reset(), f3.reset();
    CHECK(f1->waiters.load() == 1 && last->waiters.load() == 0);
    {
      SpecWaiter x = q.submit(r, false);
      CHECK(x.get() == last.get() && last->waiters.load() == 1);
      SpecWaiter y = std::move(x);
      CHECK(!x && y && last->waiters.load() == 1);
      x.reset();
      SpecWaiter z;
      z = std::move(y);
      CHECK(!y && z && last->waiters.load() == 1);
      z = q.submit(r, false);  // (assigned over: the old share goes back, the new one counts)
      CHECK(last->waiters.load() == 1);
    }
    CHECK(last->waiters.load() == 0);
    unsetenv("PINE_FAKE_FAIL");
  }
  {  // (f) shutdown ends a compiler that waits behind the gate, in time, and leaves no build directory
    fs::remove(gate);
    SpecWaiter w = q.submit(request(30), false);
    CHECK(soon([&] { return q.children[0].load() > 0 || q.children[1].load() > 0; }));
    const auto t0 = std::chrono::steady_clock::now();
    q.shutdown();
    CHECK(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(20) && done(w) && w->state.load() == kSpecFailed);
    for (const auto& e : fs::directory_iterator(cache)) CHECK(e.path().filename().string().rfind("build_", 0) != 0);
    CHECK(!q.submit(request(31), false));
  }
  fs::remove_all(dir);
  puts("spec_queue_main: ok");
  return 0;
}
