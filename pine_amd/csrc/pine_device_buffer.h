// pine_amd/csrc/pine_device_buffer.h -- who owns device memory on the host side of the library.  Every device block a plan, a
// one-shot render, a builder or a test hook holds is a DeviceBuffer<T> member or local; pinned host memory, events and streams
// are unique_ptrs with a deleter.  Nothing is freed by hand: a handle goes back when its owner goes out of scope, on every
// return path.  Included by pine_plan.h behind DevicePool, where the blocks of plans and one-shot films come from.
#pragma once

namespace pine_gpu {

// handles the owners below hold right now, all kinds together (pine_gpu_test_live_device_blocks)
inline std::atomic<long long> g_live_handles{0};

// The first failing HIP call of an operation, reported the library's way: -1, "<what>: <HIP's text>" as the last error
// (what == nullptr: no text, the caller has a fallback of its own), and HIP's own last error not left sticky.
inline int hip_error(const char* what, hipError_t e) {
  if (what) set_error(std::string(what) + ": " + hipGetErrorString(e));
  (void)hipGetLastError();
  return -1;
}
// After a kernel launch: 0, or hip_error of what the launch left.
inline int hip_launch_check(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_error(what, e);
}

enum BlockSource : bool { kFromMalloc = false, kFromPool = true };

// Test mode: $PINE_GPU_TEST_POISON=<32-bit hex word> fills every block handed out with that word before the caller sees it
// (tests/test_poisoned_memory.py; DESIGN.md 4.3.1 lists every block and who writes it first).  Read at every allocation, so
// that a test can switch it inside one process; unset, nothing here makes a HIP call.
inline std::atomic<long long> g_poisoned_blocks{0}, g_poisoned_bytes{0};  // (pine_gpu_test_poison_stats)
// 0: unset (or empty); 1: `word` is the variable's value; -1: the value is no 32-bit hex word (hex digits only, an optional 0x in
// front) -- the allocation then fails: a value that parsed as 0 would "poison" with the zeros the mode exists to avoid.
inline int poison_word(uint32_t& word) {
  const char* e = getenv("PINE_GPU_TEST_POISON");
  if (!e || !*e) return 0;
  char* end = nullptr;
  const unsigned long long v = isxdigit((unsigned char)*e) ? strtoull(e, &end, 16) : 0;
  if (!end || end == e || *end || v > 0xffffffffull) return -1;
  word = uint32_t(v);
  return 1;
}
inline int bad_poison_word(const char* what) {
  if (what) set_error(std::string(what) + ": PINE_GPU_TEST_POISON is not a 32-bit hex word");
  return -1;
}
// `bytes` of device memory at q filled with `word`: whole words, then the last 1 - 3 bytes with its low byte.  Complete on
// the device when it returns: plans launch on the caller's streams, which a fill on the null stream does not order against.
inline hipError_t poison_device_block(void* q, size_t bytes, uint32_t word) {
  const size_t words = bytes / 4, tail = bytes % 4;
  hipError_t e = words ? hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(q), int(word), words) : hipSuccess;
  if (e == hipSuccess && tail) e = hipMemset(static_cast<char*>(q) + words * 4, int(word & 0xff), tail);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) g_poisoned_blocks++, g_poisoned_bytes += (long long)bytes;
  return e;
}

// One device block of T, move-only.  It remembers the device it was allocated on and where it came from (DevicePool, or plain
// hipMalloc) and returns it the same way with that device current; the caller's current device is left as it was.
template <class T>
class DeviceBuffer {
  T* p_ = nullptr;
  int device_ = 0;
  BlockSource source_;

 public:
  explicit DeviceBuffer(BlockSource source = kFromMalloc) : source_(source) {}
  DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_), device_(o.device_), source_(o.source_) { o.p_ = nullptr; }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, device_ = o.device_, source_ = o.source_;
      o.p_ = nullptr;
    }
    return *this;
  }
  ~DeviceBuffer() { reset(); }
  T* get() const { return p_; }
  operator T*() const { return p_; }  // (DeviceScene / WorkParams views and kernel arguments stay raw pointers)

  void reset() {
    if (!p_) return;
    int keep = device_;
    (void)hipGetDevice(&keep);
    if (keep != device_) (void)hipSetDevice(device_);
    if (source_ == kFromPool) DevicePool::get().free(p_);
    else (void)hipFree(p_);
    if (keep != device_) (void)hipSetDevice(keep);
    p_ = nullptr;
    g_live_handles--;
  }
  // n elements on the current device, uninitialised (alloc_bytes: a block with something else behind its elements)
  int alloc(size_t n, const char* what) { return alloc_bytes(n * sizeof(T), what); }
  int alloc_bytes(size_t bytes, const char* what) {
    reset();
    uint32_t word = 0;
    const int poison = poison_word(word);
    if (poison < 0) return bad_poison_word(what);
    void* q = nullptr;
    const hipError_t e = source_ == kFromPool ? DevicePool::get().alloc(&q, bytes) : hipMalloc(&q, bytes);
    if (e != hipSuccess) return hip_error(what, e);
    if (!q) return 0;  // (no bytes asked for)
    p_ = static_cast<T*>(q);
    (void)hipGetDevice(&device_);
    g_live_handles++;
    if (poison) {  // a pooled block over its rounded size: the slack behind `bytes` is memory a kernel could read
      const size_t block = source_ == kFromPool ? DevicePool::get().block_bytes(q, bytes) : bytes;
      if (const hipError_t pe = poison_device_block(q, block, word)) {
        reset();
        return hip_error(what, pe);
      }
    }
    return 0;
  }
  // the first n elements from / to the host
  int write(const T* src, size_t n, const char* what) {
    const hipError_t e = n ? hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
    return e == hipSuccess ? 0 : hip_error(what, e);
  }
  int download(T* dst, size_t n, const char* what) const {
    const hipError_t e = n ? hipMemcpy(dst, p_, n * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess;
    return e == hipSuccess ? 0 : hip_error(what, e);
  }
  // allocate and fill (nothing to copy still gets one element: a kernel argument is never null)
  int upload(const T* src, size_t n, const char* what) { return alloc(std::max<size_t>(n, 1), what) || write(src, n, what) ? -1 : 0; }
  int upload(const std::vector<T>& v, const char* what) { return upload(v.data(), v.size(), what); }
};

// Pinned host memory, events and streams: unique_ptrs whose deleters hand the handle back.
struct HandleDeleter {
  void operator()(hipEvent_t e) const { (void)hipEventDestroy(e), g_live_handles--; }
  void operator()(hipStream_t s) const { (void)hipStreamDestroy(s), g_live_handles--; }
  void operator()(void* pinned) const { (void)hipHostFree(pinned), g_live_handles--; }
};
using EventOwner = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, HandleDeleter>;
using StreamOwner = std::unique_ptr<std::remove_pointer_t<hipStream_t>, HandleDeleter>;
template <class T>
using PinnedOwner = std::unique_ptr<T[], HandleDeleter>;

inline int create_event(EventOwner& out, unsigned flags, const char* what) {
  hipEvent_t e = nullptr;
  if (const hipError_t err = hipEventCreateWithFlags(&e, flags)) return hip_error(what, err);
  out.reset(e), g_live_handles++;
  return 0;
}
inline int create_stream(StreamOwner& out, unsigned flags, const char* what) {
  hipStream_t s = nullptr;
  if (const hipError_t err = hipStreamCreateWithFlags(&s, flags)) return hip_error(what, err);
  out.reset(s), g_live_handles++;
  return 0;
}
template <class T>
int alloc_pinned(PinnedOwner<T>& out, size_t n, unsigned flags, const char* what) {
  uint32_t word = 0;
  const int poison = poison_word(word);
  if (poison < 0) return bad_poison_word(what);
  void* q = nullptr;
  if (const hipError_t err = hipHostMalloc(&q, n * sizeof(T), flags)) return hip_error(what, err);
  out.reset(static_cast<T*>(q)), g_live_handles++;
  if (poison) {
    unsigned char* b = static_cast<unsigned char*>(q);  // (whole words, then the word's low byte, as on the device)
    const size_t bytes = n * sizeof(T), whole = bytes & ~size_t(3);
    for (size_t i = 0; i < bytes; i++) b[i] = (unsigned char)(i < whole ? word >> (8 * (i % 4)) : word);
    g_poisoned_blocks++, g_poisoned_bytes += (long long)bytes;
  }
  return 0;
}

}  // namespace pine_gpu
