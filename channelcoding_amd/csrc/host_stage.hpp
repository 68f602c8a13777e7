// host_stage.hpp -- staging of the host-pointer entry points; included by capi.hip only.
// CopyPool moves pageable caller memory, HostStage owns a handle's two streams and their buffers, and staged_call
// is the one chunk loop that every host-pointer entry point runs.
#pragma once

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "cc_internal.hpp"

namespace ccamd {

// Staging of the host-pointer entry points ("no hidden allocation per call; thread-safe per
// stream").  Owned by the handle, created on first use: two private streams and, per stream, grow-only device
// buffers.  A host-pointer call cuts the batch into chunks that alternate between the two streams -- the upload of
// chunk k + 1 overlaps the kernel and the download of chunk k -- and waits for ITS streams only
// (hipStreamSynchronize, never hipDeviceSynchronize: other streams of the caller keep running).  Calls on one
// handle are serialised by `lock`; different handles are independent.
// Copies between pageable caller memory and the page-locked staging ring are plain memcpy calls spread over a few
// worker threads (one thread moves ~10 GB/s, the DMA engine 55 GB/s; round 2 handed pageable pointers to
// hipMemcpyAsync, which then blocks the calling thread until the data has moved and with it the pipeline:
// profiles/r02_host_path.txt, 49 ms for what upload and kernel together should do in 31).  Process-wide, created on
// first use, never joined (the workers touch no HIP state and sleep on a condition variable).
class CopyPool {
 public:
  static CopyPool &get() {
    static CopyPool *pool = new CopyPool();
    return *pool;
  }
  void copy(void *dst, const void *src, size_t bytes) {
    const size_t piece = 4u << 20;
    if (bytes <= piece || workers_ == 0) {
      std::memcpy(dst, src, bytes);
      return;
    }
    const size_t parts = std::min<size_t>((bytes + piece - 1) / piece, static_cast<size_t>(workers_) + 1);
    const size_t each = ((bytes + parts - 1) / parts + 4095) & ~static_cast<size_t>(4095);
    std::atomic<int> left{0};
    std::mutex dm;
    std::condition_variable dcv;
    size_t off = each;  // the caller's own share is [0, each)
    {
      std::lock_guard<std::mutex> g(m_);
      for (; off < bytes; off += each) {
        const size_t len = std::min(each, bytes - off);
        ++left;
        jobs_.push_back(Job{static_cast<char *>(dst) + off, static_cast<const char *>(src) + off, len, &left, &dm, &dcv});
      }
    }
    cv_.notify_all();
    std::memcpy(dst, src, std::min(each, bytes));
    std::unique_lock<std::mutex> lk(dm);
    dcv.wait(lk, [&] { return left.load() == 0; });
  }

 private:
  struct Job {
    char *dst;
    const char *src;
    size_t len;
    std::atomic<int> *left;
    std::mutex *dm;
    std::condition_variable *dcv;
  };
  CopyPool() {
    const unsigned hc = std::thread::hardware_concurrency();
    workers_ = hc >= 16 ? 7 : hc >= 8 ? 5 : hc >= 4 ? 2 : 0;  // 3 / 7 / 15 workers: 35 / 33 / 32 ms per 2^20 frames at 4 dB
    for (int i = 0; i < workers_; ++i) std::thread([this] { run(); }).detach();
  }
  void run() {
    for (;;) {
      Job j;
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return !jobs_.empty(); });
        j = jobs_.back();
        jobs_.pop_back();
      }
      std::memcpy(j.dst, j.src, j.len);
      {
        std::lock_guard<std::mutex> g(*j.dm);  // the waiter cannot leave (and destroy dm / dcv) between the two lines
        if (j.left->fetch_sub(1) == 1) j.dcv->notify_one();
      }
    }
  }
  std::mutex m_;
  std::condition_variable cv_;
  std::vector<Job> jobs_;
  int workers_ = 0;
};

struct HostStage {
  std::mutex lock;
  hipStream_t stream[2] = {nullptr, nullptr};
  struct Buf {
    void *p = nullptr;
    size_t cap = 0;
  };
  Buf buf[2][8];
  Buf pin[2][8];  // page-locked twins of buf for pageable caller memory (same slot / index)
  struct Pending {
    void *dst;
    const void *src;
    size_t bytes;
  };
  std::vector<Pending> pending[2];  // results waiting in pin[slot][*] for their stream to finish
  ~HostStage() {
    for (int slot = 0; slot < 2; ++slot) {
      if (stream[slot]) (void)hipStreamSynchronize(stream[slot]);
      for (Buf &b : buf[slot])
        if (b.p) (void)hipFree(b.p);
      for (Buf &b : pin[slot])
        if (b.p) (void)hipHostFree(b.p);
      if (stream[slot]) (void)hipStreamDestroy(stream[slot]);
    }
  }
  int init() {
    for (hipStream_t &s : stream)
      if (!s) CC_HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return CC_OK;
  }
  // A call of several chunks starts on a fresh pair of streams.  Measured (profiles/r03_host_path.txt,
  // profiles/tools/host_path_trace.py): once a stream pair has been through a call whose chunks were fed from the host
  // side with gaps (pageable caller memory), every later call on that pair runs its copies and kernels one after the
  // other -- 46 ms for 2^20 frames at 4 dB where the same call on new streams takes 25 -- for the rest of the process;
  // rocprofv3's copy trace shows the transfers of the fast case on the DMA engines next to the kernels.  Creating two
  // streams costs ~40 us, so calls of one or two chunks (below ~64 MiB) keep the pair they have.
  int fresh_streams() {
    for (hipStream_t &s : stream)
      if (s) {
        CC_HIP_TRY(hipStreamSynchronize(s));
        CC_HIP_TRY(hipStreamDestroy(s));
        s = nullptr;
      }
    return init();
  }
  int get(int slot, int idx, size_t payload, void **out) {  // grow-only; contents are not preserved
    Buf &b = buf[slot][idx];
    const size_t bytes = payload + 16;
    if (bytes > b.cap) {
      CC_HIP_TRY(hipStreamSynchronize(stream[slot]));
      if (b.p) (void)hipFree(b.p);
      b.p = nullptr;
      b.cap = 0;
      const size_t want = bytes + bytes / 4;  // grow by 25 % so that slowly growing batches do not reallocate each time
      CC_HIP_TRY(hipMalloc(&b.p, want));
      b.cap = want;
    }
    *out = b.p;
    return CC_OK;
  }
  int get_pinned(int slot, int idx, size_t bytes, void **out) {
    Buf &b = pin[slot][idx];
    if (bytes > b.cap) {
      if (b.p) (void)hipHostFree(b.p);
      b.p = nullptr;
      b.cap = 0;
      const size_t want = bytes + bytes / 4;
      CC_HIP_TRY(hipHostMalloc(&b.p, want, hipHostMallocDefault));
      b.cap = want;
    }
    *out = b.p;
    return CC_OK;
  }
  // is the caller's buffer something the DMA engines reach directly (page-locked / registered / device memory)?
  static bool dma_ready(const void *p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
      (void)hipGetLastError();  // plain malloc'ed memory: "invalid value", not an error of ours
      return false;
    }
    return a.type == hipMemoryTypeHost || a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
  }
  // host -> device on the slot's stream; `direct` = dma_ready(h_src base), decided once per call
  int upload(int slot, int idx, void *d_dst, const void *h_src, size_t bytes, bool direct) {
    if (bytes == 0) return CC_OK;
    if (!direct) {
      void *ring = nullptr;
      if (int rc = get_pinned(slot, idx, bytes, &ring)) return rc;
      CopyPool::get().copy(ring, h_src, bytes);
      h_src = ring;
    }
    CC_HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, stream[slot]));
    return CC_OK;
  }
  // device -> host behind the slot's kernels; a pageable destination receives its bytes in retire()
  int download(int slot, int idx, void *h_dst, const void *d_src, size_t bytes, bool direct) {
    if (bytes == 0) return CC_OK;
    if (direct) {
      CC_HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, stream[slot]));
      return CC_OK;
    }
    void *ring = nullptr;
    if (int rc = get_pinned(slot, idx, bytes, &ring)) return rc;
    CC_HIP_TRY(hipMemcpyAsync(ring, d_src, bytes, hipMemcpyDeviceToHost, stream[slot]));
    pending[slot].push_back(Pending{h_dst, ring, bytes});
    return CC_OK;
  }
  // wait for everything enqueued on the slot and hand its staged results to the caller's buffers
  int retire(int slot) {
    if (!stream[slot]) return CC_OK;
    const hipError_t e = hipStreamSynchronize(stream[slot]);
    if (e == hipSuccess)
      for (const Pending &q : pending[slot]) CopyPool::get().copy(q.dst, q.src, q.bytes);
    pending[slot].clear();
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize (host staging)");
    return CC_OK;
  }
  int drain() {
    const int a = retire(0), b = retire(1);
    return a != CC_OK ? a : b;
  }
};

// the handle's staging object (created on first use) with its lock held for the duration of one host-pointer call
struct StageLock {
  HostStage *st = nullptr;
  std::unique_lock<std::mutex> held;
  int rc = CC_OK;
  explicit StageLock(const cc_code *code) {
    {
      std::lock_guard<std::mutex> g(code->lazy_lock);
      if (!code->stage) code->stage = new HostStage();
      st = code->stage;
    }
    held = std::unique_lock<std::mutex>(st->lock);
    rc = st->init();
  }
  // every way out of a host-pointer call, error paths included, leaves nothing in flight that still writes to the
  // caller's buffers or reads the staging buffers (a second wait on idle streams costs microseconds)
  ~StageLock() {
    if (st && held.owns_lock()) (void)st->drain();
  }
};
// frames per chunk: about 32 MiB of the widest per-frame stream, at least 16 frames
inline size_t chunk_frames(size_t bytes_per_frame, size_t B) {
  static const size_t chunk_bytes = [] {  // CC_AMD_HOST_CHUNK_BYTES: tests force many small chunks
    const char *e = std::getenv("CC_AMD_HOST_CHUNK_BYTES");
    const long long v = e ? std::atoll(e) : 0;
    return v > 0 ? static_cast<size_t>(v) : static_cast<size_t>(32u << 20);
  }();
  size_t ch = chunk_bytes / (bytes_per_frame ? bytes_per_frame : 1);
  if (ch < 16) ch = 16;
  return ch < B ? ch : B;
}
// uploads the erasure lists of frames [c0, c0 + m) and returns device pointers with which the kernels index them
// by the GLOBAL offsets: d_er is shifted back by off[c0] elements (only [off[c0], off[c0 + m]) is ever read)
inline int upload_erasures(HostStage &st, int slot, int idx, const uint16_t *erasures, const uint32_t *offsets, size_t c0,
                           size_t m, const uint16_t **d_er, const uint32_t **d_off) {
  *d_er = nullptr;
  *d_off = nullptr;
  if (!erasures) return CC_OK;
  const size_t e0 = offsets[c0], ne = offsets[c0 + m] - e0;
  void *er = nullptr, *off = nullptr;
  if (int rc = st.get(slot, idx, (ne + 1) * sizeof(uint16_t), &er)) return rc;
  if (int rc = st.get(slot, idx + 1, (m + 1) * sizeof(uint32_t), &off)) return rc;
  if (ne) CC_HIP_TRY(hipMemcpyAsync(er, erasures + e0, ne * sizeof(uint16_t), hipMemcpyHostToDevice, st.stream[slot]));
  CC_HIP_TRY(hipMemcpyAsync(off, offsets + c0, (m + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st.stream[slot]));
  *d_er = static_cast<const uint16_t *>(er) - e0;
  *d_off = static_cast<const uint32_t *>(off);
  return CC_OK;
}

// One per-frame array of a call, typed as its launcher takes it: `per_frame` elements of T per frame.  An entry point
// lists its arrays in the order of its launch callable's pointers; the staging buffer of an array is its position in
// that list (HostStage::buf[slot][position]), so no call site names a buffer.
template <class T>
struct Arr {
  T *host;  // the caller's array
  size_t per_frame;
  bool in;      // host -> device before the launch; otherwise device -> host behind it
  bool staged;  // has a device buffer; false: the launch sees nullptr
};
template <class T>
Arr<const T> array_in(const T *p, size_t per_frame) { return {p, per_frame, true, true}; }
// an output the kernels write whether or not the caller wants it back: a buffer even when p is null (iters, nerr, status ...)
template <class T>
Arr<T> array_out(T *p, size_t per_frame) { return {p, per_frame, false, true}; }
// an output whose absence selects another kernel: p == nullptr means no buffer, and the launch sees nullptr (L, ext)
template <class T>
Arr<T> array_out_if_wanted(T *p, size_t per_frame) { return {p, per_frame, false, p != nullptr}; }

// The erasure lists of a call that takes them (both null: this call has none), and the mark of a call that never does.
// A chunk's lists go to the two staging buffers behind the call's arrays.
struct Csr {
  const uint16_t *erasures;
  const uint32_t *offsets;
  static constexpr size_t buffers = 2;
};
struct NoCsr {
  static constexpr const uint16_t *erasures = nullptr;
  static constexpr const uint32_t *offsets = nullptr;
  static constexpr size_t buffers = 0;
};
// launch(m, stream, d_er, d_off, pointers...) of a call with erasure lists, launch(m, stream, pointers...) of one without
template <class Erasures, class Launch, class... P>
int launch_on(Launch &launch, size_t m, hipStream_t stream, const uint16_t *d_er, const uint32_t *d_off, P... pointers) {
  if constexpr (Erasures::buffers != 0)
    return launch(m, stream, d_er, d_off, pointers...);
  else
    return launch(m, stream, pointers...);
}

// The chunk loop of every host-pointer entry point: B frames in chunks of chunk_frames(chunk_width, B), cut down to
// a multiple of `granule` frames (an interleaving block is never split) and never less than one granule.  For each
// chunk the launch gets its frame count, the stream to enqueue on, the chunk's erasure lists (a call with a Csr; null
// where it has none) and one typed device pointer per array, in the order the arrays are listed, and returns a status.
// What the loop keeps, and a change to it must keep:
//  - retire(slot) before the slot's buffers are touched: the chunk that used them two turns ago is home, its staged
//    results are in the caller's arrays, and get() may free and reallocate;
//  - every way out drains both streams (StageLock's destructor): no copy is left that writes to caller memory;
//  - a call of more than two chunks starts on fresh streams (HostStage::fresh_streams);
//  - dma_ready is asked once per caller array, not once per chunk;
//  - the erasure lists of a chunk are indexed by their GLOBAL offsets (the shifted base of upload_erasures);
//  - every array listed by array_in() or array_out() gets a device buffer whether or not the caller wants it back;
//    array_out_if_wanted() alone leaves one out.
template <class Erasures, class Launch, class... T, size_t... I>
int staged_call_at(std::index_sequence<I...>, const cc_code *code, size_t B, size_t chunk_width, size_t granule,
                   Erasures csr, Launch &launch, const Arr<T> &...arrays) {
  constexpr size_t N = sizeof...(T);
  static_assert(N >= 1 && N + Erasures::buffers <= std::extent<decltype(HostStage::buf), 1>::value,
                "one staging buffer per array and two for the erasure lists: HostStage::buf has no more");
  struct Staged {
    void *host;
    size_t bytes;  // per frame
    bool in, staged;
  };
  const Staged streams[N] = {
      {const_cast<void *>(static_cast<const void *>(arrays.host)), arrays.per_frame * sizeof(T), arrays.in, arrays.staged}...};
  StageLock sl(code);
  if (sl.rc != CC_OK) return sl.rc;
  HostStage &st = *sl.st;
  size_t CH = chunk_frames(chunk_width, B) / granule * granule;
  if (CH < granule) CH = granule;
  if (B > 2 * CH)
    if (int rc = st.fresh_streams()) return rc;
  // pageable caller memory goes through the page-locked ring (HostStage::upload / download); buffers the DMA engines
  // reach themselves (hipHostMalloc, hipHostRegister) are used in place
  bool direct[N];
  for (size_t i = 0; i < N; ++i) direct[i] = streams[i].staged && streams[i].host && HostStage::dma_ready(streams[i].host);
  size_t k = 0;
  for (size_t c0 = 0; c0 < B; c0 += CH, ++k) {
    const int slot = static_cast<int>(k & 1);
    const size_t m = B - c0 < CH ? B - c0 : CH;
    if (int rc = st.retire(slot)) return rc;
    void *d[N] = {};
    const uint16_t *d_er = nullptr;
    const uint32_t *d_off = nullptr;
    for (size_t i = 0; i < N; ++i)
      if (streams[i].staged)
        if (int rc = st.get(slot, static_cast<int>(i), m * streams[i].bytes, &d[i])) return rc;
    for (size_t i = 0; i < N; ++i) {
      const Staged &s = streams[i];
      if (!s.in) continue;
      if (int rc = st.upload(slot, static_cast<int>(i), d[i], static_cast<const char *>(s.host) + c0 * s.bytes, m * s.bytes, direct[i]))
        return rc;
    }
    if (int rc = upload_erasures(st, slot, static_cast<int>(N), csr.erasures, csr.offsets, c0, m, &d_er, &d_off)) return rc;
    if (int rc = launch_on<Erasures>(launch, m, st.stream[slot], d_er, d_off, static_cast<T *>(d[I])...)) return rc;
    for (size_t i = 0; i < N; ++i) {
      const Staged &s = streams[i];
      if (s.in || !s.staged || !s.host) continue;
      if (int rc = st.download(slot, static_cast<int>(i), static_cast<char *>(s.host) + c0 * s.bytes, d[i], m * s.bytes, direct[i]))
        return rc;
    }
  }
  return st.drain();
}
template <class Erasures, class Launch, class... T>
int staged_call(const cc_code *code, size_t B, size_t chunk_width, size_t granule, Erasures csr, Launch launch, Arr<T>... arrays) {
  return staged_call_at(std::index_sequence_for<T...>(), code, B, chunk_width, granule, csr, launch, arrays...);
}

}  // namespace ccamd
